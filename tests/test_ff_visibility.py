"""CPU tests of tests/ff_visibility.py: which far-field list entries a check can see.

1. The motivation, pinned: for the mixed cases of test_gpu_tile_batches.py (strong damped lines beside weak ones) the
   share of list entries whose loss would stay below the lnprob bars is computed and printed (pytest -s).  It is a
   record, not a bar: those cases keep their role of mixing every class.
2. THE CONDITION of the probe cases (ff_visibility.probe_case), asserted: under the zero-residual allowance every
   far-deep, far-shallow, mid and wide entry (fp32: every far entry, in the fp32 sense of far) of every probe case has
   visibility >= 3 -- counted twice, dropped, or credited to the wrong tile of its batch under either packing -- so a
   kernel that loses one returns chi^2 >= 9 where tests/test_gpu_ff_controls.py demands <= 1.  Some tile has more than 8
   far lines (the second slot pair of ff_coefficients / the second slot group of ff32_coefficients runs) and some tile
   has at most 8.
3. The tightened fp32 allowance of the probe cases (zr.make_case(probe_tile=...)) is nowhere larger than the default
   one inside its tile.
"""
import numpy as np
import pytest

import ff_visibility as fv
import test_gpu_tile_batches as tb
import zero_residual as zr

TABLE_CASES = ("P2048", "P2304", "P5120", "P2404", "P4352-steps")


def test_existing_cases_hide_entries_from_the_lnprob_bars():
    """share of (line, tile) entries of walker 0 whose loss moves lnprob by less than the bar (fp64 1e-9 max(1, |lnprob|),
    fp32 1e-3 |lnprob|)"""
    hidden64, hidden32 = [], []
    for name in TABLE_CASES:
        rows = [fv.lnprob_shares(name, K) for K in tb.KS]
        print("%-12s K=1/7/16: entries %s, share hidden from the fp64 bar %s, from the fp32 bar %s" % (
            name, " / ".join("%d" % r[0] for r in rows), " / ".join("%.2f" % r[1] for r in rows),
            " / ".join("%.2f" % r[2] for r in rows)))
        assert all(r[0] > 0 and 0.0 <= r[1] <= r[2] <= 1.0 for r in rows)      # (the fp32 bar is the wider one)
        hidden64 += [r[1] for r in rows]
        hidden32 += [r[2] for r in rows]
    # the helper does distinguish: something is visible and something is hidden under either bar
    assert min(hidden64) < 0.5 < max(hidden32)


def _probes():
    return [(name, "f64", None) for name in fv.PROBE_SHAPES] + [(name, "f32", v) for name in fv.PROBE_SHAPES for v in fv.F32_VARIANTS]


@pytest.mark.parametrize("name,dtype,variant", _probes())
def test_every_entry_of_a_probe_case_is_visible(name, dtype, variant):
    p = fv.probe_case(name, dtype, variant)
    assert np.isfinite(p.sigma).all() and (p.sigma > 0).all()
    classes = fv.CLASSES if dtype == "f64" else fv.CLASSES[:2]
    worst = {}
    for mutation, packing in (("twice", 256), ("drop", 256), ("wrong_tile", 256), ("wrong_tile", 64)):
        vis = fv.probe_visibility(p, mutation, packing)
        assert set(vis) == set(classes)
        for c in classes:
            v = vis[c][~np.isnan(vis[c])]
            if mutation != "wrong_tile":
                assert v.size > 0, (c, "no entry of this class")
            worst[c] = min(worst.get(c, np.inf), v.min())
    print("%s %s%s: least visibility %s" % (name, dtype, " " + variant if variant else "",
                                            ", ".join("%s %.3g" % (c, worst[c]) for c in classes)))
    assert min(worst.values()) >= fv.MARGIN, worst


@pytest.mark.parametrize("name", fv.PROBE_SHAPES)
def test_probe_lists_reach_every_slot_group(name):
    nfar = fv.far_counts(fv.probe_case(name, "f64"))
    assert nfar.min() <= 8 < nfar.max(), nfar
    short, long = (fv.far_counts(fv.probe_case(name, "f32", v)) for v in ("short", "long"))
    assert 0 < short.max() <= 8 and long.max() == 9, (short, long)      # 9: the least that reaches the second group
    # the slot-8 control of the GPU test exists: a far-shallow entry in place >= 8 of its list
    p = fv.probe_case(name, "f64")
    e = fv.entries(p.x, p.t)
    assert any(fv.list_slot(p, k, j) >= 8 for k, j in zip(*np.nonzero(e["far-shallow"])))


@pytest.mark.parametrize("name", ("P2304", "P4352-steps"))
def test_tightened_fp32_allowance_never_exceeds_the_default(name):
    p = fv.probe_case(name, "f32", "long")
    c0 = p.cases[0]
    default = zr.make_case("default", p.x, c0.truth, c0.region.n_comp, dtype="f32", pad=50.0 * np.max(np.abs(np.diff(p.x))))
    assert (p.sigma <= default.sigma).all()
    assert (p.sigma < default.sigma).any()
    for j, c in enumerate(p.cases):          # each copy: its tile, HUGE_NOISE elsewhere
        inside = np.arange(p.x.size) // fv.TILE == j
        assert (c.sigma[~inside] == zr.HUGE_NOISE).all() and (c.sigma[inside] < 1.0).all()


def test_batch_neighbours():
    # workgroup per walker, 9 tiles: wavefront 0 holds tiles 0, 4, 8 (one batch), the others two tiles each
    assert [fv.batch_neighbour(j, 9, 256) for j in range(9)] == [4, 5, 6, 7, 8, 1, 2, 3, 4]
    # one wavefront, 9 tiles: batches (0..3), (4..7), (8)
    assert [fv.batch_neighbour(j, 9, 64) for j in range(9)] == [1, 2, 3, 2, 5, 6, 7, 6, -1]
    # 20 tiles, workgroup per walker: tile 16 opens wavefront 0's second batch alone
    assert fv.batch_neighbour(16, 20, 256) == -1 and fv.batch_neighbour(12, 20, 256) == 8
