"""GPU tests (-m gpu) of the far-field lists on the probe cases of tests/ff_visibility.py: zero-residual regions in which
EVERY far-deep, far-shallow, mid and wide (line, tile) entry changes its tile's flux by at least 3 allowances (the
condition is asserted on the CPU, tests/test_ff_visibility.py), at the batching shapes of test_gpu_tile_batches.py.

  1. chi^2 <= 1 for every walker of every probe case (zr.check), fp64 and fp32, workgroup and wavefront per walker, two
     long regions behind a 300-pixel one (pix_off 300 and 300 + P: no multiple of 256), together and alone, bit-equal.
     fp32: one copy of the region per tile, each with the tightened allowance of that tile (zr.make_case(probe_tile=...)).
  2. two sampler steps of a split-only ensemble: every stored lnprob is prior - chi^2 / 2 with chi^2 within the allowance.
  3. negative controls.  The data of a control are those a kernel would fit exactly that LOSES one list entry (line k over
     tile j): the correct kernel must then fail, with chi^2 >= 9, in tile j and in no other (one copy of the region per
     tile, HUGE_NOISE outside it, as zr.localise does).  One control per kind of entry and per batching edge: a deep far
     line, a shallow far line in place >= 8 of its list, a mid line, a wide line, the last tile of a partial batch, the
     first tile behind a full batch; every control region lies behind the lead region (a tile of a second region).
     Nothing here makes a kernel misbehave: only the data differ.
"""
import functools

import numpy as np
import pytest

import ff_visibility as fv
import zero_residual as zr

pytestmark = pytest.mark.gpu

W = 64
PACKINGS = (256, 64)
F32_PROBES = tuple((name, v) for name in fv.PROBE_SHAPES for v in fv.F32_VARIANTS)


def _ctx(dtype, packing):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=vamp_amd.F64 if dtype == "f64" else vamp_amd.F32)
    ctx.set_packing(packing)
    return ctx


@functools.lru_cache(maxsize=None)
def _family(name, dtype, variant, permute):
    """the W walkers of a probe (shared by its tile copies: one truth), read-only"""
    p = fv.probe_case(name, dtype, variant)
    th = zr.walker_family(p.cases[0], W, np.random.default_rng(len(name) + 7 * permute), permute=permute)
    th.setflags(write=False)
    return th


@functools.lru_cache(maxsize=None)
def _lead_family(dtype):
    th = zr.walker_family(fv.lead_case(dtype), W, np.random.default_rng(300), permute=False)
    th.setflags(write=False)
    return th


def _regions(dtype, probes, permute=True):
    """[lead] + the probes' regions, and their walkers"""
    cases, th = [fv.lead_case(dtype)], [_lead_family(dtype)]
    for name, variant in probes:
        p = fv.probe_case(name, dtype, variant)
        cases += list(p.cases)
        th += [_family(name, dtype, variant, permute)] * len(p.cases)
    return cases, th


def _together_and_alone(dtype, packing, cases, th, alone, label):
    with _ctx(dtype, packing) as ctx:
        zr.set_cases(ctx, cases)
        zr.print_report(label, zr.check(ctx, cases, th, label))
        together = {r: ctx.lnprob(th[r], region=r) for r in alone}
    for r in alone:
        with _ctx(dtype, packing) as ctx:
            zr.set_cases(ctx, [cases[r]])
            zr.check(ctx, [cases[r]], [th[r]], label + " alone")
            assert np.array_equal(ctx.lnprob(th[r]), together[r]), (label, cases[r].name, "together != alone")


# -- 1. every probe case within its allowance ---------------------------------------------------------------------
@pytest.mark.parametrize("pair", fv.PROBE_PAIRS, ids="+".join)
@pytest.mark.parametrize("packing", PACKINGS)
def test_probe_cases_fp64(packing, pair):
    cases, th = _regions("f64", [(name, None) for name in pair])
    _together_and_alone("f64", packing, cases, th, (1, 2), "probe f64 packing %d" % packing)


@pytest.mark.parametrize("name,variant", F32_PROBES)
@pytest.mark.parametrize("packing", PACKINGS)
def test_probe_cases_fp32(packing, name, variant):
    cases, th = _regions("f32", [(name, variant)])
    _together_and_alone("f32", packing, cases, th, (1, len(cases) - 1), "probe f32 packing %d" % packing)


# -- 2. the sampler's own evaluations -------------------------------------------------------------------------------
def _sampler(dtype, packing, probes):
    cases, th = _regions(dtype, probes, permute=False)
    with _ctx(dtype, packing) as ctx:
        zr.set_cases(ctx, cases)
        ctx.sampler_init(th, seed=2304, split_block=W)
        res = ctx.run(2)
    report = {}
    for case, ch, lp in zip(cases, res["chain"], res["lnprob"]):
        n, Wc, D = ch.shape
        prior = zr.log_prior_batch(case.region, ch.reshape(n * Wc, D)).reshape(n, Wc)
        assert np.isfinite(lp).all() and np.isfinite(prior).all(), case.name
        chi = -2.0 * (lp - prior)
        assert chi.min() >= -2.0 * zr.LNP_IDENTITY[dtype] * np.abs(lp).max(), (case.name, chi.min())
        e = zr.normalised(case, np.maximum(chi, 0.0))
        report[case.name + " " + str(len(report))] = float(e.max())
        assert e.max() <= 1.0, (case.name, e.max(), np.unravel_index(np.argmax(e), e.shape))
        assert np.unique(ch[:, :, case.splits[0][0] * case.region.q]).size > Wc, case.name      # the splits did move
    zr.print_report("sampler %s packing %d" % (dtype, packing), report)


@pytest.mark.parametrize("pair", fv.PROBE_PAIRS, ids="+".join)
@pytest.mark.parametrize("packing", PACKINGS)
def test_two_sampler_steps_fp64(packing, pair):
    _sampler("f64", packing, [(name, None) for name in pair])


@pytest.mark.parametrize("name,variant", [("P2304", "long"), ("P5120", "long"), ("P4352-steps", "short")])
@pytest.mark.parametrize("packing", PACKINGS)
def test_two_sampler_steps_fp32(packing, name, variant):
    _sampler("f32", packing, [(name, variant)])


# -- 3. negative controls ---------------------------------------------------------------------------------------------
def _pick(p, kind):
    """(k, j) of the control of one kind: an entry of the probe's own lists"""
    e = fv.entries(p.x, p.t, p.dtype == "f32")
    far = e["far-deep"] | e["far-shallow"]
    if kind in ("far-deep", "mid", "wide"):
        k, j = np.argwhere(e[kind])[-1]
    elif kind == "far-shallow slot 8":
        k, j = next((k, j) for k, j in np.argwhere(e["far-shallow"]) if fv.list_slot(p, k, j) >= 8)
    else:
        # workgroup per walker: wavefront 0 of P2304 holds tiles 0, 4, 8 -- a batch of three, tile 8 its last; of P5120
        # tiles 0, 4, 8, 12 and, alone in a second batch, 16.  One wavefront per walker: tile 8 of 9 is a batch of one,
        # tile 16 of 20 opens the fifth batch
        j = {"last of a partial batch": 8, "first behind a full batch": 16}[kind]
        assert p.name == {8: "P2304", 16: "P5120"}[j] and fv.batch_neighbour(16, 20, 256) == -1
        k = np.flatnonzero(far[:, j])[1]
    return int(k), int(j)


CONTROLS = [("f64", "P2304", None, "far-deep"), ("f64", "P2304", None, "far-shallow slot 8"), ("f64", "P4352-steps", None, "mid"),
            ("f64", "P2304-down", None, "wide"), ("f64", "P2304", None, "last of a partial batch"),
            ("f64", "P5120", None, "first behind a full batch"),
            ("f32", "P2304", "long", "far-deep"), ("f32", "P2404", "long", "far-shallow slot 8"),
            ("f32", "P2304", "short", "last of a partial batch"), ("f32", "P5120", "long", "first behind a full batch")]


@pytest.mark.parametrize("dtype,name,variant,kind", CONTROLS, ids=lambda v: str(v).replace(" ", "-"))
@pytest.mark.parametrize("packing", PACKINGS)
def test_negative_control_fails_in_its_tile_only(packing, dtype, name, variant, kind):
    k, j = _pick(fv.probe_case(name, dtype, variant), kind)
    control = fv.probe_case(name, dtype, variant, drop=(k, j))
    copies = fv.tile_copies(control)
    ordered = kind == "far-shallow slot 8"            # the place in the list is that of the truth's order of lines
    if ordered:
        assert fv.list_slot(control, k, j) >= 8
    th = _family(name, dtype, variant, permute=not ordered)
    cases = [fv.lead_case(dtype)] + copies
    with _ctx(dtype, packing) as ctx:
        zr.set_cases(ctx, cases)
        lnp, chi = ctx.lnprob_all([_lead_family(dtype)] + [th] * len(copies), return_chi2=True)
    chi = chi[1:]
    assert np.isfinite(lnp).all() and np.isfinite(chi).all()
    others = np.delete(chi, j, axis=0)
    print("control %s %s%s packing %d, %s: line %d over tile %d: chi^2 there %.3g .. %.3g, elsewhere <= %.3g" % (
        dtype, name, " " + variant if variant else "", packing, kind, k, j, chi[j].min(), chi[j].max(), others.max()))
    assert chi[j].min() >= fv.MARGIN ** 2, (kind, k, j, chi[j].min())
    assert others.max() <= 1.0, (kind, k, j, np.unravel_index(np.argmax(others), others.shape), others.max())
