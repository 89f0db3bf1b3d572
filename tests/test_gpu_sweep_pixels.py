"""GPU tests (-m gpu): the chi^2 sweep's model flux, pixel by pixel, on zero-residual regions (tests/zero_residual.py).

The data are the oracle's model flux of a truth, the noise is a per-pixel allowance derived from DESIGN.md's error
statements, and every walker shares the truth's exact model (permutations of its lines, amplitude splits of coincident
lines, a free sd).  chi^2 <= 1 then proves that every pixel of every walker is within its allowance, through the paths
only the sweep takes (far-field interpolant, Taylor tables, tile interpolant of wide lines, caps, the degree-11 exp)
and at production walker counts: the oracle runs once per region.  Covered:
  1. the launch bench.py times (P = 16 384, K = 16, NBZ3, W = 65 536, automatic packing) in fp64 and fp32, and the same
     region at small W under every packing;
  2. every line class of the long-region sweep at P = 16 384, 4096, 3000, 1000 on ascending, descending and uneven grids;
  3. all 421 q1422 regions (their data replaced by the model of a truth of their own) and synthetic short regions of
     every P mod 32, at packings 0 and 16, class streams on and off, and production-size packed launch classes;
  4. GAUSS3, VOIGT4, NBZ3 and free sd;
  5. the sampler's own evaluations: every stored lnprob of a split-only ensemble is prior - chi^2 / 2 with chi^2
     within the allowance, resident and not;
  6. a negative control: 2 sigma_i added at one far-field pixel of the headline fails the check at that tile.
Each test prints the worst normalised error sqrt(chi^2) of every case (pytest -s).
"""
import functools
import os

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import zero_residual as zr
from test_gpu_parity import FAR_FIELD_CASES

pytestmark = pytest.mark.gpu

LONG_P = (16384, 4096, 3000, 1000)
WIDE_MAX = float(os.environ.get("VAMP_TEST_WIDE_MAX", "0.75"))      # VAMP_WIDE_MAX of the library under test


@pytest.fixture(scope="module", params=[0, 64, 16, 256, 65], ids=["pack-auto", "pack-64", "pack-16", "pack-256", "pack-64t"])
def hip_ctx32(request):
    """fp32 / Humlicek-W4 context on device 0, once per walker packing (the packings of conftest.hip_ctx)."""
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=vamp_amd.F32)
    ctx.set_packing(request.param)
    ctx.packing_request = request.param
    yield ctx
    ctx.close()



def _run(ctx, cases, W, seed, label, **kw):
    rng = np.random.default_rng(seed)
    zr.set_cases(ctx, cases)
    th = [zr.walker_family(c, W, rng, **kw) for c in cases]
    report = zr.check(ctx, cases, th, label)
    zr.print_report(label, report)
    return report


@functools.lru_cache(maxsize=None)
def _headline(dtype):
    return zr.headline_case(dtype)


@functools.lru_cache(maxsize=None)
def _line_classes(kind, dtype):
    cases = []
    for i, P in enumerate(LONG_P):
        cases += zr.line_class_cases(P, kind, dtype, 1000 + 10 * i + len(kind), wide_max=WIDE_MAX,
                                     far_field_cases=FAR_FIELD_CASES)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def _q1422(dtype):
    from tools.bench_c3 import build_regions
    xs, _, _, ks = build_regions()
    rng = np.random.default_rng(1422)
    return tuple(zr.short_case("q1422 r%d P=%d K=%d" % (r, len(x), k), x, k, rng, dtype) for r, (x, k) in enumerate(zip(xs, ks)))


@functools.lru_cache(maxsize=None)
def _short_synthetic(dtype, mode=vo.MODE_VOIGT4, sd=False):
    """P = 2 .. 96 (every residue of P mod 32, the tail rounds of the short-region sweep), 1 .. 4 lines"""
    rng = np.random.default_rng(96 + mode + 3 * sd)
    nbz = np.array([0.7, 1215.67, 2.4e15, 4.0e10]) if mode == vo.MODE_NBZ3 else None
    out = []
    for P in range(2, 97):
        x = zr.grid(P, ("ascending", "descending", "uneven")[P % 3], rng)
        out.append(zr.short_case("short P=%d" % P, x, 1 + P % 4, rng, dtype, mode=mode, sample_sd=sd, nbz=nbz))
    return tuple(out)


def _long_ok(ctx):
    if ctx.packing_request in (16, 65):
        pytest.skip("long regions: one walker per wavefront or workgroup")


# -- 1. the headline launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_headline_launch_at_bench_size(dtype):
    """The launch bench.py times: make_workload's truth, W = 65 536 permutations of its 16 lines, automatic packing
    (the workgroup-per-walker kernels, 1.07e9 walker-pixels)."""
    import vamp_amd
    case = _headline(dtype)
    with vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype.upper())) as ctx:
        _run(ctx, [case], 65536, 1, "headline W=65536 " + dtype)


def test_headline_small_ensemble(hip_ctx):
    _long_ok(hip_ctx)
    _run(hip_ctx, [_headline("f64")], 64, 2, "headline W=64 f64 packing %d" % hip_ctx.packing_request)


def test_headline_small_ensemble_fp32(hip_ctx32):
    _long_ok(hip_ctx32)
    _run(hip_ctx32, [_headline("f32")], 64, 2, "headline W=64 f32 packing %d" % hip_ctx32.packing_request)


# -- 2. every line class of the long-region sweep ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ascending", "descending", "uneven"])
def test_long_region_line_classes(hip_ctx, kind):
    _long_ok(hip_ctx)
    _run(hip_ctx, list(_line_classes(kind, "f64")), 16, 3, "lines f64 packing %d" % hip_ctx.packing_request)


@pytest.mark.parametrize("kind", ["ascending", "descending", "uneven"])
def test_long_region_line_classes_fp32(hip_ctx32, kind):
    _long_ok(hip_ctx32)
    _run(hip_ctx32, list(_line_classes(kind, "f32")), 16, 3, "lines f32 packing %d" % hip_ctx32.packing_request)


# -- 3. short regions and launch classes ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("packing", [0, 16])
def test_q1422_and_short_regions(dtype, packing):
    """All 421 q1422 regions and the 95 synthetic short ones in one context, W = 32, class streams on and off."""
    import vamp_amd
    cases = list(_q1422(dtype)) + list(_short_synthetic(dtype))
    with vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype.upper())) as ctx:
        ctx.set_packing(packing)
        for cs in (1, 0):
            ctx.set_option("class_streams", cs)
            _run(ctx, cases, 32, 4, "short %s packing %d class_streams %d" % (dtype, packing, cs))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_packed_launch_classes_at_production_size(dtype):
    """W = 32 768 (automatic packing packs launches of >= 16 384 walkers): q1422 regions of every launch class (one,
    two, three and more lines, below and above 96 px) and synthetic short regions of 32 consecutive P, class streams
    on and off."""
    import vamp_amd
    q = _q1422(dtype)
    ks = [c.region.n_comp for c in q]
    ps = [c.region.x.size for c in q]
    pick = []
    for want in ((1, 0, 60), (2, 0, 96), (3, 0, 96), (4, 96, 200), (8, 0, 96), (8, 96, 10000), (5, 200, 10000)):
        pick += [r for r in range(len(q)) if (ks[r] == want[0] or (want[0] >= 4 and ks[r] >= want[0])) and want[1] <= ps[r] < want[2]][:1]
    cases = [q[r] for r in pick] + list(_short_synthetic(dtype))[30:62]
    with vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype.upper())) as ctx:
        for cs in (1, 0):
            ctx.set_option("class_streams", cs)
            _run(ctx, cases, 32768, 5, "production W=32768 %s class_streams %d" % (dtype, cs))


# -- 4. modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sd", [(vo.MODE_GAUSS3, False), (vo.MODE_VOIGT4, False), (vo.MODE_NBZ3, False),
                                     (vo.MODE_VOIGT4, True), (vo.MODE_GAUSS3, True)],
                         ids=["gauss3", "voigt4", "nbz3", "voigt4-sd", "gauss3-sd"])
def test_modes(hip_ctx, mode, sd):
    """Short regions of every P mod 32 under every packing, and a 4096-pixel region of 8 + 1 lines where the packing
    takes long regions.  Free sd: chi^2 is the unweighted sum (f - m)^2, bounded by the largest sigma_i."""
    rng = np.random.default_rng(40 + mode + 3 * sd)
    cases = list(_short_synthetic("f64", mode, sd))
    if hip_ctx.packing_request not in (16, 65):
        nbz = np.array([0.7, 1215.67, 2.4e15, 4.0e10]) if mode == vo.MODE_NBZ3 else None
        t = zr.line_class_truths(zr.grid(4096, "ascending", rng), rng, WIDE_MAX, FAR_FIELD_CASES)["ff mixed"][0][:8]
        if mode == vo.MODE_NBZ3:
            t[:, 2] = nbz[0]
        t, pair = zr.with_split(t, 0, 0.3)
        cases.append(zr.make_case("long P=4096", zr.grid(4096, "ascending", rng), zr.native_to_mode(t, mode, nbz), 9,
                                  mode=mode, sample_sd=sd, nbz=nbz, splits=(pair,)))
    _run(hip_ctx, cases, 32, 6, "mode %d sd %d packing %d" % (mode, sd, hip_ctx.packing_request))


# -- 5. the sampler's own evaluations ---------------------------------------------------------------------------------
def _sampler_cases(dtype, long):
    """split-only ensembles: one 4096-pixel region of 10 + 1 lines (workgroup-per-walker kernels, never resident), or
    six short regions of 2 .. 6 lines (packed classes, resident when asked)"""
    rng = np.random.default_rng(5 if long else 6)
    if long:
        x = zr.grid(4096, "uneven", rng)
        t = zr.line_class_truths(x, rng, WIDE_MAX, FAR_FIELD_CASES)["ff headline-like"][0][:10]
        t, pair = zr.with_split(t, 3, 0.4)
        return [zr.make_case("sampler P=4096", x, t.ravel(), 11, dtype=dtype, splits=(pair,))]
    return [zr.short_case("sampler P=%d" % P, zr.grid(P, "ascending", rng), K, rng, dtype)
            for P, K in ((30, 2), (44, 3), (90, 5), (160, 4), (300, 6), (23, 2))]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["short-resident", "short-launches", "long"])
def test_sampler_split_only_ensembles(dtype, shape):
    """20 steps of a split-only ensemble (every walker the truth, the coincident pair's amplitude split anew): every
    proposal the stretch move makes is a zero-residual point, so every lnprob the sampler stores is prior - chi^2 / 2
    with chi^2 within the allowance."""
    import vamp_amd
    cases = _sampler_cases(dtype, shape == "long")
    W = 32
    rng = np.random.default_rng(11)
    th = [zr.walker_family(c, W, rng, permute=False) for c in cases]
    with vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype.upper())) as ctx:
        ctx.set_option("resident", 2 if shape == "short-resident" else 0)
        zr.set_cases(ctx, cases)
        zr.check(ctx, cases, th, "sampler start")
        ctx.sampler_init(th, seed=2024, split_block=W)
        res = ctx.run(20)
    chains = res["chain"] if len(cases) > 1 else [res["chain"]]
    lnps = res["lnprob"] if len(cases) > 1 else [res["lnprob"]]
    nacc = res["n_accept"] if len(cases) > 1 else [res["n_accept"]]
    report = {}
    for case, ch, lp, na in zip(cases, chains, lnps, nacc):
        n, Wc, D = ch.shape
        prior = zr.log_prior_batch(case.region, ch.reshape(n * Wc, D)).reshape(n, Wc)
        assert np.isfinite(lp).all() and np.isfinite(prior).all(), case.name
        chi = -2.0 * (lp - prior)
        assert chi.min() >= -2.0 * zr.LNP_IDENTITY[dtype] * np.abs(lp).max(), (case.name, chi.min())
        e = zr.normalised(case, np.maximum(chi, 0.0))
        report[case.name] = float(e.max())
        assert e.max() <= 1.0, (case.name, e.max(), np.unravel_index(np.argmax(e), e.shape))
        assert na.sum() > 0, case.name
        moved = ch[:, :, case.splits[0][0] * case.region.q]
        assert np.unique(moved).size > Wc, case.name           # the splits did move
    zr.print_report("sampler %s %s" % (dtype, shape), report)


# -- 6. negative control ----------------------------------------------------------------------------------------------
def test_negative_control_one_far_field_pixel():
    """2 sigma_j added to the headline's data at one far-field pixel j: every walker fails, at the tile of j."""
    import vamp_amd
    j = zr.far_pixel(_headline("f64"))
    case = zr.headline_case("f64", data_shift=lambda s: np.where(np.arange(s.size) == j, 2.0 * s, 0.0))
    with vamp_amd.HipContext(device=0) as ctx:
        with pytest.raises(AssertionError) as err:
            _run(ctx, [case], 64, 7, "negative control")
    tile = j // zr.TILE
    assert "64 walkers beyond the allowance" in str(err.value), str(err.value)
    assert "tile %d, pixels [%d, %d)" % (tile, tile * zr.TILE, (tile + 1) * zr.TILE) in str(err.value), str(err.value)
