"""GPU tests (-m gpu): the sampler kernels leave the exact target invariant.

Every other sampler test holds k_half_step, k_run_resident and the host library to the oracle's restatement of the stretch
move over a few steps; none compares a DISTRIBUTION a kernel produced with an exact one.  Here every leg builds a context of
R identical regions (their draws are keyed by the region index: R independent ensembles), starts every walker from an exact
draw of the target, runs T steps and asserts on the N = R W = 65 536 final walkers (tests/sampler_stats.py, DESIGN.md
"Sampler statistics"), printing each figure first (run with -s):

  1. KS: sqrt(N) D_N of every parameter against its exact marginal CDF < 3.3 + sqrt(N) eps (Kolmogorov tail 7e-10);
  2. acceptance: |acc - p_acc| <= 5 sqrt(se_run^2 + se_ref^2) against the direct integral, with se_run <= 3e-4 and
     se_ref <= 2e-4 as conditions;
  3. correlation (prior legs, where the target is a product): |corr| sqrt(N) < 6 for every pair of parameters;
  4. state: the returned lnprob is ctx.lnprob of the returned positions (1e-9 relative in fp64, the fp32 file's 1e-3 in
     fp32) and no walker sits at -inf.

Prior legs (flat likelihood: flux = 1, noise = 1e8, so the target is the prior; x = 0 .. P - 1; T = 200, or 800 for D >= 12):
  a GAUSS3 K 1 P 8 (D 3, one/two-line class)      b VOIGT4 K 1 P 8 (D 4, one/two-line class)
  c VOIGT4 K 4 P 40 (D 16, four walkers per wavefront)      d VOIGT4 K 3 P 128 (D 12, blend)
  e GAUSS3 K 12 P 40 and VOIGT4 K 17 P 40 (D 36, 68: 9..16 lines, more than 16 lines)      f VOIGT4 K 2 P 600 (D 8, long region)
as 1024 x 64 with one launch per half-step, 4 seeds x 256 x 64 in the resident loop and 16 x 4096, through conftest's
packings where the shape admits them (as tests/test_gpu_parity.py: packings 16 / 65 hold 8 lines, the workgroup-per-walker
packing is for long regions and is not resident), a and c in fp32 as well.  Posterior legs: one Gaussian line on 24 pixels
against the quadrature, T = 100, fixed noise in fp64 and fp32 and the product's default free sd in fp64.
Which path ran is read from vamp_kernel_timing's count (one interval per run in the resident loop, one per half-step
otherwise), which class from vamp_region_class.
"""
import numpy as np
import pytest

import sampler_stats as ss

pytestmark = pytest.mark.gpu

N = 65536
CK_SMALL, CK_MID, CK_WIDE, CK_SMALL2, CK_XL = 0, 1, 2, 3, 4
LEG_CLASS = {"a": CK_SMALL2, "b": CK_SMALL2, "c": CK_SMALL, "d": CK_MID, "e12": CK_WIDE, "e17": CK_XL, "f": CK_WIDE}      # automatic packing
FORCED_CLASS = {16: CK_SMALL, 65: CK_MID, 64: CK_WIDE, 256: CK_WIDE}
# ensembles: (R, W, "resident" option, seeds); 2 = the resident loop wherever the kernel can run, 0 = one launch per half-step,
# 1 = automatic (W / 2 = 2048 movers do not fit a workgroup's round: one launch per half-step)
ENSEMBLES = {"1024x64-launch": (1024, 64, 0, (101,)), "4x256x64-resident": (256, 64, 2, (201, 202, 203, 204)), "16x4096": (16, 4096, 1, (301,))}
LEG_ENSEMBLES = [(leg, e) for leg in ("a", "b", "c") for e in ENSEMBLES] + [("d", "16x4096"), ("d", "1024x64-launch"), ("f", "16x4096")]
LNP_BAR = {"f64": 1e-9, "f32": 1e-3}


@pytest.fixture(scope="module", params=[0, 64, 16, 256, 65], ids=["pack-auto", "pack-64", "pack-16", "pack-256", "pack-64t"])
def hip_ctx32(request):
    """fp32 / Humlicek-W4 context on device 0, once per walker packing (the packings of conftest.hip_ctx)."""
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=vamp_amd.F32)
    ctx.set_packing(request.param)
    ctx.packing_request = request.param
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def plain_ctx():
    """fp64 and fp32 contexts with automatic packing, for the legs that do not go through the packings"""
    import vamp_amd
    ctxs = {"f64": vamp_amd.HipContext(device=0), "f32": vamp_amd.HipContext(device=0, dtype=vamp_amd.F32)}
    for c in ctxs.values():
        c.packing_request = 0
    yield ctxs
    for c in ctxs.values():
        c.close()


def _admits(ctx, leg, ensemble):
    K, P = ss.PRIOR_LEGS[leg][1], ss.PRIOR_LEGS[leg][2]
    if ctx.packing_request in (16, 65) and K > 8:
        pytest.skip("packings 16 and 65 hold 8 lines")
    if ctx.packing_request == 256 and P < 512:
        pytest.skip("short regions: the workgroup-per-walker packing is for long regions")
    if ctx.packing_request == 256 and ENSEMBLES[ensemble][2] == 2:
        pytest.skip("workgroup-per-walker shapes are not resident")


_STARTS = {}


def _start(target, seed, n):
    """exact start draws, kept per (target, seed): the forms and dtypes of a leg share them, nothing changes them"""
    key = (id(target), seed, n)
    if key not in _STARTS:
        _STARTS[key] = target.draw(n, np.random.default_rng(seed))
    return _STARTS[key]


def _run_leg(ctx, label, leg_data, ensemble, dtype, want_class, corr):
    data, target, (p_ref, se_ref) = leg_data
    R, W, resident, seeds = ENSEMBLES[ensemble]
    assert R * W * len(seeds) == N
    T = data["T"]
    Xs, accs = [], []
    for seed in seeds:
        X0 = _start(target, seed, R * W) if not corr else target.draw(R * W, np.random.default_rng(seed))
        X, lnp, nacc, intervals, kind = ss.run_context(ctx, data, X0, R, W, seed=seed, resident=resident)
        assert kind == want_class, (label, "class", kind, want_class)
        assert intervals == (1 if resident == 2 else 2 * T), (label, "path", intervals)
        ss.assert_state_consistent(ctx, X, lnp, R, W, LNP_BAR[dtype])
        Xs.append(X)
        accs.append(nacc)
    fig = ss.leg_figures(np.concatenate(Xs), np.concatenate(accs), R * len(seeds), W, T, target, p_ref, se_ref, corr)
    ss.assert_leg(label, fig)


def _prior(ctx, leg, ensemble, dtype):
    want = LEG_CLASS[leg] if ctx.packing_request == 0 or ss.PRIOR_LEGS[leg][1] > 16 else FORCED_CLASS[ctx.packing_request]
    label = "MI355X %s leg %s %s packing %d" % (dtype, leg, ensemble, ctx.packing_request)
    _run_leg(ctx, label, ss.prior_leg(leg), ensemble, dtype, want, corr=True)


@pytest.mark.parametrize("leg,ensemble", LEG_ENSEMBLES)
def test_prior_is_invariant(hip_ctx, leg, ensemble):
    _admits(hip_ctx, leg, ensemble)
    _prior(hip_ctx, leg, ensemble, "f64")


@pytest.mark.parametrize("leg,ensemble", [(leg, e) for leg in ("a", "c") for e in ENSEMBLES])
def test_prior_is_invariant_fp32(hip_ctx32, leg, ensemble):
    _admits(hip_ctx32, leg, ensemble)
    _prior(hip_ctx32, leg, ensemble, "f32")


@pytest.mark.parametrize("leg", ["e12", "e17"])
def test_prior_is_invariant_with_many_lines(hip_ctx, leg):
    """9 .. 16 lines (one walker per wavefront) and more than 16 lines (every line per pixel), D = 36 and 68: the same bars;
    KS has little power at these dimensions in 800 steps, acceptance carries the leg (tests/sampler_stats.py prints so)"""
    _admits(hip_ctx, leg, "16x4096")
    _prior(hip_ctx, leg, "16x4096", "f64")


@pytest.fixture(scope="module")
def line_posterior():
    """the quadrature of the one-line posterior, both forms, built once on the host"""
    return {False: ss.posterior_leg(False, N), True: ss.posterior_leg(True, N)}


@pytest.mark.parametrize("ensemble", list(ENSEMBLES))
@pytest.mark.parametrize("form", ["fixed-f64", "fixed-f32", "sd-f64"])
def test_posterior_of_one_gaussian_line_is_invariant(plain_ctx, line_posterior, form, ensemble):
    kind, dtype = form.split("-")
    leg = line_posterior[kind == "sd"]
    assert leg[1].eps <= leg[1].eps_bar
    label = "MI355X %s posterior (%s) %s" % (dtype, "free sd, D 4" if kind == "sd" else "fixed noise, D 3", ensemble)
    _run_leg(plain_ctx[dtype], label, leg, ensemble, dtype, CK_SMALL2, corr=False)
