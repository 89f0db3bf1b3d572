"""The line-major node stage of the fp64 far-field loop (ff_classify_batch_np, ff_node_pass, sweep_range_ff_np) on the GPU.

  * the node sums and the folded class sets, copied out by the test hook vampdbg_node_sums, against the numpy restatement
    (tests/node_pass_ref.py) on the regions of tests/node_pass_cases.py -- full batches, a full batch plus one tile, no
    full batch at all, a tail, a descending and a stepped grid; K = 1, 7, 16.  tests/test_node_pass.py asserts on the CPU
    what the regions are chosen for;
  * the log-posterior and twenty steps of the sampler on the same regions against the oracle, at the bars of
    tests/test_gpu_parity.py (fp64: 1e-9 max(1, |lnprob|); positions to 1e-10 with identical accept counts);
  * a walker with both guard bits (a line of y = 1e-300, a line that reaches beyond X_FAR);
  * batches of moment tiles: all four tiles done from their moments, and one tile admitted on the data alone and turned
    away by the guard after the node stage.

Bars of the node sums.  Full batches, against the restatement, which evaluates the same fractions on the same classes in
extended precision: the kernel's rounding alone -- an m-level fraction is 2m + 4 fused operations on positive terms and a
Newton reciprocal, every one good to an ulp, 16 for the deepest; the bar is 64 ulps of the sum of the terms' magnitudes,
plus the Taylor tables' stated 2e-14 (voigt_math.hpp) of the wide and mid lines' share.  Other tiles, against scipy's wofz:
the fractions' stated accuracy at the lower ends of their ranges, 9e-13 of a value (ff_eval2), doubled."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import node_pass_cases as nc
import node_pass_ref as npr
import test_gpu_ff_zone as fz
import tile_moments_ref as tm

ULP = 2.0 ** -53
PACKINGS = [0, 256, 64]
STEPS = 20


def _context(packing, c):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0)
    ctx.set_packing(packing)
    ctx.set_regions(c["x"], c["flux"], c["noise"], c["K"], mode=vamp_amd.MODE_VOIGT4, bounds=c["bounds"])
    return ctx


def _node_sums(ctx, theta, ntile):
    fn = ctx._lib.vampdbg_node_sums
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    th = np.ascontiguousarray(theta, np.float64)
    nodes, sets = np.full((ntile, 16), np.nan), np.zeros((ntile, 5), np.uint32)
    n = fn(ctx._h, 0, th.ctypes.data, nodes.ctypes.data, sets.ctypes.data)
    assert n == ntile, (n, ctx._lib.vamp_last_error())
    return nodes, sets


@pytest.mark.gpu
@pytest.mark.parametrize("K", nc.KS)
@pytest.mark.parametrize("name", list(nc.SHAPES))
def test_node_sums_match_the_restatement(name, K):
    c = nc.case(name, K)
    x, ntile = c["x"], c["x"].size // nc.TILE
    full, rest = npr.batches(ntile)
    worst_full = worst_rest = 0.0
    with _context(256, c) as ctx:
        for w in (0, 1, K + 2):
            native = c["th"][w].reshape(K, 4)
            got, gsets = _node_sums(ctx, c["th"][w], ntile)
            assert np.isfinite(got).all()
            want, mag, magw = npr.node_sums(native, x)
            ref_sets = npr.class_sets(native, x)
            heads = {int(s["tiles"][0]): s for s in ref_sets}
            for t in range(ntile):
                if t in heads:
                    s = heads[t]
                    assert [int(v) for v in gsets[t]] == [s["far"], s["n6"], s["n4"], s["n3"], s["wide"]], (w, t)
                else:
                    assert (gsets[t] == 0xffffffff).all(), (w, t)
            if len(full):
                ft = full.reshape(-1)
                tol = 64 * ULP * mag[ft] + 4e-14 * magw[ft]
                err = np.abs(got[ft] - want[ft])
                worst_full = max(worst_full, np.max(err / np.maximum(tol, 1e-300)))
            if rest:
                err = np.abs(got[rest] - want[rest])
                worst_rest = max(worst_rest, np.max(err / np.maximum(2 * 9e-13 * mag[rest], 1e-300)))
    print(f"{name} K={K}: node sums nearest their bars: full batches {worst_full:.3f}, other tiles {worst_rest:.3f}")
    assert worst_full <= 1.0 and worst_rest <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("K", nc.KS)
@pytest.mark.parametrize("name", list(nc.SHAPES))
@pytest.mark.parametrize("packing", PACKINGS)
def test_lnprob_matches_oracle(packing, name, K):
    c = nc.case(name, K)
    with _context(packing, c) as ctx:
        got = ctx.lnprob(c["th"])
    want = c["want"]
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
    print(f"pack {packing} {name} K={K}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err:.2e}")
    assert err <= 1e-9


@functools.lru_cache(maxsize=None)
def _oracle_run(name, K):
    c = nc.case(name, K)
    return vo.run_sampler(lambda q: vo.log_prob_batch_fast(c["reg"], q), c["th"], c["want"], STEPS, seed=4096 + K, block=nc.W)


@pytest.mark.gpu
@pytest.mark.parametrize("K", nc.KS)
@pytest.mark.parametrize("name", list(nc.SHAPES))
@pytest.mark.parametrize("packing", PACKINGS)
def test_twenty_steps_match_oracle(packing, name, K):
    c = nc.case(name, K)
    chain, lchain, nacc = _oracle_run(name, K)
    with _context(packing, c) as ctx:
        ctx.sampler_init(c["th"], seed=4096 + K, a=2.0, split_block=nc.W)
        res = ctx.run(STEPS)
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)


# ---- the guard path -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def guard_case():
    """P4096, K = 7 with one line of y = 1e-300 and one so narrow that the region's ends lie beyond X_FAR in its z"""
    base = nc.case("P4096", 7)
    t = base["t"].copy()
    x = base["x"]
    t[0] = (2.0, 0.5 * (x[256 * 4] + x[256 * 5 - 1]), 0.0, 30.0)
    t[0, 2] = 1e-300 * t[0, 3] / vo.SQRT_LN2                                   # y = L sqrt(ln 2) / G = 1e-300
    t[1] = (1.5, 0.5 * (x[256 * 8] + x[256 * 9 - 1]), 0.02, 0.2)               # s |x_end - c| = 2 sqrt(ln 2) / 0.2 * ~2000 > 1e4
    s1 = 2.0 * vo.SQRT_LN2 / t[1, 3]
    assert t[0, 2] * vo.SQRT_LN2 / t[0, 3] < 1e-9 and s1 * np.max(np.abs(x - t[1, 1])) > 1.0e4
    th = np.stack([np.roll(t, w % 7, axis=0).reshape(-1) for w in range(nc.W)])
    want = vo.log_prob_batch_fast(base["reg"], th)
    return dict(base, t=t, th=th, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", PACKINGS)
def test_guard_walker(packing):
    c = guard_case()
    with _context(packing, c) as ctx:
        got = ctx.lnprob(c["th"])
    err = np.max(np.abs(got - c["want"]) / np.maximum(1.0, np.abs(c["want"])))
    print(f"pack {packing} guard walker: worst error {err:.2e}")
    assert np.isfinite(got).all() and err <= 1e-9


# ---- batches of moment tiles ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moment_case(kind):
    """P = 4096, two lines.  "all": both lines in the last tiles, noise 0.05 -- every tile of class 0's batch (0, 4, 8, 12)
    has no near line and takes the moment form.  "turned": a damped line in tile 3 whose wing absorbs ~0.4 at tile 0's
    nodes, data only 0.3 as deep as the model, noise 0.015 -- tile 0 is admitted on the data alone (ff_moments_try) and
    turned away by the guard after the node stage; tiles 8 and 12 of its batch take the moment form, tile 4 has the line near."""
    P, K = 4096, 2
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    rng = np.random.default_rng(len(kind))
    centre = lambda i: 0.5 * (x[256 * i] + x[256 * i + 255])
    if kind == "all":
        sd, depth = 0.05, 1.0
        t = np.array([[1.0, centre(15), 1.0, 30.0], [2.0, centre(14) + 20.0, 0.5, 15.0]])
    else:
        sd, depth = 0.015, 0.3
        t = np.array([[25.0, centre(3), 200.0, 20.0], [1.0, centre(15), 1.0, 30.0]])
    noise = np.full(P, sd)
    bounds = np.array([[x.min() - 50.0, x.max() + 50.0, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    model = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=noise, **kw), t.reshape(-1))
    flux = 1.0 - depth * (1.0 - model) + rng.normal(0, sd, P)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    th = np.stack([np.roll(t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape)), w % K, axis=0).reshape(-1)
                   for w in range(nc.W)])
    want = vo.log_prob_batch_fast(reg, th)
    # the restated guard, tile by tile, for walker 0
    S, Q, C0 = tm.tile_moments(x, flux, noise)
    near = tm.classify(t[None], x)[2][0]
    amax = np.abs(-np.expm1(-npr.node_sums_exact(t, x))).max(1)
    q0 = Q[:, :, 0].sum(1)
    tries = ~near.any(0) & tm.guard_try(C0, q0)
    takes = tries & tm.guard_ok(C0, q0, amax)
    return dict(x=x, flux=flux, noise=noise, bounds=bounds, K=K, th=th, want=want, tries=tries, takes=takes)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all", "turned"])
@pytest.mark.parametrize("packing", PACKINGS)
def test_moment_batches(packing, kind):
    c = moment_case(kind)
    batch0 = [0, 4, 8, 12]
    if kind == "all":
        assert c["takes"][batch0].all()
    else:
        assert c["tries"][0] and not c["takes"][0] and c["takes"][[8, 12]].all()
    with _context(packing, c) as ctx:
        got = ctx.lnprob(c["th"])
    err = np.max(np.abs(got - c["want"]) / np.maximum(1.0, np.abs(c["want"])))
    print(f"pack {packing} moment batch '{kind}': worst error {err:.2e}; bar {fz.BAR:.1e}")
    assert np.isfinite(got).all() and err <= fz.BAR
