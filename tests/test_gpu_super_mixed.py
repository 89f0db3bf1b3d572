"""The distant pass (VAMP_SUPER_NODES) chosen walker by walker inside the one loop of the walkers without a guard bit: one
launch holds walkers that take the pass, walkers with a line wide for every tile (wide_all: the same loop, the pass
skipped at one scalar branch per batch) and walkers with a guard bit (the guarded copy of the loop).

Walkers: the recipe of tests/test_gpu_super_nodes.py (its seven kinds in turn), W = 64, K = 1, 2, 15, 16 lines.
Regions: P = 4096 (one group of 16 tiles: four batches, the smallest region that has a batch), P = 4452 (one group, a tile
no group holds and a tail of 100 px), P = 8192 (two groups).

Bars: the log-posterior against the oracle and packing 64 against packing 256 at 1e-9 max(1, |lnprob|), the bar of the
neighbouring tests; two stretch steps against the oracle's stretch move evaluating its proposals with the library's own
vamp_lnprob (tests/test_gpu_parity.py's construction): the same accept decisions, positions to 1e-10; the log-posterior
of one walker alone, among others, through k_lnprob and through a half-step: the same bits; a line stepped across the
distance from which it is distant: the two sides' node sums apart by no more than the node sums' bar of
tests/test_gpu_super_nodes.py (64 ulps of the terms' magnitudes + 4e-14 of the wide lines' share) on either side, and the
log-posterior by that bar carried at unit gain into chi^2, see test_a_line_stepped_across_the_threshold."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import node_pass_ref as npr
import super_nodes_ref as snr
from test_gpu_super_nodes import KINDS, SD, ULP, W, _apart, _context, _node_sums, grid, walker

PS = (4096, 4096 + 256 + 100, 8192)
KS = (1, 2, 15, 16)


@functools.lru_cache(maxsize=None)
def case(P, K):
    x = grid(P)
    rng = np.random.default_rng(7000 * P + K)
    nat = np.stack([walker(KINDS[w % len(KINDS)], K, rng, x) for w in range(W)])
    th = nat.reshape(W, 4 * K)
    noise = np.full(P, SD)
    bounds = np.array([[x.min() - 50.0, x.max() + 50.0, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=noise, **kw), th[0]) + rng.normal(0, SD, P)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    want = vo.log_prob_batch_fast(reg, th)
    for a in (x, flux, noise, th, want, bounds, nat):
        a.setflags(write=False)
    return dict(x=x, flux=flux, noise=noise, th=th, nat=nat, want=want, bounds=bounds, K=K, reg=reg)


def _kinds(c):
    """per walker: takes the pass for some batch / has a line wide for every tile or a guard bit"""
    takes = np.array([snr.super_ok(n, c["x"]) and any(s["dist"] for s in snr.class_sets(n, c["x"])) for n in c["nat"]])
    barred = np.array([not snr.super_ok(n, c["x"]) for n in c["nat"]])
    return takes, barred


def test_every_launch_holds_every_kind_of_walker():
    """on the host: walkers that take the pass, wide_all walkers and guard walkers sit side by side in every case"""
    for P in PS:
        for K in KS:
            c = case(P, K)
            takes, barred = _kinds(c)
            kinds = np.array([KINDS[w % len(KINDS)] for w in range(W)])
            assert takes.sum() >= W // 7 and (barred & (kinds == "wide")).sum() >= 9 and (barred & (kinds == "guard")).sum() >= 9, (P, K)
            assert not (takes & barred).any()
            assert np.isfinite(c["want"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", PS)
def test_lnprob_of_a_mixed_launch(P, K):
    c = case(P, K)
    got = {}
    for packing in (256, 64):
        with _context(packing, c) as ctx:
            got[packing] = ctx.lnprob(c["th"])
    want = c["want"]
    for packing, g in got.items():
        err = np.max(np.abs(g - want) / np.maximum(1.0, np.abs(want)))
        print(f"P={P} K={K} pack {packing}: worst error {err:.2e}")
        assert np.isfinite(g).all() and err <= 1e-9
    apart = _apart(got[64], got[256])
    print(f"P={P} K={K}: packings apart by {apart:.2e}")
    assert apart <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", PS)
def test_two_steps_of_a_mixed_ensemble(P, K):
    c = case(P, K)
    th = np.array(c["th"])
    with _context(0, c) as ctx, _context(0, c) as ev:
        # (vamp_lnprob runs n points in the shape of an n-walker ensemble: a half-step's W / 2 proposals, each twice)
        fn = lambda q: ev.lnprob(np.concatenate([q, q]))[:len(q)]
        lnp0 = ev.lnprob(th)
        ctx.sampler_init(th, seed=4242 + K, a=2.0, split_block=16)
        res = ctx.run(2)
        chain, lchain, nacc = vo.run_sampler(fn, th, lnp0, 2, seed=4242 + K, block=16)
    print(f"P={P} K={K}: accepted {int(nacc.sum())} of {2 * W}")
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)
    # and the ensemble's stored log-posterior against the oracle itself
    err = np.max(np.abs(res["lnprob"][-1] - vo.log_prob_batch_fast(c["reg"], res["chain"][-1])) / np.maximum(1.0, np.abs(res["lnprob"][-1])))
    assert err <= 1e-9, err


def _same_bits_four_ways(c, w, others, partner):
    """Walker w's proposal against `partner` with z = 1 (the walker itself to rounding), accepted whatever its value: its
    log-posterior as a half-step of a two-walker ensemble records it, as a half-step records it in which 31 of `others`
    move beside it in an ensemble of 64, from k_lnprob alone and from k_lnprob among the 63 `others`"""
    th = c["th"]
    always = -1.0e300
    pool = th[np.resize(np.asarray(others), W - 1)]
    with _context(0, c) as ctx:
        ctx.sampler_init(np.stack([th[w], th[partner]]), seed=1, split_block=2)
        ctx.half_step_ext([0], [1], [1.0], [always])
        X, lnp, nacc, _ = ctx.get_state()
        assert nacc[0] == 1
        Y, step_alone = X[0].copy(), lnp[0]
        n = W // 2
        ens = np.concatenate([th[w][None, :], pool[:n - 1], th[partner][None, :], pool[n - 1:W - 2]])
        ctx.sampler_init(ens, seed=1, split_block=W)
        ctx.half_step_ext(np.arange(n), np.full(n, n), np.ones(n), np.full(n, always))
        X2, lnp2, nacc2, _ = ctx.get_state()
        assert nacc2[0] == 1 and np.array_equal(X2[0], Y)
        step_among = lnp2[0]
        alone = ctx.lnprob(Y[None, :])[0]
        among = ctx.lnprob(np.concatenate([pool[:40], Y[None, :], pool[40:]]))[40]
    return Y, (alone, among, step_alone, step_among)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", PS)
def test_the_pass_is_a_function_of_the_walker_alone(P, K):
    c = case(P, K)
    x = c["x"]
    takes, barred = _kinds(c)
    kinds = np.array([KINDS[w % len(KINDS)] for w in range(W)])
    others = [int(v) for v in np.flatnonzero(barred)]          # wide_all and guard walkers, in turn
    assert len(others) >= 18
    partner, others = others[0], others[1:]
    for name, w in (("pass", int(np.flatnonzero(takes & (kinds == "all"))[0])), ("wide_all", int(np.flatnonzero(kinds == "wide")[1]))):
        oth = [o for o in others if o != w]
        Y, vals = _same_bits_four_ways(c, w, oth, partner)
        nat = Y.reshape(K, 4)
        if name == "pass":
            assert snr.super_ok(nat, x) and any(s["dist"] for s in snr.class_sets(nat, x))
        else:
            assert not snr.super_ok(nat, x)
        print(f"P={P} K={K} {name}: alone, among, half-step alone, half-step among = " + ", ".join(repr(float(v)) for v in vals))
        assert np.isfinite(vals[0]) and all(v == vals[0] for v in vals), (name, vals)
        want = vo.log_prob_batch_fast(c["reg"], Y[None, :])[0]
        assert abs(vals[0] - want) <= 1e-9 * max(1.0, abs(want))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_a_line_stepped_across_the_threshold(K):
    """Line 0's centre at the first representable value from which the line is distant for super-tile 0, and at the one
    before it (the recipe's thr+ and thr-): on one side the line goes through the 16 super-nodes of batch 0, on the other
    through the batch's ordinary pairs.  The bar is the node sums' own, tol = 64 ulps mag + 4e-14 magw
    (tests/test_gpu_super_nodes.py): each side within tol of its restatement, and the two sides' node sums of batch 0
    within tol+ + tol- of each other, node by node.  For the log-posterior the same bar is carried at unit gain through
    lnprob = -1/2 sum r^2, r = (f - exp(-tau)) w: sum over the batch's pixels of |r| w m (tol+ + tol-) of their tile (no
    allowance for the interpolation's gain: stricter than the bound), plus what the step itself moves, the two sides
    being two points one ulp of c apart: sum |r| w m amp s ulp(c) (|dH/dX| < 1)."""
    P = 4096
    x = grid(P)
    nat = {kind: walker(kind, K, np.random.default_rng(31 + K), x) for kind in ("thr+", "thr-")}
    assert np.array_equal(nat["thr+"][1:], nat["thr-"][1:]) and np.array_equal(nat["thr+"][0, [0, 2, 3]], nat["thr-"][0, [0, 2, 3]])
    c_hi, c_lo = nat["thr+"][0, 1], nat["thr-"][0, 1]
    assert c_lo == np.nextafter(c_hi, -np.inf)
    sets = {kind: snr.class_sets(n, x)[0] for kind, n in nat.items()}
    assert sets["thr+"]["dist"] & 1 and not sets["thr-"]["dist"] & 1
    c = dict(case(P, K))
    th = np.stack([nat["thr+"].reshape(-1), nat["thr-"].reshape(-1)])
    with _context(256, c) as ctx:
        ctx._lib.vampdbg_super_nodes.restype = C.c_int
        on = bool(ctx._lib.vampdbg_super_nodes())
        got = ctx.lnprob(th)
        nodes = {kind: _node_sums(ctx, th[i], P // 256)[0] for i, kind in enumerate(("thr+", "thr-"))}
    reg = c["reg"]
    w = 1.0 / c["noise"]
    bar = 0.0
    tol_t = np.zeros(P // 256)
    tol_n = np.zeros((4, 16))
    for kind, n in nat.items():
        want, mag, magw = snr.node_sums(n, x, super_on=on)
        tol = 64 * ULP * mag + 4e-14 * magw
        assert np.all(np.abs(nodes[kind][:4] - want[:4]) <= tol[:4]), kind
        tol_t[:4] += tol[:4].max(1)
        tol_n += tol[:4]
    for i, kind in enumerate(("thr+", "thr-")):
        m = vo.model_flux(reg, th[i])
        sens = np.abs((c["flux"] - m) * w) * w * m
        a, _, L, G = nat[kind][0]
        amp, s = a * L * np.sqrt(np.pi) * npr.SQRT_LN2 / G, 2.0 * npr.SQRT_LN2 / G
        d_tau = np.repeat(tol_t, 256) + amp * s * (c_hi - c_lo)
        bar = max(bar, float(np.sum(sens * d_tau)))
    apart = abs(got[0] - got[1])
    node_apart = np.max(np.abs(nodes["thr+"][:4] - nodes["thr-"][:4]) / np.maximum(tol_n, 1e-300))
    print(f"K={K} (distant pass {'on' if on else 'off'}): lnprob {float(got[0])!r} / {float(got[1])!r}, apart {apart:.3e}, bar {bar:.3e}; "
          f"node sums apart {node_apart:.3f} of tol+ + tol-")
    assert node_apart <= 1.0
    assert np.isfinite(got).all() and apart <= bar
