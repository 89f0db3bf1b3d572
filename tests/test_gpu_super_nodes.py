"""Batches of four adjacent tiles (VAMP_DEAL_ADJ) and the distant pass (VAMP_SUPER_NODES) of the fp64 far-field loop on
the GPU, through the test hook vampdbg_node_sums_adj and vamp_lnprob.

Regions: P = 4096 (16 tiles: one adjacent batch per wavefront), P = 4396 (the same and a tail of 300 px), P = 3840 (15
tiles: no whole group, so no adjacent batch: the tile-by-tile stage alone).  K = 1 .. 16 lines, 64 walkers of seven kinds:

    all      every line inside the last super-tile: every line distant from the first one, near or far for its own
    none     every line in the middle half of the region: no line distant from any super-tile
    thr+     line 0 at the first representable centre that is distant from super-tile 0; thr-: the one before it
    mixed    lines in the outer super-tiles and in the middle: distant for one batch, near for another
    guard    `all` with a line of y = 1e-300: the guarded copy, which keeps the ordinary pass
    wide     `all` with a line wider than every tile (wide_all): the ordinary pass too

Checks: the node sums and the sets of the ordinary pairs against the restatement (tests/super_nodes_ref.py) at the bars of
tests/test_gpu_node_pass.py -- 64 ulps of the terms' magnitudes + 4e-14 of the wide lines' share on the adjacent batches,
2 x 9e-13 against scipy's wofz elsewhere; the log-posterior against the oracle at 1e-9 max(1, |lnprob|) in both
parameterisations, and packing 64 against packing 256 at the same bar."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import node_pass_ref as npr
import super_nodes_ref as snr
import tile_moments_ref as tm

ULP = 2.0 ** -53
W, SD = 64, 0.05
KINDS = ("all", "none", "thr+", "thr-", "mixed", "guard", "wide")
PS = (4096, 4396, 3840)


def grid(P):
    return np.arange(P, dtype=np.float64) - (P - 1) / 2.0


def walker(kind, K, rng, x):
    """native[K, 4] = (A, c, L, G)"""
    P = x.size
    st0 = snr.super_tile(x, [0, 1, 2, 3]) if P >= 1024 else None
    last = (x[256 * 12 + 20], x[min(256 * 16, P) - 21])                  # inside the last super-tile's tiles
    mid = (-1000.0, 1000.0)
    A, G, L = rng.uniform(0.5, 3.0, K), rng.uniform(20.0, 60.0, K), 10.0 ** rng.uniform(-1.0, 0.5, K)
    if kind in ("all", "guard", "wide"):
        c = rng.uniform(*last, K)
    elif kind == "mixed":
        c = np.where(np.arange(K) % 3 == 0, rng.uniform(*last, K), np.where(np.arange(K) % 3 == 1, rng.uniform(x[20], x[1000], K),
                                                                            rng.uniform(*mid, K)))
    else:
        c = rng.uniform(*mid, K)
    if kind in ("thr+", "thr-"):
        Mid, Half = st0
        G[0], L[0] = 30.0, 1.0
        s0 = 2.0 * npr.SQRT_LN2 / G[0]
        y0 = L[0] * npr.SQRT_LN2 / G[0]
        c0 = Mid + Half + snr.SUPER_DIST * Half             # (the distance decides: every operation of it rounds as the kernel's)
        while not snr.super_distant(c0, s0, y0, Mid, Half)[0]:
            c0 = np.nextafter(c0, np.inf)
        while snr.super_distant(np.nextafter(c0, Mid), s0, y0, Mid, Half)[0]:
            c0 = np.nextafter(c0, Mid)
        c[0] = c0 if kind == "thr+" else np.nextafter(c0, Mid)
    if kind == "guard":
        L[0] = 1e-300 * G[0] / npr.SQRT_LN2
    if kind == "wide":
        G[0], c[0] = 400.0, rng.uniform(*mid)
    return np.stack([A, c, L, G], 1)


@functools.lru_cache(maxsize=None)
def case(P, K):
    x = grid(P)
    rng = np.random.default_rng(100 * P + K)
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
    return dict(x=x, flux=flux, noise=noise, th=th, nat=nat, want=want, bounds=bounds, K=K)


def _context(packing, c, **kw):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0)
    ctx.set_packing(packing)
    ctx.set_regions(c["x"], c["flux"], c["noise"], c["K"], mode=kw.pop("mode", vamp_amd.MODE_VOIGT4), bounds=c.get("bounds"), **kw)
    return ctx


def _apart(a, b):
    """two packings against each other, in the unit of the suite's bar (the one-walker-per-wavefront shape has no Taylor
    tables: its near lines round differently, so the shapes agree to the bar, not to the bit)"""
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def _node_sums(ctx, theta, ntile):
    fn = ctx._lib.vampdbg_node_sums_adj
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    th = np.ascontiguousarray(theta, np.float64)
    nodes, sets = np.full((ntile, 16), np.nan), np.zeros((ntile, 5), np.uint32)
    n = fn(ctx._h, 0, th.ctypes.data, nodes.ctypes.data, sets.ctypes.data)
    assert n == ntile, (n, ctx._lib.vamp_last_error())
    return nodes, sets


def test_the_walkers_are_what_they_are_named_for():
    """on the host: which walkers have distant lines, and where"""
    for K in (1, 2, 7, 16):
        c = case(4096, K)
        x = c["x"]
        for w, kind in enumerate(KINDS):
            sets = snr.class_sets(c["nat"][w], x)
            d0, dany = sets[0]["dist"], any(s["dist"] for s in sets)
            if kind == "all":
                assert d0 == (1 << K) - 1 and sets[3]["dist"] == 0
            elif kind in ("none", "guard", "wide", "thr-"):
                assert not dany, (K, kind)
            elif kind == "thr+":
                assert d0 == 1
            elif K >= 2:
                assert d0 and sets[3]["dist"] and d0 != sets[3]["dist"]           # distant for one batch, not for another
            assert snr.super_ok(c["nat"][w], x) == (kind not in ("guard", "wide"))
    assert len(snr.batches(15)[0]) == 0 and len(snr.batches(17)[0]) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("K", (1, 2, 7, 16))
@pytest.mark.parametrize("P", PS)
def test_node_sums_match_the_restatement(P, K):
    c = case(P, K)
    x, ntile = c["x"], P // 256
    full, rest = snr.batches(ntile)
    worst_full = worst_rest = 0.0
    with _context(256, c) as ctx:
        ctx._lib.vampdbg_super_nodes.restype = C.c_int
        on = bool(ctx._lib.vampdbg_super_nodes())         # the library as built: with the distant pass or without
        for w in range(3 * len(KINDS)):                   # three walkers of every kind
            native = c["nat"][w]
            got, gsets = _node_sums(ctx, c["th"][w], ntile)
            assert np.isfinite(got).all()
            want, mag, magw = snr.node_sums(native, x, super_on=on)
            heads = {int(s["tiles"][0]): s for s in snr.class_sets(native, x, super_on=on)}
            for t in range(ntile):
                if t in heads:
                    s = heads[t]
                    assert [int(v) for v in gsets[t]] == [s["far"], s["n6"], s["n4"], s["n3"], s["wide"]], (KINDS[w % len(KINDS)], t)
                else:
                    assert (gsets[t] == 0xffffffff).all(), (KINDS[w % len(KINDS)], t)
            if len(full):
                ft = full.reshape(-1)
                tol = 64 * ULP * mag[ft] + 4e-14 * magw[ft]
                ratio = np.abs(got[ft] - want[ft]) / np.maximum(tol, 1e-300)
                print(f"P={P} K={K} {KINDS[w % len(KINDS)]:6s}: node sums of the adjacent batches at {ratio.max():.3f} of their bar")
                worst_full = max(worst_full, ratio.max())
            if rest:
                worst_rest = max(worst_rest, np.max(np.abs(got[rest] - want[rest]) / np.maximum(2 * 9e-13 * mag[rest], 1e-300)))
    print(f"P={P} K={K} (distant pass {'on' if on else 'off'}): node sums nearest their bars: adjacent batches {worst_full:.3f}, other tiles {worst_rest:.3f}")
    assert worst_full <= 1.0 and worst_rest <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("K", range(1, 17))
def test_lnprob_matches_oracle_and_packings_agree(K):
    c = case(4096, K)
    got = {}
    for packing in (0, 256, 64):
        with _context(packing, c) as ctx:
            got[packing] = ctx.lnprob(c["th"])
    want = c["want"]
    assert np.isfinite(want).all()
    for packing, g in got.items():
        err = np.max(np.abs(g - want) / np.maximum(1.0, np.abs(want)))
        print(f"pack {packing} K={K}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err:.2e}")
        assert np.isfinite(g).all() and err <= 1e-9
    assert _apart(got[64], got[256]) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("K", (7, 16))
@pytest.mark.parametrize("P", PS[1:])
def test_lnprob_with_a_tail_and_without_a_batch(P, K):
    c = case(P, K)
    got = {}
    for packing in (256, 64):
        with _context(packing, c) as ctx:
            got[packing] = ctx.lnprob(c["th"])
    err = max(np.max(np.abs(g - c["want"]) / np.maximum(1.0, np.abs(c["want"]))) for g in got.values())
    print(f"P={P} K={K}: worst error {err:.2e}")
    assert err <= 1e-9 and _apart(got[64], got[256]) <= 1e-9


@functools.lru_cache(maxsize=None)
def nbz_case(K):
    from bench import make_workload
    wl = make_workload(P=4096, K=K, W=W, seed=77 + K, nbz=True)
    l_fixed, line, x_origin, x_scale = [float(v) for v in wl["nbz"][0]]
    r = vo.Region(x=wl["x"], flux=wl["flux"], noise=wl["noise"], n_comp=K, mode=vo.MODE_NBZ3, l_fixed=l_fixed, line=line,
                  x_origin=x_origin, x_scale=x_scale)
    # the walkers' lines in native form (the same draws in the four-parameter form, the Lorentzian width fixed): how many
    # walkers have a line distant from some batch -- the cases must exercise the distant pass in this parameterisation too
    nat = make_workload(P=4096, K=K, W=W, seed=77 + K, nbz=False)["theta0"].reshape(W, K, 4).copy()
    nat[:, :, 2] = l_fixed
    ndist = sum(any(s["dist"] for s in snr.class_sets(n, wl["x"])) for n in nat)
    return wl, vo.log_prob_batch_fast(r, wl["theta0"]), ndist


@pytest.mark.gpu
@pytest.mark.parametrize("K", (2, 5, 16))
def test_lnprob_in_the_three_parameter_form(K):
    import vamp_amd
    wl, want, ndist = nbz_case(K)
    assert ndist >= W // 2, ndist
    got = {}
    for packing in (256, 64):
        ctx = vamp_amd.HipContext(device=0)
        with ctx:
            ctx.set_packing(packing)
            ctx.set_regions(wl["x"], wl["flux"], wl["noise"], K, mode=vo.MODE_NBZ3, nbz=wl["nbz"])
            got[packing] = ctx.lnprob(wl["theta0"])
    err = max(np.max(np.abs(g - want) / np.maximum(1.0, np.abs(want))) for g in got.values())
    print(f"nbz3 K={K}: worst error {err:.2e}")
    assert np.isfinite(want).all() and err <= 1e-9 and _apart(got[64], got[256]) <= 1e-9
