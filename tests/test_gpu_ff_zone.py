"""The fp64 tile sweep with the lines' Taylor tables (workgroup per walker) takes, for a near (line, tile) pair whose
tile lies wholly inside the line's table zone, the table at once: the bit comes from the far-field classification
(vamp::ff_tile_in_zone, one 16-bit field per tile next to the far and the wide mask) instead of four votes over the
pixels' r2 in tile_voigt.  Same function, same arguments: the values are those of the other route.  What can go wrong is
the bookkeeping -- the bit of line k of tile j of a batch of four reaching another line or tile, a partial batch, a
descending grid, a walker's copy of the loop (guarded, wide) -- and a bit set for a tile that is not inside the zone,
which reads past the table's last row.

Shapes: P = 2304 (nine full tiles: the wavefronts of a workgroup get 3 / 2 / 2 / 2, so every first batch is partial),
P = 2148 (eight tiles and a tail), P = 768 under packing 64 (one walker per wavefront: the same loop without tables, which
must not see the bit); K = 1 and 16; VOIGT4 and NBZ3; ascending and descending grids; W = 64 walkers, the lines of
test_gpu_tile_tables.make_lines rotated through the slots, and planted walkers:
   3  a line on the middle of every tile: every tile has near lines
   7  all lines inside the last tile: no other tile has a near line
  11  a y < Y_TINY line, 13 a line that reaches X > X_FAR: the guarded copy of the loop   (11: VOIGT4 only)
  17  a line of 350 px: the copy with lines wider than a tile
  19  |z| = 8 of a line exactly on a tile's NEARER edge (the next tile is wholly outside the zone)
  23  |z| = 8 of a line exactly on its own tile's FARTHER edge (bit clear by the margin; tile_voigt decides)
The CPU half counts, with the host build of the predicate, the near pairs with the bit set and clear in every case and
for the planted walkers, so that each case is known to run both routes.

Bar: relative error of the log-posterior against the oracle, |delta| / max(1, |lnprob|).  The parent commit's worst
error over these very cases was measured on an MI355X (profiles/zone_bit_ab.txt) and the bar is ten times that, but
never above the project's 1e-9 and never below 1e-13; two sampler steps: identical accept counts, positions to 1e-10."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import test_gpu_tile_tables as tt
import zero_residual as zr

TILE, W, SD = tt.TILE, tt.W, tt.SD
NBZ = np.array([0.7, 1215.67, 2.4e15, 4.0e10])            # l_fixed, line, x_origin, x_scale (tests/test_gpu_sweep_pixels.py)
PAD = 4000.0
MODES = {"voigt4": vo.MODE_VOIGT4, "nbz3": vo.MODE_NBZ3}
SHAPES = ((2304, 256), (2148, 256), (768, 64))            # (P, packing)
KS = (1, 16)
KINDS = ("up", "down")
PARENT_WORST = 7.076e-14      # P = 2304, descending, K = 16, VOIGT4, workgroup per walker: the parent commit on an MI355X
BAR = min(1.0e-9, max(1.0e-13, 10.0 * PARENT_WORST))
R2_CORE, FF_DIST, WIDE_MAX, MID_Z2 = 64.0, 2.0, 0.75, 30.25       # vamp_hip.hip


def _w8(L, G):
    s, y = 2.0 * vo.SQRT_LN2 / G, L * vo.SQRT_LN2 / G
    return np.sqrt(max(R2_CORE - y * y, 0.0)) / s


def planted(x, K, mode):
    """{walker: [K', 4] rows (A, c, L, G) that replace its first lines}"""
    n, d = x.size // TILE, np.sign(x[1] - x[0])                   # tiles in index order, as the sweep deals them
    mids = [0.5 * (x[TILE * i] + x[TILE * i + TILE - 1]) for i in range(n)]
    Lx = NBZ[0] if mode == vo.MODE_NBZ3 else 0.5
    out = {
        3: [(1.0, mids[i % n] + 0.25 * (i // n), Lx, 50.0) for i in range(K)],
        7: [(0.8, x[TILE * (n - 1)] + d * (i + 0.5) * TILE / K, Lx, 6.0) for i in range(K)],
        13: [(2.0, mids[1] + 40.3, 0.01, 0.05)],
        17: [(20.0, mids[n // 2] + 17.0, Lx, 350.0)],
        19: [(1.5, x[TILE * 2] - d * _w8(Lx, 32.0), Lx, 32.0)],           # centre in tile 1, |z| = 8 on the first pixel of tile 2
        23: [(1.5, x[TILE * 2 - 1] - d * _w8(Lx, 32.0), Lx, 32.0)],       # ... on the last pixel of tile 1
    }
    if mode == vo.MODE_VOIGT4:
        out[11] = [(1.5, mids[1], 80.0 * 1.0e-10, 80.0)]
    return out


@functools.lru_cache(maxsize=None)
def case(P, kind, K, mname):
    mode = MODES[mname]
    x = tt.make_grid(P, kind)
    rng = np.random.default_rng(7 * P + 10 * K + len(kind) + mode)
    t = tt.make_lines(x, K, rng)
    if mode == vo.MODE_NBZ3:
        t[:, 2] = NBZ[0]
    noise = np.full(P, SD)
    bounds = np.array([[x.min() - PAD, x.max() + PAD, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=mode, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    nbz = NBZ if mode == vo.MODE_NBZ3 else None
    if nbz is not None:
        kw.update(l_fixed=NBZ[0], line=NBZ[1], x_origin=NBZ[2], x_scale=NBZ[3])
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=noise, **kw), zr.native_to_mode(t, mode, nbz)) + rng.normal(0, SD, P)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    plant = planted(x, K, mode)
    native = []
    for w in range(W):
        tw = np.roll(t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape)), w % K, axis=0)
        for i, row in enumerate(plant.get(w, ())[:K]):
            tw[i] = row
        if mode == vo.MODE_NBZ3:
            tw[:, 2] = NBZ[0]
        native.append(tw)
    th = np.array([zr.native_to_mode(tw, mode, nbz) for tw in native])
    return tt._freeze(dict(x=x, flux=flux, noise=noise, th=th, want=vo.log_prob_batch_fast(reg, th), bounds=bounds, reg=reg, K=K,
                           native=np.array(native), mode=mode, nbz=nbz, walkers=tuple(sorted(plant))))


CASES = [(P, pack, kind, K, m) for P, pack in SHAPES for kind in KINDS for K in KS for m in MODES]


# ---- which route each near pair takes (host) --------------------------------------------------------------------------
def _pred():
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "libff_pred_host.so")
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    return C.CDLL(so)


def routes(c):
    """[W, K, tiles] booleans (near, zone): the classification's rules (ff_classify_batch) and the predicate's host build"""
    x, nat = c["x"], c["native"]
    n = x.size // TILE
    lo, hi = x[TILE * np.arange(n)], x[TILE * np.arange(n) + TILE - 1]
    mid, half = 0.5 * (lo + hi), 0.5 * np.abs(hi - lo)
    cc, L, G = nat[:, :, 1], nat[:, :, 2], nat[:, :, 3]
    rG = 1.0 / G
    s, y = (2.0 * vo.SQRT_LN2) * rG, (L * vo.SQRT_LN2) * rG
    w8 = np.sqrt(np.maximum(R2_CORE - y * y, 0.0)) / s
    wmid = np.sqrt(np.maximum(MID_Z2 - y * y, 0.0)) / s
    dist = np.abs(mid[None, None, :] - cc[:, :, None]) - half[None, None, :]
    away = dist >= FF_DIST * half[None, None, :]
    far = away & (dist >= w8[:, :, None])
    span = np.max(np.abs(hi - lo))
    wide = ((s * (0.5 * span) <= WIDE_MAX)[:, :, None] | (away & (dist >= wmid[:, :, None]))) & ~far
    near = ~(far | wide)
    shape = near.shape
    full = lambda a: np.ascontiguousarray(np.broadcast_to(a, shape), dtype=np.float64).ravel()
    bit = np.zeros(near.size, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [full(cc[:, :, None]), full(s[:, :, None]), full(y[:, :, None]), full(mid[None, None, :]), full(half[None, None, :])]
    _pred().ff_tile_in_zone_host(C.c_int64(near.size), *[p(a) for a in args], p(bit))
    return near, bit.reshape(shape).astype(bool)


@pytest.mark.parametrize("P,pack,kind,K,m", [c for c in CASES if c[1] == 256])
def test_every_case_takes_both_routes(P, pack, kind, K, m):
    c = case(P, kind, K, m)
    assert np.isfinite(c["want"]).all()
    near, zone = routes(c)
    n_set, n_clear = int((near & zone).sum()), int((near & ~zone).sum())
    per = {w: (int((near[w] & zone[w]).sum()), int((near[w] & ~zone[w]).sum())) for w in c["walkers"]}
    msg = f"P={P} {kind} K={K} {m}: near pairs with the bit set {n_set}, clear {n_clear}; planted walkers (set, clear) {per}"
    print(msg)
    assert n_set > 0 and n_clear > 0, msg
    nt = P // TILE
    if K == 16:
        assert near[3].any(axis=0).all(), "walker 3: a tile without a near line"
        assert not near[7][:, :nt - 2].any(), "walker 7: a near line away from the last tiles"
    # walker 19: the tile at whose nearer edge |z| = 8 falls is near and NOT in the zone, its neighbour towards the centre is;
    # walker 23: the centre's own tile has its farther edge on |z| = 8: near, bit clear
    assert near[19, 0, 2] and not zone[19, 0, 2] and near[19, 0, 1] and zone[19, 0, 1], msg
    assert near[23, 0, 1] and not zone[23, 0, 1], msg


# ---- GPU --------------------------------------------------------------------------------------------------------------
def _ctx(packing):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0)
    ctx.set_packing(packing)
    return ctx


def _set(ctx, c):
    ctx.set_regions(c["x"], c["flux"], c["noise"], c["K"], mode=c["mode"], bounds=c["bounds"], nbz=None if c["nbz"] is None else c["nbz"][None, :])


@pytest.mark.gpu
@pytest.mark.parametrize("P,pack,kind,K,m", CASES)
def test_lnprob_matches_oracle(P, pack, kind, K, m):
    c = case(P, kind, K, m)
    with _ctx(pack) as ctx:
        _set(ctx, c)
        got = ctx.lnprob(c["th"])
        alone = np.array([ctx.lnprob(c["th"][w:w + 1])[0] for w in c["walkers"]])
    want = c["want"]
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"ZONE-ERR P={P} pack={pack} {kind} K={K} {m}: worst {err.max():.3e} (walker {int(err.argmax())}), "
          f"planted {', '.join('%d: %.2e' % (w, err[w]) for w in c['walkers'])}; bar {BAR:.1e}")
    assert np.array_equal(alone, got[list(c["walkers"])]), "a planted walker's value depends on its batch"
    assert err.max() <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("m", list(MODES))
@pytest.mark.parametrize("kind", KINDS)
def test_two_sampler_steps_match_oracle(kind, m):
    c = case(2304, kind, 16, m)
    with _ctx(256) as ctx:
        _set(ctx, c)
        ctx.sampler_init(c["th"], seed=2304, a=2.0, split_block=W)
        res = ctx.run(2)
    chain, lchain, nacc = vo.run_sampler(lambda q: vo.log_prob_batch_fast(c["reg"], q), c["th"], c["want"], 2, seed=2304, block=W)
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)
