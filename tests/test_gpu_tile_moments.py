"""The fp64 far-field loop sums chi^2 of a tile WITHOUT a near line from per-context data moments (sweep_range_ff,
ff_moment_chi, vamp_amd/csrc/ff_moments.hpp) when the guard vamp::ff_moments_ok admits the tile.  What can go wrong: the
moments of the wrong tile or quarter (orientation, partial batches, tile classes of the four wavefronts), a tile with a
near line taking the path, the guard letting a tile through whose cancellation matters, the mark of a finished tile
reaching another one.

Shapes: P = 1024 (one tile per wavefront of the workgroup) and P = 2304 (nine tiles: 3 / 2 / 2 / 2, every first batch is
partial), packing 256; ascending, descending and uneven ("steps": unit and double spacing alternate tile by tile) grids;
K = 1, 4, 16; NBZ3 and VOIGT4; 64 walkers (walker 0 exact, the others moved by 1e-4 and rotated through the slots).
Placements of the lines:
  a  half of the lines 330..420 pixels before the region's first pixel with damped wings (far from every tile), the
     others narrow in the region's last tile: the first two tiles at least have no near line.  sigma = 0.01.
       a1  noisy data: lnprob against the oracle within test_gpu_ff_zone's bar.
       a2  localised on the first tile (noise 1e30 elsewhere), data the model fits to ~1e-6 of a tile's chi^2: the path's
           rounding signature -- some walker's chi^2 deviates from the oracle's by more than 1e-12 of itself, every
           walker's by less than the guard's bound 2^-40 x 256.
  b  the same lines, exact data, weights 1e10 (the zero-residual form): chi^2 <= 1 for every (exact) walker, which the
     moment form cannot deliver (its rounding there is ~1e3): the guard must send these tiles pixel by pixel.
  c  a line of 1.2 half-widths on tile middles, every tile has a near line: no tile takes the path.  K = 1 on nine
     tiles: one line near all nine exists in a narrow window only (uniform grid: on the middle tile, 2.13 .. 2.22
     half-widths -- narrower and the outermost tiles are outside its Gaussian core, wider and it counts as wider than a
     tile; both go to the wide list); one_line_near_all finds the window of each grid by scanning place and width.
The host half applies the numpy model (tests/tile_moments_ref.py: classification, moments, guard) to every case, so
that each is known to be what its name says."""
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import test_gpu_ff_zone as fz
import test_gpu_tile_tables as tt
import tile_moments_ref as tm
import zero_residual as zr

TILE, W, SD = 256, 64, 0.01
SHAPES, KINDS, KS = (1024, 2304), ("up", "down", "steps"), (1, 4, 16)
MODES = fz.MODES
PLACEMENTS = ("a", "b", "c")
CASES = [(P, kind, K, m, pl) for P in SHAPES for kind in KINDS for K in KS for m in MODES for pl in PLACEMENTS]
MODEL_WALKERS = (0, 1, W - 1)


def nbz_of(x):
    """l_fixed, line, x_origin, x_scale: a fixed Lorentzian width of ten (widest) pixels, as the benchmark's workload has"""
    return np.array([10.0 * np.max(np.abs(np.diff(x))), fz.NBZ[1], fz.NBZ[2], fz.NBZ[3]])


def one_line_near_all(x, L):
    """(c, L, G) of ONE line that ff_classify_batch lists as near for every full tile of x: the middle of the window found
    by scanning places and widths with the numpy restatement of the classification"""
    xa = np.sort(x)
    cc, gg = np.meshgrid(np.linspace(xa[0], xa[-1], 361), np.geomspace(50.0, 2000.0, 800))
    native = np.stack([np.ones(cc.size), cc.ravel(), np.full(cc.size, L), gg.ravel()], axis=1)[:, None, :]
    ok = tm.classify(native, x)[2][:, 0, :].all(axis=1)
    assert ok.any(), "no single line is near every tile of this grid"
    c_ok, g_ok = cc.ravel()[ok], gg.ravel()[ok]
    g = np.median(g_ok)
    c = np.median(c_ok[np.abs(g_ok - g) <= 0.01 * g])
    cand = np.argmin((c_ok - c) ** 2 / (xa[-1] - xa[0]) ** 2 + (np.log(g_ok / g)) ** 2)
    return float(c_ok[cand]), float(L), float(g_ok[cand])


def lines(x, K, placement, mode, rng):
    xa = np.sort(x)
    dx, nt = np.max(np.diff(xa)), xa.size // TILE
    Lx = nbz_of(x)[0] if mode == vo.MODE_NBZ3 else None
    if placement == "c":
        half_max = 0.5 * max(xa[TILE * i + TILE - 1] - xa[TILE * i] for i in range(nt))
        mids = [0.5 * (xa[TILE * i] + xa[TILE * i + TILE - 1]) for i in range(nt)]
        if K == 1:
            at = [0.5 * (xa[0] + xa[-1])]
        elif K < nt:
            at = [mids[i] for i in range(1, nt, 2)][:K]
        else:
            at = [mids[i % nt] + 0.37 * (i // nt) * dx for i in range(K)]
        if K == 1 and nt == 9:
            return np.array([(rng.uniform(0.5, 1.5),) + one_line_near_all(x, Lx or 0.5)])
        return np.array([(rng.uniform(0.5, 1.5), c, Lx or 0.5, 1.2 * half_max) for c in at])
    n_left, d = (K + 1) // 2, np.sign(x[1] - x[0])               # "before" and "last" in INDEX order, as the sweep deals the tiles
    # damped wings that TOGETHER absorb a few 1e-3 in the first tile whatever K and the spacing (tau ~ 10 A L / d^2 at d
    # pixels): the moment form's rounding, ~0.1 x 8 2^-53 M, is measurable against 1e-12 of the a2 data's chi^2 (2.6e-16)
    # only from M ~ 30 on, i.e. from an absorption of ~3e-3 at sigma = 0.01 (test_cases_are_what_they_say asserts M)
    left = [(rng.uniform(14.0, 20.0) * dx / n_left, x[0] - d * rng.uniform(330.0, 420.0) * dx, Lx or rng.uniform(10.0, 20.0) * dx,
             rng.uniform(15.0, 30.0)) for _ in range(n_left)]
    last = [(rng.uniform(0.5, 2.0), x[-1] - d * rng.uniform(20.0, 200.0), Lx or 0.5, rng.uniform(6.0, 10.0)) for _ in range(K - n_left)]
    return np.array(left + last)


@functools.lru_cache(maxsize=None)
def case(P, kind, K, mname, placement):
    mode = MODES[mname]
    x = tt.make_grid(P, kind)
    rng = np.random.default_rng(P + 10 * K + len(kind) + 100 * mode + ord(placement))
    t = lines(x, K, placement, mode, rng)
    nbz = nbz_of(x) if mode == vo.MODE_NBZ3 else None
    bounds = np.array([[x.min() - fz.PAD, x.max() + fz.PAD, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=mode, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    if nbz is not None:
        kw.update(l_fixed=nbz[0], line=nbz[1], x_origin=nbz[2], x_scale=nbz[3])
    exact = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=np.ones(P), **kw), zr.native_to_mode(t, mode, nbz))
    native = []
    for w in range(W):
        moved = 0.0 if (w == 0 or placement == "b") else 1e-4
        tw = np.roll(t * (1.0 + moved * rng.standard_normal(t.shape)), w % K, axis=0)
        if mode == vo.MODE_NBZ3:
            tw[:, 2] = nbz[0]
        native.append(tw)
    th = np.array([zr.native_to_mode(tw, mode, nbz) for tw in native])
    data = {}
    if placement == "b":
        data["b"] = (exact, np.full(P, 1.0e-10))
    else:
        data["a1"] = (exact + rng.normal(0, SD, P), np.full(P, SD))
        if placement == "a":
            noise = np.full(P, zr.HUGE_NOISE)
            noise[:TILE] = SD                                   # the first tile in index order: before every "last" line
            data["a2"] = (exact + 1e-3 * SD * rng.standard_normal(P), noise)
    out = dict(x=x, th=th, native=np.array(native), K=K, mode=mode, nbz=nbz, bounds=bounds, kw=kw, data=data)
    for name, (flux, noise) in data.items():
        reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
        out["reg_" + name] = reg
        if name == "a1":
            out["want"] = vo.log_prob_batch_fast(reg, th)
        else:                                                   # chi^2 of the oracle's model flux, walker by walker
            out["chi_" + name] = np.array([np.sum(((flux - vo.model_flux(reg, q)) / noise) ** 2) for q in th])
    return tt._freeze(out)


# ---- host: every case is what its name says ----------------------------------------------------------------------------
@pytest.mark.parametrize("P,kind,K,m,pl", CASES)
def test_cases_are_what_they_say(P, kind, K, m, pl):
    c = case(P, kind, K, m, pl)
    M = tm.ff_matrix()
    name = {"a": "a1", "b": "b", "c": "a1"}[pl]
    flux, noise = c["data"][name]
    mom = tm.tile_moments(c["x"], flux, noise)
    near = tm.classify(c["native"], c["x"])[2]
    nonear = ~near.any(axis=1)                                  # [W, tiles]
    for w in MODEL_WALKERS:
        r = tm.walker_tiles(c["native"][w], c["x"], flux, noise, mom, M)
        assert np.array_equal(r["nonear"], nonear[w])
        if pl == "a":
            assert r["takes"].sum() >= 2 and r["takes"][0], (w, r["takes"], r["amax"])
        elif pl == "b":
            assert r["nonear"].sum() >= 2 and not r["takes"].any()
        else:
            assert not r["nonear"].any()
    if pl == "a":
        assert (nonear.sum(axis=1) >= 2).all()
        mom2 = tm.tile_moments(c["x"], *c["data"]["a2"])
        i0 = 0                                                  # the localised tile is the first in INDEX order
        r = tm.walker_tiles(c["native"][1], c["x"], *c["data"]["a2"], mom2, M)
        assert r["takes"][i0], "the localised tile does not take the path"
        big_m = (np.sqrt(mom2[2][i0]) + r["amax"][i0] * np.sqrt(mom2[1][i0, :, 0].sum())) ** 2
        assert big_m >= 30.0, f"M = {big_m:.2f}: the form's rounding would not show against 1e-12 of chi^2"
        tile_chi = c["chi_a2"]
        assert np.all(tile_chi < 1e-4 * TILE) and np.all(tile_chi > 0)       # fitted to ~1e-6 of a tile's chi^2 (256)
    if pl == "c":
        assert not nonear.any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _lnprob(c, name, chi=False):
    flux, noise = c["data"][name]
    with fz._ctx(256) as ctx:
        ctx.set_regions(c["x"], flux, noise, c["K"], mode=c["mode"], bounds=c["bounds"], nbz=None if c["nbz"] is None else c["nbz"][None, :])
        return ctx.lnprob(c["th"], return_chi2=chi)


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind,K,m,pl", [c for c in CASES if c[4] != "b"])
def test_lnprob_matches_oracle(P, kind, K, m, pl):
    c = case(P, kind, K, m, pl)
    got, want = _lnprob(c, "a1"), c["want"]
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"MOM-ERR P={P} {kind} K={K} {m} {pl}: worst {err.max():.3e} (walker {int(err.argmax())}); bar {fz.BAR:.1e}")
    assert err.max() <= fz.BAR


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind,K,m", [c[:4] for c in CASES if c[4] == "a"])
def test_rounding_signature_of_the_path(P, kind, K, m):
    c = case(P, kind, K, m, "a")
    _, chi = _lnprob(c, "a2", chi=True)
    want = c["chi_a2"]
    dev = np.abs(chi - want)
    print(f"MOM-SIG P={P} {kind} K={K} {m}: chi^2 {want.min():.3e} .. {want.max():.3e}; deviation {dev.min():.3e} .. {dev.max():.3e}, "
          f"largest in units of 1e-12 chi^2: {(dev / (1e-12 * want)).max():.3e}; guard bound {tm.GUARD_BOUND:.3e}")
    assert np.isfinite(chi).all()
    assert (dev > 1e-12 * want).any(), "no walker shows the moment form's rounding: the path did not run"
    assert (dev < tm.GUARD_BOUND).all()


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind,K,m", [c[:4] for c in CASES if c[4] == "b"])
def test_huge_weights_stay_per_pixel(P, kind, K, m):
    c = case(P, kind, K, m, "b")
    _, chi = _lnprob(c, "b", chi=True)
    print(f"MOM-ZERO P={P} {kind} K={K} {m}: chi^2 of exact data at weights 1e10: worst {chi.max():.3e}")
    assert np.isfinite(chi).all() and chi.max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("m", list(MODES))
@pytest.mark.parametrize("kind", KINDS)
def test_two_sampler_steps_match_oracle(kind, m):
    c = case(2304, kind, 16, m, "a")
    flux, noise = c["data"]["a1"]
    with fz._ctx(256) as ctx:
        ctx.set_regions(c["x"], flux, noise, c["K"], mode=c["mode"], bounds=c["bounds"], nbz=None if c["nbz"] is None else c["nbz"][None, :])
        ctx.sampler_init(c["th"], seed=2304, a=2.0, split_block=W)
        res = ctx.run(2)
    chain, lchain, nacc = vo.run_sampler(lambda q: vo.log_prob_batch_fast(c["reg_a1"], q), c["th"], c["want"], 2, seed=2304, block=W)
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)
