"""The node record behind the moment form of a far-field-only tile's chi^2 (k_tile_tables with VAMP_TILE_MOMENTS == 2,
ff_moment_chi_nodes, vamp_amd/csrc/ff_moments.hpp) on the GPU, packing 256:

  * the record itself, copied out by the test hook vampdbg_tile_moments, against the restatement
    (tests/tile_moments_nodes_ref.py) in extended precision, on ascending, descending and uneven grids, with and without
    a tail; the slot past the last full tile holds no record;
  * two regions of 1024 pixels behind a short one, so that neither starts on a multiple of 256 pixels: the record of
    tile `base` is slot (pix_off + base) >> 8;
  * a tile that the question before the node stage admits (vamp::ff_moments_try) and the rule after it turns away
    (vamp::ff_moments_ok): it must be swept pixel by pixel.  Two lines with damped wings 400 and 420 pixels before the
    tile (where the far-field interpolant itself is good to ~1e-14 of the optical depth: 16 Chebyshev nodes, the pole
    more than four half-widths from the tile's middle), data on the first tile only:
      shallow  amax = 0.45 at sigma = 0.01 against data 0.3 times as deep as the model;
      fitted   amax = 0.23 against data the model fits, noise 1e-3: chi^2 ~ 2.6, of which 1e-12 is a hundredth of the
               moment form's rounding at this M (0.1 x 8 2^-53 M ~ 2e-11, M > 2^18); the per-pixel form's is a few ulps
               of the model flux over sigma on each of 256 residuals of ~0.1 (measured on an MI355X: 3.3e-13 and
               4.9e-13 of chi^2, against 8.2e-15 and 9.2e-15 for the shallow data).
    The numpy model confirms both answers of the guard for each before the GPU is asked.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import test_gpu_ff_zone as fz
import test_gpu_tile_moments as gm
import test_gpu_tile_tables as tt
import tile_moments_nodes_ref as tn
import tile_moments_ref as tm
import zero_residual as zr

TILE, W, SD = 256, 64, 0.01
EPS = 2.0 ** -53
LD = np.longdouble


# ---- the record ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def record_case(P, kind):
    x = tt.make_grid(P, kind)
    rng = np.random.default_rng(P + len(kind))
    flux = 1.0 - 0.3 * np.exp(-0.5 * ((x - 40.0) / 90.0) ** 2) + rng.normal(0, 0.02, P)
    noise = 0.02 * rng.uniform(0.5, 2.0, P)
    rec = tn.node_record(x, flux, noise, dtype=LD)
    return tt._freeze(dict(x=x, flux=flux, noise=noise, rec=rec, scale=tn.record_scale(x, flux, noise)))


def _record(ctx, N):
    fn = ctx._lib.vampdbg_tile_moments
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_void_p]
    per = fn(ctx._h, None)
    assert per == tn.FFN_TILE, (per, ctx._lib.vamp_last_error())
    out = np.full((N // TILE + 1, per), np.nan)
    assert fn(ctx._h, out.ctypes.data) == per
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["up", "down", "steps"])
@pytest.mark.parametrize("P", [1024, 2304 + 100])
def test_record_matches_the_restatement(P, kind):
    import vamp_amd
    c = record_case(P, kind)
    x, nt = c["x"], P // TILE
    with fz._ctx(256) as ctx:
        ctx.set_regions(x, c["flux"], c["noise"], 1, mode=vamp_amd.MODE_VOIGT4, bounds=np.array([[x.min() - 1.0, x.max() + 1.0, 1.0e5, 1.0e5]]))
        rec = _record(ctx, P)
    Ql, Sl, Cl, Wl = c["rec"]
    qabs, sabs = c["scale"]
    Q, S = rec[:nt, :tn.FFN_S].reshape(nt, 16, 16), rec[:nt, tn.FFN_S:tn.FFN_C0]
    C0, RC, RQ = rec[:nt, tn.FFN_C0], rec[:nt, tn.FFN_RC], rec[:nt, tn.FFN_RQ]
    assert np.isfinite(rec).all()
    assert np.array_equal(Q, Q.transpose(0, 2, 1))
    # the restatement's own rounding (test_record_of_the_restatement): a term w^2 l_n l_m carries ~100 roundings of the
    # two basis values, the sum of 256 terms at most 256 more
    eq, es = np.abs(Q - Ql).astype(np.float64), np.abs(S - Sl).astype(np.float64)
    print(f"record P={P} {kind}: |Q' - exact| nearest its bound {np.max(eq / ((256 + 128) * 2 * EPS * qabs)):.3f}, "
          f"|S' - exact| {np.max(es / ((256 + 128) * 2 * EPS * sabs)):.3f}")
    assert np.all(eq <= (256 + 128) * 2 * EPS * qabs) and np.all(es <= (256 + 128) * 2 * EPS * sabs)
    assert np.all(np.abs(C0 - Cl) <= 300 * 2 * EPS * C0)
    assert np.all(np.abs(RC - np.sqrt(Cl)) <= 300 * 2 * EPS * RC) and np.all(np.abs(RQ - np.sqrt(Wl)) <= 300 * 2 * EPS * RQ)
    assert (rec[:nt, tn.FFN_RQ + 1:] == 0).all()                # the padding
    assert (rec[nt:] == 0).all(), "a slot without a full tile holds a record"


# ---- two regions off the 256-pixel raster ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_regions_off_the_raster():
    import vamp_amd
    cases = [gm.case(1024, "up", 4, "voigt4", "a"), gm.case(1024, "down", 4, "voigt4", "a")]
    x0 = np.arange(100, dtype=np.float64)
    xs = [x0] + [c["x"] for c in cases]
    fl = [np.ones(100)] + [c["data"]["a1"][0] for c in cases]
    no = [np.full(100, SD)] + [c["data"]["a1"][1] for c in cases]
    bounds = np.vstack([np.array([[-10.0, 110.0, 1.0e5, 1.0e5]])] + [c["bounds"] for c in cases])
    with fz._ctx(256) as ctx:
        ctx.set_regions(xs, fl, no, [4, 4, 4], mode=vamp_amd.MODE_VOIGT4, bounds=bounds)
        got = [ctx.lnprob(c["th"], region=r + 1) for r, c in enumerate(cases)]
    for r, c in enumerate(cases):
        err = np.abs(got[r] - c["want"]) / np.maximum(1.0, np.abs(c["want"]))
        print(f"region {r + 1} at pixel {100 + 1024 * r}: worst {err.max():.3e}; bar {fz.BAR:.1e}")
        assert np.isfinite(got[r]).all() and err.max() <= fz.BAR


# ---- admitted before the node stage, turned away after it ------------------------------------------------------------
VARIANTS = {"shallow": (0.45, 0.3, 1.0), "fitted": (0.23, 1.0, 0.1)}       # amax, depth of the data / the model's, noise / SD


@functools.lru_cache(maxsize=None)
def turned_away_case(kind, variant):
    amax, depth, nfac = VARIANTS[variant]
    P, K = 1024, 2
    x = tt.make_grid(P, kind)
    d = np.sign(x[1] - x[0])
    rng = np.random.default_rng(len(kind) + len(variant))
    t = np.array([(1.0, x[0] - d * c, 100.0, 20.0) for c in (400.0, 420.0)])         # (A, c, L, G)
    an, a0 = tn.node_absorption(t, x, 0)
    for _ in range(3):                                                               # amplitudes so that the largest node absorption is amax
        t[:, 0] *= np.log1p(-amax) / np.log1p(-a0)
        an, a0 = tn.node_absorption(t, x, 0)
    bounds = np.array([[x.min() - fz.PAD, x.max() + fz.PAD, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    exact = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=np.ones(P), **kw), zr.native_to_mode(t, vo.MODE_VOIGT4, None))
    noise = np.full(P, zr.HUGE_NOISE)
    noise[:TILE] = SD
    flux = 1.0 - depth * (1.0 - exact) + nfac * SD * rng.standard_normal(P)
    native = np.array([np.roll(t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape)), w % K, axis=0) for w in range(W)])
    th = np.array([zr.native_to_mode(tw, vo.MODE_VOIGT4, None) for tw in native])
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    chi = np.array([np.sum(((flux - vo.model_flux(reg, q)) / noise) ** 2) for q in th])
    prior = np.array([vo.log_prior(reg, q) for q in th])
    return tt._freeze(dict(x=x, flux=flux, noise=noise, native=native, th=th, bounds=bounds, chi=chi, amax=amax, prior=prior))


CASES = [(kind, v) for kind in ("up", "down") for v in VARIANTS]


@pytest.mark.parametrize("kind,variant", CASES)
def test_turned_away_case_is_what_it_says(kind, variant):
    c = turned_away_case(kind, variant)
    Q, S, C0, W2 = tn.node_record(c["x"], c["flux"], c["noise"])
    far, wide, near = tm.classify(c["native"], c["x"])
    assert far[:, :, 0].all() and not near[:, :, 0].any()
    assert np.isfinite(c["prior"]).all() and np.isfinite(c["chi"]).all(), "a walker outside the prior has no chi^2"
    for w in gm.MODEL_WALKERS:
        an, amax = tn.node_absorption(c["native"][w], c["x"], 0)
        assert abs(amax - c["amax"]) < 1e-3
        r = np.sqrt(C0[0]) + amax * np.sqrt(W2[0])
        print(f"{kind} {variant} walker {w}: sqrt C0 = {np.sqrt(C0[0]):.1f}, amax = {amax:.4f}, r = {r:.1f} (admitted up to 512)")
        assert tm.guard_try(C0[0], W2[0]), "the data alone turn the tile away: the node stage is never asked"
        assert not tm.guard_ok(C0[0], W2[0], amax), "the rule admits the tile"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", CASES)
def test_turned_away_tile_is_swept_pixel_by_pixel(kind, variant):
    import vamp_amd
    c = turned_away_case(kind, variant)
    with fz._ctx(256) as ctx:
        ctx.set_regions(c["x"], c["flux"], c["noise"], 2, mode=vamp_amd.MODE_VOIGT4, bounds=c["bounds"])
        _, chi = ctx.lnprob(c["th"], return_chi2=True)
    dev = np.abs(chi - c["chi"]) / c["chi"]
    print(f"TURNED-AWAY {kind} {variant}: chi^2 {c['chi'].min():.4e} .. {c['chi'].max():.4e}; largest deviation {dev.max():.3e} of itself")
    assert np.isfinite(chi).all() and dev.max() <= 1e-12
