"""GPU tests of libvamp_pred.so against the numpy restatement (tests/predictive_ref.py).

The bars are derived from the flux bar 1e-12 of tests/test_gpu_posterior.py, not fitted: a flux error df moves
l = -1/2 ((y - f) / sigma)^2 - ... by |y - f| / sigma^2 df, so with d_p = 1e-12 max_s |y_p - f_sp| / sigma_sp^2 (from the
restatement, over the good samples) lppd and ll_mean get d_p + 1e-12 max(1, |value|), p_waic_pix gets
2 sqrt(pwaic_p) d_p + 1e-12 max(1, pwaic_p), a group sum the sum of its pixels' bars, elpd_se 1e-9 relative; counts and
the NaN / inf patterns must be equal (predictive_ref.check).  Test chains are 1 % balls around the point the data were
made from, which keeps d_p small: tests/test_predictive.py shows that a dropped sample, a missing ln sigma, the wrong
variance denominator and a plain mean each miss these bars by more than six orders of magnitude.  Prior draws are kept
for the bad-sample cases.  Every case prints its worst error / bar (profiles/predictive_limits.txt)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import evidence_ref
import posterior_ref as pref
import predictive_ref as ref
from conftest import GOLDEN, ROOT, load_golden
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu


def _x(P, descending=False):
    x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
    return x[::-1].copy() if descending else x


def _group(rng, P, K, mode, N, W, sd, descending=False):
    """data made from a point of the prior with widths of a pixel or more, and a 1 % ball around it as the chain"""
    x = _x(P, descending)
    q = 4 if mode == vo.MODE_VOIGT4 else 3
    th0 = pref.draw_prior(rng, x, K, mode, 1)[0]
    th0[2::q] += 0.5
    if q == 4:
        th0[3::4] += 1.0
    noise = 0.04 + 0.02 * rng.random(P)
    flux = np.exp(-pref.sample_taus(x, th0[None], K, mode)[0].sum(axis=0)) + noise * rng.standard_normal(P)
    centre = np.append(th0, 0.05) if sd else th0
    return {"x": x, "flux": flux, "noise": None if sd else noise, "chain": pref.ball(rng, centre, N * W).reshape(N, W, -1),
            "K": K, "mode": mode, "sd": bool(sd)}


def _run(groups, **kw):
    from vamp_amd.predictive import pointwise_predictive
    return pointwise_predictive([g["x"] for g in groups], [g["flux"] for g in groups], [g["noise"] for g in groups],
                                [g["chain"] for g in groups], [g["K"] for g in groups], [g["mode"] for g in groups], **kw)


def _want(g):
    return ref.pointwise(g["x"], g["flux"], g["noise"], g["chain"], g["K"], g["mode"], g["sd"])


def _as_dict(rec):
    return {k: getattr(rec, k) for k in ref.FLAT}


def _check(rec, g, label):
    """a PredictiveRecord against the restatement at the derived bars; prints the worst error / bar"""
    worst = ref.check(_as_dict(rec), _want(g), label)
    print("predictive %-58s S %5d P %3d K %2d worst error / bar %.3g" % (label, g["chain"].shape[0] * g["chain"].shape[1], g["x"].size, g["K"], worst))
    np.testing.assert_array_equal(rec.elpd, rec.lppd - rec.p_waic_pix)
    assert rec.waic == -2.0 * rec.elpd_waic or (np.isnan(rec.waic) and np.isnan(rec.elpd_waic))


def _identical(a, b):
    for name in ref.FLAT:
        assert np.array_equal(np.asarray(getattr(a, name)), np.asarray(getattr(b, name)), equal_nan=name not in ref.CNT), name


# ---- path switches --------------------------------------------------------------------------------------------
def test_owner_widths_modes_noise_forms_ragged_descending():
    """one call: P = 32 | 33 x K = 4 | 5 (the 16-lane and the 64-lane owner side by side) in both modes, free sd and known
    noise alternating, every other abscissa descending, and ragged neighbours of 2, 17 and 300 pixels and 1, 8 and 17 lines"""
    rng = np.random.default_rng(61)
    groups = []
    for mode in (vo.MODE_GAUSS3, vo.MODE_VOIGT4):
        for P in (32, 33):
            for K in (4, 5):
                groups.append(_group(rng, P, K, mode, 3, 8, sd=(len(groups) + mode) % 2, descending=len(groups) % 2 == 1))
        for P, K in ((2, 1), (17, 8), (300, 17)):
            groups.append(_group(rng, P, K, mode, 3, 8, sd=(P + mode) % 2, descending=P == 17))
    assert {g["sd"] for g in groups} == {False, True}
    for g, rec in zip(groups, _run(groups)):
        _check(rec, g, "mode=%d P=%d K=%d free_sd=%d" % (g["mode"], g["x"].size, g["K"], g["sd"]))
        assert rec.n_bad == 0 and rec.n_used == 24


def test_samples_around_a_workgroup_and_the_longest_column():
    """S = 1, 2, 63, 64, 65 and 129 (the 64 samples of an evaluation workgroup, and one per thread of the column stage),
    and S = 16 384 on two pixels: every thread of the column stage holds its 16 entries"""
    rng = np.random.default_rng(62)
    shapes = [(1, 1), (1, 2), (9, 7), (8, 8), (5, 13), (43, 3), (128, 128)]
    groups = [_group(rng, 2 if N * W == 16384 else 5, 1 + i % 2, vo.MODE_GAUSS3, N, W, sd=i % 2) for i, (N, W) in enumerate(shapes)]
    got = _run(groups)
    for g, rec, (N, W) in zip(groups, got, shapes):
        _check(rec, g, "S=%d" % (N * W))
        assert rec.n_used == N * W
    assert np.isnan(got[0].p_waic_pix).all() and np.isnan(got[0].elpd_waic) and np.isfinite(got[0].lppd).all()      # one sample
    assert np.array_equal(got[0].lppd, got[0].ll_mean) and np.isfinite(got[1].p_waic_pix).all()


def test_largest_and_smallest_evaluation_launch_repeat_bit_for_bit():
    """K = 32 at P = 65: the largest launch of the evaluation (51 200 bytes of dynamic LDS; no kernel of this library asks
    for more than 64 KiB, the column stage holds its entries in registers), two rounds of pixels; a K = 1 launch beside it
    and between two runs of the large one, which must agree bit for bit"""
    rng = np.random.default_rng(63)
    big, small = _group(rng, 65, 32, vo.MODE_VOIGT4, 2, 4, sd=1), _group(rng, 5, 1, vo.MODE_GAUSS3, 2, 4, sd=0)
    first = _run([big])[0]
    tiny = _run([small])[0]
    again = _run([big])[0]
    _identical(first, again)
    both = _run([small, big])
    _identical(both[1], first)
    _identical(both[0], tiny)
    _check(first, big, "K=32 P=65 (largest launch)")
    _check(tiny, small, "K=1 P=5 (smallest launch)")


def test_voigt_from_gaussian_to_lorentzian():
    """one line whose L / G runs from 0 and 1e-12 to 1e3 over the samples"""
    rng = np.random.default_rng(64)
    ratios = np.array([0.0, 1e-12, 1e-9, 1e-6, 1e-3, 0.03, 0.3, 1.0, 3.0, 30.0, 300.0, 1e3])
    x = _x(44)
    theta = np.stack([np.array([1.5, 0.7, r * 2.0, 2.0, 0.05]) for r in ratios])
    noise = np.full(44, 0.05)
    flux = np.exp(-pref.sample_taus(x, theta[7:8], 1, vo.MODE_VOIGT4)[0].sum(axis=0)) + noise * rng.standard_normal(44)
    for sd in (False, True):
        g = {"x": x, "flux": flux, "noise": None if sd else noise, "chain": theta[:, :5 if sd else 4].reshape(4, 3, -1).copy(), "K": 1,
             "mode": vo.MODE_VOIGT4, "sd": sd}
        _check(_run([g])[0], g, "L/G 0 .. 1e3 free_sd=%d" % sd)


# ---- bad and extreme samples ----------------------------------------------------------------------------------
def test_bad_and_extreme_samples():
    rng = np.random.default_rng(65)
    # a NaN parameter, sigma <= 0, sd = 0, sd < 0 and a NaN sd among prior draws: counted, left out
    a = _group(rng, 9, 2, vo.MODE_GAUSS3, 5, 6, sd=1)
    th = a["chain"].reshape(30, -1)
    th[:15] = pref.draw_prior(rng, a["x"], 2, vo.MODE_GAUSS3, 15, True)
    th[:15, 2::3] += 0.05
    th[3, 1] = np.nan
    th[8, 5] = 0.0
    th[11, -1] = 0.0
    th[20, -1] = -0.05
    th[29, -1] = np.nan
    # a good sample whose flux is NaN: amplitudes +-1e300 at L / G = 1e10 (tau = inf - inf)
    b = _group(rng, 9, 2, vo.MODE_VOIGT4, 3, 7, sd=0)
    b["chain"].reshape(21, -1)[7] = [1e300, 0.3, 1e10, 1.0, -1e300, -0.2, 1e10, 1.0]
    # a good sample whose residual over sd overflows when squared: l = -inf
    c = _group(rng, 9, 1, vo.MODE_GAUSS3, 3, 7, sd=1)
    c["chain"].reshape(21, -1)[5, -1] = 1e-200
    # bad samples only
    d = _group(rng, 9, 1, vo.MODE_VOIGT4, 3, 7, sd=0)
    d["chain"][:, :, 3] = 0.0
    got = _run([a, b, c, d])
    for g, rec, label in zip((a, b, c, d), got, ("bad samples counted", "a NaN flux", "l = -inf", "bad samples only")):
        _check(rec, g, label)
    assert (got[0].n_bad, got[0].n_used) == (5, 25) and np.isfinite(got[0].elpd_waic)
    assert got[1].n_bad == 0 and np.isnan(got[1].lppd).all() and np.isnan(got[1].ll_mean).all() and np.isnan(got[1].p_waic_pix).all()
    assert got[2].n_bad == 0 and np.isfinite(got[2].lppd).all() and np.isneginf(got[2].ll_mean).all() and np.isnan(got[2].p_waic_pix).all()
    assert (got[3].n_bad, got[3].n_used, got[3].n_high) == (21, 0, 0) and np.isnan(got[3].lppd).all() and np.isnan(got[3].elpd_se)


# ---- bit for bit ----------------------------------------------------------------------------------------------
def _three(seed=66):
    rng = np.random.default_rng(seed)
    groups = [_group(rng, 5, 1, 0, 4, 5, sd=1), _group(rng, 70, 3, 1, 20, 25, sd=0), _group(rng, 40, 2, 0, 10, 13, sd=1, descending=True)]
    groups[1]["chain"].reshape(500, -1)[[3, 77]] = np.nan
    return groups


def test_packing_and_group_order_do_not_change_a_bit():
    """a scratch of exactly one column of the largest group (S = 500: each of its pixels is a pass of its own) against
    the default, and every order of the three groups under a scratch of three such columns"""
    import itertools
    groups = _three()
    one = _run(groups)
    for a, b in zip(one, _run(groups, scratch_bytes=8 * 500)):
        _identical(a, b)
    for order in itertools.permutations(range(3)):
        for i, rec in zip(order, _run([groups[i] for i in order], scratch_bytes=8 * 1500)):
            _identical(rec, one[i])
    assert one[1].n_bad == 2
    for g, rec in zip(groups, one):
        _check(rec, g, "three groups, P=%d" % g["x"].size)


def test_scratch_of_exactly_one_column_of_the_largest_group():
    """S = 20, 17, 20 on P = 3, 1, 2 under scratch_bytes = 8 * 20: six passes of one column each, the S = 17 group in a
    pass that has 3 doubles to spare, a group boundary on every pass boundary (the plan: tests/test_chain_groups.py);
    every output equals the default-scratch call's bit for bit, and one byte less is an error"""
    rng = np.random.default_rng(67)
    groups = [_group(rng, 3, 1, vo.MODE_GAUSS3, 5, 4, sd=0), _group(rng, 1, 2, vo.MODE_VOIGT4, 17, 1, sd=1),
              _group(rng, 2, 2, vo.MODE_GAUSS3, 10, 2, sd=0, descending=True)]
    assert [g["chain"].shape[0] * g["chain"].shape[1] for g in groups] == [20, 17, 20]
    one = _run(groups)
    for a, b in zip(one, _run(groups, scratch_bytes=8 * 20)):
        _identical(a, b)
    for g, rec in zip(groups, one):
        _check(rec, g, "one column per pass, P=%d" % g["x"].size)
        assert rec.n_bad == 0
    from vamp_amd._pred_lib import PredError
    with pytest.raises(PredError, match="less than one column"):
        _run(groups, scratch_bytes=8 * 20 - 1)


def test_every_output_alone():
    """each output with every other pointer NULL equals the full call's; the group sums are formed also when the
    per-pixel outputs are not asked for"""
    from vamp_amd import predictive
    groups = _three(67)
    args = ([g["x"] for g in groups], [g["flux"] for g in groups], [g["noise"] for g in groups], [g["K"] for g in groups],
            [g["mode"] for g in groups], [int(g["sd"]) for g in groups], [g["chain"].ctypes.data for g in groups], False,
            [g["chain"].shape[1] * g["chain"].shape[2] for g in groups], [g["chain"].shape[0] for g in groups], [g["chain"].shape[1] for g in groups])
    full = predictive._call(0, *args)
    assert sorted(full) == sorted(ref.FLAT)
    for only in ref.FLAT:
        got = predictive._call(0, *args, want=(only,))
        assert list(got) == [only] and got[only].dtype == full[only].dtype
        assert np.array_equal(got[only], full[only], equal_nan=only not in ref.CNT), only
    assert predictive._call(0, *args, want=()) == {}


def test_device_chain_of_three_regions_and_a_callers_stream():
    """the chain HipContext.run_dev wrote for three regions with free sd, read in place (ld = total_theta), against the
    same chain from the host; then the same device chain on a stream that is not the default one"""
    import torch
    import vamp_amd
    from vamp_amd import _sidelib, predictive
    rng = np.random.default_rng(68)
    groups = [_group(rng, P, K, vo.MODE_GAUSS3, 1, 16, sd=1) for P, K in ((20, 1), (33, 2), (45, 3))]
    for g in groups:                                   # the start lies inside the prior: sigma < (P - 1) / 2
        g["chain"][:, :, 2:-1:3] = np.minimum(g["chain"][:, :, 2:-1:3], 0.4 * (g["x"].size - 1))
    n_keep, W = 12, 16
    xs, fs = [g["x"] for g in groups], [g["flux"] for g in groups]
    with vamp_amd.HipContext(device=0) as ctx:
        ctx.set_regions(xs, fs, [np.ones_like(f) for f in fs], [g["K"] for g in groups], mode=vamp_amd.MODE_GAUSS3, sample_sd=True)
        ctx.sampler_init([g["chain"][0] for g in groups], seed=79, a=2.0, split_block=W)
        dev = torch.device("cuda", 0)
        chain_t = torch.zeros((n_keep, ctx.total_theta), dtype=torch.float64, device=dev)
        lnp_t = torch.zeros((n_keep, ctx.total_walkers), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.run_dev(n_keep * 2, thin=2, chain_ptr=chain_t.data_ptr(), lnprob_ptr=lnp_t.data_ptr())
        recs = predictive.context_predictive(ctx, chain_t.data_ptr(), n_keep, xs, fs, [None] * 3)
        bases, total = _sidelib.region_bases(ctx, chain_t.data_ptr()), ctx.total_theta
        host = chain_t.cpu().numpy()
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        assert stream.cuda_stream != 0
        on_stream = predictive._call(0, xs, fs, [None] * 3, [g["K"] for g in groups], [0] * 3, [1] * 3, bases, True, [total] * 3, [n_keep] * 3,
                                     [W] * 3, stream=stream.cuda_stream)
    assert len(recs) == 3
    off = 0
    for g, rec in zip(groups, recs):
        D = g["chain"].shape[2]
        g["chain"] = host[:, off:off + W * D].reshape(n_keep, W, D).copy()
        off += W * D
        assert rec.n_used + rec.n_bad == n_keep * W
    assert not any(np.array_equal(g["chain"][0], g["chain"][-1]) for g in groups)          # the walkers moved
    for g, rec, h in zip(groups, recs, _run(groups)):
        _identical(rec, h)
        _check(rec, g, "device chain, P=%d" % g["x"].size)
    for rec, s in zip(recs, predictive._split(on_stream, [x.size for x in xs], [1] * 3)):
        _identical(rec, s)


# ---- the surface ----------------------------------------------------------------------------------------------
def _simba_region(i, line="H1215"):
    g = load_golden("simba_spectra.npz")
    s, e = g[line + "_region_pixels"][i]
    return vo.region_from_spectrum(g[line + "_wavelength"], g[line + "_flux"], g[line + "_noise"], s, e)


def _fit_group(fit):
    return {"x": fit._x, "flux": fit._flux, "noise": None if fit._sample_sd else fit.noise, "chain": fit._chain_dev, "K": fit._n,
            "mode": int(fit._mode), "sd": bool(fit._sample_sd)}


def test_vpfit_waic():
    from vamp_amd.vpfits import VPfit
    nu, fl, no = _simba_region(0)
    fit = VPfit(seed=2025)
    fit.nwalkers = 32
    fit.initialise_model(nu, fl, 2, voigt=True)
    fit.mcmc_fit(iterations=120, burnin=40, thinning=4)
    rec = fit.mcmc.waic()
    assert fit.mcmc.waic() is rec and fit._sample_sd and rec.step == 1
    _check(rec, _fit_group(fit), "VPfit on a simba region")
    assert rec.n_bad == 0 and np.isfinite(rec.elpd_waic) and rec.p_waic > 0 and rec.lppd.shape == fl.shape


def test_vpspectrum_predictive_two_regions():
    from vamp_amd.vpfits import VPfit
    from vamp_amd.vpspectrum import VPspectrum
    g = load_golden("simba_spectra.npz")
    spec = VPspectrum(1215.6701, verbose=False)
    spec.set_arrays(g["H1215_wavelength"], g["H1215_flux"], g["H1215_noise"])
    spec.region_pixels = [[int(s), int(e)] for s, e in g["H1215_region_pixels"][[0, 2]]]      # (regions 0 and 1 overlap)
    spec.regions = []
    for j, (s, e) in enumerate(spec.region_pixels):
        region = spec._region(s, e)
        fit = VPfit(seed=50 + j)
        fit.nwalkers = 16
        fit.initialise_model(region.frequency_array, region.flux_array, 1 + j, voigt=False)
        fit.mcmc_fit(iterations=60, burnin=20, thinning=2)
        region.fit, region.n = fit, 1 + j
        spec.regions.append(region)
    pred = spec.predictive()
    npx = len(spec.flux_array)
    outside = np.ones(npx, bool)
    for j, (s, e) in enumerate(spec.region_pixels):
        outside[s:e] = False
        fit = spec.regions[j].fit
        got = {k: pred[k][s:e][::-1] for k in ref.PIX}
        got.update({k: pred[k][j] for k in ref.GRP + ref.CNT})
        worst = ref.check(got, _want(_fit_group(fit)), "spectrum region %d" % j)
        print("predictive %-58s worst error / bar %.3g" % ("VPspectrum.predictive region %d" % j, worst))
        assert pred["waic"][j] == -2.0 * pred["elpd_waic"][j] and pred["n_comp"][j] == 1 + j and pred["time_step"][j] == 1
        assert spec.regions[j].fit.mcmc.waic().elpd_waic == pred["elpd_waic"][j]
    for k in ref.PIX + ("elpd",):
        assert pred[k].shape == (npx,) and np.isnan(pred[k][outside]).all() and np.isfinite(pred[k][~outside]).all()


def test_do_vamp_predictive_writes_the_file(tmp_path):
    from vamp_amd import h5min
    out = tmp_path / "out"
    spec = tmp_path / "spectrum_4.h5"
    shutil.copy(os.path.join(GOLDEN, "simba_H1215.h5"), spec)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    rc = subprocess.run([sys.executable, "-m", "vamp_amd.do_vamp", str(spec), "1215.6701", "--output_folder", str(out),
                         "--conv_attempts", "1", "--walkers", "32", "--iterations", "300", "--burn", "100", "--thin", "5",
                         "--seed", "3", "--predictive"], env=env, capture_output=True, text=True, timeout=900)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [ln for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    assert len(lines) == 1
    rec = json.loads(lines[0][len("vamp_perf "):])
    assert 0.0 <= rec["predictive_seconds"] < rec["seconds"] + 60 and "posterior_seconds" not in rec
    path = out / "spectrum_4_gauss_predictive.h5"
    assert path.exists()
    pred = h5min.read(str(path))
    nreg = rec["regions"]
    assert pred["elpd_waic"].shape == (nreg,) and pred["n_comp"].sum() == rec["lines"] and np.all(pred["n_used"] > 0)
    np.testing.assert_array_equal(pred["waic"], -2.0 * pred["elpd_waic"])
    inside = np.isfinite(pred["lppd"])
    assert 0 < inside.sum() <= rec["pixels_in_regions"]                                            # (regions may overlap)
    assert np.array_equal(inside, np.isfinite(pred["elpd"])) and np.all(pred["p_waic_pix"][inside] >= 0)
    assert np.all(np.isfinite(pred["elpd_waic"])) and np.all(pred["elpd_se"] > 0)


# ---- the ladder -----------------------------------------------------------------------------------------------
def _ladder(lines):
    from vamp_amd import predictive
    from vamp_amd.vpregion import VPregion
    x, flux, noise = evidence_ref.gauss_line_data(32, lines, 0.1, 4)
    reg = VPregion(1.0e3 + x, flux, noise, seed=12, nwalkers=32)
    assert reg.n == 1
    reg.region_fit(verbose=False, iterations=300, thin=5, burn=100, criterion='waic')
    for n in sorted(reg.predictive)[:-1]:
        rise, se = predictive.compare(reg.predictive[n], reg.predictive[n + 1])
        print("predictive ladder of %d-line data: n = %d -> %d elpd_waic rises by %.3f, paired standard error %.3f" % (len(lines), n, n + 1, rise, se))
    assert reg.fit._n == reg.n and reg.fit.predictive is reg.predictive[reg.n] and sorted(reg.predictive) == list(range(1, reg.n + 2))
    assert len(reg.fit.bic_array) == 3
    return reg


def test_region_fit_by_waic_finds_two_lines():
    assert _ladder([(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)]).n == 2


def test_region_fit_by_waic_keeps_one_line():
    assert _ladder([(1.2, 9.0, 2.0)]).n == 1
