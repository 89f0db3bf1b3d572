"""GPU tests of libvamp_post.so against the numpy restatement (tests/posterior_ref.py).

Tolerances are derived, not measured: the device flux meets the oracle's to 1e-12 (test_bench_shape_against_oracle,
test_lnprob_matches_golden) and the kernel uses the same evaluator; order statistics, their interpolations, the mean
and the centred sd move by at most the largest per-value error, and the tree sum over at most 16 384 terms adds about
1e-14.  So every flux statistic gets atol 1e-12 (flux <= 1) and every equivalent-width statistic atol
1e-12 * P * |width|; the NaN pattern, n_used and n_bad must be equal."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import posterior_ref as ref
from conftest import GOLDEN, ROOT, load_golden
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)
FLUX_ATOL = 1e-12


def _same(got, want, P, width, what=""):
    """a PosteriorSummary against ref.summaries' dict; prints each figure before it asserts"""
    assert (got.n_used, got.n_bad) == (want["n_used"], want["n_bad"]), (what, got.n_used, got.n_bad, want["n_used"], want["n_bad"])
    ew_atol = 1e-12 * P * abs(width)
    worst = {}
    for name in ref.FLAT[:9]:
        a, b = np.asarray(getattr(got, name), dtype=float), np.asarray(want[name], dtype=float)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), (what, name, "NaN / inf pattern")
        fin = np.isfinite(b)
        worst[name] = float(np.max(np.abs(a[fin] - b[fin]))) if fin.any() else 0.0
    print("posterior", what, "P", P, "width", width, "max abs err", json.dumps(worst))
    for name, err in worst.items():
        assert err <= (FLUX_ATOL if name.startswith("flux") else ew_atol), (what, name, err)


def _x(P, descending=False):
    x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
    return x[::-1].copy() if descending else x


def _identical(a, b):
    for name in ref.FLAT:
        assert np.array_equal(np.asarray(getattr(a, name)), np.asarray(getattr(b, name)), equal_nan=name not in ("n_used", "n_bad")), name


def test_column_kernel_sizes_and_bad_samples():
    """S = 1, 2, 42, 64, 65, 255, 257, 300 (more than one element per thread of the sort's first steps, powers of two
    and their neighbours) and the cap 16 384; probabilities 0, 0.5 and 1; an all-bad ensemble; three bad samples"""
    from vamp_amd.posterior import posterior_summaries
    rng = np.random.default_rng(41)
    shapes = [(1, 1), (1, 2), (7, 6), (8, 8), (5, 13), (15, 17), (257, 1), (20, 15), (128, 128), (7, 6), (20, 15)]
    xs, chains, ks = [], [], []
    for i, (N, W) in enumerate(shapes):
        big = N * W == 16384
        K, P = (1, 3) if big else (1 + i % 2, 5)
        x = _x(P)
        th = ref.draw_prior(rng, x, K, vo.MODE_GAUSS3, N * W)
        th[:, 2::3] += 0.05                      # a width of exactly ~0 is legal but makes every flux 1
        xs.append(x); ks.append(K); chains.append(th.reshape(N, W, -1))
    chains[9][:, :, 2] = -1.0                    # every sample bad
    flat = chains[10].reshape(300, -1)
    flat[17, 0] = np.nan; flat[120, 2] = 0.0; flat[299, 1] = np.inf
    got = posterior_summaries(xs, chains, ks, vo.MODE_GAUSS3, probs=PROBS, pixel_width=0.5)
    for i, (x, c, K, g) in enumerate(zip(xs, chains, ks, got)):
        _same(g, ref.summaries(x, c, K, vo.MODE_GAUSS3, probs=PROBS, pixel_width=0.5), x.size, 0.5, "S=%d" % (c.shape[0] * c.shape[1]))
    assert got[9].n_used == 0 and got[9].n_bad == 42 and np.isnan(got[9].flux_q).all() and np.isnan(got[9].ew_mean)
    assert got[10].n_bad == 3 and got[8].n_used == 16384
    assert np.array_equal(got[0].flux_q[0], got[0].flux_q[-1]) and got[0].ew_sd == 0.0      # one sample: every quantile is it


def _golden_region():
    g = load_golden("lnprob_cases.npz")
    name = "H1215_r0_K4_m1_sd0"
    return g[name + "_x"], g[name + "_flux"], g[name + "_noise"], g[name + "_theta"], g[name + "_lnprob"]


def test_evaluation_both_modes_ragged_padded_descending():
    """one ragged call: both modes x K in {1, 4, 8, 17} x P in {2, 17, 44, 300} (the 16-lane form and the wavefront
    form, one and several rounds of pixels), sample_sd 0 and 1, rows padded (ld > W D, the padding NaN), every other
    abscissa descending; half of each ensemble drawn from the prior, half a 1 % ball; and the golden region with a
    ball around a golden theta"""
    from vamp_amd import posterior
    rng = np.random.default_rng(42)
    N, W = 3, 8
    groups = []
    for mode in (vo.MODE_GAUSS3, vo.MODE_VOIGT4):
        for K in (1, 4, 8, 17):
            for P in (2, 17, 44, 300):
                sd = (K + P) % 2
                x = _x(P, descending=len(groups) % 2 == 1)
                th = ref.draw_prior(rng, x, K, mode, N * W, bool(sd))
                th[N * W // 2:] = ref.ball(rng, th[0], N * W - N * W // 2)
                groups.append((x, th.reshape(N, W, -1), K, mode, sd, 0.1 + 0.01 * len(groups)))
    gx, _, _, gth, glnp = _golden_region()
    groups.append((gx, ref.ball(rng, gth[np.isfinite(glnp)][0], N * W).reshape(N, W, -1), 4, vo.MODE_VOIGT4, 0, 0.03))
    raws, lds = [], []
    for x, c, K, mode, sd, w in groups:
        D = c.shape[2]
        ld = W * D + 1 + len(raws) % 5
        raw = np.full((N, ld), np.nan)
        raw[:, :W * D] = c.reshape(N, W * D)
        raws.append(raw); lds.append(ld)
    probs = np.asarray(PROBS)
    flat = posterior._call(0, [g[0] for g in groups], [g[2] for g in groups], [g[3] for g in groups], [g[4] for g in groups],
                           [r.ctypes.data for r in raws], False, lds, [N] * len(groups), [W] * len(groups), [g[5] for g in groups], probs)
    got = posterior._split(flat, [g[0].size for g in groups], [g[2] for g in groups], probs, [1] * len(groups))
    for (x, c, K, mode, sd, w), g in zip(groups, got):
        _same(g, ref.summaries(x, c, K, mode, bool(sd), PROBS, w), x.size, w, "mode=%d K=%d P=%d sd=%d" % (mode, K, x.size, sd))
        assert g.n_bad == 0


def test_pass_packing_does_not_change_a_bit():
    """P = 300, S = 500 under a 64 KiB scratch: 16 columns per pass, so the region is split over 19 pixel ranges; with
    neighbours that share passes.  Neither the order statistics nor the equivalent-width sums (added in pixel order,
    continued from pass to pass) depend on the packing: every output equals the single-pass call's bit for bit."""
    from vamp_amd.posterior import posterior_summaries
    rng = np.random.default_rng(43)
    xs, chains, ks, modes = [], [], [], []
    for P, N, W, K, mode in ((5, 4, 5, 1, 0), (300, 20, 25, 3, 1), (7, 4, 5, 2, 1), (40, 10, 50, 2, 0)):
        x = _x(P)
        th = ref.draw_prior(rng, x, K, mode, N * W)
        th[1:] = ref.ball(rng, th[0], N * W - 1, rel=0.05)
        xs.append(x); chains.append(th.reshape(N, W, -1)); ks.append(K); modes.append(mode)
    chains[1].reshape(500, -1)[[3, 77]] = np.nan
    one = posterior_summaries(xs, chains, ks, modes, probs=PROBS, pixel_width=0.7)
    many = posterior_summaries(xs, chains, ks, modes, probs=PROBS, pixel_width=0.7, scratch_bytes=64 * 1024)
    for a, b in zip(one, many):
        _identical(a, b)
    assert one[1].n_bad == 2
    _same(many[1], ref.summaries(xs[1], chains[1], 3, 1, probs=PROBS, pixel_width=0.7), 300, 0.7, "split region")


def test_device_chain_read_in_place_equals_the_host_call():
    """the chain run_dev wrote for the golden region, read in place with ld = total_theta"""
    import torch
    import vamp_amd
    from vamp_amd.posterior import context_posterior, posterior_summaries
    x, f, n, th, _ = _golden_region()
    n_keep = 40
    with vamp_amd.HipContext(device=0) as ctx:
        ctx.set_regions(x, f, n, 4, mode=vamp_amd.MODE_VOIGT4)
        good = th[np.isfinite(ctx.lnprob(th))]
        W = good.shape[0] - good.shape[0] % 2
        ctx.sampler_init(good[:W], seed=78, a=2.0, split_block=W)
        dev = torch.device("cuda", 0)
        chain_t = torch.zeros((n_keep, ctx.total_theta), dtype=torch.float64, device=dev)
        lnp_t = torch.zeros((n_keep, ctx.total_walkers), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.run_dev(n_keep * 2, thin=2, chain_ptr=chain_t.data_ptr(), lnprob_ptr=lnp_t.data_ptr())
        recs = context_posterior(ctx, chain_t.data_ptr(), n_keep, x, probs=PROBS, pixel_width=0.2)
        host = chain_t.cpu().numpy().reshape(n_keep, W, 16)
    assert len(recs) == 1 and recs[0].n_used == n_keep * W
    _identical(recs[0], posterior_summaries(x, host, 4, 1, probs=PROBS, pixel_width=0.2))
    _same(recs[0], ref.summaries(x, host, 4, 1, probs=PROBS, pixel_width=0.2), x.size, 0.2, "device chain")


def _simba_region(i, line="H1215"):
    g = load_golden("simba_spectra.npz")
    s, e = g[line + "_region_pixels"][i]
    nu, fl, no = vo.region_from_spectrum(g[line + "_wavelength"], g[line + "_flux"], g[line + "_noise"], s, e)
    return nu, fl, no, np.flip(g[line + "_wavelength"][s:e], 0)


def _check_fit(fit, lam):
    band = fit.mcmc.flux_band(probs=PROBS)
    ew = fit.mcmc.equivalent_widths(lam, probs=PROBS)
    P = lam.size
    width = abs(lam[-1] - lam[0]) / (P - 1)
    want = ref.summaries(fit._x, fit._chain_dev, fit._n, int(fit._mode), bool(fit._sample_sd), PROBS, 1.0)
    np.testing.assert_allclose(band["mean"], want["flux_mean"], rtol=0, atol=FLUX_ATOL)
    np.testing.assert_allclose(band["sd"], want["flux_sd"], rtol=0, atol=FLUX_ATOL)
    for i, p in enumerate(PROBS):
        np.testing.assert_allclose(band["quantiles"][p], want["flux_q"][i], rtol=0, atol=FLUX_ATOL)
        assert abs(ew["EW"]["quantiles"][p] - want["ew_q"][i] * width) <= 1e-12 * P * width
        for k in range(fit._n):
            assert abs(ew["components"][k]["quantiles"][p] - want["comp_ew_q"][k, i] * width) <= 1e-12 * P * width
    assert abs(ew["EW"]["mean"] - want["ew_mean"] * width) <= 1e-12 * P * width
    assert abs(ew["EW"]["sd"] - want["ew_sd"] * width) <= 1e-12 * P * width
    assert ew["pixel_width"] == pytest.approx(width) and ew["n_used"] == want["n_used"] and ew["n_bad"] == 0
    assert np.all(band["quantiles"][0.0] <= band["quantiles"][1.0])


def test_vpfit_flux_band_and_equivalent_widths():
    from vamp_amd.vpfits import VPfit
    nu, fl, no, lam = _simba_region(0)
    fit = VPfit(seed=2025)
    fit.nwalkers = 32
    fit.initialise_model(nu, fl, 2, voigt=True)
    fit.mcmc_fit(iterations=120, burnin=40, thinning=4)
    before = dict(fit.mcmc.stats()["xexp_0"])
    _check_fit(fit, lam)
    assert fit.mcmc.stats()["xexp_0"] == before


def test_vpspectrum_posterior_summaries_two_regions():
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
    post = spec.posterior_summaries(probs=(0.16, 0.5, 0.84))
    npx = len(spec.flux_array)
    assert post["total_q"].shape == (3, npx) and post["EW_q"].shape == (2, 3) and post["line_EW_q"].shape == (3, 3)
    outside = np.ones(npx, bool)
    o = 0
    for j, (s, e) in enumerate(spec.region_pixels):
        outside[s:e] = False
        fit = spec.regions[j].fit
        lam = spec.wavelength_array[s:e]
        width = abs(lam[-1] - lam[0]) / (e - s - 1)
        want = ref.summaries(fit._x, fit._chain_dev, fit._n, 0, True, (0.16, 0.5, 0.84), width)
        np.testing.assert_allclose(post["total_mean"][s:e], want["flux_mean"][::-1], rtol=0, atol=FLUX_ATOL)
        np.testing.assert_allclose(post["total_sd"][s:e], want["flux_sd"][::-1], rtol=0, atol=FLUX_ATOL)
        np.testing.assert_allclose(post["total_q"][:, s:e], want["flux_q"][:, ::-1], rtol=0, atol=FLUX_ATOL)
        atol = 1e-12 * (e - s) * width
        assert abs(post["EW_mean"][j] - want["ew_mean"]) <= atol and abs(post["EW_sd"][j] - want["ew_sd"]) <= atol
        np.testing.assert_allclose(post["EW_q"][j], want["ew_q"], rtol=0, atol=atol)
        np.testing.assert_allclose(post["line_EW_q"][o:o + fit._n], want["comp_ew_q"], rtol=0, atol=atol)
        np.testing.assert_allclose(post["line_EW_mean"][o:o + fit._n], want["comp_ew_mean"], rtol=0, atol=atol)
        o += fit._n
    assert np.all(post["total_mean"][outside] == 1) and np.all(post["total_sd"][outside] == 0) and np.all(post["total_q"][:, outside] == 1)


def test_do_vamp_posterior_writes_the_file(tmp_path):
    from vamp_amd import h5min
    out = tmp_path / "out"
    spec = tmp_path / "spectrum_4.h5"
    shutil.copy(os.path.join(GOLDEN, "simba_H1215.h5"), spec)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    rc = subprocess.run([sys.executable, "-m", "vamp_amd.do_vamp", str(spec), "1215.6701", "--output_folder", str(out),
                         "--conv_attempts", "1", "--walkers", "32", "--iterations", "300", "--burn", "100", "--thin", "5",
                         "--seed", "3", "--posterior"], env=env, capture_output=True, text=True, timeout=900)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [ln for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    assert len(lines) == 1
    rec = json.loads(lines[0][len("vamp_perf "):])
    assert 0.0 <= rec["posterior_seconds"] < rec["seconds"] + 60
    path = out / "spectrum_4_gauss_posterior.h5"
    assert path.exists()
    try:
        import h5py
        with h5py.File(path, "r") as f:
            post = {k: f[k][()] for k in f}
    except ImportError:
        post = h5min.read(str(path))
    fm = h5min.read(str(out / "spectrum_4_gauss_flux_model.h5")) if not _has_h5py() else _read_h5py(out / "spectrum_4_gauss_flux_model.h5")
    nreg, npx = rec["regions"], fm["total"].size
    assert post["probs"].tolist() == [0.025, 0.16, 0.5, 0.84, 0.975]
    assert post["total_mean"].shape == (npx,) and post["total_q"].shape == (5, npx)
    assert post["EW_mean"].shape == (nreg,) and post["EW_q"].shape == (nreg, 5) and post["line_EW_q"].shape == (rec["lines"], 5)
    assert np.all(np.diff(post["total_q"], axis=0) >= 0) and np.all(post["total_sd"] >= 0)
    assert np.all(np.diff(post["EW_q"], axis=1) >= 0) and np.all(np.isfinite(post["line_EW_mean"]))
    inside = np.zeros(npx, bool)
    for s, e in fm["region_pixels"]:
        inside[int(s):int(e)] = True
    assert np.all(post["total_mean"][~inside] == 1) and np.all(post["total_sd"][~inside] == 0)
    assert np.all(post["total_mean"][inside] <= 1) and np.all(post["total_mean"][inside] >= 0)


def _has_h5py():
    try:
        import h5py  # noqa: F401
        return True
    except ImportError:
        return False


def _read_h5py(path):
    import h5py
    with h5py.File(path, "r") as f:
        return {k: f[k][()] for k in f}
