"""GPU tests (-m gpu) of libvamp_fisher.so: the Jacobian, gradient, information matrix, covariance and ln det of every
fixture case (tests/golden/fisher/fisher_cases.npz: 40-digit mpmath, rounded to fp64) at the bars of tests/fisher_ref.py,
bit-for-bit independence of a point from the rest of the call, the statuses, and the Python surface.

Bars (b = clip(2 E_id, 1e-12, 1e-10) per case, E_id the error of the scipy-identity restatement of J, a = J / sigma):
    |dJ_pd| <= b max_p |J_pd|
    |dg_d|  <= b P max_p |a_pd| max_p |r_p / sigma_p| + 4 P eps sum_p |a_pd r_p / sigma_p|
    |dI_ij| <= (2 b + 4 eps) P max_p |a_pi| max_p |a_pj|
    |dS_ij| <= D kappa (2 b P + 8 D eps) sqrt(S_ii S_jj),  |d logdet| <= D kappa (2 b P + 8 D eps)      (kappa <= 1e6)
    max |C S - 1| <= 8 D^2 eps kappa of the kernel's own scaled information and covariance
plus the fp64 rounding of the prior's own terms on the amplitude entries (fisher_ref.bar_prior: the bars above bound
the sums over the pixels only), and, for what the issue sets no bar, from the flux bar |df_p| <= b the posterior and predictive tests hold:
    |d chi2| <= 2 b sum_p |r_p| / sigma_p^2 + 4 P eps chi2;  free sd: |dg_sd| <= (that + 4 eps (chi2 + P)) / sd,  |dI_sd,sd| <= 4 eps I_sd,sd
The worst error over its bar is printed per case (profiles/fisher_limits.txt holds a run's figures)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fisher_ref as ref
from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu

CASES = ref.load_cases(os.path.join(GOLDEN, "fisher", "fisher_cases.npz"))
KAPPA_MAX = 1e6
FIELDS = ("grad", "info", "cov", "sigma", "logdet", "chi2", "status", "jac")


def _points(cases, **kw):
    from vamp_amd import fisher
    return fisher.fisher_points([c["x"] for c in cases], [c["flux"] for c in cases], [c["noise"] for c in cases],
                                [c["theta"] for c in cases], [c["K"] for c in cases], [c["mode"] for c in cases], **kw)


_cache = {}


def _batch():
    if "batch" not in _cache:
        _cache["batch"] = _points(CASES, jac=True)
    return _cache["batch"]


def _same(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k)), equal_nan=True) for k in FIELDS
               if getattr(a, k) is not None and getattr(b, k) is not None)


def _ratios(c, r, prior=True):
    """worst error over bar of J, g, I (and of cov, logdet, C S - 1 when the case's kappa allows): a dict"""
    b = ref.bar_b(c["e_id"])
    sig = np.full(c["P"], c["theta"][-1]) if c["sd"] else c["noise"]
    a = c["jac"] / sig[:, None]
    flux_model, _ = ref.jacobian(c["x"], c["theta"], c["K"], c["mode"], c["sd"])
    rs = (c["flux"] - flux_model) / sig
    with np.errstate(all="ignore"):
        out = {"jac": np.nanmax(np.where(ref.bar_jac(c["jac"], b) > 0, np.abs(r.jac - c["jac"]) / ref.bar_jac(c["jac"], b),
                                         np.where(r.jac == c["jac"], 0.0, np.inf)))}
        if c["kind"] == "jac":
            return out
        grad, info = (c["grad"], c["info"]) if prior else (c["grad_noprior"], c["info_noprior"])
        bg, bi = ref.bar_grad(a, rs, b), ref.bar_info(a, b)
        if prior:
            pg, pi = ref.bar_prior(c["theta"], c["K"], c["mode"], c["D"])
            bg, bi = bg + pg, bi + np.diag(pi)
        bc = 2 * b * float(np.sum(np.abs(rs) / sig)) + 4 * c["P"] * ref.EPS * c["chi2"]
        if c["sd"]:      # the free sd's entries are closed forms of chi^2, P and sd
            bg[-1] = (bc + 4 * ref.EPS * (c["chi2"] + c["P"])) / c["theta"][-1]
            bi[-1, -1] = 4 * ref.EPS * info[-1, -1]
        zero = lambda e, bar: np.where(bar > 0, e / bar, np.where(e == 0, 0.0, np.inf))
        out["grad"] = float(np.max(zero(np.abs(r.grad - grad), bg)))
        out["info"] = float(np.max(zero(np.abs(r.info - info), bi)))
        out["chi2"] = abs(r.chi2 - c["chi2"]) / bc
        if prior and c["kind"] == "full" and c["kappa"] <= KAPPA_MAX:
            D, P, kap = c["D"], c["P"], c["kappa"]
            out["cov"] = float(np.max(np.abs(r.cov - c["cov"]) / ref.bar_cov(c["cov"], kap, b, P)))
            out["logdet"] = abs(r.logdet - c["logdet"]) / ref.bar_logdet(D, kap, b, P)
            d = np.sqrt(np.diag(r.info))
            C, S = r.info / np.outer(d, d), r.cov * np.outer(d, d)
            out["CS-1"] = float(np.max(np.abs(C @ S - np.eye(D)))) / (8 * D * D * ref.EPS * kap)
    return out


def _check(c, r, prior=True):
    worst = _ratios(c, r, prior)
    print(f"{c['name']:30s} D={c['D']:2d} P={c['P']:3d} status={r.status} kappa={c['kappa']:.2e} b={ref.bar_b(c['e_id']):.1e} "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (c["name"], k, v)
    if c["kind"] == "full" and c["kappa"] <= KAPPA_MAX and prior:
        assert r.status == 0 and np.allclose(r.sigma, np.sqrt(np.diag(r.cov)), rtol=1e-15, atol=0)
        assert np.array_equal(r.info, r.info.T) and np.array_equal(r.cov, r.cov.T)
    if c["kind"] == "flat":
        assert r.status == 1 and np.all(np.isnan(r.cov)) and np.all(np.isnan(r.sigma)) and np.isnan(r.logdet)


def test_every_fixture_case_in_one_call():
    for c, r in zip(CASES, _batch()):
        _check(c, r)


def test_one_case_per_call_equals_the_batch_bit_for_bit():
    for c, r in zip(CASES, _batch()):
        assert _same(_points([c], jac=True)[0], r), c["name"]


def test_reversed_batch_order_changes_nothing():
    got = _points(CASES[::-1], jac=True)[::-1]
    assert all(_same(a, b) for a, b in zip(got, _batch()))


def test_several_points_per_group_host_and_device_and_a_callers_stream():
    """the 4 walkers of a golden region as ONE group of 4 points, ld > D; the same from device memory on a stream of the
    caller's: both equal the one-point groups of the batch bit for bit"""
    import torch
    from vamp_amd import fisher
    by_region = {}
    for i, c in enumerate(CASES):
        if c["kind"] == "full" and "_w" in c["name"]:
            by_region.setdefault(c["name"].rsplit("_w", 1)[0], []).append(i)
    names = [n for n in by_region if len(by_region[n]) == 4][:6]
    assert len(names) == 6
    first = [CASES[by_region[n][0]] for n in names]
    args = ([c["x"] for c in first], [c["flux"] for c in first], [c["noise"] for c in first], [c["K"] for c in first],
            [c["mode"] for c in first], [int(c["sd"]) for c in first])
    ld = [c["D"] + 3 for c in first]
    pts = [np.full((4, l), np.nan) for l in ld]
    for p, n in zip(pts, names):
        for j, i in enumerate(by_region[n]):
            p[j, :CASES[i]["D"]] = CASES[i]["theta"]
    dims, n_pix = [c["D"] for c in first], [c["P"] for c in first]
    host = fisher._call(0, *args, [p.ctypes.data for p in pts], False, ld, [4] * 6)
    dev_pts = [torch.from_numpy(p).to("cuda:0") for p in pts]
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    dev = fisher._call(0, *args, [t.data_ptr() for t in dev_pts], True, ld, [4] * 6, stream=stream.cuda_stream)
    for flat in (host, dev):
        recs = fisher._split(flat, dims, n_pix, [4] * 6, True)
        for n, rr in zip(names, recs):
            for i, r in zip(by_region[n], rr):
                assert _same(r, _batch()[i]), (n, i)


def test_context_fisher_reads_device_rows_of_all_regions():
    """two Voigt regions of a context, three rows [sum of D] of their points side by side in device memory: every record
    equals the one-point call of the batch"""
    import torch
    import vamp_amd
    from vamp_amd import fisher
    names = ["H1215_r0_K4_m1_sd0", "H1215_r2_K4_m1_sd0"]
    idx = [[i for i, c in enumerate(CASES) if c["name"].startswith(n + "_w")][:3] for n in names]
    first = [CASES[i[0]] for i in idx]
    rows = np.stack([np.concatenate([CASES[idx[0][j]]["theta"], CASES[idx[1][j]]["theta"]]) for j in range(3)])
    with vamp_amd.HipContext(device=0) as ctx:
        ctx.set_regions([c["x"] for c in first], [c["flux"] for c in first], [c["noise"] for c in first], [4, 4], mode=vamp_amd.MODE_VOIGT4)
        dev = torch.from_numpy(rows).to("cuda:0")
        torch.cuda.synchronize()
        recs = fisher.context_fisher(ctx, dev.data_ptr(), [c["x"] for c in first], [c["flux"] for c in first], [c["noise"] for c in first],
                                     n_points=3, jac=True)
        with pytest.raises(ValueError, match="noise is None exactly"):
            fisher.context_fisher(ctx, dev.data_ptr(), [c["x"] for c in first], [c["flux"] for c in first], [None, None])
    assert [len(r) for r in recs] == [3, 3]
    for g in range(2):
        for j in range(3):
            assert _same(recs[g][j], _batch()[idx[g][j]]), (g, j)


def test_each_output_alone():
    from vamp_amd import fisher
    cs = [c for c in CASES if c["kind"] == "full"][:5]
    args = ([c["x"] for c in cs], [c["flux"] for c in cs], [c["noise"] for c in cs], [c["K"] for c in cs], [c["mode"] for c in cs],
            [int(c["sd"]) for c in cs], [c["theta"].ctypes.data for c in cs], False, [c["D"] for c in cs], [1] * 5)
    full = fisher._call(0, *args)
    for k in FIELDS:
        alone = fisher._call(0, *args, want=(k,))
        assert set(alone) == {k} and np.array_equal(alone[k], full[k], equal_nan=True), k
    assert fisher._call(0, *args, want=()) == {}


def test_without_the_prior():
    cs = [c for c in CASES if c["kind"] == "full"]
    for c, r in zip(cs, _points(cs, jac=True, with_prior=False)):
        _check(c, r, prior=False)


def test_status_1_keeps_gradient_information_and_jacobian():
    flat = [i for i, c in enumerate(CASES) if c["kind"] == "flat"]
    assert [CASES[i]["name"] for i in flat] == ["flat_L0", "flat_twins"]
    for i in flat:
        r = _batch()[i]
        assert r.status == 1 and np.all(np.isfinite(r.grad)) and np.all(np.isfinite(r.info)) and np.all(np.isfinite(r.jac))
    assert np.all(_batch()[flat[0]].jac[:, 1] == 0.0) and np.any(_batch()[flat[0]].jac[:, 2] != 0.0)      # L = 0: tau = 0, dtau/dL is not


def test_status_2_leaves_its_neighbours_alone():
    from vamp_amd import fisher
    voigt = next(c for c in CASES if c["name"].startswith("H1215_r0_K2_m1_sd1"))      # Voigt, free sd
    good = voigt["theta"]
    bad = []
    for d, v in ((3, 0.0), (5, np.nan), (len(good) - 1, 0.0), (2, -1.0), (0, np.inf)):     # G = 0, NaN, sd = 0, L < 0, A = inf
        t = good.copy()
        t[d] = v
        bad.append(t)
    pts = np.array([good, bad[0], good, bad[1], bad[2], good, bad[3], bad[4], good])
    recs = fisher.fisher_points(voigt["x"], voigt["flux"], None, pts, voigt["K"], voigt["mode"], jac=True)
    alone = fisher.fisher_points(voigt["x"], voigt["flux"], None, good, voigt["K"], voigt["mode"], jac=True)
    assert [r.status for r in recs] == [0, 2, 0, 2, 2, 0, 2, 2, 0]
    for r in recs:
        if r.status == 2:
            assert all(np.all(np.isnan(np.asarray(getattr(r, k), dtype=np.float64))) for k in FIELDS if k != "status")
        else:
            assert _same(r, alone)
    gauss = next(c for c in CASES if c["name"].startswith("H1215_r0_K2_m0_sd0"))
    t = gauss["theta"].copy()
    t[2] = 0.0                                                                              # sigma = 0
    two = fisher.fisher_points(gauss["x"], gauss["flux"], gauss["noise"], np.array([t, gauss["theta"]]), 2, 0)
    assert [r.status for r in two] == [2, 0]


def test_refusals():
    from vamp_amd import fisher
    from vamp_amd._fisher_lib import FisherError
    c = CASES[0]
    args = ([c["x"]], [c["flux"]], [c["noise"]], [c["K"]], [c["mode"]], [0], [c["theta"].ctypes.data], False, [c["D"]], [1])

    def swap(i, v):
        a = list(args)
        a[i] = v
        return a
    for a, word in ((swap(4, [2]), "NBZ3"), (swap(3, [17]), "n_comp"), (swap(2, [None]), "noise"), (swap(9, [0]), "n_points"),
                    (swap(0, [np.append(c["x"][:-1], np.nan)]), "finite"), (swap(2, [np.zeros_like(c["x"])]), "positive")):
        with pytest.raises(FisherError, match=word):
            fisher._call(0, *a)
    with pytest.raises(FisherError, match="ld"):
        fisher._call(0, *swap(8, [c["D"] - 1])[:9], [2])
    with pytest.raises(FisherError, match="no HIP device"):
        fisher._call(99, *args)


def test_fit_fisher_at_the_map():
    """VPfit.fisher() after map_estimate on the one-Gaussian-line, 24-pixel data of tests/test_gpu_evidence.py: equal to
    fisher_points at _theta_dev, converted; the gradient against sqrt(diag I).  The simplex stops when its points agree
    to 1e-3 in ln p: a point within 1e-3 of the maximum along direction d has g_d^2 / (2 I_dd) <= 1e-3, so the bar is
    |g_d| / sqrt(I_dd) <= sqrt(2e-3) = 0.045.  Measured on an MI355X: 1.3e-4, 3.8e-5, 1.1e-4; scipy's fmin on the oracle's
    log_prob reaches 2.2e-3, 1.4e-3, 2.0e-3 on the same data with the same tolerances (tests/test_fisher.py measures it:
    the bar is not tighter than that)."""
    import evidence_ref
    from vamp_amd import fisher
    from vamp_amd.vpfits import VPfit
    x, flux, noise = evidence_ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
    fit = VPfit(noise=noise, seed=5)
    fit.initialise_model(1.0e3 + 2.0 * x, flux, 1, voigt=False)
    fit.map_estimate()
    rec = fit.fisher()
    assert fit.fisher() is rec and rec.names == ["xexp_0", "est_centroid_0", "est_sigma_0"] and rec.status == 0
    raw = fisher.fisher_points(fit._x, fit._flux, fit.noise, fit._theta_dev, 1, 0)
    s = fit._scale
    assert np.array_equal(rec.cov, raw.cov * np.outer(s, s)) and np.array_equal(rec.grad, raw.grad / s)
    assert np.array_equal(rec.info, raw.info / np.outer(s, s)) and np.array_equal(rec.sigma, raw.sigma * np.abs(s))
    ratio = np.abs(rec.grad) * rec.sigma
    print("MAP", fit._to_caller(fit._theta_dev), "sigma", rec.sigma, "|g| sigma", ratio, "|g| / sqrt(diag I)", np.abs(rec.grad) / np.sqrt(np.diag(rec.info)))
    assert np.all(np.abs(rec.grad) / np.sqrt(np.diag(rec.info)) <= np.sqrt(2e-3))
    assert abs(rec.sigma[0] / 1.2) < 0.2 and 0.0 < rec.sigma[1] < 2.0 and 0.0 < rec.sigma[2] < 2.0      # a 12-sigma line: percent-level errors
    fit._theta_dev = fit._theta_dev * 1.01           # the point moved: the cache does not answer for it
    assert fit.fisher() is not rec


def _read_h5(path):
    try:
        import h5py
        with h5py.File(path, "r") as f:
            return {k: f[k][()] for k in f}
    except ImportError:
        from vamp_amd import h5min
        return h5min.read(str(path))


def test_spectrum_fisher_writes_and_reads_back(tmp_path):
    from vamp_amd.vpfits import VPfit
    from vamp_amd.vpspectrum import VPspectrum
    g = load_golden("simba_spectra.npz")
    spec = VPspectrum(1215.6701, verbose=False)
    spec.set_arrays(g["H1215_wavelength"], g["H1215_flux"], g["H1215_noise"])
    spec.region_pixels = [[int(s), int(e)] for s, e in g["H1215_region_pixels"][[0, 2]]]
    spec.regions = []
    for j, (s, e) in enumerate(spec.region_pixels):
        region = spec._region(s, e)
        fit = VPfit(seed=50 + j)
        fit.initialise_model(region.frequency_array, region.flux_array, 1 + j, voigt=bool(j))
        fit.map_estimate()
        region.fit, region.n = fit, 1 + j
        spec.regions.append(region)
    out = spec.fisher()
    assert set(out) == {"std_a", "std_c", "std_s", "std_L", "line_region", "status", "logdet", "chi2", "grad_norm", "n_comp"}
    assert out["std_a"].shape == (3,) and out["line_region"].tolist() == [0, 1, 1] and out["n_comp"].tolist() == [1, 2]
    assert np.isnan(out["std_L"][0]) and out["status"].shape == (2,)
    r0 = spec.regions[0].fit.fisher()
    assert r0.names[-1] == "sd" and out["std_a"][0] == r0.sigma[0] and out["std_s"][0] == r0.sigma[2]
    nu = spec.regions[0].fit.estimated_variables[0]["centroid"].value
    from vamp_amd.physics import Freq2wave
    assert out["std_c"][0] == Freq2wave(nu) * r0.sigma[1] / nu
    spec.output_filename = str(tmp_path / "spectrum_0_voigt_")
    path = spec.write_fisher(out)
    assert path.endswith("spectrum_0_voigt_fisher.h5")
    back = _read_h5(path)
    assert set(back) == set(out)
    for k in out:
        np.testing.assert_array_equal(back[k], out[k])


def test_do_vamp_fisher_writes_the_file(tmp_path):
    out = tmp_path / "out"
    spec = tmp_path / "spectrum_4.h5"
    shutil.copy(os.path.join(GOLDEN, "simba_H1215.h5"), spec)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    rc = subprocess.run([sys.executable, "-m", "vamp_amd.do_vamp", str(spec), "1215.6701", "--output_folder", str(out),
                         "--conv_attempts", "1", "--walkers", "32", "--iterations", "60", "--burn", "20", "--thin", "2",
                         "--seed", "3", "--batched", "--fisher"], env=env, capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [ln for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    assert len(lines) == 1
    rec = json.loads(lines[0][len("vamp_perf "):])
    assert 0.0 <= rec["fisher_seconds"] < rec["seconds"] + 60
    fish = _read_h5(out / "spectrum_4_gauss_fisher.h5")
    assert fish["status"].shape == (rec["regions"],) and fish["std_a"].shape == (rec["lines"],) and int(fish["n_comp"].sum()) == rec["lines"]
    ok = fish["status"][fish["line_region"]] == 0
    assert np.all(fish["std_a"][ok] > 0) and np.all(fish["std_c"][ok] > 0) and np.all(fish["std_s"][ok] > 0)
    assert set(np.unique(fish["status"])) <= {0, 1}
