"""GPU tests (-m gpu) of libvamp_metric.so: every case goes through metric_ref.check -- the library's eigenvalues against
the 40-digit fixture, its residual and orthogonality, and cov, prec, logdet, chol and the counts each against the
restatement evaluated on the library's OWN outputs of the stage before, at the bars derived or CPU-measured in
tests/metric_ref.py -- at the smallest shapes where a path changes (the pad, the second pass over indices >= 64, the
raised LDS limit, the matrices-per-workgroup count and one past it); then the statuses in the middle of a batch,
bit-for-bit independence of a matrix from the rest of the call, the regions whose Fisher information is singular, and
the Python surface.  The worst error over its bar is printed per case and stage (profiles/metric_limits.txt holds a
run's figures)."""
import os

import numpy as np
import pytest

import metric_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("eig", "vec", "cov", "prec", "chol", "logdet", "off", "n_low", "n_high", "sweeps_used", "status")
MATS = ("vec", "cov", "prec", "chol")


def _unflatten(flat, dims, n_mats):
    """the outputs of ``metric._call`` as one dict per matrix"""
    out, ov, om, op = [], 0, 0, 0
    for D, M in zip(dims, n_mats):
        for _ in range(M):
            r = {k: flat[k][om:om + D * D].reshape(D, D) for k in MATS if k in flat}
            if "eig" in flat:
                r["eig"] = flat["eig"][ov:ov + D]
            r.update({k: float(flat[k][op]) for k in ("logdet", "off") if k in flat})
            r.update({k: int(flat[k][op]) for k in ("n_low", "n_high", "sweeps_used", "status") if k in flat})
            out.append(r)
            ov, om, op = ov + D, om + D * D, op + 1
    return out


def _groups(groups, n_sweeps=None, **kw):
    """one library call; a group is a list of cases that share D, scales, kind and clamps.  One dict per matrix."""
    from vamp_amd import metric
    mats = [np.ascontiguousarray(np.stack([c["mat"] for c in g])) for g in groups]
    dims = [len(g[0]["scale"]) for g in groups]
    n_mats = [len(g) for g in groups]
    flat = metric._call(0, mats, dims, dims, n_mats, [g[0]["scale"] for g in groups], [g[0]["kind"] for g in groups],
                        [g[0]["lam_lo"] for g in groups], [g[0]["lam_hi"] for g in groups], n_sweeps or metric.DEFAULT_SWEEPS, **kw)
    return _unflatten(flat, dims, n_mats)


def _lib(cases, n_sweeps=None, **kw):
    """one library call, a group per case"""
    return _groups([[c] for c in cases], n_sweeps, **kw)


def _same(a, b, keys=KEYS):
    keys = [k for k in keys if k in a and k in b]
    differ = [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]
    if differ:
        print("differ:", differ)
    return not differ and bool(keys)


def _report(label, worst):
    print(f"{label:24s} " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


G = ref.golden_cases


# ---- every stage at its bar ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.case_names())
def test_every_stage_at_its_bar(name):
    from vamp_amd import metric
    c = G()[name]
    D = len(c["scale"])
    got = _lib([c])[0]
    w = ref.check(got, c, ref.golden_bars()[D], metric.DEFAULT_SWEEPS, name)
    _report(f"{name} sweeps={got['sweeps_used']} n_low={got['n_low']} n_high={got['n_high']}", w)
    assert got["status"] == 0 and got["sweeps_used"] <= metric.DEFAULT_SWEEPS
    # the counts of the exact eigenvalues: no reference eigenvalue lies within the bar of a clamp (tests/test_metric.py)
    assert (got["n_low"], got["n_high"]) == ref.clamp(c["eig_ref"], c)[1:]
    if name.startswith(("identity", "diagonal")):
        assert got["sweeps_used"] == 1 and got["off"] == 0.0
    if name.startswith("cov_zero"):
        assert got["n_high"] == min(2, D - 1) and got["n_low"] == 0
    if name.startswith("halfzero"):
        assert got["n_low"] == D // 2
    if name.startswith("negative"):
        assert got["n_low"] >= int(np.sum(c["eig_ref"] < 0)) >= 1 and got["eig"][0] < 0


def test_zero_variance_without_an_upper_clamp_is_status_1():
    """kind 1 with a zero-variance direction and lam_hi = +inf: cov keeps the direction, so it does not factor"""
    c = dict(G()["cov_zero_D5"], lam_hi=np.inf)
    got = _lib([c])[0]
    ref.check(got, c, ref.golden_bars()[5])
    assert got["status"] == 1 and np.all(np.isnan(got["chol"])) and np.all(np.isfinite(got["cov"])) and got["n_high"] == 0


# ---- the workgroup's edges ----------------------------------------------------------------------------------------------
def _scaled_copies(c, n):
    """n matrices that share c's scales: c's matrix times 2^m, exactly"""
    return [dict(c, mat=c["mat"] * 2.0 ** m, eig_ref=None) for m in range(n)]


@pytest.mark.parametrize("D", ref.DIMS)
def test_matrices_per_workgroup_and_one_past(D):
    """a group of as many matrices as share a workgroup at this D, and one more: each is the matrix alone, bit for bit"""
    from vamp_amd import metric
    per_wg, lds = metric.plan(D)
    assert 1 <= per_wg <= 4 and lds <= 159 * 1024 and (per_wg == 4 or metric.plan(D)[1] // per_wg * (per_wg + 1) > 159 * 1024)
    copies = _scaled_copies(G()[f"wide_D{D}"], per_wg + 1)
    alone = [_lib([c])[0] for c in copies]
    assert len({a["eig"].tobytes() for a in alone}) == len(alone)
    for n in (per_wg, per_wg + 1):
        got = _groups([copies[:n]])
        assert all(_same(g, a) for g, a in zip(got, alone)), n
    print(f"D={D}: {per_wg} matrices per workgroup, {lds} bytes of LDS")


def test_largest_shape_after_a_small_call_is_the_same_bits():
    """D = 65 takes more dynamic LDS than a launch gets by default: the limit is raised once, whatever was launched first"""
    big, small = G()["negative_D65"], G()["wide_D2"]
    first = _lib([big])[0]
    ref.check(first, big, ref.golden_bars()[65])
    _lib([small])
    assert _same(_lib([big])[0], first)


# ---- statuses and independence -----------------------------------------------------------------------------------------
def _ragged():
    g = G()
    return [g["wide_D5"], g["wide_D65"], g["wide_D1"], g["cov_zero_D17"], g["wide_D64"], g["halfzero_D5"], g["wide_D2"], g["negative_D17"],
            g["wide_D63"], g["identity_D17"], g["wide_D48"], g["wide_D3"], g["wide_D4"]]


def test_alone_batch_reversed_device_matrices_stream_and_null_outputs():
    import torch
    from vamp_amd import metric
    cases = _ragged()
    got = _lib(cases)
    for c, g in zip(cases, got):
        assert _same(_lib([c])[0], g), c["name"]
    assert all(_same(a, b) for a, b in zip(_lib(cases[::-1])[::-1], got))
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(_lib(cases, stream=stream.cuda_stream), got))
    # matrices in device memory, with a leading dimension beyond D
    dims, ones = [len(c["scale"]) for c in cases], [1] * len(cases)
    ld = [D + 3 for D in dims]
    dev = []
    for c, D in zip(cases, dims):
        t = torch.full((D, D + 3), float("nan"), dtype=torch.float64, device="cuda:0")
        t[:, :D] = torch.tensor(c["mat"], dtype=torch.float64)
        dev.append(t)
    torch.cuda.synchronize()
    args = ([c["scale"] for c in cases], [c["kind"] for c in cases], [c["lam_lo"] for c in cases], [c["lam_hi"] for c in cases],
            metric.DEFAULT_SWEEPS)
    flat = metric._call(0, [t.data_ptr() for t in dev], ld, dims, ones, *args, is_device=True)
    assert all(_same(a, b) for a, b in zip(_unflatten(flat, dims, ones), got))
    # host matrices with that leading dimension
    host = [np.ascontiguousarray(t.cpu().numpy()) for t in dev]
    assert all(_same(a, b) for a, b in zip(_unflatten(metric._call(0, host, ld, dims, ones, *args), dims, ones), got))
    # cov and chol into the caller's device memory
    n_mat = sum(D * D for D in dims)
    d_cov, d_chol = (torch.full((n_mat,), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    mats = [np.ascontiguousarray(c["mat"]) for c in cases]
    flat = metric._call(0, mats, dims, dims, ones, *args, device_out={"cov": d_cov.data_ptr(), "chol": d_chol.data_ptr()})
    torch.cuda.synchronize()
    assert "cov" not in flat and "chol" not in flat
    flat.update(cov=d_cov.cpu().numpy(), chol=d_chol.cpu().numpy())
    assert all(_same(a, b) for a, b in zip(_unflatten(flat, dims, ones), got))
    # every output alone
    for keep in KEYS:
        flat = metric._call(0, mats, dims, dims, ones, *args, skip=tuple(k for k in KEYS if k != keep))
        assert set(flat) == {keep}
        assert all(np.array_equal(a[keep], g[keep], equal_nan=True) for a, g in zip(_unflatten(flat, dims, ones), got)), keep


def test_statuses_in_the_middle_of_a_batch():
    """one sweep only: a dense D = 17 matrix is not done (3), a NaN entry (2), and the neighbours -- matrices that need no
    rotation -- are what they are alone"""
    g = G()
    nan_entry = dict(g["wide_D5"], mat=g["wide_D5"]["mat"].copy())
    nan_entry["mat"][3, 1] = np.nan
    upper_nan = dict(g["diagonal_D5"], mat=g["diagonal_D5"]["mat"].copy())
    upper_nan["mat"][1, 3] = np.nan                       # not read
    inf_entry = dict(g["negative_D17"], mat=g["negative_D17"]["mat"].copy())
    inf_entry["mat"][16, 16] = np.inf
    cases = [g["identity_D5"], g["wide_D17"], g["diagonal_D17"], nan_entry, upper_nan, inf_entry, g["diagonal_D65"], g["wide_D65"], g["identity_D65"]]
    got = _lib(cases, n_sweeps=1)
    assert [r["status"] for r in got] == [0, 3, 0, 2, 0, 2, 0, 3, 0]
    for c, r in zip(cases, got):
        ref.check(r, c, ref.golden_bars()[len(c["scale"])] if r["status"] != 3 else dict(eig=np.inf, resid=np.inf, orth=np.inf), 1, c["name"])
        assert _same(_lib([c], n_sweeps=1)[0], r), c["name"]
    assert _same(got[4], _lib([g["diagonal_D5"]], n_sweeps=1)[0])
    assert got[1]["sweeps_used"] == 1 and np.all(np.isfinite(got[1]["eig"])) and np.all(np.isfinite(got[1]["vec"]))
    # with the default count the same batch is done where its entries are finite, and the finished ones have not moved
    full = _lib(cases)
    assert [r["status"] for r in full] == [0, 0, 0, 2, 0, 2, 0, 0, 0]
    assert all(_same(full[i], got[i]) for i in (0, 2, 3, 4, 5, 6, 8))


# ---- the regions the metric is for: a singular Fisher information --------------------------------------------------------------
@pytest.mark.parametrize("n_lines", [2, 3])
def test_duplicate_lines_get_a_metric_where_the_fisher_factor_fails(n_lines):
    from vamp_amd import fisher, hmc, laplace, metric
    from vamp_amd.vpfits import VPfit
    x, flux, noise, theta = ref.duplicate_lines_case(n_lines)
    D = theta.size
    fish = fisher.fisher_points(x, flux, noise, theta, n_lines, 1)
    assert fish.status == 1 and np.all(np.isfinite(fish.info))
    # the default path of fits_hmc has no metric there
    fit = VPfit(noise=noise, seed=5)
    fit.initialise_model(1.0e3 + 2.0 * np.arange(x.size), flux, n_lines, voigt=True)
    assert np.array_equal(fit._x, x)
    fit._theta_dev = theta.copy()
    plain = hmc.fits_hmc([fit], n_chains=4, n_steps=20, n_burn=5, tune_rounds=1, tune_steps=5)[0]
    assert plain.status == 1 and plain.chain is None
    # the regularised metric
    scale = metric.prior_scales(x, n_lines, 1, False)
    rec = metric.regularise(np.asarray(fish.info), scale, want=("vec", "prec"))
    case = ref.make_case(fish.info, scale)
    bars = ref.measured_bars([case])[D]
    got = {k: getattr(rec, k) for k in KEYS}
    w = ref.check(got, case, bars, metric.DEFAULT_SWEEPS, f"{n_lines} lines")
    want = ref.run(case, metric.DEFAULT_SWEEPS)
    _report(f"{n_lines} lines n_low={rec.n_low} eig={np.array2string(rec.eig[:4], precision=3)}", w)
    assert rec.status == 0 and rec.n_low == want["n_low"] >= 3 and rec.n_high == want["n_high"]
    # its factor samples, its covariance proposes.  The repaired directions have the prior's width -- 16 pixels for a width
    # whose value is 2 -- and are flat to first order only, so the step is sized for them: L eps = 0.16 prior widths keeps
    # most trajectories inside the prior (the restatement accepts 9 in 10 there, and none at eps = 0.2)
    start = hmc.draw_starts(theta, 0.05 * rec.chol, 8, np.random.default_rng(1),
                            lambda t: hmc.inside_prior(t, n_lines, 1, False, *hmc.derived_bounds(x, 1)))
    run = hmc.hmc_points(x, flux, noise, start, rec.chol, n_lines, 1, 0.02, n_steps=100, n_burn=10, n_leap=8)
    acc = float(np.mean(run.accept_rate))
    print("acceptance", acc, "walls", int(run.n_wall.sum()))
    assert run.status == 0 and np.all(run.chain_status == 0) and np.all(np.isfinite(run.chain)) and 0.0 < acc < 1.0
    # the proposal likewise: at the default inflate = 1.5 all but 8 of 1024 draws of prior width fall outside the prior and
    # khat is +inf by the header's rule (fewer than M + 1 finite ratios); a quarter of the prior's width leaves enough
    lap = laplace.laplace_points(x, flux, noise, theta, rec.cov, n_lines, 1, n_samples=2048, inflate=0.25)
    print("khat", lap.khat, "lnZ", lap.lnZ, "n_out", lap.n_out, "ess", lap.ess)
    assert lap.status == 0 and np.isfinite(lap.khat) and 0 < lap.n_out < 2048
    # and fits_hmc / fits_laplace take it
    reg = hmc.fits_hmc([fit], n_chains=4, n_steps=20, n_burn=5, tune_rounds=1, tune_steps=5, metric="regularised")[0]
    assert reg.status == 0 and reg.chain is not None and reg.metric == "regularised" and reg.n_low == rec.n_low
    lreg = laplace.fits_laplace([fit], n_samples=2048, inflate=0.25, metric="regularised")[0]
    assert lreg.status == 0 and lreg.n_low == rec.n_low and np.isfinite(lreg.khat)


def test_a_positive_definite_information_is_left_alone():
    """a golden Fisher case with lam_lo far below its spectrum: n_low = 0, and cov is the inverse of the information, to
    four times the error the restatement itself shows (evaluated in long double)"""
    import fisher_ref
    from conftest import ROOT
    from vamp_amd import metric
    cases = {c["name"]: c for c in fisher_ref.load_cases(os.path.join(ROOT, "tests", "golden", "fisher", "fisher_cases.npz"))}
    for name in ("pix_P65", "K16_gauss"):
        fc = cases[name]
        info = np.asarray(fc["info"], dtype=np.float64)
        D = len(info)
        scale = 1.0 / np.sqrt(np.diag(info))                      # B is then the scaled information: unit diagonal
        case = ref.make_case(info, scale, 0, 2.0 ** -60, np.inf)
        want = ref.run(case, metric.DEFAULT_SWEEPS)
        LD = np.longdouble
        err = lambda cov: float(np.max(np.abs(cov.astype(LD) @ info.astype(LD) - np.eye(D, dtype=LD))))
        bar = max(ref.MEASURED_FACTOR * err(want["cov"]), ref.MIN_BAR_EPS * ref.EPS)
        rec = metric.regularise(info, scale, lam_lo=2.0 ** -60, lam_hi=np.inf, want=("vec", "prec"))
        ref.check({k: getattr(rec, k) for k in KEYS}, case, ref.measured_bars([case])[D], metric.DEFAULT_SWEEPS, name)
        print(f"{name}: D={D} kappa={fc['kappa']:.3g} |cov H - I| = {err(rec.cov):.3g}, bar {bar:.3g} (restatement {err(want['cov']):.3g})")
        assert rec.status == 0 and rec.n_low == 0 and rec.n_high == 0 and want["n_low"] == 0
        assert err(rec.cov) <= bar


# ---- the Python surface -------------------------------------------------------------------------------------------------
def test_fit_hmc_and_laplace_with_the_regularised_metric():
    import evidence_ref
    from vamp_amd.vpfits import VPfit
    x, flux, noise = evidence_ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    fit = VPfit(noise=noise, seed=5)
    fit.initialise_model(1.0e3 + 2.0 * x, flux, 2, voigt=False)
    fit.map_estimate()
    plain = fit.hmc(n_chains=4, n_steps=40, n_burn=10, seed=3)
    rec = fit.hmc(n_chains=4, n_steps=40, n_burn=10, seed=3, metric="regularised")
    assert plain.metric == "fisher" and plain.n_low is None and rec is not plain
    assert rec.metric == "regularised" and rec.status == 0 and isinstance(rec.n_low, int) and isinstance(rec.n_high, int)
    assert rec.chain.shape == plain.chain.shape and np.all(np.isfinite(rec.chain))
    a = fit.laplace(n_samples=512)
    b = fit.laplace(n_samples=512, metric="regularised")
    assert a.metric == "fisher" and b.metric == "regularised" and b is not a and b.status == 0 and isinstance(b.n_low, int)
    assert fit.laplace(n_samples=512, metric="regularised") is b


def test_do_vamp_hmc_metric_regularised_writes_n_low(tmp_path):
    import json
    import shutil
    import subprocess
    import sys
    from conftest import ROOT
    from vamp_amd import h5min
    out = tmp_path / "out"
    spec = tmp_path / "spectrum_4.h5"
    shutil.copy(os.path.join(ROOT, "tests", "golden", "simba_H1215.h5"), spec)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    rc = subprocess.run([sys.executable, "-m", "vamp_amd.do_vamp", str(spec), "1215.6701", "--output_folder", str(out),
                         "--conv_attempts", "1", "--walkers", "32", "--iterations", "60", "--burn", "20", "--thin", "2",
                         "--seed", "3", "--batched", "--hmc", "--metric", "regularised"], env=env, capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    perf = [json.loads(ln[len("vamp_perf "):]) for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    back = h5min.read(str(out / "spectrum_4_gauss_hmc.h5"))
    R = perf[0]["regions"]
    print({k: back[k] for k in ("status", "n_low", "n_high")})
    assert back["n_low"].shape == (R,) and back["n_high"].shape == (R,) and back["n_low"].dtype == np.int32
    assert np.all(back["n_low"][back["status"] == 0] >= 0) and int((back["status"] == 0).sum()) >= 1
