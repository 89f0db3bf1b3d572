"""CPU tests of the Fisher-matrix library's arithmetic and Python surface (no GPU): the host build of the derivative
evaluator (vamp_amd/csrc/voigt_grad.hpp) against the 40-digit fixture at the bar of the GPU tests, a planted error that
shows the bar can be missed, the restatement (tests/fisher_ref.py) against closed forms, the formulas against central
differences of the oracle, and vamp_amd.fisher's argument checks and unit conversion."""
import ctypes as C
import os

import numpy as np
import pytest

import fisher_ref as ref
from conftest import GOLDEN, ROOT
from oracle import vamp_oracle as vo

CASES = ref.load_cases(os.path.join(GOLDEN, "fisher", "fisher_cases.npz"))
BY_NAME = {c["name"]: c for c in CASES}
WALKERS = [c for c in CASES if c["kind"] == "full" and "_w" in c["name"]]       # the kappa-selected walkers of lnprob_cases.npz


@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "tests", "host", "libvoigt_grad_host.so")
    if not os.path.exists(path):
        pytest.fail(path + " is not built: run __graft_entry__.build()")
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    for fn in (lib.voigt_grad_n, lib.voigt_grad_planted_n):
        fn.restype, fn.argtypes = None, [C.c_int, dp, dp, dp]
    return lib


def _host_jacobian(lib, c, planted=False):
    """J of a Voigt case from the host build of the evaluator, combined as fisher.hip combines it"""
    fn = lib.voigt_grad_planted_n if planted else lib.voigt_grad_n
    dp = C.POINTER(C.c_double)
    x, th, K = c["x"], c["theta"], c["K"]
    tau, dt = np.zeros(c["P"]), np.zeros((c["P"], c["D"]))
    for k in range(K):
        A, cen, L, G = th[4 * k:4 * k + 4]
        s, y = 2.0 * ref.SQRT_LN2 / G, L * ref.SQRT_LN2 / G
        u = np.ascontiguousarray((x - cen) * s)
        yy = np.full_like(u, y)
        out = np.empty((u.size, 4))
        fn(u.size, u.ctypes.data_as(dp), yy.ctypes.data_as(dp), out.ctypes.data_as(dp))
        Ks, Ku, TL, TG = out.T
        tau += A * y * Ks
        dt[:, 4 * k:4 * k + 4] = np.stack([y * Ks, -A * y * ref.SQRT_PI * s * Ku, A * ref.SQRT_PI * (0.5 * s) * TL,
                                           -(A * y * ref.SQRT_PI / G) * TG], axis=1)
    return -np.exp(-tau)[:, None] * dt


def _jac_ratio(c, J):
    bar = ref.bar_jac(c["jac"], ref.bar_b(c["e_id"]))
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bar > 0, np.abs(J - c["jac"]) / bar, np.where(J == c["jac"], 0.0, np.inf))))


def test_the_fixture_holds_the_cases_of_the_issue():
    names = [c["name"] for c in CASES]
    assert len(WALKERS) == 96 and all(c["kappa"] <= 1e6 for c in WALKERS)
    assert [n for n in names if n.startswith("sweep_")] == ["sweep_LG%g" % r for r in (0, 1e-12, 1e-6, 1e-3, 0.1, 1, 10, 100, 1e3)]
    assert [BY_NAME["pix_P%d" % p]["P"] for p in (1, 63, 64, 65, 129)] == [1, 63, 64, 65, 129]
    assert (BY_NAME["K16_voigt_sd"]["D"], BY_NAME["K16_voigt_sd"]["P"], BY_NAME["K16_gauss"]["D"]) == (65, 65, 48)
    far = BY_NAME["far_line"]
    assert (far["theta"][5] - far["x"].max()) / far["theta"][7] >= 1e4
    assert os.path.getsize(os.path.join(GOLDEN, "fisher", "fisher_cases.npz")) < 800_000


def test_host_evaluator_meets_the_bar_on_every_voigt_case(host):
    worst = {}
    for c in CASES:
        if c["mode"] == 1 and not c["sd"]:
            worst[c["name"]] = _jac_ratio(c, _host_jacobian(host, c))
    print({k: round(v, 4) for k, v in worst.items() if k.startswith(("sweep", "far", "pix", "flat"))}, "walkers' worst", max(worst.values()))
    assert len(worst) >= 50 and max(worst.values()) <= 1.0, max(worst, key=worst.get)


def test_planted_identity_in_the_large_z_branch_misses_the_bar(host):
    """with the large-|z| branch replaced by the identity on the same w, the y = 100 case misses its bar (and passes
    with the evaluator as it is): the comparison can fail"""
    c = BY_NAME["sweep_LG100"]
    good, planted = _jac_ratio(c, _host_jacobian(host, c)), _jac_ratio(c, _host_jacobian(host, c, planted=True))
    print("sweep_LG100: error / bar", good, "planted", planted)
    assert good <= 1.0 < planted
    small = BY_NAME["sweep_LG0.1"]                       # every pixel in the core: the planted branch is never taken
    assert np.array_equal(_host_jacobian(host, small), _host_jacobian(host, small, planted=True))


def test_L_equal_zero_keeps_the_gaussian_core_in_dtau_dL(host):
    c = BY_NAME["sweep_LG0"]
    J = _host_jacobian(host, c)
    A, cen, _, G = c["theta"]
    u = (c["x"] - cen) * 2.0 * ref.SQRT_LN2 / G
    assert np.all(J[:, [0, 1, 3]] == 0.0)                # tau = 0 at L = 0: only dtau/dL is left, f = 1
    np.testing.assert_allclose(J[:, 2], -A * ref.SQRT_PI * (ref.SQRT_LN2 / G) * np.exp(-u * u), rtol=1e-14, atol=1e-300)


def test_restatement_against_closed_forms():
    x = np.arange(30.0)
    th = np.array([1e-6, 14.2, 2.5])                     # optically thin: f = 1, J_A = -e
    noise = np.full(30, 0.05)
    f, J = ref.jacobian(x, th, 1, 0)
    o = ref.from_jacobian(J, f, np.ones(30), noise, th, 1, 0)
    e = np.exp(-0.5 * ((x - 14.2) / 2.5) ** 2)
    assert o["info"][0, 0] == pytest.approx(np.sum(e * e) / 0.05 ** 2 + 1e12, rel=1e-5)
    assert ref.from_jacobian(J, f, np.ones(30), noise, th, 1, 0, with_prior=False)["info"][0, 0] == pytest.approx(np.sum(e * e) / 0.05 ** 2, rel=3e-6)
    for c in WALKERS[::7]:
        np.testing.assert_allclose(c["cov"] @ c["info"], np.eye(c["D"]), atol=8 * c["D"] ** 2 * ref.EPS * c["kappa"] * np.sqrt(
            np.outer(np.diag(c["cov"]), 1.0 / np.diag(c["cov"]))).max())
        if c["e_id"] > 1e-13:
            continue                                      # (the identity of the restatement's J has failed: large damping)
        f, J = ref.jacobian(c["x"], c["theta"], c["K"], c["mode"], c["sd"])
        o = ref.from_jacobian(J, f, c["flux"], c["noise"], c["theta"], c["K"], c["mode"])
        assert abs(o["logdet"] - c["logdet"]) <= ref.bar_logdet(c["D"], c["kappa"], ref.bar_b(c["e_id"]), c["P"])


def _region(c):
    return vo.Region(x=c["x"], flux=c["flux"], noise=np.ones_like(c["x"]) if c["sd"] else c["noise"], n_comp=c["K"], mode=c["mode"],
                     sample_sd=c["sd"])


def test_formulas_against_central_differences_of_the_oracle():
    """J against model_flux and grad against log_prob, step h = 1e-6 |theta_d|, at 1e-6 of the column maximum (J) and of the
    sum of the gradient's absolute terms (grad), plus the differences' own errors: their rounding eps |value| / h and
    their truncation, taken from the same difference at h / 2 (a centre given in Hz has |theta_d| = 2e15 and a step
    of two line widths: there the truncation is all there is)"""
    checked = 0
    for c in WALKERS[::3]:
        R, th = _region(c), c["theta"]
        sig = np.full(c["P"], th[-1]) if c["sd"] else c["noise"]
        a = c["jac"] / sig[:, None]
        rs = (c["flux"] - vo.model_flux(R, th)) / sig
        lnp = vo.log_prob(R, th)
        for d in range(c["D"]):
            h = 1e-6 * abs(th[d])
            if h == 0.0:
                continue
            up, dn = th.copy(), th.copy()
            up[d] += h
            dn[d] -= h
            if not (np.isfinite(vo.log_prob(R, up)) and np.isfinite(vo.log_prob(R, dn))):
                continue                                  # the step leaves the prior's support
            u2, d2 = th.copy(), th.copy()
            u2[d] += 0.5 * h
            d2[d] -= 0.5 * h
            dJ = (vo.model_flux(R, up) - vo.model_flux(R, dn)) / (up[d] - dn[d])
            dJ2 = (vo.model_flux(R, u2) - vo.model_flux(R, d2)) / (u2[d] - d2[d])
            colmax = np.abs(c["jac"][:, d]).max()
            assert np.abs(dJ - c["jac"][:, d]).max() <= 1e-6 * colmax + 4 * ref.EPS / h + 2 * np.abs(dJ - dJ2).max(), (c["name"], d)
            dg = (vo.log_prob(R, up) - vo.log_prob(R, dn)) / (up[d] - dn[d])
            dg2 = (vo.log_prob(R, u2) - vo.log_prob(R, d2)) / (u2[d] - d2[d])
            size = np.sum(np.abs(a[:, d] * rs)) + (1.0 / abs(th[d]) + 1.0 if d < c["D"] - c["sd"] and d % ref.q_of(c["mode"]) == 0 else 0.0)
            if c["sd"] and d == c["D"] - 1:
                size = (c["chi2"] + c["P"]) / th[d]
            assert abs(dg - c["grad"][d]) <= 1e-6 * size + 4 * ref.EPS * abs(lnp) / h + 2 * abs(dg - dg2), (c["name"], d, dg, c["grad"][d])
            checked += 1
    assert checked > 200


def test_fmin_on_the_oracle_ends_inside_the_bar_of_the_gpu_test():
    """what scipy's fmin (xtol = ftol = 1e-3, PyMC's MAP.fit) reaches on the one-Gaussian-line, 24-pixel data of
    tests/test_gpu_evidence.py: |g_d| / sqrt(I_dd) at its end, against the sqrt(2e-3) test_gpu_fisher.py asks of the
    device's simplex"""
    from scipy.optimize import fmin
    import evidence_ref
    x, flux, noise = evidence_ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
    R = vo.Region(x=x, flux=flux, noise=noise, n_comp=1, mode=vo.MODE_GAUSS3)
    best = fmin(lambda t: -vo.log_prob(R, t), np.array([0.9, 12.5, 3.2]), xtol=1e-3, ftol=1e-3, maxiter=2000, disp=False)
    f, J = ref.jacobian(x, best, 1, 0)
    o = ref.from_jacobian(J, f, flux, noise, best, 1, 0)
    ratio = np.abs(o["grad"]) / np.sqrt(np.diag(o["info"]))
    print("fmin ends at", best, "|g| / sqrt(diag I)", ratio)
    assert np.all(ratio <= np.sqrt(2e-3))


# ---- the Python surface, without a GPU ---------------------------------------------------------------------
def test_argument_checks_come_before_the_library():
    from vamp_amd import fisher
    x, y, n = np.arange(10.0), np.ones(10), np.full(10, 0.1)
    with pytest.raises(ValueError, match="does not hold"):
        fisher.fisher_points(x, y, n, np.ones(5), 1, 1)
    with pytest.raises(ValueError, match="does not hold"):
        fisher.fisher_points(x, y, None, np.ones(3), 1, 0)               # free sd: D = 4
    with pytest.raises(ValueError, match="mode 2"):
        fisher.fisher_points(x, y, n, np.ones(6), 2, 2)
    with pytest.raises(ValueError, match="n_comp"):
        fisher.fisher_points(x, y, n, np.ones(51), 17, 0)
    with pytest.raises(ValueError, match="one abscissa"):
        fisher.fisher_points([x], [y], [n, n], [np.ones(3)], 1, 0)
    with pytest.raises(ValueError, match="non-empty"):
        fisher.fisher_points(x, y, n, np.ones((0, 3)), 1, 0)
    with pytest.raises(ValueError, match="split"):
        fisher.fisher_points(x, y, n, np.broadcast_to(np.ones(48), (fisher.MAX_MATRIX_DOUBLES // 48 ** 2 + 1, 48)), 16, 0)
    assert fisher.fisher_points([], [], [], [], 1, 0) == [] and fisher.fits_fisher([]) == []


def test_unit_conversion_equals_the_restatement_in_caller_units():
    """a record in device units x = (nu - mid) / dnu, converted with the scales of VPfit._to_caller, against the
    restatement computed directly on the caller's abscissa at the caller's point"""
    from vamp_amd.fisher import FisherRecord
    c = BY_NAME["H1215_r0_K2_m1_sd1_w0"]
    dnu, mid = 3.7e9, 2.4e15
    scale = np.array([1.0, dnu, dnu, dnu] * 2 + [1.0])
    shift = np.array([0.0, mid, 0.0, 0.0] * 2 + [0.0])
    f, J = ref.jacobian(c["x"], c["theta"], 2, 1, True)
    o = ref.from_jacobian(J, f, c["flux"], None, c["theta"], 2, 1)
    dev = FisherRecord(o["grad"], o["info"], o["cov"], np.sqrt(np.diag(o["cov"])), o["logdet"], o["chi2"], 0, jac=J)
    rec = dev.to_units(scale, names=["n%d" % i for i in range(9)])
    th2 = c["theta"] * scale + shift
    f2, J2 = ref.jacobian(c["x"] * dnu + mid, th2, 2, 1, True)
    o2 = ref.from_jacobian(J2, f2, c["flux"], None, th2, 2, 1)
    rel = lambda a, b: np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    # x * dnu + mid rounds at 1e-16 * mid / dnu = 1e-10 of a pixel: the caller-unit restatement is the noisier side
    assert rel(rec.jac, J2) < 1e-6 and rel(rec.info, o2["info"]) < 1e-6 and rel(rec.grad, o2["grad"]) < 1e-5
    assert rel(rec.cov, o2["cov"]) < 1e-4 and rel(rec.sigma, np.sqrt(np.diag(o2["cov"]))) < 1e-4
    assert abs(rec.logdet - o2["logdet"]) < 1e-4 and rec.chi2 == pytest.approx(o2["chi2"], rel=1e-8)
    assert np.allclose(rec.corr, dev.corr, rtol=1e-12, atol=1e-12) and rec.names[0] == "n0" and rec.status == 0
    with pytest.raises(ValueError, match="scales"):
        dev.to_units(scale[:-1])


def test_build_exports_the_flags_and_the_eighth_library():
    from vamp_amd import build as vb
    assert vb.FISHER_FLAGS is vb.SIDE_FLAGS and vb.FISHER_OUT.endswith("libvamp_fisher.so")
    assert all(os.path.exists(d) for d in vb.FISHER_DEPS)
