"""GPU tests (-m gpu) of libvamp_laplace.so: every case goes through laplace_ref.check -- the library's draws, theta, ln q,
ln p, khat, weights, ln Z and moments each against the restatement evaluated on the library's OWN outputs of the stage
before, at the bars derived in tests/laplace_ref.py -- at the smallest shapes where a path changes; then bit-for-bit
independence of a group from the rest of the call, the statuses, khat against libvamp_loo.so, the quadrature bound and
the Python surface.  The worst error over its bar is printed per case and stage (profiles/laplace_limits.txt holds a
run's figures)."""
import math

import numpy as np
import pytest

import evidence_ref
import laplace_ref as ref
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu

GROUP = ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "lnp_centre", "n_out", "status")
SAMPLES = ("theta", "z", "lnp", "lnq", "lw")


def _args(cases):
    return dict(xs=[c["x"] for c in cases], fluxes=[c["flux"] for c in cases], noises=[c["noise"] for c in cases],
                n_comp=[c["n_comp"] for c in cases], modes=[c["mode"] for c in cases], sample_sd=[int(c["sample_sd"]) for c in cases],
                bounds=[None if c["bounds"] is None else np.array(c["bounds"]) for c in cases], region_ids=[c["region_id"] for c in cases],
                centres=[c["centre"] for c in cases], chols=[c["chol"] for c in cases], n_samples=cases[0]["S"], seed=cases[0]["seed"])


def _unflatten(flat, cases):
    """the flat arrays of ``laplace._call`` as one dict per group (what ``check`` takes)"""
    out, ov, om = [], 0, 0
    for g, c in enumerate(cases):
        D = c["centre"].size
        r = {k: flat[k][g] for k in GROUP if k in flat}
        r.update({k: flat[k][ov:ov + D] for k in ("mean", "sd") if k in flat})
        if "cov" in flat:
            r["cov"] = flat["cov"][om:om + D * D].reshape(D, D)
        r.update({k: flat[k][g] for k in SAMPLES if k in flat})
        out.append(r)
        ov, om = ov + D, om + D * D
    return out


def _lib(cases, **kw):
    """one library call for cases of one S and seed, every output asked for"""
    from vamp_amd import laplace
    assert len({(c["S"], c["seed"]) for c in cases}) == 1
    return _unflatten(laplace._call(0, **_args(cases), **kw), cases)


def _same(a, b):
    """whether two results agree bit for bit in every output both hold; the outputs that differ are printed"""
    differ = [k for k in a if k in b and not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]
    if differ:
        print("differ:", differ)
    return not differ and bool(set(a) & set(b))


def _report(label, worst):
    print(f"{label:42s} " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


def gauss_case(S, sd=False, seed=ref.QUAD_SEED, region_id=0):
    """the one-line quadrature case; with ``sd``: the same data with the free sd as a fourth parameter"""
    c = ref.quadrature_case()
    if not sd:
        return dict(c, S=S, seed=seed, region_id=region_id)
    chol = np.zeros((4, 4))
    chol[:3, :3] = c["chol"]
    chol[3] = [0.002, -0.001, 0.003, 0.02]
    return ref.make_case(c["x"], c["flux"], None, 1, 0, np.append(c["centre"], 0.1), chol, S, seed, region_id)


def lines_case(P, K, mode, sd, S, seed=5, region_id=1, full=True):
    """K well separated lines on P pixels with a full lower factor around the truth"""
    rng = np.random.default_rng(1000 * P + 10 * K + mode)
    x = np.arange(float(P))
    q = 4 if mode == 1 else 3
    cen = (np.arange(K) + 0.5) * P / K
    width = max(0.8, 0.12 * P / K)
    lines = [[0.6 + 0.05 * k, cen[k], width] if mode == 0 else [0.6 + 0.05 * k, cen[k], 0.4 * width, 1.8 * width] for k in range(K)]
    theta = np.array(lines).ravel()
    R = vo.Region(x=x, flux=np.ones(P), noise=np.ones(P), n_comp=K, mode=mode)
    flux = vo.model_flux(R, theta) + 0.05 * rng.standard_normal(P)
    centre = np.append(theta, 0.05) if sd else theta
    D = centre.size
    scale = np.tile([0.03, 0.05, 0.04, 0.04][:q], K)
    scale = np.append(scale, 0.004) if sd else scale
    low = np.tril(rng.uniform(-0.3, 0.3, (D, D)), -1) if full else np.zeros((D, D))
    chol = (low + np.eye(D)) * scale[:, None]
    chol[np.triu_indices(D, 1)] = np.nan                  # the upper triangle is not read
    return ref.make_case(x, flux, None if sd else np.full(P, 0.05), K, mode, centre, chol, S, seed, region_id)


# ---- every stage at its bar ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [20, 21, 64, 65, 1024, 1025, 16384])
def test_sample_counts(S):
    """M = 4 | 5 (no smoothing | smoothing), one workgroup of rows and one more (the centre's row moves to the next),
    one round of the weights' threads and one more, the longest column; D = 3, the 16-lane group"""
    c = gauss_case(S)
    got = _lib([c])[0]
    worst = ref.check(got, c, f"S={S}")
    _report(f"S={S} khat={got['khat']:.3f} lnZ={got['lnZ']:.4f} se={got['lnZ_se']:.4f} ess={got['ess']:.0f}", worst)
    assert got["status"] == 0 and (np.isinf(got["khat"]) if S == 20 else np.isfinite(got["khat"]))


@pytest.mark.parametrize("name", ["D4", "D65"])
def test_dimensions(name):
    """D = 4: the free sd, two whole pairs; D = 65: 16 Voigt lines and the sd, 33 pairs of which the last is half used, C
    full, the wide group with every record and table slot in use"""
    c = gauss_case(130, sd=True) if name == "D4" else lines_case(200, 16, 1, True, 130)
    assert c["centre"].size == int(name[1:])
    got = _lib([c])[0]
    _report(f"{name} n_out={got['n_out']} khat={got['khat']:.3f}", ref.check(got, c, name))
    assert got["status"] == 0 and got["n_out"] < c["S"] // 2


@pytest.mark.parametrize("P", [32, 33])
@pytest.mark.parametrize("K", [4, 5])
def test_around_the_narrow_group(P, K):
    """P = 32 | 33 x K = 4 | 5 Voigt lines with free sd: only (32, 4) takes the 16-lane group; S = 65 leaves the last group of a
    wavefront without a row"""
    c = lines_case(P, K, 1, True, 65)
    got = _lib([c])[0]
    _report(f"P={P} K={K} n_out={got['n_out']}", ref.check(got, c, f"P={P} K={K}"))
    assert got["status"] == 0


def test_one_pixel():
    c = ref.make_case([3.0], [0.4], [0.1], 1, 0, [0.9, 3.2, 1.5], np.linalg.cholesky(np.diag([0.5, 1.5, 0.8]) ** 2 + 0.01), 65, 9, 2,
                      bounds=(0.0, 6.0, 3.0, 7.0))
    got = _lib([c])[0]
    _report(f"P=1 n_out={got['n_out']}", ref.check(got, c, "P=1"))
    assert got["status"] == 0 and 0 < got["n_out"] < 65


def test_rejected_draws_are_counted_exactly():
    """a Voigt line with L on its lower bound: about half the draws are outside, and n_out is the restatement's"""
    c = ref.voigt_edge_case()
    got = _lib([c])[0]
    _report(f"L=0 n_out={got['n_out']}/{c['S']}", ref.check(got, c, "L on its bound"))
    want = ref.run(c)
    assert got["n_out"] == want["n_out"] and np.array_equal(np.isneginf(got["lnp"]), np.isneginf(want["lnp"]))
    assert 0.35 * c["S"] < got["n_out"] < 0.65 * c["S"]


def _all_rejected_case():
    """five Voigt lines, every centre on the upper bound of c, every L on 0 and every G on its upper bound, a diagonal
    factor: a draw is inside only if 15 signs agree"""
    K, P = 5, 40
    x = np.arange(float(P))
    fw = (P - 1) / 2.0 * 2 * math.sqrt(2 * math.log(2.0))
    centre = np.tile([0.5, P - 1.0, 0.0, fw], K)
    return ref.make_case(x, np.ones(P), np.full(P, 0.1), K, 1, centre, np.diag(np.full(4 * K, 1e-3)), 21, 3, 7,
                         bounds=(0.0, P - 1.0, (P - 1) / 2.0, fw))


def test_every_draw_rejected():
    c = _all_rejected_case()
    got = _lib([c])[0]
    ref.check(got, c, "every draw rejected")
    assert got["status"] == 0 and got["n_out"] == c["S"] and np.isneginf(got["lnZ"]) and np.isfinite(got["lnp_centre"])
    assert np.isnan(got["khat"]) and np.all(np.isnan(got["mean"])) and np.all(np.isnan(got["cov"])) and np.all(np.isfinite(got["theta"]))


# ---- statuses and independence -----------------------------------------------------------------------------------
def _batch():
    S, seed = 65, 11
    ok = [gauss_case(S, seed=seed, region_id=3), lines_case(33, 5, 1, True, S, seed, 4), gauss_case(S, sd=True, seed=seed, region_id=5)]
    no_factor = lines_case(40, 2, 0, False, S, seed, 6)
    no_factor["chol"][3, 3] = 0.0
    nan_entry = lines_case(40, 2, 0, False, S, seed, 7)
    nan_entry["chol"][4, 1] = np.nan
    outside = lines_case(40, 2, 1, False, S, seed, 8)
    outside["centre"][2] = -0.01                          # L_fwhm < 0
    return [ok[0], no_factor, ok[1], outside, nan_entry, ok[2]]


def test_status_1_and_2_in_the_middle_of_a_batch():
    cases = _batch()
    got = _lib(cases)
    assert [g["status"] for g in got] == [0, 1, 0, 2, 1, 0]
    for c, g in zip(cases, got):
        ref.check(g, c, f"region {c['region_id']}")
    two = got[3]
    assert np.all(np.isfinite(two["theta"])) and np.all(np.isfinite(two["lnq"])) and np.isneginf(two["lnp_centre"]) and np.all(np.isnan(two["lw"]))


def test_a_group_alone_reversed_and_on_a_stream_equals_the_batch_bit_for_bit():
    import torch
    cases = _batch()
    got = _lib(cases)
    for c, g in zip(cases, got):
        assert _same(_lib([c])[0], g), c["region_id"]
    assert all(_same(a, b) for a, b in zip(_lib(cases[::-1])[::-1], got))
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(_lib(cases, stream=stream.cuda_stream), got))


def test_device_outputs_and_null_outputs_change_nothing():
    import torch
    from vamp_amd import laplace
    cases = _batch()
    got = _lib(cases)
    S = cases[0]["S"]
    # theta of every group and z of every other group into the caller's device memory
    th = [torch.full((S, c["centre"].size), 7.0, dtype=torch.float64, device="cuda:0") for c in cases]
    zz = [torch.full((S, c["centre"].size), 7.0, dtype=torch.float64, device="cuda:0") if i % 2 == 0 else None for i, c in enumerate(cases)]
    torch.cuda.synchronize()
    flat = laplace._call(0, **_args(cases), device_ptrs={"theta": [t.data_ptr() for t in th], "z": [None if t is None else t.data_ptr() for t in zz]})
    torch.cuda.synchronize()
    dev = _unflatten(flat, cases)
    for g, d, t, zt in zip(got, dev, th, zz):
        assert "theta" not in d and _same(d, g)
        assert np.array_equal(t.cpu().numpy(), g["theta"], equal_nan=True)
        assert zt is None or np.array_equal(zt.cpu().numpy(), g["z"], equal_nan=True)
    # every output alone, and none of the per-sample ones
    names = GROUP + ("mean", "sd", "cov")
    for keep in names:
        flat = laplace._call(0, **_args(cases), want=(), skip=tuple(k for k in names if k != keep))
        assert set(flat) == {keep}
        alone = _unflatten(flat, cases)
        assert all(np.array_equal(a[keep], g[keep], equal_nan=True) for a, g in zip(alone, got)), keep
    only = _unflatten(laplace._call(0, **_args(cases), want=("lw",)), cases)
    assert all("theta" not in a and _same(a, g) for a, g in zip(only, got))


def test_khat_equals_the_loo_library_on_the_same_ratios():
    """an all-finite case: khat against vamp_amd.loo.loo_from_loglik of the [S, 1] matrix -r, within 2e-10 (the two
    libraries' bars of 1e-10 against the restatement, added)"""
    from vamp_amd import loo
    for S in (21, 1025, 4096):
        c = gauss_case(S, seed=31)
        got = _lib([c])[0]
        assert got["n_out"] == 0
        r = got["lnp"] - got["lnq"]
        rec = loo.loo_from_loglik(np.ascontiguousarray(-r[:, None]))
        print("S", S, "khat", got["khat"], "loo", rec.khat[0], "difference", got["khat"] - rec.khat[0])
        assert abs(got["khat"] - rec.khat[0]) <= 2e-10 * max(1.0, abs(rec.khat[0]))


# ---- accuracy ------------------------------------------------------------------------------------------------------
def test_lnZ_against_quadrature():
    """the issue's bound on the device: |lnZ - 8.227| <= 4 lnZ_se + 0.02 with lnZ_se <= 0.05 at S = 4096, inflate 1.5, the
    seed of tests/test_laplace.py, through the public call (the Fisher covariance is fisher_ref's at scipy's MAP)"""
    from vamp_amd import laplace
    c = ref.quadrature_case()
    cov = c["chol"] @ c["chol"].T / 1.5 ** 2
    rec = laplace.laplace_points(c["x"], c["flux"], c["noise"], c["centre"], cov, 1, 0, n_samples=4096, inflate=1.5, seed=ref.QUAD_SEED,
                                 want=SAMPLES)
    want = ref.quadrature_run()
    print("device lnZ", rec.lnZ, "se", rec.lnZ_se, "psis", rec.lnZ_psis, "laplace", rec.lnZ_laplace, "khat", rec.khat, "ess", rec.ess,
          "| restatement", want["lnZ"], want["lnZ_se"], want["khat"], "| quadrature", ref.QUAD_LNZ)
    assert rec.status == 0 and rec.ok and rec.lnZ_se <= 0.05
    assert abs(rec.lnZ - ref.QUAD_LNZ) <= 4 * rec.lnZ_se + 0.02
    assert abs(rec.lnZ_psis - ref.QUAD_LNZ) <= 4 * rec.lnZ_se + 0.02
    assert rec.lnZ_laplace == pytest.approx(rec.lnp_centre + 1.5 * math.log(2 * math.pi) + 0.5 * np.linalg.slogdet(cov)[1], abs=1e-9)
    # laplace_points factors inflate^2 cov itself: a factor an ulp off the case's, so the restatement runs on the record's own
    case = dict(c, chol=np.linalg.cholesky(1.5 ** 2 * cov))
    _report("quadrature case", ref.check(ref.from_record(rec), case, "quadrature"))
    assert rec.lnZ == pytest.approx(want["lnZ"], abs=1e-6) and rec.khat == pytest.approx(want["khat"], abs=1e-4)


def test_fit_laplace_at_the_map():
    """VPfit.laplace() after map_estimate on the one-line (K = 1) and two-line (K = 2) data of the evidence tests, beside the
    tempered ladder's recorded values.  Asserted: status 0, and that the one-line estimate agrees with the ladder's within
    4 combined standard errors + 0.02.  Measured on an MI355X: K = 1 lnZ 8.2198 +- 0.0129, khat -0.61, ESS 2432 (the ladder:
    8.218 +- 0.041); K = 2 on the two-line data lnZ 8.5029 +- 0.0210, khat -0.13, ESS 1453 (the ladder's recorded K = 2 figure,
    5.083 +- 1.373, is printed beside it: with that standard error it is no yardstick)"""
    from vamp_amd import laplace
    from vamp_amd.vpfits import VPfit
    ladder = {1: (8.218, 0.041), 2: (5.083, 1.373)}
    data = {1: evidence_ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3), 2: evidence_ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)}
    recs = {}
    for K, (x, flux, noise) in data.items():
        fit = VPfit(noise=noise, seed=5)
        fit.initialise_model(1.0e3 + 2.0 * x, flux, K, voigt=False)
        fit.map_estimate()
        rec = recs[K] = fit.laplace()
        print(f"K={K}: lnZ {rec.lnZ:.4f} +- {rec.lnZ_se:.4f} (psis {rec.lnZ_psis:.4f}, plain Laplace {rec.lnZ_laplace:.4f}) khat {rec.khat:.3f} "
              f"ess {rec.ess:.0f} n_out {rec.n_out} status {rec.status} | ladder {ladder[K][0]} +- {ladder[K][1]}")
        print("   mean", rec.mean, "sd", rec.sd, "MAP", fit._to_caller(fit._theta_dev))
        assert fit.laplace() is rec and rec.names == fit._names and rec.status == 0
        raw = laplace.fits_laplace([fit])[0]
        assert raw.lnZ == rec.lnZ and np.array_equal(raw.mean, rec.mean)
    one = recs[1]
    assert abs(one.lnZ - ladder[1][0]) <= 4 * math.hypot(one.lnZ_se, ladder[1][1]) + 0.02
