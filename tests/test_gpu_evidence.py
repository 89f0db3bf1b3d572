"""GPU tests (-m gpu) of libvamp_evid.so: the device's ln L / ln pi against the oracle, short trajectories of the
tempered ladder against the numpy restatement (tests/evidence_ref.py), determinism, batch independence, the accuracy
of ln Z against brute-force quadrature, model order, and the Python surface.

Tolerances: ln L and ln pi 1e-9 * max(1, |value|) with the same -inf pattern (the bound of the main library's
lnprob); trajectories rtol 1e-10 / atol 1e-12 (the bound of smoke() for the main sampler) with identical swap
decisions; ln Z within 4 standard errors + 0.02 of the quadrature, the standard error itself at most 0.15."""
import functools
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import evidence_ref as ref
from conftest import GOLDEN, ROOT, load_golden
from evidence_cases import SEED, as_dict as _as_dict, check_lnlike as _check_lnlike, synthetic as _synthetic
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu


def test_lnlike_matches_oracle_on_the_golden_cases():
    g = load_golden("lnprob_cases.npz")
    seen = set()
    for name in g["cases"]:
        name = str(name)
        mode = int(name.split("_m")[1].split("_")[0])
        if mode == vo.MODE_NBZ3:
            continue
        K, sd = int(name.split("_K")[1].split("_")[0]), bool(int(name.split("_sd")[1]))
        R = ref.make_region(g[name + "_x"], g[name + "_flux"], g[name + "_noise"], K, mode, sd)
        assert _check_lnlike(R, g[name + "_theta"], False, name) > 0, name           # bounds derived by the library
        seen.add((mode, sd))
    assert seen == {(0, False), (0, True), (1, False), (1, True)}


@pytest.mark.parametrize("P", [1, 15, 16, 17, 63, 64, 65, 300])
def test_lnlike_pixel_counts(P):
    for mode, sd, K in ((0, False, 2), (1, True, 2), (1, False, 5)):
        R, theta = _synthetic(P, K, mode, sd)
        assert _check_lnlike(R, theta, True, (P, mode, sd, K)) >= 30


@pytest.mark.parametrize("K", [1, 4, 5, 8])
def test_lnlike_line_counts(K):
    for mode, sd, P in ((0, True, 24), (1, False, 24), (0, False, 40), (1, True, 90)):      # 16-lane groups up to K = 4 and 32 px
        R, theta = _synthetic(P, K, mode, sd)
        assert _check_lnlike(R, theta, True, (K, mode, sd, P)) >= 30


def test_lnlike_descending_abscissa():
    for mode, P in ((0, 17), (1, 65)):
        R, theta = _synthetic(P, 2, mode, False, descending=True)
        up, _ = _synthetic(P, 2, mode, False)
        assert R.x[0] > R.x[-1]
        _check_lnlike(R, theta, True, ("descending", mode))
        _check_lnlike(R, theta, False, ("descending, derived bounds", mode))        # min / max of x, either direction
        from vamp_amd import evidence
        a = evidence.lnlike(_as_dict(R), theta)[0]
        b = evidence.lnlike(_as_dict(up), theta)[0]
        fin = np.isfinite(a)
        np.testing.assert_allclose(a[fin], b[fin], rtol=1e-12)


# ---- trajectories ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_regions():
    rng = np.random.default_rng(5)
    out = []
    for P, K, mode, sd in ((17, 1, 0, False), (65, 2, 1, True), (300, 8, 0, False)):
        x = np.arange(float(P)) - 0.5 * (P - 1)
        lines = [(rng.uniform(0.4, 1.5), rng.uniform(x[0], x[-1]), rng.uniform(1.0, 4.0)) for _ in range(K)]
        flux = np.exp(-sum(vo.gauss_function(x, *ln) for ln in lines)) + 0.05 * rng.standard_normal(P)
        out.append(ref.make_region(x, flux, np.full(P, 0.05), K, mode, sd))
    return tuple(out)


IDS = (11, 3, 40)


def _starts(regions, W, supplied):
    return [ref.prior_draws(R, 99000 + g, W, SEED + 1) for g, R in enumerate(regions)] if supplied else None


@functools.lru_cache(maxsize=None)
def _reference(T, W, supplied):
    regions = _mixed_regions()
    return ref.run(regions, IDS, ref.default_betas(T), W, 6, 0, 2, SEED, starts=_starts(regions, W, supplied))


@functools.lru_cache(maxsize=None)
def _device(T, W, supplied, only=None):
    from vamp_amd import evidence
    regions = _mixed_regions()
    starts = _starts(regions, W, supplied)
    sel = range(3) if only is None else [only]
    recs = evidence.log_evidence([_as_dict(regions[g], IDS[g], bounds=False) for g in sel], n_temps=T, walkers=W, steps=6, burn=0, swap_every=2,
                                 seed=SEED, start=None if starts is None else [starts[g] for g in sel], return_chain=True, trace=True)
    return recs


@pytest.mark.parametrize("supplied", [False, True], ids=["prior-start", "given-start"])
@pytest.mark.parametrize("T,W", [(2, 4), (3, 6), (5, 24)])
def test_trajectory_matches_the_restatement(T, W, supplied):
    want, got = _reference(T, W, supplied), _device(T, W, supplied)
    moved = 0
    for g in range(3):
        w, d = want[g], got[g]
        assert d.chain.shape == w["chain"].shape and d.lnl_trace.shape == (6, T, W) and d.swap_trace.shape == (2, T - 1, W)
        assert np.array_equal(d.swap_trace, w["swap_trace"]), g
        np.testing.assert_allclose(d.lnl_trace, w["lnl_trace"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(d.chain, w["chain"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(d.chain_lnl, w["chain_lnl"], rtol=1e-10, atol=1e-12)
        np.testing.assert_array_equal(d.chain_lnl, d.lnl_trace[:, -1])
        np.testing.assert_allclose(d.move_accept, w["move_accept"], rtol=0, atol=1e-15)
        np.testing.assert_allclose(d.swap_accept, w["swap_accept"], rtol=0, atol=1e-15)
        np.testing.assert_allclose(d.mean_lnL, w["mean_lnL"], rtol=1e-10)
        np.testing.assert_allclose(d.var_lnL, w["var_lnL"], rtol=1e-8, atol=1e-12)
        assert d.lnZ == pytest.approx(w["lnZ"], rel=1e-9, abs=1e-9) and d.lnZ_ti == pytest.approx(w["lnZ_ti"], rel=1e-9, abs=1e-9)
        assert math.isnan(d.lnZ_se)                                   # fewer than 8 kept steps
        np.testing.assert_array_equal(d.betas, ref.default_betas(T))
        moved += int(w["move_accept"].sum() > 0) + int(w["swap_trace"].sum() > 0)
    assert moved >= 4        # the comparison saw accepted moves and accepted swaps


def test_same_seed_is_bit_identical_and_a_region_alone_equals_the_batch():
    from vamp_amd import evidence
    regions = _mixed_regions()
    batch = _device(5, 24, False)
    again = evidence.log_evidence([_as_dict(regions[g], IDS[g], bounds=False) for g in range(3)], n_temps=5, walkers=24, steps=6, burn=0,
                                  swap_every=2, seed=SEED, return_chain=True, trace=True)
    for g in range(3):
        alone = _device(5, 24, False, only=g)[0]
        for other in (again[g], alone):
            for k in ("chain", "chain_lnl", "lnl_trace", "swap_trace", "mean_lnL", "var_lnL", "move_accept", "swap_accept"):
                assert np.array_equal(getattr(batch[g], k), getattr(other, k)), (g, k)
            assert batch[g].lnZ == other.lnZ and batch[g].lnZ_ti == other.lnZ_ti
    other_seed = evidence.log_evidence(_as_dict(regions[0], IDS[0]), n_temps=5, walkers=24, steps=6, burn=0, swap_every=2, seed=SEED + 1,
                                       return_chain=True)
    assert not np.array_equal(other_seed.chain, batch[0].chain)


def test_device_chain_output_equals_the_host_one():
    import ctypes as C
    import torch
    from vamp_amd import _evid_lib, evidence
    R = _mixed_regions()[0]
    host = evidence.log_evidence(_as_dict(R, 11, bounds=False), n_temps=3, walkers=6, steps=6, burn=2, swap_every=2, seed=SEED, return_chain=True)
    lib = _evid_lib.load()
    chain = torch.zeros((4, 6, 3), dtype=torch.float64, device="cuda")
    cll = torch.zeros((4, 6), dtype=torch.float64, device="cuda")
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    i32 = lambda v: np.array([v], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lnz = np.empty(1)
    torch.cuda.synchronize()
    rc = lib.vamp_evid_run(0, None, 1, one(R.x), one(R.flux), one(R.noise), i32(17), i32(1), i32(0), i32(0), None, i32(11), 3, None, 6, 6, 2, 2,
                           SEED, 2.0, None, lnz.ctypes.data_as(C.POINTER(C.c_double)), *([None] * 6), (C.c_void_p * 1)(chain.data_ptr()),
                           (C.c_void_p * 1)(cll.data_ptr()), 1, None, None)
    _evid_lib.check(rc, lib)
    assert lnz[0] == host.lnZ
    assert np.array_equal(chain.cpu().numpy(), host.chain) and np.array_equal(cll.cpu().numpy(), host.chain_lnl)


def test_refusals_that_need_the_device():
    from vamp_amd import _evid_lib, evidence
    R = _mixed_regions()[0]
    start = ref.prior_draws(R, 1, 6, SEED)
    start[4, 1] = R.c_hi + 1.0
    with pytest.raises(_evid_lib.EvidError, match="start walker 4 of rung 0 is outside the prior"):
        evidence.log_evidence(_as_dict(R), n_temps=3, walkers=6, steps=4, burn=0, start=start)
    with pytest.raises(_evid_lib.EvidError, match="no HIP device"):
        evidence.log_evidence(_as_dict(R), n_temps=3, walkers=6, steps=4, burn=0, device=4096)


# ---- accuracy and model order ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _order_runs():
    """K = 1 and K = 2 on the one-line and on the two-line data, defaults (T = 16, W = 32, burn 200, 400 kept): one call"""
    from vamp_amd import evidence
    one = ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
    two = ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    regs = [{"x": d[0], "flux": d[1], "noise": d[2], "n_comp": K, "mode": 0} for d in (one, two) for K in (1, 2)]
    return one, evidence.log_evidence(regs, seed=SEED)


def test_lnZ_against_quadrature():
    """the issue's bound: |lnZ - quadrature| <= 4 lnZ_se + 0.02 with lnZ_se <= 0.15.  Measured on an MI355X with this
    seed: lnZ 8.2183, se 0.0412 against 8.2270 (the trapezoid: 7.9699); the figures are printed before the assertions"""
    (x, flux, noise), recs = _order_runs()
    quad = ref.quadrature_lnZ(x, flux, noise, 80)
    r = recs[0]
    print("lnZ", r.lnZ, "se", r.lnZ_se, "ti", r.lnZ_ti, "quadrature", quad, "move", r.move_accept, "swap", r.swap_accept)
    assert quad == pytest.approx(8.227, abs=2e-3)
    assert r.lnZ_se <= 0.15
    assert abs(r.lnZ - quad) <= 4 * r.lnZ_se + 0.02
    assert math.isfinite(r.lnZ_ti)                      # the trapezoid sits about 0.25 low on this ladder: reported, not asserted
    assert r.mean_lnL[-1] > r.mean_lnL[0] and np.all((r.move_accept > 0.05) & (r.move_accept < 0.95)) and np.all(r.swap_accept > 0.05)


def test_model_order():
    _, recs = _order_runs()
    one1, one2, two1, two2 = recs
    print("one line: K=1", one1.lnZ, one1.lnZ_se, "K=2", one2.lnZ, one2.lnZ_se, "| two lines: K=1", two1.lnZ, two1.lnZ_se, "K=2", two2.lnZ, two2.lnZ_se)
    assert two2.lnZ - two1.lnZ > 20
    assert one2.lnZ <= one1.lnZ + 4 * math.hypot(one1.lnZ_se, one2.lnZ_se)


def test_region_fit_by_evidence_finds_two_lines():
    from vamp_amd.vpregion import VPregion
    x, flux, noise = ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    reg = VPregion(1.0e3 + x, flux, noise, seed=12, nwalkers=32)
    assert reg.n == 1
    reg.region_fit(verbose=False, iterations=300, thin=5, burn=100, criterion="evidence")
    print({n: (r.lnZ, r.lnZ_se) for n, r in reg.evidences.items()})
    assert reg.n == 2 and reg.fit._n == 2 and sorted(reg.evidences) == [1, 2, 3]
    assert reg.fit.evidence is reg.evidences[2] and len(reg.fit.bic_array) == 3


# ---- the Python surface ------------------------------------------------------------------------------------
def test_fit_and_spectrum_evidences(tmp_path):
    from vamp_amd import h5min
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
        fit.nwalkers = 32
        fit.initialise_model(region.frequency_array, region.flux_array, 1 + j, voigt=False)
        fit.mcmc_fit(iterations=60, burnin=20, thinning=2)
        region.fit, region.n = fit, 1 + j
        spec.regions.append(region)
    kw = dict(steps=120, burn=40, n_temps=8)
    fit = spec.regions[0].fit
    rec = fit.log_evidence(**kw)
    assert fit.evidence is rec and math.isfinite(rec.lnZ) and rec.lnZ_se >= 0 and rec.betas.size == 8 and rec.chain is None
    ev = spec.evidences(**kw)
    assert set(ev) == {"lnZ", "lnZ_se", "lnZ_ti", "n_comp", "betas", "mean_lnL", "var_lnL", "move_accept", "swap_accept"}
    assert ev["lnZ"].shape == (2,) and ev["mean_lnL"].shape == (2, 8) and ev["swap_accept"].shape == (2, 7) and np.all(np.isfinite(ev["lnZ"]))
    assert ev["n_comp"].tolist() == [1, 2] and spec.regions[1].fit.evidence.lnZ == ev["lnZ"][1]
    assert ev["lnZ"][0] == rec.lnZ               # region 0 of the batch and the fit alone: the same keys, the same start
    spec.output_filename = str(tmp_path / "spectrum_0_gauss_")
    path = spec.write_evidence(ev)
    assert path.endswith("spectrum_0_gauss_evidence.h5")
    back = _read_h5(path)
    assert set(back) == set(ev)
    for k in ev:
        np.testing.assert_array_equal(back[k], ev[k])


def _read_h5(path):
    try:
        import h5py
        with h5py.File(path, "r") as f:
            return {k: f[k][()] for k in f}
    except ImportError:
        from vamp_amd import h5min
        return h5min.read(str(path))


def test_do_vamp_evidence_writes_the_file(tmp_path):
    out = tmp_path / "out"
    spec = tmp_path / "spectrum_4.h5"
    shutil.copy(os.path.join(GOLDEN, "simba_H1215.h5"), spec)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    rc = subprocess.run([sys.executable, "-m", "vamp_amd.do_vamp", str(spec), "1215.6701", "--output_folder", str(out),
                         "--conv_attempts", "1", "--walkers", "32", "--iterations", "300", "--burn", "100", "--thin", "5",
                         "--seed", "3", "--evidence"], env=env, capture_output=True, text=True, timeout=900)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [ln for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    assert len(lines) == 1
    rec = json.loads(lines[0][len("vamp_perf "):])
    assert 0.0 <= rec["evidence_seconds"] < rec["seconds"] + 60
    ev = _read_h5(out / "spectrum_4_gauss_evidence.h5")
    nreg = rec["regions"]
    assert ev["lnZ"].shape == (nreg,) and ev["betas"].shape == (16,) and ev["mean_lnL"].shape == (nreg, 16)
    fits8 = ev["n_comp"] <= 8                     # a fit of more lines than the library takes has NaN rows
    assert np.all(np.isfinite(ev["lnZ"][fits8])) and np.all(ev["lnZ_se"][fits8] >= 0) and fits8.any() and int(ev["n_comp"].sum()) == rec["lines"]
