"""GPU tests (-m gpu) of libvamp_hmc.so: every case goes through hmc_ref.check -- the library's momenta, proposals, energy
errors, accept decisions, walls, kept states and counts each against the restatement evaluated on the library's OWN
outputs of the stage before, at the bars derived or measured in tests/hmc_ref.py -- at the smallest shapes where a path
changes; then the walls, the statuses, bit-for-bit independence of a chain from the rest of the call, reversal and the
order of the energy error on the device, invariance of the exact posterior, and the Python surface.  The worst error
over its bar is printed per case and stage (profiles/hmc_limits.txt holds a run's figures)."""
import os

import numpy as np
import pytest

import evidence_ref
import hmc_ref as ref
import sampler_stats

pytestmark = pytest.mark.gpu

PER_CHAIN = ("n_accept", "n_wall", "chain_status", "dH_mean", "dH_max")
LISTS = ("chain", "last", "lnp", "mom", "prop", "prop_mom", "dH", "acc")


def _args(cases):
    c0 = cases[0]
    assert len({(c["L"], c["n_steps"], c["n_burn"], c["thin"], c["step0"], c["seed"]) for c in cases}) == 1
    return dict(xs=[c["x"] for c in cases], fluxes=[c["flux"] for c in cases], noises=[c["noise"] for c in cases],
                n_comp=[c["n_comp"] for c in cases], modes=[c["mode"] for c in cases], sample_sd=[int(c["sample_sd"]) for c in cases],
                bounds=[None if c["bounds"] is None else np.array(c["bounds"]) for c in cases], region_ids=[c["region_id"] for c in cases],
                n_chains=[len(c["start"]) for c in cases], chain_id0=[c["chain_id0"] for c in cases], starts=[c["start"] for c in cases],
                chols=[c["chol"] for c in cases], eps=[c["eps"] for c in cases], jitter=[c["jitter"] for c in cases], n_leap=c0["L"],
                n_steps=c0["n_steps"], n_burn=c0["n_burn"], thin=c0["thin"], step0=c0["step0"], seed=c0["seed"])


def _unflatten(flat, cases):
    """the outputs of ``hmc._call`` as one dict per group (what ``check`` takes)"""
    out, o = [], 0
    for g, c in enumerate(cases):
        n = len(c["start"])
        r = {k: flat[k][o:o + n] for k in PER_CHAIN if k in flat}
        r.update({k: flat[k][g] for k in LISTS if k in flat})
        if "status" in flat:
            r["status"] = int(flat["status"][g])
        out.append(r)
        o += n
    return out


def _lib(cases, **kw):
    """one library call for cases of one set of call parameters, every output asked for"""
    from vamp_amd import hmc
    return _unflatten(hmc._call(0, **_args(cases), **kw), cases)


def _same(a, b, keys=None):
    """whether two results agree bit for bit in every output both hold; the outputs that differ are printed"""
    keys = [k for k in (keys or a) if k in a and k in b]
    differ = [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]
    if differ:
        print("differ:", differ)
    return not differ and bool(keys)


def _report(label, worst):
    print(f"{label:36s} " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ---- every stage at its bar ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.SHAPES)
def test_single_leap_steps_at_first_order_bars(name):
    """L = 1, seven moves kept every third (thin does not divide n_steps), n_burn = 0, no jitter"""
    c = ref.shape_case(name, 1)
    got = _lib([c])[0]
    _report(f"L=1 {name} acc={np.bincount(got['acc'].ravel(), minlength=3)}", ref.check(got, c, name))
    assert got["status"] == 0 and got["chain"].shape == (3, len(c["start"]), c["start"].shape[1])


@pytest.mark.parametrize("name", ref.SHAPES)
def test_eight_leaps_at_measured_bars(name):
    """L = 8, five moves of which the last is kept (n_burn = n_steps - 1), jitter 0.5.  The bars are measured on the CPU at
    this very case: the fp64 restatement against the longdouble one with perturbed gradients, times four"""
    c = ref.shape_case(name, 8)
    bars = ref.measured_bars(c)
    got = _lib([c])[0]
    w = ref.check(got, c, name, bars=bars)
    _report(f"L=8 {name} bars prop={bars['prop']:.2g} mom={bars['prop_mom']:.2g} dH={bars['dH']:.2g}", w)
    assert got["status"] == 0 and got["chain"].shape[0] == 1


def test_accept_decisions():
    c = ref.decisions_case()
    got = _lib([c])[0]
    w = ref.check(got, c, "decisions")
    _report(f"decisions acc={np.bincount(got['acc'].ravel(), minlength=3)}", w)
    assert w["undecided"] <= ref.MAX_UNDECIDED and 0.2 * got["acc"].size < np.sum(got["acc"] == 0) < 0.8 * got["acc"].size
    assert np.array_equal(got["acc"], ref.run(c)["acc"])


def test_walls():
    """starts next to L_fwhm = 0: acc = 2 exactly where the restatement has it, the state unchanged bit for bit after a
    wall, n_wall counted exactly"""
    c = ref.wall_case()
    got = _lib([c])[0]
    want = ref.run(c)
    _report(f"walls {np.bincount(got['acc'].ravel(), minlength=3)}", ref.check(got, c, "walls"))
    assert np.array_equal(got["acc"], want["acc"]) and np.array_equal(got["n_wall"], want["n_wall"])
    walls = got["acc"] == 2
    assert 0.3 * walls.size < walls.sum() < 0.8 * walls.size and np.all(np.isnan(got["dH"][walls]))
    for ch in range(walls.shape[1]):
        for t in range(walls.shape[0]):
            if walls[t, ch]:
                before = c["start"][ch] if t == 0 else got["chain"][t - 1, ch]
                assert np.array_equal(got["chain"][t, ch], before) and (t == 0 or got["lnp"][t, ch] == got["lnp"][t - 1, ch])


# ---- statuses and independence -----------------------------------------------------------------------------------
def _batch(L=1):
    """groups of different D, P and C in one call, with a group without a factor and a chain with a bad start among them"""
    kw = dict(seed=11)
    ok = [ref.shape_case("C5", L, region_id=3, **kw), ref.shape_case("P33K5", L, region_id=4, **kw), ref.shape_case("D3", L, region_id=5, **kw),
          ref.shape_case("D65", L, region_id=9, **kw)]
    no_factor = ref.shape_case("C4", L, region_id=6, **kw)
    no_factor["chol"][3, 3] = 0.0
    nan_entry = ref.shape_case("D4", L, region_id=7, **kw)
    nan_entry["chol"][3, 1] = np.nan
    bad_start = ref.shape_case("P65", L, region_id=8, **kw)
    bad_start["start"][1, 2] = -0.01                        # L_fwhm < 0 in chain 1 of 3
    return [ok[0], no_factor, ok[1], bad_start, nan_entry, ok[2], ok[3]]


def test_statuses_in_the_middle_of_a_batch():
    cases = _batch()
    got = _lib(cases)
    assert [g["status"] for g in got] == [0, 1, 0, 0, 1, 0, 0]
    for c, g in zip(cases, got):
        ref.check(g, c, f"region {c['region_id']}")
    assert list(got[3]["chain_status"]) == [0, 2, 0] and np.all(np.isnan(got[3]["chain"][:, 1])) and np.all(np.isfinite(got[3]["chain"][:, [0, 2]]))
    # the other chains of the group are those of a call without the bad one
    c = cases[3]
    for i in (0, 2):
        alone = _lib([dict(c, start=c["start"][i:i + 1], chain_id0=i)])[0]
        assert all(np.array_equal(alone[k][:, 0], got[3][k][:, i]) for k in ("chain", "lnp", "mom", "prop", "prop_mom", "dH", "acc"))
    eps0 = dict(cases[0], eps=0.0)
    assert _lib([eps0])[0]["status"] == 1 and _lib([dict(cases[0], jitter=1.0)])[0]["status"] == 1


@pytest.mark.parametrize("L", [1, 8])
def test_a_group_alone_reversed_and_on_a_stream_equals_the_batch_bit_for_bit(L):
    import torch
    cases = _batch(L)
    got = _lib(cases)
    for c, g in zip(cases, got):
        assert _same(_lib([c])[0], g), c["region_id"]
    assert all(_same(a, b) for a, b in zip(_lib(cases[::-1])[::-1], got))
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(_lib(cases, stream=stream.cuda_stream), got))


def test_a_chain_alone_through_chain_id0():
    c = ref.shape_case("C9", 8)
    got = _lib([c])[0]
    for i in (0, 3, 4, 8):
        alone = _lib([dict(c, start=c["start"][i:i + 1], chain_id0=i)])[0]
        assert all(np.array_equal(alone[k][:, 0], got[k][:, i]) for k in ("chain", "lnp", "mom", "prop", "prop_mom", "dH", "acc")), i
        assert all(alone[k][0] == got[k][i] for k in PER_CHAIN)
    # a chain among larger groups (another number of chains per workgroup) is the same chain
    big = ref.shape_case("D65", 8)
    both = _lib([c, big])
    assert _same(both[0], got) and _same(both[1], _lib([big])[0])


def test_device_arrays_null_outputs_given_momenta_and_a_continued_run():
    import torch
    from vamp_amd import hmc
    cases = [ref.shape_case("C5", 8, region_id=3), ref.shape_case("P33K5", 8, region_id=4)]
    got = _lib(cases)
    n_keep = got[0]["chain"].shape[0]
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0").contiguous()
    starts = [dev(c["start"]) for c in cases]
    chains = [torch.full((n_keep,) + c["start"].shape, 7.0, dtype=torch.float64, device="cuda:0") for c in cases]
    lasts = [torch.full(c["start"].shape, 7.0, dtype=torch.float64, device="cuda:0") for c in cases]
    torch.cuda.synchronize()
    args = _args(cases)
    flat = hmc._call(0, **args, device_ptrs={"start": [t.data_ptr() for t in starts], "chain": [t.data_ptr() for t in chains],
                                            "last": [lasts[0].data_ptr(), None]})
    torch.cuda.synchronize()
    for g, d, ch in zip(got, _unflatten(flat, cases), chains):
        assert "chain" not in d and _same(d, g) and np.array_equal(ch.cpu().numpy(), g["chain"])
    assert np.array_equal(lasts[0].cpu().numpy(), got[0]["last"]) and float(lasts[1].min()) == 7.0
    # every per-chain output alone, and no trace
    for keep in PER_CHAIN + ("status",):
        flat = hmc._call(0, **args, want=(), skip=tuple(k for k in PER_CHAIN + ("status", "chain", "last", "lnp") if k != keep))
        assert set(flat) == {keep}
        assert all(np.array_equal(a[keep], g[keep], equal_nan=True) for a, g in zip(_unflatten(flat, cases), got)), keep
    assert all(_same(a, g) and "mom" not in a for a, g in zip(_unflatten(hmc._call(0, **args, want=("dH",)), cases), got))
    # the library's own momenta given back reproduce the run
    again = _lib(cases, mom_in=[g["mom"] for g in got])
    assert all(_same(a, g) for a, g in zip(again, got))
    ref.check(again[0], cases[0], "momenta given", bars=ref.measured_bars(cases[0]), mom_in=got[0]["mom"])
    # a run continued from `last` with the step offset is the run: 3 + 4 single-leap moves against 7
    whole = [ref.shape_case("C5", 1, region_id=3), ref.shape_case("P33K5", 1, region_id=4)]
    full = _lib([dict(c, thin=1) for c in whole])
    first = _lib([dict(c, thin=1, n_steps=3) for c in whole])
    second = _lib([dict(c, thin=1, n_steps=4, step0=3, start=f["last"]) for c, f in zip(whole, first)])
    for f, a, b in zip(full, first, second):
        assert all(np.array_equal(np.concatenate([a[k], b[k]]), f[k]) for k in ("chain", "lnp", "mom", "prop", "dH", "acc"))
        assert np.array_equal(b["last"], f["last"])


# ---- the integrator on the device ----------------------------------------------------------------------------------
def test_reversal_on_the_device():
    """one move of L = 8 from the start; a second call from the first one's ``prop`` with -``prop_mom`` as the given momentum
    returns to the start, at the bar of the CPU test (the gradient the way back meets is the way there's, evaluated again)"""
    from test_hmc import reversal_bar
    for mode, sd in ((0, False), (0, True), (1, False), (1, True)):
        c = ref.lines_case(40 if mode == 0 else 65, 2, mode, sd, 4, 8, 1)
        there = _lib([c])[0]
        assert not np.any(there["acc"] == 2)
        back = _lib([dict(c, start=there["prop"][0])], mom_in=[-there["prop_mom"]])[0]
        scale = ref.metric_scale(c)
        for i in range(4):
            bar = reversal_bar(c, c["start"][i], there["mom"][0, i])
            err = max(float(np.max(np.abs(back["prop"][0, i] - c["start"][i]) / scale)), float(np.max(np.abs(back["prop_mom"][0, i] + there["mom"][0, i]))))
            print("mode", mode, "sd", sd, "chain", i, "reversal error", err, "bar", bar)
            assert err <= bar


def test_energy_error_is_second_order_on_the_device():
    for a, b in ref.ratio_cases():
        da, db = _lib([a])[0]["dH"][0], _lib([b])[0]["dH"][0]
        ratio = np.abs(da) / np.abs(db)
        print("mode", a["mode"], "sd", a["sample_sd"], "ratios", ratio)
        assert np.all((ratio >= 3.0) & (ratio <= 5.0))


# ---- invariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd", [False, True])
def test_exact_posterior_stays_invariant_on_the_device(sd):
    """the CPU test's honest leg on the device: N = 4096 chains from exact draws, the same T, eps and L; the marginals pass
    KS_BAR and the acceptance is within ACC_SIGMAS of the restatement's on the same starts (standard errors from the
    scatter of the chains' own rates)"""
    post, X0, chol, kw = ref.invariance_leg(sd)
    c = ref.make_case(post.x, post.flux, None if sd else post.noise_fixed, 1, 0, X0, chol, kw["eps"], kw["n_leap"], kw["n_steps"], 77,
                      n_burn=kw["n_steps"] - 1, region_id=2)
    from vamp_amd import hmc
    flat = hmc._call(0, **_args([c]), want=())
    X = flat["last"][0]
    assert np.all(flat["chain_status"] == 0) and np.array_equal(X, flat["chain"][0][0])
    ks = ref.ks_of(post, X)
    rate = flat["n_accept"] / kw["n_steps"]
    _, n_ref, _ = ref.vector_hmc(post, X0, chol, kw["eps"], kw["n_leap"], kw["n_steps"], np.random.default_rng(ref.INVARIANCE_SEED))
    rate_ref = n_ref / kw["n_steps"]
    se = np.hypot(rate.std(ddof=1), rate_ref.std(ddof=1)) / np.sqrt(len(X0))
    print("sd", sd, "ks", np.round(ks, 2), "acceptance", rate.mean(), "restatement", rate_ref.mean(), "se", se, "walls", flat["n_wall"].mean() / kw["n_steps"])
    assert max(ks) < sampler_stats.KS_BAR
    assert abs(rate.mean() - rate_ref.mean()) <= sampler_stats.ACC_SIGMAS * se


# ---- the Python surface --------------------------------------------------------------------------------------------
def test_fits_hmc_diagnostics_and_posterior_take_the_chain():
    """fits_hmc on the two-line data of tests/test_gpu_laplace.py: the record's chain goes unchanged into
    ``HmcRecord.diagnostics()`` (libvamp_diag.so) and ``posterior.posterior_summaries`` (libvamp_post.so)"""
    from vamp_amd import hmc, posterior
    from vamp_amd.vpfits import VPfit
    x, flux, noise = evidence_ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    fit = VPfit(noise=noise, seed=5)
    fit.initialise_model(1.0e3 + 2.0 * x, flux, 2, voigt=False)
    fit.map_estimate()
    rec = fit.hmc(n_chains=8, n_steps=120, n_burn=40, seed=3)
    assert fit.hmc(n_chains=8, n_steps=120, n_burn=40, seed=3) is rec and rec.names == fit._names
    raw = hmc.fits_hmc([fit], n_chains=8, n_steps=120, n_burn=40, seed=3)[0]
    assert np.array_equal(raw.chain, rec.chain)
    d = rec.diagnostics()
    mean, sd, q = rec.summary()
    print("eps", rec.eps, "accept", rec.accept_rate.mean(), "walls", rec.n_wall.sum(), "r_hat", d.r_hat, "n_eff", d.n_eff)
    print("mean", mean, "sd", sd, "MAP", fit._to_caller(fit._theta_dev))
    D = len(fit._scale)
    assert rec.status == 0 and rec.chain.shape == (80, 8, D) and np.all(rec.chain_status == 0) and np.all(np.isfinite(rec.chain))
    assert 0.3 < rec.accept_rate.mean() <= 1.0 and d.r_hat.shape == (D,) and np.all(np.isfinite(d.r_hat)) and np.all(d.n_eff > 0)
    assert np.all(np.abs(mean - fit._to_caller(fit._theta_dev)) < 5 * sd)
    # the chain in device units, as the chain consumers take a fit's
    dev = (rec.chain - fit._shift) / fit._scale
    summ = posterior.posterior_summaries(fit._x, np.ascontiguousarray(dev), 2, 0, sample_sd=bool(fit._sample_sd))
    assert summ.n_used == 80 * 8 and summ.n_bad == 0 and summ.flux_mean.shape == x.shape and np.all(np.isfinite(summ.flux_mean))
    assert np.max(np.abs(summ.flux_mean - flux)) < 0.5


def test_do_vamp_hmc_writes_hmc_h5(tmp_path):
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
                         "--seed", "3", "--batched", "--hmc"], env=env, capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    perf = [json.loads(ln[len("vamp_perf "):]) for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    line = [json.loads(ln[len("vamp_hmc "):]) for ln in rc.stdout.splitlines() if ln.startswith("vamp_hmc ")]
    assert len(perf) == 1 and len(line) == 1 and "hmc_seconds" not in perf[0]
    print(line[0])
    back = h5min.read(str(out / "spectrum_4_gauss_hmc.h5"))
    R = perf[0]["regions"]
    assert back["status"].shape == (R,) and back["eps"].shape == (R,) and int(back["n_comp"].sum()) == perf[0]["lines"]
    n_par = back["par_region"].size
    assert back["mean"].shape == (n_par,) and back["quantiles"].shape == (n_par, 3) and back["r_hat"].shape == (n_par,)
    assert set(np.unique(back["status"])) <= {0, 1} and line[0]["regions_sampled"] == int((back["status"] == 0).sum()) >= 1
    ok = back["status"][back["par_region"]] == 0
    assert np.all(np.isfinite(back["mean"][ok])) and np.all(back["sd"][ok] > 0) and np.all(back["n_eff"][ok] > 0)
    assert np.all(back["quantiles"][ok, 0] <= back["quantiles"][ok, 1]) and np.all(back["quantiles"][ok, 1] <= back["quantiles"][ok, 2])
    assert np.all(back["accept_rate"][back["status"] == 0] > 0) and np.all(back["eps"][back["status"] == 0] > 0)
