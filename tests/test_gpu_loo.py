"""GPU tests of libvamp_loo.so against the numpy restatement (tests/loo_ref.py).

The column stage is compared on exact inputs: vamp_loo_from_loglik gets the restatement's own log-likelihood matrix, so
the same doubles go in on both sides and only the arithmetic of PSIS differs.  Bars (loo_ref.bars): khat 1e-10 max(1,
|khat|), elpd_loo_pix 1e-11 max(1, |v|), p_loo_pix that plus the same bar on lppd, a group sum the sum of its pixels'
bars, elpd_loo_se 1e-9 relative; the +-inf and NaN patterns, n_high_k and the counts equal.  tests/test_loo.py shows on
the CPU that the float64 restatement sits at 1e-13 (khat) and 2e-15 (elpd) of an extended-precision one on these very
inputs -- three orders inside the bars, and above the M ulp amplification of L_j = M (...) -- that no khat of them lies
within 1e-6 of 0.7, and that a tail length off by one, a missing prior, a missing truncation, a cutoff taken inside the
tail and a dropped sample each miss the bars by 1e4 or more.  The evaluation is compared through the returned matrix:
l_sp at the flux bar of the posterior tests carried through, 1e-12 |y - f| / sigma^2 + 1e-12 max(1, |l|), and lppd at
predictive_ref.bars; and every PSIS output of vamp_loo_pointwise must be, bit for bit, what vamp_loo_from_loglik makes
of that matrix.  Every case prints its worst error / bar (profiles/loo_limits.txt)."""
import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import evidence_ref
import loo_ref as ref
import posterior_ref as pref
import predictive_ref
from conftest import GOLDEN, ROOT
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu

_ID = lambda c: "S%d-%s-sd%d" % (c[1], c[2], c[3])


def _records(flat, n_pix):
    """per-group dicts of the header's outputs from a call's flat arrays"""
    out, op = [], 0
    for g, P in enumerate(n_pix):
        out.append({**{k: flat[k][op:op + P] for k in ref.PIX if k in flat}, **{k: flat[k][g] for k in ref.GRP + ref.CNT if k in flat}})
        op += P
    return out


def _from_loglik(mats, skips=None, device_input=False, **kw):
    """vamp_loo_from_loglik on host matrices, or on copies of them in device memory"""
    from vamp_amd import loo
    mats = [np.ascontiguousarray(m, dtype=np.float64) for m in mats]
    shape = ([m.shape[0] for m in mats], [m.shape[1] for m in mats])
    if device_input:
        import torch
        dev = [torch.tensor(m, device="cuda:0") for m in mats]
        torch.cuda.synchronize()
        flat = loo._call_loglik(0, [t.data_ptr() for t in dev], *shape, skips, True, **kw)
    else:
        flat = loo._call_loglik(0, [m.ctypes.data for m in mats], *shape, skips, False, **kw)
    return _records(flat, shape[1])


def _same(a, b, keys=ref.FLAT):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=k not in ref.CNT), k


def _report(label, S, P, worst):
    print("loo %-62s S %5d P %3d worst error / bar %.3g" % (label, S, P, worst))


# ---- 1. the column stage on exact inputs ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.COLUMN_CASES, ids=_ID)
def test_column_stage_on_the_restatement_s_matrix(case):
    ll, want = ref.column_case(case)
    fin = np.isfinite(want["khat"])
    assert not fin.any() or np.min(np.abs(want["khat"][fin] - ref.HIGH_KHAT)) > 1e-6
    host = _from_loglik([ll])[0]
    _report("column stage %s, host matrix" % _ID(case), ll.shape[0], ll.shape[1], ref.check(host, want, _ID(case)))
    assert host["n_used"] == case[1] and host["n_bad"] == 0
    dev = _from_loglik([ll], device_input=True)[0]
    _same(host, dev)


def test_column_stage_with_skipped_samples():
    """n = 20 from S = 23 and n = 21 from S = 24: three skipped rows, never read (they hold NaN), first, inside and last"""
    mats, skips, wants = [], [], []
    for case in ref.COLUMN_CASES[:2]:
        ll, want = ref.column_case(case)
        S = ll.shape[0] + 3
        skip = np.isin(np.arange(S), (0, 11, S - 1)).astype(np.uint8)
        full = np.full((S, ll.shape[1]), np.nan)
        full[skip == 0] = ll
        mats.append(full)
        skips.append(skip)
        wants.append(dict(want, n_bad=3))
    assert [w["n_used"] for w in wants] == [20, 21]
    for label, got in (("host", _from_loglik(mats, skips)), ("device", _from_loglik(mats, skips, device_input=True))):
        for g, w in zip(got, wants):
            _report("skip on three samples, %s matrix, n = %d" % (label, w["n_used"]), w["n_used"] + 3, 44, ref.check(g, w, label))
    assert np.isposinf(got[0]["khat"]).all() and np.isfinite(got[1]["khat"]).all()
    no_skip = _from_loglik(mats[:1], [None])[0]                    # the NaN rows are read when nothing says to skip them
    assert np.isnan(no_skip["elpd_loo_pix"]).all() and no_skip["n_used"] == 23


# ---- 2. and 3. the evaluation, and one column code ---------------------------------------------------------------
def _eval_groups():
    """K = 4 Voigt with known noise (G <= 0 and a NaN parameter among the samples), K = 2 Gauss with free sd (sd <= 0 and a
    NaN parameter), and the Gauss data cut to 30 pixels: a 16-lane group owns a sample"""
    groups = []
    for seed, S, data, sd, W, cut in ((51, 129, "K4", False, 1, None), (52, 65, "K2", True, 5, None), (53, 66, "K2", False, 6, 30)):
        x, flux, noise, theta, K, mode = ref.ball_case(seed, S, data, sd)
        if data == "K4":
            theta[7, 3] = -1.0
            theta[9, 4] = np.nan
        elif sd:
            theta[11, -1] = 0.0
            theta[64, 1] = np.nan
        sl = slice(0, cut)
        groups.append({"x": x[sl].copy(), "flux": flux[sl].copy(), "noise": None if noise is None else noise[sl].copy(),
                       "chain": theta.reshape(S // W, W, -1).copy(), "K": K, "mode": mode, "sd": sd})
    return groups


def _pointwise_args(groups):
    return ([g["x"] for g in groups], [g["flux"] for g in groups], [g["noise"] for g in groups], [g["K"] for g in groups],
            [g["mode"] for g in groups], [int(g["sd"]) for g in groups], [g["chain"].ctypes.data for g in groups], False,
            [g["chain"].shape[1] * g["chain"].shape[2] for g in groups], [g["chain"].shape[0] for g in groups], [g["chain"].shape[1] for g in groups])


def _want(g):
    return ref.pointwise(g["x"], g["flux"], g["noise"], g["chain"], g["K"], g["mode"], g["sd"])


@pytest.fixture(scope="module")
def evaluated():
    """(groups, the flat result of ONE vamp_loo_pointwise call with the ll output, the restatements)"""
    from vamp_amd import loo
    groups = _eval_groups()
    flat = loo._call(0, *_pointwise_args(groups), want=ref.FLAT + ("ll",))
    return groups, flat, [_want(g) for g in groups]


def test_evaluation_against_the_restatement(evaluated):
    groups, flat, wants = evaluated
    recs = _records(flat, [g["x"].size for g in groups])
    assert [w["n_bad"] for w in wants] == [2, 2, 0]
    for g, rec, ll, w in zip(groups, recs, flat["ll"], wants):
        S, P = w["ll"].shape
        assert ll.shape == (S, P) and (rec["n_used"], rec["n_bad"]) == (w["n_used"], w["n_bad"])
        assert np.isnan(ll[w["bad"]]).all() and np.isfinite(ll[~w["bad"]]).all()
        good = ~w["bad"]
        bar = 1e-12 * w["dl"][good] + 1e-12 * np.maximum(1.0, np.abs(w["ll"][good]))
        worst = float(np.max(np.abs(ll[good] - w["ll"][good]) / bar))
        lppd_bar = predictive_ref.bars(w)["lppd"]
        worst_lppd = float(np.max(np.abs(rec["lppd"] - w["lppd"]) / lppd_bar))
        _report("evaluation K=%d mode=%d free_sd=%d: l_sp" % (g["K"], g["mode"], g["sd"]), S, P, worst)
        _report("evaluation K=%d mode=%d free_sd=%d: lppd" % (g["K"], g["mode"], g["sd"]), S, P, worst_lppd)
        assert worst <= 1.0 and worst_lppd <= 1.0
        assert np.isfinite(rec["elpd_loo_pix"]).all() and np.isfinite(rec["khat"]).all() and np.isfinite(rec["elpd_loo"])
        np.testing.assert_array_equal(rec["p_loo_pix"], rec["lppd"] - rec["elpd_loo_pix"])


def test_pointwise_is_from_loglik_of_its_own_matrix_bit_for_bit(evaluated):
    groups, flat, wants = evaluated
    skips = [np.isnan(ll).all(axis=1).astype(np.uint8) for ll in flat["ll"]]
    assert [int(s.sum()) for s in skips] == [2, 2, 0]
    again = _from_loglik(flat["ll"], skips)
    for a, b in zip(_records(flat, [g["x"].size for g in groups]), again):
        _same(a, b)
    for a, b in zip(again, _from_loglik(flat["ll"], skips, device_input=True)):
        _same(a, b)


def test_lppd_and_counts_are_the_predictive_library_s_bit_for_bit(evaluated):
    """WAIC and PSIS-LOO rest on one l_sp: vamp_pred_pointwise on the same arguments, at the default scratch and at one
    column of the largest group (S = 129) per pass, returns the lppd, n_used and n_bad of the vamp_loo_pointwise call"""
    from vamp_amd import predictive
    groups, flat, _ = evaluated
    args = _pointwise_args(groups)
    for scratch in (0, 8 * 129):
        pred = predictive._call(0, *args, scratch_bytes=scratch)
        for k in ("lppd", "n_used", "n_bad"):
            assert pred[k].dtype == flat[k].dtype and np.array_equal(pred[k], flat[k], equal_nan=k not in ref.CNT), (k, scratch)


# ---- 4. no bit changes --------------------------------------------------------------------------------------------
def _run(groups, **kw):
    from vamp_amd.loo import pointwise_loo
    return pointwise_loo([g["x"] for g in groups], [g["flux"] for g in groups], [g["noise"] for g in groups],
                         [g["chain"] for g in groups], [g["K"] for g in groups], [g["mode"] for g in groups], **kw)


def _identical(a, b):
    for name in ref.FLAT:
        assert np.array_equal(np.asarray(getattr(a, name)), np.asarray(getattr(b, name)), equal_nan=name not in ref.CNT), name


def test_packing_and_group_order_do_not_change_a_bit(evaluated):
    """a scratch of exactly one column of the largest group (S = 129: each of its pixels is a pass of its own) against the
    default, every order of the three groups under a scratch of three such columns, and the same for vamp_loo_from_loglik"""
    groups, flat, _ = evaluated
    one = _run(groups)
    for rec, d in zip(one, _records(flat, [g["x"].size for g in groups])):
        _same({k: getattr(rec, k) for k in ref.FLAT}, d)
    for a, b in zip(one, _run(groups, scratch_bytes=8 * 129)):
        _identical(a, b)
    for order in itertools.permutations(range(3)):
        for i, rec in zip(order, _run([groups[i] for i in order], scratch_bytes=8 * 3 * 129)):
            _identical(rec, one[i])
    from vamp_amd._loo_lib import LooError
    with pytest.raises(LooError, match="less than one column"):
        _run(groups, scratch_bytes=8 * 129 - 1)
    mats = [ref.column_case(c)[0] for c in ref.COLUMN_CASES[3:6]]          # S = 65, 129, 225
    whole = _from_loglik(mats)
    for a, b in zip(whole, _from_loglik(mats, scratch_bytes=8 * 225)):
        _same(a, b)
    for order in itertools.permutations(range(3)):
        for i, rec in zip(order, _from_loglik([mats[i] for i in order], scratch_bytes=8 * 3 * 225)):
            _same(rec, whole[i])


def test_every_output_alone(evaluated):
    """each output with every other pointer NULL equals the full call's, the matrix included; the group sums are formed
    also when the per-pixel outputs are not asked for"""
    from vamp_amd import loo
    groups, full, _ = evaluated
    args = _pointwise_args(groups)
    for only in ref.FLAT:
        got = loo._call(0, *args, want=(only,))
        assert list(got) == [only] and got[only].dtype == full[only].dtype
        assert np.array_equal(got[only], full[only], equal_nan=only not in ref.CNT), only
    got = loo._call(0, *args, want=("ll",))
    assert list(got) == ["ll"]
    for a, b in zip(got["ll"], full["ll"]):
        np.testing.assert_array_equal(a, b)
    assert loo._call(0, *args, want=()) == {}
    mats = [ll for ll in full["ll"]]
    shape = ([m.shape[0] for m in mats], [m.shape[1] for m in mats])
    whole = loo._call_loglik(0, [m.ctypes.data for m in mats], *shape)
    for only in ref.FLAT:
        got = loo._call_loglik(0, [m.ctypes.data for m in mats], *shape, want=(only,))
        assert list(got) == [only] and np.array_equal(got[only], whole[only], equal_nan=only not in ref.CNT), only


def test_device_chain_of_three_regions_and_a_callers_stream():
    """the chain HipContext.run_dev wrote for three regions with free sd, read in place (ld = total_theta) through
    context_loo, against the same chain from the host; then the same device chain on a stream that is not the default"""
    import torch
    import vamp_amd
    from vamp_amd import _sidelib, loo
    rng = np.random.default_rng(68)
    groups = []
    for P, K in ((20, 1), (33, 2), (45, 3)):
        x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
        th0 = pref.draw_prior(rng, x, K, vo.MODE_GAUSS3, 1)[0]
        th0[2::3] += 0.5
        flux = np.exp(-pref.sample_taus(x, th0[None], K, vo.MODE_GAUSS3)[0].sum(axis=0)) + 0.05 * rng.standard_normal(P)
        chain = pref.ball(rng, np.append(th0, 0.05), 16).reshape(1, 16, -1)
        chain[:, :, 2:-1:3] = np.minimum(chain[:, :, 2:-1:3], 0.4 * (P - 1))       # the start lies inside the prior
        groups.append({"x": x, "flux": flux, "noise": None, "chain": chain, "K": K, "mode": vo.MODE_GAUSS3, "sd": True})
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
        recs = loo.context_loo(ctx, chain_t.data_ptr(), n_keep, xs, fs, [None] * 3)
        bases, total = _sidelib.region_bases(ctx, chain_t.data_ptr()), ctx.total_theta
        host = chain_t.cpu().numpy()
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        assert stream.cuda_stream != 0
        on_stream = loo._call(0, xs, fs, [None] * 3, [g["K"] for g in groups], [0] * 3, [1] * 3, bases, True, [total] * 3, [n_keep] * 3,
                              [W] * 3, stream=stream.cuda_stream)
    assert len(recs) == 3
    off = 0
    for g, rec in zip(groups, recs):
        D = g["chain"].shape[2]
        g["chain"] = host[:, off:off + W * D].reshape(n_keep, W, D).copy()
        off += W * D
        assert rec.n_used + rec.n_bad == n_keep * W and rec.elpd is rec.elpd_loo_pix and rec.looic == -2.0 * rec.elpd_loo
    assert not any(np.array_equal(g["chain"][0], g["chain"][-1]) for g in groups)          # the walkers moved
    for g, rec, h in zip(groups, recs, _run(groups)):
        _identical(rec, h)
        w = _want(g)
        assert (rec.n_used, rec.n_bad) == (w["n_used"], w["n_bad"])
        assert np.all(np.abs(rec.lppd - w["lppd"]) <= predictive_ref.bars(w)["lppd"])
    for rec, s in zip(recs, loo._split(on_stream, [x.size for x in xs], [1] * 3)):
        _identical(rec, s)


# ---- 5. the edge rules on the device ------------------------------------------------------------------------------
def test_edge_rules_on_the_device():
    """a constant column, 190 tied largest ratios, x_q = 0, an ordinary column; NaN, -inf and +inf entries; one sample;
    a matrix whose samples are all skipped between two ordinary ones"""
    rng = np.random.default_rng(2)
    ties = rng.normal(-1.0, 0.3, (200, 4))
    ties[:, 0] = -0.7
    ties[:, 1] = np.where(np.arange(200) < 190, -2.0, -0.5)
    order = np.argsort(ties[:, 2])
    ties[order[30:41], 2] = ties[order[40], 2]
    bad = np.random.default_rng(3).normal(-1.0, 0.3, (50, 4))
    bad[7, 1] = np.nan
    bad[9, 2] = -np.inf
    bad[11, 3] = np.inf
    one = np.array([[-1.5, -0.25]])
    mats = [ties, bad, one, ties[:, ::-1].copy(), bad[:, :1].copy()]
    skips = [None, None, None, np.ones(200, dtype=np.uint8), None]
    got = _from_loglik(mats, skips)
    for label, g, m, s in zip(("ties", "NaN and +-inf entries", "one sample", "every sample skipped", "after the skipped group"), got, mats, skips):
        _report("edge rules: " + label, m.shape[0], m.shape[1], ref.check(g, ref.from_loglik(m, s), label))
    assert np.isposinf(got[0]["khat"][:3]).all() and np.isfinite(got[0]["khat"][3]) and np.isfinite(got[0]["elpd_loo_pix"]).all()
    assert got[0]["n_high_k"] == 3 + int(got[0]["khat"][3] > 0.7)
    for k in ("elpd_loo_pix", "p_loo_pix", "khat"):
        assert np.isfinite(got[1][k][0]) and np.isnan(got[1][k][1:]).all(), k
    assert np.isnan(got[1]["lppd"][1]) and np.isfinite(got[1]["lppd"][2]) and np.isnan(got[1]["elpd_loo"]) and got[1]["n_high_k"] == 0
    assert np.array_equal(got[2]["elpd_loo_pix"], one[0]) and np.isposinf(got[2]["khat"]).all()
    assert (got[3]["n_used"], got[3]["n_bad"], got[3]["n_high_k"]) == (0, 200, 0)
    for k in ref.PIX + ref.GRP:
        assert np.isnan(got[3][k]).all(), k
    assert np.isfinite(got[4]["elpd_loo"]) and np.isnan(got[4]["elpd_loo_se"])          # one pixel: no standard error


def test_all_bad_group_inside_a_batch_of_good_ones(evaluated):
    groups, flat, _ = evaluated
    dead = {**groups[0], "chain": groups[0]["chain"].copy()}
    dead["chain"][:, :, 3] = 0.0                       # G <= 0 in every sample
    recs = _run([groups[1], dead, groups[2]])
    alone = _records(flat, [g["x"].size for g in groups])
    for rec, d in ((recs[0], alone[1]), (recs[2], alone[2])):
        _same({k: getattr(rec, k) for k in ref.FLAT}, d)
    r = recs[1]
    assert (r.n_used, r.n_bad, r.n_high_k) == (0, 129, 0) and np.isnan(r.elpd_loo) and np.isnan(r.elpd_loo_se) and np.isnan(r.p_loo)
    for k in ref.PIX:
        assert np.isnan(getattr(r, k)).all(), k


# ---- 6. the ladder ------------------------------------------------------------------------------------------------
def _ladder(lines):
    from vamp_amd import predictive
    from vamp_amd.vpregion import VPregion
    x, flux, noise = evidence_ref.gauss_line_data(32, lines, 0.1, 4)
    reg = VPregion(1.0e3 + x, flux, noise, seed=12, nwalkers=32)
    assert reg.n == 1
    reg.region_fit(verbose=False, iterations=300, thin=5, burn=100, criterion='loo')
    for n in sorted(reg.loo)[:-1]:
        rise, se = predictive.compare(reg.loo[n], reg.loo[n + 1])
        print("loo ladder of %d-line data: n = %d -> %d elpd_loo rises by %.3f, paired standard error %.3f; khat > 0.7 on %d and %d of %d pixels"
              % (len(lines), n, n + 1, rise, se, reg.loo[n].n_high_k, reg.loo[n + 1].n_high_k, len(reg.loo[n].khat)))
    assert reg.fit._n == reg.n and reg.fit.loo is reg.loo[reg.n] and sorted(reg.loo) == list(range(1, reg.n + 2))
    assert len(reg.fit.bic_array) == 3 and not hasattr(reg, "predictive")
    return reg


def test_region_fit_by_loo_finds_two_lines():
    assert _ladder([(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)]).n == 2


def test_region_fit_by_loo_keeps_one_line():
    assert _ladder([(1.2, 9.0, 2.0)]).n == 1


# ---- 7. the command line ------------------------------------------------------------------------------------------
def test_do_vamp_loo_writes_the_file(tmp_path):
    from vamp_amd import h5min
    out = tmp_path / "out"
    spec = tmp_path / "spectrum_4.h5"
    shutil.copy(os.path.join(GOLDEN, "simba_H1215.h5"), spec)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    rc = subprocess.run([sys.executable, "-m", "vamp_amd.do_vamp", str(spec), "1215.6701", "--output_folder", str(out),
                         "--conv_attempts", "1", "--walkers", "32", "--iterations", "300", "--burn", "100", "--thin", "5",
                         "--seed", "3", "--loo"], env=env, capture_output=True, text=True, timeout=900)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [ln for ln in rc.stdout.splitlines() if ln.startswith("vamp_perf ")]
    assert len(lines) == 1
    rec = json.loads(lines[0][len("vamp_perf "):])
    assert 0.0 <= rec["loo_seconds"] < rec["seconds"] + 60 and "predictive_seconds" not in rec
    path = out / "spectrum_4_gauss_loo.h5"
    assert path.exists() and not (out / "spectrum_4_gauss_predictive.h5").exists()
    got = h5min.read(str(path))
    nreg = rec["regions"]
    assert set(got) == {"elpd_loo_pix", "p_loo_pix", "khat", "lppd", "elpd_loo", "elpd_loo_se", "p_loo", "looic", "n_high_k", "n_used",
                        "n_bad", "n_comp", "time_step"}
    assert got["elpd_loo"].shape == (nreg,) and got["n_comp"].sum() == rec["lines"] and np.all(got["n_used"] > 0)
    np.testing.assert_array_equal(got["looic"], -2.0 * got["elpd_loo"])
    inside = np.isfinite(got["lppd"])
    assert 0 < inside.sum() <= rec["pixels_in_regions"]                                            # (regions may overlap)
    assert np.array_equal(inside, np.isfinite(got["elpd_loo_pix"])) and not np.isnan(got["khat"][inside]).any()
    assert np.all(np.isfinite(got["elpd_loo"])) and np.all(got["elpd_loo_se"] > 0) and np.all(got["n_high_k"] >= 0)
