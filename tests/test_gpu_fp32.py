"""GPU tests (-m gpu) of the fp32 / Humlicek-W4 context (BASELINE.json config 5) held to the fp64 path's coverage,
and of the "class_streams" switch in both dtypes.

Stated tolerance against the fp64 oracle, per (region, walker):
  |delta chi^2| / chi^2 <= 1e-3, median over a case <= 1e-4, |delta lnprob| <= 1e-3 max(1, |lnprob|),
  identical finite / -inf pattern.
Exact wherever both sides run the same arithmetic:
  - lnprob_all == lnprob region by region; model, model_all and line_records of an fp32 context == an fp64 one
    (k_model and k_line_records have no fp32 instantiation);
  - the sampler's trajectory == the oracle's stretch move driven by a second fp32 context's lnprob (_movers_fn: the
    proposals take the shape of the device's movers): chain to 1e-10, n_accept equal, lnprob chain to 1e-9;
  - the resident step loop, the device MAP search and resume / thin: the fp64 tests' bit-for-bit checks;
  - class_streams 1 == 0 bit for bit.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import vamp_oracle as vo
import test_gpu_parity as tp
from test_gpu_parity import _case, _mixed_short_context

pytestmark = pytest.mark.gpu

CHI_MAX, CHI_MEDIAN, LNP_MAX = 1e-3, 1e-4, 1e-3
NARROW_PX = 1e-3          # fp32 cannot resolve a Gaussian width of ~1e-6 px (test_fp32_humlicek_path)


@pytest.fixture(scope="module", params=[0, 64, 16, 256, 65], ids=["pack-auto", "pack-64", "pack-16", "pack-256", "pack-64t"])
def hip_ctx32(request):
    """fp32 / Humlicek-W4 context on device 0, once per walker packing (the packings of conftest.hip_ctx)."""
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=vamp_amd.F32)
    ctx.set_packing(request.param)
    ctx.packing_request = request.param
    yield ctx
    ctx.close()


def _twin(ctx, dtype_name="F32"):
    """a second context of the given dtype with ctx's packing (set_regions still to be called)"""
    import vamp_amd
    t = vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype_name))
    t.set_packing(ctx.packing_request)
    return t


def _set_case(ctx, x, f, n, K, mode, sd, nbz):
    ctx.set_regions(x, f, n, K, mode=mode, sample_sd=sd, nbz=None if nbz is None else nbz[None, :])


def _oracle_region(x, f, n, K, mode, sd, nbz):
    r = vo.Region(x=x, flux=f, noise=n, n_comp=K, mode=mode, sample_sd=sd)
    if nbz is not None:
        r.l_fixed, r.line, r.x_origin, r.x_scale = [float(v) for v in nbz]
    return r


def _narrow(r, th, x):
    """walkers with a line of Gaussian width <= NARROW_PX pixels (FWHM for Voigt / (N, b, z), sigma for Gaussians)"""
    px = np.median(np.abs(np.diff(x)))
    out = np.zeros(th.shape[0], dtype=bool)
    for w in range(th.shape[0]):
        if not np.all(np.isfinite(th[w])):
            continue
        with np.errstate(all="ignore"):
            comps = vo.native_components(r, th[w])
        out[w] = any(abs(c[-1] if r.mode != vo.MODE_GAUSS3 else c[2]) <= NARROW_PX * px for c in comps)
    return out


def _check_fp32(name, got, chi, want, wchi, keep):
    """the stated fp32 tolerance on the walkers `keep` (finite in the oracle); returns the worst chi^2 error"""
    rel = np.abs(chi[keep] - wchi[keep]) / wchi[keep]
    err = np.abs(got[keep] - want[keep]) / np.maximum(1.0, np.abs(want[keep]))
    assert rel.max() <= CHI_MAX and np.median(rel) <= CHI_MEDIAN, (name, rel.max(), np.median(rel))
    assert err.max() <= LNP_MAX, (name, err.max())
    return rel.max()


def test_fp32_every_golden_case_against_oracle(hip_ctx32):
    """All 25 cases of lnprob_cases.npz (every mode, free sd, raw-Hz coordinates, (N, b, z)) through the fp32 path
    against the fp64 oracle: identical -inf pattern on every walker; the stated tolerance on every finite walker but
    those with a line whose Gaussian width is at most 1e-3 px: the edge walker 5 of random_thetas (1e-6 of the prior's
    width) and, in the raw-Hz case, walker 11, whose second line has G = 3.7e-4 px."""
    g = load_golden("lnprob_cases.npz")
    assert len(g["cases"]) == 25
    worst, failed = {}, {}
    for name in g["cases"]:                 # every case is checked; the failing ones are reported together
        name = str(name)
        x, f, n, K, mode, sd, nbz = _case(g, name)
        _set_case(hip_ctx32, x, f, n, K, mode, sd, nbz)
        th = g[name + "_theta"]
        got, chi = hip_ctx32.lnprob(th, return_chi2=True)
        want, wchi = g[name + "_lnprob"], g[name + "_chi2"]
        fin = np.isfinite(want)
        narrow = _narrow(_oracle_region(x, f, n, K, mode, sd, nbz), th, x)
        assert (fin & narrow).sum() <= 2, (name, np.flatnonzero(fin & narrow))
        try:
            assert np.array_equal(fin, np.isfinite(got)), "finite / -inf pattern differs"
            assert np.all(got[~fin] == -np.inf), "a non-finite lnprob that is not -inf"
            worst[name] = _check_fp32(name, got, chi, want, wchi, fin & ~narrow)
        except AssertionError as e:
            failed[name] = str(e).split("\n")[0]
    assert not failed, "failing cases: " + "; ".join(f"{k}: {v}" for k, v in failed.items())
    print("fp32 golden sweep (packing %d): worst chi^2 error per case: %s" % (
        hip_ctx32.packing_request, ", ".join("%s %.1e" % kv for kv in worst.items())))


def test_fp32_include_norm_and_bounds(hip_ctx32):
    """test_lnprob_include_norm_and_bounds in fp32: the prior's normalisation and per-region bounds."""
    g = load_golden("lnprob_cases.npz")
    name = "H1215_r1_K4_m1_sd0"
    x, f, n, K, mode, sd, _ = _case(g, name)
    th = g[name + "_theta"]
    bounds = np.array([[x[2], x[-3], 5.0, 9.0]])
    hip_ctx32.set_regions(x, f, n, K, mode=mode, include_norm=True, bounds=bounds)
    r = vo.Region(x=x, flux=f, noise=n, n_comp=K, mode=mode, include_norm=True, c_lo=x[2], c_hi=x[-3], sigma_max=5.0, fwhm_max=9.0)
    want, wchi = vo.log_prob_batch(r, th, return_chi2=True)
    got, chi = hip_ctx32.lnprob(th, return_chi2=True)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    keep = fin & ~_narrow(r, th, x)
    assert keep.sum() >= 1
    _check_fp32(name, got, chi, want, wchi, keep)


def test_fp32_lnprob_all_equals_lnprob_region_by_region(hip_ctx32):
    """A ragged batch of seven regions: lnprob_all == lnprob of each region bit for bit (lnprob and chi^2), and both
    against the oracle within the stated tolerance."""
    g = load_golden("lnprob_cases.npz")
    names = [f"H1215_r{i}_K4_m1_sd0" for i in range(3)] + [f"CII1036_r{i}_K4_m1_sd0" for i in range(4)]
    xs, fs, ns = [g[n + "_x"] for n in names], [g[n + "_flux"] for n in names], [g[n + "_noise"] for n in names]
    hip_ctx32.set_regions(xs, fs, ns, 4, mode=vo.MODE_VOIGT4)
    thetas = [g[n + "_theta"] for n in names]
    la, ca = hip_ctx32.lnprob_all(thetas, return_chi2=True)
    for r, name in enumerate(names):
        l1, c1 = hip_ctx32.lnprob(thetas[r], region=r, return_chi2=True)
        assert np.array_equal(la[r], l1) and np.array_equal(ca[r], c1, equal_nan=True), name
        want, wchi = g[name + "_lnprob"], g[name + "_chi2"]
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(l1)), name
        reg = vo.Region(x=xs[r], flux=fs[r], noise=ns[r], n_comp=4, mode=vo.MODE_VOIGT4)
        _check_fp32(name, l1, c1, want, wchi, fin & ~_narrow(reg, thetas[r], xs[r]))


def test_fp32_context_models_and_records_equal_fp64(hip_ctx32):
    """k_model and k_line_records have no fp32 instantiation: model, model_all and line_records of an fp32 context
    are those of an fp64 context bit for bit, on every golden case and every walker."""
    g = load_golden("lnprob_cases.npz")
    ref = _twin(hip_ctx32, "F64")
    try:
        for name in g["cases"]:
            name = str(name)
            x, f, n, K, mode, sd, nbz = _case(g, name)
            _set_case(hip_ctx32, x, f, n, K, mode, sd, nbz)
            _set_case(ref, x, f, n, K, mode, sd, nbz)
            th = g[name + "_theta"]
            t32, f32 = hip_ctx32.model(th[0])
            t64, f64 = ref.model(th[0])
            assert np.array_equal(t32, t64) and np.array_equal(f32, f64), name
            for w in range(th.shape[0]):
                r32, lp32 = hip_ctx32.line_records(th[w])
                r64, lp64 = ref.line_records(th[w])
                assert np.array_equal(r32, r64, equal_nan=True) and np.array_equal(lp32, lp64, equal_nan=True), (name, w)
        names = [f"H1215_r{i}_K4_m1_sd0" for i in range(3)] + ["H1215_r0_K1_m1_sd0"]
        xs, fs, ns = [g[n + "_x"] for n in names], [g[n + "_flux"] for n in names], [g[n + "_noise"] for n in names]
        ks = [4, 4, 4, 1]
        thetas = [g[n + "_theta"][0] for n in names]
        out = []
        for c in (hip_ctx32, ref):
            c.set_regions(xs, fs, ns, ks, mode=vo.MODE_VOIGT4)
            out.append(c.model_all(thetas))
        for r in range(4):
            assert np.array_equal(out[0][0][r], out[1][0][r]) and np.array_equal(out[0][1][r], out[1][1][r]), r
    finally:
        ref.close()


def _movers_fn(ev, region=0):
    """lnprob of a half-step's W/2 proposals by the context `ev`, in the shape the device evaluates its W/2 movers in.
    vamp_lnprob runs W points of a region as the W/2 movers of a W-walker ensemble (launch_lnprob), so the proposals go
    in twice: W/2 points alone would run as an ensemble of W/2 walkers, which at W >= 32 768 is a different shape."""
    return lambda q: ev.lnprob(np.concatenate([q, q]), region=region)[:len(q)]


def _check_trajectory(res_chain, res_lnp, res_nacc, chain, lchain, nacc, tag):
    assert np.array_equal(res_nacc, nacc), tag
    assert np.allclose(res_chain, chain, rtol=1e-10, atol=1e-12), tag
    assert np.allclose(res_lnp, lchain, rtol=1e-9, atol=0), tag


@pytest.mark.parametrize("block", [8, 16])
def test_fp32_stretch_philox_trajectory(hip_ctx32, block):
    """k_half_step<true, ..> on stretch_traj.npz: 12 steps against the oracle's stretch move (the same counter-based
    draws) evaluating its proposals with a second fp32 context."""
    g = load_golden("stretch_traj.npz")
    ev = _twin(hip_ctx32)
    try:
        for c in (hip_ctx32, ev):
            c.set_regions(g["x"], g["flux"], g["noise"], 1, mode=vo.MODE_VOIGT4)
        seed = 0x1234ABCD5678EF01
        hip_ctx32.sampler_init(g["X0"], seed=seed, a=2.0, split_block=block)
        res = hip_ctx32.run(12)
        lnp0 = ev.lnprob(g["X0"])
        assert np.array_equal(hip_ctx32.lnprob(g["X0"]), lnp0)
        chain, lchain, nacc = vo.run_sampler_batch(_movers_fn(ev), g["X0"], lnp0, 12, seed=seed, block=block)
        _check_trajectory(res["chain"], res["lnprob"], res["n_accept"], chain, lchain, nacc, block)
        assert nacc.sum() > 0
    finally:
        ev.close()


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_fp32_mixed_context_trajectory(hip_ctx32, variant):
    """A mixed multi-region context (every launch class; Voigt, Gaussian, Voigt + free sd, (N, b, z)): four sampler
    steps of every region against the oracle's stretch move on a second fp32 context's lnprob."""
    rng = np.random.default_rng(140 + variant)
    W = 32
    xs, fs, ns, Ks, ths, kw = _mixed_short_context(rng, variant, W, with_xl=hip_ctx32.packing_request not in (16, 65))
    ev = _twin(hip_ctx32)
    try:
        for c in (hip_ctx32, ev):
            c.set_regions(xs, fs, ns, Ks, **kw)
        hip_ctx32.sampler_init(ths, seed=606, split_block=8)
        res = hip_ctx32.run(4)
        total = 0
        for r in range(len(xs)):
            fn = _movers_fn(ev, r)
            chain, lchain, nacc = vo.run_sampler_batch(fn, ths[r], ev.lnprob(ths[r], region=r), 4, seed=606, block=8, region=r,
                                                       walker_off=r * W)
            _check_trajectory(res["chain"][r], res["lnprob"][r], res["n_accept"][r], chain, lchain, nacc, (variant, r))
            total += nacc.sum()
        assert total > 0
    finally:
        ev.close()


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("W", [32, 70])
def test_fp32_resident_step_loop_equals_launch_per_half_step(hip_ctx32, variant, W):
    """k_run_resident<true, ..> against one launch per half-step: test_resident_step_loop_equals_launch_per_half_step
    (bit for bit) on the fp32 context."""
    tp.test_resident_step_loop_equals_launch_per_half_step(hip_ctx32, variant, W)


@pytest.mark.parametrize("mode,sd", [(vo.MODE_GAUSS3, True), (vo.MODE_VOIGT4, True), (vo.MODE_VOIGT4, False)])
def test_fp32_map_search_on_device_equals_host_driven(hip_ctx32, mode, sd):
    """k_map_search<true, ..> against the host-driven search: test_map_search_on_device_equals_host_driven
    (bit for bit) on the fp32 context."""
    tp.test_map_search_on_device_equals_host_driven(hip_ctx32, mode, sd)


def test_fp32_sampler_resume_and_thin(hip_ctx32):
    """run(12) == run(5) + run(7), thinning, get/set_state: test_sampler_resume_and_thin on the fp32 context."""
    tp.test_sampler_resume_and_thin(hip_ctx32)


def _class_streams_pair(ctx, run, option_resident):
    """run(ctx) with class_streams 1 and 0 (resident option fixed); returns both results"""
    out = {}
    try:
        ctx.set_option("resident", option_resident)
        for cs in (1, 0):
            ctx.set_option("class_streams", cs)
            out[cs] = run(ctx)
    finally:
        ctx.set_option("class_streams", 1)
        ctx.set_option("resident", 1)
    return out[1], out[0]


def _assert_same_runs(a, b):
    (ca, la, na, sa), (cb, lb, nb, sb) = a, b
    assert np.array_equal(ca, cb) and np.array_equal(la, lb) and np.array_equal(na, nb)
    assert sa[3] == sb[3]
    for r in range(len(sa[0])):
        assert np.array_equal(sa[0][r], sb[0][r]) and np.array_equal(sa[1][r], sb[1][r]) and np.array_equal(sa[2][r], sb[2][r]), r


@pytest.mark.parametrize("dtype", ["F64", "F32"])
def test_class_streams_equal_sequential_classes(dtype):
    """launch_half forks the launch classes of a half-step onto separate streams, each class with its own slice of the
    draw buffers, when a context has several classes and >= 4 PACK_MIN_WALKERS movers: all 421 q1422 regions at
    W = 320 (134 720 walkers).  Chain, lnprob chain, acceptance counts and final state with the classes forked
    == with the classes in sequence, bit for bit."""
    import vamp_amd
    from tools.bench_c3 import build_regions, start_walkers
    xs, fs, ns, ks = build_regions()
    W = 320
    rng = np.random.default_rng(320)
    th = [start_walkers(rng, x, k, W) for x, k in zip(xs, ks)]
    with vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype)) as ctx:
        ctx.set_regions(xs, fs, ns, ks, mode=vamp_amd.MODE_VOIGT4)
        kinds, ncls = ctx.region_classes()
        assert ncls > 1, (ncls, sorted(set(kinds)))
        assert len(xs) * W // 2 >= 4 * 16384          # PACK_MIN_WALKERS * 4: launch_half forks

        def run(c):
            c.sampler_init(th, seed=4210, split_block=32)
            ch, lc, na, _ = c.run_flat(3)
            return ch, lc, na, c.get_state()

        forked, sequential = _class_streams_pair(ctx, run, 0)
    _assert_same_runs(forked, sequential)
    assert forked[2].sum() > 0


@pytest.mark.parametrize("dtype", ["F64", "F32"])
def test_class_streams_equal_sequential_classes_resident(dtype):
    """run_resident forks its launch classes on any context of more than one class: a small ensemble (W = 32) of the
    mixed context -- short regions, blends with per-walker tables, a region of 18 lines -- through the resident loop
    with the classes forked == in sequence, bit for bit."""
    import vamp_amd
    rng = np.random.default_rng(77)
    W = 32
    xs, fs, ns, Ks, ths, kw = _mixed_short_context(rng, 0, W, with_xl=True)
    with vamp_amd.HipContext(device=0, dtype=getattr(vamp_amd, dtype)) as ctx:
        ctx.set_regions(xs, fs, ns, Ks, **kw)
        kinds, ncls = ctx.region_classes()
        # a small ensemble merges the short-region classes (0, 3) into one; blends (1) and > 16 lines (4) stay apart
        assert {0, 3} & set(kinds) and {1, 4} <= set(kinds), kinds

        def run(c):
            c.sampler_init(ths, seed=91, split_block=W)
            ch, lc, na, _ = c.run_flat(6, thin=2)
            return ch, lc, na, c.get_state()

        forked, sequential = _class_streams_pair(ctx, run, 2)
    _assert_same_runs(forked, sequential)
    assert forked[2].sum() > 0
