"""GPU tests of libvamp_post.so where it changes path (cases and restated LDS arithmetic: tests/side_limit_cases.py; CPU
controls: tests/test_side_limits.py): k_post_eval above 64 KiB of dynamic LDS and just under, 16-lane groups in a pass
whose LDS stride is a K = 32 neighbour's, the narrow-form corner, the pixel rounds and the workgroup's 64-sample border,
the evaluator's regimes, a NaN among a column's values, NULL outputs, a caller's stream with device-resident groups, and
one column per pass.  Compared with tests/posterior_ref.py through _same of tests/test_gpu_posterior.py: the bars are
its derived ones, 1e-12 for flux statistics and 1e-12 P |width| for equivalent widths."""
import ctypes as C

import numpy as np
import pytest

import posterior_ref as ref
import side_limit_cases as sc
from oracle import vamp_oracle as vo
from test_gpu_posterior import PROBS, _identical, _same

pytestmark = pytest.mark.gpu

assert PROBS == sc.PROBS


def _groups(cases, seed):
    rng = np.random.default_rng(seed)
    return [sc.drawn_group(rng, P, K, mode, N, W, sd) + (K, mode, sd) for mode, K, P, N, W, sd in cases]


def _run(groups, width=0.3, **kw):
    from vamp_amd.posterior import posterior_summaries
    return posterior_summaries([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups], [g[3] for g in groups],
                               [g[4] for g in groups], probs=PROBS, pixel_width=width, **kw)


def _check(groups, got, width=0.3, tag=""):
    for (x, c, K, mode, sd), g in zip(groups, got):
        want = ref.summaries(x, c, K, mode, bool(sd), PROBS, width)
        _same(g, want, x.size, width, "%s mode=%d K=%d P=%d S=%d sd=%d" % (tag, mode, K, x.size, c.shape[0] * c.shape[1], sd))
        assert g.n_bad == 0


def test_eval_above_64_kib_of_lds_with_narrow_groups_in_the_pass():
    """K = 32 (119 840 B) at P = 2, 64, 65, 129 and K = 18 (68 320 B) at S = 64, 65, 129 in both modes, with two 16-lane
    groups between the K = 32 ones: the launch's LDS is the largest item's, so the narrow groups run at its stride and must
    give the bits they give alone.  Then the big call again after the small one, bit for bit: whichever of them is the
    process's first call, the raised limit holds for the other"""
    lds = [sc.post_eval_lds_bytes(K, P) for _, K, P, *_ in sc.BIG_LDS]
    assert max(lds) == 119840 == sc.EVAL_MAX_LDS and {b for b, c in zip(lds, sc.BIG_LDS) if c[1] == 18} == {68320}
    assert sum(b > sc.DEFAULT_LDS for b in lds) == len(lds) - 2      # all but the two narrow groups need the raised limit
    groups = _groups(sc.BIG_LDS, 51)
    big = _run(groups)
    _check(groups, big, tag="big-lds")
    narrow = [groups[i] for i in sc.BIG_LDS_NARROW]
    assert max(sc.post_eval_lds_bytes(g[2], g[0].size) for g in narrow) < sc.DEFAULT_LDS
    alone = _run(narrow)
    for i, a in zip(sc.BIG_LDS_NARROW, alone):
        _identical(big[i], a)
    for a, b in zip(big, _run(groups)):
        _identical(a, b)


def test_eval_just_under_64_kib():
    mode, K, P, N, W, sd = sc.JUST_UNDER
    assert sc.post_eval_lds_bytes(K, P) == 64640 < sc.DEFAULT_LDS < sc.post_eval_lds_bytes(K + 1, P)
    groups = _groups([sc.JUST_UNDER], 52)
    _check(groups, _run(groups), tag="just-under")


def test_narrow_corner():
    """(P, K) in {32, 33} x {4, 5}: only (32, 4) takes 16 lanes.  S = 17 and 20: a second round of one sample, or of four"""
    assert [sc.group_lanes(K, P) for _, K, P, *_ in sc.NARROW_CORNER[:4]] == [16, 64, 64, 64]
    groups = _groups(sc.NARROW_CORNER, 53)
    got = _run(groups)
    _check(groups, got, tag="narrow-corner")
    for i, (mode, K, P, N, W, sd) in enumerate(sc.NARROW_CORNER):
        if (P, K) == (32, 4):
            _identical(got[i], _run([groups[i]])[0])


def test_evaluator_regimes():
    """G in {1e-3 .. 300} x L / G in {0, 1e-12 .. 1e3} x A in {0.5, 50}, one Voigt line per group of one sample, then the
    same lines in pairs: k_post_eval's own copy of the evaluation through every regime of the evaluator"""
    from vamp_amd.posterior import posterior_summaries
    groups = sc.regime_groups()
    got = posterior_summaries([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups], vo.MODE_VOIGT4, probs=PROBS)
    worst = 0.0
    for (x, c, K), g in zip(groups, got):
        want = ref.summaries(x, c, K, vo.MODE_VOIGT4, probs=PROBS)
        assert (g.n_used, g.n_bad) == (1, 0)
        assert np.array_equal(g.flux_q[0], g.flux_mean) and np.array_equal(g.flux_q[-1], g.flux_mean) and np.all(g.flux_sd == 0)
        worst = max(worst, float(np.max(np.abs(g.flux_mean - want["flux_mean"]))))
        _same(g, want, x.size, 1.0, "regime " + " ".join("%g" % v for v in c.ravel()))
    print("regime sweep: worst flux error", worst)


def test_a_nan_among_the_values_of_a_column():
    """a good sample whose flux is NaN makes every statistic of the flux and of the region's equivalent width NaN, as in
    numpy; its lines' sums are finite and -inf (times the width), and there the library follows numpy as well, down to the
    NaN of a quantile that lands on the infinite order statistic (p = 0, and p = 1 under a negative width)"""
    from vamp_amd.posterior import posterior_summaries
    cases = [sc.nan_flux_group(w) for w in (0.5, -0.5)]
    rng = np.random.default_rng(54)
    x0, c0 = sc.drawn_group(rng, 9, 2, vo.MODE_VOIGT4, 3, 7)               # an ordinary neighbour
    got = posterior_summaries([c[0] for c in cases] + [x0], [c[1] for c in cases] + [c0], 2, vo.MODE_VOIGT4, probs=PROBS,
                              pixel_width=[c[2] for c in cases] + [0.5])
    for (x, chain, w), g in zip(cases, got):
        with np.errstate(all="ignore"):
            want = ref.summaries(x, chain, 2, vo.MODE_VOIGT4, probs=PROBS, pixel_width=w)
        assert (g.n_used, g.n_bad) == (21, 0) and np.isnan(g.flux_q).all() and np.isnan(g.ew_mean) and np.isnan(g.ew_q).all()
        assert np.isinf(g.comp_ew_mean[1]) and np.isnan(g.comp_ew_sd[1]) and np.isnan(g.comp_ew_q[1][0 if w > 0 else -1])
        _same(g, want, x.size, w, "nan-flux width=%g" % w)
    _same(got[2], ref.summaries(x0, c0, 2, vo.MODE_VOIGT4, probs=PROBS, pixel_width=0.5), 9, 0.5, "nan-flux neighbour")


def _call_some(xs, n_comp, modes, sample_sd, chains, widths, only):
    """posterior._call for host chains with every output pointer NULL but ``only``; returns that output"""
    from vamp_amd import _post_lib
    from vamp_amd.posterior import _FLAT
    lib = _post_lib.load()
    G, Q = len(chains), len(PROBS)
    probs = np.asarray(PROBS, dtype=np.float64)
    tp, tk = int(sum(x.size for x in xs)), int(np.sum(n_comp))
    shape = {"flux_mean": tp, "flux_sd": tp, "flux_q": tp * Q, "ew_mean": G, "ew_sd": G, "ew_q": (G, Q), "comp_ew_mean": tk,
             "comp_ew_sd": tk, "comp_ew_q": (tk, Q), "n_used": G, "n_bad": G}
    out = np.full(shape[only], -7, dtype=np.int32 if only in ("n_used", "n_bad") else np.float64)
    xp = (C.c_void_p * G)(*[x.ctypes.data for x in xs])
    bp = (C.c_void_p * G)(*[c.ctypes.data for c in chains])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    n_pix, n_comp, modes, sample_sd = i32([x.size for x in xs]), i32(n_comp), i32(modes), i32(sample_sd)
    n_keep, walkers = i32([c.shape[0] for c in chains]), i32([c.shape[1] for c in chains])
    ld = np.ascontiguousarray([c.shape[1] * c.shape[2] for c in chains], dtype=np.int64)
    widths = np.ascontiguousarray(widths, dtype=np.float64)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    args = [out.ctypes.data_as(ip if k in ("n_used", "n_bad") else dp) if k == only else None for k in _FLAT]
    _post_lib.check(lib.vamp_post_summaries(
        0, C.c_void_p(0), G, xp, n_pix.ctypes.data_as(ip), n_comp.ctypes.data_as(ip), modes.ctypes.data_as(ip),
        sample_sd.ctypes.data_as(ip), bp, 0, ld.ctypes.data_as(C.POINTER(C.c_int64)), n_keep.ctypes.data_as(ip),
        walkers.ctypes.data_as(ip), widths.ctypes.data_as(dp), Q, probs.ctypes.data_as(dp), 0, *args), lib)
    return out


FRAME_CASES = [(1, 2, 20, 3, 7, 1), (0, 5, 33, 2, 9, 0), (1, 3, 70, 5, 13, 0)]       # three groups, ragged in everything


@pytest.mark.parametrize("only", ref.FLAT)
def test_every_output_but_one_null(only):
    """the header lets any output pointer be NULL: the one that is fetched equals the full call's bit for bit"""
    from vamp_amd import posterior
    groups = _groups(FRAME_CASES, 55)
    xs, chains = [g[0] for g in groups], [np.ascontiguousarray(g[1]) for g in groups]
    ks, modes, sds = [g[2] for g in groups], [g[3] for g in groups], [g[4] for g in groups]
    widths = [0.2, 0.3, 0.4]
    full = posterior._call(0, xs, ks, modes, sds, [c.ctypes.data for c in chains], False, [c.shape[1] * c.shape[2] for c in chains],
                           [c.shape[0] for c in chains], [c.shape[1] for c in chains], widths, np.asarray(PROBS))
    got = _call_some(xs, ks, modes, sds, chains, widths, only)
    assert got.shape == full[only].shape and np.array_equal(got, full[only], equal_nan=False), only


def test_callers_stream_and_three_device_resident_groups():
    """three groups in separate device tensors with rows longer than W D, one with the free sd, on a stream that is not the
    default one: every output equals the host-chain call's bit for bit"""
    import torch
    from vamp_amd import posterior
    groups = _groups(FRAME_CASES, 56)
    dev = torch.device("cuda", 0)
    probs = np.asarray(PROBS)
    xs, ks, modes, sds = [g[0] for g in groups], [g[2] for g in groups], [g[3] for g in groups], [g[4] for g in groups]
    widths = [0.2, 0.3, 0.4]
    raws, lds = [], []
    for i, g in enumerate(groups):
        N, W, D = g[1].shape
        ld = W * D + 3 + 2 * i
        raw = np.full((N, ld), np.nan)
        raw[:, :W * D] = g[1].reshape(N, W * D)
        raws.append(raw); lds.append(ld)
    ns, ws = [g[1].shape[0] for g in groups], [g[1].shape[1] for g in groups]
    host = posterior._call(0, xs, ks, modes, sds, [r.ctypes.data for r in raws], False, lds, ns, ws, widths, probs)
    tens = [torch.from_numpy(r).to(dev) for r in raws]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    assert stream.cuda_stream != 0
    got = posterior._call(0, xs, ks, modes, sds, [t.data_ptr() for t in tens], True, lds, ns, ws, widths, probs, stream=stream.cuda_stream)
    for name in ref.FLAT:
        assert np.array_equal(got[name], host[name], equal_nan=False), name
    recs = posterior._split(got, [x.size for x in xs], ks, probs, [1] * 3)
    for (x, c, K, mode, sd), g, w in zip(groups, recs, widths):
        _same(g, ref.summaries(x, c, K, mode, bool(sd), PROBS, w), x.size, w, "device groups on a stream")


def test_scratch_of_exactly_one_column_of_the_largest_group():
    """scratch_bytes = 8 S_max: the largest group goes one column per pass, the others floor(S_max / S) columns; every
    output equals the default-scratch call's bit for bit"""
    groups = _groups(FRAME_CASES, 57)
    s_max = max(g[1].shape[0] * g[1].shape[1] for g in groups)
    assert sorted(g[1].shape[0] * g[1].shape[1] for g in groups) == [18, 21, 65] and s_max == 65
    one = _run(groups)
    many = _run(groups, scratch_bytes=8 * s_max)
    for a, b in zip(one, many):
        _identical(a, b)
    _check(groups, many, tag="one column per pass")
    from vamp_amd._post_lib import PostError
    with pytest.raises(PostError):
        _run(groups, scratch_bytes=8 * s_max - 8)
