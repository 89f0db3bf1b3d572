"""GPU tests of libvamp_relabel.so against the numpy restatement (tests/relabel_ref.py).

The optimality bar is derived, not fitted: each of the <= 2K potentials of the shortest-augmenting-path solver is updated
at most K^2 times, and each update rounds once relative to the largest entry, so B_s = 2 K^3 2^-52 max_ij C_s(i, j)
(relabel_ref.bar).  Required of every good sample: the restatement's cost of the KERNEL's permutation <= the
restatement's optimum + B_s, and the returned cost within B_s of the former.  For K <= 6 the permutation must equal brute
force wherever the second-best total exceeds the best by more than 2 B_s; the samples left out as near ties may be at
most 1 % of a case (tests/test_relabel.py asserts on the CPU that the inputs of the exact comparison have none).  What
only moves data -- the relabelled chain, in place against out of place, host against device chains, the batch order, a
caller's stream, every output alone -- is compared bit for bit.  The moments (label_mean, label_sd, scale_used) are
compared at 1e-12 of the largest |value| of their parameter, against the restatement's moments under the kernel's own
permutations.  tests/test_relabel.py shows that a row-greedy assignment misses the optimality bar by nine orders of
magnitude and more, so these comparisons would see it.  Every round of the iteration is held to relabel_ref.check_rounds
(chained one-round calls against one call of R rounds, the descent of J, the fixed point), which tests/test_relabel.py shows
to fail on five planted errors of the host loop.  Every case prints its worst error / bar
(profiles/relabel_limits.txt)."""
import numpy as np
import pytest

import evidence_ref
import relabel_ref as ref

pytestmark = pytest.mark.gpu

FLAT = ref.FLAT


def _report(label, worst, extra=""):
    print("relabel %-74s worst error / bar %.3g%s" % (label, worst, extra))


# ---- 1. the solver through vamp_relabel_assign --------------------------------------------------------------------
def _matrices(rng, kind, n, K):
    if kind == "random":
        return rng.random((n, K, K)) * 10.0
    if kind == "integer":
        return rng.integers(0, 4, (n, K, K)).astype(np.float64)
    if kind == "constant":
        return np.full((n, K, K), 2.5)
    if kind == "identity optimal":
        return rng.random((n, K, K)) + 5.0 - 5.0 * np.eye(K)[None]
    if kind == "anti-diagonal optimal":
        return rng.random((n, K, K)) + 5.0 - 5.0 * np.eye(K)[::-1][None]
    assert kind == "wide range"
    return 10.0 ** rng.uniform(-12.0, 12.0, (n, K, K))


@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 16, 17, 32])
def test_solver_on_arbitrary_matrices(K):
    from vamp_amd import relabel
    rng = np.random.default_rng(500 + K)
    ident = np.arange(K)
    for kind in ("random", "integer", "constant", "identity optimal", "anti-diagonal optimal", "wide range"):
        worst = 0.0
        for n in (1, 7, 8, 9, 65):                                  # ragged lane groups in a wavefront
            C_ = _matrices(rng, kind, n, K)
            perm, total = relabel.assign(C_)
            perm = perm.astype(np.int64)
            assert np.array_equal(np.sort(perm, axis=1), np.tile(ident, (n, 1))), (kind, n)
            _, opt = ref.assign_scipy(C_)
            mine = ref.perm_cost(C_, perm)
            B = ref.bar(C_)
            if kind in ("integer", "constant"):                     # exact arithmetic: the totals are equal, ties or not
                assert np.array_equal(total, opt) and np.array_equal(mine, opt), (kind, n)
            else:
                assert np.all(mine <= opt + B) and np.all(np.abs(total - mine) <= B), (kind, n)
                worst = max(worst, float(np.max(np.maximum(mine - opt, np.abs(total - mine)) / B)))
            if kind == "identity optimal":
                assert np.array_equal(perm, np.tile(ident, (n, 1)))
            if kind == "anti-diagonal optimal":
                assert np.array_equal(perm, np.tile(ident[::-1], (n, 1)))
        _report("solver K=%d %s, n = 1 | 7 | 8 | 9 | 65" % (K, kind), worst)


@pytest.mark.parametrize("K", [1, 2, 9, 17, 32])
def test_solver_returns_on_matrices_that_are_not_finite(K):
    """a NaN or +inf entry: the identity, total NaN, and the call returns; the matrices beside it in the wavefront are
    solved as if it were not there"""
    from vamp_amd import relabel
    rng = np.random.default_rng(520 + K)
    C_ = rng.random((19, K, K)) * 10.0
    clean_perm, clean_total = relabel.assign(C_)
    C_[3, K - 1, 0] = np.nan
    C_[8, 0, K - 1] = np.inf
    C_[18] = np.nan
    C_[10, K // 2, K // 2] = -np.inf
    perm, total = relabel.assign(C_)
    hit = np.isin(np.arange(19), (3, 8, 10, 18))
    assert np.isnan(total[hit]).all() and np.array_equal(perm[hit], np.tile(np.arange(K), (4, 1)))
    assert np.array_equal(perm[~hit], clean_perm[~hit]) and np.array_equal(total[~hit], clean_total[~hit])


@pytest.mark.parametrize("K", [2, 8, 9, 32])
def test_solver_on_finite_matrices_whose_potentials_overflow(K):
    """entries up to 1.7e308 pass the finiteness check, but their sums do not stay finite: the call returns, every
    permutation is valid, and a matrix either has a finite total that is its permutation's cost or the identity and NaN"""
    from vamp_amd import relabel
    rng = np.random.default_rng(540 + K)
    C_ = rng.uniform(0.5, 1.7, (33, K, K)) * 1e308
    C_[::3] *= 1e-300                                               # every third matrix is harmless
    perm, total = relabel.assign(C_)
    perm = perm.astype(np.int64)
    assert np.array_equal(np.sort(perm, axis=1), np.tile(np.arange(K), (33, 1)))
    gave_up = np.isnan(total)
    assert np.array_equal(perm[gave_up], np.tile(np.arange(K), (int(gave_up.sum()), 1))) and not gave_up[::3].any()
    with np.errstate(over="ignore"):
        mine = ref.perm_cost(C_, perm)
    assert np.all(np.isfinite(total[~gave_up])) and np.all(np.abs(total[~gave_up] - mine[~gave_up]) <= ref.bar(C_)[~gave_up])
    _, opt = ref.assign_scipy(C_[::3])
    assert np.all(mine[::3] <= opt + ref.bar(C_[::3]))
    print("relabel solver K=%d entries near DBL_MAX: %d of 22 matrices given up (identity, NaN)" % (K, gave_up.sum()))


# ---- 2. chains against the restatement -----------------------------------------------------------------------------
_group, _samples = ref.group, ref.samples          # shared with the CPU tests of the rounds checker (tests/relabel_ref.py)


def _run(groups, max_iter=1, out="apart", want=FLAT, device=False, stream=None):
    """one vamp_relabel_chains call; per group a dict of its outputs and ``out`` (the buffer the relabelled chain went
    to: a sentinel-filled copy's, the input's own (in place), or None).  ``device``: the chains are copied to device
    memory first and the relabelled chain comes back from there"""
    from vamp_amd import relabel
    bufs = [g["buf"].copy() for g in groups]
    outs = None if out is None else bufs if out == "in place" else [np.full_like(b, -555.0) for b in bufs]
    keep = []
    if device:
        import torch
        t_in = [torch.tensor(b, device="cuda:0") for b in bufs]
        t_out = None if out is None else t_in if out == "in place" else [torch.tensor(o, device="cuda:0") for o in outs]
        torch.cuda.synchronize()
        keep = [t_in, t_out]
        in_ptr, out_ptr = [t.data_ptr() for t in t_in], None if t_out is None else [t.data_ptr() for t in t_out]
    else:
        in_ptr, out_ptr = [b.ctypes.data for b in bufs], None if outs is None else [o.ctypes.data for o in outs]
    ld = [b.shape[1] for b in bufs]
    flat = relabel._call(0, [g["K"] for g in groups], [g["mode"] for g in groups], [g["sd"] for g in groups], in_ptr, device, ld,
                         [g["n_keep"] for g in groups], [g["W"] for g in groups], [g["ref"] for g in groups], [g["scale"] for g in groups],
                         max_iter, out_ptr, ld, device, stream=stream, want=want)
    if device and outs is not None:
        import torch
        torch.cuda.synchronize()
        outs = [t.cpu().numpy() for t in keep[1]]
    return [dict({k: flat[k][i] for k in flat}, out=None if outs is None else outs[i], input=bufs[i] if out != "in place" else None)
            for i in range(len(groups))]


_moment_bar, _check = ref.moment_bar, ref.check_round


SHAPES = (7, 8, 9, 63, 64, 65, 129)


@pytest.mark.parametrize("sd", [0, 1])
@pytest.mark.parametrize("q", [3, 4])
@pytest.mark.parametrize("K", [1, 2, 3, 6, 9, 17, 32])
def test_prior_wide_chains_against_the_restatement(K, q, sd):
    """the hard case, every line anywhere: S = 7 .. 129 at W = 1, one library call for the seven chains; then W = 5 with
    padded rows, a given scale, a NaN in a line parameter (bad) and a NaN in the sd alone (not bad)"""
    rng = np.random.default_rng(600 + 100 * K + 10 * q + sd)
    mode = q - 3
    groups = [_group(ref.prior_wide(rng, S, K, q, sd), 1, K, mode, sd, ref.lines(ref.prior_wide(rng, 1, K, q), K, q)[0]) for S in SHAPES]
    th = ref.prior_wide(rng, 65, K, q, sd)
    th[11, q * K - 1] = np.nan
    th[40, 0] = np.inf
    if sd:
        th[20, -1] = np.nan
    groups.append(_group(th, 5, K, mode, sd, ref.lines(ref.prior_wide(rng, 1, K, q), K, q)[0], pad=3))
    groups.append(_group(ref.prior_wide(rng, 35, K, q, sd), 7, K, mode, sd, ref.lines(ref.prior_wide(rng, 1, K, q), K, q)[0],
                         scale=np.array([1.0, 30.0, 15.0, 15.0][:q]), pad=1))
    got = _run(groups)
    worst = max(_check(r, g, "K=%d q=%d sd=%d group %d" % (K, q, sd, i)) for i, (r, g) in enumerate(zip(got, groups)))
    assert got[7]["n_bad"] == 2 and (not sd or np.isnan(got[7]["out"][4, groups[7]["D"] - 1]))      # sample 20 = row 4, walker 0: its sd
    _report("prior-wide chains K=%d q=%d sd=%d, S = 7 .. 129, W = 1 | 5 | 7" % (K, q, sd), worst)


@pytest.mark.parametrize("K,q", ref.EXACT_CASES)
def test_exact_permutations_on_two_thousand_prior_wide_samples(K, q):
    th, r = ref.exact_case(K, q)
    g = _group(th, 8, K, q - 3, 0, r, scale=np.ones(q))
    got = _run([g])[0]
    worst = _check(got, g, "exact K=%d q=%d" % (K, q))
    C_ = ref.cost_matrices(ref.lines(th, K, q), r, np.ones(q))
    pb, _, gap = ref.assign_brute(C_)
    assert np.all(gap > 2 * ref.bar(C_)) and np.array_equal(got["perm"], pb)        # no near tie (test_relabel.py): every one
    _report("exact permutations K=%d q=%d, 2 000 prior-wide samples" % (K, q), worst, ", smallest gap %.3g bars" % (gap / ref.bar(C_)).min())


@pytest.mark.parametrize("K", range(1, 33))
def test_planted_permutations_are_returned(K):
    """lines 10 scale units apart with jitter 1, every sample's lines shuffled: the permutation is the planted one"""
    rng = np.random.default_rng(700 + K)
    worst = 0.0
    for q, sd in ((3, 1), (4, 0)):
        th, r, perm = ref.planted(rng, 66, K, q, sd)
        g = _group(th, 6, K, q - 3, sd, r, scale=np.ones(q), pad=2)
        got = _run([g])[0]
        worst = max(worst, _check(got, g, "planted K=%d q=%d" % (K, q), exact=False))
        assert np.array_equal(got["perm"], perm)
        # relabelled a second time against the first call's label means: the identity everywhere
        again = _group(got["out"][:, :6 * g["D"]].reshape(-1, g["D"]), 6, K, q - 3, sd, got["label_mean"], scale=np.ones(q))
        second = _run([again])[0]
        assert np.array_equal(second["perm"], np.tile(np.arange(K), (66, 1))) and second["n_switched"] == 0
        assert np.array_equal(second["out"], again["buf"])
    _report("planted permutations K=%d" % K, worst)


def test_edges_no_good_sample_one_good_sample_and_an_overflowing_cost():
    bad = np.full((9, 7), np.nan)
    one = np.full((9, 7), np.nan)
    one[4] = [1.0, 5.0, 2.0, 0.5, -5.0, 1.0, 0.1]
    huge = np.tile([1.0, 5.0, 2.0, 0.5, -5.0, 1.0, 0.1], (9, 1))
    huge[2, 1] = 1e200                                              # finite, but its squared distance is not
    r = np.array([[0.5, -5.0, 1.0], [1.0, 5.0, 2.0]])
    groups = [_group(a, 1, 2, 0, 1, r) for a in (bad, one, huge)]
    got = _run(groups[:2], max_iter=3) + _run(groups[2:], max_iter=1)      # (a second round's reference would hold the 1e200)
    assert (got[0]["n_used"], got[0]["n_bad"], got[0]["n_switched"], got[0]["n_changed"]) == (0, 9, 0, 0)
    assert np.isnan(got[0]["label_mean"]).all() and np.isnan(got[0]["label_sd"]).all() and np.all(got[0]["scale"] == 1.0)
    assert np.array_equal(got[0]["out"], groups[0]["buf"], equal_nan=True)
    assert (got[1]["n_used"], got[1]["n_bad"], got[1]["n_switched"]) == (1, 8, 1) and list(got[1]["perm"][4]) == [1, 0]
    assert np.array_equal(got[1]["label_mean"], [[0.5, -5.0, 1.0], [1.0, 5.0, 2.0]]) and np.isnan(got[1]["label_sd"]).all()
    assert list(got[1]["out"][4]) == [0.5, -5.0, 1.0, 1.0, 5.0, 2.0, 0.1]
    assert got[2]["n_used"] == 9 and got[2]["n_bad"] == 0 and np.isnan(got[2]["cost"][2]) and list(got[2]["perm"][2]) == [0, 1]
    assert got[2]["n_switched"] == 8 and np.isfinite(np.delete(got[2]["cost"], 2)).all()


# ---- 3. bit for bit ---------------------------------------------------------------------------------------------
def _mixed_groups(rng):
    a = _group(ref.prior_wide(rng, 130, 3, 4, 1), 5, 3, 1, 1, ref.lines(ref.prior_wide(rng, 1, 3, 4), 3, 4)[0], pad=2)
    th, r, _ = ref.planted(rng, 66, 17, 3, 0)
    b = _group(th, 6, 17, 0, 0, r + 0.3)
    chain, mixed, _ = ref.two_line_chain(rng, N=30, W=8)
    c = _group(mixed.reshape(-1, 7), 8, 2, 0, 1, chain[0, 1, :6].reshape(2, 3))
    return [a, b, c]


def _same(x, y, keys=FLAT):
    for k in keys:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


def test_in_place_device_chains_batch_order_stream_and_single_outputs_change_no_bit():
    import torch
    rng = np.random.default_rng(800)
    groups = _mixed_groups(rng)
    base = _run(groups, max_iter=5)
    assert base[2]["n_iter"] in (2, 3) and base[0]["n_iter"] >= 2
    for got in (_run(groups, max_iter=5, out="in place"), _run(groups, max_iter=5, device=True),
                _run(groups, max_iter=5, out="in place", device=True)):
        for b, r, g in zip(base, got, groups):
            _same(b, r)
            WD = g["W"] * g["D"]
            assert np.array_equal(r["out"][:, :WD], b["out"][:, :WD], equal_nan=True) and np.all(r["out"][:, WD:] == (-777.0 if r["input"] is None else -555.0))
    for b, r in zip(base[::-1], _run(groups[::-1], max_iter=5)):
        _same(b, r)
        assert np.array_equal(b["out"], r["out"])
    alone = _run(groups[1:2], max_iter=5)[0]
    _same(base[1], alone)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert stream.cuda_stream != 0
    for b, r in zip(base, _run(groups, max_iter=5, device=True, stream=stream.cuda_stream)):
        _same(b, r)
        assert np.array_equal(b["out"], r["out"])
    for k in FLAT:                                                  # every output alone, the others NULL, no chain
        for b, r in zip(base, _run(groups, max_iter=5, out=None, want=(k,))):
            assert set(r) == {k, "out", "input"}
            _same(b, r, (k,))
    only_chain = _run(groups, max_iter=5, want=())
    for b, r in zip(base, only_chain):
        assert np.array_equal(b["out"], r["out"])


def test_device_chain_of_a_context_in_place():
    """the chain HipContext.run_dev wrote for three regions, relabelled through context_relabel: first reading only, then
    in place, against the same chain from the host; the other regions' columns of a row are not touched"""
    import torch
    import vamp_amd
    from vamp_amd import relabel
    rng = np.random.default_rng(810)
    n_keep, W = 12, 16
    specs = [(24, [(1.0, 12.0, 2.0)]), (40, [(1.2, 10.0, 2.0), (0.9, 28.0, 2.5)]), (56, [(1.0, 10.0, 2.0), (0.8, 28.0, 2.0), (1.1, 44.0, 3.0)])]
    data = [evidence_ref.gauss_line_data(P, lines, 0.05, 5 + i) for i, (P, lines) in enumerate(specs)]
    xs, fs = [d[0] for d in data], [d[1] for d in data]
    starts, refs = [], []
    for P, lines in specs:
        K = len(lines)
        th = np.empty((W, 3 * K + 1))
        for w in range(W):
            order = rng.permutation(K)                              # every walker starts in its own labelling
            for j, k in enumerate(order):
                A, c, s = lines[k]
                th[w, 3 * j:3 * j + 3] = (A * (1 + 0.05 * rng.standard_normal()), c + 0.2 * rng.standard_normal(), s * (1 + 0.05 * rng.standard_normal()))
            th[w, -1] = 0.05 * (1 + 0.1 * rng.random())
        starts.append(th)
        refs.append(np.array(lines))
    with vamp_amd.HipContext(device=0) as ctx:
        ctx.set_regions(xs, fs, [np.ones_like(f) for f in fs], [len(l) for _, l in specs], mode=vamp_amd.MODE_GAUSS3, sample_sd=True)
        ctx.sampler_init(starts, seed=81, a=2.0, split_block=W)
        dev = torch.device("cuda", 0)
        chain_t = torch.zeros((n_keep, ctx.total_theta), dtype=torch.float64, device=dev)
        lnp_t = torch.zeros((n_keep, ctx.total_walkers), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.run_dev(n_keep * 2, thin=2, chain_ptr=chain_t.data_ptr(), lnprob_ptr=lnp_t.data_ptr())
        host = chain_t.cpu().numpy()
        recs = relabel.context_relabel(ctx, chain_t.data_ptr(), n_keep, refs, max_iter=6)
        torch.cuda.synchronize()
        assert np.array_equal(chain_t.cpu().numpy(), host)          # reading only
        recs_in = relabel.context_relabel(ctx, chain_t.data_ptr(), n_keep, refs, max_iter=6, in_place=True)
        torch.cuda.synchronize()
        after = chain_t.cpu().numpy()
    off = 0
    for (P, lines), rec, rec_in in zip(specs, recs, recs_in):
        K = len(lines)
        D = 3 * K + 1
        chain = host[:, off:off + W * D].reshape(n_keep, W, D).copy()
        h = relabel.relabel_chains(chain, K, 0, 1, np.array(lines), max_iter=6, return_chain=True)
        for k in FLAT[:5] + ("n_iter", "n_changed", "n_switched", "n_used", "n_bad", "converged"):
            assert np.array_equal(getattr(rec, k), getattr(h, k), equal_nan=True) and np.array_equal(getattr(rec_in, k), getattr(h, k), equal_nan=True), k
        assert np.array_equal(after[:, off:off + W * D].reshape(n_keep, W, D), h.chain) and np.array_equal(h.chain, h.gather(chain))
        if K > 1:
            assert rec.n_switched > 0 and rec.converged              # the walkers' own labellings are undone
            centres = h.chain[:, :, 1:3 * K:3]
            assert np.all(np.abs(centres - np.array(lines)[:, 1]) < 6.0)
        off += W * D
    assert off == host.shape[1]


# ---- 4. rounds --------------------------------------------------------------------------------------------------
def test_rounds_on_a_two_line_chain_with_walkers_swapped_at_random():
    rng = np.random.default_rng(820)
    chain, mixed, swapped = ref.two_line_chain(rng)
    start = chain[0, 1, :6].reshape(2, 3)
    g, clean_g = _group(mixed.reshape(-1, 7), 16, 2, 0, 1, start), _group(chain.reshape(-1, 7), 16, 2, 0, 1, start)
    got, clean = _run([g, clean_g], max_iter=10)
    want = ref.relabel(mixed, 2, 0, 1, start, None, 10)
    unswapped = ref.relabel(chain, 2, 0, 1, start, None, 10)
    assert got["n_iter"] <= 3 and (got["n_iter"], got["n_changed"], got["n_switched"]) == (want["n_iter"], want["n_changed"], want["n_switched"])
    assert got["n_changed"] == 0 and np.array_equal(got["perm"], want["perm"])
    assert np.array_equal(got["out"], clean_g["buf"]) and np.array_equal(clean["out"], clean_g["buf"])    # the unswapped chain, bit for bit
    bar = _moment_bar(ref.lines(chain.reshape(-1, 7), 2, 3))
    worst = 0.0
    for k, target in (("label_sd", unswapped["label_sd"]), ("label_mean", unswapped["label_mean"])):
        err = np.abs(got[k] - target) / bar
        assert np.all(err <= 1.0), (k, err.max())
        assert np.array_equal(got[k], clean[k])                     # fixed-order sums of the same numbers
        worst = max(worst, float(err.max()))
    err = np.abs(got["scale"] - unswapped["scale"]) / bar
    assert np.all(err <= 1.0)
    worst = max(worst, float(err.max()))
    one = _run([g], max_iter=1)[0]
    assert one["n_iter"] == 1 and one["n_changed"] == one["n_switched"] > 0          # one round is reported as not converged
    from vamp_amd import relabel
    rec = relabel.relabel_chains(mixed, 2, 0, 1, start, max_iter=1)
    assert not rec.converged and relabel.relabel_chains(mixed, 2, 0, 1, start).converged
    two = _run([g], max_iter=2)[0]
    assert two["n_iter"] == 2 and (two["n_changed"] == 0) == (want["n_iter"] == 2)
    _report("rounds: two-line chain, %d of 16 walkers swapped, n_iter %d" % (swapped.sum(), got["n_iter"]), worst)


def _rounds_extra(res):
    return ", stop %s, J %.6g -> %.6g in %d rounds" % (res["stop"], res["J"][0], res["J"][-1], len(res["J"]))


@pytest.mark.parametrize("given", [True, False], ids=["given", "pooled"])
@pytest.mark.parametrize("case", ref.ROUNDS_CASES, ids=lambda c: "K%d-q%d-sd%d-sep%g" % c[:4])
def test_every_round_on_crowded_chains(case, given):
    """relabel_ref.check_rounds on the library: chained one-round calls against one R-round call for every R <= R_MAX bit
    for bit, n_iter, n_changed and converged, every round to the solver's bar, the descent of J and the fixed point;
    host chains out of place, and the cases with padded rows (one per lane width) in place on device chains as well"""
    g, label = ref.rounds_case(case, given), ref.rounds_label(case, given)
    res = ref.check_rounds(lambda groups, R: _run(groups, max_iter=R), g, label, ref.R_MAX)
    _report(label, res["worst"], _rounds_extra(res))
    if given and case[7]:
        dev = ref.check_rounds(lambda groups, R: _run(groups, max_iter=R, out="in place", device=True), g, label + " in place", ref.R_MAX)
        assert dev["stop"] == res["stop"] and dev["J"] == res["J"]
        _report(label + ", device chain in place", dev["worst"], _rounds_extra(dev))


def test_groups_of_one_call_stop_in_different_rounds():
    """six groups that stop in rounds of their own, or not at all: in one call, in reversed order and under round limits
    at the smallest, a middle and the largest stop, every group's outputs and chain are those of its own call, bit for bit"""
    rng = np.random.default_rng(830)
    _, mixed, _ = ref.two_line_chain(rng)
    th9, r9, _ = ref.planted(rng, 66, 9, 3, 1)
    groups = [ref.rounds_case(ref.ROUNDS_CASES[0], True),                                          # crowded K = 3: stops
              _group(mixed.reshape(-1, 7), 16, 2, 0, 1, mixed[0, 1, :6].reshape(2, 3)),            # the two-line chain
              ref.rounds_case(ref.ROUNDS_CASES[4], False),                                         # crowded K = 17: does not stop
              _group(np.full((9, 7), np.nan), 1, 2, 0, 1, np.array([[0.5, -5.0, 1.0], [1.0, 5.0, 2.0]])),      # every sample bad
              _group(ref.crowded_chain(rng, 70, 1, 4, 2.5, 1)[0], 7, 1, 1, 1, np.array([[0.8, 0.0, 1.5, 1.2]]), pad=1),
              _group(th9, 6, 9, 0, 1, r9, scale=np.ones(3), pad=2)]                                # planted K = 9, the truth as reference
    base = _run(groups, max_iter=ref.R_MAX)
    n_iter = [int(b["n_iter"]) for b in base]
    print("relabel groups of one call: n_iter %s, n_changed %s" % (n_iter, [int(b["n_changed"]) for b in base]))
    assert len(set(n_iter)) >= 3 and n_iter[2] == ref.R_MAX and base[2]["n_changed"] > 0 and n_iter[5] == 2 and n_iter[3] == n_iter[4] == 2
    assert base[3]["n_used"] == 0 and base[0]["n_changed"] == 0 and 3 <= n_iter[0] < ref.R_MAX
    stops = sorted({n for n, b in zip(n_iter, base) if b["n_changed"] == 0})
    limits = sorted({stops[0], stops[len(stops) // 2], (stops[0] + stops[-1]) // 2, stops[-1], ref.R_MAX})
    assert len(limits) >= 4
    for R in limits:
        both = base if R == ref.R_MAX else _run(groups, max_iter=R)
        back = _run(groups[::-1], max_iter=R)[::-1]
        for i, g in enumerate(groups):
            alone = _run([g], max_iter=R)[0]
            for got in (both[i], back[i]):
                _same(alone, got)
                assert np.array_equal(alone["out"], got["out"], equal_nan=True), (R, i)
            assert alone["n_iter"] == min(R, n_iter[i]), (R, i)


def test_the_product_s_chain_shape_180_by_64():
    """n_keep = 180, W = 64 (11 520 samples), free sd, one- to four-line regions in one call of three rounds under the pooled
    scale: k_colsum's 3 (q K = 3, 4) and 5 (q K = 6) workgroups per group and 15 at q K = 12.  The batched call's scale
    and moments against numpy, every group alone against batched bit for bit, and the rounds checker at R_max = 3"""
    rng = np.random.default_rng(840)
    groups = []
    for K, q in ((1, 3), (1, 4), (2, 3), (4, 3)):
        th, start = ref.crowded_chain(rng, 11520, K, q, 2.5, 1)
        groups.append(_group(th, 64, K, q - 3, 1, start))
    got = _run(groups, max_iter=3)
    for g, r in zip(groups, got):
        K, q = g["K"], ref.Q_OF_MODE[g["mode"]]
        label = "product shape 180 x 64, K=%d q=%d" % (K, q)
        th = _samples(g)
        v = ref.lines(th, K, q)[~ref.bad_samples(th, K, q)]
        want = ref.pooled_scale(v)
        assert r["n_bad"] == 2 and np.all(np.abs(r["scale"] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), label
        worst = _check(r, g, label, max_iter=3)                     # counts, data movement, the moments under its own permutations
        alone = _run([g], max_iter=3)[0]
        _same(alone, r)
        assert np.array_equal(alone["out"], r["out"], equal_nan=True), label
        res = ref.check_rounds(lambda grp, R: _run(grp, max_iter=R), g, label, 3)
        _report(label, max(worst, res["worst"]), _rounds_extra(res))


def test_edges_of_the_first_stage_task_split():
    """one | two workgroups of k_colsum (256 / (q K) chunks of 64 samples each): S = 5 440 | 5 441 at q K = 3, 4 096 | 4 097
    at q K = 4, 2 688 | 2 689 at q K = 6, W = 1, under the pooled scale: scale and moments at the bars of every other case"""
    rng = np.random.default_rng(850)
    groups, labels = [], []
    for K, q, S in ((1, 3, 5440), (1, 4, 4096), (2, 3, 2688)):
        for extra in (0, 1):
            th, start = ref.crowded_chain(rng, S + extra, K, q, 2.5, extra)
            groups.append(_group(th, 1, K, q - 3, extra, start))
            labels.append("first-stage split K=%d q=%d S=%d" % (K, q, S + extra))
    for g, r, label in zip(groups, _run(groups), labels):
        _report(label, _check(r, g, label))
    for g, r, label in zip(groups, _run(groups, max_iter=2), labels):                              # the sums through the permutations
        _check(r, g, label, max_iter=2)
        assert r["n_iter"] == 2


# ---- 5. end to end ----------------------------------------------------------------------------------------------
def test_stats_of_a_fit_whose_walkers_labels_were_swapped_after_sampling():
    """the two-line test data of the WAIC tests: stats(relabel=True) of the chain with half the walkers' labels swapped
    gives the per-line standard deviations of the unswapped chain; stats() gives the inflated ones"""
    from vamp_amd.vpfits import VPfit
    x, flux, noise = evidence_ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    fit = VPfit(seed=12)
    fit.nwalkers = 32
    fit.initialise_model(1.0e3 + x, flux, 2, voigt=False)
    fit.map_estimate()
    fit.mcmc_fit(iterations=300, burnin=100, thinning=5)
    lnp = fit._lnp_chain.copy()
    N, W, D = fit._chain_dev.shape
    own = fit.mcmc.relabel()
    print("relabel end to end: the sampled chain itself has %d of %d samples switched, %d rounds" % (own.n_switched, own.n_used, own.n_iter))
    assert own.converged
    # the unswapped chain: the sampled one in one labelling (the sampler's own walkers need not share one)
    chain = own.gather(fit._chain_dev)
    fit._ingest_chain(chain, lnp, np.zeros(W), N, N, 1.0, scored="skip", set_values=False)
    plain = {nm: dict(fit.mcmc.stats()[nm]) for nm in fit.mcmc.stats()}
    diag_plain = fit.mcmc.diagnostics()
    assert fit.mcmc.relabel().n_switched == 0 and fit.mcmc.relabel().converged      # relabelling twice changes nothing
    swapped = chain.copy()
    half = np.arange(W) % 2 == 1
    swapped[:, half, :6] = chain[:, half][:, :, [3, 4, 5, 0, 1, 2]]
    fit._ingest_chain(swapped, lnp, np.zeros(W), N, N, 1.0, scored="skip", set_values=False)
    inflated, back = fit.mcmc.stats(), fit.mcmc.stats(relabel=True)
    rec = fit.mcmc.relabel()
    assert rec.converged and rec.n_switched == N * W // 2 and rec.n_bad == 0
    worst = 0.0
    for nm in plain:
        for k in ("standard deviation", "mean"):
            assert back[nm][k] == pytest.approx(plain[nm][k], rel=1e-12), (nm, k)
            worst = max(worst, abs(back[nm][k] - plain[nm][k]) / (1e-12 * abs(plain[nm][k])))
    for nm in ("est_centroid_0", "est_centroid_1"):                 # half of slot k's samples are now the other line's
        print("relabel end to end: %s standard deviation %.4g as sampled, %.4g relabelled" % (nm, inflated[nm]["standard deviation"], back[nm]["standard deviation"]))
        assert inflated[nm]["standard deviation"] > back[nm]["standard deviation"]
    np.testing.assert_array_equal(fit.mcmc.trace("est_centroid_0", relabel=True)[:], fit._to_caller(chain.reshape(-1, D))[:, 1])
    d0, d1 = fit.mcmc.diagnostics(), fit.mcmc.diagnostics(relabel=True)
    print("relabel end to end: R-hat of est_centroid_0 %.4g as sampled, %.4g relabelled" % (d0["est_centroid_0"]["r_hat"], d1["est_centroid_0"]["r_hat"]))
    assert d1 == diag_plain and d0["est_centroid_0"]["r_hat"] > d1["est_centroid_0"]["r_hat"]
    _report("end to end: stats(relabel=True) against the unswapped chain's stats()", worst)
