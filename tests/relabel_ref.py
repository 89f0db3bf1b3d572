"""numpy restatement of include/vamp_relabel.h: line vectors, bad samples, the pooled scale, the cost matrices, the
assignment (brute force over every permutation for K <= 6, scipy's linear_sum_assignment above), the rounds and the
moments; the optimality bar of the GPU comparison; a row-greedy assignment as the planted error; the inputs the CPU
and the GPU tests share; the stand-in for the library call that the wiring tests use; one group of a library call and
the check of one round of it (check_round); and the rounds checker (check_rounds) with its crowded chains, its case table
and the planted errors of the host loop (``plant=`` of relabel).

Sums are numpy's (pairwise), not the kernel's chunked folds: the comparisons allow for that in their bars."""
import itertools

import numpy as np

Q_OF_MODE = {0: 3, 1: 4}
BRUTE_MAX_K = 6
EPS = 2.0 ** -52


def lines(flat, K, q):
    """[S, D] samples -> [S, K, q] line vectors (a view where it can be)"""
    return flat[:, :K * q].reshape(flat.shape[0], K, q)


def bad_samples(flat, K, q):
    """[S] bool: any of the q K line parameters is not finite (the sd is not looked at)"""
    return ~np.isfinite(flat[:, :K * q]).all(axis=1)


def pooled_scale(v):
    """[q] from the good samples' [n, K, q] line vectors: the sd (n - 1) of parameter d over all K lines and samples"""
    n, K, q = v.shape
    if n * K < 2:
        return np.ones(q)
    with np.errstate(all="ignore"):
        sd = v.reshape(n * K, q).std(axis=0, ddof=1)
    return np.where(np.isfinite(sd) & (sd > 0), sd, 1.0)


def cost_matrices(v, ref, scale):
    """C[s, i, j] = sum_d ((v[s, i, d] - ref[j, d]) / scale[d])^2, summed in d order"""
    S, K, q = v.shape
    C = np.zeros((S, K, K))
    with np.errstate(all="ignore"):
        for d in range(q):
            t = (v[:, :, None, d] - ref[None, None, :, d]) / scale[d]
            C += t * t
    return C


def perm_cost(C, perm):
    """sum_j C[s, perm[s, j], j], summed in j order"""
    S, K, _ = C.shape
    tot = np.zeros(S)
    rows = np.arange(S)
    for j in range(K):
        tot = tot + C[rows, perm[:, j], j]
    return tot


_PERMS = {}


def _perms(K):
    if K not in _PERMS:
        _PERMS[K] = np.array(list(itertools.permutations(range(K))), dtype=np.int64)
    return _PERMS[K]


def brute_totals(C):
    """[S, K!] totals of every permutation, in itertools' order"""
    S, K, _ = C.shape
    P = _perms(K)
    tot = np.zeros((S, len(P)))
    for j in range(K):
        tot = tot + C[:, P[:, j], j]
    return tot


def assign_brute(C):
    """(perm [S, K], total [S], gap [S]): the best permutation of every matrix by exhaustion; gap = second best - best
    (inf for K = 1)"""
    S, K, _ = C.shape
    assert K <= BRUTE_MAX_K
    tot = brute_totals(C)
    best = tot.argmin(axis=1)
    perm = _perms(K)[best]
    if tot.shape[1] > 1:
        two = np.partition(tot, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    else:
        gap = np.full(S, np.inf)
    return perm, perm_cost(C, perm), gap


def assign_scipy(C):
    """(perm [S, K], total [S]) by scipy.optimize.linear_sum_assignment: label j <- line perm[j]"""
    from scipy.optimize import linear_sum_assignment
    S, K, _ = C.shape
    perm = np.empty((S, K), dtype=np.int64)
    for s in range(S):
        rows, cols = linear_sum_assignment(C[s])
        perm[s, cols] = rows
    return perm, perm_cost(C, perm)


def assign(C):
    """(perm, total): brute force for K <= 6, scipy above"""
    if C.shape[1] <= BRUTE_MAX_K:
        perm, tot, _ = assign_brute(C)
        return perm, tot
    return assign_scipy(C)


def assign_greedy_rows(C):
    """THE PLANTED ERROR: line after line takes the nearest label still free"""
    S, K, _ = C.shape
    perm = np.empty((S, K), dtype=np.int64)
    for s in range(S):
        free = list(range(K))
        for i in range(K):
            j = min(free, key=lambda c: C[s, i, c])
            perm[s, j] = i
            free.remove(j)
    return perm, perm_cost(C, perm)


def bar(C):
    """B_s = 2 K^3 2^-52 max_ij C_s(i, j): each of the <= 2K potentials is updated at most K^2 times, and each update
    rounds once relative to the largest entry"""
    K = C.shape[1]
    return 2.0 * K ** 3 * EPS * C.reshape(C.shape[0], -1).max(axis=1)


def gather(flat, perm, K, q):
    """the relabelled copy of [S, D] samples: line j <- line perm[s, j]; the sd stays"""
    out = flat.copy()
    v = lines(flat, K, q)
    out[:, :K * q] = np.take_along_axis(v, perm[:, :, None], axis=1).reshape(flat.shape[0], K * q)
    return out


PLANTS = ("means through the inverse permutation", "reference not moved", "prev never updated", "bad samples in the means' n",
          "n_iter is the round limit")


def relabel(chain, K, mode, sd, ref, scale=None, max_iter=10, solver=assign, plant=None):
    """The whole call on one [N, W, D] chain (or [S, D] samples); returns a dict with the header's outputs: perm
    [S, K] (int64), cost [S], label_mean / label_sd [K, q], scale [q], n_iter, n_changed, n_switched, n_used, n_bad,
    chain (the relabelled copy, in the input's shape) and costs (the last round's matrices of the good samples, with
    their sample indices in `good`).  ``plant`` (one of PLANTS) switches on one deliberate error of the host loop or of
    the moments, for the tests that show the rounds checker below would see it."""
    assert plant is None or plant in PLANTS
    q = Q_OF_MODE[mode]
    flat = np.ascontiguousarray(chain, dtype=np.float64).reshape(-1, np.shape(chain)[-1])
    assert flat.shape[1] == q * K + sd
    S = flat.shape[0]
    bad = bad_samples(flat, K, q)
    good = np.flatnonzero(~bad)
    v = lines(flat, K, q)[good]
    scale = pooled_scale(v) if scale is None else np.asarray(scale, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64).reshape(K, q).copy()
    prev = np.tile(np.arange(K), (len(good), 1))

    def relabelled(perm):
        through = np.argsort(perm, axis=1) if plant == "means through the inverse permutation" else perm
        return np.take_along_axis(v, through[:, :, None], axis=1)

    def means(moved):
        if not len(good):
            return np.full((K, q), np.nan)
        return moved.sum(axis=0) / S if plant == "bad samples in the means' n" else moved.mean(axis=0)

    n_iter = 0
    for r in range(1, max_iter + 1):
        C = cost_matrices(v, ref, scale)
        finite = np.isfinite(C).all(axis=(1, 2))
        perm = np.tile(np.arange(K), (len(good), 1))
        tot = np.full(len(good), np.nan)
        if finite.any():
            perm[finite], tot[finite] = solver(C[finite])
        n_changed = int((perm != prev).any(axis=1).sum())
        if plant != "prev never updated":
            prev = perm
        if r > 1 and n_changed == 0:
            n_iter = r
            break
        if r == max_iter:
            n_iter = r
            break
        if plant != "reference not moved":
            ref = means(relabelled(perm))
    if plant == "n_iter is the round limit":
        n_iter = max_iter
    moved = relabelled(perm)
    with np.errstate(all="ignore"):
        mean = means(moved)
        sdev = moved.std(axis=0, ddof=1) if len(good) > 1 else np.full((K, q), np.nan)
    full_perm = np.tile(np.arange(K), (S, 1))
    full_perm[good] = perm
    cost = np.full(S, np.nan)
    cost[good] = tot
    return {"perm": full_perm, "cost": cost, "label_mean": mean, "label_sd": sdev, "scale": scale, "n_iter": n_iter,
            "n_changed": n_changed, "n_switched": int((perm != np.arange(K)).any(axis=1).sum()), "n_used": len(good),
            "n_bad": int(bad.sum()), "chain": gather(flat, full_perm, K, q).reshape(np.shape(chain)), "costs": C, "good": good,
            "last_ref": ref}


# ---- inputs the CPU and the GPU tests share -----------------------------------------------------------------------
def prior_wide(rng, S, K, q, sd=0, span=100.0):
    """[S, D] samples as wide as a prior: amplitudes in (0, 3), centres over the region, widths in (0, span / 2): the
    hard case, every line anywhere"""
    th = np.empty((S, q * K + sd))
    for k in range(K):
        th[:, q * k] = rng.uniform(0.0, 3.0, S)
        th[:, q * k + 1] = rng.uniform(-0.5 * span, 0.5 * span, S)
        for d in range(2, q):
            th[:, q * k + d] = rng.uniform(0.0, 0.5 * span, S)
    if sd:
        th[:, -1] = rng.uniform(0.0, 1.0, S)
    return th


def planted(rng, S, K, q, sd=0):
    """(samples [S, D], reference [K, q], planted perm [S, K]): lines 10 scale units apart in every parameter with
    jitter 1 (scale = 1), each sample's lines shuffled; relabelling against the reference must return the shuffle"""
    ref = 10.0 * np.arange(K)[:, None] + np.arange(q)[None, :] * 0.25
    v = ref[None] + rng.standard_normal((S, K, q))
    perm = np.array([rng.permutation(K) for _ in range(S)])
    th = np.empty((S, q * K + sd))
    # the sample's line perm[s, j] holds label j's vector, so the optimal pi(j) is perm[s, j]
    shuffled = np.empty_like(v)
    np.put_along_axis(shuffled, perm[:, :, None], v, axis=1)
    th[:, :q * K] = shuffled.reshape(S, q * K)
    if sd:
        th[:, -1] = rng.uniform(0.0, 1.0, S)
    return th, ref, perm


EXACT_CASES = ((2, 3), (3, 4), (6, 4))             # (K, q) of the exact-permutation comparison: 2 000 prior-wide samples each


def exact_case(K, q):
    """the samples, reference and unit scale of an exact-permutation case, the same on the CPU and on the GPU"""
    rng = np.random.default_rng(7000 + 10 * K + q)
    th = prior_wide(rng, 2000, K, q)
    ref = lines(prior_wide(rng, 1, K, q), K, q)[0]
    return th, ref


def two_line_chain(rng, N=40, W=16, sd=1, base=((0.8, -5.0, 1.5), (0.5, 5.0, 2.5))):
    """a two-line GAUSS3 chain [N, W, D] around ``base`` with jitter (0.05, 1, 0.1), and the same chain with the labels of
    random walkers swapped: (unswapped chain, swapped chain, the swapped walkers [W] bool; walker 0 is, walker 1 is not).
    The default lines are 10 jitters apart in centre and differ in every parameter, so a relabelling restores the
    unswapped chain exactly"""
    K, q = 2, 3
    v = np.array(base)[None, None] + rng.standard_normal((N, W, K, q)) * np.array([0.05, 1.0, 0.1])
    chain = np.empty((N, W, q * K + sd))
    chain[:, :, :q * K] = v.reshape(N, W, q * K)
    if sd:
        chain[:, :, -1] = rng.uniform(0.1, 0.2, (N, W))
    swapped = rng.random(W) < 0.5
    swapped[:2] = (True, False)
    mixed = chain.copy()
    mixed[:, swapped, :q * K] = v[:, swapped][:, :, ::-1].reshape(N, int(swapped.sum()), q * K)
    return chain, mixed, swapped


def crossing_chain(rng, N=40, W=16, sd=1):
    """``two_line_chain`` with lines that differ in centre alone, by 4 jitters: their centres cross in some samples, which
    is where a greedy assignment goes wrong"""
    return two_line_chain(rng, N, W, sd, base=((0.8, -2.0, 1.5), (0.8, 2.0, 1.5)))


def crowded_chain(rng, S, K, q, sep, sd=0):
    """(samples [S, D], start reference [K, q]): K lines whose centres are ``sep`` jitters apart and whose other
    parameters are alike, with jitter (0.05, 1, 0.1, 0.1); every sample's lines are shuffled, and the start reference
    is the first sample's lines, so the first round mislabels many samples and the rounds have work to do.  Two
    samples carry a NaN and an inf in a line parameter (bad, left out); with ``sd`` one sample has a NaN in its sd
    alone (not bad)."""
    base = np.tile(np.array([0.8, 0.0, 1.5, 1.2])[:q], (K, 1))
    base[:, 1] = sep * (np.arange(K) - 0.5 * (K - 1))
    v = base[None] + rng.standard_normal((S, K, q)) * np.array([0.05, 1.0, 0.1, 0.1])[:q]
    for s in range(S):
        v[s] = v[s, rng.permutation(K)]
    th = np.empty((S, q * K + sd))
    th[:, :q * K] = v.reshape(S, q * K)
    if sd:
        th[:, -1] = rng.uniform(0.1, 0.2, S)
        th[S // 2, -1] = np.nan
    start = v[0].copy()
    th[S // 3, q * K - 1] = np.nan
    th[2 * S // 3, 1] = np.inf
    return th, start


# ---- the stand-in for the library call --------------------------------------------------------------------------
def fake_relabel_host(calls):
    """what tests put in place of ``vamp_amd.relabel._relabel_host``: the restatement, one dict per chain; every call is
    noted in ``calls`` as (chains, max_iter)"""
    def host(arrays, n_comp, modes, sds, refs, scales, max_iter, device, want_chain):
        calls.append((len(arrays), int(max_iter)))
        out = []
        for a, K, m, sd, ref, sc in zip(arrays, n_comp, modes, sds, refs, scales):
            r = relabel(a, K, m, sd, ref, sc, max_iter)
            rec = {k: r[k] for k in ("cost", "label_mean", "label_sd", "scale", "n_iter", "n_changed", "n_switched", "n_used", "n_bad")}
            rec["perm"] = r["perm"].astype(np.uint8)
            rec["chain"] = r["chain"] if want_chain else None
            out.append(rec)
        return out
    return host


# ---- one group of a library call, and one round of it against the restatement ------------------------------------------
FLAT = ("perm", "cost", "label_mean", "label_sd", "scale", "n_iter", "n_changed", "n_switched", "n_used", "n_bad")


def group(th, W, K, mode, sd, reference, scale=None, pad=0):
    """a chain [n_keep, W, D] from [S, D] samples inside a buffer whose rows are W D + pad doubles apart"""
    S, D = th.shape
    assert S % W == 0 and D == Q_OF_MODE[mode] * K + sd
    buf = np.full((S // W, W * D + pad), -777.0)
    buf[:, :W * D] = th.reshape(S // W, W * D)
    return {"buf": buf, "W": W, "D": D, "K": K, "mode": mode, "sd": sd, "ref": np.asarray(reference, dtype=np.float64), "scale": scale,
            "n_keep": S // W}


def samples(g):
    return g["buf"][:, :g["W"] * g["D"]].reshape(-1, g["D"])


def moment_bar(v):
    """1e-12 of the largest |value| of every parameter type [q]"""
    return 1e-12 * np.maximum(np.abs(v).reshape(-1, v.shape[-1]).max(axis=0), 1e-300)


def check_round(got, g, label, max_iter=1, exact=True):
    """one group's outputs at max_iter = 1 against the restatement; returns the worst error / bar"""
    K, q, sd, W, D = g["K"], Q_OF_MODE[g["mode"]], g["sd"], g["W"], g["D"]
    th = samples(g)
    S = th.shape[0]
    want = relabel(th, K, g["mode"], sd, g["ref"], g["scale"], max_iter)
    good = want["good"]
    bad = np.setdiff1d(np.arange(S), good)
    perm = got["perm"].astype(np.int64)
    assert perm.shape == (S, K) and got["cost"].shape == (S,)
    assert (got["n_used"], got["n_bad"]) == (want["n_used"], want["n_bad"]) == (len(good), len(bad)), label
    assert np.array_equal(perm[bad], np.tile(np.arange(K), (len(bad), 1))) and np.isnan(got["cost"][bad]).all(), label
    assert np.array_equal(np.sort(perm, axis=1), np.tile(np.arange(K), (S, 1))), label
    worst = 0.0
    v = lines(th, K, q)[good]
    # the scale first: the costs below are the restatement's under the scale the KERNEL used
    if len(good):
        sb = 1e-12 * np.maximum(1.0, np.abs(want["scale"]))
        assert np.all(np.abs(got["scale"] - want["scale"]) <= sb), (label, got["scale"], want["scale"])
        worst = max(worst, float(np.max(np.abs(got["scale"] - want["scale"]) / sb)))
    if g["scale"] is not None:
        assert np.array_equal(got["scale"], g["scale"])
    if max_iter == 1 and len(good):
        C_ = cost_matrices(v, g["ref"].reshape(K, q), got["scale"])
        assert np.isfinite(C_).all()
        _, opt = assign(C_)
        mine = perm_cost(C_, perm[good])
        B = bar(C_)
        if K == 1:      # no solver: the returned cost is one entry of the matrix, which is the restatement's bit for bit
            assert np.array_equal(got["cost"][good], C_[:, 0, 0]), label
        assert np.all(mine <= opt + B), (label, float(np.max((mine - opt) / B)))
        assert np.all(np.abs(got["cost"][good] - mine) <= B), (label, float(np.max(np.abs(got["cost"][good] - mine) / B)))
        worst = max(worst, float(np.max(np.maximum(mine - opt, np.abs(got["cost"][good] - mine)) / np.maximum(B, 1e-300))))
        if 1 < K <= BRUTE_MAX_K and exact:
            pb, _, gap = assign_brute(C_)
            clear = gap > 2 * B
            assert (~clear).mean() <= 0.01 and np.array_equal(perm[good][clear], pb[clear]), label
        ident = np.arange(K)
        assert got["n_switched"] == int((perm[good] != ident).any(axis=1).sum()) == got["n_changed"] and got["n_iter"] == 1, label
    # data movement, bit for bit
    if got.get("out") is not None:
        moved = gather(th, perm, K, q)
        out = got["out"]
        assert np.array_equal(out[:, :W * D].reshape(S, D), moved, equal_nan=True), label
        pad = out[:, W * D:]
        assert np.all(pad == (-777.0 if got["input"] is None else -555.0)), label                  # the padding comes back untouched
        if got["input"] is not None:
            assert np.array_equal(got["input"], g["buf"], equal_nan=True), label                   # and out of place the input
    # the moments under the kernel's own permutations
    moved = np.take_along_axis(v, perm[good][:, :, None], axis=1)
    if len(good) >= 1:
        mb = moment_bar(v)
        err = np.abs(got["label_mean"] - moved.mean(axis=0)) / mb
        assert np.all(err <= 1.0), (label, "label_mean", err.max())
        worst = max(worst, float(err.max()))
    else:
        assert np.isnan(got["label_mean"]).all() and np.isnan(got["label_sd"]).all()
    if len(good) >= 2:
        err = np.abs(got["label_sd"] - moved.std(axis=0, ddof=1)) / moment_bar(v)
        assert np.all(err <= 1.0), (label, "label_sd", err.max())
        worst = max(worst, float(err.max()))
    elif len(good) == 1:
        assert np.isnan(got["label_sd"]).all()
    return worst


# ---- every round of the iteration ---------------------------------------------------------------------------------
def restated_call(plant=None):
    """``call(groups, max_iter)`` of the rounds checker with the restatement (``plant``: with one planted error) in the
    library's place: per group the FLAT outputs, ``out`` (a sentinel-filled buffer the relabelled chain went to) and
    ``input``, as the GPU tests' own call returns them"""
    def call(groups, max_iter):
        res = []
        for g in groups:
            r = relabel(samples(g), g["K"], g["mode"], g["sd"], g["ref"], g["scale"], max_iter, plant=plant)
            rec = {k: r[k] for k in FLAT}
            rec["perm"] = r["perm"].astype(np.uint8)
            out = np.full_like(g["buf"], -555.0)
            out[:, :g["W"] * g["D"]] = r["chain"].reshape(g["n_keep"], g["W"] * g["D"])
            rec["out"], rec["input"] = out, g["buf"].copy()
            res.append(rec)
        return res
    return call


def converged_of(got):
    """``converged`` of the Python record (vamp_amd.relabel.RelabelRecord) made of one group's outputs"""
    from vamp_amd.relabel import RelabelRecord
    K = got["perm"].shape[1]
    return RelabelRecord(got["perm"].reshape(1, -1, K), got["cost"].reshape(1, -1), got["label_mean"], got["label_sd"], got["scale"],
                         got["n_iter"], got["n_changed"], got["n_switched"], got["n_used"], got["n_bad"]).converged


CLOSED = ("perm", "cost", "label_mean", "label_sd", "scale", "n_switched", "n_used", "n_bad", "out")


def check_rounds(call, g, label, R_max):
    """Every round of one group's iteration, with ``call(groups, max_iter) -> per-group outputs`` the library on the GPU
    or the restatement on the CPU.  Returns {"worst": worst error / bar, "stop": the round that changed nothing (None:
    none up to R_max), "J": [J_1 ..], "gap": the smallest best / second-best gap of any round in bars (K <= 6)}.

    Chained.  c_1 is one round from the group's start reference and scale argument; c_r one round from c_{r-1}'s
    label_mean and c_1's scale, the doubles passed back as they came.  ``stop`` is the first r >= 2 whose permutations
    equal those of r - 1 on every sample.  Every c_r goes through ``check_round``: optimal to the solver's bar against
    brute force or scipy, the returned cost, exact permutations where the gap is clear, the moments under its own
    permutations, the chain moved bit for bit and the padding untouched.

    Closure.  For every R in 1 .. R_max one call of R rounds returns what c_min(R, stop) returned, bit for bit (CLOSED);
    n_iter = min(R, stop); n_changed counts the good samples whose permutation differs between the last two rounds
    (round 0: the identity); and the Python record says ``converged`` exactly when stop <= R.

    Descent.  The scale is fixed and every cost matrix finite (both asserted).  With J(pi, m) = sum_s sum_j
    |v_s,pi_s(j) - m_j|^2 in scale units, a round is two steps that each minimise J over their own argument: for fixed
    permutations the label means are the m that minimise every term's sum of squares, so J(pi_r, m_{r+1}) <= J(pi_r, m_r);
    and for fixed m the assignment minimises every sample's term over pi_s, to its bar B_s.  Hence
    J_{r+1} <= J_r + sum_s B_s(r + 1) + 4 n 2^-52 J_r: the solver bars of the round plus the rounding of the two n-term sums
    that are compared (the means' own rounding enters J squared and is far below either).  J is the restatement's cost
    of the permutations under test.  A sequence that falls over finitely many labellings ends: the iteration terminates.

    Fixed point.  Where ``stop`` exists, the output chain relabelled against its own label_mean under that scale gives
    the identity everywhere, n_switched = 0, and comes back unchanged."""
    one = lambda grp, R: call([grp], R)[0]
    K, q, W, D = g["K"], Q_OF_MODE[g["mode"]], g["W"], g["D"]
    th = samples(g)
    good = np.flatnonzero(~bad_samples(th, K, q))
    v, n = lines(th, K, q)[good], len(good)
    ident = np.tile(np.arange(K), (th.shape[0], 1))
    c, refs, worst, stop = [one(g, 1)], [g["ref"].reshape(K, q)], 0.0, None
    worst = check_round(c[0], g, label + " round 1")
    fixed = c[0]["scale"].copy()
    for r in range(2, R_max + 1):
        gr = dict(g, ref=c[-1]["label_mean"].copy(), scale=fixed)
        c.append(one(gr, 1))
        refs.append(gr["ref"])
        worst = max(worst, check_round(c[-1], gr, label + " round %d" % r))
        if np.array_equal(c[-1]["perm"], c[-2]["perm"]):
            stop = r
            break
    # descent
    J, gap = [], np.inf
    for r, (cr, m) in enumerate(zip(c, refs), 1):
        assert np.array_equal(cr["scale"], fixed), "descent: the scale of round %d is not round 1's (%s)" % (r, label)
        C_ = cost_matrices(v, m, fixed)
        assert np.isfinite(C_).all(), "descent: a cost matrix of round %d is not finite (%s)" % (r, label)
        J.append(float(perm_cost(C_, cr["perm"].astype(np.int64)[good]).sum()))
        B = bar(C_)
        if 1 < K <= BRUTE_MAX_K:
            gap = min(gap, float((assign_brute(C_)[2] / B).min()))
        if r > 1:
            margin = float(B.sum()) + 4.0 * n * EPS * J[-2]
            assert J[-1] <= J[-2] + margin, "descent: J_%d = %.17g > J_%d = %.17g + %.3g (%s)" % (r, J[-1], r - 1, J[-2], margin, label)
            worst = max(worst, (J[-1] - J[-2]) / margin)
    # closure
    for R in range(1, R_max + 1):
        f = one(g, R)
        m = R if stop is None else min(R, stop)
        cm = c[m - 1]
        for k in CLOSED:
            assert np.array_equal(np.asarray(f[k]), np.asarray(cm[k]), equal_nan=True), \
                "closure: %s of %d rounds in one call is not that of chained round %d (%s)" % (k, R, m, label)
        assert f["n_iter"] == m, "closure: n_iter = %d after %d rounds in one call, chained stop %s (%s)" % (f["n_iter"], R, stop, label)
        before = ident if m == 1 else c[m - 2]["perm"].astype(np.int64)
        changed = int((cm["perm"].astype(np.int64) != before).any(axis=1)[good].sum())
        assert f["n_changed"] == changed, "closure: n_changed = %d after %d rounds, %d samples differ between rounds %d and %d (%s)" % (
            f["n_changed"], R, changed, m - 1, m, label)
        assert converged_of(f) == (stop is not None and stop <= R), "closure: converged after %d rounds, chained stop %s (%s)" % (R, stop, label)
    # fixed point
    if stop is not None:
        last = c[stop - 1]
        buf = g["buf"].copy()
        buf[:, :W * D] = last["out"][:, :W * D]
        gf = dict(g, buf=buf, ref=last["label_mean"].copy(), scale=fixed)
        again = one(gf, 1)
        assert np.array_equal(again["perm"], ident) and again["n_switched"] == 0, "fixed point: the relabelled chain is relabelled again (%s)" % label
        assert np.array_equal(again["out"][:, :W * D], buf[:, :W * D], equal_nan=True), "fixed point: the chain came back changed (%s)" % label
        worst = max(worst, check_round(again, gf, label + " fixed point"))
    return {"worst": worst, "stop": stop, "J": J, "gap": gap}


# the crowded chains of the rounds tests, the same on the CPU and on the GPU: (K, q, sd, sep, seed, S, W, pad).  Every
# case is run under the pooled scale and under GIVEN_SCALE, the jitters themselves.  Under the pooled scale the centres'
# scale grows with K sep while the other parameters' stays at their jitter, so neighbouring lines lie 3.5 / K scale
# units apart under a noise of one unit per other parameter: the iteration crawls, and most cases do not stop within
# R_MAX rounds.  Under the jitters the lines are ``sep`` units apart and the cases at sep = 2.5 stop in 3 .. 8 rounds.
R_MAX = 12
GIVEN_SCALE = (0.05, 1.0, 0.1, 0.1)
ROUNDS_CASES = ((3, 3, 0, 2.5, 1200, 192, 1, 0), (3, 4, 1, 2.5, 1201, 192, 6, 2), (6, 3, 1, 2.5, 1500, 192, 1, 0),
                (9, 4, 0, 2.5, 1800, 130, 5, 3), (17, 3, 1, 2.5, 2600, 130, 1, 0), (32, 4, 0, 2.5, 4100, 130, 10, 1),
                (32, 3, 1, 1.5, 4101, 130, 1, 0))


def rounds_case(case, given):
    """the group of one ROUNDS_CASES entry; ``given``: under GIVEN_SCALE, else under the pooled scale"""
    K, q, sd, sep, seed, S, W, pad = case
    th, start = crowded_chain(np.random.default_rng(seed), S, K, q, sep, sd)
    return group(th, W, K, q - 3, sd, start, scale=np.array(GIVEN_SCALE[:q]) if given else None, pad=pad)


def rounds_label(case, given):
    return "crowded K=%d q=%d sd=%d sep=%g S=%d W=%d %s scale" % (case[:4] + case[5:7] + ("given" if given else "pooled",))
