"""numpy restatement of include/vamp_relabel.h: line vectors, bad samples, the pooled scale, the cost matrices, the
assignment (brute force over every permutation for K <= 6, scipy's linear_sum_assignment above), the rounds and the
moments; the optimality bar of the GPU comparison; a row-greedy assignment as the planted error; the inputs the CPU
and the GPU tests share; and the stand-in for the library call that the wiring tests use.

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


def relabel(chain, K, mode, sd, ref, scale=None, max_iter=10, solver=assign):
    """The whole call on one [N, W, D] chain (or [S, D] samples); returns a dict with the header's outputs: perm
    [S, K] (int64), cost [S], label_mean / label_sd [K, q], scale [q], n_iter, n_changed, n_switched, n_used, n_bad,
    chain (the relabelled copy, in the input's shape) and costs (the last round's matrices of the good samples, with
    their sample indices in `good`)."""
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
    n_iter = 0
    for r in range(1, max_iter + 1):
        C = cost_matrices(v, ref, scale)
        finite = np.isfinite(C).all(axis=(1, 2))
        perm = np.tile(np.arange(K), (len(good), 1))
        tot = np.full(len(good), np.nan)
        if finite.any():
            perm[finite], tot[finite] = solver(C[finite])
        n_changed = int((perm != prev).any(axis=1).sum())
        prev = perm
        if r > 1 and n_changed == 0:
            n_iter = r
            break
        if r == max_iter:
            n_iter = r
            break
        moved = np.take_along_axis(v, perm[:, :, None], axis=1)
        ref = moved.mean(axis=0) if len(good) else np.full((K, q), np.nan)
    moved = np.take_along_axis(v, perm[:, :, None], axis=1)
    with np.errstate(all="ignore"):
        mean = moved.mean(axis=0) if len(good) else np.full((K, q), np.nan)
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
