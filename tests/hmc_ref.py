"""Numpy restatement of preconditioned HMC (include/vamp_hmc.h): the yardstick of tests/test_hmc.py
and tests/test_gpu_hmc.py, written once for both.  The draws are the oracle's Philox, ln p is evidence_ref.lnlike_lnprior
(the oracle's log_prior and log_like), the gradient is fisher_ref's (scipy's wofz and the identity for w').

``run(case, plant=None)`` is the whole call for one group; ``plant`` switches on one deliberate error.  ``check(got, case)``
holds a result -- the library's, or a planted restatement's -- to the restatement evaluated on the result's OWN outputs of
the stage before, so that each stage answers for its own arithmetic only.  The state a step starts from is rebuilt from
the result's own ``acc`` and ``prop`` (the last accepted proposal, or the start), its momentum is the result's ``mom``:

    mom        against the restated draws                                  32 eps max(1, rho)   (laplace_ref's bar on z)
    prop, prop_mom, dH   one restated step from (state, mom_got)           L = 1: ``step_bars``; L > 1: ``measured_bars``
    acc        walls exactly where the restated step has them; accept decisions wherever |log u - dH_ref| > 1e-6
    chain, last   the rebuilt states on the kept grid                      bit for bit (they are copies)
    lnp        ln p at the kept states against the oracle                  1e-9 max(1, |value|)
    counts     n_accept, n_wall from acc exactly; dH_mean, dH_max from dH_got to (n + 2) eps

The first-order bars of one leapfrog step (L = 1), ``step_bars``.  With gb(theta) the bar on the gradient at theta --
fisher_ref.bar_grad at b = 1e-10, the widest evaluator bar the Fisher tests grant (fisher_ref.bar_b), plus
fisher_ref.bar_prior, and for the free sd's entry 2 e_lnp / sd + 8 eps (chi2 / sd + P / sd) with e_lnp = 1e-9 max(1, |ln L|),
because d(grad_sd) = d(chi2_raw) / sd^3 and -chi2_raw / (2 sd^2) is a term of ln L -- and n = D + 2 roundings per fma
chain of D terms:
    p_half = p + (eps / 2) C^T g(theta):        e_half  = (eps / 2) |C^T| gb(theta) + n eps_m (eps / 2) |C^T| |g| + eps_m |p|
    theta' = theta + eps C p_half:              e_theta = eps |C| e_half + n eps_m eps |C| |p_half| + eps_m |theta|
    p' = p_half + (eps / 2) C^T g(theta'):      e_mom   = e_half + (eps / 2) |C^T| (gb(theta') + |H_gn| e_theta) + n eps_m (eps / 2) |C^T| |g'| + eps_m |p_half|
    dH = (ln p' - |p'|^2 / 2) - (ln p - |p|^2 / 2):
                                                e_dH    = 1e-9 (max(1, |ln p'|) + max(1, |ln p|)) + |g'| . e_theta + |p'| . e_mom
                                                          + n eps_m (|p'|^2 + |p|^2)
where |H_gn| e_theta, the movement of g' with theta', is bounded by a central difference of the restated gradient along
e_theta (it is second order and far below the other terms; it is there so that the bar is closed).  eps_t itself carries
4 eps_m relative, which multiplies every term with eps and is added.

The bars of L > 1, ``measured_bars``: the float64 restatement against the same restatement with the integrator in
np.longdouble and every gradient perturbed by +-gb (all plus, all minus, two random sign patterns), at the test's own
cases, starts and restated momenta; the bar is four times the worst difference per quantity (theta' relative to the
metric's scale sqrt(diag C C^T), p' and dH absolute), the factor 4 covering the kernel's other order of summation.
profiles/hmc_limits.txt holds the values (``python tests/hmc_ref.py`` prints them)."""
import math

import numpy as np

import evidence_ref
import fisher_ref
from oracle import vamp_oracle as vo

STREAM_MOMENTUM, STREAM_HMC_ACCEPT = 6, 7
EPS = 2.0 ** -52
Z_BAR_ULPS = 32.0
B_EVAL = 1e-10                # the evaluator's bar on J (the top of fisher_ref.bar_b's range)
LNP_REL = 1e-9                # the evidence tests' bar on ln p
DECISION_GAP = 1e-6           # accept decisions are compared where |log u - dH| exceeds this
MAX_UNDECIDED = 0.01          # at most this share of a case's steps may be left out
MEASURED_FACTOR = 4.0
PLANTS = ("C for C^T", "a full first momentum step", "the last z dropped at even D", "a stale g after a rejection", "a shifted thin grid")
# "H0 from the previous proposal": ln p of the previous proposal stands in H0 for the state's, also after a rejection
BROKEN = ("accept always", "dH without the kinetic terms", "H0 from the previous proposal")
LD = np.longdouble
_M = vo.MASK32


def make_case(x, flux, noise, n_comp, mode, start, chol, eps, n_leap, n_steps, seed, jitter=0.0, n_burn=0, thin=1, step0=0, region_id=0,
              chain_id0=0, bounds=None):
    """one group of a call with the call's parameters; ``noise`` None = free sd; ``start`` [C, D]"""
    return {"x": np.asarray(x, dtype=np.float64), "flux": np.asarray(flux, dtype=np.float64),
            "noise": None if noise is None else np.asarray(noise, dtype=np.float64), "n_comp": int(n_comp), "mode": int(mode),
            "sample_sd": noise is None, "start": np.atleast_2d(np.asarray(start, dtype=np.float64)).copy(),
            "chol": np.asarray(chol, dtype=np.float64), "eps": float(eps), "jitter": float(jitter), "L": int(n_leap), "n_steps": int(n_steps),
            "n_burn": int(n_burn), "thin": int(thin), "step0": int(step0), "seed": int(seed), "region_id": int(region_id),
            "chain_id0": int(chain_id0), "bounds": None if bounds is None else tuple(bounds)}


def region_of(case):
    if "_region" not in case:
        case["_region"] = evidence_ref.make_region(case["x"], case["flux"], case["noise"], case["n_comp"], case["mode"], case["sample_sd"],
                                                   case["bounds"])
    return case["_region"]


def kept_steps(n_steps, n_burn, thin, plant=None):
    shift = 1 if plant == "a shifted thin grid" else 0
    return [t for t in range(n_steps) if t >= n_burn + shift and (t - n_burn - shift) % thin == 0]


# ---- the draws ----------------------------------------------------------------------------------------------------
def _u53(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def momentum_draws(steps, chains, D, region_id, seed, plant=None):
    """(z [T, C, D], rho [T, C, D]) for the absolute steps ``steps`` and the chain identities ``chains``: counter
    {T, c 64 + j, STREAM_MOMENTUM, region_id}, key (seed lo, seed hi), through the oracle's vectorised Philox"""
    npair = (D + 1) // 2
    t, c, j = np.meshgrid(np.asarray(steps, dtype=np.uint64), np.asarray(chains, dtype=np.uint64), np.arange(npair, dtype=np.uint64), indexing="ij")
    c0, c1, c2, c3 = vo._philox_vec(t, c * np.uint64(64) + j, STREAM_MOMENTUM, region_id, seed & _M, (seed >> 32) & _M)
    u1, u2 = 1.0 - _u53(c0, c1), _u53(c2, c3)
    rho = np.sqrt(-2.0 * np.log(u1))
    a = (2.0 * np.pi) * u2
    z = np.stack([rho * np.cos(a), rho * np.sin(a)], axis=3).reshape(t.shape[0], t.shape[1], 2 * npair)
    if plant == "the last z dropped at even D" and D % 2 == 0:
        z[:, :, D - 1] = 0.0
    return np.ascontiguousarray(z[:, :, :D]), np.repeat(rho, 2, axis=2)[:, :, :D]


def accept_draws(steps, chains, region_id, seed):
    """(u in (0, 1] [T, C], u' in [0, 1) [T, C]): counter {T, c 64 + 63, STREAM_HMC_ACCEPT, region_id}"""
    t, c = np.meshgrid(np.asarray(steps, dtype=np.uint64), np.asarray(chains, dtype=np.uint64), indexing="ij")
    c0, c1, c2, c3 = vo._philox_vec(t, c * np.uint64(64) + np.uint64(63), STREAM_HMC_ACCEPT, region_id, seed & _M, (seed >> 32) & _M)
    return 1.0 - _u53(c0, c1), _u53(c2, c3)


def step_sizes(case, uprime):
    return case["eps"] * (1.0 + case["jitter"] * (2.0 * uprime - 1.0))


# ---- the target ---------------------------------------------------------------------------------------------------
def target(case, theta):
    """ln p = ln pi + ln L of one vector, or -inf for a rejected point (outside the prior, or no finite ln L)"""
    ll, lp = evidence_ref.lnlike_lnprior(region_of(case), np.asarray(theta, dtype=np.float64))
    return lp + ll if lp > -np.inf and np.isfinite(ll) else -np.inf


def value_and_grad(case, theta, with_bar=False):
    """(ln p, grad [D]) at one vector -- grad is vamp_fisher.h's with with_prior = 1 -- or (-inf, None) for a rejected
    point; ``with_bar``: also gb [D], the bar on the gradient (this module's docstring)"""
    theta = np.asarray(theta, dtype=np.float64)
    lnp = target(case, theta)
    if not np.isfinite(lnp):
        return (-np.inf, None, None) if with_bar else (-np.inf, None)
    K, mode, sd = case["n_comp"], case["mode"], case["sample_sd"]
    with np.errstate(all="ignore"):
        f, J = fisher_ref.jacobian(case["x"], theta, K, mode, sd)
        o = fisher_ref.from_jacobian(J, f, case["flux"], case["noise"], theta, K, mode)
    if not with_bar:
        return lnp, o["grad"]
    D, P = theta.size, len(case["x"])
    gb = fisher_ref.bar_grad(o["a"], o["rs"], B_EVAL) + fisher_ref.bar_prior(theta, K, mode, D)[0]
    if sd:
        s = theta[-1]
        ll = lnp - vo.log_prior(region_of(case), theta)
        gb[-1] = 2.0 * LNP_REL * max(1.0, abs(ll)) / s + 8 * EPS * (o["chi2"] / s + P / s)
    return lnp, o["grad"], gb


# ---- one step -------------------------------------------------------------------------------------------------------
def leapfrog(case, theta, lnp, g, p, eps, dtype=np.float64, plant=None, perturb=None):
    """the trajectory of one step from the state (theta, ln p, g) with momentum p and step size eps: a dict with theta',
    p', ln p', g', dH and ``wall``.  The integrator's arithmetic is in ``dtype`` (the target itself is fp64);
    ``perturb(gb)`` returns what is added to every evaluated gradient (``measured_bars``)."""
    T = dtype
    C = np.tril(case["chol"]).astype(T)
    kickM = C if plant == "C for C^T" else C.T
    L = case["L"]
    th, p, eps = np.asarray(theta, dtype=T).copy(), np.asarray(p, dtype=T).copy(), T(eps)
    H0 = T(lnp) - T(0.5) * np.sum(p * p)
    p = p + (eps if plant == "a full first momentum step" else eps / 2) * (kickM @ np.asarray(g, dtype=T))
    lnpn, gn = None, None
    for l in range(L):
        th = th + eps * (C @ p)
        if perturb is None:
            lnpn, gn = value_and_grad(case, np.asarray(th, dtype=np.float64))
        else:
            lnpn, gn, gb = value_and_grad(case, np.asarray(th, dtype=np.float64), with_bar=True)
            gn = None if gn is None else np.asarray(gn, dtype=T) + perturb(gb)
        if gn is None:
            return {"theta": np.asarray(th, dtype=np.float64), "p": np.asarray(p, dtype=np.float64), "wall": True, "dH": np.nan, "lnp": -np.inf, "g": None}
        p = p + (eps if l + 1 < L else eps / 2) * (kickM @ np.asarray(gn, dtype=T))
    dH = (T(lnpn) - T(0.5) * np.sum(p * p)) - H0
    return {"theta": np.asarray(th, dtype=np.float64) if T is np.float64 else th, "p": np.asarray(p, dtype=np.float64) if T is np.float64 else p,
            "wall": False, "dH": float(dH) if T is np.float64 else dH, "lnp": lnpn, "g": gn}


def run(case, plant=None, broken=None, mom_in=None):
    """the whole call for one group: a dict with the library's outputs (include/vamp_hmc.h), fp64.  ``broken``: one of
    BROKEN, a move that does not leave the target invariant (tests/test_hmc.py)"""
    start, D = case["start"], case["start"].shape[1]
    nC, n_steps = start.shape[0], case["n_steps"]
    keep = kept_steps(n_steps, case["n_burn"], case["thin"], plant)
    n_keep = len(kept_steps(n_steps, case["n_burn"], case["thin"]))
    steps = case["step0"] + np.arange(n_steps)
    ids = case["chain_id0"] + np.arange(nC)
    out = {"chain": np.full((n_keep, nC, D), np.nan), "lnp": np.full((n_keep, nC), np.nan), "last": np.full((nC, D), np.nan),
           "mom": np.full((n_steps, nC, D), np.nan), "prop": np.full((n_steps, nC, D), np.nan), "prop_mom": np.full((n_steps, nC, D), np.nan),
           "dH": np.full((n_steps, nC), np.nan), "acc": np.zeros((n_steps, nC), dtype=np.int32), "n_accept": np.zeros(nC, dtype=np.int32),
           "n_wall": np.zeros(nC, dtype=np.int32), "dH_mean": np.full(nC, np.nan), "dH_max": np.full(nC, np.nan),
           "chain_status": np.zeros(nC, dtype=np.int32), "status": 0}
    low = np.tril(case["chol"])
    if not (np.isfinite(low).all() and np.all(np.diag(low) > 0) and np.isfinite(case["eps"]) and case["eps"] > 0 and 0 <= case["jitter"] < 1):
        out["status"] = 1
        out["chain_status"][:] = 1
        return out
    z = momentum_draws(steps, ids, D, case["region_id"], case["seed"], plant)[0] if mom_in is None else np.asarray(mom_in, dtype=np.float64)
    u, up = accept_draws(steps, ids, case["region_id"], case["seed"])
    eps = step_sizes(case, up)
    for c in range(nC):
        th = start[c].copy()
        lnp, g = value_and_grad(case, th)
        if g is None:
            out["chain_status"][c] = 2
            continue
        kept, prev = 0, None
        absdh = []
        for t in range(n_steps):
            p0 = z[t, c]
            tr = leapfrog(case, th, lnp, g, p0, eps[t, c], plant=plant)
            out["mom"][t, c], out["prop"][t, c], out["prop_mom"][t, c] = p0, tr["theta"], tr["p"]
            dH = tr["dH"]
            if not tr["wall"]:
                if broken == "dH without the kinetic terms":
                    dH = tr["lnp"] - lnp
                elif broken == "H0 from the previous proposal" and prev is not None:
                    dH = (tr["lnp"] - 0.5 * float(np.sum(tr["p"] ** 2))) - (prev - 0.5 * float(np.sum(p0 ** 2)))
                prev = tr["lnp"]
                absdh.append(abs(dH))
            out["dH"][t, c] = dH
            accept = (not tr["wall"]) and (broken == "accept always" or math.log(u[t, c]) < dH)
            out["acc"][t, c] = 2 if tr["wall"] else int(accept)
            if accept:
                th, lnp, g = tr["theta"], tr["lnp"], tr["g"]
            elif plant == "a stale g after a rejection" and not tr["wall"]:
                g = tr["g"]
            if t in keep and kept < n_keep:
                out["chain"][kept, c], out["lnp"][kept, c] = th, lnp
                kept += 1
        out["last"][c] = th
        out["n_accept"][c] = int(np.sum(out["acc"][:, c] == 1))
        out["n_wall"][c] = int(np.sum(out["acc"][:, c] == 2))
        if absdh:
            out["dH_mean"][c], out["dH_max"][c] = float(np.sum(absdh)) / len(absdh), float(np.max(absdh))
    return out


# ---- the bars -------------------------------------------------------------------------------------------------------
def step_bars(case, theta, lnp, g, gb, p, eps, tr):
    """(e_theta [D], e_mom [D], e_dH) of one L = 1 step ``tr`` = leapfrog(...) from (theta, ln p, g) with the bar gb on g"""
    C = np.abs(np.tril(case["chol"]))
    D = theta.size
    n = D + 2
    h = 0.5 * eps
    p_half = p + h * (np.tril(case["chol"]).T @ g)
    e_half = h * (C.T @ gb) + n * EPS * h * (C.T @ np.abs(g)) + EPS * np.abs(p)
    e_theta = eps * (C @ e_half) + n * EPS * eps * (C @ np.abs(p_half)) + EPS * np.abs(theta)
    _, gn, gbn = value_and_grad(case, tr["theta"], with_bar=True)
    moved = np.zeros(D)
    lo, hi = value_and_grad(case, tr["theta"] - e_theta)[1], value_and_grad(case, tr["theta"] + e_theta)[1]
    if lo is not None and hi is not None:
        moved = np.abs(hi - lo)
    e_mom = e_half + h * (C.T @ (gbn + moved)) + n * EPS * h * (C.T @ np.abs(gn)) + EPS * np.abs(p_half)
    e_dH = LNP_REL * (max(1.0, abs(tr["lnp"])) + max(1.0, abs(lnp))) + float(np.abs(gn) @ e_theta) + float(np.abs(tr["p"]) @ e_mom) \
        + n * EPS * float(np.sum(tr["p"] ** 2) + np.sum(p ** 2))
    rel = 1.0 + 4 * EPS
    return e_theta * rel + 4 * EPS * np.abs(tr["theta"] - theta), e_mom * rel + 4 * EPS * np.abs(tr["p"] - p), e_dH * rel


def metric_scale(case):
    low = np.tril(case["chol"])
    return np.sqrt(np.sum(low * low, axis=1))


def measured_bars(case, n_steps=None):
    """{"prop": relative to metric_scale, "prop_mom": absolute, "dH": absolute, "worst": the three worst differences}: four
    times the worst difference between the fp64 restatement and the longdouble one with perturbed gradients, over the
    case's chains and its first ``n_steps`` steps, every step from the fp64 restatement's own state and momentum"""
    start, D = case["start"], case["start"].shape[1]
    nC = start.shape[0]
    n_steps = case["n_steps"] if n_steps is None else n_steps
    steps = case["step0"] + np.arange(n_steps)
    ids = case["chain_id0"] + np.arange(nC)
    z = momentum_draws(steps, ids, D, case["region_id"], case["seed"])[0]
    u, up = accept_draws(steps, ids, case["region_id"], case["seed"])
    eps = step_sizes(case, up)
    rng = np.random.default_rng(12345)
    signs = [lambda gb: gb, lambda gb: -gb, lambda gb: gb * rng.choice([-1.0, 1.0], gb.size), lambda gb: gb * rng.choice([-1.0, 1.0], gb.size)]
    scale = metric_scale(case)
    worst = {"prop": 0.0, "prop_mom": 0.0, "dH": 0.0}
    for c in range(nC):
        th = start[c].copy()
        lnp, g, gb = value_and_grad(case, th, with_bar=True)
        if g is None:
            continue
        for t in range(n_steps):
            tr = leapfrog(case, th, lnp, g, z[t, c], eps[t, c])
            if not tr["wall"]:
                for s in signs:
                    hi = leapfrog(case, th, lnp, np.asarray(g, dtype=LD) + s(gb), z[t, c], eps[t, c], dtype=LD, perturb=s)
                    if hi["wall"]:
                        continue
                    worst["prop"] = max(worst["prop"], float(np.max(np.abs(hi["theta"] - tr["theta"]) / scale)))
                    worst["prop_mom"] = max(worst["prop_mom"], float(np.max(np.abs(hi["p"] - tr["p"]))))
                    worst["dH"] = max(worst["dH"], float(abs(hi["dH"] - tr["dH"])))
                if math.log(u[t, c]) < tr["dH"]:
                    th, lnp, g = tr["theta"], tr["lnp"], tr["g"]
                    gb = value_and_grad(case, th, with_bar=True)[2]
    return {"prop": MEASURED_FACTOR * worst["prop"], "prop_mom": MEASURED_FACTOR * worst["prop_mom"], "dH": MEASURED_FACTOR * worst["dH"],
            "worst": worst}


# ---- the check ------------------------------------------------------------------------------------------------------
def _ratio(err, bar):
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf)), initial=0.0))


def _bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check(got, case, label="", bars=None, mom_in=None):
    """asserts one group's result ``got`` (dict of the header's outputs, every trace included) against the restatement on
    its own outputs of the stage before; returns the worst error / bar per stage (dict), and under "undecided" the share
    of steps whose accept decision was too close to compare.  ``bars``: ``measured_bars`` of the case (needed when L > 1);
    ``mom_in``: the momenta the call was given in place of the draws.  Each assertion's message opens with the stage's name."""
    start, D = case["start"], case["start"].shape[1]
    nC, n_steps, L = start.shape[0], case["n_steps"], case["L"]
    worst = {}
    want_status = run(dict(case, n_steps=1, n_burn=0, start=start[:1]))["status"]
    assert got["status"] == want_status, (label, "status", got["status"], want_status)
    if want_status == 1:
        for k in ("chain", "lnp", "last", "mom", "prop", "prop_mom", "dH", "dH_mean", "dH_max"):
            assert np.all(np.isnan(got[k])), (label, "status 1", k)
        assert np.all(got["chain_status"] == 1) and not np.any(got["acc"]) and not np.any(got["n_accept"]) and not np.any(got["n_wall"]), \
            (label, "status 1", "counts")
        return worst
    assert L == 1 or bars is not None, "measured bars are needed when L > 1"
    steps = case["step0"] + np.arange(n_steps)
    ids = case["chain_id0"] + np.arange(nC)
    u, up = accept_draws(steps, ids, case["region_id"], case["seed"])
    eps = step_sizes(case, up)
    keep = kept_steps(n_steps, case["n_burn"], case["thin"])
    scale = metric_scale(case)
    live = []
    for c in range(nC):
        lnp0 = target(case, start[c])
        if not np.isfinite(lnp0):
            assert got["chain_status"][c] == 2, (label, "chain_status", c, got["chain_status"][c])
            for k in ("chain", "lnp", "mom", "prop", "prop_mom", "dH"):
                assert np.all(np.isnan(got[k][:, c])), (label, "status 2", k, c)
            assert np.all(np.isnan(got["last"][c])) and np.isnan(got["dH_mean"][c]) and np.isnan(got["dH_max"][c]), (label, "status 2", "last", c)
            assert not np.any(got["acc"][:, c]) and got["n_accept"][c] == 0 and got["n_wall"][c] == 0, (label, "status 2", "counts", c)
        else:
            assert got["chain_status"][c] == 0, (label, "chain_status", c, got["chain_status"][c])
            live.append(c)
    # the momenta
    if mom_in is None:
        z_ref, rho = momentum_draws(steps, ids, D, case["region_id"], case["seed"])
        worst["mom"] = _ratio(np.abs(got["mom"][:, live] - z_ref[:, live]), Z_BAR_ULPS * EPS * np.maximum(1.0, rho[:, live]))
        assert worst["mom"] <= 1.0, (label, "mom", worst["mom"])
    else:
        assert _bits(got["mom"][:, live], np.asarray(mom_in)[:, live]), (label, "mom", "not the given momenta")
    worst.update(prop=0.0, prop_mom=0.0, dH=0.0, lnp=0.0)
    undecided = 0
    for c in live:
        th = start[c].copy()
        lnp, g, gb = value_and_grad(case, th, with_bar=True)
        kept = 0
        for t in range(n_steps):
            p0 = got["mom"][t, c]
            tr = leapfrog(case, th, lnp, g, p0, eps[t, c])
            assert (got["acc"][t, c] == 2) == tr["wall"], (label, "acc", "wall", c, t, int(got["acc"][t, c]), tr["wall"])
            if tr["wall"]:
                assert np.isnan(got["dH"][t, c]), (label, "dH", "not NaN at a wall", c, t)
            else:
                if L == 1:
                    e_th, e_p, e_dh = step_bars(case, th, lnp, g, gb, p0, eps[t, c], tr)
                else:
                    e_th, e_p, e_dh = bars["prop"] * scale, bars["prop_mom"], bars["dH"]
                r = _ratio(np.abs(got["prop"][t, c] - tr["theta"]), e_th)
                assert r <= 1.0, (label, "prop", c, t, r)
                worst["prop"] = max(worst["prop"], r)
                r = _ratio(np.abs(got["prop_mom"][t, c] - tr["p"]), e_p)
                assert r <= 1.0, (label, "prop_mom", c, t, r)
                worst["prop_mom"] = max(worst["prop_mom"], r)
                r = _ratio(abs(got["dH"][t, c] - tr["dH"]), e_dh)
                assert r <= 1.0, (label, "dH", c, t, r, got["dH"][t, c], tr["dH"])
                worst["dH"] = max(worst["dH"], r)
                logu = math.log(u[t, c])
                if abs(logu - tr["dH"]) > DECISION_GAP:
                    assert got["acc"][t, c] == int(logu < tr["dH"]), (label, "acc", "decision", c, t, int(got["acc"][t, c]), logu, tr["dH"])
                else:
                    undecided += 1
                    assert got["acc"][t, c] in (0, 1), (label, "acc", "value", c, t)
                if got["acc"][t, c] == 1:                          # the library's own proposal is the next state
                    th = got["prop"][t, c].copy()
                    lnp, g, gb = value_and_grad(case, th, with_bar=True)
                    assert g is not None, (label, "acc", "an accepted proposal the target rejects", c, t)
            if t in keep:
                assert _bits(got["chain"][kept, c], th), (label, "chain", "not the state after step", c, t)
                r = abs(got["lnp"][kept, c] - lnp) / (LNP_REL * max(1.0, abs(lnp)))
                assert r <= 1.0, (label, "lnp", c, t, r)
                worst["lnp"] = max(worst["lnp"], r)
                kept += 1
        assert kept == got["chain"].shape[0], (label, "chain", "n_keep", kept, got["chain"].shape[0])
        assert _bits(got["last"][c], th), (label, "last", c)
        a = got["acc"][:, c]
        assert got["n_accept"][c] == int(np.sum(a == 1)) and got["n_wall"][c] == int(np.sum(a == 2)), (label, "counts", c)
        free = np.abs(got["dH"][a != 2, c])
        if free.size:
            tol = (free.size + 2) * EPS
            assert abs(got["dH_mean"][c] - float(np.sum(free.astype(LD)) / free.size)) <= tol * float(np.mean(free)) + 1e-300, (label, "counts", "dH_mean", c)
            assert got["dH_max"][c] == float(np.max(free)), (label, "counts", "dH_max", c)
        else:
            assert np.isnan(got["dH_mean"][c]) and np.isnan(got["dH_max"][c]), (label, "counts", "dH of walls only", c)
    worst["undecided"] = undecided / max(1, len(live) * n_steps)
    assert worst["undecided"] <= MAX_UNDECIDED, (label, "acc", "too many decisions too close to compare", worst["undecided"])
    return worst


# ---- the inputs the tests share ----------------------------------------------------------------------------------
NOISE = 0.05                  # of ``lines_data``


def lines_data(P, K, mode, sd, seed_shift=0):
    """(x, flux, noise or None, theta) of K well separated lines on P pixels, as tests/test_gpu_laplace.py's lines_case, at
    the noise NOISE"""
    rng = np.random.default_rng(1000 * P + 10 * K + mode + seed_shift)
    x = np.arange(float(P))
    cen = (np.arange(K) + 0.5) * P / K
    width = max(0.8, 0.12 * P / K)
    lines = [[0.6 + 0.05 * k, cen[k], width] if mode == 0 else [0.6 + 0.05 * k, cen[k], 0.4 * width, 1.8 * width] for k in range(K)]
    theta = np.array(lines).ravel()
    R = vo.Region(x=x, flux=np.ones(P), noise=np.ones(P), n_comp=K, mode=mode)
    flux = vo.model_flux(R, theta) + NOISE * rng.standard_normal(P)
    return x, flux, (None if sd else np.full(P, NOISE)), (np.append(theta, NOISE) if sd else theta)


def metric_at(x, flux, noise, theta, K, mode):
    """the lower Cholesky factor of the Fisher covariance at theta (fisher_ref), the metric the product uses"""
    f, J = fisher_ref.jacobian(x, theta, K, mode, noise is None)
    cov = fisher_ref.from_jacobian(J, f, flux, noise, theta, K, mode)["cov"]
    return np.linalg.cholesky(0.5 * (cov + cov.T))


def lines_case(P, K, mode, sd, n_chains, n_leap, n_steps, seed=5, eps=0.6, spread=0.5, **kw):
    """``lines_data`` with the full lower factor of tests/test_gpu_laplace.py's lines_case around the truth as the metric (the
    Fisher covariance of narrow blended lines is no metric: their posterior is a curved ridge), chains started at truth +
    spread C z (z from a seeded numpy generator)"""
    x, flux, noise, theta = lines_data(P, K, mode, sd)
    q = 4 if mode == 1 else 3
    D = theta.size
    rng = np.random.default_rng(7 + P + K)
    scale = np.tile([0.03, 0.05, 0.04, 0.04][:q], K)
    scale = np.append(scale, 0.004) if sd else scale
    chol = (np.tril(rng.uniform(-0.3, 0.3, (D, D)), -1) + np.eye(D)) * scale[:, None]
    start = theta + spread * rng.standard_normal((n_chains, D)) @ chol.T
    chol[np.triu_indices(D, 1)] = np.nan                      # the upper triangle is not read
    return make_case(x, flux, noise, K, mode, start, chol, eps, n_leap, n_steps, seed, **kw)


def from_record(rec, status=None):
    """a ``vamp_amd.hmc.HmcRecord`` made with every trace as the dict ``check`` takes"""
    out = {k: getattr(rec, k) for k in ("chain", "lnp", "last", "mom", "prop", "prop_mom", "dH", "acc", "n_wall", "dH_mean", "dH_max",
                                         "chain_status", "status")}
    out["n_accept"] = np.rint(rec.accept_rate * rec.n_steps).astype(np.int32)
    return out


if __name__ == "__main__":          # the figures of profiles/hmc_limits.txt
    import test_gpu_hmc
    for name, case in test_gpu_hmc.l8_cases().items():
        b = measured_bars(case)
        print(f"{name:28s} worst prop {b['worst']['prop']:.3e} prop_mom {b['worst']['prop_mom']:.3e} dH {b['worst']['dH']:.3e}   "
              f"bar prop {b['prop']:.3e} prop_mom {b['prop_mom']:.3e} dH {b['dH']:.3e}")


# ---- a vectorised HMC on the one-line Gaussian posterior of tests/sampler_stats.py (the invariance tests) -------------
def gauss_line_value_grad(post, X):
    """(ln p [N], grad [N, D]) of sampler_stats.GaussLinePosterior ``post`` at the rows of X, -inf (and a zero gradient)
    outside the prior: the closed form of one Gaussian line, vectorised over the rows; tests/test_hmc.py holds it to
    ``value_and_grad``"""
    X = np.asarray(X, dtype=np.float64)
    lnp = post.logp(X)
    ok = np.isfinite(lnp)
    A, c, s = X[:, 0:1], X[:, 1:2], X[:, 2:3]
    with np.errstate(all="ignore"):
        u = (post.x[None, :] - c) / s
        e = np.exp(-0.5 * u * u)
        m = np.exp(-A * e)
        r = post.flux[None, :] - m
        var = X[:, 3:4] ** 2 if post.sample_sd else post.noise_fixed[None, :] ** 2
        w = -m * r / var
        g = np.stack([np.sum(w * e, axis=1) + 1.0 / A[:, 0] - 1.0, np.sum(w * A * e * u / s, axis=1), np.sum(w * A * e * u * u / s, axis=1)], axis=1)
        if post.sample_sd:
            sd = X[:, 3]
            g = np.column_stack([g, np.sum(r * r, axis=1) / sd ** 3 - post.P / sd])
    return lnp, np.where(ok[:, None], g, 0.0)


def vector_hmc(post, X0, chol, eps, n_leap, n_steps, rng, jitter=0.0, broken=None):
    """``n_steps`` moves of the header's step for the N independent chains X0 [N, D] on ``post``, momenta and uniforms
    from ``rng``; ``broken``: one of BROKEN.  Returns (X [N, D], accepted steps per chain [N], walls per chain [N])"""
    C = np.tril(chol)
    X = np.array(X0, dtype=np.float64)
    lnp, g = gauss_line_value_grad(post, X)
    N = len(X)
    n_acc, n_wall = np.zeros(N), np.zeros(N)
    prev = None
    for _ in range(n_steps):
        p = p0 = rng.standard_normal(X.shape)
        e = (eps * (1.0 + jitter * (2.0 * rng.random(N) - 1.0)))[:, None]
        H0 = lnp - 0.5 * np.sum(p * p, axis=1)
        p = p + 0.5 * e * (g @ C)
        th, alive = X.copy(), np.ones(N, dtype=bool)
        lnpn, gn = lnp, g
        for l in range(n_leap):
            th = np.where(alive[:, None], th + e * (p @ C.T), th)
            lnpn, gn = gauss_line_value_grad(post, th)
            alive &= np.isfinite(lnpn)
            p = p + (1.0 if l + 1 < n_leap else 0.5) * e * (gn @ C)
        H1 = lnpn - 0.5 * np.sum(p * p, axis=1)
        dH = H1 - H0
        if broken == "dH without the kinetic terms":
            dH = lnpn - lnp
        elif broken == "H0 from the previous proposal" and prev is not None:
            dH = H1 - (prev - 0.5 * np.sum(p0 * p0, axis=1))
        prev = np.where(alive, lnpn, lnp)
        with np.errstate(all="ignore"):
            accept = alive & (np.ones(N, dtype=bool) if broken == "accept always" else np.log(1.0 - rng.random(N)) < dH)
        X = np.where(accept[:, None], th, X)
        lnp = np.where(accept, lnpn, lnp)
        g = np.where(accept[:, None], gn, g)
        n_acc += accept
        n_wall += ~alive
    return X, n_acc, n_wall


INVARIANCE = {False: dict(eps=1.32, n_leap=2, n_steps=60), True: dict(eps=0.95, n_leap=2, n_steps=60)}      # per sd form
INVARIANCE_SEED = 1
INVARIANCE_N = 4096


def invariance_leg(sample_sd):
    """(the posterior, exact starts [N, D], the metric's factor, the leg's eps / n_leap / n_steps) of one invariance leg:
    the metric is the Cholesky factor of the covariance of 20 000 further exact draws"""
    import sampler_stats
    post = sampler_stats.gauss_line_posterior(sample_sd, INVARIANCE_N)
    rng = np.random.default_rng(2024 + int(sample_sd))
    X0 = post.draw(INVARIANCE_N, rng)
    chol = np.linalg.cholesky(np.cov(post.draw(20000, rng).T))
    return post, X0, chol, INVARIANCE[bool(sample_sd)]


def ks_of(post, X):
    import sampler_stats
    return [sampler_stats.ks_lambda(X[:, d], post.cdf(d)) for d in range(X.shape[1])]


# ---- the cases of tests/test_gpu_hmc.py (tests/test_hmc.py shows on the CPU that no accept decision of theirs is too close) ----
CALLS = {1: dict(n_leap=1, n_steps=7, thin=3, n_burn=0, jitter=0.0),         # thin does not divide n_steps; n_burn = 0
         8: dict(n_leap=8, n_steps=5, thin=2, n_burn=4, jitter=0.5)}         # n_burn = n_steps - 1: one kept state
SHAPES = ("P1", "P63", "P64", "P65", "P129", "D3", "D4", "D48", "D65", "P32K4", "P32K5", "P33K4", "P33K5", "C1", "C4", "C5", "C9")


def shape_case(name, L, seed=5, region_id=1, chain_id0=0):
    """one of SHAPES with the call parameters CALLS[L]: P = 1, 63 | 64 | 65 (the tile), 129 (three tiles); D = 3, 4, 48 and 65
    (16 Voigt lines and the sd: 33 pairs, one z dropped; two rounds of lanes); P = 32 | 33 x K = 4 | 5; C = 1, 4 | 5 (a
    workgroup and one more), 9 -- three chains otherwise"""
    kw = dict(CALLS[L], seed=seed, region_id=region_id, chain_id0=chain_id0)
    L_, n = kw.pop("n_leap"), kw.pop("n_steps")
    if name == "P1":
        chol = np.linalg.cholesky(np.diag([0.1, 0.3, 0.2]) ** 2 + 0.001)
        start = np.array([0.9, 3.2, 1.5]) + 0.5 * np.random.default_rng(3).standard_normal((3, 3)) @ chol.T
        return make_case([3.0], [0.4], [0.1], 1, 0, start, chol, 0.3, L_, n, bounds=(0.0, 6.0, 3.0, 7.0), **kw)
    if name[0] == "P" and "K" not in name:
        return lines_case(int(name[1:]), 2, 1, True, 3, L_, n, **kw)
    if name[0] == "P":
        P, K = name[1:].split("K")
        return lines_case(int(P), int(K), 1, True, 3, L_, n, **kw)
    if name[0] == "C":
        return lines_case(40, 2, 0, True, int(name[1:]), L_, n, **kw)
    P, K, mode, sd = {"D3": (40, 1, 0, False), "D4": (40, 1, 0, True), "D48": (160, 12, 1, False), "D65": (200, 16, 1, True)}[name]
    c = lines_case(P, K, mode, sd, 3, L_, n, **kw)
    assert c["start"].shape[1] == int(name[1:])
    return c


def wall_case(n_steps=12, n_chains=4):
    """tests/laplace_ref.py's voigt_edge_case as chains: one Voigt line whose true L_fwhm is 0, so that the posterior leans on
    the lower bound; the chains start next to it and make one leapfrog step per move, and a proposal leaves the prior by
    the sign of one momentum, about every second time"""
    x = np.arange(24.0)
    flux = np.exp(-vo.voigt_function(x, 11.3, 1.2, 0.0, 5.0)) + 0.05 * np.random.default_rng(3).standard_normal(24)
    chol = np.linalg.cholesky(np.diag([0.05, 0.1, 0.3, 0.2]) ** 2 + 0.001)
    start = np.tile([1.2, 11.3, 0.002, 5.0], (n_chains, 1))
    return make_case(x, flux, np.full(24, 0.05), 1, 1, start, chol, 0.5, 1, n_steps, 11, region_id=4)


def decisions_case():
    """nine chains of 24 single-leap moves at a step size that has about every third proposal rejected"""
    return lines_case(40, 2, 0, True, 9, 1, 24, eps=1.5, seed=21, region_id=6)


def ratio_cases(eps=0.1):
    """[(case at eps with L = 4, case at eps / 2 with L = 8)] for Gauss and Voigt, fixed noise and free sd: the same
    trajectory time, one step, six chains; the restatement's |dH| ratios lie in 3.9 .. 4.02"""
    out = []
    for P, K, mode, sd in ((40, 2, 0, False), (40, 2, 0, True), (65, 2, 1, False), (65, 2, 1, True)):
        c = lines_case(P, K, mode, sd, 6, 4, 1, eps=eps)
        out.append((c, dict(c, L=8, eps=eps / 2)))
    return out
