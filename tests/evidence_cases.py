"""What the evidence tests share (tests/test_gpu_evidence.py, tests/test_gpu_evidence_limits.py and the CPU controls of
tests/test_evidence_limits.py): the region dict of an oracle Region, the comparison of the device's ln L / ln pi with the
oracle, the synthetic regions, the one-region cases at the structural limits of libvamp_evid.so, the restated LDS size of
k_evid_steps, and the bar of the block standard error."""
import numpy as np

import evidence_ref as ref
from oracle import vamp_oracle as vo

SEED = 0x5EED0123456789
DTAB_N = 44                      # vamp::DTAB_N of voigt_math.hpp: the near-axis table of one Voigt line
REC = 7                          # kRec of evidence.hip: doubles of a line record
DEFAULT_LDS = 64 * 1024          # what a launch gets without hipFuncSetAttribute(MaxDynamicSharedMemorySize)


def as_dict(R, region_id=0, bounds=True):
    d = {"x": R.x, "flux": R.flux, "noise": None if R.sample_sd else R.noise, "n_comp": R.n_comp, "mode": R.mode, "sample_sd": R.sample_sd,
         "region_id": region_id}
    if bounds:
        d["bounds"] = (R.c_lo, R.c_hi, R.sigma_max, R.fwhm_max)
    return d


def check_lnlike(R, theta, bounds, tag):
    from vamp_amd import evidence
    got_ll, got_lp = evidence.lnlike(as_dict(R, bounds=bounds), theta)
    want_ll, want_lp = ref.lnlike_batch(R, theta)
    inside = want_lp > -np.inf
    assert np.array_equal(got_lp > -np.inf, inside), tag
    assert np.all(got_lp[~inside] == -np.inf) and np.all(np.isnan(got_ll[~inside])), tag
    err = np.abs(got_lp[inside] - want_lp[inside]) / np.maximum(1.0, np.abs(want_lp[inside]))
    assert err.size == 0 or err.max() <= 1e-9, (tag, "lnprior", err.max())
    fin = np.isfinite(want_ll) & inside
    assert np.array_equal(np.isfinite(got_ll) & inside, fin), tag
    assert np.all(got_ll[inside & ~fin] == -np.inf), tag
    err = np.abs(got_ll[fin] - want_ll[fin]) / np.maximum(1.0, np.abs(want_ll[fin]))
    assert err.size == 0 or err.max() <= 1e-9, (tag, "lnlike", err.max())
    return int(fin.sum())


def synthetic(P, K, mode, sd, descending=False, seed=0):
    """a region of P pixels with K lines and 40 parameter vectors: prior draws, some pushed outside the prior"""
    rng = np.random.default_rng(100 * P + 10 * K + mode + seed)
    x = np.arange(float(P)) - 0.37 * P
    lo, hi = (x[0], x[-1]) if P > 1 else (-3.0, 3.0)
    lines = [(rng.uniform(0.3, 2.0), rng.uniform(lo, hi), rng.uniform(0.5, 3.0)) for _ in range(K)]
    flux = np.exp(-sum(vo.gauss_function(x, *ln) for ln in lines)) + 0.05 * rng.standard_normal(P)
    if descending:
        x, flux = x[::-1].copy(), flux[::-1].copy()
    smax = (hi - lo) / 2.0
    R = ref.make_region(x, flux, np.full(P, 0.05), K, mode, sd, bounds=(lo, hi, smax, smax * 2 * np.sqrt(2 * np.log(2.0))))
    theta = np.concatenate([ref.prior_draws(R, 7 + j, 10, SEED) for j in range(4)])
    theta[3, 0] = -0.1                      # A < 0
    theta[5, 1] = hi + 1.0                  # c outside
    theta[8, R.q - 1] = 1.01 * (R.sigma_max if mode == 0 else R.fwhm_max)
    if sd:
        theta[11, -1] = 1.5
    theta[13, 2] *= 1e-3                    # a very narrow line
    return R, theta


def limit_region(P, K, mode, sd):
    """one region of the cases at the limits: x centred on 0, K Gaussian lines, noise 0.05, derived bounds"""
    rng = np.random.default_rng(5 + 100 * P + K)
    x = np.arange(float(P)) - 0.5 * (P - 1)
    lines = [(rng.uniform(0.4, 1.5), rng.uniform(x[0], x[-1]), rng.uniform(1.0, 4.0)) for _ in range(K)]
    flux = np.exp(-sum(vo.gauss_function(x, *ln) for ln in lines)) + 0.05 * rng.standard_normal(P)
    return ref.make_region(x, flux, np.full(P, 0.05), K, mode, sd)


# name -> P, K, mode, sd, T (or the ladder itself), W, steps, burn, swap_every, region_id, a
LIMIT_CASES = {
    "big-lds": (40, 8, 1, True, 2, 256, 2, 0, 1, 7, 2.0),                # 85 808 B of dynamic LDS: raise_lds_limit, 32 rounds per half
    "just-under": (33, 8, 0, False, 2, 256, 2, 0, 1, 7, 2.0),            # 55 824 B: no raise; 64 lanes at P = 33
    "narrow-w34": (24, 2, 0, False, 3, 34, 4, 1, 2, 7, 2.0),             # 17 movers on the 16 slots of 16 lanes: a second round of one
    "narrow-w40": (24, 2, 0, False, 3, 40, 4, 1, 2, 7, 2.0),             # 20 movers: a second round of four
    "narrow-w66": (24, 2, 0, False, 3, 66, 4, 1, 2, 7, 2.0),             # 33 movers: a third round of one
    "narrow-corner": (32, 4, 1, True, 3, 66, 3, 0, 2, 7, 2.0),           # P = 32, K = 4: the last narrow shape, D = 17 on 16 lanes
    "ladder-64": (17, 1, 0, False, 64, 4, 11, 2, 3, 7, 2.0),             # T at its limit, launches of 3, 3, 3, 2 steps, burn off the swap grid
    "ladder-33": (17, 2, 1, True, 33, 6, 12, 3, 5, 7, 2.0),              # odd T, launches of 5, 5, 2 steps, n_keep = 9
    "high-id": (17, 1, 0, False, 5, 24, 6, 0, 2, (2 ** 31 - 1) // 5 - 1, 2.0),      # walker ids above 2^32 in every draw key
    "own-ladder": (65, 2, 1, True, (0.0, 0.01, 0.3, 1.0), 10, 9, 1, 4, 7, 1.5),      # the caller's betas, a = 1.5, n_keep = 8 exactly
}


def limit_case(name):
    """-> (Region, betas, W, steps, burn, swap_every, region_id, a)"""
    P, K, mode, sd, T, W, steps, burn, swap_every, rid, a = LIMIT_CASES[name]
    betas = ref.default_betas(T) if isinstance(T, int) else np.array(T, dtype=np.float64)
    return limit_region(P, K, mode, sd), betas, W, steps, burn, swap_every, rid, a


def steps_lds_bytes(P, K, mode, sd, W):
    """dynamic LDS of a k_evid_steps launch for one region: the head, the rung's [W, D] state with ln L and ln pi, then one
    slot (proposal, line records, near-axis tables) per group of lanes that owns a mover"""
    q = 4 if mode == 1 else 3
    D = q * K + int(bool(sd))
    lanes = 16 if (P <= 32 and K <= 4) else 64
    slot_doubles = D + K * REC + (K * DTAB_N if mode == 1 else 0)
    return 8 * (2 + W * (D + 2)) + 8 * 4 * (64 // lanes) * slot_doubles


def se_bar(zb_ref):
    """the bar of lnZ_se.  Each block estimate zb is the functional ln Z is (a sum of max-shifted log mean exp), so by the
    project's bar of ln Z the device's zb agrees with the restatement's to 1e-9 max(1, |zb|).  The standard error is the
    sample standard deviation of the 8 values over sqrt 8, s / sqrt 8 with s = |zb - mean| / sqrt 7; s is 1 / sqrt 7-Lipschitz
    in the centred vector, whose norm moves by at most |delta zb| <= sqrt 8 max |delta zb|.  So the standard error moves by at
    most max |delta zb| / sqrt 7 < 1e-9 max(1, max_b |zb|): the bar."""
    return 1e-9 * max(1.0, float(np.max(np.abs(zb_ref))))
