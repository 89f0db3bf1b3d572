"""CPU controls of tests/test_gpu_evidence_limits.py (restatement only): the bar that test puts on the block standard error
can fail -- a block border one step off, or a kept step dropped, moves lnZ_se by more than 1000 bars --, the cases at the
limits are what their names say, and the restatement returns the block estimates the bar is built on."""
import math

import numpy as np
import pytest

import evidence_ref as ref
from evidence_cases import DEFAULT_LDS, LIMIT_CASES, limit_case, se_bar, steps_lds_bytes


def _trace(n_keep=83, T=16, W=32, seed=1):
    """ln L ~ N(mu_j, 0.5^2) per rung, mu rising with beta (test_reductions_on_a_known_trace, at the ladder of part 2), plus
    an offset of unit variance that a step's walkers share, as an ensemble that moves together has: without it a border moved
    across two steps that happen to resemble each other changes lnZ_se by only 16 bars"""
    rng = np.random.default_rng(seed)
    return np.linspace(-30.0, -5.0, T)[None, :, None] + 0.5 * rng.standard_normal((n_keep, T, W)) + rng.standard_normal((n_keep, 1, 1))


def test_reduce_returns_the_block_estimates():
    betas = ref.default_betas(16)
    tr = _trace()
    rec = ref.reduce(tr, betas)
    bd = ref.block_borders(83)
    assert bd == [0, 10, 20, 31, 41, 51, 62, 72, 83] and ref.block_borders(8) == list(range(9)) and ref.block_borders(15)[:4] == [0, 1, 3, 5]
    assert rec["zb"].shape == (8,)
    for b in range(8):
        assert rec["zb"][b] == ref.stepping_stone(tr[bd[b]:bd[b + 1]], betas)
    assert rec["lnZ_se"] == pytest.approx(np.std(rec["zb"], ddof=1) / math.sqrt(8.0), rel=1e-15)
    assert ref.reduce(tr[:7], betas)["zb"] is None and math.isnan(ref.reduce(tr[:7], betas)["lnZ_se"])
    again = ref.reduce(tr, betas, borders=bd)
    assert again["lnZ_se"] == rec["lnZ_se"]


def test_the_bar_of_the_standard_error_can_fail():
    """n_keep = 83 (unequal blocks): every single border moved by one step either way, and the last kept step dropped, each
    change lnZ_se by at least 1000 times the bar |se - se_ref| <= 1e-9 max(1, max |zb|) of the GPU test; so does the
    population deviation in place of the sample's.  What the bar allows stays inside it: every zb moved by its own
    1e-9 max(1, |zb|), away from the mean"""
    betas = ref.default_betas(16)
    tr = _trace()
    rec = ref.reduce(tr, betas)
    bar = se_bar(rec["zb"])
    assert 0 < bar < 1e-7 and rec["lnZ_se"] > 1000 * bar
    bd = ref.block_borders(83)
    moved = []
    for b in range(1, 8):
        for step in (-1, 1):
            other = list(bd)
            other[b] += step
            moved.append(abs(ref.reduce(tr, betas, borders=other)["lnZ_se"] - rec["lnZ_se"]))
    dropped = abs(ref.reduce(tr[:-1], betas)["lnZ_se"] - rec["lnZ_se"])
    first = abs(ref.reduce(tr[1:], betas)["lnZ_se"] - rec["lnZ_se"])
    print("bar", bar, "se", rec["lnZ_se"], "a border moved: min", min(moved), "the last step dropped", dropped, "the first", first)
    assert min(moved) >= 1000 * bar and dropped >= 1000 * bar and first >= 1000 * bar
    # the population deviation (over 8, not 7) is far outside too
    assert abs(np.std(rec["zb"]) / math.sqrt(8.0) - rec["lnZ_se"]) >= 1000 * bar
    zb = rec["zb"]
    worst = zb + 1e-9 * np.maximum(1.0, np.abs(zb)) * np.sign(zb - zb.mean())
    assert abs(np.std(worst, ddof=1) / math.sqrt(8.0) - rec["lnZ_se"]) <= bar


def test_the_limit_cases_are_what_they_claim():
    lds = {k: steps_lds_bytes(*v[:4], v[5]) for k, v in LIMIT_CASES.items()}
    assert lds["big-lds"] == 85808 > DEFAULT_LDS > lds["just-under"] == 55824
    for name, (P, K, mode, sd, T, W, steps, burn, swap_every, rid, a) in LIMIT_CASES.items():
        R, betas, *_ = limit_case(name)
        assert R.x.size == P and R.ndim == (4 if mode else 3) * K + int(sd) and betas[0] == 0.0 and betas[-1] == 1.0
        assert (rid + 1) * betas.size <= 2 ** 31 - 1
        if name.startswith("narrow"):
            assert P <= 32 and K <= 4 and W // 2 > 16                    # more movers than 16-lane groups in a workgroup
        if name in ("big-lds", "just-under", "own-ladder"):
            assert P > 32 or K > 4
    P, K, mode, sd, T, W, steps, burn, swap_every, rid, a = LIMIT_CASES["ladder-64"]
    assert T == 64 and steps % swap_every == 2 and burn % swap_every != 0 and steps - burn == 9
    P, K, mode, sd, T, W, steps, burn, swap_every, rid, a = LIMIT_CASES["high-id"]
    assert (rid * T) * W >= 2 ** 32 and (rid + 1) * T <= 2 ** 31 - 1 < (rid + 2) * T
    assert LIMIT_CASES["own-ladder"][6] - LIMIT_CASES["own-ladder"][7] == 8


def test_a_zero_width_has_no_lnlike_in_the_restatement():
    """the oracle's closed prior ranges contain the width 0; the restatement turns its division by zero into ln L = -inf"""
    x = np.arange(9.0)
    Rv = ref.make_region(x, np.ones(9), np.full(9, 0.1), 1, 1)
    Rg = ref.make_region(x, np.ones(9), np.full(9, 0.1), 1, 0)
    for R, th in ((Rv, [1.0, 4.0, 1.0, 0.0]), (Rv, [1.0, 4.5, 0.0, 0.0]), (Rg, [1.0, 4.0, 0.0])):
        ll, lp = ref.lnlike_lnprior(R, np.array(th))
        assert ll == -np.inf and math.isfinite(lp) and ref.target(lp, ll, 1.0) == -np.inf
    ll, lp = ref.lnlike_lnprior(Rv, np.array([1.0, 4.0, 0.0, 1.0]))      # L_fwhm = 0: finite
    assert math.isfinite(ll) and math.isfinite(lp)
