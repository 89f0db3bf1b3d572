"""The host half that libvamp_post.so, libvamp_pred.so and libvamp_loo.so share (vamp_amd/csrc/chain_groups.hpp), through a stand-alone
program (tests/host/chain_groups_host.cpp) built with AddressSanitizer and UBSan:

  * plan_passes against a restatement of the greedy rule, and against the properties the GPU tests
    test_pass_packing_does_not_change_a_bit / test_packing_and_group_order_do_not_change_a_bit rest on: every group's
    ranges tile its pixels once and in order, no pass exceeds the cap, is empty, or closes while the next column would
    still fit, offsets are the running sums and scratch_len is the largest pass;
  * check_chain_groups: every shared message, byte for byte, and what it hands back for groups that pass;
  * check_chain_data (the predictive and LOO libraries): every data message, byte for byte, after the shared checks, and
    tot_noise; pack_chain_data: the offsets, every value in its place, nothing for a group without noise.
"""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "fn: "


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cg") / "chain_groups_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "chain_groups_host.cpp")])

    def run(lines):
        res = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
        out = res.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


# ---- the planner --------------------------------------------------------------------------------------------------
PLANS = {                                                  # name: (cap, S, P)
    "cap == s_max: one column per pass": (5, (5, 3), (3, 2)),
    "cap == S P": (28, (7,), (4,)),
    "cap == S P - 1": (27, (7,), (4,)),
    "group boundary on a pass boundary": (8, (4, 4), (2, 3)),
    "the GPU tests' groups, one column of the largest": (20, (20, 17, 20), (3, 1, 2)),
    "the GPU tests' groups, cap 47": (47, (20, 17, 20), (3, 1, 2)),
    "a later group's column exceeds what is left": (12, (3, 10), (2, 2)),
    "64 groups of one pixel in one pass": (64 * 5, (5,) * 64, (1,) * 64),
    "one group, one pixel, one sample": (1, (1,), (1,)),
    "ragged": (100, (33, 7, 50, 1, 100), (5, 40, 3, 17, 2)),
}


def greedy(cap, S, P):
    """fit = (cap - used) // S; fit == 0 closes the pass and retries; np = min(P - p0, fit); groups in order"""
    ranges, first, used, longest = [], [], 0, 0
    for g, (s, p) in enumerate(zip(S, P)):
        p0 = 0
        while p0 < p:
            fit = (cap - used) // s
            if fit == 0:
                assert used > 0
                used = 0
                continue
            if used == 0:
                first.append(len(ranges))
            n = min(p - p0, fit)
            ranges.append((g, p0, n, used, len(first) - 1))
            used += n * s
            longest = max(longest, used)
            p0 += n
    return longest, first, ranges


def parse_plan(line):
    head, first, *ranges = [[int(v) for v in part.split()] for part in line[len("plan "):].split("|")]
    assert head[1] == len(first)
    return head[0], first, [tuple(r) for r in ranges]


@pytest.fixture(scope="module")
def plans(program):
    lines = ["plan %d %d %s" % (cap, len(S), " ".join("%d %d" % sp for sp in zip(S, P))) for cap, S, P in PLANS.values()]
    return dict(zip(PLANS, (parse_plan(ln) for ln in program(lines))))


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_is_the_greedy_rule_and_keeps_its_properties(plans, name):
    cap, S, P = PLANS[name]
    scratch_len, first, ranges = plans[name]
    assert (scratch_len, first, ranges) == greedy(cap, S, P)
    # every group's ranges tile [0, P) once, in order; groups in order
    assert [r[0] for r in ranges] == sorted(r[0] for r in ranges) and {r[0] for r in ranges} == set(range(len(S)))
    for g in range(len(S)):
        mine = [r for r in ranges if r[0] == g]
        assert mine[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(mine, mine[1:])) and mine[-1][1] + mine[-1][2] == P[g]
        assert all(r[2] >= 1 for r in mine)
        assert len({r[4] for r in mine}) == len(mine)              # never two ranges of a group in one pass
    # passes: numbered in order, none empty, `first` their first ranges, offsets the running sums, none above the cap
    n_pass = len(first)
    assert [r[4] for r in ranges] == sorted(r[4] for r in ranges) and {r[4] for r in ranges} == set(range(n_pass))
    used = []
    for i in range(n_pass):
        mine = [r for r in ranges if r[4] == i]
        assert ranges.index(mine[0]) == first[i]
        run = 0
        for g, p0, n, off, _ in mine:
            assert off == run
            run += n * S[g]
        assert 0 < run <= cap
        used.append(run)
    assert scratch_len == max(used)
    # a pass closes only when the next column does not fit
    for i in range(n_pass - 1):
        assert S[ranges[first[i + 1]][0]] > cap - used[i]


def test_named_plans_are_what_they_claim(plans):
    assert [r[2] for r in plans["cap == s_max: one column per pass"][2]] == [1] * 5
    assert len(plans["cap == S P"][1]) == 1 and [r[2] for r in plans["cap == S P - 1"][2]] == [3, 1]
    assert plans["group boundary on a pass boundary"][2] == [(0, 0, 2, 0, 0), (1, 0, 2, 0, 1), (1, 2, 1, 0, 2)]
    assert [r[4] for r in plans["the GPU tests' groups, one column of the largest"][2]] == list(range(6))
    assert plans["the GPU tests' groups, cap 47"][2] == [(0, 0, 2, 0, 0), (0, 2, 1, 0, 1), (1, 0, 1, 20, 1), (2, 0, 2, 0, 2)]
    assert plans["a later group's column exceeds what is left"][2] == [(0, 0, 2, 0, 0), (1, 0, 1, 0, 1), (1, 1, 1, 0, 2)]
    assert plans["64 groups of one pixel in one pass"][:2] == (320, [0])
    assert plans["one group, one pixel, one sample"] == (1, [0], [(0, 0, 1, 0, 0)])


# ---- the checks ---------------------------------------------------------------------------------------------------
def group(n_pix=7, n_comp=2, mode=0, sd=0, n_keep=10, walkers=4, ld=24, base_null=0, x_null=0, bad_pixel=-1):
    return "%d %d %d %d %d %d %d %d %d %d" % (n_pix, n_comp, mode, sd, n_keep, walkers, ld, base_null, x_null, bad_pixel)


AT = FN + "group 0: "
MESSAGES = [
    ((-1, [group()]), FN + "scratch_bytes must not be negative"),
    ((0, [group(base_null=1)]), AT + "NULL base pointer"),
    ((0, [group(x_null=1)]), AT + "NULL abscissa"),
    ((0, [group(n_pix=0)]), AT + "n_pix must be positive"),
    ((0, [group(n_comp=0)]), AT + "n_comp = 0 is outside 1 .. 32"),
    ((0, [group(n_comp=33, ld=4 * 99)]), AT + "n_comp = 33 is outside 1 .. 32"),
    ((0, [group(mode=2)]), AT + "mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout"),
    ((0, [group(mode=3)]), AT + "mode must be 0 (GAUSS3) or 1 (VOIGT4)"),
    ((0, [group(sd=2)]), AT + "sample_sd must be 0 or 1"),
    ((0, [group(n_keep=0)]), AT + "n_keep and walkers must be positive"),
    ((0, [group(walkers=0)]), AT + "n_keep and walkers must be positive"),
    ((0, [group(n_keep=16385, walkers=1, ld=6)]), AT + "n_keep * walkers = 16385 exceeds 16384 (HINT)"),
    ((0, [group(n_keep=128, walkers=129, ld=129 * 6)]), AT + "n_keep * walkers = 16512 exceeds 16384 (HINT)"),
    ((0, [group(ld=23)]), AT + "ld < walkers * ndim"),
    ((0, [group(sd=1, ld=27)]), AT + "ld < walkers * ndim"),
    ((0, [group(bad_pixel=3)]), AT + "the abscissa is not finite at pixel 3"),
    ((0, [group(), group(mode=1, ld=31)]), FN + "group 1: ld < walkers * ndim"),
    ((8 * 40 - 1, [group()]), FN + "scratch_bytes = 319 is less than one column of the largest group (320 bytes)"),
    ((8 * 40 - 1, [group(n_keep=1), group(), group(n_keep=2)]),
     FN + "scratch_bytes = 319 is less than one column of the largest group (320 bytes)"),
]


def test_every_shared_message_byte_for_byte(program):
    out = program(["check %d %d %s" % (scratch, len(groups), " ".join(groups)) for (scratch, groups), _ in MESSAGES])
    assert out == ["error " + want for _, want in MESSAGES]


def test_what_the_checks_hand_back(program):
    groups = [group(), group(n_pix=3, n_comp=3, mode=1, sd=1, n_keep=5, walkers=8, ld=200), group(n_pix=1, n_comp=32, mode=1, ld=4 * 128,
                                                                                                   n_keep=4096)]
    out = program(["check %d 3 %s" % (scratch, " ".join(groups)) for scratch in (0, 8 * 16384, 8 * 16384 + 7, 1 << 40)])
    tail = " 16384 11 16464 | 40 6 | 40 13 | 16384 128"
    assert out == ["ok %d" % cap + tail for cap in ((256 << 20) // 8, 16384, 16384, (1 << 40) // 8)]


# ---- the data checks and the packing ------------------------------------------------------------------------------
def data_group(flux_null=0, noise_given=None, bad_flux=-1, flux_value="nan", bad_noise=-1, noise_value="0", **chain):
    """a group of the chain checks with its data: a noise is given exactly when the sd is not sampled, unless told"""
    given = int(not chain.get("sd", 0)) if noise_given is None else noise_given
    return group(**chain) + " %d %d %d %s %d %s" % (flux_null, given, bad_flux, flux_value, bad_noise, noise_value)


AT1 = FN + "group 1: "
DATA_MESSAGES = [
    ([data_group(), data_group(flux_null=1)], AT1 + "NULL flux"),
    ([data_group(), data_group(sd=1, ld=28, noise_given=1)], AT1 + "noise must be NULL when sample_sd is set: the chain's sd is the noise"),
    ([data_group(), data_group(noise_given=0)], AT1 + "NULL noise without sample_sd"),
    ([data_group(), data_group(bad_flux=5, flux_value="nan")], AT1 + "the flux is not finite at pixel 5"),
    ([data_group(), data_group(bad_flux=6, flux_value="-inf")], AT1 + "the flux is not finite at pixel 6"),
    ([data_group(), data_group(bad_noise=4, noise_value="0")], AT1 + "the noise is not finite and positive at pixel 4"),
    ([data_group(), data_group(bad_noise=0, noise_value="-1")], AT1 + "the noise is not finite and positive at pixel 0"),
    ([data_group(), data_group(bad_noise=6, noise_value="inf")], AT1 + "the noise is not finite and positive at pixel 6"),
    ([data_group(), data_group(bad_noise=2, noise_value="nan")], AT1 + "the noise is not finite and positive at pixel 2"),
    ([data_group(bad_flux=3)], AT + "the flux is not finite at pixel 3"),
    # the order within a group and between groups: flux pointer, noise form, then pixel by pixel flux before noise
    ([data_group(bad_noise=1), data_group(flux_null=1)], AT + "the noise is not finite and positive at pixel 1"),
    ([data_group(flux_null=1, noise_given=0)], AT + "NULL flux"),
    ([data_group(noise_given=0, bad_flux=0)], AT + "NULL noise without sample_sd"),
    ([data_group(bad_flux=2, bad_noise=1)], AT + "the noise is not finite and positive at pixel 1"),
    ([data_group(bad_flux=2, bad_noise=2)], AT + "the flux is not finite at pixel 2"),
    # a shared rule wins over a data rule, also one of a later group
    ([data_group(flux_null=1, mode=3)], AT + "mode must be 0 (GAUSS3) or 1 (VOIGT4)"),
    ([data_group(flux_null=1), data_group(ld=23)], AT1 + "ld < walkers * ndim"),
    ([data_group(bad_flux=0, bad_pixel=6)], AT + "the abscissa is not finite at pixel 6"),
]


def test_every_data_message_byte_for_byte_after_the_shared_checks(program):
    out = program(["data 0 %d %s" % (len(groups), " ".join(groups)) for groups, _ in DATA_MESSAGES])
    assert out == ["error " + want for _, want in DATA_MESSAGES]
    out = program(["data %d 1 %s" % (8 * 40 - 1, data_group(flux_null=1))])
    assert out == ["error " + FN + "scratch_bytes = 319 is less than one column of the largest group (320 bytes)"]


def test_data_that_pass_hand_back_the_noise_pixels(program):
    groups = [data_group(n_pix=3), data_group(n_pix=1, sd=1, ld=28), data_group(n_pix=2)]
    assert program(["data 0 3 " + " ".join(groups), "data 0 1 " + groups[1], "data 0 1 " + groups[2]]) == ["ok 5", "ok 0", "ok 2"]


def test_packing_three_groups_known_noise_free_sd_known_noise(program):
    P, given = (3, 1, 2), (1, 0, 1)
    head, values = program(["pack 0 3 " + " ".join("%d %d" % pg for pg in zip(P, given))])[0][len("pack "):].split("|")
    assert [int(v) for v in head.split()] == [0, 6, 12, 17, 22, 22]        # x | flux | noise | ln noise | end, the vector's size
    h = [float(v) for v in values.split()]
    x = [100.0 * g + p + 0.25 for g in range(3) for p in range(P[g])]
    flux = [-(100.0 * g + p) - 0.5 for g in range(3) for p in range(P[g])]
    noise = [0.5 + (10.0 * g + p) / 64.0 for g in (0, 2) for p in range(P[g])]     # no slot for the free-sd group
    assert h == x + flux + noise + [math.log(n) for n in noise]


def test_the_libraries_hints_are_todays():
    csrc = os.path.join(ROOT, "vamp_amd", "csrc")
    assert '"a column must fit the LDS; subsample in time: ld * step, ceil(n_keep / step)"' in open(os.path.join(csrc, "posterior.hip")).read()
    assert '"subsample in time: ld * step, ceil(n_keep / step)", cg' in open(os.path.join(csrc, "predictive.hip")).read()
