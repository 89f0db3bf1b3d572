"""Host half of the moment form of a far-field-only tile's chi^2 (vamp_amd/csrc/ff_moments.hpp, sweep_range_ff):

  * the guard vamp::ff_moments_ok as the kernels compile it, through a stand-alone program (tests/host/ff_moments_host.cpp)
    built with AddressSanitizer and UBSan: its value at the bound, on either side of it, for NaN and infinities, for the
    weights of the zero-residual suites and for ordinary data; and that the rule it states (r <= 2^9) IS the rule of the
    issue (8 2^-53 r^2 <= 2^-40 256);
  * the identity moment form = direct sum on random data, to the rounding the guard assumes (8 2^-53 M);
  * the moments of tests/tile_moments_ref.py (the restatement of k_tile_tables) against sums in extended precision, on
    ascending, descending and uneven grids, and that a descending grid has the moments of its mirror image;
  * the numpy model on a sample of the benchmark's workload: the share of (walker, tile) pairs that take the path and the
    deviation from the exact sum beside the per-pixel form's (profiles/tile_moments_ab.txt records both for 64 walkers).
"""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import tile_moments_ref as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def guard_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ffm") / "ff_moments_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "ff_moments_host.cpp")])
    return exe


def run_guard(exe, triples):
    text = "".join("%s %s %s\n" % tuple(float(v).hex() if math.isfinite(v) else repr(float(v)) for v in t) for t in triples)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    lines = res.stdout.split("\n")
    run_guard.tried = [ln[1:] == "t" for ln in lines[1:1 + len(triples)]]        # ff_moments_try of the same (root_c0, root_q0)
    return lines[0].split(), [ln[:1] == "1" for ln in lines[1:1 + len(triples)]]


def exact_rule(rc, rq, amax):
    """fma(amax, rq, rc) <= 512 in exact arithmetic: the sum rounds to nearest-even, 512 is even in its last place"""
    v = Fraction(amax) * Fraction(rq) + Fraction(rc)
    return v <= Fraction(512) + Fraction(1, 2 ** 44)


def test_guard_as_compiled(guard_program):
    up, down = np.nextafter(512.0, np.inf), np.nextafter(512.0, 0.0)
    cases = [(512.0, 0.0, 0.0), (up, 0.0, 0.0), (down, 0.0, 0.0), (0.0, 512.0, 1.0), (0.0, up, 1.0), (256.0, 1024.0, 0.25),
             (256.0, 1024.0, float(np.nextafter(0.25, 1.0))), (0.0, 0.0, 0.0), (80.0, 1600.0, 0.05), (80.0, 1600.0, 0.27), (80.0, 1600.0, 0.28),
             (16.0, 1600.0, 1e-5), (1.6e9, 1.6e11, 0.0), (0.0, 1.6e11, 1e-5), (0.0, 1.6e11, 0.0), (1e300, 1e300, 1e300)]
    rng = np.random.default_rng(5)
    cases += [tuple(v) for v in np.stack([rng.uniform(0, 600, 200), 10.0 ** rng.uniform(0, 12, 200), 10.0 ** rng.uniform(-8, 0, 200)], axis=1)]
    head, got = run_guard(guard_program, cases)
    want = [exact_rule(*c) for c in cases]
    assert got == want, [c for c, g, w in zip(cases, got, want) if g != w]
    # the question asked before the node stage: the rule with amax = 0 and 2 root_c0 <= 2^9; never true where the rule
    # itself cannot hold for any amax >= root_c0 / root_q0
    tried = run_guard.tried
    assert tried == [exact_rule(c[0], c[1], 0.0) and 2.0 * c[0] <= 512.0 for c in cases]
    assert sum(tried) > 20 and sum(not t for t in tried) > 20
    assert all(t or not exact_rule(c[0], c[1], max(c[2], c[0] / c[1])) for c, t in zip(cases, tried) if c[1] > 0)
    assert sum(got) > 20 and sum(not g for g in got) > 20
    # the zero-residual suites: weights of 1e10 and more over 256 pixels never qualify, whatever the model
    assert not got[12] and not got[13]
    # NaN and infinities compare false
    special = [(float("nan"), 1.0, 0.0), (1.0, float("nan"), 0.1), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 0.0), (1.0, float("inf"), 0.5)]
    assert run_guard(guard_program, special)[1] == [False] * len(special)
    # layout and constants, and the rule as the issue states it: 8 2^-53 r^2 <= 2^-40 x 256  <=>  r <= 2^9
    ns, nq, qrow, s_off, tile, c0, rc, rq = [int(v) for v in head[:8]]
    ulps, bound, rmax = [float.fromhex(v) for v in head[8:]]
    assert (ns, nq) == (tm.NS, tm.NQ) and qrow >= nq + 1 and s_off == 4 * qrow and tile == s_off + 4 * ns
    assert len({c0, rc, rq}) == 3 and all(v % qrow == nq for v in (c0, rc, rq))            # the spare slot of three rows
    assert (ulps, bound) == (tm.GUARD_ULPS, tm.GUARD_BOUND) and bound == 2.0 ** -40 * 256
    assert Fraction(ulps) * Fraction(EPS) * Fraction(rmax) ** 2 == Fraction(bound)
    for r in (down, 512.0, up):
        assert (ulps * EPS * (r * r) <= bound) == (r <= rmax)


def _random_tile(rng, sd, depth):
    x = np.arange(tm.TILE, dtype=np.float64) + rng.uniform(-1e4, 1e4)
    mid, half, up, u, q = tm.tile_geometry(x)
    b = rng.standard_normal((4, tm.NS)) * depth * 0.5 ** np.arange(tm.NS)[None, :]
    noise = np.full(tm.TILE, sd) * rng.uniform(0.5, 2.0, tm.TILE)
    a = np.zeros(tm.TILE)
    for j in range(tm.DEG, -1, -1):
        a = a * u[0] + b[q, j]
    flux = 1.0 - a + rng.normal(0, 1, tm.TILE) * noise
    return x, flux, noise, b, u[0], q, np.abs(a).max()


@pytest.mark.parametrize("sd,depth", [(0.01, 0.01), (0.01, 0.2), (0.05, 0.5), (1e-3, 1e-3), (1e-10, 0.1)])
def test_moment_form_is_the_direct_sum_to_rounding(sd, depth):
    rng = np.random.default_rng(int(1e6 * depth) + 7)
    worst = 0.0
    for _ in range(40):
        x, flux, noise, b, u, q, amax = _random_tile(rng, sd, depth)
        S, Q, C0 = tm.tile_moments(x, flux, noise)
        got = tm.chi2_moments(b, S[0], Q[0], C0[0])
        ld = np.longdouble
        want = tm.chi2_direct(b.astype(ld), u.astype(ld), q, flux.astype(ld), noise.astype(ld))
        r = math.sqrt(C0[0]) + amax * math.sqrt(Q[0, :, 0].sum())
        worst = max(worst, abs(float(got - want)) / (tm.GUARD_ULPS * EPS * r * r))
    print(f"sd={sd} depth={depth}: worst |moment form - direct sum| = {worst:.3f} of 8 2^-53 M")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ["up", "down", "steps"])
def test_moments_of_the_restatement(kind):
    P = 2304 + 100                                                   # nine full tiles and a tail the tables never cover
    x = np.cumsum(np.where((np.arange(P) // tm.TILE) % 2 == 0, 1.0, 2.0)) if kind == "steps" else np.arange(P, dtype=np.float64)
    x = x - 0.5 * (x[0] + x[-1])
    if kind == "down":
        x = x[::-1].copy()
    rng = np.random.default_rng(len(kind))
    flux = 1.0 - 0.3 * np.exp(-0.5 * ((x - 40.0) / 90.0) ** 2) + rng.normal(0, 0.02, P)
    noise = 0.02 * rng.uniform(0.5, 2.0, P)
    S, Q, C0 = tm.tile_moments(x, flux, noise)
    assert S.shape == (9, 4, tm.NS) and Q.shape == (9, 4, tm.NQ) and C0.shape == (9,)
    Sl, Ql, Cl = tm.tile_moments(x, flux, noise, dtype=np.longdouble)
    _, _, _, u, q = tm.tile_geometry(x)
    assert np.abs(u).max() <= 1.0 + 1e-12 and [int((q == k).sum()) for k in range(4)] == [64] * 4
    w2 = (1.0 / noise[:2304].reshape(9, 256)) ** 2
    sabs = (w2 * np.abs(flux[:2304].reshape(9, 256) - 1)).sum(axis=1)
    # a sum of 64 terms |t| <= w^2 |u|^n: 64 roundings of the sum, n of the power, 3 of the term
    assert np.all(np.abs(Q - Ql) <= (64 + 30) * 2 * EPS * Q[:, :, :1])
    assert np.all(np.abs(S - Sl) <= (64 + 30) * 2 * EPS * sabs[:, None, None])
    assert np.all(np.abs(C0 - Cl) <= 300 * 2 * EPS * C0)
    assert np.allclose(Q[:, :, 0].sum(axis=1), w2.sum(axis=1), rtol=1e-14)
    # quarters in coefficient order: the mirror image of the grid (same abscissae, same data) has the same moments
    xm = x[:2304]
    Sa, Qa, Ca = tm.tile_moments(xm, flux[:2304], noise[:2304])
    Sb, Qb, Cb = tm.tile_moments(xm[::-1].copy(), flux[:2304][::-1].copy(), noise[:2304][::-1].copy())
    assert np.all(np.abs(Sb[::-1] - Sa) <= 200 * 2 * EPS * sabs[:, None, None])
    assert np.all(np.abs(Qb[::-1] - Qa) <= 200 * 2 * EPS * Qa[:, :, :1])
    assert np.all(np.abs(Cb[::-1] - Ca) <= 600 * EPS * Ca)


def test_model_on_a_sample_of_the_benchmark():
    import bench
    from oracle import vamp_oracle as vo
    wl = bench.make_workload(W=64)
    x, f, sd = wl["x"], wl["flux"], wl["noise"]
    l_fixed, line, x_origin, x_scale = [float(v) for v in wl["nbz"][0]]
    reg = vo.Region(x=x, flux=f, noise=sd, n_comp=wl["K"], mode=wl["mode"], l_fixed=l_fixed, line=line, x_origin=x_origin, x_scale=x_scale)
    th = wl["theta0"][:4]
    want = vo.log_prob_batch_fast(reg, th)
    M, mom = tm.ff_matrix(), tm.tile_moments(x, f, sd)
    takes = tiles = 0
    for w in range(th.shape[0]):
        r = tm.walker_tiles(np.array(vo.native_components(reg, th[w])), x, f, sd, mom, M)
        takes, tiles = takes + int(r["takes"].sum()), tiles + r["takes"].size
        assert abs(-0.5 * r["exact"].sum() - (want[w] - vo.log_prior(reg, th[w]))) <= 1e-9 * abs(want[w])      # the model's exact sum is the oracle's
        t = r["takes"]
        dev_m, dev_p = np.abs(r["moment"] - r["exact"])[t], np.abs(r["pixel"] - r["exact"])[t]
        print(f"walker {w}: {int(t.sum())} of {t.size} tiles; worst tile deviation: moment form {dev_m.max():.2e}, per pixel {dev_p.max():.2e}")
        assert np.all(dev_m <= dev_p + tm.GUARD_BOUND)
        assert np.array_equal(r["moment"][~t], r["pixel"][~t])
    print(f"share of (walker, tile) pairs on the moment path: {takes} / {tiles}")
    assert takes >= tiles / 4
