"""The distant pass of the fp64 far-field node stage (VAMP_SUPER_NODES) on the host: vamp::ff_super_distant,
ff_super_tile and super_order through a host build (tests/host/super_nodes_host.cpp), the cosine table of
vamp_amd/csrc/ff_super.inc, and the numpy restatement tests/super_nodes_ref.py.

  * a line the predicate calls distant from a batch's super-tile is far, by the per-tile classification, for each of the
    four tiles, and no node of them asks for a fraction deeper than three levels -- on uniform, stepped and stretched
    grids, both directions, thresholds hit exactly from either side by nextafter;
  * the table against a direct cosine sum in extended precision;
  * the order of the distant lines against a literal restatement;
  * the distant path (super-node values by scipy's wofz, the transform and Clenshaw's recurrence in double precision)
    against direct evaluation at the 64 tile nodes: widths 20 - 800 px, dampings y = 1e-6 - 10, distances from exactly
    the threshold to the far end of a 16 384-pixel region.  The bar is the node sums' own (tests/test_gpu_node_pass.py):
    64 ulps of the sum of the terms' magnitudes;
  * two planted errors must fail that bar: a threshold of 2 half-widths, and the table transposed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import node_pass_ref as npr
import super_nodes_ref as snr
import tile_moments_ref as tm

ULP = 2.0 ** -53
P = 16384


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "tests", "host", "libsuper_nodes_host.so")
    src = os.path.join(ROOT, "tests", "host", "super_nodes_host.cpp")
    hdrs = [os.path.join(ROOT, "vamp_amd", "csrc", f) for f in ("ff_predicates.hpp", "ff_super.inc", "voigt_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def grids():
    up = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    steps = np.cumsum(np.where((np.arange(P) // 256) % 2 == 0, 1.0, 2.0))
    steps -= 0.5 * (steps[0] + steps[-1])
    stretch = np.cumsum(1.0 + 0.5 * np.arange(P) / P)              # spacing grows by half across the region
    stretch -= 0.5 * (stretch[0] + stretch[-1])
    return {"up": up, "down": up[::-1].copy(), "steps": steps, "stretch": stretch}


def host_distant(lib, c, s, y, Mid, Half):
    n = c.size
    a = [np.ascontiguousarray(np.broadcast_to(v, n), np.float64) for v in (c, s, y, Mid, Half)]
    d, r2e = np.zeros(n, np.uint8), np.zeros(n)
    lib.super_distant_host(C.c_int64(n), *[_p(v) for v in a], _p(d), _p(r2e))
    return d.astype(bool), r2e


def threshold_centre(Mid, Half, s, y, side, factor=snr.SUPER_DIST):
    """the centre, beyond the `side` edge of the super-tile, at the smallest distance that is distant"""
    need = max(factor * Half, np.sqrt(max(snr.R2_M3 - y * y, 0.0)) / s)
    return Mid + side * (Half + need)


def need_is_distance(Mid, Half, s, y, factor):
    return factor * Half >= (1.0 + 1e-9) * np.sqrt(max(snr.R2_M3 - y * y, 0.0)) / s


def test_super_tile_and_factor(lib):
    lib.super_dist_factor_host.restype = C.c_double
    assert lib.super_dist_factor_host() == snr.SUPER_DIST == 4.0
    for name, x in grids().items():
        mid, half = tm.tile_geometry(x)[:2]
        full = snr.batches(mid.size)[0]
        Mid, Half = np.zeros(len(full)), np.zeros(len(full))
        a, b = full[:, 0], full[:, -1]
        lib.super_tile_host(C.c_int64(len(full)), _p(np.ascontiguousarray(mid[a])), _p(np.ascontiguousarray(half[a])),
                            _p(np.ascontiguousarray(mid[b])), _p(np.ascontiguousarray(half[b])), _p(Mid), _p(Half))
        for i, tiles in enumerate(full):
            lo, hi = x[256 * tiles[0]], x[256 * tiles[-1] + 255]
            assert np.isclose(Mid[i], 0.5 * (lo + hi), rtol=0, atol=1e-9) and np.isclose(Half[i], 0.5 * abs(hi - lo), rtol=1e-14), name
            assert (Mid[i], Half[i]) == snr.super_tile(x, tiles)


@pytest.mark.parametrize("name", ["up", "down", "steps", "stretch"])
def test_distant_implies_far_and_three_levels(lib, name):
    x = grids()[name]
    mid, half = tm.tile_geometry(x)[:2]
    full = snr.batches(mid.size)[0]
    rng = np.random.default_rng(7)
    K = 4000
    G = np.exp(rng.uniform(np.log(20.0), np.log(800.0), K))
    yv = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), K))
    native = np.stack([np.ones(K), rng.uniform(x.min() - 50.0, x.max() + 50.0, K), yv * G / npr.SQRT_LN2, G], 1)
    # a quarter of the lines sit exactly at their threshold for a random super-tile, on the true or the false side of it
    for i in range(0, K, 4):
        tiles = full[rng.integers(len(full))]
        Mid, Half = snr.super_tile(x, tiles)
        s, y, _ = npr.line_sy(native[i])
        c = threshold_centre(Mid, Half, s, y, rng.choice([-1.0, 1.0]))
        native[i, 1] = np.nextafter(c, Mid if i % 8 else 2 * c - Mid)
    s, y, _ = npr.line_sy(native)
    far = tm.classify(native[None], x)[0][0]
    r2n = npr.node_r2(native, x)
    seen = at_edge = 0
    for tiles in full:
        Mid, Half = snr.super_tile(x, tiles)
        d, r2e = host_distant(lib, native[:, 1], s, y, Mid, Half)
        dn, r2n_ref = snr.super_distant(native[:, 1], s, y, Mid, Half)
        # (the header forms the edge bound with one fused operation, numpy with two: they may part within rounding of R2_M3)
        assert np.allclose(r2e, r2n_ref, rtol=1e-14) and (np.abs(r2e[d != dn] - snr.R2_M3) < 1e-10).all()
        assert far[d][:, tiles].all()
        assert (npr.depth_of(r2n[d][:, tiles]) <= 3).all()
        assert (r2n[d][:, tiles].min(axis=(1, 2)) >= r2e[d]).all()             # the edge bound bounds every node
        seen += int(d.sum())
        at_edge += int((d & (np.abs(np.abs(Mid - native[:, 1]) - Half - snr.SUPER_DIST * Half) < 1e-9 * Half)).sum())
    assert seen > 1000 and at_edge > 0
    # NaN compares false
    assert not host_distant(lib, np.array([np.nan, 0.0, 0.0]), np.array([1.0, np.nan, 1.0]), np.array([0.1, 0.1, np.nan]), 1e5, 1.0)[0].any()
    assert host_distant(lib, np.array([0.0]), np.array([1.0]), np.array([0.1]), 1e5, 1.0)[0].all()


def test_table_is_the_cosine_transform(lib):
    Ct = snr.table()
    raw = np.zeros(256)
    lib.super_table_host(_p(raw))
    assert np.array_equal(raw.reshape(8, 16, 2).transpose(1, 0, 2).reshape(16, 16), Ct)
    k, n = np.arange(16, dtype=np.longdouble)[:, None], np.arange(16, dtype=np.longdouble)[None, :]
    want = np.cos(k * np.arccos(np.longdouble(-1.0)) * (n + 0.5) / 16) / 8
    want[0] /= 2
    assert np.max(np.abs(Ct - want)) <= 2.0 ** -56                                # half an ulp of the largest entry
    # ... and it turns node values of T_m into the unit coefficient vector
    t = snr.cheb_nodes()
    for m in range(16):
        coef = Ct @ np.cos(m * np.arccos(t))
        assert np.allclose(coef, np.eye(16)[m], rtol=0, atol=4e-15)       # (cos(m arccos t) itself carries m ulps)


def test_order_of_the_distant_lines(lib):
    rng = np.random.default_rng(3)
    dist = rng.integers(0, 1 << 16, 20000, dtype=np.uint32)
    d3 = (dist & rng.integers(0, 1 << 16, 20000, dtype=np.uint32)).astype(np.uint32)
    dist[:3], d3[:3] = (0, 0xffff, 0xffff), (0, 0, 0xffff)
    seq, cnt = np.zeros(dist.size, np.uint64), np.zeros((dist.size, 3), np.int32)
    lib.super_order_host(C.c_int64(dist.size), _p(dist), _p(d3), _p(seq), _p(cnt))
    for i in range(dist.size):
        order = snr.distant_order(dict(dist=int(dist[i]), d3=int(d3[i])))
        got = [(int(seq[i]) >> (4 * j)) & 15 for j in range(len(order))]
        assert got == [k for k, _ in order]
        assert len(order) == 16 or int(seq[i]) >> (4 * len(order)) == 0
        assert cnt[i, 0] == len(order) and cnt[i, 1] == (len(order) + 7) // 8
        assert cnt[i, 2] == len({j // 8 for j, (_, dep) in enumerate(order) if dep == 3})


def distant_path_error(x, tiles, native, factor=snr.SUPER_DIST, Ctab=None):
    """worst |interpolated - direct| / (64 ulps of the value) over the 64 tile nodes of the batch, for one line"""
    mid, half = tm.tile_geometry(x)[:2]
    tn = snr.cheb_nodes()
    Mid, Half = snr.super_tile(x, tiles)
    s, y, amp = npr.line_sy(native[None])
    fsum = amp[0] * npr.exact(np.abs(Mid + Half * tn - native[1]) * s[0], y[0])          # float64: the kernel's precision
    worst = 0.0
    for t in tiles:
        xn = mid[t] + half[t] * tn
        got = snr.interpolate(fsum, (xn - Mid) / Half, Ctab)
        want = amp[0] * npr.exact(np.abs(xn - native[1]) * s[0], y[0])
        worst = max(worst, np.max(np.abs(got - want) / (64 * ULP * np.abs(want))))
    return worst


def _cases(x, factor=snr.SUPER_DIST):
    full = snr.batches(x.size // 256)[0]
    for tiles in (full[0], full[len(full) // 2], full[-1]):
        Mid, Half = snr.super_tile(x, tiles)
        for G in (20.0, 57.0, 200.0, 800.0):
            for yv in (1e-6, 1e-2, 1.0, 10.0):
                s = 2.0 * npr.SQRT_LN2 / G
                for side in (-1.0, 1.0):
                    c0 = threshold_centre(Mid, Half, s, yv, side, factor)
                    end = x.max() + 50.0 if side > 0 else x.min() - 50.0
                    if (c0 - end) * side > 0:
                        continue                                   # the threshold lies beyond the region's end
                    for f in (0.0, 0.01, 0.1, 0.5, 1.0):
                        c = c0 + f * (end - c0)
                        if f == 0.0:        # the first representable centre on the distant side of the threshold
                            if need_is_distance(Mid, Half, s, yv, factor):
                                c = np.nextafter(c, Mid)
                                for _ in range(8):
                                    if snr.super_distant(c, s, yv, Mid, Half, factor)[0]:
                                        break
                                    c = np.nextafter(c, end)
                            else:           # (the edge bound decides, through a fused operation: a relative 1e-12 inside)
                                c += side * 1e-12 * abs(c - Mid)
                        yield tiles, np.array([1.5, c, yv * G / npr.SQRT_LN2, G])


@pytest.mark.parametrize("name", ["up", "down", "steps", "stretch"])
def test_distant_path_matches_direct_evaluation(lib, name):
    x = grids()[name]
    worst, n = 0.0, 0
    for tiles, native in _cases(x):
        Mid, Half = snr.super_tile(x, tiles)
        s, y, _ = npr.line_sy(native[None])
        assert host_distant(lib, native[1:2], s, y, Mid, Half)[0][0]
        worst = max(worst, distant_path_error(x, tiles, native))
        n += 1
    print(f"{name}: {n} (super-tile, line) cases, worst error {worst:.3f} of the bar (64 ulps of the value)")
    assert n >= 200 and worst <= 1.0


def test_planted_errors_fail(lib):
    x = grids()["up"]
    # a threshold of 2 half-widths: the lines between 2 and 4 half-widths miss the bar
    w2 = max(distant_path_error(x, tiles, native, factor=2.0) for tiles, native in _cases(x, factor=2.0))
    # the table transposed
    wt = max(distant_path_error(x, tiles, native, Ctab=snr.table().T.copy()) for tiles, native in list(_cases(x))[:20])
    print(f"planted: threshold 2 -> {w2:.1f} bars, transposed table -> {wt:.3g} bars")
    assert w2 > 1.0 and wt > 1.0


def test_restated_node_sums_agree_with_the_exact_sums():
    """the whole restatement (ordinary pairs, wide lines, distant lines) of the benchmark's walkers against scipy's wofz at
    the fractions' stated accuracy, and some lines are distant"""
    x, nat = npr.headline_natives(W=2)
    for native in nat:
        got, mag, _ = snr.node_sums(native, x)
        want = npr.node_sums_exact(native, x)
        assert any(s["dist"] for s in snr.class_sets(native, x))
        assert np.max(np.abs(got - want) / np.maximum(2 * 9e-13 * mag, 1e-300)) <= 1.0
