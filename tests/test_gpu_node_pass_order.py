"""The node pass as runs of one depth (ff_node_pass with VAMP_NP_CLASS_RUNS: vamp::np_pair_order, one counted loop per
depth, the records of a pair read by every lane one pair ahead) on the GPU: node sums and class sets through the test
hook vampdbg_node_sums against the numpy restatement (tests/node_pass_ref.py), at the bars of tests/test_gpu_node_pass.py
-- full batches to 64 ulps of the sum of the terms' magnitudes plus the tables' 2e-14 of the wide lines' share, the
other tiles to twice the fractions' 9e-13.

Regions: P = 4096 (16 tiles: one full batch per wavefront) and P = 5376 (21 tiles: a full batch per wavefront and a
remainder of one or two tiles through the tile-by-tile stage).  Walkers, by what the runs can get wrong in class 0's
batch (tiles 0, 4, 8, 12) -- each asserted on the CPU restatement before anything runs, so that a case cannot miss it:

    one        K = 1: a single pair, the line with itself
    same       K = 2, both lines in one class: one run of one pair, the others empty
    each       K = 4, one line in each class: every run odd, both pairs cross a class border
    gap        K = 3, classes 6, 3 and 2: a middle run empty, the first pair crosses two borders
    single     K = 1, a line far for exactly one tile of the batch: three rows of lanes take the idle argument
    none       K = 1, no far line at all: the pass runs no pair
    guard      `each` with a line of y = 1e-300: the guard walker's single run through ff_eval2
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import node_pass_ref as npr
import tile_moments_ref as tm

ULP = 2.0 ** -53
TILE = 256
SIZES = (4096, 5376)
BATCH0 = [0, 4, 8, 12]
# line widths G that put a line at the centre of tile 1 -- 640 px from tile 4, the nearest tile of the batch it is far
# for -- into the 6-, 4-, 3- and 2-level class: r2e = (640 * 2 sqrt(ln 2) / G)^2 against 100 / 300 / 2000
G6, G4, G3, G2 = 120.0, 80.0, 40.0, 10.0


def grid(P):
    return np.arange(P, dtype=np.float64) - (P - 1) / 2.0


def walkers(P):
    """name -> (native[K, 4] rows (A, c, L, G), class counts (n6, n4 \\ n6, n3 \\ n4, far \\ n3) wanted of class 0's first batch)"""
    x = grid(P)
    c1 = 0.5 * (x[TILE] + x[2 * TILE - 1])
    c14 = 0.5 * (x[14 * TILE] + x[15 * TILE - 1])
    line = lambda G, dc=0.0, A=1.0, L=1.0: (A, c1 + dc, L, G)
    each = [line(G4, 3.0), line(G2, -2.0, 2.0), line(G6), line(G3, 5.0, 1.5)]
    tiny = [line(G4, 3.0), line(G2, -2.0, 2.0, 1e-300 * G2 / vo.SQRT_LN2), line(G6), line(G3, 5.0, 1.5)]
    return {
        "one": (np.array([line(G6)]), (1, 0, 0, 0)),
        "same": (np.array([line(G3), line(G3 + 2.0, 30.0, 0.7)]), (0, 0, 2, 0)),
        "each": (np.array(each), (1, 1, 1, 1)),
        "gap": (np.array([line(G2, 4.0), line(G6), line(G3, -6.0, 2.0)]), (1, 0, 1, 1)),
        "single": (np.array([(1.0, c14, 1.0, 600.0)]), (1, 0, 0, 0)),       # (far from 4.8 G on: tile 0 alone, just inside r2e < 100)
        "none": (np.array([(1.0, c1, 1.0, 3000.0)]), (0, 0, 0, 0)),
        "guard": (np.array(tiny), (1, 1, 1, 1)),
    }


NAMES = ("one", "same", "each", "gap", "single", "none", "guard")


def class_counts(sets):
    pop = lambda m: bin(m).count("1")
    return (pop(sets["n6"]), pop(sets["n4"] & ~sets["n6"]), pop(sets["n3"] & ~sets["n4"]), pop(sets["far"] & ~sets["n3"]))


@functools.lru_cache(maxsize=None)
def reference(P, name):
    """the restatement's node sums and class sets of the walker: computed once, shared, read-only"""
    x = grid(P)
    native, counts = walkers(P)[name]
    sets = npr.class_sets(native, x)
    want, mag, magw = npr.node_sums(native, x)
    far = tm.classify(native[None], x)[0][0]
    for a in (want, mag, magw, far):
        a.setflags(write=False)
    return dict(x=x, native=native, counts=counts, sets=sets, want=want, mag=mag, magw=magw, far=far)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("P", SIZES)
def test_case_has_its_classes(P, name):
    r = reference(P, name)
    first = next(s for s in r["sets"] if list(s["tiles"]) == BATCH0)
    assert class_counts(first) == r["counts"], (class_counts(first), r["counts"])
    walk = npr.walk(first)
    if name == "each":          # pairs (6, 4) at depth 6 and (3, 2) at depth 3
        assert [d for _, _, d in walk] == [6, 3] and all(k1 is not None for _, k1, _ in walk)
    if name == "gap":           # (6, 3) at depth 6, then the 2-level line with itself
        assert [d for _, _, d in walk] == [6, 2] and walk[1][1] is None
    if name == "single":
        assert r["far"][0, BATCH0].sum() == 1
    if name == "none":
        assert not r["far"].any()
    if name == "guard":
        nat = r["native"]
        assert (nat[:, 2] * vo.SQRT_LN2 / nat[:, 3]).min() < 1e-290
    full, rest = npr.batches(r["x"].size // TILE)
    assert len(full) == 4 and len(rest) == (0 if P == 4096 else 5)


def _context(x, K):
    import vamp_amd
    rng = np.random.default_rng(K)
    noise = np.full(x.size, 0.05)
    flux = 1.0 + rng.normal(0, 0.05, x.size)
    bounds = np.array([[x.min() - 50.0, x.max() + 50.0, 1.0e5, 1.0e5]])
    ctx = vamp_amd.HipContext(device=0)
    ctx.set_packing(256)
    ctx.set_regions(x, flux, noise, K, mode=vamp_amd.MODE_VOIGT4, bounds=bounds)
    return ctx


def _node_sums(ctx, theta, ntile):
    fn = ctx._lib.vampdbg_node_sums
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    th = np.ascontiguousarray(theta, np.float64)
    nodes, sets = np.full((ntile, 16), np.nan), np.zeros((ntile, 5), np.uint32)
    n = fn(ctx._h, 0, th.ctypes.data, nodes.ctypes.data, sets.ctypes.data)
    assert n == ntile, (n, ctx._lib.vamp_last_error())
    return nodes, sets


@pytest.mark.gpu
@pytest.mark.parametrize("P", SIZES)
def test_node_sums_match_the_restatement(P):
    x = grid(P)
    ntile = P // TILE
    full, rest = npr.batches(ntile)
    by_K = {}
    for name in NAMES:
        by_K.setdefault(reference(P, name)["native"].shape[0], []).append(name)
    for K, names in sorted(by_K.items()):
        with _context(x, K) as ctx:
            for name in names:
                r = reference(P, name)
                got, gsets = _node_sums(ctx, r["native"].reshape(-1), ntile)
                assert np.isfinite(got).all(), name
                heads = {int(s["tiles"][0]): s for s in r["sets"]}
                for t in range(ntile):
                    if t in heads:
                        s = heads[t]
                        assert [int(v) for v in gsets[t]] == [s["far"], s["n6"], s["n4"], s["n3"], s["wide"]], (name, t)
                    else:
                        assert (gsets[t] == 0xffffffff).all(), (name, t)
                ft = full.reshape(-1)
                tol = 64 * ULP * r["mag"][ft] + 4e-14 * r["magw"][ft]
                worst_full = np.max(np.abs(got[ft] - r["want"][ft]) / np.maximum(tol, 1e-300))
                worst_rest = 0.0
                if rest:
                    worst_rest = np.max(np.abs(got[rest] - r["want"][rest]) / np.maximum(2 * 9e-13 * r["mag"][rest], 1e-300))
                print(f"P={P} {name}: node sums nearest their bars: full batches {worst_full:.3f}, other tiles {worst_rest:.3f}")
                assert worst_full <= 1.0 and worst_rest <= 1.0, name
