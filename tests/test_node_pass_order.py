"""The order in which the node pass of a full batch takes the batch's far lines (vamp::np_pair_order,
vamp_amd/csrc/ff_predicates.hpp; reached through a host build, tests/host/np_order_host.cpp) against a literal
restatement of the loop it replaced: the next line of the deepest class that has one, twice per pass, the pass at the
depth found when it began, an odd last line paired with a copy of itself that adds nothing.

The node sums are bit-equal to that loop's only if the sequence, the members of every pair, every pair's depth and the
line that pairs with itself are the same, so all four are compared:

  * every nested choice n6 <= n4 <= n3 <= far over K = 1 .. 5 lines (5^K each: a line is absent or in one of four classes);
  * 1e5 random nested choices over 16 lines, every class size from 0 to 16 among them;
  * two planted errors the comparison must see: a pair evaluated one class too shallow (the pair counts rounded down, so
    the pair an odd class ends with runs at the next class's depth), and an odd last line of a class paired inside its
    class -- with itself -- instead of with the first line of the next class."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT

DEPTHS = (6, 4, 3, 2)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "tests", "host", "libnp_order_host.so")
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ctz(m):
    return (m & -m).bit_length() - 1


def parent_loop(far, n6, n4, n3):
    """the loop of ff_node_pass before the runs: [(k0, k1, live1, depth)], k1 = k0 and live1 False for the odd last line"""
    rest, out = far, []
    while rest:
        depth = 6 if n6 else 4 if n4 else 3 if n3 else 2
        kk, live = [0, 0], [False, False]
        for t in range(2):
            live[t] = rest != 0
            if live[t]:
                kk[t] = ctz(n6 if n6 else n4 if n4 else n3 if n3 else rest)
                keep = ~(1 << kk[t])
                rest &= keep; n6 &= keep; n4 &= keep; n3 &= keep
            else:
                kk[t] = kk[0]
        out.append((kk[0], kk[1], live[1], depth))
    return out


def decode(seq, solo, pairs):
    """the pairs an (seq, solo, pairs) triple makes ff_node_pass run, in the restatement's form: run d takes pairs[d] pairs at
    DEPTHS[d] from the sequence's next two nibbles; the second slot of a pair adds its line unless solo holds its bit"""
    out, seq = [], int(seq)
    for d, depth in enumerate(DEPTHS):
        for _ in range(int(pairs[d])):
            k0, k1 = seq & 15, (seq >> 4) & 15
            seq >>= 8
            out.append((k0, k1, not (int(solo) >> k1) & 1, depth))
    return out, seq


def native_orders(lib, sets):
    """np_pair_order of every row of sets[n, 4] = (far, n6, n4, n3)"""
    s = np.ascontiguousarray(sets, np.uint32)
    n = s.shape[0]
    cols = [np.ascontiguousarray(s[:, i]) for i in range(4)]
    seq, solo, pairs = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 4), np.int32)
    lib.np_pair_order_host(C.c_int64(n), *[_p(c) for c in cols], _p(seq), _p(solo), _p(pairs))
    return seq, solo, pairs


def difference(row, triple):
    """None, or what differs between the restated loop on row = (far, n6, n4, n3) and the triple"""
    want = parent_loop(*[int(v) for v in row])
    got, left = decode(*triple)
    if left != 0:
        return f"lines left in the sequence after the last pair: {left:#x}"
    if len(got) != len(want):
        return f"{len(got)} pairs, the loop runs {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g[:2] != w[:2]:
            return f"pair {i}: lines {g[:2]}, the loop takes {w[:2]}"
        if g[3] != w[3]:
            return f"pair {i} {g[:2]}: depth {g[3]}, the loop's {w[3]}"
        if g[2] != w[2]:
            return f"pair {i} {g[:2]}: second slot live {g[2]}, the loop's {w[2]}"
    if want and not want[-1][2]:
        if int(triple[1]) != 1 << want[-1][0]:
            return f"solo {int(triple[1]):#x}, the loop pairs line {want[-1][0]} with itself"
    elif int(triple[1]) != 0:
        return f"solo {int(triple[1]):#x} with an even number of lines"
    return None


def nested(levels):
    """(far, n6, n4, n3) from levels[..., K] in 0 .. 4: 0 absent, 1 far only, 2 also in n3, 3 also in n4, 4 also in n6"""
    w = np.uint32(1) << np.arange(levels.shape[-1], dtype=np.uint32)
    f = lambda lo: ((levels >= lo) * w).sum(-1).astype(np.uint32)
    return np.stack([f(1), f(4), f(3), f(2)], axis=-1)


def exhaustive_sets():
    rows = []
    for K in range(1, 6):
        rows.append(nested(np.array(list(itertools.product(range(5), repeat=K)))))
    return np.concatenate(rows)


def random_sets(n=100000, seed=7):
    """16 lines; the chance of each level drawn per row, so that empty, odd, even and full classes all occur"""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(5, 0.5), n)
    u = rng.random((n, 16))
    return nested((u[:, :, None] > np.cumsum(p, -1)[:, None, :]).sum(-1).clip(0, 4))


def test_exhaustive_up_to_five_lines(lib):
    sets = exhaustive_sets()
    assert sets.shape[0] == sum(5 ** K for K in range(1, 6))
    seq, solo, pairs = native_orders(lib, sets)
    for i, row in enumerate(sets):
        d = difference(row, (seq[i], solo[i], pairs[i]))
        assert d is None, ([hex(int(v)) for v in row], d)


def test_random_sets_of_sixteen_lines(lib):
    sets = random_sets()
    seq, solo, pairs = native_orders(lib, sets)
    sizes = set()
    for i, row in enumerate(sets):
        d = difference(row, (seq[i], solo[i], pairs[i]))
        assert d is None, ([hex(int(v)) for v in row], d)
        sizes.add(bin(int(row[0])).count("1"))
    assert sizes == set(range(17)), sorted(sizes)                      # no far line at all .. all sixteen


# ---- planted errors -----------------------------------------------------------------------------------------------------
def class_lists(row):
    far, n6, n4, n3 = [int(v) for v in row]
    masks = (n6, n4 & ~n6, n3 & ~n4, far & ~n3)
    return [[k for k in range(16) if m >> k & 1] for m in masks]


def pack(order):
    return sum(k << (4 * i) for i, k in enumerate(order))


def planted_shallow(row):
    """the right sequence with every run's count rounded DOWN: the pair an odd class ends with runs one class too shallow"""
    cl = class_lists(row)
    order = [k for c in cl for k in c]
    odd = len(order) & 1
    cum = np.cumsum([len(c) for c in cl])
    h = [int(c) // 2 for c in cum[:3]] + [(int(cum[3]) + 1) // 2]
    # an error wherever a pair begins with the odd last line of the classes down to some depth above the shallowest
    matters = any(int(c) & 1 for c in cum[:3])
    return (pack(order + order[-1:] * odd), (1 << order[-1]) if odd else 0, [h[0], h[1] - h[0], h[2] - h[1], h[3] - h[2]]), matters


def planted_inclass(row):
    """every class paired inside itself: its odd last line with itself, not with the first line of the next class"""
    cl = class_lists(row)
    order, solo, pairs = [], 0, []
    for c in cl:
        order += c + c[-1:] * (len(c) & 1)
        solo |= (1 << c[-1]) if len(c) & 1 else 0
        pairs.append((len(c) + 1) // 2)
    # an error wherever an odd class is followed by a line of a shallower class
    matters = any(len(c) & 1 and any(len(n) for n in cl[i + 1:]) for i, c in enumerate(cl))
    return (pack(order), solo, pairs), matters


@pytest.mark.parametrize("plant", [planted_shallow, planted_inclass])
def test_planted_errors_are_seen(plant):
    sets = exhaustive_sets()
    seen = clean = 0
    for row in sets:
        t, matters = plant(row)
        d = difference(row, t)
        assert (d is not None) == matters, ([hex(int(v)) for v in row], d)
        seen += matters
        clean += not matters
    assert seen > 1000 and clean > 100, (seen, clean)
