"""numpy restatement of the node stage of the fp64 far-field loop with batches of four ADJACENT tiles (VAMP_DEAL_ADJ) and
the distant pass (VAMP_SUPER_NODES; vamp_hip.hip: sweep_range_ff_np, ff_classify_batch_np, ff_super_pass).

Tile class p of a region takes tiles 16 m + 4 p .. 16 m + 4 p + 3 of every whole group of 16 tiles as one batch; the
tiles no group holds keep the tile-by-tile stage.  A batch's four tiles form a super-tile [Mid - Half, Mid + Half], from
the first abscissa of its first tile to the last of its last.  A line whose centre lies >= SUPER_DIST Half beyond the
super-tile's edge with an edge bound (dist s)^2 + y^2 >= R2_M3 there, and which is far for each of the four tiles, is
DISTANT: it leaves the batch's ordinary sets and is evaluated at the 16 Chebyshev nodes of the super-tile, eight lines
per iteration (the three-level lines first; an iteration that holds one runs at three levels, the others at two).  The 16
sums become Chebyshev coefficients through the constant table of vamp_amd/csrc/ff_super.inc, and Clenshaw's recurrence
at t = (x_node - Mid) / Half hands the polynomial to the tiles' own nodes.  A walker with a guard bit or with a line wide
for every tile has no distant line.

    python tests/super_nodes_ref.py      per-wavefront near-pair counts of the two dealings on the benchmark's ensemble
"""
import os

import numpy as np

import node_pass_ref as npr
import tile_moments_ref as tm

TILE, NODES, BATCH, PARTS = npr.TILE, npr.NODES, npr.BATCH, npr.PARTS
GROUP = BATCH * PARTS
SUPER_DIST = 4.0                      # VAMP_SUPER_DIST
R2_M3, R2_M2 = npr.R2_M3, npr.R2_M2
Y_TINY, X_FAR = 1.0e-9, 1.0e4         # voigt_math.hpp: the guard bits (ff_guard_bits)
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table():
    """C[k, n] of vamp_amd/csrc/ff_super.inc (layout [n/2][k][n%2])"""
    txt = open(os.path.join(_ROOT, "vamp_amd", "csrc", "ff_super.inc")).read()
    body = txt[txt.index("{", txt.index("FF_SUPER_C[")) + 1:txt.rindex("}")]
    v = np.array([float(s) for s in body.replace("\n", " ").split(",") if s.strip()])
    assert v.size == NODES * NODES
    return v.reshape(NODES // 2, NODES, 2).transpose(1, 0, 2).reshape(NODES, NODES)


def cheb_nodes():
    return np.cos(np.pi * (np.arange(NODES) + 0.5) / NODES)


def batches(ntile):
    """(full, rest): the batches of four adjacent tiles, group by group and class by class, and the tiles no group holds"""
    ng = ntile // GROUP
    full = [[GROUP * m + BATCH * p + j for j in range(BATCH)] for m in range(ng) for p in range(PARTS)]
    return np.array(full, int).reshape(-1, BATCH), list(range(GROUP * ng, ntile))


def super_tile(x, tiles):
    """(Mid, Half) of the batch `tiles`, as vamp::ff_super_tile forms them from the tile table"""
    mid, half = tm.tile_geometry(x)[:2]
    a, b = tiles[0], tiles[-1]
    lo, hi = min(mid[a] - half[a], mid[b] - half[b]), max(mid[a] + half[a], mid[b] + half[b])
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def super_distant(c, s, y, Mid, Half, factor=SUPER_DIST):
    """vamp::ff_super_distant and its edge bound"""
    distS = np.abs(Mid - c) - Half
    r2e = (distS * s) ** 2 + y * y
    return (distS >= factor * Half) & (r2e >= R2_M3), r2e


def super_ok(native, x):
    """the walker takes the distant pass at all: no guard bit, no line wide for every tile"""
    s, y, _ = npr.line_sy(native)
    half = tm.tile_geometry(x)[1]
    tiny = ~(y >= Y_TINY)
    reach = ~(s * np.maximum(np.abs(x[0] - native[:, 1]), np.abs(x[-1] - native[:, 1])) <= X_FAR)
    wide_all = s * half.max() <= 0.75
    return not (tiny.any() or reach.any() or wide_all.any())


def class_sets(native, x, factor=SUPER_DIST, super_on=True):
    """The sets of every adjacent batch of one walker: {tiles, far, n6, n4, n3, wide} as the ordinary pairs see them (the
    distant lines taken out), dist and d3, Mid and Half"""
    far, wide, _ = [m[0] for m in tm.classify(native[None], x)]
    r2e = npr.edge_r2(native, x)
    s, y, _ = npr.line_sy(native)
    ok = super_on and super_ok(native, x)          # (super_on False: a library built without the distant pass)
    out = []
    for tiles in batches(far.shape[1])[0]:
        f, r = far[:, tiles], r2e[:, tiles]
        Mid, Half = super_tile(x, tiles)
        d, rS = super_distant(native[:, 1], s, y, Mid, Half, factor)
        d = d & f.all(1) & ok
        keep = ~d
        out.append(dict(tiles=tiles, far=npr.bits(f.any(1) & keep), n6=npr.bits((f & (r < npr.R2_M4)).any(1) & keep),
                        n4=npr.bits((f & (r < R2_M3)).any(1) & keep), n3=npr.bits((f & (r < R2_M2)).any(1) & keep),
                        wide=npr.bits(wide[:, tiles].any(1)), dist=npr.bits(d), d3=npr.bits(d & (rS < R2_M2)), Mid=Mid, Half=Half))
    return out


def distant_order(sets):
    """[(line, depth)] in the order of vamp::super_order: three-level lines first, eight per iteration, an iteration at the
    depth of its deepest line"""
    ks = [k for k in range(16) if sets["d3"] >> k & 1] + [k for k in range(16) if (sets["dist"] & ~sets["d3"]) >> k & 1]
    it3 = (bin(sets["d3"]).count("1") + 7) // 8
    return [(k, 3 if i // 8 < it3 else 2) for i, k in enumerate(ks)]


def interpolate(fsum, t, C=None):
    """Clenshaw's recurrence at t[...] on the Chebyshev coefficients C fsum of the 16 super-node sums, in the precision of
    fsum"""
    C = table() if C is None else C
    coef = (C.astype(fsum.dtype) * fsum[None, :]).sum(1)
    t = np.asarray(t, fsum.dtype)
    b1, b2 = np.zeros_like(t), np.zeros_like(t)
    for k in range(NODES - 1, 0, -1):
        b1, b2 = 2 * t * b1 + (coef[k] - b2), b1
    return t * b1 + (coef[0] - b2)


def node_sums(native, x, factor=SUPER_DIST, C=None, exact_super=False, super_on=True):
    """nodes[nt, 16], mag, magw of one walker as the hook's adjacent form gives them: the ordinary pairs and the wide lines as
    tests/node_pass_ref.py restates them, the distant lines through the super-nodes -- the kernel's fractions there, in
    extended precision (exact_super: scipy's wofz), the transform and the recurrence in extended precision on the table
    as it is stored.  factor, C: planted errors (a shallower threshold, another table)."""
    mid, half = tm.tile_geometry(x)[:2]
    tn = cheb_nodes()
    far, wide, _ = [m[0] for m in tm.classify(native[None], x)]
    s, y, amp = npr.line_sy(native)
    nt = mid.size
    xn = mid[:, None] + half[:, None] * tn[None, :]
    X = np.abs(xn[None] - native[:, 1, None, None]) * s[:, None, None]
    out, mag, magw = np.zeros((nt, NODES)), np.zeros((nt, NODES)), np.zeros((nt, NODES))
    full, rest = batches(nt)
    for sets in class_sets(native, x, factor, super_on):
        tiles = sets["tiles"]
        if sets["dist"]:
            xs = sets["Mid"] + sets["Half"] * tn
            fsum = np.zeros(NODES, np.longdouble)
            for k, depth in distant_order(sets):
                Xs = np.abs(xs - native[k, 1]) * s[k]
                fsum += np.longdouble(amp[k]) * (npr.exact(Xs, y[k]) if exact_super else npr.fraction(depth, Xs, y[k]))
            for t in tiles:
                p = interpolate(fsum, (xn[t] - sets["Mid"]) / sets["Half"], C)
                out[t] += np.asarray(p, np.float64)
                mag[t] += np.abs(np.asarray(p, np.float64))
        for k0, k1, depth in npr.walk(sets):
            for k in (k0, k1):
                if k is None:
                    continue
                for t in tiles:
                    if far[k, t]:
                        term = amp[k] * npr.fraction(depth, X[k, t], y[k])
                        out[t] += term
                        mag[t] += np.abs(term)
        for k in range(native.shape[0]):
            for t in tiles:
                if wide[k, t]:
                    term = amp[k] * npr.exact(X[k, t], y[k])
                    out[t] += term
                    mag[t] += np.abs(term)
                    magw[t] += np.abs(term)
    for t in rest:
        for k in np.flatnonzero(far[:, t] | wide[:, t]):
            term = amp[k] * npr.exact(X[k, t], y[k])
            out[t] += term
            mag[t] += np.abs(term)
    return out, mag, magw


def near_pairs_per_wave(native, x):
    """near (line, tile) pairs of the four tile classes, (round-robin tiles, adjacent batches): the tile loops' load"""
    near = tm.classify(native[None], x)[2][0].sum(0)            # per tile
    nt = near.size
    rr = np.array([near[p::PARTS].sum() for p in range(PARTS)])
    full, rest = batches(nt)
    adj = np.zeros(PARTS, int)
    for i, tiles in enumerate(full):
        adj[i % PARTS] += near[tiles].sum()
    for t in rest:
        adj[(t - GROUP * (nt // GROUP)) % PARTS] += near[t]
    return rr, adj


if __name__ == "__main__":
    for name, kw in (("headline", {}), ("dispersed", dict(ensemble="dispersed"))):
        x, nat = npr.headline_natives(W=64, **kw)
        rr, adj, nd, nf = np.zeros(PARTS), np.zeros(PARTS), 0, 0
        worst_rr = worst_adj = 0.0
        for n in nat:
            a, b = near_pairs_per_wave(n, x)
            rr += a
            adj += b
            worst_rr, worst_adj = max(worst_rr, a.max() / a.mean()), max(worst_adj, b.max() / b.mean())
            for sets in class_sets(n, x):
                nd += 4 * bin(sets["dist"]).count("1")
            nf += tm.classify(n[None], x)[0][0].sum()
        print(f"{name:10s} near pairs per wavefront and walker: round-robin {np.round(rr / len(nat), 1)}, adjacent {np.round(adj / len(nat), 1)}; "
              f"busiest / mean, worst walker: {worst_rr:.3f} / {worst_adj:.3f}; distant share of the far pairs {nd / nf:.2f}")
