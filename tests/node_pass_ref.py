"""numpy restatement of the line-major node stage of the fp64 far-field loop (vamp_hip.hip: ff_classify_batch_np,
ff_node_pass) and the instruction model behind its design.

A wavefront sweeps one tile class (tiles p, p + 4, p + 8, ... of the region's full tiles) four tiles -- one batch -- at
a time.  For a full batch the node values of all four tiles are formed line by line: the lines that are far for some
tile of the batch are folded into nested sets by the deepest continued fraction any of those tiles needs, judged from
the edge bound r2e = (dist s)^2 + y^2 of the classification; the m-level fraction is the 2m-point Gauss-Hermite rule of
w's integral.  Tiles left over after a class's full batches keep the tile-by-tile stage.

    python tests/node_pass_ref.py        prints the model's lane-instructions per tile for the benchmark's ensembles
"""
import numpy as np

import tile_moments_ref as tm

TILE, NODES, BATCH, PARTS = tm.TILE, 16, 4, 4
R2_M4, R2_M3, R2_M2 = 100.0, 300.0, 2000.0       # VAMP_FF_R2_M4 / M3 / M2: below them the 6- / 4- / 3-level fraction
DEPTHS = (6, 4, 3, 2)
COST = {2: 20, 3: 26, 4: 32, 6: 44}               # vector instructions of one evaluation
SQRT_LN2 = tm.SQRT_LN2


def depth_of(r2):
    """the shallowest fraction valid at |z|^2 = r2"""
    return np.where(r2 < R2_M4, 6, np.where(r2 < R2_M3, 4, np.where(r2 < R2_M2, 3, 2)))


def line_sy(native):
    """(s, y, amp) of native[..., 4] = (A, c, L, G): X = |x - c| s, amp sqrt(pi) H(X, y) the optical depth"""
    A, L, G = native[..., 0], native[..., 2], native[..., 3]
    s, y = 2.0 * SQRT_LN2 / G, L * SQRT_LN2 / G
    return s, y, A * y


def fraction(m, X, y):
    """sqrt(pi) Re w(X + i y) by the 2m-point Gauss-Hermite rule: (1 / sqrt(pi)) sum_j w_j y / ((X - t_j)^2 + y^2), summed
    in extended precision (every term is positive: the restatement's own rounding is far below the rule's error)"""
    t, w = np.polynomial.hermite.hermgauss(2 * m)
    X, y = np.asarray(X, np.longdouble)[..., None], np.asarray(y, np.longdouble)[..., None]
    return np.asarray((w * y / ((X - t) ** 2 + y * y)).sum(-1) / np.sqrt(np.longdouble(np.pi)), np.float64)


def exact(X, y):
    from scipy.special import wofz
    return np.sqrt(np.pi) * wofz(X + 1j * y).real


def batches(ntile):
    """(full, rest): the full batches as rows of four tile indices, in the order class 0's batches, class 1's, ...; and
    the tiles that keep the tile-by-tile stage"""
    full, rest = [], []
    for p in range(PARTS):
        mine = list(range(p, ntile, PARTS))
        nb = len(mine) // BATCH
        full += [mine[BATCH * b:BATCH * b + BATCH] for b in range(nb)]
        rest += mine[BATCH * nb:]
    return np.array(full, int).reshape(-1, BATCH), sorted(rest)


def edge_r2(native, x):
    """r2e[K, nt] of one walker's lines (native[K, 4]) against the full tiles"""
    mid, half = tm.tile_geometry(x)[:2]
    s, y, _ = line_sy(native)
    dist = np.abs(mid[None, :] - native[:, 1, None]) - half[None, :]
    return (dist * s[:, None]) ** 2 + (y * y)[:, None]


def node_r2(native, x):
    """r2[K, nt, 16] at the tiles' Chebyshev nodes"""
    mid, half = tm.tile_geometry(x)[:2]
    nodes = tm.ff_matrix()[1]
    s, y, _ = line_sy(native)
    xn = mid[:, None] + half[:, None] * nodes[None, :]
    X = np.abs(xn[None] - native[:, 1, None, None]) * s[:, None, None]
    return X * X + (y * y)[:, None, None]


def bits(mask):
    return int(sum(1 << int(k) for k in np.flatnonzero(mask)))


def class_sets(native, x):
    """The folded sets of every full batch of one walker: a list of dicts {tiles, far, n6, n4, n3, wide} with the sets as
    bit masks over the lines, nested n6 <= n4 <= n3 <= far as the kernel keeps them"""
    far, wide, _ = [m[0] for m in tm.classify(native[None], x)]
    r2e = edge_r2(native, x)
    out = []
    for tiles in batches(far.shape[1])[0]:
        f, r = far[:, tiles], r2e[:, tiles]
        out.append(dict(tiles=tiles, far=bits(f.any(1)), n6=bits((f & (r < R2_M4)).any(1)), n4=bits((f & (r < R2_M3)).any(1)),
                        n3=bits((f & (r < R2_M2)).any(1)), wide=bits(wide[:, tiles].any(1))))
    return out


def set_depth(sets, k):
    return 6 if sets["n6"] >> k & 1 else 4 if sets["n4"] >> k & 1 else 3 if sets["n3"] >> k & 1 else 2


def walk(sets):
    """the pairs of the pass, deepest class first: [(k0, k1 or None, depth of the pair)]"""
    order = sorted((k for k in range(16) if sets["far"] >> k & 1), key=lambda k: (-set_depth(sets, k), k))
    return [(order[i], order[i + 1] if i + 1 < len(order) else None, set_depth(sets, order[i])) for i in range(0, len(order), 2)]


def node_sums(native, x, plant=None):
    """nodes[nt, 16], mag[nt, 16] (the sum of the terms' magnitudes) and magw[nt, 16] (the wide and mid lines' share of
    it) of one walker: full batches line by line as the pass forms them, the other tiles from the exact function.  plant: one of the errors the tests must be able to see --
    "shallow" (every class folded one level too shallow), "rowshift" (tile j of a batch reads tile j + 1's far mask),
    "nearfar" (a line far for some tile of the batch is added as far on all four), "widefar" (the wide pass also runs on
    the tiles where its line is far)."""
    mid, half = tm.tile_geometry(x)[:2]
    nodes = tm.ff_matrix()[1]
    far, wide, _ = [m[0] for m in tm.classify(native[None], x)]
    s, y, amp = line_sy(native)
    nt = mid.size
    xn = mid[:, None] + half[:, None] * nodes[None, :]
    X = np.abs(xn[None] - native[:, 1, None, None]) * s[:, None, None]                # [K, nt, 16]
    out, mag, magw = np.zeros((nt, NODES)), np.zeros((nt, NODES)), np.zeros((nt, NODES))
    shallower = {6: 4, 4: 3, 3: 2, 2: 2}
    full, rest = batches(nt)
    for sets in class_sets(native, x):
        tiles = sets["tiles"]
        for k0, k1, depth in walk(sets):
            m = shallower[depth] if plant == "shallow" else depth
            for k in (k0, k1):
                if k is None:
                    continue
                for j, t in enumerate(tiles):
                    src = tiles[(j + 1) % BATCH] if plant == "rowshift" else t
                    if far[k, src] or plant == "nearfar":
                        term = amp[k] * fraction(m, X[k, t], y[k])
                        out[t] += term
                        mag[t] += np.abs(term)
        for k in range(native.shape[0]):
            for t in tiles:
                if wide[k, t] or (plant == "widefar" and sets["wide"] >> k & 1 and far[k, t]):
                    term = amp[k] * exact(X[k, t], y[k])
                    out[t] += term
                    mag[t] += np.abs(term)
                    magw[t] += np.abs(term)
    for t in rest:
        for k in np.flatnonzero(far[:, t] | wide[:, t]):
            term = amp[k] * exact(X[k, t], y[k])
            out[t] += term
            mag[t] += np.abs(term)
    return out, mag, magw


def node_sums_exact(native, x):
    """the same sums from scipy's wofz alone"""
    mid, half = tm.tile_geometry(x)[:2]
    nodes = tm.ff_matrix()[1]
    far, wide, _ = [m[0] for m in tm.classify(native[None], x)]
    out = np.zeros((mid.size, NODES))
    for t in range(mid.size):
        sel = far[:, t] | wide[:, t]
        if sel.any():
            out[t] = tm.voigt_tau(mid[t] + half[t] * nodes, native[sel]).sum(0)
    return out


def chi2_from_nodes(native, x, flux, noise, nodes_tau):
    """chi^2 of the full tiles with the interpolated lines' optical depth taken from nodes_tau[nt, 16]: the transform,
    Horner's rule, the near lines exactly, exp per pixel"""
    Mat = tm.ff_matrix()[0]
    mid, half, up, u, q = tm.tile_geometry(x)
    near = tm.classify(native[None], x)[2][0]
    nt = mid.size
    total = 0.0
    for i in range(nt):
        sl = slice(i * TILE, (i + 1) * TILE)
        coef = (Mat @ nodes_tau[i]).reshape(4, tm.NS)
        tau = np.zeros(TILE)
        for j in range(tm.DEG, -1, -1):
            tau = tau * u[i] + coef[q, j]
        if near[:, i].any():
            tau = tau + tm.voigt_tau(x[sl], native[near[:, i]]).sum(0)
        total += (((flux[sl] - np.exp(-tau)) / noise[sl]) ** 2).sum()
    return total


# ---- the instruction model --------------------------------------------------------------------------------------------
def model_costs(native, x):
    """Evaluation lane-instructions per tile of one walker, (tile by tile, line-major).  Tile by tile: a tile's far list
    is ordered deep lines (dist < w25) first; a lane takes list entries grp, 4 + grp, 8 + grp, 12 + grp, two calls of two
    evaluations each, the depth of a call the deepest any of its points needs.  Line-major: two evaluations per pair of
    the batch's walk, at the pair's class."""
    far = tm.classify(native[None], x)[0][0]
    r2n = node_r2(native, x).min(-1)                                     # [K, nt]: the deepest any node needs
    s, y, _ = line_sy(native)
    mid, half = tm.tile_geometry(x)[:2]
    dist = np.abs(mid[None, :] - native[:, 1, None]) - half[None, :]
    w25 = np.sqrt(np.maximum(625.0 - y * y, 0.0)) / s
    nt = mid.size
    old = 0.0
    for t in range(nt):
        ks = np.flatnonzero(far[:, t])
        deep = dist[ks, t] < w25[ks]
        lst = list(ks[deep]) + list(ks[~deep])
        for call in (lst[:8], lst[8:]):
            if call:
                old += 2 * COST[int(depth_of(min(r2n[k, t] for k in call)))]
    new, full_tiles = 0.0, 0
    for sets in class_sets(native, x):
        new += sum(2 * COST[d] for _, _, d in walk(sets))
        full_tiles += BATCH
    return old / nt, (new / full_tiles if full_tiles else float("nan"))


def headline_natives(P=16384, K=16, W=64, seed=20240517, ensemble="truth", width_scale=1.0):
    """(x, native[W, K, 4]) of the benchmark's workload (bench.py make_workload, the same draws)"""
    rng = np.random.default_rng(seed)
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    scale = max(P / 16384.0, 1.0 / 16) * width_scale
    c, A = rng.uniform(-0.45 * P, 0.45 * P, K), rng.uniform(0.2, 3.0, K)
    G, L = rng.uniform(20.0, 200.0, K) * scale, rng.uniform(1.0, 20.0, K) * scale
    L = np.full(K, 10.0 * scale)
    rng.normal(0.0, 0.01, P)
    nat = np.stack([A, c, L, G], axis=1)[None] * (1.0 + 1e-3 * rng.standard_normal((W, K, 4)))
    if ensemble == "dispersed":
        r2 = np.random.default_rng(seed + 1)
        nat[:, :, 0] = r2.gamma(2.0, 1.0, (W, K))
        nat[:, :, 1] = r2.uniform(x[0], x[-1], (W, K))
        nat[:, :, 3] = np.exp(r2.uniform(np.log(5.0 * scale), np.log(800.0 * scale), (W, K)))
    fwhm_max = (x[-1] - x[0]) / 2.0 * 2.35482004503094938202
    nat[:, :, 0] = np.clip(nat[:, :, 0], 1e-6, None)
    nat[:, :, 1] = np.clip(nat[:, :, 1], x[0], x[-1])
    nat[:, :, 2:] = np.clip(nat[:, :, 2:], 1e-6, fwhm_max)
    return x, nat


if __name__ == "__main__":
    for name, kw in (("headline", {}), ("dispersed", dict(ensemble="dispersed")), ("width-scale 4", dict(width_scale=4.0)),
                     ("width-scale 0.25", dict(width_scale=0.25))):
        x, nat = headline_natives(W=16, **kw)
        c = np.array([model_costs(n, x) for n in nat]).mean(0)
        print(f"{name:18s} evaluation lane-instructions per tile: tile by tile {c[0]:6.1f}, line-major {c[1]:6.1f}")
