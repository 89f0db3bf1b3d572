"""numpy restatement of the node form of a far-field-only tile's chi^2 (helper, not a test module).

The absorption of a full tile without a near line is the degree-15 interpolant through the tile's 16 Chebyshev nodes,
a(x) = sum_n l_n(t) a_n with t = (x - mid) / half and l_n the Lagrange basis of the nodes t_n (the last 16 entries of
vamp_amd/csrc/ff_matrix.inc; the node abscissae are mid + half t_n whatever the grid's orientation).  So

    sum w^2 ((f - 1) + a)^2 = C0 + sum_n a_n (2 S'_n + sum_m Q'_nm a_m),
    S'_n = sum w^2 (f - 1) l_n,   Q'_nm = sum w^2 l_n l_m,   C0 = sum w^2 (f - 1)^2,

with the record (Q', S', C0, sum w^2) belonging to the data alone (k_tile_tables, VAMP_TILE_MOMENTS == 2; layout FFN_* in
vamp_amd/csrc/ff_moments.hpp).  Everything here follows the kernels: the basis in its barycentric form with the
denominator summed in node order, the record's sums in the kernel's order (eight chains and a tree; C0 and sum w^2 in
the wavefronts' butterflies), the form as the lanes of ff_moment_chi_nodes add it and the wavefront's butterfly sums it.
"""
import numpy as np

import tile_moments_ref as tm

TILE, NODES = tm.TILE, tm.NODES
FFN_S, FFN_C0, FFN_RC, FFN_RQ, FFN_TILE = 256, 272, 273, 274, 280      # vamp_amd/csrc/ff_moments.hpp


def nodes():
    """t_n = cos(pi (n + 1/2) / 16), n = 0..15, as the kernels read them"""
    return tm.ff_matrix()[1]


def tile_t(x):
    """(mid[nt], half[nt], t[nt, 256]) of a region's full tiles: the pixel's place in its tile, -1 .. 1"""
    nt = x.size // TILE
    xt = x[:nt * TILE].reshape(nt, TILE)
    lo, hi = xt[:, 0], xt[:, -1]
    mid, half = 0.5 * (lo + hi), 0.5 * np.abs(hi - lo)
    return mid, half, (xt - mid[:, None]) / half[:, None]


def lagrange(t, tn=None, dtype=np.float64):
    """l[..., 16] at t[...]: (w_n / (t - t_n)) / sum_m w_m / (t - t_m), w_n = (-1)^n sqrt((1 - t_n)(1 + t_n)); a pixel
    at a node has 1 there and 0 elsewhere"""
    tn = (nodes() if tn is None else tn).astype(dtype)
    t = np.asarray(t).astype(dtype)
    one = dtype(1)
    w = np.sqrt((one - tn) * (one + tn)) * np.where(np.arange(NODES) % 2 == 1, -one, one)
    diff = t[..., None] - tn
    hit = diff == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = w / diff
        den = np.zeros(t.shape, dtype)
        for n in range(NODES):
            den = den + c[..., n]
        ell = c / den[..., None]
    at = hit.any(axis=-1)
    ell[at] = hit[at].astype(dtype)
    return ell


def node_record(x, flux, noise, dtype=np.float64):
    """(Q[nt, 16, 16], S[nt, 16], C0[nt], W2[nt]) of the full tiles; every sum in k_tile_tables' order"""
    mid, half, t = tile_t(x)
    nt = mid.size
    ell = lagrange(t, dtype=dtype)
    w = (1.0 / noise[:nt * TILE].reshape(nt, TILE)).astype(dtype)       # (the context holds the weights in double)
    w2 = w * w
    d = flux[:nt * TILE].reshape(nt, TILE).astype(dtype) - 1
    w2d = w2 * d
    Q, S = np.zeros((8, nt, NODES, NODES), dtype), np.zeros((8, nt, NODES), dtype)
    for i in range(TILE):               # eight chains over the pixels i = k mod 8 ...
        Q[i % 8] = Q[i % 8] + w2[:, i, None, None] * (ell[:, i, :, None] * ell[:, i, None, :])
        S[i % 8] = S[i % 8] + w2d[:, i, None] * ell[:, i, :]
    tree = lambda v: ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))       # ... added as a tree
    # C0 and sum w^2: the butterfly of each wavefront's 64 pixels, then the four wavefronts' sums
    c0 = np.stack([[wave_sum(v[64 * k:64 * k + 64]) for k in range(4)] for v in w2d * d])
    q0 = np.stack([[wave_sum(v[64 * k:64 * k + 64]) for k in range(4)] for v in w2])
    four = lambda v: (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
    return tree(Q), tree(S), four(c0), four(q0)


def record_scale(x, flux, noise):
    """what the record's rounding is measured against: (sum w^2 |l_n l_m| [nt, 16, 16], sum w^2 |f - 1| |l_n| [nt, 16])"""
    mid, half, t = tile_t(x)
    nt = mid.size
    ell = np.abs(lagrange(t))
    w2 = (1.0 / noise[:nt * TILE].reshape(nt, TILE)) ** 2
    d = np.abs(flux[:nt * TILE].reshape(nt, TILE) - 1)
    return np.einsum("tp,tpn,tpm->tnm", w2, ell, ell), np.einsum("tp,tpn->tn", w2 * d, ell)


def lane_terms(a, S, Q, C0):
    """the 64 lanes' shares of one tile: lane 16 g + n holds a_n (sum_{k<4} Q[n, 4 g + k] a_{4 g + k} + S_n / 2), two
    chains of two; lane 0 adds C0"""
    a = np.asarray(a)
    terms = np.zeros(64, a.dtype)
    for g in range(4):
        for n in range(NODES):
            m = 4 * g
            acc0 = Q[n, m] * a[m] + a.dtype.type(0.5) * S[n]
            acc1 = Q[n, m + 1] * a[m + 1]
            acc0 = Q[n, m + 2] * a[m + 2] + acc0
            acc1 = Q[n, m + 3] * a[m + 3] + acc1
            terms[16 * g + n] = a[n] * (acc0 + acc1)
    terms[0] = terms[0] + C0
    return terms


def wave_sum(v):
    """the wavefront's butterfly: v += v[lane ^ off] for off = 32, 16, .., 1; every lane ends with the same sum"""
    v = np.array(v)
    lane = np.arange(v.size)
    off = v.size // 2
    while off >= 1:
        v = v + v[lane ^ off]
        off //= 2
    return v[0]


def chi2_nodes(a, S, Q, C0):
    """chi^2 of one tile from its node values a[16] as the lanes form and the wavefront sums it"""
    return wave_sum(lane_terms(a, S, Q, C0))


def chi2_direct(a, t, flux, noise):
    """the same sum pixel by pixel in the arithmetic of a's type: sum w^2 ((f - 1) + sum_n l_n(t) a_n)^2"""
    a = np.asarray(a)
    ell = lagrange(t, dtype=a.dtype.type)
    return ((((flux.astype(a.dtype) - 1) + ell @ a) / noise.astype(a.dtype)) ** 2).sum()


def node_absorption(native, x, tile):
    """(a_n[16], amax) of one walker's lines native[K', 4] at the nodes of tile `tile` of x: a_n = -expm1(-tau_n)"""
    mid, half, _ = tile_t(x)
    an = -np.expm1(-tm.voigt_tau(mid[tile] + half[tile] * nodes(), native).sum(axis=0))
    return an, np.abs(an).max()
