"""Host half of the node form of a far-field-only tile's chi^2 (ff_moment_chi_nodes, k_tile_tables with
VAMP_TILE_MOMENTS == 2; tests/tile_moments_nodes_ref.py is the restatement):

  * identity: node form = long-double direct sum of the interpolant to the rounding the guard assumes, 8 2^-53 M with
    M = (sqrt C0 + amax sqrt sum w^2)^2 -- a condition, not a measurement;
  * the record: Q' symmetric, sum_n l_n = 1, the same record for a grid and its mirror image;
  * agreement of the two interpolants (Lagrange basis / the four series of the 56 x 16 matrix) on smooth absorptions;
  * detectability: the restatement on the a2 data of tests/test_gpu_tile_moments.py deviates from the oracle's chi^2 by more
    than 1e-12 of it for some walker and by less than the guard's bound for all, so that
    test_rounding_signature_of_the_path keeps its meaning when the kernels sum the node form;
  * planted errors fail the identity.
"""
import math

import numpy as np
import pytest

import test_gpu_tile_moments as gm
import tile_moments_nodes_ref as tn
import tile_moments_ref as tm

EPS = 2.0 ** -53
LD = np.longdouble
SETTINGS = [(0.01, 0.01), (0.01, 0.2), (0.05, 0.5), (1e-3, 1e-3), (1e-10, 0.1), (0.01, 7.7e-4)]


def _smooth_nodes(rng, depth):
    """node values of a smooth absorption of size `depth`: a Chebyshev series with halving coefficients"""
    c = rng.standard_normal(tn.NODES) * depth * 0.5 ** np.arange(tn.NODES)
    return np.polynomial.chebyshev.chebval(tn.nodes(), c)


def _random_tile(rng, sd, depth, down=False):
    x = np.arange(tn.TILE, dtype=np.float64) + rng.uniform(-1e4, 1e4)
    if down:
        x = x[::-1].copy()
    a = _smooth_nodes(rng, depth)
    t = tn.tile_t(x)[2][0]
    noise = np.full(tn.TILE, sd) * rng.uniform(0.5, 2.0, tn.TILE)
    flux = 1.0 - tn.lagrange(t) @ a + rng.normal(0, 1, tn.TILE) * noise
    return x, flux, noise, a, t


def _share(x, flux, noise, a, t, plant=None):
    """|node form - long-double direct sum| in units of 8 2^-53 M; `plant`: an error planted into the form's inputs"""
    Q, S, C0, W2 = [v[0] for v in tn.node_record(x, flux, noise)]
    af = a
    if plant == "columns":                                  # a column block of Q' in another block's place
        Q = Q.copy()
        Q[:, 0:4], Q[:, 4:8] = Q[:, 4:8].copy(), Q[:, 0:4].copy()
    elif plant == "no_s":                                   # 2 S' dropped
        S = np.zeros_like(S)
    elif plant == "reversed":                               # node order taken from the grid's orientation
        af = a[::-1].copy()
    got = tn.chi2_nodes(af, S, Q, C0)
    want = tn.chi2_direct(a.astype(LD), t, flux, noise)
    r = math.sqrt(C0) + np.abs(a).max() * math.sqrt(W2)
    return abs(float(got - want)) / (tm.GUARD_ULPS * EPS * r * r)


@pytest.mark.parametrize("sd,depth", SETTINGS)
def test_node_form_is_the_direct_sum_to_rounding(sd, depth):
    rng = np.random.default_rng(int(1e6 * depth) + 11)
    worst = max(_share(*_random_tile(rng, sd, depth, down=bool(k % 2))) for k in range(40))
    print(f"sd={sd} depth={depth}: worst |node form - direct sum| = {worst:.3f} of 8 2^-53 M")
    assert worst <= 1.0


@pytest.mark.parametrize("plant", ["columns", "no_s", "reversed"])
@pytest.mark.parametrize("sd,depth", [(0.01, 0.01), (0.05, 0.5)])
def test_planted_errors_fail_the_identity(sd, depth, plant):
    rng = np.random.default_rng(int(1e6 * depth) + 13)
    shares = [_share(*_random_tile(rng, sd, depth, down=True), plant=plant) for _ in range(10)]
    print(f"sd={sd} depth={depth} {plant}: |planted form - direct sum| = {min(shares):.3g} .. {max(shares):.3g} of 8 2^-53 M")
    assert min(shares) > 1.0


@pytest.mark.parametrize("kind", ["up", "down", "steps"])
def test_record_of_the_restatement(kind):
    P = 2304 + 100
    x = np.cumsum(np.where((np.arange(P) // tn.TILE) % 2 == 0, 1.0, 2.0)) if kind == "steps" else np.arange(P, dtype=np.float64)
    x = x - 0.5 * (x[0] + x[-1])
    if kind == "down":
        x = x[::-1].copy()
    rng = np.random.default_rng(len(kind))
    flux = 1.0 - 0.3 * np.exp(-0.5 * ((x - 40.0) / 90.0) ** 2) + rng.normal(0, 0.02, P)
    noise = 0.02 * rng.uniform(0.5, 2.0, P)
    Q, S, C0, W2 = tn.node_record(x, flux, noise)
    assert Q.shape == (9, 16, 16) and S.shape == (9, 16) and C0.shape == (9,) and W2.shape == (9,)
    assert np.array_equal(Q, Q.transpose(0, 2, 1))                          # w^2 (l_n l_m): symmetric to the bit
    t = tn.tile_t(x)[2]
    ell = tn.lagrange(t)
    assert np.abs(t).max() <= 1.0 and np.abs(ell.sum(axis=-1) - 1.0).max() <= 64 * EPS
    assert np.abs(ell).sum(axis=-1).max() < 3.0                             # the Lebesgue constant of 16 Chebyshev nodes
    assert np.allclose(Q.sum(axis=(1, 2)), W2, rtol=1e-13)
    # against sums in extended precision.  A term w^2 l_n l_m: l is a quotient of sums of 16 terms c_m with
    # sum |c_m| / |sum c_m| < 3, i.e. ~50 roundings each, ~100 for the product, and the sum of 256 terms adds 256
    Ql, Sl, Cl, Wl = tn.node_record(x, flux, noise, dtype=LD)
    qabs, sabs = tn.record_scale(x, flux, noise)
    assert np.all(np.abs(Q - Ql) <= (256 + 128) * 2 * EPS * qabs)
    assert np.all(np.abs(S - Sl) <= (256 + 128) * 2 * EPS * sabs)
    assert np.all(np.abs(C0 - Cl) <= 300 * 2 * EPS * C0) and np.all(np.abs(W2 - Wl) <= 300 * 2 * EPS * W2)
    # the mirror image of the grid (same abscissae, same data): the same record, tiles in reverse order
    xm, fm, nm = x[:2304], flux[:2304], noise[:2304]
    A = tn.node_record(xm, fm, nm)
    B = tn.node_record(xm[::-1].copy(), fm[::-1].copy(), nm[::-1].copy())
    qa, sa = tn.record_scale(xm, fm, nm)
    assert np.all(np.abs(B[0][::-1] - A[0]) <= (256 + 128) * 4 * EPS * qa)
    assert np.all(np.abs(B[1][::-1] - A[1]) <= (256 + 128) * 4 * EPS * sa)
    assert np.all(np.abs(B[2][::-1] - A[2]) <= 600 * 2 * EPS * A[2]) and np.all(np.abs(B[3][::-1] - A[3]) <= 600 * 2 * EPS * A[3])


def test_pixel_at_a_node():
    t = np.concatenate([tn.nodes()[[0, 7, 15]], [0.3]])
    ell = tn.lagrange(t)
    assert np.isfinite(ell).all()
    assert np.array_equal(ell[0], np.eye(16)[0]) and np.array_equal(ell[1], np.eye(16)[7]) and np.array_equal(ell[2], np.eye(16)[15])
    near = tn.lagrange(np.nextafter(tn.nodes()[7], 1.0))
    assert abs(near[7] - 1.0) < 1e-12 and np.abs(np.delete(near, 7)).max() < 1e-12


def test_interpolants_agree_on_smooth_absorptions():
    """far wings as the classification admits them (centre >= 2 half-widths beyond the tile's edge): the interpolant
    through the nodes in the Lagrange basis against the four series of the 56 x 16 matrix, pixel by pixel"""
    Mat, nodes = tm.ff_matrix()
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in range(40):
        x = np.arange(tn.TILE, dtype=np.float64) + rng.uniform(-1e4, 1e4)
        if k % 2:
            x = x[::-1].copy()
        mid, half, up, u, q = tm.tile_geometry(x)
        t = tn.tile_t(x)[2][0]
        c = mid[0] + rng.choice([-1.0, 1.0]) * half[0] * rng.uniform(3.0, 6.0)
        g = rng.uniform(2.0, 40.0)
        an = rng.uniform(1e-4, 0.2) * (half[0] ** 2 + g * g) / ((mid[0] + half[0] * nodes - c) ** 2 + g * g)
        b = (Mat @ an).reshape(4, tm.NS)
        series = np.zeros(tn.TILE)
        for j in range(tm.DEG, -1, -1):
            series = series * u[0] + b[q, j]
        worst = max(worst, np.abs(series - tn.lagrange(t) @ an).max() / np.abs(an).max())
    print(f"largest per-pixel difference of the two interpolants: {worst:.3e} of amax")
    assert worst < 1e-12


@pytest.mark.parametrize("P,kind,K,m", [c[:4] for c in gm.CASES if c[4] == "a"])
def test_a2_data_show_the_node_form(P, kind, K, m):
    c = gm.case(P, kind, K, m, "a")
    flux, noise = c["data"]["a2"]
    x = c["x"]
    Q, S, C0, W2 = tn.node_record(x, flux, noise)
    far, wide, near = tm.classify(c["native"], x)
    dev = np.zeros(gm.W)
    for w in range(gm.W):
        # the first tile in index order holds the data (noise 1e30 beyond it: 1e-60 of a chi^2 either way)
        assert not near[w, :, 0].any()
        an, amax = tn.node_absorption(c["native"][w][far[w, :, 0] | wide[w, :, 0]], x, 0)
        assert tm.guard_try(C0[0], W2[0]) and tm.guard_ok(C0[0], W2[0], amax)
        dev[w] = abs(tn.chi2_nodes(an, S[0], Q[0], C0[0]) - c["chi_a2"][w])
    want = c["chi_a2"]
    print(f"NODE-SIG P={P} {kind} K={K} {m}: deviation {dev.min():.3e} .. {dev.max():.3e}, largest in units of 1e-12 chi^2: "
          f"{(dev / (1e-12 * want)).max():.3e}; guard bound {tm.GUARD_BOUND:.3e}")
    assert (dev > 1e-12 * want).any()
    assert (dev < tm.GUARD_BOUND).all()
