"""What the limit tests of libvamp_post.so and libvamp_diag.so share (tests/test_gpu_posterior_limits.py,
tests/test_gpu_diag_limits.py and the CPU controls of tests/test_side_limits.py): the case tables, the restated size
arithmetic of the two libraries -- restated, not imported, so that a case can say which path it takes and a control
can prove it -- and the numpy copies of the device-side merges in which the controls plant an error."""
import functools

import numpy as np

import chain_diag_ref as dref
import posterior_ref as pref
from oracle import vamp_oracle as vo

DEFAULT_LDS = 64 * 1024          # what a launch gets without hipFuncSetAttribute(MaxDynamicSharedMemorySize)
PROBS = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)      # PROBS of tests/test_gpu_posterior.py

# ---- posterior: the restated LDS arithmetic of k_post_eval ------------------------------------------------------------
DTAB_N = 44                      # vamp::DTAB_N of voigt_math.hpp
POST_REC = 6                     # kRec of posterior.hip
POST_MAX_K = 32                  # VAMP_POST_MAX_COMPONENTS
POST_WAVES = 4                   # kEvalWaves
EVAL_MAX_LDS = 119840            # kEvalMaxLds: what raise_lds_limit asks for k_post_eval


def group_lanes(K, P):
    """vamp::group_lanes with the narrow form on: 16 lanes own a sample of <= 4 lines on <= 32 pixels, else a wavefront"""
    return 16 if (P <= 32 and K <= 4) else 64


def slot_doubles(K, lanes):
    """LDS of one sample: K records and near-axis tables, and the [K + 1][lanes + 1] tile of the decrements"""
    return K * (POST_REC + DTAB_N) + (K + 1) * (lanes + 1)


def post_eval_lds_bytes(K, P):
    """dynamic LDS of a k_post_eval launch whose largest item is (K, P): four wavefronts of 64 / lanes slots"""
    lanes = group_lanes(K, P)
    return 8 * POST_WAVES * (64 // lanes) * slot_doubles(K, lanes)


# ---- posterior: cases ---------------------------------------------------------------------------------------------------
def centred_x(P):
    return np.arange(P, dtype=np.float64) - 0.5 * (P - 1)


def drawn_group(rng, P, K, mode, N, W, sd=False):
    """(x, chain [N, W, D]): half of the ensemble from the prior, half a 1 % ball around its first sample"""
    x = centred_x(P)
    S = N * W
    th = pref.draw_prior(rng, x, K, mode, S, bool(sd))
    if S > 1:
        th[S // 2:] = pref.ball(rng, th[0], S - S // 2)
    return x, th.reshape(N, W, -1)


# (mode, K, P, N, W, sample_sd) in call order.  K = 32 with the free sd is D = 129; S = N W = 5, 64, 65, 129 (the task
# boundary of a workgroup: 64 samples); the two narrow groups sit between K = 32 neighbours, whose 119 840 B launch they share
BIG_LDS = [(1, 32, 2, 1, 5, 1), (0, 2, 20, 4, 5, 0), (1, 32, 64, 1, 5, 1), (1, 4, 32, 4, 5, 1), (1, 32, 65, 1, 5, 1),
           (1, 32, 129, 1, 5, 1), (1, 18, 70, 4, 16, 0), (0, 18, 70, 4, 16, 0), (1, 18, 70, 5, 13, 0), (0, 18, 70, 5, 13, 0),
           (1, 18, 70, 3, 43, 0), (0, 18, 70, 3, 43, 0)]
BIG_LDS_NARROW = (1, 3)          # their places in BIG_LDS

JUST_UNDER = (1, 17, 300, 3, 8, 0)                     # 64 640 B: the largest launch that needs no raise

# (P, K) x mode x S: S = 17 and 20 are a second round of one sample, or of four, on the 16 slots of a workgroup's narrow rounds
NARROW_CORNER = [(mode, K, P, 1, S, 0) for mode in (0, 1) for S in (17, 20) for P in (32, 33) for K in (4, 5)]

REGIME_G = (1e-3, 0.3, 3.0, 300.0)
REGIME_RATIO = (0.0, 1e-12, 1e-6, 1e-3, 0.1, 1.0, 10.0, 1e3)       # L / G
REGIME_A = (0.5, 50.0)
REGIME_P, REGIME_CENTRE = 65, 0.3


def regime_lines():
    """(A, c, L, G) of the evaluator sweep, G slowest"""
    return [(A, REGIME_CENTRE, r * G, G) for G in REGIME_G for r in REGIME_RATIO for A in REGIME_A]


def regime_x():
    return np.arange(REGIME_P, dtype=np.float64) - (REGIME_P - 1) // 2          # unit spacing


def regime_groups():
    """(x, chain [1, 1, D], K): every line alone, then neighbouring entries paired.  One sample per group, so every flux
    statistic is that sample's flux"""
    lines, x = regime_lines(), regime_x()
    out = [(x, np.array(ln, dtype=np.float64).reshape(1, 1, 4), 1) for ln in lines]
    out += [(x, np.array(lines[i] + lines[i + 1], dtype=np.float64).reshape(1, 1, 8), 2) for i in range(0, len(lines), 2)]
    return out


def regime_points():
    """(X, y) of every (line, pixel) of the sweep in the evaluator's units: X = 2 sqrt(ln 2) |x - c| / G, y = sqrt(ln 2) L / G"""
    s = np.sqrt(np.log(2.0))
    x = regime_x()
    X = np.concatenate([2.0 * s * np.abs(x - c) / G for _, c, _, G in regime_lines()])
    y = np.concatenate([np.full(x.size, s * L / G) for _, _, L, G in regime_lines()])
    return X, y


def nan_flux_group(width):
    """21 good samples of two Voigt lines, one of which (sample 7) has a NaN flux: amplitudes +-1e300 at L / G = 1e10, so
    that A y overflows in the library and the product A L sqrt(pi ln 2) / G in the oracle: tau = inf - inf"""
    rng = np.random.default_rng(47)
    x = centred_x(9)
    th = pref.draw_prior(rng, x, 2, vo.MODE_VOIGT4, 21)
    th[7] = [1e300, 0.3, 1e10, 1.0, -1e300, -0.2, 1e10, 1.0]
    return x, th.reshape(3, 7, 8), width


# ---- diagnostics: the restated task arithmetic ------------------------------------------------------------------------
DIAG_SMALL_N = 2048              # kSmallN: R = 8 lags per lane and 256 threads up to here, R = 16 and 512 threads above
DIAG_TILE_SMALL = 4096           # kTileSmall
DIAG_TILE_LARGE = 8192 + 32      # kTileLarge
DIAG_MAX_WC = 64                 # kMaxWc


def diag_chunk(N):
    """walkers_per_chunk of chain_diag.hip"""
    wc = DIAG_TILE_SMALL // (N + 16) if N <= DIAG_SMALL_N else DIAG_TILE_LARGE // (N + 32)
    return min(wc, DIAG_MAX_WC)


def diag_nchunks(N, W):
    wc = diag_chunk(N)
    return (W + wc - 1) // wc


# ---- diagnostics: cases -------------------------------------------------------------------------------------------------
# More than 64 chunks per pair: name -> (N, W, D, seed, parameter that gets the offset, k, agreement measured at k and k + 1).
# k is the largest power of ten of the offset at which the float64 restatement still agrees to 1e-10 with direct sums in
# np.longdouble (test_side_limits.py::test_offset_cases_k_is_the_largest_the_restatement_carries measures both figures)
MANY_CHUNKS = {
    "wc1-200": (2048, 200, 2, 61, 1, 7, 8.5e-12, 2.5e-10),
    "wc2-65": (1400, 130, 3, 62, 2, 7, 1.9e-11, 4.2e-10),
    "large-wc1-70": (4100, 70, 1, 63, 0, 7, 1.7e-11, 2.9e-10),
}
MANY_CHUNKS_COUNTS = {"wc1-200": (1, 200), "wc2-65": (2, 65), "large-wc1-70": (1, 70)}       # (Wc, chunks)
OFFSET_RTOL = 1e-10


@functools.lru_cache(maxsize=None)
def many_chunks_chain(name, k=None):
    """the AR(1) chain of a MANY_CHUNKS case; its marked parameter moved by 10^k (the table's k unless given)"""
    N, W, D, seed, d, k_tab = MANY_CHUNKS[name][:6]
    x = dref.ar1(np.random.default_rng(seed), N, W, D, 0.5)
    x[:, :, d] += 10.0 ** (k_tab if k is None else k)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def many_chunks_want(name):
    return dref.diagnostics(many_chunks_chain(name))


def direct_longdouble(x, c=5.0):
    """tau, r_hat and the window of ONE parameter's [N, W] series by the definition (DESIGN.md "Chain diagnostics"), with
    direct lag sums in np.longdouble: lags are added until the window rule holds, so the cost is O(N W M)"""
    x = np.asarray(x, dtype=np.longdouble)
    N, W = x.shape
    n = N // 2
    y = x - x.mean(0)
    c0 = (y * y).sum(0)
    P, tau, M = np.longdouble(0), None, None
    for k in range(N):
        P = P + ((y[:N - k] * y[k:]).sum(0) / c0).mean()
        tau = 2 * P - 1
        if k >= c * tau:
            M = k
            break
    assert M is not None
    seq = np.concatenate([x[:n], x[N - n:]], axis=1)
    means = seq.mean(0)
    V = (((seq - means) ** 2).sum(0) / (n - 1)).mean()
    B = n * ((means - means.mean()) ** 2).sum() / (2 * W - 1)
    return tau, np.sqrt(((n - 1) / np.longdouble(n) * V + B / n) / V), M


def offset_agreement(name, k):
    """largest relative difference of (tau, r_hat) between the float64 restatement and the longdouble direct sums on the
    offset parameter of a MANY_CHUNKS case at offset 10^k; the windows must be equal"""
    d = MANY_CHUNKS[name][4]
    x = many_chunks_chain(name, k)[:, :, d:d + 1]
    tau, _, rh, win, _ = dref.diagnostics(x)
    t_ld, r_ld, M = direct_longdouble(x[:, :, 0])
    if int(win[0]) != M:
        return np.inf
    return float(max(abs(tau[0] / t_ld - 1), abs(rh[0] / r_ld - 1)))


# path and chunk boundaries: (N, W, D) in call order; the N = 3 group in the middle is answered on the host
BOUNDARY_SHAPES = ([(48, 130, 2), (49, 130, 2), (2048, 5, 2), (2049, 5, 2), (8192, 3, 1)] +
                   [(N, 66, 2) for N in (4, 5, 8, 9, 15)] + [(3, 40, 2)] + [(N, 66, 2) for N in (16, 17, 31, 32, 33)] +
                   [(200, 1, 2), (1000, 5, 2)])

WINDOW_FACTORS = (1.0, 2.5, 10.0)
WINDOW_SHAPE = (993, 64, 3)
LONG_WINDOW = (2000, 16, 2, 0.98, 71)                   # N, W, D, rho, seed: every window beyond lag 128 (asserted)

STUCK_SHAPE = (300, 130, 4)                             # Wc 12, 11 chunks, the last one of 10 walkers


def stuck_chain():
    N, W, D = STUCK_SHAPE
    x = dref.ar1(np.random.default_rng(72), N, W, D, 0.5)
    wc = diag_chunk(N)
    x[:, W - 5, 0] = x[0, W - 5, 0]                      # one stuck walker, in the last chunk
    x[:, 3 * wc:4 * wc, 1] = x[0, 3 * wc:4 * wc, 1]      # every walker of chunk 3 stuck (w_inv = 0 for the whole chunk)
    x[:, :, 2] = x[0, :, 2]                              # every walker constant at its own value: V = 0, B > 0
    return x


NONFINITE_SHAPES = ((300, 30, 4), (2100, 5, 4))         # small path: Wc 12, 3 chunks; large path: Wc 3, 2 chunks


def nonfinite_chains(shape, seed):
    """two four-parameter groups of one shape.  First: a NaN in an ordinary walker, a +inf, a NaN in an otherwise constant
    walker, a clean parameter.  Second: a NaN in a walker of the last chunk, a clean parameter, a -inf beside a stuck
    walker, a parameter with a stuck walker and no value that is not finite"""
    N, W, D = shape
    rng = np.random.default_rng(seed)
    a, b = dref.ar1(rng, N, W, D, 0.5), dref.ar1(rng, N, W, D, 0.5)
    a[N // 3, 1, 0] = np.nan
    a[N - 1, 2, 1] = np.inf
    a[:, 0, 2] = 4.25
    a[7, 0, 2] = np.nan
    b[0, W - 1, 0] = np.nan
    b[:, 1, 2] = -1.5
    b[N // 2, W - 2, 2] = -np.inf
    b[:, 2, 3] = 0.5
    return a, b


# ---- numpy copies of two device-side merges, for the planted errors of the controls ---------------------------------------
def chan_combine(a, b, wrong_count=False):
    """chan_combine of chain_diag.hip on (n, mean, M2) triples; ``wrong_count`` plants the error: the merged triple keeps
    the receiving side's count"""
    (na, ma, m2a), (nb, mb, m2b) = a, b
    if nb == 0.0:
        return a
    if na == 0.0:
        return b
    nn, d = na + nb, mb - ma
    return (na if wrong_count else nn), ma + d * (nb / nn), m2a + m2b + d * d * (na * nb / nn)


def finish_r_hat(x, wrong_lane=None):
    """split-R-hat of one parameter's [N, W] series the way the two kernels build it: Welford over the 2 wn sequence means
    of every chunk, the chunks merged per lane (ch = lane, lane + 64, ...) and then down a shuffle tree.  ``wrong_lane``:
    that lane's per-lane merges use the planted wrong count"""
    N, W = x.shape
    n, wc = N // 2, diag_chunk(N)
    parts, ssq = [], 0.0
    for w0 in range(0, W, wc):
        cnt = mean = m2 = 0.0
        for w in range(w0, min(w0 + wc, W)):
            for h in (x[:n, w], x[N - n:, w]):
                hm = h.sum() / n
                cnt += 1.0
                d = hm - mean
                mean += d / cnt
                m2 += d * (hm - mean)
                ssq += ((h - hm) ** 2).sum() / (n - 1)
        parts.append((cnt, mean, m2))
    lanes = [(0.0, 0.0, 0.0)] * 64
    for ch, p in enumerate(parts):
        lanes[ch % 64] = chan_combine(lanes[ch % 64], p, wrong_count=(ch % 64 == wrong_lane and ch >= 64))
    o = 32
    while o >= 1:
        for lane in range(64 - o):
            lanes[lane] = chan_combine(lanes[lane], lanes[lane + o]) if lane < o else lanes[lane]
        o >>= 1
    m2 = lanes[0][2]
    B, V = n / (2.0 * W - 1.0) * m2, ssq / (2.0 * W)
    return np.sqrt(((n - 1.0) / n * V + B / n) / V)


def decrement_sums(tau, owners=None):
    """the K + 1 decrement sums of one sample the way k_post_eval's wide form adds them: rounds of 64 pixels leave
    1 - exp(-tau_k) and 1 - flux in a [K + 1][64] tile, and lane j < owners adds row j in pixel order.  tau [K, P];
    owners = K + 1 unless a control drops the last summing lane"""
    K, P = tau.shape
    owners = K + 1 if owners is None else owners
    acc = np.zeros(K + 1)
    for r0 in range(0, P, 64):
        t = tau[:, r0:r0 + 64]
        tile = np.vstack([1.0 - np.exp(-t), 1.0 - np.exp(-t.sum(0))[None, :]])
        for j in range(owners):
            for v in tile[j]:
                acc[j] += v
    return acc
