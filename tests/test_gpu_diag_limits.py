"""GPU tests of libvamp_diag.so where it changes path (cases and restated task arithmetic: tests/side_limit_cases.py; CPU
controls: tests/test_side_limits.py): more than 64 chunks per pair with a parameter far from zero, the chunk-size and
path boundaries from both sides, the edges of the register-blocked lag loop, W = 1 and a last chunk of one walker, window
factors other than 5, a window that carries over several 64-lag blocks, stuck chunks, R-hat = +inf, the rule for values
that are not finite, and a caller's stream with device-resident groups.  Compared with tests/chain_diag_ref.py through
_same of tests/test_gpu_chain_diagnostics.py: rtol 1e-9, equal windows, equal `reliable`."""
import numpy as np
import pytest

import chain_diag_ref as ref
import side_limit_cases as sc
from test_gpu_chain_diagnostics import _same

pytestmark = pytest.mark.gpu


def _worst(got, want):
    """largest relative difference of the finite tau and r_hat (printed, not asserted: _same asserts)"""
    out = []
    g = got if isinstance(got, tuple) else (got.tau, got.n_eff, got.r_hat)
    for a, b in ((g[0], want[0]), (g[2], want[2])):
        fin = np.isfinite(b) & (np.abs(b) > 1e-12)
        out.append(float(np.max(np.abs(a[fin] / b[fin] - 1))) if fin.any() else 0.0)
    return out


@pytest.mark.parametrize("name", list(sc.MANY_CHUNKS))
def test_more_than_64_chunks_per_pair(name):
    """k_chain_finish's per-lane chan_combine loop and the shuffle tree behind it, with one parameter at 10^k: without
    Chan's merge of the chunks' sequence means R-hat would lose k digits"""
    from vamp_amd.diagnostics import chain_diagnostics
    N, W, D, seed, d, k = sc.MANY_CHUNKS[name][:6]
    assert (sc.diag_chunk(N), sc.diag_nchunks(N, W)) == sc.MANY_CHUNKS_COUNTS[name] and sc.diag_nchunks(N, W) > 64
    x = sc.many_chunks_chain(name)
    assert x.shape == (N, W, D) and abs(x[:, :, d].mean() / 10.0 ** k - 1) < 1e-3
    got = chain_diagnostics(np.array(x))
    want = sc.many_chunks_want(name)
    print("diag", name, "chunks", sc.diag_nchunks(N, W), "offset 1e%d" % k, "max rel err tau, r_hat", _worst(got, want))
    _same(got, want)
    assert np.all(got.reliable)


def test_path_and_chunk_boundaries_in_one_ragged_call():
    """N = 48 | 49 (Wc 64 -> 63), 2048 | 2049 (R 8 -> 16, the LDS attribute), 8192 with three walkers, N around the
    multiples of R on the small path (n - 1 = 1 in the half variances at N = 4, 5), W = 1 (2 W - 1 = 1), W = Wc + 1, and the
    N = 3 group the host answers in the middle; rows longer than W D"""
    from vamp_amd import diagnostics
    rng = np.random.default_rng(64)
    shapes = sc.BOUNDARY_SHAPES
    assert [sc.diag_chunk(N) for N in (48, 49, 2048, 2049, 8192, 1000)] == [64, 63, 1, 3, 1, 4]
    blocks, want, lds = [], [], []
    for N, W, D in shapes:
        ld = W * D + int(rng.integers(1, 9))
        raw = rng.standard_normal((N, ld)) * 3.0 + 100.0
        x = ref.ar1(rng, N, W, D, float(rng.uniform(0.0, 0.9)))
        raw[:, :W * D] = x.reshape(N, W * D) * rng.uniform(0.01, 100.0) + rng.uniform(-1e3, 1e3)
        blocks.append(np.ascontiguousarray(raw))
        want.append(ref.diagnostics(raw[:, :W * D].reshape(N, W, D)))
        lds.append(ld)
    flat = diagnostics._call(0, [b.ctypes.data for b in blocks], False, lds, [s[0] for s in shapes], [s[1] for s in shapes],
                             [s[2] for s in shapes], 5.0)
    o = 0
    for (N, W, D), w in zip(shapes, want):
        got = tuple(a[o:o + D] for a in flat)
        print("diag boundary N %d W %d Wc %d chunks %d window" % (N, W, sc.diag_chunk(N) if N >= 4 else 0, sc.diag_nchunks(N, W) if N >= 4 else 0),
              w[3], "max rel err tau, r_hat", _worst(got, w))
        _same(got, w)
        o += D
    assert o == flat[0].size


def test_window_factors():
    from vamp_amd.diagnostics import chain_diagnostics
    x = ref.ar1(np.random.default_rng(65), *sc.WINDOW_SHAPE, 0.8)
    windows = []
    for c in sc.WINDOW_FACTORS:
        want = ref.diagnostics(x, c=c)
        got = chain_diagnostics(x, c=c)
        print("diag window factor", c, "window", want[3], "max rel err tau, r_hat", _worst(got, want))
        _same(got, want)
        windows.append(want[3])
    assert np.all(windows[0] < windows[1]) and np.all(windows[1] < windows[2])      # the factor is used


def test_window_beyond_two_blocks_of_lags():
    """rho = 0.98: the window lies beyond lag 128, so the prefix sum's carry crosses at least two 64-lag blocks"""
    from vamp_amd.diagnostics import chain_diagnostics
    N, W, D, rho, seed = sc.LONG_WINDOW
    x = ref.ar1(np.random.default_rng(seed), N, W, D, rho)
    want = ref.diagnostics(x)
    assert np.all(want[3] > 128), want[3]
    got = chain_diagnostics(x)
    print("diag long window", want[3], "max rel err tau, r_hat", _worst(got, want))
    _same(got, want)


def test_stuck_chunks_and_every_walker_constant():
    from vamp_amd.diagnostics import chain_diagnostics
    N, W, D = sc.STUCK_SHAPE
    assert sc.diag_chunk(N) == 12 and sc.diag_nchunks(N, W) == 11
    x = sc.stuck_chain()
    got = chain_diagnostics(x)
    _same(got, ref.diagnostics(x))
    assert np.all(got.tau[:3] == np.inf) and np.all(got.n_eff[:3] == 0) and np.all(got.window[:3] == -1) and not got.reliable[:3].any()
    assert np.isfinite(got.r_hat[:2]).all() and got.r_hat[2] == np.inf
    assert np.isfinite(got.tau[3]) and got.window[3] > 0 and got.reliable[3]


@pytest.mark.parametrize("shape, seed", list(zip(sc.NONFINITE_SHAPES, (81, 82))))
def test_values_that_are_not_finite(shape, seed):
    """the rule of include/vamp_diag.h on both paths: a NaN or an infinity anywhere in a parameter's series gives NaN,
    window -1, not reliable for that parameter and no other; it comes before "stuck" """
    from vamp_amd.diagnostics import chain_diagnostics
    assert sc.diag_nchunks(shape[0], shape[1]) > 1
    a, b = sc.nonfinite_chains(shape, seed)
    ga, gb = chain_diagnostics([a, b])
    _same(ga, ref.diagnostics(a))
    _same(gb, ref.diagnostics(b))
    for g, bad, clean in ((ga, [0, 1, 2], [3]), (gb, [0, 2], [1])):
        for arr in (g.tau, g.n_eff, g.r_hat):
            assert np.isnan(arr[bad]).all() and np.isfinite(arr[clean]).all()
        assert np.all(g.window[bad] == -1) and not g.reliable[bad].any() and g.reliable[clean].all()
    assert gb.tau[3] == np.inf and gb.n_eff[3] == 0 and gb.window[3] == -1 and np.isfinite(gb.r_hat[3])      # stuck, and finite


def test_callers_stream_and_three_device_resident_groups():
    """three groups in separate device tensors with rows longer than W D, on a stream that is not the default one: every
    output equals the host call's bit for bit"""
    import torch
    from vamp_amd import diagnostics
    rng = np.random.default_rng(66)
    shapes = [(180, 70, 3), (2100, 4, 2), (49, 130, 1)]
    raws, lds = [], []
    for i, (N, W, D) in enumerate(shapes):
        ld = W * D + 2 + 3 * i
        raw = rng.standard_normal((N, ld))
        raw[:, :W * D] = ref.ar1(rng, N, W, D, 0.6).reshape(N, W * D)
        raws.append(raw); lds.append(ld)
    ns, ws, ds = ([s[j] for s in shapes] for j in range(3))
    host = diagnostics._call(0, [r.ctypes.data for r in raws], False, lds, ns, ws, ds, 5.0)
    dev = torch.device("cuda", 0)
    tens = [torch.from_numpy(r).to(dev) for r in raws]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    assert stream.cuda_stream != 0
    got = diagnostics._call(0, [t.data_ptr() for t in tens], True, lds, ns, ws, ds, 5.0, stream=stream.cuda_stream)
    for a, b in zip(got, host):
        assert np.array_equal(a, b, equal_nan=False)
    o = 0
    for (N, W, D), raw in zip(shapes, raws):
        _same(tuple(a[o:o + D] for a in got), ref.diagnostics(raw[:, :W * D].reshape(N, W, D)))
        o += D
