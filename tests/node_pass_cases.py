"""Regions and walkers shared by tests/test_node_pass.py (CPU) and tests/test_gpu_node_pass.py: the line kinds of
tests/test_gpu_tile_batches.py on region sizes chosen for the line-major node stage -- with tile class p of a region
swept four tiles (p, p + 4, p + 8, p + 12) at a time:

    P4096   16 tiles: one full batch per class            P5120   20: a full batch plus one tile through the old stage
    P4352   17: 5 / 4 / 4 / 4                              P2304   9: no full batch, the old stage alone
    P4196   16 tiles and a tail of 100 px                 P4096-down, P4352-steps: a descending and a stepped grid
"""
import functools

import numpy as np

from oracle import vamp_oracle as vo

TILE, W, SD = 256, 64, 0.05
SHAPES = {"P4096": (4096, "up"), "P5120": (5120, "up"), "P4352": (4352, "up"), "P2304": (2304, "up"), "P4196": (4196, "up"),
          "P4096-down": (4096, "down"), "P4352-steps": (4352, "steps")}
KS = (1, 7, 16)


def grid(name):
    P, kind = SHAPES[name]
    if kind == "steps":         # tiles of unit and of double pixel spacing alternate
        x = np.cumsum(np.where((np.arange(P) // TILE) % 2 == 0, 1.0, 2.0))
        return x - 0.5 * (x[0] + x[-1])
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    return x[::-1].copy() if kind == "down" else x


def lines(name, K):
    """[K, 4] rows (A, c, L, G).  Kinds as in tests/test_gpu_tile_batches.py: damped, narrow, medium, broad ("mid"), wide.
    Narrow and medium lines sit inside single tiles of class 0's and class 1's first batch, so that each is near for one
    tile of a batch and far -- at depths that grow with the distance -- for the other three."""
    x = grid(name)
    P = x.size
    rng = np.random.default_rng(4000 * P + K)
    xa = np.sort(x)
    dxmax = np.max(np.diff(xa))
    centre = lambda i: 0.5 * (xa[TILE * i] + xa[TILE * i + TILE - 1])
    edge = lambda i: 0.5 * (xa[TILE * i - 1] + xa[TILE * i])
    ntile = P // TILE
    kinds = {
        "damped": lambda c: (10.0 ** rng.uniform(0.5, 2.477), c, rng.uniform(30, 300), rng.uniform(5, 30)),
        "narrow": lambda c: (rng.uniform(0.5, 5.0), c, 10.0 ** rng.uniform(-2, 0), rng.uniform(2, 18)),
        "medium": lambda c: (rng.uniform(0.5, 3.0), c, 10.0 ** rng.uniform(-1, 0.5), rng.uniform(40, 60) * dxmax),
        "broad": lambda c: (rng.uniform(0.3, 1.5), c, 10.0 ** rng.uniform(-1, 0.5), rng.uniform(175, 190) * dxmax),
        "wide": lambda c: (rng.uniform(10.0, 30.0), c, rng.uniform(5.0, 15.0), rng.uniform(310, 400) * dxmax),
    }
    if K == 1:
        plan = [("medium", centre(4))]
    elif K == 7:
        plan = [("damped", xa[-1] + 5.0 * dxmax), ("narrow", centre(0)), ("medium", centre(4) + 40.0), ("broad", centre(5) - 60.0),
                ("wide", rng.uniform(xa[0], xa[-1])), ("narrow", centre(8) + 90.0), ("damped", edge(ntile - 1))]
    else:
        plan = [("damped", xa[0] - 3.0 * dxmax), ("damped", xa[-1] + 5.0 * dxmax), ("damped", centre(5) + 30.0),
                ("narrow", centre(0)), ("narrow", edge(2)), ("narrow", centre(4) - 70.0), ("narrow", centre(min(12, ntile - 1))),
                ("medium", centre(4) + 55.0), ("medium", centre(1) - 20.0), ("medium", centre(8)),
                ("broad", centre(5) - 200.0 * dxmax), ("broad", centre(6)), ("broad", centre(1) + 10.0),
                ("wide", rng.uniform(xa[0], xa[-1])), ("wide", rng.uniform(xa[0], xa[-1])), ("narrow", edge(ntile - 1))]
    assert len(plan) == K
    t = np.array([kinds[kind](c) for kind, c in plan])
    return t[rng.permutation(K)]


@functools.lru_cache(maxsize=None)
def case(name, K):
    """Grid, data, the W walkers (walker w: the lines rotated by w places; walker 0 exact, the others moved by 1e-4) and
    the oracle's log-posterior: computed once, shared, read-only"""
    x = grid(name)
    t = lines(name, K)
    rng = np.random.default_rng(11)
    noise = np.full(x.size, SD)
    pad = 50.0 * np.max(np.abs(np.diff(x)))
    bounds = np.array([[x.min() - pad, x.max() + pad, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(x.size), noise=noise, **kw), t.reshape(-1)) + rng.normal(0, SD, x.size)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    th = np.empty((W, 4 * K))
    for w in range(W):
        tw = t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape))
        th[w] = np.roll(tw, w % K, axis=0).reshape(-1)
    want = vo.log_prob_batch_fast(reg, th)
    for a in (x, flux, noise, th, want, bounds):
        a.setflags(write=False)
    return dict(x=x, flux=flux, noise=noise, th=th, want=want, bounds=bounds, reg=reg, t=t, K=K)
