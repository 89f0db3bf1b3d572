"""GPU tests (-m gpu): every kernel shape of the log-posterior sweep at the region sizes the planner can hand it.

Which shape (struct Pack, csrc/vamp_hip.hip) a region runs in is decided from the CONTEXT's mean region length, the
region's line count, the packing request and the ensemble size; the region's own length only decides the blend class.
So the packed shapes (PackSmall2: 8 lanes per walker, PackSmall: 16 lanes) and the blend shape (PackMid) meet regions of
thousands of pixels: one long trough in an ordinary spectrum, or packings 16 / 65 on anything of <= 8 lines.  Every row
below says how its shape is reached, asserts through the test hook ``vampdbg_launch_plan`` that it was reached, and then
checks arithmetic:

  1. dispersed walkers (a fifth of them outside the prior or non-finite, at random positions) against the oracle, on
     data with at most four MARKED pixels (the first, pixel 512, the first of the shape's last partial tile, the last):
     a marked pixel has a tenth of the noise and its flux lowered by 0.5, so that it holds >= 1e-2 of chi^2 for most
     walkers and a dropped or doubly counted pixel breaks the fp32 bar too;
  2. the zero-residual check of tests/zero_residual.py, pixel by pixel;
  3. fp64: the same walkers under packing 64 (and 256 for regions of >= 2048 px) agree to the fp64 bar (the header's
     "all shapes agree to rounding" is a statement about fp64; fp32 shapes differ by W4's own error);
  4. vamp_lnprob(region) equals the region's slice of vamp_lnprob_all bit for bit, and the hook reports one shape for
     the sampler, vamp_lnprob_all and vamp_lnprob(region);
  5. four sampler steps against the oracle's stretch move, resident and not; two steps of W = 1024 (and of W = 512 in
     fp32) on the large rows, whose dispersed walkers -- a fifth outside the prior -- are also held against the oracle;
  6. the device MAP search equals the host-driven one bit for bit and its optimum's lnprob is the oracle's;
  7. negative controls: 2 sigma added at one pixel of the last partial tile and of a full tile beyond pixel 512.

Bars: fp64 |d lnprob| <= 1e-9 max(1, |lnprob|), chi^2 1e-11 relative, -inf exactly and in the same places
(test_gpu_parity.py); fp32 chi^2 <= 1e-3 relative against the fp64 device path under the same packing
(soak_short_regions.py).  The checks that need no shape (1, 2, 5) take a context factory and also run against the host
implementation of the ABI (tests/test_cpu_boundary.py), which proves without a GPU that the rows' inputs and bars are
satisfiable.  Run with -s: every row prints the shape the hook reported and its worst normalised error.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import zero_residual as zr

pytestmark = pytest.mark.gpu

# enum Shape of csrc/vamp_hip.hip (what vampdbg_launch_plan reports) and the launch classes of csrc/host_plan.hpp
SH_SMALL, SH_MID, SH_WIDE, SH_SMALL2 = 0, 1, 2, 6
SH_NAME = {0: "SH_SMALL", 1: "SH_MID", 2: "SH_WIDE", 3: "SH_WIDE_FULL", 4: "SH_SPLIT", 5: "SH_SPLIT_FULL", 6: "SH_SMALL2", 7: "SH_XL"}
CK_SMALL, CK_MID, CK_SMALL2 = 0, 1, 3
# pixels of one full tile of a shape: PK::LPW * pixels_per_lane<PK>() = lanes per walker (16, 8, 64: struct Pack) times
# VAMP_SMALL_TPIX = VAMP_TPIX = 4.  The lengths below are chosen around these; check_hook compares them with the
# lanes per walker the hook reports (threads per workgroup / walkers per workgroup).
TILE = {SH_SMALL: 64, SH_SMALL2: 32, SH_MID: 256}
PIXELS_PER_LANE = 4
GRIDS = ("ascending", "descending", "uneven")
W1 = 64                       # walkers per region of check 1
# oracle budget of the large rows, in pixels x lines of a region: the fp64 sampler replay at W = 1024 evaluates a region 2048
# times, the outside-prior check 512 / 1024 times.  One- and two-line subjects up to (2049, 2) are always taken; of the
# subjects of three to eight lines the replay takes the shortest of >= 513 px, (577, 3), the outside-prior check the longest
# within its budget, (2049, 3) and (1000, 5).  (4113, 2) and (4113, 8) are left to the fp32 legs (device oracle), to check 1 at
# W = 64 and to the zero-residual check.  CPU cost of the module: DESIGN.md section 6.
WORK2, REPLAY_WORK, PRIOR_WORK = 4200, 2000, 6200
BLEND_P = (96, 512)           # blends: 3 .. 8 lines over 96 .. 512 pixels (host_plan.hpp Limits)


@dataclasses.dataclass(frozen=True)
class Row:
    name: str
    packing: int
    subjects: tuple                 # ((P, K), ...): the regions the row is about
    fillers: tuple = (0, 0)         # automatic rows: short regions of 1 .. 2 lines and of 3 .. 8 lines around them
    mode: int = vo.MODE_VOIGT4
    sd: bool = False
    seed: int = 0


def _tiles(t, k=9):
    return (k * t - 1, k * t, k * t + 1)


# packing 16: PackSmall on one class; 9 tiles -1 / 0 / +1, the four ragged lengths, 1 / 2 / 3 / 8 lines
_P16 = _tiles(TILE[SH_SMALL]) + (513, 1000, 2049, 4113)
# packing 65: PackMid; the blend path ends at 512, the fall-back starts at 513 (its tail round never runs at a multiple
# of 256, so 9 tiles -1 / +1 and no multiple)
_P65 = (448, 449, 512, 513, 1000, 2049, 4113, 9 * TILE[SH_MID] - 1, 9 * TILE[SH_MID] + 1)
ROWS = {r.name: r for r in (
    Row("pack16", 16, tuple((P, (1, 2, 3, 8)[(i + j) % 4]) for i, P in enumerate(_P16) for j in (0, 2)), seed=1),
    Row("pack16-gauss3", 16, ((1000, 3),), mode=vo.MODE_GAUSS3, seed=2),
    Row("pack16-nbz3", 16, ((2049, 2),), mode=vo.MODE_NBZ3, seed=3),
    Row("pack16-sd", 16, ((513, 8),), sd=True, seed=4),
    Row("pack65", 65, tuple((P, (1, 3, 8)[(i + j) % 3]) for i, P in enumerate(_P65) for j in (0, 1)), seed=5),
    # automatic, spectrum-like: the mean region stays <= 128 px, so a few outliers need ~100 fillers of ~30 px.  Per class
    # 32 .. 63 regions: at W = 1024 (512 movers per region) a class then holds >= 16 384 movers and packs, at W = 512 it
    # holds < 16 384 and runs one walker per wavefront, at W <= 256 the ensemble is small and everything of <= 8 lines
    # that is not a blend is ONE class of PackSmall.
    Row("auto-a", 0, ((513, 1), (4113, 2)) + tuple(zip(_tiles(TILE[SH_SMALL2]), (1, 2, 1)))
        + ((513, 8), (2049, 3)) + tuple(zip(_tiles(TILE[SH_SMALL]), (5, 8, 3))) + ((512, 8), (95, 3), (96, 3)),
        fillers=(48, 52), seed=6),
    Row("auto-b", 0, ((1000, 1), (2049, 2), (1000, 5), (4113, 8)), fillers=(42, 42), seed=7),
)}
NBZ = np.array([0.7, 1215.67, 2.4e15, 4.0e10])


def is_blend(row, P, K):
    return row.packing == 0 and 3 <= K <= 8 and BLEND_P[0] <= P <= BLEND_P[1] and row.mode != vo.MODE_GAUSS3


def want_kind(row, P, K):
    """vamp_region_class: the partition of large ensembles"""
    if row.packing == 16:
        return CK_SMALL
    if row.packing == 65 or is_blend(row, P, K):
        return CK_MID
    return CK_SMALL2 if K <= 2 else CK_SMALL


def want_shape(row, P, K, W):
    """the shape the issue's table names for a region of this row in a W-walker ensemble (W / 2 movers per region)"""
    if row.packing == 16:
        return SH_SMALL
    if row.packing == 65 or is_blend(row, P, K):
        return SH_MID
    if W // 2 <= 128:
        return SH_SMALL                     # small ensembles: one merged class, sixteen lanes per walker
    n_class = sum(1 for p, k in row_shapes(row) if not is_blend(row, p, k) and (k <= 2) == (K <= 2))
    if n_class * (W // 2) >= 16384:
        return SH_SMALL2 if K <= 2 else SH_SMALL
    return SH_WIDE


def row_shapes(row):
    n2, n8 = row.fillers
    fill = [(20 + (7 * i) % 21, 1 + i % 2) for i in range(n2)] + [(20 + (11 * i) % 21, 3 + i % 6) for i in range(n8)]
    return list(row.subjects) + fill


def marks_for(P, tile):
    """at most four marked pixels: the first, pixel 512, the first of the last partial tile, the last"""
    m = {0, P - 1}
    if P > 512:
        m.add(512)
    if P % tile:
        m.add(P - P % tile)
    return sorted(m)


def dispersed(x, K, W, rng, n_bad, nan_at=2):
    """[W, 4 K] walkers spread over decades (test_random_long_regions_match_oracle's ranges), a line on either edge, a
    crowded blend where K >= 4, and n_bad walkers outside the prior or non-finite at random positions"""
    lo, hi = float(x.min()), float(x.max())
    span = hi - lo
    th = np.empty((W, K, 4))
    th[:, :, 0] = 10.0 ** rng.uniform(-2, 1.7, (W, K))
    th[:, :, 1] = rng.uniform(lo, hi, (W, K))
    th[:, :, 2] = 10.0 ** rng.uniform(-6, np.log10(0.4 * span), (W, K))
    th[:, :, 3] = 10.0 ** rng.uniform(-1.3, np.log10(0.4 * span), (W, K))
    th[0, 0, 1], th[1, 0, 1] = hi, lo
    if K >= 4:
        n = max(1, W // 8)
        c0 = rng.uniform(lo + 0.1 * span, hi - 0.1 * span, (n, 1))
        th[2:2 + n, :4, 1] = c0 + rng.uniform(-2.0, 2.0, (n, 4)) * span / (x.size - 1)
    th = th.reshape(W, 4 * K)
    bad = np.sort(rng.choice(W, n_bad, replace=False))
    for i, b in enumerate(bad):
        j = int(rng.integers(0, K))
        if i % 4 == 0:
            th[b, 4 * j] = -0.1
        elif i % 4 == 1:
            th[b, 4 * j + 1] = hi + 3.0
        elif i % 4 == 2:
            th[b, 4 * j + nan_at] = np.nan              # (modes without L: the amplitude)
        else:
            th[b, 4 * j + 3] = np.inf
    return np.ascontiguousarray(th), bad


def ball(x, K, W, rng):
    """[W, 4 K] in-prior start of the sampler and the MAP search: weak lines spread over the region, 2 % apart"""
    lo, hi = float(x.min()), float(x.max())
    span = hi - lo
    base = np.empty((K, 4))
    base[:, 0] = rng.uniform(0.05, 0.4, K)
    base[:, 1] = lo + (np.arange(K) + rng.uniform(0.3, 0.7, K)) / K * span
    base[:, 2] = rng.uniform(0.005, 0.03, K) * span
    base[:, 3] = rng.uniform(0.02, 0.1, K) * span
    th = base[None] * (1.0 + 0.02 * rng.standard_normal((W, K, 4)))
    th[:, :, 1] = base[None, :, 1] + 0.002 * span * rng.standard_normal((W, K))
    return np.ascontiguousarray(th.reshape(W, 4 * K))


def to_mode(th, row):
    """(A, c, L, G) walkers -> the row's parameters"""
    W = th.shape[0]
    t = th.reshape(W, -1, 4)
    if row.mode == vo.MODE_GAUSS3:
        out = np.stack([t[:, :, 0], t[:, :, 1], t[:, :, 3] / vo.FWHM_PER_SIGMA], axis=2).reshape(W, -1)
    elif row.mode == vo.MODE_NBZ3:
        with np.errstate(all="ignore"):
            out = np.array([zr.native_to_mode(tw, vo.MODE_NBZ3, NBZ) for tw in t])
    else:
        out = th
    if row.sd:
        out = np.hstack([out, np.linspace(0.05, 0.6, W)[:, None]])
    return np.ascontiguousarray(out)


def oracle_region(row, x, flux, noise, K):
    """the oracle's Region of an upload (x, flux, noise); a descending upload is built on the reversed arrays: Region
    derives its bounds from x[-1] - x[0]"""
    if x[0] > x[-1]:
        x, flux, noise = x[::-1].copy(), flux[::-1].copy(), noise[::-1].copy()
    kw = dict(l_fixed=NBZ[0], line=NBZ[1], x_origin=NBZ[2], x_scale=NBZ[3]) if row.mode == vo.MODE_NBZ3 else {}
    return vo.Region(x=x, flux=flux, noise=noise, n_comp=K, mode=row.mode, sample_sd=row.sd, **kw)


def chi_pixels(reg, th):
    """the oracle's ((f - m) / sigma)^2 per walker and pixel, with a free sd the unweighted (f - m)^2 the library returns as
    chi^2 (Voigt: log_prob_batch_fast's operations over all walkers; the other modes: vo.model_flux walker by walker)"""
    with np.errstate(all="ignore"):
        if reg.mode == vo.MODE_VOIGT4:
            t = th[:, :4 * reg.n_comp].reshape(th.shape[0], -1, 4)
            tau = np.zeros((th.shape[0], reg.x.size))
            for k in range(t.shape[1]):
                tau = tau + vo.voigt_function(reg.x[None, :], t[:, k, 1, None], t[:, k, 0, None], t[:, k, 2, None], t[:, k, 3, None])
            m = np.exp(-tau)
        else:
            m = np.array([vo.model_flux(reg, t) for t in th])
        return (reg.flux[None, :] - m) ** 2 if reg.sample_sd else ((reg.flux[None, :] - m) / reg.noise[None, :]) ** 2


class Inputs:
    """everything of a row that does not need a device, built once: the upload with its marked pixels, the dispersed
    walkers of check 1, the oracle's answers, and the conditions the issue puts on them (asserted here)"""

    def __init__(self, row):
        rng = np.random.default_rng(7100 + row.seed)
        self.row = row
        self.shapes = row_shapes(row)
        self.n_sub = len(row.subjects)
        self.xs, self.fs, self.ns, self.regs, self.th, self.want, self.chi, self.marks = [], [], [], [], [], [], [], []
        for r, (P, K) in enumerate(self.shapes):
            x = zr.grid(P, GRIDS[(r + row.seed) % 3], rng)
            noise = np.full(P, 0.05)
            flux = np.clip(1.0 + rng.normal(0, 0.05, P), 0, None)
            tile = TILE[want_shape(row, P, K, W1)]
            marks = marks_for(P, tile) if r < self.n_sub else []
            noise[marks] = 0.005
            flux[marks] = np.clip(flux[marks] - 0.5, 0, None)
            reg = oracle_region(row, x, flux, noise, K)
            th, bad = dispersed(x, K, W1, rng, W1 // 5, nan_at=2 if row.mode == vo.MODE_VOIGT4 else 0)
            thm = to_mode(th, row)
            want = vo.log_prob_batch_fast(reg, thm)
            fin = np.isfinite(want)
            # condition of check 1: under the oracle alone exactly the walkers put outside the prior are -inf
            assert np.array_equal(np.flatnonzero(~fin), bad) and np.all(want[~fin] == -np.inf), (row.name, P, K)
            chi = np.full(W1, np.nan)
            cp = chi_pixels(reg, thm[fin])
            chi[fin] = cp.sum(axis=1)
            if not row.sd:      # (a free sd replaces the noise: the marks weigh nothing there, the row keeps the other checks)
                for m in marks:
                    # condition of the marks: at least half of the finite walkers hold >= 1e-2 of chi^2 in the pixel
                    mo = m if x[0] < x[-1] else P - 1 - m
                    share = cp[:, mo] / chi[fin]
                    assert np.mean(share >= 1e-2) >= 0.5, (row.name, P, K, m, float(np.median(share)))
            self.xs.append(x); self.fs.append(flux); self.ns.append(noise); self.regs.append(reg)
            self.th.append(thm); self.want.append(want); self.chi.append(chi); self.marks.append(marks)
        self.Ks = [K for _, K in self.shapes]
        if row.packing == 0:
            assert np.mean([P for P, _ in self.shapes]) <= 128.0           # the context stays spectrum-like
        self.kinds = [want_kind(row, P, K) for P, K in self.shapes]
        self._cases = {}

    def upload(self, ctx):
        kw = dict(nbz=np.tile(NBZ, (len(self.xs), 1))) if self.row.mode == vo.MODE_NBZ3 else {}
        ctx.set_regions(self.xs, self.fs, self.ns, self.Ks, mode=self.row.mode, sample_sd=self.row.sd, **kw)
        assert ctx.region_classes()[0] == self.kinds, (self.row.name, ctx.region_classes()[0], self.kinds)

    def cases(self, dtype):
        """the zero-residual cases of the same regions (check 2)"""
        if dtype not in self._cases:
            rng = np.random.default_rng(7200 + self.row.seed)
            nbz = NBZ if self.row.mode == vo.MODE_NBZ3 else None
            self._cases[dtype] = [zr.short_case("%s r%d P=%d K=%d" % (self.row.name, r, P, K), self.xs[r], K, rng, dtype,
                                                mode=self.row.mode, sample_sd=self.row.sd, nbz=nbz)
                                  for r, (P, K) in enumerate(self.shapes)]
        return self._cases[dtype]

    def replayed(self):
        """regions whose sampler chains the oracle replays at W <= 64 (and the fp32 legs, whose oracle evaluates on the device,
        at any W): the subjects and the first filler of either kind"""
        n2 = self.row.fillers[0]
        return list(range(self.n_sub)) + [self.n_sub + i for i in (0, n2) if self.n_sub + i < len(self.xs)]

    def oracle_subjects(self, work8, longest):
        """the subjects the fp64 oracle takes at W = 512 / 1024, where it evaluates a region 512 .. 2048 times: every one-
        and two-line subject of <= WORK2 pixels x lines and ONE of three to eight lines of <= work8 (the longest, or the
        shortest of >= 513 px).  The others keep checks 2 and 4 and the -inf pattern there, and the fp32 legs."""
        sub = [r for r in range(self.n_sub) if self.Ks[r] <= 2 and self.shapes[r][0] * self.Ks[r] <= WORK2]
        more = [r for r in range(self.n_sub) if self.Ks[r] > 2 and self.shapes[r][0] >= 513 and self.shapes[r][0] * self.Ks[r] <= work8]
        more.sort(key=lambda r: self.shapes[r][0])
        return sub + (more[-1:] if longest else more[:1])


@functools.lru_cache(maxsize=None)
def inputs(name):
    return Inputs(ROWS[name])


def _dt(dtype):
    import vamp_amd
    return vamp_amd.F64 if dtype == "f64" else vamp_amd.F32


def _lists(res):
    return {k: (v if isinstance(v, list) else [v]) for k, v in res.items() if k != "seconds"}


# ---- checks that need no shape: they take a context factory mk(dtype, packing) -----------------------------------------
def check_dispersed(mk, name, dtype):
    """check 1; returns (lnprob [R, W], chi^2 [R, W]) of the row's context and the worst error in units of its bar"""
    inp = inputs(name)
    with mk(dtype, inp.row.packing) as ctx:
        inp.upload(ctx)
        got, chi = ctx.lnprob_all(inp.th, return_chi2=True)
    ref = None
    if dtype == "f32":
        with mk("f64", inp.row.packing) as ctx:
            inp.upload(ctx)
            ref = ctx.lnprob_all(inp.th, return_chi2=True)
    worst = 0.0
    for r in range(len(inp.xs)):
        want = inp.want[r]
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got[r])) and np.all(got[r][~fin] == -np.inf), (name, dtype, r, "pattern")
        if dtype == "f64":
            e = np.max(np.abs(got[r][fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))) / 1e-9
            e = max(e, np.max(np.abs(chi[r][fin] - inp.chi[r][fin]) / inp.chi[r][fin]) / 1e-11)
        else:
            assert np.array_equal(fin, np.isfinite(ref[0][r])), (name, r)
            e = np.max(np.abs(chi[r][fin] - ref[1][r][fin]) / np.maximum(ref[1][r][fin], 1e-300)) / 1e-3
        worst = max(worst, float(e))
        assert e <= 1.0, (name, dtype, r, inp.shapes[r], "error / bar = %.3g" % e)
    return got, chi, worst


def check_zero(mk, name, dtype, W, cases=None, ctx=None):
    """check 2: zr.check on a zero-residual family of the row's regions; returns the worst sqrt(chi^2)"""
    inp = inputs(name)
    cases = cases if cases is not None else inp.cases(dtype)
    rng = np.random.default_rng(7300 + W)
    th = [zr.walker_family(c, W, rng) for c in cases]
    own = ctx is None
    ctx = ctx if ctx is not None else mk(dtype, inp.row.packing)
    try:
        zr.set_cases(ctx, cases)
        report = zr.check(ctx, cases, th, "%s %s W=%d" % (name, dtype, W))
    finally:
        if own:
            ctx.close()
    return max(report.values())


def start_walkers(inp, W, seed):
    rng = np.random.default_rng(seed)
    return [to_mode(ball(x, K, W, rng), inp.row) for x, K in zip(inp.xs, inp.Ks)]


def check_sampler(mk, name, dtype, W=32, steps=4, block=8, resident=None):
    """check 5: `steps` stretch steps of every region from an in-prior start against the oracle's stretch move (fp32: the
    oracle's move evaluating through a second fp32 context, in the shape of the W / 2 movers of a half-step).  W <= 256:
    every walker and count exactly; larger: test_packed_launch_classes_at_production_size's allowance of <= 2 walkers per
    region whose accept margin is at rounding level.  Returns the run's results."""
    inp = inputs(name)
    th = start_walkers(inp, W, 7400 + W)
    with mk(dtype, inp.row.packing) as ctx:
        inp.upload(ctx)
        if resident is not None:
            ctx.set_option("resident", resident)
        lnp0 = ctx.lnprob_all(th)
        assert np.isfinite(lnp0).all(), name
        ctx.sampler_init(th, seed=606, split_block=block)
        ctx.kernel_timing(True)
        res = _lists(ctx.run(steps))
        res["launches"] = ctx.kernel_timing(False)[1]
    ev = None
    if dtype == "f32":
        ev = mk("f32", inp.row.packing)
        inp.upload(ev)
    try:
        n2 = inp.row.fillers[0]
        large = ev is None and W > 256
        for r in (inp.oracle_subjects(REPLAY_WORK, False) + [inp.n_sub, inp.n_sub + n2]) if large else inp.replayed():
            if ev is None:
                fn = lambda q, reg=inp.regs[r]: vo.log_prob_batch_fast(reg, q)
                start = fn(th[r])
                assert np.max(np.abs(start - lnp0[r]) / np.maximum(1.0, np.abs(start))) <= 1e-9, (name, r)
            else:
                fn = lambda q, r=r: ev.lnprob(np.concatenate([q, q]), region=r)[:len(q)]
                start = lnp0[r]
            chain, lchain, nacc = vo.run_sampler_batch(fn, th[r], start, steps, seed=606, block=block, region=r, walker_off=r * W)
            if W <= 256:
                assert np.allclose(res["chain"][r], chain, rtol=1e-10, atol=1e-12), (name, dtype, r, inp.shapes[r])
                assert np.array_equal(res["n_accept"][r], nacc), (name, dtype, r)
                assert np.allclose(res["lnprob"][r], lchain, rtol=1e-9, atol=1e-9), (name, dtype, r)
            else:
                ok = np.all(np.abs(res["chain"][r] - chain) <= 1e-10 * np.abs(chain) + 1e-12, axis=(0, 2))
                assert (~ok).sum() <= 2 and np.abs(res["n_accept"][r] - nacc).sum() <= 2, (name, dtype, r, int((~ok).sum()))
                assert np.allclose(res["lnprob"][r][:, ok], lchain[:, ok], rtol=1e-9, atol=1e-9), (name, dtype, r)
        assert sum(int(n.sum()) for n in res["n_accept"]) > 0, name
    finally:
        if ev is not None:
            ev.close()
    return res


def host_abi_row(mk, name, dtype):
    """checks 1, 2 and 5 of a row at W <= 64 with contexts from `mk`: what tests/test_cpu_boundary.py runs against the
    host implementation of the ABI"""
    _, _, w1 = check_dispersed(mk, name, dtype)
    w2 = check_zero(mk, name, dtype, 32)
    check_sampler(mk, name, dtype)
    return w1, w2


# ---- the hook ---------------------------------------------------------------------------------------------------------
def launch_plan(ctx, movers, entry, region=-1):
    """[(kind, shape, walkers per workgroup, threads, regions)] of the launches an entry point makes for `movers` movers
    per region (vampdbg_launch_plan; entry 0 sampler, 1 lnprob_all, 2 lnprob(region), 3 MAP search)"""
    fn = ctx._lib.vampdbg_launch_plan
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    rows = (C.c_longlong * 40)()
    n = fn(ctx._h, movers, entry, region, 8, rows)
    assert 1 <= n <= 8, (n, ctx._lib.vamp_last_error())
    return [tuple(rows[5 * i:5 * i + 5]) for i in range(n)]


def check_hook(ctx, inp, W, regions, label):
    """the hook reports the shape the row names for every listed region, the same through the sampler's, lnprob_all's and
    lnprob(region)'s entry (W points are W / 2 movers of a W-walker ensemble); returns {shape name: regions}"""
    seen = {}
    for r in regions:
        P, K = inp.shapes[r]
        per_entry = [launch_plan(ctx, W // 2, e, r) for e in (0, 1, 2)]
        assert all(len(p) == 1 for p in per_entry) and per_entry[0] == per_entry[1] == per_entry[2], (label, r, per_entry)
        kind, shape, wpb, threads, _ = per_entry[0][0]
        assert shape == want_shape(inp.row, P, K, W), (label, r, (P, K), SH_NAME[shape], SH_NAME[want_shape(inp.row, P, K, W)])
        if shape in TILE:
            assert threads // wpb * PIXELS_PER_LANE == TILE[shape], (label, SH_NAME[shape], threads, wpb)
        seen.setdefault(SH_NAME[shape], []).append((P, K))
    return seen


def check_entries(ctx, inp, th, regions, label):
    """check 4: lnprob(region) equals the region's slice of lnprob_all bit for bit (NaN chi^2 of walkers outside the prior
    included)"""
    la, ca = ctx.lnprob_all(th, return_chi2=True)
    for r in regions:
        l1, c1 = ctx.lnprob(th[r], region=r, return_chi2=True)
        assert np.array_equal(l1, la[r]) and np.array_equal(c1, ca[r], equal_nan=True), (
            label, r, inp.shapes[r], int((l1 != la[r]).sum()), "walkers differ between vamp_lnprob(region) and vamp_lnprob_all")
    return la, ca


def check_outside_prior(inp, th, la, ca, dtype, label):
    """Walkers outside the prior or non-finite at random positions, in the shape a large ensemble runs (the eight groups of
    a PackSmall2 wavefront leave before the sweep independently), against references that do not share that shape: every
    region's -inf pattern is the prior's; fp64: lnprob of Inputs.oracle_subjects against the oracle; fp32: chi^2 of every region against the fp64 device path, check 1's bar"""
    for r in range(len(inp.xs)):
        fin = np.isfinite(zr.log_prior_batch(inp.regs[r], th[r]))
        assert 0 < (~fin).sum() and np.array_equal(fin, np.isfinite(la[r])) and np.all(la[r][~fin] == -np.inf), (label, r, inp.shapes[r])
    worst = 0.0
    if dtype == "f64":
        for r in inp.oracle_subjects(PRIOR_WORK, True):
            want = vo.log_prob_batch_fast(inp.regs[r], th[r])
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(la[r])), (label, r)
            e = np.max(np.abs(la[r][fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))) / 1e-9
            worst = max(worst, float(e))
            assert e <= 1.0, (label, r, inp.shapes[r], "error / bar = %.3g" % e)
    else:
        with gpu("f64", inp.row.packing) as ref:
            inp.upload(ref)
            rl, rc = ref.lnprob_all(th, return_chi2=True)
        for r in range(len(inp.xs)):
            fin = np.isfinite(rl[r])
            assert np.array_equal(fin, np.isfinite(la[r])), (label, r)
            e = np.max(np.abs(ca[r][fin] - rc[r][fin]) / np.maximum(rc[r][fin], 1e-300)) / 1e-3
            worst = max(worst, float(e))
            assert e <= 1.0, (label, r, inp.shapes[r], "error / bar = %.3g" % e)
    return worst


def resident_plan(ctx):
    fn = ctx._lib.vampdbg_resident_plan
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    rows = (C.c_longlong * 32)()
    n = fn(ctx._h, 8, rows)
    assert 1 <= n <= 8
    return [tuple(rows[4 * i:4 * i + 4]) for i in range(n)]


def gpu(dtype, packing):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=_dt(dtype))
    ctx.set_packing(packing)
    return ctx


def wide_walkers(inp, W, seed):
    rng = np.random.default_rng(seed)
    return [to_mode(dispersed(x, K, W, rng, W // 5, nan_at=2 if inp.row.mode == vo.MODE_VOIGT4 else 0)[0], inp.row)
            for x, K in zip(inp.xs, inp.Ks)]


def check_resident(name, dtype, W=32, steps=4):
    """check 5, second half: resident = 2 equals resident = 0 bit for bit where the resident plan has a workgroup for every
    class (one timed launch per run instead of one per half-step)"""
    ref = check_sampler(gpu, name, dtype, W=W, steps=steps, resident=0)
    inp = inputs(name)
    th = start_walkers(inp, W, 7400 + W)
    with gpu(dtype, inp.row.packing) as ctx:
        inp.upload(ctx)
        ctx.set_option("resident", 2)
        ctx.sampler_init(th, seed=606, split_block=8)
        plan = resident_plan(ctx)
        ctx.kernel_timing(True)
        res = _lists(ctx.run(steps))
        launches = ctx.kernel_timing(False)[1]
    is_resident = all(nw >= 1 for _, nw, _, _ in plan)
    assert launches == (1 if is_resident else 2 * steps), (name, dtype, plan, launches)
    assert ref["launches"] == 2 * steps
    for key in ("chain", "lnprob", "n_accept"):
        for a, b in zip(res[key], ref[key]):
            assert np.array_equal(a, b), (name, dtype, key, "resident = 2 differs from resident = 0")
    return is_resident


def check_cross_shape(name, got, chi):
    """check 3 (fp64): the row's lnprob against packing 64, and against packing 256 on the regions of >= 2048 px"""
    inp = inputs(name)
    worst, worst_chi = 0.0, 0.0
    for packing in (64, 256):
        pick = [r for r, (P, _) in enumerate(inp.shapes) if packing == 64 or P >= 2048]
        if not pick:
            continue
        kw = dict(nbz=np.tile(NBZ, (len(pick), 1))) if inp.row.mode == vo.MODE_NBZ3 else {}
        with gpu("f64", packing) as ctx:
            ctx.set_regions([inp.xs[r] for r in pick], [inp.fs[r] for r in pick], [inp.ns[r] for r in pick], [inp.Ks[r] for r in pick],
                            mode=inp.row.mode, sample_sd=inp.row.sd, **kw)
            shapes = {s for _, s, _, _, _ in launch_plan(ctx, W1 // 2, 1)}
            assert not shapes & {SH_SMALL, SH_SMALL2, SH_MID}, (name, packing, shapes)      # another shape indeed
            o, oc = ctx.lnprob_all([inp.th[r] for r in pick], return_chi2=True)
        for i, r in enumerate(pick):
            fin = np.isfinite(inp.want[r])
            assert np.array_equal(fin, np.isfinite(o[i])), (name, packing, r)
            # the lnprob bar: packings 64 / 256 sum distant lines through the far-field interpolant, which reproduces a wing
            # to 3e-11 of its own value, so their chi^2 is not held to the 1e-11 of the per-pixel shapes
            e = np.max(np.abs(o[i][fin] - got[r][fin]) / np.maximum(1.0, np.abs(got[r][fin]))) / 1e-9
            worst = max(worst, float(e))
            worst_chi = max(worst_chi, float(np.max(np.abs(oc[i][fin] - chi[r][fin]) / chi[r][fin])))      # measured, printed
            assert e <= 1.0, (name, "packing %d against the row's shape" % packing, r, inp.shapes[r], "error / bar = %.3g" % e)
    return worst, worst_chi


def check_map(name, dtype, iterlim=40):
    """check 6: map_device 1 equals 0 bit for bit; lnprob_best is the oracle's at theta_best (fp64: 1e-9; fp32: the fp32
    bar on lnprob, 1e-3 relative, test_gpu_fp32.py)"""
    inp = inputs(name)
    starts = [t[0] for t in start_walkers(inp, 2, 7500)]
    out = {}
    with gpu(dtype, inp.row.packing) as ctx:
        inp.upload(ctx)
        plan = {s for _, s, _, _, _ in launch_plan(ctx, 1, 3)}
        assert plan <= {SH_SMALL, SH_MID}, plan            # the MAP search is a small ensemble: no PackSmall2, nothing wide
        for dev in (1, 0):
            ctx.set_option("map_device", dev)
            out[dev] = ctx.map_all(starts, iterlim=iterlim)
    for r in range(len(inp.xs)):
        assert np.array_equal(out[1][0][r], out[0][0][r]), (name, dtype, r, inp.shapes[r], "theta_best")
    assert np.array_equal(out[1][1], out[0][1]) and np.array_equal(out[1][3], out[0][3]), (name, dtype)
    assert out[1][3].max() > 0
    for r in inp.replayed():
        want = vo.log_prob_batch_fast(inp.regs[r], out[1][0][r][None, :])[0]
        tol = 1e-9 * max(1.0, abs(want)) if dtype == "f64" else 1e-3 * abs(want)
        assert abs(out[1][1][r] - want) <= tol, (name, dtype, r, out[1][1][r], want)


# ---- the rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", [n for n in ROWS if ROWS[n].packing])
def test_forced_packing_rows(name, dtype):
    """Packing 16 (PackSmall) and 65 (PackMid: blend path up to 512 px, fall-back beyond) on regions of 448 .. 4113 px."""
    inp = inputs(name)
    subjects = list(range(inp.n_sub))
    with gpu(dtype, inp.row.packing) as ctx:
        inp.upload(ctx)
        seen = check_hook(ctx, inp, W1, subjects, name)
        check_hook(ctx, inp, 32, subjects, name)
        check_entries(ctx, inp, inp.th, subjects, "%s %s W=%d" % (name, dtype, W1))
        check_entries(ctx, inp, [t[:32] for t in inp.th], subjects, "%s %s W=32" % (name, dtype))
    got, chi, w1 = check_dispersed(gpu, name, dtype)
    w2 = check_zero(gpu, name, dtype, 32)
    w3, w3c = check_cross_shape(name, got, chi) if dtype == "f64" else (float("nan"), float("nan"))
    res = check_resident(name, dtype)
    print("shape matrix %s %s: hook %s; dispersed error / bar %.3g, zero-residual sqrt(chi2) %.3g, cross-shape error / bar %.3g "
          "(chi2 relative difference %.3g), resident loop %s" % (name, dtype, seen, w1, w2, w3, w3c, res))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["auto-a", "auto-b"])
def test_automatic_rows_small_ensembles(name, dtype):
    """Automatic packing, spectrum-like context, W = 32 / 64: everything of <= 8 lines that is not a blend runs PackSmall,
    whatever its length; (512, 8) and (96, 3) are blends (PackMid), (513, 8) and (95, 3) are not."""
    inp = inputs(name)
    everything = list(range(len(inp.xs)))
    with gpu(dtype, 0) as ctx:
        inp.upload(ctx)
        seen = check_hook(ctx, inp, W1, everything, name)
        check_hook(ctx, inp, 32, everything, name)
        check_entries(ctx, inp, [t[:32] for t in inp.th], everything, "%s %s W=32" % (name, dtype))
    if name == "auto-a":
        assert set(seen["SH_MID"]) == {(512, 8), (96, 3)} and {(513, 8), (95, 3)} <= set(seen["SH_SMALL"]), seen
    got, chi, w1 = check_dispersed(gpu, name, dtype)
    w2 = check_zero(gpu, name, dtype, 32)
    w3, w3c = check_cross_shape(name, got, chi) if dtype == "f64" else (float("nan"), float("nan"))
    res = check_resident(name, dtype)
    check_map(name, dtype)
    print("shape matrix %s %s W<=64: hook %s; dispersed error / bar %.3g, zero-residual sqrt(chi2) %.3g, cross-shape error / bar "
          "%.3g (chi2 relative difference %.3g), resident loop %s" % (name, dtype, {k: len(v) for k, v in seen.items()}, w1, w2, w3, w3c, res))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("W", [512, 1024])
@pytest.mark.parametrize("name", ["auto-a", "auto-b"])
def test_automatic_rows_large_ensembles(name, W, dtype):
    """The same contexts at W = 1024 (every short class holds >= 16 384 movers: PackSmall2 for one and two lines, PackSmall
    for three to eight, draws from k_draws) and at W = 512 in between (one walker per wavefront: SH_WIDE)."""
    inp = inputs(name)
    everything = list(range(len(inp.xs)))
    with gpu(dtype, 0) as ctx:
        inp.upload(ctx)
        seen = check_hook(ctx, inp, W, everything, name)
        want = {"SH_SMALL2", "SH_SMALL"} if W == 1024 else {"SH_WIDE"}
        assert {k for k in seen if k != "SH_MID"} == want, seen
        label = "%s %s W=%d" % (name, dtype, W)
        th = wide_walkers(inp, W, 7600 + W)
        la, ca = check_entries(ctx, inp, th, everything, label)
        w2 = check_zero(gpu, name, dtype, W, ctx=ctx)
    w1 = check_outside_prior(inp, th, la, ca, dtype, label)
    # two sampler steps.  In between (W = 512) the fp32 leg: its oracle evaluates through vamp_lnprob(region), which ran another
    # shape than the sampler there until it counted the movers of the region's class
    if W == 1024 or dtype == "f32":
        check_sampler(gpu, name, dtype, W=W, steps=2, block=W)
    print("shape matrix %s: hook %s; dispersed error / bar %.3g, zero-residual sqrt(chi2) %.3g" % (label, {k: len(v) for k, v in seen.items()}, w1, w2))


def test_one_line_regions_pack_eight_walkers_only_in_full_launches():
    """include/vamp_hip.h, vamp_ctx_set_packing: a one-line region runs four walkers per wavefront in a small ensemble
    (W = 128: 64 movers per region), one in between, and eight only in a launch of >= 16 384 movers."""
    inp = inputs("auto-a")
    with gpu("f64", 0) as ctx:
        inp.upload(ctx)
        r = inp.shapes.index((513, 1))
        assert [launch_plan(ctx, 64, e, r)[0][1] for e in (0, 1, 2)] == [SH_SMALL] * 3
        assert [launch_plan(ctx, 256, e, r)[0][1] for e in (0, 1, 2)] == [SH_WIDE] * 3            # in between: a wavefront each
        assert [launch_plan(ctx, 512, e, r)[0][1] for e in (0, 1, 2)] == [SH_SMALL2] * 3
        assert launch_plan(ctx, 512, 3, r)[0][1] == SH_SMALL


# ---- 7. negative controls ---------------------------------------------------------------------------------------------
NEGATIVE = {"PackSmall": ("pack16", (2049, 8), 32), "PackMid fall-back": ("pack65", (2049, 8), 32), "PackSmall2": ("auto-b", (2049, 2), 1024)}


@pytest.mark.parametrize("where", ["last partial tile", "full tile beyond 512"])
@pytest.mark.parametrize("shape", list(NEGATIVE))
def test_negative_control_one_pixel(shape, where):
    """2 sigma_j added to the data of a 2049-pixel region at pixel j = 2048 (the one pixel of the last partial tile of every
    shape) or j = 1300 (a full tile beyond pixel 512): check 2 fails for every walker, at the tile of j."""
    name, (P, K), W = NEGATIVE[shape]
    inp = inputs(name)
    r = inp.shapes.index((P, K))
    j = P - 1 if where == "last partial tile" else 1300
    assert (P - 1) % TILE[SH_SMALL] == 0 and (P - 1) % TILE[SH_MID] == 0 and j > 512
    cases = list(inp.cases("f64"))
    cases[r] = zr.make_case(cases[r].name, inp.xs[r], cases[r].truth, K, splits=cases[r].splits,
                            data_shift=lambda s: np.where(np.arange(s.size) == j, 2.0 * s, 0.0))
    with gpu("f64", inp.row.packing) as ctx:
        zr.set_cases(ctx, cases)
        got = launch_plan(ctx, W // 2, 1, r)[0][1]
        assert got == want_shape(inp.row, P, K, W), SH_NAME[got]
        # (every walker beyond the allowance is the verdict of the shape asserted above; the tile is then found by zr.localise
        # through nine copies of the region, a context of its own that need not run that shape: it localises the data)
        with pytest.raises(AssertionError) as err:
            check_zero(gpu, name, "f64", W, cases=cases, ctx=ctx)
    tile = j // zr.TILE
    msg = str(err.value)
    assert "%d walkers beyond the allowance" % W in msg and msg.count("beyond the allowance") == 1, msg
    assert "tile %d, pixels [%d, %d)" % (tile, tile * zr.TILE, min(P, (tile + 1) * zr.TILE)) in msg, msg
