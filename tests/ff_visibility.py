"""Would the suite notice a wrong far-field list entry?  (helper, not collected by pytest)

The far-field sweep keeps, per tile of 256 pixels, a far list (deep lines first) and a wide list (lines wider than a
tile, and "mid" lines between far and near).  A fault of the classification -- an entry dropped, counted twice, or
written to the row of another tile of its batch -- changes the model over ONE tile by ONE line's optical depth there.
``visibility`` measures every such (line k, full tile j, class) entry against a check:

  ("sigma", sigma)         the zero-residual allowance (tests/zero_residual.py): max over the tile's pixels of
                           f*_i |1 - e^{-d tau_i}| / sigma_i, d tau the mutation's change of the optical depth.  chi^2 of
                           the check is at least the square of this, and the check demands chi^2 <= 1.
  ("lnprob", region, bar)  an lnprob bar against the oracle: |delta lnprob| / bar with the region's own data and noise.

Mutations: "drop" (-tau_k on tile j), "twice" (+tau_k on tile j: for the allowance this is the f* (1 - e^{-tau_k}) / sigma
of the probe cases' condition, the smaller of the two), "wrong_tile" (-tau_k on tile j, +tau_k at the pixels of the next
tile of j's batch -- the previous one for the batch's last tile; NaN where a batch holds one tile).

The predicates are those of the kernel (ff_classify_batch) in their numpy restatement, test_gpu_tile_batches.classes;
``entries`` names its masks and knows that fp32 contexts have a far list only (far = outside the Gaussian core).

The probe cases (``probe_case``) are zero-residual regions in which EVERY entry is visible: see PROBE CONDITION below.
"""
import dataclasses
import functools

import numpy as np

from oracle import vamp_oracle as vo
import test_gpu_tile_batches as tb
import zero_residual as zr

TILE = tb.TILE
FF_BATCH = 4                      # tiles classified per pass (vamp_hip.hip)
CLASSES = ("far-deep", "far-shallow", "mid", "wide")
MARGIN = 3.0                      # PROBE CONDITION: every claimed entry has visibility >= MARGIN under the allowance:
                                  # a kernel that loses it returns chi^2 >= 9 where the check demands <= 1.  The factor
                                  # covers a fault that loses part of an entry and the step from tau_k to 1 - e^{-tau_k}.


def entries(x, t, f32=False):
    """{class: bool [K, tiles]} of the list entries a context of this dtype keeps.  fp32: the far list only."""
    far, deep, midc, wide = tb.classes(x, t, f32)
    out = {"far-deep": deep, "far-shallow": far & ~deep}
    if not f32:
        out["mid"] = midc
        out["wide"] = wide & ~midc          # (a mid line is on the wide list too: counted once, as mid)
    return out


def waves_of(packing):
    return 4 if packing == 256 else 1      # workgroup per walker: tile j belongs to wavefront j mod 4


def batch_neighbour(j, ntile, packing):
    """the tile whose list row lies next to tile j's in the batch of j's wavefront, or -1"""
    nw = waves_of(packing)
    place = j // nw                         # j is the wavefront's place-th tile
    first = place - place % FF_BATCH
    for p in (place + 1, place - 1):
        n = p * nw + j % nw
        if first <= p < first + FF_BATCH and 0 <= n < ntile:
            return n
    return -1


def line_taus(x, t):
    r = vo.Region(x=x, flux=np.ones(x.size), noise=np.ones(x.size), n_comp=t.shape[0], mode=vo.MODE_VOIGT4,
                  c_lo=-np.inf, c_hi=np.inf, sigma_max=np.inf, fwhm_max=np.inf)
    return vo.component_taus(r, np.asarray(t, dtype=np.float64).reshape(-1))


def visibility(x, t, f32, check, mutation="twice", packing=256):
    """{class: float [K, tiles]}: the visibility of every entry (NaN where the pair is no entry of that class)."""
    taus = line_taus(x, t)
    fstar = np.exp(-taus.sum(0))
    ntile = x.size // TILE
    sl = lambda j: slice(TILE * j, TILE * (j + 1))

    def measure(changes):                   # changes: [(tile, d tau over that tile)]
        if check[0] == "sigma":
            return max(np.max(fstar[sl(j)] * np.abs(-np.expm1(-d)) / check[1][sl(j)]) for j, d in changes)
        _, reg, bar = check
        dl = 0.0
        for j, d in changes:
            f, n = reg.flux[sl(j)], reg.noise[sl(j)]
            dl += -0.5 * np.sum(((f - fstar[sl(j)] * np.exp(-d)) ** 2 - (f - fstar[sl(j)]) ** 2) / n ** 2)
        return abs(dl) / bar

    out = {}
    for name, mask in entries(x, t, f32).items():
        v = np.full(mask.shape, np.nan)
        for k, j in zip(*np.nonzero(mask)):
            tk = taus[k, sl(j)]
            if mutation == "drop":
                v[k, j] = measure([(j, -tk)])
            elif mutation == "twice":
                v[k, j] = measure([(j, tk)])
            else:
                n = batch_neighbour(j, ntile, packing)
                if n >= 0:
                    v[k, j] = measure([(j, -tk), (n, taus[k, sl(n)])])
        out[name] = v
    return out


def invisible_share(vis):
    """(entries, share of them with visibility < 1) over all classes"""
    v = np.concatenate([a[~np.isnan(a)] for a in vis.values()])
    return v.size, float(np.mean(v < 1.0)) if v.size else 0.0


def lnprob_shares(name, K):
    """the existing mixed cases of test_gpu_tile_batches: walker 0, one entry dropped, against the tests' two bars"""
    c = tb.case(name, K)
    lnp = abs(float(c["want"][0]))
    n, s64 = invisible_share(visibility(c["x"], c["t"], False, ("lnprob", c["reg"], 1e-9 * max(1.0, lnp)), "drop"))
    _, s32 = invisible_share(visibility(c["x"], c["t"], False, ("lnprob", c["reg"], 1e-3 * lnp), "drop"))
    return n, s64, s32


# ---- probe cases -----------------------------------------------------------------------------------------------------
PROBE_SHAPES = ("P2048", "P2304", "P5120", "P2404", "P2304-down", "P4352-steps")      # of tb.SHAPES: one batching edge each
PROBE_PAIRS = (("P2048", "P2304"), ("P5120", "P2404"), ("P2304-down", "P4352-steps"))  # the two long regions of a context
LEAD_PX = 300                     # a short region ahead of them: pix_off 300 and 300 + P, no multiple of 256


def probe_lines(name):
    """[K, 4] rows (A, c, L, G) of comparable strength.  fp64 (K = 15): eleven damped lines (A ~ 20, L ~ 5 px, G ~ 30 px)
    clustered in the second tile -- far from every tile two and more away, deep for the nearest of them, more than 8 of
    them so that the second slot pair of ff_coefficients runs, none far from the first three tiles -- two broad lines whose
    |z| < 8 zone reaches tiles outside their Gaussian core (mid), two lines wider than a tile (wide)."""
    x = tb.grid(name)
    xa = np.sort(x)
    dx = np.max(np.diff(xa))
    rng = np.random.default_rng(x.size + len(name))
    hub = 0.5 * (xa[TILE] + xa[2 * TILE - 1])
    rows = [(rng.uniform(15, 25), hub + off * dx + rng.uniform(-0.5, 0.5), rng.uniform(4, 6) * dx, rng.uniform(25, 35) * dx)
            for off in np.linspace(-100, 100, 11)]
    for frac, g in ((0.35, 180.0), (0.8, 186.0)):
        L, G = 5.0 * dx, g * dx
        rows.append((float(zr.amp_for_peak([L], [G], 0.6)[0]), xa[0] + frac * (xa[-1] - xa[0]) + 0.3, L, G))
    for frac, g in ((0.55, 330.0), (0.15, 360.0)):
        L, G = 8.0 * dx, g * dx
        rows.append((float(zr.amp_for_peak([L], [G], 0.4)[0]), xa[0] + frac * (xa[-1] - xa[0]) + 0.7, L, G))
    return np.array(rows)


# fp32: a far list only, evaluated by ff32_coefficients in two slot groups: list entries 0..7 (one per group of 8 lanes)
# and, when the list is longer than 8, entries 8..15.  Under the fp32 allowance an entry is visible only if its line
# carries about 1 % of the largest optical depth within a tile's reach (eps_rel 2e-4 x sqrt(256) x MARGIN), so the fp32
# probes are far-only clusters of EQUAL lines at one place, damped strongly enough (A ~ 60, L ~ 16 px) that the wing is
# above the absolute floor 16 x 3e-7 x MARGIN at the far end of every shape.  Two list lengths, the smallest that reach
# each slot group: "short" 3 lines (4 entries with the split: first group only) and "long" 8 lines (9 entries: the
# ninth is the only one of the second group).  The split line has twice the amplitude, so that each of its parts is an
# entry like the others.
F32_VARIANTS = {"short": 3, "long": 8}


def probe_lines32(name, K):
    x = tb.grid(name)
    xa = np.sort(x)
    dx = np.max(np.diff(xa))
    rng = np.random.default_rng(32 + x.size + len(name) + K)
    hub = 0.5 * (xa[2 * TILE] + xa[3 * TILE - 1])          # middle of the third tile: of unit spacing on the steps grid
    return np.array([(rng.uniform(55, 65), hub + off * dx + rng.uniform(-0.5, 0.5), rng.uniform(15, 17) * dx, rng.uniform(28, 32) * dx)
                     for off in np.linspace(-6, 6, K)])


@dataclasses.dataclass
class Probe:
    name: str
    dtype: str
    t: np.ndarray              # [K, 4] the lines as the kernel sees them (line 0 split, its other part last)
    cases: tuple               # the zr.Case regions to upload: fp64 the region itself, fp32 one copy per tile, localised
    sigma: np.ndarray          # the allowance every pixel is checked against (fp32: each tile's from its own copy)
    drop: tuple = None         # (k, j) of a negative control

    @property
    def x(self):
        return self.cases[0].region.x

    @property
    def ntile(self):
        return self.x.size // TILE


@functools.lru_cache(maxsize=None)
def probe_case(name, dtype="f64", variant=None, drop=None):
    """The zero-residual probe region of a shape (fp32: ``variant`` of F32_VARIANTS).  ``drop`` = (k, j): the data are
    those a kernel fits exactly that loses line k over tile j (the negative controls); the allowance is that of the
    unchanged case."""
    f32 = dtype == "f32"
    x = tb.grid(name)
    t = probe_lines32(name, F32_VARIANTS[variant]) if f32 else probe_lines(name)
    if f32:
        t[0, 0] *= 2.0                      # both parts of the split line are as strong as the other lines
    comps, pair = zr.with_split(t, 0, 0.5 if f32 else 0.37)
    pad = 50.0 * np.max(np.abs(np.diff(x)))
    shift = None
    if drop is not None:
        k, j = drop
        taus = line_taus(x, comps)
        d = np.zeros(x.size)
        d[TILE * j:TILE * (j + 1)] = np.exp(-taus.sum(0))[TILE * j:TILE * (j + 1)] * np.expm1(taus[k, TILE * j:TILE * (j + 1)])
        shift = lambda sigma: d
    label = "probe %s %s%s%s" % (name, dtype, " " + variant if variant else "", " without line %d in tile %d" % drop if drop else "")
    make = lambda **kw: zr.make_case(label, x, comps.ravel(), comps.shape[0], dtype=dtype, pad=pad, splits=(pair,),
                                     data_shift=shift, **kw)
    if not f32:
        case = make()
        return Probe(name, dtype, comps, (case,), case.sigma, drop)
    copies = tuple(make(probe_tile=j) for j in range((x.size + TILE - 1) // TILE))
    sigma = np.concatenate([c.sigma[TILE * j:TILE * (j + 1)] for j, c in enumerate(copies)])
    return Probe(name, dtype, comps, copies, sigma, drop)


def tile_copies(p):
    """one copy of the region per tile (the ragged last one included), the allowance inside it, HUGE_NOISE outside: what
    zr.localise uploads.  fp32 probes are such copies already."""
    if p.dtype == "f32":
        return list(p.cases)
    case = p.cases[0]
    out = []
    for j in range((p.x.size + TILE - 1) // TILE):
        n = np.full(p.x.size, zr.HUGE_NOISE)
        n[TILE * j:TILE * (j + 1)] = case.sigma[TILE * j:TILE * (j + 1)]
        out.append(dataclasses.replace(case, region=dataclasses.replace(case.region, noise=n)))
    return out


@functools.lru_cache(maxsize=None)
def lead_case(dtype):
    rng = np.random.default_rng(LEAD_PX)
    return zr.short_case("lead P=%d" % LEAD_PX, zr.grid(LEAD_PX, "ascending", rng), 3, rng, dtype)


def probe_visibility(p, mutation="twice", packing=256):
    """visibility of every entry of a probe case under its own allowance"""
    return visibility(p.x, p.t, p.dtype == "f32", ("sigma", p.sigma), mutation, packing)


def far_counts(p):
    e = entries(p.x, p.t, p.dtype == "f32")
    return (e["far-deep"] | e["far-shallow"]).sum(0)


def list_slot(p, k, j):
    """place of line k in tile j's far list when the walker holds the lines in the truth's order: deep lines first"""
    e = entries(p.x, p.t, p.dtype == "f32")
    deep, far = e["far-deep"][:, j], (e["far-deep"] | e["far-shallow"])[:, j]
    assert far[k]
    return int(deep[:k].sum()) if deep[k] else int(deep.sum() + (far & ~deep)[:k].sum())
