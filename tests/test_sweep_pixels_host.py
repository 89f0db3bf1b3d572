"""CPU tests of the zero-residual harness (tests/zero_residual.py) through the host build of the C ABI
(oracle/libvamp_cpu.so: every pixel evaluated directly, no far field, no Taylor tables).  The host library must sit
inside the fp64 allowance on every case family the GPU module runs, which proves the harness and the allowances
without a GPU; the negative control shows the gap the new check closes: a one-pixel error of 2 sigma_i fails it, and
the same error moves a noisy region's lnprob by less than the existing 1e-9 max(1, |lnprob|) bar."""
import numpy as np
import pytest

from oracle import vamp_oracle as vo
import zero_residual as zr
from test_cpu_boundary import cpu_lib  # noqa: F401  (fixture)
from test_gpu_parity import FAR_FIELD_CASES


@pytest.fixture
def host_ctx(cpu_lib):  # noqa: F811
    import vamp_amd
    ctx = vamp_amd.HipContext(lib=cpu_lib)
    yield ctx
    ctx.close()


def _run(ctx, cases, W, seed, label):
    rng = np.random.default_rng(seed)
    zr.set_cases(ctx, cases)
    th = [zr.walker_family(c, W, rng) for c in cases]
    report = zr.check(ctx, cases, th, label)
    zr.print_report(label, report)
    return report


def test_log_prior_batch_is_the_oracle_prior():
    rng = np.random.default_rng(0)
    for mode, sd in ((vo.MODE_VOIGT4, False), (vo.MODE_GAUSS3, True), (vo.MODE_NBZ3, False)):
        x = zr.grid(300, "ascending", rng)
        nbz = np.array([0.7, 1215.67, 2.4e15, 4.0e10]) if mode == vo.MODE_NBZ3 else None
        case = zr.short_case("prior", x, 4, rng, "f64", mode=mode, sample_sd=sd, nbz=nbz)
        th = zr.walker_family(case, 64, rng)
        th[::7, 0] *= -1.0                                     # some walkers outside the prior
        th[::5, 1] += 1e3 * (x[-1] - x[0]) if mode != vo.MODE_NBZ3 else 1.0
        want = np.array([vo.log_prior(case.region, t) for t in th])
        assert np.array_equal(zr.log_prior_batch(case.region, th), want)


def test_walker_families_share_the_exact_model():
    rng = np.random.default_rng(1)
    case = zr.line_class_cases(500, "uneven", "f64", 5, families=["saturated"])[0]
    th = zr.walker_family(case, 16, rng)
    assert len({t.tobytes() for t in th}) == 16
    for t in th:
        assert np.allclose(vo.model_flux(case.region, t), case.region.flux, rtol=1e-14, atol=1e-16)
    x, truth, nbz = zr.headline_truth(P=2048, K=6)
    wl = __import__("bench").make_workload(P=2048, K=6, W=64, nbz=True)
    assert np.array_equal(wl["x"], x) and np.array_equal(wl["nbz"][0], nbz)
    d = (wl["theta0"] - truth[None, :]).reshape(64, 6, 3)
    rel = np.abs(d[:, :, :2] / truth.reshape(6, 3)[None, :, :2])    # the bench's walkers: truth x (1 + 1e-3 N(0, 1))
    assert rel.max() < 0.01 and np.median(rel) < 2e-3 and np.abs(d[:, :, 2]).max() < 1e-4


@pytest.mark.parametrize("kind", ["ascending", "descending", "uneven"])
def test_host_line_classes_within_the_fp64_allowance(host_ctx, kind):
    cases = []
    for i, P in enumerate((1000, 3000)):
        cases += zr.line_class_cases(P, kind, "f64", 100 + i, far_field_cases=FAR_FIELD_CASES)
    _run(host_ctx, cases, 8, 3, "host " + kind)


def test_host_headline_within_the_fp64_allowance(host_ctx):
    case = zr.headline_case("f64")
    _run(host_ctx, [case], 4, 4, "host headline")


@pytest.mark.parametrize("mode,sd", [(vo.MODE_GAUSS3, False), (vo.MODE_VOIGT4, False), (vo.MODE_NBZ3, False),
                                     (vo.MODE_VOIGT4, True), (vo.MODE_GAUSS3, True)])
def test_host_modes_and_short_regions(host_ctx, mode, sd):
    rng = np.random.default_rng(20 + mode + 3 * sd)
    nbz = np.array([0.7, 1215.67, 2.4e15, 4.0e10]) if mode == vo.MODE_NBZ3 else None
    cases = [zr.short_case("P=%d" % P, zr.grid(P, "ascending", rng), 1 + P % 4, rng, "f64", mode=mode, sample_sd=sd, nbz=nbz)
             for P in list(range(2, 40)) + [96, 300, 1200]]
    _run(host_ctx, cases, 8, 5, "host mode %d sd %d" % (mode, sd))


def test_one_pixel_error_is_caught_here_and_missed_by_the_lnprob_bar(host_ctx):
    """Both sides of the gap: f* + 2 sigma_j at one far-field pixel j (what a kernel erring by 2 sigma_j there returns)."""
    base = zr.line_class_cases(4096, "ascending", "f64", 7, far_field_cases=FAR_FIELD_CASES, families=["ff headline-like"])[0]
    j = zr.far_pixel(base)
    bump = lambda s: np.where(np.arange(s.size) == j, 2.0 * s, 0.0)
    bad = zr.line_class_cases(4096, "ascending", "f64", 7, far_field_cases=FAR_FIELD_CASES, families=["ff headline-like"])[0]
    bad = zr.make_case(bad.name, bad.region.x, bad.truth, bad.region.n_comp, splits=bad.splits, data_shift=bump)
    assert np.array_equal(bad.sigma, base.sigma)
    rng = np.random.default_rng(8)
    th = zr.walker_family(base, 8, rng)
    zr.set_cases(host_ctx, [base])
    zr.check(host_ctx, [base], [th], "control")
    zr.set_cases(host_ctx, [bad])
    with pytest.raises(AssertionError) as err:
        zr.check(host_ctx, [bad], [th], "control")
    tile = j // zr.TILE
    assert "tile %d, pixels [%d, %d)" % (tile, tile * zr.TILE, (tile + 1) * zr.TILE) in str(err.value), str(err.value)
    # the same error on noisy data (S/N 100) moves lnprob by far less than the 1e-9 max(1, |lnprob|) bar
    noisy = base.region.flux + rng.normal(0.0, 0.01, base.region.x.size)
    noise = np.full(noisy.size, 0.01)
    lnp = []
    for f in (noisy, noisy + bump(base.sigma)):
        host_ctx.set_regions(base.region.x, f, noise, base.region.n_comp, bounds=base.bounds[None, :])
        lnp.append(host_ctx.lnprob(th))
    assert np.all(np.isfinite(lnp[0]))
    assert np.all(np.abs(lnp[1] - lnp[0]) <= 1e-9 * np.maximum(1.0, np.abs(lnp[0])))
