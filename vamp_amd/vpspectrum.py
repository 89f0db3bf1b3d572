"""``VPspectrum`` -- spectrum-level orchestration (reference vamp_1.0/vpspectrum.py:21-539): read a
spectrum, find detection regions, fit every region through ``VPregion`` (and so through the HIP
hot path), harvest physical parameters, write the result files.

Host-side numpy, as in the reference (it runs once per spectrum).  Intended behaviour of the main
path is reproduced; the reference's defects on rarely taken branches are not:
undefined names in ``split_difficult_region`` (vpspectrum.py:190,198,225) and in the forced
component increase (:309,316), and the missing h5py dependency is replaced by ``h5min`` (the
subset of HDF5 these files need, in the layout h5py's defaults write; h5py is used when importable).
"""
import os

import numpy as np

from .physics import (ColumnDensity, DopplerParameter, EquivalentWidthFlux, EquivalentWidthTau, ErrorB, ErrorN,
                      Freq2wave, Tau2flux, Wave2freq)
from .vpfits import VPfit
from .vpregion import VPregion

def read_spectrum_file(path):
    """wavelength, flux, noise of a spectrum file: HDF5 (h5py when available, else the minimal
    reader of vamp_amd/h5min.py), ``.npz``, or a 4-column text file (wavelength, velocity, flux,
    noise) such as vamp_1.0/data/q1422.cont."""
    if path.endswith((".cont", ".txt", ".dat")):
        a = np.loadtxt(path)
        return a[:, 0].copy(), a[:, 2].copy(), a[:, 3].copy()
    if path.endswith(".npz"):
        d = np.load(path, allow_pickle=False)
        return d["wavelength"], d["flux"], d["noise"]
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:
        with h5py.File(path, "r") as data:
            return np.array(data["wavelength"][:]), np.array(data["flux"][:]), np.array(data["noise"][:])
    from . import h5min
    data = h5min.read(path)
    return data["wavelength"], data["flux"], data["noise"]


def _same_convolve(a, kernel):
    """np.convolve(a, kernel, 'same') for len(a) == len(kernel), skipping the kernel's exact zeros
    (a Gaussian of sigma <= 10 px underflows to 0.0 beyond ~390 px; the reference convolves the
    full-length kernel, O(N^2), which is minutes for the 49 106-pixel q1422 spectrum)."""
    n = a.size
    nz = np.nonzero(kernel)[0]
    lo, hi = nz[0], nz[-1]
    full = np.convolve(a, kernel[lo:hi + 1], "full")          # full[k'] = full_conv[k' + lo]
    out = np.zeros(n)
    first = (n - 1) // 2 - lo                                  # 'same' keeps full_conv[(n-1)//2 : (n-1)//2 + n]
    src_lo, src_hi = max(first, 0), min(first + n, full.size)
    out[src_lo - first:src_hi - first] = full[src_lo:src_hi]
    return out


def detection_regions(wavelength, flux, noise, min_region_width=2, N_sigma=4.0, extend=False, std_min=2, std_max=11,
                      buffer=3):
    """Detection regions of vpspectrum.py:67-175 (vectorised restatement).

    Equivalent width of the flux decrement per pixel, matched-filtered with Gaussians of
    sigma = std_min .. std_max-1 px; a region is a run of pixels whose best detection ratio
    exceeds N_sigma with flux < 1, longer than min_region_width, kept if some pixel is an
    N_sigma decrement on its own, and padded by ``buffer`` pixels.  Returns (pixels, waves)."""
    wl = np.asarray(wavelength, dtype=np.float64)
    fl = np.asarray(flux, dtype=np.float64)
    no = np.asarray(noise, dtype=np.float64)
    n = wl.size
    dw = np.zeros(n)
    dw[1:-1] = 0.5 * np.abs(wl[:-2] - wl[2:])
    dec = 1.0 - fl
    dec = np.where(dec < no, 0.0, dec)
    flux_ew = dw * dec
    noise_ew = dw * no
    flux_ew[[0, -1]] = 0.0
    noise_ew[[0, -1]] = 0.0
    xarr = np.arange(n) - (n - 1) / 2.0
    det = np.full(n, -np.inf)
    inner = slice(1, n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        for std in range(std_min, std_max):
            g = VPfit.GaussFunction(xarr, 1.0, 0.0, std)
            ff = _same_convolve(flux_ew, g)
            nf = _same_convolve(np.square(noise_ew), np.square(g))
            ratio = ff[inner] * (1.0 / np.sqrt(nf[inner]))
            better = ratio > det[inner]                       # NaN never replaces (as the reference's `>`)
            det[inner] = np.where(better, ratio, det[inner])
    # run detection; pixel 0 can never start a region (the reference uses start == 0 as "none")
    runs, start = [], 0
    above = (det > N_sigma) & (fl < 1.0)
    below = (det < N_sigma) | (fl > 1.0)
    for i in range(n):
        if start == 0 and above[i]:
            start = i
        elif start != 0 and below[i]:
            if (i - start) > min_region_width:
                runs.append([start, i])
            start = 0
    if extend:
        grown = []
        for s, e in runs:
            i = s
            while i > 0 and fl[i] < 1.0:
                i -= 1
            j = e
            while j < n - 1 and fl[j] < 1.0:
                j += 1
            grown.append([i, j])
        runs = grown
    pixels, waves = [], []
    for k, (s, e) in enumerate(runs):
        if k < len(runs) - 1 and e > runs[k + 1][0]:
            e = runs[k + 1][1]
        strong = np.nonzero((1.0 - fl[s:e]) > np.abs(no[s:e]) * N_sigma)[0]
        if strong.size:
            if s >= buffer:
                s -= buffer
            if e < n - buffer:
                e += buffer
            pixels.append([s, e])
            waves.append([wl[s], wl[e]])
    return pixels, waves


BATCH_MAX_LINES = 8          # lines per region in a ragged batch (vamp_amd/batched.py: the packed launch shapes)

class VPspectrum():

    def __init__(self, line, spectrum_file=None, out_folder=None, voigt=False, chi_limit=1.5, mcmc_cov=False,
                 get_mcmc_err=True, convergence_attempts=10, chi_sq_maximum=10., max_single_region_components=15,
                 ideal_single_region_components=5, min_region_percentage=2., nwalkers=None, iterations=3000, thin=15,
                 burn=300, seed=None, verbose=True, dtype=None, device=0):
        """Arguments as vpspectrum.py:23-52; nwalkers / iterations / thin / burn / seed / verbose / dtype / device
        are new and forwarded to the region fits (dtype: "f64" -- the reference's arithmetic -- or "f32" = the
        Humlicek-W4 path of BASELINE.json config 5; None: $VAMP_DTYPE, else fp64)."""
        from . import hip_backend as _hb
        self.dtype = _hb.resolve_dtype(dtype)
        self.device = device
        self.line = line
        self.spectrum_file = spectrum_file
        self.out_folder = out_folder
        self.voigt = voigt
        self.chi_limit = chi_limit
        self.mcmc_cov = mcmc_cov
        self.get_mcmc_err = get_mcmc_err
        self.convergence_attempts = convergence_attempts
        self.chi_sq_maximum = chi_sq_maximum
        self.max_single_region_components = max_single_region_components
        self.ideal_single_region_components = ideal_single_region_components
        self.min_region_percentage = min_region_percentage
        self.nwalkers, self.iterations, self.thin, self.burn = nwalkers, iterations, thin, burn
        self.seed, self.verbose = seed, verbose
        if spectrum_file is not None:
            self.read_from_spectrum_file()

    def set_arrays(self, wavelength, flux, noise):
        self.wavelength_array = np.asarray(wavelength, dtype=np.float64)
        self.flux_array = np.asarray(flux, dtype=np.float64)
        self.noise_array = np.asarray(noise, dtype=np.float64)
        self.frequency_array = Wave2freq(self.wavelength_array)

    def read_from_spectrum_file(self):
        """vpspectrum.py:58-64"""
        self.set_arrays(*read_spectrum_file(self.spectrum_file))

    def compute_detection_regions(self, min_region_width=2, N_sigma=4.0, extend=False, std_min=2, std_max=11):
        """vpspectrum.py:67-175; sets ``region_pixels`` and ``region_waves``."""
        if self.verbose:
            print('Computing detection regions...')
        self.num_pixels = len(self.wavelength_array)
        self.region_pixels, self.region_waves = detection_regions(
            self.wavelength_array, self.flux_array, self.noise_array, min_region_width, N_sigma, extend, std_min, std_max)
        if self.verbose:
            print('Found {} detection regions.'.format(len(self.region_pixels)))

    def _region(self, start, end, voigt=None):
        """slice + flip so that frequency ascends (vpspectrum.py:274-279)"""
        f = np.flip(self.flux_array[start:end], 0)
        n = np.flip(self.noise_array[start:end], 0)
        nu = np.flip(self.frequency_array[start:end], 0)
        return VPregion(nu, f, n, voigt=self.voigt if voigt is None else voigt, chi_limit=self.chi_limit,
                        nwalkers=self.nwalkers, seed=None if self.seed is None else self.seed + 7 * start,
                        dtype=self.dtype, device=self.device)

    def split_difficult_region(self):
        """If the whole spectrum is ONE region that wants more than ``max_single_region_components``
        lines, cut it at flux maxima into about n/ideal pieces, each at least ``min_region_percentage``
        per cent of the pixels (intent of vpspectrum.py:178-241)."""
        self.difficult_fit = False
        if len(self.region_pixels) != 1:
            return
        start, end = self.region_pixels[0]
        region = self._region(start, end, voigt=False)
        if region.n <= self.max_single_region_components:
            return
        self.difficult_fit = True
        want = max(2, region.n // self.ideal_single_region_components)
        flux = self.flux_array[start:end]
        n_cand = min(flux.size, 10 * want)
        cand = np.argpartition(flux, -n_cand)[-n_cand:]
        cand = cand[np.argsort(flux[cand])][::-1] + start          # highest flux first, absolute pixels
        min_size = (end - start) * (self.min_region_percentage / 100.0)
        cuts = [start, end]
        for c in cand:
            if len(cuts) == want + 1:
                break
            if all(abs(int(c) - p) >= min_size for p in cuts):
                cuts.append(int(c))
        cuts.sort()
        self.region_pixels = [[a, b] for a, b in zip(cuts[:-1], cuts[1:])]
        self.region_waves = [[self.wavelength_array[a], self.wavelength_array[b]] for a, b in self.region_pixels]
        if self.verbose:
            print("Split one {}-component region into {} regions.".format(region.n, len(self.region_pixels)))

    def fit_spectrum(self, batched=False):
        """Detect regions, fit each (retrying up to ``convergence_attempts`` times, keeping the best
        reduced chi^2), harvest N, b, EW, centres and their errors (vpspectrum.py:243-442).
        Returns the ``params`` dict.  ``batched=True`` runs the BIC ladders of all regions together
        (one kernel launch per half-step for the whole spectrum, vamp_amd/batched.py) with the same
        retry / keep-best loop over the regions still above the chi^2 limit; regions that want more
        lines than the packed launch shapes hold (8) form a second ragged batch of up to
        VAMP_MAX_COMPONENTS = 32 lines each."""
        self.compute_detection_regions(min_region_width=2)
        self.split_difficult_region()
        if batched:
            return self._fit_spectrum_batched()
        empty = lambda: np.array([])
        self.params = {k: empty() for k in ('b', 'b_std', 'N', 'N_std', 'EW', 'centers', 'region_numbers')}
        nreg = len(self.region_pixels)
        self.flux_model = {'total': np.ones(len(self.flux_array)), 'chi_squared': np.zeros(nreg),
                           'region_pixels': self.region_pixels, 'amplitude': empty(), 'sigmas': empty(),
                           'centers': empty(), 'region_numbers': empty(), 'EW': np.zeros(nreg), 'std_a': empty(),
                           'std_s': empty(), 'std_c': empty(), 'cov_as': empty(), 'difficult_fit': self.difficult_fit}
        self.regions = []
        for j, (start, end) in enumerate(self.region_pixels):
            waves = np.flip(self.wavelength_array[start:end], 0)
            region = self._region(start, end)
            best_chi, best_fit = self._fit_region_attempts(region)
            region.fit = best_fit
            region.best_chi_squared = best_chi
            region.n = len(region.fit.estimated_profiles)
            self._harvest(j, start, end, waves, region)
            self.regions.append(region)
        if self.out_folder is not None:
            name = os.path.basename(self.spectrum_file or "spectrum")
            name = name[:name.find('.')] if '.' in name else name
            self.output_filename = os.path.join(self.out_folder, name) + ('_voigt_' if self.voigt else '_gauss_')
            self.plot_spectrum()
            self.write_file()
        return self.params

    def _fit_region_attempts(self, region):
        """The reference's per-region retry loop (vpspectrum.py:281-348): up to ``convergence_attempts``
        fits, keeping the best reduced chi^2; a region that wants more than
        ``max_single_region_components`` lines is flagged ``difficult_fit``, gets 2 attempts (1 beyond
        1.5 x that number) and three times the chi^2 limit.  Returns (best reduced chi^2, its fit)."""
        fluxes, noise = region.flux_array, region.noise_array
        attempts = self.convergence_attempts
        if region.n > self.max_single_region_components:           # vpspectrum.py:287-294
            attempts = 1 if region.n > 1.5 * self.max_single_region_components else 2
            self.flux_model['difficult_fit'] = True
        best_chi, best_fit = -1.0, None
        tried_n, tried_chi = [], []
        for _ in range(attempts):
            region.estimate_n()
            # after three poor fits with the same n, force one more component (intent of :306-321)
            while tried_n.count(region.n) > 2 and \
                    min(c for n_, c in zip(tried_n, tried_chi) if n_ == region.n) > self.chi_sq_maximum:
                region.n += 1
            limit = region.chi_limit * 3 if region.n > self.max_single_region_components else region.chi_limit
            region.region_fit(verbose=self.verbose, iterations=self.iterations, thin=self.thin, burn=self.burn)
            region.set_freedom()
            chi = region.fit.ReducedChisquared(fluxes, region.fit.total.value, noise, region.freedom)
            tried_n.append(region.n)
            tried_chi.append(chi)
            if self.verbose:
                print('Reduced chi squared is {:.2f}'.format(chi))
            if best_fit is None or chi < best_chi:
                if best_fit is not None:
                    region._release(best_fit)            # (the device context of a fit that is dropped)
                best_chi, best_fit = chi, region.fit
            else:
                region._release(region.fit)
            if best_chi < limit:
                break
        return best_chi, best_fit

    def _fit_spectrum_batched(self):
        from .batched import BatchedRegionLadder
        empty = lambda: np.array([])
        self.params = {k: empty() for k in ('b', 'b_std', 'N', 'N_std', 'EW', 'centers', 'region_numbers')}
        nreg = len(self.region_pixels)
        self.flux_model = {'total': np.ones(len(self.flux_array)), 'chi_squared': np.zeros(nreg),
                           'region_pixels': self.region_pixels, 'amplitude': empty(), 'sigmas': empty(),
                           'centers': empty(), 'region_numbers': empty(), 'EW': np.zeros(nreg), 'std_a': empty(),
                           'std_s': empty(), 'std_c': empty(), 'cov_as': empty(), 'difficult_fit': self.difficult_fit}
        self.regions = [self._region(s, e) for s, e in self.region_pixels]
        # the reference's retry loop (vpspectrum.py:281-348) for all regions at once: every attempt re-estimates n
        # and runs the ladder of the regions whose best reduced chi^2 is still above their limit, with fresh
        # draws; a region keeps the best fit it has seen.  Two batches, by the launch shapes they run on: regions
        # that want <= BATCH_MAX_LINES lines (the packed shapes of real spectra) and the few that want more (a
        # second ragged batch, a wavefront per walker, up to VAMP_MAX_COMPONENTS = 32 lines) -- those are NOT clamped to 8 and retried against an
        # unscaled limit: as in the reference a region beyond max_single_region_components is flagged
        # difficult_fit, gets 2 attempts (1 beyond 1.5 x) and three times the chi^2 limit (:287-294, 325-327)
        from .batched import MAX_COMPONENTS
        best = {}
        small, big = [], []
        for i, r in enumerate(self.regions):
            r.estimate_n()
            (big if r.n > BATCH_MAX_LINES else small).append(i)
        ctx = None
        for group, cap in ((small, BATCH_MAX_LINES), (big, MAX_COMPONENTS)):
            left = {}
            for i in group:
                n0 = self.regions[i].n
                left[i] = max(1, int(self.convergence_attempts))
                if n0 > self.max_single_region_components:
                    left[i] = 1 if n0 > 1.5 * self.max_single_region_components else 2
                    self.flux_model['difficult_fit'] = True
                    if self.verbose:
                        print("region {}: {} lines estimated: difficult fit ({} attempt(s), 3 x the chi^2 limit)".format(i, n0, left[i]))
            pending, attempt = list(group), 0
            while pending:
                regs = [self.regions[i] for i in pending]
                limits = {}
                for i, r in zip(pending, regs):
                    r.estimate_n()
                    # the limit follows the n ESTIMATED for this attempt, before the ladder grows it (vpspectrum.py:325-327,
                    # as _fit_region_attempts does)
                    limits[i] = r.chi_limit * 3 if r.n > self.max_single_region_components else r.chi_limit
                    r.n = min(r.n, cap)
                ladder = BatchedRegionLadder(regs, nwalkers=self.nwalkers or 64, iterations=self.iterations, thin=self.thin,
                                             burn=self.burn, seed=(self.seed or 0) + 7727 * attempt + (0 if cap == BATCH_MAX_LINES else 15485863),
                                             verbose=self.verbose, ctx=ctx, dtype=self.dtype, device=self.device)
                ctx = ladder.ctx
                ladder.run()
                still = []
                for i, region in zip(pending, regs):
                    region.set_freedom()
                    chi = region.fit.ReducedChisquared(region.flux_array, region.fit.total.value, region.noise_array, region.freedom)
                    if i not in best or chi < best[i][0]:
                        best[i] = (chi, region.fit)
                    left[i] -= 1
                    if not (best[i][0] < limits[i]) and left[i] > 0:
                        still.append(i)
                attempt += 1
                if self.verbose:
                    print("attempt {} (<= {} lines): {} of {} regions go again".format(attempt, cap, len(still), len(group)))
                pending = still
        if ctx is not None:
            ctx.close()
        for j, ((start, end), region) in enumerate(zip(self.region_pixels, self.regions)):
            region.best_chi_squared, region.fit = best[j]
            region.n = len(region.fit.estimated_profiles)
            region.set_freedom()
            self._harvest(j, start, end, np.flip(self.wavelength_array[start:end], 0), region)
        if self.out_folder is not None:
            name = os.path.basename(self.spectrum_file or "spectrum")
            name = name[:name.find('.')] if '.' in name else name
            self.output_filename = os.path.join(self.out_folder, name) + ('_voigt_' if self.voigt else '_gauss_')
            self.plot_spectrum()
            self.write_file()
        return self.params

    def _harvest(self, j, start, end, waves, region):
        """fit -> flux model and physical parameters of region j (vpspectrum.py:351-426)"""
        fit, n = region.fit, region.n
        fm, pr = self.flux_model, self.params
        fm['chi_squared'][j] = region.best_chi_squared
        fm['total'][start:end] = np.flip(fit.total.value, 0)
        fm['region_%d_wave' % j] = np.flip(waves, 0)
        comp = np.ones((n, end - start))
        for k in range(n):
            comp[k] = np.flip(Tau2flux(fit.estimated_profiles[k].value), 0)
        fm['region_%d_flux' % j] = comp
        fm['EW'][j] = EquivalentWidthFlux(edges=fm['region_%d_wave' % j], fluxes=comp)
        ev = fit.estimated_variables
        heights = np.array([ev[i]['amplitude'].value for i in range(n)])
        centers = np.array([Freq2wave(ev[i]['centroid'].value) for i in range(n)])
        if region.voigt:
            sigmas = VPfit.GaussianWidth(np.array([ev[i]['G_fwhm'].value for i in range(n)]))
        else:
            sigmas = np.array([ev[i]['sigma'].value for i in range(n)])
        numbers = np.arange(n)
        for key, val in (('amplitude', heights), ('centers', centers), ('region_numbers', numbers), ('sigmas', sigmas)):
            fm[key] = np.append(fm[key], val)
        if self.mcmc_cov:
            cov = fit.chain_covariance(n, voigt=region.voigt)
            std_a, std_s, std_c = (np.sqrt(cov[:, i, i]) for i in range(3))
            cov_as = cov[:, 0, 1]
            for key, val in (('std_a', std_a), ('std_s', std_s), ('std_c', std_c), ('cov_as', cov_as)):
                fm[key] = np.append(fm[key], val)
            pr['N_std'] = np.append(pr['N_std'], ErrorN(heights, sigmas, std_a, std_s, cov_as))
        elif self.get_mcmc_err:
            stats = fit.mcmc.stats()
            std_s = np.array([stats['est_sigma_%d' % i]['standard deviation'] for i in range(n)])
            std_a = np.array([stats['xexp_%d' % i]['standard deviation'] for i in range(n)])
            fm['std_s'] = np.append(fm['std_s'], std_s)
            fm['std_a'] = np.append(fm['std_a'], std_a)
            pr['b_std'] = np.append(pr['b_std'], ErrorB(std_s, self.line))
            pr['N_std'] = np.append(pr['N_std'], ErrorN(amplitude=heights, sigma=sigmas, std_a=std_a, std_s=std_s,
                                                        cov_as=np.zeros(n)))
        pr['b'] = np.append(pr['b'], DopplerParameter(sigmas, self.line))
        pr['N'] = np.append(pr['N'], ColumnDensity(heights, sigmas))
        pr['centers'] = np.append(pr['centers'], centers)
        pr['region_numbers'] = np.append(pr['region_numbers'], numbers)
        for k in range(n):
            pr['EW'] = np.append(pr['EW'], EquivalentWidthTau(fit.estimated_profiles[k].value, [waves[0], waves[-1]]))

    def posterior_summaries(self, probs=None, scratch_bytes=0):
        """After ``fit_spectrum``: the posterior band of the fitted flux and the equivalent widths with credible intervals,
        from ONE GPU call over the kept fits (vamp_amd.posterior).  A dict in wavelength order (flipped like ``_harvest``):
        ``probs`` [Q]; ``total_mean`` / ``total_sd`` [n_pixels] and ``total_q`` [Q, n_pixels] (1 / 0 / 1 outside regions);
        ``EW_mean`` / ``EW_sd`` [n_regions] and ``EW_q`` [n_regions, Q]; ``line_EW_mean`` / ``line_EW_sd`` [n_lines] and
        ``line_EW_q`` [n_lines, Q] in the order of ``params['EW']``.  Every width is the region's pixel width
        |lambda_last - lambda_first| / (P - 1) (``EquivalentWidthFlux``'s rule), for lines too."""
        from . import posterior
        probs = np.atleast_1d(np.asarray(posterior.DEFAULT_PROBS if probs is None else probs, dtype=np.float64))
        Q, npx, regs = probs.size, len(self.flux_array), self.regions
        widths = []
        for start, end in self.region_pixels:
            lam = self.wavelength_array[start:end]
            widths.append(float(np.abs(lam[-1] - lam[0]) / max(1, len(lam) - 1)))
        have, recs = posterior.fits_posterior([r.fit for r in regs], probs=probs, pixel_width=widths, device=getattr(self, "device", 0),
                                              scratch_bytes=scratch_bytes)
        if len(have) != len(regs):
            raise RuntimeError("posterior_summaries: %d of %d regions have no chain" % (len(regs) - len(have), len(regs)))
        out = {"probs": probs, "total_mean": np.ones(npx), "total_sd": np.zeros(npx), "total_q": np.ones((Q, npx)),
               "EW_mean": np.array([r.ew_mean for r in recs]), "EW_sd": np.array([r.ew_sd for r in recs]),
               "EW_q": np.array([r.ew_q for r in recs]).reshape(len(recs), Q),
               "line_EW_mean": np.concatenate([r.comp_ew_mean for r in recs] or [np.zeros(0)]),
               "line_EW_sd": np.concatenate([r.comp_ew_sd for r in recs] or [np.zeros(0)]),
               "line_EW_q": np.concatenate([r.comp_ew_q for r in recs] or [np.zeros((0, Q))], axis=0),
               "time_step": np.array([r.step for r in recs], dtype=np.int32)}
        for (start, end), r in zip(self.region_pixels, recs):
            out["total_mean"][start:end] = np.flip(r.flux_mean, 0)
            out["total_sd"][start:end] = np.flip(r.flux_sd, 0)
            out["total_q"][:, start:end] = np.flip(r.flux_q, 1)
        return out

    def write_posterior(self, post):
        """``posterior_summaries()``' dict as ``<prefix>posterior.h5``, through h5py when it is importable, else through
        vamp_amd/h5min.py, as ``write_file`` does; returns the path"""
        path = self.output_filename + 'posterior.h5'
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(path, 'a') as f:
                for p in post.keys():
                    f.create_dataset(p, data=np.array(post[p]))
        else:
            from . import h5min
            h5min.write(path, {k: np.array(v) for k, v in post.items()})
        return path

    def evidences(self, **kw):
        """After ``fit_spectrum``: ln Z of every kept fit's model from ONE GPU call (vamp_amd.evidence; keywords as
        ``evidence.log_evidence``).  A dict in region order: ``lnZ`` / ``lnZ_se`` / ``lnZ_ti`` / ``n_comp`` [n_regions],
        ``betas`` [T], ``mean_lnL`` / ``var_lnL`` / ``move_accept`` [n_regions, T], ``swap_accept`` [n_regions, T - 1].  A fit of more
        lines than the library takes (8) is left out of the call and has NaN rows."""
        from . import evidence
        fits = [r.fit for r in self.regions]
        ok = [f._n <= evidence.MAX_COMPONENTS for f in fits]
        got = iter(evidence.fits_evidence([f for f, o in zip(fits, ok) if o], device=getattr(self, "device", 0), **kw))
        recs = [next(got) if o else None for o in ok]
        T = next((len(r.betas) for r in recs if r is not None), 0)
        nan = lambda w: np.full(w, np.nan)
        col = lambda k, w: np.array([nan(w) if r is None else np.atleast_1d(getattr(r, k)) for r in recs], dtype=np.float64).reshape(len(recs), w)
        return {"lnZ": col("lnZ", 1)[:, 0], "lnZ_se": col("lnZ_se", 1)[:, 0], "lnZ_ti": col("lnZ_ti", 1)[:, 0],
                "n_comp": np.array([f._n for f in fits], dtype=np.int32),
                "betas": next((np.array(r.betas) for r in recs if r is not None), np.zeros(0)), "mean_lnL": col("mean_lnL", T),
                "var_lnL": col("var_lnL", T), "move_accept": col("move_accept", T), "swap_accept": col("swap_accept", max(0, T - 1))}

    def write_evidence(self, ev):
        """``evidences()``' dict as ``<prefix>evidence.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'evidence.h5'
        h5min.write(path, {k: np.array(v) for k, v in ev.items()})
        return path

    def predictive(self, scratch_bytes=0):
        """After ``fit_spectrum`` (batched or not): the pointwise log predictive density and WAIC of every kept fit from
        ONE GPU call over their chains (vamp_amd.predictive).  A dict: ``lppd`` / ``ll_mean`` / ``p_waic_pix`` / ``elpd``
        [n_pixels] in wavelength order (flipped like ``_harvest``; NaN outside regions), and per region ``elpd_waic`` /
        ``elpd_se`` / ``p_waic`` / ``waic`` / ``lnl_mean`` / ``n_high`` / ``n_used`` / ``n_bad`` / ``n_comp`` /
        ``time_step`` [n_regions]."""
        from . import predictive
        npx, regs = len(self.flux_array), self.regions
        have, recs = predictive.fits_predictive([r.fit for r in regs], device=getattr(self, "device", 0), scratch_bytes=scratch_bytes)
        if len(have) != len(regs):
            raise RuntimeError("predictive: %d of %d regions have no chain" % (len(regs) - len(have), len(regs)))
        out = {k: np.full(npx, np.nan) for k in ("lppd", "ll_mean", "p_waic_pix", "elpd")}
        for k in ("elpd_waic", "elpd_se", "p_waic", "waic", "lnl_mean"):
            out[k] = np.array([getattr(r, k) for r in recs], dtype=np.float64)
        for k in ("n_high", "n_used", "n_bad"):
            out[k] = np.array([getattr(r, k) for r in recs], dtype=np.int32)
        out["n_comp"] = np.array([r.fit._n for r in regs], dtype=np.int32)
        out["time_step"] = np.array([r.step for r in recs], dtype=np.int32)
        for (start, end), r in zip(self.region_pixels, recs):
            for k in ("lppd", "ll_mean", "p_waic_pix", "elpd"):
                out[k][start:end] = np.flip(getattr(r, k), 0)
        return out

    def write_predictive(self, pred):
        """``predictive()``'s dict as ``<prefix>predictive.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'predictive.h5'
        h5min.write(path, {k: np.array(v) for k, v in pred.items()})
        return path

    def loo(self, scratch_bytes=0):
        """After ``fit_spectrum`` (batched or not): PSIS-LOO of every kept fit from ONE GPU call over their chains
        (vamp_amd.loo).  A dict: ``elpd_loo_pix`` / ``p_loo_pix`` / ``khat`` / ``lppd`` [n_pixels] in wavelength order
        (flipped like ``_harvest``; NaN outside regions), and per region ``elpd_loo`` / ``elpd_loo_se`` / ``p_loo`` /
        ``looic`` / ``n_high_k`` / ``n_used`` / ``n_bad`` / ``n_comp`` / ``time_step`` [n_regions]."""
        from . import loo
        npx, regs = len(self.flux_array), self.regions
        have, recs = loo.fits_loo([r.fit for r in regs], device=getattr(self, "device", 0), scratch_bytes=scratch_bytes)
        if len(have) != len(regs):
            raise RuntimeError("loo: %d of %d regions have no chain" % (len(regs) - len(have), len(regs)))
        pix = ("elpd_loo_pix", "p_loo_pix", "khat", "lppd")
        out = {k: np.full(npx, np.nan) for k in pix}
        for k in ("elpd_loo", "elpd_loo_se", "p_loo", "looic"):
            out[k] = np.array([getattr(r, k) for r in recs], dtype=np.float64)
        for k in ("n_high_k", "n_used", "n_bad"):
            out[k] = np.array([getattr(r, k) for r in recs], dtype=np.int32)
        out["n_comp"] = np.array([r.fit._n for r in regs], dtype=np.int32)
        out["time_step"] = np.array([r.step for r in recs], dtype=np.int32)
        for (start, end), r in zip(self.region_pixels, recs):
            for k in pix:
                out[k][start:end] = np.flip(getattr(r, k), 0)
        return out

    def write_loo(self, rec):
        """``loo()``'s dict as ``<prefix>loo.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'loo.h5'
        h5min.write(path, {k: np.array(v) for k, v in rec.items()})
        return path

    def relabel(self, max_iter=None):
        """After ``fit_spectrum`` (batched or not): the relabelling that undoes label switching, of every kept fit from
        ONE GPU call over their chains (vamp_amd.relabel; each fit's ``mcmc.relabel()`` cache is filled), and the
        largest R-hat of every region before and after it from two diagnostics calls.  A dict, per region [n_regions]:
        ``n_iter`` / ``n_changed`` / ``n_switched`` / ``n_used`` / ``n_bad`` / ``n_comp`` (int32), ``converged`` (int8),
        ``max_r_hat_before`` / ``max_r_hat_after``, ``min_n_eff_before`` / ``min_n_eff_after`` (NaN for a chain too long for
        the diagnostics) and ``tau_reliable_before`` / ``tau_reliable_after`` (int8; is every parameter's tau reliable?); per
        line, region after region, ``label_mean`` / ``label_sd`` [n_lines, q] in the caller's units with ``line_region`` [n_lines]."""
        from . import diagnostics, relabel
        max_iter = relabel.DEFAULT_MAX_ITER if max_iter is None else int(max_iter)
        regs = self.regions
        fits = [r.fit for r in regs]
        device = getattr(self, "device", 0)
        have, recs = relabel.fits_relabel(fits, max_iter=max_iter, device=device)
        if len(have) != len(regs):
            raise RuntimeError("relabel: %d of %d regions have no chain" % (len(regs) - len(have), len(regs)))
        diagnostics.fits_diagnostics(fits, device=device)
        ok = [i for i, f in enumerate(fits) if f._chain_dev.shape[0] <= diagnostics.MAX_SAMPLES]
        after = diagnostics.chain_diagnostics([recs[i].gather(fits[i]._chain_dev) for i in ok], thin=[fits[i].mcmc._thin for i in ok],
                                              device=device) if ok else []
        if max_iter == relabel.DEFAULT_MAX_ITER:       # the relabelling a fit's diagnostics(relabel=True) reads
            for i, d in zip(ok, after):
                fits[i].mcmc._set_diagnostics(d, relabel=True)
        worst = lambda d: float(np.nanmax(d.r_hat)) if d is not None and np.any(~np.isnan(d.r_hat)) else np.nan
        least = lambda d: float(np.nanmin(d.n_eff)) if d is not None and np.any(~np.isnan(d.n_eff)) else np.nan
        sure = lambda d: int(d is not None and bool(np.all(d.reliable)))
        out = {k: np.array([getattr(r, k) for r in recs], dtype=np.int32) for k in ("n_iter", "n_changed", "n_switched", "n_used", "n_bad")}
        out["converged"] = np.array([r.converged for r in recs], dtype=np.int8)
        out["n_comp"] = np.array([f._n for f in fits], dtype=np.int32)
        out["max_r_hat_before"] = np.array([worst(f.mcmc._diag if i in ok else None) for i, f in enumerate(fits)], dtype=np.float64)
        by_region = dict(zip(ok, after))
        out["max_r_hat_after"] = np.array([worst(by_region.get(i)) for i in range(len(fits))], dtype=np.float64)
        first = [f.mcmc._diag if i in ok else None for i, f in enumerate(fits)]
        then = [by_region.get(i) for i in range(len(fits))]
        out["min_n_eff_before"], out["min_n_eff_after"] = (np.array([least(d) for d in ds], dtype=np.float64) for ds in (first, then))
        out["tau_reliable_before"], out["tau_reliable_after"] = (np.array([sure(d) for d in ds], dtype=np.int8) for ds in (first, then))
        q = max([r.label_mean.shape[1] for r in recs], default=3)
        mean, sd, owner = [], [], []
        for i, (f, r) in enumerate(zip(fits, recs)):
            qf = r.label_mean.shape[1]
            scale, shift = np.asarray(f._scale)[:qf], np.asarray(f._shift)[:qf]
            m, s = np.full((r.label_mean.shape[0], q), np.nan), np.full((r.label_mean.shape[0], q), np.nan)
            m[:, :qf], s[:, :qf] = r.label_mean * scale + shift, r.label_sd * np.abs(scale)
            mean.append(m); sd.append(s); owner += [i] * len(m)
        out["label_mean"] = np.concatenate(mean) if mean else np.zeros((0, q))
        out["label_sd"] = np.concatenate(sd) if sd else np.zeros((0, q))
        out["line_region"] = np.array(owner, dtype=np.int32)
        return out

    def write_relabel(self, rec):
        """``relabel()``'s dict as ``<prefix>relabel.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'relabel.h5'
        h5min.write(path, {k: np.array(v) for k, v in rec.items()})
        return path

    def fisher(self, with_prior=True):
        """After ``fit_spectrum`` (batched or not): Fisher-matrix errors of every kept fit at its current point (the MAP
        the fit ended on) from ONE GPU call (vamp_amd.fisher; each fit's ``fisher()`` cache is filled).  It reads no
        chain.  A dict; per line, in ``_harvest``'s order and units: ``std_a`` (amplitude), ``std_c`` (centre,
        wavelength), ``std_s`` (Gaussian sigma, frequency; of a Voigt line that of its G_fwhm) and ``std_L`` (L_fwhm;
        NaN for a Gaussian line) with ``line_region`` [n_lines]; per region ``status`` (0 ok, 1 information not positive
        definite, 2 bad point), ``logdet`` (ln det of the information in the caller's units), ``chi2``, ``grad_norm``
        (the largest |gradient| sqrt(cov_dd): how far from stationary the point is, in sigmas) and ``n_comp``
        [n_regions]."""
        from . import fisher
        fits = [r.fit for r in self.regions]
        recs = fisher.fits_fisher(fits, with_prior=with_prior, device=getattr(self, "device", 0))
        cols = {k: [] for k in ("std_a", "std_c", "std_s", "std_L")}
        owner = []
        for i, (f, r) in enumerate(zip(fits, recs)):
            q = f._q
            ev = f.estimated_variables
            for k in range(f._n):
                sg = r.sigma[q * k:q * k + q]
                nu = ev[k]['centroid'].value
                cols["std_a"].append(sg[0])
                cols["std_c"].append(Freq2wave(nu) * sg[1] / nu)           # lambda = c / nu
                cols["std_s"].append(VPfit.GaussianWidth(sg[3]) if f._voigt else sg[2])
                cols["std_L"].append(sg[2] if f._voigt else np.nan)
                owner.append(i)
        out = {k: np.array(v, dtype=np.float64) for k, v in cols.items()}
        out["line_region"] = np.array(owner, dtype=np.int32)
        out["status"] = np.array([r.status for r in recs], dtype=np.int32)
        out["logdet"] = np.array([r.logdet for r in recs], dtype=np.float64)
        out["chi2"] = np.array([r.chi2 for r in recs], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            out["grad_norm"] = np.array([np.max(np.abs(r.grad) * r.sigma) if r.status == 0 else np.nan for r in recs], dtype=np.float64)
        out["n_comp"] = np.array([f._n for f in fits], dtype=np.int32)
        return out

    def write_fisher(self, rec):
        """``fisher()``'s dict as ``<prefix>fisher.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'fisher.h5'
        h5min.write(path, {k: np.array(v) for k, v in rec.items()})
        return path

    def laplace(self, n_samples=4096, inflate=1.5, seed=None):
        """After ``fit_spectrum`` (batched or not): Laplace importance sampling of every kept fit at the point it ended
        on, from ONE Fisher call and ONE sampling call on the GPU (vamp_amd.laplace; each fit's ``laplace()`` cache is
        filled).  It reads no chain.  A dict; per region [n_regions]: ``lnZ`` / ``lnZ_se`` / ``lnZ_psis`` /
        ``lnZ_laplace`` / ``khat`` / ``ess``, ``n_out`` / ``status`` / ``n_comp`` (int32) and ``trusted`` (int8: status 0
        and khat <= 0.7); per line, in ``fisher()``'s order and in the fit's units (amplitude; centre, frequency; sigma
        or L_fwhm, G_fwhm, frequency): ``mean`` / ``sd`` [n_lines, q] (q = 4; the last column NaN for Gaussian lines)
        with ``line_region`` [n_lines].  A fit of more lines than the library takes (16) is left out of the call and
        has NaN rows and status -1."""
        from . import laplace
        fits = [r.fit for r in self.regions]
        ok = [f._n <= laplace.MAX_COMPONENTS for f in fits]
        got = iter(laplace.fits_laplace([f for f, o in zip(fits, ok) if o], n_samples=n_samples, inflate=inflate,
                                        seed=laplace.DEFAULT_SEED if seed is None else seed, device=getattr(self, "device", 0)))
        recs = [next(got) if o else None for o in ok]
        col = lambda k: np.array([np.nan if r is None else getattr(r, k) for r in recs], dtype=np.float64)
        out = {k: col(k) for k in ("lnZ", "lnZ_se", "lnZ_psis", "lnZ_laplace", "khat", "ess")}
        out["n_out"] = np.array([0 if r is None else r.n_out for r in recs], dtype=np.int32)
        out["status"] = np.array([-1 if r is None else r.status for r in recs], dtype=np.int32)
        out["trusted"] = np.array([int(r is not None and r.ok) for r in recs], dtype=np.int8)
        out["n_comp"] = np.array([f._n for f in fits], dtype=np.int32)
        mean, sd, owner = [], [], []
        for i, (f, r) in enumerate(zip(fits, recs)):
            q = 4 if int(f._mode) == 1 else 3
            for k in range(f._n):
                m, s = np.full(4, np.nan), np.full(4, np.nan)
                if r is not None:
                    m[:q], s[:q] = r.mean[q * k:q * k + q], r.sd[q * k:q * k + q]
                mean.append(m); sd.append(s); owner.append(i)
        out["mean"] = np.array(mean, dtype=np.float64).reshape(len(owner), 4)
        out["sd"] = np.array(sd, dtype=np.float64).reshape(len(owner), 4)
        out["line_region"] = np.array(owner, dtype=np.int32)
        return out

    def write_laplace(self, rec):
        """``laplace()``'s dict as ``<prefix>laplace.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'laplace.h5'
        h5min.write(path, {k: np.array(v) for k, v in rec.items()})
        return path

    def hmc(self, **kw):
        """After ``fit_spectrum`` (batched or not): Hamiltonian Monte Carlo chains of every kept fit from the point it ended
        on (vamp_amd.hmc.fits_hmc, keywords as there: ONE Fisher call, a few tuning calls and ONE kept run for the whole
        spectrum), and their convergence diagnostics from ONE call of libvamp_diag.so.  It reads no stretch-move chain and
        changes none.  A dict; per region [n_regions]: ``status`` (0 ok, 1 no Fisher covariance: no chain, -1 more lines
        than the library takes), ``accept_rate`` (mean over the chains), ``n_wall`` (steps that left the prior, all
        chains), ``eps``, ``n_comp``, ``n_chains`` (those whose start was accepted); per parameter, the regions one after
        the other and in the fit's units: ``mean`` / ``sd`` / ``r_hat`` / ``n_eff`` [n_par], ``quantiles`` [n_par, 3] (0.16,
        0.5, 0.84) with ``par_region`` [n_par].  With ``metric`` = "regularised" or "chain" (vamp_amd.metric) also ``n_low`` /
        ``n_high`` [n_regions], and ``status`` 1 means that the metric's status is not 0."""
        from . import diagnostics, hmc
        fits = [r.fit for r in self.regions]
        ok = [f._n <= hmc.MAX_COMPONENTS for f in fits]
        got = iter(hmc.fits_hmc([f for f, o in zip(fits, ok) if o], device=getattr(self, "device", 0), **kw))
        recs = [next(got) if o else None for o in ok]
        have = [i for i, r in enumerate(recs) if r is not None and r.status == 0 and np.any(r.chain_status == 0)
                and r.chain.shape[0] <= diagnostics.MAX_SAMPLES]
        chains = [np.ascontiguousarray(recs[i].chain[:, recs[i].chain_status == 0, :]) for i in have]
        diags = dict(zip(have, diagnostics.chain_diagnostics(chains, thin=[recs[i].thin for i in have], device=getattr(self, "device", 0)))) \
            if have else {}
        out = {"status": np.array([-1 if r is None else r.status for r in recs], dtype=np.int32),
               "accept_rate": np.array([np.nan if r is None or r.status else np.nanmean(r.accept_rate) for r in recs], dtype=np.float64),
               "n_wall": np.array([0 if r is None or r.status else int(np.sum(r.n_wall)) for r in recs], dtype=np.int32),
               "eps": np.array([np.nan if r is None else r.eps for r in recs], dtype=np.float64),
               "n_comp": np.array([f._n for f in fits], dtype=np.int32),
               "n_chains": np.array([0 if r is None or r.status else int(np.sum(r.chain_status == 0)) for r in recs], dtype=np.int32)}
        if kw.get("metric", "fisher") != "fisher":      # the directions the regularised metric repaired (-1: no record)
            out.update({k: np.array([-1 if r is None or getattr(r, k) is None else getattr(r, k) for r in recs], dtype=np.int32)
                        for k in ("n_low", "n_high")})
        cols = {k: [] for k in ("mean", "sd", "r_hat", "n_eff")}
        quant, owner = [], []
        for i, (f, r) in enumerate(zip(fits, recs)):
            D = len(f._scale)
            mean, sd, q = (np.full(D, np.nan), np.full(D, np.nan), np.full((3, D), np.nan)) if r is None or r.status else r.summary()
            d = diags.get(i)
            cols["mean"].append(mean); cols["sd"].append(sd)
            cols["r_hat"].append(np.full(D, np.nan) if d is None else d.r_hat)
            cols["n_eff"].append(np.full(D, np.nan) if d is None else d.n_eff)
            quant.append(q.T); owner += [i] * D
        out.update({k: np.concatenate(v) if v else np.zeros(0) for k, v in cols.items()})
        out["quantiles"] = np.concatenate(quant) if quant else np.zeros((0, 3))
        out["par_region"] = np.array(owner, dtype=np.int32)
        return out

    def write_hmc(self, rec):
        """``hmc()``'s dict as ``<prefix>hmc.h5`` through vamp_amd/h5min.py; returns the path"""
        from . import h5min
        path = self.output_filename + 'hmc.h5'
        h5min.write(path, {k: np.array(v) for k, v in rec.items()})
        return path

    def plot_spectrum(self):
        """total fit / components / residuals figures (vpspectrum.py:444-526); skipped without matplotlib"""
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            return
        model = self.flux_model['total']
        rows = 6
        length = len(self.flux_array) / rows
        wl = self.wavelength_array

        def brackets(ax):
            for (s, e) in self.region_pixels:
                for x, arm in ((wl[s], 0.1), (wl[min(e, len(wl) - 1)], -0.1)):
                    ax.plot((x, x), (0.9, 1.1), color='magenta')
                    ax.plot((x, x + arm), (0.9, 0.9), color='magenta')
                    ax.plot((x, x + arm), (1.1, 1.1), color='magenta')

        for tag in ('fit', 'components', 'residuals'):
            fig, ax = plt.subplots(rows, figsize=(15, 15))
            for r in range(rows):
                lo, hi = int(r * length), min(int(r * length + length), len(wl) - 1)
                if tag == 'fit':
                    ax[r].plot(wl, self.flux_array, c='black', label='Measured')
                    ax[r].plot(wl, model, c='green', label='Fit')
                elif tag == 'components':
                    for i, (s, e) in enumerate(self.region_pixels):
                        for row in self.flux_model['region_%d_flux' % i]:
                            ax[r].plot(wl[s:e], row, c='green')
                else:
                    ax[r].plot(wl, self.flux_array - model, c='blue')
                    for lvl, ls in ((1, '-'), (-1, '-'), (3, '--'), (-3, '--')):
                        ax[r].hlines(lvl, wl[0], wl[-1], color='red', linestyles=ls)
                brackets(ax[r])
                ax[r].set_xlim(wl[lo], wl[hi])
            plt.xlabel('Wavelength (A)')
            plt.ylabel('Flux')
            plt.savefig(self.output_filename + tag + '.png')
            plt.close(fig)

    def write_file(self):
        """``params`` and ``flux_model`` (vpspectrum.py:528-538) as HDF5 files: through h5py when it is
        importable, else through vamp_amd/h5min.py (same group / dataset structure; a bool such as
        ``difficult_fit`` is stored as int8)."""
        try:
            import h5py
        except ImportError:
            h5py = None
        for tag, d in (('params', self.params), ('flux_model', self.flux_model)):
            if h5py is not None:
                with h5py.File(self.output_filename + tag + '.h5', 'a') as f:
                    for p in d.keys():
                        f.create_dataset(p, data=np.array(d[p]))
            else:
                from . import h5min
                h5min.write(self.output_filename + tag + '.h5', {k: np.array(v) for k, v in d.items()})
