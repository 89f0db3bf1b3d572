"""``VPregion`` -- model selection for one absorption region (reference vamp_1.0/vpregion.py:8-91)
on top of the HIP-backed ``VPfit``.

Same constructor, attributes (``n``, ``freedom``, ``fit``, ``num_pixels`` ...) and the same
add-a-component-while-BIC-falls loop.  Host control flow only: every posterior evaluation and every
sampler step it triggers runs in libvamp_hip.so.  ``fit_region_pygadds`` (vpregion.py:94-144) is
dead Python-2 code in the reference and is not reproduced.
"""
from copy import copy

import numpy as np
from scipy.ndimage import gaussian_filter
from scipy.signal import argrelextrema

from .vpfits import VPfit

MAX_COMPONENTS = 32      # VAMP_MAX_COMPONENTS of include/vamp_hip.h (the reference sets no limit, vpspectrum.py:287-294)


class VPregion():

    def __init__(self, frequency_array, flux_array, noise_array, voigt=False, chi_limit=1.5, nwalkers=None, seed=None,
                 dtype=None, device=0):
        self.frequency_array = frequency_array
        self.flux_array = flux_array
        self.noise_array = noise_array
        self.voigt = voigt
        self.chi_limit = chi_limit
        self.num_pixels = len(flux_array)
        self.nwalkers = nwalkers
        self._seed = seed
        self.dtype, self.device = dtype, device    # per-pixel arithmetic of the fits (None: $VAMP_DTYPE, else fp64) and GPU
        self._attempt = 0         # region_fit calls so far: a retry must not replay the previous attempt's draws
        self.estimate_n()
        self.set_freedom()

    def estimate_n(self):
        """Initial guess of the number of lines: local minima of the flux smoothed with a
        sigma = 3 px Gaussian; fewer than 4 minima -> 1 (vpregion.py:21-35)."""
        self.n = argrelextrema(gaussian_filter(self.flux_array, 3), np.less)[0].shape[0]
        if self.n < 4:
            self.n = 1

    def set_freedom(self):
        """degrees of freedom = pixels - 3 n (3 n for Voigt too, vpregion.py:37-39)"""
        self.freedom = self.num_pixels - 3 * self.n

    def _fit_n(self, n, iterations, thin, burn):
        fit = VPfit(seed=None if self._seed is None else self._seed + 1000 * n + 1000003 * (self._attempt - 1),
                    dtype=self.dtype, device=self.device)
        if self.nwalkers is not None:
            fit.nwalkers = self.nwalkers
        fit.find_bic(self.frequency_array, self.flux_array, n, self.noise_array, self.freedom,
                     voigt=self.voigt, iterations=iterations, thin=thin, burn=burn)
        return fit

    def region_fit(self, verbose=True, iterations=3000, thin=15, burn=300, criterion='bic', evidence_kw=None):
        """BIC ladder of vpregion.py:42-91: fit n, then n+1, n+2, ... while the mean BIC of the
        three repeats keeps falling; stop early once the mean reduced chi^2 is under ``chi_limit``.
        The first rung is judged by the LAST of its three BICs, as in the reference (:63).
        ``criterion='evidence'``: the number of lines is chosen by ln Z instead (``_region_fit_evidence``);
        ``criterion='waic'``: by the expected log predictive density of the chains (``_region_fit_waic``);
        ``criterion='loo'``: the same ladder scored by PSIS-LOO (``_region_fit_loo``);
        ``criterion='laplace'``: by ln Z from importance sampling at each rung's MAP (``_region_fit_laplace``;
        ``evidence_kw``: keywords of ``VPfit.laplace``)."""
        if criterion == 'laplace':
            return self._region_fit_laplace(verbose, iterations, thin, burn, evidence_kw or {})
        if criterion == 'evidence':
            return self._region_fit_evidence(verbose, iterations, thin, burn, evidence_kw or {})
        if criterion == 'waic':
            return self._region_fit_waic(verbose, iterations, thin, burn)
        if criterion == 'loo':
            return self._region_fit_loo(verbose, iterations, thin, burn)
        if criterion != 'bic':
            raise ValueError("criterion must be 'bic', 'evidence' or 'waic' or 'loo' or 'laplace'")
        say = print if verbose else (lambda *a, **k: None)
        self._attempt += 1
        say("Setting initial number of lines to: {}".format(self.n))
        kept = self._fit_n(self.n, iterations, thin, burn)
        kept_bic = kept.bic_array[-1]
        while True:
            if self.n >= MAX_COMPONENTS:
                say("Reached the {}-component limit of the device kernels.".format(MAX_COMPONENTS))
                break
            self.n += 1
            say("Trying n={} lines.".format(self.n))
            trial = self._fit_n(self.n, iterations, thin, burn)
            trial_bic = float(np.average(trial.bic_array))
            if not (kept_bic > trial_bic):
                # the reference decrements n only inside `if verbose` (:82-86); the fit it keeps is
                # the previous rung, so n is restored unconditionally here
                self.n -= 1
                say("BIC rose from {:.2f} to {:.2f}: keeping n={}.".format(kept_bic, trial_bic, self.n))
                self._release(trial)
                break
            say("BIC fell from {:.2f} to {:.2f}.".format(kept_bic, trial_bic))
            self._release(kept)
            kept, kept_bic = copy(trial), trial_bic
            if np.average(trial.red_chi_array) < self.chi_limit:
                say("Reduced chi squared below {}: final n={}.".format(self.chi_limit, self.n))
                break
        self.fit = kept

    def _evidence_n(self, n, kw):
        """ln Z of the n-line model of this region: the model ``_fit_n`` fits (free sd, the fit's units)"""
        from . import evidence
        freq = np.asarray(self.frequency_array, dtype=np.float64)
        x = (freq - 0.5 * (freq[0] + freq[-1])) / ((freq[-1] - freq[0]) / (freq.size - 1))
        kw = dict(kw)
        kw.setdefault("seed", (evidence.DEFAULT_SEED if self._seed is None else self._seed) + 1000003 * (self._attempt - 1))
        return evidence.log_evidence({"x": x, "flux": self.flux_array, "noise": None, "sample_sd": True, "n_comp": n,
                                      "mode": 1 if self.voigt else 0, "region_id": n}, device=self.device or 0, **kw)

    def _region_fit_evidence(self, verbose, iterations, thin, burn, kw):
        """The ladder of vamp_2.0/vamp_src/phase/phase.py:108-139 made noise-aware: add a component while ln Z rises by
        more than the two rungs' combined standard error.  The records are kept as ``self.evidences[n]``; the kept fit
        is produced by ``find_bic`` as on the BIC path, and carries its record as ``fit.evidence``."""
        from . import evidence
        say = print if verbose else (lambda *a, **k: None)
        self._attempt += 1
        self.evidences = {self.n: self._evidence_n(self.n, kw)}
        while self.n < evidence.MAX_COMPONENTS:
            kept, trial = self.evidences[self.n], self._evidence_n(self.n + 1, kw)
            self.evidences[self.n + 1] = trial
            rise, se = trial.lnZ - kept.lnZ, float(np.hypot(kept.lnZ_se, trial.lnZ_se))
            if not rise > se:
                say("ln Z rose by {:.2f} (combined standard error {:.2f}): keeping n={}.".format(rise, se, self.n))
                break
            self.n += 1
            say("ln Z rose by {:.2f} (combined standard error {:.2f}): n={}.".format(rise, se, self.n))
        self.fit = self._fit_n(self.n, iterations, thin, burn)
        self.fit.evidence = self.evidences[self.n]

    def _waic_fit_n(self, n, iterations, thin, burn):
        """``_fit_n``, then one more ensemble run started at the fit's MAP and the MAP polish again.  ``find_bic`` samples
        BEFORE it polishes, from a ball around the first guess: what the BIC needs of that chain is its best sample, but
        WAIC averages over all of it, and at the ladder's lengths such a chain has not left its start (two-line data,
        300 steps: median ln p of the two-line chain -16 against 8 once it has).  The fit's nodes end at the MAP, as on
        the BIC path."""
        fit = self._fit_n(n, iterations, thin, burn)
        fit.mcmc.sample(iter=iterations, burn=burn, thin=thin)
        fit.map.fit(iterlim=iterations, tol=1e-3)
        return fit

    def _region_fit_waic(self, verbose, iterations, thin, burn):
        """Add a component while the expected log predictive density of the chain (vamp_amd.predictive) rises by more than
        the standard error of the difference, paired pixel by pixel.  Every rung is a ``_fit_n`` fit as on the BIC path,
        scored on a chain sampled from its MAP (``_waic_fit_n``); the records are kept as ``self.predictive[n]``, the
        kept fit carries its record as ``fit.predictive`` and the dropped fit is released."""
        from . import predictive
        say = print if verbose else (lambda *a, **k: None)
        self._attempt += 1
        say("Setting initial number of lines to: {}".format(self.n))
        kept = self._waic_fit_n(self.n, iterations, thin, burn)
        self.predictive = {self.n: kept.mcmc.waic()}
        while self.n < MAX_COMPONENTS:
            trial = self._waic_fit_n(self.n + 1, iterations, thin, burn)
            self.predictive[self.n + 1] = trial.mcmc.waic()
            rise, se = predictive.compare(self.predictive[self.n], self.predictive[self.n + 1])
            if not rise > se:
                say("elpd_waic rose by {:.2f} (paired standard error {:.2f}): keeping n={}.".format(rise, se, self.n))
                self._release(trial)
                break
            self.n += 1
            say("elpd_waic rose by {:.2f} (paired standard error {:.2f}): n={}.".format(rise, se, self.n))
            self._release(kept)
            kept = trial
        self.fit = kept
        self.fit.predictive = self.predictive[self.n]

    def _region_fit_loo(self, verbose, iterations, thin, burn):
        """The WAIC ladder's rungs (``_waic_fit_n``) scored by ``elpd_loo`` (vamp_amd.loo): add a component while it rises
        by more than the standard error of the difference, paired pixel by pixel.  The records are kept as
        ``self.loo[n]``, the kept fit carries its record as ``fit.loo`` and the dropped fit is released."""
        from . import predictive
        say = print if verbose else (lambda *a, **k: None)
        self._attempt += 1
        say("Setting initial number of lines to: {}".format(self.n))
        kept = self._waic_fit_n(self.n, iterations, thin, burn)
        self.loo = {self.n: kept.mcmc.loo()}
        while self.n < MAX_COMPONENTS:
            trial = self._waic_fit_n(self.n + 1, iterations, thin, burn)
            self.loo[self.n + 1] = trial.mcmc.loo()
            rise, se = predictive.compare(self.loo[self.n], self.loo[self.n + 1])
            if not rise > se:
                say("elpd_loo rose by {:.2f} (paired standard error {:.2f}): keeping n={}.".format(rise, se, self.n))
                self._release(trial)
                break
            self.n += 1
            say("elpd_loo rose by {:.2f} (paired standard error {:.2f}): n={}.".format(rise, se, self.n))
            self._release(kept)
            kept = trial
        self.fit = kept
        self.fit.loo = self.loo[self.n]

    def _region_fit_laplace(self, verbose, iterations, thin, burn, kw):
        """Add a component while ln Z by Laplace importance sampling (vamp_amd.laplace) rises by more than the two rungs'
        combined standard error.  Every rung is a ``_fit_n`` fit as on the BIC path, scored at the point it ended on
        (``fit.laplace()``: no further chain).  A rung whose record cannot be trusted -- status not 0, or khat above
        0.7 -- ends the ladder: it can neither be kept nor justify a further line, so the last trusted rung below it
        stays (the first rung stays whatever it is), and ``self.laplace_stop`` = (rung, reason) says so (None when the
        ladder ended on ln Z).  The records are kept as ``self.laplaces[n]``; the kept fit carries its record in its
        ``laplace()`` cache."""
        from . import laplace
        say = print if verbose else (lambda *a, **k: None)
        self._attempt += 1
        self.laplace_stop = None

        def distrust(n, rec):
            if rec.status != 0:
                return (n, "status {}".format(rec.status))
            if not rec.khat <= laplace.HIGH_KHAT:
                return (n, "khat {:.2f} above {}".format(rec.khat, laplace.HIGH_KHAT))
            return None

        say("Setting initial number of lines to: {}".format(self.n))
        kept = self._fit_n(self.n, iterations, thin, burn)
        self.laplaces = {self.n: kept.laplace(**kw)}
        self.laplace_stop = distrust(self.n, self.laplaces[self.n])
        while self.laplace_stop is None and self.n < min(MAX_COMPONENTS, laplace.MAX_COMPONENTS):
            trial = self._fit_n(self.n + 1, iterations, thin, burn)
            rec = self.laplaces[self.n + 1] = trial.laplace(**kw)
            self.laplace_stop = distrust(self.n + 1, rec)
            if self.laplace_stop is not None:
                self._release(trial)
                break
            rise, se = rec.lnZ - self.laplaces[self.n].lnZ, float(np.hypot(self.laplaces[self.n].lnZ_se, rec.lnZ_se))
            if not rise > se:
                say("ln Z rose by {:.2f} (combined standard error {:.2f}): keeping n={}.".format(rise, se, self.n))
                self._release(trial)
                break
            self.n += 1
            say("ln Z rose by {:.2f} (combined standard error {:.2f}): n={}.".format(rise, se, self.n))
            self._release(kept)
            kept = trial
        if self.laplace_stop is not None:
            say("The {}-line rung is not to be trusted ({}): the ladder stops, keeping n={}.".format(*self.laplace_stop, self.n))
        self.fit = kept

    @staticmethod
    def _release(fit):
        """Free the device context of a fit the ladder drops.  (The reference calls gc.collect() after every ladder,
        vpregion.py:90, to shed PyMC's models; a fit object and its MAP / MCMC stand-ins form a reference cycle here too,
        but its only heavy member is the context, closed here -- a full collection costs ~50 ms per ladder in a process
        that has torch loaded: 3.7 of the 6.8 s of a 20-region sequential fit.)"""
        ctx = getattr(fit, "_ctx", None)
        if ctx is not None and not getattr(fit, "_shared_ctx", False) and hasattr(ctx, "close"):
            ctx.close()
