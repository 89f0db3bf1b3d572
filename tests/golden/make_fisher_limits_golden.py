"""Writes tests/golden/fisher/fisher_limits.npz for tests/test_fisher_limits.py and tests/test_gpu_fisher_limits.py (the case
tables: tests/fisher_limit_cases.py).  Data only; mpmath is used here and nowhere in the tests.

    python tests/golden/make_fisher_limits_golden.py          (20 s of mpmath)

Evaluator cases (one Voigt line each): per pixel, at the fp64 (u, y) the kernel forms, w, w' = -2 z w + 2i / sqrt(pi) and
g = w + z w' computed with 50 + 8 log10 max(|z|, 1) digits -- each of the two cancellations costs 2 log10 |z| digits of
the continued fraction's w, and the 40 digits of make_fisher_golden.py leave only 1e-11 of g at |z| = 1e6 -- then tau
and the line's four columns of J, all rounded to fp64: <name>_ref [P, 11] = Re w, Im w, Re w', Im w', Re g, Im g, tau, J.
eval_meta = (E_sc, b_core, E_sc of fisher_ref.jacobian itself): E_sc is the worst error over the core scales of
tests/fisher_limit_cases.py of the scipy-identity restatement of J at the same (u, y), b_core = max(2 E_sc, 16 eps);
fisher_ref.jacobian forms u and y with numpy's sqrt(ln 2), an ulp from the kernel's, and its own figure is kept beside
it (the smaller of the two sets the bar).

Dealing and pixel-edge cases: the layout of fisher_cases.npz (make_fisher_golden.py: keys cases, kinds, regions, meta and
one packed array per case, read by fisher_ref.load_cases), 40 digits.  Every one must have kappa <= 1e6, asserted here,
except pixel_P2, whose information is singular by counting (kind 'flat')."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import fisher_limit_cases as fl  # noqa: E402
import fisher_ref as ref  # noqa: E402
import make_fisher_golden as mg  # noqa: E402

KAPPA_MAX = 1e6


def eval_reference(x, th):
    """[P, 11] of the module's docstring"""
    u, y, s = fl.line_uy(x, th)
    A, G = float(th[0]), float(th[3])
    rows = []
    for uv in u:
        r = max(abs(float(uv)), float(y), 1.0)
        mp.mp.dps = int(50 + 8 * np.log10(r))
        z = mp.mpc(mp.mpf(float(uv)), mp.mpf(float(y)))
        spi = mp.sqrt(mp.pi)
        w = mg.wofz_mp(z)
        wp = -2 * z * w + 2j / spi
        g = w + z * wp
        K, Ku, Ky = w.real, wp.real, -wp.imag
        ym, sm = mp.mpf(float(y)), mp.mpf(float(s))
        tau = A * ym * spi * K
        f = mp.exp(-tau)
        Q = [K, Ku, K + ym * Ky, g.real]
        pf = [ym * spi, -A * ym * spi * sm, A * spi * (sm / 2), -(A * ym * spi) / mp.mpf(G)]
        rows.append([float(w.real), float(w.imag), float(wp.real), float(wp.imag), float(g.real), float(g.imag), float(tau)]
                    + [float(-f * p * q) for p, q in zip(pf, Q)])
    mp.mp.dps = 40
    return np.array(rows)


def main():
    out = {"eval_cases": np.array(fl.EVAL_NAMES)}
    for name in fl.EVAL_NAMES:
        x, th = fl.eval_inputs(name)
        v = eval_reference(x, th)
        out[name + "_x"], out[name + "_theta"], out[name + "_ref"] = x, th, v
        out[name + "_flux"] = np.exp(-v[:, 6]) + 0.03 * np.cos(1.3 * np.arange(len(x)))
    out["eval_meta"] = np.zeros(3)
    path = os.path.join(HERE, "fisher", "fisher_limits.npz")
    np.savez_compressed(path, **out)
    e_bits = e_ref = 0.0
    for c in fl.load_eval(path)[0]:
        core_s, _ = fl.entry_scales(c)
        core = fl.is_core(c)
        scale = (np.exp(-c["tau"])[:, None] * np.abs(fl.prefactors(c))[None, :]) * core_s
        ok = core[:, None] & (scale > 0)
        _, Jr = ref.jacobian(c["x"], c["theta"], 1, 1)
        worst = [float(np.max(np.where(ok, np.abs(J - c["jac"]) / np.where(ok, scale, 1.0), 0.0))) for J in (fl.scipy_jacobian(c), Jr)]
        print(f"{c['name']:14s} P={c['P']:2d} core pixels {int(core.sum()):2d}  scipy identity over core scale: same bits {worst[0]:.2e}"
              f"  fisher_ref.jacobian {worst[1]:.2e}", flush=True)
        e_bits, e_ref = max(e_bits, worst[0]), max(e_ref, worst[1])
    e_sc = min(e_bits, e_ref)
    out["eval_meta"] = np.array([e_sc, max(2 * e_sc, 16 * fl.EPS), e_ref])
    print(f"E_sc = {e_sc:.3e} (fisher_ref.jacobian itself: {e_ref:.3e})  b_core = {out['eval_meta'][1]:.3e}", flush=True)

    cases = []          # (name, x, flux, noise or None, theta, K, mode, kind)
    for i, (name, mode, K, sd) in enumerate(fl.DEALING):
        x, lines = fl.dealing_inputs(mode, K, sd)
        flux, noise, th = mg.synth(x, lines, mode, 0.02, 200 + i, sd=sd)
        cases.append((name, x, flux, noise, th, K, mode, "full"))
    for name, mode, K, P in fl.PIXEL_EDGES:
        x, lines = fl.pixel_inputs(K, P)
        flux, noise, th = mg.synth(x, lines, mode, 0.03, 300 + P)
        cases.append((name, x, flux, noise, th, K, mode, "flat" if name == "pixel_P2" else "full"))

    out.update({"cases": np.array([c[0] for c in cases]), "kinds": np.array([c[7] for c in cases]),
                "regions": np.array([c[0] for c in cases])})
    meta = []
    for name, x, flux, noise, th, K, mode, kind in cases:
        r = mg.case_mp(x, flux, noise, th, K, mode, matrices=kind == "full")
        D = len(th)
        assert kind == "flat" or r["kappa"] <= KAPPA_MAX, (name, r["kappa"])
        assert kind == "full" or not r["kappa"] <= 1e12, (name, r["kappa"])
        nan = np.full(D, np.nan)
        r0 = mg.case_mp(x, flux, noise, th, K, mode, with_prior=False, matrices=False) if kind == "full" else None
        out.update({f"{name}_x": x, f"{name}_flux": flux})
        if noise is not None:
            out[f"{name}_noise"] = noise
        tril = np.tril_indices(D)
        out[name] = np.concatenate([th, r["grad"], nan if r0 is None else r0["grad"], nan if r0 is None else np.diag(r0["info"]),
                                    r["info"][tril], r["cov"][tril], r["jac"].ravel()])
        meta.append([K, mode, r["logdet"], r["chi2"], r["kappa"], r["e_id"]])
        print(f"{name:20s} D={D:2d} P={len(x):3d} kappa={r['kappa']:.3g} e_id={r['e_id']:.2e}", flush=True)
    out["meta"] = np.array(meta, dtype=np.float64)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 800_000


if __name__ == "__main__":
    main()
