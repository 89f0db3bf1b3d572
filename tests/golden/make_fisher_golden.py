"""Writes tests/golden/fisher/fisher_cases.npz: inputs and, from a 40-digit mpmath computation rounded to fp64, the expected
Jacobian, gradient, information matrix, covariance, ln det and chi^2 of include/vamp_fisher.h per
case; kappa, the 2-norm condition number of the scaled information; and E_id, the error of the scipy-identity
restatement of J (tests/fisher_ref.py) over the column maximum -- reference against reference.

    python tests/golden/make_fisher_golden.py

The file has a folder of its own: tests/golden/make_golden.py regenerates every .npz that lies directly in tests/golden
bit for bit (tests/test_oracle.py), and this one is made by another script, in 25 s of mpmath.

Cases: the non-NBZ cases of lnprob_cases.npz (the first 4 walkers with a finite log-posterior and kappa <= 1e6); one Voigt
line on 24 pixels over L/G from 0 to 1e3 (compared on J only); P in {1, 63, 64, 65, 129} at K = 2; K = 16 Voigt with free
sd (D = 65) on 65 pixels and K = 16 Gaussian (D = 48); a line whose centre lies 1e4 widths outside the region; the
points of status 1 (L = 0 exactly, two identical lines).
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import fisher_ref as ref  # noqa: E402

mp.mp.dps = 40
KAPPA_MAX = 1e6
SWEEP = (0.0, 1e-12, 1e-6, 1e-3, 0.1, 1.0, 10.0, 100.0, 1e3)


def wofz_mp(z):
    if abs(z) > 50:                       # Laplace's continued fraction, from the tail: converged far past 40 digits
        t = z
        for n in range(80, 0, -1):
            t = z - (mp.mpf(n) / 2) / t
        return 1j / (mp.sqrt(mp.pi) * t)
    return mp.exp(-z * z) * mp.erfc(-1j * z)


def line_terms_mp(x, th, mode):
    """per pixel (tau, [dtau / dtheta])"""
    out = []
    ln2 = mp.sqrt(mp.log(2))
    spi = mp.sqrt(mp.pi)
    if mode == 1:
        A, c, L, G = (mp.mpf(float(v)) for v in th)
        s, y = 2 * ln2 / G, L * ln2 / G
        for xv in x:
            u = (mp.mpf(float(xv)) - c) * s
            z = mp.mpc(u, y)
            w = wofz_mp(z)
            wp = -2 * z * w + 2j / spi
            K, Ku, Ky = w.real, wp.real, -wp.imag
            out.append((A * y * spi * K, [y * spi * K, -A * y * spi * s * Ku, A * spi * (ln2 / G) * (K + y * Ky),
                                          -(A * spi * y / G) * (K + u * Ku + y * Ky)]))
    else:
        A, c, sg = (mp.mpf(float(v)) for v in th)
        for xv in x:
            u = (mp.mpf(float(xv)) - c) / sg
            e = mp.exp(-u * u / 2)
            out.append((A * e, [e, A * e * u / sg, A * e * u * u / sg]))
    return out


def case_mp(x, flux, noise, theta, K, mode, with_prior=True, matrices=True):
    q = ref.q_of(mode)
    sd = noise is None
    P, Dl = len(x), q * K
    D = Dl + int(sd)
    tau = [mp.mpf(0)] * P
    dt = [[mp.mpf(0)] * D for _ in range(P)]
    for k in range(K):
        for p, (t, d) in enumerate(line_terms_mp(x, theta[q * k:q * k + q], mode)):
            tau[p] += t
            dt[p][q * k:q * k + q] = d
    f = [mp.exp(-t) for t in tau]
    J = mp.matrix(P, D)
    for p in range(P):
        for d in range(D):
            J[p, d] = -f[p] * dt[p][d]
    sig = [mp.mpf(float(theta[-1]))] * P if sd else [mp.mpf(float(v)) for v in noise]
    rs = [(mp.mpf(float(flux[p])) - f[p]) / sig[p] for p in range(P)]
    a = mp.matrix(P, D)
    for p in range(P):
        for d in range(D):
            a[p, d] = J[p, d] / sig[p]
    chi2 = mp.fsum(r * r for r in rs)
    grad = [mp.fsum(a[p, d] * rs[p] for p in range(P)) for d in range(D)]
    info = a.T * a
    if with_prior:
        for d in range(0, Dl, q):
            A = mp.mpf(float(theta[d]))
            grad[d] += 1 / A - 1
            info[d, d] += 1 / (A * A)
    if sd:
        s = mp.mpf(float(theta[-1]))
        grad[Dl] = chi2 / s - P / s
        info[Dl, Dl] = 2 * P / (s * s)
    tof = lambda m: np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])
    out = {"jac": tof(J), "grad": np.array([float(g) for g in grad]), "info": tof(info), "chi2": float(chi2)}
    out["kappa"] = ref.kappa(out["info"])
    out["cov"], out["logdet"] = np.full((D, D), np.nan), np.nan
    if matrices and out["kappa"] <= 1e12:
        try:
            # through the scaled matrix (mpmath's LU refuses pivots that are small in absolute terms: a region in Hz has
            # information entries of 1e-44); at 40 digits the scaling costs nothing
            d = [mp.sqrt(info[i, i]) for i in range(D)]
            C = mp.matrix(D, D)
            for i in range(D):
                for j in range(D):
                    C[i, j] = info[i, j] / (d[i] * d[j])
            S = mp.inverse(C)
            for i in range(D):
                for j in range(D):
                    S[i, j] = S[i, j] / (d[i] * d[j])
            out["cov"] = tof(S)
            out["logdet"] = float(mp.log(mp.det(C)) + 2 * mp.fsum(mp.log(v) for v in d))
        except ZeroDivisionError:
            pass
    _, Jid = ref.jacobian(x, np.asarray(theta, dtype=np.float64), K, mode, sd)
    cm = np.abs(out["jac"]).max(axis=0)
    with np.errstate(all="ignore"):
        e = np.abs(Jid - out["jac"]) / cm
    out["e_id"] = float(np.nanmax(np.where(cm > 0, e, 0.0)))
    return out


def synth(x, lines, mode, noise_level, seed, sd=False):
    """data of the given lines with a fixed pattern of noise, and a point beside the truth"""
    rng = np.random.default_rng(seed)
    K = len(lines)
    truth = np.array(lines, dtype=np.float64).ravel()
    f, _ = ref.jacobian(x, truth, K, mode)
    flux = f + noise_level * rng.standard_normal(len(x))
    theta = truth * (1.0 + 0.03 * rng.uniform(-1, 1, truth.size))
    if sd:
        theta = np.append(theta, noise_level * 1.1)
    return flux, (None if sd else np.full(len(x), noise_level)), theta


def main():
    g = np.load(os.path.join(HERE, "lnprob_cases.npz"), allow_pickle=False)
    cases = []          # (name, x, flux, noise or None, theta, K, mode, kind)
    done = {}           # name -> case_mp's result, where the selection computed it already

    for name in sorted({k.rsplit("_", 1)[0] for k in g.files if "_" in k}):
        if "_m2_" in name or name + "_theta" not in g.files:
            continue
        K = int(name.split("_K")[1].split("_")[0])
        mode = int(name.split("_m")[1].split("_")[0])
        sd = name.endswith("sd1")
        x, flux, noise = g[name + "_x"], g[name + "_flux"], (None if sd else g[name + "_noise"])
        taken = 0
        for w in np.flatnonzero(np.isfinite(g[name + "_lnprob"])):
            th = g[name + "_theta"][w]
            r = case_mp(x, flux, noise, th, K, mode)       # kappa of the 40-digit information: scipy's identity is no judge at large y
            if r["kappa"] > KAPPA_MAX:
                continue
            done[f"{name}_w{w}"] = r
            cases.append((f"{name}_w{w}", x, flux, noise, th, K, mode, "full"))
            taken += 1
            if taken == 4:
                break
        assert taken == 4, name

    x24 = np.arange(24.0) - 11.5
    for r in SWEEP:
        flux, noise, _ = synth(x24, [(1.3, 0.4, 3.0 * max(r, 1e-3), 3.0)], 1, 0.05, 7)
        cases.append((f"sweep_LG{r:g}", x24, flux, noise, np.array([1.3, 0.4, 3.0 * r, 3.0]), 1, 1, "jac"))

    for P in (1, 63, 64, 65, 129):
        x = np.linspace(-0.5 * P, 0.5 * P, P) if P > 1 else np.array([0.3])
        w = max(P, 24) / 12.0
        flux, noise, th = synth(x, [(1.1, -1.5 * w, 0.4 * w, w), (0.7, 1.8 * w, 0.2 * w, 0.8 * w)], 1, 0.03, 100 + P)
        cases.append((f"pix_P{P}", x, flux, noise, th, 2, 1, "full"))

    x65 = np.arange(65.0) - 32.0
    lines = [(0.4 + 0.05 * k, -30.0 + 4.0 * k, 0.5 + 0.02 * k, 1.5 + 0.05 * k) for k in range(16)]
    flux, noise, th = synth(x65, lines, 1, 0.02, 11, sd=True)
    cases.append(("K16_voigt_sd", x65, flux, noise, th, 16, 1, "full"))
    x200 = np.arange(200.0) - 99.5
    lines = [(0.5 + 0.05 * k, -90.0 + 12.0 * k, 2.0 + 0.05 * k) for k in range(16)]
    flux, noise, th = synth(x200, lines, 0, 0.02, 12)
    cases.append(("K16_gauss", x200, flux, noise, th, 16, 0, "full"))

    x40 = np.arange(40.0) - 19.5
    flux, noise, th = synth(x40, [(1.2, 1.0, 1.0, 3.0), (0.8, 19.5 + 2.5e4, 0.5, 2.0)], 1, 0.04, 13)
    cases.append(("far_line", x40, flux, noise, th, 2, 1, "full"))

    # status 1: a point with L = 0 exactly (a zero column) and a point of two identical lines
    flux, noise, th = synth(x40, [(1.2, 1.0, 1.0, 3.0)], 1, 0.04, 14)
    th[2] = 0.0
    cases.append(("flat_L0", x40, flux, noise, th, 1, 1, "flat"))
    flux, noise, th = synth(x40, [(0.6, 1.0, 2.5), (0.6, 1.0, 2.5)], 0, 0.04, 15)
    th[3:6] = th[0:3]
    cases.append(("flat_twins", x40, flux, noise, th, 2, 0, "flat"))

    # File layout (tests/fisher_ref.py's load_cases reads it): a region (x, flux, noise) is stored once under its own
    # name and shared by its points; a case is ONE array, theta | grad | grad without prior | diagonal of the information
    # without prior (only the amplitudes' entries differ) | info | cov (lower triangles, row by row) | jac, and a row
    # (K, mode, logdet, chi2, kappa, e_id) of ``meta``.
    out = {"cases": np.array([c[0] for c in cases]), "kinds": np.array([c[7] for c in cases])}
    regions, meta = [], []
    for name, x, flux, noise, th, K, mode, kind in cases:
        r = done.get(name) or case_mp(x, flux, noise, th, K, mode, matrices=kind == "full")
        D = len(th)
        nan = np.full(D, np.nan)
        r0 = case_mp(x, flux, noise, th, K, mode, with_prior=False, matrices=False) if kind == "full" else None
        region = name.rsplit("_w", 1)[0] if kind == "full" and "_w" in name else name
        regions.append(region)
        if f"{region}_x" not in out:
            out.update({f"{region}_x": x, f"{region}_flux": flux})
            if noise is not None:
                out[f"{region}_noise"] = noise
        tril = np.tril_indices(D)
        out[name] = np.concatenate([th, r["grad"], nan if r0 is None else r0["grad"], nan if r0 is None else np.diag(r0["info"]),
                                    r["info"][tril], r["cov"][tril], r["jac"].ravel()])
        meta.append([K, mode, r["logdet"], r["chi2"], r["kappa"], r["e_id"]])
        print(f"{name:32s} D={len(th):2d} P={len(x):3d} kappa={r['kappa']:.3g} e_id={r['e_id']:.2e}", flush=True)
    out["regions"], out["meta"] = np.array(regions), np.array(meta, dtype=np.float64)
    os.makedirs(os.path.join(HERE, "fisher"), exist_ok=True)
    path = os.path.join(HERE, "fisher", "fisher_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
