"""Writes tests/golden/metric/metric_cases.npz: the inputs of the test families of tests/metric_ref.py (matrix, scales, kind
and clamps) and, from mpmath's eigsy at 40 digits rounded to fp64, the eigenvalues of each case's scaled matrix B of
include/vamp_metric.h -- B exactly as fp64 holds it -- ascending.

    python tests/golden/make_metric_golden.py

The file has a folder of its own, as the Fisher fixture has: tests/golden/make_golden.py regenerates every .npz that lies
directly in tests/golden bit for bit, and this one is made by another script, in a few minutes of mpmath.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import metric_ref as ref  # noqa: E402

mp.mp.dps = 40


def main():
    out = {}
    for name in ref.case_names():
        spectrum, D = name.rsplit("_D", 1)
        c = ref.family(spectrum, int(D))
        B = ref.scaled(c)
        e = mp.eigsy(mp.matrix(B.tolist()), eigvals_only=True)
        eig = np.sort(np.array([float(v) for v in e]))
        out.update({name + "_mat": c["mat"], name + "_scale": c["scale"], name + "_par": np.array([c["kind"], c["lam_lo"], c["lam_hi"]]),
                    name + "_eig": eig})
        print(f"{name:16s} eig {eig[0]:.3e} .. {eig[-1]:.3e}", flush=True)
    os.makedirs(os.path.join(HERE, "metric"), exist_ok=True)
    np.savez(os.path.join(HERE, "metric", "metric_cases.npz"), **out)


if __name__ == "__main__":
    main()
