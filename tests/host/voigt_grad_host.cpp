// Host build of vamp_amd/csrc/voigt_grad.hpp for tests/test_fisher.py: the arithmetic of the device's derivative
// evaluator, compiled with -ffp-contract=off.
#include "../../vamp_amd/csrc/voigt_grad.hpp"

namespace {
template <bool PLANTED>
void grad_n(int n, const double* u, const double* y, double* out) {
    double dtab[vamp::DTAB_N];
    double y_tab = -1.0, pole = 0.0, hy = 0.0;
    for (int i = 0; i < n; ++i) {
        if (y[i] != y_tab) {
            y_tab = y[i];
            for (int e = 0; e < vamp::DTAB_N; ++e) dtab[e] = vamp::core_dtab_entry(e, y_tab);
            pole = vamp::core_pole_factor(y_tab);
            hy = vamp::core_hy(y_tab);
        }
        const vamp::VoigtGrad g = vamp::voigt_grad<PLANTED>(u[i], y[i], dtab, pole, hy);
        out[4 * i + 0] = g.Ks;
        out[4 * i + 1] = g.Ku;
        out[4 * i + 2] = g.TL;
        out[4 * i + 3] = g.TG;
    }
}
}  // namespace

// out[4 n]: (sqrt(pi) K, K_u, K + y K_y, K + u K_u + y K_y) at (u[i], y[i])
extern "C" void voigt_grad_n(int n, const double* u, const double* y, double* out) { grad_n<false>(n, u, y, out); }
// the same with the large-|z| branch replaced by the identity on the fractions' w
extern "C" void voigt_grad_planted_n(int n, const double* u, const double* y, double* out) { grad_n<true>(n, u, y, out); }
