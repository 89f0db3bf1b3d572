// voigt_grad.hpp -- the Voigt function and its first derivatives, for the Jacobian of the model flux (fisher.hip;
// host build: tests/host/voigt_grad_host.cpp).  Definitions: DESIGN.md section 15.
//
// With w(u + i y) = K + i M (y >= 0, u of either sign) one call returns
//     Ks = sqrt(pi) K,   Ku = K_u,   TL = K + y K_y,   TG = K + u K_u + y K_y ,
// the four combinations the derivatives of tau_k = A y sqrt(pi) K with respect to (A, c, L_fwhm, G_fwhm) are made of.
//
//   |z|^2 < 64    K and M from the centred trapezoid rule of voigt_math.hpp (the real part as voigt_core has it, the
//                 imaginary part from the same nodes), then w' = -2 z w + 2i / sqrt(pi):
//                     K_u = -2 (u K - y M),   K_y = 2 (u M + y K) - 2 / sqrt(pi).
//                 The identity amplifies the error of w by at most 2 |z|^2 <= 128 here.
//   |z|^2 >= 64   the identity cancels (K + u K_u + y K_y is O(|z|^-3) and its terms O(|z|^-1 .. |z|)), so the
//                 partial fractions are differentiated instead.  sqrt(pi) w = i sum_j c_j z / (z^2 - zeta_j) (the
//                 Gauss-Hermite form of GHFrac) gives, term by term and with no cancellation,
//                     sqrt(pi) w'         = -i sum_j c_j (z^2 + zeta_j) / (z^2 - zeta_j)^2
//                     sqrt(pi) (w + z w') = -2 i sum_j c_j zeta_j z / (z^2 - zeta_j)^2
//                 and TG = Re(w + z w'), TL = TG - u K_u.  One table serves every |z|^2 >= 64: the 12 positive nodes
//                 of the 24-point rule (GRAD_Z, GRAD_C).  The first moment the rule misses is z^-49: relative to TG
//                 itself the truncation is < 1e-16 at |z|^2 = 64 (the 6-level fraction of the value evaluator, good to
//                 3e-15 in K, would leave ~1e-11 in TG there: a derivative's series loses a factor n |z|^2).
//   y < 1e-9      the fractions miss the Gaussian core e^{-u^2} of K (voigt_math.hpp); it and its derivatives are
//                 added, so that L = 0 gives TL = e^{-u^2} at every u.
#pragma once

#include "voigt_math.hpp"

namespace vamp {

constexpr int GRAD_M = 12;
// squares of the positive nodes of the 24-point Gauss-Hermite rule and twice their normalised weights (sum = 1),
// from the eigenvalues of the rule's Jacobi matrix at 50 digits (tools/gen_voigt_tables.py, gh_nodes_squared(12))
constexpr double GRAD_Z[GRAD_M] = {0.0503618891172939512, 0.454506681563780278, 1.26958994010396148, 2.50984809723212803,
                                   4.1984156448784132,    6.36997538803063494, 9.07543423096120303, 12.3904479638094714,
                                   16.432195087675313,    21.3967559361661095, 27.6611087798460896, 36.1913603606156016};
constexpr double GRAD_C[GRAD_M] = {0.481740231093280651,   0.322919025734000173,   0.144138728034356659,   0.0422526888179350933,
                                   0.00795321785836261728, 0.000929437437558791401, 0.000064190011305491825, 2.43531949088516264e-6,
                                   4.53492334696128398e-8, 3.43732985592971604e-10, 7.42994830552479708e-13, 1.87803873780839121e-16};
// e^{-j^2/4}: the weights of the trapezoid rule's nodes about the centre node
constexpr double GRAD_CJ[CORE_J + 1] = {1.0, 0.77880078307140486825, 0.3678794411714423216, 0.10539922456186433678,
                                        0.018315638888734180294, 0.0019304541362277092422, 0.0001234098040866795495,
                                        4.7851173921290090896e-6, 1.1253517471925911451e-7, 1.6052280551856116087e-9,
                                        1.3887943864964020595e-11, 7.2877240958196924193e-14, 2.3195228302435693883e-16,
                                        4.477732441718301199e-19};

struct VoigtGrad {
    double Ks, Ku, TL, TG;
};

// sqrt(pi) (K, M) at 0 <= x < 8 from the line's near-axis table (core_dtab_entry, core_pole_factor, core_hy):
//   sqrt(pi) K = h y / sqrt(pi) sum_n e^{-(x - u_n)^2} / (u_n^2 + y^2) + pole e^{-x^2} cos 2xy
//   sqrt(pi) M = h / sqrt(pi) sum_n e^{-(x - u_n)^2} u_n / (u_n^2 + y^2) - pole e^{-x^2} sin 2xy
// with u_{n0 + j} = x - d + j h and e^{-(d - j h)^2} = e^{-d^2} e^{d j} e^{-j^2/4} (h = 1/2)
VAMP_DEV void voigt_core_w(double x, double y, const double* dtab, double pole, double hy, double& re, double& im) {
    const int n0 = (int)(x * 2.0);
    const double d = x - (n0 + 0.5) * CORE_H;            // |d| <= h/2
    const double g0 = exp_taylor(-(d * d));
    const double q = exp_taylor(d), qi = exp_taylor(-d);
    const double* p = dtab + n0 + DTAB_OFF;
    double s0 = 0.0, s1 = 0.0;
    double qp[CORE_J + 1], qm[CORE_J + 1];
    qp[0] = qm[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= CORE_J; ++j) { qp[j] = qp[j - 1] * q; qm[j] = qm[j - 1] * qi; }
#pragma unroll
    for (int j = CORE_J; j >= 1; --j) {                  // small terms first
        const double a = GRAD_CJ[j] * qp[j] * p[j], b = GRAD_CJ[j] * qm[j] * p[-j];
        s0 += a + b;
        s1 += (double)j * (a - b);
    }
    s0 += p[0];
    re = hy * (g0 * s0);
    im = (CORE_H * INV_SQRT_PI) * (g0 * ((x - d) * s0 + CORE_H * s1));
    if (pole != 0.0) {
        double sn, cs;
        sincos_small(2.0 * x * y, sn, cs);
        const double e = pole * exp_neg_sq(x);
        re += e * cs;
        im -= e * sn;
    }
}

// the large-|z| branch; x >= 0.  planted = true puts the identity on the fractions' w instead (tests only: it shows
// that the test of this branch can fail)
VAMP_DEV void voigt_grad_far(double x, double y, bool planted, double& Ks, double& Kus, double& TLs, double& TGs) {
    // |z| beyond 1e60: z is brought to unit size first, so that (z^2)^2 cannot overflow
    const double sc = (x > 1e60 || y > 1e60) ? 1.0 / fmax(x, y) : 1.0;
    const double xs = x * sc, ys = y * sc;
    const double zr = xs * xs - ys * ys, zi = 2.0 * xs * ys;      // z^2 (scaled by sc^2)
    const double sc2 = sc * sc;
    double wr = 0.0, wi = 0.0, di = 0.0, gr = 0.0, gi = 0.0;
    for (int j = GRAD_M - 1; j >= 0; --j) {                       // small terms first
        const double zt = GRAD_Z[j] * sc2;
        const double ar = zr - zt, ai = zi;                       // z^2 - zeta
        const double inv = 1.0 / (ar * ar + ai * ai);
        const double rr = ar * inv, ri = -ai * inv;               // 1 / (z^2 - zeta)
        const double r2r = rr * rr - ri * ri, r2i = 2.0 * rr * ri;    // its square
        wr += GRAD_C[j] * rr;
        wi += GRAD_C[j] * ri;
        const double br = zr + zt, bi = zi;                       // z^2 + zeta
        di += GRAD_C[j] * (br * r2i + bi * r2r);
        gr += (GRAD_C[j] * zt) * r2r;
        gi += (GRAD_C[j] * zt) * r2i;
    }
    // sqrt(pi) w = i z sum c / (z^2 - zeta);   sqrt(pi) w' = -i sum c (z^2 + zeta) / (z^2 - zeta)^2;
    // sqrt(pi) (w + z w') = -2 i z sum c zeta / (z^2 - zeta)^2      (undoing the scale: w ~ sc, w' ~ sc^2, w + z w' ~ sc)
    const double Wr = -(xs * wi + ys * wr) * sc, Wi = (xs * wr - ys * wi) * sc;     // i z s = i (x + i y)(sr + i si)
    Ks = Wr;
    Kus = di * sc2;                                               // Re(-i (dr + i di)) = di: only the imaginary part of the sum is needed
    if (!planted) {
        TGs = 2.0 * (xs * gi + ys * gr) * sc;                     // Re(-2 i z g) = 2 Im(z g)
        TLs = TGs - (xs * di) * sc;                               // u K_u, scaled before it is multiplied out
    } else {
        const double Ky = 2.0 * (x * Wi + y * Wr) - 2.0;          // sqrt(pi) K_y by the identity
        const double Kui = -2.0 * (x * Wr - y * Wi);
        Kus = Kui;
        TLs = Wr + y * Ky;
        TGs = TLs + x * Kui;
    }
    if (y < Y_TINY) {
        const double e = SQRT_PI * exp_neg_sq(x);
        Ks += e;
        Kus -= 2.0 * x * e;
        TLs += e;
        TGs += e * (1.0 - 2.0 * x * x);
    }
}

// u of either sign, y >= 0; dtab, pole, hy: the line's near-axis constants, as voigt_Hs takes them
template <bool PLANTED = false>
VAMP_DEV VoigtGrad voigt_grad(double u, double y, const double* dtab, double pole, double hy) {
    const double x = fabs(u);
    const double r2 = fma(x, x, y * y);
    double Ks, Kus, TLs, TGs;
    if (r2 < R2_CORE) {                                           // (NaN compares false: no table lookup)
        double Ms;
        voigt_core_w(x, y, dtab, pole, hy, Ks, Ms);
        Kus = -2.0 * (x * Ks - y * Ms);
        const double Kys = 2.0 * (x * Ms + y * Ks) - 2.0;
        TLs = Ks + y * Kys;
        TGs = TLs + x * Kus;
    } else {
        voigt_grad_far(x, y, PLANTED, Ks, Kus, TLs, TGs);
    }
    VoigtGrad g;
    g.Ks = Ks;
    g.Ku = (u < 0.0 ? -Kus : Kus) * INV_SQRT_PI;                  // K is even in u, K_u odd
    g.TL = TLs * INV_SQRT_PI;
    g.TG = TGs * INV_SQRT_PI;
    return g;
}

}  // namespace vamp
