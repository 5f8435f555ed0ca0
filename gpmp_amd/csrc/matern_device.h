// Device helpers shared by the Gram / gradient kernels of gram.hip and the prediction-gradient kernels of predict_grad.hip: the
// Matern polynomial, the fp64 sqrt / exp used on the hot path, and the host-side coefficient tables and parameter setup.
// Everything is internal to the translation unit that includes it.
#pragma once
#include "common.h"
#include <cfloat>
#include <cmath>
#include <vector>

namespace gpmp {
namespace {

constexpr int GT = 64;   // tile edge
constexpr int DC = 16;   // dimensions per LDS chunk

struct MaternSpec {
  int p;
  double c;                      // 2 sqrt(p + 1/2)
  double q[GPMP_MAX_P + 1];      // K(h) = exp(-t/2) sum_k q[k] t^k, t = 2 c h
  double s[GPMP_MAX_P + 1];      // (dK/dh)/h = (2c)^2 exp(-t/2) sum_{k>=1} s[k] t^(k-1)   (p >= 1)
};


__device__ __forceinline__ double matern_eval(const MaternSpec& ms, double h) {
  // maternp_kernel, gpmp/kernel/matern.py:54-64 (Horner form of the same polynomial).
  const double t = 2.0 * ms.c * h;
  double poly = ms.q[ms.p];
  for (int k = ms.p - 1; k >= 0; --k) poly = poly * t + ms.q[k];
  return exp(-ms.c * h) * poly;
}

template <int P>
__device__ __forceinline__ double matern_eval_p(const MaternSpec& ms, double h) {
  const double t = 2.0 * ms.c * h;
  double poly = ms.q[P];
#pragma unroll
  for (int k = P - 1; k >= 0; --k) poly = poly * t + ms.q[k];
  return exp(-ms.c * h) * poly;
}

__device__ __forceinline__ double matern_dispatch(const MaternSpec& ms, double h) {
  switch (ms.p) {
    case 0: return matern_eval_p<0>(ms, h);
    case 1: return matern_eval_p<1>(ms, h);
    case 2: return matern_eval_p<2>(ms, h);
    case 3: return matern_eval_p<3>(ms, h);
    case 4: return matern_eval_p<4>(ms, h);
    default: return matern_eval(ms, h);
  }
}

// ---- fp64 helpers tuned for this kernel (VALU-bound: every instruction per entry counts) ---------------------------
// All constants below travel in the kernel-argument struct: they are then loaded once into SGPRs and used as the
// scalar operand of v_fma_f64.  As C++ literals the compiler re-materialised them into VGPRs next to every use
// (22 v_mov per entry in the previous version of this kernel: a quarter of its VALU work).
struct FastExp {
  double nl2e_half;        // -log2(e) / 2
  double ln2x2_hi, ln2x2_lo;  // 2 ln 2 split so that k * hi is exact for |k| < 2^20
  double c[13];            // c[j] = 1 / (2^j j!)  -- exp(r/2) = sum_j c[j] r^j
  double tiny;             // 1e-280, added to the rsq argument (a no-op for every normal a, keeps a == 0 finite)
};

// Per entry (inlined in the kernel, four entries in lock step):
//  * sqrt(a), a >= 0: hardware 1/sqrt estimate of a + tiny (a == 0 then gives 0 without a select; NaN / inf still
//    propagate through a), one coupled Newton step, one residual correction;
//  * exp(-t/2), t >= 0: k = rint(t log2(e) / 2), r = 2 k ln2 - t in [-0.694, 0.694], exp(r/2) by a degree-12 Taylor
//    polynomial in r (remainder 0.347^13 / 13! = 1.7e-16), scaled by 2^-k: < 1 ulp of libm on [0, 745], exact 1 at 0.
__device__ __forceinline__ double fast_sqrt_pos(double a, double tiny) {
  const double y0 = __builtin_amdgcn_rsq(a + tiny);
  double g = a * y0, h = 0.5 * y0;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  const double d = fma(-g, g, a);
  return fma(d, h, g);
}
__device__ __forceinline__ double fast_exp_neg_half(const FastExp& fe, double t) {
  const double nk = rint(t * fe.nl2e_half);                 // -k
  double r = fma(-nk, fe.ln2x2_hi, -t);
  r = fma(-nk, fe.ln2x2_lo, r);
  double e = fe.c[12];
#pragma unroll
  for (int j = 11; j >= 0; --j) e = fma(e, r, fe.c[j]);
  const int k = (int)nk;
  return ldexp(e, k < -1100 ? -1100 : k);
}

__device__ __forceinline__ double matern_dk_over_h(const MaternSpec& ms, double h, double& kval) {
  const double t = 2.0 * ms.c * h;
  const double e = exp(-ms.c * h);
  double poly = ms.q[ms.p];
  for (int k = ms.p - 1; k >= 0; --k) poly = poly * t + ms.q[k];
  kval = e * poly;
  if (ms.p == 0) return h > 0.0 ? -ms.c * e / h : 0.0;
  double s = ms.s[ms.p];
  for (int k = ms.p - 1; k >= 1; --k) s = s * t + ms.s[k];
  return (2.0 * ms.c) * (2.0 * ms.c) * e * s;
}

inline void fill_fast_exp(FastExp& fe) {
  fe.nl2e_half = -0.5 * 1.4426950408889634;
  fe.ln2x2_hi = 2.0 * 6.93147180369123816490e-01;
  fe.ln2x2_lo = 2.0 * 1.90821492927058770002e-10;
  fe.tiny = 1e-280;
  double f = 1.0;
  for (int j = 0; j <= 12; ++j) {
    if (j) f *= 2.0 * j;         // 2^j j!  (exact in fp64 up to j = 12: 1.96e12)
    fe.c[j] = 1.0 / f;
  }
}

// ---- host-side helpers -------------------------------------------------------------------------
inline int fill_matern(MaternSpec& ms, int p) {
  if (p < 0 || p > GPMP_MAX_P) return -1;
  ms.p = p;
  ms.c = 2.0 * std::sqrt(p + 0.5);
  for (int k = 0; k <= GPMP_MAX_P; ++k) ms.q[k] = ms.s[k] = 0.0;
  ms.q[0] = 1.0;
  for (int i = 0; i < p; ++i) {  // a_i multiplies t^(p-i), gpmp/kernel/matern.py:59-63
    const double a = std::exp(std::lgamma(p + 1.0) - std::lgamma(2.0 * p + 1.0) + std::lgamma(p + i + 1.0) -
                              std::lgamma(i + 1.0) - std::lgamma(p - i + 1.0));
    ms.q[p - i] = a;
  }
  for (int k = 0; k <= p; ++k) ms.s[k] = (k + 1 <= p ? (k + 1) * ms.q[k + 1] : 0.0) - 0.5 * ms.q[k];
  return 0;
}

// Scale factors scale_k = factor exp(loginvrho_k) (factor 2 c: the variable t = 2 c h of the Matern polynomial; 1: plain 1 / rho_k).
inline void fill_scales(double* out, const double* loginvrho, int d, double factor) {
  for (int k = 0; k < d; ++k) out[k] = factor * std::exp(loginvrho[k]);
}

// The covariance parameters on the host, from theta = [log sigma^2, (log noise variance,) log(1 / rho_1) .. log(1 / rho_d)].
struct MaternTheta {
  MaternSpec ms;
  int d, noise;
  double sigma2;
  double noise_var;              // 0 without a noise parameter
  double nugget_scale;           // matern.py:90: without a noise parameter K gains 10 eps sigma2 I; this is 10 eps (else 0) ...
  double nugget;                 // ... and this 10 sigma2 eps
  const double* loginvrho;
  MaternTheta(const double* theta, int noise_param, int p, int dim) : d(dim), noise(noise_param ? 1 : 0) {
    fill_matern(ms, p);
    sigma2 = std::exp(theta[0]);
    noise_var = noise ? std::exp(theta[1]) : 0.0;
    nugget_scale = noise ? 0.0 : 10.0 * DBL_EPSILON;
    nugget = noise ? 0.0 : 10.0 * sigma2 * DBL_EPSILON;
    loginvrho = theta + (noise ? 2 : 1);
  }
  // per-dimension factors: 2 c / rho_k (two_c) or 1 / rho_k
  void scales(double* out, bool two_c) const { fill_scales(out, loginvrho, d, two_c ? 2.0 * ms.c : 1.0); }
  std::vector<double>* scale_vector(bool two_c) const {
    auto* v = new std::vector<double>((size_t)d);
    scales(v->data(), two_c);
    return v;
  }
  // sigma^2 q_k: K(h) = exp(-t/2) sum_k (sigma^2 q_k) t^k
  void coefficients(double* q) const {
    for (int k = 0; k <= GPMP_MAX_P; ++k) q[k] = sigma2 * ms.q[k];
  }
};

}  // namespace
}  // namespace gpmp
