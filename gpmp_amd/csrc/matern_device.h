// Device helpers shared by the Gram / gradient kernels of gram.hip (d <= GPMP_MAX_DIM, parameters in the kernel arguments) and
// gram_wide.hip (d up to GPMP_MAX_DIM_WIDE, length scales in device memory): the Matern polynomial, the fp64 sqrt / exp used on
// the hot path, the tail of a Gram tile, and their host-side coefficient tables.  Everything is internal to the translation unit
// that includes it.
#pragma once
#include "common.h"
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

// The tail of one 128 x 64 Gram tile (gram_kernel_v3 and gram_wide_kernel): acc[a][b] holds the scaled squared distance of
// this thread's entry (row0 + 8 ty + a, col0 + {2tx, 2tx+1, 32+2tx, 32+2tx+1}[b]); sqrt, then (MODE 0) the Matern polynomial
// times exp(-t/2), the diagonal term on the diagonal, and the 16-byte stores.  Coefficients come in already loaded: qc[] for a
// compile-time degree P, qk(k) for P < 0; qtop / c12 are the leading coefficients of the two Horner chains (held in VGPRs by
// the caller).
template <int P, int MODE, int NQ, class QK>
__device__ __forceinline__ void gram_tile_finish(const double (&acc)[8][4], const FastExp fe, const double (&qc)[NQ], QK qk,
                                                 double qtop, double c12, int pdeg, double dadd, bool diag_tile, bool full,
                                                 double* __restrict__ out, long ldk, int row0, int col0, int ty, int tx, int pn,
                                                 int pm) {
#pragma unroll
  for (int a = 0; a < 8; ++a, out += ldk) {
    const int row = row0 + ty * 8 + a;
    double v[4];
    // the four entries of a row advance in lock step: every line below is four independent instructions, so one wave
    // keeps the fp64 pipe fed across the ~26-deep dependent chain of an entry (measured with entry-after-entry code:
    // 2.5 waves per SIMD resident, each waiting half of the time, VALU 60 % busy)
#pragma unroll
    for (int b = 0; b < 4; ++b) v[b] = __builtin_amdgcn_rsq(acc[a][b] + fe.tiny);
    double g[4], h[4], r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) { g[b] = acc[a][b] * v[b]; h[b] = 0.5 * v[b]; }
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = fma(-h[b], g[b], 0.5);
#pragma unroll
    for (int b = 0; b < 4; ++b) { g[b] = fma(g[b], r[b], g[b]); h[b] = fma(h[b], r[b], h[b]); }
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = fma(-g[b], g[b], acc[a][b]);
#pragma unroll
    for (int b = 0; b < 4; ++b) g[b] = fma(r[b], h[b], g[b]);          // g = t = 2 c h (mode 0) or h (mode 1)
    if constexpr (MODE == 0) {
      double nk[4], e[4], poly[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) nk[b] = rint(g[b] * fe.nl2e_half);   // -k
#pragma unroll
      for (int b = 0; b < 4; ++b) r[b] = fma(-nk[b], fe.ln2x2_hi, -g[b]);
#pragma unroll
      for (int b = 0; b < 4; ++b) r[b] = fma(-nk[b], fe.ln2x2_lo, r[b]);
#pragma unroll
      for (int b = 0; b < 4; ++b) { e[b] = c12; poly[b] = qtop; }
      if constexpr (P >= 0) {
#pragma unroll
        for (int k = P - 1; k >= 0; --k)
#pragma unroll
          for (int b = 0; b < 4; ++b) poly[b] = fma(poly[b], g[b], qc[k]);
      } else {
        for (int k = pdeg - 1; k >= 0; --k) {
          const double qkv = qk(k);
#pragma unroll
          for (int b = 0; b < 4; ++b) poly[b] = fma(poly[b], g[b], qkv);
        }
      }
#pragma unroll
      for (int j = 11; j >= 0; --j)
#pragma unroll
        for (int b = 0; b < 4; ++b) e[b] = fma(e[b], r[b], fe.c[j]);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int k = (int)nk[b];                                        // saturating v_cvt_i32_f64
        v[b] = ldexp(e[b], k < -1100 ? -1100 : k) * poly[b];             // exp underflows to 0 well before 2^-1100
      }
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) v[b] = g[b];
    }
    if (diag_tile) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (row == col0 + (b >> 1) * 32 + 2 * tx + (b & 1)) v[b] += dadd;
    }
    if (full) {
      *reinterpret_cast<d2*>(out) = (d2){v[0], v[1]};
      *reinterpret_cast<d2*>(out + 32) = (d2){v[2], v[3]};
    } else if (row < pn) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int cc = (b >> 1) * 32 + 2 * tx + (b & 1);
        if (col0 + cc < pm) out[cc - 2 * tx] = v[b];
      }
    }
  }
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

}  // namespace

// ---- the wide-dimension route (gram_wide.hip): GPMP_MAX_DIM < d <= GPMP_MAX_DIM_WIDE ----------------------------------------
// The entry points of gram.hip check their arguments, compute the per-dimension factors on the host and hand them over here
// (ownership of the vector passes to the callee, which stages it into device memory in stream order: every call only enqueues).
//   gram_wide:       mode 0: K = Matern(t), t^2 = sum (scale_j (x_ij - y_kj))^2, scale_j = 2 c / rho_j, q = sigma^2 q_k; mode 1: the
//                    scaled distance (scale_j = 1 / rho_j)
//   pairwise_wide:   out[i] = sigma2 Matern(|| invrho (x_i - y_i) ||)
//   gram_deriv_wide: gpmp_matern_gram_deriv (kind 0: d / d log sigma^2, 1: noise, 2: length scale jdim)
//   grad_trace_wide: gpmp_matern_grad_trace (cross == 0) / gpmp_matern_grad_trace_cross; scale_j = 2 c / rho_j
int gram_wide(const double* x, const double* y, int n, int m, int d, int mode, int p, std::vector<double>* scale, const double* q,
              double diag_add, int lower_only, double* K, long ldk, hipStream_t st);
int pairwise_wide(const double* x, const double* y, int n, int d, int p, double sigma2, std::vector<double>* invrho, double* out,
                  hipStream_t st);
int gram_deriv_wide(const double* x, int n, int d, int p, int kind, int jdim, double sigma2, double diag_val,
                    std::vector<double>* invrho, double* out, long ld, hipStream_t st);
int grad_trace_wide(const double* M, long ldm, const double* x, int n, const double* y, int m, int d, int p, double sigma2, int noise,
                    double noise_var, std::vector<double>* scale, const double* F, const double* G, int r, long ldf, double* g_dev,
                    double* ws, int cross, hipStream_t st);
size_t grad_wide_ws_elems(int n, int d);

}  // namespace gpmp
