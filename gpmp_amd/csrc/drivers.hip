// Fused drivers behind the C ABI: one call = the whole device-side sequence, for hosts that are not Python (or the
// reference's own backend module), which bind one symbol instead of re-assembling the sequence.  They only enqueue the same
// kernels the Python layer (gpmp_amd/core) launches -- Gram build, blocked Cholesky, triangular solves, column reductions --
// plus small kernels that combine device results; results and info stay on the device.
// Zero mean:
//   negative_log_likelihood_zero_mean  (gpmp/core/likelihood.py:18-52)
//   kriging_predictor_with_zero_mean + _compute_posterior_variance (gpmp/core/kriging.py:35-67,170-199)
// Linear-predictor mean: REML value, ML / REML value + analytic gradient, leave-one-out, universal kriging and its gradient
// with respect to the prediction points, and the weights of the fitted posterior mean (gpmp_posterior_weights; its matrix-free
// evaluation is posterior_mean.hip):
//   negative_log_restricted_likelihood        gpmp/core/likelihood.py:92-129   (contrasts W = Q[:, q:], G = W^T K W)
//   its gradient w.r.t. the covariance parameters  (reference: torch autograd, gpmp/num/torch_backend.py:574-604;
//                                              criterion wrapper gpmp/kernel/parameter_selection.py:35-124)
//   _loo_with_zero_mean / _loo_with_linear_predictor_mean_cpd    gpmp/core/loo.py:65-83,103-130
// The n x n complete QR and the two n^3 products of the reference are replaced by the exact identities
//   W (W^T K W)^-1 W^T = K^-1 - U S^-1 U^T =: Qinv,   U = K^-1 P,  S = P^T K^-1 P
//   ln|W^T K W| = ln|K| + ln|S| - ln|P^T P|
// (DESIGN.md section 2); the q x q algebra (Cholesky of S and P^T P, S^-1, S^-1 b) runs in one small workgroup on the
// device, so no driver ever waits for the host.  The mean design P = mean(xi) (n x q, row-major) is passed in: mean
// functions are user callables in the reference (gpmp/core/model.py:30-52).
// The host side of the eight drivers is built from the shared steps below the kernels: one workspace layout, the covariance
// setup, factor_and_whiten, predict_solve, launch_meanspace, solve_back, launch_reml_finalize.
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int QMAX = GPMP_MAX_RANK - 1;   // mean-design columns: W = L^-1 [z, P] has 1 + q <= GPMP_MAX_RANK columns
constexpr int QLD = QMAX + 1;

// small[] layout (doubles): [0] ln|S|  [1] ln|P^T P|  [2] quad = z^T Qinv z  [3] z^T K^-1 z   [16 + a] c_a = (S^-1 b)_a
constexpr int SM_LDS = 0, SM_LDP = 1, SM_QUAD = 2, SM_ZKZ = 3, SM_C = 16, SM_TOTAL = 16 + QLD + 8;

// Y[i] = [z_i, P_i1 .. P_iq]
__global__ void pack_zp_kernel(const double* __restrict__ z, const double* __restrict__ P, long ldp, int n, int q,
                               double* __restrict__ Y, long ldy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Y[(long)i * ldy] = z[i];
  for (int a = 0; a < q; ++a) Y[(long)i * ldy + 1 + a] = P[(long)i * ldp + a];
}

// In-LDS Cholesky A = R R^T (lower, in place) of a q x q matrix by one workgroup; returns the first failing pivot (1-based) or 0.
// A pivot that is not above q * eps * (its original diagonal entry) counts as a failure: the matrix is singular to working
// precision (a rank-deficient mean design leaves a pivot of rounding-error size, of either sign).
__device__ int chol_lds(double (*A)[QLD + 1], int q, int* fail, double* d0) {
  const int t = threadIdx.x, nt = blockDim.x;
  for (int k = t; k < q; k += nt) d0[k] = A[k][k];
  for (int k = 0; k < q; ++k) {
    __syncthreads();
    if (t == 0) {
      const double dkk = A[k][k];
      if (!(dkk > (double)q * 2.220446049250313e-16 * d0[k])) { if (*fail == 0) *fail = k + 1; A[k][k] = 1.0; } else A[k][k] = sqrt(dkk);
    }
    __syncthreads();
    const double piv = A[k][k];
    for (int i = k + 1 + t; i < q; i += nt) A[i][k] /= piv;
    __syncthreads();
    const int rem = q - k - 1;
    for (int idx = t; idx < rem * rem; idx += nt) {
      const int i = k + 1 + idx / rem, j = k + 1 + idx % rem;
      if (j <= i) A[i][j] -= A[i][k] * A[j][k];
    }
  }
  __syncthreads();
  return *fail;
}

// One workgroup.  Gm: (1 + q) x (1 + q) Gram matrix of W = L^-1 [z, P] (row k, column j at Gm[k * ldg + j]);
// PtP: q x q.  Writes small[] (see above) and Sinv (q x q, ld = lds); a non-positive pivot of S or P^T P sets
// *info = n + pivot (LAPACK-style continuation of the potrf numbering) if *info was 0.
__global__ void __launch_bounds__(256) meanspace_kernel(const double* __restrict__ Gm, long ldg, const double* __restrict__ PtP,
                                                        long ldp, int q, int n, double* __restrict__ small,
                                                        double* __restrict__ Sinv, long lds, int* info) {
  extern __shared__ __attribute__((aligned(16))) double ms_lds[];   // 2 (q x q) images + b + c: 84 KB, above the static limit
  double (*A)[QLD + 1] = reinterpret_cast<double (*)[QLD + 1]>(ms_lds);
  double (*R)[QLD + 1] = reinterpret_cast<double (*)[QLD + 1]>(ms_lds + QLD * (QLD + 1));     // R^-1 (lower)
  double* b = ms_lds + 2 * QLD * (QLD + 1);
  double* c = b + QLD;
  double* d0 = c + QLD;
  __shared__ int fail;
  const int t = threadIdx.x, nt = blockDim.x;
  if (t == 0) fail = 0;
  // ---- ln |P^T P|
  for (int idx = t; idx < q * q; idx += nt) {
    const int i = idx / q, j = idx % q;
    A[i][j] = 0.5 * (PtP[(long)i * ldp + j] + PtP[(long)j * ldp + i]);
  }
  __syncthreads();
  chol_lds(A, q, &fail, d0);
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < q; ++k) s += log(A[k][k]);
    small[SM_LDP] = 2.0 * s;
  }
  __syncthreads();
  // ---- S = sym(Gm[1:, 1:]), b = Gm[1:, 0]
  for (int idx = t; idx < q * q; idx += nt) {
    const int i = idx / q, j = idx % q;
    A[i][j] = 0.5 * (Gm[(long)(1 + i) * ldg + 1 + j] + Gm[(long)(1 + j) * ldg + 1 + i]);
  }
  for (int i = t; i < q; i += nt) b[i] = Gm[(long)(1 + i) * ldg];
  __syncthreads();
  chol_lds(A, q, &fail, d0);
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < q; ++k) s += log(A[k][k]);
    small[SM_LDS] = 2.0 * s;
    small[SM_ZKZ] = Gm[0];
  }
  // ---- R^-1: column j by forward substitution (thread j)
  for (int j = t; j < q; j += nt) {
    for (int i = 0; i < q; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int l = j; l < i; ++l) s -= A[i][l] * R[l][j];
      R[i][j] = (i < j) ? 0.0 : s / A[i][i];
    }
  }
  __syncthreads();
  // ---- S^-1 = R^-T R^-1
  for (int idx = t; idx < q * q; idx += nt) {
    const int i = idx / q, j = idx % q;
    double s = 0.0;
    for (int l = (i > j ? i : j); l < q; ++l) s += R[l][i] * R[l][j];
    Sinv[(long)i * lds + j] = s;
    A[i][j] = s;
  }
  __syncthreads();
  for (int i = t; i < q; i += nt) {
    double s = 0.0;
    for (int j = 0; j < q; ++j) s += A[i][j] * b[j];
    c[i] = s;
    small[SM_C + i] = s;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < q; ++i) s += b[i] * c[i];
    small[SM_QUAD] = Gm[0] - s;
    if (fail != 0) atomicCAS(info, 0, n + fail);
  }
}

// value = 1/2 ((n - q) ln 2 pi + ln|K| + ln|S| - ln|P^T P| + quad); +inf when anything failed (likelihood.py:123-124)
__global__ void reml_finalize_kernel(const double* logdetK, const double* small, const double* ssq, int q, int n, const int* info,
                                     double* out) {
  double v;
  if (q > 0) v = 0.5 * ((double)(n - q) * 1.8378770664093454835606594728112 + *logdetK + small[SM_LDS] - small[SM_LDP] + small[SM_QUAD]);
  else v = 0.5 * ((double)n * 1.8378770664093454835606594728112 + *logdetK + *ssq);
  if (*info != 0 || !(v == v) || v > DBL_MAX || v < -DBL_MAX) v = __builtin_huge_val();
  *out = v;
}

// Row i: U_i = X[i, 1:], alpha_i = X[i, 0];  US_i = U_i S^-1;  beta_i = alpha_i - U_i c.
//   F[i] = [US_i, beta_i],  G[i] = [U_i, beta_i]     (low-rank part of Qinv - beta beta^T for gpmp_matern_grad_trace)
//   loo (dcol != NULL): Qd = dcol_i - US_i . U_i ;  eloo = beta_i / Qd ;  sigma2loo = 1 / Qd ;  zloo = z_i - eloo
__global__ void __launch_bounds__(256) rows_kernel(const double* __restrict__ X, long ldx, const double* __restrict__ Sinv, long lds,
                                                   const double* __restrict__ small, int q, int n, double* __restrict__ F,
                                                   double* __restrict__ G, long ldf, const double* __restrict__ dcol,
                                                   const double* __restrict__ z, const int* __restrict__ info,
                                                   double* __restrict__ zloo, double* __restrict__ s2loo, double* __restrict__ eloo) {
  __shared__ double S[QLD][QLD + 1];
  __shared__ double cs[QLD];
  for (int idx = threadIdx.x; idx < q * q; idx += blockDim.x) S[idx / q][idx % q] = Sinv[(long)(idx / q) * lds + idx % q];
  for (int a = threadIdx.x; a < q; a += blockDim.x) cs[a] = small[SM_C + a];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* xr = X + (long)i * ldx;
  double beta = xr[0], usu = 0.0;
  for (int a = 0; a < q; ++a) beta -= xr[1 + a] * cs[a];
  for (int a = 0; a < q; ++a) {
    double s = 0.0;
    for (int l = 0; l < q; ++l) s += xr[1 + l] * S[l][a];
    usu += s * xr[1 + a];
    if (F != nullptr) { F[(long)i * ldf + a] = s; G[(long)i * ldf + a] = xr[1 + a]; }
  }
  if (F != nullptr) { F[(long)i * ldf + q] = beta; G[(long)i * ldf + q] = beta; }
  if (dcol != nullptr) {
    const double nan = __builtin_nan("");
    const bool bad = *info != 0;
    const double qd = dcol[i] - usu;
    const double e = beta / qd;
    eloo[i] = bad ? nan : e;
    s2loo[i] = bad ? nan : 1.0 / qd;
    zloo[i] = bad ? nan : z[i] - e;
  }
}

// g[j] <- 1/2 g[j] (gpmp_matern_grad_trace returns the plain traces); zeros when the factorisation failed (the
// criterion is +inf there and the selection wrappers return a zero gradient, numpy_backend.py:344-350)
__global__ void grad_finalize2_kernel(double* g, int len, const int* info) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < len) g[j] = (*info != 0) ? 0.0 : 0.5 * g[j];
}

// nll = 1/2 (n ln 2 pi + ln|K| + z^T K^-1 z); +inf when the factorisation failed (the reference's safe_inf
// convention, likelihood.py:47-48) or the value is not finite.
__global__ void nll_finalize_kernel(const double* logdet, const double* quad, const int* info, int n, double* out) {
  double v = 0.5 * ((double)n * 1.8378770664093454835606594728112 + *logdet + *quad);
  if (*info != 0 || !(v == v) || v > DBL_MAX || v < -DBL_MAX) v = __builtin_huge_val();
  *out = v;
}

// zpm[j] = D[0][j];  zpv[j] = sigma2 - D[1][j]  (optionally clamped at 0: Model.predict, core/model.py:290-296)
__global__ void predict_finalize_kernel(const double* D, long ldo, int m, double sigma2, int clamp, const int* info,
                                        double* zpm, double* zpv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const bool bad = *info != 0;
  const double nan = __builtin_nan("");
  double v = sigma2 - D[ldo + j];
  if (clamp && v < 0.0) v = 0.0;
  zpm[j] = bad ? nan : D[j];
  zpv[j] = bad ? nan : v;
}

// ---- prediction with a linear mean (universal kriging, gpmp/core/kriging.py:69-167 restated over the Schur complement) -------
// Per prediction point j, with V = L^-1 K(xi, xt), W = L^-1 [z, P] = [w, Wp], S = Wp^T Wp, c = S^-1 Wp^T w, D = V^T W:
//   r_j = D[1:, j] - Pt[j, :]          (what the Lagrange multipliers mu_j = S^-1 r_j have to absorb)
//   mean_j = D[0, j] - c . r_j,        var_j = sigma^2 - (colsumsq(V)_j - r_j^T S^-1 r_j)
__global__ void __launch_bounds__(256) predict_mean_finalize_kernel(const double* __restrict__ D, long ldd, const double* __restrict__ Pt,
                                                                    long ldpt, int m, int q, const double* __restrict__ Sinv, long lds,
                                                                    const double* __restrict__ small, double sigma2, int clamp,
                                                                    const int* info, double* __restrict__ zpm, double* __restrict__ zpv) {
  extern __shared__ double pm_lds[];           // Sinv (q x q) | c (q)
  double* Si = pm_lds;
  double* cs = pm_lds + (size_t)q * q;
  for (int idx = threadIdx.x; idx < q * q; idx += blockDim.x) Si[idx] = Sinv[(long)(idx / q) * lds + idx % q];
  for (int a = threadIdx.x; a < q; a += blockDim.x) cs[a] = small[SM_C + a];
  __syncthreads();
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  double mean = D[j], quad = 0.0;
  for (int a = 0; a < q; ++a) {
    const double ra = D[(long)(1 + a) * ldd + j] - Pt[(long)j * ldpt + a];
    mean -= cs[a] * ra;
    double ta = 0.0;
    for (int b = 0; b < q; ++b) ta += Si[a * q + b] * (D[(long)(1 + b) * ldd + j] - Pt[(long)j * ldpt + b]);
    quad += ra * ta;
  }
  double v = sigma2 - (D[(long)(1 + q) * ldd + j] - quad);
  if (clamp && v < 0.0) v = 0.0;
  const bool bad = *info != 0;
  const double nan = __builtin_nan("");
  zpm[j] = bad ? nan : mean;
  zpv[j] = bad ? nan : v;
}

// ---- gradient of the prediction with respect to the prediction points (gpmp_predict_grad) --------------------------------
// Per point t, as predict_mean_finalize_kernel, plus mu_t = S^-1 r_t (q x m, ld ldmu) and the unclamped variance (q = 0: no r).
__global__ void __launch_bounds__(256) pgrad_point_kernel(const double* __restrict__ D, long ldd, const double* __restrict__ Pt,
                                                          long ldpt, int m, int q, const double* __restrict__ Sinv, long lds,
                                                          const double* __restrict__ small, double sigma2, int clamp, const int* info,
                                                          double* __restrict__ zpm, double* __restrict__ zpv, double* __restrict__ vraw,
                                                          double* __restrict__ mu, long ldmu) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  double mean = D[j], quad = 0.0;
  for (int a = 0; a < q; ++a) {
    double ta = 0.0;
    for (int b = 0; b < q; ++b) ta += Sinv[(long)a * lds + b] * (D[(long)(1 + b) * ldd + j] - Pt[(long)j * ldpt + b]);
    const double ra = D[(long)(1 + a) * ldd + j] - Pt[(long)j * ldpt + a];
    mean -= small[SM_C + a] * ra;
    quad += ra * ta;
    mu[(long)a * ldmu + j] = ta;
  }
  const double v = sigma2 - (D[(long)(1 + q) * ldd + j] - quad);
  vraw[j] = v;
  const bool bad = *info != 0;
  const double nan = __builtin_nan("");
  zpm[j] = bad ? nan : mean;
  zpv[j] = bad ? nan : ((clamp && v < 0.0) ? 0.0 : v);
}

// y_i = w_i - Wp_i . beta   (beta = S^-1 Wp^T w = small[SM_C]); K^-1 y is the weight vector of the mean gradient
__global__ void pgrad_gamma_kernel(const double* __restrict__ W, long ldw, int n, int q, const double* __restrict__ small,
                                   double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = W[(long)i * ldw];
  for (int a = 0; a < q; ++a) v -= W[(long)i * ldw + 1 + a] * small[SM_C + a];
  y[i] = v;
}

// gm[t][j] += beta . J[t][:, j];   gv[t][j] = -2 gv[t][j] - 2 mu_t . J[t][:, j]  (0 where the variance was clamped); NaN on failure
__global__ void pgrad_finalize_kernel(double* __restrict__ gm, double* __restrict__ gv, const double* __restrict__ J, int m, int d, int q,
                                      const double* __restrict__ small, const double* __restrict__ mu, long ldmu,
                                      const double* __restrict__ vraw, int clamp, const int* info) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)m * d) return;
  const int t = (int)(idx / d), j = (int)(idx - (long)t * d);
  const bool bad = *info != 0;
  const double nan = __builtin_nan("");
  double g = gm[idx];
  for (int a = 0; a < q; ++a) g += small[SM_C + a] * J[((long)t * q + a) * d + j];
  gm[idx] = bad ? nan : g;
  if (gv != nullptr) {
    double h = -2.0 * gv[idx];
    for (int a = 0; a < q; ++a) h -= 2.0 * mu[(long)a * ldmu + t] * J[((long)t * q + a) * d + j];
    if (clamp && vraw[t] < 0.0) h = 0.0;
    gv[idx] = bad ? nan : h;
  }
}

// alpha <- NaN and beta <- NaN when the factorisation failed, else beta = small[SM_C] (gpmp_posterior_weights)
__global__ void weights_finalize_kernel(double* __restrict__ alpha, int n, double* __restrict__ beta, int q,
                                        const double* __restrict__ small, const int* info) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = *info != 0;
  const double nan = __builtin_nan("");
  if (i < n && bad) alpha[i] = nan;
  if (i < q) beta[i] = bad ? nan : small[SM_C + i];
}

// ---- host side: the steps the drivers share --------------------------------------------------------------------------------

// One workspace layout for all eight drivers.  K, dinv and cd are always there; an entry point names the other groups it uses
// and nothing else is reserved.  The order of the slots is fixed (K at offset 0: it holds L on return).
enum : unsigned {
  WS_T = 1u << 0,       // T: L^-1 (gradient, LOO)
  WS_W = 1u << 1,       // W = L^-1 [z, P] as its own n x (1 + q) block (the prediction drivers keep it behind the columns of Kit)
  WS_X = 1u << 2,       // X = L^-T W
  WS_FG = 1u << 3,      // F, G: low-rank rows of the gradient trace, and its workspace gws
  WS_KIT = 1u << 4,     // Kit = [K(xi, xt) | z | P | parity column] and D = [V^T W; colsumsq(V)]
  WS_MEAN = 1u << 5,    // Gm, PtP, Sinv, small: the mean-space algebra
  WS_SCAL = 1u << 6,    // scal: [0] log-det, [1] quadratic form
  WS_DCOL = 1u << 7,    // dcol: diag(K^-1) (LOO); cd then serves n columns
  WS_PGRAD = 1u << 8,   // y, vraw, mu, red: gradient of the prediction
};
struct DriverLayout {
  long ldn, ldm, ldq;
  size_t K, dinv, T, W, X, F, G, Kit, Gm, PtP, Sinv, small, scal, D, dcol, cd, y, vraw, mu, red, gws, sws, sws_elems, total;
};
// m = 0 for the drivers without prediction points
DriverLayout driver_layout(int n, int m, int d, int q, unsigned use) {
  DriverLayout l = {};
  l.ldn = pad16(n);
  l.ldm = pad16(m + 2 + q);          // K(xi, xt) | z | P | (a zero column when that keeps the column count even)
  l.ldq = pad16(1 + q);
  const size_t nq = (size_t)n * l.ldq, q1 = (size_t)(q > 0 ? q : 1);
  WsCursor c;
  l.K = c.take((size_t)n * l.ldn);
  l.dinv = c.take(gpmp_dinv_elems(n));
  if (use & WS_T) l.T = c.take((size_t)n * l.ldn);
  if (use & WS_W) l.W = c.take(nq);
  if (use & WS_X) l.X = c.take(nq);
  if (use & WS_FG) { l.F = c.take(nq); l.G = c.take(nq); }
  if (use & WS_KIT) l.Kit = c.take((size_t)n * l.ldm);
  if (use & WS_MEAN) {
    l.Gm = c.take((size_t)(2 + q) * l.ldq);     // rows k <= q: W^T W; row 1 + q: column sums of squares
    l.PtP = c.take((size_t)(1 + q) * l.ldq);
    l.Sinv = c.take(q1 * l.ldq);
    l.small = c.take(SM_TOTAL);
  }
  if (use & WS_SCAL) l.scal = c.take(16);
  if (use & WS_KIT) l.D = c.take((size_t)(2 + q) * l.ldm);
  if (use & WS_DCOL) l.dcol = c.take((size_t)n);
  const size_t cd_cols = (use & WS_DCOL) ? (size_t)n : (size_t)(m > 1 + q ? m : 1 + q);
  l.cd = c.take(cd_cols * (size_t)gpmp_coldots_ws_rows(n));
  if (use & WS_PGRAD) {
    l.y = c.take((size_t)n);
    l.vraw = c.take((size_t)m);
    l.mu = c.take(q1 * l.ldm);
    l.red = c.take(gpmp_predict_grad_reduce_ws_elems(n, m, d));
  }
  if (use & WS_FG) l.gws = c.take(gpmp_grad_ws_elems(n, d));
  // last, so that every other slot stays where it was: the Strassen scratch of the prediction solve's large updates (nothing below
  // the thresholds, see gpmp_strassen_ws_elems), sized for the solve's m + 1 + q columns rounded up to even
  if (use & WS_KIT) {
    l.sws_elems = gpmp_strassen_ws_elems(n, (m + 1 + q) + ((m + 1 + q) & 1));
    l.sws = c.take(l.sws_elems);
  }
  l.total = c.at;
  return l;
}
constexpr unsigned USE_NLL = WS_W | WS_SCAL;
constexpr unsigned USE_REML = WS_W | WS_MEAN | WS_SCAL;
constexpr unsigned USE_NLL_GRAD = USE_REML | WS_T | WS_X | WS_FG;
constexpr unsigned USE_LOO = USE_REML | WS_T | WS_X | WS_DCOL;
constexpr unsigned USE_PREDICT = WS_KIT;
constexpr unsigned USE_PREDICT_MEAN = WS_KIT | WS_MEAN;
constexpr unsigned USE_PREDICT_GRAD = WS_KIT | WS_MEAN | WS_PGRAD;
constexpr unsigned USE_WEIGHTS = WS_W | WS_MEAN | WS_SCAL;     // the weights land in the caller's vectors: no X, no y slot

// The covariance as the drivers hand it on.  Built only after the argument checks have passed theta_host.
struct Cov {
  const double* theta;
  int d, p, noise;
  double sigma2, diag;               // diag: what the Gram of K gains on its diagonal -- noise variance, or the nugget (matern.py:90)
  Cov(const double* theta_host, int d_, int p_, int noise_) : theta(theta_host), d(d_), p(p_), noise(noise_) {
    const MaternTheta th(theta_host, noise_, p_, d_);
    sigma2 = th.sigma2;
    diag = noise_ ? th.noise_var : th.nugget;
  }
};

int check_common(const double* x, const double* z, const double* P, long ldp, int n, int d, int q, const double* theta_host,
                 const double* ws, const int* info_dev) {
  GPMP_ARG(x != nullptr, 1, "x is NULL");
  GPMP_ARG(z != nullptr, 2, "z is NULL");
  GPMP_ARG(q >= 0 && q <= QMAX, 7, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(q == 0 || (P != nullptr && ldp >= q), 3, "P is NULL or ldp < q");
  GPMP_ARG(n > q && n <= GPMP_MAX_EXTENT, 5, "n <= q or above GPMP_MAX_EXTENT");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 6, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(theta_host != nullptr, 9, "theta is NULL");
  GPMP_ARG(ws != nullptr, 11, "ws is NULL");
  GPMP_ARG(info_dev != nullptr, 13, "info_dev is NULL");
  return 0;
}

// Y = [z | P] (n rows, leading dimension ldy); q = 0: z alone, P may be NULL
int stage_zp(const double* z, const double* P, long ldp, int n, int q, double* Y, long ldy, hipStream_t st) {
  hipLaunchKernelGGL(pack_zp_kernel, dim3((n + 255) / 256), dim3(256), 0, st, z, P, ldp, n, q, Y, ldy);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

// Gram (lower) -> Cholesky -> W = L^-1 [z, P] -> ln|K|.  Leaves L in ws + l.K, W in ws + l.W, ln|K| in ws + l.scal.
int factor_and_whiten(const Cov& cov, const DriverLayout& l, const double* x, const double* z, const double* P, long ldp, int n,
                      int q, double* ws, int* info_dev, gpmp_stream_t stream) {
  double* K = ws + l.K;
  double* dinv = ws + l.dinv;
  double* W = ws + l.W;
  int rc = gpmp_matern_gram(x, nullptr, n, n, cov.d, cov.p, cov.theta, cov.noise, cov.diag, 1, K, l.ldn, stream);
  if (rc) return rc;
  rc = gpmp_potrf_lower_async(K, n, l.ldn, dinv, info_dev, stream);
  if (rc) return rc;
  rc = stage_zp(z, P, ldp, n, q, W, l.ldq, as_stream(stream));
  if (rc) return rc;
  rc = gpmp_trsm_lower(K, n, l.ldn, dinv, W, 1 + q, l.ldq, 0, nullptr, stream);
  if (rc) return rc;
  return gpmp_logdet_chol(K, n, l.ldn, ws + l.scal, stream);
}

// Gram of W = L^-1 [z, P] (n x (1 + q), leading dimension ldw) and, with a mean design, P^T P and the q x q algebra.
int launch_meanspace(const DriverLayout& l, const double* W, long ldw, const double* P, long ldp, int n, int q, double* ws,
                     int* info_dev, gpmp_stream_t stream) {
  int rc = gpmp_coldots(W, n, 1 + q, ldw, W, 1 + q, ldw, ws + l.Gm, l.ldq, ws + l.cd, stream);
  if (rc || q == 0) return rc;
  rc = gpmp_coldots(P, n, q, ldp, P, q, ldp, ws + l.PtP, l.ldq, ws + l.cd, stream);
  if (rc) return rc;
  const size_t ms_bytes = sizeof(double) * (2 * QLD * (QLD + 1) + 3 * QLD);
  static DeviceOnce attr_once;
  if (const long long dev_bit = attr_once.need()) {
    if (dev_bit < 0) { set_error("hipGetDevice failed or device ordinal above 62"); return -1; }
    GPMP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(meanspace_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)ms_bytes));
    attr_once.done(dev_bit);
  }
  hipLaunchKernelGGL(meanspace_kernel, dim3(1), dim3(256), ms_bytes, as_stream(stream), ws + l.Gm, l.ldq, ws + l.PtP, l.ldq, q, n,
                     ws + l.small, ws + l.Sinv, l.ldq, info_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

// The common start of gpmp_reml, gpmp_nll_grad and gpmp_loo
int factor_and_meanspace(const Cov& cov, const DriverLayout& l, const double* x, const double* z, const double* P, long ldp, int n,
                         int q, double* ws, int* info_dev, gpmp_stream_t stream) {
  const int rc = factor_and_whiten(cov, l, x, z, P, ldp, n, q, ws, info_dev, stream);
  return rc ? rc : launch_meanspace(l, ws + l.W, l.ldq, P, ldp, n, q, ws, info_dev, stream);
}

int launch_reml_finalize(const DriverLayout& l, int q, int n, double* ws, const int* info_dev, double* value_dev, hipStream_t st) {
  hipLaunchKernelGGL(reml_finalize_kernel, dim3(1), dim3(1), 0, st, ws + l.scal, ws + l.small, ws + l.Gm + (size_t)(1 + q) * l.ldq,
                     q, n, info_dev, value_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

// X = L^-T W = K^-1 [z, P]
int solve_back(const DriverLayout& l, int n, int q, double* ws, gpmp_stream_t stream) {
  double* X = ws + l.X;
  GPMP_HIP_TRY(hipMemcpyAsync(X, ws + l.W, sizeof(double) * (size_t)n * l.ldq, hipMemcpyDeviceToDevice, as_stream(stream)));
  return gpmp_trsm_lower(ws + l.K, n, l.ldn, ws + l.dinv, X, 1 + q, l.ldq, 1, nullptr, stream);
}

// The common start of the prediction drivers.  [z, P] ride along as 1 + q more right-hand sides: [V | W] =
// L^-1 [K(xi, xt) | z | P] in ONE solve, in place and panel by panel behind the factorisation at chain-bound sizes (the separate
// few-column sweep for W was 0.17 ms of a 5.3 ms prediction at n = 4096 and waited for the end of the factorisation; as columns
// of the solve it is hidden like the rest).  An even column count keeps the LDS-direct GEMM's fast path.
// Leaves L in ws + l.K, V in ws + l.Kit and W behind it, at ws + l.Kit + m (leading dimension ldm for both).
int predict_solve(const Cov& cov, const DriverLayout& l, const double* xi, const double* zi, const double* Pi, long ldpi,
                  const double* xt, int n, int m, int q, double* ws, int* info_dev, gpmp_stream_t stream) {
  hipStream_t st = as_stream(stream);
  double* K = ws + l.K;
  double* Kit = ws + l.Kit;
  int rc = gpmp_matern_gram(xi, nullptr, n, n, cov.d, cov.p, cov.theta, cov.noise, cov.diag, 1, K, l.ldn, stream);
  if (rc) return rc;
  rc = gpmp_matern_gram(xi, xt, n, m, cov.d, cov.p, cov.theta, cov.noise, 0.0, 0, Kit, l.ldm, stream);
  if (rc) return rc;
  rc = stage_zp(zi, Pi, ldpi, n, q, Kit + m, l.ldm, st);
  if (rc) return rc;
  const int mb = (m + 1 + q) + ((m + 1 + q) & 1);
  if (mb > m + 1 + q) GPMP_HIP_TRY(hipMemset2DAsync(Kit + m + 1 + q, (size_t)l.ldm * sizeof(double), 0, sizeof(double), n, st));
  return potrf_trsm_lower_ws(K, n, l.ldn, ws + l.dinv, info_dev, Kit, mb, l.ldm, l.sws_elems ? ws + l.sws : nullptr, l.sws_elems, st);
}
}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_nll_ws_elems(int n) { return n > 0 ? driver_layout(n, 0, 1, 0, USE_NLL).total : 0; }

extern "C" int gpmp_nll_zero_mean(const double* x, const double* z, int n, int d, int p, const double* theta_host,
                                  int noise, double* ws, double* nll_dev, int* info_dev, gpmp_stream_t stream) {
  GPMP_ARG(x != nullptr, 1, "x is NULL");
  GPMP_ARG(z != nullptr, 2, "z is NULL");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 3, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(theta_host != nullptr, 6, "theta is NULL");
  GPMP_ARG(ws != nullptr, 8, "ws is NULL");
  GPMP_ARG(nll_dev != nullptr, 9, "nll_dev is NULL");
  GPMP_ARG(info_dev != nullptr, 10, "info_dev is NULL");
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, 0, d, 0, USE_NLL);
  double* scal = ws + l.scal;
  int rc = factor_and_whiten(cov, l, x, z, nullptr, 0, n, 0, ws, info_dev, stream);      // w = L^-1 z: n x 1, ld 16
  if (rc) return rc;
  rc = gpmp_coldots(ws + l.W, n, 1, l.ldq, nullptr, 0, 1, scal + 1, 1, ws + l.cd, stream);   // sum of squares of the one column
  if (rc) return rc;
  hipLaunchKernelGGL(nll_finalize_kernel, dim3(1), dim3(1), 0, as_stream(stream), scal, scal + 1, info_dev, n, nll_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t gpmp_predict_ws_elems(int n, int m) { return (n > 0 && m > 0) ? driver_layout(n, m, 1, 0, USE_PREDICT).total : 0; }

extern "C" int gpmp_predict_zero_mean(const double* xi, const double* zi, const double* xt, int n, int m, int d, int p,
                                      const double* theta_host, int noise, int zero_neg_variances, double* ws,
                                      double* zpm_dev, double* zpv_dev, int* info_dev, gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(zi != nullptr, 2, "zi is NULL");
  GPMP_ARG(xt != nullptr, 3, "xt is NULL");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 4, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 5, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(theta_host != nullptr, 8, "theta is NULL");
  GPMP_ARG(ws != nullptr, 11, "ws is NULL");
  GPMP_ARG(zpm_dev != nullptr && zpv_dev != nullptr, 12, "output is NULL");
  GPMP_ARG(info_dev != nullptr, 14, "info_dev is NULL");
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, m, d, 0, USE_PREDICT);
  double* Kit = ws + l.Kit;
  double* D = ws + l.D;
  int rc = predict_solve(cov, l, xi, zi, nullptr, 0, xt, n, m, 0, ws, info_dev, stream);
  if (rc) return rc;
  rc = gpmp_coldots(Kit, n, m, l.ldm, Kit + m, 1, l.ldm, D, l.ldm, ws + l.cd, stream);      // V^T w and colsumsq(V)
  if (rc) return rc;
  hipLaunchKernelGGL(predict_finalize_kernel, dim3((m + 255) / 256), dim3(256), 0, as_stream(stream), D, l.ldm, m, cov.sigma2,
                     zero_neg_variances, info_dev, zpm_dev, zpv_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t gpmp_reml_ws_elems(int n, int q) {
  return (n > 0 && q >= 0 && q <= QMAX) ? driver_layout(n, 0, 1, q, USE_REML).total : 0;
}

extern "C" int gpmp_reml(const double* x, const double* z, const double* P, long ldp, int n, int d, int q, int p,
                         const double* theta_host, int noise, double* ws, double* value_dev, int* info_dev,
                         gpmp_stream_t stream) {
  int rc = check_common(x, z, P, ldp, n, d, q, theta_host, ws, info_dev);
  if (rc) return rc;
  GPMP_ARG(value_dev != nullptr, 12, "value_dev is NULL");
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, 0, d, q, USE_REML);
  rc = factor_and_meanspace(cov, l, x, z, P, ldp, n, q, ws, info_dev, stream);
  if (rc) return rc;
  return launch_reml_finalize(l, q, n, ws, info_dev, value_dev, as_stream(stream));
}

extern "C" size_t gpmp_nll_grad_ws_elems(int n, int d, int q) {
  return (n > 0 && q >= 0 && q <= QMAX && d >= 1) ? driver_layout(n, 0, d, q, USE_NLL_GRAD).total : 0;
}

extern "C" int gpmp_nll_grad(const double* x, const double* z, const double* P, long ldp, int n, int d, int q, int p,
                             const double* theta_host, int noise, double* ws, double* value_dev, double* grad_dev,
                             int* info_dev, gpmp_stream_t stream) {
  int rc = check_common(x, z, P, ldp, n, d, q, theta_host, ws, info_dev);
  if (rc) return rc;
  GPMP_ARG(value_dev != nullptr, 12, "value_dev is NULL");
  GPMP_ARG(grad_dev != nullptr, 13, "grad_dev is NULL");
  hipStream_t st = as_stream(stream);
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, 0, d, q, USE_NLL_GRAD);
  rc = factor_and_meanspace(cov, l, x, z, P, ldp, n, q, ws, info_dev, stream);
  if (rc) return rc;
  rc = launch_reml_finalize(l, q, n, ws, info_dev, value_dev, st);
  if (rc) return rc;
  rc = solve_back(l, n, q, ws, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(rows_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ws + l.X, l.ldq, ws + l.Sinv, l.ldq, ws + l.small, q, n,
                     ws + l.F, ws + l.G, l.ldq, (const double*)nullptr, (const double*)nullptr, info_dev, (double*)nullptr,
                     (double*)nullptr, (double*)nullptr);
  GPMP_HIP_TRY(hipGetLastError());
  // K^-1 (lower) = T^T T over the factor's own buffer: L is dead once T and X exist
  double* K = ws + l.K;
  double* T = ws + l.T;
  rc = gpmp_trtri_lower(K, n, l.ldn, ws + l.dinv, T, l.ldn, stream);
  if (rc) return rc;
  rc = gpmp_lauum_lower(T, n, l.ldn, K, l.ldn, stream);
  if (rc) return rc;
  rc = gpmp_matern_grad_trace(K, l.ldn, x, n, d, p, theta_host, noise, ws + l.F, ws + l.G, q + 1, l.ldq, grad_dev, ws + l.gws, stream);
  if (rc) return rc;
  const int glen = 1 + (noise ? 1 : 0) + d;
  hipLaunchKernelGGL(grad_finalize2_kernel, dim3((glen + 127) / 128), dim3(128), 0, st, grad_dev, glen, info_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t gpmp_loo_ws_elems(int n, int q) {
  return (n > 0 && q >= 0 && q <= QMAX) ? driver_layout(n, 0, 1, q, USE_LOO).total : 0;
}

extern "C" int gpmp_loo(const double* x, const double* z, const double* P, long ldp, int n, int d, int q, int p,
                        const double* theta_host, int noise, double* ws, double* zloo_dev, double* sigma2loo_dev,
                        double* eloo_dev, int* info_dev, gpmp_stream_t stream) {
  int rc = check_common(x, z, P, ldp, n, d, q, theta_host, ws, info_dev);
  if (rc) return rc;
  GPMP_ARG(zloo_dev != nullptr && sigma2loo_dev != nullptr && eloo_dev != nullptr, 12, "output is NULL");
  hipStream_t st = as_stream(stream);
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, 0, d, q, USE_LOO);
  rc = factor_and_meanspace(cov, l, x, z, P, ldp, n, q, ws, info_dev, stream);
  if (rc) return rc;
  rc = solve_back(l, n, q, ws, stream);
  if (rc) return rc;
  // diag(K^-1) = column sums of squares of T = L^-1 (gpmp/core/linalg.py:17-46)
  double* T = ws + l.T;
  rc = gpmp_trtri_lower(ws + l.K, n, l.ldn, ws + l.dinv, T, l.ldn, stream);
  if (rc) return rc;
  rc = gpmp_coldots(T, n, n, l.ldn, nullptr, 0, 1, ws + l.dcol, n, ws + l.cd, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(rows_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ws + l.X, l.ldq, ws + l.Sinv, l.ldq, ws + l.small, q, n,
                     (double*)nullptr, (double*)nullptr, l.ldq, ws + l.dcol, z, info_dev, zloo_dev, sigma2loo_dev, eloo_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t gpmp_predict_mean_ws_elems(int n, int m, int q) {
  return (n > 0 && m > 0 && q >= 1 && q <= QMAX) ? driver_layout(n, m, 1, q, USE_PREDICT_MEAN).total : 0;
}

extern "C" int gpmp_predict_mean(const double* xi, const double* zi, const double* Pi, long ldpi, const double* xt, const double* Pt,
                                 long ldpt, int n, int m, int d, int q, int p, const double* theta_host, int noise,
                                 int zero_neg_variances, double* ws, double* zpm_dev, double* zpv_dev, int* info_dev,
                                 gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(zi != nullptr, 2, "zi is NULL");
  GPMP_ARG(q >= 1 && q <= QMAX, 11, "q outside [1, GPMP_MAX_RANK - 1] (q = 0: gpmp_predict_zero_mean)");
  GPMP_ARG(Pi != nullptr && ldpi >= q, 3, "Pi is NULL or ldpi < q");
  GPMP_ARG(xt != nullptr, 5, "xt is NULL");
  GPMP_ARG(Pt != nullptr && ldpt >= q, 6, "Pt is NULL or ldpt < q");
  GPMP_ARG(n > q && n <= GPMP_MAX_EXTENT, 8, "n <= q or above GPMP_MAX_EXTENT");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 9, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 10, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(theta_host != nullptr, 13, "theta is NULL");
  GPMP_ARG(ws != nullptr, 16, "ws is NULL");
  GPMP_ARG(zpm_dev != nullptr && zpv_dev != nullptr, 17, "output is NULL");
  GPMP_ARG(info_dev != nullptr, 19, "info_dev is NULL");
  hipStream_t st = as_stream(stream);
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, m, d, q, USE_PREDICT_MEAN);
  double* Kit = ws + l.Kit;
  double* W = Kit + m;
  const long ldw = l.ldm;
  int rc = predict_solve(cov, l, xi, zi, Pi, ldpi, xt, n, m, q, ws, info_dev, stream);
  if (rc) return rc;
  rc = launch_meanspace(l, W, ldw, Pi, ldpi, n, q, ws, info_dev, stream);
  if (rc) return rc;
  rc = gpmp_coldots(Kit, n, m, l.ldm, W, 1 + q, ldw, ws + l.D, l.ldm, ws + l.cd, stream);         // V^T [w, Wp] and colsumsq(V)
  if (rc) return rc;
  const size_t fin_bytes = sizeof(double) * ((size_t)q * q + q);
  static DeviceOnce attr_once;
  if (const long long dev_bit = attr_once.need()) {
    if (dev_bit < 0) { set_error("hipGetDevice failed or device ordinal above 62"); return -1; }
    GPMP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(predict_mean_finalize_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * ((size_t)QMAX * QMAX + QMAX))));
    attr_once.done(dev_bit);
  }
  hipLaunchKernelGGL(predict_mean_finalize_kernel, dim3((m + 255) / 256), dim3(256), fin_bytes, st, ws + l.D, l.ldm, Pt, ldpt, m, q,
                     ws + l.Sinv, l.ldq, ws + l.small, cov.sigma2, zero_neg_variances, info_dev, zpm_dev, zpv_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t gpmp_predict_grad_ws_elems(int n, int m, int d, int q) {
  if (n < 1 || n > GPMP_MAX_EXTENT || m < 1 || m > GPMP_MAX_EXTENT || d < 1 || d > GPMP_MAX_DIM_WIDE || q < 0 || q > QMAX) return 0;
  return driver_layout(n, m, d, q, USE_PREDICT_GRAD).total;
}

extern "C" int gpmp_predict_grad(const double* xi, const double* zi, const double* Pi, long ldpi, const double* xt, const double* Pt,
                                 long ldpt, const double* J, int n, int m, int d, int q, int p, const double* theta_host, int noise,
                                 int zero_neg_variances, int with_variance_gradient, double* ws, double* zpm_dev, double* zpv_dev,
                                 double* gzpm_dev, double* gzpv_dev, int* info_dev, gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(zi != nullptr, 2, "zi is NULL");
  GPMP_ARG(q >= 0 && q <= QMAX, 12, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(q == 0 || (Pi != nullptr && ldpi >= q), 3, "Pi is NULL or ldpi < q");
  GPMP_ARG(xt != nullptr, 5, "xt is NULL");
  GPMP_ARG(q == 0 || (Pt != nullptr && ldpt >= q), 6, "Pt is NULL or ldpt < q");
  GPMP_ARG(q == 0 || J != nullptr, 8, "J is NULL with q > 0");
  GPMP_ARG(n > q && n <= GPMP_MAX_EXTENT, 9, "n <= q or above GPMP_MAX_EXTENT");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 10, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 11, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 13, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(theta_host != nullptr, 14, "theta is NULL");
  GPMP_ARG(ws != nullptr, 18, "ws is NULL");
  GPMP_ARG(zpm_dev != nullptr && zpv_dev != nullptr, 19, "zpm or zpv is NULL");
  GPMP_ARG(gzpm_dev != nullptr, 21, "gzpm is NULL");
  GPMP_ARG(with_variance_gradient == 0 || gzpv_dev != nullptr, 22, "gzpv is NULL with with_variance_gradient != 0");
  GPMP_ARG(info_dev != nullptr, 23, "info_dev is NULL");
  hipStream_t st = as_stream(stream);
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, m, d, q, USE_PREDICT_GRAD);
  double* K = ws + l.K;
  double* dinv = ws + l.dinv;
  double* Kit = ws + l.Kit;
  double* W = Kit + m;
  const long ldw = l.ldm;
  int rc = predict_solve(cov, l, xi, zi, Pi, ldpi, xt, n, m, q, ws, info_dev, stream);
  if (rc) return rc;
  if (q > 0) {
    rc = launch_meanspace(l, W, ldw, Pi, ldpi, n, q, ws, info_dev, stream);
    if (rc) return rc;
  }
  rc = gpmp_coldots(Kit, n, m, l.ldm, W, 1 + q, ldw, ws + l.D, l.ldm, ws + l.cd, stream);         // V^T [w, Wp] and colsumsq(V)
  if (rc) return rc;
  hipLaunchKernelGGL(pgrad_point_kernel, dim3((m + 255) / 256), dim3(256), 0, st, ws + l.D, l.ldm, Pt, ldpt, m, q, ws + l.Sinv, l.ldq,
                     ws + l.small, cov.sigma2, zero_neg_variances, info_dev, zpm_dev, zpv_dev, ws + l.vraw, ws + l.mu, l.ldm);
  GPMP_HIP_TRY(hipGetLastError());
  // mean weights K^-1 (z - P beta) = L^-T (w - Wp beta)
  double* y = ws + l.y;
  hipLaunchKernelGGL(pgrad_gamma_kernel, dim3((n + 255) / 256), dim3(256), 0, st, W, ldw, n, q, ws + l.small, y);
  GPMP_HIP_TRY(hipGetLastError());
  rc = gpmp_trsm_lower(K, n, l.ldn, dinv, y, 1, 1, 1, nullptr, stream);
  if (rc) return rc;
  const double* lam = nullptr;
  if (with_variance_gradient) {
    // kriging weights Lambda = L^-T (V - Wp mu), overwriting V (kriging.py:88-101 restated)
    if (q > 0) {
      rc = gpmp_dgemm(0, 0, n, m, q, -1.0, W + 1, ldw, ws + l.mu, l.ldm, 1.0, Kit, l.ldm, 0, stream);
      if (rc) return rc;
    }
    rc = gpmp_trsm_lower(K, n, l.ldn, dinv, Kit, m, l.ldm, 1, nullptr, stream);
    if (rc) return rc;
    lam = Kit;
  }
  rc = gpmp_predict_grad_reduce(xi, xt, n, m, d, p, theta_host, noise, y, lam, l.ldm, gzpm_dev, with_variance_gradient ? gzpv_dev : nullptr,
                                ws + l.red, stream);
  if (rc) return rc;
  const long md = (long)m * d;
  hipLaunchKernelGGL(pgrad_finalize_kernel, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, st, gzpm_dev,
                     with_variance_gradient ? gzpv_dev : nullptr, J, m, d, q, ws + l.small, ws + l.mu, l.ldm, ws + l.vraw,
                     zero_neg_variances, info_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t gpmp_posterior_weights_ws_elems(int n, int q) {
  return (n > 0 && n <= GPMP_MAX_EXTENT && q >= 0 && q <= QMAX) ? driver_layout(n, 0, 1, q, USE_WEIGHTS).total : 0;
}

extern "C" int gpmp_posterior_weights(const double* xi, const double* zi, const double* Pi, long ldpi, int n, int d, int q, int p,
                                      const double* theta_host, int noise, double* ws, double* alpha_dev, double* beta_dev,
                                      int* info_dev, gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(zi != nullptr, 2, "zi is NULL");
  GPMP_ARG(q >= 0 && q <= QMAX, 7, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(q == 0 || (Pi != nullptr && ldpi >= q), 3, "Pi is NULL or ldpi < q");
  GPMP_ARG(n > q && n <= GPMP_MAX_EXTENT, 5, "n <= q or above GPMP_MAX_EXTENT");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 6, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 8, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(theta_host != nullptr, 9, "theta is NULL");
  GPMP_ARG(ws != nullptr, 11, "ws is NULL");
  GPMP_ARG(alpha_dev != nullptr, 12, "alpha_dev is NULL");
  GPMP_ARG(q == 0 || beta_dev != nullptr, 13, "beta_dev is NULL with q > 0");
  GPMP_ARG(info_dev != nullptr, 14, "info_dev is NULL");
  hipStream_t st = as_stream(stream);
  const Cov cov(theta_host, d, p, noise);
  const DriverLayout l = driver_layout(n, 0, d, q, USE_WEIGHTS);
  int rc = factor_and_whiten(cov, l, xi, zi, Pi, ldpi, n, q, ws, info_dev, stream);
  if (rc) return rc;
  if (q > 0) {
    rc = launch_meanspace(l, ws + l.W, l.ldq, Pi, ldpi, n, q, ws, info_dev, stream);
    if (rc) return rc;
  }
  // alpha = K^-1 (z - P beta) = L^-T (w - Wp beta), beta = S^-1 Wp^T w
  hipLaunchKernelGGL(pgrad_gamma_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ws + l.W, l.ldq, n, q, ws + l.small, alpha_dev);
  GPMP_HIP_TRY(hipGetLastError());
  rc = gpmp_trsm_lower(ws + l.K, n, l.ldn, ws + l.dinv, alpha_dev, 1, 1, 1, nullptr, stream);
  if (rc) return rc;
  const int len = n > q ? n : q;
  hipLaunchKernelGGL(weights_finalize_kernel, dim3((len + 255) / 256), dim3(256), 0, st, alpha_dev, n, beta_dev, q, ws + l.small,
                     info_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}
