// Posterior mean from stored weights, matrix-free: with alpha = K^-1 (z - P beta) and beta from gpmp_posterior_weights,
//   zpm[t]     = sum_i alpha_i sigma^2 K_p(h_it) + Pt[t] . beta
//   gzpm[t][j] = sigma^2 rho_j^-2 sum_i alpha_i S(h_it) (x_tj - x_ij) + sum_a beta_a J[t][a][j],   S(h) = K_p'(h) / h
// in ONE visit of every (i, t) entry: the distance, the square root and the exponential serve the value and the gradient.  No
// n x m block is ever stored and no diagonal term is added (xt are new points).  The gradient term is 0 at h = 0 for every p
// (the limit for p >= 1, the reference's subgradient convention for p = 0, as pg_weight of predict_grad.hip).
//
// Per entry the value repeats the arithmetic of the Gram kernel (gram.hip, gram_kernel_v3) operation for operation -- both points
// scaled by 2 c / rho_j BEFORE the subtraction, the same sqrt / exp / Horner chain over sigma^2 q_k -- so sigma^2 K_p(h_it) is the
// entry gpmp_matern_gram(xi, xt) writes, bit for bit, and zpm differs from G^T alpha only in the order of the sum.  The scaled
// observation points are written once per call by a pre-pass (n d doubles of the workspace) and read wave-uniformly; the
// gradient accumulates the UNSCALED differences x_tj - x_ij (no cancellation between two rounded products).
//
// Layout (predict_grad_kernel's): one wave per (tile of 64 prediction points, slice of the observation points); lane = prediction
// point, x_t and the accumulators (one value, optionally DT gradient components) in registers, x_i and alpha_i read
// wave-uniformly, PM_IB observation points in lock step so that one wave keeps the fp64 pipe fed across the dependent sqrt / exp
// chain.  Slices over i fill the machine when m is small: slice 0 writes the outputs themselves, slices s >= 1 a bounded partial
// buffer in the workspace; the finalize kernel sums the slices in a fixed order and adds the mean part.  No atomics: two runs on
// the same inputs are bit-identical.  1 <= d <= GPMP_MAX_DIM only (the length scales travel in the kernel arguments).
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int PM_TM = 64;                 // prediction points per wave
constexpr int PM_IB = 4;                  // observation points in lock step
constexpr int PM_TARGET_WAVES = 4096;     // 256 CUs x 16 waves
constexpr int PM_MIN_ROWS = 64;           // observation points per slice, at least
constexpr long PM_PART_CAP = 1L << 22;    // doubles of partials (32 MB)

// (never written inside a kernel: one store into the by-value block and the compiler keeps a private copy of it in scratch memory)
struct PmParams {
  const double* xi;              // n x d
  double* sxi;                   // n x d, scaled by 2 c / rho_j (workspace, written by the pre-pass)
  const double* alpha;           // n
  const double* xt;              // m x d
  double* val;                   // slice 0 of the value (zpm, m)
  double* grad;                  // slice 0 of the gradient (gzpm, m x d), or NULL
  double* part;                  // slices 1.. : [slice - 1][m][width], width = 1 (+ d with the gradient): value, then the gradient
  const double* Pt;              // mean part (q > 0)
  const double* beta;
  const double* J;
  long ldpt;
  int n, m, d, q, rows_per_slice, nslices, width;
  double scale[GPMP_MAX_DIM];    // 2 c / rho_j
  double qs[GPMP_MAX_P + 1];     // sigma^2 q_k:  sigma^2 K_p(h) = exp(-t/2) sum_k qs[k] t^k, t = 2 c h
  double ss[GPMP_MAX_P + 1];     // sigma^2 s_k:  sigma^2 S(h) / (2c)^2 = exp(-t/2) sum_{k>=1} ss[k] t^(k-1)   (p >= 1)
  int p;
  FastExp fe;
};

__global__ void pm_scale_points_kernel(PmParams p) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)p.n * p.d) return;
  p.sxi[idx] = p.scale[idx % p.d] * p.xi[idx];
}

template <int DT, bool G>
__global__ void __launch_bounds__(64) posterior_mean_kernel(PmParams p) {
  constexpr int GD = G ? DT : 1;
  const int lane = threadIdx.x;
  const int t = blockIdx.x * PM_TM + lane;
  const int slice = blockIdx.y;
  const int d = p.d, m = p.m, pdeg = p.p;
  const bool valid = t < m;
  const int tc = valid ? t : m - 1;
  const double* __restrict__ xi = p.xi;
  const double* __restrict__ sxi = p.sxi;
  const double* __restrict__ alpha = p.alpha;
  const double* __restrict__ xt = p.xt + (long)tc * d;
  double ys[DT], y[GD], ag[GD];
  {
    // a plain product, as the Gram kernel stages its points: never fused into the subtraction below
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < DT; ++j) ys[j] = j < d ? p.scale[j] * xt[j] : 0.0;
  }
  if constexpr (G) {
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      y[j] = j < d ? xt[j] : 0.0;
      ag[j] = 0.0;
    }
  }
  double av = 0.0;
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  for (int ib = i0; ib < i1; ib += PM_IB) {
    // a short last block repeats the slice's last point with weight 0
    const double* sr[PM_IB];
    const double* xr[PM_IB];
    double a[PM_IB], t2[PM_IB];
#pragma unroll
    for (int b = 0; b < PM_IB; ++b) {
      const int i = min(ib + b, i1 - 1);
      sr[b] = sxi + (long)i * d;
      xr[b] = xi + (long)i * d;
      a[b] = ib + b < i1 ? alpha[i] : 0.0;
      t2[b] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      if (j < d) {
#pragma unroll
        for (int b = 0; b < PM_IB; ++b) {
          const double sd = sr[b][j] - ys[j];
          t2[b] = fma(sd, sd, t2[b]);
        }
      }
    }
    double tt[PM_IB], e[PM_IB], poly[PM_IB];
#pragma unroll
    for (int b = 0; b < PM_IB; ++b) tt[b] = fast_sqrt_pos(t2[b], p.fe.tiny);
#pragma unroll
    for (int b = 0; b < PM_IB; ++b) e[b] = fast_exp_neg_half(p.fe, tt[b]);
    const double qtop = p.qs[pdeg];
#pragma unroll
    for (int b = 0; b < PM_IB; ++b) poly[b] = qtop;
    for (int k = pdeg - 1; k >= 0; --k) {
      const double qk = p.qs[k];
#pragma unroll
      for (int b = 0; b < PM_IB; ++b) poly[b] = fma(poly[b], tt[b], qk);
    }
    double kv[PM_IB];
#pragma unroll
    for (int b = 0; b < PM_IB; ++b) {
      kv[b] = e[b] * poly[b];
      av = fma(a[b], kv[b], av);
    }
    if constexpr (G) {
      double w[PM_IB];
      if (pdeg == 0) {
#pragma unroll
        for (int b = 0; b < PM_IB; ++b) w[b] = tt[b] > 0.0 ? -0.5 * kv[b] / tt[b] : 0.0;
      } else {
        const double stop = p.ss[pdeg];
#pragma unroll
        for (int b = 0; b < PM_IB; ++b) w[b] = stop;
        for (int k = pdeg - 1; k >= 1; --k) {
          const double sk = p.ss[k];
#pragma unroll
          for (int b = 0; b < PM_IB; ++b) w[b] = fma(w[b], tt[b], sk);
        }
#pragma unroll
        for (int b = 0; b < PM_IB; ++b) w[b] *= e[b];
      }
#pragma unroll
      for (int b = 0; b < PM_IB; ++b) w[b] *= a[b];
#pragma unroll
      for (int j = 0; j < DT; ++j) {
        if (j < d) {
#pragma unroll
          for (int b = 0; b < PM_IB; ++b) ag[j] = fma(w[b], y[j] - xr[b][j], ag[j]);
        }
      }
    }
  }
  if (!valid) return;
  if (slice == 0) {
    p.val[t] = av;
    if constexpr (G) {
#pragma unroll
      for (int j = 0; j < DT; ++j)
        if (j < d) p.grad[(long)t * d + j] = ag[j];
    }
  } else {
    double* __restrict__ o = p.part + ((long)(slice - 1) * m + t) * p.width;
    o[0] = av;
    if constexpr (G) {
#pragma unroll
      for (int j = 0; j < DT; ++j)
        if (j < d) o[1 + j] = ag[j];
    }
  }
}

// L lanes per output (consecutive lanes of one wave): column 0 of point t is the value, column 1 + j component j of the gradient.
// Lane l adds the partial slices l, l + L, ... in that order, the lanes are combined by a fixed butterfly, slice 0 is added last;
// then the gradient's factor (2 c / rho_j)^2 and the mean part.  One lane per output would walk up to 4095 dependent loads when m
// is small; the order of the sum depends only on (nslices, L), so two runs agree bit for bit.
template <int L>
__global__ void __launch_bounds__(256) posterior_mean_finalize_kernel(PmParams p) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int w = p.width;
  const long total = (long)p.m * w;
  const int sub = (int)(gid % L);
  const bool live = gid / L < total;
  const long idx = live ? gid / L : total - 1;          // (idle lanes still take part in the butterfly)
  const int t = (int)(idx / w), c = (int)(idx - (long)t * w);
  const int q = p.q;
  const double* __restrict__ part = p.part;
  double s = 0.0;
#pragma unroll 4
  for (int k = sub; k + 1 < p.nslices; k += L) s += part[((long)k * p.m + t) * w + c];
#pragma unroll
  for (int o = L / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (!live || sub != 0) return;
  s += c == 0 ? p.val[t] : p.grad[(long)t * p.d + c - 1];
  if (c == 0) {
    for (int a = 0; a < q; ++a) s = fma(p.Pt[(long)t * p.ldpt + a], p.beta[a], s);
    p.val[t] = s;
  } else {
    const int j = c - 1;
    const double sj = p.scale[j];
    s = sj * sj * s;
    for (int a = 0; a < q; ++a) s = fma(p.beta[a], p.J[((long)t * q + a) * p.d + j], s);
    p.grad[(long)t * p.d + j] = s;
  }
}

struct PmLayout {
  size_t sxi, part, total;
};
PmLayout pm_layout(int n, int m, int d, bool grad) {
  PmLayout l;
  // partials bounded independently of the tile count, so that the query grows with n, m and d
  const long by_rows = ((long)n + PM_MIN_ROWS - 1) / PM_MIN_ROWS;
  long part = (by_rows - 1) * (long)m * (grad ? 1 + d : 1);
  if (part > PM_PART_CAP) part = PM_PART_CAP;
  WsCursor c;
  l.sxi = c.take((size_t)n * d);
  l.part = c.take((size_t)(part > 0 ? part : 1));
  l.total = c.at;
  return l;
}

int pm_slices(int n, int m, int width) {
  const int ntiles = (m + PM_TM - 1) / PM_TM;
  long ns = (PM_TARGET_WAVES + ntiles - 1) / ntiles;
  const long by_rows = ((long)n + PM_MIN_ROWS - 1) / PM_MIN_ROWS;
  const long by_cap = 1 + PM_PART_CAP / ((long)m * width);
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  return ns < 1 ? 1 : (int)ns;
}

template <int DT>
void launch_tier(const PmParams& gp, dim3 grid, hipStream_t st) {
  if (gp.grad != nullptr) hipLaunchKernelGGL((posterior_mean_kernel<DT, true>), grid, dim3(64), 0, st, gp);
  else hipLaunchKernelGGL((posterior_mean_kernel<DT, false>), grid, dim3(64), 0, st, gp);
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_posterior_mean_ws_elems(int n, int m, int d, int with_gradient) {
  if (n < 1 || n > GPMP_MAX_EXTENT || m < 1 || m > GPMP_MAX_EXTENT || d < 1 || d > GPMP_MAX_DIM) return 0;
  return pm_layout(n, m, d, with_gradient != 0).total;
}

extern "C" int gpmp_posterior_mean(const double* xi, const double* alpha, const double* xt, const double* Pt, long ldpt,
                                   const double* beta, const double* J, int n, int m, int d, int q, int p,
                                   const double* theta_host, int noise, double* ws, double* zpm_dev, double* gzpm_dev,
                                   gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(alpha != nullptr, 2, "alpha is NULL");
  GPMP_ARG(xt != nullptr, 3, "xt is NULL");
  GPMP_ARG(q >= 0 && q < GPMP_MAX_RANK, 11, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(q == 0 || (Pt != nullptr && ldpt >= q), 4, "Pt is NULL or ldpt < q");
  GPMP_ARG(q == 0 || beta != nullptr, 6, "beta is NULL with q > 0");
  GPMP_ARG(q == 0 || gzpm_dev == nullptr || J != nullptr, 7, "J is NULL with q > 0 and a gradient output");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 8, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 9, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM, 10, "d outside [1, GPMP_MAX_DIM] (no wide-dimension variant of this kernel)");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 12, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(theta_host != nullptr, 13, "theta is NULL");
  GPMP_ARG(ws != nullptr, 15, "ws is NULL");
  GPMP_ARG(zpm_dev != nullptr, 16, "zpm is NULL");
  hipStream_t st = as_stream(stream);
  const bool grad = gzpm_dev != nullptr;
  const PmLayout l = pm_layout(n, m, d, grad);
  const MaternTheta th(theta_host, noise, p, d);
  PmParams gp;
  std::memset(&gp, 0, sizeof(gp));
  gp.xi = xi;
  gp.sxi = ws + l.sxi;
  gp.alpha = alpha;
  gp.xt = xt;
  gp.val = zpm_dev;
  gp.grad = gzpm_dev;
  gp.part = ws + l.part;
  gp.Pt = Pt;
  gp.beta = beta;
  gp.J = J;
  gp.ldpt = ldpt;
  gp.n = n;
  gp.m = m;
  gp.d = d;
  gp.q = q;
  gp.width = grad ? 1 + d : 1;
  gp.nslices = pm_slices(n, m, gp.width);
  gp.rows_per_slice = (n + gp.nslices - 1) / gp.nslices;
  th.scales(gp.scale, true);
  th.coefficients(gp.qs);
  for (int k = 0; k <= GPMP_MAX_P; ++k) gp.ss[k] = th.sigma2 * th.ms.s[k];
  gp.p = p;
  fill_fast_exp(gp.fe);
  const long nd = (long)n * d;
  hipLaunchKernelGGL(pm_scale_points_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  const dim3 grid((m + PM_TM - 1) / PM_TM, gp.nslices);
  if (d <= 4) launch_tier<4>(gp, grid, st);
  else if (d <= 8) launch_tier<8>(gp, grid, st);
  else if (d <= 16) launch_tier<16>(gp, grid, st);
  else if (d <= 32) launch_tier<32>(gp, grid, st);
  else launch_tier<GPMP_MAX_DIM>(gp, grid, st);
  GPMP_HIP_TRY(hipGetLastError());
  // lanes per output of the finalize: as many as keep a lane's walk over the slices short
  const long outs = (long)m * gp.width;
  const int lanes = gp.nslices > 64 ? 64 : (gp.nslices > 8 ? 8 : 1);
  const dim3 fgrid((unsigned)((outs * lanes + 255) / 256));
  if (lanes == 64) hipLaunchKernelGGL(posterior_mean_finalize_kernel<64>, fgrid, dim3(256), 0, st, gp);
  else if (lanes == 8) hipLaunchKernelGGL(posterior_mean_finalize_kernel<8>, fgrid, dim3(256), 0, st, gp);
  else hipLaunchKernelGGL(posterior_mean_finalize_kernel<1>, fgrid, dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}
