// Gradient of the posterior mean / variance with respect to the prediction points: the fused cross-gradient reduction
//   G[t][j] = sum_i w_it d k(x_i, x_t) / d x_tj = sigma^2 rho_j^-2 sum_i w_it S(h_it) (x_tj - x_ij),   S(h) = K_p'(h) / h
// for a per-point weight vector u (w_it = u_i) and / or a per-entry weight matrix Lambda (w_it = Lambda_it), in one visit of
// every (i, t) entry.  With t = 2 c h (the variable of the Matern polynomial), S(h) = (2c)^2 e^{-t/2} sum_{k>=1} s_k t^(k-1)
// (MaternSpec.s, p >= 1) and -c e^{-t/2} / h (p = 0); the term is 0 at h = 0 for every p (the limit for p >= 1, the
// reference's custom_sqrt convention for p = 0).  The differences x_tj - x_ij are accumulated directly (no x_t sum_i w -
// sum_i w x_i cancellation), so the epilogue is one factor per dimension: sigma^2 (2c / rho_j)^2.
//
// Layout: one wave per (tile of 64 prediction points, slice of the observation points); lane = prediction point, the loop over
// i reads x_i wave-uniformly.  d <= GPMP_MAX_DIM: x_t and the accumulators in registers, the length scales in the kernel
// arguments.  Above: x_t and the accumulators stay in memory (the point row, the output row of the slice), the length scales in
// device memory, and the entries of a block of WIB observation points share each pass over the dimensions.  Slice 0 writes the
// output array itself, slices s >= 1 a bounded partial buffer in the workspace; a finalize kernel sums the slices and scales.
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int PG_TM = 64;                 // prediction points per wave
constexpr int PG_TARGET_WAVES = 4096;     // 256 CUs x 16 waves
constexpr int PG_MIN_ROWS = 64;           // observation points per slice, at least
constexpr long PG_PART_CAP = 1L << 22;    // doubles of partials per weight kind (32 MB)
constexpr int WIB = 8;                    // wide route: observation points per pass over the dimensions

struct PgParams {
  const double* xi;
  const double* xt;
  const double* u;
  const double* lam;
  long ldl;
  double* gu;                    // slice 0 of the u kind (the output, m x d)
  double* gl;
  double* part;                  // slices 1.. : [kind][slice - 1][m][d]
  long part_kind;                // doubles per kind in part
  int n, m, d, rows_per_slice;
  const double* scale_dev;       // wide route: 2 c / rho_j in device memory
  double scale[GPMP_MAX_DIM];    // register tier: 2 c / rho_j
  MaternSpec ms;
  FastExp fe;
};

// S(h) / (2c)^2 from t = 2 c h (a finite 0 at t = 0)
__device__ __forceinline__ double pg_weight(const MaternSpec& ms, const FastExp& fe, double t2) {
  const double tt = fast_sqrt_pos(t2, fe.tiny);
  const double e = fast_exp_neg_half(fe, tt);
  if (ms.p == 0) return tt > 0.0 ? -0.5 * e / tt : 0.0;
  double sp = ms.s[ms.p];
  for (int k = ms.p - 1; k >= 1; --k) sp = fma(sp, tt, ms.s[k]);
  return e * sp;
}

template <int DT, bool HU, bool HL>
__global__ void __launch_bounds__(64) predict_grad_kernel(PgParams p) {
  const int lane = threadIdx.x;
  const int t = blockIdx.x * PG_TM + lane;
  const int slice = blockIdx.y;
  const int d = p.d, m = p.m;
  const bool valid = t < m;
  const int tc = valid ? t : m - 1;
  const double* __restrict__ xi = p.xi;
  const double* __restrict__ xt = p.xt + (long)tc * d;
  const double* __restrict__ u = p.u;
  const double* __restrict__ lam = p.lam;
  double y[DT], au[DT], al[DT];
#pragma unroll
  for (int j = 0; j < DT; ++j) {
    y[j] = j < d ? xt[j] : 0.0;
    au[j] = 0.0;
    al[j] = 0.0;
  }
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  for (int i = i0; i < i1; ++i) {
    const double* __restrict__ xr = xi + (long)i * d;
    double t2 = 0.0;
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      if (j < d) {
        const double sd = (y[j] - xr[j]) * p.scale[j];
        t2 = fma(sd, sd, t2);
      }
    }
    const double e = pg_weight(p.ms, p.fe, t2);
    double wu = 0.0, wl = 0.0;
    if constexpr (HU) wu = u[i] * e;
    if constexpr (HL) wl = (valid ? lam[(long)i * p.ldl + t] : 0.0) * e;
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      if (j < d) {
        const double df = y[j] - xr[j];
        if constexpr (HU) au[j] = fma(wu, df, au[j]);
        if constexpr (HL) al[j] = fma(wl, df, al[j]);
      }
    }
  }
  if (!valid) return;
  double* ou = slice == 0 ? p.gu : p.part + (long)(slice - 1) * m * d;
  double* ol = slice == 0 ? p.gl : p.part + p.part_kind + (long)(slice - 1) * m * d;
#pragma unroll
  for (int j = 0; j < DT; ++j) {
    if (j < d) {
      if constexpr (HU) ou[(long)t * d + j] = au[j];
      if constexpr (HL) ol[(long)t * d + j] = al[j];
    }
  }
}

template <bool HU, bool HL>
__global__ void __launch_bounds__(64) predict_grad_wide_kernel(PgParams p) {
  const int lane = threadIdx.x;
  const int t = blockIdx.x * PG_TM + lane;
  const int slice = blockIdx.y;
  const int d = p.d, m = p.m;
  const bool valid = t < m;
  const int tc = valid ? t : m - 1;
  const double* __restrict__ xi = p.xi;
  const double* __restrict__ y = p.xt + (long)tc * d;
  const double* __restrict__ sc = p.scale_dev;
  double* ou = (slice == 0 ? p.gu : p.part + (long)(slice - 1) * m * d) + (long)tc * d;
  double* ol = (slice == 0 ? p.gl : p.part + p.part_kind + (long)(slice - 1) * m * d) + (long)tc * d;
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  for (int ib = i0; ib < i1; ib += WIB) {
    const int nb = min(WIB, i1 - ib);
    double t2[WIB];
#pragma unroll
    for (int b = 0; b < WIB; ++b) t2[b] = 0.0;
    for (int j = 0; j < d; ++j) {
      const double yj = y[j], s = sc[j];
#pragma unroll
      for (int b = 0; b < WIB; ++b) {
        if (b < nb) {
          const double sd = (yj - xi[(long)(ib + b) * d + j]) * s;
          t2[b] = fma(sd, sd, t2[b]);
        }
      }
    }
    double wu[WIB], wl[WIB];
#pragma unroll
    for (int b = 0; b < WIB; ++b) {
      const double e = b < nb ? pg_weight(p.ms, p.fe, t2[b]) : 0.0;
      wu[b] = (HU && b < nb) ? p.u[ib + b] * e : 0.0;
      wl[b] = (HL && b < nb && valid) ? p.lam[(long)(ib + b) * p.ldl + t] * e : 0.0;
    }
    if (!valid) continue;
    const bool first = ib == i0;
    for (int j = 0; j < d; ++j) {
      const double yj = y[j];
      double su = first ? 0.0 : (HU ? ou[j] : 0.0);
      double sl = first ? 0.0 : (HL ? ol[j] : 0.0);
#pragma unroll
      for (int b = 0; b < WIB; ++b) {
        if (b < nb) {
          const double df = yj - xi[(long)(ib + b) * d + j];
          if constexpr (HU) su = fma(wu[b], df, su);
          if constexpr (HL) sl = fma(wl[b], df, sl);
        }
      }
      if constexpr (HU) ou[j] = su;
      if constexpr (HL) ol[j] = sl;
    }
  }
  // an empty slice (possible only for the last one) still owns its output rows
  if (valid && i0 >= i1) {
    for (int j = 0; j < d; ++j) {
      if constexpr (HU) ou[j] = 0.0;
      if constexpr (HL) ol[j] = 0.0;
    }
  }
}

// out[t][j] = sigma^2 scale_j^2 (slice 0 + sum of the partial slices)
__global__ void predict_grad_finalize_kernel(double* __restrict__ out, const double* __restrict__ part, int nparts, long m_d, int d,
                                             const double* __restrict__ scale, double sigma2) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m_d) return;
  double s = out[idx];
  for (int k = 0; k < nparts; ++k) s += part[(long)k * m_d + idx];
  const double sj = scale[idx % d];
  out[idx] = sigma2 * sj * sj * s;
}

int pg_slices(int n, int m, int d) {
  const int ntiles = (m + PG_TM - 1) / PG_TM;
  long ns = (PG_TARGET_WAVES + ntiles - 1) / ntiles;
  const long by_rows = ((long)n + PG_MIN_ROWS - 1) / PG_MIN_ROWS;
  const long by_cap = 1 + PG_PART_CAP / ((long)m * d);
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  return ns < 1 ? 1 : (int)ns;
}

struct PgLayout {
  size_t scale, part, part_kind, total;
};
PgLayout pg_layout(int n, int m, int d) {
  PgLayout l;
  // partials bounded independently of the tile count, so that the query grows with n, m and d
  const long by_rows = ((long)n + PG_MIN_ROWS - 1) / PG_MIN_ROWS;
  long kind = (by_rows - 1) * (long)m * d;
  if (kind > PG_PART_CAP) kind = PG_PART_CAP;
  l.scale = 0;
  l.part = (size_t)pad16(d);
  l.part_kind = (size_t)pad16(kind);
  l.total = l.part + 2 * l.part_kind;
  return l;
}

template <int DT>
void launch_tier(const PgParams& gp, dim3 grid, hipStream_t st) {
  if (gp.u != nullptr && gp.lam != nullptr) hipLaunchKernelGGL((predict_grad_kernel<DT, true, true>), grid, dim3(64), 0, st, gp);
  else if (gp.u != nullptr) hipLaunchKernelGGL((predict_grad_kernel<DT, true, false>), grid, dim3(64), 0, st, gp);
  else hipLaunchKernelGGL((predict_grad_kernel<DT, false, true>), grid, dim3(64), 0, st, gp);
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_predict_grad_reduce_ws_elems(int n, int m, int d) {
  if (n < 1 || n > GPMP_MAX_EXTENT || m < 1 || m > GPMP_MAX_EXTENT || d < 1 || d > GPMP_MAX_DIM_WIDE) return 0;
  return pg_layout(n, m, d).total;
}

extern "C" int gpmp_predict_grad_reduce(const double* xi, const double* xt, int n, int m, int d, int p, const double* theta_host,
                                        int noise, const double* u, const double* lam, long ldl, double* gu_dev, double* gl_dev,
                                        double* ws, gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(xt != nullptr, 2, "xt is NULL");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 3, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 4, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 5, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 6, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(theta_host != nullptr, 7, "theta is NULL");
  GPMP_ARG((u == nullptr) == (gu_dev == nullptr), 9, "u and gu must be given together");
  GPMP_ARG(lam == nullptr || ldl >= m, 11, "ldl < m");
  GPMP_ARG((lam == nullptr) == (gl_dev == nullptr), 10, "Lambda and gl must be given together");
  GPMP_ARG(u != nullptr || lam != nullptr, 9, "neither u nor Lambda is given");
  GPMP_ARG(ws != nullptr, 14, "ws is NULL");
  hipStream_t st = as_stream(stream);
  const PgLayout l = pg_layout(n, m, d);
  PgParams gp;
  std::memset(&gp, 0, sizeof(gp));
  const MaternTheta th(theta_host, noise, p, d);
  gp.ms = th.ms;
  fill_fast_exp(gp.fe);
  if (d <= GPMP_MAX_DIM) th.scales(gp.scale, true);
  // the factors in device memory (finalize, wide route)
  double* scale_dev = ws + l.scale;
  if (hipError_t ce = stage_vector(th.scale_vector(true), scale_dev, st)) return hip_fail(ce, "staging the length scales");
  const int ns = pg_slices(n, m, d);
  gp.xi = xi;
  gp.xt = xt;
  gp.u = u;
  gp.lam = lam;
  gp.ldl = ldl;
  gp.gu = gu_dev;
  gp.gl = gl_dev;
  gp.part = ws + l.part;
  gp.part_kind = (long)l.part_kind;
  gp.n = n;
  gp.m = m;
  gp.d = d;
  gp.rows_per_slice = (n + ns - 1) / ns;
  gp.scale_dev = scale_dev;
  const dim3 grid((m + PG_TM - 1) / PG_TM, ns);
  if (d <= 4) launch_tier<4>(gp, grid, st);
  else if (d <= 8) launch_tier<8>(gp, grid, st);
  else if (d <= 16) launch_tier<16>(gp, grid, st);
  else if (d <= 32) launch_tier<32>(gp, grid, st);
  else if (d <= GPMP_MAX_DIM) launch_tier<GPMP_MAX_DIM>(gp, grid, st);
  else if (u != nullptr && lam != nullptr) hipLaunchKernelGGL((predict_grad_wide_kernel<true, true>), grid, dim3(64), 0, st, gp);
  else if (u != nullptr) hipLaunchKernelGGL((predict_grad_wide_kernel<true, false>), grid, dim3(64), 0, st, gp);
  else hipLaunchKernelGGL((predict_grad_wide_kernel<false, true>), grid, dim3(64), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  const long md = (long)m * d;
  const unsigned fblocks = (unsigned)((md + 255) / 256);
  if (u != nullptr) {
    hipLaunchKernelGGL(predict_grad_finalize_kernel, dim3(fblocks), dim3(256), 0, st, gu_dev, ws + l.part, ns - 1, md, d, scale_dev, th.sigma2);
    GPMP_HIP_TRY(hipGetLastError());
  }
  if (lam != nullptr) {
    hipLaunchKernelGGL(predict_grad_finalize_kernel, dim3(fblocks), dim3(256), 0, st, gl_dev, ws + l.part + l.part_kind, ns - 1, md, d,
                       scale_dev, th.sigma2);
    GPMP_HIP_TRY(hipGetLastError());
  }
  return 0;
}
