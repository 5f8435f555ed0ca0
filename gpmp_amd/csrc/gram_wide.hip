// The wide-dimension route: Gram / distance tiles, pairwise values, derivative matrices and the gradient trace for inputs of
// GPMP_MAX_DIM < d <= GPMP_MAX_DIM_WIDE.  The kernels of gram.hip keep the d length scales in their argument block (scalar
// registers) and one register accumulator per dimension in the gradient trace; neither scales to hundreds of dimensions.  Here
// the length scales live in device memory and d is streamed through LDS in chunks, both for the distance and for the
// per-dimension gradient sums, so nothing in a kernel grows with d.
//
// Numerics are those of gram.hip: distances by direct differences of pre-scaled coordinates (the reference's cdist, never the
// |x|^2 + |y|^2 - 2 x.y expansion), the same sqrt / exp / Matern tail (matern_device.h), and the same summation order over the
// dimensions -- a point set padded with zero coordinates gives the same K on both routes.
#include "matern_device.h"
#include <cfloat>

namespace gpmp {
namespace {

// ---- stream-ordered staging of the per-dimension factors ------------------------------------------------------------------
// Copies *v into dst (device) behind the work already on st; the host vector is freed by a host function enqueued behind the
// copy (the call stays enqueue-only).  Takes ownership of v in every case.
int stage_vector(std::vector<double>* v, double* dst, hipStream_t st) {
  hipError_t ce = hipMemcpyAsync(dst, v->data(), sizeof(double) * v->size(), hipMemcpyHostToDevice, st);
  if (ce == hipSuccess) ce = hipLaunchHostFunc(st, [](void* q) { delete static_cast<std::vector<double>*>(q); }, v);
  if (ce != hipSuccess) {
    (void)hipStreamSynchronize(st);
    delete v;
    set_error("HIP error %s staging the length scales", hipGetErrorString(ce));
    return -100;
  }
  return 0;
}

// A stream-ordered device copy of the factors for one call (every call its own buffer: concurrent calls on different streams
// never share one); freed in stream order when the owner goes out of scope, i.e. behind the kernels enqueued meanwhile.
struct StagedScales {
  double* dev = nullptr;
  hipStream_t st;
  explicit StagedScales(hipStream_t s) : st(s) {}
  int stage(std::vector<double>* v) {
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&dev), sizeof(double) * v->size(), st);
    if (e != hipSuccess) {
      dev = nullptr;
      delete v;
      return hip_fail(e, "hipMallocAsync (length scales)");
    }
    return stage_vector(v, dev, st);
  }
  ~StagedScales() {
    if (dev != nullptr) (void)hipFreeAsync(dev, st);
  }
};

// ---- Gram / scaled-distance tile ------------------------------------------------------------------------------------------
struct GramWideParams {
  const double* x;
  const double* y;
  double* K;
  long ldk;
  int n, m, d;
  int same, lower_only, aligned;
  int p;
  double diag_add;
  const double* scale;           // device, d values: mode 0: 2 c / rho_j; mode 1: 1 / rho_j
  double q[GPMP_MAX_P + 1];      // sigma^2 q_k
  FastExp fe;
};

// gram_kernel_v3's tiling (128 x 64 outputs per 256-thread workgroup, 8 x 4 per thread, DC dimensions per LDS chunk); the chunk
// loop already streams d, only the scale factors now come from device memory (read while staging, once per element).
// Per entry: 2 d VALU instructions of distance + the tail of gram_kernel_v3.
template <int P, int MODE>
__global__ void __launch_bounds__(256) gram_wide_kernel(GramWideParams p) {
  __shared__ __attribute__((aligned(16))) double xs[DC][128];
  __shared__ __attribute__((aligned(16))) double ys[DC][GT];
  const int tj = blockIdx.x, ti = blockIdx.y;
  const int row0 = ti * 128, col0 = tj * GT;
  if (p.lower_only && col0 > row0 + 127) return;
  const double* __restrict__ px = p.x;
  const double* __restrict__ sc = p.scale;
  const int pn = p.n, pm = p.m, d = p.d;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const double* __restrict__ yp = p.same ? px : p.y;

  double acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

  for (int k0 = 0; k0 < d; k0 += DC) {
    if (k0) __syncthreads();
    const int kc = (d - k0) < DC ? (d - k0) : DC;
    for (int idx = t; idx < 128 * kc; idx += 256) {
      const int r = idx / kc, k = idx - r * kc;
      xs[k][r] = (row0 + r < pn) ? sc[k0 + k] * px[(long)(row0 + r) * d + k0 + k] : 0.0;
    }
    for (int idx = t; idx < GT * kc; idx += 256) {
      const int r = idx / kc, k = idx - r * kc;
      ys[k][r] = (col0 + r < pm) ? sc[k0 + k] * yp[(long)(col0 + r) * d + k0 + k] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const d4 xa0 = *reinterpret_cast<const d4*>(&xs[k][ty * 8]);
      const d4 xa1 = *reinterpret_cast<const d4*>(&xs[k][ty * 8 + 4]);
      const d2 y0 = *reinterpret_cast<const d2*>(&ys[k][2 * tx]);
      const d2 y1 = *reinterpret_cast<const d2*>(&ys[k][32 + 2 * tx]);
      const double yb[4] = {y0[0], y0[1], y1[0], y1[1]};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double d0 = xa0[a] - yb[b], d1 = xa1[a] - yb[b];
          acc[a][b] = fma(d0, d0, acc[a][b]);
          acc[a + 4][b] = fma(d1, d1, acc[a + 4][b]);
        }
    }
  }

  const bool full = p.aligned && (row0 + 128 <= pn) && (col0 + GT <= pm);
  const bool diag_tile = p.same && (col0 < row0 + 128) && (col0 + GT > row0);
  double* __restrict__ out = p.K + (long)(row0 + ty * 8) * p.ldk + col0 + 2 * tx;
  const int pdeg = (P >= 0) ? P : p.p;
  constexpr int NQ = P >= 0 ? P + 1 : 1;
  double qc[NQ] = {};
  if constexpr (P >= 0) {
#pragma unroll
    for (int k = 0; k <= P; ++k) qc[k] = p.q[k];
  }
  double qtop = p.q[pdeg], c12 = p.fe.c[12];
  asm volatile("" : "+v"(qtop), "+v"(c12));
  gram_tile_finish<P, MODE>(acc, p.fe, qc, [&](int k) { return p.q[k]; }, qtop, c12, pdeg, p.diag_add, diag_tile, full, out,
                            p.ldk, row0, col0, ty, tx, pn, pm);
}

// ---- pairwise values and derivative matrices: one thread per entry, a loop over d ------------------------------------------
__global__ void pairwise_wide_kernel(const double* __restrict__ x, const double* __restrict__ y, int n, int d, int same,
                                     double sigma2, const double* __restrict__ invrho, MaternSpec ms, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double h = 0.0;
  if (!same) {
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
      const double df = invrho[k] * (x[(long)i * d + k] - y[(long)i * d + k]);
      s = fma(df, df, s);
    }
    h = sqrt(s);
  }
  out[i] = sigma2 * matern_dispatch(ms, h);
}

__global__ void gram_deriv_wide_kernel(const double* __restrict__ x, int n, int d, int jdim, int kind, double sigma2,
                                       double diag_val, const double* __restrict__ invrho, MaternSpec ms, double* __restrict__ out,
                                       long ld) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (k >= n) return;
  double v = 0.0;
  if (kind == 1) {
    v = (i == k) ? diag_val : 0.0;
  } else {
    double s = 0.0, dj = 0.0;
    for (int c = 0; c < d; ++c) {
      const double df = invrho[c] * (x[(long)i * d + c] - x[(long)k * d + c]);
      s = fma(df, df, s);
      if (c == jdim) dj = df * df;
    }
    const double h = sqrt(s);
    double kval;
    const double dk = matern_dk_over_h(ms, h, kval);
    if (kind == 0) v = sigma2 * kval + ((i == k) ? diag_val : 0.0);
    else v = sigma2 * dk * dj;
  }
  out[(long)i * ld + k] = v;
}

// ---- gradient trace -------------------------------------------------------------------------------------------------------
// Same quantities as grad_trace_kernel (gram.hip), with M = Kinv - F G^T (or the rectangular cross block):
//   col 0: sum M K,  col 1 + j: sum M (K'(h)/h) (scale_j delta_j)^2,  col d + 1: trace(M)
// per 64 x 64 tile of M, 4 x 4 entries per thread.  Pass 1 streams d through LDS for t^2 and keeps the entry weights
// W = M (K'(h)/h) in registers; pass 2 streams d again and, per dimension of a chunk, sums W delta_j^2 over the tile: per thread in
// registers, then over the workgroup through LDS (all 256 threads share the WDC-column transposition), into this workgroup's row of
// per-block partials (width d + 2).  About 2 d (pass 1) + 3 d (pass 2) VALU instructions per entry, no n x n buffer.
constexpr int WDC = 16;          // dimensions per chunk
constexpr int RED_LD = 257;      // padded row of the per-chunk reduction image (conflict-light column reads)
constexpr int GRAD_WIDE_BLOCKS = 512;

struct GradWideParams {
  const double* M;
  long ldm;
  const double* x;
  const double* y;               // cross: column points (m of them); else x
  const double* F;
  const double* G;
  long ldf;
  int n, m, d, r;
  int ntiles, ntiles_c;          // tiles of the traversal; cross: tiles per tile row
  const double* scale;           // device, d values: 2 c / rho_j
  double* partial;               // [gridDim.x][d + 2]
  MaternSpec ms;
  FastExp fe;
};

template <bool CROSS>
__global__ void __launch_bounds__(256) grad_trace_wide_kernel(GradWideParams p) {
  extern __shared__ __attribute__((aligned(16))) double smw[];
  double* fs = smw;                   // [r][GT]  F rows of the tile's i block
  double* gs = fs + p.r * GT;         // [r][GT]  G rows of the tile's k block
  __shared__ __attribute__((aligned(16))) double xs[WDC][GT];
  __shared__ __attribute__((aligned(16))) double ys[WDC][GT];
  __shared__ double red[WDC * RED_LD];
  __shared__ double red2[16][WDC + 1];
  __shared__ double red3[4][2];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const double* __restrict__ pM = p.M;
  const double* __restrict__ px = p.x;
  const double* __restrict__ py = CROSS ? p.y : p.x;
  const double* __restrict__ sc = p.scale;
  double* __restrict__ part = p.partial + (long)blockIdx.x * (p.d + 2);
  const int pn = p.n, d = p.d, ncols = CROSS ? p.m : p.n;
  double g0 = 0.0, gtr = 0.0;

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const bool first = tile == (int)blockIdx.x;
    int ti, tj;
    if constexpr (CROSS) {
      ti = tile / p.ntiles_c;
      tj = tile - ti * p.ntiles_c;
    } else {
      ti = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
      while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
      while (ti * (ti + 1) / 2 > tile) --ti;
      tj = tile - ti * (ti + 1) / 2;
    }
    const int row0 = ti * GT, col0 = tj * GT;
    auto stage = [&](int k0, int kc) {
      for (int idx = t; idx < GT * kc; idx += 256) {
        const int rr = idx / kc, k = idx - rr * kc;
        const double s = sc[k0 + k];
        xs[k][rr] = (row0 + rr < pn) ? s * px[(long)(row0 + rr) * d + k0 + k] : 0.0;
        ys[k][rr] = (col0 + rr < ncols) ? s * py[(long)(col0 + rr) * d + k0 + k] : 0.0;
      }
    };
    __syncthreads();
    for (int idx = t; idx < p.r * GT; idx += 256) {
      const int rr = idx / p.r, a = idx % p.r;
      fs[a * GT + rr] = (row0 + rr < pn) ? p.F[(long)(row0 + rr) * p.ldf + a] : 0.0;
      gs[a * GT + rr] = (col0 + rr < ncols) ? p.G[(long)(col0 + rr) * p.ldf + a] : 0.0;
    }
    // ---- pass 1: t^2 = sum_j (scale_j delta_j)^2
    double h2[4][4], w[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) { h2[a][b] = 0.0; w[a][b] = 0.0; }
    for (int k0 = 0; k0 < d; k0 += WDC) {
      const int kc = (d - k0) < WDC ? (d - k0) : WDC;
      if (k0) __syncthreads();
      stage(k0, kc);
      __syncthreads();
      for (int k = 0; k < kc; ++k) {
        const d4 xa = *reinterpret_cast<const d4*>(&xs[k][ty * 4]);
        const d4 yb = *reinterpret_cast<const d4*>(&ys[k][tx * 4]);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = xa[a] - yb[b];
            h2[a][b] = fma(df, df, h2[a][b]);
          }
      }
    }
    // ---- weights (as grad_trace_kernel)
    for (int a2 = 0; a2 < p.r; ++a2) {
      const d4 fa = *reinterpret_cast<const d4*>(&fs[a2 * GT + ty * 4]);
      const d4 gb = *reinterpret_cast<const d4*>(&gs[a2 * GT + tx * 4]);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) w[a][b] = fma(fa[a], gb[b], w[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = row0 + ty * 4 + a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int col = col0 + tx * 4 + b;
        double wt = 0.0;
        if constexpr (CROSS) {
          if (row < pn && col < ncols) wt = 1.0;
        } else {
          if (row < pn && col < pn) wt = col < row ? 2.0 : (col == row ? 1.0 : 0.0);
        }
        double mval = 0.0;
        if (wt != 0.0) mval = wt * (pM[(long)row * p.ldm + col] - w[a][b]);
        const double tt = fast_sqrt_pos(h2[a][b], p.fe.tiny);
        const double e = fast_exp_neg_half(p.fe, tt);
        double poly = p.ms.q[p.ms.p];
        for (int k = p.ms.p - 1; k >= 0; --k) poly = fma(poly, tt, p.ms.q[k]);
        const double kval = e * poly;
        double dk;
        if (p.ms.p == 0) {
          dk = tt > 0.0 ? -0.5 * e / tt : 0.0;       // subgradient 0 at coincident points (ref_gradients_p0)
        } else {
          double sp = p.ms.s[p.ms.p];
          for (int k = p.ms.p - 1; k >= 1; --k) sp = fma(sp, tt, p.ms.s[k]);
          dk = e * sp;
        }
        g0 = fma(mval, kval, g0);
        if (!CROSS && row == col) gtr += mval;
        w[a][b] = mval * dk;
      }
    }
    // ---- pass 2: per dimension j, sum_tile W (scale_j delta_j)^2
    for (int k0 = 0; k0 < d; k0 += WDC) {
      const int kc = (d - k0) < WDC ? (d - k0) : WDC;
      __syncthreads();               // xs / ys / red / red2 free
      stage(k0, kc);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < WDC; ++k) {
        double s = 0.0;
        if (k < kc) {
          const d4 xa = *reinterpret_cast<const d4*>(&xs[k][ty * 4]);
          const d4 yb = *reinterpret_cast<const d4*>(&ys[k][tx * 4]);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const double df = xa[a] - yb[b];
              s = fma(w[a][b], df * df, s);
            }
        }
        red[k * RED_LD + t] = s;
      }
      __syncthreads();
      {
        // thread (j = t % 16, grp = t / 16) sums the 16 values of group grp for dimension k0 + j
        const int j = t & 15, grp = t >> 4;
        const double* src = red + j * RED_LD + grp * 16;
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += src[i];
        red2[grp][j] = s;
      }
      __syncthreads();
      if (t < kc) {
        double s = 0.0;
#pragma unroll
        for (int grp = 0; grp < 16; ++grp) s += red2[grp][t];
        double* dst = part + 1 + k0 + t;
        *dst = first ? s : *dst + s;   // this thread owns this column of the block's row for the whole launch
      }
    }
  }

  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    g0 += __shfl_xor(g0, o);
    gtr += __shfl_xor(gtr, o);
  }
  if (lane == 0) { red3[wave][0] = g0; red3[wave][1] = gtr; }
  __syncthreads();
  if (t == 0) {
    part[0] = red3[0][0] + red3[1][0] + red3[2][0] + red3[3][0];
    part[d + 1] = red3[0][1] + red3[1][1] + red3[2][1] + red3[3][1];
  }
}

// Sums the per-block partials (one thread per column, blocks in order) and scales them:
//   cross == 0 (gpmp_matern_grad_trace): g = [sigma2 s_0 + nugget_scale sigma2 tr, (noise_var tr), sigma2 s_1..d]
//   cross != 0 (gpmp_matern_grad_trace_cross): g = sigma2 s_0..d
__global__ void grad_wide_finalize_kernel(const double* __restrict__ partial, int nblocks, int d, int cross, int noise, double sigma2,
                                          double nugget_scale, double noise_var, double* __restrict__ g) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d) return;
  const long width = (long)d + 2;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(long)b * width + k];
  if (cross) {
    g[k] = sigma2 * s;
    return;
  }
  if (k == 0) {
    double tr = 0.0;
    for (int b = 0; b < nblocks; ++b) tr += partial[(long)b * width + d + 1];
    g[0] = sigma2 * s + nugget_scale * sigma2 * tr;
    if (noise) g[1] = noise_var * tr;
  } else {
    g[(noise ? 1 : 0) + k] = sigma2 * s;
  }
}

template <int P, int MODE>
void launch_gram_wide(const GramWideParams& gp, hipStream_t st) {
  dim3 grid((gp.m + GT - 1) / GT, (gp.n + 127) / 128);
  hipLaunchKernelGGL((gram_wide_kernel<P, MODE>), grid, dim3(256), 0, st, gp);
}

}  // namespace

int gram_wide(const double* x, const double* y, int n, int m, int d, int mode, int p, std::vector<double>* scale, const double* q,
              double diag_add, int lower_only, double* K, long ldk, hipStream_t st) {
  StagedScales sc(st);
  int rc = sc.stage(scale);
  if (rc) return rc;
  GramWideParams gp;
  gp.x = x; gp.y = y; gp.K = K; gp.ldk = ldk;
  gp.n = n; gp.m = m; gp.d = d;
  gp.same = (y == nullptr); gp.lower_only = (y == nullptr) ? lower_only : 0;
  gp.aligned = ((reinterpret_cast<uintptr_t>(K) & 15) == 0) && ((ldk & 1) == 0);
  gp.p = p;
  gp.diag_add = diag_add;
  gp.scale = sc.dev;
  for (int k = 0; k <= GPMP_MAX_P; ++k) gp.q[k] = q[k];
  fill_fast_exp(gp.fe);
  {
    ProfScope ps(PK_GRAM, st, 8.0 * (double)n * (double)m * (gp.lower_only ? 0.5 : 1.0));
    if (mode != 0) {
      launch_gram_wide<0, 1>(gp, st);
    } else {
      switch (p) {
        case 0: launch_gram_wide<0, 0>(gp, st); break;
        case 1: launch_gram_wide<1, 0>(gp, st); break;
        case 2: launch_gram_wide<2, 0>(gp, st); break;
        case 3: launch_gram_wide<3, 0>(gp, st); break;
        default: launch_gram_wide<-1, 0>(gp, st); break;
      }
    }
  }
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

int pairwise_wide(const double* x, const double* y, int n, int d, int p, double sigma2, std::vector<double>* invrho, double* out,
                  hipStream_t st) {
  StagedScales sc(st);
  int rc = sc.stage(invrho);
  if (rc) return rc;
  MaternSpec ms;
  fill_matern(ms, p);
  hipLaunchKernelGGL(pairwise_wide_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, y, n, d, (y == nullptr || y == x) ? 1 : 0,
                     sigma2, (const double*)sc.dev, ms, out);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

int gram_deriv_wide(const double* x, int n, int d, int p, int kind, int jdim, double sigma2, double diag_val,
                    std::vector<double>* invrho, double* out, long ld, hipStream_t st) {
  StagedScales sc(st);
  int rc = sc.stage(invrho);
  if (rc) return rc;
  MaternSpec ms;
  fill_matern(ms, p);
  hipLaunchKernelGGL(gram_deriv_wide_kernel, dim3((n + 255) / 256, n), dim3(256), 0, st, x, n, d, jdim, kind, sigma2, diag_val,
                     (const double*)sc.dev, ms, out, ld);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

size_t grad_wide_ws_elems(int n, int d) {
  (void)n;
  return (size_t)GRAD_WIDE_BLOCKS * ((size_t)d + 2) + (size_t)d;     // per-block partials | the d scale factors
}

int grad_trace_wide(const double* M, long ldm, const double* x, int n, const double* y, int m, int d, int p, double sigma2, int noise,
                    double noise_var, std::vector<double>* scale, const double* F, const double* G, int r, long ldf, double* g_dev,
                    double* ws, int cross, hipStream_t st) {
  GradWideParams gp;
  gp.M = M; gp.ldm = ldm; gp.x = x; gp.y = cross ? y : x; gp.F = F; gp.G = G; gp.ldf = ldf;
  gp.n = n; gp.m = cross ? m : n; gp.d = d; gp.r = r;
  const long side = (n + GT - 1) / GT;
  long nt;
  if (cross) {
    gp.ntiles_c = (m + GT - 1) / GT;
    nt = side * gp.ntiles_c;
  } else {
    gp.ntiles_c = 0;
    nt = side * (side + 1) / 2;
  }
  if (nt >= 0x7FFFFFFFL) {
    delete scale;
    set_error("argument 4: too many tiles");
    return -4;
  }
  gp.ntiles = (int)nt;
  const int nblocks = gp.ntiles < GRAD_WIDE_BLOCKS ? gp.ntiles : GRAD_WIDE_BLOCKS;
  gp.partial = ws;
  double* scale_dev = ws + (size_t)GRAD_WIDE_BLOCKS * ((size_t)d + 2);
  int rc = stage_vector(scale, scale_dev, st);
  if (rc) return rc;
  gp.scale = scale_dev;
  fill_matern(gp.ms, p);
  fill_fast_exp(gp.fe);
  const size_t lds = sizeof(double) * 2 * (size_t)r * GT;
  auto go = [&](auto kern, DeviceOnce& once) -> int {
    if (const long long dev_bit = once.need()) {
      if (dev_bit < 0) { set_error("hipGetDevice failed or device ordinal above 62"); return -1; }
      GPMP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(sizeof(double) * 2 * GPMP_MAX_RANK * GT)));
      once.done(dev_bit);
    }
    ProfScope ps(PK_GRAD, st, (double)nt * GT * GT);
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), lds, st, gp);
    GPMP_HIP_TRY(hipGetLastError());
    return 0;
  };
  static DeviceOnce once_sym, once_cross;
  rc = cross ? go(grad_trace_wide_kernel<true>, once_cross) : go(grad_trace_wide_kernel<false>, once_sym);
  if (rc) return rc;
  const double eps = 2.220446049250313e-16;
  const double nugget_scale = noise ? 0.0 : 10.0 * eps;   // matern.py:90: nugget = 10 sigma2 eps
  hipLaunchKernelGGL(grad_wide_finalize_kernel, dim3((d + 1 + 255) / 256), dim3(256), 0, st, ws, nblocks, d, cross, noise, sigma2,
                     nugget_scale, noise_var, g_dev);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace gpmp
