// Posterior mean from stored weights, matrix-free, for ANY input dimension 1 <= d <= GPMP_MAX_DIM_WIDE and s >= 1 observation
// columns: with A = K^-1 (Z - P B) (n x s) and B (q x s) from gpmp_posterior_weights_multi,
//   O[t][c] = sum_i sigma^2 K_p(h_it) A[i][c] + sum_a Pt[t][a] B[a][c]                                           (m x s, ldo)
// The register-tier kernels (posterior_mean.hip, posterior_mean_multi.hip) keep the lane's whole scaled x_t resident and take the
// length scales in the kernel arguments, so they stop at GPMP_MAX_DIM.  This kernel streams d: the scales live in device memory
// (staged into the workspace per call, as the *WideParams blocks of gram.hip), the observation points pass through LDS in chunks of
// dimensions and the lane's x_t in sub-chunks through registers.  The single-column case is s = 1 (lda = ldo = 1): at these d the
// 2 d distance instructions of an entry outweigh the one matrix instruction that contracts it.
//
// Value bits.  Per entry the arithmetic is gram_kernel_v3's on its wide route, operation for operation: both points scaled by
// 2 c / rho_j BEFORE the subtraction (a plain product, never fused; the observation points once per call in a pre-pass into the
// workspace, x_t on load), fma(delta, delta, acc) over j in ascending order into ONE accumulator per entry, then the sqrt / exp /
// Horner chain over sigma^2 q_k (matern_lockstep).  No norm expansion.  Dimensions past d are zeros on both sides -- fma(0, 0, acc)
// is acc -- so a point set padded with zero coordinates gives the same entries, and O differs from G^T A, G =
// gpmp_matern_gram(xi, xt), only in the order of the sum over i.
//
// Split.  A workgroup is 4 waves and owns PMW_TM = 128 prediction points, one slice of the observation points and one block of
// 16 CT columns (blockIdx.x / .y / .z).  Wave w owns the TWO point tiles 32 w .. 32 w + 15 and 32 w + 16 .. 32 w + 31.  With the
// operand map of gemm_f64.hip (A: lane l holds A[row l & 15][k l >> 4]) lane l owns, of every point tile, point l & 15 and, of
// every group g of 4 observation points, observation 4 g + (l >> 4): its register tile is 2 x 16 squared-distance accumulators
// over the PMW_CH = 64 observation points of a chunk, and each finished entry is directly the A operand of one
// v_mfma_f64_16x16x4_f64 per column tile.  No entry is evaluated twice in a workgroup.
//
// Data movement.  Per observation chunk the dimensions stream in LDS chunks of PMW_DC = 32 (64 rows, row stride 34 doubles: the
// four rows of a 16-byte read fall into different banks), and within one in register sub-chunks of PMW_DR = 8: the lane loads and
// scales 2 x 8 coordinates of its two points, then every 16-byte LDS read (two dimensions of one observation point) serves four
// (entry, dimension) pairs -- 8 LDS reads per 64 vector instructions, against 6 in gram_kernel_v3.  One load of x_t serves all 64
// observation points of the chunk (0.125 bytes of x_t per (entry, dimension)).  After the last LDS chunk the Matern tail runs in
// lock step over batches of 4 entries (two groups x two point tiles), and each batch's matrix instructions alternate between the
// point tiles and the CT column tiles, so consecutive instructions never wait for each other's accumulator.  The B operand of
// column tile ct is the staged row A[4 g + (l >> 4)][16 ct + (l & 15)] (64 rows, row stride 80).
//
// Edges.  As posterior_mean_multi.hip: an observation row past the end of the slice is staged as the slice's LAST point with its
// row of A as zeros (a finite entry times 0); a prediction row t >= m computes on point m - 1 and is not stored; columns c >= s are
// zeros in the B operand and are not stored; nothing beyond column s of a row of A, B or O is touched.  CT is chosen per call
// (s <= 16, 32, 48: 1, 2, 3; else 4); column blocks are 64 wide.
//
// Slices over i fill the machine when m is small: slice 0 writes O, slices k >= 1 a bounded partial buffer [k - 1][m][s] in the
// workspace (at most 4 M doubles); the finalize kernel -- one lane per (t, c) -- adds the slices in a fixed order and then the mean
// part; a call of one slice and q = 0 skips it.  No atomics: two calls on the same inputs give the same bits.
//
// Resources (compiler's remarks, no scratch and no spill in any instance; two workgroups per CU): see DESIGN.md section 4.
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int PMW_TM = 128;                // prediction points per workgroup (two tiles of 16 per wave)
constexpr int PMW_TP = 2;                  // point tiles per wave
constexpr int PMW_CB = 64;                 // columns per column block: 16 CT
constexpr int PMW_CH = 64;                 // observation points per chunk: 16 groups of 4
constexpr int PMW_NG = PMW_CH / 4;         // groups per chunk = squared-distance accumulators per point tile and lane
constexpr int PMW_DC = 32;                 // dimensions per LDS chunk
constexpr int PMW_DR = 8;                  // dimensions of x_t per register sub-chunk
constexpr int PMW_SXLD = PMW_DC + 2;       // row stride of the staged points
constexpr int PMW_ALD = 80;                // row stride of the staged rows of A
constexpr int PMW_TARGET_WGS = 1024;       // workgroups a call is sliced towards (two are resident per CU); not tuned
constexpr int PMW_MIN_ROWS = 4 * PMW_CH;   // observation points per slice, at least
constexpr long PMW_PART_CAP = 1L << 22;    // doubles of partials (32 MB)
constexpr int PMW_FIN_BLOCKS = 1 << 16;    // workgroups of the finalize kernel, at most (it strides over the outputs)

constexpr int pmw_ct(int s) { return s <= 16 ? 1 : s <= 32 ? 2 : s <= 48 ? 3 : 4; }

// (never written inside a kernel: one store into the by-value block and the compiler keeps a private copy of it in scratch memory)
struct PmwParams {
  const double* xi;              // n x d
  double* sxi;                   // n x d, scaled by 2 c / rho_j (workspace, written by the pre-pass)
  const double* scale;           // d values 2 c / rho_j (workspace, staged per call)
  const double* A;               // n x s weights (lda)
  const double* xt;              // m x d
  double* O;                     // m x s (ldo): slice 0, then the result
  double* part;                  // slices 1.. : [slice - 1][m][s]
  const double* Pt;              // mean part (q > 0): m x q (ldpt)
  const double* B;               // q x s (ldb)
  long lda, ldo, ldpt, ldb;
  int n, m, s, d, q, rows_per_slice, nslices, p;
  double qs[GPMP_MAX_P + 1];     // sigma^2 q_k:  sigma^2 K_p(h) = exp(-t/2) sum_k qs[k] t^k, t = 2 c h
  FastExp fe;
};

// Chunk staging (between the two barriers of the dimension loop; 4 threads per chunk row, so a thread keeps ONE row address):
// dimensions k0 .. k0 + 31 of the scaled observation points ic .. ic + 63, zeros past d.
__device__ __forceinline__ void pmw_stage_points(const PmwParams& p, double* sx, int ic, int i1, int k0) {
  const int r = threadIdx.x >> 2, j0 = threadIdx.x & 3, d = p.d;
  const double* __restrict__ src = p.sxi + (long)min(ic + r, i1 - 1) * d + k0;
#pragma unroll
  for (int j = j0; j < PMW_DC; j += 4) sx[r * PMW_SXLD + j] = k0 + j < d ? src[j] : 0.0;
}

// ... and columns c0 .. c0 + 16 CT - 1 of their rows of A (once per observation chunk).
template <int CT>
__device__ __forceinline__ void pmw_stage_weights(const PmwParams& p, double* sa, int ic, int i1, int c0) {
  const int r = threadIdx.x >> 2, j0 = threadIdx.x & 3;
  const bool live = ic + r < i1;
  const double* __restrict__ ar = p.A + (long)(live ? ic + r : i1 - 1) * p.lda + c0;
#pragma unroll
  for (int c = j0; c < 16 * CT; c += 4) sa[r * PMW_ALD + c] = (live && c0 + c < p.s) ? ar[c] : 0.0;
}

// One register sub-chunk: dimensions jb .. jb + 7 of the lane's two points, scaled on load (zeros past d), against the 16 rows
// row0 + 4 g of the staged chunk.  Every accumulator takes its dimensions in ascending order.
__device__ __forceinline__ void pmw_distances(const PmwParams& p, const double* const (&xt)[PMW_TP], int jb,
                                              const double* row0, double (&t2)[PMW_TP][PMW_NG]) {
  const int d = p.d;
  double y[PMW_TP][PMW_DR];
  {
    // plain products, as the Gram kernel stages its points: never fused into the subtractions below
#pragma clang fp contract(off)
    if (jb + PMW_DR <= d) {
#pragma unroll
      for (int u = 0; u < PMW_DR; ++u) {
        const double sc = p.scale[jb + u];
#pragma unroll
        for (int tp = 0; tp < PMW_TP; ++tp) y[tp][u] = sc * xt[tp][jb + u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < PMW_DR; ++u) {
        const bool in = jb + u < d;
        const double sc = in ? p.scale[jb + u] : 0.0;
#pragma unroll
        for (int tp = 0; tp < PMW_TP; ++tp) y[tp][u] = in ? sc * xt[tp][jb + u] : 0.0;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < PMW_DR; u += 2) {
#pragma unroll
    for (int g = 0; g < PMW_NG; ++g) {
      const d2 v = *reinterpret_cast<const d2*>(row0 + 4 * g * PMW_SXLD + u);
#pragma unroll
      for (int tp = 0; tp < PMW_TP; ++tp) {
        const double e0 = v[0] - y[tp][u];
        t2[tp][g] = fma(e0, e0, t2[tp][g]);
        const double e1 = v[1] - y[tp][u + 1];
        t2[tp][g] = fma(e1, e1, t2[tp][g]);
      }
    }
  }
}

template <int CT>
__global__ void __launch_bounds__(256, 2) pmw_contract_kernel(PmwParams p) {
  __shared__ __attribute__((aligned(16))) double sx[PMW_CH * PMW_SXLD];
  __shared__ double sa[PMW_CH * PMW_ALD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pt = lane & 15, kk = lane >> 4;
  const int d = p.d, m = p.m, s = p.s;
  const int t0 = blockIdx.x * PMW_TM + wave * 16 * PMW_TP;
  const int slice = blockIdx.y;
  const int c0 = blockIdx.z * PMW_CB;
  const double* xt[PMW_TP];
#pragma unroll
  for (int tp = 0; tp < PMW_TP; ++tp) xt[tp] = p.xt + (long)min(t0 + 16 * tp + pt, m - 1) * d;
  d4 acc[PMW_TP][CT];
#pragma unroll
  for (int tp = 0; tp < PMW_TP; ++tp)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[tp][ct] = d4{0.0, 0.0, 0.0, 0.0};
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  for (int ic = i0; ic < i1; ic += PMW_CH) {
    double t2[PMW_TP][PMW_NG];
#pragma unroll
    for (int tp = 0; tp < PMW_TP; ++tp)
#pragma unroll
      for (int g = 0; g < PMW_NG; ++g) t2[tp][g] = 0.0;
    for (int k0 = 0; k0 < d; k0 += PMW_DC) {
      __syncthreads();                   // the previous chunk (and, with k0 == 0, the previous rows of A) has been read
      pmw_stage_points(p, sx, ic, i1, k0);
      if (k0 == 0) pmw_stage_weights<CT>(p, sa, ic, i1, c0);
      __syncthreads();
      const int jend = min(d, k0 + PMW_DC);
#pragma unroll 1
      for (int jb = k0; jb < jend; jb += PMW_DR) pmw_distances(p, xt, jb, sx + kk * PMW_SXLD + (jb - k0), t2);
    }
    // the Matern tail in lock step over groups 2 b, 2 b + 1 of both point tiles, then their matrix instructions
#pragma unroll
    for (int b = 0; b < PMW_NG / 2; ++b) {
      const double tb[4] = {t2[0][2 * b], t2[1][2 * b], t2[0][2 * b + 1], t2[1][2 * b + 1]};
      double tt[4], e[4], kv[4];
      matern_lockstep(p.fe, p.qs, p.p, tb, tt, e, kv);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double* __restrict__ br = sa + (4 * (2 * b + h) + kk) * PMW_ALD + pt;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const double bv = br[16 * ct];
#pragma unroll
          for (int tp = 0; tp < PMW_TP; ++tp)
            acc[tp][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[2 * h + tp], bv, acc[tp][ct], 0, 0, 0);
        }
      }
    }
  }
  // C/D register r of lane l: row (l >> 4) + 4 r = prediction point, column l & 15
  double* __restrict__ out = slice > 0 ? p.part + (long)(slice - 1) * m * s : p.O;
  const long ldout = slice > 0 ? (long)s : p.ldo;
#pragma unroll
  for (int tp = 0; tp < PMW_TP; ++tp)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c = c0 + 16 * ct + pt;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + 16 * tp + 4 * r + kk;
        if (t < m && c < s) out[(long)t * ldout + c] = acc[tp][ct][r];
      }
    }
}

// One lane per output (t, c), columns fastest: the partial slices in their order, then slice 0 (the output itself), then the mean part.
__global__ void __launch_bounds__(256) pmw_finalize_kernel(PmwParams p) {
  const int s = p.s, q = p.q;
  const long total = (long)p.m * s;
  const double* __restrict__ part = p.part;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long t = idx / s;
    const int c = (int)(idx - t * s);
    double* dst = p.O + t * p.ldo + c;
    double v = 0.0;
#pragma unroll 4
    for (int k = 0; k + 1 < p.nslices; ++k) v += part[k * total + idx];
    v += *dst;
    for (int a = 0; a < q; ++a) v = fma(p.Pt[t * p.ldpt + a], p.B[(long)a * p.ldb + c], v);
    *dst = v;
  }
}

struct PmwLayout {
  size_t sxi, scale, part, total;
};
PmwLayout pmw_layout(int n, int m, int s, int d) {
  PmwLayout l;
  // partials bounded independently of the tile count, so that the query grows with n, m, s and d only
  const long by_rows = ((long)n + PMW_MIN_ROWS - 1) / PMW_MIN_ROWS;
  const long outs = (long)m * s;                   // <= 2^42; the product with by_rows - 1 is taken only where it stays below the cap
  const long part = by_rows - 1 > PMW_PART_CAP / outs ? PMW_PART_CAP : (by_rows - 1) * outs;
  WsCursor c;
  l.sxi = c.take((size_t)n * d);
  l.scale = c.take((size_t)d);
  l.part = c.take((size_t)(part > 0 ? part : 1));
  l.total = c.at;
  return l;
}

// observation points per slice: a multiple of the chunk, so that only a slice's last chunk is short
int pmw_rows_per_slice(int n, int m, int s) {
  const long wgs = (long)((m + PMW_TM - 1) / PMW_TM) * ((s + PMW_CB - 1) / PMW_CB);
  long ns = (PMW_TARGET_WGS + wgs - 1) / wgs;
  const long by_rows = ((long)n + PMW_MIN_ROWS - 1) / PMW_MIN_ROWS;
  const long by_cap = 1 + PMW_PART_CAP / ((long)m * s);
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  if (ns < 1) ns = 1;
  const long rows = ((long)n + ns - 1) / ns;
  return (int)((rows + PMW_CH - 1) / PMW_CH * PMW_CH);
}

// The scales into the workspace, the pre-pass, the contraction and the finalize kernel of one call (arguments checked).
int pmw_enqueue(const double* xi, const double* A, long lda, const double* xt, const double* Pt, long ldpt, const double* B, long ldb,
                int n, int m, int s, int d, int q, int p, const double* theta_host, int noise, double* ws, double* O, long ldo,
                hipStream_t st) {
  const MaternTheta th(theta_host, noise, p, d);
  const PmwLayout l = pmw_layout(n, m, s, d);
  PmwParams gp;
  std::memset(&gp, 0, sizeof(gp));
  gp.xi = xi;
  gp.sxi = ws + l.sxi;
  gp.scale = ws + l.scale;
  gp.A = A;
  gp.xt = xt;
  gp.O = O;
  gp.part = ws + l.part;
  gp.Pt = Pt;
  gp.B = B;
  gp.lda = lda;
  gp.ldo = ldo;
  gp.ldpt = ldpt;
  gp.ldb = ldb;
  gp.n = n;
  gp.m = m;
  gp.s = s;
  gp.d = d;
  gp.q = q;
  gp.p = p;
  gp.rows_per_slice = pmw_rows_per_slice(n, m, s);
  gp.nslices = (n + gp.rows_per_slice - 1) / gp.rows_per_slice;
  th.coefficients(gp.qs);
  fill_fast_exp(gp.fe);
  if (hipError_t e = stage_vector(th.scale_vector(true), ws + l.scale, st)) {
    set_error("HIP error %s staging the length scales", hipGetErrorString(e));
    return -100;
  }
  const long nd = (long)n * d;
  hipLaunchKernelGGL(scale_points_kernel<PmwParams>, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  const dim3 grid((m + PMW_TM - 1) / PMW_TM, gp.nslices, (s + PMW_CB - 1) / PMW_CB);
  switch (pmw_ct(s)) {
    case 1: hipLaunchKernelGGL(pmw_contract_kernel<1>, grid, dim3(256), 0, st, gp); break;
    case 2: hipLaunchKernelGGL(pmw_contract_kernel<2>, grid, dim3(256), 0, st, gp); break;
    case 3: hipLaunchKernelGGL(pmw_contract_kernel<3>, grid, dim3(256), 0, st, gp); break;
    default: hipLaunchKernelGGL(pmw_contract_kernel<4>, grid, dim3(256), 0, st, gp);
  }
  GPMP_HIP_TRY(hipGetLastError());
  if (gp.nslices > 1 || q > 0) {
    const long fin = ((long)m * s + 255) / 256;
    hipLaunchKernelGGL(pmw_finalize_kernel, dim3((unsigned)(fin < PMW_FIN_BLOCKS ? fin : PMW_FIN_BLOCKS)), dim3(256), 0, st, gp);
    GPMP_HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_posterior_mean_wide_ws_elems(int n, int m, int s, int d) {
  const bool ok = n >= 1 && n <= GPMP_MAX_EXTENT && m >= 1 && m <= GPMP_MAX_EXTENT && s >= 1 && s <= GPMP_MAX_COLUMNS && d >= 1 &&
                  d <= GPMP_MAX_DIM_WIDE;
  return ok ? pmw_layout(n, m, s, d).total : 0;
}

extern "C" int gpmp_posterior_mean_wide(const double* xi, const double* A, long lda, const double* xt, const double* Pt, long ldpt,
                                        const double* B, long ldb, int n, int m, int s, int d, int q, int p,
                                        const double* theta_host, int noise, double* ws, double* O_dev, long ldo,
                                        gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(A != nullptr, 2, "A is NULL");
  GPMP_ARG(xt != nullptr, 4, "xt is NULL");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 9, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 10, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(s >= 1 && s <= GPMP_MAX_COLUMNS, 11, "s outside [1, GPMP_MAX_COLUMNS]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 12, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(q >= 0 && q < GPMP_MAX_RANK, 13, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 14, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(lda >= s, 3, "lda < s");
  GPMP_ARG(q == 0 || (Pt != nullptr && ldpt >= q), 5, "Pt is NULL or ldpt < q");
  GPMP_ARG(q == 0 || (B != nullptr && ldb >= s), 7, "B is NULL or ldb < s");
  GPMP_ARG(theta_host != nullptr, 15, "theta is NULL");
  GPMP_ARG(ws != nullptr, 17, "ws is NULL");
  GPMP_ARG(O_dev != nullptr, 18, "O is NULL");
  GPMP_ARG(ldo >= s, 19, "ldo < s");
  return pmw_enqueue(xi, A, lda, xt, Pt, ldpt, B, ldb, n, m, s, d, q, p, theta_host, noise, ws, O_dev, ldo, as_stream(stream));
}
