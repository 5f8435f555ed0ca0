// Posterior mean for MANY observation columns from stored weights, matrix-free: with A = K^-1 (Z - P B) (n x s) and B (q x s) from
// gpmp_posterior_weights_multi,
//   O[t][c] = sum_i sigma^2 K_p(h_it) A[i][c] + sum_a Pt[t][a] B[a][c],        t < m, c < s
// Every entry sigma^2 K_p(h_it) is evaluated ONCE per block of up to 64 columns and contracted against all of them by
// v_mfma_f64_16x16x4_f64: the kernel's own VALU output is the A operand of the matrix instruction.  No n x m block is stored.
//
// Per entry the arithmetic is posterior_mean.hip's (hence gram.hip's, gram_kernel_v3) operation for operation -- both points
// scaled by 2 c / rho_j BEFORE the subtraction (a plain product, never fused), the same sqrt / exp / Horner chain over sigma^2 q_k
// -- so the entry is the one gpmp_matern_gram(xi, xt) writes, bit for bit, and O differs from G^T A only in the order of the sum.
//
// Split.  A workgroup is 4 waves and owns 64 prediction points, one slice of the observation points and one block of up to 64
// columns (blockIdx.x / .y / .z).  Wave w owns points 16 w .. 16 w + 15; with the operand map of gemm_f64.hip (A: lane l holds
// A[row l & 15][k l >> 4]) lane l evaluates the entry of point l & 15 and observation 4 g + (l >> 4) of group g, so one lane
// evaluates one entry per matrix instruction and no entry is evaluated twice in a workgroup.  The lane keeps its scaled x_t in
// registers (dimension tiers 4 / 8 / 16 / 32 / 64) and CT = 1 .. 4 accumulator tiles of 16 points x 16 columns (8 VGPRs each,
// architectural: the library is built with -amdgpu-mfma-vgpr-form=1).  Four lanes of a wave need four different observation rows,
// so the workgroup stages chunks of PMM_CH = 32 scaled observation points (row stride d | 1 doubles: the four rows of a read fall
// into different banks) and the matching rows of A (64 columns, row stride 80: lanes l and l + 16 fall into different bank
// halves) in LDS; the B operand of tile ct is A[4 g + (l >> 4)][16 ct + (l & 15)].  PMM_IB = 4 groups (16 observation points)
// run in lock step through the distance / sqrt / exp / Horner chain, then their 4 CT matrix instructions issue interleaved over
// the column tiles, so that consecutive instructions never wait for each other's accumulator.
//
// Edges.  An observation row past the end of the slice is staged as the slice's LAST point with its rows of A as zeros (a finite
// entry times 0, never a NaN); a prediction row t >= m computes on point m - 1 and is not stored; columns c >= s are zeros in the
// B operand and are not stored; nothing beyond column s of a row of A or O is touched (lda, ldo >= s).  CT is chosen per CALL
// (s <= 16, 32, 48: 1, 2, 3; else 4) and blockIdx.z walks blocks of 64 columns, so with s > 64 the last block runs all four tiles
// even where s % 64 <= 48 leaves some of them zero: up to three quarters of that block's matrix instructions and staging are
// spent on zeros (the entry arithmetic, the larger share, is needed for the block's first column anyway).
//
// Slices over i fill the machine when m is small: slice 0 writes O itself, slices k >= 1 a bounded partial buffer in the
// workspace; the finalize kernel adds the slices in a fixed order and then the mean part.  No atomics: two runs on the same
// inputs are bit-identical.  Value only; 1 <= d <= GPMP_MAX_DIM (the length scales travel in the kernel arguments).
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int PMM_TM = 64;                 // prediction points per workgroup (16 per wave)
constexpr int PMM_CB = 64;                 // columns per workgroup, at most (4 tiles of 16)
constexpr int PMM_IB = 4;                  // observation groups (of 4 points) in lock step
constexpr int PMM_CH = 32;                 // observation points per LDS chunk (two lock-step batches)
constexpr int PMM_ALD = 80;                // row stride of the staged rows of A
constexpr int PMM_SXLD = GPMP_MAX_DIM + 1; // row stride of the staged points, at most
constexpr int PMM_TARGET_WGS = 1024;       // workgroups a call is sliced towards: a few per CU (1 .. 4 are resident, by tier); not tuned
constexpr int PMM_MIN_ROWS = 4 * PMM_CH;   // observation points per slice, at least
constexpr long PMM_PART_CAP = 1L << 22;    // doubles of partials (32 MB)

// (never written inside a kernel: one store into the by-value block and the compiler keeps a private copy of it in scratch memory)
struct PmmParams {
  const double* xi;              // n x d
  double* sxi;                   // n x d, scaled by 2 c / rho_j (workspace, written by the pre-pass)
  const double* A;               // n x s weights (lda)
  const double* xt;              // m x d
  double* O;                     // m x s (ldo): slice 0, then the result
  double* part;                  // slices 1.. : [slice - 1][m][s]
  const double* Pt;              // mean part (q > 0): m x q (ldpt)
  const double* B;               // q x s (ldb)
  long lda, ldo, ldpt, ldb;
  int n, m, s, d, q, rows_per_slice, nslices, p;
  double scale[GPMP_MAX_DIM];    // 2 c / rho_j
  double qs[GPMP_MAX_P + 1];     // sigma^2 q_k:  sigma^2 K_p(h) = exp(-t/2) sum_k qs[k] t^k, t = 2 c h
  FastExp fe;
};

// the product of pm_scale_points_kernel (posterior_mean.hip): one rounding, as the Gram kernel stages its points
__global__ void pmm_scale_points_kernel(PmmParams p) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)p.n * p.d) return;
  p.sxi[idx] = p.scale[idx % p.d] * p.xi[idx];
}

template <int DT, int CT>
__global__ void __launch_bounds__(256) pmm_contract_kernel(PmmParams p) {
  __shared__ double sx[PMM_CH * PMM_SXLD];
  __shared__ double sa[PMM_CH * PMM_ALD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pt = lane & 15, kk = lane >> 4;
  const int d = p.d, m = p.m, s = p.s, pdeg = p.p;
  const int sxld = d | 1;
  const int t0 = blockIdx.x * PMM_TM + wave * 16;
  const int slice = blockIdx.y;
  const int c0 = blockIdx.z * PMM_CB;
  const int tc = min(t0 + pt, m - 1);
  const double* __restrict__ sxi = p.sxi;
  const double* __restrict__ A = p.A;
  const double* __restrict__ xt = p.xt + (long)tc * d;
  const long lda = p.lda;
  double ys[DT];
  {
    // a plain product, as the Gram kernel stages its points: never fused into the subtraction below
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < DT; ++j) ys[j] = j < d ? p.scale[j] * xt[j] : 0.0;
  }
  d4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = d4{0.0, 0.0, 0.0, 0.0};
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  // staging roles: 8 threads per chunk row
  const int srow = tid >> 3, scol = tid & 7;
  for (int ic = i0; ic < i1; ic += PMM_CH) {
    __syncthreads();                     // the previous chunk has been read
    {
      const int i = ic + srow;
      const bool live = i < i1;
      const double* __restrict__ src = sxi + (long)(live ? i : i1 - 1) * d;
      for (int j = scol; j < d; j += 8) sx[srow * sxld + j] = src[j];
      const double* __restrict__ ar = A + (long)(live ? i : i1 - 1) * lda;
#pragma unroll
      for (int c = scol; c < 16 * CT; c += 8) sa[srow * PMM_ALD + c] = (live && c0 + c < s) ? ar[c0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int h = 0; h < PMM_CH; h += 4 * PMM_IB) {
      if (ic + h >= i1) break;           // (wave-uniform: nothing but zero rows is left in this chunk)
      const double* sr[PMM_IB];
      double t2[PMM_IB];
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) {
        sr[b] = sx + (h + 4 * b + kk) * sxld;
        t2[b] = 0.0;
      }
#pragma unroll
      for (int j = 0; j < DT; ++j) {
        if (j < d) {
#pragma unroll
          for (int b = 0; b < PMM_IB; ++b) {
            const double sd = sr[b][j] - ys[j];
            t2[b] = fma(sd, sd, t2[b]);
          }
        }
      }
      double tt[PMM_IB], e[PMM_IB], poly[PMM_IB];
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) tt[b] = fast_sqrt_pos(t2[b], p.fe.tiny);
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) e[b] = fast_exp_neg_half(p.fe, tt[b]);
      const double qtop = p.qs[pdeg];
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) poly[b] = qtop;
      for (int k = pdeg - 1; k >= 0; --k) {
        const double qk = p.qs[k];
#pragma unroll
        for (int b = 0; b < PMM_IB; ++b) poly[b] = fma(poly[b], tt[b], qk);
      }
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) {
        const double kv = e[b] * poly[b];
        const double* __restrict__ br = sa + (h + 4 * b + kk) * PMM_ALD + pt;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv, br[16 * ct], acc[ct], 0, 0, 0);
      }
    }
  }
  // C/D register r of lane l: row (l >> 4) + 4 r = prediction point, column l & 15
  double* __restrict__ out = slice == 0 ? p.O : p.part + (long)(slice - 1) * m * s;
  const long ldout = slice == 0 ? p.ldo : (long)s;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int c = c0 + 16 * ct + pt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = t0 + 4 * r + kk;
      if (t < m && c < s) out[(long)t * ldout + c] = acc[ct][r];
    }
  }
}

// One lane per output: the partial slices in their order, then slice 0 (O itself), then the mean part.
__global__ void __launch_bounds__(256) pmm_finalize_kernel(PmmParams p) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int s = p.s, q = p.q;
  if (idx >= (long)p.m * s) return;
  const long t = idx / s;
  const int c = (int)(idx - t * s);
  const double* __restrict__ part = p.part;
  const long stride = (long)p.m * s;
  double v = 0.0;
#pragma unroll 4
  for (int k = 0; k + 1 < p.nslices; ++k) v += part[k * stride + idx];
  v += p.O[t * p.ldo + c];
  for (int a = 0; a < q; ++a) v = fma(p.Pt[t * p.ldpt + a], p.B[(long)a * p.ldb + c], v);
  p.O[t * p.ldo + c] = v;
}

struct PmmLayout {
  size_t sxi, part, total;
};
PmmLayout pmm_layout(int n, int m, int s, int d) {
  PmmLayout l;
  // partials bounded independently of the tile count, so that the query grows with n, m, s and d only
  const long by_rows = ((long)n + PMM_MIN_ROWS - 1) / PMM_MIN_ROWS;
  const long ms = (long)m * s;                   // <= 2^42; the product with by_rows - 1 is taken only where it stays below the cap
  const long part = by_rows - 1 > PMM_PART_CAP / ms ? PMM_PART_CAP : (by_rows - 1) * ms;
  WsCursor c;
  l.sxi = c.take((size_t)n * d);
  l.part = c.take((size_t)(part > 0 ? part : 1));
  l.total = c.at;
  return l;
}

// observation points per slice: a multiple of the LDS chunk, so that only a slice's last chunk is short
int pmm_rows_per_slice(int n, int m, int s) {
  const long wgs = (long)((m + PMM_TM - 1) / PMM_TM) * ((s + PMM_CB - 1) / PMM_CB);
  long ns = (PMM_TARGET_WGS + wgs - 1) / wgs;
  const long by_rows = ((long)n + PMM_MIN_ROWS - 1) / PMM_MIN_ROWS;
  const long by_cap = 1 + PMM_PART_CAP / ((long)m * s);
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  if (ns < 1) ns = 1;
  const long rows = ((long)n + ns - 1) / ns;
  return (int)((rows + PMM_CH - 1) / PMM_CH * PMM_CH);
}

template <int DT>
void launch_tier(const PmmParams& gp, dim3 grid, hipStream_t st) {
  if (gp.s <= 16) hipLaunchKernelGGL((pmm_contract_kernel<DT, 1>), grid, dim3(256), 0, st, gp);
  else if (gp.s <= 32) hipLaunchKernelGGL((pmm_contract_kernel<DT, 2>), grid, dim3(256), 0, st, gp);
  else if (gp.s <= 48) hipLaunchKernelGGL((pmm_contract_kernel<DT, 3>), grid, dim3(256), 0, st, gp);
  else hipLaunchKernelGGL((pmm_contract_kernel<DT, 4>), grid, dim3(256), 0, st, gp);
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_posterior_mean_multi_ws_elems(int n, int m, int s, int d) {
  if (n < 1 || n > GPMP_MAX_EXTENT || m < 1 || m > GPMP_MAX_EXTENT || s < 1 || s > GPMP_MAX_COLUMNS || d < 1 || d > GPMP_MAX_DIM) return 0;
  return pmm_layout(n, m, s, d).total;
}

extern "C" int gpmp_posterior_mean_multi(const double* xi, const double* A, long lda, const double* xt, const double* Pt, long ldpt,
                                         const double* B, long ldb, int n, int m, int s, int d, int q, int p,
                                         const double* theta_host, int noise, double* ws, double* O_dev, long ldo,
                                         gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(A != nullptr, 2, "A is NULL");
  GPMP_ARG(xt != nullptr, 4, "xt is NULL");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 9, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 10, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(s >= 1 && s <= GPMP_MAX_COLUMNS, 11, "s outside [1, GPMP_MAX_COLUMNS]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM, 12, "d outside [1, GPMP_MAX_DIM] (no wide-dimension variant of this kernel)");
  GPMP_ARG(q >= 0 && q < GPMP_MAX_RANK, 13, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 14, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(lda >= s, 3, "lda < s");
  GPMP_ARG(q == 0 || (Pt != nullptr && ldpt >= q), 5, "Pt is NULL or ldpt < q");
  GPMP_ARG(q == 0 || (B != nullptr && ldb >= s), 7, "B is NULL or ldb < s");
  GPMP_ARG(theta_host != nullptr, 15, "theta is NULL");
  GPMP_ARG(ws != nullptr, 17, "ws is NULL");
  GPMP_ARG(O_dev != nullptr, 18, "O is NULL");
  GPMP_ARG(ldo >= s, 19, "ldo < s");
  hipStream_t st = as_stream(stream);
  const PmmLayout l = pmm_layout(n, m, s, d);
  const MaternTheta th(theta_host, noise, p, d);
  PmmParams gp;
  std::memset(&gp, 0, sizeof(gp));
  gp.xi = xi;
  gp.sxi = ws + l.sxi;
  gp.A = A;
  gp.xt = xt;
  gp.O = O_dev;
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
  gp.rows_per_slice = pmm_rows_per_slice(n, m, s);
  gp.nslices = (n + gp.rows_per_slice - 1) / gp.rows_per_slice;
  gp.p = p;
  th.scales(gp.scale, true);
  th.coefficients(gp.qs);
  fill_fast_exp(gp.fe);
  const long nd = (long)n * d;
  hipLaunchKernelGGL(pmm_scale_points_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  const dim3 grid((m + PMM_TM - 1) / PMM_TM, gp.nslices, (s + PMM_CB - 1) / PMM_CB);
  if (d <= 4) launch_tier<4>(gp, grid, st);
  else if (d <= 8) launch_tier<8>(gp, grid, st);
  else if (d <= 16) launch_tier<16>(gp, grid, st);
  else if (d <= 32) launch_tier<32>(gp, grid, st);
  else launch_tier<GPMP_MAX_DIM>(gp, grid, st);
  GPMP_HIP_TRY(hipGetLastError());
  if (gp.nslices > 1 || q > 0) {
    const long outs = (long)m * s;
    hipLaunchKernelGGL(pmm_finalize_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, gp);
    GPMP_HIP_TRY(hipGetLastError());
  }
  return 0;
}
