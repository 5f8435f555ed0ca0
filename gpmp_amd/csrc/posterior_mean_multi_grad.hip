// Posterior mean AND its Jacobian for many observation columns from stored weights, matrix-free: with A (n x s) and B (q x s) from
// gpmp_posterior_weights_multi,
//   O[t][c]    = sum_i sigma^2 K_p(h_it) A[i][c] + sum_a Pt[t][a] B[a][c]                                  (m x s, ldo)
//   G[t][j][c] = sigma^2 rho_j^-2 sum_i S(h_it) (x_tj - x_ij) A[i][c] + sum_a B[a][c] J[(t q + a) d + j]   (m x d x s, ldg)
// S(h) = K_p'(h) / h; the gradient term of a coincident pair is 0 for every p (posterior_mean.hip's rule, its p = 0 convention).
// The outputs are d + 1 COMPONENTS per (point, column) -- component 0 the value, component 1 + j the gradient along dimension j --
// and every one of them is a contraction of the same column block of A with an n x m matrix that is never stored: its entries are
// the A operand of v_mfma_f64_16x16x4_f64, kv = sigma^2 K_p(h_it) for component 0 and w delta_j for component 1 + j, with
// w = sigma^2 S(h_it) / (2 c)^2 and delta_j the SCALED difference (2 c / rho_j) (x_tj - x_ij).  The B operand, the staged row of A,
// is shared by all components.
//
// Value bits.  Component 0 repeats posterior_mean_multi.hip (hence gram.hip, gram_kernel_v3) operation for operation: both points
// scaled by 2 c / rho_j before the subtraction (a plain product, never fused), the same sqrt / exp / Horner chain over sigma^2 q_k;
// the entry is the one gpmp_matern_gram(xi, xt) writes, bit for bit.
//
// Difference.  The gradient accumulates the scaled differences and the finalize kernel applies 2 c / rho_j ONCE (the single-column
// kernel accumulates x_tj - x_ij and applies the square): no unscaled copy of the chunk in LDS.  Both scaled points carry one
// rounding, so delta_j has the extra absolute error 2^-53 (2 c / rho_j) (|x_tj| + |x_ij|): relative to the term, 2^-53 (|x_tj| +
// |x_ij|) / |x_tj - x_ij|, which only matters for pairs closer than 1e-7 of their coordinates.  A coincident pair scales to the
// same bits and contributes an exact 0.
//
// Split.  A workgroup is 4 waves and owns 64 prediction points x one slice of the observations x one block of 16 CT columns x one
// BLOCK OF COMPONENTS (blockIdx.x / .y / .z, .z = column block x component blocks + component block).  With the operand map of
// posterior_mean_multi.hip lane l owns point l & 15 and observation 4 g + (l >> 4) of group g; it computes t^2, the square root,
// the fast exponential and both Horner chains (K_p and S) once per entry, PMG_IB = 4 groups in lock step, then issues the matrix
// instructions of the 4 groups x live components x CT column tiles, consecutive ones on different accumulators.  Every component
// block repeats the entry arithmetic (it needs all d dimensions); at 64 cycles per matrix instruction that is the smaller share
// (d = 8: 4 x 9 matrix instructions per group at CT = 4).  Accumulators are the scarce resource (8 architectural VGPRs per tile, -amdgpu-mfma-vgpr-form=1):
//
//   CT (s <= 16, 32, 48, more)          1     2     3     4
//   components per block, at most      12     8     5     4        (12 .. 16 accumulator tiles, 96 .. 128 VGPRs)
//
// The d + 1 components are dealt evenly over ceil((d + 1) / that) blocks (d = 8, CT = 4: 3 blocks of 3); a block skips the slots
// it does not use by a wave-uniform branch.  The scaled x_t of the lane's point lives in registers for d <= 8 and d <= 16 and in
// LDS (64 points, row stride d | 1) above; the scaled x_t of the block's own components is always in registers.  Observation
// points and rows of A are staged as in the value kernel: chunks of 32 scaled points (row stride d | 1) and their 16 CT columns
// of A (row stride 80).  VGPRs by (tier, CT), from the compiler's resource remarks (no scratch, no spill in any instance):
//
//   d <= 8 :  CT 1 .. 4   199  240  220  224      36 KB of LDS
//   d <= 16:  CT 1 .. 4   215  256  236  240      36 KB
//   d <= 64:  CT 1 .. 4   207  248  228  232      69 KB
//
// so two workgroups are resident per CU (two waves per SIMD).  Measured: the fp64 matrix instructions and the fp64
// vector pipe do not overlap here, a call costs about (component blocks) x (entry arithmetic) + (d + 1) CT matrix instructions.
//
// Edges (the value kernel's).  An observation row past the end of the slice is staged as the slice's last point with zero weights;
// a prediction row t >= m computes on point m - 1 and is not stored; columns c >= s are zeros in the B operand and are not stored;
// nothing beyond column s of a row of A, B, O or G is touched.
//
// Slices over i fill the machine when m is small: slice 0 writes O and G themselves (G still unscaled), slices k >= 1 a bounded
// partial buffer [k - 1][m][d + 1][s] in the workspace (at most 4 M doubles for both outputs together).  The finalize kernel -- one
// lane per (t, component, c) -- adds the slices in a fixed order, applies 2 c / rho_j and then the mean part.  No atomics: two
// calls on the same inputs give the same bits.  1 <= d <= GPMP_MAX_DIM (the length scales travel in the kernel arguments).
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int PMG_TM = 64;                 // prediction points per workgroup (16 per wave)
constexpr int PMG_IB = 4;                  // observation groups (of 4 points) in lock step
constexpr int PMG_CH = 32;                 // observation points per LDS chunk (two lock-step batches)
constexpr int PMG_ALD = 80;                // row stride of the staged rows of A
constexpr int PMG_SXLD = GPMP_MAX_DIM + 1; // row stride of the staged points, at most
constexpr int PMG_TARGET_WGS = 1024;       // workgroups a call is sliced towards (the value kernel's figure; not tuned)
constexpr int PMG_MIN_ROWS = 4 * PMG_CH;   // observation points per slice, at least
constexpr long PMG_PART_CAP = 1L << 22;    // doubles of partials (32 MB), value and gradient together
constexpr int PMG_FIN_BLOCKS = 1 << 16;    // workgroups of the finalize kernel, at most (it strides over the outputs)

constexpr int pmg_ct(int s) { return s <= 16 ? 1 : s <= 32 ? 2 : s <= 48 ? 3 : 4; }
constexpr int pmg_nc(int ct) { return ct == 1 ? 12 : ct == 2 ? 8 : ct == 3 ? 5 : 4; }

// (never written inside a kernel: one store into the by-value block and the compiler keeps a private copy of it in scratch memory)
struct PmgParams {
  const double* xi;              // n x d
  double* sxi;                   // n x d, scaled by 2 c / rho_j (workspace, written by the pre-pass)
  const double* A;               // n x s weights (lda)
  const double* xt;              // m x d
  double* O;                     // m x s (ldo): slice 0, then the result
  double* G;                     // m x d x s (ldg): slice 0 (unscaled), then the result
  double* part;                  // slices 1.. : [slice - 1][m][d + 1][s]
  const double* Pt;              // mean part (q > 0): m x q (ldpt)
  const double* B;               // q x s (ldb)
  const double* J;               // m x q x d
  long lda, ldo, ldg, ldpt, ldb;
  int n, m, s, d, q, rows_per_slice, nslices, p;
  int ncb, ncl;                  // component blocks; components per block (the last block may have fewer)
  double scale[GPMP_MAX_DIM];    // 2 c / rho_j
  double qs[GPMP_MAX_P + 1];     // sigma^2 q_k:  sigma^2 K_p(h) = exp(-t/2) sum_k qs[k] t^k, t = 2 c h
  double ss[GPMP_MAX_P + 1];     // sigma^2 s_k:  sigma^2 S(h) / (2c)^2 = exp(-t/2) sum_{k>=1} ss[k] t^(k-1)   (p >= 1)
  FastExp fe;
};

// the product of pm_scale_points_kernel (posterior_mean.hip): one rounding, as the Gram kernel stages its points
__global__ void pmg_scale_points_kernel(PmgParams p) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)p.n * p.d) return;
  p.sxi[idx] = p.scale[idx % p.d] * p.xi[idx];
}

// DT: dimensions of x_t held in registers (8, 16), or 0: x_t in LDS (any d <= GPMP_MAX_DIM)
template <int DT, int CT>
__global__ void __launch_bounds__(256) pmg_contract_kernel(PmgParams p) {
  constexpr bool YL = DT == 0;
  constexpr int NC = pmg_nc(CT);
  __shared__ double sx[PMG_CH * PMG_SXLD];
  __shared__ double sa[PMG_CH * PMG_ALD];
  __shared__ double sy[YL ? PMG_TM * PMG_SXLD : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pt = lane & 15, kk = lane >> 4;
  const int d = p.d, m = p.m, s = p.s, pdeg = p.p;
  const int sxld = d | 1;
  const int t0 = blockIdx.x * PMG_TM + wave * 16;
  const int slice = blockIdx.y;
  const int cb = blockIdx.z % p.ncb;
  const int c0 = (blockIdx.z / p.ncb) * (16 * CT);
  const int comp0 = cb * p.ncl;                       // first component of this block: 0 is the value, 1 + j dimension j
  const int nlive = min(p.ncl, d + 1 - comp0);        // (>= 1 by the choice of ncb)
  const int tc = min(t0 + pt, m - 1);
  const double* __restrict__ sxi = p.sxi;
  const double* __restrict__ A = p.A;
  const double* __restrict__ xt = p.xt + (long)tc * d;
  const long lda = p.lda;
  double ys[YL ? 1 : DT], yb[NC];
  int jb[NC];                                         // the dimension of slot k (wave-uniform; slot 0 of block 0 does not use it)
  {
    // plain products, as the Gram kernel stages its points: never fused into the subtractions below
#pragma clang fp contract(off)
    if constexpr (YL) {
      for (int e = tid; e < PMG_TM * d; e += 256) {
        const int r = e / d, j = e - r * d;
        sy[r * sxld + j] = p.scale[j] * p.xt[(long)min((int)blockIdx.x * PMG_TM + r, m - 1) * d + j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < DT; ++j) ys[j] = j < d ? p.scale[j] * xt[j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      jb[k] = min(max(comp0 + k - 1, 0), d - 1);
      yb[k] = p.scale[jb[k]] * xt[jb[k]];
    }
  }
  const double* yl = sy + (wave * 16 + pt) * sxld;
  d4 acc[NC * CT];
#pragma unroll
  for (int a = 0; a < NC * CT; ++a) acc[a] = d4{0.0, 0.0, 0.0, 0.0};
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  // staging roles: 8 threads per chunk row
  const int srow = tid >> 3, scol = tid & 7;
  for (int ic = i0; ic < i1; ic += PMG_CH) {
    __syncthreads();                     // the previous chunk has been read
    {
      const int i = ic + srow;
      const bool live = i < i1;
      const double* __restrict__ src = sxi + (long)(live ? i : i1 - 1) * d;
      for (int j = scol; j < d; j += 8) sx[srow * sxld + j] = src[j];
      const double* __restrict__ ar = A + (long)(live ? i : i1 - 1) * lda;
#pragma unroll
      for (int c = scol; c < 16 * CT; c += 8) sa[srow * PMG_ALD + c] = (live && c0 + c < s) ? ar[c0 + c] : 0.0;
    }
    __syncthreads();                     // (the first one also publishes sy)
#pragma unroll 1
    for (int h = 0; h < PMG_CH; h += 4 * PMG_IB) {
      if (ic + h >= i1) break;           // (wave-uniform: nothing but zero rows is left in this chunk)
      const double* sr[PMG_IB];
      double t2[PMG_IB];
#pragma unroll
      for (int b = 0; b < PMG_IB; ++b) {
        sr[b] = sx + (h + 4 * b + kk) * sxld;
        t2[b] = 0.0;
      }
      if constexpr (YL) {
#pragma unroll 4
        for (int j = 0; j < d; ++j) {
          const double yj = yl[j];
#pragma unroll
          for (int b = 0; b < PMG_IB; ++b) {
            const double sd = sr[b][j] - yj;
            t2[b] = fma(sd, sd, t2[b]);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < DT; ++j) {
          if (j < d) {
#pragma unroll
            for (int b = 0; b < PMG_IB; ++b) {
              const double sd = sr[b][j] - ys[j];
              t2[b] = fma(sd, sd, t2[b]);
            }
          }
        }
      }
      double tt[PMG_IB], e[PMG_IB], kv[PMG_IB], w[PMG_IB];
#pragma unroll
      for (int b = 0; b < PMG_IB; ++b) tt[b] = fast_sqrt_pos(t2[b], p.fe.tiny);
#pragma unroll
      for (int b = 0; b < PMG_IB; ++b) e[b] = fast_exp_neg_half(p.fe, tt[b]);
      const double qtop = p.qs[pdeg];
#pragma unroll
      for (int b = 0; b < PMG_IB; ++b) kv[b] = qtop;
      for (int k = pdeg - 1; k >= 0; --k) {
        const double qk = p.qs[k];
#pragma unroll
        for (int b = 0; b < PMG_IB; ++b) kv[b] = fma(kv[b], tt[b], qk);
      }
#pragma unroll
      for (int b = 0; b < PMG_IB; ++b) kv[b] = e[b] * kv[b];
      // w = sigma^2 S / (2 c)^2, as posterior_mean_kernel derives it
      if (pdeg == 0) {
#pragma unroll
        for (int b = 0; b < PMG_IB; ++b) w[b] = tt[b] > 0.0 ? -0.5 * kv[b] / tt[b] : 0.0;
      } else {
        const double stop = p.ss[pdeg];
#pragma unroll
        for (int b = 0; b < PMG_IB; ++b) w[b] = stop;
        for (int k = pdeg - 1; k >= 1; --k) {
          const double sk = p.ss[k];
#pragma unroll
          for (int b = 0; b < PMG_IB; ++b) w[b] = fma(w[b], tt[b], sk);
        }
#pragma unroll
        for (int b = 0; b < PMG_IB; ++b) w[b] *= e[b];
      }
#pragma unroll
      for (int b = 0; b < PMG_IB; ++b) {
        const double* __restrict__ br = sa + (h + 4 * b + kk) * PMG_ALD + pt;
        double bv[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) bv[ct] = br[16 * ct];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          if (k < nlive) {               // (wave-uniform)
            double av = w[b] * (yb[k] - sr[b][jb[k]]);
            if (k == 0 && comp0 == 0) av = kv[b];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
              acc[k * CT + ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[ct], acc[k * CT + ct], 0, 0, 0);
          }
        }
      }
    }
  }
  // C/D register r of lane l: row (l >> 4) + 4 r = prediction point, column l & 15
  const int d1 = d + 1;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    if (k < nlive) {
      const int comp = comp0 + k;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = c0 + 16 * ct + pt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = t0 + 4 * r + kk;
          if (t < m && c < s) {
            double* dst;
            if (slice > 0) dst = p.part + (((long)(slice - 1) * m + t) * d1 + comp) * s + c;
            else if (comp == 0) dst = p.O + (long)t * p.ldo + c;
            else dst = p.G + ((long)t * d + comp - 1) * p.ldg + c;
            *dst = acc[k * CT + ct][r];
          }
        }
      }
    }
  }
}

// One lane per output (t, component, c), columns fastest: the partial slices in their order, then slice 0 (the output itself), for
// a gradient component the factor 2 c / rho_j, then the mean part.
__global__ void __launch_bounds__(256) pmg_finalize_kernel(PmgParams p) {
  const int s = p.s, q = p.q, d = p.d, d1 = p.d + 1;
  const long total = (long)p.m * d1 * s;
  const double* __restrict__ part = p.part;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long tq = idx / s;
    const int c = (int)(idx - tq * s);
    const long t = tq / d1;
    const int comp = (int)(tq - t * d1);
    double* dst = comp == 0 ? p.O + t * p.ldo + c : p.G + (t * d + comp - 1) * p.ldg + c;
    double v = 0.0;
#pragma unroll 4
    for (int k = 0; k + 1 < p.nslices; ++k) v += part[k * total + idx];
    v += *dst;
    if (comp == 0) {
      for (int a = 0; a < q; ++a) v = fma(p.Pt[t * p.ldpt + a], p.B[(long)a * p.ldb + c], v);
    } else {
      const int j = comp - 1;
      v = p.scale[j] * v;
      for (int a = 0; a < q; ++a) v = fma(p.B[(long)a * p.ldb + c], p.J[(t * q + a) * d + j], v);
    }
    *dst = v;
  }
}

struct PmgLayout {
  size_t sxi, part, total;
};
PmgLayout pmg_layout(int n, int m, int s, int d) {
  PmgLayout l;
  // partials bounded independently of the tile count, so that the query grows with n, m, s and d only
  const long by_rows = ((long)n + PMG_MIN_ROWS - 1) / PMG_MIN_ROWS;
  const long outs = (long)m * s * (d + 1);         // <= 2^49; the product with by_rows - 1 is taken only where it stays below the cap
  const long part = by_rows - 1 > PMG_PART_CAP / outs ? PMG_PART_CAP : (by_rows - 1) * outs;
  WsCursor c;
  l.sxi = c.take((size_t)n * d);
  l.part = c.take((size_t)(part > 0 ? part : 1));
  l.total = c.at;
  return l;
}

// observation points per slice: a multiple of the LDS chunk, so that only a slice's last chunk is short
int pmg_rows_per_slice(int n, int m, int s, int d, int ncb) {
  const int cols = 16 * pmg_ct(s);
  const long wgs = (long)((m + PMG_TM - 1) / PMG_TM) * ((s + cols - 1) / cols) * ncb;
  long ns = (PMG_TARGET_WGS + wgs - 1) / wgs;
  const long by_rows = ((long)n + PMG_MIN_ROWS - 1) / PMG_MIN_ROWS;
  const long by_cap = 1 + PMG_PART_CAP / ((long)m * s * (d + 1));
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  if (ns < 1) ns = 1;
  const long rows = ((long)n + ns - 1) / ns;
  return (int)((rows + PMG_CH - 1) / PMG_CH * PMG_CH);
}

template <int DT>
void launch_tier(const PmgParams& gp, dim3 grid, hipStream_t st) {
  switch (pmg_ct(gp.s)) {
    case 1: hipLaunchKernelGGL((pmg_contract_kernel<DT, 1>), grid, dim3(256), 0, st, gp); break;
    case 2: hipLaunchKernelGGL((pmg_contract_kernel<DT, 2>), grid, dim3(256), 0, st, gp); break;
    case 3: hipLaunchKernelGGL((pmg_contract_kernel<DT, 3>), grid, dim3(256), 0, st, gp); break;
    default: hipLaunchKernelGGL((pmg_contract_kernel<DT, 4>), grid, dim3(256), 0, st, gp);
  }
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_posterior_mean_multi_grad_ws_elems(int n, int m, int s, int d) {
  if (n < 1 || n > GPMP_MAX_EXTENT || m < 1 || m > GPMP_MAX_EXTENT || s < 1 || s > GPMP_MAX_COLUMNS || d < 1 || d > GPMP_MAX_DIM) return 0;
  return pmg_layout(n, m, s, d).total;
}

extern "C" int gpmp_posterior_mean_multi_grad(const double* xi, const double* A, long lda, const double* xt, const double* Pt,
                                              long ldpt, const double* B, long ldb, const double* J, int n, int m, int s, int d,
                                              int q, int p, const double* theta_host, int noise, double* ws, double* O_dev,
                                              long ldo, double* G_dev, long ldg, gpmp_stream_t stream) {
  GPMP_ARG(xi != nullptr, 1, "xi is NULL");
  GPMP_ARG(A != nullptr, 2, "A is NULL");
  GPMP_ARG(xt != nullptr, 4, "xt is NULL");
  GPMP_ARG(n > 0 && n <= GPMP_MAX_EXTENT, 10, "n outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 11, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(s >= 1 && s <= GPMP_MAX_COLUMNS, 12, "s outside [1, GPMP_MAX_COLUMNS]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM, 13, "d outside [1, GPMP_MAX_DIM] (no wide-dimension variant of this kernel)");
  GPMP_ARG(q >= 0 && q < GPMP_MAX_RANK, 14, "q outside [0, GPMP_MAX_RANK - 1]");
  GPMP_ARG(p >= 0 && p <= GPMP_MAX_P, 15, "p outside [0, GPMP_MAX_P]");
  GPMP_ARG(lda >= s, 3, "lda < s");
  GPMP_ARG(q == 0 || (Pt != nullptr && ldpt >= q), 5, "Pt is NULL or ldpt < q");
  GPMP_ARG(q == 0 || (B != nullptr && ldb >= s), 7, "B is NULL or ldb < s");
  GPMP_ARG(q == 0 || J != nullptr, 9, "J is NULL with q > 0");
  GPMP_ARG(theta_host != nullptr, 16, "theta is NULL");
  GPMP_ARG(ws != nullptr, 18, "ws is NULL");
  GPMP_ARG(O_dev != nullptr, 19, "O is NULL");
  GPMP_ARG(ldo >= s, 20, "ldo < s");
  GPMP_ARG(G_dev != nullptr, 21, "G is NULL");
  GPMP_ARG(ldg >= s, 22, "ldg < s");
  hipStream_t st = as_stream(stream);
  const PmgLayout l = pmg_layout(n, m, s, d);
  const MaternTheta th(theta_host, noise, p, d);
  PmgParams gp;
  std::memset(&gp, 0, sizeof(gp));
  gp.xi = xi;
  gp.sxi = ws + l.sxi;
  gp.A = A;
  gp.xt = xt;
  gp.O = O_dev;
  gp.G = G_dev;
  gp.part = ws + l.part;
  gp.Pt = Pt;
  gp.B = B;
  gp.J = J;
  gp.lda = lda;
  gp.ldo = ldo;
  gp.ldg = ldg;
  gp.ldpt = ldpt;
  gp.ldb = ldb;
  gp.n = n;
  gp.m = m;
  gp.s = s;
  gp.d = d;
  gp.q = q;
  gp.p = p;
  // the d + 1 components dealt evenly over the fewest blocks the accumulators allow; no block is empty
  const int ct = pmg_ct(s), nc = pmg_nc(ct);
  gp.ncl = (d + 1 + (d + nc) / nc - 1) / ((d + nc) / nc);
  gp.ncb = (d + gp.ncl) / gp.ncl;
  gp.rows_per_slice = pmg_rows_per_slice(n, m, s, d, gp.ncb);
  gp.nslices = (n + gp.rows_per_slice - 1) / gp.rows_per_slice;
  th.scales(gp.scale, true);
  th.coefficients(gp.qs);
  for (int k = 0; k <= GPMP_MAX_P; ++k) gp.ss[k] = th.sigma2 * th.ms.s[k];
  fill_fast_exp(gp.fe);
  const long nd = (long)n * d;
  hipLaunchKernelGGL(pmg_scale_points_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  const dim3 grid((m + PMG_TM - 1) / PMG_TM, gp.nslices, (s + 16 * ct - 1) / (16 * ct) * gp.ncb);
  if (d <= 8) launch_tier<8>(gp, grid, st);
  else if (d <= 16) launch_tier<16>(gp, grid, st);
  else launch_tier<0>(gp, grid, st);
  GPMP_HIP_TRY(hipGetLastError());
  const long fin = ((long)m * s * (d + 1) + 255) / 256;
  hipLaunchKernelGGL(pmg_finalize_kernel, dim3((unsigned)(fin < PMG_FIN_BLOCKS ? fin : PMG_FIN_BLOCKS)), dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  return 0;
}
