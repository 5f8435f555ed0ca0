// Posterior mean for MANY observation columns from stored weights, matrix-free, with or without its Jacobian: with
// A = K^-1 (Z - P B) (n x s) and B (q x s) from gpmp_posterior_weights_multi,
//   O[t][c]    = sum_i sigma^2 K_p(h_it) A[i][c] + sum_a Pt[t][a] B[a][c]                                  (m x s, ldo)
//   G[t][j][c] = sigma^2 rho_j^-2 sum_i S(h_it) (x_tj - x_ij) A[i][c] + sum_a B[a][c] J[(t q + a) d + j]   (m x d x s, ldg)
// S(h) = K_p'(h) / h; the gradient term of a coincident pair is 0 for every p (posterior_mean.hip's rule, its p = 0 convention).
// gpmp_posterior_mean_multi computes O (ONE component per (point, column)), gpmp_posterior_mean_multi_grad O and G (d + 1
// COMPONENTS: component 0 the value, component 1 + j the gradient along dimension j).  Every component is a contraction of the same
// column block of A with an n x m matrix that is never stored: its entries are the A operand of v_mfma_f64_16x16x4_f64, evaluated
// ONCE per column block by the kernel's own VALU code, and the B operand, the staged row of A, is shared by all components.  One
// kernel template, one finalize kernel and one host set-up serve both entries, so component 0 of the gradient pass is the value
// entry's result by construction (bit for bit wherever both run the same number of slices).
//
// Value bits.  Per entry the arithmetic is posterior_mean.hip's (hence gram.hip's, gram_kernel_v3) operation for operation -- both
// points scaled by 2 c / rho_j BEFORE the subtraction (a plain product, never fused), the same sqrt / exp / Horner chain over
// sigma^2 q_k (matern_lockstep) -- so the entry kv is the one gpmp_matern_gram(xi, xt) writes, bit for bit, and O differs from
// G^T A only in the order of the sum.
//
// Split.  A workgroup is 4 waves and owns 64 prediction points, one slice of the observation points, one block of 16 CT columns and
// one block of components (blockIdx.x / .y / .z, .z = column block x component blocks + component block).  Wave w owns points
// 16 w .. 16 w + 15; with the operand map of gemm_f64.hip (A: lane l holds A[row l & 15][k l >> 4]) lane l evaluates the entry of
// point l & 15 and observation 4 g + (l >> 4) of group g, so one lane evaluates one entry per matrix instruction and no entry is
// evaluated twice in a workgroup.  Accumulator tiles are 16 points x 16 columns (8 VGPRs each, architectural: the library is built
// with -amdgpu-mfma-vgpr-form=1).  Four lanes of a wave need four different observation rows, so the workgroup stages chunks of
// PMM_CH = 32 scaled observation points (row stride d | 1 doubles: the four rows of a read fall into different banks) and the
// matching rows of A (16 CT columns, row stride 80: lanes l and l + 16 fall into different bank halves) in LDS; the B operand of
// tile ct is A[4 g + (l >> 4)][16 ct + (l & 15)].  PMM_IB = 4 groups (16 observation points) run in lock step through the distance
// / sqrt / exp / Horner chain, then their matrix instructions issue interleaved over the components and column tiles, so that
// consecutive instructions never wait for each other's accumulator.
//
// Edges.  An observation row past the end of the slice is staged as the slice's LAST point with its rows of A as zeros (a finite
// entry times 0, never a NaN); a prediction row t >= m computes on point m - 1 and is not stored; columns c >= s are zeros in the
// B operand and are not stored; nothing beyond column s of a row of A, B, O or G is touched (lda, ldb, ldo, ldg >= s).  CT is
// chosen per CALL (s <= 16, 32, 48: 1, 2, 3; else 4) and column blocks are 64 wide, so with s > 64 the last block runs all four
// tiles even where s % 64 <= 48 leaves some of them zero: up to three quarters of that block's matrix instructions and staging are
// spent on zeros (the entry arithmetic, the larger share of the value pass, is needed for the block's first column anyway).
//
// Slices over i fill the machine when m is small: slice 0 writes O and G themselves (G still unscaled), slices k >= 1 a bounded
// partial buffer [k - 1][m][components][s] in the workspace (at most 4 M doubles).  The finalize kernel -- one lane per
// (t, component, c) -- adds the slices in a fixed order, applies a gradient component's factor and then the mean part; a value call
// of one slice and q = 0 skips it.  No atomics: two calls on the same inputs give the same bits.  1 <= d <= GPMP_MAX_DIM (the
// length scales travel in the kernel arguments).
//
// The value instances (NC = 1) keep the lane's scaled x_t in registers (dimension tiers 4 / 8 / 16 / 32 / 64) and CT accumulator
// tiles; 1 .. 4 workgroups are resident per CU, by tier.
//
// The gradient instances add, per entry, w = sigma^2 S(h_it) / (2 c)^2 (matern_lockstep_w); the A operand of component 1 + j is
// w delta_j with delta_j the SCALED difference (2 c / rho_j) (x_tj - x_ij), and the finalize kernel applies 2 c / rho_j ONCE (the
// single-column kernel accumulates x_tj - x_ij and applies the square): no unscaled copy of the chunk in LDS.  Both scaled points
// carry one rounding, so delta_j has the extra absolute error 2^-53 (2 c / rho_j) (|x_tj| + |x_ij|): relative to the term, 2^-53
// (|x_tj| + |x_ij|) / |x_tj - x_ij|, which only matters for pairs closer than 1e-7 of their coordinates.  A coincident pair scales
// to the same bits and contributes an exact 0.  Every component block repeats the entry arithmetic (it needs all d dimensions); at
// 64 cycles per matrix instruction that is the smaller share (d = 8: 4 x 9 matrix instructions per group at CT = 4).  Accumulators
// are the scarce resource:
//
//   CT (s <= 16, 32, 48, more)          1     2     3     4
//   components per block, at most      12     8     5     4        (12 .. 16 accumulator tiles, 96 .. 128 VGPRs)
//
// The d + 1 components are dealt evenly over ceil((d + 1) / that) blocks (d = 8, CT = 4: 3 blocks of 3); a block skips the slots
// it does not use by a wave-uniform branch.  The scaled x_t of the lane's point lives in registers for d <= 8 and d <= 16 and in
// LDS (64 points, row stride d | 1) above; the scaled x_t of the block's own components is always in registers.  VGPRs by
// (tier, CT), from the compiler's resource remarks (no scratch, no spill in any instance):
//
//   value     d <= 4 :  CT 1 .. 4    58   68   80   88
//             d <= 8 :  CT 1 .. 4    66   76   88   96
//             d <= 16:  CT 1 .. 4    83   93  105  113
//             d <= 32:  CT 1 .. 4   115  125  139  145
//             d <= 64:  CT 1 .. 4   180  190  204  210     36 KB of LDS in every value instance
//   gradient  d <= 8 :  CT 1 .. 4   199  222  208  214      36 KB of LDS
//             d <= 16:  CT 1 .. 4   215  239  224  230      36 KB
//             d <= 64:  CT 1 .. 4   207  230  216  222      69 KB
//
// so two workgroups of a gradient instance are resident per CU (two waves per SIMD).  (Value, d <= 16, CT 4: 107 with the lines
// of matern_lockstep written out in the kernel -- the same operations in another block order after inlining; no other instance
// differs, and four workgroups are resident either way.)  Measured: the fp64 matrix instructions and the fp64 vector
// pipe do not overlap here, a gradient call costs about (component blocks) x (entry arithmetic) + (d + 1) CT matrix instructions.
#include "matern_device.h"

namespace gpmp {
namespace {

constexpr int PMM_TM = 64;                 // prediction points per workgroup (16 per wave)
constexpr int PMM_CB = 64;                 // columns per column block: 16 CT, and a second block exists only with CT = 4
constexpr int PMM_IB = 4;                  // observation groups (of 4 points) in lock step
constexpr int PMM_CH = 32;                 // observation points per LDS chunk (two lock-step batches)
constexpr int PMM_ALD = 80;                // row stride of the staged rows of A
constexpr int PMM_SXLD = GPMP_MAX_DIM + 1; // row stride of the staged points, at most
constexpr int PMM_TARGET_WGS = 1024;       // workgroups a call is sliced towards: a few per CU (1 .. 4 are resident, by tier); not tuned
constexpr int PMM_MIN_ROWS = 4 * PMM_CH;   // observation points per slice, at least
constexpr long PMM_PART_CAP = 1L << 22;    // doubles of partials (32 MB), all components together
constexpr int PMM_FIN_BLOCKS = 1 << 16;    // workgroups of the finalize kernel, at most (it strides over the outputs)

constexpr int pmm_ct(int s) { return s <= 16 ? 1 : s <= 32 ? 2 : s <= 48 ? 3 : 4; }
constexpr int pmm_nc(int ct) { return ct == 1 ? 12 : ct == 2 ? 8 : ct == 3 ? 5 : 4; }

// A value call leaves G, J, ldg and ss zero and has ncomp = ncb = ncl = 1.
// (never written inside a kernel: one store into the by-value block and the compiler keeps a private copy of it in scratch memory)
struct PmmParams {
  const double* xi;              // n x d
  double* sxi;                   // n x d, scaled by 2 c / rho_j (workspace, written by the pre-pass)
  const double* A;               // n x s weights (lda)
  const double* xt;              // m x d
  double* O;                     // m x s (ldo): slice 0, then the result
  double* G;                     // m x d x s (ldg): slice 0 (unscaled), then the result
  double* part;                  // slices 1.. : [slice - 1][m][ncomp][s]
  const double* Pt;              // mean part (q > 0): m x q (ldpt)
  const double* B;               // q x s (ldb)
  const double* J;               // m x q x d
  long lda, ldo, ldg, ldpt, ldb;
  int n, m, s, d, q, rows_per_slice, nslices, p;
  int ncomp;                     // components per (point, column): 1, or d + 1 with the gradient
  int ncb, ncl;                  // component blocks; components per block (the last block may have fewer)
  double scale[GPMP_MAX_DIM];    // 2 c / rho_j
  double qs[GPMP_MAX_P + 1];     // sigma^2 q_k:  sigma^2 K_p(h) = exp(-t/2) sum_k qs[k] t^k, t = 2 c h
  double ss[GPMP_MAX_P + 1];     // sigma^2 s_k:  sigma^2 S(h) / (2c)^2 = exp(-t/2) sum_{k>=1} ss[k] t^(k-1)   (p >= 1)
  FastExp fe;
};

// Chunk staging (between the two barriers of the chunk loop; 8 threads per chunk row): the scaled observation points ic .. ic + 31
// and columns c0 .. c0 + 16 CT - 1 of their rows of A.
template <int CT>
__device__ __forceinline__ void pmm_stage(const PmmParams& p, double* sx, double* sa, int ic, int i1, int c0) {
  const int srow = threadIdx.x >> 3, scol = threadIdx.x & 7;
  const int d = p.d, sxld = d | 1;
  const int i = ic + srow;
  const bool live = i < i1;
  const double* __restrict__ src = p.sxi + (long)(live ? i : i1 - 1) * d;
  for (int j = scol; j < d; j += 8) sx[srow * sxld + j] = src[j];
  const double* __restrict__ ar = p.A + (long)(live ? i : i1 - 1) * p.lda;
#pragma unroll
  for (int c = scol; c < 16 * CT; c += 8) sa[srow * PMM_ALD + c] = (live && c0 + c < p.s) ? ar[c0 + c] : 0.0;
}

// The entries of the lane's point and the staged rows sr[0 .. 3]: tt, e and kv of matern_lockstep.  The scaled point is ys (DT
// dimensions in registers, zeros past d) or, with DT = 0, the LDS row yl.
template <int DT>
__device__ __forceinline__ void pmm_entries(const PmmParams& p, const double* const (&sr)[PMM_IB], const double (&ys)[DT ? DT : 1],
                                            const double* yl, double (&tt)[PMM_IB], double (&e)[PMM_IB], double (&kv)[PMM_IB]) {
  const int d = p.d;
  double t2[PMM_IB];
#pragma unroll
  for (int b = 0; b < PMM_IB; ++b) t2[b] = 0.0;
  if constexpr (DT == 0) {
#pragma unroll 4
    for (int j = 0; j < d; ++j) {
      const double yj = yl[j];
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) {
        const double sd = sr[b][j] - yj;
        t2[b] = fma(sd, sd, t2[b]);
      }
    }
  } else {
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
  }
  matern_lockstep(p.fe, p.qs, p.p, t2, tt, e, kv);
}

// DT: dimensions of x_t held in registers, or 0: x_t in LDS (any d <= GPMP_MAX_DIM).  NC: component slots of a workgroup; NC = 1
// is the value instance, whose only component is component 0 (no w, no component blocks).
template <int DT, int CT, int NC>
__global__ void __launch_bounds__(256) pmm_contract_kernel(PmmParams p) {
  constexpr bool YL = DT == 0, GRAD = NC > 1;
  __shared__ double sx[PMM_CH * PMM_SXLD];
  __shared__ double sa[PMM_CH * PMM_ALD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pt = lane & 15, kk = lane >> 4;
  const int d = p.d, m = p.m, s = p.s;
  const int sxld = d | 1;
  const int t0 = blockIdx.x * PMM_TM + wave * 16;
  const int slice = blockIdx.y;
  const int c0 = (GRAD ? blockIdx.z / p.ncb : blockIdx.z) * PMM_CB;
  const int ncomp = GRAD ? d + 1 : 1;
  const int comp0 = GRAD ? blockIdx.z % p.ncb * p.ncl : 0;     // first component of this block: 0 is the value, 1 + j dimension j
  const int nlive = GRAD ? min(p.ncl, ncomp - comp0) : 1;      // (>= 1 by the choice of ncb)
  const int tc = min(t0 + pt, m - 1);
  const double* __restrict__ xt = p.xt + (long)tc * d;
  const double* yl = nullptr;
  double ys[YL ? 1 : DT], yb[NC];
  int jb[NC];                                                  // the dimension of slot k (wave-uniform; slot 0 of block 0 does not use it)
  {
    // plain products, as the Gram kernel stages its points: never fused into the subtractions below
#pragma clang fp contract(off)
    if constexpr (YL) {
      __shared__ double sy[PMM_TM * PMM_SXLD];                 // (published by the first barrier of the chunk loop)
      for (int e = tid; e < PMM_TM * d; e += 256) {
        const int r = e / d, j = e - r * d;
        sy[r * sxld + j] = p.scale[j] * p.xt[(long)min((int)blockIdx.x * PMM_TM + r, m - 1) * d + j];
      }
      yl = sy + (wave * 16 + pt) * sxld;
    } else {
#pragma unroll
      for (int j = 0; j < DT; ++j) ys[j] = j < d ? p.scale[j] * xt[j] : 0.0;
    }
    if constexpr (GRAD) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        jb[k] = min(max(comp0 + k - 1, 0), d - 1);
        yb[k] = p.scale[jb[k]] * xt[jb[k]];
      }
    }
  }
  d4 acc[NC * CT];
#pragma unroll
  for (int a = 0; a < NC * CT; ++a) acc[a] = d4{0.0, 0.0, 0.0, 0.0};
  const int i0 = slice * p.rows_per_slice;
  const int i1 = min(p.n, i0 + p.rows_per_slice);
  for (int ic = i0; ic < i1; ic += PMM_CH) {
    __syncthreads();                     // the previous chunk has been read
    pmm_stage<CT>(p, sx, sa, ic, i1, c0);
    __syncthreads();
#pragma unroll 1
    for (int h = 0; h < PMM_CH; h += 4 * PMM_IB) {
      if (ic + h >= i1) break;           // (wave-uniform: nothing but zero rows is left in this chunk)
      const double* sr[PMM_IB];
#pragma unroll
      for (int b = 0; b < PMM_IB; ++b) sr[b] = sx + (h + 4 * b + kk) * sxld;
      double tt[PMM_IB], e[PMM_IB], kv[PMM_IB];
      pmm_entries<DT>(p, sr, ys, yl, tt, e, kv);
      if constexpr (!GRAD) {
#pragma unroll
        for (int b = 0; b < PMM_IB; ++b) {
          const double* __restrict__ br = sa + (h + 4 * b + kk) * PMM_ALD + pt;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[b], br[16 * ct], acc[ct], 0, 0, 0);
        }
      } else {
        double w[PMM_IB];
        matern_lockstep_w(p.ss, p.p, tt, e, kv, w);
#pragma unroll
        for (int b = 0; b < PMM_IB; ++b) {
          const double* __restrict__ br = sa + (h + 4 * b + kk) * PMM_ALD + pt;
          double bv[CT];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) bv[ct] = br[16 * ct];
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            if (k < nlive) {             // (wave-uniform)
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
  }
  // C/D register r of lane l: row (l >> 4) + 4 r = prediction point, column l & 15
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    if (k < nlive) {
      const int comp = comp0 + k;
      // row t of this component: part[slice - 1][t][comp], O[t] or G[t][comp - 1]
      double* __restrict__ out = slice > 0   ? p.part + ((long)(slice - 1) * m * ncomp + comp) * s
                                 : comp == 0 ? p.O
                                             : p.G + (comp - 1) * p.ldg;
      const long ldout = slice > 0 ? (long)ncomp * s : comp == 0 ? p.ldo : d * p.ldg;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = c0 + 16 * ct + pt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = t0 + 4 * r + kk;
          if (t < m && c < s) out[(long)t * ldout + c] = acc[k * CT + ct][r];
        }
      }
    }
  }
}

// One lane per output (t, component, c), columns fastest: the partial slices in their order, then slice 0 (the output itself), for
// a gradient component the factor 2 c / rho_j, then the mean part.
__global__ void __launch_bounds__(256) pmm_finalize_kernel(PmmParams p) {
  const int s = p.s, q = p.q, d = p.d, nco = p.ncomp;
  const long total = (long)p.m * nco * s;
  const double* __restrict__ part = p.part;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long tq = idx / s;
    const int c = (int)(idx - tq * s);
    const long t = tq / nco;
    const int comp = (int)(tq - t * nco);
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

struct PmmLayout {
  size_t sxi, part, total;
};
PmmLayout pmm_layout(int n, int m, int s, int d, int ncomp) {
  PmmLayout l;
  // partials bounded independently of the tile count, so that the query grows with n, m, s and d only
  const long by_rows = ((long)n + PMM_MIN_ROWS - 1) / PMM_MIN_ROWS;
  const long outs = (long)m * s * ncomp;           // <= 2^49; the product with by_rows - 1 is taken only where it stays below the cap
  const long part = by_rows - 1 > PMM_PART_CAP / outs ? PMM_PART_CAP : (by_rows - 1) * outs;
  WsCursor c;
  l.sxi = c.take((size_t)n * d);
  l.part = c.take((size_t)(part > 0 ? part : 1));
  l.total = c.at;
  return l;
}

// observation points per slice: a multiple of the LDS chunk, so that only a slice's last chunk is short
int pmm_rows_per_slice(int n, int m, int s, int ncomp, int ncb) {
  const long wgs = (long)((m + PMM_TM - 1) / PMM_TM) * ((s + PMM_CB - 1) / PMM_CB) * ncb;
  long ns = (PMM_TARGET_WGS + wgs - 1) / wgs;
  const long by_rows = ((long)n + PMM_MIN_ROWS - 1) / PMM_MIN_ROWS;
  const long by_cap = 1 + PMM_PART_CAP / ((long)m * s * ncomp);
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  if (ns < 1) ns = 1;
  const long rows = ((long)n + ns - 1) / ns;
  return (int)((rows + PMM_CH - 1) / PMM_CH * PMM_CH);
}

// The parameter block of either entry from its (checked) arguments; G == NULL is the value call.
PmmParams pmm_setup(const double* xi, const double* A, long lda, const double* xt, const double* Pt, long ldpt, const double* B,
                    long ldb, const double* J, int n, int m, int s, int d, int q, int p, const double* theta_host, int noise,
                    double* ws, double* O, long ldo, double* G, long ldg) {
  const MaternTheta th(theta_host, noise, p, d);
  PmmParams gp;
  std::memset(&gp, 0, sizeof(gp));
  gp.ncomp = G != nullptr ? d + 1 : 1;
  const PmmLayout l = pmm_layout(n, m, s, d, gp.ncomp);
  gp.xi = xi;
  gp.sxi = ws + l.sxi;
  gp.A = A;
  gp.xt = xt;
  gp.O = O;
  gp.G = G;
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
  // the components dealt evenly over the fewest blocks the accumulators allow; no block is empty
  const int nc = G != nullptr ? pmm_nc(pmm_ct(s)) : 1, blocks = (gp.ncomp + nc - 1) / nc;
  gp.ncl = (gp.ncomp + blocks - 1) / blocks;
  gp.ncb = (gp.ncomp + gp.ncl - 1) / gp.ncl;
  gp.rows_per_slice = pmm_rows_per_slice(n, m, s, gp.ncomp, gp.ncb);
  gp.nslices = (n + gp.rows_per_slice - 1) / gp.rows_per_slice;
  th.scales(gp.scale, true);
  th.coefficients(gp.qs);
  if (G != nullptr)
    for (int k = 0; k <= GPMP_MAX_P; ++k) gp.ss[k] = th.sigma2 * th.ms.s[k];
  fill_fast_exp(gp.fe);
  return gp;
}

template <int DT, bool GRAD>
void launch_tier(const PmmParams& gp, dim3 grid, hipStream_t st) {
  switch (pmm_ct(gp.s)) {
    case 1: hipLaunchKernelGGL((pmm_contract_kernel<DT, 1, GRAD ? pmm_nc(1) : 1>), grid, dim3(256), 0, st, gp); break;
    case 2: hipLaunchKernelGGL((pmm_contract_kernel<DT, 2, GRAD ? pmm_nc(2) : 1>), grid, dim3(256), 0, st, gp); break;
    case 3: hipLaunchKernelGGL((pmm_contract_kernel<DT, 3, GRAD ? pmm_nc(3) : 1>), grid, dim3(256), 0, st, gp); break;
    default: hipLaunchKernelGGL((pmm_contract_kernel<DT, 4, GRAD ? pmm_nc(4) : 1>), grid, dim3(256), 0, st, gp);
  }
}

// The pre-pass, the contraction and the finalize kernel of one call.
int pmm_enqueue(const PmmParams& gp, hipStream_t st) {
  const int d = gp.d;
  const long nd = (long)gp.n * d;
  hipLaunchKernelGGL(scale_points_kernel<PmmParams>, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, gp);
  GPMP_HIP_TRY(hipGetLastError());
  const dim3 grid((gp.m + PMM_TM - 1) / PMM_TM, gp.nslices, (gp.s + PMM_CB - 1) / PMM_CB * gp.ncb);
  if (gp.G == nullptr) {
    if (d <= 4) launch_tier<4, false>(gp, grid, st);
    else if (d <= 8) launch_tier<8, false>(gp, grid, st);
    else if (d <= 16) launch_tier<16, false>(gp, grid, st);
    else if (d <= 32) launch_tier<32, false>(gp, grid, st);
    else launch_tier<GPMP_MAX_DIM, false>(gp, grid, st);
  } else {
    if (d <= 8) launch_tier<8, true>(gp, grid, st);
    else if (d <= 16) launch_tier<16, true>(gp, grid, st);
    else launch_tier<0, true>(gp, grid, st);
  }
  GPMP_HIP_TRY(hipGetLastError());
  if (gp.G != nullptr || gp.nslices > 1 || gp.q > 0) {
    const long fin = ((long)gp.m * gp.s * gp.ncomp + 255) / 256;
    hipLaunchKernelGGL(pmm_finalize_kernel, dim3((unsigned)(fin < PMM_FIN_BLOCKS ? fin : PMM_FIN_BLOCKS)), dim3(256), 0, st, gp);
    GPMP_HIP_TRY(hipGetLastError());
  }
  return 0;
}

bool pmm_in_range(int n, int m, int s, int d) {
  return n >= 1 && n <= GPMP_MAX_EXTENT && m >= 1 && m <= GPMP_MAX_EXTENT && s >= 1 && s <= GPMP_MAX_COLUMNS && d >= 1 && d <= GPMP_MAX_DIM;
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_posterior_mean_multi_ws_elems(int n, int m, int s, int d) {
  return pmm_in_range(n, m, s, d) ? pmm_layout(n, m, s, d, 1).total : 0;
}

extern "C" size_t gpmp_posterior_mean_multi_grad_ws_elems(int n, int m, int s, int d) {
  return pmm_in_range(n, m, s, d) ? pmm_layout(n, m, s, d, d + 1).total : 0;
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
  return pmm_enqueue(pmm_setup(xi, A, lda, xt, Pt, ldpt, B, ldb, nullptr, n, m, s, d, q, p, theta_host, noise, ws, O_dev, ldo, nullptr, 0),
                     as_stream(stream));
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
  return pmm_enqueue(pmm_setup(xi, A, lda, xt, Pt, ldpt, B, ldb, J, n, m, s, d, q, p, theta_host, noise, ws, O_dev, ldo, G_dev, ldg),
                     as_stream(stream));
}
