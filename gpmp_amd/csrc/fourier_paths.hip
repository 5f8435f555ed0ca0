// Function-space sample paths: s random trigonometric sums over r features evaluated at m points in ONE launch,
//   out[t][c] = sum_{k<r} cos(2 pi (sum_{j<d} xt[t][j] omega[k][j] + phase[k])) W[k][c]                          (m x s, ldo)
// with frequencies and phases in TURNS.  The m x r block of features cos(2 pi u_tk) is never stored: every 16 x 16 tile of it is
// born in the accumulator registers of one matrix product, turned into cosines there and consumed from the same registers as an
// operand of the next product.  1 <= d <= GPMP_MAX_DIM_WIDE (d is streamed), 1 <= s <= GPMP_MAX_COLUMNS.
//
// The two products.  v_mfma_f64_16x16x4_f64 (operand map of gemm_f64.hip): A lane l holds A[row l & 15][k l >> 4], B lane l holds
// B[k l >> 4][column l & 15], C/D register q of lane l is C[row (l >> 4) + 4 q][column l & 15].  The PHASE product is taken
// transposed, U^T = Omega X^T + phase 1^T: features are the rows (A operand: the staged rows of Omega), points the columns (B
// operand: the staged points), and the initial accumulator of register q is phase[4 q + (l >> 4)] in every column.  Register q of
// lane l then holds u of feature 4 q + (l >> 4) and point l & 15 -- which is the A-operand layout of a product with the POINTS as
// rows and the four features 4 q .. 4 q + 3 as its k-group.  So after the cosine, register q is directly the A operand of the q-th
// CONTRACTION instruction of the tile, whose B operand is W[4 q + (l >> 4)][column l & 15] from the staged rows of W: a 16 x 16
// tile of features costs ceil(d / 4) + 4 CT matrix instructions and four cosines per lane, and no lane ever moves a feature.
//
// Split.  A workgroup is 4 waves and owns FP_TM = 128 points, one slice of the features and one block of 16 CT columns
// (blockIdx.x / .y / .z).  Wave w owns the two point tiles 32 w .. 32 w + 15 and 32 w + 16 .. 32 w + 31 and keeps 2 x CT output
// accumulator tiles for the whole slice.  Features pass in chunks of FP_FC = 32 (two feature tiles): 2 x 2 phase tiles per wave.
//
// Data movement.  Per feature chunk the workgroup stages the 32 rows of Omega in LDS in chunks of FP_DC = 32 dimensions (row
// stride 34 doubles: the 16 rows x 2 k of a half-wave read fall into 32 different double-wide banks), the same dimensions of its
// 128 points (same stride; staged ONCE per workgroup when d <= 32, the phase accumulators otherwise run across the dimension
// chunks), the 32 rows of W (16 CT columns, row stride 80 as posterior_mean_multi.hip) and the 32 phases.  Dimensions past d are
// zeros on both sides, so d is padded to the instruction's k by exact zeros.  Per group of four dimensions a wave reads 2 + 2
// operands for 4 instructions.
//
// Cosine.  In turns the argument reduction is exact: f = u - rint(u) in [-1/2, 1/2], k = rint(2 f), g = f - k / 2 in [-1/4, 1/4]
// (both subtractions exact), cos(2 pi u) = (-1)^k cos(2 pi g) with (-1)^k = 1 - 2 k^2.  cos(2 pi g) is the even Taylor polynomial
// of degree 11 in z = g^2 (coefficients (-1)^n (2 pi)^2n / (2n)!, remainder (pi / 2)^24 / 24! = 8e-20), Horner by fma.  Rounding:
// the last step is fma(z, p1, 1) with |p1| <= 19.8 carrying about 24 u of absolute error (u = 2^-53), times z <= 1/16; with the
// roundings of z, of the coefficient c1 and of the result the absolute error is below 5 u = 2.5 eps for every u (the bound that
// tests/test_fourier_paths_gpu.py allows the cosine is 4 eps).  The 12 coefficients travel in the kernel arguments (scalar
// operands, as FastExp); the 8 cosines of one feature tile (2 point tiles x 4 registers) run in lock step.
//
// Edges.  A feature row past the end of the slice is staged as Omega = 0, phase = 0, W = 0 (cos(0) times 0); a point t >= m
// computes on point m - 1 and is not stored; columns c >= s are zeros in the B operand and are not stored; nothing beyond column
// d of a row of xt or omega, or column s of a row of W or out, is touched (ldomega >= d, ldw, ldo >= s).  CT is chosen per call
// (s <= 16, 32, 48: 1, 2, 3; else 4) and column blocks are 64 wide; every column block repeats the phases and cosines.
//
// Slices over the features fill the machine when m is small: slice 0 writes out, slices k >= 1 a bounded partial buffer
// [k - 1][m][s] in the workspace (at most 4 M doubles); the finalize kernel -- one lane per (t, c) -- adds the slices in a fixed
// order; a call of one slice skips it.  No atomics: two calls on the same inputs give the same bits.
//
// Resources (compiler's remarks; no scratch and no spill in any instance): 62 KB of LDS, two workgroups per CU; VGPRs by CT in
// DESIGN.md section 4.
#include "common.h"

namespace gpmp {
namespace {

constexpr int FP_TM = 128;                 // points per workgroup (two tiles of 16 per wave)
constexpr int FP_TP = 2;                   // point tiles per wave
constexpr int FP_FC = 32;                  // features per chunk
constexpr int FP_FT = FP_FC / 16;          // feature tiles per chunk
constexpr int FP_CB = 64;                  // columns per column block: 16 CT
constexpr int FP_DC = 32;                  // dimensions per LDS chunk
constexpr int FP_LD = FP_DC + 2;           // row stride of the staged rows of Omega and of the staged points
constexpr int FP_WLD = 80;                 // row stride of the staged rows of W
constexpr int FP_NCOEF = 12;               // coefficients of the cosine polynomial (degree 11 in g^2)
constexpr int FP_TARGET_WGS = 512;         // workgroups a call is sliced towards (two are resident per CU); not tuned
constexpr int FP_MIN_ROWS = 4 * FP_FC;     // features per slice, at least
constexpr long FP_PART_CAP = 1L << 22;     // doubles of partials (32 MB)
constexpr int FP_FIN_BLOCKS = 1 << 16;     // workgroups of the finalize kernel, at most (it strides over the outputs)

constexpr int fp_ct(int s) { return s <= 16 ? 1 : s <= 32 ? 2 : s <= 48 ? 3 : 4; }

// (never written inside a kernel: one store into the by-value block and the compiler keeps a private copy of it in scratch memory)
struct FpParams {
  const double* xt;              // m x d
  const double* omega;           // r x d (ldomega), turns per unit
  const double* phase;           // r, turns
  const double* W;               // r x s (ldw)
  double* out;                   // m x s (ldo): slice 0, then the result
  double* part;                  // slices 1.. : [slice - 1][m][s]
  long ldomega, ldw, ldo;
  int m, r, s, d, rows_per_slice, nslices;
  double cc[FP_NCOEF];           // cos(2 pi g) = sum_n cc[n] g^2n
};

// cos(2 pi v[i]) in place, N entries in lock step: every step runs across the whole batch before the next one starts, so the
// dependent chain of one entry never starves the fp64 pipe.
template <int N>
__device__ __forceinline__ void fp_cos_turns(const FpParams& p, double (&v)[N]) {
  double sg[N], z[N], c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = v[i] - rint(v[i]);            // f, exact
#pragma unroll
  for (int i = 0; i < N; ++i) sg[i] = rint(v[i] + v[i]);           // k in {-1, 0, 1}
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = fma(-0.5, sg[i], v[i]);       // g, exact
#pragma unroll
  for (int i = 0; i < N; ++i) sg[i] = fma(-2.0 * sg[i], sg[i], 1.0);   // (-1)^k
#pragma unroll
  for (int i = 0; i < N; ++i) z[i] = v[i] * v[i];
  const double ctop = p.cc[FP_NCOEF - 1];
#pragma unroll
  for (int i = 0; i < N; ++i) c[i] = ctop;
#pragma unroll
  for (int n = FP_NCOEF - 2; n >= 0; --n) {
    const double cn = p.cc[n];
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] = fma(c[i], z[i], cn);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = sg[i] * c[i];
}

// Chunk staging, between the two barriers of the dimension loop.  Dimensions j0 .. j0 + 31 of the features kc .. kc + 31 (8
// threads per row), zeros past d and past the slice ...
__device__ __forceinline__ void fp_stage_omega(const FpParams& p, double* so, int kc, int k1, int j0) {
  const int row = threadIdx.x >> 3, col = threadIdx.x & 7;
  const bool live = kc + row < k1;
  const double* __restrict__ src = p.omega + (long)(live ? kc + row : k1 - 1) * p.ldomega + j0;
#pragma unroll
  for (int j = col; j < FP_DC; j += 8) so[row * FP_LD + j] = (live && j0 + j < p.d) ? src[j] : 0.0;
}

// ... the same dimensions of the workgroup's 128 points (a row past m is point m - 1) ...
__device__ __forceinline__ void fp_stage_points(const FpParams& p, double* sx, int tw, int j0) {
  for (int e = threadIdx.x; e < FP_TM * FP_DC; e += 256) {
    const int row = e >> 5, j = e & (FP_DC - 1);
    sx[row * FP_LD + j] = j0 + j < p.d ? p.xt[(long)min(tw + row, p.m - 1) * p.d + j0 + j] : 0.0;
  }
}

// ... and, once per feature chunk, columns c0 .. c0 + 16 CT - 1 of the chunk's rows of W and its phases.
template <int CT>
__device__ __forceinline__ void fp_stage_weights(const FpParams& p, double* sw, double* sp, int kc, int k1, int c0) {
  const int row = threadIdx.x >> 3, col = threadIdx.x & 7;
  const bool live = kc + row < k1;
  const double* __restrict__ wr = p.W + (long)(live ? kc + row : k1 - 1) * p.ldw + c0;
#pragma unroll
  for (int c = col; c < 16 * CT; c += 8) sw[row * FP_WLD + c] = (live && c0 + c < p.s) ? wr[c] : 0.0;
  if (threadIdx.x < FP_FC) sp[threadIdx.x] = kc + (int)threadIdx.x < k1 ? p.phase[kc + threadIdx.x] : 0.0;
}

template <int CT>
__global__ void __launch_bounds__(256, 2) fp_paths_kernel(FpParams p) {
  __shared__ double so[FP_FC * FP_LD];
  __shared__ double sx[FP_TM * FP_LD];
  __shared__ double sw[FP_FC * FP_WLD];
  __shared__ double sp[FP_FC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pt = lane & 15, kk = lane >> 4;
  const int d = p.d, m = p.m, s = p.s;
  const int tw = blockIdx.x * FP_TM;                 // first point of the workgroup
  const int t0 = tw + wave * 16 * FP_TP;             // ... of the wave
  const int slice = blockIdx.y;
  const int c0 = blockIdx.z * FP_CB;
  const int k0 = slice * p.rows_per_slice;
  const int k1 = min(p.r, k0 + p.rows_per_slice);
  d4 acc[FP_TP][CT];
#pragma unroll
  for (int tp = 0; tp < FP_TP; ++tp)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[tp][ct] = d4{0.0, 0.0, 0.0, 0.0};
  const double* __restrict__ arow = so + pt * FP_LD + kk;                              // A operand of the phase product: feature pt (+ 16 ft)
  const double* __restrict__ brow = sx + (wave * 16 * FP_TP + pt) * FP_LD + kk;        // B operand: point pt (+ 16 tp)
  for (int kc = k0; kc < k1; kc += FP_FC) {
    d4 u[FP_FT][FP_TP];
    for (int j0 = 0; j0 < d; j0 += FP_DC) {
      __syncthreads();                   // the previous chunk (with j0 == 0: the previous rows of W and phases too) has been read
      fp_stage_omega(p, so, kc, k1, j0);
      if (j0 == 0) fp_stage_weights<CT>(p, sw, sp, kc, k1, c0);
      if (d > FP_DC || kc == k0) fp_stage_points(p, sx, tw, j0);
      __syncthreads();
      if (j0 == 0) {
#pragma unroll
        for (int ft = 0; ft < FP_FT; ++ft) {
          const d4 ph = d4{sp[16 * ft + kk], sp[16 * ft + 4 + kk], sp[16 * ft + 8 + kk], sp[16 * ft + 12 + kk]};
#pragma unroll
          for (int tp = 0; tp < FP_TP; ++tp) u[ft][tp] = ph;
        }
      }
      const int ng = (min(d - j0, FP_DC) + 3) >> 2;
      for (int g = 0; g < ng; ++g) {
        double a[FP_FT], b[FP_TP];
#pragma unroll
        for (int ft = 0; ft < FP_FT; ++ft) a[ft] = arow[16 * ft * FP_LD + 4 * g];
#pragma unroll
        for (int tp = 0; tp < FP_TP; ++tp) b[tp] = brow[16 * tp * FP_LD + 4 * g];
#pragma unroll
        for (int ft = 0; ft < FP_FT; ++ft)
#pragma unroll
          for (int tp = 0; tp < FP_TP; ++tp) u[ft][tp] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ft], b[tp], u[ft][tp], 0, 0, 0);
      }
    }
    // the cosines of one feature tile in lock step, then its contraction: register q of u is the A operand of features 4 q .. 4 q + 3
#pragma unroll
    for (int ft = 0; ft < FP_FT; ++ft) {
      double cv[4 * FP_TP];
#pragma unroll
      for (int tp = 0; tp < FP_TP; ++tp)
#pragma unroll
        for (int q = 0; q < 4; ++q) cv[4 * tp + q] = u[ft][tp][q];
      fp_cos_turns(p, cv);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double* __restrict__ wr = sw + (16 * ft + 4 * q + kk) * FP_WLD + pt;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const double bv = wr[16 * ct];
#pragma unroll
          for (int tp = 0; tp < FP_TP; ++tp)
            acc[tp][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv[4 * tp + q], bv, acc[tp][ct], 0, 0, 0);
        }
      }
    }
  }
  // C/D register q of lane l: row (l >> 4) + 4 q = point, column l & 15
  double* __restrict__ out = slice > 0 ? p.part + (long)(slice - 1) * m * s : p.out;
  const long ldout = slice > 0 ? (long)s : p.ldo;
#pragma unroll
  for (int tp = 0; tp < FP_TP; ++tp)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c = c0 + 16 * ct + pt;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = t0 + 16 * tp + 4 * q + kk;
        if (t < m && c < s) out[(long)t * ldout + c] = acc[tp][ct][q];
      }
    }
}

// One lane per output (t, c), columns fastest: the partial slices in their order, then slice 0 (the output itself).
__global__ void __launch_bounds__(256) fp_finalize_kernel(FpParams p) {
  const int s = p.s;
  const long total = (long)p.m * s;
  const double* __restrict__ part = p.part;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long t = idx / s;
    double* dst = p.out + t * p.ldo + (idx - t * s);
    double v = 0.0;
#pragma unroll 4
    for (int k = 0; k + 1 < p.nslices; ++k) v += part[k * total + idx];
    *dst = v + *dst;
  }
}

// partials bounded independently of the tile count, so that the query grows with m, r and s only
size_t fp_part_elems(int m, int r, int s) {
  const long by_rows = ((long)r + FP_MIN_ROWS - 1) / FP_MIN_ROWS;
  const long outs = (long)m * s;                   // <= 2^42; the product with by_rows - 1 is taken only where it stays below the cap
  const long part = by_rows - 1 > FP_PART_CAP / outs ? FP_PART_CAP : (by_rows - 1) * outs;
  return (size_t)pad16(part > 0 ? part : 1);
}

// features per slice: a multiple of the chunk, so that only a slice's last chunk is short
int fp_rows_per_slice(int m, int r, int s) {
  const long wgs = (long)((m + FP_TM - 1) / FP_TM) * ((s + FP_CB - 1) / FP_CB);
  long ns = (FP_TARGET_WGS + wgs - 1) / wgs;
  const long by_rows = ((long)r + FP_MIN_ROWS - 1) / FP_MIN_ROWS;
  const long by_cap = 1 + FP_PART_CAP / ((long)m * s);
  if (ns > by_rows) ns = by_rows;
  if (ns > by_cap) ns = by_cap;
  if (ns < 1) ns = 1;
  const long rows = ((long)r + ns - 1) / ns;
  return (int)((rows + FP_FC - 1) / FP_FC * FP_FC);
}

bool fp_in_range(int m, int r, int s, int d) {
  return m >= 1 && m <= GPMP_MAX_EXTENT && r >= 1 && r <= GPMP_MAX_EXTENT && s >= 1 && s <= GPMP_MAX_COLUMNS && d >= 1 &&
         d <= GPMP_MAX_DIM_WIDE;
}

}  // namespace
}  // namespace gpmp

using namespace gpmp;

extern "C" size_t gpmp_fourier_paths_ws_elems(int m, int r, int s, int d) {
  return fp_in_range(m, r, s, d) ? fp_part_elems(m, r, s) : 0;
}

extern "C" int gpmp_fourier_paths(const double* xt, const double* omega, long ldomega, const double* phase, const double* W, long ldw,
                                  int m, int r, int s, int d, double* ws, double* out, long ldo, gpmp_stream_t stream) {
  GPMP_ARG(xt != nullptr, 1, "xt is NULL");
  GPMP_ARG(omega != nullptr, 2, "omega is NULL");
  GPMP_ARG(phase != nullptr, 4, "phase is NULL");
  GPMP_ARG(W != nullptr, 5, "W is NULL");
  GPMP_ARG(m > 0 && m <= GPMP_MAX_EXTENT, 7, "m outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(r > 0 && r <= GPMP_MAX_EXTENT, 8, "r outside [1, GPMP_MAX_EXTENT]");
  GPMP_ARG(s >= 1 && s <= GPMP_MAX_COLUMNS, 9, "s outside [1, GPMP_MAX_COLUMNS]");
  GPMP_ARG(d >= 1 && d <= GPMP_MAX_DIM_WIDE, 10, "d outside [1, GPMP_MAX_DIM_WIDE]");
  GPMP_ARG(ldomega >= d, 3, "ldomega < d");
  GPMP_ARG(ldw >= s, 6, "ldw < s");
  GPMP_ARG(ws != nullptr, 11, "ws is NULL");
  GPMP_ARG(out != nullptr, 12, "out is NULL");
  GPMP_ARG(ldo >= s, 13, "ldo < s");
  hipStream_t st = as_stream(stream);
  FpParams gp;
  std::memset(&gp, 0, sizeof(gp));
  gp.xt = xt;
  gp.omega = omega;
  gp.phase = phase;
  gp.W = W;
  gp.out = out;
  gp.part = ws;
  gp.ldomega = ldomega;
  gp.ldw = ldw;
  gp.ldo = ldo;
  gp.m = m;
  gp.r = r;
  gp.s = s;
  gp.d = d;
  gp.rows_per_slice = fp_rows_per_slice(m, r, s);
  gp.nslices = (r + gp.rows_per_slice - 1) / gp.rows_per_slice;
  // (-1)^n (2 pi)^2n / (2n)! in extended precision, rounded once
  long double term = 1.0L;
  const long double two_pi = 6.283185307179586476925286766559L;
  for (int n = 0; n < FP_NCOEF; ++n) {
    if (n) term *= -(two_pi * two_pi) / (long double)((2 * n - 1) * (2 * n));
    gp.cc[n] = (double)term;
  }
  const dim3 grid((m + FP_TM - 1) / FP_TM, gp.nslices, (s + FP_CB - 1) / FP_CB);
  switch (fp_ct(s)) {
    case 1: hipLaunchKernelGGL(fp_paths_kernel<1>, grid, dim3(256), 0, st, gp); break;
    case 2: hipLaunchKernelGGL(fp_paths_kernel<2>, grid, dim3(256), 0, st, gp); break;
    case 3: hipLaunchKernelGGL(fp_paths_kernel<3>, grid, dim3(256), 0, st, gp); break;
    default: hipLaunchKernelGGL(fp_paths_kernel<4>, grid, dim3(256), 0, st, gp);
  }
  GPMP_HIP_TRY(hipGetLastError());
  if (gp.nslices > 1) {
    const long fin = ((long)m * s + 255) / 256;
    hipLaunchKernelGGL(fp_finalize_kernel, dim3((unsigned)(fin < FP_FIN_BLOCKS ? fin : FP_FIN_BLOCKS)), dim3(256), 0, st, gp);
    GPMP_HIP_TRY(hipGetLastError());
  }
  return 0;
}
