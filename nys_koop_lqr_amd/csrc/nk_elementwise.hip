// Small element-wise and reduction kernels of the O(m^3) stage with their launchers: copies, fills, axpby, the residual
// and norm reductions of the square-root iterations (per-block partials finished by a single-block pass: a fixed summation
// order), the column sums of the RMSE scorer, and the doubled-precision residual and contraction guard of the refinement
// of the regularised solves.
#include "nk_common.h"
#include "nk_tn.h"

#include <algorithm>

namespace nk {

__device__ __forceinline__ void add_diag_kernel_body(double* A, int64_t lda, int n, double v) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[(int64_t)i * lda + i] += v;
}
__global__ void __launch_bounds__(256) add_diag_kernel(double* A, int64_t lda, int n, double v) { add_diag_kernel_body(A, lda, n, v); }
NK_BATCHED_TWIN(add_diag_kernel, (256), double*, int64_t, int, double)
__device__ __forceinline__ void copy2d_kernel_body(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd, int64_t rows, int64_t cols) {
  const int64_t total = rows * cols;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols, c = e - r * cols;
    dst[r * ldd + c] = src[r * lds + c];
  }
}
__global__ void __launch_bounds__(256) copy2d_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd, int64_t rows, int64_t cols) { copy2d_kernel_body(src, lds, dst, ldd, rows, cols); }
NK_BATCHED_TWIN(copy2d_kernel, (256), const double*, int64_t, double*, int64_t, int64_t, int64_t)
__device__ __forceinline__ void axpby2d_kernel_body(double a, const double* __restrict__ X, int64_t ldx, double b, double* __restrict__ Y, int64_t ldy, int64_t rows, int64_t cols) {
  const int64_t total = rows * cols;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols, c = e - r * cols;
    const double y = (b == 0.0) ? 0.0 : b * Y[r * ldy + c];
    Y[r * ldy + c] = a * X[r * ldx + c] + y;
  }
}
__global__ void __launch_bounds__(256) axpby2d_kernel(double a, const double* __restrict__ X, int64_t ldx, double b, double* __restrict__ Y, int64_t ldy, int64_t rows, int64_t cols) { axpby2d_kernel_body(a, X, ldx, b, Y, ldy, rows, cols); }
NK_BATCHED_TWIN(axpby2d_kernel, (256), double, const double*, int64_t, double, double*, int64_t, int64_t, int64_t)
__device__ __forceinline__ bool launch_skipped(const double* state, int step) {
  if (state == nullptr) return false;
  const double f = state[0];
  return f != 0.0 && f <= (double)step;
}
__device__ __forceinline__ void scale_add_identity_kernel_body(double a, const double* __restrict__ X, int64_t ldx, double c, double* __restrict__ Y, int64_t ldy, int n, const double* skip_state, int skip_step) {
  if (launch_skipped(skip_state, skip_step)) return;
  const int64_t total = (int64_t)n * n;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / n, col = e - r * n;
    Y[r * ldy + col] = a * X[r * ldx + col] + (r == col ? c : 0.0);
  }
}
__global__ void __launch_bounds__(256) scale_add_identity_kernel(double a, const double* __restrict__ X, int64_t ldx, double c, double* __restrict__ Y, int64_t ldy, int n, const double* skip_state, int skip_step) { scale_add_identity_kernel_body(a, X, ldx, c, Y, ldy, n, skip_state, skip_step); }
NK_BATCHED_TWIN(scale_add_identity_kernel, (256), double, const double*, int64_t, double, double*, int64_t, int, const double*, int)
__device__ __forceinline__ void fill_kernel_body(double* A, int64_t lda, int64_t rows, int64_t cols, double v) {
  const int64_t total = rows * cols;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols, c = e - r * cols;
    A[r * lda + c] = v;
  }
}
__global__ void __launch_bounds__(256) fill_kernel(double* A, int64_t lda, int64_t rows, int64_t cols, double v) { fill_kernel_body(A, lda, rows, cols, v); }
NK_BATCHED_TWIN(fill_kernel, (256), double*, int64_t, int64_t, int64_t, double)

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// per-block partial sums of (M - I)^2; finished by a second single-block pass (deterministic order)
__device__ __forceinline__ void frob_mi_partial_kernel_body(const double* __restrict__ M, int64_t ldm, int n, double* __restrict__ partial, const double* skip_state, int skip_step) {
  if (launch_skipped(skip_state, skip_step)) return;  // the stale partials give the old residual: harmless
  __shared__ double sh[4];
  const int64_t total = (int64_t)n * n;
  double s = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / n, c = e - r * n;
    const double v = M[r * ldm + c] - (r == c ? 1.0 : 0.0);
    s = fma(v, v, s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void __launch_bounds__(256) frob_mi_partial_kernel(const double* __restrict__ M, int64_t ldm, int n, double* __restrict__ partial, const double* skip_state, int skip_step) { frob_mi_partial_kernel_body(M, ldm, n, partial, skip_state, skip_step); }
NK_BATCHED_TWIN(frob_mi_partial_kernel, (256), const double*, int64_t, int, double*, const double*, int)
// per-block partial [sum of squares, trace]; finished by sum_partials_kernel on each half
__device__ __forceinline__ void sumsq_trace_partial_kernel_body(const double* __restrict__ M, int64_t ldm, int n, double* __restrict__ partial, int nblocks) {
  __shared__ double sh[8];
  const int64_t total = (int64_t)n * n;
  double s = 0.0, t = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / n, c = e - r * n;
    const double v = M[r * ldm + c];
    s = fma(v, v, s);
    if (r == c) t += v;
  }
  s = wave_sum(s);
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; sh[4 + (threadIdx.x >> 6)] = t; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
    partial[nblocks + blockIdx.x] = sh[4] + sh[5] + sh[6] + sh[7];
  }
}
__global__ void __launch_bounds__(256) sumsq_trace_partial_kernel(const double* __restrict__ M, int64_t ldm, int n, double* __restrict__ partial, int nblocks) { sumsq_trace_partial_kernel_body(M, ldm, n, partial, nblocks); }
NK_BATCHED_TWIN(sumsq_trace_partial_kernel, (256), const double*, int64_t, int, double*, int)
__device__ __forceinline__ void sum_partials_kernel_body(const double* __restrict__ partial, int count, double* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += blockDim.x) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void __launch_bounds__(256) sum_partials_kernel(const double* __restrict__ partial, int count, double* __restrict__ out) { sum_partials_kernel_body(partial, count, out); }
NK_BATCHED_TWIN(sum_partials_kernel, (256), const double*, int, double*)
// one wave per row: |row| sums, then max over rows via a second pass
__device__ __forceinline__ void abs_rowsum_kernel_body(const double* __restrict__ M, int64_t ldm, int n, double* __restrict__ rowsum) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  double s = 0.0;
  for (int c = threadIdx.x & 63; c < n; c += 64) s += fabs(M[(int64_t)row * ldm + c]);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) rowsum[row] = s;
}
__global__ void __launch_bounds__(256) abs_rowsum_kernel(const double* __restrict__ M, int64_t ldm, int n, double* __restrict__ rowsum) { abs_rowsum_kernel_body(M, ldm, n, rowsum); }
NK_BATCHED_TWIN(abs_rowsum_kernel, (256), const double*, int64_t, int, double*)
__device__ __forceinline__ void max_kernel_body(const double* __restrict__ v, int count, double* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += blockDim.x) s = fmax(s, v[i]);
  s = wave_max(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
__global__ void __launch_bounds__(256) max_kernel(const double* __restrict__ v, int count, double* __restrict__ out) { max_kernel_body(v, count, out); }
NK_BATCHED_TWIN(max_kernel, (256), const double*, int, double*)

// Column sums of squared differences (the RMSE scorer): each workgroup reduces a slab of rows for 64 columns with
// coalesced row reads; wavefront reduction across the 4 waves through LDS; per-slab partials are summed in order.
__device__ __forceinline__ void colsum_sqdiff_partial_kernel_body(const double* __restrict__ P, int64_t ldp, const double* __restrict__ Y, int64_t ldy, int64_t rows, int cols, int rows_per_block, double* __restrict__ partial) {
  __shared__ double sh[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  double s = 0.0;
  if (col < cols)
    for (int64_t r = r0 + w; r < r1; r += 4) {
      const double v = P[r * ldp + col] - Y[r * ldy + col];
      s = fma(v, v, s);
    }
  sh[w][threadIdx.x & 63] = s;
  __syncthreads();
  if (w == 0 && col < cols)
    partial[(int64_t)blockIdx.y * cols + col] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}
__global__ void __launch_bounds__(256) colsum_sqdiff_partial_kernel(const double* __restrict__ P, int64_t ldp, const double* __restrict__ Y, int64_t ldy, int64_t rows, int cols, int rows_per_block, double* __restrict__ partial) { colsum_sqdiff_partial_kernel_body(P, ldp, Y, ldy, rows, cols, rows_per_block, partial); }
NK_BATCHED_TWIN(colsum_sqdiff_partial_kernel, (256), const double*, int64_t, const double*, int64_t, int64_t, int, int, double*)
__device__ __forceinline__ void colsum_finish_kernel_body(const double* __restrict__ partial, int nslabs, int cols, double* __restrict__ colsum) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols) return;
  double s = 0.0;
  for (int k = 0; k < nslabs; ++k) s += partial[(int64_t)k * cols + col];
  colsum[col] = s;
}
__global__ void __launch_bounds__(256) colsum_finish_kernel(const double* __restrict__ partial, int nslabs, int cols, double* __restrict__ colsum) { colsum_finish_kernel_body(partial, nslabs, cols, colsum); }
NK_BATCHED_TWIN(colsum_finish_kernel, (256), const double*, int, int, double*)

// Res (nr x mq) = R - X P with every dot product accumulated in DOUBLED precision (Ogita / Rump / Oishi's Dot2: the exact
// product by an fma, the exact sum by Knuth's TwoSum, the error terms summed aside): the residual of the refinement step of
// the regularised solves.  A residual formed in plain fp64 carries a rounding error of eps |X| |P| -- as large as the
// residual itself, and the "correction" solved from it moves the solution AWAY from the true one (measured, also with
// LAPACK's factor in NumPy: the cloth fixture's A goes from 4e-5 to 2e-3 off the reference); with the doubled-precision
// residual each step contracts the forward error by cond(P) x the factor's backward error.  10 flop per term on the vector
// ALU: 0.1 ms at m = 200, ~4 ms at m = 2000 -- paid only by fits whose pivots say they need it.
__device__ __forceinline__ void resid_dd_kernel_body(const double* __restrict__ X, int64_t ldx, const double* __restrict__ P,
                                                     int64_t ldp, const double* __restrict__ R, int64_t ldr,
                                                     double* __restrict__ Res, int64_t ldres, int nr, int mq) {
#pragma clang fp contract(off)  // the error-free transformations below need the product and the sum rounded separately
  constexpr int T = 64, BK = 16;
  __shared__ double Xs[T][BK + 1];
  __shared__ double Ps[BK][T + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
  double s[4][4], e[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      s[a][b] = (i < nr && j < mq) ? R[(int64_t)i * ldr + j] : 0.0;
      e[a][b] = 0.0;
    }
  for (int k0 = 0; k0 < mq; k0 += BK) {
#pragma unroll
    for (int t = tid; t < T * BK; t += 256) {
      const int ii = t / BK, kk = t % BK;   // X tile: k fastest (rows of X are contiguous in k)
      const int i = i0 + ii, k = k0 + kk;
      Xs[ii][kk] = (i < nr && k < mq) ? -X[(int64_t)i * ldx + k] : 0.0;
      const int kq = t / T, jj = t % T;     // P tile: j fastest
      const int kp = k0 + kq, j = j0 + jj;
      Ps[kq][jj] = (kp < mq && j < mq) ? P[(int64_t)kp * ldp + j] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < BK; ++kk) {
      double xv[4], pv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xv[a] = Xs[ty + 16 * a][kk];
#pragma unroll
      for (int b = 0; b < 4; ++b) pv[b] = Ps[kk][tx + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double h = xv[a] * pv[b];
          const double r = __builtin_fma(xv[a], pv[b], -h);  // x y = h + r exactly
          const double t = s[a][b] + h;                       // s + h = t + q exactly (TwoSum)
          const double z = t - s[a][b];
          const double q = (s[a][b] - (t - z)) + (h - z);
          s[a][b] = t;
          e[a][b] += q + r;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < nr && j < mq) Res[(int64_t)i * ldres + j] = s[a][b] + e[a][b];
    }
}
__global__ void __launch_bounds__(256) resid_dd_kernel(const double* __restrict__ X, int64_t ldx, const double* __restrict__ P, int64_t ldp, const double* __restrict__ R, int64_t ldr, double* __restrict__ Res, int64_t ldres, int nr, int mq) { resid_dd_kernel_body(X, ldx, P, ldp, R, ldr, Res, ldres, nr, mq); }
NK_BATCHED_TWIN(resid_dd_kernel, (256), const double*, int64_t, const double*, int64_t, const double*, int64_t, double*, int64_t, int, int)

// Guard of the refinement steps: a step is applied only while the corrections contract.  Per-block partial sums of squares of
// the correction dX and of the solution X (rows x cols each) ...
__device__ __forceinline__ void refine_norms_partial_kernel_body(const double* __restrict__ dX, int64_t ldd, const double* __restrict__ X, int64_t ldx, int64_t rows, int64_t cols, double* __restrict__ partial, int nblocks) {
  __shared__ double sh[8];
  const int64_t total = rows * cols;
  double s = 0.0, t = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols, c = e - r * cols;
    const double v = dX[r * ldd + c], w = X[r * ldx + c];
    s = fma(v, v, s);
    t = fma(w, w, t);
  }
  s = wave_sum(s);
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; sh[4 + (threadIdx.x >> 6)] = t; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
    partial[nblocks + blockIdx.x] = sh[4] + sh[5] + sh[6] + sh[7];
  }
}
__global__ void __launch_bounds__(256) refine_norms_partial_kernel(const double* __restrict__ dX, int64_t ldd, const double* __restrict__ X, int64_t ldx, int64_t rows, int64_t cols, double* __restrict__ partial, int nblocks) { refine_norms_partial_kernel_body(dX, ldd, X, ldx, rows, cols, partial, nblocks); }
NK_BATCHED_TWIN(refine_norms_partial_kernel, (256), const double*, int64_t, const double*, int64_t, int64_t, int64_t, double*, int)
// ... and the verdict (one block).  state = [alive, |dX|^2 of the last accepted step, accepted steps, |dX_0| / |X|].  Step 0 is
// accepted when |dX_0| <= |X| / 4 -- the ratio estimates cond x (backward error of the factor), the contraction per step; a
// numerically singular system that happened to factor (gelsd would truncate it) gives >= 1 here and is left alone -- and a
// later step when its correction is at most half the previous one.  Once a step is rejected all later ones are.
__device__ __forceinline__ void refine_gate_kernel_body(const double* __restrict__ partial, int nblocks, int step, double* __restrict__ state) {
  __shared__ double sh[8];
  double s = 0.0, t = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) { s += partial[i]; t += partial[nblocks + i]; }
  s = wave_sum(s);
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; sh[4 + (threadIdx.x >> 6)] = t; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double dx2 = sh[0] + sh[1] + sh[2] + sh[3], x2 = sh[4] + sh[5] + sh[6] + sh[7];
    const bool alive = step == 0 ? true : state[0] != 0.0;
    const double ref2 = step == 0 ? 0.0625 * x2 : 0.25 * state[1];
    const bool ok = alive && dx2 <= ref2;  // false for NaN
    state[0] = ok ? 1.0 : 0.0;
    if (ok) state[1] = dx2;
    state[2] = (step == 0 ? 0.0 : state[2]) + (ok ? 1.0 : 0.0);
    if (step == 0) state[3] = x2 > 0.0 ? sqrt(dx2 / x2) : 0.0;
  }
}
__global__ void __launch_bounds__(256) refine_gate_kernel(const double* __restrict__ partial, int nblocks, int step, double* __restrict__ state) { refine_gate_kernel_body(partial, nblocks, step, state); }
NK_BATCHED_TWIN(refine_gate_kernel, (256), const double*, int, int, double*)
__device__ __forceinline__ void guarded_add_kernel_body(const double* __restrict__ dX, int64_t ldd, double* __restrict__ X, int64_t ldx, int64_t rows, int64_t cols, const double* __restrict__ state) {
  if (state[0] == 0.0) return;
  const int64_t total = rows * cols;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / cols, c = e - r * cols;
    X[r * ldx + c] += dX[r * ldd + c];
  }
}
__global__ void __launch_bounds__(256) guarded_add_kernel(const double* __restrict__ dX, int64_t ldd, double* __restrict__ X, int64_t ldx, int64_t rows, int64_t cols, const double* __restrict__ state) { guarded_add_kernel_body(dX, ldd, X, ldx, rows, cols, state); }
NK_BATCHED_TWIN(guarded_add_kernel, (256), const double*, int64_t, double*, int64_t, int64_t, int64_t, const double*)


int launch_add_diag(nk_ctx* ctx, double* A, int64_t lda, int n, double v) {
  if (n <= 0) return NK_OK;
  hipLaunchKernelGGL(add_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, A, lda, n, v);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_copy2d(nk_ctx* ctx, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return NK_OK;
  hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for(rows * cols, ctx->num_cu)), dim3(256), 0, ctx->stream, src, lds, dst,
                     ldd, rows, cols);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_axpby2d(nk_ctx* ctx, double a, const double* X, int64_t ldx, double b, double* Y, int64_t ldy, int64_t rows,
                   int64_t cols) {
  if (rows <= 0 || cols <= 0) return NK_OK;
  hipLaunchKernelGGL(axpby2d_kernel, dim3(grid_for(rows * cols, ctx->num_cu)), dim3(256), 0, ctx->stream, a, X, ldx, b,
                     Y, ldy, rows, cols);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_resid_dd(nk_ctx* ctx, const double* X, int64_t ldx, const double* P, int64_t ldp, const double* R, int64_t ldr,
                    double* Res, int64_t ldres, int nr, int mq) {
  if (nr <= 0 || mq <= 0) return NK_OK;
  hipLaunchKernelGGL(resid_dd_kernel, dim3((mq + 63) / 64, (nr + 63) / 64), dim3(256), 0, ctx->stream, X, ldx, P, ldp, R,
                     ldr, Res, ldres, nr, mq);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_refine_apply(nk_ctx* ctx, const double* dX, int64_t ldd, double* X, int64_t ldx, int64_t rows, int64_t cols, int step,
                        double* state, double* partial /* 2 * refine_partial_blocks() doubles */) {
  if (rows <= 0 || cols <= 0) return NK_OK;
  const int blocks = std::min(grid_for(rows * cols, ctx->num_cu), refine_partial_blocks());
  hipLaunchKernelGGL(refine_norms_partial_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dX, ldd, (const double*)X, ldx, rows,
                     cols, partial, blocks);
  hipLaunchKernelGGL(refine_gate_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)partial, blocks, step, state);
  hipLaunchKernelGGL(guarded_add_kernel, dim3(grid_for(rows * cols, ctx->num_cu)), dim3(256), 0, ctx->stream, dX, ldd, X, ldx,
                     rows, cols, (const double*)state);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_scale_add_identity(nk_ctx* ctx, double a, const double* X, int64_t ldx, double c, double* Y, int64_t ldy,
                              int n, const TnSkip* skip) {
  if (n <= 0) return NK_OK;
  hipLaunchKernelGGL(scale_add_identity_kernel, dim3(grid_for((int64_t)n * n, ctx->num_cu)), dim3(256), 0, ctx->stream,
                     a, X, ldx, c, Y, ldy, n, skip ? skip->state : nullptr, skip ? skip->step : 0);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_fill(nk_ctx* ctx, double* A, int64_t lda, int64_t rows, int64_t cols, double v) {
  if (rows <= 0 || cols <= 0) return NK_OK;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(rows * cols, ctx->num_cu)), dim3(256), 0, ctx->stream, A, lda, rows,
                     cols, v);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
int launch_frob_minus_identity(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* d_out, const TnSkip* skip) {
  const ArenaMark mk = arena_mark(ctx);
  const int blocks = grid_for((int64_t)n * n, ctx->num_cu);
  double* partial = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)blocks, &partial));
  hipLaunchKernelGGL(frob_mi_partial_kernel, dim3(blocks), dim3(256), 0, ctx->stream, M, ldm, n, partial,
                     skip ? skip->state : nullptr, skip ? skip->step : 0);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, ctx->stream, partial, blocks, d_out);
  NK_HIP(hipGetLastError());
  arena_release(ctx, mk);
  return NK_OK;
}
int launch_frob_mi_partials(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* partial, int* count, const TnSkip* skip) {
  const int blocks = grid_for((int64_t)n * n, ctx->num_cu);
  hipLaunchKernelGGL(frob_mi_partial_kernel, dim3(blocks), dim3(256), 0, ctx->stream, M, ldm, n, partial,
                     skip ? skip->state : nullptr, skip ? skip->step : 0);
  NK_HIP(hipGetLastError());
  *count = blocks;
  return NK_OK;
}
int launch_sumsq_trace(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* d_sumsq, double* d_trace) {
  const ArenaMark mk = arena_mark(ctx);
  const int blocks = grid_for((int64_t)n * n, ctx->num_cu);
  double* partial = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)2 * blocks, &partial));
  hipLaunchKernelGGL(sumsq_trace_partial_kernel, dim3(blocks), dim3(256), 0, ctx->stream, M, ldm, n, partial, blocks);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, ctx->stream, partial, blocks, d_sumsq);
  if (d_trace) hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, ctx->stream, partial + blocks, blocks, d_trace);
  NK_HIP(hipGetLastError());
  arena_release(ctx, mk);
  return NK_OK;
}
int launch_max_abs_rowsum(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* d_out) {
  const ArenaMark mk = arena_mark(ctx);
  double* rs = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n, &rs));
  hipLaunchKernelGGL(abs_rowsum_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, M, ldm, n, rs);
  hipLaunchKernelGGL(max_kernel, dim3(1), dim3(256), 0, ctx->stream, rs, n, d_out);
  NK_HIP(hipGetLastError());
  arena_release(ctx, mk);
  return NK_OK;
}
int launch_colsum_sqdiff(nk_ctx* ctx, const double* P, int64_t ldp, const double* Y, int64_t ldy, int64_t rows,
                         int cols, double* d_colsum) {
  const ArenaMark mk = arena_mark(ctx);
  const int rpb = 256;
  const int nslabs = (int)((rows + rpb - 1) / rpb);
  double* partial = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)nslabs * cols, &partial));
  hipLaunchKernelGGL(colsum_sqdiff_partial_kernel, dim3((cols + 63) / 64, nslabs), dim3(256), 0, ctx->stream, P, ldp, Y,
                     ldy, rows, cols, rpb, partial);
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((cols + 255) / 256), dim3(256), 0, ctx->stream, partial, nslabs, cols,
                     d_colsum);
  NK_HIP(hipGetLastError());
  arena_release(ctx, mk);
  return NK_OK;
}

}  // namespace nk
