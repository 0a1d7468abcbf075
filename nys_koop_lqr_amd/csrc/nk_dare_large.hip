// Riccati solver for ONE problem of any size up to NK_DARE_LARGE_MAX_M: the doubling iteration of nk_dare.hip (and of
// lqr.dare_doubling, its NumPy statement) as a chain of ordinary launches on the context's stream.
//   A_0 = A, G_0 = B R^-1 B', H_0 = Q;  per step  W = I + G H,  [X_A | X_G] = W^-1 [A_k | G],
//   A+ = A_k X_A,  G+ = sym(G + A_k X_G A_k'),  H+ = H + sym(A_k' H X_A);  stop at |H+ - H|_1 <= tol |H+|_1.
//   P = H, K = (R + sym(B'PB))^-1 B'PA.
// Every m x m product is a launch_gemm call.  The solve with W is a blocked LU with partial row pivoting on the augmented
// matrix [W | A_k | G] (M x 3M row-major, M = m rounded up to 16, zero padding, padded diagonal of W one), column blocks of
// DARE_LU_NB = 64.  A block step is four launches:
//   panel   one workgroup factors the nb columns in place in device memory (64 columns = the 64 lanes of a wave, one wave
//           per row: every access is one coalesced 512-byte row segment), records the pivot rows;
//   swap    the recorded exchanges on every column outside the panel, one thread per column;
//   row     U12 = L11^-1 A12 over all columns to the right (right-hand sides included), L11 in LDS, one thread per column;
//   trail   A22 -= L21 U12, launch_gemm with alpha = -1, beta = 1 (contraction 64: four k-steps of the generic engine, no
//           K slices -- nk_gemm_plan.h keeps at least 8 k-steps per slice).
// The backward substitution walks the block rows upwards: X_blk = U11^-1 RHS_blk (U11 in LDS, one thread per column), then
// launch_gemm updates the rows above.
// No kernel waits for another workgroup: no flags, no spinning, no atomics.  Kernels synchronise with __syncthreads() only,
// every loop is bounded by M, p, the block width or max_iter.  Every kernel of the chain reads the device status word first
// and returns when it is non-zero, so a breakdown costs the rest of one step.  The host synchronises once per doubling step
// and reads three words (status, |dH|_1, |H+|_1); the stopping decision is taken there.  All reductions have a fixed order:
// the results are the same bits from call to call.
#include "nk_common.h"

#include <chrono>

namespace nk {

constexpr int DARE_LU_NB = 64;          // column block of the LU = lanes of a wave (the panel kernel relies on it)
constexpr int DARE_PANEL_THREADS = 1024;
constexpr int DARE_PANEL_WAVES = DARE_PANEL_THREADS / 64;
constexpr int DARE_COL_THREADS = 128;   // row / upper kernels: one thread per column
constexpr int DARE_PMAX = NK_DARE_LARGE_MAX_P;
static_assert(DARE_LU_NB == 64, "the panel kernel maps panel columns to the lanes of one wave");

// ---- elementwise kernels -------------------------------------------------------------------------------------------

// out = scale * sym(X + Y) (Y may be null: the plain form), M x M, one thread per pair i <= j writes both entries, so out
// may be X or Y.  The two entries get the same bits.
__global__ void __launch_bounds__(256) dare_sym_kernel(const int* __restrict__ status, double* out, int64_t ldo, const double* X,
                                                       int64_t ldx, const double* Y, int64_t ldy, int M, double scale) {
  if (*status != 0) return;
  const int64_t total = (int64_t)M * M;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / M), j = (int)(e - (int64_t)i * M);
    if (j < i) continue;
    double sij = X[(int64_t)i * ldx + j], sji = X[(int64_t)j * ldx + i];
    if (Y) {
      sij += Y[(int64_t)i * ldy + j];
      sji += Y[(int64_t)j * ldy + i];
    }
    const double v = scale * (0.5 * (sij + sji));
    out[(int64_t)i * ldo + j] = v;
    out[(int64_t)j * ldo + i] = v;
  }
}

// the augmented matrix of a step: W (already G H) gets its unit diagonal, the right-hand sides are A_k and G
__global__ void __launch_bounds__(256) dare_assemble_kernel(const int* __restrict__ status, double* WX, int64_t ldw,
                                                            const double* __restrict__ Ak, const double* __restrict__ G, int M) {
  if (*status != 0) return;
  const int64_t total = (int64_t)M * M;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / M), j = (int)(e - (int64_t)i * M);
    double* row = WX + (int64_t)i * ldw;
    row[M + j] = Ak[e];
    row[2 * M + j] = G[e];
    if (i == j) row[j] += 1.0;
  }
}

// H+ = H + sym(T) in place, one wave per row; rowd[i] = sum_j |sym(T)_ij|, rowh[i] = sum_j |H+_ij| (lane partials over
// j = lane, lane + 64, ... in index order, then the fixed butterfly of wave_sum64_dpp)
__global__ void __launch_bounds__(256) dare_h_update_kernel(const int* __restrict__ status, double* H, const double* __restrict__ T,
                                                            int M, double* rowd, double* rowh) {
  if (*status != 0) return;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;  // wave-uniform
  double sd = 0.0, sh = 0.0;
  for (int j = lane; j < M; j += 64) {
    const double d = 0.5 * (T[(int64_t)i * M + j] + T[(int64_t)j * M + i]);
    const double h = H[(int64_t)i * M + j] + d;
    H[(int64_t)i * M + j] = h;
    sd += fabs(d);
    sh += fabs(h);
  }
  sd = wave_sum64_dpp(sd);
  sh = wave_sum64_dpp(sh);
  if (lane == 0) { rowd[i] = sd; rowh[i] = sh; }
}

// the two norms from the row sums: one workgroup, thread t takes rows t, t + 256, ..., then the 256 partial maxima in index
// order.  ctl: [0] the status word (an int), [1] |dH|_1, [2] |H+|_1.  Non-finite sums set the status to 2.
__global__ void __launch_bounds__(256) dare_norm_kernel(double* ctl, const double* __restrict__ rowd,
                                                        const double* __restrict__ rowh, int M) {
  int* status = reinterpret_cast<int*>(ctl);
  if (*status != 0) return;
  __shared__ double md[256], mh[256];
  __shared__ int bad[256];
  const int tid = threadIdx.x;
  double nd = 0.0, nh = 0.0;
  int nf = 0;
  for (int i = tid; i < M; i += 256) {
    const double a = rowd[i], b = rowh[i];
    if (!isfinite(a) || !isfinite(b)) nf = 1;
    nd = fmax(nd, a);
    nh = fmax(nh, b);
  }
  md[tid] = nd; mh[tid] = nh; bad[tid] = nf;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t) {
      nd = fmax(nd, md[t]);
      nh = fmax(nh, mh[t]);
      nf |= bad[t];
    }
    ctl[1] = nd;
    ctl[2] = nh;
    if (nf) *status = 2;
  }
}

// ---- the p x p systems ---------------------------------------------------------------------------------------------

// lower Cholesky factor of the p x p matrix in S (row stride DARE_PMAX), in place, by one thread; false on a pivot that is
// not positive and finite
__device__ bool dare_large_chol(double* S, int p) {
  for (int j = 0; j < p; ++j) {
    double d = S[j * DARE_PMAX + j];
    for (int k = 0; k < j; ++k) d -= S[j * DARE_PMAX + k] * S[j * DARE_PMAX + k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    d = sqrt(d);
    S[j * DARE_PMAX + j] = d;
    for (int i = j + 1; i < p; ++i) {
      double v = S[i * DARE_PMAX + j];
      for (int k = 0; k < j; ++k) v -= S[i * DARE_PMAX + k] * S[j * DARE_PMAX + k];
      S[i * DARE_PMAX + j] = v / d;
    }
  }
  return true;
}

// start: R = L L' (R null: the identity), Y = L^-1 B' (p rows of M entries, zero beyond column m).  One workgroup.
__global__ void __launch_bounds__(256) dare_start_kernel(int* status, const double* __restrict__ R, int64_t ldr,
                                                         const double* __restrict__ B, int64_t ldb, int m, int p, int M, double* Y) {
  if (*status != 0) return;
  __shared__ double S[DARE_PMAX * DARE_PMAX];
  __shared__ int fail;
  const int tid = threadIdx.x;
  for (int e = tid; e < DARE_PMAX * DARE_PMAX; e += 256) {
    const int a = e / DARE_PMAX, b = e % DARE_PMAX;
    S[e] = (a < p && b < p) ? (R ? R[(int64_t)a * ldr + b] : (a == b ? 1.0 : 0.0)) : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    fail = dare_large_chol(S, p) ? 0 : 1;
    if (fail) *status = 2;
  }
  __syncthreads();
  if (fail) return;
  for (int j = tid; j < M; j += 256) {
    double y[DARE_PMAX];  // fully unrolled: stays in registers
#pragma unroll
    for (int a = 0; a < DARE_PMAX; ++a) {
      if (a < p) {
        double v = j < m ? B[(int64_t)j * ldb + a] : 0.0;
#pragma unroll
        for (int k = 0; k < a; ++k) v -= S[a * DARE_PMAX + k] * y[k];
        y[a] = v / S[a * DARE_PMAX + a];
        Y[(int64_t)a * M + j] = y[a];
      } else {
        y[a] = 0.0;
      }
      asm volatile("" ::: "memory");  // keep the row's LDS reads with the row
    }
  }
}

// gain: S = R + sym(BPB) = L L', K = S^-1 F, one column of K per thread.  BPB: p x p (row stride DARE_PMAX), F: p x m
// (row stride ldf).  One workgroup.
__global__ void __launch_bounds__(256) dare_gain_kernel(int* status, const double* __restrict__ R, int64_t ldr,
                                                        const double* __restrict__ BPB, const double* __restrict__ F, int64_t ldf,
                                                        int m, int p, double* K, int64_t ldk) {
  if (*status != 0) return;
  __shared__ double S[DARE_PMAX * DARE_PMAX];
  __shared__ int fail;
  const int tid = threadIdx.x;
  for (int e = tid; e < DARE_PMAX * DARE_PMAX; e += 256) {
    const int a = e / DARE_PMAX, b = e % DARE_PMAX;
    double v = 0.0;
    if (a < p && b < p) {
      const double r = R ? R[(int64_t)a * ldr + b] : (a == b ? 1.0 : 0.0);
      v = r + 0.5 * (BPB[a * DARE_PMAX + b] + BPB[b * DARE_PMAX + a]);
    }
    S[e] = v;
  }
  __syncthreads();
  if (tid == 0) {
    fail = dare_large_chol(S, p) ? 0 : 1;
    if (fail) *status = 2;
  }
  __syncthreads();
  if (fail) return;
  for (int j = tid; j < m; j += 256) {
    double y[DARE_PMAX];
#pragma unroll
    for (int a = 0; a < DARE_PMAX; ++a) {
      if (a < p) {
        double v = F[(int64_t)a * ldf + j];
#pragma unroll
        for (int k = 0; k < a; ++k) v -= S[a * DARE_PMAX + k] * y[k];
        y[a] = v / S[a * DARE_PMAX + a];
      } else {
        y[a] = 0.0;
      }
      asm volatile("" ::: "memory");  // keep the row's LDS reads with the row
    }
#pragma unroll
    for (int a = DARE_PMAX - 1; a >= 0; --a) {
      if (a < p) {
        double v = y[a];
#pragma unroll
        for (int k = a + 1; k < DARE_PMAX; ++k)
          if (k < p) v -= S[k * DARE_PMAX + a] * y[k];
        y[a] = v / S[a * DARE_PMAX + a];
      }
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int a = 0; a < DARE_PMAX; ++a)
      if (a < p) K[(int64_t)a * ldk + j] = y[a];
  }
}

// ---- blocked LU ----------------------------------------------------------------------------------------------------

// Panel: columns k0 .. k0 + nb - 1, rows k0 .. M - 1 of WX, in place in device memory.  Lane c of every wave owns panel
// column c; wave w takes the rows j + 1 + w, j + 1 + w + 16, ... of column step j, eight rows in flight per lane.  While
// a wave updates its rows it keeps the first maximum of |a| of the NEXT column, so the pivot search costs no pass of its
// own: sixteen candidates in LDS, combined by one thread in wave order with the smaller row index winning ties.
// ipiv[k0 + j] = the (absolute) row exchanged with row k0 + j.
__global__ void __launch_bounds__(DARE_PANEL_THREADS) dare_lu_panel_kernel(int* status, double* WX, int64_t ld, int M, int k0, int nb,
                                                                           int* ipiv) {
  if (*status != 0) return;
  __shared__ double urow[DARE_LU_NB];
  __shared__ double wbest[DARE_PANEL_WAVES];
  __shared__ int wrow[DARE_PANEL_WAVES];
  __shared__ int pivrow;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* P = WX + (int64_t)k0 * ld + k0;
  const int nr = M - k0;
  const bool mine = lane < nb;
  // candidates of column 0 (every lane scans its own column; only lane j's result is used at step j)
  double best = -1.0;
  int bi = nr;
  for (int r = wave; r < nr; r += DARE_PANEL_WAVES) {
    double a = mine ? fabs(P[(int64_t)r * ld + lane]) : 0.0;
    if (a != a) a = __builtin_huge_val();
    if (a > best) { best = a; bi = r; }
  }
  for (int j = 0; j < nb; ++j) {
    if (lane == j) { wbest[wave] = best; wrow[wave] = bi; }
    __threadfence_block();
    __syncthreads();  // every wave has finished the update of step j - 1
    if (tid == 0) {
      double b = wbest[0];
      int r = wrow[0];
      for (int w = 1; w < DARE_PANEL_WAVES; ++w)
        if (wbest[w] > b || (wbest[w] == b && wrow[w] < r)) { b = wbest[w]; r = wrow[w]; }
      pivrow = r;  // j <= r < nr: row j itself is always among the candidates
    }
    __syncthreads();
    const int pr = pivrow;
    if (wave == 0 && mine) {
      const double a = P[(int64_t)j * ld + lane];
      const double b = P[(int64_t)pr * ld + lane];
      if (pr != j) {
        P[(int64_t)j * ld + lane] = b;
        P[(int64_t)pr * ld + lane] = a;
      }
      urow[lane] = b;
      if (lane == 0) ipiv[k0 + j] = k0 + pr;
    }
    __threadfence_block();
    __syncthreads();
    const double piv = urow[j];
    if (piv == 0.0 || !isfinite(piv)) {  // the same LDS word for every thread: uniform
      if (tid == 0) *status = 2;
      return;
    }
    const double u = mine ? urow[lane] : 0.0;
    best = -1.0;
    bi = nr;
    for (int r0 = j + 1 + wave; r0 < nr; r0 += 8 * DARE_PANEL_WAVES) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = r0 + q * DARE_PANEL_WAVES;
        v[q] = (mine && r < nr) ? P[(int64_t)r * ld + lane] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = r0 + q * DARE_PANEL_WAVES;
        const double l = __shfl(v[q], j, 64) / piv;
        if (lane > j) v[q] -= l * u;
        else if (lane == j) v[q] = l;
        if (r < nr) {  // wave-uniform
          if (mine && lane >= j) P[(int64_t)r * ld + lane] = v[q];
          double a = fabs(v[q]);
          if (a != a) a = __builtin_huge_val();
          if (a > best) { best = a; bi = r; }
        }
      }
    }
  }
}

// the panel's nb row exchanges, in order, on every column outside the panel
__global__ void __launch_bounds__(256) dare_lu_swap_kernel(const int* __restrict__ status, double* WX, int64_t ld, int N, int k0, int nb,
                                                           const int* __restrict__ ipiv) {
  if (*status != 0) return;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N || (c >= k0 && c < k0 + nb)) return;
  for (int j = 0; j < nb; ++j) {
    const int r = k0 + j, pr = ipiv[r];
    if (pr != r) {
      double* a = WX + (int64_t)r * ld + c;
      double* b = WX + (int64_t)pr * ld + c;
      const double t = *a;
      *a = *b;
      *b = t;
    }
  }
}

// U12 = L11^-1 A12: rows k0 .. k0 + nb - 1, columns k0 + nb .. N - 1; L11 (unit lower) in LDS.  One thread per column, sixteen
// rows at a time in registers (nb is a multiple of 16): the rows of the chunks above are read back as stored.
__global__ void __launch_bounds__(DARE_COL_THREADS) dare_lu_row_kernel(const int* __restrict__ status, double* WX, int64_t ld, int N,
                                                                       int k0, int nb) {
  if (*status != 0) return;
  __shared__ double L[DARE_LU_NB * DARE_LU_NB];
  for (int e = threadIdx.x; e < nb * DARE_LU_NB; e += DARE_COL_THREADS) {
    const int i = e >> 6, k = e & 63;
    L[e] = k < i ? WX[(int64_t)(k0 + i) * ld + k0 + k] : 0.0;
  }
  __syncthreads();
  const int c = k0 + nb + blockIdx.x * DARE_COL_THREADS + threadIdx.x;
  if (c >= N) return;
  double* col = WX + (int64_t)k0 * ld + c;
  for (int b0 = 0; b0 < nb; b0 += 16) {
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = col[(int64_t)(b0 + i) * ld];
    for (int k = 0; k < b0; ++k) {
      const double x = col[(int64_t)k * ld];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] -= L[(b0 + i) * DARE_LU_NB + k] * x;
    }
#pragma unroll
    for (int i = 1; i < 16; ++i) {
#pragma unroll
      for (int k = 0; k < i; ++k) v[i] -= L[(b0 + i) * DARE_LU_NB + b0 + k] * v[k];
      asm volatile("" ::: "memory");  // keep the row's LDS reads with the row
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) col[(int64_t)(b0 + i) * ld] = v[i];
  }
}

// X_blk = U11^-1 RHS_blk: rows k0 .. k0 + nb - 1 of the right-hand-side columns c0 .. N - 1; U11 (upper) in LDS.  One thread
// per column, sixteen rows at a time from the last chunk upwards.
__global__ void __launch_bounds__(DARE_COL_THREADS) dare_lu_upper_kernel(const int* __restrict__ status, double* WX, int64_t ld, int c0,
                                                                         int N, int k0, int nb) {
  if (*status != 0) return;
  __shared__ double U[DARE_LU_NB * DARE_LU_NB];
  for (int e = threadIdx.x; e < nb * DARE_LU_NB; e += DARE_COL_THREADS) {
    const int i = e >> 6, k = e & 63;
    U[e] = (k >= i && k < nb) ? WX[(int64_t)(k0 + i) * ld + k0 + k] : 0.0;
  }
  __syncthreads();
  const int c = c0 + blockIdx.x * DARE_COL_THREADS + threadIdx.x;
  if (c >= N) return;
  double* col = WX + (int64_t)k0 * ld + c;
  for (int b0 = nb - 16; b0 >= 0; b0 -= 16) {
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = col[(int64_t)(b0 + i) * ld];
    for (int k = b0 + 16; k < nb; ++k) {
      const double x = col[(int64_t)k * ld];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] -= U[(b0 + i) * DARE_LU_NB + k] * x;
    }
#pragma unroll
    for (int i = 15; i >= 0; --i) {
#pragma unroll
      for (int k = i + 1; k < 16; ++k) v[i] -= U[(b0 + i) * DARE_LU_NB + b0 + k] * v[k];
      v[i] /= U[(b0 + i) * DARE_LU_NB + b0 + i];
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) col[(int64_t)(b0 + i) * ld] = v[i];
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------

namespace {

struct PhaseClock {  // NYSKOOP_DARE_TIMING=1: the stream is synchronised around every phase and the host clock read
  nk_ctx* ctx;
  bool on;
  double* slot = nullptr;
  std::chrono::steady_clock::time_point t0;
  int begin(double* s) {
    if (!on) return NK_OK;
    NK_HIP(hipStreamSynchronize(ctx->stream));
    slot = s;
    t0 = std::chrono::steady_clock::now();
    return NK_OK;
  }
  int end() {
    if (!on) return NK_OK;
    NK_HIP(hipStreamSynchronize(ctx->stream));
    *slot += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return NK_OK;
  }
};

thread_local DareLargeTimes tl_times;

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// W^-1 [A_k | G] in place on the augmented matrix
int lu_solve(nk_ctx* ctx, int* status, double* WX, int M, int* ipiv) {
  const int N = 3 * M;
  const int64_t ld = N;
  for (int k0 = 0; k0 < M; k0 += DARE_LU_NB) {
    const int nb = M - k0 < DARE_LU_NB ? M - k0 : DARE_LU_NB;
    hipLaunchKernelGGL(dare_lu_panel_kernel, dim3(1), dim3(DARE_PANEL_THREADS), 0, ctx->stream, status, WX, ld, M, k0, nb, ipiv);
    hipLaunchKernelGGL(dare_lu_swap_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, ctx->stream, status, WX, ld, N, k0, nb, ipiv);
    const int right = N - k0 - nb;  // >= 2M
    hipLaunchKernelGGL(dare_lu_row_kernel, dim3(blocks_for(right, DARE_COL_THREADS)), dim3(DARE_COL_THREADS), 0, ctx->stream, status,
                       WX, ld, N, k0, nb);
    NK_HIP(hipGetLastError());
    const int below = M - k0 - nb;
    if (below > 0)
      NK_TRY(launch_gemm(ctx, false, false, below, right, nb, -1.0, WX + (int64_t)(k0 + nb) * ld + k0, ld,
                         WX + (int64_t)k0 * ld + k0 + nb, ld, 1.0, WX + (int64_t)(k0 + nb) * ld + k0 + nb, ld));
  }
  const int last = ((M - 1) / DARE_LU_NB) * DARE_LU_NB;
  for (int k0 = last; k0 >= 0; k0 -= DARE_LU_NB) {
    const int nb = M - k0 < DARE_LU_NB ? M - k0 : DARE_LU_NB;
    hipLaunchKernelGGL(dare_lu_upper_kernel, dim3(blocks_for(2 * M, DARE_COL_THREADS)), dim3(DARE_COL_THREADS), 0, ctx->stream, status,
                       WX, ld, M, N, k0, nb);
    NK_HIP(hipGetLastError());
    if (k0 > 0)
      NK_TRY(launch_gemm(ctx, false, false, k0, 2 * M, nb, -1.0, WX + k0, ld, WX + (int64_t)k0 * ld + M, ld, 1.0, WX + M, ld));
  }
  return NK_OK;
}

}  // namespace

void dare_large_last_times(DareLargeTimes* out) { *out = tl_times; }

size_t dare_large_ws_bytes(int m) {
  const size_t M = (size_t)dare_pad(m);
  // A_k, its successor, G, H, two temporaries, the augmented matrix; Y (later B'P) and F (p rows of M each, p <= 32); the
  // p x p product; the row sums; the control words; the pivot rows
  return (9 * M * M + 2 * DARE_PMAX * M + DARE_PMAX * DARE_PMAX + 2 * M + 8) * sizeof(double) + M * sizeof(int);
}

int launch_dare_large(nk_ctx* ctx, const DareLargeArgs& a, DareLargeResult* res) {
  const int m = a.m, p = a.p, M = dare_pad(m);
  const int64_t MM = (int64_t)M * M, ldw = 3 * (int64_t)M;
  struct Ws {  // a dedicated allocation, released before the call returns (the context's workspace only grows)
    double* p = nullptr;
    ~Ws() { if (p) (void)hipFree(p); }
  } ws;
  const size_t bytes = dare_large_ws_bytes(m);
  {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ws.p), bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      ws.p = nullptr;
      set_error("dare_large: the workspace for m = %d (%zu bytes) does not fit: %s", m, bytes, hipGetErrorString(e));
      return NK_ERR_OOM;
    }
  }
  double* Ak = ws.p;
  double* An = Ak + MM;
  double* G = An + MM;
  double* H = G + MM;
  double* T1 = H + MM;
  double* T2 = T1 + MM;
  double* WX = T2 + MM;
  double* Y = WX + 3 * MM;                    // p x M: L^-1 B', later B'P
  double* F = Y + (int64_t)DARE_PMAX * M;     // p x M: B'PA
  double* BPB = F + (int64_t)DARE_PMAX * M;
  double* rowd = BPB + DARE_PMAX * DARE_PMAX;
  double* rowh = rowd + M;
  double* ctl = rowh + M;  // 8 doubles: [0] status word, [1] |dH|_1, [2] |H+|_1
  int* ipiv = reinterpret_cast<int*>(ctl + 8);
  int* status = reinterpret_cast<int*>(ctl);
  const bool timing = getenv("NYSKOOP_DARE_TIMING") != nullptr;
  PhaseClock clk{ctx, timing};
  tl_times = DareLargeTimes{};
  const auto t_begin = std::chrono::steady_clock::now();

  // zero: the padding of every operand, the control words, the pivot rows
  NK_HIP(hipMemsetAsync(ws.p, 0, bytes, ctx->stream));
  NK_TRY(launch_copy2d(ctx, a.A, a.lda, Ak, M, m, m));
  const int egrid = grid_for(MM, ctx->num_cu);
  if (a.C) {  // H_0 = c sym(C'C)
    NK_TRY(launch_gemm(ctx, true, false, m, m, a.d, 1.0, a.C, a.ldc, a.C, a.ldc, 0.0, T1, M));
    hipLaunchKernelGGL(dare_sym_kernel, dim3(egrid), dim3(256), 0, ctx->stream, status, H, (int64_t)M, T1, (int64_t)M,
                       (const double*)nullptr, (int64_t)0, M, a.c);
  } else {
    NK_TRY(launch_copy2d(ctx, a.Q, a.ldq, H, M, m, m));
  }
  hipLaunchKernelGGL(dare_start_kernel, dim3(1), dim3(256), 0, ctx->stream, status, a.R, a.ldr, a.B, a.ldb, m, p, M, Y);
  NK_HIP(hipGetLastError());
  NK_TRY(launch_gemm(ctx, true, false, M, M, p, 1.0, Y, M, Y, M, 0.0, G, M));  // G_0 = Y'Y

  int st = 0, iters = 0;
  bool converged = false;
  double delta = __builtin_nan("");
  double* h = ctx->h_scalars + HS_SCRATCH;
  auto read_status = [&](int* word) -> int {  // the status word and the two norms, behind everything queued so far
    NK_HIP(hipMemcpyAsync(h, ctl, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    __builtin_memcpy(word, h, sizeof(int));
    return NK_OK;
  };
  {  // a factorisation of R that broke down ends the call here, with no step taken
    int word = 0;
    NK_TRY(read_status(&word));
    if (word != 0) st = 2;
  }
  for (int it = 0; it < a.max_iter && st == 0 && !converged; ++it) {
    NK_TRY(clk.begin(&tl_times.ms_products));
    NK_TRY(launch_gemm(ctx, false, false, M, M, M, 1.0, G, M, H, M, 0.0, WX, ldw));
    hipLaunchKernelGGL(dare_assemble_kernel, dim3(egrid), dim3(256), 0, ctx->stream, status, WX, ldw, Ak, G, M);
    NK_HIP(hipGetLastError());
    NK_TRY(clk.end());
    NK_TRY(clk.begin(&tl_times.ms_lu));
    NK_TRY(lu_solve(ctx, status, WX, M, ipiv));
    NK_TRY(clk.end());
    NK_TRY(clk.begin(&tl_times.ms_products));
    const double* XA = WX + M;
    const double* XG = WX + 2 * M;
    // G+ = sym(G + A_k X_G A_k')
    NK_TRY(launch_gemm(ctx, false, false, M, M, M, 1.0, Ak, M, XG, ldw, 0.0, T1, M));
    NK_TRY(launch_gemm(ctx, false, true, M, M, M, 1.0, T1, M, Ak, M, 0.0, T2, M));
    hipLaunchKernelGGL(dare_sym_kernel, dim3(egrid), dim3(256), 0, ctx->stream, status, G, (int64_t)M, G, (int64_t)M,
                       (const double*)T2, (int64_t)M, M, 1.0);
    NK_HIP(hipGetLastError());
    // H+ = H + sym(A_k' H X_A), the row sums and the two norms
    NK_TRY(launch_gemm(ctx, true, false, M, M, M, 1.0, Ak, M, H, M, 0.0, T1, M));
    NK_TRY(launch_gemm(ctx, false, false, M, M, M, 1.0, T1, M, XA, ldw, 0.0, T2, M));
    hipLaunchKernelGGL(dare_h_update_kernel, dim3(blocks_for(M, 4)), dim3(256), 0, ctx->stream, status, H, T2, M, rowd, rowh);
    hipLaunchKernelGGL(dare_norm_kernel, dim3(1), dim3(256), 0, ctx->stream, ctl, rowd, rowh, M);
    NK_HIP(hipGetLastError());
    NK_TRY(clk.end());
    // the one host synchronisation of the step: status and the two norms
    const auto ts = std::chrono::steady_clock::now();
    int word = 0;
    NK_TRY(read_status(&word));
    if (timing) tl_times.ms_sync += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
    iters = it + 1;
    if (word != 0) { st = 2; break; }
    const double nd = h[1], nh = h[2];
    delta = nh > 0.0 ? nd / nh : nd;
    converged = nd <= a.tol * nh;
    if (!converged) {
      NK_TRY(clk.begin(&tl_times.ms_products));
      NK_TRY(launch_gemm(ctx, false, false, M, M, M, 1.0, Ak, M, XA, ldw, 0.0, An, M));  // A+ = A_k X_A
      NK_TRY(clk.end());
      double* t = Ak; Ak = An; An = t;
    }
  }
  if (st == 0 && !converged) st = 1;

  if (st == 0) {  // K = (R + sym(B'PB))^-1 B'PA with P = H
    NK_TRY(launch_gemm(ctx, true, false, p, m, m, 1.0, a.B, a.ldb, H, M, 0.0, Y, M));          // B'P
    NK_TRY(launch_gemm(ctx, false, false, p, p, m, 1.0, Y, M, a.B, a.ldb, 0.0, BPB, DARE_PMAX)); // (B'P) B
    NK_TRY(launch_gemm(ctx, false, false, p, m, m, 1.0, Y, M, a.A, a.lda, 0.0, F, M));          // (B'P) A
    hipLaunchKernelGGL(dare_gain_kernel, dim3(1), dim3(256), 0, ctx->stream, status, a.R, a.ldr, BPB, F, (int64_t)M, m, p, a.outK,
                       a.ldk);
    NK_HIP(hipGetLastError());
    if (a.outP) NK_TRY(launch_copy2d(ctx, H, M, a.outP, a.ldp, m, m));
    int word = 0;
    NK_TRY(read_status(&word));
    if (word != 0) st = 2;
  }
  if (st != 0) {
    NK_TRY(launch_fill(ctx, a.outK, a.ldk, p, m, __builtin_nan("")));
    if (a.outP) NK_TRY(launch_fill(ctx, a.outP, a.ldp, m, m, __builtin_nan("")));
  }
  NK_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is released on return
  tl_times.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  tl_times.steps = iters;
  res->status = st;
  res->iters = iters;
  res->delta = delta;
  return NK_OK;
}

}  // namespace nk
