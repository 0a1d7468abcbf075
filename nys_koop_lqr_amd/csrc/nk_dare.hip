// Batched discrete algebraic Riccati solver: the gain K = dlqr(A, B, Q, R) of the LQR sweeps (lqr.py, benchmark_lqr_hjb.py:293)
// for many independent problems in one launch.  ONE workgroup of 256 threads owns ONE problem from its first to its last
// instruction: nothing crosses workgroups (no flags, no spinning), every loop is bounded by max_iter, m or p.
//
// Structure-preserving doubling (lqr.dare_doubling is the NumPy statement of the same steps):
//   A_0 = A, G_0 = B R^-1 B', H_0 = Q;  per step  W = I + G H,  [X_A | X_G] = W^-1 [A_k | G],
//   A+ = A_k X_A,  G+ = sym(G + A_k X_G A_k'),  H+ = H + sym(A_k' H X_A);  stop at |H+ - H|_1 <= tol |H+|_1.
//   P = H, K = (R + B'PB)^-1 B'PA.
// Products: v_mfma_f64_16x16x4_f64 through one device function (wg_gemm, nk_wg_gemm.h), operand panels staged in LDS, every wave takes
// 16 x 16 output tiles, contraction in chunks of 16 in index order (the summation order depends on the sizes alone).
// The solve with W: LU with partial row pivoting, panels of 16 columns in LDS, applied to [W | A_k | G] as one augmented
// matrix (so the forward substitution of the 2m right-hand-side columns happens block step by block step with the
// elimination), then the backward substitution one 16-row block at a time; the trailing updates are wg_gemm calls.
// Workspace (device memory, per problem, touched by its own workgroup only, ordered by __syncthreads()): A_k, G, H, one
// temporary (M x M each) and the augmented matrix (M x 3M), M = m rounded up to 16; padding is zero, the padded diagonal of
// W is one.
#include "nk_common.h"
#include "nk_wg_gemm.h"

namespace nk {

constexpr int DARE_PLD = 17;  // LDS row stride of the LU panel (up to 256 rows x 16 columns)

struct DareLds : WgGemmLds {  // As, Bs: the panels of wg_gemm
  double panel[DARE_MAX_M * DARE_PLD];
  double rowd[DARE_MAX_M];  // row sums of |H+ - H|
  double rowh[DARE_MAX_M];  // row sums of |H+|
  double S[DARE_MAX_P * DARE_MAX_P];  // p x p systems (R, R + B'PB) and their Cholesky factors
  double scal[4];           // [0] last relative step, [1] |H+ - H|_1, [2] |H+|_1
  int ipiv[16];
  int flag[4];              // [0] pivot row of the current column, [1] failure, [2] converged
};

// In-place solve W X = Y on the augmented matrix WX = [W | Y] (M x 3M, leading dimension 3M): X replaces Y.
// Returns false (for every thread alike) on a zero or non-finite pivot.
__device__ bool dare_lu_solve(double* WX, int M, DareLds& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = 3 * M;
  const int64_t ld = N;
  for (int r0 = 0; r0 < M; r0 += 16) {
    const int nr = M - r0;
    for (int e = tid; e < nr * 16; e += DARE_THREADS) s.panel[(e >> 4) * DARE_PLD + (e & 15)] = WX[(int64_t)(r0 + (e >> 4)) * ld + r0 + (e & 15)];
    __syncthreads();
    for (int j = 0; j < 16; ++j) {
      if (wave == 0) {
        // first maximum of |column j| over rows j .. nr-1 (a NaN counts as the largest): lanes scan in index order, then a
        // butterfly that prefers the smaller row index on ties
        double best = -1.0;
        int bi = nr;
        for (int i = j + lane; i < nr; i += 64) {
          double v = fabs(s.panel[i * DARE_PLD + j]);
          if (v != v) v = __builtin_huge_val();
          if (v > best) { best = v; bi = i; }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const double ob = __shfl_xor(best, off);
          const int oi = __shfl_xor(bi, off);
          if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) s.flag[0] = bi;
      }
      __syncthreads();
      const int pr = s.flag[0];  // j <= pr < nr: row j itself is always scanned (two barriers follow before the next write)
      if (tid < 16 && pr != j) {
        const double t = s.panel[j * DARE_PLD + tid];
        s.panel[j * DARE_PLD + tid] = s.panel[pr * DARE_PLD + tid];
        s.panel[pr * DARE_PLD + tid] = t;
      }
      if (tid == 0) s.ipiv[j] = pr;
      __syncthreads();
      const double piv = s.panel[j * DARE_PLD + j];
      if (piv == 0.0 || !isfinite(piv)) return false;  // the same LDS word for every thread: uniform
      for (int i = j + 1 + tid; i < nr; i += DARE_THREADS) {
        const double l = s.panel[i * DARE_PLD + j] / piv;
        s.panel[i * DARE_PLD + j] = l;
        for (int c = j + 1; c < 16; ++c) s.panel[i * DARE_PLD + c] -= l * s.panel[j * DARE_PLD + c];
      }
      __syncthreads();
    }
    for (int e = tid; e < nr * 16; e += DARE_THREADS) WX[(int64_t)(r0 + (e >> 4)) * ld + r0 + (e & 15)] = s.panel[(e >> 4) * DARE_PLD + (e & 15)];
    // the panel's row exchanges on every other column (factor columns to the left, trailing matrix and right-hand sides)
    for (int c = tid; c < N; c += DARE_THREADS) {
      if (c >= r0 && c < r0 + 16) continue;
      for (int j = 0; j < 16; ++j) {
        const int pr = s.ipiv[j];
        if (pr != j) {
          double* a = WX + (int64_t)(r0 + j) * ld + c;
          double* b = WX + (int64_t)(r0 + pr) * ld + c;
          const double t = *a;
          *a = *b;
          *b = t;
        }
      }
    }
    __syncthreads();
    // row block of U and of the forward-substituted right-hand sides: L11^-1 (unit lower, in the panel) times rows r0 .. r0+15
    for (int c = r0 + 16 + tid; c < N; c += DARE_THREADS) {
      double v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = WX[(int64_t)(r0 + i) * ld + c];
#pragma unroll
      for (int i = 1; i < 16; ++i) {
#pragma unroll
        for (int k = 0; k < i; ++k) v[i] -= s.panel[i * DARE_PLD + k] * v[k];
        asm volatile("" ::: "memory");  // keep the row's LDS reads with the row: hoisting all 120 costs 240 registers
      }
#pragma unroll
      for (int i = 1; i < 16; ++i) WX[(int64_t)(r0 + i) * ld + c] = v[i];
    }
    __syncthreads();
    if (nr > 16) {
      const DareOp L21{WX + (int64_t)(r0 + 16) * ld + r0, ld, nr - 16, 16, false};
      const DareOp U12{WX + (int64_t)r0 * ld + r0 + 16, ld, 16, N - r0 - 16, false};
      wg_gemm<2>(WX + (int64_t)(r0 + 16) * ld + r0 + 16, ld, nr - 16, N - r0 - 16, 16, L21, U12, s);
    }
  }
  // backward substitution on the 2M right-hand-side columns, one 16-row block at a time
  for (int r0 = M - 16; r0 >= 0; r0 -= 16) {
    s.panel[(tid >> 4) * DARE_PLD + (tid & 15)] = WX[(int64_t)(r0 + (tid >> 4)) * ld + r0 + (tid & 15)];
    __syncthreads();
    for (int c = M + tid; c < N; c += DARE_THREADS) {
      double v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = WX[(int64_t)(r0 + i) * ld + c];
#pragma unroll
      for (int i = 15; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < 16; ++k) v[i] -= s.panel[i * DARE_PLD + k] * v[k];
        v[i] /= s.panel[i * DARE_PLD + i];
        asm volatile("" ::: "memory");
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) WX[(int64_t)(r0 + i) * ld + c] = v[i];
    }
    __syncthreads();
    if (r0 > 0) {
      const DareOp U01{WX + r0, ld, r0, 16, false};
      const DareOp Xr{WX + (int64_t)r0 * ld + M, ld, 16, 2 * M, false};
      wg_gemm<2>(WX + M, ld, r0, 2 * M, 16, U01, Xr, s);
    }
  }
  return true;
}

// lower Cholesky factor of the p x p matrix in S (row stride DARE_MAX_P), in place, by one thread; false on a pivot that is
// not positive and finite
__device__ bool dare_small_chol(double* S, int p) {
  for (int j = 0; j < p; ++j) {
    double d = S[j * DARE_MAX_P + j];
    for (int k = 0; k < j; ++k) d -= S[j * DARE_MAX_P + k] * S[j * DARE_MAX_P + k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    d = sqrt(d);
    S[j * DARE_MAX_P + j] = d;
    for (int i = j + 1; i < p; ++i) {
      double v = S[i * DARE_MAX_P + j];
      for (int k = 0; k < j; ++k) v -= S[i * DARE_MAX_P + k] * S[j * DARE_MAX_P + k];
      S[i * DARE_MAX_P + j] = v / d;
    }
  }
  return true;
}

__global__ void __launch_bounds__(DARE_THREADS, 2) dare_batch_kernel(const DareRec* table, double tol, int max_iter) {
  __shared__ DareLds s;
  const DareRec rec = table[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = rec.m, p = rec.p, M = rec.M;
  const int64_t MM = (int64_t)M * M;
  double* Ak = rec.ws;
  double* G = Ak + MM;
  double* H = G + MM;
  double* T = H + MM;
  double* WX = T + MM;  // M x 3M: [W | X_A | X_G]
  const int64_t ldw = 3 * (int64_t)M;

  // ---- start values --------------------------------------------------------------------------------------------
  for (int64_t e = tid; e < MM; e += DARE_THREADS) {
    const int i = (int)(e / M), j = (int)(e % M);
    Ak[e] = (i < m && j < m) ? rec.A[(int64_t)i * rec.lda + j] : 0.0;
  }
  if (rec.C) {  // H_0 = c sym(C'C): the cost of the sweeps, formed from the model's reconstruction operator
    const DareOp Ct{rec.C, rec.ldc, rec.d, m, true};
    const DareOp Cn{rec.C, rec.ldc, rec.d, m, false};
    wg_gemm<0>(T, M, M, M, rec.d, Ct, Cn, s);
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      H[e] = rec.c * (0.5 * (T[e] + T[(int64_t)j * M + i]));
    }
  } else {
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      H[e] = (i < m && j < m) ? rec.Q[(int64_t)i * rec.ldq + j] : 0.0;
    }
  }
  if (tid < DARE_MAX_P * DARE_MAX_P) {
    const int a = tid / DARE_MAX_P, b = tid % DARE_MAX_P;
    s.S[tid] = (a < p && b < p) ? (rec.R ? rec.R[a * p + b] : (a == b ? 1.0 : 0.0)) : 0.0;
  }
  if (tid == 0) { s.flag[1] = 0; s.flag[2] = 0; s.scal[0] = __builtin_nan(""); }
  __syncthreads();
  if (rec.q_only) {  // nk_model_lqr_cost: hand the cost matrix back, nothing else
    for (int e = tid; e < m * m; e += DARE_THREADS) rec.outP[(int64_t)(e / m) * m + e % m] = H[(int64_t)(e / m) * M + e % m];
    if (tid == 0) { *rec.status = 0; *rec.iters = 0; }
    return;
  }
  if (tid == 0 && !dare_small_chol(s.S, p)) s.flag[1] = 1;
  __syncthreads();
  int status = s.flag[1] ? 2 : 0;
  int iters = 0;
  if (status == 0) {
    // Y = L^-1 B' (p x m, in T with row stride M), G_0 = Y'Y
    for (int j = tid; j < M; j += DARE_THREADS) {
      double y[DARE_MAX_P];  // fully unrolled: stays in registers
#pragma unroll
      for (int a = 0; a < DARE_MAX_P; ++a) {
        if (a < p) {
          double v = j < m ? rec.B[(int64_t)j * rec.ldb + a] : 0.0;
#pragma unroll
          for (int k = 0; k < a; ++k) v -= s.S[a * DARE_MAX_P + k] * y[k];
          y[a] = v / s.S[a * DARE_MAX_P + a];
          T[(int64_t)a * M + j] = y[a];
        }
      }
    }
    __syncthreads();
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      double g = 0.0;
      for (int a = 0; a < p; ++a) g += T[(int64_t)a * M + i] * T[(int64_t)a * M + j];
      G[e] = g;
    }
    __syncthreads();
  }

  // ---- doubling steps --------------------------------------------------------------------------------------------
  bool converged = false;
  for (int it = 0; it < max_iter && status == 0 && !converged; ++it) {
    // W = I + G H; right-hand sides [A_k | G]
    wg_gemm<0>(WX, ldw, M, M, M, DareOp{G, M, M, M, false}, DareOp{H, M, M, M, false}, s);
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      WX[i * ldw + M + j] = Ak[e];
      WX[i * ldw + 2 * M + j] = G[e];
      if (i == j) WX[i * ldw + j] += 1.0;
    }
    __syncthreads();
    if (!dare_lu_solve(WX, M, s)) { status = 2; break; }
    const DareOp XA{WX + M, ldw, M, M, false};
    const DareOp XG{WX + 2 * M, ldw, M, M, false};
    // G+ = sym(G + A_k X_G A_k')  (the W block of the augmented matrix is free now: the second temporary)
    wg_gemm<0>(T, M, M, M, M, DareOp{Ak, M, M, M, false}, XG, s);
    wg_gemm<0>(WX, ldw, M, M, M, DareOp{T, M, M, M, false}, DareOp{Ak, M, M, M, true}, s);
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      if (j < i) continue;  // one thread per pair writes both entries
      const double sij = G[(int64_t)i * M + j] + WX[i * ldw + j];
      const double sji = G[(int64_t)j * M + i] + WX[j * ldw + i];
      const double g = 0.5 * (sij + sji);
      G[(int64_t)i * M + j] = g;
      G[(int64_t)j * M + i] = g;
    }
    __syncthreads();
    // H+ = H + sym(A_k' H X_A), with the row sums of the stopping test (H is symmetric: row sums = column sums)
    wg_gemm<0>(T, M, M, M, M, DareOp{Ak, M, M, M, true}, DareOp{H, M, M, M, false}, s);
    wg_gemm<0>(WX, ldw, M, M, M, DareOp{T, M, M, M, false}, XA, s);
    for (int i = wave; i < M; i += DARE_THREADS / 64) {
      double sd = 0.0, sh = 0.0;
      for (int j = lane; j < M; j += 64) {
        const double d = 0.5 * (WX[i * ldw + j] + WX[j * ldw + i]);
        const double h = H[(int64_t)i * M + j] + d;
        H[(int64_t)i * M + j] = h;
        sd += fabs(d);
        sh += fabs(h);
      }
      sd = wave_sum64_dpp(sd);
      sh = wave_sum64_dpp(sh);
      if (lane == 0) { s.rowd[i] = sd; s.rowh[i] = sh; }
    }
    __syncthreads();
    if (tid == 0) {
      double nd = 0.0, nh = 0.0;
      bool finite = true;
      for (int i = 0; i < M; ++i) {
        finite = finite && isfinite(s.rowd[i]) && isfinite(s.rowh[i]);
        nd = fmax(nd, s.rowd[i]);
        nh = fmax(nh, s.rowh[i]);
      }
      s.flag[1] = finite ? 0 : 1;
      s.flag[2] = (finite && nd <= tol * nh) ? 1 : 0;
      s.scal[0] = nh > 0.0 ? nd / nh : nd;
    }
    __syncthreads();
    iters = it + 1;
    if (s.flag[1]) { status = 2; break; }
    converged = s.flag[2] != 0;
    if (!converged) {
      // A+ = A_k X_A into the temporary, which then changes places with A_k
      wg_gemm<0>(T, M, M, M, M, DareOp{Ak, M, M, M, false}, XA, s);
      double* t = Ak; Ak = T; T = t;
    }
  }
  if (status == 0 && !converged) status = 1;
  __syncthreads();

  // ---- gain: K = (R + B'PB)^-1 B'PA with P = H -------------------------------------------------------------------
  if (status == 0) {
    double* PB = T;                             // m x p, row stride DARE_MAX_P
    double* F = T + (int64_t)M * DARE_MAX_P;    // p x m, row stride M
    for (int e = tid; e < m * p; e += DARE_THREADS) {
      const int i = e / p, a = e % p;
      double v = 0.0;
      for (int j = 0; j < m; ++j) v += H[(int64_t)i * M + j] * rec.B[(int64_t)j * rec.ldb + a];
      PB[i * DARE_MAX_P + a] = v;
    }
    __syncthreads();
    if (tid < p * p) {
      const int a = tid / p, b = tid % p;
      double v = 0.0;
      for (int i = 0; i < m; ++i) v += rec.B[(int64_t)i * rec.ldb + a] * PB[i * DARE_MAX_P + b];
      s.rowd[tid] = v;
    }
    for (int e = tid; e < p * m; e += DARE_THREADS) {
      const int a = e / m, j = e % m;
      double v = 0.0;
      for (int i = 0; i < m; ++i) v += PB[i * DARE_MAX_P + a] * rec.A[(int64_t)i * rec.lda + j];
      F[(int64_t)a * M + j] = v;
    }
    __syncthreads();
    if (tid < p * p) {
      const int a = tid / p, b = tid % p;
      const double r = rec.R ? rec.R[a * p + b] : (a == b ? 1.0 : 0.0);
      s.S[a * DARE_MAX_P + b] = r + 0.5 * (s.rowd[a * p + b] + s.rowd[b * p + a]);
    }
    __syncthreads();
    if (tid == 0) s.flag[1] = dare_small_chol(s.S, p) ? 0 : 1;
    __syncthreads();
    if (s.flag[1]) status = 2;
  }
  if (status == 0) {
    double* F = T + (int64_t)M * DARE_MAX_P;
    for (int j = tid; j < m; j += DARE_THREADS) {
      double y[DARE_MAX_P];  // fully unrolled: stays in registers
#pragma unroll
      for (int a = 0; a < DARE_MAX_P; ++a) {
        if (a < p) {
          double v = F[(int64_t)a * M + j];
#pragma unroll
          for (int k = 0; k < a; ++k) v -= s.S[a * DARE_MAX_P + k] * y[k];
          y[a] = v / s.S[a * DARE_MAX_P + a];
        }
      }
#pragma unroll
      for (int a = DARE_MAX_P - 1; a >= 0; --a) {
        if (a < p) {
          double v = y[a];
#pragma unroll
          for (int k = a + 1; k < DARE_MAX_P; ++k)
            if (k < p) v -= s.S[k * DARE_MAX_P + a] * y[k];
          y[a] = v / s.S[a * DARE_MAX_P + a];
        }
      }
#pragma unroll
      for (int a = 0; a < DARE_MAX_P; ++a)
        if (a < p) rec.outK[(int64_t)a * m + j] = y[a];
    }
    if (rec.outP)
      for (int e = tid; e < m * m; e += DARE_THREADS) rec.outP[e] = H[(int64_t)(e / m) * M + e % m];
  } else {
    const double nan = __builtin_nan("");
    for (int e = tid; e < p * m; e += DARE_THREADS) rec.outK[e] = nan;
    if (rec.outP)
      for (int e = tid; e < m * m; e += DARE_THREADS) rec.outP[e] = nan;
  }
  if (tid == 0) {
    *rec.status = status;
    *rec.iters = iters;
    if (rec.delta) *rec.delta = s.scal[0];
  }
}

int launch_dare(nk_ctx* ctx, const DareRec* table_dev, int count, double tol, int max_iter) {
  NK_REQUIRE(table_dev != nullptr && count >= 1 && max_iter >= 0, "dare: bad launch arguments");
  hipLaunchKernelGGL(dare_batch_kernel, dim3(count), dim3(DARE_THREADS), 0, ctx->stream, table_dev, tol, max_iter);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
