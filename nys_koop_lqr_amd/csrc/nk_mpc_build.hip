// The controllers of the MPC sweeps, built on the device: for many independent units in one launch, the Newton polish of
// the Riccati stage's gain, the condensed problem (H, F) of lqr.mpc_condense and the output rows (G, T) of
// lqr.mpc_condense_outputs.  ONE workgroup of 256 threads owns ONE unit from its first to its last instruction: nothing
// crosses workgroups (no flags, no spinning), every loop is bounded by N, m, p or an iteration cap.
//
// Stages (lqr.dare_newton_smith, lqr.mpc_condense_blocked and lqr.mpc_condense_outputs are the NumPy statements):
//   1. Newton (Hewer) steps from the Riccati stage's K and P, each as a correction of P:  Ac = A - B K,
//      Y = sym((Ac'P Ac - P) + (Q + K'RK)), then the squared Smith iteration  D = sym(Ac' Y Ac), Y += D, stop at
//      |D|_1 <= tol |Y|_1, else Ac = Ac Ac;  P += Y,  K = (R + sym(B'PB))^-1 B'PA.
//   2. The stacks G_k = A^k B (one m x m by m x p product each), Q G and P G (one product each).
//   3. Horner, all block columns at once: for l = N .. 0:  W = A' W;  block column j of W += (P if l == N else Q) G_{l-1-j}
//      for j < min(l, N);  for l >= 1 block row l-1 of H, columns 0 .. l-1, = 2 B' W.  F = 2 W'.
//   4. H is mirrored from its lower triangle, the diagonal blocks get + 2 sym(R): H leaves the kernel bitwise symmetric.
//   5. Output rows: R_0 = the selected rows of C, R_k = R_{k-1} A (row k of T), R_{k-1} B (the blocks of G; the blocks
//      above the diagonal are written as exact zeros).
// Every product with a dimension of 16 or more goes through wg_gemm (v_mfma_f64_16x16x4_f64, nk_wg_gemm.h); operands whose
// sizes are no multiple of 16 are read through its bounds-checked operand form and padded with zeros.  W is double
// buffered (wg_gemm's result must not overlap its operands).  Every summation order is fixed by (m, p, N, nc, Ny) alone.
// Workspace (device memory, per unit, touched by its own workgroup only, ordered by __syncthreads()): nk_mpc_build_pack.h.
#include "nk_common.h"
#include "nk_wg_gemm.h"

namespace nk {

constexpr int MB_P = MPC_BUILD_MAX_P;

struct MpcBuildLds : WgGemmLds {  // As, Bs: the panels of wg_gemm
  double rowd[MPC_BUILD_MAX_M];  // row sums of |D|
  double rowh[MPC_BUILD_MAX_M];  // row sums of |X|
  double S[MB_P * MB_P];         // p x p systems and their Cholesky factors
  double Rs[MB_P * MB_P];        // R (identity when the record has none)
  double bpb[MB_P * MB_P];
  int flag[4];                   // [1] failure, [2] converged
};

// lower Cholesky factor of the p x p matrix in S (row stride MB_P), in place, by one thread
__device__ bool mb_small_chol(double* S, int p) {
  for (int j = 0; j < p; ++j) {
    double d = S[j * MB_P + j];
    for (int k = 0; k < j; ++k) d -= S[j * MB_P + k] * S[j * MB_P + k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    d = sqrt(d);
    S[j * MB_P + j] = d;
    for (int i = j + 1; i < p; ++i) {
      double v = S[i * MB_P + j];
      for (int k = 0; k < j; ++k) v -= S[i * MB_P + k] * S[j * MB_P + k];
      S[i * MB_P + j] = v / d;
    }
  }
  return true;
}

// K = (R + sym(B'XB))^-1 B'XA into outK (p x m dense), X in the padded M x M slot; PB (m x MB_P) and F (p rows of stride M)
// are temporaries.  Returns false (for every thread alike) when R + B'XB is not positive definite.
__device__ bool mb_gain(const MpcBuildRec& rec, const double* X, double* PB, double* F, double* outK, MpcBuildLds& s) {
  const int tid = threadIdx.x, m = rec.m, p = rec.p, M = rec.M;
  for (int e = tid; e < m * p; e += DARE_THREADS) {
    const int i = e / p, a = e % p;
    double v = 0.0;
    for (int j = 0; j < m; ++j) v += X[(int64_t)i * M + j] * rec.B[(int64_t)j * rec.ldb + a];
    PB[i * MB_P + a] = v;
  }
  __syncthreads();
  if (tid < p * p) {
    const int a = tid / p, b = tid % p;
    double v = 0.0;
    for (int i = 0; i < m; ++i) v += rec.B[(int64_t)i * rec.ldb + a] * PB[i * MB_P + b];
    s.bpb[a * MB_P + b] = v;
  }
  for (int e = tid; e < p * m; e += DARE_THREADS) {
    const int a = e / m, j = e % m;
    double v = 0.0;
    for (int i = 0; i < m; ++i) v += PB[i * MB_P + a] * rec.A[(int64_t)i * rec.lda + j];
    F[(int64_t)a * M + j] = v;
  }
  __syncthreads();
  if (tid < p * p) {
    const int a = tid / p, b = tid % p;
    s.S[a * MB_P + b] = s.Rs[a * MB_P + b] + 0.5 * (s.bpb[a * MB_P + b] + s.bpb[b * MB_P + a]);
  }
  __syncthreads();
  if (tid == 0) s.flag[1] = mb_small_chol(s.S, p) ? 0 : 1;
  __syncthreads();
  if (s.flag[1]) return false;
  for (int j = tid; j < m; j += DARE_THREADS) {
    double y[MB_P];  // fully unrolled: stays in registers
#pragma unroll
    for (int a = 0; a < MB_P; ++a) {
      if (a < p) {
        double v = F[(int64_t)a * M + j];
#pragma unroll
        for (int k = 0; k < a; ++k) v -= s.S[a * MB_P + k] * y[k];
        y[a] = v / s.S[a * MB_P + a];
      }
    }
#pragma unroll
    for (int a = MB_P - 1; a >= 0; --a) {
      if (a < p) {
        double v = y[a];
#pragma unroll
        for (int k = a + 1; k < MB_P; ++k)
          if (k < p) v -= s.S[k * MB_P + a] * y[k];
        y[a] = v / s.S[a * MB_P + a];
      }
    }
#pragma unroll
    for (int a = 0; a < MB_P; ++a)
      if (a < p) outK[(int64_t)a * m + j] = y[a];
  }
  __syncthreads();
  return true;
}

__global__ void __launch_bounds__(DARE_THREADS, 2) mpc_build_kernel(const MpcBuildRec* table, double ntol, int nmax) {
  __shared__ MpcBuildLds s;
  const MpcBuildRec rec = table[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = rec.m, p = rec.p, N = rec.N, nc = rec.nc, Ny = rec.Ny, M = rec.M, NVP = rec.NVP;
  const int nv = N * p;
  const int64_t MM = (int64_t)M * M, MW = (int64_t)M * NVP;
  double* Qm = rec.sq;
  double* X = Qm + MM;
  double* Ac = X + MM;
  double* T = Ac + MM;
  double* D = T + MM;
  double* Y = D + MM;  // the correction of a Newton step
  double* Gs = rec.wide;
  double* QG = Gs + MW;
  double* PG = QG + MW;
  double* Wc = PG + MW;
  double* Wn = Wc + MW;
  double* t16 = Wn + MW;                  // M x 16
  double* Ra = t16 + (int64_t)16 * M;     // 16 x M
  double* Rb = Ra + (int64_t)16 * M;      // 16 x M
  double* tH = Rb + (int64_t)16 * M;      // 16 x NVP
  double* RB = tH + (int64_t)16 * NVP;    // Ny x nc x p
  const DareOp opA{rec.A, rec.lda, m, m, false};
  const DareOp opAt{rec.A, rec.lda, m, m, true};

  int status = rec.pre_status ? *rec.pre_status : rec.pre_status_imm;
  int squarings = 0;

  if (status == 0) {
    // ---- the cost, R and the terminal cost in their padded places -----------------------------------------------------
    if (rec.C) {  // Q = c sym(C'C), the product and the symmetrisation of the Riccati kernel
      const DareOp Ct{rec.C, rec.ldc, rec.d, m, true};
      const DareOp Cn{rec.C, rec.ldc, rec.d, m, false};
      wg_gemm<0>(T, M, M, M, rec.d, Ct, Cn, s);
      for (int64_t e = tid; e < MM; e += DARE_THREADS) {
        const int i = (int)(e / M), j = (int)(e % M);
        Qm[e] = rec.c * (0.5 * (T[e] + T[(int64_t)j * M + i]));
      }
    } else {
      for (int64_t e = tid; e < MM; e += DARE_THREADS) {
        const int i = (int)(e / M), j = (int)(e % M);
        Qm[e] = (i < m && j < m) ? rec.Q[(int64_t)i * rec.ldq + j] : 0.0;
      }
    }
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      X[e] = (i < m && j < m) ? rec.Pin[(int64_t)i * m + j] : 0.0;
    }
    if (tid < MB_P * MB_P) {
      const int a = tid / MB_P, b = tid % MB_P;
      const double r = (a < p && b < p) ? (rec.R ? rec.R[a * p + b] : (a == b ? 1.0 : 0.0)) : 0.0;
      s.Rs[tid] = r;
      s.S[tid] = r;
    }
    if (tid == 0) { s.flag[1] = 0; s.flag[2] = 0; }
    __syncthreads();
    if (tid == 0 && !mb_small_chol(s.S, p)) s.flag[1] = 1;
    __syncthreads();
    if (s.flag[1]) status = 2;
  }

  // ---- the gain: the Riccati stage's, polished by Newton steps; or formed from the given terminal cost -----------------
  if (status == 0) {
    if (rec.Kin) {
      for (int e = tid; e < p * m; e += DARE_THREADS) rec.outK[e] = rec.Kin[e];
      __syncthreads();
    } else if (!mb_gain(rec, X, t16, Ra, rec.outK, s)) {
      status = 2;
    }
  }
  for (int step = 0; step < rec.newton_steps && rec.Kin && status == 0; ++step) {
    const double* K = rec.outK;
    // Ac = A - B K and Q + (K'R) K into Y; then the residual (Ac'X Ac - X) + (Q + K'RK) of the current X, symmetrised
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      double ac = 0.0, x0 = 0.0;
      if (i < m && j < m) {
        double bk = 0.0, krk = 0.0;
#pragma unroll
        for (int a = 0; a < MB_P; ++a)
          if (a < p) bk += rec.B[(int64_t)i * rec.ldb + a] * K[(int64_t)a * m + j];
        ac = rec.A[(int64_t)i * rec.lda + j] - bk;
#pragma unroll
        for (int b = 0; b < MB_P; ++b) {
          if (b < p) {
            double kr = 0.0;
#pragma unroll
            for (int a = 0; a < MB_P; ++a)
              if (a < p) kr += K[(int64_t)a * m + i] * s.Rs[a * MB_P + b];
            krk += kr * K[(int64_t)b * m + j];
          }
        }
        x0 = Qm[e] + krk;
      }
      Ac[e] = ac;
      Y[e] = x0;
    }
    __syncthreads();
    wg_gemm<0>(T, M, M, M, M, DareOp{Ac, M, M, M, true}, DareOp{X, M, M, M, false}, s);
    wg_gemm<0>(D, M, M, M, M, DareOp{T, M, M, M, false}, DareOp{Ac, M, M, M, false}, s);
    for (int64_t e = tid; e < MM; e += DARE_THREADS) D[e] = (D[e] - X[e]) + Y[e];
    __syncthreads();
    for (int64_t e = tid; e < MM; e += DARE_THREADS) {
      const int i = (int)(e / M), j = (int)(e % M);
      Y[e] = 0.5 * (D[e] + D[(int64_t)j * M + i]);
    }
    __syncthreads();
    // the squared Smith iteration on the correction Y
    bool converged = false;
    for (int it = 0; it < nmax && status == 0 && !converged; ++it) {
      wg_gemm<0>(T, M, M, M, M, DareOp{Ac, M, M, M, true}, DareOp{Y, M, M, M, false}, s);
      wg_gemm<0>(D, M, M, M, M, DareOp{T, M, M, M, false}, DareOp{Ac, M, M, M, false}, s);
      for (int i = wave; i < M; i += DARE_THREADS / 64) {
        double sd = 0.0, sh = 0.0;
        for (int j = lane; j < M; j += 64) {
          const double d = 0.5 * (D[(int64_t)i * M + j] + D[(int64_t)j * M + i]);
          const double y = Y[(int64_t)i * M + j] + d;
          Y[(int64_t)i * M + j] = y;
          sd += fabs(d);
          sh += fabs(y);
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
        s.flag[2] = (finite && nd <= ntol * nh) ? 1 : 0;
      }
      __syncthreads();
      ++squarings;
      if (s.flag[1]) { status = 2; break; }
      converged = s.flag[2] != 0;
      if (!converged) {
        wg_gemm<0>(T, M, M, M, M, DareOp{Ac, M, M, M, false}, DareOp{Ac, M, M, M, false}, s);
        double* t = Ac; Ac = T; T = t;
      }
    }
    if (status == 0 && converged) {
      for (int64_t e = tid; e < MM; e += DARE_THREADS) X[e] += Y[e];
      __syncthreads();
    }
    if (status == 0 && !converged) status = 3;
    if (status == 0 && !mb_gain(rec, X, t16, Ra, rec.outK, s)) status = 2;
  }
  __syncthreads();

  if (status == 0) {
    if (rec.outP)
      for (int e = tid; e < m * m; e += DARE_THREADS) rec.outP[e] = X[(int64_t)(e / m) * M + e % m];

    // ---- the stacks G_k = A^k B, Q G, P G ---------------------------------------------------------------------------------
    for (int64_t e = tid; e < MW; e += DARE_THREADS) {
      const int i = (int)(e / NVP), c = (int)(e % NVP);
      Gs[e] = (i < m && c < p) ? rec.B[(int64_t)i * rec.ldb + c] : 0.0;
      Wc[e] = 0.0;
    }
    __syncthreads();
    for (int k = 1; k < N; ++k) {
      wg_gemm<0>(t16, 16, M, 16, m, opA, DareOp{Gs + (k - 1) * p, NVP, m, p, false}, s);
      for (int e = tid; e < m * p; e += DARE_THREADS) Gs[(int64_t)(e / p) * NVP + k * p + e % p] = t16[(e / p) * 16 + e % p];
      __syncthreads();
    }
    wg_gemm<0>(QG, NVP, M, NVP, M, DareOp{Qm, M, M, M, false}, DareOp{Gs, NVP, M, NVP, false}, s);
    wg_gemm<0>(PG, NVP, M, NVP, M, DareOp{X, M, M, M, false}, DareOp{Gs, NVP, M, NVP, false}, s);

    // ---- Horner on all block columns; the lower block rows of H as it goes ------------------------------------------------
    for (int l = N; l >= 0; --l) {
      if (l == N) {  // A' 0
        for (int64_t e = tid; e < MW; e += DARE_THREADS) Wn[e] = 0.0;
        __syncthreads();
      } else {
        wg_gemm<0>(Wn, NVP, M, NVP, m, opAt, DareOp{Wc, NVP, M, NVP, false}, s);
      }
      const double* src = l == N ? PG : QG;
      const int ncol = (l < N ? l : N) * p;
      for (int64_t e = tid; e < (int64_t)M * ncol; e += DARE_THREADS) {
        const int i = (int)(e / ncol), c = (int)(e % ncol);
        const int j = c / p, a = c % p;
        Wn[(int64_t)i * NVP + c] += src[(int64_t)i * NVP + (l - 1 - j) * p + a];
      }
      __syncthreads();
      if (l >= 1) {
        wg_gemm<0>(tH, NVP, 16, NVP, m, DareOp{rec.B, rec.ldb, m, p, true}, DareOp{Wn, NVP, M, NVP, false}, s);
        for (int e = tid; e < p * l * p; e += DARE_THREADS) {
          const int a = e / (l * p), c = e % (l * p);
          rec.outH[(int64_t)((l - 1) * p + a) * nv + c] = 2.0 * tH[(int64_t)a * NVP + c];
        }
        __syncthreads();
      }
      double* t = Wc; Wc = Wn; Wn = t;
    }
    for (int64_t e = tid; e < (int64_t)nv * m; e += DARE_THREADS) {
      const int c = (int)(e / m), i = (int)(e % m);
      rec.outF[e] = 2.0 * Wc[(int64_t)i * NVP + c];
    }
    // ---- H from its lower triangle; + 2 sym(R) on the diagonal blocks (one thread per pair writes both entries) -----------
    for (int e = tid; e < nv * nv; e += DARE_THREADS) {
      const int r = e / nv, c = e % nv;
      if (c > r) continue;
      double v = rec.outH[(int64_t)r * nv + c];
      if (r / p == c / p) {
        const int a = r % p, b = c % p;
        v = v + 2.0 * ((s.Rs[a * MB_P + b] + s.Rs[b * MB_P + a]) / 2);
      }
      rec.outH[(int64_t)r * nv + c] = v;
      rec.outH[(int64_t)c * nv + r] = v;
    }
    __syncthreads();

    // ---- output rows ------------------------------------------------------------------------------------------------------
    if (nc > 0) {
      for (int e = tid; e < 16 * M; e += DARE_THREADS) {
        const int c = e / M, j = e % M;
        // comps is read from the table: indexing the copy of the record would put it in scratch
        Ra[e] = (c < nc && j < m) ? rec.Crows[(int64_t)table[blockIdx.x].comps[c] * rec.ldcr + j] : 0.0;
      }
      __syncthreads();
      for (int k = 1; k <= Ny; ++k) {
        if (tid < nc * p) {  // R_{k-1} B
          const int c = tid / p, a = tid % p;
          double v = 0.0;
          for (int i = 0; i < m; ++i) v += Ra[c * M + i] * rec.B[(int64_t)i * rec.ldb + a];
          RB[((k - 1) * nc + c) * p + a] = v;
        }
        wg_gemm<0>(Rb, M, 16, M, m, DareOp{Ra, M, 16, M, false}, opA, s);
        for (int e = tid; e < nc * m; e += DARE_THREADS)
          rec.outT[(int64_t)((k - 1) * nc + e / m) * m + e % m] = Rb[(e / m) * M + e % m];
        double* t = Ra; Ra = Rb; Rb = t;
      }
      __syncthreads();
      for (int e = tid; e < Ny * nc * nv; e += DARE_THREADS) {
        const int row = e / nv, col = e % nv;
        const int k = row / nc + 1, c = row % nc, j = col / p, a = col % p;
        rec.outG[e] = j < k ? RB[((k - 1 - j) * nc + c) * p + a] : 0.0;
      }
    }
    __syncthreads();

    // ---- non-finite results are a failure -----------------------------------------------------------------------------------
    bool bad = false;
    for (int e = tid; e < nv * nv; e += DARE_THREADS) bad = bad || !isfinite(rec.outH[e]);
    for (int64_t e = tid; e < (int64_t)nv * m; e += DARE_THREADS) bad = bad || !isfinite(rec.outF[e]);
    for (int e = tid; e < p * m; e += DARE_THREADS) bad = bad || !isfinite(rec.outK[e]);
    if (nc > 0) {
      for (int e = tid; e < Ny * nc * nv; e += DARE_THREADS) bad = bad || !isfinite(rec.outG[e]);
      for (int64_t e = tid; e < (int64_t)Ny * nc * m; e += DARE_THREADS) bad = bad || !isfinite(rec.outT[e]);
    }
    if (__syncthreads_or(bad ? 1 : 0)) status = 2;
  }

  if (status != 0) {
    const double nan = __builtin_nan("");
    for (int e = tid; e < nv * nv; e += DARE_THREADS) rec.outH[e] = nan;
    for (int64_t e = tid; e < (int64_t)nv * m; e += DARE_THREADS) rec.outF[e] = nan;
    for (int e = tid; e < p * m; e += DARE_THREADS) rec.outK[e] = nan;
    if (rec.outP)
      for (int e = tid; e < m * m; e += DARE_THREADS) rec.outP[e] = nan;
    if (nc > 0) {
      for (int e = tid; e < Ny * nc * nv; e += DARE_THREADS) rec.outG[e] = nan;
      for (int64_t e = tid; e < (int64_t)Ny * nc * m; e += DARE_THREADS) rec.outT[e] = nan;
    }
  }
  if (tid == 0) {
    *rec.status = status;
    *rec.iters = squarings;
  }
}

int launch_mpc_build(nk_ctx* ctx, const MpcBuildRec* table_dev, int count, double newton_tol, int newton_max_iter) {
  NK_REQUIRE(table_dev != nullptr && count >= 1 && newton_max_iter >= 0, "mpc_build: bad launch arguments");
  hipLaunchKernelGGL(mpc_build_kernel, dim3(count), dim3(DARE_THREADS), 0, ctx->stream, table_dev, newton_tol,
                     newton_max_iter);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
