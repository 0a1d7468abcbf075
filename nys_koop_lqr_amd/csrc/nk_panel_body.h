// Panel solve of the blocked Cholesky, per 16 rows: shared by the launch-per-step chain (nk_trail.hip) and the dataflow
// factorisation (nk_chol_flow.hip), so that both compute the same bits.
#pragma once
#include "nk_chol.h"
#include "nk_potrf_body.h"  // (d4)

namespace nk {

// ---------------------------------------------------------------------------------------------------------------
// Panel solve of one block step:  P <- P L_jj^-T  (rows x 64 against the 64 x 64 diagonal block; in place: a workgroup reads
// exactly the 64 rows it writes, and only after all of them have been read).  Register-only like the trailing update.
//
// The product with the explicitly inverted block, P1 = P Linv^T, is what makes this step a GEMM -- and on its own it is not
// backward stable: its error grows with cond(L_jj) (2e6 on the first block of config 2's system), and through it the whole
// blocked solve carried a backward error of 6 eps where LAPACK's substitution leaves 0.3 eps (tools/illcond_diag.py; the
// same numbers from a NumPy emulation of this algorithm).  One correction step from the DATA restores it,
//     P2 = P1 + (P - P1 L_jj^T) Linv^T,
// three 64-wide products instead of one.  All three run on the matrix pipe in the TRANSPOSED form (D = Linv P^T: output
// column = panel row), because in that form the accumulator of one product is, register for register, the b-operand of the
// next: lane (l15, l4) of an accumulator holds P1[r(l15)][4 t + l4], t = 4 j + reg, and with the contraction index dealt as
// k = 4 t + l4 that is exactly the b-operand of instruction t -- no LDS, no lane exchange.  The raw panel rows are loaded in
// the same dealing and serve both as b-operand of the first product and as the minuend of the residual.
// Columns beyond `nb` (a short last block; only the right-hand-side rows of an augmented system get there) are masked.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PANEL_ROWS = CHOL_PANEL_ROWS;  // rows per workgroup of the panel solve: four waves of 16
// Rows m0 .. m0 + 15 of the panel, one wave (lane 0..63); every wave of the workgroup calls it (one barrier inside).
__device__ __forceinline__ void chol_panel_rows(const PanelSys& s, int m0, int lane) {
  __builtin_amdgcn_s_setprio(2);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int nb = s.nb;
  const double* __restrict__ Li = s.Linv;
  const double* __restrict__ Ld = s.Linv + CHOL_NB * CHOL_NB;
  // raw rows: a[t] = P[r][4 t + l4]
  double a[16];
  {
    const double* pr = s.P + (int64_t)min(m0 + l15, s.rows - 1) * s.ldp + l4;
    if (nb == CHOL_NB) {
#pragma unroll
      for (int t = 0; t < 16; ++t) a[t] = pr[4 * t];
    } else {
#pragma unroll
      for (int t = 0; t < 16; ++t) a[t] = (4 * t + l4 < nb) ? pr[4 * t] : 0.0;
    }
  }
  // a-operands: rows of the inverse, k = 4 t + l4
  double li[4][16];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 16; ++t) li[j][t] = Li[(16 * j + l15) * CHOL_NB + 4 * t + l4];
  // 1.  P1 = P Linv^T
  // (t outer, j inner everywhere: four independent accumulator chains in flight -- a dependent fp64 matrix instruction waits
  // ~200 cycles for its predecessor, three times its issue interval)
  d4 p1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) p1[j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) p1[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(li[j][t], a[t], p1[j], 0, 0, 0);
  if (s.fix == 2 || (s.fix == 1 && s.Linv[2 * CHOL_NB * CHOL_NB] != 0.0)) {  // (uniform: one word per block)
    // 2.  Rsd = P - P1 L_jj^T   (a-operand: minus the rows of the factor block; the accumulator starts from the raw rows)
    d4 rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rs[j] = d4{a[4 * j], a[4 * j + 1], a[4 * j + 2], a[4 * j + 3]};
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rs[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Ld[(16 * j + l15) * CHOL_NB + 4 * t + l4], p1[t >> 2][t & 3], rs[j], 0, 0, 0);
    // 3.  P2 = P1 + Rsd Linv^T
    d4 p2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) p2[j] = p1[j];
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) p2[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(li[j][t], rs[t >> 2][t & 3], p2[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) p1[j] = p2[j];
  }
  // every wave of the workgroup must have its raw rows in registers before any wave overwrites (waves own disjoint
  // rows, so this is only needed against the clamped loads of the last, partial tile)
  __syncthreads();
  const int row = m0 + l15;
  if (row < s.rows) {
    double* pw = s.P + (int64_t)row * s.ldp + l4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (nb == CHOL_NB || 16 * j + 4 * reg + l4 < nb) pw[16 * j + 4 * reg] = p1[j][reg];
  }
}

}  // namespace nk
