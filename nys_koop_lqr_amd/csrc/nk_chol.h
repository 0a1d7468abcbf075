// Blocked Cholesky: the host interface (nk_chol.hip, nk_chol_flow.hip), the argument records of its kernels and their
// launchers (nk_potrf.hip, nk_trail.hip, nk_trsm.hip).  The block geometry is nk_chol_plan.h.
#pragma once
#include <stdlib.h>

#include "nk_common.h"
#include "nk_chol_plan.h"

namespace nk {

// in-place lower Cholesky of P (m x m, ld), Linv workspace holds inverted diagonal blocks
int cholesky_lower(nk_ctx* ctx, double* P, int64_t ldp, int m, double* Linv /* nblk*CHOL_WS */);
int cholesky_solve(nk_ctx* ctx, const double* L, int64_t ldl, int m, const double* Linv, double* R, int64_t ldr,
                   int nrhs);  // R <- (L L^T)^{-1} R in place
// the same for TWO independent systems advanced in lock step, every per-block kernel launched once for both
// (the chains are latency bound: pairing halves their length)
struct CholSys {
  double* P = nullptr;   // matrix, overwritten by its lower factor
  int64_t ldp = 0;
  int m = 0;
  // Augmented form (cholesky_aug_pair): `extra` further rows below the m x m matrix hold the right-hand sides
  // TRANSPOSED (extra x m); the factorisation's panel / trailing updates carry them along (= forward substitution for
  // free) and a backward pass leaves X^T = (P^-1 R)^T = R^T P^-1 in their place.
  int extra = 0;
  bool backward = true;  // false: stop after the factorisation (the extra rows then hold R^T L^-T)
  double* Linv = nullptr;
  double* pivlog = nullptr;  // optional device array of m doubles: the factorisation logs every pivot here
  double* R = nullptr;   // right-hand sides (solve only), overwritten by the solution
  int64_t ldr = 0;
  int nrhs = 0;
};
int cholesky_lower_pair(nk_ctx* ctx, const CholSys* sys, int nsys);
int cholesky_lower_pair_async(nk_ctx* ctx, const CholSys* sys, int nsys);  // no host synchronisation
int cholesky_check_pair(nk_ctx* ctx, const CholSys* sys, int nsys);       // verdict of the async factorisation
int cholesky_solve_pair(nk_ctx* ctx, const CholSys* sys, int nsys);
// factor + backward substitution on the extra rows, no host sync
// pause / pause_step: before block step pause_step the chain's stream waits for the (already recorded) event `pause`
int cholesky_aug_pair_async(nk_ctx* ctx, const CholSys* sys, int nsys, hipEvent_t pause = nullptr, int pause_step = -1);
// which systems of the last (paired) factorisation on the current stream met a non-positive pivot (synchronises)
// piv_ratio (optional, nsys entries): smallest / largest pivot of each factorisation (0 when it failed)
int cholesky_fail_flags(nk_ctx* ctx, const CholSys* sys, int nsys, int* failed /* nsys entries */, double* piv_ratio = nullptr);

constexpr int CHOL_NB = CHOL_BLOCK;
static_assert(CHOL_NB == 64, "the kernels of the chain are written for 64 x 64 blocks (one lane per row, K = 64 rank updates)");
// workspace per diagonal block of a blocked factorisation (CholSys::Linv): the inverted 64 x 64 diagonal block of the factor
// followed by the diagonal block itself, both dense row-major with exact zeros above the diagonal and identity padding
// beyond a short last block.  The factor rides along because every product with the explicit inverse is followed by one
// correction step  x += (b - x L_jj) L_jj^-1  (see chol_panel_kernel): multiplying by an explicit inverse alone is not
// backward stable -- its error grows with cond(L_jj), 1e6 on the kernel matrices here.
constexpr int CHOL_WS = 2 * CHOL_NB * CHOL_NB + 8;  // (+ one verdict word, padded to 64 bytes)
// the verdict word behind the two blocks: 1.0 when ||L_jj||_F ||L_jj^-1||_F exceeds this and the products with the inverse
// take the correction step (potrf_diag_kernel)
constexpr double CHOL_FIX_KAPPA = 8.0 * CHOL_NB;
// NYSKOOP_CHOL_FIX (read per launch: same-process A/B; for measurements only): 0 = never correct, 2 = always, default 1 = where
// the verdict word says so
inline int chol_fix_enabled() {
  const char* e = getenv("NYSKOOP_CHOL_FIX");
  return (e && e[0] == '0') ? 0 : ((e && e[0] == '2') ? 2 : 1);
}
inline bool chol_fuse_enabled() {  // NYSKOOP_CHOL_FUSE=0 (read per call): separate launches, for A/B runs and the bit-identity test
  const char* e = getenv("NYSKOOP_CHOL_FUSE");
  return !(e && e[0] == '0');
}
// the factorisation of cholesky_aug_pair_async as one tile-dataflow launch (nk_chol_flow.hip): same bits as the chain;
// NYSKOOP_CHOL_FLOW=0 (read per call) keeps the launch-per-step chain
bool chol_flow_enabled();
int cholesky_flow_pair(nk_ctx* ctx, const CholSys* sys, int nsys);
// failure flag of the systems of a dataflow factorisation that stopped waiting (a bounded wait ran out): cholesky_fail_flags
// reports it as is (failed[q] == CHOL_FLOW_GIVEUP) and counts CNT_CHOL_FLOW_GIVEUP; the caller re-runs the chain
constexpr int CHOL_FLOW_GIVEUP = -0x40000000;

// ---- argument records of the chain's kernels, one slot per system of a pair (a slot without work keeps its zeros)
struct PotrfBatch {  // potrf_diag_kernel (nk_potrf_body.h)
  double* A[2];
  int64_t lda[2];
  int nb[2];                   // order of the block; 0: the system has none
  double* Linv[2];             // its CHOL_WS workspace
  int* info[2];
  unsigned long long* piv[2];  // [min, max] pivot of the whole factorisation as bit patterns (positive doubles order like
                               // their bit patterns)
  double* plog[2];             // optional: every pivot of this block, in order (the numerical-rank verdict of
                               // cholesky_fail_flags looks for an isolated cluster of rounding-level pivots)
};
struct PanelSys {  // chol_panel_kernel (nk_panel_body.h)
  double* P;
  int64_t ldp;
  const double* Linv;  // CHOL_WS doubles: 64 x 64 inverse, then the 64 x 64 factor block (dense, identity padded)
  int rows;
  int nb;              // valid columns of the block
  int fix;             // correction step: 0 never, 1 where the block's verdict word says so, 2 always
  int nblocks;         // chol_panel_workgroups(rows)
};
struct PanelBatch {
  PanelSys s[2];
};
struct TrailSys {  // chol_trail_kernel (nk_trail.hip)
  const double* P;  // panel: rows x 64
  int64_t ldp;
  double* C;        // trailing matrix: rows x rem (lower tiles of the leading rem x rem part + all tiles below it)
  int64_t ldc;
  int rows, rem;
  int tiles_n;      // chol_trail_tiles(rows, rem)
  int nblocks;      // ... and its workgroups
};
struct TrailBatch {
  TrailSys s[2];
};

// ---- launchers: each takes finished records (nk_chol.hip fills them from the plan) and launches nothing when no slot has work
// diagonal blocks of step `blk` (nk_potrf.hip); failures are flagged through pb.info
int launch_potrf_diag_pair(nk_ctx* ctx, const PotrfBatch& pb, int blk);
// panel solves P <- P L_jj^-T (nk_trail.hip)
int launch_chol_panel_pair(nk_ctx* ctx, const PanelBatch& pb);
// trailing updates C -= P P^T, K = 64 (nk_trail.hip)
int launch_chol_trail_pair(nk_ctx* ctx, const TrailBatch& tb);
// ... fused with the diagonal-block factorisation of the NEXT block step `blk` (pb.A[q] == tb.s[q].C): one launch instead of
// two, the diagonal kernel off the critical path
int launch_chol_trail_potrf_pair(nk_ctx* ctx, const TrailBatch& tb, const PotrfBatch& pb, int blk);
// E_q <- E_q L_q^-1 on the extra rows of up to two factored systems, one launch (nk_trsm.hip)
int launch_trsm_right_lower_pair(nk_ctx* ctx, const CholSys* sys, int nsys);

}  // namespace nk
