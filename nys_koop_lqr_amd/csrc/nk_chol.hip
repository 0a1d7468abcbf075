// Blocked Cholesky (lower) of up to two symmetric positive definite systems advanced in lock step, built on the fp64 MFMA
// GEMM engine, with inverted diagonal blocks: the plain factorisation with its block substitutions, and the augmented form
// with the right-hand sides riding along as extra rows + a single-launch backward substitution (nk_trsm.hip), replacing
// scipy.linalg.lstsq on the (numerically full-rank) regularised normal matrices (regressors.py:155,165).  A non-positive
// pivot is reported as NK_ERR_NOT_SPD; there is no silent rank truncation.
#include "nk_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace nk {

// ---------------------------------------------------------------------------------------------------------------
// blocked Cholesky (lower) with inverted diagonal blocks
// ---------------------------------------------------------------------------------------------------------------
// potrf_diag_kernel lives in nk_potrf.hip (fully unrolled, slow to compile)
int launch_potrf_diag_pair(nk_ctx* ctx, double* const* Ajj, const int64_t* lda, const int* nb, double* const* Linv,
                           int nsys, int blk, double* const* plog);

// failure flags and [min, max] pivot slots of the current stream's two systems: flags <- 0, min <- +inf, max <- 0
__device__ __forceinline__ void reset_pivots_kernel_body(int* info, unsigned long long* piv) {
  if (threadIdx.x < 4) piv[threadIdx.x] = (threadIdx.x & 1) ? 0ull : 0x7FF0000000000000ull;
  if (threadIdx.x < 2) info[threadIdx.x] = 0;
}
__global__ void __launch_bounds__(256) reset_pivots_kernel(int* info, unsigned long long* piv) { reset_pivots_kernel_body(info, piv); }
NK_BATCHED_TWIN(reset_pivots_kernel, (256), int*, unsigned long long*)
static int reset_pivots(nk_ctx* ctx) {
  hipLaunchKernelGGL(reset_pivots_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->d_info + info_base(ctx),
                     ctx->d_piv + 2 * info_base(ctx));
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// order, workspace and pivot log of diagonal block jb + 1 of every system (order 0: the system has no such block)
static void next_block(const CholSys* sys, int nsys, int jb, int* nbn, double** Lin, double** Pln) {
  constexpr int NB = CHOL_NB;
  const int j1 = (jb + 1) * NB;
  for (int q = 0; q < nsys; ++q) {
    const CholSys& y = sys[q];
    if (j1 >= y.m) continue;
    nbn[q] = y.m - j1 < NB ? y.m - j1 : NB;
    Lin[q] = y.Linv + (size_t)(jb + 1) * CHOL_WS;
    Pln[q] = y.pivlog ? y.pivlog + j1 : nullptr;
  }
}

// Operands of block step jb of up to two systems (a system that has no such block keeps order 0 and empty calls)
struct CholStep {
  double* Ajj[2] = {nullptr, nullptr};  // diagonal block
  double* Li[2] = {nullptr, nullptr};   // its workspace (CHOL_WS doubles)
  double* Pl[2] = {nullptr, nullptr};   // its slice of the pivot log
  int64_t lda[2] = {0, 0};
  int nbj[2] = {0, 0};                  // its order
  GemmCall panel[2], trail[2];
};
// extra[q]: rows below the m x m matrix of system q that ride along (the right-hand sides of the augmented form); zeros for
// the plain factorisation
static void chol_step_operands(const CholSys* sys, int nsys, int jb, const int* extra, CholStep* st) {
  constexpr int NB = CHOL_NB;
  const int j0 = jb * NB;
  for (int q = 0; q < nsys; ++q) {
    const CholSys& y = sys[q];
    if (j0 >= y.m) continue;
    const int nbj = st->nbj[q] = y.m - j0 < NB ? y.m - j0 : NB;
    st->Ajj[q] = y.P + (int64_t)j0 * y.ldp + j0;
    st->lda[q] = y.ldp;
    st->Li[q] = y.Linv + (size_t)jb * CHOL_WS;
    st->Pl[q] = y.pivlog ? y.pivlog + j0 : nullptr;
    const int rem = y.m - j0 - nbj;   // rows of the square part below the diagonal block
    const int rows = rem + extra[q];  // ... plus the extra rows
    if (rows <= 0) continue;
    double* pnl = y.P + (int64_t)(j0 + nbj) * y.ldp + j0;
    // panel <- panel * Linv_jj^T   (in place: one n-tile, every workgroup reads exactly the rows it writes)
    GemmCall& panel = st->panel[q];
    panel.M = rows; panel.N = nbj; panel.K = nbj;
    panel.A = pnl; panel.lda = y.ldp; panel.B = st->Li[q]; panel.ldb = NB;
    panel.C = pnl; panel.ldc = y.ldp;
    if (rem <= 0) continue;
    // trailing <- trailing - panel * panel^T  (lower tiles of the square part, full tiles for the extra rows)
    GemmCall& trail = st->trail[q];
    trail.M = rows; trail.N = rem; trail.K = nbj; trail.alpha = -1.0; trail.beta = 1.0;
    trail.A = pnl; trail.lda = y.ldp; trail.B = pnl; trail.ldb = y.ldp;
    trail.C = y.P + (int64_t)(j0 + nbj) * y.ldp + (j0 + nbj); trail.ldc = y.ldp;
    trail.opts.tri = TRI_LOWER;
  }
}

// K = 64 rank update: specialised kernel (nk_trail.hip), generic engine otherwise
static int chol_trail_update(nk_ctx* ctx, const GemmCall* calls, int nsys) {
  int rc_trail = NK_OK;
  if (!launch_chol_trail_pair(ctx, calls, nsys, &rc_trail)) NK_TRY(launch_gemm_pair(ctx, false, true, calls, nsys));
  return rc_trail;
}

// Launches of block step jb: the diagonal block unless the previous step's fused launch factored it (*diag_done), the panel,
// and -- with `trailing` -- the trailing update, in one launch with the factorisation of the next diagonal block where
// `fuse_next` asks for it and the shapes allow (*diag_done is then set for the next step).
static int chol_step_launches(nk_ctx* ctx, const CholSys* sys, int nsys, int jb, const CholStep& st, bool trailing,
                              bool fuse_next, bool* diag_done) {
  if (!*diag_done) NK_TRY(launch_potrf_diag_pair(ctx, st.Ajj, st.lda, st.nbj, st.Li, nsys, jb, st.Pl));
  *diag_done = false;
  {
    int rc_panel = NK_OK;  // 64 x 64 panel product: specialised kernel (nk_trail.hip), generic engine otherwise
    if (!launch_chol_panel_pair(ctx, st.panel, nsys, &rc_panel)) NK_TRY(launch_gemm_pair(ctx, false, true, st.panel, nsys));
    NK_TRY(rc_panel);
  }
  if (!trailing) return NK_OK;
  if (fuse_next) {
    int rc_f = NK_OK;
    int nbn[2] = {0, 0};
    double* Lin[2] = {nullptr, nullptr};
    double* Pln[2] = {nullptr, nullptr};
    next_block(sys, nsys, jb, nbn, Lin, Pln);
    if (launch_chol_trail_potrf_pair(ctx, st.trail, nsys, nbn, Lin, jb + 1, Pln, &rc_f)) {
      NK_TRY(rc_f);
      *diag_done = true;
      return NK_OK;
    }
  }
  return chol_trail_update(ctx, st.trail, nsys);
}

int cholesky_lower_pair_async(nk_ctx* ctx, const CholSys* sys, int nsys) {
  constexpr int NB = CHOL_NB;
  NK_REQUIRE(nsys >= 1 && nsys <= 2, "cholesky_lower_pair: 1..2 systems");
  NK_TRY(reset_pivots(ctx));
  int nblk = 0;
  for (int q = 0; q < nsys; ++q) nblk = std::max(nblk, (sys[q].m + NB - 1) / NB);
  const bool fuse = chol_fuse_enabled();
  const int no_extra[2] = {0, 0};  // (CholSys::extra is not read here)
  bool diag_done = false;
  for (int jb = 0; jb < nblk; ++jb) {
    CholStep st;
    chol_step_operands(sys, nsys, jb, no_extra, &st);
    NK_TRY(chol_step_launches(ctx, sys, nsys, jb, st, true, fuse && jb + 1 < nblk, &diag_done));
  }
  return NK_OK;
}

// Host-side verdict of the factorisations queued by cholesky_lower_pair_async (synchronises the current stream).
int cholesky_check_pair(nk_ctx* ctx, const CholSys* sys, int nsys) {
  int failed[2] = {0, 0};
  NK_TRY(cholesky_fail_flags(ctx, sys, nsys, failed));
  for (int q = 0; q < nsys; ++q)
    if (failed[q] != 0) {
      if (failed[q] > 0)
        set_error("Cholesky: non-positive pivot at index %d of %d (system %d is numerically rank deficient; the "
                  "reference's lstsq would truncate here)", failed[q] - 1, sys[q].m, q);
      else
        set_error("Cholesky: system %d (order %d) has an isolated cluster of rounding-level pivots: an exact null space (the "
                  "reference's lstsq truncates it)", q, sys[q].m);
      return NK_ERR_NOT_SPD;
    }
  return NK_OK;
}

// Verdict of the (paired) factorisation queued last on the current stream: failed[q] > 0 when system q met a
// non-positive pivot (index + 1), -1 when its pivots show an EXACT null space: a cluster of pivots at the rounding level of
// the factorisation (<= 8 m eps d_max) that a factor >= 1000 separates from all other pivots -- duplicated landmarks,
// a rank-deficient Gram matrix -- where rounding merely happened to leave the pivots positive.  (Needs sys[q].pivlog; without it
// only d_min <= eps d_max counts.)  A spectrum that decays CONTINUOUSLY to that level -- the ill-conditioned kernel systems of
// a hyper-parameter grid: genuine pivots of 1e-13 d_max across the whole gamma = 1e-7 row of the cloth grid -- has no such
// gap and is solved at full rank: there the reference's own rank decision is rounding noise and the
// SVD path would cost 100 x more for an answer no closer to it.  Synchronises the current stream.
int cholesky_fail_flags(nk_ctx* ctx, const CholSys* sys, int nsys, int* failed, double* piv_ratio) {
  const int ib = info_base(ctx);
  std::vector<double> plog[2];
  NK_HIP(hipMemcpyAsync(ctx->h_info + ib, ctx->d_info + ib, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipMemcpyAsync(ctx->h_piv + 2 * ib, ctx->d_piv + 2 * ib, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        ctx->stream));
  for (int q = 0; q < nsys; ++q)
    if (sys[q].pivlog) {
      plog[q].resize((size_t)sys[q].m);
      NK_HIP(hipMemcpyAsync(plog[q].data(), sys[q].pivlog, sizeof(double) * sys[q].m, hipMemcpyDeviceToHost, ctx->stream));
    }
  NK_HIP(hipStreamSynchronize(ctx->stream));
  const double eps = 2.220446049250313e-16;
  for (int q = 0; q < nsys; ++q) {
    failed[q] = ctx->h_info[ib + q];
    if (piv_ratio) piv_ratio[q] = 0.0;
    if (failed[q] == CHOL_FLOW_GIVEUP) {  // the dataflow factorisation stopped waiting: the caller re-runs the chain
      if (q == 0) count_event(CNT_CHOL_FLOW_GIVEUP);
      continue;
    }
    if (failed[q] != 0) continue;
    double dmin, dmax;
    memcpy(&dmin, &ctx->h_piv[2 * (ib + q)], 8);
    memcpy(&dmax, &ctx->h_piv[2 * (ib + q) + 1], 8);
    if (!(dmax > 0.0)) continue;
    if (piv_ratio) piv_ratio[q] = dmin / dmax;
    if (dmin <= eps * dmax) { failed[q] = -1; continue; }
    if (plog[q].empty()) continue;
    std::sort(plog[q].begin(), plog[q].end());
    const double window = 8.0 * (double)sys[q].m * eps * dmax;
    size_t k = 0;
    while (k < plog[q].size() && plog[q][k] <= window) ++k;
    if (k > 0 && k < plog[q].size() && plog[q][k] >= 1000.0 * plog[q][k - 1]) failed[q] = -1;
  }
  return NK_OK;
}

int cholesky_lower_pair(nk_ctx* ctx, const CholSys* sys, int nsys) {
  NK_TRY(cholesky_lower_pair_async(ctx, sys, nsys));
  return cholesky_check_pair(ctx, sys, nsys);
}

// Factorisation of [P; R^T] with the right-hand sides riding along as extra rows, then the backward substitution on
// those rows.  Per block step: potrf (both systems), panel, trailing; the backward pass is a single launch in which
// every workgroup carries a band of rows through the whole substitution.  The separate forward substitution
// (2 launches per block) disappears.
//
// LOOK-AHEAD.  The chain is latency bound: per block step a one-wave diagonal factorisation (~42 us), the panel product
// (~12 us) and the rank-64 trailing update (~33 us), each waiting for the one before.  Only the NEXT block column of the
// trailing matrix is needed to go on, so the update is split: the next 64 columns are updated on the chain's own stream
// (one tile column), the rest of the trailing matrix on a second stream of the same priority, beside the next step's
// diagonal block and panel.  Dependencies: rest(j) needs panel(j) [event P] and rest(j-1) [stream order]; the narrow update
// of step j needs rest(j-1) [event R] -- the column it touches received its older updates there.  Members of a lock-step
// group record everything into one sequence (events are no-ops there), which is a valid order of the same graph.
int cholesky_aug_pair_async(nk_ctx* ctx, const CholSys* sys, int nsys, hipEvent_t pause, int pause_step) {
  constexpr int NB = CHOL_NB;
  NK_REQUIRE(nsys >= 1 && nsys <= 2, "cholesky_aug_pair: 1..2 systems");
  NK_TRY(reset_pivots(ctx));
  int nblk = 0, mmin = sys[0].m;
  for (int q = 0; q < nsys; ++q) {
    nblk = std::max(nblk, (sys[q].m + NB - 1) / NB);
    mmin = std::min(mmin, sys[q].m);
  }
  // the whole factorisation as one tile-dataflow launch (nk_chol_flow.hip, same bits); lock-step groups record the chain below
  if (!ctx->chol_flow_off && mmin >= 256 && !ctx_recording(ctx) && chol_flow_enabled()) {
    if (pause != nullptr && pause_step >= 0 && pause_step < nblk) NK_HIP(hipStreamWaitEvent(ctx->stream, pause, 0));
    NK_TRY(cholesky_flow_pair(ctx, sys, nsys));
    NK_TRY(launch_trsm_right_lower_pair(ctx, sys, nsys));
    return NK_OK;
  }
  // Measured inside the headline fit (bench.py, same box): with the look-ahead the fit is 1.4 ms SLOWER -- the chain shares
  // the chip with the square-root iteration's GEMMs, its kernels crawl for lack of issue slots rather than for lack of
  // parallelism, and a second stream of them takes more from the GEMMs than the shorter dependency chain gives back.
  // Off by default; NYSKOOP_CHOL_LOOKAHEAD=1 turns it on for chains on the main stream (a stand-alone nk_solve_spd on an
  // idle chip gains from it).
  static const bool la_env = getenv("NYSKOOP_CHOL_LOOKAHEAD") && getenv("NYSKOOP_CHOL_LOOKAHEAD")[0] == '1';
  // which look-ahead stream pairs with the current one (none for callers on other streams)
  const int la = ctx->stream == ctx->stream_main ? 1 : -1;
  const bool lookahead = la_env && la >= 0 && nblk >= 4 && !ctx_recording(ctx);
  hipStream_t s_chain = ctx->stream;
  hipStream_t s_rest = lookahead ? ctx->stream_la[la] : ctx->stream;
  hipEvent_t* la_evt = lookahead ? ctx->ev_la[la] : nullptr;  // [0..1] panel done (parity of the step), [2..3] rest done
  bool rest_pending = false;
  hipEvent_t last_rest = nullptr;
  if (lookahead) {  // the look-ahead stream starts behind whatever the chain's stream has queued so far
    count_event(CNT_CHOL_LOOKAHEAD);
    NK_HIP(hipEventRecord(la_evt[1], s_chain));
    NK_HIP(hipStreamWaitEvent(s_rest, la_evt[1], 0));
  }
  const bool fuse = chol_fuse_enabled();
  int extra[2] = {0, 0};
  for (int q = 0; q < nsys; ++q) extra[q] = sys[q].extra;
  bool diag_done = false;
  for (int jb = 0; jb < nblk; ++jb) {
    if (pause != nullptr && jb == pause_step) NK_HIP(hipStreamWaitEvent(ctx->stream, pause, 0));
    CholStep st;
    chol_step_operands(sys, nsys, jb, extra, &st);
    NK_TRY(chol_step_launches(ctx, sys, nsys, jb, st, !lookahead, fuse && jb + 1 < nblk, &diag_done));
    if (lookahead) {
      // the trailing update split: the next block column (all rows) | everything to the right of it
      GemmCall next[2], rest[2];
      bool any_rest = false;
      for (int q = 0; q < nsys; ++q) {
        const GemmCall& trail = st.trail[q];
        const int rem = (int)trail.N, rows = (int)trail.M;
        if (rem <= 0) continue;
        const int nbn = rem < NB ? rem : NB;
        next[q] = trail;
        next[q].N = nbn;
        if (rem > nbn) {
          rest[q] = trail;
          rest[q].M = rows - nbn; rest[q].N = rem - nbn;
          rest[q].A = rest[q].B = trail.A + (int64_t)nbn * trail.lda;
          rest[q].C = trail.C + (int64_t)nbn * trail.ldc + nbn;
          any_rest = true;
        }
      }
      hipEvent_t evP = la_evt[jb & 1], evR = la_evt[2 + (jb & 1)], evR_prev = la_evt[2 + ((jb + 1) & 1)];
      NK_HIP(hipEventRecord(evP, s_chain));                               // panel(jb) is complete
      if (rest_pending) NK_HIP(hipStreamWaitEvent(s_chain, evR_prev, 0));  // the next column has its older updates
      NK_TRY(chol_trail_update(ctx, next, nsys));
      rest_pending = false;
      if (any_rest) {
        ctx->stream = s_rest;
        NK_HIP(hipStreamWaitEvent(s_rest, evP, 0));
        const int rc = chol_trail_update(ctx, rest, nsys);
        if (rc == NK_OK) NK_HIP(hipEventRecord(evR, s_rest));
        last_rest = evR;
        ctx->stream = s_chain;
        NK_TRY(rc);
        rest_pending = true;
      }
    }
  }
  if (lookahead && last_rest) NK_HIP(hipStreamWaitEvent(s_chain, last_rest, 0));  // (the chain also ends behind the last rest)
  // backward on the extra rows E (extra x m, now holding (L^-1 R)^T):  E <- E L^-1, one launch (nk_trsm.hip)
  NK_TRY(launch_trsm_right_lower_pair(ctx, sys, nsys));
  return NK_OK;
}

int cholesky_solve_pair(nk_ctx* ctx, const CholSys* sys, int nsys) {
  constexpr int NB = CHOL_NB;
  NK_REQUIRE(nsys >= 1 && nsys <= 2, "cholesky_solve_pair: 1..2 systems");
  int nblk = 0;
  for (int q = 0; q < nsys; ++q) nblk = std::max(nblk, (sys[q].m + NB - 1) / NB);
  const ArenaMark mk = arena_mark(ctx);
  double* tmp[2] = {nullptr, nullptr};
  for (int q = 0; q < nsys; ++q) NK_TRY(arena_alloc_t(ctx, (size_t)NB * sys[q].ldr, &tmp[q]));
  // One diagonal-block solve  R_j <- op(L_jj)^-1 R_j : the product with the explicitly inverted block, then one correction
  // step from the data (the product alone is not backward stable, see chol_panel_kernel):
  //   X = Linv R_j ;  X += Linv (R_j - L_jj X)
  auto diag_solve = [&](int jb, bool trans) -> int {
    const int j0 = jb * NB;
    GemmCall g1[2], g2[2], g3[2];
    for (int q = 0; q < nsys; ++q) {
      const CholSys& y = sys[q];
      if (j0 >= y.m) continue;
      const int nbj = y.m - j0 < NB ? y.m - j0 : NB;
      const double* Li = y.Linv + (size_t)jb * CHOL_WS;
      const double* Ld = Li + NB * NB;
      double* Rj = y.R + (int64_t)j0 * y.ldr;
      NK_TRY(launch_copy2d(ctx, Rj, y.ldr, tmp[q], y.ldr, nbj, y.nrhs));
      g1[q].M = nbj; g1[q].N = y.nrhs; g1[q].K = nbj; g1[q].A = Li; g1[q].lda = NB; g1[q].B = tmp[q]; g1[q].ldb = y.ldr;
      g1[q].C = Rj; g1[q].ldc = y.ldr;
      g2[q] = g1[q]; g2[q].A = Ld; g2[q].B = Rj; g2[q].C = tmp[q]; g2[q].alpha = -1.0; g2[q].beta = 1.0;
      g3[q] = g1[q]; g3[q].beta = 1.0;
    }
    NK_TRY(launch_gemm_pair(ctx, trans, false, g1, nsys));
    NK_TRY(launch_gemm_pair(ctx, trans, false, g2, nsys));
    NK_TRY(launch_gemm_pair(ctx, trans, false, g3, nsys));
    return NK_OK;
  };
  // forward: L T = R
  for (int jb = 0; jb < nblk; ++jb) {
    const int j0 = jb * NB;
    GemmCall upd[2];
    for (int q = 0; q < nsys; ++q) {
      const CholSys& y = sys[q];
      if (j0 >= y.m) continue;
      const int nbj = y.m - j0 < NB ? y.m - j0 : NB;
      double* Rj = y.R + (int64_t)j0 * y.ldr;
      const int rem = y.m - j0 - nbj;
      if (rem > 0) {
        upd[q].M = rem; upd[q].N = y.nrhs; upd[q].K = nbj; upd[q].alpha = -1.0; upd[q].beta = 1.0;
        upd[q].A = y.P + (int64_t)(j0 + nbj) * y.ldp + j0; upd[q].lda = y.ldp; upd[q].B = Rj; upd[q].ldb = y.ldr;
        upd[q].C = y.R + (int64_t)(j0 + nbj) * y.ldr; upd[q].ldc = y.ldr;
      }
    }
    NK_TRY(diag_solve(jb, false));
    NK_TRY(launch_gemm_pair(ctx, false, false, upd, nsys));
  }
  // backward: L^T X = T
  for (int jb = nblk - 1; jb >= 0; --jb) {
    const int j0 = jb * NB;
    GemmCall upd[2];
    for (int q = 0; q < nsys; ++q) {
      const CholSys& y = sys[q];
      if (j0 >= y.m) continue;
      const int nbj = y.m - j0 < NB ? y.m - j0 : NB;
      double* Rj = y.R + (int64_t)j0 * y.ldr;
      if (j0 > 0) {
        upd[q].M = j0; upd[q].N = y.nrhs; upd[q].K = nbj; upd[q].alpha = -1.0; upd[q].beta = 1.0;
        upd[q].A = y.P + (int64_t)j0 * y.ldp; upd[q].lda = y.ldp; upd[q].B = Rj; upd[q].ldb = y.ldr;
        upd[q].C = y.R; upd[q].ldc = y.ldr;
      }
    }
    NK_TRY(diag_solve(jb, true));
    NK_TRY(launch_gemm_pair(ctx, true, false, upd, nsys));
  }
  arena_release(ctx, mk);
  return NK_OK;
}

int cholesky_lower(nk_ctx* ctx, double* P, int64_t ldp, int m, double* Linv) {
  CholSys y;
  y.P = P; y.ldp = ldp; y.m = m; y.Linv = Linv;
  return cholesky_lower_pair(ctx, &y, 1);
}

int cholesky_solve(nk_ctx* ctx, const double* L, int64_t ldl, int m, const double* Linv, double* R, int64_t ldr,
                   int nrhs) {
  CholSys y;
  y.P = const_cast<double*>(L); y.ldp = ldl; y.m = m; y.Linv = const_cast<double*>(Linv); y.R = R; y.ldr = ldr;
  y.nrhs = nrhs;
  return cholesky_solve_pair(ctx, &y, 1);
}

}  // namespace nk
