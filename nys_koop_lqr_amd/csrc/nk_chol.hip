// Blocked Cholesky (lower) of up to two symmetric positive definite systems advanced in lock step, built on the fp64 MFMA
// GEMM engine, with inverted diagonal blocks: the plain factorisation with its block substitutions, and the augmented form
// with the right-hand sides riding along as extra rows + a single-launch backward substitution (nk_trsm.hip), replacing
// scipy.linalg.lstsq on the (numerically full-rank) regularised normal matrices (regressors.py:155,165).  A non-positive
// pivot is reported as NK_ERR_NOT_SPD; there is no silent rank truncation.
#include "nk_common.h"
#include "nk_chol.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace nk {

// ---------------------------------------------------------------------------------------------------------------
// blocked Cholesky (lower) with inverted diagonal blocks
// ---------------------------------------------------------------------------------------------------------------
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

// the most block steps of any system of a pair
static int pair_blocks(const CholSys* sys, int nsys) {
  int nblk = 0;
  for (int q = 0; q < nsys; ++q) nblk = std::max(nblk, chol_blocks(sys[q].m));
  return nblk;
}

// diagonal-block record of the current stream with both slots empty (the failure flag and pivot slots are set for both)
static PotrfBatch potrf_batch(nk_ctx* ctx) {
  PotrfBatch pb = {};
  for (int q = 0; q < 2; ++q) {
    pb.info[q] = ctx->d_info + info_base(ctx) + q;
    pb.piv[q] = ctx->d_piv + 2 * (info_base(ctx) + q);
  }
  return pb;
}
// slot q <- diagonal block jb (order nb, top left corner A) of system y
static void potrf_slot(PotrfBatch& pb, int q, const CholSys& y, int jb, double* A, int nb) {
  pb.A[q] = A; pb.lda[q] = y.ldp; pb.nb[q] = nb;
  pb.Linv[q] = y.Linv + (size_t)jb * CHOL_WS;
  pb.plog[q] = y.pivlog ? y.pivlog + jb * CHOL_NB : nullptr;
}
// trailing update of the rows x rem matrix C by the panel P (rows x CHOL_NB)
static TrailSys trail_sys(const double* P, int64_t ldp, double* C, int64_t ldc, int rows, int rem) {
  const CholTrailTiles t = chol_trail_tiles(rows, rem);
  TrailSys s = {};
  s.P = P; s.ldp = ldp; s.C = C; s.ldc = ldc; s.rows = rows; s.rem = rem;
  s.tiles_n = t.tiles_n; s.nblocks = t.workgroups;
  return s;
}
// one part of a split trailing update t (look-ahead)
static TrailSys trail_part(const TrailSys& t, const CholTrailPart& p) {
  return trail_sys(t.P + (int64_t)p.row0 * t.ldp, t.ldp, t.C + (int64_t)p.row0 * t.ldc + p.col0, t.ldc, p.rows, p.cols);
}

// Records of block step jb of up to two systems (a system that has no such block, or no such launch, keeps an empty slot)
struct CholStep {
  PotrfBatch diag;   // the diagonal blocks
  PanelBatch panel;  // panel <- panel * Linv_jj^T   (in place: every workgroup reads exactly the rows it writes)
  TrailBatch trail;  // trailing <- trailing - panel * panel^T  (lower tiles of the square part, full tiles for the extra rows)
  PotrfBatch next;   // the diagonal blocks of step jb + 1: the top left corners of the trailing matrices
  bool has_next;     // ... of which there is at least one
};
// extra[q]: rows below the m x m matrix of system q that ride along (the right-hand sides of the augmented form); zeros for
// the plain factorisation.  The shapes are the plan's (nk_chol_plan.h); what the kernels take for granted of them is checked
// here, where the records are filled.
static int chol_step_operands(nk_ctx* ctx, const CholSys* sys, int nsys, int jb, const int* extra, CholStep* st) {
  *st = CholStep{};
  st->diag = potrf_batch(ctx);
  st->next = potrf_batch(ctx);
  const int fix = chol_fix_enabled();
  for (int q = 0; q < nsys; ++q) {
    const CholSys& y = sys[q];
    const CholStepShape sh = chol_step_shape(y.m, extra[q], jb);
    if (sh.nbj == 0) continue;
    NK_REQUIRE(sh.nbj <= CHOL_NB && (!sh.trail || (sh.panel && sh.nbj == CHOL_NB && sh.rows >= sh.rem)) &&
                   (sh.nb_next == 0 || sh.trail),
               "blocked Cholesky: block step %d of a system of order %d (+%d rows) has no shape the kernels take", jb, y.m,
               extra[q]);
    potrf_slot(st->diag, q, y, jb, y.P + (int64_t)sh.j0 * y.ldp + sh.j0, sh.nbj);
    if (!sh.panel) continue;
    double* pnl = y.P + (int64_t)(sh.j0 + sh.nbj) * y.ldp + sh.j0;
    PanelSys& p = st->panel.s[q];  // (the workspace holds the inverse with leading dimension CHOL_NB, as the kernel reads it)
    p.P = pnl; p.ldp = y.ldp; p.Linv = st->diag.Linv[q]; p.rows = sh.rows; p.nb = sh.nbj; p.fix = fix;
    p.nblocks = chol_panel_workgroups(sh.rows);
    if (!sh.trail) continue;
    // (the kernel contracts over a whole panel of CHOL_NB columns and walks the lower tiles of rows >= rem: required above)
    st->trail.s[q] = trail_sys(pnl, y.ldp, pnl + sh.nbj, y.ldp, sh.rows, sh.rem);  // (C starts right of the panel's top)
    if (sh.nb_next == 0) continue;
    potrf_slot(st->next, q, y, jb + 1, st->trail.s[q].C, sh.nb_next);
    st->has_next = true;
  }
  return NK_OK;
}

// Launches of block step jb: the diagonal block unless the previous step's fused launch factored it (*diag_done), the panel,
// and -- with `trailing` -- the trailing update, in one launch with the factorisation of the next diagonal block where `fuse`
// asks for it and there is one (*diag_done is then set for the next step).
static int chol_step_launches(nk_ctx* ctx, int jb, const CholStep& st, bool trailing, bool fuse, bool* diag_done) {
  if (!*diag_done) NK_TRY(launch_potrf_diag_pair(ctx, st.diag, jb));
  *diag_done = false;
  NK_TRY(launch_chol_panel_pair(ctx, st.panel));
  if (!trailing) return NK_OK;
  if (fuse && st.has_next) {
    NK_TRY(launch_chol_trail_potrf_pair(ctx, st.trail, st.next, jb + 1));
    *diag_done = true;
    return NK_OK;
  }
  return launch_chol_trail_pair(ctx, st.trail);
}

int cholesky_lower_pair_async(nk_ctx* ctx, const CholSys* sys, int nsys) {
  NK_REQUIRE(nsys >= 1 && nsys <= 2, "cholesky_lower_pair: 1..2 systems");
  NK_TRY(reset_pivots(ctx));
  const int nblk = pair_blocks(sys, nsys);
  const bool fuse = chol_fuse_enabled();
  const int no_extra[2] = {0, 0};  // (CholSys::extra is not read here)
  bool diag_done = false;
  for (int jb = 0; jb < nblk; ++jb) {
    CholStep st;
    NK_TRY(chol_step_operands(ctx, sys, nsys, jb, no_extra, &st));
    NK_TRY(chol_step_launches(ctx, jb, st, true, fuse, &diag_done));
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
  NK_REQUIRE(nsys >= 1 && nsys <= 2, "cholesky_aug_pair: 1..2 systems");
  NK_TRY(reset_pivots(ctx));
  const int nblk = pair_blocks(sys, nsys);
  int ms[2] = {0, 0}, extra[2] = {0, 0};
  for (int q = 0; q < nsys; ++q) {
    ms[q] = sys[q].m;
    extra[q] = sys[q].extra;
  }
  // the whole factorisation as one tile-dataflow launch (nk_chol_flow.hip, same bits); lock-step groups record the chain below
  if (chol_route_is_flow(ms, nsys, !ctx->chol_flow_off && !ctx_recording(ctx) && chol_flow_enabled())) {
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
  bool diag_done = false;
  for (int jb = 0; jb < nblk; ++jb) {
    if (pause != nullptr && jb == pause_step) NK_HIP(hipStreamWaitEvent(ctx->stream, pause, 0));
    CholStep st;
    NK_TRY(chol_step_operands(ctx, sys, nsys, jb, extra, &st));
    NK_TRY(chol_step_launches(ctx, jb, st, !lookahead, fuse, &diag_done));
    if (lookahead) {
      // the trailing update split (chol_lookahead_split): the next block column (all rows) | everything to the right of it
      TrailBatch next = {}, rest = {};
      bool any_rest = false;
      for (int q = 0; q < nsys; ++q) {
        const TrailSys& trail = st.trail.s[q];
        const CholLookahead split = chol_lookahead_split(trail.rows, trail.rem);
        if (split.next.cols > 0) next.s[q] = trail_part(trail, split.next);
        if (split.rest.cols > 0) {
          rest.s[q] = trail_part(trail, split.rest);
          any_rest = true;
        }
      }
      hipEvent_t evP = la_evt[jb & 1], evR = la_evt[2 + (jb & 1)], evR_prev = la_evt[2 + ((jb + 1) & 1)];
      NK_HIP(hipEventRecord(evP, s_chain));                               // panel(jb) is complete
      if (rest_pending) NK_HIP(hipStreamWaitEvent(s_chain, evR_prev, 0));  // the next column has its older updates
      NK_TRY(launch_chol_trail_pair(ctx, next));
      rest_pending = false;
      if (any_rest) {
        ctx->stream = s_rest;
        NK_HIP(hipStreamWaitEvent(s_rest, evP, 0));
        const int rc = launch_chol_trail_pair(ctx, rest);
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
  const int nblk = pair_blocks(sys, nsys);
  const ArenaMark mk = arena_mark(ctx);
  double* tmp[2] = {nullptr, nullptr};
  for (int q = 0; q < nsys; ++q) NK_TRY(arena_alloc_t(ctx, (size_t)NB * sys[q].ldr, &tmp[q]));
  auto rhs_block = [&](int q, int jb) { return sys[q].R + (int64_t)jb * NB * sys[q].ldr; };
  // One diagonal-block solve  R_j <- op(L_jj)^-1 R_j : the product with the explicitly inverted block, then one correction
  // step from the data (the product alone is not backward stable, see chol_panel_kernel):
  //   X = Linv R_j ;  X += Linv (R_j - L_jj X)
  auto diag_solve = [&](int jb, bool trans) -> int {
    GemmCall g1[2], g2[2], g3[2];
    for (int q = 0; q < nsys; ++q) {
      const CholSys& y = sys[q];
      const int nbj = chol_block_order(y.m, jb);
      if (nbj == 0) continue;
      const double* Li = y.Linv + (size_t)jb * CHOL_WS;
      const double* Ld = Li + NB * NB;
      double* Rj = rhs_block(q, jb);
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
  // R[u.row0 ..] -= op(L[block]) R_jb for the update u of block jb; A: the block of the factor, rows x k (forward) or
  // k x rows read transposed (backward)
  auto update = [&](int q, int jb, const CholSolveUpdate& u, const double* A, GemmCall& g) {
    if (u.rows == 0) return;
    const CholSys& y = sys[q];
    g.M = u.rows; g.N = y.nrhs; g.K = u.k; g.alpha = -1.0; g.beta = 1.0;
    g.A = A; g.lda = y.ldp; g.B = rhs_block(q, jb); g.ldb = y.ldr;
    g.C = y.R + (int64_t)u.row0 * y.ldr; g.ldc = y.ldr;
  };
  // forward: L T = R
  for (int jb = 0; jb < nblk; ++jb) {
    GemmCall upd[2];
    for (int q = 0; q < nsys; ++q) {
      const CholSolveUpdate u = chol_solve_forward(sys[q].m, jb);
      update(q, jb, u, sys[q].P + (int64_t)u.row0 * sys[q].ldp + jb * NB, upd[q]);
    }
    NK_TRY(diag_solve(jb, false));
    NK_TRY(launch_gemm_pair(ctx, false, false, upd, nsys));
  }
  // backward: L^T X = T
  for (int jb = nblk - 1; jb >= 0; --jb) {
    GemmCall upd[2];
    for (int q = 0; q < nsys; ++q)
      update(q, jb, chol_solve_backward(sys[q].m, jb), sys[q].P + (int64_t)jb * NB * sys[q].ldp, upd[q]);
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
