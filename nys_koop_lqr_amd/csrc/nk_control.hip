// Rollouts and the lifted closed loop behind the C ABI, assembled from the device launchers.
#include "nk_common.h"
#include "nk_api_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <mutex>

using namespace nk;

// z_{t+1} = G [z_t; u_t] (+ bias) for t < T-1 on Zall ([b][t][m], row 0 of every trajectory already holds z_0 unless
// `chain.lift`), then x = C z for every (b, t).  One launch for the recursion when G fits in LDS, a matrix-vector /
// GEMM launch per step otherwise.
static bool chain_mw_enabled() {
  static const bool on = [] { const char* e = getenv("NYSKOOP_CHAIN_MW"); return !(e && e[0] == '0'); }();
  return on;
}
// One multi-workgroup recursion on the device at a time (two side by side can starve each other of workgroup slots,
// nk_rollout.hip): held from the launch to the synchronisation that ends the call.
static std::mutex g_chain_mw_mutex;

// Is the single-launch multi-workgroup recursion the path for this chain?  Not inside a lock-step group (its launches
// are deferred to the group's flush, the mutex could not cover them), not for more trajectories than fit beside each
// other unless they are few (<= 16: chunks of launches still beat a launch per step; beyond that the per-step GEMM
// amortises its launches over the batch).
static bool chain_mw_wanted(nk_ctx* ctx, const ChainArgs& chain) {
  const bool allowed = chain_mw_enabled() && !ctx_recording(ctx);
  return chain_mw_wanted_plan(chain.m, chain.pu, chain.U ? chain.pu : 0, chain.lift ? chain.d : 0, chain.T, chain.batch,
                              ctx->num_cu, allowed);
}

static bool chain_mw_gave_up(nk_ctx* ctx) {
  int row = 0, step = 0, traj = 0;
  if (!lifted_chain_mw_timed_out(ctx, &row, &step, &traj)) {
    const char* hook = getenv("NYSKOOP_CHAIN_MW_TEST_GIVEUP");  // test hook: pretend the wait gave up (tests/)
    const bool forced = hook != nullptr && hook[0] == '1';
    if (forced) count_event(CNT_CHAIN_GIVEUP);
    return forced;
  }
  count_event(CNT_CHAIN_GIVEUP);
  if (getenv("NYSKOOP_TRACE"))
    fprintf(stderr, "[nyskoop] single-launch recursion timed out (row %d, step %d, trajectory %d): repeating stepwise\n", row,
            step, traj);
  return true;
}

static int rollout_steps(nk_ctx* ctx, ChainArgs chain, bool z0_in_place, bool use_mw) {
  const int m = chain.m, p = chain.pu, T = chain.T, batch = chain.batch;
  // the branch is the plan's (nk_chain_plan.h: what the tests mirror and assert); use_mw carries the conditions that are
  // no arithmetic (the switch, a recording context, the repeat after a give-up) and chain_mw_wanted's verdict
  const ChainPlan plan = chain_plan(m, p, chain.lift ? chain.d : 0, T, batch, ctx->num_cu, /*batch_invariant=*/false,
                                    chain.bias != nullptr && chain.bias_stride != 0, use_mw);
  if (plan.route == ROUTE_CHAIN) return launch_lifted_chain(ctx, chain);
  NK_REQUIRE(!chain.lift && z0_in_place, "rollout_steps: internal: the stepwise path needs z_0 in place");
  NK_REQUIRE((plan.route == ROUTE_MW) == use_mw, "rollout_steps: internal: the plan and the caller disagree on the route");
  if (plan.route == ROUTE_MW) {
    // trajectories that are resident side by side: (CUs / workgroups per trajectory group) groups of `nt`
    const int nb = chain_mw_chunk(m, batch, ctx->num_cu);
    NK_TRY(lifted_chain_mw_reset(ctx));
    for (int b0 = 0; b0 < batch; b0 += nb) {
      ChainArgs sub = chain;
      sub.batch = batch - b0 < nb ? batch - b0 : nb;
      sub.Zall = chain.Zall + (int64_t)b0 * chain.z_stride;
      if (chain.U) sub.U = chain.U + (int64_t)b0 * chain.u_stride;
      if (chain.bias) sub.bias = chain.bias + (int64_t)b0 * chain.bias_stride;
      NK_TRY(launch_lifted_chain_mw(ctx, sub));
    }
    return lifted_chain_mw_fetch_status(ctx);
  }
  double* Zall = chain.Zall;
  const int64_t ldz = chain.z_stride;
  for (int t = 0; t + 1 < T; ++t) {
    if (plan.route == ROUTE_STEP) {  // matrix-vector chain: one wave per row of G, trajectories in groups of 8
      for (int b0 = 0; b0 < batch; b0 += STEP_MAX_BATCH) {
        const int nb = batch - b0 < STEP_MAX_BATCH ? batch - b0 : STEP_MAX_BATCH;
        // the kernel takes one bias vector: trajectories with their own bias go one by one
        if (chain.bias && chain.bias_stride != 0) {
          for (int b = b0; b < b0 + nb; ++b)
            NK_TRY(launch_lifted_step(ctx, chain.G, chain.ldg, m, m, p, Zall + (int64_t)b * ldz + (int64_t)t * m, ldz,
                                      p > 0 ? chain.U + (int64_t)b * chain.u_stride + (int64_t)t * p : nullptr,
                                      chain.u_stride, chain.bias + (int64_t)b * chain.bias_stride,
                                      Zall + (int64_t)b * ldz + (int64_t)(t + 1) * m, ldz, 1));
        } else {
          NK_TRY(launch_lifted_step(ctx, chain.G, chain.ldg, m, m, p, Zall + (int64_t)b0 * ldz + (int64_t)t * m, ldz,
                                    p > 0 ? chain.U + (int64_t)b0 * chain.u_stride + (int64_t)t * p : nullptr,
                                    chain.u_stride, chain.bias, Zall + (int64_t)b0 * ldz + (int64_t)(t + 1) * m, ldz, nb));
        }
      }
    } else {
      double* zn = Zall + (int64_t)(t + 1) * m;
      double beta = 0.0;
      if (chain.bias) {  // z' = bias + ...
        NK_TRY(launch_copy2d(ctx, chain.bias, chain.bias_stride, zn, ldz, batch, m));
        beta = 1.0;
      }
      NK_TRY(launch_gemm(ctx, false, true, batch, m, m, 1.0, Zall + (int64_t)t * m, ldz, chain.G, chain.ldg, beta, zn, ldz));
      if (p > 0)
        NK_TRY(launch_gemm(ctx, false, true, batch, m, p, 1.0, chain.U + (int64_t)t * p, chain.u_stride, chain.G + m,
                           chain.ldg, 1.0, zn, ldz));
    }
  }
  return NK_OK;
}

// The recursion of `ch`, then what `after` queues behind it, then the one synchronisation of the attempt.  When the
// single-launch multi-workgroup recursion is the path (chain_mw_wanted) the mutex is held for the whole call, and when
// a wave of it gave up waiting for its neighbours (the device was oversubscribed) the trajectories are not valid: z_0 is
// untouched, so everything is repeated once with one launch per step.
// batch_invariant (the error mode): the bits must not depend on the batch or on the schedule -- an ordinary context and a
// lock-step member must agree, the sweep is checked bit for bit against the plain loop.  Beyond the single-launch chain
// that rules out the multi-workgroup recursion and the per-step GEMM of batches above 16 (another summation order): the
// matrix-vector steps are walked 16 trajectories at a time, the path a member takes for a small batch.
template <class After>
static int run_chain(nk_ctx* ctx, const ChainArgs& ch, bool z0_in_place, bool batch_invariant, After after) {
  const bool try_mw = !batch_invariant && chain_mw_wanted(ctx, ch);
  std::unique_lock<std::mutex> mw_lock(g_chain_mw_mutex, std::defer_lock);
  if (try_mw) mw_lock.lock();
  for (int attempt = 0; attempt < 2; ++attempt) {
    const bool mw = try_mw && attempt == 0;
    if (batch_invariant && !lifted_chain_ok(ch.m, ch.pu, ch.lift ? ch.d : 0)) {
      for (int b0 = 0; b0 < ch.batch; b0 += STEP_INVARIANT_CHUNK) {
        ChainArgs sub = ch;
        sub.batch = ch.batch - b0 < STEP_INVARIANT_CHUNK ? ch.batch - b0 : STEP_INVARIANT_CHUNK;
        sub.Zall = ch.Zall + (int64_t)b0 * ch.z_stride;
        if (ch.U) sub.U = ch.U + (int64_t)b0 * ch.u_stride;
        NK_TRY(rollout_steps(ctx, sub, z0_in_place, false));
      }
    } else {
      NK_TRY(rollout_steps(ctx, ch, z0_in_place, mw));
    }
    NK_TRY(after());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    if (!(mw && chain_mw_gave_up(ctx))) break;
  }
  return NK_OK;
}

static int rollout_impl(nk_ctx* ctx, const nk_model* mdl, const double* G, int64_t ldg, const double* Cop, int64_t ldc,
                        int m, int d, int p, const double* x0, int64_t ldx0, const double* z0, const double* U, int32_t T,
                        int32_t batch, double* out_x, double* out_z, const double* traj_true = nullptr,
                        double* err_out = nullptr) {
  // x0 != nullptr: lift through the model; otherwise z0 (batch x m) holds the lifted initial states.
  // traj_true != nullptr (nk_rollout_err): the true trajectories (batch x T x d) are staged whole, x0 = their rows 0, and
  // instead of the trajectory the call returns err_out[b] = (sse, ssim) (HOST, batch x 2) reduced on the device; out_x and
  // out_z are absent.  Staging and recursion are the same in both modes.
  const bool err_mode = traj_true != nullptr;
  const bool from_state = err_mode || x0 != nullptr;
  const int64_t nin = err_mode ? (int64_t)T * d : (x0 ? d : m);
  const int64_t ldin = err_mode ? (int64_t)T * d : (x0 ? ldx0 : m);
  const double* first = err_mode ? traj_true : (x0 ? x0 : z0);
  const bool have_u = p > 0 && T > 1;
  double* Zall = nullptr;  // [batch][T][m]
  NK_TRY(arena_alloc_t(ctx, (size_t)batch * T * m, &Zall));
  const int64_t ldz = (int64_t)T * m;
  ChainArgs ch;
  ch.G = G; ch.ldg = ldg; ch.m = m; ch.pu = p; ch.T = T; ch.batch = batch; ch.Zall = Zall; ch.z_stride = ldz;
  ch.u_stride = (int64_t)T * p;
  CallStage st(ctx);
  MatIn xin, uin;
  MatOut ox, oz, oe;
  st.in(&xin, first, ldin, batch, nin);
  if (have_u) st.in(&uin, U, (int64_t)T * p, batch, (int64_t)T * p);
  if (err_mode) {
    st.out(&oe, err_out, 2, batch, 2);
  } else {
    st.out(&ox, out_x, d, (int64_t)batch * T, d);
    st.out(&oz, out_z, m, (int64_t)batch * T, m);
  }
  NK_TRY(st.commit());
  if (err_mode) NK_TRY(st.resident(&xin, nin));  // every row of the true trajectories is read by the error kernel
  if (!have_u) ch.pu = (T > 1) ? p : 0;
  bool z0_in_place = false;
  if (from_state && mdl->kind != NK_MODEL_SPLINE && lifted_chain_ok(m, ch.pu, d)) {  // the lift is done by the chain kernel itself
    ch.lift = true; ch.x0 = xin.ptr; ch.x0_stride = xin.ld; ch.Zl = mdl->Z; ch.d = d; ch.winv = mdl->winv;
    ch.Sinv = mdl->Sinv; ch.ktype = mdl->ktype; ch.sigma0 = mdl->sigma0;
  } else if (from_state) {
    NK_TRY(lift_device(ctx, mdl, xin.ptr, xin.ld, batch, Zall, ldz));  // z_0 = phi(x_0) for every trajectory
    z0_in_place = true;
    // the single-launch chain (no lift of its own: a spline model, or d too large for its LDS) reads z_0 from there
    if (lifted_chain_ok(m, ch.pu, 0)) { ch.z0 = Zall; ch.z0_stride = ldz; }
  } else if (lifted_chain_ok(m, ch.pu, 0)) {
    ch.z0 = xin.ptr; ch.z0_stride = xin.ld;
  } else {
    NK_TRY(launch_copy2d(ctx, xin.ptr, xin.ld, Zall, ldz, batch, m));
    z0_in_place = true;
  }
  // the stepwise / multi-workgroup paths read the controls from every wave of every step: not from page-locked host
  // memory (an uncached PCIe read per wave, ~30 us per step at m = 500) but from a device copy
  if (z0_in_place && have_u) NK_TRY(st.resident(&uin, (int64_t)T * p));
  ch.U = have_u ? uin.ptr : nullptr;
  NK_TRY(run_chain(ctx, ch, z0_in_place, /*batch_invariant=*/err_mode, [&]() -> int {
    if (err_mode) {  // x_true - C z and C z squared and summed per trajectory where z lies: no product, no trajectory copy
      NK_TRY(launch_traj_err(ctx, Zall, ldz, Cop, ldc, xin.ptr, xin.ld, m, d, T, batch, oe.dev));
    } else {
      NK_TRY(launch_gemm(ctx, false, true, (int64_t)batch * T, d, m, 1.0, Zall, m, Cop, ldc, 0.0, ox.dev, ox.ld));
      if (out_z) NK_TRY(launch_copy2d(ctx, Zall, m, oz.dev, oz.ld, (int64_t)batch * T, m));
    }
    return st.queue_outputs();
  }));
  st.deliver();
  return NK_OK;
}

namespace nk {

int rollout_err_run(nk_ctx* ctx, const nk_model* mdl, const double* traj, const double* U, int32_t T, int32_t batch,
                           double* err_abs, double* err_rel) {
  const int m = mdl->m, d = mdl->d, p = mdl->p, mp = m + p;
  std::vector<double> e((size_t)batch * 2);
  NK_TRY(rollout_impl(ctx, mdl, mdl->A, mp, mdl->C, m, m, d, p, nullptr, 0, nullptr, U, T, batch, nullptr, nullptr, traj,
                      e.data()));
  for (int b = 0; b < batch; ++b) {
    const double sse = e[(size_t)2 * b], ssim = e[(size_t)2 * b + 1];
    if (err_abs) err_abs[b] = std::sqrt(sse / ((double)d * (double)T));
    if (err_rel) err_rel[b] = std::sqrt(sse) / std::sqrt(ssim) * 100.0;
  }
  return NK_OK;
}

}  // namespace nk

extern "C" {

int nk_rollout(nk_ctx* ctx, const nk_model* mdl, const double* x0, int64_t ldx0, const double* U, int32_t T,
               int32_t batch, double* out_x, double* out_z) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && x0 && out_x, "nk_rollout: null argument");
  NK_REQUIRE(mdl->has_ops, "nk_rollout: model holds no fitted operators");
  NK_REQUIRE(T >= 1 && batch >= 1 && ldx0 >= mdl->d, "nk_rollout: bad sizes");
  const int m = mdl->m, d = mdl->d, p = mdl->p, mp = m + p;
  NK_REQUIRE(p == 0 || T == 1 || U != nullptr, "nk_rollout: controls missing");
  return rollout_impl(ctx, mdl, mdl->A, mp, mdl->C, m, m, d, p, x0, ldx0, nullptr, U, T, batch, out_x, out_z);
}

int nk_rollout_err(nk_ctx* ctx, const nk_model* mdl, const double* traj, const double* U, int32_t T, int32_t batch,
                   double* err_abs, double* err_rel) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && traj, "nk_rollout_err: null argument");
  NK_REQUIRE(mdl->has_ops, "nk_rollout_err: model holds no fitted operators");
  NK_REQUIRE(T >= 1 && batch >= 1 && batch <= 65535, "nk_rollout_err: bad sizes");
  NK_REQUIRE(traj_err_tile(mdl->m) >= 1, "nk_rollout_err: m = %d is beyond the error kernel's range (4096)", mdl->m);
  NK_REQUIRE(mdl->p == 0 || T == 1 || U != nullptr, "nk_rollout_err: controls missing");
  return rollout_err_run(ctx, mdl, traj, U, T, batch, err_abs, err_rel);
}

int nk_linear_rollout(nk_ctx* ctx, const double* A, const double* B, const double* Cop, int32_t m, int32_t d, int32_t p,
                      const double* z0, const double* U, int32_t T, int32_t batch, double* out_x, double* out_z) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(A && Cop && z0 && out_x, "nk_linear_rollout: null argument");
  NK_REQUIRE(m >= 1 && d >= 1 && p >= 0 && T >= 1 && batch >= 1, "nk_linear_rollout: bad sizes");
  NK_REQUIRE(p == 0 || (B != nullptr && (T == 1 || U != nullptr)), "nk_linear_rollout: B or controls missing");
  const int mp = m + p;
  const int64_t ldg = mp + (mp & 1);
  double* G = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)m * ldg, &G));
  MatIn a, b, c;
  NK_TRY(stage_in(ctx, A, m, m, m, &a));
  NK_TRY(launch_copy2d(ctx, a.ptr, a.ld, G, ldg, m, m));
  if (p > 0) {
    NK_TRY(stage_in(ctx, B, p, m, p, &b));
    NK_TRY(launch_copy2d(ctx, b.ptr, b.ld, G + m, ldg, m, p));
  }
  NK_TRY(stage_in(ctx, Cop, m, d, m, &c));
  return rollout_impl(ctx, nullptr, G, ldg, c.ptr, c.ld, m, d, p, nullptr, 0, z0, U, T, batch, out_x, out_z);
}

int nk_closed_loop_batch(nk_ctx* ctx, const nk_model* mdl, const double* K, const double* phi0, const double* phi_ref,
                         int32_t steps, int32_t batch, double* out_x, double* out_u) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && K && phi0 && phi_ref && out_x && out_u, "nk_closed_loop: null argument");
  NK_REQUIRE(mdl->has_ops && steps >= 1 && batch >= 1 && mdl->p > 0, "nk_closed_loop: bad model or sizes");
  const int m = mdl->m, d = mdl->d, p = mdl->p, mp = m + p;
  CallStage st(ctx);
  MatIn k, f0, fr;
  MatOut ox, ou;
  st.in(&k, K, m, p, m);
  st.in(&f0, phi0, m, batch, m);
  st.in(&fr, phi_ref, m, batch, m);
  st.out(&ox, out_x, d, (int64_t)batch * steps, d);
  st.out(&ou, out_u, p, (int64_t)batch * steps, p);
  NK_TRY(st.commit());
  // phi_{t+1} = A phi_t + B K (phi_ref - phi_t) = (A - B K) phi_t + B K phi_ref: one matrix-vector step per time step
  // (algebraically the loop of benchmark_lqr_cloth.py:79-84; the controls u_t = K (phi_ref - phi_t) are recovered for all
  // steps at once afterwards)
  double *Phi = nullptr, *Acl = nullptr, *kref = nullptr, *cvec = nullptr, *Dm = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)batch * steps * m, &Phi));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Acl));
  NK_TRY(arena_alloc_t(ctx, (size_t)batch * p + 8, &kref));
  NK_TRY(arena_alloc_t(ctx, (size_t)batch * m, &cvec));
  NK_TRY(arena_alloc_t(ctx, (size_t)batch * steps * m, &Dm));
  NK_TRY(launch_copy2d(ctx, mdl->A, mp, Acl, m, m, m));
  NK_TRY(launch_gemm(ctx, false, false, m, m, p, -1.0, mdl->B, mp, k.ptr, k.ld, 1.0, Acl, m));     // A - B K
  NK_TRY(launch_gemm(ctx, false, true, batch, p, m, 1.0, fr.ptr, fr.ld, k.ptr, k.ld, 0.0, kref, p));  // K phi_ref
  NK_TRY(launch_gemm(ctx, false, true, batch, m, p, 1.0, kref, p, mdl->B, mp, 0.0, cvec, m));         // B K phi_ref
  ChainArgs ch;
  ch.G = Acl; ch.ldg = m; ch.m = m; ch.pu = 0; ch.T = steps; ch.batch = batch; ch.Zall = Phi;
  ch.z_stride = (int64_t)steps * m; ch.bias = cvec; ch.bias_stride = m;
  bool z0_in_place = false;
  if (lifted_chain_ok(m, 0, 0)) {
    ch.z0 = f0.ptr; ch.z0_stride = f0.ld;
  } else {
    NK_TRY(launch_copy2d(ctx, f0.ptr, f0.ld, Phi, ch.z_stride, batch, m));
    z0_in_place = true;
  }
  NK_TRY(run_chain(ctx, ch, z0_in_place, /*batch_invariant=*/false, [&]() -> int {
    // u_t = K (phi_ref - phi_t) for all t: D = 1 phi_ref^T - Phi, U = D K^T
    NK_TRY(launch_ref_minus_traj(ctx, fr.ptr, fr.ld, Phi, ch.z_stride, Dm, ch.z_stride, steps, m, batch));
    NK_TRY(launch_gemm(ctx, false, true, (int64_t)batch * steps, p, m, 1.0, Dm, m, k.ptr, k.ld, 0.0, ou.dev, ou.ld));
    NK_TRY(launch_gemm(ctx, false, true, (int64_t)batch * steps, d, m, 1.0, Phi, m, mdl->C, m, 0.0, ox.dev, ox.ld));  // x_t = C phi_t
    return st.queue_outputs();
  }));
  st.deliver();
  return NK_OK;
}

int nk_closed_loop(nk_ctx* ctx, const nk_model* mdl, const double* K, const double* phi0, const double* phi_ref,
                   int32_t steps, double* out_x, double* out_u) {
  return nk_closed_loop_batch(ctx, mdl, K, phi0, phi_ref, steps, 1, out_x, out_u);
}

}  // extern "C"
