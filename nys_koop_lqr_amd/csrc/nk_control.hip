// Rollouts, closed loops, plant loops and the batched Riccati solver behind the C ABI, assembled from the device launchers.
#include "nk_common.h"
#include "nk_api_internal.h"
#include "nk_plant.h"

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
  if (!chain_mw_enabled() || ctx_recording(ctx) || chain.T < 3) return false;
  if (lifted_chain_ok(chain.m, chain.pu, chain.lift ? chain.d : 0)) return false;
  if (!lifted_chain_mw_ok(ctx, chain.m, chain.U ? chain.pu : 0)) return false;
  const int nt = chain_mw_group(chain.m, chain.batch);
  const int64_t groups = (chain.batch + nt - 1) / nt;
  return groups <= 16 || groups * chain_mw_workgroups(chain.m) <= ctx->num_cu;
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
  if (lifted_chain_ok(m, p, chain.lift ? chain.d : 0)) return launch_lifted_chain(ctx, chain);
  NK_REQUIRE(!chain.lift && z0_in_place, "rollout_steps: internal: the stepwise path needs z_0 in place");
  if (use_mw) {
    // trajectories that are resident side by side: (CUs / workgroups per trajectory group) groups of `nt`
    const int nt = chain_mw_group(m, batch);
    int nb = ctx->num_cu / chain_mw_workgroups(m);
    if (nb < 1) nb = 1;
    nb *= nt;
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
    if (batch <= 16) {  // matrix-vector chain: one wave per row of G, trajectories in groups of 8
      for (int b0 = 0; b0 < batch; b0 += 8) {
        const int nb = batch - b0 < 8 ? batch - b0 : 8;
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
      for (int b0 = 0; b0 < ch.batch; b0 += 16) {
        ChainArgs sub = ch;
        sub.batch = ch.batch - b0 < 16 ? ch.batch - b0 : 16;
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

// One problem of the batched Riccati solver as the two entry points hand it over: operands in host memory (nk_dare_batch;
// dense copies are packed and staged with one copy per array kind) or in a model's device allocation (the model entries).
struct DareItem {
  int m = 0, p = 0, d = 0;
  const double *hA = nullptr, *hB = nullptr, *hQ = nullptr, *hR = nullptr;  // host operands ...
  int64_t lda = 0, ldb = 0, ldq = 0, ldr = 0;
  const double *dA = nullptr, *dB = nullptr, *dC = nullptr;                 // ... or device operands (lda, ldb; ldc = m)
  double c = 0.0;
  double *outK = nullptr, *outP = nullptr, *out_delta = nullptr;            // host results
  int q_only = 0;
};

// Runs the items in launches whose workspace stays under NK_DARE_WS_CAP_BYTES; every argument has been checked.
static int dare_run(nk_ctx* ctx, const std::vector<DareItem>& items, double tol, int max_iter, int32_t* out_status,
                    int32_t* out_iters) {
  const size_t n = items.size();
  size_t b = 0;
  while (b < n) {
    size_t e = b, ws = 0;
    while (e < n) {
      const size_t w = dare_ws_doubles(dare_pad(items[e].m)) * 8;
      if (e > b && ws + w > (size_t)NK_DARE_WS_CAP_BYTES) break;
      ws += w;
      ++e;
    }
    const size_t cnt = e - b;
    const ArenaMark mk = arena_mark(ctx);
    // host staging: one block per array kind, one block for the results
    size_t nA = 0, nB = 0, nR = 0, nK = 0, nP = 0;
    for (size_t u = b; u < e; ++u) {
      const DareItem& it = items[u];
      if (it.hA) { nA += (size_t)it.m * it.m; nB += (size_t)it.m * it.p; }
      if (it.hR) nR += (size_t)it.p * it.p;
      nK += (size_t)it.p * it.m;
      if (it.outP) nP += (size_t)it.m * it.m;
    }
    std::vector<double> hA(nA), hQ(nA), hB(nB), hR(nR);
    double *dA = nullptr, *dQ = nullptr, *dB = nullptr, *dR = nullptr, *dW = nullptr, *dOut = nullptr;
    int* dInt = nullptr;
    DareRec* dTab = nullptr;
    if (nA) { NK_TRY(arena_alloc_t(ctx, nA, &dA)); NK_TRY(arena_alloc_t(ctx, nA, &dQ)); NK_TRY(arena_alloc_t(ctx, nB, &dB)); }
    if (nR) NK_TRY(arena_alloc_t(ctx, nR, &dR));
    NK_TRY(arena_alloc_t(ctx, ws / 8, &dW));
    const size_t nOut = nK + nP + cnt;
    NK_TRY(arena_alloc_t(ctx, nOut, &dOut));
    NK_TRY(arena_alloc_t(ctx, 2 * cnt, &dInt));
    NK_TRY(arena_alloc_t(ctx, cnt, &dTab));
    std::vector<DareRec> recs(cnt);
    size_t oA = 0, oB = 0, oR = 0, oK = 0, oP = nK, oW = 0;
    for (size_t u = b; u < e; ++u) {
      const DareItem& it = items[u];
      DareRec& r = recs[u - b];
      const int m = it.m, p = it.p;
      r = DareRec{};
      r.m = m; r.p = p; r.M = dare_pad(m); r.d = it.d; r.c = it.c; r.q_only = it.q_only;
      if (it.hA) {
        for (int i = 0; i < m; ++i) {
          std::copy(it.hA + (int64_t)i * it.lda, it.hA + (int64_t)i * it.lda + m, hA.data() + oA + (size_t)i * m);
          std::copy(it.hQ + (int64_t)i * it.ldq, it.hQ + (int64_t)i * it.ldq + m, hQ.data() + oA + (size_t)i * m);
          std::copy(it.hB + (int64_t)i * it.ldb, it.hB + (int64_t)i * it.ldb + p, hB.data() + oB + (size_t)i * p);
        }
        r.A = dA + oA; r.lda = m; r.Q = dQ + oA; r.ldq = m; r.B = dB + oB; r.ldb = p;
        oA += (size_t)m * m; oB += (size_t)m * p;
      } else {
        r.A = it.dA; r.lda = it.lda; r.B = it.dB; r.ldb = it.ldb; r.C = it.dC; r.ldc = m;
      }
      if (it.hR) {
        for (int a = 0; a < p; ++a) std::copy(it.hR + (int64_t)a * it.ldr, it.hR + (int64_t)a * it.ldr + p, hR.data() + oR + (size_t)a * p);
        r.R = dR + oR;
        oR += (size_t)p * p;
      }
      r.ws = dW + oW; oW += dare_ws_doubles(r.M);
      r.outK = dOut + oK; oK += (size_t)p * m;
      if (it.outP) { r.outP = dOut + oP; oP += (size_t)m * m; }
      r.delta = dOut + nK + nP + (u - b);
      r.status = dInt + (u - b);
      r.iters = dInt + cnt + (u - b);
    }
    if (nA) {
      NK_HIP(hipMemcpyAsync(dA, hA.data(), nA * 8, hipMemcpyHostToDevice, ctx->stream));
      NK_HIP(hipMemcpyAsync(dQ, hQ.data(), nA * 8, hipMemcpyHostToDevice, ctx->stream));
      NK_HIP(hipMemcpyAsync(dB, hB.data(), nB * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    if (nR) NK_HIP(hipMemcpyAsync(dR, hR.data(), nR * 8, hipMemcpyHostToDevice, ctx->stream));
    NK_HIP(hipMemcpyAsync(dTab, recs.data(), cnt * sizeof(DareRec), hipMemcpyHostToDevice, ctx->stream));
    NK_TRY(launch_dare(ctx, dTab, (int)cnt, tol, max_iter));
    std::vector<double> hOut(nOut);
    std::vector<int> hInt(2 * cnt);
    NK_HIP(hipMemcpyAsync(hOut.data(), dOut, nOut * 8, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemcpyAsync(hInt.data(), dInt, 2 * cnt * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    oK = 0; oP = nK;
    for (size_t u = b; u < e; ++u) {
      const DareItem& it = items[u];
      const size_t km = (size_t)it.p * it.m, mm = (size_t)it.m * it.m;
      if (it.outK) std::copy(hOut.data() + oK, hOut.data() + oK + km, it.outK);
      oK += km;
      if (it.outP) { std::copy(hOut.data() + oP, hOut.data() + oP + mm, it.outP); oP += mm; }
      if (it.out_delta) *it.out_delta = hOut[nK + nP + (u - b)];
      if (out_status) out_status[u] = hInt[u - b];
      if (out_iters) out_iters[u] = hInt[cnt + (u - b)];
    }
    arena_release(ctx, mk);
    b = e;
  }
  return NK_OK;
}

static int dare_check_common(nk_ctx* ctx, const char* who, double tol, int32_t max_iter) {
  NK_REQUIRE(!ctx_recording(ctx), "%s: not available to the members of a lock-step group", who);
  NK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "%s: tol must be finite and non-negative", who);
  NK_REQUIRE(max_iter >= 1 && max_iter <= 1000, "%s: max_iter = %d must lie in 1 .. 1000", who, max_iter);
  return NK_OK;
}

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

int nk_plant_step(int plant, double Ts, const double* x, const double* u, double* x_next) {
  NK_REQUIRE(plant_dim(plant) > 0, "nk_plant_step: unknown plant %d", plant);
  NK_REQUIRE(x && u && x_next, "nk_plant_step: null argument");
  double xn[PLANT_MAX_D];
  if (plant == NK_PLANT_DUFFING) plant_step<NK_PLANT_DUFFING>(Ts, x, u[0], xn);
  else if (plant == NK_PLANT_DOUBLE_INTEGRATOR) plant_step<NK_PLANT_DOUBLE_INTEGRATOR>(Ts, x, u[0], xn);
  else plant_step<NK_PLANT_HJB>(Ts, x, u[0], xn);
  for (int k = 0; k < plant_dim(plant); ++k) x_next[k] = xn[k];
  return NK_OK;
}

int nk_plant_loop(nk_ctx* ctx, const nk_model* mdl, int plant, double Ts, const double* K, const double* x0,
                  const double* x_ref, int32_t steps, int32_t batch, double* out_x, double* out_u) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_plant_loop: not available to the members of a lock-step group");
  NK_REQUIRE(mdl && K && x0 && x_ref && out_x && out_u, "nk_plant_loop: null argument");
  NK_REQUIRE(plant_dim(plant) > 0, "nk_plant_loop: unknown plant %d", plant);
  NK_REQUIRE(mdl->p == 1, "nk_plant_loop: the plants have one input, the model has %d", mdl->p);
  NK_REQUIRE(mdl->d == plant_dim(plant), "nk_plant_loop: the %s has %d states, the model has %d", plant_name(plant),
             plant_dim(plant), mdl->d);
  NK_REQUIRE(steps >= 1 && batch >= 1, "nk_plant_loop: steps = %d and batch = %d must be positive", steps, batch);
  NK_REQUIRE(mdl->m <= plant_loop_max_m(), "nk_plant_loop: m = %d landmarks, at most %d fit one workgroup", mdl->m,
             plant_loop_max_m());
  const bool spline = mdl->kind == NK_MODEL_SPLINE;
  NK_REQUIRE(spline ? mdl->ktype == NK_KERNEL_TPS
                    : (mdl->ktype == NK_KERNEL_RBF || mdl->ktype == NK_KERNEL_MATERN52 || mdl->ktype == NK_KERNEL_LINEAR),
             "nk_plant_loop: kernel type %d is not supported for this model", mdl->ktype);
  NK_REQUIRE(std::isfinite(Ts), "nk_plant_loop: Ts is not finite");
  const int m = mdl->m, d = mdl->d;
  MatIn k, xi, xr;
  MatOut ox, ou;
  NK_TRY(stage_in(ctx, K, m, 1, m, &k));
  NK_TRY(stage_in(ctx, x0, d, batch, d, &xi));
  NK_TRY(stage_in(ctx, x_ref, d, batch, d, &xr));
  NK_TRY(stage_out(ctx, out_x, d, (int64_t)batch * (steps + 1), d, &ox));
  NK_TRY(stage_out(ctx, out_u, 1, (int64_t)batch * steps, 1, &ou));
  // u = K phi = K (k S^-1)^T = (S^-1 K^T) . k: the product nk_lift forms, contracted with the gain first
  const double* w = k.ptr;
  if (!spline) {
    double* wf = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)m + 2, &wf));
    NK_TRY(launch_gemm(ctx, false, true, m, 1, m, 1.0, mdl->Sinv, m, k.ptr, k.ld, 0.0, wf, 1));
    w = wf;
  }
  NK_TRY(launch_plant_loop(ctx, mdl, plant, Ts, w, xi.ptr, xi.ld, xr.ptr, xr.ld, steps, batch, ox.dev, ox.ld, ou.dev,
                           ou.ld));
  NK_TRY(finish_out(ctx, ox));
  NK_TRY(finish_out(ctx, ou));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_plant_loop_multi(nk_ctx* ctx, int plant, double Ts, int32_t steps, const nk_plant_unit* units, int32_t n_units,
                        const double* u_opt, int32_t n_uopt, double* out_x, double* out_u, double* scores) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_plant_loop_multi: not available to the members of a lock-step group");
  NK_REQUIRE(plant_dim(plant) > 0, "nk_plant_loop_multi: unknown plant %d", plant);
  NK_REQUIRE(units != nullptr && n_units >= 1, "nk_plant_loop_multi: n_units = %d units at %p: at least one is needed",
             n_units, (const void*)units);
  NK_REQUIRE(steps >= 1, "nk_plant_loop_multi: steps = %d must be positive", steps);
  NK_REQUIRE(std::isfinite(Ts), "nk_plant_loop_multi: Ts is not finite");
  NK_REQUIRE(out_x || out_u || scores, "nk_plant_loop_multi: out_x, out_u and scores are all null: nothing to return");
  NK_REQUIRE(n_uopt >= 0 && (n_uopt == 0 || u_opt != nullptr), "nk_plant_loop_multi: n_uopt = %d rows of a null u_opt",
             n_uopt);
  NK_REQUIRE(!is_device_ptr(scores), "nk_plant_loop_multi: scores must be host memory");
  const int d = plant_dim(plant);
  // every unit is checked before anything is queued; the staging layout is laid out on the way (slots start on 256 bytes
  // and a gain row has the even leading dimension stage_in gives it in nk_plant_loop: the fold sees the same operands)
  auto slot = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
  std::vector<size_t> k_off((size_t)n_units), w_off((size_t)n_units);
  size_t in_doubles = 0, w_doubles = 0;
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    const nk_model* mdl = un.model;
    NK_REQUIRE(mdl && un.K && un.x0 && un.x_ref, "nk_plant_loop_multi: unit %d: null argument", u);
    NK_REQUIRE(mdl->device == ctx->device, "nk_plant_loop_multi: unit %d: the model lives on device %d, the context on %d",
               u, mdl->device, ctx->device);
    NK_REQUIRE(mdl->p == 1, "nk_plant_loop_multi: unit %d: the plants have one input, the model has %d", u, mdl->p);
    NK_REQUIRE(mdl->d == d, "nk_plant_loop_multi: unit %d: the %s has %d states, the model has %d", u, plant_name(plant), d,
               mdl->d);
    NK_REQUIRE(mdl->m >= 1 && mdl->m <= plant_loop_max_m(),
               "nk_plant_loop_multi: unit %d: m = %d landmarks, at most %d fit one workgroup", u, mdl->m, plant_loop_max_m());
    const bool spline = mdl->kind == NK_MODEL_SPLINE;
    NK_REQUIRE(spline ? mdl->ktype == NK_KERNEL_TPS
                      : (mdl->ktype == NK_KERNEL_RBF || mdl->ktype == NK_KERNEL_MATERN52 || mdl->ktype == NK_KERNEL_LINEAR),
               "nk_plant_loop_multi: unit %d: kernel type %d is not supported for this model", u, mdl->ktype);
    NK_REQUIRE(un.uopt >= -1 && un.uopt < n_uopt, "nk_plant_loop_multi: unit %d: uopt = %d, u_opt has %d rows", u, un.uopt,
               n_uopt);
    NK_REQUIRE(!is_device_ptr(un.K) && !is_device_ptr(un.x0) && !is_device_ptr(un.x_ref),
               "nk_plant_loop_multi: unit %d: K, x0 and x_ref must be host memory", u);
    k_off[u] = in_doubles;
    in_doubles += slot((size_t)mdl->m + (mdl->m & 1)) + slot(2 * (size_t)d);  // K | x0, x_ref
    if (!spline) {
      w_off[u] = w_doubles;
      w_doubles += slot((size_t)mdl->m + 2);
    }
  }
  // one staging block for every gain, initial state and reference: one copy
  std::vector<double> h_in(in_doubles, 0.0);
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    const int m = un.model->m;
    double* dst = h_in.data() + k_off[u];
    std::copy(un.K, un.K + m, dst);
    dst += slot((size_t)m + (m & 1));
    std::copy(un.x0, un.x0 + d, dst);
    std::copy(un.x_ref, un.x_ref + d, dst + d);
  }
  double *d_in = nullptr, *d_w = nullptr, *d_sc = nullptr;
  NK_TRY(arena_alloc_t(ctx, in_doubles, &d_in));
  NK_HIP(hipMemcpyAsync(d_in, h_in.data(), in_doubles * 8, hipMemcpyHostToDevice, ctx->stream));
  if (w_doubles) NK_TRY(arena_alloc_t(ctx, w_doubles, &d_w));
  if (scores) NK_TRY(arena_alloc_t(ctx, (size_t)n_units * 4, &d_sc));
  MatIn uo;
  MatOut ox, ou;
  if (n_uopt > 0) NK_TRY(stage_in(ctx, u_opt, steps, n_uopt, steps, &uo));
  if (out_x) NK_TRY(stage_out(ctx, out_x, d, (int64_t)n_units * (steps + 1), d, &ox));
  if (out_u) NK_TRY(stage_out(ctx, out_u, 1, (int64_t)n_units * steps, 1, &ou));
  std::vector<PlantLoopUnit> recs((size_t)n_units);
  std::vector<int> ktypes((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    const nk_model* mdl = un.model;
    const int m = mdl->m;
    const double* k_dev = d_in + k_off[u];
    const double* xs = k_dev + slot((size_t)m + (m & 1));
    // u = K phi = K (k S^-1)^T = (S^-1 K^T) . k, the fold of nk_plant_loop by the same call; the folds of all units are
    // queued back to back, nothing waits between them
    const double* w = k_dev;
    if (mdl->kind != NK_MODEL_SPLINE) {
      double* wf = d_w + w_off[u];
      NK_TRY(launch_gemm(ctx, false, true, m, 1, m, 1.0, mdl->Sinv, m, k_dev, m + (m & 1), 0.0, wf, 1));
      w = wf;
    }
    PlantLoopUnit& r = recs[u];
    r.Z = mdl->Z; r.winv = mdl->winv; r.w = w; r.x0 = xs; r.xref = xs + d;
    r.out_x = out_x ? ox.dev + (int64_t)u * (steps + 1) * ox.ld : nullptr; r.ldx = out_x ? ox.ld : 0;
    r.out_u = out_u ? ou.dev + (int64_t)u * steps * ou.ld : nullptr; r.ldu = out_u ? ou.ld : 0;
    r.u_opt = un.uopt >= 0 ? uo.ptr + (int64_t)un.uopt * uo.ld : nullptr;
    r.score = scores ? d_sc + 4 * (size_t)u : nullptr;
    r.sigma0sq = mdl->sigma0 * mdl->sigma0; r.m = m; r.reserved = 0;
    ktypes[u] = mdl->ktype;
  }
  NK_TRY(launch_plant_loop_multi(ctx, plant, Ts, steps, recs.data(), ktypes.data(), n_units));
  if (out_x) NK_TRY(finish_out(ctx, ox));
  if (out_u) NK_TRY(finish_out(ctx, ou));
  if (scores) NK_HIP(hipMemcpyAsync(scores, d_sc, (size_t)n_units * 32, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (h_in and recs are read by the copies queued above)
  return NK_OK;
}

int nk_closed_loop_multi(nk_ctx* ctx, int32_t steps, double c, const nk_loop_unit* units, int32_t n_units, double* out_x,
                         double* out_u, double* out_ucum, double* out_err, double* scores) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_closed_loop_multi: not available to the members of a lock-step group");
  NK_REQUIRE(units != nullptr && n_units >= 1, "nk_closed_loop_multi: n_units = %d units at %p: at least one is needed",
             n_units, (const void*)units);
  NK_REQUIRE(steps >= 1, "nk_closed_loop_multi: steps = %d must be positive", steps);
  NK_REQUIRE(std::isfinite(c) && c >= 0.0, "nk_closed_loop_multi: c must be finite and non-negative");
  NK_REQUIRE(out_x || out_u || out_ucum || out_err || scores,
             "nk_closed_loop_multi: out_x, out_u, out_ucum, out_err and scores are all null: nothing to return");
  NK_REQUIRE(!is_device_ptr(scores), "nk_closed_loop_multi: scores must be host memory");
  // every unit is checked before anything is queued; the staging block (slots start on 256 bytes) and the dense,
  // unit-major output offsets are laid out on the way
  auto slot = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
  const bool scored = out_err != nullptr || scores != nullptr;
  std::vector<size_t> in_off((size_t)n_units), ws_off((size_t)n_units), x_off((size_t)n_units), u_off((size_t)n_units),
      uc_off((size_t)n_units);
  size_t in_doubles = 0, ws_doubles = 0, x_doubles = 0, u_doubles = 0, uc_doubles = 0;
  for (int u = 0; u < n_units; ++u) {
    const nk_loop_unit& un = units[u];
    const nk_model* mdl = un.model;
    NK_REQUIRE(mdl != nullptr, "nk_closed_loop_multi: unit %d: the model is null", u);
    NK_REQUIRE(mdl->p >= 1 && mdl->p <= LOOP_MULTI_MAX_P, "nk_closed_loop_multi: unit %d: p = %d inputs must lie in 1 .. %d", u,
               mdl->p, LOOP_MULTI_MAX_P);
    NK_REQUIRE(mdl->m >= 1 && mdl->m <= LOOP_MULTI_MAX_M,
               "nk_closed_loop_multi: unit %d: m = %d must lie in 1 .. %d (larger models: nk_closed_loop)", u, mdl->m,
               LOOP_MULTI_MAX_M);
    NK_REQUIRE(mdl->d >= 1, "nk_closed_loop_multi: unit %d: d = %d", u, mdl->d);
    NK_REQUIRE(mdl->has_ops, "nk_closed_loop_multi: unit %d: the model holds no fitted operators", u);
    NK_REQUIRE(mdl->device == ctx->device, "nk_closed_loop_multi: unit %d: the model lives on device %d, the context on %d", u,
               mdl->device, ctx->device);
    NK_REQUIRE(un.K && un.phi0 && un.phi_ref, "nk_closed_loop_multi: unit %d: null argument (K, phi0, phi_ref)", u);
    NK_REQUIRE(un.target != nullptr || !scored,
               "nk_closed_loop_multi: unit %d: target is null, but out_err or scores are requested", u);
    NK_REQUIRE(!is_device_ptr(un.K) && !is_device_ptr(un.phi0) && !is_device_ptr(un.phi_ref) && !is_device_ptr(un.target) &&
                   !is_device_ptr(un.u_init),
               "nk_closed_loop_multi: unit %d: K, phi0, phi_ref, target and u_init must be host memory", u);
    const size_t m = (size_t)mdl->m, p = (size_t)mdl->p, d = (size_t)mdl->d;
    in_off[u] = in_doubles;
    in_doubles += slot(p * m) + 2 * slot(m) + slot(d) + slot(p);  // K | phi0 | phi_ref | target | u_init
    ws_off[u] = ws_doubles;
    ws_doubles += slot((size_t)steps * m) + 2 * slot((size_t)steps);  // phi_t | sum u^2 | sum (x - target)^2, per step
    x_off[u] = x_doubles;
    x_doubles += (size_t)steps * d;
    u_off[u] = u_doubles;
    u_doubles += (size_t)steps * p;
    uc_off[u] = uc_doubles;
    uc_doubles += ((size_t)steps + 1) * p;
  }
  // one staging block for every gain, lifted state, target and seed: one copy
  std::vector<double> h_in(in_doubles, 0.0);
  for (int u = 0; u < n_units; ++u) {
    const nk_loop_unit& un = units[u];
    const size_t m = (size_t)un.model->m, p = (size_t)un.model->p, d = (size_t)un.model->d;
    double* dst = h_in.data() + in_off[u];
    std::copy(un.K, un.K + p * m, dst);
    dst += slot(p * m);
    std::copy(un.phi0, un.phi0 + m, dst);
    dst += slot(m);
    std::copy(un.phi_ref, un.phi_ref + m, dst);
    dst += slot(m);
    if (un.target) std::copy(un.target, un.target + d, dst);
    dst += slot(d);
    if (un.u_init) std::copy(un.u_init, un.u_init + p, dst);
  }
  double *d_in = nullptr, *d_ws = nullptr, *d_sc = nullptr;
  NK_TRY(arena_alloc_t(ctx, in_doubles, &d_in));
  NK_HIP(hipMemcpyAsync(d_in, h_in.data(), in_doubles * 8, hipMemcpyHostToDevice, ctx->stream));
  NK_TRY(arena_alloc_t(ctx, ws_doubles, &d_ws));
  if (scores) NK_TRY(arena_alloc_t(ctx, (size_t)n_units * 4, &d_sc));
  // a dense output: the caller's device memory as it is, or an arena block that one copy brings back
  struct Out { double* host; double* dev; size_t doubles; };
  Out outs[4] = {{out_x, nullptr, x_doubles}, {out_u, nullptr, u_doubles}, {out_ucum, nullptr, uc_doubles},
                 {out_err, nullptr, (size_t)n_units * steps}};
  for (Out& o : outs) {
    if (!o.host) continue;
    if (is_device_ptr(o.host)) { o.dev = o.host; o.host = nullptr; }
    else NK_TRY(arena_alloc_t(ctx, o.doubles, &o.dev));
  }
  std::vector<LoopMultiUnit> recs((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_model* mdl = units[u].model;
    const size_t m = (size_t)mdl->m, p = (size_t)mdl->p, d = (size_t)mdl->d;
    LoopMultiUnit& r = recs[u];
    r = LoopMultiUnit{};
    r.G = mdl->A; r.ldg = mdl->m + mdl->p; r.C = mdl->C;
    const double* in = d_in + in_off[u];
    r.K = in; in += slot(p * m);
    r.phi0 = in; in += slot(m);
    r.phi_ref = in; in += slot(m);
    r.target = units[u].target ? in : nullptr; in += slot(d);
    r.u_init = in;
    double* ws = d_ws + ws_off[u];
    r.Phi = ws; ws += slot((size_t)steps * m);
    r.usq = ws; ws += slot((size_t)steps);
    r.sse = ws;
    r.out_x = outs[0].dev ? outs[0].dev + x_off[u] : nullptr; r.ldx = mdl->d;
    r.out_u = outs[1].dev ? outs[1].dev + u_off[u] : nullptr; r.ldu = mdl->p;
    r.out_ucum = outs[2].dev ? outs[2].dev + uc_off[u] : nullptr; r.ldc = mdl->p;
    r.out_err = outs[3].dev ? outs[3].dev + (size_t)u * steps : nullptr;
    r.score = scores ? d_sc + 4 * (size_t)u : nullptr;
    r.m = mdl->m; r.p = mdl->p; r.d = mdl->d;
  }
  NK_TRY(launch_closed_loop_multi(ctx, recs.data(), n_units, steps, c));
  for (const Out& o : outs)
    if (o.host) NK_HIP(hipMemcpyAsync(o.host, o.dev, o.doubles * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (scores) NK_HIP(hipMemcpyAsync(scores, d_sc, (size_t)n_units * 32, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (h_in and recs are read by the copies queued above)
  return NK_OK;
}

int nk_dare_batch(nk_ctx* ctx, const nk_dare_problem* problems, int32_t n, double tol, int32_t max_iter,
                  int32_t* out_status, int32_t* out_iters) {
  NK_TRY(check_ctx(ctx));
  NK_TRY(dare_check_common(ctx, "nk_dare_batch", tol, max_iter));
  NK_REQUIRE(problems != nullptr && n >= 1, "nk_dare_batch: n = %d problems at %p: at least one is needed", n,
             (const void*)problems);
  NK_REQUIRE(out_status != nullptr, "nk_dare_batch: out_status is null");
  std::vector<DareItem> items((size_t)n);
  for (int u = 0; u < n; ++u) {  // everything is checked before anything is queued
    const nk_dare_problem& pr = problems[u];
    NK_REQUIRE(pr.m >= 1 && pr.m <= DARE_MAX_M, "nk_dare_batch: problem %d: m = %d must lie in 1 .. %d", u, pr.m, DARE_MAX_M);
    NK_REQUIRE(pr.p >= 1 && pr.p <= DARE_MAX_P, "nk_dare_batch: problem %d: p = %d must lie in 1 .. %d", u, pr.p, DARE_MAX_P);
    NK_REQUIRE(pr.A && pr.B && pr.Q && pr.R && pr.out_K, "nk_dare_batch: problem %d: null argument", u);
    NK_REQUIRE(pr.lda >= pr.m && pr.ldq >= pr.m && pr.ldb >= pr.p && pr.ldr >= pr.p,
               "nk_dare_batch: problem %d: leading dimension too small", u);
    NK_REQUIRE(!is_device_ptr(pr.A) && !is_device_ptr(pr.B) && !is_device_ptr(pr.Q) && !is_device_ptr(pr.R) &&
                   !is_device_ptr(pr.out_K) && !is_device_ptr(pr.out_P) && !is_device_ptr(pr.out_delta),
               "nk_dare_batch: problem %d: operands and results must be host memory", u);
    DareItem& it = items[u];
    it.m = pr.m; it.p = pr.p;
    it.hA = pr.A; it.lda = pr.lda; it.hB = pr.B; it.ldb = pr.ldb; it.hQ = pr.Q; it.ldq = pr.ldq; it.hR = pr.R; it.ldr = pr.ldr;
    it.outK = pr.out_K; it.outP = pr.out_P; it.out_delta = pr.out_delta;
  }
  return dare_run(ctx, items, tol, max_iter, out_status, out_iters);
}

static int dare_check_model(nk_ctx* ctx, const char* who, const nk_model* mdl, int u) {
  NK_REQUIRE(mdl != nullptr, "%s: model %d is null", who, u);
  NK_REQUIRE(mdl->device == ctx->device, "%s: model %d lives on device %d, the context on %d", who, u, mdl->device,
             ctx->device);
  NK_REQUIRE(mdl->has_ops, "%s: model %d has no fitted operators", who, u);
  NK_REQUIRE(mdl->m >= 1 && mdl->m <= DARE_MAX_M, "%s: model %d: m = %d must lie in 1 .. %d", who, u, mdl->m, DARE_MAX_M);
  NK_REQUIRE(mdl->p >= 1 && mdl->p <= DARE_MAX_P, "%s: model %d: p = %d must lie in 1 .. %d", who, u, mdl->p, DARE_MAX_P);
  return NK_OK;
}

int nk_model_lqr_gain_batch(nk_ctx* ctx, const nk_model* const* models, int32_t n, double c, const double* R, double tol,
                            int32_t max_iter, double* out_K, int32_t* out_status, int32_t* out_iters) {
  NK_TRY(check_ctx(ctx));
  NK_TRY(dare_check_common(ctx, "nk_model_lqr_gain_batch", tol, max_iter));
  NK_REQUIRE(models != nullptr && n >= 1, "nk_model_lqr_gain_batch: n = %d models at %p: at least one is needed", n,
             (const void*)models);
  NK_REQUIRE(out_K != nullptr && out_status != nullptr, "nk_model_lqr_gain_batch: null output");
  NK_REQUIRE(std::isfinite(c) && c >= 0.0, "nk_model_lqr_gain_batch: c must be finite and non-negative");
  NK_REQUIRE(!is_device_ptr(out_K) && !is_device_ptr(R), "nk_model_lqr_gain_batch: R and out_K must be host memory");
  std::vector<DareItem> items((size_t)n);
  size_t off = 0;
  for (int u = 0; u < n; ++u) {
    const nk_model* mdl = models[u];
    NK_TRY(dare_check_model(ctx, "nk_model_lqr_gain_batch", mdl, u));
    NK_REQUIRE(R == nullptr || mdl->p == models[0]->p,
               "nk_model_lqr_gain_batch: model %d has %d inputs, R is %d x %d", u, mdl->p, models[0]->p, models[0]->p);
    DareItem& it = items[u];
    it.m = mdl->m; it.p = mdl->p; it.d = mdl->d; it.c = c;
    it.dA = mdl->A; it.dB = mdl->B; it.lda = it.ldb = mdl->m + mdl->p; it.dC = mdl->C;
    it.hR = R; it.ldr = mdl->p;
    it.outK = out_K + off;
    off += (size_t)mdl->p * mdl->m;
  }
  return dare_run(ctx, items, tol, max_iter, out_status, out_iters);
}

int nk_model_lqr_cost(nk_ctx* ctx, const nk_model* model, double c, double* Q, int64_t ldq) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_model_lqr_cost: not available to the members of a lock-step group");
  NK_TRY(dare_check_model(ctx, "nk_model_lqr_cost", model, 0));
  NK_REQUIRE(Q != nullptr && ldq >= model->m && !is_device_ptr(Q), "nk_model_lqr_cost: Q must be host memory with ldq >= m");
  NK_REQUIRE(std::isfinite(c), "nk_model_lqr_cost: c is not finite");
  const int m = model->m;
  std::vector<double> q((size_t)m * m);
  std::vector<DareItem> items(1);
  DareItem& it = items[0];
  it.m = m; it.p = model->p; it.d = model->d; it.c = c;
  it.dA = model->A; it.dB = model->B; it.lda = it.ldb = m + model->p; it.dC = model->C;
  it.outP = q.data(); it.q_only = 1;
  int32_t st = 0;
  NK_TRY(dare_run(ctx, items, 0.0, 1, &st, nullptr));
  for (int i = 0; i < m; ++i) std::copy(q.begin() + (size_t)i * m, q.begin() + (size_t)(i + 1) * m, Q + (int64_t)i * ldq);
  return NK_OK;
}

}  // extern "C"
