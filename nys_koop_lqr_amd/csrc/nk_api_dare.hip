// The Riccati entry points behind the C ABI (nk_dare_batch, nk_model_lqr_gain_batch, nk_model_lqr_cost): checks, staging of
// the problems and one launch of the batched solver (nk_dare.hip) per workspace-capped group; and the two entries of the
// launch-chain solver for one problem of any size (nk_dare_large, nk_model_lqr_gain: nk_dare_large.hip).
#include "nk_common.h"
#include "nk_api_internal.h"

#include <cmath>
#include <algorithm>
#include <vector>

using namespace nk;

// One problem of the batched Riccati solver as the two entry points hand it over: operands in host memory (nk_dare_batch;
// dense copies are packed and staged with one copy) or in a model's device allocation (the model entries).
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
  for (size_t b = 0, e = 0; b < n; b = e) {
    size_t ws = 0;
    for (e = b; e < n; ++e) {
      const size_t w = dare_ws_doubles(dare_pad(items[e].m)) * 8;
      if (e > b && ws + w > (size_t)NK_DARE_WS_CAP_BYTES) break;
      ws += w;
    }
    const size_t cnt = e - b;
    const ArenaMark mk = arena_mark(ctx);
    // the host operands of the group, dense, in one staging block (nk_unit_pack.h); the results in another
    UnitPack in, out;
    struct Off { size_t A, Q, B, R, K, P; };
    std::vector<Off> off(cnt);
    auto dense = [&in](const double* src, int64_t ld, int rows, int cols) {
      const size_t at = in.reserve((size_t)rows * cols);
      for (int i = 0; i < rows; ++i) in.copy(at + (size_t)i * cols, src + (int64_t)i * ld, (size_t)cols);
      return at;
    };
    for (size_t u = b; u < e; ++u) {
      const DareItem& it = items[u];
      Off& o = off[u - b];
      if (it.hA) {
        o.A = dense(it.hA, it.lda, it.m, it.m); o.Q = dense(it.hQ, it.ldq, it.m, it.m); o.B = dense(it.hB, it.ldb, it.m, it.p);
      }
      if (it.hR) o.R = dense(it.hR, it.ldr, it.p, it.p);
      o.K = out.reserve((size_t)it.p * it.m);
      if (it.outP) o.P = out.reserve((size_t)it.m * it.m);
    }
    const size_t o_delta = out.reserve(cnt);
    double *dIn = nullptr, *dW = nullptr, *dOut = nullptr;
    int* dInt = nullptr;
    DareRec* dTab = nullptr;
    if (in.doubles()) NK_TRY(stage_pack(ctx, in, &dIn));
    NK_TRY(arena_alloc_t(ctx, ws / 8, &dW));
    NK_TRY(arena_alloc_t(ctx, out.doubles(), &dOut));
    NK_TRY(arena_alloc_t(ctx, 2 * cnt, &dInt));
    NK_TRY(arena_alloc_t(ctx, cnt, &dTab));
    std::vector<DareRec> recs(cnt);
    size_t oW = 0;
    for (size_t u = b; u < e; ++u) {
      const DareItem& it = items[u];
      const Off& o = off[u - b];
      DareRec& r = recs[u - b];
      r = DareRec{};
      r.m = it.m; r.p = it.p; r.M = dare_pad(it.m); r.d = it.d; r.c = it.c; r.q_only = it.q_only;
      if (it.hA) {
        r.A = dIn + o.A; r.lda = it.m; r.Q = dIn + o.Q; r.ldq = it.m; r.B = dIn + o.B; r.ldb = it.p;
      } else {
        r.A = it.dA; r.lda = it.lda; r.B = it.dB; r.ldb = it.ldb; r.C = it.dC; r.ldc = it.m;
      }
      if (it.hR) r.R = dIn + o.R;
      r.ws = dW + oW; oW += dare_ws_doubles(r.M);
      r.outK = dOut + o.K;
      if (it.outP) r.outP = dOut + o.P;
      r.delta = dOut + o_delta + (u - b);
      r.status = dInt + (u - b);
      r.iters = dInt + cnt + (u - b);
    }
    NK_HIP(hipMemcpyAsync(dTab, recs.data(), cnt * sizeof(DareRec), hipMemcpyHostToDevice, ctx->stream));
    NK_TRY(launch_dare(ctx, dTab, (int)cnt, tol, max_iter));
    std::vector<double> hOut(out.doubles());
    std::vector<int> hInt(2 * cnt);
    NK_HIP(hipMemcpyAsync(hOut.data(), dOut, hOut.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemcpyAsync(hInt.data(), dInt, 2 * cnt * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t u = b; u < e; ++u) {
      const DareItem& it = items[u];
      const Off& o = off[u - b];
      if (it.outK) std::copy(hOut.data() + o.K, hOut.data() + o.K + (size_t)it.p * it.m, it.outK);
      if (it.outP) std::copy(hOut.data() + o.P, hOut.data() + o.P + (size_t)it.m * it.m, it.outP);
      if (it.out_delta) *it.out_delta = hOut[o_delta + (u - b)];
      if (out_status) out_status[u] = hInt[u - b];
      if (out_iters) out_iters[u] = hInt[cnt + (u - b)];
    }
    arena_release(ctx, mk);
  }
  return NK_OK;
}

static int dare_check_common(nk_ctx* ctx, const char* who, double tol, int32_t max_iter) {
  NK_REQUIRE(!ctx_recording(ctx), "%s: not available to the members of a lock-step group", who);
  NK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "%s: tol must be finite and non-negative", who);
  NK_REQUIRE(max_iter >= 1 && max_iter <= 1000, "%s: max_iter = %d must lie in 1 .. 1000", who, max_iter);
  return NK_OK;
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

extern "C" {

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

// The two entries of the launch-chain solver (nk_dare_large.hip): operands staged as nk_gemm stages its own (host memory is
// copied into the arena, device memory is used in place), one solver call, the results copied back.
static int dare_large_run(nk_ctx* ctx, DareLargeArgs& a, double* out_K, double* out_P, double* out_delta,
                          int32_t* out_status, int32_t* out_iters) {
  MatOut k, pm;
  NK_TRY(stage_out(ctx, out_K, a.m, a.p, a.m, &k));
  a.outK = k.dev; a.ldk = k.ld;
  if (out_P) {
    NK_TRY(stage_out(ctx, out_P, a.m, a.m, a.m, &pm));
    a.outP = pm.dev; a.ldp = pm.ld;
  }
  DareLargeResult res;
  NK_TRY(launch_dare_large(ctx, a, &res));
  NK_TRY(finish_out(ctx, k));
  if (out_P) NK_TRY(finish_out(ctx, pm));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  *out_status = res.status;
  if (out_iters) *out_iters = res.iters;
  if (out_delta) *out_delta = res.delta;
  return NK_OK;
}

int nk_dare_large(nk_ctx* ctx, int32_t m, int32_t p, const double* A, int64_t lda, const double* B, int64_t ldb,
                  const double* Q, int64_t ldq, const double* R, int64_t ldr, double tol, int32_t max_iter, double* out_K,
                  double* out_P, double* out_delta, int32_t* out_status, int32_t* out_iters) {
  NK_TRY(check_ctx(ctx));
  NK_TRY(dare_check_common(ctx, "nk_dare_large", tol, max_iter));
  NK_REQUIRE(m >= 1 && m <= NK_DARE_LARGE_MAX_M, "nk_dare_large: m = %d must lie in 1 .. %d", m, NK_DARE_LARGE_MAX_M);
  NK_REQUIRE(p >= 1 && p <= NK_DARE_LARGE_MAX_P, "nk_dare_large: p = %d must lie in 1 .. %d", p, NK_DARE_LARGE_MAX_P);
  NK_REQUIRE(A && B && Q && R && out_K && out_status, "nk_dare_large: null argument");
  NK_REQUIRE(lda >= m && ldq >= m && ldb >= p && ldr >= p, "nk_dare_large: leading dimension too small");
  DareLargeArgs a;
  a.m = m; a.p = p; a.tol = tol; a.max_iter = max_iter;
  MatIn ma, mb, mq, mr;
  NK_TRY(stage_in(ctx, A, lda, m, m, &ma));
  NK_TRY(stage_in(ctx, B, ldb, m, p, &mb));
  NK_TRY(stage_in(ctx, Q, ldq, m, m, &mq));
  NK_TRY(stage_in(ctx, R, ldr, p, p, &mr));
  a.A = ma.ptr; a.lda = ma.ld; a.B = mb.ptr; a.ldb = mb.ld; a.Q = mq.ptr; a.ldq = mq.ld; a.R = mr.ptr; a.ldr = mr.ld;
  return dare_large_run(ctx, a, out_K, out_P, out_delta, out_status, out_iters);
}

int nk_model_lqr_gain(nk_ctx* ctx, const nk_model* model, double c, const double* R, double tol, int32_t max_iter,
                      double* out_K, int32_t* out_status, int32_t* out_iters) {
  NK_TRY(check_ctx(ctx));
  NK_TRY(dare_check_common(ctx, "nk_model_lqr_gain", tol, max_iter));
  NK_REQUIRE(model != nullptr, "nk_model_lqr_gain: the model is null");
  NK_REQUIRE(model->device == ctx->device, "nk_model_lqr_gain: the model lives on device %d, the context on %d", model->device,
             ctx->device);
  NK_REQUIRE(model->has_ops, "nk_model_lqr_gain: the model has no fitted operators");
  NK_REQUIRE(model->m >= 1 && model->m <= NK_DARE_LARGE_MAX_M, "nk_model_lqr_gain: m = %d must lie in 1 .. %d", model->m,
             NK_DARE_LARGE_MAX_M);
  NK_REQUIRE(model->p >= 1 && model->p <= NK_DARE_LARGE_MAX_P, "nk_model_lqr_gain: p = %d must lie in 1 .. %d", model->p,
             NK_DARE_LARGE_MAX_P);
  NK_REQUIRE(out_K != nullptr && out_status != nullptr, "nk_model_lqr_gain: null output");
  NK_REQUIRE(std::isfinite(c) && c >= 0.0, "nk_model_lqr_gain: c must be finite and non-negative");
  DareLargeArgs a;
  a.m = model->m; a.p = model->p; a.d = model->d; a.tol = tol; a.max_iter = max_iter;
  a.A = model->A; a.B = model->B; a.lda = a.ldb = model->m + model->p;
  a.C = model->C; a.ldc = model->m; a.c = c;
  if (R) {
    MatIn mr;
    NK_TRY(stage_in(ctx, R, model->p, model->p, model->p, &mr));
    a.R = mr.ptr; a.ldr = mr.ld;
  }
  return dare_large_run(ctx, a, out_K, nullptr, nullptr, out_status, out_iters);
}

int nk_dare_large_times(double out[5]) {
  NK_REQUIRE(out != nullptr, "nk_dare_large_times: out is null");
  DareLargeTimes t;
  dare_large_last_times(&t);
  out[0] = t.ms_total; out[1] = t.ms_lu; out[2] = t.ms_products; out[3] = t.ms_sync; out[4] = (double)t.steps;
  return NK_OK;
}

}  // extern "C"