// The controller-build entry points behind the C ABI (nk_mpc_build_batch, nk_model_mpc_build_batch): checks, staging of the
// units (nk_mpc_build_pack.h: one copy in, one copy out per workspace-capped group), the Riccati stage by the existing
// solvers (one launch of the batched solver over the units with m <= 256, the launch-chain solver for each larger one) and
// one launch of the build kernel (nk_mpc_build.hip) per group.
#include "nk_common.h"
#include "nk_api_internal.h"
#include "nk_mpc_build_pack.h"

#include <cmath>
#include <algorithm>
#include <vector>

using namespace nk;

namespace {

struct BuildItem {
  MpcBuildShape sh;
  int d = 0;
  double c = 0.0;
  const double *hA = nullptr, *hB = nullptr, *hQ = nullptr, *hR = nullptr, *hP = nullptr, *hC = nullptr;  // host operands
  int64_t lda = 0, ldb = 0, ldq = 0, ldr = 0, ldp = 0, ldc = 0;
  const double *dA = nullptr, *dB = nullptr, *dC = nullptr;  // ... or a model's device operands ([A B]: ld m + p; C: ld m)
  int comps[MPC_BUILD_MAX_NC] = {0, 1, 2, 3};
  double *oH = nullptr, *oF = nullptr, *oK = nullptr, *oP = nullptr, *oG = nullptr, *oT = nullptr;  // host results, dense
};

struct SolverArgs {
  double tol, newton_tol;
  int max_iter, newton_steps, newton_max_iter;
};

// device time of the calling thread's last build call, by events around the launches (nk_mpc_build_times)
struct BuildTimes {
  double ms_riccati = 0.0, ms_build = 0.0;
  int groups = 0;
};
thread_local BuildTimes g_times;

struct BuildEvents {  // created per call: the contexts' event slots belong to the fit
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~BuildEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct ArenaScope {  // what a group allocates is released on every way out of it
  nk_ctx* ctx;
  ArenaMark mk;
  explicit ArenaScope(nk_ctx* c) : ctx(c), mk(arena_mark(c)) {}
  ~ArenaScope() { arena_release(ctx, mk); }
};

bool riccati_small(const BuildItem& it) { return !it.sh.have_P && it.sh.m <= (size_t)DARE_MAX_M; }

size_t item_ws_bytes(const BuildItem& it) {
  const MpcBuildShape& s = it.sh;
  size_t w = mpc_build_ws_doubles(s.m, s.N * s.p, s.nc ? s.Ny : 0, s.nc, s.p);
  if (!s.have_P) w += unit_slot(s.p * s.m) + unit_slot(s.m * s.m);
  if (riccati_small(it)) w += dare_ws_doubles(dare_pad((int)s.m));
  return w * 8;
}

// Runs the items in groups whose device workspace stays under NK_DARE_WS_CAP_BYTES; every argument has been checked.
int mpc_build_run(nk_ctx* ctx, const std::vector<BuildItem>& items, const SolverArgs& sa, int32_t* out_status,
                  int32_t* out_iters) {
  const size_t n = items.size();
  g_times = BuildTimes{};
  BuildEvents evs;
  for (hipEvent_t& e : evs.ev) NK_HIP(hipEventCreate(&e));
  for (size_t b = 0, e = 0; b < n; b = e) {
    size_t bytes = 0;
    for (e = b; e < n; ++e) {
      const size_t w = item_ws_bytes(items[e]);
      if (e > b && bytes + w > (size_t)NK_DARE_WS_CAP_BYTES) break;
      bytes += w;
    }
    const size_t cnt = e - b;
    const ArenaScope scope(ctx);
    UnitPack in, out, ws;
    std::vector<MpcBuildOffsets> off(cnt);
    size_t dare_doubles = 0, n_small = 0;
    for (size_t u = b; u < e; ++u) {
      const BuildItem& it = items[u];
      off[u - b] = pack_mpc_build_unit(in, out, ws, it.sh, it.hA, (size_t)it.lda, it.hB, (size_t)it.ldb, it.hQ, (size_t)it.ldq,
                                       it.hR, (size_t)it.ldr, it.hP, (size_t)it.ldp, it.hC, (size_t)it.ldc);
      if (riccati_small(it)) { dare_doubles += dare_ws_doubles(dare_pad((int)it.sh.m)); ++n_small; }
    }
    double *dIn = nullptr, *dWs = nullptr, *dOut = nullptr, *dDare = nullptr;
    int* dInt = nullptr;  // per unit: Riccati status | Riccati steps | status | Smith squarings
    MpcBuildRec* dTab = nullptr;
    DareRec* dDareTab = nullptr;
    if (in.doubles()) NK_TRY(stage_pack(ctx, in, &dIn));
    NK_TRY(arena_alloc_t(ctx, ws.doubles(), &dWs));
    NK_TRY(arena_alloc_t(ctx, out.doubles(), &dOut));
    NK_TRY(arena_alloc_t(ctx, 4 * cnt, &dInt));
    NK_TRY(arena_alloc_t(ctx, cnt, &dTab));
    if (n_small) {
      NK_TRY(arena_alloc_t(ctx, dare_doubles, &dDare));
      NK_TRY(arena_alloc_t(ctx, n_small, &dDareTab));
    }
    NK_HIP(hipMemsetAsync(dInt, 0, 4 * cnt * sizeof(int), ctx->stream));

    std::vector<MpcBuildRec> recs(cnt);
    std::vector<DareRec> drecs;
    std::vector<int> large_iters(cnt, 0);
    size_t oD = 0;
    for (size_t u = b; u < e; ++u) {
      const BuildItem& it = items[u];
      const MpcBuildOffsets& o = off[u - b];
      const MpcBuildShape& s = it.sh;
      MpcBuildRec& r = recs[u - b];
      r = MpcBuildRec{};
      r.m = (int)s.m; r.p = (int)s.p; r.N = (int)s.N; r.nc = (int)s.nc; r.Ny = s.nc ? (int)s.Ny : 0; r.d = it.d; r.c = it.c;
      r.M = (int)mpc_build_pad(s.m); r.NVP = (int)mpc_build_pad(s.N * s.p);
      if (s.host_ops) {
        r.A = dIn + o.A; r.lda = (int64_t)s.m; r.B = dIn + o.B; r.ldb = (int64_t)s.p; r.Q = dIn + o.Q; r.ldq = (int64_t)s.m;
      } else {
        r.A = it.dA; r.B = it.dB; r.lda = r.ldb = (int64_t)(s.m + s.p); r.C = it.dC; r.ldc = (int64_t)s.m;
      }
      if (s.have_R) r.R = dIn + o.R;
      if (s.nc) {
        if (s.host_C) { r.Crows = dIn + o.C; r.ldcr = (int64_t)s.m; } else { r.Crows = it.dC; r.ldcr = (int64_t)s.m; }
        for (int c = 0; c < MPC_BUILD_MAX_NC; ++c) r.comps[c] = it.comps[c];
      }
      r.sq = dWs + o.sq; r.wide = dWs + o.wide;
      r.outH = dOut + o.H; r.outF = dOut + o.F; r.outK = dOut + o.K;
      if (s.want_P) r.outP = dOut + o.outP;
      if (s.nc) { r.outG = dOut + o.G; r.outT = dOut + o.T; }
      r.status = dInt + 2 * cnt + (u - b);
      r.iters = dInt + 3 * cnt + (u - b);
      r.newton_steps = sa.newton_steps;
      if (s.have_P) {
        r.Pin = dIn + o.P;
      } else {
        r.Pin = dWs + o.rP; r.Kin = dWs + o.rK;
        if (riccati_small(it)) {
          DareRec dr{};
          dr.m = r.m; dr.p = r.p; dr.M = dare_pad(r.m); dr.d = it.d; dr.c = it.c;
          dr.A = r.A; dr.lda = r.lda; dr.B = r.B; dr.ldb = r.ldb; dr.Q = r.Q; dr.ldq = r.ldq; dr.C = r.C; dr.ldc = r.ldc;
          dr.R = r.R;
          dr.ws = dDare + oD; oD += dare_ws_doubles(dr.M);
          dr.outK = dWs + o.rK; dr.outP = dWs + o.rP;
          dr.status = dInt + (u - b); dr.iters = dInt + cnt + (u - b);
          drecs.push_back(dr);
          r.pre_status = dInt + (u - b);
        }
      }
    }
    NK_HIP(hipEventRecord(evs.ev[0], ctx->stream));
    if (n_small) {
      NK_HIP(hipMemcpyAsync(dDareTab, drecs.data(), n_small * sizeof(DareRec), hipMemcpyHostToDevice, ctx->stream));
      NK_TRY(launch_dare(ctx, dDareTab, (int)n_small, sa.tol, sa.max_iter));
    }
    for (size_t u = b; u < e; ++u) {  // the larger problems, one after the other on the same stream
      const BuildItem& it = items[u];
      if (it.sh.have_P || riccati_small(it)) continue;
      MpcBuildRec& r = recs[u - b];
      const MpcBuildOffsets& o = off[u - b];
      DareLargeArgs a;
      a.m = r.m; a.p = r.p; a.d = it.d; a.tol = sa.tol; a.max_iter = sa.max_iter;
      a.A = r.A; a.lda = r.lda; a.B = r.B; a.ldb = r.ldb; a.Q = r.Q; a.ldq = r.ldq; a.C = r.C; a.ldc = r.ldc; a.c = it.c;
      a.R = r.R; a.ldr = r.p;
      a.outK = dWs + o.rK; a.ldk = r.m; a.outP = dWs + o.rP; a.ldp = r.m;
      DareLargeResult res;
      NK_TRY(launch_dare_large(ctx, a, &res));
      r.pre_status_imm = res.status;
      large_iters[u - b] = res.iters;
    }
    NK_HIP(hipMemcpyAsync(dTab, recs.data(), cnt * sizeof(MpcBuildRec), hipMemcpyHostToDevice, ctx->stream));
    NK_HIP(hipEventRecord(evs.ev[1], ctx->stream));
    NK_TRY(launch_mpc_build(ctx, dTab, (int)cnt, sa.newton_tol, sa.newton_max_iter));
    NK_HIP(hipEventRecord(evs.ev[2], ctx->stream));
    std::vector<double> hOut(out.doubles());
    std::vector<int> hInt(4 * cnt);
    NK_HIP(hipMemcpyAsync(hOut.data(), dOut, hOut.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemcpyAsync(hInt.data(), dInt, 4 * cnt * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    float ms_r = 0.0f, ms_b = 0.0f;
    NK_HIP(hipEventElapsedTime(&ms_r, evs.ev[0], evs.ev[1]));
    NK_HIP(hipEventElapsedTime(&ms_b, evs.ev[1], evs.ev[2]));
    g_times.ms_riccati += ms_r; g_times.ms_build += ms_b; ++g_times.groups;
    for (size_t u = b; u < e; ++u) {
      const BuildItem& it = items[u];
      const MpcBuildOffsets& o = off[u - b];
      const MpcBuildShape& s = it.sh;
      const size_t nv = s.N * s.p, ny = s.nc ? s.Ny * s.nc : 0;
      auto give = [&hOut](double* dst, size_t at, size_t count) {
        if (dst) std::copy(hOut.data() + at, hOut.data() + at + count, dst);
      };
      give(it.oH, o.H, nv * nv);
      give(it.oF, o.F, nv * s.m);
      give(it.oK, o.K, s.p * s.m);
      if (s.want_P) give(it.oP, o.outP, s.m * s.m);
      if (ny) { give(it.oG, o.G, ny * nv); give(it.oT, o.T, ny * s.m); }
      out_status[u] = hInt[2 * cnt + (u - b)];
      if (out_iters) {
        out_iters[2 * u] = riccati_small(it) ? hInt[cnt + (u - b)] : large_iters[u - b];
        out_iters[2 * u + 1] = hInt[3 * cnt + (u - b)];
      }
    }
  }
  return NK_OK;
}

int check_solver(nk_ctx* ctx, const char* who, double tol, int32_t max_iter, int32_t newton_steps, double newton_tol,
                 int32_t newton_max_iter) {
  NK_REQUIRE(!ctx_recording(ctx), "%s: not available to the members of a lock-step group", who);
  NK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "%s: tol must be finite and non-negative", who);
  NK_REQUIRE(max_iter >= 1 && max_iter <= 1000, "%s: max_iter = %d must lie in 1 .. 1000", who, max_iter);
  NK_REQUIRE(newton_steps >= 0 && newton_steps <= 4, "%s: newton_steps = %d must lie in 0 .. 4", who, newton_steps);
  NK_REQUIRE(std::isfinite(newton_tol) && newton_tol >= 0.0, "%s: newton_tol must be finite and non-negative", who);
  NK_REQUIRE(newton_max_iter >= 1 && newton_max_iter <= 1000, "%s: newton_max_iter = %d must lie in 1 .. 1000", who,
             newton_max_iter);
  return NK_OK;
}

int check_horizon(const char* who, int u, int p, int N, int nc, int Ny) {
  NK_REQUIRE(N >= 1, "%s: problem %d: N = %d must be at least 1", who, u, N);
  NK_REQUIRE((int64_t)N * p <= NK_MPC_MAX_NV, "%s: problem %d: nv = N p = %lld must not exceed %d", who, u,
             (long long)N * p, NK_MPC_MAX_NV);
  NK_REQUIRE(nc >= 0 && nc <= MPC_BUILD_MAX_NC, "%s: problem %d: nc = %d must lie in 0 .. %d", who, u, nc, MPC_BUILD_MAX_NC);
  NK_REQUIRE(nc == 0 || (Ny >= 1 && Ny <= N), "%s: problem %d: Ny = %d must lie in 1 .. N = %d", who, u, Ny, N);
  return NK_OK;
}

}  // namespace

extern "C" {

int nk_mpc_build_batch(nk_ctx* ctx, const nk_mpc_build_problem* problems, int32_t n, double tol, int32_t max_iter,
                       int32_t newton_steps, double newton_tol, int32_t newton_max_iter, int32_t* out_status,
                       int32_t* out_iters) {
  static const char* who = "nk_mpc_build_batch";
  NK_TRY(check_ctx(ctx));
  NK_TRY(check_solver(ctx, who, tol, max_iter, newton_steps, newton_tol, newton_max_iter));
  NK_REQUIRE(problems != nullptr && n >= 1, "%s: n = %d problems at %p: at least one is needed", who, n, (const void*)problems);
  NK_REQUIRE(out_status != nullptr, "%s: out_status is null", who);
  std::vector<BuildItem> items((size_t)n);
  for (int u = 0; u < n; ++u) {  // everything is checked before anything is queued or allocated
    const nk_mpc_build_problem& pr = problems[u];
    NK_REQUIRE(pr.m >= 1 && pr.m <= MPC_BUILD_MAX_M, "%s: problem %d: m = %d must lie in 1 .. %d", who, u, pr.m, MPC_BUILD_MAX_M);
    NK_REQUIRE(pr.p >= 1 && pr.p <= MPC_BUILD_MAX_P, "%s: problem %d: p = %d must lie in 1 .. %d", who, u, pr.p, MPC_BUILD_MAX_P);
    NK_TRY(check_horizon(who, u, pr.p, pr.N, pr.nc, pr.Ny));
    const int ny = pr.nc * pr.Ny;
    struct Ptr { const char* name; const void* p; bool needed; };
    const Ptr ptrs[] = {{"A", pr.A, true}, {"B", pr.B, true}, {"Q", pr.Q, true}, {"R", pr.R, true}, {"P", pr.P, false},
                        {"C_rows", pr.C_rows, pr.nc > 0}, {"out_H", pr.out_H, true}, {"out_F", pr.out_F, true},
                        {"out_K", pr.out_K, true}, {"out_P", pr.out_P, false}, {"out_G", pr.out_G, ny > 0},
                        {"out_T", pr.out_T, ny > 0}};
    for (const Ptr& q : ptrs) {
      NK_REQUIRE(q.p != nullptr || !q.needed, "%s: problem %d: %s is null", who, u, q.name);
      NK_REQUIRE(!is_device_ptr(q.p), "%s: problem %d: %s must be host memory", who, u, q.name);
    }
    NK_REQUIRE(pr.lda >= pr.m, "%s: problem %d: lda = %lld is smaller than m", who, u, (long long)pr.lda);
    NK_REQUIRE(pr.ldb >= pr.p, "%s: problem %d: ldb = %lld is smaller than p", who, u, (long long)pr.ldb);
    NK_REQUIRE(pr.ldq >= pr.m, "%s: problem %d: ldq = %lld is smaller than m", who, u, (long long)pr.ldq);
    NK_REQUIRE(pr.ldr >= pr.p, "%s: problem %d: ldr = %lld is smaller than p", who, u, (long long)pr.ldr);
    NK_REQUIRE(pr.P == nullptr || pr.ldp >= pr.m, "%s: problem %d: ldp = %lld is smaller than m", who, u, (long long)pr.ldp);
    NK_REQUIRE(pr.nc == 0 || pr.ldc >= pr.m, "%s: problem %d: ldc = %lld is smaller than m", who, u, (long long)pr.ldc);
    BuildItem& it = items[u];
    it.sh.m = pr.m; it.sh.p = pr.p; it.sh.N = pr.N; it.sh.nc = pr.nc; it.sh.Ny = pr.nc ? pr.Ny : 0;
    it.sh.host_ops = true; it.sh.have_R = true; it.sh.have_P = pr.P != nullptr; it.sh.want_P = pr.out_P != nullptr;
    it.sh.host_C = pr.nc > 0;
    it.hA = pr.A; it.lda = pr.lda; it.hB = pr.B; it.ldb = pr.ldb; it.hQ = pr.Q; it.ldq = pr.ldq; it.hR = pr.R; it.ldr = pr.ldr;
    it.hP = pr.P; it.ldp = pr.ldp; it.hC = pr.nc ? pr.C_rows : nullptr; it.ldc = pr.ldc;
    it.oH = pr.out_H; it.oF = pr.out_F; it.oK = pr.out_K; it.oP = pr.out_P; it.oG = pr.out_G; it.oT = pr.out_T;
  }
  return mpc_build_run(ctx, items, SolverArgs{tol, newton_tol, max_iter, newton_steps, newton_max_iter}, out_status, out_iters);
}

int nk_model_mpc_build_batch(nk_ctx* ctx, const nk_model* const* models, int32_t n, double c, const double* R,
                             const nk_mpc_build_spec* specs, double tol, int32_t max_iter, int32_t newton_steps,
                             double newton_tol, int32_t newton_max_iter, const nk_mpc_build_out* outs, int32_t* out_status,
                             int32_t* out_iters) {
  static const char* who = "nk_model_mpc_build_batch";
  NK_TRY(check_ctx(ctx));
  NK_TRY(check_solver(ctx, who, tol, max_iter, newton_steps, newton_tol, newton_max_iter));
  NK_REQUIRE(models != nullptr && n >= 1, "%s: n = %d models at %p: at least one is needed", who, n, (const void*)models);
  NK_REQUIRE(specs != nullptr && outs != nullptr && out_status != nullptr, "%s: specs, outs or out_status is null", who);
  NK_REQUIRE(std::isfinite(c) && c >= 0.0, "%s: c must be finite and non-negative", who);
  NK_REQUIRE(!is_device_ptr(R), "%s: R must be host memory", who);
  std::vector<BuildItem> items((size_t)n);
  for (int u = 0; u < n; ++u) {
    const nk_model* mdl = models[u];
    const nk_mpc_build_spec& sp = specs[u];
    const nk_mpc_build_out& o = outs[u];
    NK_REQUIRE(mdl != nullptr, "%s: model %d is null", who, u);
    NK_REQUIRE(mdl->device == ctx->device, "%s: model %d lives on device %d, the context on %d", who, u, mdl->device,
               ctx->device);
    NK_REQUIRE(mdl->has_ops, "%s: model %d has no fitted operators", who, u);
    NK_REQUIRE(mdl->m >= 1 && mdl->m <= MPC_BUILD_MAX_M, "%s: model %d: m = %d must lie in 1 .. %d", who, u, mdl->m,
               MPC_BUILD_MAX_M);
    NK_REQUIRE(mdl->p >= 1 && mdl->p <= MPC_BUILD_MAX_P, "%s: model %d: p = %d must lie in 1 .. %d", who, u, mdl->p,
               MPC_BUILD_MAX_P);
    NK_REQUIRE(R == nullptr || mdl->p == models[0]->p, "%s: model %d has %d inputs, R is %d x %d", who, u, mdl->p,
               models[0]->p, models[0]->p);
    NK_TRY(check_horizon(who, u, mdl->p, sp.N, sp.nc, sp.Ny));
    for (int k = 0; k < sp.nc; ++k)
      NK_REQUIRE(sp.comps[k] >= 0 && sp.comps[k] < mdl->d, "%s: unit %d: comps[%d] = %d must lie in 0 .. d - 1 = %d", who, u,
                 k, sp.comps[k], mdl->d - 1);
    NK_REQUIRE(o.H && o.F && o.K, "%s: unit %d: H, F or K of outs is null", who, u);
    NK_REQUIRE(sp.nc == 0 || (o.G && o.T), "%s: unit %d: G or T of outs is null", who, u);
    NK_REQUIRE(!is_device_ptr(o.H) && !is_device_ptr(o.F) && !is_device_ptr(o.K) && !is_device_ptr(o.G) && !is_device_ptr(o.T),
               "%s: unit %d: the results must be host memory", who, u);
    BuildItem& it = items[u];
    it.sh.m = mdl->m; it.sh.p = mdl->p; it.sh.N = sp.N; it.sh.nc = sp.nc; it.sh.Ny = sp.nc ? sp.Ny : 0;
    it.sh.have_R = R != nullptr;
    it.d = mdl->d; it.c = c;
    it.dA = mdl->A; it.dB = mdl->B; it.dC = mdl->C;
    it.hR = R; it.ldr = mdl->p;
    for (int k = 0; k < MPC_BUILD_MAX_NC; ++k) it.comps[k] = k < sp.nc ? sp.comps[k] : 0;
    it.oH = o.H; it.oF = o.F; it.oK = o.K; it.oG = o.G; it.oT = o.T;
  }
  return mpc_build_run(ctx, items, SolverArgs{tol, newton_tol, max_iter, newton_steps, newton_max_iter}, out_status, out_iters);
}

int nk_mpc_build_times(double out[3]) {
  NK_REQUIRE(out != nullptr, "nk_mpc_build_times: out is null");
  out[0] = g_times.ms_riccati; out[1] = g_times.ms_build; out[2] = (double)g_times.groups;
  return NK_OK;
}

}  // extern "C"
