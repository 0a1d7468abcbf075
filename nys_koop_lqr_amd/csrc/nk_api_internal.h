// Helpers shared by the translation units behind the C ABI (nk_api.hip, nk_fit.hip, nk_sweep.hip, nk_control.hip);
// defined in nk_api.hip unless noted.
#pragma once
#include "nk_common.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace nk {

// ---- staging: device view of a caller matrix (rows x cols, leading dimension ld); host data is copied into the arena
struct MatIn {
  const double* ptr = nullptr;
  int64_t ld = 0;
  bool staged = false;
};
int stage_in(nk_ctx* ctx, const double* p, int64_t ld, int64_t rows, int64_t cols, MatIn* out);
struct MatOut {
  double* dev = nullptr;
  int64_t ld = 0;
  double* host = nullptr;
  int64_t host_ld = 0;
  int64_t rows = 0, cols = 0;
};
int stage_out(nk_ctx* ctx, double* p, int64_t ld, int64_t rows, int64_t cols, MatOut* out);
int finish_out(nk_ctx* ctx, const MatOut& o);

int check_ctx(nk_ctx* ctx);
// 1/lengthscale per dimension on the device (ones for the linear kernel and the thin-plate spline)
int make_winv(nk_ctx* ctx, const nk_kernel_desc* kd, int d, double* dst_dev);
int model_alloc(nk_ctx* ctx, int m, int d, int p, nk_model** out, int kind = NK_MODEL_NYSTROM);

// phi (nq x m, ld ldo) = k(Xq, Z) * Sinv, processed in row chunks; a spline model's lift is the raw block k(Xq, Z)
int lift_device(nk_ctx* ctx, const nk_model* mdl, const double* Xq, int64_t ldx, int64_t nq, double* out, int64_t ldo);
// out (nq x d) = [phi(X) | U] W^T
int predict_device(nk_ctx* ctx, const nk_model* mdl, const double* Xaug, int64_t ldx, int64_t nq, double* out, int64_t ldo);

// NYSKOOP_TRACE=1: host-side wall clock of the fit's phases on stderr (diagnostics)
struct HostTrace {
  bool on;
  std::chrono::steady_clock::time_point t0, last;
  HostTrace() : on(getenv("NYSKOOP_TRACE") != nullptr) { t0 = last = std::chrono::steady_clock::now(); }
  void mark(const char* what) {
    if (!on) return;
    auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[nk trace] %-28s +%8.3f ms (total %8.3f)\n", what,
            std::chrono::duration<double, std::milli>(now - last).count(),
            std::chrono::duration<double, std::milli>(now - t0).count());
    last = now;
  }
};
float ev_ms(nk_ctx* ctx, int a, int b);  // a, b: EV_* slots

// ---- small-call staging: the latency-bound entry points (rollouts, closed loops) read their host inputs from, and write
//      their host outputs into, one page-locked block that the GPU addresses directly -- no DMA descriptors, no staging
//      copies on the stream; the host moves the bytes with memcpy before the launch and after the one synchronisation.
struct SmallStage {
  nk_ctx* ctx = nullptr;
  size_t off = 0;
  struct Out { double* stage; double* user; int64_t user_ld; int64_t rows, cols; };
  std::vector<Out> outs;
};
constexpr size_t SMALL_STAGE_LIMIT = (size_t)4 << 20;
int small_reserve(nk_ctx* ctx, size_t bytes);
const double* small_in(SmallStage& st, const double* host, int64_t ld, int64_t rows, int64_t cols);
double* small_out(SmallStage& st, double* user, int64_t user_ld, int64_t rows, int64_t cols);
void small_finish(SmallStage& st);  // after the stream has been synchronised
inline size_t pad256(size_t doubles) { return ((doubles * 8) + 255) & ~(size_t)255; }

// the body of nk_rollout_err for a context whose arena the caller has prepared (check_ctx): the sweep gathers a unit's
// trajectories into the arena first (nk_control.hip)
int rollout_err_run(nk_ctx* ctx, const nk_model* mdl, const double* traj, const double* U, int32_t T, int32_t batch,
                    double* err_abs, double* err_rel);

}  // namespace nk
