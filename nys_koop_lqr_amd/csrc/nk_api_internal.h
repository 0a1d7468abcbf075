// Helpers shared by the translation units behind the C ABI (nk_api.hip, nk_api_compute.hip, nk_fit.hip, nk_sweep.hip,
// nk_control.hip, nk_api_loops.hip, nk_api_dare.hip, nk_api_mpc_build.hip); defined in nk_api.hip unless noted.
#pragma once
#include "nk_common.h"
#include "nk_unit_pack.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace nk {

// ---- staging: device view of a caller matrix (rows x cols, leading dimension ld); host data is copied into the arena
struct MatIn {
  const double* ptr = nullptr;
  int64_t ld = 0;
  bool staged = false;
  int64_t rows = 0, cols = 0;
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
// (this and predict_device: nk_api_compute.hip)
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

// ---- call staging of the latency-bound entry points (lift, predict, rollouts, closed loops): the entry point declares
//      its operands once, commit() picks one of two transports and fills the views, and one body works on them.
//      Page-locked transport -- chosen exactly when the 256-byte-padded operands together fit SMALL_STAGE_LIMIT and no
//      declared pointer is device memory: operands live in one page-locked block that the GPU addresses directly, with
//      tight leading dimensions -- no DMA descriptors, no staging copies on the stream; the host moves the bytes with
//      memcpy before the launch and after the one synchronisation.  Arena transport otherwise: stage_in / stage_out.
constexpr size_t SMALL_STAGE_LIMIT = (size_t)4 << 20;
inline size_t pad256(size_t doubles) { return ((doubles * 8) + 255) & ~(size_t)255; }
class CallStage {
 public:
  explicit CallStage(nk_ctx* c) : ctx(c) {}
  // declare an operand (recorded only; the views are valid after commit); a null output is skipped
  void in(MatIn* view, const double* p, int64_t ld, int64_t rows, int64_t cols) { ops.push_back({view, nullptr, p, ld, rows, cols}); }
  void out(MatOut* view, double* p, int64_t ld, int64_t rows, int64_t cols) { if (p) ops.push_back({nullptr, view, p, ld, rows, cols}); }
  int commit();
  // an input that every wave reads: when it lies in the page-locked block it is copied into the arena (leading dimension
  // ld) and the view moved there -- from HBM, not an uncached PCIe read per wave; on the arena transport nothing happens
  int resident(MatIn* view, int64_t ld);
  int queue_outputs();  // arena transport: the device-to-host copies, once per attempt; before the synchronisation
  void deliver();       // page-locked transport: the memcpy back to the caller; once, after the synchronisation
 private:
  struct Operand { MatIn* in; MatOut* out; const double* ptr; int64_t ld, rows, cols; };
  nk_ctx* ctx;
  bool pinned = false;
  std::vector<Operand> ops;
};

// the staging block of a unit-table call (nk_unit_pack.h) in the arena: its one host-to-device copy.  The pack must outlive
// the synchronisation that ends the call: the copy reads its block.
int stage_pack(nk_ctx* ctx, UnitPack& pack, double** dev);

// the body of nk_rollout_err for a context whose arena the caller has prepared (check_ctx): the sweep gathers a unit's
// trajectories into the arena first (nk_control.hip)
int rollout_err_run(nk_ctx* ctx, const nk_model* mdl, const double* traj, const double* U, int32_t T, int32_t batch,
                    double* err_abs, double* err_rel);

}  // namespace nk
