// Internal declarations shared by the libnyskoop translation units (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "nyskoop.h"
#include "nk_lockstep.h"
#include "nk_gemm_plan.h"
#include "nk_chain_plan.h"

namespace nk {

void set_error(const char* fmt, ...);

#define NK_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      nk::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return e_ == hipErrorOutOfMemory ? NK_ERR_OOM : NK_ERR_HIP;                            \
    }                                                                                        \
  } while (0)

#define NK_TRY(call)            \
  do {                          \
    int rc_ = (call);           \
    if (rc_ != NK_OK) return rc_; \
  } while (0)

#define NK_REQUIRE(cond, ...)     \
  do {                            \
    if (!(cond)) {                \
      nk::set_error(__VA_ARGS__); \
      return NK_ERR_BAD_ARG;      \
    }                             \
  } while (0)

// Grow-only HBM workspace: a list of chunks with bump pointers, reset at the start of every API call (and then
// coalesced into one chunk, so the steady state performs no hipMalloc).  All work of a context is on one stream,
// so releasing back to a mark makes the space reusable by later launches in stream order.
struct ArenaChunk {
  char* base = nullptr;
  size_t cap = 0;
  size_t off = 0;
};
struct Arena {
  std::vector<ArenaChunk> chunks;
  int cur = 0;
};
struct ArenaMark {
  int chunk;
  size_t off;
};

}  // namespace nk

// Slots of nk_ctx::ev (timing enabled).  Who records / who waits or reads:
enum {
  EV_FIT_BEGIN = 0,      // a fit's entry, main stream / the fit's statistics
  EV_STAGED = 1,         // inputs and landmarks staged, main stream / the fit's statistics
  EV_KMAT_DONE = 2,      // kernel blocks of the first pass queued (FIT_SOLVE: accumulators loaded), main / statistics
  EV_GRAM_DONE = 3,      // last Gram contraction, main stream / the fit's statistics
  EV_SOLVE_BEGIN = 4,    // main stream after it joined the side stream (spline fit: before the operators) / statistics
  EV_FIT_END = 5,        // operator products, main stream / the fit's statistics
  EV_SQRT_BEGIN = 6,     // side stream in front of the square-root iteration / statistics
  EV_SQRT_END = 7,       // side stream behind the square-root iteration / statistics
  EV_LANDMARKS = 8,      // landmark matrices built (main or preparation stream) / the preparation stream, and the main
                         // stream where it assembles the systems
  EV_SQRT_PREPARED = 9,  // sqrtm_prepare's chain, preparation stream / the side stream in front of the iteration, and the
                         // main stream in front of a fit's first Gram launch when the chain was queued ahead of it
  EV_SQRT_RESID = 10,    // residual copy of the host-checked square-root iteration (nk_sqrtm.hip) / the host, same place
  EV_SQRT_SCALARS = 11,  // sqrtm_prepare's schedule scalars on their way to the host / the host in sqrtm_finish
  EV_FORK = 12,          // scratch fork point, recorded on the main stream and waited for at once by the stream that
                         // branches off: the landmark matrices aside, the pipelined upload, the Y rows' preparation
  EV_YPREP_DONE = 13,    // Y rows prepared on the side stream (overlap_prep) / the main stream before their kernel block
  EV_GEMM_T0 = 14,       // recorded by the GEMM engines (nk_gemm*.hip) around a timed launch; read there, or by the
  EV_GEMM_T1 = 15,       // fits after their own synchronisation when the launch was timed without one (sync_timing = false)
  EV_COUNT = 16
};

// Regions of nk_ctx::h_scalars, the pinned host mirror of small device results.  Who writes (by a copy queued on its
// stream) / who reads.  Two owners may be in flight on different streams during a fit, so the regions do not overlap.
enum {
  HS_SCRATCH = 0,             // [0..3] read back right behind a synchronisation of the writer's own stream: the synchronous
                              // form of the square root (c, ||P||_F^2, trace, ||L^-1||_F^2 in SqrtPlan::d_sc's order), its
                              // residuals, the coupled iteration, the pseudo-inverse (nk_pinv.hip) / the same function
  HS_SQRT_FLAG = 8,           // verdict of the queued square-root iteration, sqrtm_finish (in a fit: side stream) / sqrtm_verdict:
  HS_SQRT_RESID_AT_FLAG = 9,  //   step + 1 of the first step below the residual bar (0: none), the residual there,
  HS_SQRT_RESID_LAST = 10,    //   the last residual seen
  HS_SQRT_C = 12,             // schedule scalars of the square root, sqrtm_prepare (in a fit: preparation stream) /
  HS_SQRT_SUMSQ = 13,         //   the early form of sqrtm_finish behind EV_SQRT_SCALARS: ||P||_inf, ||P||_F^2,
  HS_SQRT_TRACE = 14,         //   trace(P)
  HS_REFINE = 16,             // [16..23] refinement verdicts, four per system, nk_fit.hip (main stream) / read_refinement
  HS_COUNT = 64               // length of h_scalars (and of d_scalars)
};
// Device scalars of SqrtPlan::d_sc.  sqrtm_prepare writes the first four, the queued iteration of sqrtm_finish the state.
enum {
  SQ_C = 0,              // c = ||P||_inf
  SQ_SUMSQ = 1,          // ||P||_F^2
  SQ_TRACE = 2,          // trace(P)
  SQ_LINV2 = 3,          // ||L^-1||_F^2
  SQ_FLAG = 5,           // iteration state (ns_flag_kernel): step + 1 of the first step below the residual bar (0: not yet),
  SQ_RESID_AT_FLAG = 6,  //   the residual at that step,
  SQ_RESID_LAST = 7,     //   the last residual seen
  SQ_COUNT = 8
};

struct nk_member_state;
struct nk_ctx {
  int device = 0;
  hipStream_t stream = nullptr;       // CURRENT stream: every launcher uses this (swapped by nk::SideScope)
  hipStream_t stream_main = nullptr;
  hipStream_t stream_side = nullptr;  // second stream (lowest priority) for GEMM-bound work beside the main chain
  hipStream_t stream_copy = nullptr;  // device->host copies of nk_model_get_ops_async (overlap with the next call's kernels)
  hipStream_t stream_prep = nullptr;  // third stream (highest priority) for small latency-bound work queued early: its
                                      // kernels must get CU slots while a big main-stream launch still has workgroups
                                      // pending (the dispatcher serves queues in strict priority order)
  nk::Arena arena;                    // workspace of the main stream
  nk::Arena arena_side;               // workspace of the side stream (slabs must not be shared across streams)
  nk::Arena* cur_arena = nullptr;
  hipStream_t stream_la[2] = {nullptr, nullptr};  // look-ahead streams of the blocked Cholesky: [0] beside the prep stream
                                                  // (highest priority), [1] beside the main stream (middle)
  hipEvent_t ev_la[2][4] = {};                    // per look-ahead stream: panel-done / rest-done events, two of each (ring)
  int compute_f32 = 0;                            // 1: kernel blocks and Gram contractions of a fit on the fp32 engine
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_chain = nullptr;
  int* d_info = nullptr;       // device flags for factorisation failures (one int per paired system)
  unsigned long long* d_piv = nullptr;  // [min, max] Cholesky pivot per system slot (bit patterns), behind d_info's 4 slots
  unsigned long long* h_piv = nullptr;  // pinned host mirror
  double* d_scalars = nullptr; // small device scratch for reductions (HS_COUNT doubles)
  double* h_scalars = nullptr; // pinned host mirror, HS_COUNT doubles in the HS_* regions above
  int* h_info = nullptr;       // pinned host mirror of d_info (kept apart from h_scalars: both streams may be in flight)
  double* d_zeros = nullptr;   // 4 KiB zero page (K-tail rows of the LDS-DMA GEMM)
  hipEvent_t ev[EV_COUNT];  // indexed by the EV_* slots above
  int num_cu = 256;
  int kmat_mode = 0;  // 0 auto (Gram form on MFMA for d >= 32), 1 always direct differences (NYSKOOP_KMAT=direct)
  // optional refinement of the two regularised solves with doubled-precision residuals (nk_set_refine): applied to a system
  // whose smallest / largest Cholesky pivot is below refine_pivot (0 = never, the default), refine_steps steps
  double refine_pivot = 0.0;
  int refine_steps = 2;
  int strict_spd = 0; // 1: a non-positive Cholesky pivot is an error (NK_ERR_NOT_SPD) instead of entering the
                      // rank-truncating pseudo-inverse path (NYSKOOP_STRICT_SPD=1 / nk_set_strict_spd)
  hipEvent_t ev_ext = nullptr;  // ordering against a caller's stream (nk_wait_stream)
  hipEvent_t ev_up[8] = {};     // uploads of the row blocks of a fit from host arrays (pipelined with the passes)
  nk_group* group = nullptr;    // member of a lock-step group (nk_lockstep.h): stream operations are recorded and merged
  nk_member_state* gstate = nullptr;
  int* d_flow[2] = {nullptr, nullptr};  // flag words of the dataflow Cholesky (nk_chol_flow.hip), per failure-flag slot
  size_t flow_words[2] = {0, 0};
  bool spline_defer_svd = false;  // first phase of nk_spline_cv_grid: nk_spline_fit stops (NK_ERR_NOT_SPD) where it would
                                 // enter the pseudo-inverse, so that such units can be run together afterwards
  bool chol_flow_off = false;  // set by nk::ChainOnly: the re-run of a factorisation whose dataflow launch gave up
  int chol_flow_wgs = 0;       // set by nk::FlowWidth: workgroups of a dataflow Cholesky launch (0: half the CUs)
  double* h_stage = nullptr;    // page-locked, device-visible staging block for the small latency-bound calls (rollouts):
  size_t h_stage_bytes = 0;     // kernels read their inputs from it and write their results into it directly (no DMA)
};

enum { NK_MODEL_NYSTROM = 0, NK_MODEL_SPLINE = 1 };
struct nk_model {
  int device = 0;
  int32_t m = 0, d = 0, p = 0;
  int32_t ktype = 0;
  double sigma0 = 0.0;
  double jitter = 0.0;
  double* buf = nullptr;  // one allocation holding everything below
  size_t bytes = 0;
  double *A = nullptr, *B = nullptr, *C = nullptr, *W = nullptr, *S = nullptr, *Sinv = nullptr, *Z = nullptr,
         *winv = nullptr;  // winv: 1/lengthscale per dimension (d entries)
  bool has_ops = false;
  int32_t kind = 0;  // NK_MODEL_NYSTROM / NK_MODEL_SPLINE (lift = raw thin-plate-spline block, no S, Sinv: both nullptr)
  hipEvent_t ev_fetch = nullptr;  // completion of the last nk_model_get_ops_async (nullptr: nothing pending)
};

namespace nk {

// Route launches and workspace allocations to the side stream (or the given one; the side arena is shared, so work on the
// two auxiliary streams must be ordered by events) for the lifetime of the scope.
struct SideScope {
  nk_ctx* c;
  hipStream_t s0;
  Arena* a0;
  explicit SideScope(nk_ctx* ctx, hipStream_t s = nullptr) : c(ctx), s0(ctx->stream), a0(ctx->cur_arena) {
    c->stream = s ? s : c->stream_side;
    c->cur_arena = &c->arena_side;
  }
  ~SideScope() {
    c->stream = s0;
    c->cur_arena = a0;
  }
};

// For the lifetime of the scope every blocked Cholesky of the context runs as the launch-per-step chain.
struct ChainOnly {
  nk_ctx* c;
  bool b0;
  explicit ChainOnly(nk_ctx* ctx) : c(ctx), b0(ctx->chol_flow_off) { c->chol_flow_off = true; }
  ~ChainOnly() { c->chol_flow_off = b0; }
};

// For the lifetime of the scope a dataflow Cholesky launch of the context takes `wgs` workgroups (0: the default).  The
// result does not depend on it: every tile is the same arithmetic whichever workgroup draws it.
struct FlowWidth {
  nk_ctx* c;
  int w0;
  FlowWidth(nk_ctx* ctx, int wgs) : c(ctx), w0(ctx->chol_flow_wgs) { c->chol_flow_wgs = wgs; }
  ~FlowWidth() { c->chol_flow_wgs = w0; }
};

// factorisation failure flags: slots 0-1 belong to the main stream, 2-3 to the side stream (each stream may have a paired
// factorisation in flight)
inline int info_base(const nk_ctx* c) { return c->stream != c->stream_main ? 2 : 0; }

// the highest coefficient of exp_nonpos (0x3e5ade156a5dcb37) held in a vector register pair the compiler cannot re-materialise
__device__ __forceinline__ double exp_nonpos_ca() {
  double ca = __longlong_as_double(0x3e5ade156a5dcb37LL);
  asm volatile("" : "+v"(ca));
  return ca;
}
// exp(x) for x <= 0, the arithmetic of the device library's exp (same range reduction, same degree-11 Horner form with the same
// coefficients, same operation order: the same bits) -- but with the coefficients as SCALAR operands of the fused multiply-adds.
// The compiler's form keeps the accumulator in the destination (v_fmac_f64) and re-materialises every coefficient into a
// vector register pair in front of it: 18 v_mov_b32 per value, plus an upper range check that a non-positive argument
// does not need.  In the epilogue of the Gram-form kernel blocks every vector instruction
// takes issue slots from the matrix pipe the other workgroup of the CU is using: 42 -> 21 instructions per exp.
__device__ __forceinline__ double exp_nonpos(double x, double ca_v) {
  const double k = __builtin_rint(x * __longlong_as_double(0x3ff71547652b82feLL));   // log2(e)
  double r = __builtin_fma(__longlong_as_double((long long)0xbfe62e42fefa39efULL), k, x);   // -ln2, high part
  r = __builtin_fma(__longlong_as_double((long long)0xbc7abc9e3b39803fULL), k, r);          // -ln2, low part
  double p;
#define NK_EXP_STEP(c) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(r), "v"(p), "s"(c))
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(r), "v"(ca_v), "s"(__longlong_as_double(0x3e928af3fca7ab0cLL)));
  NK_EXP_STEP(__longlong_as_double(0x3ec71dee623fde64LL));
  NK_EXP_STEP(__longlong_as_double(0x3efa01997c89e6b0LL));
  NK_EXP_STEP(__longlong_as_double(0x3f2a01a014761f6eLL));
  NK_EXP_STEP(__longlong_as_double(0x3f56c16c1852b7b0LL));
  NK_EXP_STEP(__longlong_as_double(0x3f81111111122322LL));
  NK_EXP_STEP(__longlong_as_double(0x3fa55555555502a1LL));
  NK_EXP_STEP(__longlong_as_double(0x3fc5555555555511LL));
  NK_EXP_STEP(__longlong_as_double(0x3fe000000000000bLL));
#undef NK_EXP_STEP
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  // (the library's lower range check, which also keeps a NaN argument a NaN; its upper one cannot fire for x <= 0)
  return x < -1075.0 ? 0.0 : ldexp(p, (int)k);
}
__device__ __forceinline__ double exp_nonpos(double x) { return exp_nonpos(x, exp_nonpos_ca()); }

// log(x) for finite x > 0 (the thin-plate-spline epilogues; sqrt(r^2) of two distinct points).  fdlibm's __ieee754_log
// (public domain, Sun Microsystems 1993): x = 2^k (1 + f) with 1 + f in [sqrt(2)/2, sqrt(2)), s = f / (2 + f),
// log(1 + f) = f - hf^2 + s (hf^2 + R(s^2)) with fdlibm's degree-14 minimax R, k ln2 in two parts.  Plain IEEE operations
// (no contraction, correctly rounded division), so the host build of this function gives the same bits as the device.
// Error against the C library's log (glibc), measured on the host build over 2.1e7 arguments (7e6 each: uniform in the
// exponent over [1e-300, 1e300], uniform over [0.5, 2], uniform over [1 - 1e-6, 1 + 1e-6]) and a sweep of subnormals: at
// most 1 ulp, 97.3 % of the results identical.
__host__ __device__ __forceinline__ double log_pos(double x) {
#pragma clang fp contract(off)
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  uint64_t bits;
  __builtin_memcpy(&bits, &x, 8);
  int32_t hx = (int32_t)(bits >> 32);
  int k = 0;
  if (hx < 0x00100000) {  // subnormal: scale up by 2^54
    x *= 1.80143985094819840000e+16;
    k -= 54;
    __builtin_memcpy(&bits, &x, 8);
    hx = (int32_t)(bits >> 32);
  }
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  const int32_t i = (hx + 0x95f64) & 0x100000;
  bits = ((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xffffffffULL);  // x or x/2 normalised
  __builtin_memcpy(&x, &bits, 8);
  k += i >> 20;
  const double f = x - 1.0;
  const double dk = (double)k;
  if ((0x000fffff & (2 + hx)) < 3) {  // |f| < 2^-20
    if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
  }
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  if (((hx - 0x6147a) | (0x6b851 - hx)) > 0) {
    const double hfsq = 0.5 * f * f;
    return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}
// thin-plate spline of a squared distance, r^2 log(sqrt(r^2)) in the reference's order of operations (regressors.py:232);
// exactly 0 at r^2 = 0, where the reference's nan_to_num turns 0 * (-inf) into 0.  r2 >= 0.
__host__ __device__ __forceinline__ double tps_value(double r2) {
#pragma clang fp contract(off)
  return r2 > 0.0 ? r2 * log_pos(sqrt(r2)) : 0.0;
}

// ---- lock-step groups (nk_group.hip) ----------------------------------------------------------------------------
nk_group* group_new(int device, int size);
void group_attach(nk_group* g, int slot, nk_ctx* c);
void group_detach(nk_ctx* c);
int group_enter(nk_ctx* c);
int group_leave(nk_ctx* c);
void group_stats(nk_ctx* c, uint64_t out[4]);
// slow-path counters (nk_runtime_counters)
// CNT_CHOL_FLOW_GIVEUP: dataflow Cholesky launches that gave up waiting (re-run on the launch-per-step chain);
// CNT_CHOL_FLOW: dataflow Cholesky launches issued; CNT_CHOL_LOOKAHEAD: launch-per-step chains that ran with look-ahead
enum { CNT_CHAIN_GIVEUP = 0, CNT_JACOBI_GIVEUP = 1, CNT_RANK_TRUNCATED = 2, CNT_SQRT_RETRY = 3, CNT_REFINED = 4,
       CNT_CHOL_FLOW_GIVEUP = 5, CNT_CHOL_FLOW = 6, CNT_CHOL_LOOKAHEAD = 7, CNT_N = 8 };
void count_event(int which);
uint64_t read_counter(int which);
hipError_t real_stream_sync(hipStream_t s);
hipError_t real_event_sync(hipEvent_t e);

// ---- workspace -------------------------------------------------------------------------------------------
int arena_reset(nk_ctx* ctx);
ArenaMark arena_mark(nk_ctx* ctx);
void arena_release(nk_ctx* ctx, ArenaMark mk);
int arena_alloc(nk_ctx* ctx, size_t bytes, void** out);
template <typename T>
inline int arena_alloc_t(nk_ctx* ctx, size_t count, T** out) {
  return arena_alloc(ctx, count * sizeof(T), reinterpret_cast<void**>(out));
}
bool is_device_ptr(const void* p);

// ---- dynamic-LDS opt-in of a list of kernels.  Use as a function-local static, whose initialisation runs once and is
// safe when several threads make their first launch together:
//   static const hipError_t e = dynamic_lds_register(BYTES, kernel_a, kernel_b<1>, ...);  NK_TRY(dynamic_lds_status(e));
template <typename... Fn>
inline hipError_t dynamic_lds_register(int bytes, Fn*... kernels) {
  hipError_t e = hipSuccess;
  for (const void* f : {reinterpret_cast<const void*>(kernels)...})
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}
inline int dynamic_lds_status(hipError_t e) {  // a failed registration fails every launch that needs it
  if (e == hipSuccess) return NK_OK;
  set_error("hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e));
  return NK_ERR_HIP;
}

// ---- timing bracket of the GEMM engines: begin() and end() record EV_GEMM_T0 / EV_GEMM_T1 around the timed launch when the
// caller gave ms; read(sync) waits for the launch and stores the elapsed time (sync = false: the caller reads the two
// events after its own synchronisation)
struct GemmTimer {
  nk_ctx* ctx;
  float* ms;
  int mark(int slot) const {
    if (ms) NK_HIP(hipEventRecord(ctx->ev[slot], ctx->stream));
    return NK_OK;
  }
  int begin() const { return mark(EV_GEMM_T0); }
  int end() const { return mark(EV_GEMM_T1); }
  int read(bool sync) const {
    if (!ms || !sync) return NK_OK;
    NK_HIP(hipEventSynchronize(ctx->ev[EV_GEMM_T1]));
    NK_HIP(hipEventElapsedTime(ms, ctx->ev[EV_GEMM_T0], ctx->ev[EV_GEMM_T1]));
    return NK_OK;
  }
};

// ---- device launchers (all asynchronous on ctx->stream; device pointers only) ---------------------------------
// kernel matrix out[i][j] = k(A[i,:], B[j,:]); winv = 1/lengthscale (d entries, device)
int launch_kmat(nk_ctx* ctx, int ktype, const double* A, int64_t lda, int64_t nA, const double* B, int64_t ldb,
                int64_t nB, int d, const double* winv, double sigma0, double* out, int64_t ldo);

struct GemmOpts {
  int tri = TRI_FULL;  // TRI_* (nk_gemm_plan.h)
  int splitk = 0;      // 0 = choose automatically
};
// C = alpha*op(A)*op(B) + beta*C ; transA: A stored KxM ; transB: B stored NxK
int launch_gemm(nk_ctx* ctx, bool transA, bool transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
                int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc,
                const GemmOpts& opts = GemmOpts(), float* ms_kernel = nullptr);

struct GemmCall {
  int64_t M = 0, N = 0, K = 0;
  double alpha = 1.0, beta = 0.0;
  const double* A = nullptr;
  const double* B = nullptr;
  double* C = nullptr;
  int64_t lda = 0, ldb = 0, ldc = 0;
  GemmOpts opts;
};
// up to two independent problems with the same transposition flags in one launch (no split-K)
int launch_gemm_pair(nk_ctx* ctx, bool transA, bool transB, const GemmCall* calls, int ncalls);

struct TnSkip;  // device-side launch control of the TN engine (nk_tn.h)
// elementwise / reductions (nk_elementwise.hip)
// workgroups of a grid-stride launch over `total` elements; it also fixes the number of per-block partials of the
// reductions and with it their summation order
static inline int grid_for(int64_t total, int num_cu) {
  int64_t b = (total + 255) / 256;
  const int64_t cap = (int64_t)num_cu * 8;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
int launch_add_diag(nk_ctx* ctx, double* A, int64_t lda, int n, double v);
int launch_copy2d(nk_ctx* ctx, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols);
int launch_axpby2d(nk_ctx* ctx, double a, const double* X, int64_t ldx, double b, double* Y, int64_t ldy,
                   int64_t rows, int64_t cols);  // Y = a*X + b*Y
int launch_scale_add_identity(nk_ctx* ctx, double a, const double* X, int64_t ldx, double c, double* Y, int64_t ldy,
                              int n, const TnSkip* skip = nullptr);  // Y = a*X + c*I
int launch_fill(nk_ctx* ctx, double* A, int64_t lda, int64_t rows, int64_t cols, double v);
int launch_frob_minus_identity(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* d_out,
                               const TnSkip* skip = nullptr);  // sum (M-I)^2
// the per-block partials of sum (M-I)^2 alone, grid_for(n * n) of them (*count), for a caller that sums them itself
int launch_frob_mi_partials(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* partial, int* count, const TnSkip* skip);
int launch_max_abs_rowsum(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* d_out);
// d_sumsq[0] = sum of squares of M (n x n), d_trace[0] = its trace (nullptr: the sum of squares only)
int launch_sumsq_trace(nk_ctx* ctx, const double* M, int64_t ldm, int n, double* d_sumsq, double* d_trace);
int launch_colsum_sqdiff(nk_ctx* ctx, const double* P, int64_t ldp, const double* Y, int64_t ldy, int64_t rows,
                         int cols, double* d_colsum);  // colsum[j] = sum_i (P[i][j]-Y[i][j])^2

// dense SPD machinery built on the GEMM engine
int sqrtm_spd(nk_ctx* ctx, const double* P, int64_t ldp, int m, double* S, double* Sinv, int* iters, double* resid);
// the same in two phases, so that a caller can queue the latency-bound half (Cholesky factor of P and its inverse) early
// and the GEMM-bound half (Newton-Schulz polar iteration) later, both on the current stream; no host synchronisation in
// sqrtm_prepare.  The plan's buffers live in the current arena until sqrtm_finish returns.
struct SqrtPlan {
  const double* P = nullptr;
  int64_t ldp = 0;
  int m = 0;
  double* W = nullptr;     // 2m x m: lower Cholesky factor L of P on top, L^-T below
  double* Linv = nullptr;  // inverted diagonal blocks
  double* X0 = nullptr;    // L^T / sqrt(c)   (c = ||P||_inf)
  double* X0t = nullptr;   // L / sqrt(c)
  double* d_sc = nullptr;  // SQ_COUNT device scalars, the SQ_* slots above
  ArenaMark mark{0, 0};
  // verdict of sqrtm_finish: known at once for the synchronous forms, otherwise in ctx->h_scalars[HS_SQRT_FLAG ..] once the
  // stream has been synchronised (sqrtm_verdict)
  bool deferred = false;
  int rc = 0, iters = 0, kmax = 0;
  double resid = 0.0;
  // Optional rigorous lower bound of the smallest eigenvalue of P known to the caller (the jitter of K_mm + jitter I):
  // with it the step budget needs nothing from the factorisation, so sqrtm_finish queues the iteration without waiting
  // for sqrtm_prepare's kernels (`early`); a failed factorisation or an exhausted budget then surfaces in
  // sqrtm_verdict as NK_SQRT_RETRY and the caller falls back to sqrtm_spd_coupled.
  double lambda_min_hint = 0.0;
  bool early = false;
  int info_slot = 2;          // failure-flag slot of the stream sqrtm_finish ran on (sqrtm_verdict reads the early form's word there)
  bool flow_gave_up = false;  // the early form's factorisation was a dataflow launch that gave up (sqrtm_verdict)
  // The factorisation chain of sqrtm_prepare is paused before block step `pause_step` until `pause_event` (recorded by
  // the caller BEFORE sqrtm_prepare is called) has completed -- see nk_nystrom_fit: the chain must not run beside the
  // fused Gram launch.
  hipEvent_t pause_event = nullptr;
  int pause_step = -1;
};
constexpr int NK_SQRT_RETRY = 1;  // internal (positive) verdict: redo the square root with the coupled iteration
int sqrtm_spd_coupled(nk_ctx* ctx, const double* P, int64_t ldp, int m, double* S, double* Sinv, int* iters, double* resid);
int sqrtm_prepare(nk_ctx* ctx, const double* P, int64_t ldp, int m, SqrtPlan* plan);
int sqrtm_finish(nk_ctx* ctx, SqrtPlan* plan, double* S, double* Sinv);
// after the stream that ran sqrtm_finish has been synchronised: NK_OK / NK_ERR_NO_CONVERGENCE, iteration count, residual
int sqrtm_verdict(nk_ctx* ctx, SqrtPlan* plan, int* iters, double* resid);

// E_out (rows x m) = E * pinv(P) for symmetric P with LAPACK gelsd's cut-off (singular values <= rcond * sigma_max are
// dropped): one-sided Jacobi SVD on the device (nk_pinv.hip), the fallback of the regularised solves
struct PinvInfo {
  int rank = 0, sweeps = 0;
  bool converged = false;
  double sigma_max = 0.0, sigma_min_kept = 0.0, sigma_min = 0.0;
};
int pinv_right_divide(nk_ctx* ctx, const double* P, int64_t ldp, int m, const double* E, int64_t lde, int rows,
                      double* E_out, int64_t ldeo, double rcond, PinvInfo* info);

// matrix-vector step of the lifted recursion for up to 8 trajectories (nk_rollout.hip)
int launch_lifted_step(nk_ctx* ctx, const double* G, int64_t ldg, int m, int mz, int pu, const double* z, int64_t zstride,
                       const double* u, int64_t ustride, const double* bias, double* out, int64_t ostride, int batch);

// (which kernel advances a recursion, and all its size classes: nk_chain_plan.h)
// the whole recursion z_{t+1} = G [z_t; u_t] + bias for a batch of trajectories in ONE launch, G resident in LDS (m <= 128);
// optionally preceded by the lift of the initial states by the same workgroups (nk_rollout.hip)
struct ChainArgs {
  const double* G = nullptr; int64_t ldg = 0; int m = 0, pu = 0;
  const double* z0 = nullptr; int64_t z0_stride = 0;
  bool lift = false;
  const double* x0 = nullptr; int64_t x0_stride = 0;
  const double* Zl = nullptr; int d = 0; const double* winv = nullptr; const double* Sinv = nullptr; int ktype = 0;
  double sigma0 = 0.0;
  const double* U = nullptr; int64_t u_stride = 0;
  const double* bias = nullptr; int64_t bias_stride = 0;
  double* Zall = nullptr; int64_t z_stride = 0;
  int T = 0, batch = 0;
};
int launch_ref_minus_traj(nk_ctx* ctx, const double* ref, int64_t ref_stride, const double* Phi, int64_t phi_stride,
                          double* D, int64_t d_stride, int steps, int m, int batch);
// open-loop forecast error reduced on the device (nk_traj_err.hip): out[b] = (sum (x_true - C z)^2, sum (C z)^2) over the T
// steps of trajectory b, from the lifted states Zall [b][t][m]; the product C z is never stored.  m <= 4096.
// (traj_err_tile, the time steps per workgroup, is in nk_chain_plan.h)
int launch_traj_err(nk_ctx* ctx, const double* Zall, int64_t z_stride, const double* Cop, int64_t ldc, const double* Xtrue,
                    int64_t x_stride, int m, int d, int T, int batch, double* out);
int launch_lifted_chain(nk_ctx* ctx, const ChainArgs& a);
// m > 128: multi-workgroup recursion, one launch per group of trajectories that is resident at once (nk_rollout.hip)
bool lifted_chain_mw_ok(const nk_ctx* ctx, int m, int pu);
int launch_lifted_chain_mw(nk_ctx* ctx, const ChainArgs& a);
int lifted_chain_mw_reset(nk_ctx* ctx);                                       // clears the device status words
int lifted_chain_mw_fetch_status(nk_ctx* ctx);                                // queues their copy to the host
bool lifted_chain_mw_timed_out(nk_ctx* ctx, int* row, int* step, int* traj);  // after the stream has been synchronised

// LQR closed loop around one of the library's plants (nk_plant.h) in ONE launch, one workgroup per trajectory
// (nk_plant_loop.hip): w = the gain folded into the lift (m entries, p = 1), u_t = sum_j w_j (k(z_j, x_ref) - k(z_j, x_t)),
// x_{t+1} = plant(x_t, u_t); out_x rows b * (steps + 1) + t (row 0 = x_0), out_u rows b * steps + t
int plant_loop_max_m();
void plant_step_host(int plant, double Ts, const double* x, double u, double* x_next);  // nk_plant_step; plant id checked
int launch_plant_loop(nk_ctx* ctx, const nk_model* mdl, int plant, double Ts, const double* w, const double* x0,
                      int64_t x0_stride, const double* xref, int64_t xref_stride, int steps, int batch, double* out_x,
                      int64_t ldx, double* out_u, int64_t ldu);
// The record of one loop, every pointer device memory.  The single call passes the record of batch member 0 and the strides
// to the others (LoopStrides, nk_loop_lanes.h; u_opt and score null).  The multi-model form (nk_plant_loop_multi) stages one
// record per unit: sorted into classes of (kernel family, landmarks per lane, waves per workgroup; nk_loop_classes.h), moved
// with one copy and run with one launch per class; a workgroup finds its record by its block index.  out_x / out_u / u_opt /
// score may be null per unit there.
struct PlantLoopUnit {
  const double* Z;      // m x d landmarks
  const double* winv;   // d
  const double* w;      // m folded gain
  const double* x0;     // d
  const double* xref;   // d
  double* out_x;        // (steps + 1) rows of ldx, or nullptr
  double* out_u;        // steps rows of ldu, or nullptr
  const double* u_opt;  // steps controls to score against, or nullptr
  double* score;        // {sse_u, ss_opt, J, u_absmax}, or nullptr
  int64_t ldx, ldu;
  double sigma0sq;
  int m, reserved;
};
int launch_plant_loop_multi(nk_ctx* ctx, int plant, double Ts, int steps, PlantLoopUnit* units, const int* ktypes,
                            int n_units);
// The same loops around a polynomial plant the caller describes (nk_poly_plant.h; nk_poly_plant_loop and its multi form): d
// states, p inputs, the plant table by value in the kernel arguments.  One record per loop, every pointer device memory, used
// by the single call and the multi form as PlantLoopUnit is.
// W: the folded gain, entry (landmark l, input j) at w[l * w_ls + j * w_js]; out_u: steps rows of ldu, p columns; u_opt:
// steps x p, dense.  Classes of a launch: (kernel family, landmarks per lane, waves per workgroup); the kernels are
// instantiated for the states and inputs padded with exact zeros to D in {2, 4} and P in {1, 2, 4}.
struct PolyLoopUnit {
  const double* Z;      // m x d landmarks
  const double* winv;   // d
  const double* w;      // folded gain
  const double* x0;     // d
  const double* xref;   // d
  double* out_x;        // (steps + 1) rows of ldx, or nullptr (multi form)
  double* out_u;        // steps rows of ldu, or nullptr (multi form)
  const double* u_opt;  // steps x p controls to score against, or nullptr
  double* score;        // {sse_u, ss_opt, J, u_absmax}, or nullptr
  int64_t ldx, ldu, w_ls, w_js;
  double sigma0sq;
  int m, reserved;
};
int poly_loop_max_m(int d, int p);  // the class limit on m (0: d or p out of range)
int launch_poly_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, const double* w, int64_t w_ls,
                     int64_t w_js, const double* x0, int64_t x0_stride, const double* xref, int64_t xref_stride, int steps,
                     int batch, double* out_x, int64_t ldx, double* out_u, int64_t ldu);
int launch_poly_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, PolyLoopUnit* units, const int* ktypes,
                           int n_units);
// The constrained MPC loop around a polynomial plant (nk_mpc_loop.hip; nk_mpc_loop): every pointer device memory.  w: the
// folded gradient map, m x nv dense (iters = 0: nv = p and w the folded gain); M, Hinv: nv x nv dense (iters = 0: unused); bnd:
// lo, hi, dlo, dhi back to back, nv each, infinite where a bound is absent; uinit / out_info may be null.  The limit on m
// for nv variables is mpc_loop_max_m (nk_mpc.h).
int mpc_loop_check_lds(nk_ctx* ctx, int m, int nv, int* lds_max_out = nullptr);  // before anything is queued
int launch_mpc_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, int nv, int iters, double rho, double tol,
                    const double* w, const double* M, const double* Hinv, const double* bnd, const double* x0, int64_t x0_stride,
                    const double* xref, int64_t xref_stride, const double* uinit, int64_t uinit_stride, int steps, int batch,
                    double* out_x, int64_t ldx, double* out_u, int64_t ldu, double* out_info);
// The same loop with ny output rows (nk_mpc_loop.hip; nk_mpc_out_loop), nt = nv + ny lanes: w the folded map of [F; T]
// (m x nt), Kb (nt x nt) and S0 transposed (nv x nt) of mpc_out_prepare (nk_mpc_out.h); bnd: five rows of nt -- lo, hi, dlo,
// dhi (output lanes: ylo, yhi, -inf, +inf) and ycomp as a double (-1 in the input lanes).  m <= mpc_loop_max_m(nt).
int launch_mpc_out_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, int nv, int ny, int iters, double rho,
                        double tol, double theta, const double* w, const double* Kb, const double* S0t, const double* bnd,
                        const double* x0, int64_t x0_stride, const double* xref, int64_t xref_stride, const double* uinit,
                        int64_t uinit_stride, int steps, int batch, double* out_x, int64_t ldx, double* out_u, int64_t ldu,
                        double* out_info);
// The record of one MPC loop, every pointer device memory: what a workgroup of either form works on.  The single calls pass
// the record of batch member 0 and the strides to the others (LoopStrides, nk_loop_lanes.h); the multi-model forms
// (nk_mpc_loop_multi, nk_mpc_out_loop_multi) stage one record per unit, sorted into classes of (kernel family, nt = nv + ny
// padded to 16 / 32 / 64, waves per workgroup), with one copy and run one launch per class, its dynamic LDS the largest need
// among its units; a workgroup finds its record by its block index.  out_x / out_u / out_info / u_opt / score / uinit may be
// null per unit there.  Without output rows ny = 0 and theta = 0 (neither is read), bnd has four rows and Kb, S0t are M and
// H^-1 (symmetric, so its transpose); with them nt = nv + ny, the fields are those of mpc_out_prepare (nk_mpc_out.h), and
// score has the NK_MPC_OUT_N_SCORES scores (the eight of nk_mpc_loop_multi, then y_viol_max and n_y_viol).
struct MpcLoopUnit {
  const double* Z;      // m x d landmarks
  const double* winv;   // d
  const double* w;      // m x nt folded map of F or [F; T] (iters = 0: m x p folded gain), dense
  const double* Kb;     // nt x nt: M, or Kb of the folded iteration (unused for iters = 0)
  const double* S0t;    // nv x nt: H^-1, or S0 = [H^-1; G H^-1] transposed
  const double* bnd;    // rows of nt: lo, hi, dlo, dhi (infinite where the caller gave none; output lanes: ylo, yhi, -inf, inf),
                        // with output rows a fifth: ycomp as a double (-1 in the input lanes)
  const double* x0;     // d
  const double* xref;   // d
  const double* uinit;  // p, or nullptr (zeros)
  double* out_x;        // (steps + 1) rows of ldx, or nullptr (multi forms)
  double* out_u;        // steps rows of ldu, or nullptr (multi forms)
  double* out_info;     // steps rows of 2, or nullptr
  const double* u_opt;  // steps x p controls to score against, or nullptr
  double* score;        // the NK_MPC_N_SCORES / NK_MPC_OUT_N_SCORES scores, or nullptr
  int64_t ldx, ldu;
  double sigma0sq, rho, tol;
  int m, nv, iters, ny;
  double theta;  // (ny and theta behind the fields the loop without rows reads: those keep the offsets they had, and with them
                 // the scored kernels of that loop their register counts)
};
int launch_mpc_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, MpcLoopUnit* units, const int* ktypes,
                          int n_units);
int launch_mpc_out_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, MpcLoopUnit* units, const int* ktypes,
                              int n_units);

// ---- lifted closed loops of many models in ONE launch, scored on the device (nk_loop_multi.hip): one 1024-thread workgroup
// per unit, blockIdx.x = the record.  Every pointer is device memory.  Per step t < steps: u_t = K (phi_ref - phi_t),
// x_t = C phi_t, phi_{t+1} = A phi_t + B u_t.  Phi / usq / sse: the unit's scratch (steps x m, steps, steps doubles).
// Any of out_x / out_u / out_ucum / out_err / score may be null; target may be null when out_err and score are.
constexpr int LOOP_MULTI_MAX_M = 128;
constexpr int LOOP_MULTI_MAX_P = 8;
struct LoopMultiUnit {
  const double* G; int64_t ldg;  // [A | B]: m rows of m + p entries
  const double* C;               // d x m, dense
  const double* K;               // p x m, dense
  const double* phi0;            // m
  const double* phi_ref;         // m
  const double* target;          // d, or nullptr
  const double* u_init;          // p (zeros when the caller gave none)
  double* Phi;                   // steps x m: phi_t
  double* usq;                   // steps: sum_j u_{t,j}^2
  double* sse;                   // steps: sum_k (x_{t,k} - target_k)^2
  double* out_x; int64_t ldx;    // steps rows, or nullptr
  double* out_u; int64_t ldu;    // steps rows, or nullptr
  double* out_ucum; int64_t ldc; // steps + 1 rows, or nullptr
  double* out_err;               // steps, or nullptr
  double* score;                 // {J, err_final, u_sumsq, u_absmax}, or nullptr
  int m, p, d, reserved;
};
// units: host records (read by the staging copy: alive until the stream has been synchronised)
int launch_closed_loop_multi(nk_ctx* ctx, const LoopMultiUnit* units, int n_units, int steps, double c);

// ---- batched Riccati solver (nk_dare.hip): one workgroup per problem, blockIdx.x = the record.  Every pointer is device
// memory.  ws: the problem's workspace of dare_ws_doubles(M) doubles, M = m rounded up to 16.  Either Q (m x m) or C
// (d x m: the cost is c sym(C'C), formed by the kernel's own product) is set.  R: p x p dense, nullptr = identity.
constexpr int DARE_MAX_M = 256;
constexpr int DARE_MAX_P = 8;
struct DareRec {
  const double* A; int64_t lda;  // m x m
  const double* B; int64_t ldb;  // m x p
  const double* Q; int64_t ldq;  // m x m, or nullptr
  const double* C; int64_t ldc;  // d x m, or nullptr
  const double* R;               // p x p dense, or nullptr
  double c;
  double* ws;
  double* outK;    // p x m dense
  double* outP;    // m x m dense, or nullptr
  double* delta;   // last relative step, or nullptr
  int* status;     // 0 converged, 1 max_iter reached, 2 non-finite values or a singular pivot
  int* iters;
  int m, p, M, d;
  int q_only;      // 1: write the cost matrix H_0 to outP and stop (nk_model_lqr_cost)
  int reserved;
};
inline int dare_pad(int m) { return (m + 15) & ~15; }
inline size_t dare_ws_doubles(int M) { return (size_t)7 * M * M; }
int launch_dare(nk_ctx* ctx, const DareRec* table_dev, int count, double tol, int max_iter);

// ---- one Riccati problem of any size m <= NK_DARE_LARGE_MAX_M, p <= NK_DARE_LARGE_MAX_P as a chain of launches
// (nk_dare_large.hip): the same doubling steps, the products through launch_gemm, the solve a blocked LU whose block steps
// are separate kernels.  Every pointer is device memory.  Either Q (m x m) or C (d x m: the cost is c sym(C'C)) is set.
// R: p x p, or nullptr = identity.  outK: p x m, outP: m x m or nullptr; both are NaN for a status other than 0.  The
// workspace (dare_large_ws_bytes) is a dedicated allocation released before the call returns (NK_ERR_OOM when it does not
// fit, nothing written).  Synchronises the stream once per doubling step.
struct DareLargeArgs {
  int m = 0, p = 0, d = 0;
  const double* A = nullptr; int64_t lda = 0;
  const double* B = nullptr; int64_t ldb = 0;
  const double* Q = nullptr; int64_t ldq = 0;
  const double* C = nullptr; int64_t ldc = 0;
  double c = 0.0;
  const double* R = nullptr; int64_t ldr = 0;
  double tol = 1e-13;
  int max_iter = 40;
  double* outK = nullptr; int64_t ldk = 0;
  double* outP = nullptr; int64_t ldp = 0;
};
struct DareLargeResult {
  int status = 0, iters = 0;  // status as in DareRec
  double delta = 0.0;         // last relative step (NaN when no step was taken)
};
size_t dare_large_ws_bytes(int m);
int launch_dare_large(nk_ctx* ctx, const DareLargeArgs& args, DareLargeResult* res);
// host wall clock of the calling thread's last launch_dare_large.  The split (LU launches, products, the per-step
// synchronisation) is taken only with NYSKOOP_DARE_TIMING set, which synchronises the stream around every phase.
struct DareLargeTimes {
  double ms_total = 0.0, ms_lu = 0.0, ms_products = 0.0, ms_sync = 0.0;
  int steps = 0;
};
void dare_large_last_times(DareLargeTimes* out);

// ---- controller build (nk_mpc_build.hip): Newton polish of the Riccati stage's gain, the condensed problem (H, F) and the
// output rows (G, T) of one unit per workgroup, blockIdx.x = the record.  Every pointer is device memory and every matrix
// but A, B, Q, C is dense.  Either Q (m x m) or C (d x m: the cost is c sym(C'C), formed as the Riccati kernel forms it) is
// set.  Pin: the terminal cost, symmetric (given by the caller, or the Riccati stage's P); Kin: the Riccati stage's gain, or nullptr
// (then K = (R + B'PB)^-1 B'PA is formed from Pin and no Newton step is taken).  pre_status: the Riccati stage's status
// word, or nullptr (then pre_status_imm counts).  Crows: the matrix whose rows comps[0 .. nc-1] are the output rows.
// sq, wide: the workspace of nk_mpc_build_pack.h.
constexpr int MPC_BUILD_MAX_M = 512;
constexpr int MPC_BUILD_MAX_P = 4;
constexpr int MPC_BUILD_MAX_NC = 4;
struct MpcBuildRec {
  const double* A; int64_t lda;
  const double* B; int64_t ldb;
  const double* Q; int64_t ldq;
  const double* C; int64_t ldc;
  const double* R;       // p x p, or nullptr = identity
  const double* Pin;     // m x m
  const double* Kin;     // p x m, or nullptr
  const double* Crows; int64_t ldcr;
  const int* pre_status;
  double c;
  double *sq, *wide;
  double *outH, *outF, *outK, *outP, *outG, *outT;  // outP, outG, outT may be nullptr
  int* status;           // 0, or 1 / 2 of the Riccati stage, 2 (non-finite, not positive definite), 3 (Smith cap)
  int* iters;            // Smith squarings over all Newton steps
  int m, p, N, nc, Ny, d, M, NVP;
  int comps[MPC_BUILD_MAX_NC];
  int newton_steps, pre_status_imm;
};
int launch_mpc_build(nk_ctx* ctx, const MpcBuildRec* table_dev, int count, double newton_tol, int newton_max_iter);

// ---- landmark selection (nk_landmarks.hip): partial pivoted Cholesky of K(Y, Y) over the candidate rows rng ([begin, end)
// pairs of rows of the device matrix Y, nc rows in all), m steps queued without a host round trip.  positions: the
// m_selected candidate positions in pick order; resid: m entries, trace: m + 1 entries (zero past the stop).  The factor
// is a dedicated allocation released before the call returns (NK_ERR_OOM when it does not fit).
constexpr int LANDMARKS_MAX_M = 4096;
constexpr int LANDMARKS_MAX_D = 2048;  // (m + d) doubles of LDS per workgroup of the column launch
int select_landmarks_device(nk_ctx* ctx, int ktype, const double* Y, int64_t ldy, const std::vector<int64_t>& rng, int64_t nc,
                            int d, const double* winv, double sigma0, int rule, const double* u_host, int m, double tol,
                            std::vector<int64_t>* positions, std::vector<double>* resid, std::vector<double>* trace,
                            int* m_selected);

// X += dX if the refinement still contracts (verdict on the device, in state[4]: alive, |dX|^2 last accepted, accepted
// steps, |dX_0| / |X|); no host synchronisation
constexpr int refine_partial_blocks() { return 512; }
int launch_refine_apply(nk_ctx* ctx, const double* dX, int64_t ldd, double* X, int64_t ldx, int64_t rows, int64_t cols, int step,
                        double* state, double* partial);
// Res (nr x mq) = R - X P, dot products in doubled precision (compensated): the residual of the refinement steps
int launch_resid_dd(nk_ctx* ctx, const double* X, int64_t ldx, const double* P, int64_t ldp, const double* R, int64_t ldr,
                    double* Res, int64_t ldres, int nr, int mq);
}  // namespace nk

// ---- cross-lane helpers for fp64 on gfx950 (no LDS traffic): DPP moves inside a 16-lane row, v_permlane16_swap /
//      v_permlane32_swap between rows and half waves (checked lane by lane on the device by tools/reduce_probe.hip)
#if defined(__HIPCC__)
namespace nk {
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
typedef unsigned chain_u2 __attribute__((ext_vector_type(2)));
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// rows 1 and 3 (lanes 16-31, 48-63) of a change places with rows 0 and 2 of b
__device__ __forceinline__ void swap16_f64(double& a, double& b) {
  const chain_u2 lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const chain_u2 hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  a = __hiloint2double((int)hi.x, (int)lo.x);
  b = __hiloint2double((int)hi.y, (int)lo.y);
}
// lanes 32-63 of a change places with lanes 0-31 of b
__device__ __forceinline__ void swap32_f64(double& a, double& b) {
  const chain_u2 lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const chain_u2 hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  a = __hiloint2double((int)hi.x, (int)lo.x);
  b = __hiloint2double((int)hi.y, (int)lo.y);
}
// sum of one value over the 64 lanes, in every lane, without the LDS crossbar (a __shfl_down reduction is six dependent
// ds_bpermute round trips)
__device__ __forceinline__ double wave_sum64_dpp(double c) {
  c += dpp_f64<0xB1>(c);   // quad_perm [1,0,3,2]
  c += dpp_f64<0x4E>(c);   // quad_perm [2,3,0,1]
  c += dpp_f64<0x141>(c);  // row_half_mirror
  c += dpp_f64<0x140>(c);  // row_mirror: every lane of a 16-lane row holds the row total
  double a = c, b = c;
  swap16_f64(a, b);
  c = a + b;               // rows 0+1, 2+3
  a = c; b = c;
  swap32_f64(a, b);
  return a + b;
}

// Four values per lane, summed over the 32 lanes of a half wave: afterwards every lane holds the total of value
// r = 2 * bit4(lane) + bit3(lane) (checked lane by lane on the device by tools/reduce_probe.hip).  Fixed order: the
// result does not depend on anything but the inputs.
__device__ __forceinline__ double reduce_4rows_32parts(double a0, double a1, double a2, double a3, int lane) {
  swap16_f64(a0, a2);
  const double e0 = a0 + a2;  // lanes with bit4 = 0: value 0, bit4 = 1: value 2 (each over parts {q, q + 16})
  swap16_f64(a1, a3);
  const double e1 = a1 + a3;  // value 1 / value 3
  const bool hi8 = (lane & 8) != 0;
  const double keep = hi8 ? e1 : e0, send = hi8 ? e0 : e1;
  double c = keep + dpp_f64<0x140>(send);  // row_mirror: lane i <-> 15 - i
  c += dpp_f64<0xB1>(c);                   // quad_perm [1,0,3,2]
  c += dpp_f64<0x4E>(c);                   // quad_perm [2,3,0,1]
  c += dpp_f64<0x141>(c);                  // row_half_mirror: lane i <-> 7 - i
  return c;
}

// kernel value from the accumulated squared distance (RBF, Matern-5/2) or dot product (linear) of the pre-scaled
// coordinates: the epilogue of the kernel-matrix kernels, for the single-launch loops (nk_rollout.hip, nk_plant_loop.hip)
__device__ __forceinline__ double chain_kfun(int ktype, double acc, double sigma0sq) {
  if (ktype == NK_KERNEL_RBF) return exp_nonpos(-0.5 * acc);
  if (ktype == NK_KERNEL_MATERN52) {
    const double t = sqrt(acc) * 2.23606797749978969641;
    return (1.0 + t + t * t / 3.0) * exp_nonpos(-t);
  }
  return acc + sigma0sq;
}

}  // namespace nk
#endif
