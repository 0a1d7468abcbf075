// The runtime of libnyskoop.so (include/nyskoop.h): errors, arena, staging of host/device buffers, contexts, groups, the
// registry of everything the library owns, shutdown, and the lifetime of a model (create, destroy, fetch).  The compute
// entry points are in nk_api_compute.hip, the fits in nk_fit.hip, the one-call sweeps in nk_sweep.hip, rollouts and the
// lifted closed loop in nk_control.hip, the one-launch loops in nk_api_loops.hip, the Riccati entries in nk_api_dare.hip;
// what they share is declared in nk_api_internal.h.
#include "nk_common.h"
#include "nk_api_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <mutex>
#include <set>

namespace nk {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

bool is_device_ptr(const void* p) {
  if (p == nullptr) return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // unregistered host memory: clear the sticky error
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// ---- arena -----------------------------------------------------------------------------------------------------
static int arena_new_chunk(nk_ctx* ctx, Arena& a, size_t bytes) {
  ArenaChunk c;
  c.cap = bytes;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&c.base), bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("HBM workspace allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return NK_ERR_OOM;
  }
  a.chunks.push_back(c);
  if (getenv("NYSKOOP_TRACE")) fprintf(stderr, "[nyskoop] arena: new chunk of %zu MiB (%zu chunks)\n", bytes >> 20, a.chunks.size());
  return NK_OK;
}

static int arena_reset_one(nk_ctx* ctx, Arena& a) {
  if (a.chunks.size() > 1) {  // coalesce: steady state is one chunk and no hipMalloc on the hot path
    NK_HIP(hipStreamSynchronize(ctx->stream_main));
    NK_HIP(hipStreamSynchronize(ctx->stream_side));
    NK_HIP(hipStreamSynchronize(ctx->stream_prep));
    size_t total = 0;
    for (auto& c : a.chunks) {
      total += c.cap;
      (void)hipFree(c.base);
    }
    a.chunks.clear();
    NK_TRY(arena_new_chunk(ctx, a, total));
  }
  for (auto& c : a.chunks) c.off = 0;
  a.cur = 0;
  return NK_OK;
}

int arena_reset(nk_ctx* ctx) {
  ctx->stream = ctx->stream_main;
  ctx->cur_arena = &ctx->arena;
  NK_TRY(arena_reset_one(ctx, ctx->arena));
  return arena_reset_one(ctx, ctx->arena_side);
}

ArenaMark arena_mark(nk_ctx* ctx) {
  Arena& a = *ctx->cur_arena;
  if (a.chunks.empty()) return ArenaMark{0, 0};
  return ArenaMark{a.cur, a.chunks[a.cur].off};
}

void arena_release(nk_ctx* ctx, ArenaMark mk) {
  Arena& a = *ctx->cur_arena;
  if (a.chunks.empty()) return;
  for (int i = mk.chunk + 1; i < (int)a.chunks.size(); ++i) a.chunks[i].off = 0;
  a.cur = mk.chunk;
  a.chunks[a.cur].off = mk.off;
}

int arena_alloc(nk_ctx* ctx, size_t bytes, void** out) {
  Arena& a = *ctx->cur_arena;
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes == 0) bytes = 256;
  for (;;) {
    if (!a.chunks.empty()) {
      ArenaChunk& c = a.chunks[a.cur];
      if (c.off + bytes <= c.cap) {
        *out = c.base + c.off;
        c.off += bytes;
        return NK_OK;
      }
      if (a.cur + 1 < (int)a.chunks.size()) {
        ++a.cur;
        a.chunks[a.cur].off = 0;
        continue;
      }
    }
    size_t want = bytes;
    const size_t min_chunk = (size_t)256 << 20;
    if (want < min_chunk) want = min_chunk;
    if (!a.chunks.empty() && want < a.chunks.back().cap) want = a.chunks.back().cap;
    NK_TRY(arena_new_chunk(ctx, a, want));
    a.cur = (int)a.chunks.size() - 1;
  }
}

// ---- staging ---------------------------------------------------------------------------------------------------
int stage_in(nk_ctx* ctx, const double* p, int64_t ld, int64_t rows, int64_t cols, MatIn* out) {
  out->rows = rows;
  out->cols = cols;
  if (rows <= 0 || cols <= 0) {
    out->ptr = p;
    out->ld = ld;
    return NK_OK;
  }
  if (is_device_ptr(p)) {
    out->ptr = p;
    out->ld = ld;
    out->staged = false;
    return NK_OK;
  }
  const int64_t ldd = cols + (cols & 1);
  double* d = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)rows * ldd, &d));
  NK_HIP(hipMemcpy2DAsync(d, (size_t)ldd * 8, p, (size_t)ld * 8, (size_t)cols * 8, (size_t)rows, hipMemcpyHostToDevice,
                          ctx->stream));
  out->ptr = d;
  out->ld = ldd;
  out->staged = true;
  return NK_OK;
}
int stage_out(nk_ctx* ctx, double* p, int64_t ld, int64_t rows, int64_t cols, MatOut* out) {
  out->rows = rows;
  out->cols = cols;
  if (is_device_ptr(p)) {
    out->dev = p;
    out->ld = ld;
    out->host = nullptr;
    return NK_OK;
  }
  const int64_t ldd = cols + (cols & 1);
  NK_TRY(arena_alloc_t(ctx, (size_t)(rows > 0 ? rows : 1) * ldd, &out->dev));
  out->ld = ldd;
  out->host = p;
  out->host_ld = ld;
  return NK_OK;
}
int finish_out(nk_ctx* ctx, const MatOut& o) {
  if (o.host && o.rows > 0 && o.cols > 0)
    NK_HIP(hipMemcpy2DAsync(o.host, (size_t)o.host_ld * 8, o.dev, (size_t)o.ld * 8, (size_t)o.cols * 8, (size_t)o.rows,
                            hipMemcpyDeviceToHost, ctx->stream));
  return NK_OK;
}

int stage_pack(nk_ctx* ctx, UnitPack& pack, double** dev) {
  NK_TRY(arena_alloc_t(ctx, pack.doubles(), dev));
  NK_HIP(hipMemcpyAsync(*dev, pack.block(), pack.doubles() * 8, hipMemcpyHostToDevice, ctx->stream));
  return NK_OK;
}

int check_ctx(nk_ctx* ctx) {
  if (!ctx) {
    set_error("null context");
    return NK_ERR_BAD_ARG;
  }
  tl_ctx = ctx;  // the calling thread's current context (a context is used by one thread at a time)
  NK_HIP(hipSetDevice(ctx->device));
  return arena_reset(ctx);
}

int make_winv(nk_ctx* ctx, const nk_kernel_desc* kd, int d, double* dst_dev) {
  NK_REQUIRE(kd != nullptr, "null kernel descriptor");
  NK_REQUIRE(kd->type >= NK_KERNEL_RBF && kd->type <= NK_KERNEL_TPS, "unknown kernel type %d", kd->type);
  NK_REQUIRE(kd->d == d, "kernel descriptor is for %d dimensions, data has %d", kd->d, d);
  std::vector<double> w((size_t)d, 1.0);
  if (kd->type != NK_KERNEL_LINEAR && kd->type != NK_KERNEL_TPS) {
    NK_REQUIRE(kd->lengthscale != nullptr, "kernel lengthscale pointer is null");
    // sklearn _check_length_scale: an anisotropic kernel must match the data dimension
    NK_REQUIRE(kd->n_lengthscale == 1 || kd->n_lengthscale == d,
               "Anisotropic kernel must have the same number of dimensions as data (%d!=%d)", kd->n_lengthscale, d);
    for (int k = 0; k < d; ++k) {
      const double l = kd->lengthscale[kd->n_lengthscale == 1 ? 0 : k];
      NK_REQUIRE(l > 0.0 && std::isfinite(l), "lengthscale[%d] = %g is not positive", k, l);
      w[k] = 1.0 / l;
    }
  }
  NK_HIP(hipMemcpyAsync(dst_dev, w.data(), sizeof(double) * d, hipMemcpyHostToDevice, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // w is a stack vector
  return NK_OK;
}

// Model buffers are recycled through a small per-process free list: hipFree synchronises the whole device and a
// sweep creates and drops one model per fit.
struct ModelBuf {
  int device;
  size_t bytes;
  double* ptr;
};
// Everything the library owns is registered here, so that nk_shutdown can release it in a defined order BEFORE the HIP
// runtime's static destructors run, and so that destroying a handle twice (or after nk_shutdown) is a no-op.
static std::mutex g_pool_mu;
static std::vector<ModelBuf> g_pool;
static std::mutex g_reg_mu;
static std::set<nk_ctx*> g_ctxs;
static std::set<nk_model*> g_models;
static std::set<void*> g_host_blocks;

static double* pool_take(int device, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (size_t i = 0; i < g_pool.size(); ++i)
    if (g_pool[i].device == device && g_pool[i].bytes == bytes) {
      double* p = g_pool[i].ptr;
      g_pool.erase(g_pool.begin() + i);
      return p;
    }
  return nullptr;
}
static void pool_give(int device, size_t bytes, double* ptr) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool.size() < 512) {  // a lock-step group keeps one model per member in flight
      g_pool.push_back(ModelBuf{device, bytes, ptr});
      return;
    }
  }
  (void)hipSetDevice(device);
  (void)hipFree(ptr);
}
static void pool_drain() {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (auto& b : g_pool) {
    (void)hipSetDevice(b.device);
    (void)hipFree(b.ptr);
  }
  g_pool.clear();
}

int model_alloc(nk_ctx* ctx, int m, int d, int p, nk_model** out, int kind) {
  nk_model* mdl = new nk_model();
  mdl->device = ctx->device;
  mdl->m = m; mdl->d = d; mdl->p = p;
  mdl->kind = kind;
  const size_t mp = (size_t)m + p;
  const size_t nS = kind == NK_MODEL_SPLINE ? 0 : 2 * (size_t)m * m;  // S, Sinv (a spline model has neither)
  const size_t total = (size_t)m * mp /*G=[A B]*/ + (size_t)d * m /*C*/ + (size_t)d * mp /*W*/ + nS +
                       (size_t)m * d /*Z*/ + (size_t)d /*winv*/ + 64;
  mdl->bytes = total * sizeof(double);
  mdl->buf = pool_take(ctx->device, mdl->bytes);
  if (!mdl->buf) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&mdl->buf), mdl->bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      delete mdl;
      set_error("model allocation of %zu bytes failed: %s", total * sizeof(double), hipGetErrorString(e));
      return NK_ERR_OOM;
    }
  }
  double* q = mdl->buf;
  auto take = [&](size_t cnt) { double* r = q; q += (cnt + 1) & ~(size_t)1; return r; };
  mdl->A = take((size_t)m * mp);
  mdl->B = mdl->A + m;  // view into G = [A | B], leading dimension m + p
  mdl->C = take((size_t)d * m);
  mdl->W = take((size_t)d * mp);
  if (kind != NK_MODEL_SPLINE) {
    mdl->S = take((size_t)m * m);
    mdl->Sinv = take((size_t)m * m);
  }
  mdl->Z = take((size_t)m * d);
  mdl->winv = take((size_t)d);
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_models.insert(mdl);
  }
  *out = mdl;
  return NK_OK;
}


float ev_ms(nk_ctx* ctx, int a, int b) {
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]);
  return ms;
}


// ---- call staging (nk_api_internal.h)
static int small_reserve(nk_ctx* ctx, size_t bytes) {
  if (ctx->h_stage_bytes >= bytes) return NK_OK;
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  ctx->h_stage = nullptr;
  ctx->h_stage_bytes = 0;
  NK_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_stage), bytes, hipHostMallocDefault));
  ctx->h_stage_bytes = bytes;
  return NK_OK;
}
int CallStage::commit() {
  size_t need = 0;
  for (const Operand& o : ops) need += pad256((size_t)o.rows * o.cols);
  pinned = need <= SMALL_STAGE_LIMIT;
  for (size_t i = 0; pinned && i < ops.size(); ++i) pinned = !is_device_ptr(ops[i].ptr);
  if (!pinned) {
    for (const Operand& o : ops) {
      if (o.in) NK_TRY(stage_in(ctx, o.ptr, o.ld, o.rows, o.cols, o.in));
      else NK_TRY(stage_out(ctx, const_cast<double*>(o.ptr), o.ld, o.rows, o.cols, o.out));
    }
    return NK_OK;
  }
  NK_TRY(small_reserve(ctx, need));
  char* slot = reinterpret_cast<char*>(ctx->h_stage);
  for (const Operand& o : ops) {
    double* dst = reinterpret_cast<double*>(slot);
    slot += pad256((size_t)o.rows * o.cols);
    if (o.in) {
      for (int64_t r = 0; r < o.rows; ++r) memcpy(dst + r * o.cols, o.ptr + r * o.ld, (size_t)o.cols * 8);
      o.in->ptr = dst; o.in->ld = o.cols; o.in->staged = true; o.in->rows = o.rows; o.in->cols = o.cols;
    } else {
      o.out->dev = dst; o.out->ld = o.cols; o.out->host = const_cast<double*>(o.ptr); o.out->host_ld = o.ld;
      o.out->rows = o.rows; o.out->cols = o.cols;
    }
  }
  return NK_OK;
}
int CallStage::resident(MatIn* v, int64_t ld) {
  const char *lo = reinterpret_cast<const char*>(ctx->h_stage), *at = reinterpret_cast<const char*>(v->ptr);
  if (!pinned || at < lo || at >= lo + ctx->h_stage_bytes) return NK_OK;
  double* dst = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)v->rows * ld, &dst));
  NK_TRY(launch_copy2d(ctx, v->ptr, v->ld, dst, ld, v->rows, v->cols));
  v->ptr = dst;
  v->ld = ld;
  return NK_OK;
}
int CallStage::queue_outputs() {
  if (pinned) return NK_OK;
  for (const Operand& o : ops)
    if (o.out) NK_TRY(finish_out(ctx, *o.out));
  return NK_OK;
}
void CallStage::deliver() {
  if (!pinned) return;
  for (const Operand& o : ops)
    if (o.out)
      for (int64_t r = 0; r < o.rows; ++r) memcpy(o.out->host + r * o.ld, o.out->dev + r * o.cols, (size_t)o.cols * 8);
}

}  // namespace nk

using namespace nk;

// The operators of a model rebuilt from host or device copies (the two model-create entries): A, B, C staged and copied
// into the model's layout, W copied or formed as C [A B].  Without A and C the model stays without operators.
static int model_load_ops(nk_ctx* ctx, const char* who, nk_model* mdl, const double* A, const double* B, const double* C,
                          const double* W) {
  if (!(A && C)) return NK_OK;
  const int m = mdl->m, d = mdl->d, p = mdl->p, mp = m + p;
  NK_REQUIRE(p == 0 || B != nullptr, "%s: B missing", who);
  MatIn a, b, c, w;
  NK_TRY(stage_in(ctx, A, m, m, m, &a));
  NK_TRY(launch_copy2d(ctx, a.ptr, a.ld, mdl->A, mp, m, m));
  if (p > 0) {
    NK_TRY(stage_in(ctx, B, p, m, p, &b));
    NK_TRY(launch_copy2d(ctx, b.ptr, b.ld, mdl->B, mp, m, p));
  }
  NK_TRY(stage_in(ctx, C, m, d, m, &c));
  NK_TRY(launch_copy2d(ctx, c.ptr, c.ld, mdl->C, m, d, m));
  if (W) {
    NK_TRY(stage_in(ctx, W, mp, d, mp, &w));
    NK_TRY(launch_copy2d(ctx, w.ptr, w.ld, mdl->W, mp, d, mp));
  } else {
    NK_TRY(launch_gemm(ctx, false, false, d, mp, m, 1.0, mdl->C, m, mdl->A, mp, 0.0, mdl->W, mp));
  }
  mdl->has_ops = true;
  return NK_OK;
}

// one operator block of a model to the caller (host or device memory): one plain copy when both sides are dense
static hipError_t copy_ops_block(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols,
                                 hipStream_t st) {
  const hipMemcpyKind kind = is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (ldd == cols && lds == cols) return hipMemcpyAsync(dst, src, (size_t)rows * cols * 8, kind, st);
  return hipMemcpy2DAsync(dst, (size_t)ldd * 8, src, (size_t)lds * 8, (size_t)cols * 8, (size_t)rows, kind, st);
}

extern "C" {

int nk_version(void) { return NK_ABI_VERSION; }

const char* nk_last_error(void) { return g_err.c_str(); }

int nk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int nk_create(int device, nk_ctx** out) {
  NK_REQUIRE(out != nullptr, "nk_create: null output pointer");
  *out = nullptr;
  int n = nk_device_count();
  if (n <= 0) {
    set_error("no HIP device visible: libnyskoop has no CPU fallback");
    return NK_ERR_NO_DEVICE;
  }
  NK_REQUIRE(device >= 0 && device < n, "nk_create: device %d out of range (0..%d)", device, n - 1);
  // NYSKOOP_STRICT_SPD = 0 / 1 / 2, the modes of nk_set_strict_spd (unset or empty: 0); anything else is refused, as there
  int strict_env = 0;
  if (const char* st = getenv("NYSKOOP_STRICT_SPD"); st && st[0]) {
    char* end = nullptr;
    const long v = strtol(st, &end, 10);
    NK_REQUIRE(end != st && *end == '\0' && v >= 0 && v <= 2, "nk_create: NYSKOOP_STRICT_SPD=%s is not 0, 1 or 2", st);
    strict_env = (int)v;
  }
  NK_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  NK_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %d is %s; libnyskoop is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    return NK_ERR_NO_DEVICE;
  }
  nk_ctx* ctx = new nk_ctx();
  ctx->device = device;
  ctx->num_cu = prop.multiProcessorCount;
  // Three priority levels (the dispatcher serves hardware queues in strict priority order, so a queue with pending
  // workgroups starves every lower one):
  //   prep stream: highest -- a short latency-bound chain queued beside the big kernel-block / Gram launches of the main
  //                stream; its tiny kernels must get the first CU slots that free up;
  //   main stream: middle  -- the big launches and the factorisation chains;
  //   side stream: lowest  -- the GEMM-bound square-root iteration that fills the chip beside the factorisation chain.
  int prio_lo = 0, prio_hi = 0;
  NK_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  const int prio_mid = (prio_lo - prio_hi >= 2) ? (prio_lo + prio_hi) / 2 : prio_hi;
  NK_HIP(hipStreamCreateWithPriority(&ctx->stream_main, hipStreamNonBlocking, prio_mid));
  NK_HIP(hipStreamCreateWithPriority(&ctx->stream_side, hipStreamNonBlocking, prio_lo));
  NK_HIP(hipStreamCreateWithPriority(&ctx->stream_prep, hipStreamNonBlocking, prio_hi));
  NK_HIP(hipStreamCreateWithFlags(&ctx->stream_copy, hipStreamNonBlocking));
  NK_HIP(hipStreamCreateWithPriority(&ctx->stream_la[0], hipStreamNonBlocking, prio_hi));
  NK_HIP(hipStreamCreateWithPriority(&ctx->stream_la[1], hipStreamNonBlocking, prio_mid));
  for (int q = 0; q < 2; ++q)
    for (int i = 0; i < 4; ++i) NK_HIP(hipEventCreateWithFlags(&ctx->ev_la[q][i], hipEventDisableTiming));
  ctx->stream = ctx->stream_main;
  ctx->cur_arena = &ctx->arena;
  NK_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  NK_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  NK_HIP(hipEventCreateWithFlags(&ctx->ev_chain, hipEventDisableTiming));
  NK_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_info), 256));
  ctx->d_piv = reinterpret_cast<unsigned long long*>(ctx->d_info + 16);  // 8 x 8 bytes behind the 4 flag slots
  NK_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_scalars), HS_COUNT * sizeof(double)));
  // (mapped + coherent, explicitly: in lock-step groups the device stores to these mirrors directly, nk_group.hip)
  NK_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_scalars), HS_COUNT * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
  NK_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_info), 256, hipHostMallocMapped | hipHostMallocCoherent));
  ctx->h_piv = reinterpret_cast<unsigned long long*>(ctx->h_info + 16);
  for (int i = 0; i < EV_COUNT; ++i) NK_HIP(hipEventCreate(&ctx->ev[i]));
  NK_HIP(hipEventCreateWithFlags(&ctx->ev_ext, hipEventDisableTiming));
  for (int i = 0; i < 8; ++i) NK_HIP(hipEventCreateWithFlags(&ctx->ev_up[i], hipEventDisableTiming));
  const char* km = getenv("NYSKOOP_KMAT");
  ctx->kmat_mode = (km && strcmp(km, "direct") == 0) ? 1 : 0;
  ctx->strict_spd = strict_env;
  if (const char* rp = getenv("NYSKOOP_REFINE_PIVOT")) ctx->refine_pivot = atof(rp);
  if (const char* rs = getenv("NYSKOOP_REFINE_STEPS")) ctx->refine_steps = std::max(0, atoi(rs));
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_ctxs.insert(ctx);
  }
  *out = ctx;
  return NK_OK;
}

static void destroy_ctx_unregistered(nk_ctx* ctx) {
  (void)hipSetDevice(ctx->device);
  if (tl_ctx == ctx) tl_ctx = nullptr;
  group_detach(ctx);  // flushes what the member recorded; the group goes with its last member
  (void)hipStreamSynchronize(ctx->stream_main);
  (void)hipStreamSynchronize(ctx->stream_side);
  (void)hipStreamSynchronize(ctx->stream_prep);
  (void)hipStreamSynchronize(ctx->stream_copy);
  for (int q = 0; q < 2; ++q) {
    if (ctx->stream_la[q]) { (void)hipStreamSynchronize(ctx->stream_la[q]); (void)hipStreamDestroy(ctx->stream_la[q]); }
    for (int i = 0; i < 4; ++i) if (ctx->ev_la[q][i]) (void)hipEventDestroy(ctx->ev_la[q][i]);
  }
  for (auto& c : ctx->arena.chunks) (void)hipFree(c.base);
  for (auto& c : ctx->arena_side.chunks) (void)hipFree(c.base);
  (void)hipEventDestroy(ctx->ev_fork);
  (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ev_chain) (void)hipEventDestroy(ctx->ev_chain);
  if (ctx->ev_ext) (void)hipEventDestroy(ctx->ev_ext);
  for (int i = 0; i < 8; ++i) if (ctx->ev_up[i]) (void)hipEventDestroy(ctx->ev_up[i]);
  (void)hipStreamDestroy(ctx->stream_side);
  (void)hipStreamDestroy(ctx->stream_prep);
  (void)hipStreamDestroy(ctx->stream_copy);
  (void)hipFree(ctx->d_info);
  for (int i = 0; i < 2; ++i) if (ctx->d_flow[i]) (void)hipFree(ctx->d_flow[i]);
  (void)hipFree(ctx->d_scalars);
  if (ctx->d_zeros) (void)hipFree(ctx->d_zeros);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  (void)hipHostFree(ctx->h_scalars);
  (void)hipHostFree(ctx->h_info);
  for (int i = 0; i < EV_COUNT; ++i) (void)hipEventDestroy(ctx->ev[i]);
  (void)hipStreamDestroy(ctx->stream_main);
  delete ctx;
}

int nk_destroy(nk_ctx* ctx) {
  if (!ctx) return NK_OK;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_ctxs.erase(ctx) == 0) return NK_OK;  // already destroyed (nk_shutdown, or a second call)
  }
  destroy_ctx_unregistered(ctx);
  return NK_OK;
}

static int model_wait_unchecked(nk_model* mdl);
static void destroy_model_unregistered(nk_model* model, bool to_pool) {
  (void)model_wait_unchecked(model);  // a pending asynchronous fetch still reads the buffers
  if (to_pool) {
    pool_give(model->device, model->bytes, model->buf);
  } else {
    (void)hipSetDevice(model->device);
    (void)hipFree(model->buf);
  }
  delete model;
}

int nk_shutdown(void) {
  tl_ctx = nullptr;
  std::set<nk_ctx*> ctxs;
  std::set<nk_model*> models;
  std::set<void*> blocks;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    ctxs.swap(g_ctxs);
    models.swap(g_models);
    blocks.swap(g_host_blocks);
  }
  for (nk_ctx* c : ctxs) {  // drain everything first: models and pinned blocks may still be targets of queued copies
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream_main);
    (void)hipStreamSynchronize(c->stream_side);
    (void)hipStreamSynchronize(c->stream_prep);
    (void)hipStreamSynchronize(c->stream_copy);
  }
  for (nk_model* m : models) destroy_model_unregistered(m, false);
  for (nk_ctx* c : ctxs) destroy_ctx_unregistered(c);
  pool_drain();
  for (void* b : blocks) (void)hipHostFree(b);
  return NK_OK;
}

int nk_set_compute_dtype(nk_ctx* ctx, int dtype) {
  NK_REQUIRE(ctx != nullptr && (dtype == NK_DTYPE_F64 || dtype == NK_DTYPE_F32), "nk_set_compute_dtype: bad argument");
  ctx->compute_f32 = dtype == NK_DTYPE_F32 ? 1 : 0;
  return NK_OK;
}

int nk_set_strict_spd(nk_ctx* ctx, int strict) {
  NK_REQUIRE(ctx != nullptr && strict >= 0 && strict <= 2, "nk_set_strict_spd: bad argument");
  ctx->strict_spd = strict;
  return NK_OK;
}

int nk_set_refine(nk_ctx* ctx, double pivot_ratio, int32_t steps) {
  NK_REQUIRE(ctx != nullptr && pivot_ratio >= 0.0 && pivot_ratio <= 1.0 && steps >= 0 && steps <= 8, "nk_set_refine: bad argument");
  ctx->refine_pivot = pivot_ratio;
  ctx->refine_steps = steps;
  return NK_OK;
}

int nk_wait_stream(nk_ctx* ctx, void* producer_stream) {
  NK_REQUIRE(ctx != nullptr, "nk_wait_stream: null context");
  NK_HIP(hipSetDevice(ctx->device));
  if (ctx->group) {  // the group's shared stream is fed at flush time: wait for the producer here, once
    hipError_t e = real_stream_sync(reinterpret_cast<hipStream_t>(producer_stream));
    if (e != hipSuccess) { set_error("synchronising the producer stream failed: %s", hipGetErrorString(e)); return NK_ERR_HIP; }
    return NK_OK;
  }
  NK_HIP(hipEventRecord(ctx->ev_ext, reinterpret_cast<hipStream_t>(producer_stream)));
  NK_HIP(hipStreamWaitEvent(ctx->stream_main, ctx->ev_ext, 0));
  NK_HIP(hipStreamWaitEvent(ctx->stream_side, ctx->ev_ext, 0));
  NK_HIP(hipStreamWaitEvent(ctx->stream_prep, ctx->ev_ext, 0));
  NK_HIP(hipStreamWaitEvent(ctx->stream_copy, ctx->ev_ext, 0));
  return NK_OK;
}

int nk_group_create(int device, int size, nk_ctx** out) {
  NK_REQUIRE(out != nullptr && size >= 1 && size <= 256, "nk_group_create: bad argument");
  for (int i = 0; i < size; ++i) out[i] = nullptr;
  for (int i = 0; i < size; ++i) {
    int rc = nk_create(device, &out[i]);
    if (rc != NK_OK) {
      for (int j = 0; j < i; ++j) { nk_destroy(out[j]); out[j] = nullptr; }
      return rc;
    }
  }
  nk_group* g = group_new(device, size);
  if (!g) {
    for (int i = 0; i < size; ++i) { nk_destroy(out[i]); out[i] = nullptr; }
    set_error("nk_group_create: could not create the shared stream / argument table");
    return NK_ERR_HIP;
  }
  for (int i = 0; i < size; ++i) group_attach(g, i, out[i]);
  return NK_OK;
}

int nk_group_enter(nk_ctx* ctx) {
  NK_REQUIRE(ctx != nullptr, "nk_group_enter: null context");
  return group_enter(ctx);
}

int nk_group_leave(nk_ctx* ctx) {
  NK_REQUIRE(ctx != nullptr, "nk_group_leave: null context");
  tl_ctx = ctx;
  const int rc = group_leave(ctx);
  tl_ctx = nullptr;  // the thread is outside the unit: nothing it does next may be recorded for (or wait on) this member
  return rc;
}

int nk_runtime_counters(uint64_t* out, int32_t n) {
  NK_REQUIRE(out != nullptr && n >= 0, "nk_runtime_counters: bad argument");
  for (int i = 0; i < n && i < CNT_N; ++i) out[i] = nk::read_counter(i);
  return NK_OK;
}

int nk_group_stats(nk_ctx* ctx, uint64_t* out4) {
  NK_REQUIRE(ctx != nullptr && out4 != nullptr, "nk_group_stats: null argument");
  group_stats(ctx, out4);
  return NK_OK;
}

int nk_synchronize(nk_ctx* ctx) {
  NK_REQUIRE(ctx != nullptr, "null context");
  tl_ctx = ctx;
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

void* nk_stream(nk_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->stream) : nullptr; }

void* nk_host_alloc(uint64_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    set_error("hipHostMalloc of %llu bytes failed", (unsigned long long)bytes);
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(g_reg_mu);
  g_host_blocks.insert(p);
  return p;
}

void nk_host_free(void* ptr) {
  if (!ptr) return;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_host_blocks.erase(ptr) == 0) return;  // not ours, or already released by nk_shutdown
  }
  (void)hipHostFree(ptr);
}

int nk_set_kmat_mode(nk_ctx* ctx, int mode) {
  NK_REQUIRE(ctx != nullptr && (mode == 0 || mode == 1), "nk_set_kmat_mode: bad argument");
  ctx->kmat_mode = mode;
  return NK_OK;
}

int nk_model_create(nk_ctx* ctx, const nk_kernel_desc* kd, const double* Zout, int64_t ldz, int32_t m, int32_t d,
                    int32_t p, double jitter, const double* A, const double* B, const double* C, const double* W,
                    nk_model** model) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(kd && Zout && model, "nk_model_create: null argument");
  NK_REQUIRE(m > 0 && d > 0 && p >= 0 && ldz >= d, "nk_model_create: bad sizes");
  NK_REQUIRE(kd->type != NK_KERNEL_TPS, "nk_model_create: spline models come from nk_spline_model_create");
  *model = nullptr;
  nk_model* mdl = nullptr;
  NK_TRY(model_alloc(ctx, m, d, p, &mdl));
  struct Guard { nk_model* m; ~Guard() { if (m) nk_model_destroy(m); } } guard{mdl};
  mdl->ktype = kd->type; mdl->sigma0 = kd->sigma0; mdl->jitter = jitter;
  NK_TRY(make_winv(ctx, kd, d, mdl->winv));
  MatIn z;
  NK_TRY(stage_in(ctx, Zout, ldz, m, d, &z));
  NK_TRY(launch_copy2d(ctx, z.ptr, z.ld, mdl->Z, d, m, d));
  double* Kj = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Kj));
  NK_TRY(launch_kmat(ctx, kd->type, mdl->Z, d, m, mdl->Z, d, m, d, mdl->winv, kd->sigma0, Kj, m));
  NK_TRY(launch_add_diag(ctx, Kj, m, m, jitter));
  NK_TRY(sqrtm_spd(ctx, Kj, m, m, mdl->S, mdl->Sinv, nullptr, nullptr));
  NK_TRY(model_load_ops(ctx, "nk_model_create", mdl, A, B, C, W));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  guard.m = nullptr;
  *model = mdl;
  return NK_OK;
}

// rebuild a spline model from host copies (un-pickling KoopmanSplineRegressor)
int nk_spline_model_create(nk_ctx* ctx, const double* centers, int64_t ldc, int32_t m, int32_t d, int32_t p,
                           const double* A, const double* B, const double* C, const double* W, nk_model** model) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(centers && model, "nk_spline_model_create: null argument");
  NK_REQUIRE(m > 0 && d > 0 && p >= 0 && ldc >= d, "nk_spline_model_create: bad sizes");
  *model = nullptr;
  nk_model* mdl = nullptr;
  NK_TRY(model_alloc(ctx, m, d, p, &mdl, NK_MODEL_SPLINE));
  struct Guard { nk_model* m; ~Guard() { if (m) nk_model_destroy(m); } } guard{mdl};
  mdl->ktype = NK_KERNEL_TPS; mdl->sigma0 = 0.0; mdl->jitter = 0.0;
  NK_TRY(launch_fill(ctx, mdl->winv, d, 1, d, 1.0));
  MatIn z;
  NK_TRY(stage_in(ctx, centers, ldc, m, d, &z));
  NK_TRY(launch_copy2d(ctx, z.ptr, z.ld, mdl->Z, d, m, d));
  NK_TRY(model_load_ops(ctx, "nk_spline_model_create", mdl, A, B, C, W));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  guard.m = nullptr;
  *model = mdl;
  return NK_OK;
}

int nk_model_destroy(nk_model* model) {
  if (!model) return NK_OK;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_models.erase(model) == 0) return NK_OK;  // already destroyed (nk_shutdown, or a second call)
  }
  destroy_model_unregistered(model, true);
  return NK_OK;
}

int nk_model_dims(const nk_model* model, int32_t* m, int32_t* d, int32_t* p) {
  NK_REQUIRE(model != nullptr, "null model");
  if (m) *m = model->m;
  if (d) *d = model->d;
  if (p) *p = model->p;
  return NK_OK;
}

int nk_model_get(nk_ctx* ctx, const nk_model* mdl, char which, double* out, int64_t ldo) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && out, "nk_model_get: null argument");
  const int m = mdl->m, d = mdl->d, p = mdl->p, mp = m + p;
  const double* src = nullptr;
  int64_t lds = 0, rows = 0, cols = 0;
  switch (which) {
    case 'A': src = mdl->A; lds = mp; rows = m; cols = m; break;
    case 'B': src = mdl->B; lds = mp; rows = m; cols = p; break;
    case 'C': src = mdl->C; lds = m; rows = d; cols = m; break;
    case 'W': src = mdl->W; lds = mp; rows = d; cols = mp; break;
    case 'S': src = mdl->S; lds = m; rows = m; cols = m; break;
    case 'I': src = mdl->Sinv; lds = m; rows = m; cols = m; break;
  }
  if ((which == 'S' || which == 'I') && mdl->kind == NK_MODEL_SPLINE) {
    set_error("nk_model_get: a spline model has no K_mm^{1/2} / K_mm^{-1/2} ('%c')", which);
    return NK_ERR_BAD_ARG;
  }
  switch (which) {
    case 'A': case 'B': case 'C': case 'W': case 'S': case 'I': break;
    case 'Z': src = mdl->Z; lds = d; rows = m; cols = d; break;
    default: set_error("nk_model_get: unknown selector '%c'", which); return NK_ERR_BAD_ARG;
  }
  if ((which == 'A' || which == 'B' || which == 'C' || which == 'W') && !mdl->has_ops) {
    set_error("nk_model_get: model holds no fitted operators");
    return NK_ERR_BAD_ARG;
  }
  if (rows == 0 || cols == 0) return NK_OK;
  NK_REQUIRE(ldo >= cols, "nk_model_get: leading dimension too small");
  NK_HIP(hipMemcpy2DAsync(out, (size_t)ldo * 8, src, (size_t)lds * 8, (size_t)cols * 8, (size_t)rows,
                          is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_model_get_ops(nk_ctx* ctx, const nk_model* mdl, double* G, int64_t ldg, double* Cm, int64_t ldc, double* W,
                     int64_t ldw) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl != nullptr, "nk_model_get_ops: null model");
  if (!mdl->has_ops) {
    set_error("nk_model_get_ops: model holds no fitted operators");
    return NK_ERR_BAD_ARG;
  }
  const int m = mdl->m, d = mdl->d, mp = m + mdl->p;
  NK_REQUIRE((!G || ldg >= mp) && (!Cm || ldc >= m) && (!W || ldw >= mp), "nk_model_get_ops: leading dimension too small");
  // the big block on one stream, the two small ones on another: two DMA engines work at once
  if (G) NK_HIP(copy_ops_block(G, ldg, mdl->A, mp, m, mp, ctx->stream_main));
  if (Cm) NK_HIP(copy_ops_block(Cm, ldc, mdl->C, m, d, m, ctx->stream_side));
  if (W) NK_HIP(copy_ops_block(W, ldw, mdl->W, mp, d, mp, ctx->stream_side));
  NK_HIP(hipStreamSynchronize(ctx->stream_side));
  NK_HIP(hipStreamSynchronize(ctx->stream_main));
  return NK_OK;
}

int nk_model_get_ops_async(nk_ctx* ctx, nk_model* mdl, double* G, int64_t ldg, double* Cm, int64_t ldc, double* W,
                           int64_t ldw) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl != nullptr, "nk_model_get_ops_async: null model");
  if (!mdl->has_ops) {
    set_error("nk_model_get_ops_async: model holds no fitted operators");
    return NK_ERR_BAD_ARG;
  }
  const int m = mdl->m, d = mdl->d, mp = m + mdl->p;
  NK_REQUIRE((!G || ldg >= mp) && (!Cm || ldc >= m) && (!W || ldw >= mp),
             "nk_model_get_ops_async: leading dimension too small");
  NK_TRY(nk_model_wait(mdl));  // one fetch in flight per model
  // everything that produced the operators was synchronised by the producing call (fit / model_create)
  if (G) NK_HIP(copy_ops_block(G, ldg, mdl->A, mp, m, mp, ctx->stream_copy));
  if (Cm) NK_HIP(copy_ops_block(Cm, ldc, mdl->C, m, d, m, ctx->stream_copy));
  if (W) NK_HIP(copy_ops_block(W, ldw, mdl->W, mp, d, mp, ctx->stream_copy));
  if (ctx_recording(ctx)) {
    // member of a lock-step group: the copies above were RECORDED in this member's sequence and no event exists that
    // another thread could wait on, so the fetch completes here (one flush), and nothing is left pending on the model
    NK_HIP(hipStreamSynchronize(ctx->stream));
    return NK_OK;
  }
  hipEvent_t ev = nullptr;
  NK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, ctx->stream_copy);
  if (e != hipSuccess) {
    (void)hipEventDestroy(ev);
    (void)hipStreamSynchronize(ctx->stream_copy);
    set_error("hipEventRecord failed: %s", hipGetErrorString(e));
    return NK_ERR_HIP;
  }
  mdl->ev_fetch = ev;
  return NK_OK;
}

int nk_model_wait(nk_model* mdl) {
  NK_REQUIRE(mdl != nullptr, "nk_model_wait: null model");
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_models.count(mdl) == 0) return NK_OK;  // released by nk_shutdown (which waited for the fetch itself)
  }
  return model_wait_unchecked(mdl);
}

static int model_wait_unchecked(nk_model* mdl) {
  if (mdl->ev_fetch) {
    // the REAL wait, whatever context the calling thread last used: a pending fetch is always a recorded event on a
    // copy stream (fetches by group members complete inside nk_model_get_ops_async), so this must not be turned into a
    // round barrier of the caller's group
    hipError_t e = real_event_sync(mdl->ev_fetch);
    (void)hipEventDestroy(mdl->ev_fetch);
    mdl->ev_fetch = nullptr;
    if (e != hipSuccess) {
      set_error("hipEventSynchronize failed: %s", hipGetErrorString(e));
      return NK_ERR_HIP;
    }
  }
  return NK_OK;
}

}  // extern "C"
