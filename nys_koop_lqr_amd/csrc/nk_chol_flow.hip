// Blocked Cholesky of up to two augmented systems (cholesky_aug_pair_async's contract: an m x m SPD block plus `extra`
// right-hand-side rows) in ONE launch: a tile-dataflow factorisation.
//
// The launch-per-step chain (nk_chol.hip) runs 32 dependent block steps at m = 2000, each a diagonal factor, a panel launch
// and a trailing update that ends only when its slowest tile is done -- about 97 us per step against a few us of arithmetic.
// Here the work is the set of 64 x 64 tiles (i, k), i >= k, of the factor, each owned by one workgroup from start to end,
// LEFT-LOOKING:
//   C(i,k) -= P(i,j) P(k,j)^T   for j = 0 .. k-1 in ascending order (each product from zero, then subtracted),
// then the diagonal tile is factored and inverted (potrf_diag_kernel_body, one wave) or the tile below it is panel-solved
// (chol_panel_rows).  Per element that is the arithmetic of the chain in the same order -- the trailing updates of the chain
// reach an element in ascending step order too, and each is the same sequence of v_mfma_f64_16x16x4 (contraction index
// dealt as k = 32 h + 8 l4 + ks, (h, ks) order: chol_trail_kernel_body) -- so the factor, the extra rows, the diagonal
// workspaces, the pivots and the failure flag come out bit-identical.  The tile under the diagonal, (k, k-1), is computed by
// the workgroup that owns (k, k): per block step the critical path is the diagonal factor, one hand-off, that panel, one
// update.
//
// Work items are taken by an atomic ticket in an order in which every dependency of an item has a lower ticket: diagonal
// item 0, then for c = 0, 1, ...: diagonal item c + 1, then the items of column c (square rows c + 2 .., then the extra
// rows), for both systems.  A lower ticket is held by a workgroup that is already running, so the launch makes progress at
// any residency and dispatch order.  Hand-offs are agent-scope release (producer) / acquire (consumer) around one flag word
// per tile; flags, the ticket and the status word are zeroed by a memset in the same stream ahead of the launch.  Every
// wait is bounded: a workgroup that gives up sets the status word (everyone else then stops waiting) and marks the failure
// flag of every system of the launch with CHOL_FLOW_GIVEUP; the host then re-runs the factorisation on the launch-per-step
// chain (cholesky_aug_pair_async's callers).
#include <cstdio>
#include <cstdlib>

#include "nk_common.h"
#include "nk_chol.h"
#include "nk_panel_body.h"
#include "nk_potrf_body.h"

namespace nk {

namespace {

constexpr int FLOW_THREADS = 256;
constexpr int FLOW_POLL_LIMIT = 1 << 22;     // polls of one wait (~0.5 us each: seconds -- a genuine hang, nothing else)

struct FlowSys {
  double* P;
  int64_t ldp;
  int m, extra;
  double* Linv;
  double* pivlog;
  int* info;
  unsigned long long* piv;
  int* flags;  // (nblk + nex) x nblk words: tile (i, k) is final
  int nblk;    // block columns = square tile rows
  int nex;     // tile rows of the extra rows
};
struct FlowArgs {
  FlowSys s[2];
  int nsys;
  int total;  // work items
  int fix;
  int test_giveup;  // test hook (NYSKOOP_CHOL_FLOW_TEST_GIVEUP): the workgroup that draws this ticket gives up; -1: none
  int* hdr;
};

__device__ __forceinline__ int ld_flag(const int* f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// items of system q in column c (square rows c + 2 .. nblk - 1, then the extra rows)
__device__ __forceinline__ int col_items(const FlowSys& s, int c) {
  if (c < 0 || c >= s.nblk) return 0;
  return max(0, s.nblk - c - 2) + s.nex;
}

// ticket t -> system q, tile row i, block column k (i == k: the diagonal item, which also produces tile (k, k-1))
__device__ void item_of(const FlowArgs& a, int t, int& q, int& i, int& k) {
  for (int g = 0;; ++g) {
    for (int p = 0; p < a.nsys; ++p)  // diagonal items of group g
      if (g < a.s[p].nblk) {
        if (t == 0) { q = p; i = k = g; return; }
        --t;
      }
    for (int p = 0; p < a.nsys; ++p) {  // column g - 1
      const int n = col_items(a.s[p], g - 1);
      if (t < n) {
        q = p; k = g - 1;
        const int nsq = max(0, a.s[p].nblk - k - 2);
        i = t < nsq ? k + 2 + t : a.s[p].nblk + (t - nsq);
        return;
      }
      t -= n;
    }
  }
}

// rows [r0, r1) of tile row i, columns [c0, c1) of block column k
__device__ __forceinline__ void tile_rows(const FlowSys& s, int i, int& r0, int& r1) {
  if (i < s.nblk) { r0 = CHOL_NB * i; r1 = min(r0 + CHOL_NB, s.m); }
  else { r0 = s.m + CHOL_NB * (i - s.nblk); r1 = min(r0 + CHOL_NB, s.m + s.extra); }
}

// This wave's 32 x 32 quarter of a tile: C[a][b][reg] = element (rw + 16 a + l4 + 4 reg, cw + 16 b + l15).
typedef d4 Quarter[2][2];

__device__ __forceinline__ void load_quarter(const FlowSys& s, int r0, int r1, int c0, int c1, int wm, int wn, int l15, int l4,
                                             Quarter& C) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = r0 + 32 * wm + 16 * a + l4 + 4 * reg, col = c0 + 32 * wn + 16 * b + l15;
        C[a][b][reg] = (row < r1 && col < c1) ? s.P[(int64_t)row * s.ldp + col] : 0.0;
      }
}
__device__ __forceinline__ void store_quarter(const FlowSys& s, int r0, int r1, int c0, int c1, int wm, int wn, int l15, int l4,
                                              const Quarter& C) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = r0 + 32 * wm + 16 * a + l4 + 4 * reg, col = c0 + 32 * wn + 16 * b + l15;
        if (row < r1 && col < c1) s.P[(int64_t)row * s.ldp + col] = C[a][b][reg];
      }
}

// C -= P(rows r0.., block j) P(rows c0.., block j)^T: the accumulator from zero, the contraction index dealt and ordered exactly
// as in chol_trail_kernel_body (rows past r1 / c1 are clamped: they only feed entries that are never stored)
__device__ __forceinline__ void update_quarter(const FlowSys& s, int r0, int r1, int c0, int c1, int j, int wm, int wn, int l15,
                                               int l4, Quarter& C) {
  const double* pa[2];
  const double* pb[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    pa[a] = s.P + (int64_t)min(r0 + 32 * wm + 16 * a + l15, r1 - 1) * s.ldp + CHOL_NB * j + 8 * l4;
    pb[a] = s.P + (int64_t)min(c0 + 32 * wn + 16 * a + l15, c1 - 1) * s.ldp + CHOL_NB * j + 8 * l4;
  }
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double x[2][8], y[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        x[a][ks] = pa[a][32 * h + ks];
        y[a][ks] = pb[a][32 * h + ks];
      }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[a][ks], y[b][ks], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) C[a][b][reg] -= acc[a][b][reg];
  asm volatile("" ::: "memory");  // (keeps the next update's loads behind this one: registers for one update at a time)
}

// Give up: the status word stops every other wait of the launch, and the failure flag of EVERY system of the launch tells the
// host (the other waits leave their tiles unfinished too, whichever system they belong to).  A flag that already holds a
// non-positive pivot is overwritten: the host re-runs the factorisation on the launch-per-step chain, which finds it again.
__device__ __forceinline__ void give_up(const FlowArgs& a) {
  __hip_atomic_store(a.hdr + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int q = 0; q < a.nsys; ++q) atomicExch(a.s[q].info, CHOL_FLOW_GIVEUP);
}

// Wait (whole workgroup) until tiles (ia, j) and (ib, j) are final for j = jlo .. J-1, J > jlo as large as the flags allow
// (<= jhi); ib < 0: only (ia, j).  One wave polls (lane = j - jlo), relaxed; lane 0 then acquires at agent scope for the
// workgroup.  Returns J, or -1 when the launch gave up.
__device__ int wait_tiles(const FlowArgs& a, const FlowSys& s, int ia, int ib, int jlo, int jhi, int* sh) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int res = -1;
    for (int polls = 0;; ++polls) {
      const int j = jlo + lane;
      bool ok = true;
      if (j < jhi) {
        ok = ld_flag(s.flags + ia * s.nblk + j) != 0;
        if (ib >= 0) ok = ok && ld_flag(s.flags + ib * s.nblk + j) != 0;
      }
      const unsigned long long ready = __ballot(ok);
      const int run = ~ready == 0ull ? 64 : __builtin_ctzll(~ready);
      if (run > 0) { res = min(jlo + run, jhi); break; }
      if (ld_flag(a.hdr + 1) != 0) break;
      if (polls >= FLOW_POLL_LIMIT) {
        if (lane == 0) give_up(a);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (lane == 0) {
      if (res > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      sh[0] = res;
    }
  }
  __syncthreads();
  const int r = sh[0];
  __syncthreads();  // (sh is reused by the next wait)
  return r;
}

// Tile (i, k) is final: every wave's stores drained, one agent-scope release, the flag by a vector atomic store.
__device__ __forceinline__ void publish(const FlowSys& s, int i, int k) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(s.flags + i * s.nblk + k, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the whole workgroup's stores are visible to its own later loads (one CU, one L1)
__device__ __forceinline__ void local_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__device__ __forceinline__ void panel_tile(const FlowArgs& a, const FlowSys& s, int r0, int r1, int k, int wave, int lane) {
  PanelSys ps;
  ps.P = s.P + (int64_t)r0 * s.ldp + CHOL_NB * k;
  ps.ldp = s.ldp;
  ps.Linv = s.Linv + (size_t)k * CHOL_WS;
  ps.rows = r1 - r0;
  ps.nb = min(CHOL_NB, s.m - CHOL_NB * k);
  ps.fix = a.fix;
  ps.nblocks = 1;
  chol_panel_rows(ps, 16 * wave, lane);
  __builtin_amdgcn_s_setprio(0);  // (the panel body raises it for the chain; polls and updates run at the default)
}

// The diagonal factor of block k (one wave), out of line: inlined, its unrolled body and the item loop around it would need
// more registers together than a workgroup of this kernel may take beside a GEMM workgroup on the same CU.
__device__ __noinline__ void flow_potrf(double* A, int64_t lda, int nb, double* Linv, int* info, unsigned long long* piv,
                                       double* plog, int blk, int lane) {
  PotrfBatch pb;
  pb.A[0] = A; pb.lda[0] = lda; pb.nb[0] = nb; pb.Linv[0] = Linv; pb.info[0] = info; pb.piv[0] = piv; pb.plog[0] = plog;
  pb.A[1] = nullptr; pb.lda[1] = 0; pb.nb[1] = 0; pb.Linv[1] = nullptr; pb.info[1] = nullptr; pb.piv[1] = nullptr;
  pb.plog[1] = nullptr;
  potrf_diag_kernel_body<true>(pb, blk, 0, lane);
  __builtin_amdgcn_s_setprio(0);
}

__global__ void __launch_bounds__(FLOW_THREADS) chol_flow_kernel(FlowArgs a) {
  __shared__ int sh[4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  for (;;) {
    if (threadIdx.x == 0) sh[1] = atomicAdd(a.hdr, 1);
    __syncthreads();
    const int t = sh[1];
    __syncthreads();
    if (t >= a.total) return;
    if (t == a.test_giveup) {  // test hook: the give-up branch itself, taken at once (nobody waits for it: the status word is up)
      if (threadIdx.x == 0) give_up(a);
      return;
    }
    int q = 0, i = 0, k = 0;
    item_of(a, t, q, i, k);
    const FlowSys s = q ? a.s[1] : a.s[0];
    int r0, r1;
    tile_rows(s, i, r0, r1);
    const int c0 = CHOL_NB * k, c1 = min(c0 + CHOL_NB, s.m);
    if (i == k) {
      // ---- diagonal item: tile (k, k-1) first (updates, panel solve, publish), then tile (k, k) (updates, factor, publish)
      if (k > 0) {
        const int p0 = c0 - CHOL_NB;  // block column k - 1 (full)
        Quarter Cp, Cd;
        load_quarter(s, r0, r1, p0, c0, wm, wn, l15, l4, Cp);
        load_quarter(s, r0, r1, c0, c1, wm, wn, l15, l4, Cd);
        bool ok = true;
        for (int j = 0; j < k - 1 && ok;) {
          const int J = wait_tiles(a, s, k, k - 1, j, k - 1, sh);
          if (J < 0) { ok = false; break; }
          for (; j < J; ++j) {
            update_quarter(s, r0, r1, p0, c0, j, wm, wn, l15, l4, Cp);
            update_quarter(s, r0, r1, c0, c1, j, wm, wn, l15, l4, Cd);
          }
        }
        if (!ok) continue;
        // (both tiles go out: the panel solve needs every register of the wave)
        store_quarter(s, r0, r1, p0, c0, wm, wn, l15, l4, Cp);
        store_quarter(s, r0, r1, c0, c1, wm, wn, l15, l4, Cd);
        local_sync();
        if (wait_tiles(a, s, k - 1, -1, k - 1, k, sh) < 0) continue;  // diagonal block k - 1 (its inverse)
        panel_tile(a, s, r0, r1, k - 1, wave, lane);
        publish(s, k, k - 1);
        __syncthreads();
        load_quarter(s, r0, r1, c0, c1, wm, wn, l15, l4, Cd);
        update_quarter(s, r0, r1, c0, c1, k - 1, wm, wn, l15, l4, Cd);
        store_quarter(s, r0, r1, c0, c1, wm, wn, l15, l4, Cd);
        local_sync();
      }
      if (wave == 0)
        flow_potrf(s.P + (int64_t)c0 * s.ldp + c0, s.ldp, c1 - c0, s.Linv + (size_t)k * CHOL_WS, s.info, s.piv,
                   s.pivlog ? s.pivlog + c0 : nullptr, k, lane);
      publish(s, k, k);
      __syncthreads();
    } else {
      // ---- tile (i, k) below the diagonal: updates, then the panel solve once diagonal block k is out
      if (k > 0) {
        Quarter C;
        load_quarter(s, r0, r1, c0, c1, wm, wn, l15, l4, C);
        bool ok = true;
        for (int j = 0; j < k && ok;) {
          const int J = wait_tiles(a, s, i, k, j, k, sh);
          if (J < 0) { ok = false; break; }
          for (; j < J; ++j) update_quarter(s, r0, r1, c0, c1, j, wm, wn, l15, l4, C);
        }
        if (!ok) continue;
        store_quarter(s, r0, r1, c0, c1, wm, wn, l15, l4, C);
        local_sync();
      }
      if (wait_tiles(a, s, k, -1, k, k + 1, sh) < 0) continue;
      panel_tile(a, s, r0, r1, k, wave, lane);
      publish(s, i, k);
      __syncthreads();
    }
  }
}

}  // namespace

bool chol_flow_enabled() {  // NYSKOOP_CHOL_FLOW=0 (read per call): the launch-per-step chain, for A/B runs and the bit-identity test
  const char* e = getenv("NYSKOOP_CHOL_FLOW");
  return !(e && e[0] == '0');
}

// NYSKOOP_CHOL_FLOW_TEST_GIVEUP=<ticket>[,<nsys>[,<extra>]] (read per call; tests/): the workgroup that draws work item
// <ticket> of a dataflow launch takes the give-up branch instead of working on it, every other workgroup leaves through the
// status word, and the caller's recovery runs.  <nsys> / <extra> (0 or absent: any) restrict the hook to launches of that many
// systems / whose first system has that many extra rows (the K_mm launch of a fit has one system, the regularised pair
// two).  Tickets outside the launch are ignored.  Returns -1 when the hook is not set or does not apply.
static int flow_test_giveup(const CholSys* sys, int nsys, int total) {
  const char* e = getenv("NYSKOOP_CHOL_FLOW_TEST_GIVEUP");
  if (!e || !e[0]) return -1;
  long ticket = -1, want_nsys = 0, want_extra = 0;
  if (sscanf(e, "%ld,%ld,%ld", &ticket, &want_nsys, &want_extra) < 1) return -1;
  if (want_nsys > 0 && want_nsys != nsys) return -1;
  if (want_extra > 0 && want_extra != sys[0].extra) return -1;
  return (ticket >= 0 && ticket < total) ? (int)ticket : -1;
}

// The factorisation part of cholesky_aug_pair_async as one launch (after reset_pivots; the caller queues the backward pass).
int cholesky_flow_pair(nk_ctx* ctx, const CholSys* sys, int nsys) {
  NK_REQUIRE(nsys >= 1 && nsys <= 2, "cholesky_flow_pair: 1..2 systems");
  FlowArgs a;
  memset(&a, 0, sizeof(a));
  a.nsys = nsys;
  a.fix = chol_fix_enabled();
  int ms[2] = {0, 0}, extras[2] = {0, 0};
  CholFlowCounts fc[2];
  for (int q = 0; q < nsys; ++q) {
    const CholSys& y = sys[q];
    fc[q] = chol_flow_counts(y.m, y.extra);
    FlowSys& s = a.s[q];
    s.P = y.P; s.ldp = y.ldp; s.m = y.m; s.extra = y.extra; s.Linv = y.Linv; s.pivlog = y.pivlog;
    s.info = ctx->d_info + info_base(ctx) + q;
    s.piv = ctx->d_piv + 2 * (info_base(ctx) + q);
    s.nblk = fc[q].nblk;
    s.nex = fc[q].nex;
    ms[q] = y.m; extras[q] = y.extra;
  }
  const size_t words = chol_flow_words(ms, extras, nsys);
  a.total = chol_flow_items(ms, extras, nsys);
  // flag words of this stream's slot (persistent: no allocation in steady state)
  const int slot = info_base(ctx) / 2;
  if (ctx->flow_words[slot] < words) {
    if (ctx->d_flow[slot]) NK_HIP(hipFree(ctx->d_flow[slot]));
    ctx->d_flow[slot] = nullptr;
    ctx->flow_words[slot] = 0;
    NK_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->d_flow[slot]), words * sizeof(int)));
    ctx->flow_words[slot] = words;
  }
  a.test_giveup = flow_test_giveup(sys, nsys, a.total);
  a.hdr = ctx->d_flow[slot];
  int* f = a.hdr + CHOL_FLOW_HDR;
  for (int q = 0; q < nsys; ++q) {
    a.s[q].flags = f;
    f += fc[q].flags;
  }
  NK_HIP(hipMemsetAsync(a.hdr, 0, words * sizeof(int), ctx->stream));
  // Half the CUs, one workgroup on each: the launch is latency bound (the diagonal chain), a workgroup of it (320 VGPRs)
  // leaves room on its CU for one GEMM workgroup (the square-root iteration beside the pair chain), and the two chains of a
  // fit (prep and main stream) run side by side instead of one waiting for CUs the other holds.  A caller that knows what
  // runs beside the launch may ask for another width (nk::FlowWidth; same bits at any width).
  const int width = ctx->chol_flow_wgs > 0 ? ctx->chol_flow_wgs : ctx->num_cu / 2;
  const int grid = std::max(1, std::min(a.total, width));
  hipLaunchKernelGGL(chol_flow_kernel, dim3((unsigned)grid), dim3(FLOW_THREADS), 0, ctx->stream, a);
  NK_HIP(hipGetLastError());
  count_event(CNT_CHOL_FLOW);
  return NK_OK;
}

}  // namespace nk
