// Trailing update of one step of the blocked Cholesky (nk_chol.hip: cholesky_aug_pair_async):
//     C[tm, tn] -= P[tm] P[tn]^T      P = the 64-column panel of this step (rows x 64, row-major, k contiguous),
// lower tiles of the square part plus full tiles for the extra (right-hand-side) rows, for up to two systems in one
// launch.  The generic engine (nk_gemm.hip) walks K in register-staged, barrier-separated steps of 16 -- with K = 64 it
// never reaches a steady state (50 us per launch alone, ~90 us beside the square-root GEMMs, 32 launches on the critical
// path of a fit).  Here a workgroup takes both 128 x 64 panel blocks of its tile straight from global memory into
// registers in two halves of K (each lane owns 8 contiguous doubles of its rows: the contraction index is dealt to the
// lane groups, any assignment works as long as both operands use the same one), multiplies on the matrix pipe
// (4 waves x 4 x 4 tiles of v_mfma_f64_16x16x4) and read-modify-writes the 128 x 128 tile of C.  No LDS, no barriers.
#include "nk_common.h"
#include "nk_chol.h"
#include "nk_potrf_body.h"
#include "nk_panel_body.h"

namespace nk {

__device__ __forceinline__ void chol_trail_kernel_body(const TrailBatch& tb) {
  const TrailSys s = tb.s[blockIdx.y];
  if ((int)blockIdx.x >= s.nblocks) return;
  __builtin_amdgcn_s_setprio(2);  // latency-bound chain beside the GEMM-bound side stream
  // tile (tm, tn): tile row r of the lower set holds min(r + 1, tiles_n) tiles (rows past the square part are full)
  int tm = 0, tn = 0;
  {
    int rem = blockIdx.x;
    for (;;) {
      const int cnt = tm + 1 < s.tiles_n ? tm + 1 : s.tiles_n;
      if (rem < cnt) break;
      rem -= cnt;
      ++tm;
    }
    tn = rem;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int m0 = tm * 128 + wm * 64, n0 = tn * 128 + wn * 64;
  // In a 128-tile on the diagonal the 64 x 64 quarter of wave (0, 1) lies strictly above the block diagonal of the factor:
  // nothing reads it, and nk_chol_aug promises that such tiles return the input (the dataflow launch never touches them)
  if (tm == tn && wm == 0 && wn == 1) return;

  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

  // operand rows of this lane (clamped: rows past the end only feed accumulator entries that are never stored)
  const double* pa[4];
  const double* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pa[i] = s.P + (int64_t)min(m0 + 16 * i + l15, s.rows - 1) * s.ldp + 8 * l4;
    pb[i] = s.P + (int64_t)min(n0 + 16 * i + l15, s.rem - 1) * s.ldp + 8 * l4;  // column c of C <-> panel row c
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // k in [32 h, 32 h + 32): lane group l4 owns k = 32 h + 8 l4 .. + 7
    double a[4][8], b[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        a[i][ks] = pa[i][32 * h + ks];
        b[i][ks] = pb[i][32 * h + ks];
      }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][ks], b[j][ks], acc[i][j], 0, 0, 0);
  }
  // C -= acc: lane holds rows (l4 + 4 reg) of column l15 of each 16 x 16 tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = m0 + 16 * i + l4 + 4 * reg;
        const int col = n0 + 16 * j + l15;
        if (row < s.rows && col < s.rem) {
          double* c = s.C + (int64_t)row * s.ldc + col;
          *c -= acc[i][j][reg];
        }
      }
}
__global__ void __launch_bounds__(256) chol_trail_kernel(TrailBatch tb) { chol_trail_kernel_body(tb); }
NK_BATCHED_TWIN_REF(chol_trail_kernel, (256), TrailBatch)

// workgroups of a launch: the larger of the two slots (blockIdx.y selects the slot; workgroups past a slot's count leave)
template <typename Batch>
static unsigned pair_workgroups(const Batch& b) {
  return (unsigned)(b.s[0].nblocks > b.s[1].nblocks ? b.s[0].nblocks : b.s[1].nblocks);
}

int launch_chol_trail_pair(nk_ctx* ctx, const TrailBatch& tb) {
  const unsigned wgs = pair_workgroups(tb);
  if (wgs == 0) return NK_OK;
  hipLaunchKernelGGL(chol_trail_kernel, dim3(wgs, 2), dim3(256), 0, ctx->stream, tb);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Trailing update of step j AND the diagonal-block factorisation of step j + 1 in one launch.  The next diagonal block is the
// 64 x 64 sub-tile of wave 0 of workgroup 0: as soon as that wave has written it back, it factors and inverts it
// (potrf_diag_kernel_body, one wave) while the other workgroups are still on their tiles -- the ~30 us of the diagonal
// kernel leave the critical path wherever the trailing update takes as long, and every block step loses one of its three
// kernel boundaries.  Same arithmetic in the same order as the two separate launches: bit-identical results
// (NYSKOOP_CHOL_FUSE=0 issues them separately).
// ---------------------------------------------------------------------------------------------------------------
// The diagonal body takes the wave-level sync (potrf_sync<true>): its LDS arrays are touched by this one wave only, the
// __threadfence() in front of it orders the wave's own global stores of the block before its loads, and the workgroup's other
// waves need nothing from it -- they run to the end of their tiles and leave, at whatever time.
__device__ __forceinline__ void chol_trail_potrf_kernel_body(const TrailBatch& tb, const PotrfBatch& pb, int blk) {
  chol_trail_kernel_body(tb);
  if (blockIdx.x == 0 && __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0 && pb.nb[blockIdx.y] > 0) {
    __threadfence();  // this wave's own stores of the block are visible to its loads (another lane layout) below
    potrf_diag_kernel_body<true>(pb, blk, blockIdx.y, threadIdx.x & 63);
  }
}
__global__ void __launch_bounds__(256) chol_trail_potrf_kernel(TrailBatch tb, PotrfBatch pb, int blk) { chol_trail_potrf_kernel_body(tb, pb, blk); }
NK_BATCHED_TWIN_REF(chol_trail_potrf_kernel, (256), TrailBatch, PotrfBatch, int)

int launch_chol_trail_potrf_pair(nk_ctx* ctx, const TrailBatch& tb, const PotrfBatch& pb, int blk) {
  const unsigned wgs = pair_workgroups(tb);
  if (wgs == 0) return NK_OK;
  hipLaunchKernelGGL(chol_trail_potrf_kernel, dim3(wgs, 2), dim3(256), 0, ctx->stream, tb, pb, blk);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// Panel solve of the same step: chol_panel_rows (nk_panel_body.h).
__device__ __forceinline__ void chol_panel_kernel_body(const PanelBatch& pb) {
  const PanelSys s = pb.s[blockIdx.y];
  if ((int)blockIdx.x >= s.nblocks) return;
  // 16 rows per wave, 64 per workgroup: the launch is latency bound (at most 63 workgroups on 256 CUs), so the rows are
  // spread as thin as the 16-row matrix instruction allows
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  chol_panel_rows(s, blockIdx.x * PANEL_ROWS + wave * 16, threadIdx.x & 63);
}
__global__ void __launch_bounds__(256) chol_panel_kernel(PanelBatch pb) { chol_panel_kernel_body(pb); }
NK_BATCHED_TWIN_REF(chol_panel_kernel, (256), PanelBatch)

int launch_chol_panel_pair(nk_ctx* ctx, const PanelBatch& pb) {
  const unsigned wgs = pair_workgroups(pb);
  if (wgs == 0) return NK_OK;
  hipLaunchKernelGGL(chol_panel_kernel, dim3(wgs, 2), dim3(256), 0, ctx->stream, pb);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
