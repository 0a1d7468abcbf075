// Open-loop forecast error of validate_dyn_sys (benchmark_lqr_cloth.py:33-34, benchmark_lqr_classic.py:39) reduced on the
// device: for every trajectory b of a batch,  sse = sum_{t,r} (x_true[b][t][r] - (C z_t)[r])^2  and  ssim = sum_{t,r} (C z_t)[r]^2
// from the lifted states Zall ([b][t][m]) the recursion left in the arena.  The batch*T x d product C z never goes to memory:
// it replaces the product with C, the copy of the trajectory to the host and the host reduction of a scored rollout.
//
// One workgroup of 4 waves per (trajectory, tile of `tt` <= 8 time steps).  The tile's z rows are parked in LDS (tt * m
// doubles, at most 32 KB: tt = min(8, 4096 / m), a function of m alone).  Wave w takes the rows r = w, w + 4, ... of C:
// the 64 lanes stride over the columns of the row (coalesced 512-byte segments of C, conflict-free LDS reads of z), one
// load of C feeds the tt dot products of the tile, each is summed over the wave in a fixed order (wave_sum64_dpp: the total
// lands in every lane) and lane 0 folds it into the wave's two running sums in (r, t) order.  The four waves' pairs are added in wave order and
// written as ONE partial pair per workgroup with ordinary stores; a second tiny launch adds the partials of a trajectory
// in tile order.  No atomics: sse / ssim of a trajectory depend on (T, m, d) and the data only -- not on the batch, the
// grid, or whether the launch was merged with those of other lock-step members (NK_BATCHED_TWIN: same body).
#include "nk_common.h"

namespace nk {

// (TERR_TT steps per tile at most, TERR_LDS_DOUBLES of z rows per workgroup, traj_err_tile: nk_chain_plan.h)
constexpr int TERR_WAVES = 4;

__device__ __forceinline__ void traj_err_partial_kernel_body(const double* __restrict__ Zall, int64_t z_stride,
                                                             const double* __restrict__ Cop, int64_t ldc,
                                                             const double* __restrict__ Xtrue, int64_t x_stride, int m,
                                                             int d, int T, int tt, double* __restrict__ partial) {
  __shared__ double zs[TERR_LDS_DOUBLES];
  __shared__ double wsum[TERR_WAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, b = blockIdx.y, ntiles = gridDim.x;
  const int t0 = tile * tt;
  const int steps = min(tt, T - t0);  // >= 1 by the grid
  const double* z = Zall + (int64_t)b * z_stride + (int64_t)t0 * m;  // the tile's rows are contiguous: steps * m doubles
  for (int e = tid; e < steps * m; e += 64 * TERR_WAVES) zs[e] = z[e];
  __syncthreads();
  const double* xt = Xtrue + (int64_t)b * x_stride + (int64_t)t0 * d;
  double sse = 0.0, ssim = 0.0;  // kept by lane 0
  for (int r = wave; r < d; r += TERR_WAVES) {
    const double* c = Cop + (int64_t)r * ldc;
    double acc[TERR_TT];
#pragma unroll
    for (int t = 0; t < TERR_TT; ++t) acc[t] = 0.0;
    for (int k = lane; k < m; k += 64) {
      const double cv = c[k];
#pragma unroll
      for (int t = 0; t < TERR_TT; ++t)
        if (t < steps) acc[t] = fma(cv, zs[t * m + k], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < TERR_TT; ++t) {
      if (t < steps) {  // uniform over the workgroup
        const double y = wave_sum64_dpp(acc[t]);
        if (lane == 0) {
          const double df = xt[(int64_t)t * d + r] - y;
          sse = fma(df, df, sse);
          ssim = fma(y, y, ssim);
        }
      }
    }
  }
  if (lane == 0) { wsum[wave][0] = sse; wsum[wave][1] = ssim; }
  __syncthreads();
  if (tid == 0) {
    double* out = partial + ((int64_t)b * ntiles + tile) * 2;
    out[0] = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
    out[1] = ((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1];
  }
}
__global__ void __launch_bounds__(64 * TERR_WAVES) traj_err_partial_kernel(const double* __restrict__ Zall, int64_t z_stride, const double* __restrict__ Cop, int64_t ldc, const double* __restrict__ Xtrue, int64_t x_stride, int m, int d, int T, int tt, double* __restrict__ partial) { traj_err_partial_kernel_body(Zall, z_stride, Cop, ldc, Xtrue, x_stride, m, d, T, tt, partial); }
NK_BATCHED_TWIN(traj_err_partial_kernel, (64 * TERR_WAVES), const double*, int64_t, const double*, int64_t, const double*, int64_t, int, int, int, int, double*)

// out[b] = (sse, ssim) = the partial pairs of trajectory b added in tile order; one thread per trajectory
__device__ __forceinline__ void traj_err_sum_kernel_body(const double* __restrict__ partial, int ntiles, int batch,
                                                         double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const double* p = partial + (int64_t)b * ntiles * 2;
  double sse = 0.0, ssim = 0.0;
  for (int i = 0; i < ntiles; ++i) { sse += p[2 * i]; ssim += p[2 * i + 1]; }
  out[2 * b] = sse;
  out[2 * b + 1] = ssim;
}
__global__ void __launch_bounds__(64) traj_err_sum_kernel(const double* __restrict__ partial, int ntiles, int batch, double* __restrict__ out) { traj_err_sum_kernel_body(partial, ntiles, batch, out); }
NK_BATCHED_TWIN(traj_err_sum_kernel, (64), const double*, int, int, double*)

// out: batch x 2 doubles (device-visible).  Zall: [b][t][m] with trajectory stride z_stride, Xtrue: [b][t][d] with stride x_stride.
int launch_traj_err(nk_ctx* ctx, const double* Zall, int64_t z_stride, const double* Cop, int64_t ldc, const double* Xtrue,
                    int64_t x_stride, int m, int d, int T, int batch, double* out) {
  const int tt = traj_err_tile(m);
  NK_REQUIRE(tt >= 1, "open-loop error: m = %d is outside 1..%d", m, TERR_LDS_DOUBLES);
  NK_REQUIRE(d >= 1 && T >= 1 && batch >= 1 && batch <= 65535, "open-loop error: bad sizes (d=%d T=%d batch=%d)", d, T, batch);
  NK_REQUIRE(z_stride >= (int64_t)T * m && x_stride >= (int64_t)T * d && ldc >= m, "open-loop error: strides too small");
  const int ntiles = (T + tt - 1) / tt;
  double* partial = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)batch * ntiles * 2, &partial));
  hipLaunchKernelGGL(traj_err_partial_kernel, dim3((unsigned)ntiles, (unsigned)batch), dim3(64 * TERR_WAVES), 0, ctx->stream,
                     Zall, z_stride, Cop, ldc, Xtrue, x_stride, m, d, T, tt, partial);
  hipLaunchKernelGGL(traj_err_sum_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, ctx->stream, partial, ntiles,
                     batch, out);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
