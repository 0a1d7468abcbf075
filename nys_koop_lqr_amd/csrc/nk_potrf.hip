// Diagonal-block Cholesky of the blocked factorisation: the stand-alone launch (body: nk_potrf_body.h).
#include "nk_common.h"
#include "nk_chol.h"
#include "nk_potrf_body.h"

namespace nk {

// one wave per system: the wave is the whole workgroup, so the body's barriers are plain workgroup barriers
__device__ __forceinline__ void potrf_diag_kernel_body(const PotrfBatch& pb, int blk) {
  potrf_diag_kernel_body(pb, blk, blockIdx.x, threadIdx.x);
}
__global__ void __launch_bounds__(64) potrf_diag_kernel(PotrfBatch pb, int blk) { potrf_diag_kernel_body(pb, blk); }
NK_BATCHED_TWIN_REF(potrf_diag_kernel, (64), PotrfBatch, int)

int launch_potrf_diag_pair(nk_ctx* ctx, const PotrfBatch& pb, int blk) {
  hipLaunchKernelGGL(potrf_diag_kernel, dim3(2), dim3(64), 0, ctx->stream, pb, blk);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
