// Matrix square root / inverse square root of a symmetric positive definite matrix, built on the fp64 MFMA GEMM engine:
// through the polar factor of the Cholesky factor (scaled Newton-Schulz, GEMM only; the coupled Newton-Schulz iteration is
// kept as the fallback for numerically singular input), replacing scipy.linalg.sqrtm + solve(assume_a='her')
// (regressors.py:140,152,153,163,175,177).  The step arithmetic of both iterations is nk_sqrt_schedule.h.
#include "nk_common.h"
#include "nk_chol.h"
#include "nk_tn.h"
#include "nk_sqrt_schedule.h"

#include <algorithm>
#include <cmath>

namespace nk {

// ---------------------------------------------------------------------------------------------------------------
// matrix square root: coupled Newton-Schulz  Y <- Y T, Z <- T Z, T = (3I - ZY)/2,  Y0 = P/c, Z0 = I
//   Y -> (P/c)^{1/2}, Z -> (P/c)^{-1/2}.  Only M = ZY is symmetrised (mirrored upper tiles, diagonal tiles averaged with their
//   transposes); symmetrising Y and Z as well was observed to destabilise the iteration, the plain products are stable (see
//   DESIGN.md).
// ---------------------------------------------------------------------------------------------------------------
static int read_scalar(nk_ctx* ctx, const double* d_ptr, double* out) {
  NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_SCRATCH, d_ptr, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  *out = ctx->h_scalars[HS_SCRATCH];
  return NK_OK;
}

// the iterates of the coupled iteration with their true transposes (written by the GEMM epilogues), current and next
struct CoupledBufs {
  double *Y = nullptr, *Z = nullptr, *Yn = nullptr, *Zn = nullptr, *M = nullptr, *T = nullptr;
  double *Yt = nullptr, *Zt = nullptr, *Ytn = nullptr, *Ztn = nullptr;
};

// Y <- Y T, Z <- T Z with their transposes, then the buffers change roles.  Every product is issued as P^T Q with P stored
// contraction-major (fast LDS-DMA engine); Z and Y are only symmetric up to rounding and must NOT be replaced by their
// transposes (that variant diverges), so true transposes are kept alongside (written by the epilogue of the launch that
// produces Y and Z)
static int coupled_products(nk_ctx* ctx, int m, int it, CoupledBufs& b) {
  // Y T and T Z (T is exactly symmetric) share K = m: one fused launch, 2 x 256 tiles = two workgroups per CU
  TnProblem pr[2];
  pr[0].A = b.Yt; pr[0].B = b.T; pr[0].C = b.Yn; pr[0].lda = pr[0].ldb = pr[0].ldc = m; pr[0].M = pr[0].N = m;
  pr[0].Ct = b.Ytn; pr[0].ldct = m;
  pr[1].A = b.T; pr[1].B = b.Z; pr[1].C = b.Zn; pr[1].lda = pr[1].ldb = pr[1].ldc = m; pr[1].M = pr[1].N = m;
  pr[1].Ct = b.Ztn; pr[1].ldct = m;
  if (it == 0) {
    // Z_0 = I: Z_1 = T_0 (symmetric), only Y_0 T_0 needs a GEMM
    if (tn_fast_ok(pr[0]) && m >= 128) {
      NK_TRY(launch_gemm_tn_multi(ctx, pr, 1, m, 0));
    } else {
      NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, b.Yt, m, b.T, m, 0.0, b.Yn, m));
      NK_TRY(launch_transpose(ctx, b.Yn, m, b.Ytn, m, m, m));
    }
    NK_TRY(launch_copy2d(ctx, b.T, m, b.Zn, m, m, m));
    NK_TRY(launch_copy2d(ctx, b.T, m, b.Ztn, m, m, m));
  } else if (tn_fast_ok(pr[0]) && tn_fast_ok(pr[1]) && m >= 128) {
    NK_TRY(launch_gemm_tn_multi(ctx, pr, 2, m, 0));
  } else {
    NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, b.Yt, m, b.T, m, 0.0, b.Yn, m));
    NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, b.T, m, b.Z, m, 0.0, b.Zn, m));
    NK_TRY(launch_transpose(ctx, b.Yn, m, b.Ytn, m, m, m));
    NK_TRY(launch_transpose(ctx, b.Zn, m, b.Ztn, m, m, m));
  }
  std::swap(b.Y, b.Yn);
  std::swap(b.Z, b.Zn);
  std::swap(b.Yt, b.Ytn);
  std::swap(b.Zt, b.Ztn);
  return NK_OK;
}

int sqrtm_spd_coupled(nk_ctx* ctx, const double* P, int64_t ldp, int m, double* S, double* Sinv, int* iters,
                      double* resid) {
  const ArenaMark mk = arena_mark(ctx);
  const size_t mm = (size_t)m * m;
  CoupledBufs b;
  for (double** p : {&b.Y, &b.Z, &b.Yn, &b.Zn, &b.M, &b.T, &b.Yt, &b.Zt, &b.Ytn, &b.Ztn}) NK_TRY(arena_alloc_t(ctx, mm, p));
  double c = 0.0;
  NK_TRY(launch_max_abs_rowsum(ctx, P, ldp, m, ctx->d_scalars + SQ_C));
  NK_TRY(read_scalar(ctx, ctx->d_scalars + SQ_C, &c));
  if (!(c > 0.0) || !std::isfinite(c)) {
    set_error("sqrtm: matrix norm is %g", c);
    arena_release(ctx, mk);
    return NK_ERR_NOT_SPD;
  }
  NK_TRY(launch_axpby2d(ctx, 1.0 / c, P, ldp, 0.0, b.Y, m, m, m));
  NK_TRY(launch_fill(ctx, b.Z, m, m, m, 0.0));
  NK_TRY(launch_add_diag(ctx, b.Z, m, m, 1.0));
  NK_TRY(launch_transpose(ctx, b.Y, m, b.Yt, m, m, m));  // Y_0 = P / c (P symmetric only up to the caller's rounding)
  NK_TRY(launch_copy2d(ctx, b.Z, m, b.Zt, m, m, m));     // Z_0 = I
  // spectrum interval [a, b] of M_0 = Y_0 (ns_interval_estimate), measured on Y_0 = P / c itself
  NK_TRY(launch_sumsq_trace(ctx, b.Y, (int64_t)m, m, ctx->d_scalars + SQ_SUMSQ, ctx->d_scalars + SQ_TRACE));
  NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_SCRATCH, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  double a_lo = ns_interval_estimate(std::sqrt(ctx->h_scalars[HS_SCRATCH + SQ_SUMSQ]), ctx->h_scalars[HS_SCRATCH + SQ_TRACE], m);
  double b_hi = 1.0;
  GemmOpts sym;
  sym.tri = TRI_UPPER_MIRROR;
  const int maxit = NS_MAX_STEPS;
  double r = 1e300, r_prev = 1e300;
  int it = 0;
  bool ok = false;
  for (; it < maxit; ++it) {
    if (it == 0) {
      // Z_0 = I: M_0 = Y_0, taken as (Y_0 + Y_0^T)/2 so that T_0 is exactly symmetric (no GEMM)
      NK_TRY(launch_copy2d(ctx, b.Y, m, b.M, m, m, m));
      NK_TRY(launch_axpby2d(ctx, 0.5, b.Yt, m, 0.5, b.M, m, m, m));
    } else {
      NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, b.Zt, m, b.Y, m, 0.0, b.M, m, sym));
      // The mirrored mode copies whole tiles across the diagonal and leaves the 128 x 128 diagonal tiles as computed.  Those
      // are symmetric to the last bit for a product X^T X, but for Z Y only up to rounding -- and Z <- T Z below is issued as
      // T^T Z, which a T that is not exactly symmetric turns into another iteration (3 to 8 times the error of the intended
      // one at cond 1e6, tests/test_gpu_sqrtm.py).  Average M with its transpose; T is free until the step is formed.
      NK_TRY(launch_transpose(ctx, b.M, m, b.T, m, m, m));
      NK_TRY(launch_axpby2d(ctx, 0.5, b.T, m, 0.5, b.M, m, m, m));
    }
    // a_lo over-estimates the smallest eigenvalue of M: while it is below 1/2 the iteration cannot have converged
    // (||M - I||_F / sqrt(m) >= (1 - lambda_min) / sqrt(m)), so the residual reduction and its host round trip are
    // skipped during the growth phase
    if (a_lo >= 0.5 || it + 1 == maxit) {
      NK_TRY(launch_frob_minus_identity(ctx, b.M, m, m, ctx->d_scalars));
      double r2 = 0.0;
      NK_TRY(read_scalar(ctx, ctx->d_scalars, &r2));
      r_prev = r;
      r = std::sqrt(r2 / m);
      if (!std::isfinite(r)) break;
      // quadratic convergence: once the previous residual was below 1e-7 this iterate sits on the rounding floor
      if (r < 5e-14 || r_prev < 1e-7) {
        ok = true;
        break;
      }
    }
    // scaled step: T = s (3I - s^2 M)/2 with the scale of the interval (ns_scale)
    const double s2 = ns_scale(a_lo, b_hi);
    const double sc = std::sqrt(s2);
    ns_advance(s2, a_lo, b_hi);
    NK_TRY(launch_scale_add_identity(ctx, -0.5 * s2 * sc, b.M, m, 1.5 * sc, b.T, m, m));
    NK_TRY(coupled_products(ctx, m, it, b));
  }
  if (iters) *iters = it;
  if (resid) *resid = r;
  NK_TRY(x_align());
  if (!ok) {
    set_error("sqrtm: Newton-Schulz did not converge (residual %g after %d iterations)", r, it);
    arena_release(ctx, mk);
    return NK_ERR_NO_CONVERGENCE;
  }
  const double sc = std::sqrt(c);
  NK_TRY(launch_axpby2d(ctx, sc, b.Y, m, 0.0, S, m, m, m));
  NK_TRY(launch_axpby2d(ctx, 1.0 / sc, b.Z, m, 0.0, Sinv, m, m, m));
  arena_release(ctx, mk);
  return NK_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// matrix square root through the polar decomposition of the Cholesky factor:  P = L L^T,  L^T = Q H  with Q orthogonal
// and H = (L L^T)^{1/2} = P^{1/2}, hence  S = Q^T L^T  and  S^-1 = L^-T Q.   Q is the limit of the scaled Newton-Schulz
// iteration  X <- X T,  T = s (3 I - s^2 X^T X) / 2,  X_0 = L^T / sqrt(||P||_inf): the eigenvalues of M = X^T X follow
// exactly the map of the coupled iteration above (M_0 = P / c in both), so the step count is the same, but a step costs
// one symmetric product (half the tiles) and ONE full product instead of two -- 3 m^3 flop instead of 5 m^3 -- and the
// full product is a single 256-tile launch at m = 2000 that leaves every CU one workgroup slot for the factorisation
// chain running beside it.  The price is one more latency-bound blocked Cholesky (with the identity riding along as
// extra rows, which leaves L^-T), queued by sqrtm_prepare long before the iteration is needed.
// ---------------------------------------------------------------------------------------------------------------
// Xt = L * s on and below the diagonal, zero above (the factorisation leaves the old upper triangle in place);
// X = Xt^T;  s = 1 / sqrt(d_c[0])
__device__ __forceinline__ void tri_scale_both_kernel_body(const double* __restrict__ L, int64_t ldl, int m, const double* __restrict__ d_c, double* __restrict__ Xt, double* __restrict__ X) {
  __shared__ double tile[32][33];
  const double s = 1.0 / sqrt(d_c[0]);
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int i = by + r, j = bx + tx;
    double v = 0.0;
    if (i < m && j <= i) v = L[(int64_t)i * ldl + j] * s;
    if (i < m && j < m) Xt[(int64_t)i * m + j] = v;
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i = bx + r, j = by + tx;
    if (i < m && j < m) X[(int64_t)i * m + j] = tile[tx][r];
  }
}
__global__ void __launch_bounds__(256) tri_scale_both_kernel(const double* __restrict__ L, int64_t ldl, int m, const double* __restrict__ d_c, double* __restrict__ Xt, double* __restrict__ X) { tri_scale_both_kernel_body(L, ldl, m, d_c, Xt, X); }
NK_BATCHED_TWIN(tri_scale_both_kernel, (256), const double*, int64_t, int, const double*, double*, double*)

int sqrtm_prepare(nk_ctx* ctx, const double* P, int64_t ldp, int m, SqrtPlan* plan) {
  plan->P = P; plan->ldp = ldp; plan->m = m;
  plan->mark = arena_mark(ctx);
  const size_t mm = (size_t)m * m;
  const int nblk = (m + CHOL_NB - 1) / CHOL_NB;
  NK_TRY(arena_alloc_t(ctx, 2 * mm, &plan->W));
  NK_TRY(arena_alloc_t(ctx, (size_t)nblk * CHOL_WS, &plan->Linv));
  NK_TRY(arena_alloc_t(ctx, mm, &plan->X0));
  NK_TRY(arena_alloc_t(ctx, mm, &plan->X0t));
  NK_TRY(arena_alloc_t(ctx, (size_t)SQ_COUNT, &plan->d_sc));
  NK_TRY(launch_max_abs_rowsum(ctx, P, ldp, m, plan->d_sc + SQ_C));
  NK_TRY(launch_sumsq_trace(ctx, P, ldp, m, plan->d_sc + SQ_SUMSQ, plan->d_sc + SQ_TRACE));
  // the three scalars of the scaling schedule are on the host long before the iteration is queued
  NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_SQRT_C, plan->d_sc + SQ_C, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipEventRecord(ctx->ev[EV_SQRT_SCALARS], ctx->stream));
  double* E = plan->W + mm;
  NK_TRY(launch_copy2d(ctx, P, ldp, plan->W, m, m, m));
  NK_TRY(launch_fill(ctx, E, m, m, m, 0.0));
  NK_TRY(launch_add_diag(ctx, E, m, m, 1.0));
  CholSys y;
  y.P = plan->W; y.ldp = m; y.m = m; y.extra = m; y.backward = false; y.Linv = plan->Linv;
  NK_TRY(cholesky_aug_pair_async(ctx, &y, 1, plan->pause_event, plan->pause_step));  // W <- [L ; L^-T]
  // ||L^-1||_F^2 (the extra rows hold L^-T): 1 / it bounds the smallest eigenvalue of P from below
  NK_TRY(launch_sumsq_trace(ctx, E, (int64_t)m, m, plan->d_sc + SQ_LINV2, nullptr));
  const int tb = (m + 31) / 32;
  hipLaunchKernelGGL(tri_scale_both_kernel, dim3(tb, tb), dim3(256), 0, ctx->stream, plan->W, (int64_t)m, m, plan->d_sc + SQ_C,
                     plan->X0t, plan->X0);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// convergence bookkeeping of the queued iteration: fixed-order sum of the per-block partials of sum (M - I)^2, then
// state[0] = step + 1 of the first step whose residual is below 1e-7 (0: not yet), state[1] = that residual,
// state[2] = last residual seen
__device__ __forceinline__ void ns_flag_kernel_body(const double* __restrict__ partial, int count, int m, int step, double* __restrict__ state) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += blockDim.x) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double r = sqrt((sh[0] + sh[1] + sh[2] + sh[3]) / m);
    state[2] = r;
    if (state[0] == 0.0 && r < 1e-7) {
      state[0] = (double)(step + 1);
      state[1] = r;
    }
  }
}
__global__ void __launch_bounds__(256) ns_flag_kernel(const double* __restrict__ partial, int count, int m, int step, double* __restrict__ state) { ns_flag_kernel_body(partial, count, m, step, state); }
NK_BATCHED_TWIN(ns_flag_kernel, (256), const double*, int, int, int, double*)

// S = Q^T L^T = sqrt(c) Q^T X_0 ;  S^-1 = L^-T Q = (L^-1)^T Q with L^-1 = (extra rows)^T   (Q = the converged iterate)
// Q_even / select: the iterate after an even number of steps and the device word holding the step count (queued form)
static int sqrtm_polar_products(nk_ctx* ctx, SqrtPlan* plan, const double* Q, double* scratch, double c, double* S,
                                double* Sinv, const double* Q_even = nullptr, const double* select = nullptr) {
  const int m = plan->m;
  const size_t mm = (size_t)m * m;
  double* Linv_full = scratch;
  NK_TRY(launch_transpose(ctx, plan->W + mm, m, Linv_full, m, m, m));
  TnProblem pr[2];
  pr[0].A = Q; pr[0].B = plan->X0; pr[0].C = S; pr[0].lda = pr[0].ldb = pr[0].ldc = m; pr[0].M = pr[0].N = m;
  pr[0].alpha = std::sqrt(c);
  pr[0].ktrim = KTRIM_B_UPPER;  // X_0 = L^T / sqrt(c) is upper triangular
  pr[1].ktrim = KTRIM_A_LOWER;  // L^-1 is lower triangular
  pr[1].A = Linv_full; pr[1].B = Q; pr[1].C = Sinv; pr[1].lda = pr[1].ldb = pr[1].ldc = m; pr[1].M = pr[1].N = m;
  pr[0].A_even = Q_even;
  pr[1].B_even = Q_even;
  TnSkip sel;
  sel.select = select;
  if (tn_fast_ok(pr[0]) && tn_fast_ok(pr[1]) && m >= 128) {
    NK_TRY(launch_gemm_tn_multi(ctx, pr, 2, m, 0, nullptr, true, select ? &sel : nullptr));
  } else {
    NK_TRY(launch_gemm(ctx, true, false, m, m, m, pr[0].alpha, Q, m, plan->X0, m, 0.0, S, m));
    NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, Linv_full, m, Q, m, 0.0, Sinv, m));
  }
  return NK_OK;
}

// ---- the forms of sqrtm_finish ------------------------------------------------------------------------------------
// what the host needs of sqrtm_prepare's device scalars
struct SqrtScalars {
  double c = 0.0, sumsq = 0.0, trace = 0.0, linv2 = 0.0;
};

// Early form: with a caller-supplied eigenvalue bound nothing of the factorisation is needed to queue the iteration; the host
// only waits for the three schedule scalars, copied right at the start of sqrtm_prepare.  An unusable norm withdraws the form.
static int scalars_early(nk_ctx* ctx, SqrtPlan* plan, SqrtScalars* sc) {
  NK_HIP(hipEventSynchronize(ctx->ev[EV_SQRT_SCALARS]));
  sc->c = ctx->h_scalars[HS_SQRT_C]; sc->sumsq = ctx->h_scalars[HS_SQRT_SUMSQ]; sc->trace = ctx->h_scalars[HS_SQRT_TRACE];
  if (!(sc->c > 0.0) || !std::isfinite(sc->c)) plan->early = false;
  return NK_OK;
}

// Synchronous form: the four scalars and the verdict word of the factorisation (ctx->h_info[ib])
static int scalars_synchronous(nk_ctx* ctx, SqrtPlan* plan, int ib, SqrtScalars* sc) {
  NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_SCRATCH, plan->d_sc, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipMemcpyAsync(ctx->h_info + ib, ctx->d_info + ib, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // the one host round trip of the square root
  const double* h = ctx->h_scalars + HS_SCRATCH;
  sc->c = h[SQ_C]; sc->sumsq = h[SQ_SUMSQ]; sc->trace = h[SQ_TRACE]; sc->linv2 = h[SQ_LINV2];
  return NK_OK;
}

// the dataflow factorisation gave up waiting: the whole square root once more with the launch-per-step chain
static int sqrtm_again_on_chain(nk_ctx* ctx, SqrtPlan* plan, double* S, double* Sinv) {
  count_event(CNT_CHOL_FLOW_GIVEUP);
  arena_release(ctx, plan->mark);
  ChainOnly chain(ctx);
  SqrtPlan again;
  NK_TRY(sqrtm_prepare(ctx, plan->P, plan->ldp, plan->m, &again));
  const int rc = sqrtm_finish(ctx, &again, S, Sinv);
  *plan = again;
  return rc;
}

// not numerically positive definite for the Cholesky route (e.g. a rank-deficient kernel matrix with a jitter below the
// rounding level): the coupled iteration needs no factorisation
static int sqrtm_coupled_fallback(nk_ctx* ctx, SqrtPlan* plan, double* S, double* Sinv) {
  arena_release(ctx, plan->mark);
  plan->rc = sqrtm_spd_coupled(ctx, plan->P, plan->ldp, plan->m, S, Sinv, &plan->iters, &plan->resid);
  return plan->rc;
}

// Buffers of the polar iteration X <- X T: the iterate and its transpose, current (read) and next (written), M = X^T X and T.
// X_0 is the plan's; X_j lives in Xa for odd j and in Xb for even j.
struct PolarIter {
  int m = 0;
  double c = 0.0;
  double *Xa = nullptr, *Xta = nullptr, *Xb = nullptr, *Xtb = nullptr, *M = nullptr, *T = nullptr;
  const double *X = nullptr, *Xt = nullptr;
  double *Xn = nullptr, *Xtn = nullptr;
  bool fast = false;  // the X T products take the LDS-DMA engine (transposed copy from the epilogue)
};
static int polar_setup(nk_ctx* ctx, const SqrtPlan* plan, double c, PolarIter* it) {
  const int m = it->m = plan->m;
  const size_t mm = (size_t)m * m;
  it->c = c;
  NK_TRY(arena_alloc_t(ctx, mm, &it->Xa));
  NK_TRY(arena_alloc_t(ctx, mm, &it->Xta));
  NK_TRY(arena_alloc_t(ctx, mm, &it->Xb));
  NK_TRY(arena_alloc_t(ctx, mm, &it->Xtb));
  NK_TRY(arena_alloc_t(ctx, mm, &it->M));
  NK_TRY(arena_alloc_t(ctx, mm, &it->T));
  it->X = plan->X0; it->Xt = plan->X0t;
  it->Xn = it->Xa; it->Xtn = it->Xta;
  TnProblem probe;
  probe.A = it->Xta; probe.B = it->T; probe.C = it->Xa; probe.lda = probe.ldb = probe.ldc = m; probe.M = probe.N = m;
  it->fast = m >= 128 && tn_fast_ok(probe);
  return NK_OK;
}
// M_0 = X_0^T X_0 = L L^T / c = P / c, taken as the average of P and P^T (no GEMM)
static int polar_first_m(nk_ctx* ctx, const SqrtPlan* plan, const PolarIter& it) {
  const int m = it.m;
  NK_TRY(launch_transpose(ctx, plan->P, plan->ldp, it.M, m, m, m));
  NK_TRY(launch_axpby2d(ctx, 0.5 / it.c, plan->P, plan->ldp, 0.5 / it.c, it.M, m, m, m));
  return NK_OK;
}
// X <- X T with the transposed copy (from the epilogue of the fast launch, or by a transpose), then the buffers change roles
static int polar_x_times_t(nk_ctx* ctx, PolarIter& it, int splitk, const TnSkip* skip) {
  const int m = it.m;
  if (it.fast) {
    TnProblem pr;
    pr.A = it.Xt; pr.B = it.T; pr.C = it.Xn; pr.lda = pr.ldb = pr.ldc = m; pr.M = pr.N = m; pr.Ct = it.Xtn; pr.ldct = m;
    NK_TRY(launch_gemm_tn_multi(ctx, &pr, 1, m, splitk, nullptr, true, skip));
  } else {
    NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, it.Xt, m, it.T, m, 0.0, it.Xn, m));
    NK_TRY(launch_transpose(ctx, it.Xn, m, it.Xtn, m, m, m));
  }
  it.X = it.Xn; it.Xt = it.Xtn;
  it.Xn = (it.Xn == it.Xa) ? it.Xb : it.Xa;
  it.Xtn = (it.Xtn == it.Xta) ? it.Xtb : it.Xta;
  return NK_OK;
}

// The whole iteration queued without host round trips (m >= 1024 on the LDS-DMA engine).  The step count is data dependent,
// so (a) a rigorous lower bound of the smallest eigenvalue -- the caller's (jitter) in the early form, otherwise
// lambda_min(P) >= 1 / ||L^-1||_F^2 -- run through the scaling schedule (ns_queued_schedule) gives the latest step kmax at
// which the iteration can converge, and (b) the launches of steps after the one that actually converged return at once on
// the device (TnSkip), and the two final products pick the buffer that holds the converged iterate by the parity of the
// step count (also on the device).  The verdict is read by sqrtm_verdict.
static int polar_queued(nk_ctx* ctx, SqrtPlan* plan, PolarIter& it, double a_lo, double linv2, double* S, double* Sinv) {
  const int m = it.m;
  const double c = it.c;
  const NsSchedule sch = ns_queued_schedule(a_lo, plan->early ? 0.9 * plan->lambda_min_hint / c : 0.5 / (c * linv2));
  const int kmax = sch.kmax;
  double* state = plan->d_sc + SQ_FLAG;
  NK_HIP(hipMemsetAsync(state, 0, 3 * sizeof(double), ctx->stream));
  double* rpart = nullptr;
  {
    const size_t mt = (size_t)(m + 127) / 128;
    const size_t need = std::max((size_t)grid_for((int64_t)m * m, ctx->num_cu), mt * (mt + 1) / 2 * 8);
    NK_TRY(arena_alloc_t(ctx, need, &rpart));
  }
  for (int k = 0; k < kmax; ++k) {
    TnSkip skip;
    skip.state = state; skip.step = k;
    int npart = 0;  // residual partials written by the reduce kernel of the M product (k > 0)
    if (k == 0) {
      NK_TRY(polar_first_m(ctx, plan, it));
    } else {
      // M = X^T X and, from the same epilogue, T = s (3 I - s^2 M) / 2 (its coefficients come from the schedule)
      const double s2k = sch.s2[k], sck = std::sqrt(s2k);
      TnProblem pm;
      pm.A = it.X; pm.B = it.X; pm.C = it.M; pm.lda = pm.ldb = pm.ldc = m; pm.M = pm.N = m; pm.tri = TRI_UPPER_MIRROR;
      pm.Caff = it.T; pm.aff_a = -0.5 * s2k * sck; pm.aff_c = 1.5 * sck;
      TnSkip skip_m = skip;
      skip_m.resid_partials = rpart; skip_m.resid_count = &npart;
      NK_TRY(launch_gemm_tn_multi(ctx, &pm, 1, m, 0, nullptr, true, &skip_m));
    }
    if (sch.check[k]) {
      // M_0 (no product) or a single-slice product: separate pass over M for the partials
      if (npart == 0) NK_TRY(launch_frob_mi_partials(ctx, it.M, (int64_t)m, m, rpart, &npart, &skip));
      // sum of the partials in index order and the convergence flag (one launch)
      hipLaunchKernelGGL(ns_flag_kernel, dim3(1), dim3(256), 0, ctx->stream, rpart, npart, m, k, state);
      NK_HIP(hipGetLastError());
    }
    if (k == 0) {
      const double s2 = sch.s2[0], sc = std::sqrt(s2);
      NK_TRY(launch_scale_add_identity(ctx, -0.5 * s2 * sc, it.M, m, 1.5 * sc, it.T, m, m, &skip));
    }
    // one K slice: at most one workgroup slot per CU is taken, the other stays free for the factorisation chain on the
    // main stream (a two-slice launch would take every slot for its whole duration)
    NK_TRY(polar_x_times_t(ctx, it, 1, &skip));
  }
  // the step count state[0] = j picks the operand on the device: Xa for odd j, Xb for even j
  NK_TRY(sqrtm_polar_products(ctx, plan, it.Xa, it.T, c, S, Sinv, it.Xb, state));
  NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_SQRT_FLAG, state, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (plan->early)  // the verdict of the factorisation travels with the verdict of the iteration
    NK_HIP(hipMemcpyAsync(ctx->h_info + plan->info_slot, ctx->d_info + plan->info_slot, sizeof(int), hipMemcpyDeviceToHost,
                          ctx->stream));
  plan->deferred = true;
  plan->kmax = kmax;
  arena_release(ctx, plan->mark);
  return NK_OK;
}

// Small / unaligned matrices: convergence read by the host, one step behind the queue.  They are launch bound, and the spare
// steps the rigorous step budget adds (about five at m = 500, six launches each) would cost more than the few
// synchronisations of this loop.
static int polar_host_checked(nk_ctx* ctx, SqrtPlan* plan, PolarIter& it, double a_lo, double* S, double* Sinv) {
  const int m = it.m;
  GemmOpts sym;
  sym.tri = TRI_UPPER_MIRROR;
  const int maxit = NS_MAX_STEPS;
  double b_hi = 1.0, r = 1e300;
  int k = 0;
  bool ok = false;
  for (; k < maxit; ++k) {
    if (k == 0) NK_TRY(polar_first_m(ctx, plan, it));
    else NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, it.X, m, it.X, m, 0.0, it.M, m, sym));  // M = X^T X
    const bool check = a_lo >= 0.5 || k + 2 >= maxit;
    if (check) {
      NK_TRY(launch_frob_minus_identity(ctx, it.M, m, m, ctx->d_scalars));
      NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_SCRATCH, ctx->d_scalars, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      NK_HIP(hipEventRecord(ctx->ev[EV_SQRT_RESID], ctx->stream));
    }
    const double s2 = ns_scale(a_lo, b_hi);
    const double sc = std::sqrt(s2);
    ns_advance(s2, a_lo, b_hi);
    NK_TRY(launch_scale_add_identity(ctx, -0.5 * s2 * sc, it.M, m, 1.5 * sc, it.T, m, m));
    NK_TRY(polar_x_times_t(ctx, it, 0, nullptr));
    if (check) {
      NK_HIP(hipEventSynchronize(ctx->ev[EV_SQRT_RESID]));
      r = std::sqrt(ctx->h_scalars[HS_SCRATCH] / m);
      if (!std::isfinite(r)) break;
      if (r < 1e-7) {
        ok = true;
        ++k;
        break;
      }
    }
  }
  plan->iters = k;
  plan->resid = r;
  NK_TRY(x_align());  // lock-step groups: the iteration count differs from unit to unit; re-align the launch sequences here
  if (!ok) {
    set_error("sqrtm: Newton-Schulz did not converge (residual %g after %d iterations)", r, k);
    arena_release(ctx, plan->mark);
    plan->rc = NK_ERR_NO_CONVERGENCE;
    return plan->rc;
  }
  NK_TRY(sqrtm_polar_products(ctx, plan, it.X, it.T, it.c, S, Sinv));
  arena_release(ctx, plan->mark);
  return NK_OK;
}

int sqrtm_finish(nk_ctx* ctx, SqrtPlan* plan, double* S, double* Sinv) {
  const int m = plan->m;
  const int ib = info_base(ctx);
  plan->deferred = false;
  plan->info_slot = ib;
  plan->rc = NK_OK; plan->iters = 0; plan->resid = 0.0;
  // the early form is for large aligned matrices whose caller supplied an eigenvalue bound
  plan->early = plan->lambda_min_hint > 0.0 && m >= 1024 && m % 2 == 0;
  SqrtScalars sc;
  if (plan->early) NK_TRY(scalars_early(ctx, plan, &sc));
  if (!plan->early) {
    NK_TRY(scalars_synchronous(ctx, plan, ib, &sc));
    if (ctx->h_info[ib] == CHOL_FLOW_GIVEUP) return sqrtm_again_on_chain(ctx, plan, S, Sinv);
    const char* hook = getenv("NYSKOOP_SQRT_FORCE_COUPLED");  // test hook, read per call: take the fallback (tests/)
    const bool forced = hook && hook[0] == '1';
    if (forced || ctx->h_info[ib] != 0 || !(sc.c > 0.0) || !std::isfinite(sc.c) || !(sc.linv2 > 0.0) || !std::isfinite(sc.linv2))
      return sqrtm_coupled_fallback(ctx, plan, S, Sinv);
  }
  PolarIter it;
  NK_TRY(polar_setup(ctx, plan, sc.c, &it));
  // spectrum interval [a, 1] of M_0 = P / c, as in the coupled iteration
  const double a_lo = ns_interval_estimate(std::sqrt(sc.sumsq) / sc.c, sc.trace / sc.c, m);
  // Queue the whole iteration (no host round trips) for large matrices on the LDS-DMA engine; the others are host checked
  const bool queued = it.fast && m >= 1024;
  if (plan->early && !queued) {  // cannot happen for the shapes `early` is set for; keep the contract simple
    set_error("sqrtm: internal: early queueing needs the LDS-DMA path");
    return NK_ERR_BAD_ARG;
  }
  return queued ? polar_queued(ctx, plan, it, a_lo, sc.linv2, S, Sinv) : polar_host_checked(ctx, plan, it, a_lo, S, Sinv);
}

int sqrtm_verdict(nk_ctx* ctx, SqrtPlan* plan, int* iters, double* resid) {
  if (plan->deferred) {
    const double flag = ctx->h_scalars[HS_SQRT_FLAG], last = ctx->h_scalars[HS_SQRT_RESID_LAST];
    plan->deferred = false;
    const int word = ctx->h_info[plan->info_slot];
    if (plan->early && (word != 0 || flag == 0.0 || !std::isfinite(last))) {
      plan->flow_gave_up = word == CHOL_FLOW_GIVEUP;
      if (plan->flow_gave_up) count_event(CNT_CHOL_FLOW_GIVEUP);
      plan->iters = plan->kmax;
      plan->resid = last;
      plan->rc = NK_SQRT_RETRY;
    } else if (flag == 0.0 || !std::isfinite(last)) {
      plan->iters = plan->kmax;
      plan->resid = last;
      plan->rc = NK_ERR_NO_CONVERGENCE;
      set_error("sqrtm: Newton-Schulz did not converge (residual %g after %d iterations)", plan->resid, plan->kmax);
    } else {
      plan->iters = (int)flag;
      plan->resid = ctx->h_scalars[HS_SQRT_RESID_AT_FLAG];
      plan->rc = NK_OK;
    }
  }
  if (iters) *iters = plan->iters;
  if (resid) *resid = plan->resid;
  return plan->rc;
}

int sqrtm_spd(nk_ctx* ctx, const double* P, int64_t ldp, int m, double* S, double* Sinv, int* iters, double* resid) {
  SqrtPlan plan;
  NK_TRY(sqrtm_prepare(ctx, P, ldp, m, &plan));
  NK_TRY(sqrtm_finish(ctx, &plan, S, Sinv));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return sqrtm_verdict(ctx, &plan, iters, resid);
}

}  // namespace nk
