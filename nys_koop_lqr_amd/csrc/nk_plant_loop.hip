// LQR closed loop around the TRUE plant (lqr_control of benchmark_lqr_hjb.py:73-97 and benchmark_lqr_classic.py:67-89) as
// ONE launch: every step lifts the measured state, forms u = K (phi(x_ref) - phi(x)) and advances the plant by one
// Runge-Kutta step (nk_plant.h).  The gain is folded into the lift once per call,
//     w = S^-1 K^T  (m entries, p = 1; spline models: w = K^T),     u_t = sum_j w_j (k(z_j, x_ref) - k(z_j, x_t)),
// so a step costs m kernel values over d <= 2 coordinates and one dot product of length m instead of an m x m product.
// The difference of the two kernel values is taken landmark by landmark BEFORE the product with w_j: the cancellation of
// u near the reference state then happens on numbers of order one, not on two dot products of the size of |w|.
//
// One workgroup per trajectory, the whole loop inside it, nothing from the host per step.  A step is a latency chain
// (kernel values -> reduction -> plant -> next kernel values), so the workgroup is the SMALLEST that holds the landmarks
// at LPT per lane: one wave up to m = 256 (LPT = 1 up to 64 landmarks, 4 beyond), ceil(m / 256) waves up to m = 4096.
// Each lane keeps its landmarks (scaled by 1 / lengthscale), their kernel values at x_ref and its entries of w in
// registers for all steps.  Per step: LPT kernel values with the arithmetic of the kernel-matrix kernels (nk_kmat.hip:
// rounded products with 1 / lengthscale, difference, FMAs over the coordinates in index order, the same epilogue), LPT
// FMAs, a DPP reduction over the wave; with several waves one LDS word per wave, ONE workgroup barrier, and a DPP
// reduction of the (zero padded) 16 words that every wave performs alike.  Every summation order is fixed by m alone, so
// a trajectory has the same bits alone or in any batch.  All lanes advance the plant (same operands, same bits); thread
// 0 stores x_{t+1} and u_t with ordinary vector stores that nothing in the loop waits for.
#include "nk_common.h"
#include "nk_loop_lanes.h"
#include "nk_plant.h"
#include "nk_poly_plant.h"
#include "nk_poly_lanes.h"

#include <type_traits>

namespace nk {

constexpr int PLANT_LOOP_LPT = 4;
constexpr int PLANT_LOOP_MAX_M = 64 * PLANT_LOOP_LPT * PLANT_LOOP_MAX_WAVES;

// sum_j w_j (kref_j - k(z_j, x)) over the landmarks of the workgroup, the same bits in every lane
template <int KTYPE, int D, int LPT>
__device__ __forceinline__ double plant_feedback(const double* x, const double* wi, const double (&zs)[LPT][D],
                                                 const double (&wj)[LPT], const double (&kref)[LPT], double sigma0sq,
                                                 double* red, int lane, int wave, bool multi) {
  double xs[D];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < D; ++k) xs[k] = x[k] * wi[k];
  }
  double part = 0.0;
#pragma unroll
  for (int l = 0; l < LPT; ++l) part = fma(wj[l], kref[l] - plant_kval<KTYPE, D>(xs, zs[l], sigma0sq), part);
  double s = wave_sum64_dpp(part);
  if (multi) {  // uniform over the workgroup
    if (lane == 0) red[wave] = s;
    // LDS-only barrier (the global stores of earlier steps need not have retired: nothing reads them back)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    s = row_sum16_dpp(red[lane & 15]);
  }
  return s;
}

// One loop, as a workgroup sees it, is a PlantLoopUnit (nk_common.h).  nk_plant_loop builds the record from the record of batch
// member 0 and the block index (unit_of_block, nk_loop_lanes.h); nk_plant_loop_multi reads it from a table in device memory,
// blockIdx.x = the record.
// The loop of one workgroup.  SCORED = false: the body of nk_plant_loop (out_x, out_u always stored, no scores).
// SCORED = true: out_x / out_u may be null (uniform over the workgroup), and the four scores of include/nyskoop.h are
// accumulated in registers (the helpers of nk_loop_lanes.h with one input) -- every lane holds u_t and x_{t+1} -- and stored
// once by thread 0 after the last step.
template <int PLANT, int KTYPE, int LPT, bool SCORED>
__device__ __forceinline__ void plant_loop_body(const PlantLoopUnit& P, double Ts, int steps, double (&red)[2][PLANT_LOOP_MAX_WAVES]) {
  constexpr int D = PlantDim<PLANT>::value;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const bool multi = nthreads > 64;
  if (tid < 2 * PLANT_LOOP_MAX_WAVES) (&red[0][0])[tid] = 0.0;  // words of waves that do not exist stay zero
  double wi[D], zs[LPT][D], wj[LPT], kref[LPT], x[D], xr[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    wi[k] = P.winv[k];
    x[k] = P.x0[k];
    xr[k] = P.xref[k];
  }
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
      const int j = tid + l * nthreads;
      const bool have = j < P.m;  // a slot without a landmark: weight 0, landmark 0 (finite kernel value, exact 0 product)
      wj[l] = have ? P.w[j] : 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) zs[l][k] = have ? P.Z[(int64_t)j * D + k] * wi[k] : 0.0;
    }
    double xrs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xrs[k] = xr[k] * wi[k];
#pragma unroll
    for (int l = 0; l < LPT; ++l) kref[l] = plant_kval<KTYPE, D>(xrs, zs[l], P.sigma0sq);
  }
  double* ox = P.out_x;
  double* ou = P.out_u;
  const bool st_x = !SCORED || ox != nullptr, st_u = !SCORED || ou != nullptr;
  if (tid == 0 && st_x) {
#pragma unroll
    for (int k = 0; k < D; ++k) ox[k] = x[k];
  }
  double sse = 0.0, sso = 0.0, J = 0.0, umax = 0.0, uo[1] = {0.0};  // the scores (SCORED only)
  const double* uopt = SCORED ? P.u_opt : nullptr;
  if (SCORED) {
    J = sum_sq_ordered(x);
    if (uopt) uo[0] = uopt[0];
  }
  __syncthreads();  // red is zeroed
  for (int t = 0; t < steps; ++t) {
    // buffer t & 1: a wave still reading it in step t is at most one barrier behind the wave that writes it again in t + 2
    const double u[1] = {plant_feedback<KTYPE, D, LPT>(x, wi, zs, wj, kref, P.sigma0sq, red[t & 1], lane, wave, multi)};
    double xn[D];
    plant_step<PLANT>(Ts, x, u[0], xn);
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xn[k];
    if (SCORED) {
      score_cost_step(x, u, J, umax);
      if (uopt) score_uopt_step(u, uo, uopt, (int64_t)(t + 1 < steps ? t + 1 : t), 1, sse, sso);
    }
    if (tid == 0) store_step(ou, st_u, P.ldu, ox, st_x, P.ldx, (int64_t)t, u, 1, x, D);
  }
  if (SCORED && tid == 0 && P.score) {
    P.score[0] = sse;
    P.score[1] = sso;
    P.score[2] = J;
    P.score[3] = umax;
  }
}

template <int PLANT, int KTYPE, int LPT>
__global__ void __launch_bounds__(LPT == 1 ? 64 : 64 * PLANT_LOOP_MAX_WAVES)
    plant_loop_kernel(PlantLoopUnit base, LoopStrides strides, double Ts) {
  __shared__ double red[2][PLANT_LOOP_MAX_WAVES];  // one partial sum per wave, two buffers (parity of the step)
  plant_loop_body<PLANT, KTYPE, LPT, false>(unit_of_block(base, strides, blockIdx.x), Ts, strides.steps, red);
}

// the multi-model form: unit blockIdx.x of `table` (all units of a launch share KTYPE, LPT and the block size)
template <int PLANT, int KTYPE, int LPT>
__global__ void __launch_bounds__(LPT == 1 ? 64 : 64 * PLANT_LOOP_MAX_WAVES)
    plant_loop_multi_kernel(const PlantLoopUnit* __restrict__ table, double Ts, int steps) {
  __shared__ double red[2][PLANT_LOOP_MAX_WAVES];
  const PlantLoopUnit U = table[blockIdx.x];
  plant_loop_body<PLANT, KTYPE, LPT, true>(U, Ts, steps, red);
}

bool plant_loop_ok(int m) { return m >= 1 && m <= PLANT_LOOP_MAX_M; }

// The workgroup shape of a model of m landmarks: one wave with one landmark per lane up to 64, PLANT_LOOP_LPT per lane beyond.
static void plant_loop_class(int m, int* lpt, int* waves) {
  if (m <= 64) {
    *lpt = 1;
    *waves = 1;
  } else {
    *lpt = PLANT_LOOP_LPT;
    *waves = (m + 64 * PLANT_LOOP_LPT - 1) / (64 * PLANT_LOOP_LPT);
  }
}

// ---- dispatch: a run-time id becomes a template argument, handed to f as a std::integral_constant
template <class F>
static auto with_plant(int plant, F&& f) {  // (the id has been checked: plant_dim(plant) > 0)
  if (plant == NK_PLANT_DUFFING) return f(std::integral_constant<int, NK_PLANT_DUFFING>{});
  if (plant == NK_PLANT_DOUBLE_INTEGRATOR) return f(std::integral_constant<int, NK_PLANT_DOUBLE_INTEGRATOR>{});
  return f(std::integral_constant<int, NK_PLANT_HJB>{});
}
// launch(plant, kernel family, landmarks per lane) for a launch whose workgroups have `lpt` landmarks per lane
template <class F>
static int plant_loop_dispatch(const char* who, int plant, int ktype, int lpt, F&& launch) {
  NK_TRY(with_plant(plant, [&](auto pl) {
    return with_kernel_family(who, ktype, [&](auto kt) {
      if (lpt == 1) launch(pl, kt, std::integral_constant<int, 1>{});
      else launch(pl, kt, std::integral_constant<int, PLANT_LOOP_LPT>{});
    });
  }));
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// nk_plant_step: one step of the plant in the host build of nk_plant.h (x_next may be x)
void plant_step_host(int plant, double Ts, const double* x, double u, double* x_next) {
  double xn[PLANT_MAX_D];
  with_plant(plant, [&](auto pl) { plant_step<decltype(pl)::value>(Ts, x, u, xn); });
  for (int k = 0; k < plant_dim(plant); ++k) x_next[k] = xn[k];
}

// all pointers device memory; w: the folded gain (m entries); out_x: batch * (steps + 1) rows of d, out_u: batch * steps
// rows of one
int launch_plant_loop(nk_ctx* ctx, const nk_model* mdl, int plant, double Ts, const double* w, const double* x0,
                      int64_t x0_stride, const double* xref, int64_t xref_stride, int steps, int batch, double* out_x,
                      int64_t ldx, double* out_u, int64_t ldu) {
  NK_REQUIRE(plant_dim(plant) == mdl->d && plant_loop_ok(mdl->m) && steps >= 1 && batch >= 1, "plant_loop: bad sizes");
  PlantLoopUnit U;  // batch member 0
  U.Z = mdl->Z; U.winv = mdl->winv; U.w = w; U.m = mdl->m; U.reserved = 0; U.sigma0sq = mdl->sigma0 * mdl->sigma0;
  U.x0 = x0; U.xref = xref; U.out_x = out_x; U.ldx = ldx; U.out_u = out_u; U.ldu = ldu;
  U.u_opt = nullptr; U.score = nullptr;
  const LoopStrides strides{x0_stride, xref_stride, 0, steps};
  int lpt = 0, waves = 0;
  plant_loop_class(mdl->m, &lpt, &waves);
  return plant_loop_dispatch("plant_loop", plant, mdl->ktype, lpt, [&](auto pl, auto kt, auto lp) {
    hipLaunchKernelGGL((plant_loop_kernel<decltype(pl)::value, decltype(kt)::value, decltype(lp)::value>), dim3(batch),
                       dim3(64 * waves), 0, ctx->stream, U, strides, Ts);
  });
}
int plant_loop_max_m() { return PLANT_LOOP_MAX_M; }

// ---- multi-model form ------------------------------------------------------------------------------------------------
// units: host records holding device pointers, ktypes: the kernel family of each.  The records run through
// launch_loop_classes (nk_loop_lanes.h) in classes of (kernel family, landmarks per lane, waves): `units` is reordered in place
// and must stay alive until the stream has been synchronised.
int launch_plant_loop_multi(nk_ctx* ctx, int plant, double Ts, int steps, PlantLoopUnit* units, const int* ktypes,
                            int n_units) {
  NK_REQUIRE(plant_dim(plant) > 0 && steps >= 1 && n_units >= 1, "plant_loop_multi: bad sizes");
  for (int u = 0; u < n_units; ++u) NK_REQUIRE(plant_loop_ok(units[u].m), "plant_loop_multi: unit %d: bad m", u);
  auto key_of = [&](int u) {
    LoopClass k{ktypes[u], 0, 0};
    plant_loop_class(units[u].m, &k.shape, &k.waves);
    return k;
  };
  return launch_loop_classes(ctx, units, n_units, key_of, nullptr, [&](const PlantLoopUnit* first, int count, const LoopClass& k, long) {
    return plant_loop_dispatch("plant_loop_multi", plant, k.ktype, k.shape, [&](auto pl, auto kt, auto lp) {
      hipLaunchKernelGGL((plant_loop_multi_kernel<decltype(pl)::value, decltype(kt)::value, decltype(lp)::value>), dim3(count),
                         dim3(64 * k.waves), 0, ctx->stream, first, Ts, steps);
    });
  });
}

// =====================================================================================================================
// The same loop around a polynomial plant the caller describes (nk_poly_plant.h): d <= 4 states, p <= 4 inputs.
// The gain is folded into W = S^-1 K^T (m x p; spline models: K^T), u_j = sum_l W[l][j] (kref_l - k(z_l, x_t)): a lane
// keeps its landmarks, their reference values and its rows of W in registers, forms P partial sums and reduces them with P
// DPP wave reductions (independent chains, interleaved by the scheduler); with several waves P LDS words per wave, still
// ONE LDS-only barrier per step, and the 16-word DPP reduction once per input.  The plant table arrives by value in the
// kernel arguments, compiled by the host into a PolyProgram, and is evaluated in the lanes of every wave (PolyLanes): all
// terms at once, the row sums in table order through v_readlane, all control flow uniform.  The kernels are instantiated for D in {2, 4} and P in {1, 2, 4}; states, landmarks coordinates, inverse
// length scales, weights and controls beyond the plant's d and p are exact zeros, which changes no bit of the others.
// Every summation order is fixed by m and P alone.
// =====================================================================================================================
constexpr int poly_pad_p(int p) { return p == 3 ? 4 : p; }
// Landmarks per lane of the workgroups of more than 64 landmarks: the most (of 4, 2, 1) at which both 16-wave kernels of the
// class (the scored one needs more) keep everything in their 128 registers per lane -- no scratch; DESIGN.md 5d lists what
// the compiler reports.  The class limit on m is 1024 times this number.
constexpr int poly_lpt(int D, int P) { return D == 2 ? (P <= 2 ? 4 : 2) : (P <= 2 ? 2 : 1); }

// u_j = sum_l W[l][j] (kref_l - k(z_l, x)) for j < P, the same bits in every lane
template <int KTYPE, int D, int P, int LPT>
__device__ __forceinline__ void poly_feedback(const double* x, const double* wi, const double (&zs)[LPT][D],
                                              const double (&wj)[LPT][P], const double (&kref)[LPT], double sigma0sq,
                                              double (&red)[P][PLANT_LOOP_MAX_WAVES], int lane, int wave, bool multi,
                                              double* u) {
  double xs[D];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < D; ++k) xs[k] = x[k] * wi[k];
  }
  double part[P];
#pragma unroll
  for (int j = 0; j < P; ++j) part[j] = 0.0;
#pragma unroll
  for (int l = 0; l < LPT; ++l) {
    const double dk = kref[l] - plant_kval<KTYPE, D>(xs, zs[l], sigma0sq);
#pragma unroll
    for (int j = 0; j < P; ++j) part[j] = fma(wj[l][j], dk, part[j]);
  }
#pragma unroll
  for (int j = 0; j < P; ++j) u[j] = wave_sum64_dpp(part[j]);
  if (multi) {  // uniform over the workgroup
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < P; ++j) red[j][wave] = u[j];
    }
    // LDS-only barrier (the global stores of earlier steps need not have retired: nothing reads them back)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = row_sum16_dpp(red[j][lane & 15]);
  }
}

// The loop of one workgroup; SCORED as in plant_loop_body, the sums of the scores running over the inputs in index order.
template <int KTYPE, int LPT, int D, int P, bool SCORED>
__device__ __forceinline__ void poly_loop_body(const PolyLoopUnit& U, const PolyProgram& pl, int steps,
                                               double (&red)[2][P][PLANT_LOOP_MAX_WAVES]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const int d = pl.d, p = pl.p;
  const bool multi = nthreads > 64;
  for (int i = tid; i < 2 * P * PLANT_LOOP_MAX_WAVES; i += nthreads) (&red[0][0][0])[i] = 0.0;  // words of absent waves stay zero
  const PolyLanes tb(pl, lane);
  double wi[D], zs[LPT][D], wj[LPT][P], kref[LPT], x[D], xr[D], u[P];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const bool have = k < d;
    wi[k] = have ? U.winv[k] : 0.0;
    x[k] = have ? U.x0[k] : 0.0;
    xr[k] = have ? U.xref[k] : 0.0;
  }
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
      const int i = tid + l * nthreads;
      const bool have = i < U.m;  // a slot without a landmark: weights 0, landmark 0 (finite kernel value, exact 0 products)
#pragma unroll
      for (int j = 0; j < P; ++j) wj[l][j] = (have && j < p) ? U.w[(int64_t)i * U.w_ls + (int64_t)j * U.w_js] : 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) zs[l][k] = (have && k < d) ? U.Z[(int64_t)i * d + k] * wi[k] : 0.0;
    }
    double xrs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xrs[k] = xr[k] * wi[k];
#pragma unroll
    for (int l = 0; l < LPT; ++l) kref[l] = plant_kval<KTYPE, D>(xrs, zs[l], U.sigma0sq);
  }
  double* ox = U.out_x;
  double* ou = U.out_u;
  const bool st_x = !SCORED || ox != nullptr, st_u = !SCORED || ou != nullptr;
  if (tid == 0 && st_x) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k < d) ox[k] = x[k];
  }
  double sse = 0.0, sso = 0.0, J = 0.0, umax = 0.0, uo[P];
#pragma unroll
  for (int j = 0; j < P; ++j) uo[j] = 0.0;
  const double* uopt = SCORED ? U.u_opt : nullptr;
  if (SCORED) {
    J = sum_sq_ordered(x);
    if (uopt) {
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (j < p) uo[j] = uopt[j];
    }
  }
  __syncthreads();  // red is zeroed
  for (int t = 0; t < steps; ++t) {
    // buffer t & 1: a wave still reading it in step t is at most one barrier behind the wave that writes it again in t + 2
    poly_feedback<KTYPE, D, P, LPT>(x, wi, zs, wj, kref, U.sigma0sq, red[t & 1], lane, wave, multi, u);
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = j < p ? u[j] : 0.0;
    double xn[D];
    poly_plant_step<D, P>(tb, x, u, xn);
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xn[k];
    if (SCORED) {
      score_cost_step(x, u, J, umax);
      if (uopt) score_uopt_step(u, uo, uopt, (int64_t)(t + 1 < steps ? t + 1 : t), p, sse, sso);
    }
    if (tid == 0) store_step(ou, st_u, U.ldu, ox, st_x, U.ldx, (int64_t)t, u, p, x, d);
  }
  if (SCORED && tid == 0 && U.score) {
    U.score[0] = sse;
    U.score[1] = sso;
    U.score[2] = J;
    U.score[3] = umax;
  }
}

// WG: the largest workgroup a kernel is launched with (64: one wave with one landmark per lane; else 16 waves)
template <int KTYPE, int LPT, int D, int P, int WG>
__global__ void __launch_bounds__(WG) poly_loop_kernel(PolyLoopUnit base, LoopStrides strides, PolyProgram pl) {
  __shared__ double red[2][P][PLANT_LOOP_MAX_WAVES];  // per input one partial sum per wave, two buffers (parity of the step)
  poly_loop_body<KTYPE, LPT, D, P, false>(unit_of_block(base, strides, blockIdx.x), pl, strides.steps, red);
}

// the multi-model form: unit blockIdx.x of `table` (all units of a launch share KTYPE, LPT and the block size)
template <int KTYPE, int LPT, int D, int P, int WG>
__global__ void __launch_bounds__(WG)
    poly_loop_multi_kernel(const PolyLoopUnit* __restrict__ table, PolyProgram pl, int steps) {
  __shared__ double red[2][P][PLANT_LOOP_MAX_WAVES];
  const PolyLoopUnit U = table[blockIdx.x];
  poly_loop_body<KTYPE, LPT, D, P, true>(U, pl, steps, red);
}

int poly_loop_max_m(int d, int p) {
  if (d < 1 || d > NK_POLY_MAX_D || p < 1 || p > NK_POLY_MAX_P) return 0;
  return 64 * poly_lpt(poly_pad_d(d), poly_pad_p(p)) * PLANT_LOOP_MAX_WAVES;
}

// The workgroup shape of a model of m landmarks in the class (D, P): one wave with one landmark per lane up to 64, the
// class's landmarks per lane beyond.
static void poly_loop_class(int m, int lpt_class, int* lpt, int* waves) {
  if (m <= 64) {
    *lpt = 1;
    *waves = 1;
  } else {
    *lpt = lpt_class;
    *waves = (m + 64 * lpt_class - 1) / (64 * lpt_class);
  }
}

// launch(kernel family, landmarks per lane, D, P, workgroup bound) for the plant's class; many = false: one wave with one
// landmark per lane
template <class F>
static int poly_loop_dispatch(const char* who, int d, int p, int ktype, bool many, F&& launch) {
  auto with_lpt = [&](auto kt, auto dd, auto pp) {
    constexpr int L = poly_lpt(decltype(dd)::value, decltype(pp)::value);
    if (many) launch(kt, std::integral_constant<int, L>{}, dd, pp, std::integral_constant<int, 64 * PLANT_LOOP_MAX_WAVES>{});
    else launch(kt, std::integral_constant<int, 1>{}, dd, pp, std::integral_constant<int, 64>{});
  };
  auto with_p = [&](auto kt, auto dd) {
    switch (poly_pad_p(p)) {
      case 1: with_lpt(kt, dd, std::integral_constant<int, 1>{}); break;
      case 2: with_lpt(kt, dd, std::integral_constant<int, 2>{}); break;
      default: with_lpt(kt, dd, std::integral_constant<int, 4>{}); break;
    }
  };
  NK_TRY(with_kernel_family(who, ktype, [&](auto kt) {
    if (poly_pad_d(d) == 2) with_p(kt, std::integral_constant<int, 2>{});
    else with_p(kt, std::integral_constant<int, 4>{});
  }));
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// all pointers device memory; out_x: batch * (steps + 1) rows of d, out_u: batch * steps rows of p
int launch_poly_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, const double* w, int64_t w_ls,
                     int64_t w_js, const double* x0, int64_t x0_stride, const double* xref, int64_t xref_stride, int steps,
                     int batch, double* out_x, int64_t ldx, double* out_u, int64_t ldu) {
  NK_REQUIRE(plant.d == mdl->d && plant.p == mdl->p && mdl->m >= 1 && mdl->m <= poly_loop_max_m(plant.d, plant.p) &&
                 steps >= 1 && batch >= 1, "poly_plant_loop: bad sizes");
  PolyLoopUnit U;  // batch member 0
  U.Z = mdl->Z; U.winv = mdl->winv; U.w = w; U.w_ls = w_ls; U.w_js = w_js; U.m = mdl->m; U.reserved = 0;
  U.sigma0sq = mdl->sigma0 * mdl->sigma0;
  U.x0 = x0; U.xref = xref; U.out_x = out_x; U.ldx = ldx; U.out_u = out_u; U.ldu = ldu;
  U.u_opt = nullptr; U.score = nullptr;
  const LoopStrides strides{x0_stride, xref_stride, 0, steps};
  const PolyProgram prog = poly_compile(plant);
  int lpt = 0, waves = 0;
  poly_loop_class(mdl->m, poly_lpt(poly_pad_d(plant.d), poly_pad_p(plant.p)), &lpt, &waves);
  return poly_loop_dispatch("poly_plant_loop", plant.d, plant.p, mdl->ktype, waves > 1 || lpt > 1, [&](auto kt, auto lp, auto dd, auto pp, auto wg) {
    hipLaunchKernelGGL((poly_loop_kernel<decltype(kt)::value, decltype(lp)::value, decltype(dd)::value, decltype(pp)::value,
                                         decltype(wg)::value>),
                       dim3(batch), dim3(64 * waves), 0, ctx->stream, U, strides, prog);
  });
}

// The multi-model form, as launch_plant_loop_multi: classes of (kernel family, landmarks per lane, waves).  `units` is
// reordered in place and must stay alive until the stream has been synchronised.
int launch_poly_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, PolyLoopUnit* units, const int* ktypes,
                           int n_units) {
  NK_REQUIRE(steps >= 1 && n_units >= 1, "poly_plant_loop_multi: bad sizes");
  const int max_m = poly_loop_max_m(plant.d, plant.p);
  NK_REQUIRE(max_m > 0, "poly_plant_loop_multi: bad plant");
  const int lpt_class = poly_lpt(poly_pad_d(plant.d), poly_pad_p(plant.p));
  for (int u = 0; u < n_units; ++u)
    NK_REQUIRE(units[u].m >= 1 && units[u].m <= max_m, "poly_plant_loop_multi: unit %d: bad m", u);
  auto key_of = [&](int u) {
    LoopClass k{ktypes[u], 0, 0};
    poly_loop_class(units[u].m, lpt_class, &k.shape, &k.waves);
    return k;
  };
  const PolyProgram prog = poly_compile(plant);
  return launch_loop_classes(ctx, units, n_units, key_of, nullptr, [&](const PolyLoopUnit* first, int count, const LoopClass& k, long) {
    return poly_loop_dispatch("poly_plant_loop_multi", plant.d, plant.p, k.ktype, k.waves > 1 || k.shape > 1, [&](auto kt, auto lp, auto dd, auto pp, auto wg) {
      hipLaunchKernelGGL((poly_loop_multi_kernel<decltype(kt)::value, decltype(lp)::value, decltype(dd)::value, decltype(pp)::value,
                                                 decltype(wg)::value>),
                         dim3(count), dim3(64 * k.waves), 0, ctx->stream, first, prog, steps);
    });
  });
}

}  // namespace nk
