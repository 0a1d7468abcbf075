// What the single-launch closed loops share (nk_plant_loop.hip, nk_mpc_loop.hip): the small lane helpers, the record of batch
// member b from the record of member 0, ONE statement of each score and of a step's stores, the lift set-up and the gradient
// pass of the MPC loops, and on the host the kernel-family switch and the class launcher of the multi-model forms.  Every device
// helper is inlined, works on values, and spells its arithmetic in the order the loops always had: the explicit fma calls and
// the `fp contract(off)` blocks are part of the results' bits.
#pragma once
#include "nk_common.h"
#include "nk_loop_classes.h"
#include "nk_poly_lanes.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace nk {

// sum of one value over the 16 lanes of a DPP row, in every lane of the row
__device__ __forceinline__ double row_sum16_dpp(double c) {
  c += dpp_f64<0xB1>(c);   // quad_perm [1,0,3,2]
  c += dpp_f64<0x4E>(c);   // quad_perm [2,3,0,1]
  c += dpp_f64<0x141>(c);  // row_half_mirror
  c += dpp_f64<0x140>(c);  // row_mirror
  return c;
}

// max of one value over the 64 lanes, in every lane (the butterfly of wave_sum64_dpp)
__device__ __forceinline__ double wave_max64_dpp(double c) {
  c = fmax(c, dpp_f64<0xB1>(c));
  c = fmax(c, dpp_f64<0x4E>(c));
  c = fmax(c, dpp_f64<0x141>(c));
  c = fmax(c, dpp_f64<0x140>(c));
  double a = c, b = c;
  swap16_f64(a, b);
  c = fmax(a, b);
  a = c; b = c;
  swap32_f64(a, b);
  return fmax(a, b);
}

// the value of lane j (uniform) in every lane
__device__ __forceinline__ double lane_bcast(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// A record read from a device table carries generic pointers, and generic (flat) accesses count against the LDS counter too:
// the per-step "s_waitcnt lgkmcnt(0)" before a barrier would then wait for global loads and stores.  The pointers the step
// loop of the MPC bodies uses are therefore given the global address space by hand (kernel arguments get it from the compiler).
typedef const double __attribute__((address_space(1)))* gconst_f64;
typedef double __attribute__((address_space(1)))* gmut_f64;

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// ---- a batch as one record: the kernels of the single calls take the record of member 0 and the strides to member b
struct LoopStrides {
  int64_t x0, xref, uinit;  // doubles between the members' initial states, references (0: shared) and seed controls
  int steps;
};
template <class Unit>
__device__ __forceinline__ Unit unit_of_block(const Unit& base, const LoopStrides& s, int b) {
  Unit U = base;
  U.x0 = base.x0 + (int64_t)b * s.x0;
  U.xref = base.xref + (int64_t)b * s.xref;
  U.out_x = base.out_x + (int64_t)b * (s.steps + 1) * base.ldx;  // rows b * (steps + 1) + t
  U.out_u = base.out_u + (int64_t)b * s.steps * base.ldu;        // rows b * steps + t
  return U;
}
__device__ __forceinline__ MpcLoopUnit unit_of_block(const MpcLoopUnit& base, const LoopStrides& s, int b) {
  MpcLoopUnit U = unit_of_block<MpcLoopUnit>(base, s, b);
  U.uinit = base.uinit ? base.uinit + (int64_t)b * s.uinit : nullptr;
  U.out_info = base.out_info ? base.out_info + (int64_t)b * s.steps * 2 : nullptr;  // rows b * steps + t, 2 columns
  return U;
}

// ---- the scores: sse = sum (u_t - u_opt[t])^2, sso = sum u_opt[t]^2, J = the running cost of the reference's
// open_loop_control in its order, umax = max |u_t|, NaN from the first NaN control on
// v_0^2 + v_1^2 + ... in index order, every product and sum rounded
template <int N>
__device__ __forceinline__ double sum_sq_ordered(const double (&v)[N]) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double sq = v[k] * v[k];
    s = k == 0 ? sq : s + sq;
  }
  return s;
}
// the larger of v and cur; a NaN enters once and stays: no later comparison is true
__device__ __forceinline__ double sticky_max(double v, double cur) { return (v > cur || v != v) ? v : cur; }
// one step of J and umax from x_{t+1} and u_t
template <int D, int P>
__device__ __forceinline__ void score_cost_step(const double (&x)[D], const double (&u)[P], double& J, double& umax) {
#pragma clang fp contract(off)
  const double sx = sum_sq_ordered(x), su = sum_sq_ordered(u);
#pragma unroll
  for (int j = 0; j < P; ++j) umax = sticky_max(fabs(u[j]), umax);
  J = (J + sx) + su;
}
// one step of sse and sso over the inputs in index order; uo: the row of u_opt of this step, replaced by row tn (next step's
// values, loaded a step ahead: not on the chain).  The loads stand in a loop of their own behind the sums: inside the loop of
// the sums they cost the scored polynomial kernels up to six VGPRs.
template <int P, class Ptr>
__device__ __forceinline__ void score_uopt_step(const double (&u)[P], double (&uo)[P], Ptr uopt, int64_t tn, int p,
                                                double& sse, double& sso) {
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double df = u[j] - uo[j];
      const double dsq = df * df, osq = uo[j] * uo[j];
      sse = sse + dsq;
      sso = sso + osq;
    }
  }
#pragma unroll
  for (int j = 0; j < P; ++j)
    if (j < p) uo[j] = uopt[tn * p + j];
}

// the stores of step t, by one thread: u_t (p of P entries) and x_{t+1} (d of D entries)
template <int D, int P, class Ptr>
__device__ __forceinline__ void store_step(Ptr ou, bool st_u, int64_t ldu, Ptr ox, bool st_x, int64_t ldx, int64_t t,
                                           const double (&u)[P], int p, const double (&x)[D], int d) {
  if (st_u) {
#pragma unroll
    for (int j = 0; j < P; ++j)
      if (j < p) ou[t * ldu + j] = u[j];
  }
  if (st_x) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k < d) ox[(t + 1) * ldx + k] = x[k];
  }
}

// ---- the MPC loops: one landmark per lane
// the lift set-up of thread tid: inverse length scales, its scaled landmark, the initial state and its kernel value at x_ref
template <int KTYPE, int D>
__device__ __forceinline__ void mpc_lift_setup(const MpcLoopUnit& Q, int d, int tid, double (&wi)[D], double (&zs)[D],
                                               double (&x)[D], double& kref) {
  const double* x0 = Q.x0;
  const double* xrp = Q.xref;
  const bool have = tid < Q.m;  // a lane without a landmark: landmark 0, and its dk is never read
#pragma unroll
  for (int k = 0; k < D; ++k) {
    wi[k] = k < d ? Q.winv[k] : 0.0;
    x[k] = k < d ? x0[k] : 0.0;
  }
  {
#pragma clang fp contract(off)
    double xrs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      zs[k] = (have && k < d) ? Q.Z[(int64_t)tid * d + k] * wi[k] : 0.0;
      xrs[k] = (k < d ? xrp[k] : 0.0) * wi[k];
    }
    kref = plant_kval<KTYPE, D>(xrs, zs, Q.sigma0sq);
  }
}
// The per-wave pass over W (m x nt in LDS): this wave's sum of W[l][lane] dk_l over ITS landmarks l0 .. l0 + cnt - 1 in index
// order, dk_l = k(z_l, x) - kref_l arriving by v_readlane, stored as word 64 wave + lane of `part`; then the LDS-only barrier
// (the global stores of earlier steps need not have retired: nothing reads them back).  The word's index is formed here from
// wave and lane: handed the address of the wave's words instead, every MPC kernel takes one or two VGPRs more.
template <int KTYPE, int D>
__device__ __forceinline__ void mpc_w_pass(const double (&x)[D], const double (&wi)[D], const double (&zs)[D], double kref,
                                           double sigma0sq, const double* Wl, int nt, int l0, int cnt, bool row, int lane,
                                           int wave, double* part) {
  double dk;
  {
#pragma clang fp contract(off)
    double xs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xs[k] = x[k] * wi[k];
    dk = plant_kval<KTYPE, D>(xs, zs, sigma0sq) - kref;
  }
  double acc = 0.0;
  {
    const double* wr = Wl + (size_t)l0 * nt + (row ? lane : 0);  // lanes without a row read column 0 and drop the sum
    for (int l = 0; l < cnt; ++l) acc = fma(wr[(size_t)l * nt], lane_bcast(dk, l), acc);
  }
  part[64 * wave + lane] = row ? acc : 0.0;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// f(kernel family), the run-time id as a std::integral_constant
template <class F>
inline int with_kernel_family(const char* who, int ktype, F&& f) {
  switch (ktype) {
    case NK_KERNEL_RBF: f(std::integral_constant<int, NK_KERNEL_RBF>{}); break;
    case NK_KERNEL_MATERN52: f(std::integral_constant<int, NK_KERNEL_MATERN52>{}); break;
    case NK_KERNEL_LINEAR: f(std::integral_constant<int, NK_KERNEL_LINEAR>{}); break;
    case NK_KERNEL_TPS: f(std::integral_constant<int, NK_KERNEL_TPS>{}); break;
    default: set_error("%s: unknown kernel type %d", who, ktype); return NK_ERR_BAD_ARG;
  }
  return NK_OK;
}

// launch(kernel family, D, NP) for a model's kernel family, the plant's padded states and nv lanes of the QP
template <class F>
inline int mpc_loop_dispatch(const char* who, int ktype, int d, int nv, F&& go) {
  return with_kernel_family(who, ktype, [&](auto kt) {
    auto with_nv = [&](auto dd) {
      if (nv <= 16) go(kt, dd, std::integral_constant<int, 16>{});
      else if (nv <= 32) go(kt, dd, std::integral_constant<int, 32>{});
      else go(kt, dd, std::integral_constant<int, 64>{});
    };
    if (poly_pad_d(d) == 2) with_nv(std::integral_constant<int, 2>{});
    else with_nv(std::integral_constant<int, 4>{});
  });
}

// The multi-model forms: `units` (host records holding device pointers, already checked) are sorted into the classes of
// nk_loop_classes.h -- stable, so the order inside a class is the caller's --, staged with ONE copy and run with one
// launch(first record on the device, count, class, largest LDS need) per class.  key_of(u) / lds_of(u): the class and the LDS
// need of the caller's unit u (lds_of = nullptr: the loops need no dynamic LDS, and launch gets 0).  `units` is reordered in
// place and must stay alive until the stream has been synchronised (the copy reads it).
template <class Unit, class KeyOf, class LdsOf, class Launch>
int launch_loop_classes(nk_ctx* ctx, Unit* units, int n_units, KeyOf&& key_of, LdsOf&& lds_of, Launch&& launch) {
  std::vector<LoopClass> keys((size_t)n_units);
  std::vector<long> lds;
  for (int u = 0; u < n_units; ++u) {
    keys[(size_t)u] = key_of(u);
    if constexpr (!std::is_null_pointer_v<std::decay_t<LdsOf>>) lds.push_back(lds_of(u));
  }
  const LoopClassPlan plan = plan_loop_classes(keys.data(), n_units, lds.empty() ? nullptr : lds.data());
  {
    std::vector<Unit> sorted((size_t)n_units);
    for (int u = 0; u < n_units; ++u) sorted[(size_t)u] = units[plan.perm[(size_t)u]];
    std::copy(sorted.begin(), sorted.end(), units);
  }
  Unit* table = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n_units, &table));
  NK_HIP(hipMemcpyAsync(table, units, sizeof(Unit) * (size_t)n_units, hipMemcpyHostToDevice, ctx->stream));
  for (const LoopRun& run : plan.runs) NK_TRY(launch((const Unit*)table + run.begin, run.end - run.begin, run.key, run.lds));
  return NK_OK;
}

}  // namespace nk
