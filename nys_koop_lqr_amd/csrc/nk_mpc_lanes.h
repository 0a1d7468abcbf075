// The small lane helpers the two MPC loops share (nk_mpc_loop.hip, nk_mpc_out_loop.hip).
#pragma once
#include "nk_common.h"
#include "nk_poly_lanes.h"

#include <type_traits>

namespace nk {

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
// loop uses are therefore given the global address space by hand (kernel arguments get it from the compiler).
typedef const double __attribute__((address_space(1)))* gconst_f64;
typedef double __attribute__((address_space(1)))* gmut_f64;

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// launch(kernel family, D, NVP), host side, for a model's kernel family, the plant's padded states and nv lanes of the QP
template <class F>
inline int mpc_loop_dispatch(const char* who, int ktype, int d, int nv, F&& go) {
  auto with_nv = [&](auto kt, auto dd) {
    if (nv <= 16) go(kt, dd, std::integral_constant<int, 16>{});
    else if (nv <= 32) go(kt, dd, std::integral_constant<int, 32>{});
    else go(kt, dd, std::integral_constant<int, 64>{});
  };
  auto with_d = [&](auto kt) {
    if (poly_pad_d(d) == 2) with_nv(kt, std::integral_constant<int, 2>{});
    else with_nv(kt, std::integral_constant<int, 4>{});
  };
  switch (ktype) {
    case NK_KERNEL_RBF: with_d(std::integral_constant<int, NK_KERNEL_RBF>{}); break;
    case NK_KERNEL_MATERN52: with_d(std::integral_constant<int, NK_KERNEL_MATERN52>{}); break;
    case NK_KERNEL_LINEAR: with_d(std::integral_constant<int, NK_KERNEL_LINEAR>{}); break;
    case NK_KERNEL_TPS: with_d(std::integral_constant<int, NK_KERNEL_TPS>{}); break;
    default: set_error("%s: unknown kernel type %d", who, ktype); return NK_ERR_BAD_ARG;
  }
  return NK_OK;
}

}  // namespace nk
