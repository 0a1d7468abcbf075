// Staging layout of the controller build (nk_mpc_build_batch, nk_model_mpc_build_batch; nk_api_mpc_build.hip): host only, no
// HIP include, so that a plain C++17 compiler builds it (tests/mpc_build_pack_main.cpp).
//
// A call lays the host operands of a group of units out in ONE block of doubles (`in`, one host-to-device copy), the results
// in another (`out`, one device-to-host copy), and the per-unit device workspace in a third that no host bytes exist for
// (`ws`).  Every piece is dense (leading dimension = its column count), starts on a slot boundary (nk_unit_pack.h) and is
// +0.0 beyond the doubles copied into it.
#pragma once
#include "nk_unit_pack.h"

namespace nk {

constexpr size_t MPC_BUILD_NONE = ~(size_t)0;  // the offset of a piece that the unit does not have

inline size_t mpc_build_pad(size_t n) { return (n + 15) & ~(size_t)15; }

// What a unit is, as far as the layout goes.  host_ops: A, B, Q, R travel in `in` (nk_mpc_build_batch; a model's operators
// stay where they are); have_R: R travels (the model entry with R = NULL has the identity); have_P: the terminal cost is given
// (no Riccati stage: nothing of it in `ws`); want_P: P travels back; nc, Ny: the output rows (nc = 0: none); host_C: the nc
// rows of C travel in `in`.
struct MpcBuildShape {
  size_t m = 0, p = 0, N = 0, nc = 0, Ny = 0;
  bool host_ops = false, have_R = false, have_P = false, want_P = false, host_C = false;
};

struct MpcBuildOffsets {
  // `in`
  size_t A = MPC_BUILD_NONE, B = MPC_BUILD_NONE, Q = MPC_BUILD_NONE, R = MPC_BUILD_NONE, P = MPC_BUILD_NONE,
         C = MPC_BUILD_NONE;
  // `out`: H (nv x nv), F (nv x m), K (p x m), P (m x m), G (Ny nc x nv), T (Ny nc x m)
  size_t H = 0, F = 0, K = 0, outP = MPC_BUILD_NONE, G = MPC_BUILD_NONE, T = MPC_BUILD_NONE;
  // `ws`: the Riccati stage's K (p x m) and P (m x m), dense; the six M x M slots; the NVP-wide area
  size_t rK = MPC_BUILD_NONE, rP = MPC_BUILD_NONE, sq = 0, wide = 0;
};

// doubles of the NVP-wide area: G stack, Q G, P G, W twice (M x NVP each); one M x 16 and two 16 x M temporaries, one
// 16 x NVP temporary; the nc x p products R_k B of the output rows (Ny of them)
inline size_t mpc_build_wide_doubles(size_t M, size_t NVP, size_t Ny, size_t nc, size_t p) {
  return 5 * M * NVP + 16 * M + 2 * 16 * M + 16 * NVP + unit_slot(Ny * nc * p);
}
// doubles of a unit's workspace without the Riccati stage's results
inline size_t mpc_build_ws_doubles(size_t m, size_t nv, size_t Ny, size_t nc, size_t p) {
  const size_t M = mpc_build_pad(m), NVP = mpc_build_pad(nv);
  return unit_slot(6 * M * M) + unit_slot(mpc_build_wide_doubles(M, NVP, Ny, nc, p));
}

inline MpcBuildOffsets pack_mpc_build_unit(UnitPack& in, UnitPack& out, UnitPack& ws, const MpcBuildShape& s, const double* A,
                                           size_t lda, const double* B, size_t ldb, const double* Q, size_t ldq,
                                           const double* R, size_t ldr, const double* P, size_t ldp, const double* C,
                                           size_t ldc) {
  MpcBuildOffsets o;
  const size_t m = s.m, p = s.p, nv = s.N * s.p, ny = s.nc ? s.Ny * s.nc : 0;
  auto dense = [&in](const double* src, size_t ld, size_t rows, size_t cols) {
    const size_t at = in.reserve(rows * cols);
    if (src)
      for (size_t i = 0; i < rows; ++i) in.copy(at + i * cols, src + i * ld, cols);
    return at;
  };
  if (s.host_ops) {
    o.A = dense(A, lda, m, m);
    o.B = dense(B, ldb, m, p);
    o.Q = dense(Q, ldq, m, m);
  }
  if (s.have_R) o.R = dense(R, ldr, p, p);
  if (s.have_P) o.P = dense(P, ldp, m, m);
  if (s.host_C && s.nc) o.C = dense(C, ldc, s.nc, m);
  o.H = out.reserve(nv * nv);
  o.F = out.reserve(nv * m);
  o.K = out.reserve(p * m);
  if (s.want_P) o.outP = out.reserve(m * m);
  if (ny) {
    o.G = out.reserve(ny * nv);
    o.T = out.reserve(ny * m);
  }
  if (!s.have_P) {
    o.rK = ws.reserve(p * m);
    o.rP = ws.reserve(m * m);
  }
  const size_t M = mpc_build_pad(m), NVP = mpc_build_pad(nv);
  o.sq = ws.reserve(6 * M * M);
  o.wide = ws.reserve(mpc_build_wide_doubles(M, NVP, s.nc ? s.Ny : 0, s.nc, p));
  return o;
}

}  // namespace nk
