// Staging layout of the unit-table calls (nk_plant_loop_multi, nk_mpc_loop_multi, nk_mpc_out_loop_multi, nk_closed_loop_multi;
// nk_api_loops.hip): host only, no HIP include, so that a plain C++17 compiler builds it (tests/unit_pack_main.cpp,
// tests/mpc_unit_pack_main.cpp, tests/mpc_out_unit_pack_main.cpp).
//
// A call lays the operands of all its units out in ONE block of doubles that a single host-to-device copy moves; the
// device records then point into the copy.  Every piece starts on a slot boundary (32 doubles = 256 bytes) and what a
// piece reserves beyond the doubles copied into it is +0.0.  A region that only the device writes (a workspace, the
// folded gains) is laid out with the same offsets and never asks for the block: no host bytes exist for it.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstring>
#include <vector>

namespace nk {

// the slot rule: sizes round up to 32 doubles
inline size_t unit_slot(size_t doubles) { return (doubles + 31) & ~(size_t)31; }

// Reserved length of a gain row of m entries (p = 1): the even leading dimension that stage_in gives the 1 x m gain of
// nk_plant_loop, so that the fold of a unit sees the operands of the single call.
inline size_t gain_row_reserve(size_t m) { return m + (m & 1); }

class UnitPack {
 public:
  // slot(doubles) zero doubles at the end of the layout; the offset of the first
  size_t reserve(size_t doubles) {
    const size_t at = total_;
    total_ += unit_slot(doubles);
    return at;
  }
  // `count` doubles from `src` go to offset `at` of a reserved piece (a null source leaves the zeros); `src` is read by
  // block() and must stay alive until then
  void copy(size_t at, const double* src, size_t count) {
    assert(at + count <= total_);
    if (src && count) pieces_.push_back(Piece{src, at, count});
  }
  size_t append(const double* src, size_t count, size_t reserve_doubles) {
    assert(count <= reserve_doubles);
    const size_t at = reserve(reserve_doubles);
    copy(at, src, count);
    return at;
  }
  size_t append(const double* src, size_t count) { return append(src, count, count); }
  size_t doubles() const { return total_; }
  // the finished block for the one copy: doubles() doubles, valid while the pack lives and nothing is added
  const double* block() {
    block_.assign(total_, 0.0);
    for (const Piece& p : pieces_) memcpy(block_.data() + p.at, p.src, p.count * sizeof(double));
    return block_.data();
  }

 private:
  struct Piece { const double* src; size_t at, count; };
  size_t total_ = 0;
  std::vector<Piece> pieces_;
  std::vector<double> block_;
};

// ---- the two layouts ---------------------------------------------------------------------------------------------------
// A plant unit (nk_plant_loop_multi).  `in`: K (reserved as a gain row) | x0, x_ref together in one piece of 2 d.
// `folds` (device only): the folded gain of a unit that has one, m + 2 doubles.
struct PlantUnitOffsets { size_t K = 0, x0 = 0, x_ref = 0, w = 0; };
inline PlantUnitOffsets pack_plant_unit(UnitPack& in, UnitPack& folds, const double* K, const double* x0, const double* x_ref,
                                        size_t m, size_t d, bool fold) {
  PlantUnitOffsets o;
  o.K = in.append(K, m, gain_row_reserve(m));
  o.x0 = in.reserve(2 * d);
  o.x_ref = o.x0 + d;
  in.copy(o.x0, x0, d);
  in.copy(o.x_ref, x_ref, d);
  if (fold) o.w = folds.reserve(m + 2);
  return o;
}

// A unit of the polynomial-plant form (nk_poly_plant_loop_multi), p inputs.  `in`: the p rows of K, each with the leading
// dimension of a gain row (what stage_in gives the p x m gain of nk_poly_plant_loop) | x0, x_ref together in one piece of
// 2 d.  `folds` (device only): the folded gain of a unit that has one, m p + 2 doubles.
struct PolyUnitOffsets { size_t K = 0, x0 = 0, x_ref = 0, w = 0; };
inline PolyUnitOffsets pack_poly_unit(UnitPack& in, UnitPack& folds, const double* K, const double* x0, const double* x_ref,
                                      size_t m, size_t d, size_t p, bool fold) {
  PolyUnitOffsets o;
  const size_t ldk = gain_row_reserve(m);
  o.K = in.reserve(p * ldk);
  for (size_t j = 0; j < p; ++j) in.copy(o.K + j * ldk, K + j * m, m);
  o.x0 = in.reserve(2 * d);
  o.x_ref = o.x0 + d;
  in.copy(o.x0, x0, d);
  in.copy(o.x_ref, x_ref, d);
  if (fold) o.w = folds.reserve(m * p + 2);
  return o;
}

// A unit of the constrained MPC loop (nk_mpc_loop_multi), nv decision variables (iters = 0: nv = p and G the gain K).
// `in`: the constants [M | H^-1 | lo hi dlo dhi] in one piece of 2 nn + 4 nv doubles (nn = nv^2; nn = 0 when `qp` is false:
// the saturated LQR has no M and no H^-1) | G -- fold = true: its nv rows of m entries, each with the leading dimension of
// a gain row (what stage_in gives the nv x m matrix of nk_mpc_loop); fold = false (a spline model): the m x nv transpose
// the caller formed, dense | x0, x_ref, u_init together in one piece of 2 d + p (a null u_init leaves zeros).
// `folds` (device only): the folded W of a unit that has one, m nv + 2 doubles.
// A unit that shares model and description with an earlier unit of the call may share that unit's prepared pieces (the
// constants, G and the fold): pack_mpc_unit_state lays out its own x0, x_ref, u_init alone and the other offsets are copied.
struct MpcUnitOffsets { size_t M = 0, Hinv = 0, bnd = 0, G = 0, x0 = 0, x_ref = 0, u_init = 0, w = 0; };
inline void pack_mpc_unit_state(UnitPack& in, MpcUnitOffsets& o, const double* x0, const double* x_ref, const double* u_init,
                                size_t d, size_t p) {
  o.x0 = in.reserve(2 * d + p);
  o.x_ref = o.x0 + d;
  o.u_init = o.x_ref + d;
  in.copy(o.x0, x0, d);
  in.copy(o.x_ref, x_ref, d);
  in.copy(o.u_init, u_init, p);
}
inline MpcUnitOffsets pack_mpc_unit(UnitPack& in, UnitPack& folds, const double* consts, const double* G, const double* x0,
                                    const double* x_ref, const double* u_init, size_t m, size_t nv, size_t d, size_t p, bool qp,
                                    bool fold) {
  MpcUnitOffsets o;
  const size_t nn = qp ? nv * nv : 0;
  o.M = in.append(consts, 2 * nn + 4 * nv);
  o.Hinv = o.M + nn;
  o.bnd = o.M + 2 * nn;
  if (fold) {
    const size_t ldg = gain_row_reserve(m);
    o.G = in.reserve(nv * ldg);
    for (size_t i = 0; i < nv; ++i) in.copy(o.G + i * ldg, G + i * m, m);
  } else {
    o.G = in.append(G, m * nv);
  }
  pack_mpc_unit_state(in, o, x0, x_ref, u_init, d, p);
  if (fold) o.w = folds.reserve(m * nv + 2);
  return o;
}

// A unit of nk_mpc_out_loop_multi with output rows, nt = nv + ny lanes.  `in`: the constants [Kb | S0' | lo hi dlo dhi ycomp]
// in one piece of nt^2 + nv nt + 5 nt doubles (what mpc_out_prepare and the bounds of nk_mpc_out_loop give) | FT = [F; T] --
// fold = true: its nt rows of m entries, each with the leading dimension of a gain row (what stage_in gives the nt x m
// matrix of nk_mpc_out_loop); fold = false (a spline model): the m x nt transpose the caller formed, dense | x0, x_ref,
// u_init together in one piece of 2 d + p (a null u_init leaves zeros).  `folds` (device only): the folded W of a unit that
// has one, m nt + 2 doubles.  Units that share model, description and output description may share the prepared pieces of
// the first of them: pack_mpc_out_unit_state lays out x0, x_ref, u_init alone and the other offsets are copied.
struct MpcOutUnitOffsets { size_t Kb = 0, S0t = 0, bnd = 0, FT = 0, x0 = 0, x_ref = 0, u_init = 0, w = 0; };
inline void pack_mpc_out_unit_state(UnitPack& in, MpcOutUnitOffsets& o, const double* x0, const double* x_ref,
                                    const double* u_init, size_t d, size_t p) {
  o.x0 = in.reserve(2 * d + p);
  o.x_ref = o.x0 + d;
  o.u_init = o.x_ref + d;
  in.copy(o.x0, x0, d);
  in.copy(o.x_ref, x_ref, d);
  in.copy(o.u_init, u_init, p);
}
inline MpcOutUnitOffsets pack_mpc_out_unit(UnitPack& in, UnitPack& folds, const double* consts, const double* FT,
                                           const double* x0, const double* x_ref, const double* u_init, size_t m, size_t nv,
                                           size_t ny, size_t d, size_t p, bool fold) {
  MpcOutUnitOffsets o;
  const size_t nt = nv + ny;
  o.Kb = in.append(consts, nt * nt + nv * nt + 5 * nt);
  o.S0t = o.Kb + nt * nt;
  o.bnd = o.S0t + nv * nt;
  if (fold) {
    const size_t ldg = gain_row_reserve(m);
    o.FT = in.reserve(nt * ldg);
    for (size_t i = 0; i < nt; ++i) in.copy(o.FT + i * ldg, FT + i * m, m);
  } else {
    o.FT = in.append(FT, m * nt);
  }
  pack_mpc_out_unit_state(in, o, x0, x_ref, u_init, d, p);
  if (fold) o.w = folds.reserve(m * nt + 2);
  return o;
}

// A loop unit (nk_closed_loop_multi).  `in`: K (p x m) | phi0 | phi_ref | target (d, may be null) | u_init (p, may be null).
// `ws` (device only): phi_t of every step | sum u^2 per step | sum (x - target)^2 per step.
struct LoopUnitOffsets { size_t K = 0, phi0 = 0, phi_ref = 0, target = 0, u_init = 0, Phi = 0, usq = 0, sse = 0; };
inline LoopUnitOffsets pack_loop_unit(UnitPack& in, UnitPack& ws, const double* K, const double* phi0, const double* phi_ref,
                                      const double* target, const double* u_init, size_t m, size_t p, size_t d, size_t steps) {
  LoopUnitOffsets o;
  o.K = in.append(K, p * m);
  o.phi0 = in.append(phi0, m);
  o.phi_ref = in.append(phi_ref, m);
  o.target = in.append(target, d);
  o.u_init = in.append(u_init, p);
  o.Phi = ws.reserve(steps * m);
  o.usq = ws.reserve(steps);
  o.sse = ws.reserve(steps);
  return o;
}

}  // namespace nk
