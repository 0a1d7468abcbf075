// Route of a lifted recursion z_{t+1} = G [z_t; u_t] (+ bias) (nk_rollout.hip, nk_control.hip, nk_traj_err.hip): which
// kernel advances it, in how many launches, with which template instantiation and block sizes.  Host only, no HIP include,
// so that a plain C++17 compiler builds it (tests/chain_plan_main.cpp): pure functions of integers.  Every rule below is
// known here and nowhere else; tests/rollout_reference.py mirrors it line by line.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nk {

// ---- the single-workgroup chain (lifted_chain_kernel): G in the registers of one 1024-thread workgroup
constexpr int CHAIN_THREADS = 1024;
constexpr int CHAIN_KPT = 5;                // columns of G per thread (stride 32)
constexpr int CHAIN_ZU = 32 * CHAIN_KPT;    // padded length of [z ; u] in LDS (160)
constexpr int CHAIN_MAX_M = 128;
constexpr int CHAIN_BIAS_DOUBLES = 128;
constexpr int CHAIN_TB_MAX = 1024;          // most steps of controls per staged block
constexpr size_t CHAIN_LDS_MAX = 64 * 1024;

inline int chain_d_pad(int d_lift) { return d_lift > 0 ? d_lift + (d_lift & 1) : 0; }
// LDS doubles without the control block
inline size_t chain_fixed_doubles(int d_lift) {
  return 3 * (size_t)CHAIN_ZU + CHAIN_BIAS_DOUBLES + (size_t)chain_d_pad(d_lift) + 2;
}
inline bool lifted_chain_ok(int m, int pu, int d_lift) {
  if (!(m >= 1 && m <= CHAIN_MAX_M && pu >= 0 && m + pu <= CHAIN_ZU)) return false;
  return (chain_fixed_doubles(d_lift) + (size_t)pu * 16) * sizeof(double) <= CHAIN_LDS_MAX;  // >= 16 steps of controls per block
}
// steps per staged block of controls (pu: the control columns that are really read, 0 without controls)
inline int chain_tb(int pu, int d_lift, int T) {
  int tb = T > 1 ? T - 1 : 1;
  if (pu > 0) {
    const size_t room = (CHAIN_LDS_MAX - chain_fixed_doubles(d_lift) * sizeof(double)) / (sizeof(double) * (size_t)pu);
    if ((size_t)tb > room) tb = (int)room;
    if (tb > CHAIN_TB_MAX) tb = CHAIN_TB_MAX;
  }
  return tb;
}
inline size_t chain_lds_bytes(int pu, int d_lift, int tb) {
  return chain_fixed_doubles(d_lift) * sizeof(double) + (size_t)tb * (size_t)pu * sizeof(double);
}
inline int chain_control_blocks(int T, int tb) { return T > 1 ? (T - 1 + tb - 1) / tb : 0; }

// ---- the multi-workgroup chain (lifted_chain_mw_kernel<KPT, NT>)
constexpr int MW_KPT = 32;    // most 64-wide chunks of the state per lane: m <= 2048
constexpr int MW_ROWS = 16;   // rows (waves) per workgroup
constexpr int MW_MAX_PU = 64;
constexpr int MW_FEW_GROUPS = 16;  // so few groups are chunked over several launches rather than stepped

// the KPT instantiation for ceil(m / 64) chunks
inline int chain_mw_kpt_class(int kpt) { return kpt <= 4 ? 4 : kpt <= 8 ? 8 : kpt <= 16 ? 16 : 32; }
// trajectories per workgroup for a batch: NT * ceil(m / 64) <= 32 (the LDS image of the NT state vectors, two buffers)
inline int chain_mw_group(int m, int batch) {
  const int kpt = (m + 63) / 64;
  int nt = 1;
  while (nt < 4 && 2 * nt * chain_mw_kpt_class(kpt) <= 32 && 2 * nt <= batch) nt *= 2;
  return nt;
}
inline int chain_mw_workgroups(int m) { return (m + MW_ROWS - 1) / MW_ROWS; }
inline bool chain_mw_fits(int m, int pu, int num_cu) {
  return m >= 1 && m <= 64 * MW_KPT && pu >= 0 && pu <= MW_MAX_PU && chain_mw_workgroups(m) <= num_cu;
}
// Is the single-launch multi-workgroup recursion the path?  pu: the control columns of the chain, pu_read: those that are
// really read (0 without controls); allowed: the conditions that are no arithmetic (the switch is on, the context is not
// recording a lock-step group).
inline bool chain_mw_wanted_plan(int m, int pu, int pu_read, int d_lift, int T, int batch, int num_cu, bool allowed) {
  if (!allowed || T < 3) return false;
  if (lifted_chain_ok(m, pu, d_lift)) return false;
  if (!chain_mw_fits(m, pu_read, num_cu)) return false;
  const int nt = chain_mw_group(m, batch);
  const int64_t groups = (batch + nt - 1) / nt;
  return groups <= MW_FEW_GROUPS || groups * chain_mw_workgroups(m) <= num_cu;
}
// trajectories of one launch: (CUs / workgroups per trajectory group) groups of `nt`, resident side by side
inline int chain_mw_chunk(int m, int batch, int num_cu) {
  const int nt = chain_mw_group(m, batch);
  int nb = num_cu / chain_mw_workgroups(m);
  if (nb < 1) nb = 1;
  return nb * nt;
}

// ---- one launch per step
constexpr int STEP_MAX_BATCH = 8;      // trajectories of one matrix-vector launch
constexpr int STEP_GEMV_BATCH = 16;    // beyond: one GEMM per step
constexpr int STEP_INVARIANT_CHUNK = 16;  // batch-invariant recursions walk the matrix-vector steps so many at a time
inline bool step_is_gemv(int batch) { return batch <= STEP_GEMV_BATCH; }
// launches of one time step (the matrix-vector kernel takes one bias vector: trajectories with their own go one by one)
inline int step_launches(int batch, bool per_trajectory_bias) {
  return per_trajectory_bias ? batch : (batch + STEP_MAX_BATCH - 1) / STEP_MAX_BATCH;
}

// ---- the fused score (traj_err_partial_kernel): time steps per workgroup (0: m out of range)
constexpr int TERR_TT = 8;              // most time steps per tile
constexpr int TERR_LDS_DOUBLES = 4096;  // 32 KB of z rows per workgroup
inline int traj_err_tile(int m) {
  if (m < 1 || m > TERR_LDS_DOUBLES) return 0;
  const int tt = TERR_LDS_DOUBLES / m;
  return tt < TERR_TT ? tt : TERR_TT;
}

// ---- the whole decision: rollout_steps (nk_control.hip) branches on its route
enum ChainRoute { ROUTE_CHAIN = 0, ROUTE_MW = 1, ROUTE_STEP = 2, ROUTE_GEMM = 3 };
struct ChainPlan {
  int route = ROUTE_STEP;
  bool lift_in_kernel = false;     // CHAIN: z_0 = k(x_0, Z) S^-1 by the chain kernel itself
  int tb = 0, blocks = 0;          // CHAIN: steps per control block, control blocks
  int kpt = 0, nt = 0;             // MW: the instantiation lifted_chain_mw_kernel<kpt, nt> (of the first launch)
  int groups = 0, launches = 0;    // MW: trajectory groups of the first launch, launches of the call
  int launches_per_step = 0;       // STEP / GEMM: launches of one time step over the whole batch
};
// p: control columns (0 without controls or when T == 1); d_lift: dimension of the states a Nystrom model lifts from, 0 when
// z_0 is given or lifted elsewhere (explicit operators, spline model, closed loop); mw_allowed: the multi-workgroup switch is
// on and the context is not recording a lock-step group.
inline ChainPlan chain_plan(int m, int p, int d_lift, int T, int batch, int num_cu, bool batch_invariant,
                            bool per_trajectory_bias, bool mw_allowed = true) {
  ChainPlan pl;
  const int pu = T > 1 ? p : 0;
  pl.lift_in_kernel = d_lift > 0 && lifted_chain_ok(m, pu, d_lift);
  const int dl = pl.lift_in_kernel ? d_lift : 0;
  if (lifted_chain_ok(m, pu, dl)) {
    pl.route = ROUTE_CHAIN;
    pl.tb = chain_tb(pu, dl, T);
    pl.blocks = chain_control_blocks(T, pl.tb);
    return pl;
  }
  if (!batch_invariant && chain_mw_wanted_plan(m, pu, pu, dl, T, batch, num_cu, mw_allowed)) {
    pl.route = ROUTE_MW;
    const int nb = chain_mw_chunk(m, batch, num_cu);
    const int first = batch < nb ? batch : nb;
    pl.kpt = chain_mw_kpt_class((m + 63) / 64);
    pl.nt = chain_mw_group(m, first);
    pl.groups = (first + pl.nt - 1) / pl.nt;
    pl.launches = (batch + nb - 1) / nb;
    return pl;
  }
  if (batch_invariant) {  // matrix-vector steps, STEP_INVARIANT_CHUNK trajectories at a time
    pl.route = ROUTE_STEP;
    for (int b0 = 0; b0 < batch; b0 += STEP_INVARIANT_CHUNK)
      pl.launches_per_step += step_launches(batch - b0 < STEP_INVARIANT_CHUNK ? batch - b0 : STEP_INVARIANT_CHUNK, per_trajectory_bias);
    return pl;
  }
  if (step_is_gemv(batch)) {
    pl.route = ROUTE_STEP;
    pl.launches_per_step = step_launches(batch, per_trajectory_bias);
  } else {
    pl.route = ROUTE_GEMM;
    pl.launches_per_step = (per_trajectory_bias ? 1 : 0) + 1 + (pu > 0 ? 1 : 0);
  }
  return pl;
}

}  // namespace nk
