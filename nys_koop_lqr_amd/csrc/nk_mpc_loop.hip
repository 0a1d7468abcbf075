// Constrained Koopman MPC around a polynomial plant as ONE launch (nk_mpc_loop and, with limits on predicted states,
// nk_mpc_out_loop; include/nyskoop.h): every step lifts the measured state, forms the gradient g = F (phi(x_t) - phi(x_ref)) of
// the condensed QP, runs the fixed-step ADMM iteration of the interface under box and rate limits, applies the first move and
// advances the plant by one Runge-Kutta step (nk_poly_plant.h).  One workgroup per trajectory, ceil(m / 64) <= 8 waves, one
// landmark per lane, nothing from the host per step.  ONE loop body, mpc_loop_body<KTYPE, D, NP, OUT, SCORED>, on nt lanes of the
// first wave: nt = nv without output rows (OUT = false), nt = nv + ny with them; what only one form has stands under
// `if constexpr (OUT)`, so each form compiles the statements it always had.
//   gradient:  F (OUT: [F; T]) is folded into the lift once per call, W = S^-1 F' (m x nt, row l at W + l nt; spline models: F'),
//              and copied to LDS.  A lane evaluates dk_l = k(z_l, x_t) - k(z_l, x_ref) for its landmark (the arithmetic of
//              plant_kval); wave w sums W[l][i] dk_l over ITS OWN 64 landmarks in index order, lane i owning row i and dk_l
//              arriving by v_readlane (no LDS round trip, no barrier); one LDS word per wave and row, ONE barrier, and the first
//              wave adds the words in wave order: lane i < nv holds g_i, lane nv + r the shift t_r of output row r.
//   QP:        in the first wave only, then a broadcast -- with five to eight waves on four SIMDs a QP replicated in every
//              wave would share its issue slots with a second copy of itself, and the iteration is the long part of a step.
//              Lane i owns row i: its row of M (OUT: of Kb, s_K = (s_1, s_3)) in registers (NP doubles), the right-hand side
//              broadcast entry by entry with v_readlane (two per entry) into NP FMAs in index order; D and D' are shifts by p
//              lanes among the input lanes (ds_bpermute, no memory); max |s - z| by a DPP / permlane butterfly; the stop is
//              uniform over the wave.  An output lane carries one row: its shifted bounds (ylo_r - x_ref[ycomp_r]) - t_r where an
//              input lane holds lo / hi, the soft prox c + theta (v - c), and zeros in the rate slot, so it takes no part in the
//              shifts.  H^-1 (OUT: S0 = [H^-1; G H^-1], stored transposed) is needed once per step, for the start: lane i reads
//              word j nt + i of global memory (32 KB at most, the same for every workgroup, cache resident) -- LDS is W's.
//   plant:     the same wave advances the plant (PolyLanes: all terms at once in the lanes) and writes x_{t+1} to LDS; a
//              second barrier, and every wave reads it.  Two LDS-only barriers per step.
// iters = 0 (the saturated LQR, OUT = false only) runs the same kernel with W = S^-1 K' (nv := p): v = -g and the two clips.
// Every summation order is fixed by (m, nv, ny, p) alone, so a trajectory has the same bits alone or in any batch.
// The kernels of the single calls build the record of their trajectory (MpcLoopUnit, nk_common.h) from the record of batch
// member 0 and the block index; the multi-model forms (nk_mpc_loop_multi, nk_mpc_out_loop_multi) read it from a device table,
// one launch per class of (kernel family, D, NP, waves), and score every unit in its first wave; a unit has the bits of the
// single call whatever else the launch holds.
#include "nk_common.h"
#include "nk_mpc.h"
#include "nk_loop_lanes.h"
#include "nk_poly_lanes.h"

#include <algorithm>
#include <type_traits>

namespace nk {

// The loop of one workgroup on the record of one trajectory.  SCORED = false: the single calls (out_x and out_u are stored,
// out_info when it is given, nothing is scored).  SCORED = true: the multi-model forms -- every output may be null, and lane 0
// of the first wave accumulates the scores in step order: the floating-point ones in the spare words of the broadcast state
// (mpc_lds_doubles reserves 16 words: x_{t+1} takes 4, the scores 5, with output rows 6), the counters as wave-uniform
// integers.  y_viol_max / n_y_viol (OUT): an output lane keeps its ABSOLUTE bounds and its component and forms
// max(ylo - x_{t+1}[c], x_{t+1}[c] - yhi, 0) from the new state, which every lane of the first wave holds (the plant step
// works on broadcast values only); one butterfly gives the maximum of the step, a ballot its NaN case.
template <int KTYPE, int D, int NP, bool OUT, bool SCORED>
__device__ __forceinline__ void mpc_loop_body(const MpcLoopUnit& Q, const PolyProgram& pl, int steps, double* mpc_lds) {
  constexpr int P = NK_POLY_MAX_P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const int m = Q.m, nv = Q.nv, d = pl.d, p = pl.p;
  int nt = nv;
  if constexpr (OUT) nt = Q.nv + Q.ny;
  bool cheap = false;
  if constexpr (!OUT) cheap = Q.iters == 0;
  double* Wl = mpc_lds;                       // m x nt
  double* part = Wl + (size_t)m * nt;         // waves x 64
  double* xb = part + 64 * waves;             // D words of x_{t+1}
  double* sc = xb + 4;                        // SCORED: sse_u, ss_opt, J, u_absmax, r_max, OUT: y_viol_max (lane 0 of the first wave only)
  for (int i = tid; i < m * nt; i += nthreads) Wl[i] = Q.w[i];
  const PolyLanes tb(pl, lane);
  double wi[D], zs[D], x[D], kref;
  mpc_lift_setup<KTYPE, D>(Q, d, tid, wi, zs, x, kref);
  // the first wave: lane i < nv owns decision variable i, lane nv + r output row r
  const bool var = lane < nv;
  bool row = var, outl = false;
  const double inf = __builtin_huge_val();
  double theta = 0.0;
  if constexpr (OUT) {
    row = lane < nt;
    outl = row && !var;
    theta = outl ? Q.theta : 0.0;
  }
  double Krow[NP], lo = -inf, hi = inf, dlo0 = -inf, dhi0 = inf, uprev = 0.0;
  double ylo_a = -inf, yhi_a = inf;  // OUT, SCORED: the absolute bounds of an output lane with a component (yc >= 0)
  int yc = -1;
#pragma unroll
  for (int j = 0; j < NP; ++j) Krow[j] = 0.0;
  if (wave == 0 && row) {
    if (!cheap) {
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (j < nt) Krow[j] = Q.Kb[lane * nt + j];
    }
    lo = Q.bnd[lane]; hi = Q.bnd[nt + lane]; dlo0 = Q.bnd[2 * nt + lane]; dhi0 = Q.bnd[3 * nt + lane];
    if constexpr (OUT) {
      if (outl) {  // absolute state bounds: one rounded subtraction per trajectory
        const int c = (int)Q.bnd[4 * nt + lane];
        if (c >= 0) {
          if (SCORED) {
            ylo_a = lo; yhi_a = hi; yc = c;
          }
          const double xr = Q.xref[c];
          lo = lo - xr;
          hi = hi - xr;
        }
      }
    }
    if (lane < p && Q.uinit) uprev = Q.uinit[lane];
  }
  const gmut_f64 ox = (gmut_f64)Q.out_x, ou = (gmut_f64)Q.out_u, oi = (gmut_f64)Q.out_info;
  const bool st_x = !SCORED || ox != nullptr, st_u = !SCORED || ou != nullptr;
  if (tid == 0 && st_x) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k < d) ox[k] = x[k];
  }
  const gconst_f64 uopt = SCORED ? (gconst_f64)Q.u_opt : nullptr;
  double uo[P];
#pragma unroll
  for (int j = 0; j < P; ++j) uo[j] = 0.0;
  long long it_sum = 0;
  int n_lim = 0, n_it = 0, n_yv = 0;
  if (SCORED && tid == 0) {
    sc[0] = 0.0; sc[1] = 0.0; sc[2] = sum_sq_ordered(x); sc[3] = 0.0; sc[4] = 0.0;
    if constexpr (OUT) sc[5] = 0.0;
    if (uopt) {
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (j < p) uo[j] = uopt[j];
    }
  }
  const int l0 = 64 * wave, cnt = min(64, m - l0);  // this wave's landmarks
  __syncthreads();  // W is in LDS
  for (int t = 0; t < steps; ++t) {
    mpc_w_pass<KTYPE, D>(x, wi, zs, kref, Q.sigma0sq, Wl, nt, l0, cnt, row, lane, wave, part);
    if (wave == 0) {  // uniform over the wave
      double gt = 0.0;  // g_i in an input lane, t_r in an output lane
      for (int w = 0; w < waves; ++w) gt = gt + part[64 * w + lane];
      double g = gt;
      if constexpr (OUT) g = var ? gt : 0.0;
      // bounds of this step: the first p rate rows are shifted by the control applied last, the output rows by t
      const double dlo = lane < p ? uprev + dlo0 : dlo0, dhi = lane < p ? uprev + dhi0 : dhi0;
      double blo = lo, bhi = hi;
      if constexpr (OUT) {
        blo = outl ? lo - gt : lo;
        bhi = outl ? hi - gt : hi;
      }
      // A NaN in the gradient (a NaN state), in a shifted rate bound (a NaN seed, inf - inf), in t or in a shifted output bound:
      // the NumPy statement of the iteration clips with np.minimum / np.maximum, which hand a NaN on -- every variable is NaN
      // after the first product, all `iters` iterations run, the residual is NaN and so is the control.  fmin / fmax would
      // drop the NaN and return a bound, so such a step is decided here, once, and the iteration stays as it is for every
      // other step.
      bool nanlane;
      if constexpr (OUT) nanlane = row && (gt != gt || dlo != dlo || dhi != dhi || blo != blo || bhi != bhi);
      else nanlane = var && (g != g || dlo != dlo || dhi != dhi);
      const bool nanstep = __ballot(nanlane) != 0;  // uniform over the wave
      // the rate slot of s: D among the input lanes only, an output lane (nv <= lane) keeps zeros
      auto rate_slot = [&](double s, double shifted) {
        const double ds = lane >= p ? s - shifted : s;
        if constexpr (OUT) return var ? ds : 0.0;
        else return ds;
      };
      // the prox of the box slot: the clip, for a soft output row c + theta (v - c)
      auto box_prox = [&](double v) {
        const double c1 = clipd(v, blo, bhi);
        if constexpr (OUT) return theta != 0.0 ? c1 + theta * (v - c1) : c1;
        else return c1;
      };
      double s1 = 0.0, z1, r = 0.0;
      int it = 0;
      if (cheap) {
        z1 = -g;
      } else if (nanstep) {
        z1 = __builtin_nan("");
        r = z1;
        it = Q.iters;
      } else {
        double a = 0.0;
        // (without output rows S0t = H^-1 is symmetric: entry `lane` of row j is entry j of row `lane`)
        const gconst_f64 hc = (gconst_f64)Q.S0t + (row ? lane : 0);
        for (int j = 0; j < nv; ++j) a = fma(hc[j * nt], lane_bcast(gt, j), a);  // lanes j < nv hold g_j
        s1 = row ? -a : 0.0;
        const int up = lane >= p ? lane - p : lane, dn = lane + p < 64 ? lane + p : lane;
        double sh = __shfl(s1, up, 64);
        double s2 = rate_slot(s1, sh);
        z1 = box_prox(s1);
        double z2 = clipd(s2, dlo, dhi), l1 = 0.0, l2 = 0.0;
        r = wave_max64_dpp(fmax(fabs(s1 - z1), fabs(s2 - z2)));
        while (it < Q.iters && !(r <= Q.tol && (it == 0 || Q.tol > 0.0))) {  // uniform: r is the same in every lane
          const double w2 = z2 - l2;
          const double w2n = __shfl(w2, dn, 64);
          const double dt = lane + p < nv ? w2 - w2n : w2;  // (an output lane: w2 = 0)
          const double rhs = Q.rho * ((z1 - l1) + dt) - g;
          double U = 0.0;
#pragma unroll
          for (int j = 0; j < NP; ++j) U = fma(Krow[j], lane_bcast(rhs, j), U);
          s1 = U;
          sh = __shfl(s1, up, 64);
          s2 = rate_slot(s1, sh);
          z1 = box_prox(s1 + l1);
          z2 = clipd(s2 + l2, dlo, dhi);
          l1 = l1 + (s1 - z1);
          l2 = l2 + (s2 - z2);
          r = wave_max64_dpp(fmax(fabs(s1 - z1), fabs(s2 - z2)));
          ++it;
        }
      }
      // the control: both clips, the rate clip last (lanes < p; the others carry values nobody reads)
      const double uc = clipd(clipd(z1, lo, hi), dlo, dhi);
      double un;
      if constexpr (OUT) un = nanstep ? __builtin_nan("") : uc;
      else un = (nanstep && (nanlane || !cheap)) ? __builtin_nan("") : uc;  // (iters = 0: entry by entry)
      if (SCORED) {  // a clip returns the bound itself: the comparisons are exact; the counts are the same in every lane
        const int its = __builtin_amdgcn_readfirstlane(it);
        it_sum += its;
        n_it += its > 0;
        // (under lane < p, so the output lanes never count)
        n_lim += __builtin_popcountll(__ballot(lane < p && (un == lo || un == hi || un == dlo || un == dhi)));
      }
      uprev = un;
      double u[P], xn[D];
#pragma unroll
      for (int j = 0; j < P; ++j) u[j] = j < p ? lane_bcast(un, j) : 0.0;
      poly_plant_step<D, P>(tb, x, u, xn);
      double yv = 0.0;  // OUT, SCORED: the largest excursion of x_{t+1} past the absolute bounds of the output rows, NaN when one is
      if constexpr (OUT && SCORED) {
#pragma clang fp contract(off)
        double xc = xn[0];  // xn is the same in every lane: the plant step works on broadcast values
#pragma unroll
        for (int k = 1; k < D; ++k) xc = yc == k ? xn[k] : xc;
        const double below = ylo_a - xc, above = xc - yhi_a;  // one rounded subtraction each
        const bool nanrow = yc >= 0 && (below != below || above != above);
        const double mine = (yc >= 0 && !nanrow) ? fmax(fmax(below, above), 0.0) : 0.0;
        const bool nany = __ballot(nanrow) != 0;  // uniform over the wave
        yv = wave_max64_dpp(mine);
        yv = nany ? __builtin_nan("") : yv;
        n_yv += yv > 0.0;
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) xb[k] = xn[k];
        // (spelled out, not store_step of nk_loop_lanes.h: through the helper the 32-lane kernels ran 2-5 % slower per step)
        if (st_u) {
#pragma unroll
          for (int j = 0; j < P; ++j)
            if (j < p) ou[(int64_t)t * Q.ldu + j] = u[j];
        }
        if (st_x) {
#pragma unroll
          for (int k = 0; k < D; ++k)
            if (k < d) ox[(int64_t)(t + 1) * Q.ldx + k] = xn[k];
        }
        if (oi) {
          oi[2 * (int64_t)t] = (double)it;
          oi[2 * (int64_t)t + 1] = r;
        }
        if (SCORED) {  // the residual and the excursion under the NaN rule of u_absmax
          double J = sc[2], umax = sc[3];
          score_cost_step(xn, u, J, umax);
          sc[2] = J;
          sc[3] = umax;
          sc[4] = sticky_max(r, sc[4]);
          if constexpr (OUT) sc[5] = sticky_max(yv, sc[5]);
          if (uopt) {
            double sse = sc[0], sso = sc[1];
            score_uopt_step(u, uo, uopt, (int64_t)(t + 1 < steps ? t + 1 : t), p, sse, sso);
            sc[0] = sse; sc[1] = sso;
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xb[k];
  }
  if (SCORED && tid == 0 && Q.score) {
    double* s = Q.score;
    s[0] = sc[0]; s[1] = sc[1]; s[2] = sc[2]; s[3] = sc[3];
    s[4] = (double)it_sum; s[5] = sc[4]; s[6] = (double)n_lim; s[7] = (double)n_it;
    if constexpr (OUT) {
      s[8] = sc[5]; s[9] = (double)n_yv;
    }
  }
}

// the single calls: the record of block b from the record of batch member 0
template <int KTYPE, int D, int NVP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES) mpc_loop_kernel(MpcLoopUnit base, LoopStrides strides, PolyProgram pl) {
  extern __shared__ double mpc_lds[];
  mpc_loop_body<KTYPE, D, NVP, false, false>(unit_of_block(base, strides, blockIdx.x), pl, strides.steps, mpc_lds);
}
template <int KTYPE, int D, int NTP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES) mpc_out_loop_kernel(MpcLoopUnit base, LoopStrides strides, PolyProgram pl) {
  extern __shared__ double mpc_out_lds[];
  mpc_loop_body<KTYPE, D, NTP, true, false>(unit_of_block(base, strides, blockIdx.x), pl, strides.steps, mpc_out_lds);
}

// the multi-model forms: unit blockIdx.x of `table` (all units of a launch share KTYPE, NP and the block size)
template <int KTYPE, int D, int NVP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES)
    mpc_loop_multi_kernel(const MpcLoopUnit* __restrict__ table, PolyProgram pl, int steps) {
  extern __shared__ double mpc_lds[];
  const MpcLoopUnit U = table[blockIdx.x];
  mpc_loop_body<KTYPE, D, NVP, false, true>(U, pl, steps, mpc_lds);
}
template <int KTYPE, int D, int NTP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES)
    mpc_out_loop_multi_kernel(const MpcLoopUnit* __restrict__ table, PolyProgram pl, int steps) {
  extern __shared__ double mpc_out_lds[];
  const MpcLoopUnit U = table[blockIdx.x];
  mpc_loop_body<KTYPE, D, NTP, true, true>(U, pl, steps, mpc_out_lds);
}

// The LDS a loop of (m, nv) needs against what the device gives one workgroup: NK_ERR_BAD_ARG when it does not fit.  The entry
// point calls this before anything is queued.
int mpc_loop_check_lds(nk_ctx* ctx, int m, int nv, int* lds_max_out) {
  const size_t lds = sizeof(double) * (size_t)mpc_lds_doubles(m, nv);
  int lds_max = 0;
  NK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  NK_REQUIRE(lds <= (size_t)lds_max, "mpc_loop: %zu bytes of LDS for m = %d and nv = %d, the device gives a workgroup %d", lds,
             m, nv, lds_max);
  if (lds_max_out) *lds_max_out = lds_max;
  return NK_OK;
}

// one launch of KERN with lds_doubles of dynamic LDS; the kernel is registered for it once
template <auto KERN, class... Args>
static int mpc_launch(nk_ctx* ctx, int lds_max, int grid, int waves, long lds_doubles, const Args&... args) {
  static const hipError_t e = dynamic_lds_register(std::min(lds_max, MPC_LDS_DOUBLES * 8), KERN);
  NK_TRY(dynamic_lds_status(e));
  hipLaunchKernelGGL(KERN, dim3(grid), dim3(64 * waves), sizeof(double) * (size_t)lds_doubles, ctx->stream, args...);
  return NK_OK;
}

// The single calls: Q is the record of batch member 0, its sizes checked by the caller.
template <bool OUT>
static int launch_mpc_single(nk_ctx* ctx, const char* who, int ktype, const nk_poly_plant& plant, const MpcLoopUnit& Q,
                             const LoopStrides& strides, int batch) {
  const int m = Q.m, nt = Q.nv + Q.ny, waves = (m + 63) / 64;
  int lds_max = 0;
  NK_TRY(mpc_loop_check_lds(ctx, m, nt, &lds_max));
  const PolyProgram prog = poly_compile(plant);
  int rc_lds = NK_OK;
  NK_TRY(mpc_loop_dispatch(who, ktype, plant.d, nt, [&](auto kt, auto dd, auto np) {
    constexpr int KT = decltype(kt)::value, DD = decltype(dd)::value, NP = decltype(np)::value;
    rc_lds = mpc_launch<(OUT ? mpc_out_loop_kernel<KT, DD, NP> : mpc_loop_kernel<KT, DD, NP>)>(
        ctx, lds_max, batch, waves, mpc_lds_doubles(m, nt), Q, strides, prog);
  }));
  NK_TRY(rc_lds);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// The multi-model forms: the records (sizes checked by the caller) run through launch_loop_classes (nk_loop_lanes.h) in classes
// of (kernel family, padded lanes, waves), a launch's dynamic LDS the largest need among its units.
template <bool OUT>
static int launch_mpc_multi(nk_ctx* ctx, const char* who, const nk_poly_plant& plant, int steps, MpcLoopUnit* units,
                            const int* ktypes, int n_units, int lds_max) {
  const PolyProgram prog = poly_compile(plant);
  auto key_of = [&](int u) {
    const int nt = units[u].nv + units[u].ny;
    return LoopClass{ktypes[u], nt <= 16 ? 16 : nt <= 32 ? 32 : 64, (units[u].m + 63) / 64};
  };
  auto lds_of = [&](int u) { return mpc_lds_doubles(units[u].m, units[u].nv + units[u].ny); };
  NK_TRY(launch_loop_classes(ctx, units, n_units, key_of, lds_of, [&](const MpcLoopUnit* first, int count, const LoopClass& k, long lds) {
    int rc_lds = NK_OK;
    NK_TRY(mpc_loop_dispatch(who, k.ktype, plant.d, k.shape, [&](auto kt, auto dd, auto np) {
      constexpr int KT = decltype(kt)::value, DD = decltype(dd)::value, NP = decltype(np)::value;
      rc_lds = mpc_launch<(OUT ? mpc_out_loop_multi_kernel<KT, DD, NP> : mpc_loop_multi_kernel<KT, DD, NP>)>(
          ctx, lds_max, count, k.waves, lds, first, prog, steps);
    }));
    return rc_lds;
  }));
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// the record of batch member 0 of a single call (ny = 0, theta = 0: no output rows)
static MpcLoopUnit mpc_record(const nk_model* mdl, int nv, int ny, int iters, double rho, double tol, double theta, const double* w,
                              const double* Kb, const double* S0t, const double* bnd, const double* x0, const double* xref,
                              const double* uinit, double* out_x, int64_t ldx, double* out_u, int64_t ldu, double* out_info) {
  MpcLoopUnit Q;
  Q.Z = mdl->Z; Q.winv = mdl->winv; Q.w = w; Q.Kb = Kb; Q.S0t = S0t; Q.bnd = bnd;
  Q.x0 = x0; Q.xref = xref; Q.uinit = uinit;
  Q.out_x = out_x; Q.ldx = ldx; Q.out_u = out_u; Q.ldu = ldu; Q.out_info = out_info;
  Q.u_opt = nullptr; Q.score = nullptr;
  Q.sigma0sq = mdl->sigma0 * mdl->sigma0; Q.rho = rho; Q.tol = tol; Q.theta = theta;
  Q.m = mdl->m; Q.nv = nv; Q.ny = ny; Q.iters = iters;
  return Q;
}

// all pointers device memory; w: m x nv dense (cheap: nv = p); bnd: 4 x nv
int launch_mpc_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, int nv, int iters, double rho, double tol,
                    const double* w, const double* M, const double* Hinv, const double* bnd, const double* x0, int64_t x0_stride,
                    const double* xref, int64_t xref_stride, const double* uinit, int64_t uinit_stride, int steps, int batch,
                    double* out_x, int64_t ldx, double* out_u, int64_t ldu, double* out_info) {
  const int m = mdl->m;
  NK_REQUIRE(plant.d == mdl->d && plant.p == mdl->p && nv >= 1 && nv <= NK_MPC_MAX_NV && m >= 1 && m <= mpc_loop_max_m(nv) &&
                 steps >= 1 && batch >= 1 && iters >= 0, "mpc_loop: bad sizes");
  const MpcLoopUnit Q = mpc_record(mdl, nv, 0, iters, rho, tol, 0.0, w, M, Hinv, bnd, x0, xref, uinit, out_x, ldx, out_u, ldu, out_info);
  return launch_mpc_single<false>(ctx, "mpc_loop", mdl->ktype, plant, Q, LoopStrides{x0_stride, xref_stride, uinit_stride, steps}, batch);
}

// all pointers device memory; w: m x nt dense; Kb: nt x nt; S0t: nv x nt; bnd: 5 x nt
int launch_mpc_out_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, int nv, int ny, int iters, double rho,
                        double tol, double theta, const double* w, const double* Kb, const double* S0t, const double* bnd,
                        const double* x0, int64_t x0_stride, const double* xref, int64_t xref_stride, const double* uinit,
                        int64_t uinit_stride, int steps, int batch, double* out_x, int64_t ldx, double* out_u, int64_t ldu,
                        double* out_info) {
  const int m = mdl->m, nt = nv + ny;
  NK_REQUIRE(plant.d == mdl->d && plant.p == mdl->p && nv >= 1 && ny >= 1 && nt <= NK_MPC_MAX_NV && m >= 1 &&
                 m <= mpc_loop_max_m(nt) && steps >= 1 && batch >= 1 && iters >= 1, "mpc_out_loop: bad sizes");
  const MpcLoopUnit Q = mpc_record(mdl, nv, ny, iters, rho, tol, theta, w, Kb, S0t, bnd, x0, xref, uinit, out_x, ldx, out_u, ldu, out_info);
  return launch_mpc_single<true>(ctx, "mpc_out_loop", mdl->ktype, plant, Q, LoopStrides{x0_stride, xref_stride, uinit_stride, steps}, batch);
}

int launch_mpc_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, MpcLoopUnit* units, const int* ktypes,
                          int n_units) {
  NK_REQUIRE(steps >= 1 && n_units >= 1, "mpc_loop_multi: bad sizes");
  int lds_max = 0;
  NK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  for (int u = 0; u < n_units; ++u) {
    const int m = units[u].m, nv = units[u].nv;
    NK_REQUIRE(units[u].ny == 0 && nv >= 1 && nv <= NK_MPC_MAX_NV && m >= 1 && m <= mpc_loop_max_m(nv) && units[u].iters >= 0 &&
                   sizeof(double) * (size_t)mpc_lds_doubles(m, nv) <= (size_t)lds_max, "mpc_loop_multi: unit %d: bad sizes", u);
  }
  return launch_mpc_multi<false>(ctx, "mpc_loop_multi", plant, steps, units, ktypes, n_units, lds_max);
}

int launch_mpc_out_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, MpcLoopUnit* units, const int* ktypes,
                              int n_units) {
  NK_REQUIRE(steps >= 1 && n_units >= 1, "mpc_out_loop_multi: bad sizes");
  int lds_max = 0;
  NK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  for (int u = 0; u < n_units; ++u) {
    const int m = units[u].m, nv = units[u].nv, ny = units[u].ny, nt = nv + ny;
    NK_REQUIRE(nv >= 1 && ny >= 1 && nt <= NK_MPC_MAX_NV && m >= 1 && m <= mpc_loop_max_m(nt) && units[u].iters >= 1 &&
                   sizeof(double) * (size_t)mpc_lds_doubles(m, nt) <= (size_t)lds_max, "mpc_out_loop_multi: unit %d: bad sizes", u);
  }
  return launch_mpc_multi<true>(ctx, "mpc_out_loop_multi", plant, steps, units, ktypes, n_units, lds_max);
}

}  // namespace nk
