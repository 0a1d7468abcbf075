// The constrained Koopman MPC loop with limits on predicted states (nk_mpc_out_loop, include/nyskoop.h) as ONE launch: the
// loop of nk_mpc_loop.hip on nt = nv + ny lanes of the first wave, with the folded iteration of the interface.  One workgroup
// per trajectory, ceil(m / 64) <= 8 waves, one landmark per lane, nothing from the host per step.
//   fold:      W = S^-1 [F; T]' (m x nt, row l at W + l nt; spline models: [F; T]') is copied to LDS once.  The per-wave sums
//              of mpc_loop_body give lane i < nv its g_i and lane nv + r its t_r in the same pass: ONE barrier, and the first
//              wave adds the words in wave order.
//   QP:        in the first wave only.  Lane i < nt owns entry i of s_K = (s_1, s_3): its row of Kb in registers (NTP
//              doubles), q broadcast entry by entry with v_readlane into NTP FMAs in index order.  An input lane (i < nv)
//              carries its box row and its rate row (D and D' are shifts by p lanes among the input lanes); an output lane
//              carries one row: its shifted bounds (ylo_r - x_ref[ycomp_r]) - t_r where an input lane holds lo / hi, the
//              soft prox c + theta (v - c), and zeros in the rate slot, so it takes no part in the shifts.  S0 = [H^-1; G H^-1]
//              is needed once per step: it is stored transposed (nv x nt), lane i reads word j nt + i of global memory.
//   plant:     as in mpc_loop_body; two LDS-only barriers per step.
// Every summation order is fixed by (m, nv, ny, p) alone, so a trajectory has the same bits alone or in any batch.
// The multi-model form (nk_mpc_out_loop_multi) runs the SAME loop body on one record per unit (MpcOutLoopUnit, nk_common.h),
// selected from a device table by the block index, one launch per class of (kernel family, D, NTP, waves), and scores every
// unit in its first wave; a unit has the bits of the single call whatever else the launch holds.
#include "nk_common.h"
#include "nk_mpc.h"
#include "nk_mpc_lanes.h"
#include "nk_poly_lanes.h"

#include <algorithm>
#include <vector>

namespace nk {

struct MpcOutParams {
  const double* Z;      // m x d landmarks
  const double* winv;   // d
  const double* w;      // m x nt folded map of [F; T], dense
  const double* Kb;     // nt x nt
  const double* S0t;    // nv x nt: S0 transposed
  const double* bnd;    // 5 x nt: lo, hi, dlo, dhi (input lanes; output lanes: ylo, yhi, -inf, inf), ycomp as a double
  const double* x0; int64_t x0_stride;        // batch x d
  const double* xref; int64_t xref_stride;    // batch x d
  const double* uinit; int64_t uinit_stride;  // batch x p, or nullptr (zeros)
  double* out_x; int64_t ldx;                 // rows b * (steps + 1) + t, d columns
  double* out_u; int64_t ldu;                 // rows b * steps + t, p columns
  double* out_info;                           // rows b * steps + t, 2 columns, or nullptr
  double sigma0sq, rho, tol, theta;
  int m, nv, ny, iters, steps;
};

// The loop of one workgroup on the record of one trajectory.  SCORED = false: nk_mpc_out_loop (out_x and out_u are stored,
// out_info when it is given, nothing is scored).  SCORED = true: the multi-model form -- every output may be null, and lane 0
// of the first wave accumulates the ten scores of nk_mpc_out_loop_multi in step order.  The first eight are those of
// mpc_loop_body, computed as there; the floating-point ones live in the spare words of the broadcast state (mpc_lds_doubles
// reserves 16 words: x_{t+1} takes 4, the scores 6), the counters are wave-uniform integers.  y_viol_max / n_y_viol: an output lane keeps its ABSOLUTE bounds and its component and
// forms max(ylo - x_{t+1}[c], x_{t+1}[c] - yhi, 0) from the new state, which every lane of the first wave holds (the plant
// step works on broadcast values only); one butterfly gives the maximum of the step, a ballot its NaN case.
template <int KTYPE, int D, int NTP, bool SCORED>
__device__ __forceinline__ void mpc_out_loop_body(const MpcOutLoopUnit& Q, const PolyProgram& pl, int steps, double* mpc_out_lds) {
  constexpr int P = NK_POLY_MAX_P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const int m = Q.m, nv = Q.nv, nt = Q.nv + Q.ny, d = pl.d, p = pl.p;
  double* Wl = mpc_out_lds;                   // m x nt
  double* part = Wl + (size_t)m * nt;         // waves x 64
  double* xb = part + 64 * waves;             // D words of x_{t+1}
  double* sc = xb + 4;                        // SCORED: sse_u, ss_opt, J, u_absmax, r_max, y_viol_max (lane 0 of the first wave only)
  for (int i = tid; i < m * nt; i += nthreads) Wl[i] = Q.w[i];
  const PolyLanes tb(pl, lane);
  const double* x0 = Q.x0;
  const double* xrp = Q.xref;
  double wi[D], zs[D], x[D], kref;
  const bool have = tid < m;  // a lane without a landmark: landmark 0, and its dk is never read
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
  // the first wave: lane i < nv owns decision variable i, lane nv + r output row r
  const bool row = lane < nt, var = lane < nv, outl = row && !var;
  const double inf = __builtin_huge_val();
  const double theta = outl ? Q.theta : 0.0;
  double Krow[NTP], lo = -inf, hi = inf, dlo0 = -inf, dhi0 = inf, uprev = 0.0;
  double ylo_a = -inf, yhi_a = inf;  // SCORED: the absolute bounds of an output lane with a component (yc >= 0)
  int yc = -1;
#pragma unroll
  for (int j = 0; j < NTP; ++j) Krow[j] = 0.0;
  if (wave == 0 && row) {
#pragma unroll
    for (int j = 0; j < NTP; ++j)
      if (j < nt) Krow[j] = Q.Kb[lane * nt + j];
    lo = Q.bnd[lane]; hi = Q.bnd[nt + lane]; dlo0 = Q.bnd[2 * nt + lane]; dhi0 = Q.bnd[3 * nt + lane];
    if (outl) {  // absolute state bounds: one rounded subtraction per trajectory
      const int c = (int)Q.bnd[4 * nt + lane];
      if (c >= 0) {
        if (SCORED) {
          ylo_a = lo; yhi_a = hi; yc = c;
        }
        const double xr = xrp[c];
        lo = lo - xr;
        hi = hi - xr;
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
#pragma clang fp contract(off)
    double J = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double sq = x[k] * x[k];
      J = k == 0 ? sq : J + sq;
    }
    sc[0] = 0.0; sc[1] = 0.0; sc[2] = J; sc[3] = 0.0; sc[4] = 0.0; sc[5] = 0.0;
    if (uopt) {
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (j < p) uo[j] = uopt[j];
    }
  }
  const int l0 = 64 * wave, cnt = min(64, m - l0);  // this wave's landmarks
  __syncthreads();  // W is in LDS
  for (int t = 0; t < steps; ++t) {
    double dk;
    {
#pragma clang fp contract(off)
      double xs[D];
#pragma unroll
      for (int k = 0; k < D; ++k) xs[k] = x[k] * wi[k];
      dk = plant_kval<KTYPE, D>(xs, zs, Q.sigma0sq) - kref;
    }
    double acc = 0.0;
    {
      const double* wr = Wl + (size_t)l0 * nt + (row ? lane : 0);  // lanes without a row read column 0 and drop the sum
      for (int l = 0; l < cnt; ++l) acc = fma(wr[(size_t)l * nt], lane_bcast(dk, l), acc);
    }
    part[64 * wave + lane] = row ? acc : 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave == 0) {  // uniform over the wave
      double gt = 0.0;  // g_i in an input lane, t_r in an output lane
      for (int w = 0; w < waves; ++w) gt = gt + part[64 * w + lane];
      const double g = var ? gt : 0.0;
      // bounds of this step: the first p rate rows are shifted by the control applied last, the output rows by t
      const double dlo = lane < p ? uprev + dlo0 : dlo0, dhi = lane < p ? uprev + dhi0 : dhi0;
      const double blo = outl ? lo - gt : lo, bhi = outl ? hi - gt : hi;
      // the NaN rule of mpc_loop_body, extended to t and to the shifted output bounds
      const bool nanlane = row && (gt != gt || dlo != dlo || dhi != dhi || blo != blo || bhi != bhi);
      const bool nanstep = __ballot(nanlane) != 0;  // uniform over the wave
      double s1 = 0.0, z1, r = 0.0;
      int it = 0;
      if (nanstep) {
        z1 = __builtin_nan("");
        r = z1;
        it = Q.iters;
      } else {
        double a = 0.0;
        const gconst_f64 sc = (gconst_f64)Q.S0t + (row ? lane : 0);
        for (int j = 0; j < nv; ++j) a = fma(sc[j * nt], lane_bcast(gt, j), a);  // lanes j < nv hold g_j
        s1 = row ? -a : 0.0;
        // D among the input lanes only: an output lane (nv <= lane) keeps zeros in its rate slot
        const int up = lane >= p ? lane - p : lane, dn = lane + p < 64 ? lane + p : lane;
        double sh = __shfl(s1, up, 64);
        double s2 = var ? (lane >= p ? s1 - sh : s1) : 0.0;
        double c1 = clipd(s1, blo, bhi);
        z1 = theta != 0.0 ? c1 + theta * (s1 - c1) : c1;
        double z2 = clipd(s2, dlo, dhi), l1 = 0.0, l2 = 0.0;
        r = wave_max64_dpp(fmax(fabs(s1 - z1), fabs(s2 - z2)));
        while (it < Q.iters && !(r <= Q.tol && (it == 0 || Q.tol > 0.0))) {  // uniform: r is the same in every lane
          const double w2 = z2 - l2;
          const double w2n = __shfl(w2, dn, 64);
          const double dt = lane + p < nv ? w2 - w2n : w2;  // (an output lane: w2 = 0)
          const double q = Q.rho * ((z1 - l1) + dt) - g;
          double U = 0.0;
#pragma unroll
          for (int j = 0; j < NTP; ++j) U = fma(Krow[j], lane_bcast(q, j), U);
          s1 = U;
          sh = __shfl(s1, up, 64);
          s2 = var ? (lane >= p ? s1 - sh : s1) : 0.0;
          const double v1 = s1 + l1;
          c1 = clipd(v1, blo, bhi);
          z1 = theta != 0.0 ? c1 + theta * (v1 - c1) : c1;
          z2 = clipd(s2 + l2, dlo, dhi);
          l1 = l1 + (s1 - z1);
          l2 = l2 + (s2 - z2);
          r = wave_max64_dpp(fmax(fabs(s1 - z1), fabs(s2 - z2)));
          ++it;
        }
      }
      // the control: both clips, the rate clip last (lanes < p; the others carry values nobody reads)
      const double uc = clipd(clipd(z1, lo, hi), dlo, dhi);
      const double un = nanstep ? __builtin_nan("") : uc;
      if (SCORED) {  // as in mpc_loop_body; under lane < p, so the output lanes never count
        const int its = __builtin_amdgcn_readfirstlane(it);
        it_sum += its;
        n_it += its > 0;
        n_lim += __builtin_popcountll(__ballot(lane < p && (un == lo || un == hi || un == dlo || un == dhi)));
      }
      uprev = un;
      double u[P], xn[D];
#pragma unroll
      for (int j = 0; j < P; ++j) u[j] = j < p ? lane_bcast(un, j) : 0.0;
      poly_plant_step<D, P>(tb, x, u, xn);
      double yv = 0.0;  // SCORED: the largest excursion of x_{t+1} past the absolute bounds of the output rows, NaN when one is
      if (SCORED) {
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
        if (SCORED) {  // the sums of mpc_loop_body, and the two maxima under the NaN rule of u_absmax
#pragma clang fp contract(off)
          double sx = 0.0, su = 0.0, umax = sc[3];
#pragma unroll
          for (int k = 0; k < D; ++k) {
            const double sq = xn[k] * xn[k];
            sx = k == 0 ? sq : sx + sq;
          }
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const double sq = u[j] * u[j];
            su = j == 0 ? sq : su + sq;
            const double au = fabs(u[j]);
            umax = (au > umax || au != au) ? au : umax;  // a NaN enters once and stays: no later comparison is true
          }
          sc[2] = (sc[2] + sx) + su;
          sc[3] = umax;
          const double rmax = sc[4];
          sc[4] = (r > rmax || r != r) ? r : rmax;
          const double ymax = sc[5];
          sc[5] = (yv > ymax || yv != yv) ? yv : ymax;
          if (uopt) {
            const int64_t tn = t + 1 < steps ? t + 1 : t;
            double sse = sc[0], sso = sc[1];
#pragma unroll
            for (int j = 0; j < P; ++j) {
              const double df = u[j] - uo[j];
              const double dsq = df * df, osq = uo[j] * uo[j];
              sse = sse + dsq;
              sso = sso + osq;
              if (j < p) uo[j] = uopt[tn * p + j];  // next step's values, loaded a step ahead (not on the chain)
            }
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
    s[8] = sc[5]; s[9] = (double)n_yv;
  }
}

template <int KTYPE, int D, int NTP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES) mpc_out_loop_kernel(MpcOutParams Q, PolyProgram pl) {
  extern __shared__ double mpc_out_lds[];
  const int64_t b = blockIdx.x;
  MpcOutLoopUnit U;
  U.Z = Q.Z; U.winv = Q.winv; U.w = Q.w; U.Kb = Q.Kb; U.S0t = Q.S0t; U.bnd = Q.bnd;
  U.x0 = Q.x0 + b * Q.x0_stride;
  U.xref = Q.xref + b * Q.xref_stride;
  U.uinit = Q.uinit ? Q.uinit + b * Q.uinit_stride : nullptr;
  U.out_x = Q.out_x + b * (Q.steps + 1) * Q.ldx; U.ldx = Q.ldx;
  U.out_u = Q.out_u + b * Q.steps * Q.ldu; U.ldu = Q.ldu;
  U.out_info = Q.out_info ? Q.out_info + b * Q.steps * 2 : nullptr;
  U.u_opt = nullptr; U.score = nullptr;
  U.sigma0sq = Q.sigma0sq; U.rho = Q.rho; U.tol = Q.tol; U.theta = Q.theta;
  U.m = Q.m; U.nv = Q.nv; U.ny = Q.ny; U.iters = Q.iters;
  mpc_out_loop_body<KTYPE, D, NTP, false>(U, pl, Q.steps, mpc_out_lds);
}

// the multi-model form: unit blockIdx.x of `table` (all units of a launch share KTYPE, NTP and the block size)
template <int KTYPE, int D, int NTP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES)
    mpc_out_loop_multi_kernel(const MpcOutLoopUnit* __restrict__ table, PolyProgram pl, int steps) {
  extern __shared__ double mpc_out_lds[];
  const MpcOutLoopUnit U = table[blockIdx.x];
  mpc_out_loop_body<KTYPE, D, NTP, true>(U, pl, steps, mpc_out_lds);
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
  const int waves = (m + 63) / 64;
  const size_t lds = sizeof(double) * (size_t)mpc_lds_doubles(m, nt);
  int lds_max = 0;
  NK_TRY(mpc_loop_check_lds(ctx, m, nt, &lds_max));
  MpcOutParams Q;
  Q.Z = mdl->Z; Q.winv = mdl->winv; Q.w = w; Q.Kb = Kb; Q.S0t = S0t; Q.bnd = bnd;
  Q.x0 = x0; Q.x0_stride = x0_stride; Q.xref = xref; Q.xref_stride = xref_stride; Q.uinit = uinit; Q.uinit_stride = uinit_stride;
  Q.out_x = out_x; Q.ldx = ldx; Q.out_u = out_u; Q.ldu = ldu; Q.out_info = out_info;
  Q.sigma0sq = mdl->sigma0 * mdl->sigma0; Q.rho = rho; Q.tol = tol; Q.theta = theta;
  Q.m = m; Q.nv = nv; Q.ny = ny; Q.iters = iters; Q.steps = steps;
  const PolyProgram prog = poly_compile(plant);
  int rc_lds = NK_OK;
  NK_TRY(mpc_loop_dispatch("mpc_out_loop", mdl->ktype, plant.d, nt, [&](auto kt, auto dd, auto np) {
    auto* kern = mpc_out_loop_kernel<decltype(kt)::value, decltype(dd)::value, decltype(np)::value>;
    static const hipError_t e = dynamic_lds_register(std::min(lds_max, MPC_LDS_DOUBLES * 8), kern);  // once per instantiation
    rc_lds = dynamic_lds_status(e);
    if (rc_lds != NK_OK) return;
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64 * waves), lds, ctx->stream, Q, prog);
  }));
  NK_TRY(rc_lds);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// The multi-model form, as launch_mpc_loop_multi: the records are sorted (stable) into classes of (kernel family, padded
// lanes, waves), staged with ONE copy and run with one launch per class.  `units` is reordered in place and must stay alive
// until the stream has been synchronised.
int launch_mpc_out_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, MpcOutLoopUnit* units, const int* ktypes,
                              int n_units) {
  NK_REQUIRE(steps >= 1 && n_units >= 1, "mpc_out_loop_multi: bad sizes");
  int lds_max = 0;
  NK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  struct Key { int ktype, ntp, waves, idx; };
  std::vector<Key> keys((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const int m = units[u].m, nv = units[u].nv, ny = units[u].ny, nt = nv + ny;
    NK_REQUIRE(nv >= 1 && ny >= 1 && nt <= NK_MPC_MAX_NV && m >= 1 && m <= mpc_loop_max_m(nt) && units[u].iters >= 1 &&
                   sizeof(double) * (size_t)mpc_lds_doubles(m, nt) <= (size_t)lds_max, "mpc_out_loop_multi: unit %d: bad sizes", u);
    keys[u] = Key{ktypes[u], nt <= 16 ? 16 : nt <= 32 ? 32 : 64, (m + 63) / 64, u};
  }
  auto less = [](const Key& a, const Key& b) {
    if (a.ktype != b.ktype) return a.ktype < b.ktype;
    if (a.ntp != b.ntp) return a.ntp < b.ntp;
    return a.waves < b.waves;
  };
  std::stable_sort(keys.begin(), keys.end(), less);
  {
    std::vector<MpcOutLoopUnit> sorted((size_t)n_units);
    for (int u = 0; u < n_units; ++u) sorted[u] = units[keys[u].idx];
    std::copy(sorted.begin(), sorted.end(), units);
  }
  const PolyProgram prog = poly_compile(plant);
  MpcOutLoopUnit* table = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n_units, &table));
  NK_HIP(hipMemcpyAsync(table, units, sizeof(MpcOutLoopUnit) * (size_t)n_units, hipMemcpyHostToDevice, ctx->stream));
  auto lds_of = [](const MpcOutLoopUnit& r) { return mpc_lds_doubles(r.m, r.nv + r.ny); };
  for (int b = 0; b < n_units;) {
    int e = b + 1;
    long lds_doubles = lds_of(units[b]);
    for (; e < n_units && !less(keys[b], keys[e]); ++e) lds_doubles = std::max(lds_doubles, lds_of(units[e]));
    const Key& k = keys[b];
    const MpcOutLoopUnit* first = table + b;
    int rc_lds = NK_OK;
    NK_TRY(mpc_loop_dispatch("mpc_out_loop_multi", k.ktype, plant.d, k.ntp, [&](auto kt, auto dd, auto np) {
      auto* kern = mpc_out_loop_multi_kernel<decltype(kt)::value, decltype(dd)::value, decltype(np)::value>;
      static const hipError_t er = dynamic_lds_register(std::min(lds_max, MPC_LDS_DOUBLES * 8), kern);  // once per instantiation
      rc_lds = dynamic_lds_status(er);
      if (rc_lds != NK_OK) return;
      hipLaunchKernelGGL(kern, dim3(e - b), dim3(64 * k.waves), sizeof(double) * (size_t)lds_doubles, ctx->stream, first, prog,
                         steps);
    }));
    NK_TRY(rc_lds);
    b = e;
  }
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
