// Constrained Koopman MPC around a polynomial plant as ONE launch (nk_mpc_loop, include/nyskoop.h): every step lifts the
// measured state, forms the gradient g = F (phi(x_t) - phi(x_ref)) of the condensed QP, runs the fixed-step ADMM iteration of
// the interface under box and rate limits, applies the first move and advances the plant by one Runge-Kutta step
// (nk_poly_plant.h).  One workgroup per trajectory, ceil(m / 64) <= 8 waves, one landmark per lane, nothing from the host
// per step.
//   gradient:  F is folded into the lift once per call, W = S^-1 F' (m x nv, row l at W + l nv; spline models: F'), and
//              copied to LDS.  A lane evaluates dk_l = k(z_l, x_t) - k(z_l, x_ref) for its landmark (the arithmetic of
//              plant_kval); wave w sums W[l][i] dk_l over ITS OWN 64 landmarks in index order, lane i owning variable i and
//              dk_l arriving by v_readlane (no LDS round trip, no barrier); one LDS word per wave and variable, ONE barrier,
//              and the first wave adds the words in wave order.
//   QP:        in the first wave only, then a broadcast -- with five to eight waves on four SIMDs a QP replicated in every
//              wave would share its issue slots with a second copy of itself, and the iteration is the long part of a step.
//              Lane i owns decision variable i: its row of M in registers (NVP doubles), the right-hand side broadcast entry
//              by entry with v_readlane (two per entry) into NVP FMAs in index order; D and D' are shifts by p lanes
//              (ds_bpermute, no memory); max |s - z| by a DPP / permlane butterfly; the stop is uniform over the wave.  H^-1
//              is needed once per step (the start U_unc = -H^-1 g): its rows are read from global memory (32 KB at most,
//              the same for every workgroup, cache resident) -- LDS is W's.
//   plant:     the same wave advances the plant (PolyLanes: all terms at once in the lanes) and writes x_{t+1} to LDS; a
//              second barrier, and every wave reads it.  Two LDS-only barriers per step.
// iters = 0 (the saturated LQR) runs the same kernel with W = S^-1 K' (nv := p): v = -g and the two clips.
// Every summation order is fixed by (m, nv, p) alone, so a trajectory has the same bits alone or in any batch.
// The multi-model form (nk_mpc_loop_multi) runs the SAME loop body on one record per unit (MpcLoopUnit, nk_common.h), selected
// from a device table by the block index, one launch per class of (kernel family, D, NVP, waves), and scores every unit in
// lane 0 of its first wave; a unit has the bits of the single call whatever else the launch holds.
#include "nk_common.h"
#include "nk_mpc.h"
#include "nk_mpc_lanes.h"
#include "nk_poly_lanes.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace nk {

struct MpcLoopParams {
  const double* Z;      // m x d landmarks
  const double* winv;   // d
  const double* w;      // m x nv folded gradient map (iters = 0: m x p folded gain), dense
  const double* M;      // nv x nv (unused for iters = 0)
  const double* Hinv;   // nv x nv
  const double* bnd;    // 4 x nv: lo, hi, dlo, dhi (infinite where the caller gave none)
  const double* x0; int64_t x0_stride;        // batch x d
  const double* xref; int64_t xref_stride;    // batch x d
  const double* uinit; int64_t uinit_stride;  // batch x p, or nullptr (zeros)
  double* out_x; int64_t ldx;                 // rows b * (steps + 1) + t, d columns
  double* out_u; int64_t ldu;                 // rows b * steps + t, p columns
  double* out_info;                           // rows b * steps + t, 2 columns, or nullptr
  double sigma0sq, rho, tol;
  int m, nv, iters, steps;
};

// The loop of one workgroup on the record of one trajectory.  SCORED = false: nk_mpc_loop (out_x and out_u are stored, out_info
// when it is given, nothing is scored).  SCORED = true: the multi-model form -- every output may be null, and lane 0 of the
// first wave accumulates the eight scores of nk_mpc_loop_multi in step order: the five floating-point ones in the spare words
// of the broadcast state (mpc_lds_doubles reserves 16 words, x_{t+1} takes D <= 4), the three counters as wave-uniform integers.
template <int KTYPE, int D, int NVP, bool SCORED>
__device__ __forceinline__ void mpc_loop_body(const MpcLoopUnit& Q, const PolyProgram& pl, int steps, double* mpc_lds) {
  constexpr int P = NK_POLY_MAX_P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const int m = Q.m, nv = Q.nv, d = pl.d, p = pl.p;
  const bool cheap = Q.iters == 0;
  double* Wl = mpc_lds;                       // m x nv
  double* part = Wl + (size_t)m * nv;         // waves x 64
  double* xb = part + 64 * waves;             // D words of x_{t+1}
  double* sc = xb + 4;                        // SCORED: sse_u, ss_opt, J, u_absmax, r_max (lane 0 of the first wave only)
  for (int i = tid; i < m * nv; i += nthreads) Wl[i] = Q.w[i];
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
  // the first wave: lane i owns decision variable i
  const bool var = lane < nv;
  const double inf = __builtin_huge_val();
  double Mrow[NVP], lo = -inf, hi = inf, dlo0 = -inf, dhi0 = inf, uprev = 0.0;
#pragma unroll
  for (int j = 0; j < NVP; ++j) Mrow[j] = 0.0;
  if (wave == 0 && var) {
    if (!cheap) {
#pragma unroll
      for (int j = 0; j < NVP; ++j)
        if (j < nv) Mrow[j] = Q.M[lane * nv + j];
    }
    lo = Q.bnd[lane]; hi = Q.bnd[nv + lane]; dlo0 = Q.bnd[2 * nv + lane]; dhi0 = Q.bnd[3 * nv + lane];
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
  int n_lim = 0, n_it = 0;
  if (SCORED && tid == 0) {
#pragma clang fp contract(off)
    double J = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double sq = x[k] * x[k];
      J = k == 0 ? sq : J + sq;
    }
    sc[0] = 0.0; sc[1] = 0.0; sc[2] = J; sc[3] = 0.0; sc[4] = 0.0;
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
      const double* wr = Wl + (size_t)l0 * nv + (var ? lane : 0);  // lanes without a variable read column 0 and drop the sum
      for (int l = 0; l < cnt; ++l) acc = fma(wr[(size_t)l * nv], lane_bcast(dk, l), acc);
    }
    part[64 * wave + lane] = var ? acc : 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave == 0) {  // uniform over the wave
      double g = 0.0;
      for (int w = 0; w < waves; ++w) g = g + part[64 * w + lane];
      // bounds of this step: the first p rate rows are shifted by the control applied last
      const double dlo = lane < p ? uprev + dlo0 : dlo0, dhi = lane < p ? uprev + dhi0 : dhi0;
      // A NaN in the gradient (a NaN state) or in a shifted rate bound (a NaN seed, inf - inf): the NumPy statement of the
      // iteration clips with np.minimum / np.maximum, which hand a NaN on -- every variable is NaN after the first product, all
      // `iters` iterations run, the residual is NaN and so is the control.  fmin / fmax would drop the NaN and return a bound,
      // so such a step is decided here, once, and the iteration stays as it is for every other step.
      const bool nanlane = var && (g != g || dlo != dlo || dhi != dhi);
      const bool nanstep = __ballot(nanlane) != 0;  // uniform over the wave
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
        const gconst_f64 hc = (gconst_f64)Q.Hinv + (var ? lane : 0);  // symmetric: entry `lane` of row j is entry j of row `lane`
        for (int j = 0; j < nv; ++j) a = fma(hc[j * nv], lane_bcast(g, j), a);
        s1 = var ? -a : 0.0;
        const int up = lane >= p ? lane - p : lane, dn = lane + p < 64 ? lane + p : lane;
        double sh = __shfl(s1, up, 64);
        double s2 = lane >= p ? s1 - sh : s1;
        z1 = clipd(s1, lo, hi);
        double z2 = clipd(s2, dlo, dhi), l1 = 0.0, l2 = 0.0;
        r = wave_max64_dpp(fmax(fabs(s1 - z1), fabs(s2 - z2)));
        while (it < Q.iters && !(r <= Q.tol && (it == 0 || Q.tol > 0.0))) {  // uniform: r is the same in every lane
          const double w2 = z2 - l2;
          const double w2n = __shfl(w2, dn, 64);
          const double dt = lane + p < nv ? w2 - w2n : w2;
          const double rhs = Q.rho * ((z1 - l1) + dt) - g;
          double U = 0.0;
#pragma unroll
          for (int j = 0; j < NVP; ++j) U = fma(Mrow[j], lane_bcast(rhs, j), U);
          s1 = U;
          sh = __shfl(s1, up, 64);
          s2 = lane >= p ? s1 - sh : s1;
          z1 = clipd(s1 + l1, lo, hi);
          z2 = clipd(s2 + l2, dlo, dhi);
          l1 = l1 + (s1 - z1);
          l2 = l2 + (s2 - z2);
          r = wave_max64_dpp(fmax(fabs(s1 - z1), fabs(s2 - z2)));
          ++it;
        }
      }
      // the control: both clips, the rate clip last (lanes < p; the others carry values nobody reads)
      const double uc = clipd(clipd(z1, lo, hi), dlo, dhi);
      const double un = (nanstep && (nanlane || !cheap)) ? __builtin_nan("") : uc;  // (iters = 0: entry by entry)
      if (SCORED) {  // a clip returns the bound itself: the comparisons are exact; the counts are the same in every lane
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
        if (SCORED) {  // the sums of poly_loop_body (nk_plant_loop.hip), and the residual under the NaN rule of u_absmax
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
  }
}

template <int KTYPE, int D, int NVP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES) mpc_loop_kernel(MpcLoopParams Q, PolyProgram pl) {
  extern __shared__ double mpc_lds[];
  const int b = blockIdx.x;
  MpcLoopUnit U;
  U.Z = Q.Z; U.winv = Q.winv; U.w = Q.w; U.M = Q.M; U.Hinv = Q.Hinv; U.bnd = Q.bnd;
  U.x0 = Q.x0 + (int64_t)b * Q.x0_stride;
  U.xref = Q.xref + (int64_t)b * Q.xref_stride;
  U.uinit = Q.uinit ? Q.uinit + (int64_t)b * Q.uinit_stride : nullptr;
  U.out_x = Q.out_x + (int64_t)b * (Q.steps + 1) * Q.ldx; U.ldx = Q.ldx;
  U.out_u = Q.out_u + (int64_t)b * Q.steps * Q.ldu; U.ldu = Q.ldu;
  U.out_info = Q.out_info ? Q.out_info + (int64_t)b * Q.steps * 2 : nullptr;
  U.u_opt = nullptr; U.score = nullptr;
  U.sigma0sq = Q.sigma0sq; U.rho = Q.rho; U.tol = Q.tol;
  U.m = Q.m; U.nv = Q.nv; U.iters = Q.iters; U.reserved = 0;
  mpc_loop_body<KTYPE, D, NVP, false>(U, pl, Q.steps, mpc_lds);
}

// the multi-model form: unit blockIdx.x of `table` (all units of a launch share KTYPE, NVP and the block size)
template <int KTYPE, int D, int NVP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES)
    mpc_loop_multi_kernel(const MpcLoopUnit* __restrict__ table, PolyProgram pl, int steps) {
  extern __shared__ double mpc_lds[];
  const MpcLoopUnit U = table[blockIdx.x];
  mpc_loop_body<KTYPE, D, NVP, true>(U, pl, steps, mpc_lds);
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

// all pointers device memory; w: m x nv dense (cheap: nv = p); bnd: 4 x nv
int launch_mpc_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant& plant, int nv, int iters, double rho, double tol,
                    const double* w, const double* M, const double* Hinv, const double* bnd, const double* x0, int64_t x0_stride,
                    const double* xref, int64_t xref_stride, const double* uinit, int64_t uinit_stride, int steps, int batch,
                    double* out_x, int64_t ldx, double* out_u, int64_t ldu, double* out_info) {
  const int m = mdl->m;
  NK_REQUIRE(plant.d == mdl->d && plant.p == mdl->p && nv >= 1 && nv <= NK_MPC_MAX_NV && m >= 1 && m <= mpc_loop_max_m(nv) &&
                 steps >= 1 && batch >= 1 && iters >= 0, "mpc_loop: bad sizes");
  const int waves = (m + 63) / 64;
  const size_t lds = sizeof(double) * (size_t)mpc_lds_doubles(m, nv);
  int lds_max = 0;
  NK_TRY(mpc_loop_check_lds(ctx, m, nv, &lds_max));
  MpcLoopParams Q;
  Q.Z = mdl->Z; Q.winv = mdl->winv; Q.w = w; Q.M = M; Q.Hinv = Hinv; Q.bnd = bnd;
  Q.x0 = x0; Q.x0_stride = x0_stride; Q.xref = xref; Q.xref_stride = xref_stride; Q.uinit = uinit; Q.uinit_stride = uinit_stride;
  Q.out_x = out_x; Q.ldx = ldx; Q.out_u = out_u; Q.ldu = ldu; Q.out_info = out_info;
  Q.sigma0sq = mdl->sigma0 * mdl->sigma0; Q.rho = rho; Q.tol = tol;
  Q.m = m; Q.nv = nv; Q.iters = iters; Q.steps = steps;
  const PolyProgram prog = poly_compile(plant);
  int rc_lds = NK_OK;
  NK_TRY(mpc_loop_dispatch("mpc_loop", mdl->ktype, plant.d, nv, [&](auto kt, auto dd, auto np) {
    auto* kern = mpc_loop_kernel<decltype(kt)::value, decltype(dd)::value, decltype(np)::value>;
    static const hipError_t e = dynamic_lds_register(std::min(lds_max, MPC_LDS_DOUBLES * 8), kern);  // once per instantiation
    rc_lds = dynamic_lds_status(e);
    if (rc_lds != NK_OK) return;
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64 * waves), lds, ctx->stream, Q, prog);
  }));
  NK_TRY(rc_lds);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// The multi-model form: the records are sorted (stable) into classes of (kernel family, padded variables, waves), staged with
// ONE copy and run with one launch per class.  `units` is reordered in place and must stay alive until the stream has been
// synchronised.
int launch_mpc_loop_multi(nk_ctx* ctx, const nk_poly_plant& plant, int steps, MpcLoopUnit* units, const int* ktypes,
                          int n_units) {
  NK_REQUIRE(steps >= 1 && n_units >= 1, "mpc_loop_multi: bad sizes");
  int lds_max = 0;
  NK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  struct Key { int ktype, nvp, waves, idx; };
  std::vector<Key> keys((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const int m = units[u].m, nv = units[u].nv;
    NK_REQUIRE(nv >= 1 && nv <= NK_MPC_MAX_NV && m >= 1 && m <= mpc_loop_max_m(nv) && units[u].iters >= 0 &&
                   sizeof(double) * (size_t)mpc_lds_doubles(m, nv) <= (size_t)lds_max, "mpc_loop_multi: unit %d: bad sizes", u);
    keys[u] = Key{ktypes[u], nv <= 16 ? 16 : nv <= 32 ? 32 : 64, (m + 63) / 64, u};
  }
  auto less = [](const Key& a, const Key& b) {
    if (a.ktype != b.ktype) return a.ktype < b.ktype;
    if (a.nvp != b.nvp) return a.nvp < b.nvp;
    return a.waves < b.waves;
  };
  std::stable_sort(keys.begin(), keys.end(), less);
  {
    std::vector<MpcLoopUnit> sorted((size_t)n_units);
    for (int u = 0; u < n_units; ++u) sorted[u] = units[keys[u].idx];
    std::copy(sorted.begin(), sorted.end(), units);
  }
  const PolyProgram prog = poly_compile(plant);
  MpcLoopUnit* table = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n_units, &table));
  NK_HIP(hipMemcpyAsync(table, units, sizeof(MpcLoopUnit) * (size_t)n_units, hipMemcpyHostToDevice, ctx->stream));
  for (int b = 0; b < n_units;) {
    int e = b + 1;
    long lds_doubles = mpc_lds_doubles(units[b].m, units[b].nv);
    for (; e < n_units && !less(keys[b], keys[e]); ++e) lds_doubles = std::max(lds_doubles, mpc_lds_doubles(units[e].m, units[e].nv));
    const Key& k = keys[b];
    const MpcLoopUnit* first = table + b;
    int rc_lds = NK_OK;
    NK_TRY(mpc_loop_dispatch("mpc_loop_multi", k.ktype, plant.d, k.nvp, [&](auto kt, auto dd, auto np) {
      auto* kern = mpc_loop_multi_kernel<decltype(kt)::value, decltype(dd)::value, decltype(np)::value>;
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
