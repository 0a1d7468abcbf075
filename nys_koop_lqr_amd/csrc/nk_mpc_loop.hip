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
#include "nk_common.h"
#include "nk_mpc.h"
#include "nk_poly_lanes.h"

#include <type_traits>

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

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

template <int KTYPE, int D, int NVP>
__global__ void __launch_bounds__(64 * MPC_MAX_WAVES) mpc_loop_kernel(MpcLoopParams Q, PolyProgram pl) {
  extern __shared__ double mpc_lds[];
  constexpr int P = NK_POLY_MAX_P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const int m = Q.m, nv = Q.nv, d = pl.d, p = pl.p, b = blockIdx.x;
  const bool cheap = Q.iters == 0;
  double* Wl = mpc_lds;                       // m x nv
  double* part = Wl + (size_t)m * nv;         // waves x 64
  double* xb = part + 64 * waves;             // D words of x_{t+1}
  for (int i = tid; i < m * nv; i += nthreads) Wl[i] = Q.w[i];
  const PolyLanes tb(pl, lane);
  const double* x0 = Q.x0 + (int64_t)b * Q.x0_stride;
  const double* xrp = Q.xref + (int64_t)b * Q.xref_stride;
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
    if (lane < p && Q.uinit) uprev = Q.uinit[(int64_t)b * Q.uinit_stride + lane];
  }
  double* ox = Q.out_x + (int64_t)b * (Q.steps + 1) * Q.ldx;
  double* ou = Q.out_u + (int64_t)b * Q.steps * Q.ldu;
  double* oi = Q.out_info ? Q.out_info + (int64_t)b * Q.steps * 2 : nullptr;
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k < d) ox[k] = x[k];
  }
  const int l0 = 64 * wave, cnt = min(64, m - l0);  // this wave's landmarks
  __syncthreads();  // W is in LDS
  for (int t = 0; t < Q.steps; ++t) {
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
      double s1 = 0.0, z1, r = 0.0;
      int it = 0;
      if (cheap) {
        z1 = -g;
      } else {
        double a = 0.0;
        const double* hc = Q.Hinv + (var ? lane : 0);  // symmetric: entry `lane` of row j is entry j of row `lane`
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
      const double un = clipd(clipd(z1, lo, hi), dlo, dhi);
      uprev = un;
      double u[P], xn[D];
#pragma unroll
      for (int j = 0; j < P; ++j) u[j] = j < p ? lane_bcast(un, j) : 0.0;
      poly_plant_step<D, P>(tb, x, u, xn);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) xb[k] = xn[k];
#pragma unroll
        for (int j = 0; j < P; ++j)
          if (j < p) ou[(int64_t)t * Q.ldu + j] = u[j];
#pragma unroll
        for (int k = 0; k < D; ++k)
          if (k < d) ox[(int64_t)(t + 1) * Q.ldx + k] = xn[k];
        if (oi) {
          oi[2 * (int64_t)t] = (double)it;
          oi[2 * (int64_t)t + 1] = r;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xb[k];
  }
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
  auto go = [&](auto kt, auto dd, auto np) {
    auto* kern = mpc_loop_kernel<decltype(kt)::value, decltype(dd)::value, decltype(np)::value>;
    static const hipError_t e = dynamic_lds_register(std::min(lds_max, MPC_LDS_DOUBLES * 8), kern);  // once per instantiation
    rc_lds = dynamic_lds_status(e);
    if (rc_lds != NK_OK) return;
    hipLaunchKernelGGL(kern, dim3(batch), dim3(64 * waves), lds, ctx->stream, Q, prog);
  };
  auto with_nv = [&](auto kt, auto dd) {
    if (nv <= 16) go(kt, dd, std::integral_constant<int, 16>{});
    else if (nv <= 32) go(kt, dd, std::integral_constant<int, 32>{});
    else go(kt, dd, std::integral_constant<int, 64>{});
  };
  auto with_d = [&](auto kt) {
    if (poly_pad_d(plant.d) == 2) with_nv(kt, std::integral_constant<int, 2>{});
    else with_nv(kt, std::integral_constant<int, 4>{});
  };
  switch (mdl->ktype) {
    case NK_KERNEL_RBF: with_d(std::integral_constant<int, NK_KERNEL_RBF>{}); break;
    case NK_KERNEL_MATERN52: with_d(std::integral_constant<int, NK_KERNEL_MATERN52>{}); break;
    case NK_KERNEL_LINEAR: with_d(std::integral_constant<int, NK_KERNEL_LINEAR>{}); break;
    case NK_KERNEL_TPS: with_d(std::integral_constant<int, NK_KERNEL_TPS>{}); break;
    default: set_error("mpc_loop: unknown kernel type %d", mdl->ktype); return NK_ERR_BAD_ARG;
  }
  NK_TRY(rc_lds);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
