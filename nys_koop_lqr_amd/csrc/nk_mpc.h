// The condensed QP of the constrained Koopman MPC (nk_mpc_desc, include/nyskoop.h) on the host: the one validation of a
// description, the two inverses a call forms once (H^-1 and M = (H + rho (I + D'D))^-1, by Cholesky) and the fixed-step ADMM
// iteration whose order of operations the interface states.  nk_mpc_qp_host is this file behind the C ABI; the device loop
// (nk_mpc_loop.hip) runs the same steps with one lane per decision variable.  No HIP include: a plain C++17 compiler builds
// this header (tests/mpc_main.cpp).
#pragma once
#include "nyskoop.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <vector>

namespace nk {

constexpr int MPC_MAX_P = 4;
constexpr int MPC_MAX_WAVES = 8;               // 512 threads: a lane keeps a row of M in registers without scratch
constexpr int MPC_LDS_DOUBLES = 160 * 1024 / 8;  // the LDS budget of one workgroup

// LDS doubles of a loop: W (m x nv), one partial sum per wave and variable slot, the broadcast state
inline long mpc_lds_doubles(int m, int nv) { return (long)m * nv + 64L * ((m + 63) / 64) + 16; }
inline int mpc_loop_max_m(int nv) {
  if (nv < 1 || nv > NK_MPC_MAX_NV) return 0;
  int m = 64 * MPC_MAX_WAVES;
  while (m > 0 && mpc_lds_doubles(m, nv) > MPC_LDS_DOUBLES) --m;
  return m;
}

// The bound of constraint row i (i < nv) of a description: a NULL array is the infinite bound.
inline double mpc_bound(const double* a, int i, double missing) { return a ? a[i] : missing; }

// The one validation of a description, before anything is computed.  True for a valid one; otherwise false with the field
// named in msg.  (H positive definite: mpc_prepare.)
inline bool mpc_desc_check(const nk_mpc_desc* ds, char* msg, size_t len) {
  if (!ds) return snprintf(msg, len, "the description is null"), false;
  if (ds->p < 1 || ds->p > MPC_MAX_P) return snprintf(msg, len, "mpc: p = %d must lie in 1 .. %d", ds->p, MPC_MAX_P), false;
  if (ds->N < 1 || ds->N > NK_MPC_MAX_NV || ds->N * ds->p > NK_MPC_MAX_NV)
    return snprintf(msg, len, "mpc: N = %d with p = %d: nv = N p must lie in 1 .. %d", ds->N, ds->p, NK_MPC_MAX_NV), false;
  if (ds->m < 1) return snprintf(msg, len, "mpc: m = %d must be positive", ds->m), false;
  if (ds->iters < 0) return snprintf(msg, len, "mpc: iters = %d must not be negative", ds->iters), false;
  if (!std::isfinite(ds->rho) || !(ds->rho > 0.0)) return snprintf(msg, len, "mpc: rho = %g must be finite and positive", ds->rho), false;
  if (!std::isfinite(ds->tol) || ds->tol < 0.0) return snprintf(msg, len, "mpc: tol = %g must be finite and not negative", ds->tol), false;
  const int nv = ds->N * ds->p;
  for (int i = 0; i < nv; ++i) {
    const double inf = std::numeric_limits<double>::infinity();
    const double lo = mpc_bound(ds->lo, i, -inf), hi = mpc_bound(ds->hi, i, inf);
    const double dlo = mpc_bound(ds->dlo, i, -inf), dhi = mpc_bound(ds->dhi, i, inf);
    if (!(lo <= hi) || lo == inf || hi == -inf) return snprintf(msg, len, "mpc: lo[%d] = %g, hi[%d] = %g: lo <= hi is required", i, lo, i, hi), false;
    if (!(dlo <= dhi) || dlo == inf || dhi == -inf)
      return snprintf(msg, len, "mpc: dlo[%d] = %g, dhi[%d] = %g: dlo <= dhi is required", i, dlo, i, dhi), false;
  }
  if (ds->iters == 0) {
    if (!ds->K) return snprintf(msg, len, "mpc: K is null (iters = 0 is the saturated LQR)"), false;
    for (long i = 0; i < (long)ds->p * ds->m; ++i)
      if (!std::isfinite(ds->K[i])) return snprintf(msg, len, "mpc: K is not finite"), false;
    return true;
  }
  if (!ds->H) return snprintf(msg, len, "mpc: H is null"), false;
  if (!ds->F) return snprintf(msg, len, "mpc: F is null"), false;
  double hmax = 0.0;
  for (int i = 0; i < nv * nv; ++i) {
    if (!std::isfinite(ds->H[i])) return snprintf(msg, len, "mpc: H is not finite"), false;
    hmax = std::fmax(hmax, std::fabs(ds->H[i]));
  }
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j < i; ++j)
      if (std::fabs(ds->H[i * nv + j] - ds->H[j * nv + i]) > 1e-12 * hmax)
        return snprintf(msg, len, "mpc: H is not symmetric at (%d, %d)", i, j), false;
  for (long i = 0; i < (long)nv * ds->m; ++i)
    if (!std::isfinite(ds->F[i])) return snprintf(msg, len, "mpc: F is not finite"), false;
  return true;
}

// inv (n x n, dense) = A^-1 for symmetric positive definite A (the lower triangle is read): A = L L', inv = L^-T L^-1.
// False when a pivot is not positive.
inline bool mpc_spd_inverse(const double* A, int n, double* inv) {
  std::vector<double> L((size_t)n * n, 0.0), Li((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    double dg = A[j * n + j];
    for (int k = 0; k < j; ++k) dg -= L[j * n + k] * L[j * n + k];
    if (!(dg > 0.0) || !std::isfinite(dg)) return false;
    const double l = std::sqrt(dg);
    L[j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double s = A[i * n + j];
      for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
      L[i * n + j] = s / l;
    }
  }
  for (int c = 0; c < n; ++c) {  // column c of L^-1 by forward substitution
    Li[c * n + c] = 1.0 / L[c * n + c];
    for (int i = c + 1; i < n; ++i) {
      double s = 0.0;
      for (int k = c; k < i; ++k) s -= L[i * n + k] * Li[k * n + c];
      Li[i * n + c] = s / L[i * n + i];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = i; k < n; ++k) s += Li[k * n + i] * Li[k * n + j];
      inv[i * n + j] = inv[j * n + i] = s;
    }
  return true;
}

// Hinv = H^-1 and M = (H + rho (I + D'D))^-1 (nv x nv each) of a checked description with iters > 0.  I + D'D is block
// tridiagonal: 3 I (the last block: 2 I) on the diagonal, -I beside it.
inline bool mpc_prepare(const nk_mpc_desc& ds, double* Hinv, double* M, char* msg, size_t len) {
  const int nv = ds.N * ds.p, p = ds.p;
  if (!mpc_spd_inverse(ds.H, nv, Hinv)) return snprintf(msg, len, "mpc: H is not positive definite"), false;
  std::vector<double> A(ds.H, ds.H + (size_t)nv * nv);
  for (int i = 0; i < nv; ++i) {
    A[i * nv + i] += ds.rho * (i + p < nv ? 3.0 : 2.0);
    if (i + p < nv) {
      A[i * nv + i + p] -= ds.rho;
      A[(i + p) * nv + i] -= ds.rho;
    }
  }
  if (!mpc_spd_inverse(A.data(), nv, M)) return snprintf(msg, len, "mpc: H + rho (I + D'D) is not positive definite"), false;
  return true;
}

inline double mpc_clip(double v, double lo, double hi) { return std::fmin(std::fmax(v, lo), hi); }

// The saturated control from v (p entries): clip(clip(v, lo, hi), u_prev + dlo, u_prev + dhi), the rate clip last.  A NaN in v
// or in a shifted rate bound gives a NaN control, as np.minimum / np.maximum of the NumPy statement do (fmin / fmax would
// drop it and return a bound).
inline void mpc_saturate(const nk_mpc_desc& ds, const double* v, const double* u_prev, double* u) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int j = 0; j < ds.p; ++j) {
    const double up = u_prev ? u_prev[j] : 0.0;
    const double dlo = up + mpc_bound(ds.dlo, j, -inf), dhi = up + mpc_bound(ds.dhi, j, inf);
    const double a = mpc_clip(v[j], mpc_bound(ds.lo, j, -inf), mpc_bound(ds.hi, j, inf));
    u[j] = (std::isnan(v[j]) || std::isnan(dlo) || std::isnan(dhi)) ? std::numeric_limits<double>::quiet_NaN()
                                                                  : mpc_clip(a, dlo, dhi);
  }
}

// One solve with g = F e given: the iteration of include/nyskoop.h.  z1 (nv): the first nv entries of z; info: {iterations
// run, final max |s - z|}.
inline void mpc_qp(const nk_mpc_desc& ds, const double* Hinv, const double* M, const double* g, const double* u_prev,
                   double* u, double* z1_out, double* info) {
  const int nv = ds.N * ds.p, p = ds.p;
  const double inf = std::numeric_limits<double>::infinity(), rho = ds.rho;
  double lo[NK_MPC_MAX_NV], hi[NK_MPC_MAX_NV], dlo[NK_MPC_MAX_NV], dhi[NK_MPC_MAX_NV];
  double s1[NK_MPC_MAX_NV], s2[NK_MPC_MAX_NV], z1[NK_MPC_MAX_NV], z2[NK_MPC_MAX_NV], l1[NK_MPC_MAX_NV], l2[NK_MPC_MAX_NV];
  double w2[NK_MPC_MAX_NV], rhs[NK_MPC_MAX_NV];
  for (int i = 0; i < nv; ++i) {
    const double shift = i < p ? (u_prev ? u_prev[i] : 0.0) : 0.0;
    lo[i] = mpc_bound(ds.lo, i, -inf);
    hi[i] = mpc_bound(ds.hi, i, inf);
    dlo[i] = mpc_bound(ds.dlo, i, -inf) + shift;
    dhi[i] = mpc_bound(ds.dhi, i, inf) + shift;
  }
  // a NaN in the gradient or in a shifted rate bound: in the NumPy statement every variable is NaN after the first product,
  // all iterations run, the residual and the control are NaN; the step is decided here as the device loop decides it
  bool nanstep = false;
  for (int i = 0; i < nv; ++i) nanstep = nanstep || std::isnan(g[i]) || std::isnan(dlo[i]) || std::isnan(dhi[i]);
  if (nanstep) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int j = 0; j < p; ++j) u[j] = nan;
    if (z1_out)
      for (int i = 0; i < nv; ++i) z1_out[i] = nan;
    if (info) {
      info[0] = (double)ds.iters;
      info[1] = nan;
    }
    return;
  }
  double r = 0.0;
  for (int i = 0; i < nv; ++i) {
    double acc = 0.0;
    for (int j = 0; j < nv; ++j) acc += Hinv[i * nv + j] * g[j];
    s1[i] = -acc;
  }
  for (int i = 0; i < nv; ++i) {
    s2[i] = i >= p ? s1[i] - s1[i - p] : s1[i];
    z1[i] = mpc_clip(s1[i], lo[i], hi[i]);
    z2[i] = mpc_clip(s2[i], dlo[i], dhi[i]);
    l1[i] = l2[i] = 0.0;
    r = std::fmax(r, std::fmax(std::fabs(s1[i] - z1[i]), std::fabs(s2[i] - z2[i])));
  }
  int k = 0;
  while (k < ds.iters && !(r <= ds.tol && (k == 0 || ds.tol > 0.0))) {
    for (int i = 0; i < nv; ++i) w2[i] = z2[i] - l2[i];
    for (int i = 0; i < nv; ++i) {
      const double dt = i + p < nv ? w2[i] - w2[i + p] : w2[i];
      rhs[i] = rho * ((z1[i] - l1[i]) + dt) - g[i];
    }
    for (int i = 0; i < nv; ++i) {
      double acc = 0.0;
      for (int j = 0; j < nv; ++j) acc += M[i * nv + j] * rhs[j];
      s1[i] = acc;
    }
    r = 0.0;
    for (int i = 0; i < nv; ++i) {
      s2[i] = i >= p ? s1[i] - s1[i - p] : s1[i];
      z1[i] = mpc_clip(s1[i] + l1[i], lo[i], hi[i]);
      z2[i] = mpc_clip(s2[i] + l2[i], dlo[i], dhi[i]);
      l1[i] = l1[i] + (s1[i] - z1[i]);
      l2[i] = l2[i] + (s2[i] - z2[i]);
      r = std::fmax(r, std::fmax(std::fabs(s1[i] - z1[i]), std::fabs(s2[i] - z2[i])));
    }
    ++k;
  }
  mpc_saturate(ds, z1, u_prev, u);
  if (z1_out)
    for (int i = 0; i < nv; ++i) z1_out[i] = z1[i];
  if (info) {
    info[0] = (double)k;
    info[1] = r;
  }
}

// nk_mpc_qp_host on a description: 0, or -1 with the message in msg.
inline int mpc_qp_host(const nk_mpc_desc* ds, const double* e, const double* u_prev, double* out_u, double* out_z, double* out_info,
                       char* msg, size_t len) {
  if (!mpc_desc_check(ds, msg, len)) return -1;
  if (!e || !out_u) return snprintf(msg, len, "null argument (e, out_u)"), -1;
  const int nv = ds->N * ds->p, p = ds->p, m = ds->m;
  if (ds->iters == 0) {
    double v[MPC_MAX_P];
    for (int j = 0; j < p; ++j) {
      double acc = 0.0;
      for (int l = 0; l < m; ++l) acc += ds->K[(size_t)j * m + l] * e[l];
      v[j] = -acc;
    }
    mpc_saturate(*ds, v, u_prev, out_u);
    if (out_info) out_info[0] = out_info[1] = 0.0;
    return 0;
  }
  std::vector<double> Hinv((size_t)nv * nv), M((size_t)nv * nv), g((size_t)nv);
  if (!mpc_prepare(*ds, Hinv.data(), M.data(), msg, len)) return -1;
  for (int i = 0; i < nv; ++i) {
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc += ds->F[(size_t)i * m + l] * e[l];
    g[i] = acc;
  }
  mpc_qp(*ds, Hinv.data(), M.data(), g.data(), u_prev, out_u, out_z, out_info);
  return 0;
}

}  // namespace nk
