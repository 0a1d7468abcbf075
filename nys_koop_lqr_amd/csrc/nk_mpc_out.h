// Limits on predicted states in the constrained Koopman MPC (nk_mpc_out beside nk_mpc_desc, include/nyskoop.h) on the host:
// the validation of the output rows, the matrices a call forms once (M = (H + rho (I + D'D + G'G))^-1 by Cholesky, the folded
// Kb = [[M, M G'], [G M, G M G']] and S0 = [H^-1; G H^-1]) and the folded fixed-step ADMM iteration whose order of operations
// the interface states.  nk_mpc_out_qp_host is this file behind the C ABI; the device loop (nk_mpc_loop.hip, OUT = true) runs the same
// steps with one lane per entry of s_K = (s_1, s_3).  No HIP include: a plain C++17 compiler builds this header
// (tests/mpc_out_main.cpp).
#pragma once
#include "nk_mpc.h"

namespace nk {

constexpr int MPC_OUT_MAX_D = 4;  // the states of the plants of the loop: ycomp of the host solve is checked against it

inline int mpc_out_ycomp(const nk_mpc_out* out, int r) { return out->ycomp ? out->ycomp[r] : -1; }

// The validation of a description with output rows, before anything is computed; d: the states ycomp may name.  True for a
// valid pair; otherwise false with the field named in msg.  (The matrices positive definite: mpc_out_prepare.)
inline bool mpc_out_check(const nk_mpc_desc* ds, const nk_mpc_out* out, int d, char* msg, size_t len) {
  if (!mpc_desc_check(ds, msg, len)) return false;
  if (ds->iters < 1)
    return snprintf(msg, len, "mpc_out: iters = %d must be at least 1 (the saturated LQR is nk_mpc_loop's)", ds->iters), false;
  if (!out) return snprintf(msg, len, "mpc_out: the output description is null"), false;
  const int nv = ds->N * ds->p, ny = out->ny;
  if (ny < 1 || ny > NK_MPC_MAX_NV - nv)
    return snprintf(msg, len, "mpc_out: ny = %d with nv = %d: ny must lie in 1 .. %d (nv + ny <= %d)", ny, nv,
                    NK_MPC_MAX_NV - nv, NK_MPC_MAX_NV), false;
  if (!(out->y_weight > 0.0))
    return snprintf(msg, len, "mpc_out: y_weight = %g must be positive (inf: hard rows)", out->y_weight), false;
  if (!out->G) return snprintf(msg, len, "mpc_out: G is null"), false;
  if (!out->T) return snprintf(msg, len, "mpc_out: T is null"), false;
  for (long i = 0; i < (long)ny * nv; ++i)
    if (!std::isfinite(out->G[i])) return snprintf(msg, len, "mpc_out: G is not finite"), false;
  for (long i = 0; i < (long)ny * ds->m; ++i)
    if (!std::isfinite(out->T[i])) return snprintf(msg, len, "mpc_out: T is not finite"), false;
  const double inf = std::numeric_limits<double>::infinity();
  for (int r = 0; r < ny; ++r) {
    const double lo = mpc_bound(out->ylo, r, -inf), hi = mpc_bound(out->yhi, r, inf);
    if (!(lo <= hi) || lo == inf || hi == -inf)
      return snprintf(msg, len, "mpc_out: ylo[%d] = %g, yhi[%d] = %g: ylo <= yhi is required", r, lo, r, hi), false;
    const int c = mpc_out_ycomp(out, r);
    if (c < -1 || c >= d) return snprintf(msg, len, "mpc_out: ycomp[%d] = %d must lie in -1 .. %d", r, c, d - 1), false;
  }
  return true;
}

// Kb (nt x nt, nt = nv + ny) and S0 transposed (S0t[j nt + i] = S0[i][j], nv x nt: lane i of the device loop reads
// consecutive words) of a checked pair.
inline bool mpc_out_prepare(const nk_mpc_desc& ds, const nk_mpc_out& out, double* Kb, double* S0t, char* msg, size_t len) {
  const int nv = ds.N * ds.p, p = ds.p, ny = out.ny, nt = nv + ny;
  const double* G = out.G;
  std::vector<double> Hinv((size_t)nv * nv), M((size_t)nv * nv), A(ds.H, ds.H + (size_t)nv * nv), MG((size_t)nv * ny);
  if (!mpc_spd_inverse(ds.H, nv, Hinv.data())) return snprintf(msg, len, "mpc: H is not positive definite"), false;
  for (int i = 0; i < nv; ++i) {
    A[i * nv + i] += ds.rho * (i + p < nv ? 3.0 : 2.0);
    if (i + p < nv) {
      A[i * nv + i + p] -= ds.rho;
      A[(i + p) * nv + i] -= ds.rho;
    }
  }
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int r = 0; r < ny; ++r) s += G[r * nv + i] * G[r * nv + j];
      A[i * nv + j] += ds.rho * s;
      if (j < i) A[j * nv + i] += ds.rho * s;
    }
  if (!mpc_spd_inverse(A.data(), nv, M.data()))
    return snprintf(msg, len, "mpc_out: M^-1 = H + rho (I + D'D + G'G) is not positive definite"), false;
  for (int i = 0; i < nv; ++i)
    for (int r = 0; r < ny; ++r) {
      double s = 0.0;
      for (int k = 0; k < nv; ++k) s += M[i * nv + k] * G[r * nv + k];
      MG[(size_t)i * ny + r] = s;
    }
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j < nv; ++j) Kb[i * nt + j] = M[i * nv + j];
  for (int i = 0; i < nv; ++i)
    for (int r = 0; r < ny; ++r) {
      double gm = 0.0;  // (G M)[r][i]
      for (int k = 0; k < nv; ++k) gm += G[r * nv + k] * M[k * nv + i];
      Kb[i * nt + nv + r] = Kb[(nv + r) * nt + i] = (MG[(size_t)i * ny + r] + gm) / 2;
    }
  for (int r = 0; r < ny; ++r)
    for (int s = 0; s < ny; ++s) {
      double a = 0.0;  // (G (M G'))[r][s]
      for (int k = 0; k < nv; ++k) a += G[r * nv + k] * MG[(size_t)k * ny + s];
      Kb[(nv + r) * nt + nv + s] = a;
    }
  for (int r = 0; r < ny; ++r)
    for (int s = 0; s < r; ++s) {
      const double a = (Kb[(nv + r) * nt + nv + s] + Kb[(nv + s) * nt + nv + r]) / 2;
      Kb[(nv + r) * nt + nv + s] = Kb[(nv + s) * nt + nv + r] = a;
    }
  for (int j = 0; j < nv; ++j) {
    for (int i = 0; i < nv; ++i) S0t[j * nt + i] = Hinv[i * nv + j];
    for (int r = 0; r < ny; ++r) {
      double s = 0.0;
      for (int k = 0; k < nv; ++k) s += G[r * nv + k] * Hinv[k * nv + j];
      S0t[j * nt + nv + r] = s;
    }
  }
  return true;
}

inline double mpc_out_theta(double rho, double y_weight) { return std::isinf(y_weight) ? 0.0 : rho / (rho + y_weight); }

// The bound of output row r in error coordinates: b = ylo_r - x_ref[ycomp_r], one rounded subtraction (no shift for
// ycomp = -1 or without x_ref).
inline double mpc_out_bound(const nk_mpc_out& out, const double* a, int r, double missing, const double* x_ref) {
  const double b = mpc_bound(a, r, missing);
  const int c = mpc_out_ycomp(&out, r);
  return (x_ref && c >= 0) ? b - x_ref[c] : b;
}

// the prox of an output row: c = clip(v), z = c + theta (v - c)  (theta = 0: the hard clip)
inline double mpc_out_prox(double v, double lo, double hi, double theta) {
  const double c = mpc_clip(v, lo, hi);
  return theta != 0.0 ? c + theta * (v - c) : c;
}

// One solve with g = F e and t = T e given: the folded iteration of include/nyskoop.h.  zK (nt): (z_1, z_3); info:
// {iterations run, final max |s - z|}.
inline void mpc_out_qp(const nk_mpc_desc& ds, const nk_mpc_out& out, const double* Kb, const double* S0t, const double* g,
                       const double* t, const double* x_ref, const double* u_prev, double* u, double* zK_out, double* info) {
  constexpr int NT = NK_MPC_MAX_NV;
  const int nv = ds.N * ds.p, p = ds.p, ny = out.ny, nt = nv + ny;
  const double inf = std::numeric_limits<double>::infinity(), rho = ds.rho, theta = mpc_out_theta(rho, out.y_weight);
  double lo[NT], hi[NT], dlo[NT], dhi[NT], ylo[NT], yhi[NT];
  double sK[NT], s2[NT], zK[NT], z2[NT], lK[NT], l2[NT], w2[NT], q[NT];
  for (int i = 0; i < nv; ++i) {
    const double shift = i < p ? (u_prev ? u_prev[i] : 0.0) : 0.0;
    lo[i] = mpc_bound(ds.lo, i, -inf);
    hi[i] = mpc_bound(ds.hi, i, inf);
    dlo[i] = mpc_bound(ds.dlo, i, -inf) + shift;
    dhi[i] = mpc_bound(ds.dhi, i, inf) + shift;
  }
  for (int r = 0; r < ny; ++r) {
    ylo[r] = mpc_out_bound(out, out.ylo, r, -inf, x_ref) - t[r];
    yhi[r] = mpc_out_bound(out, out.yhi, r, inf, x_ref) - t[r];
  }
  // the NaN rule of mpc_qp, extended to t and to the shifted output bounds
  bool nanstep = false;
  for (int i = 0; i < nv; ++i) nanstep = nanstep || std::isnan(g[i]) || std::isnan(dlo[i]) || std::isnan(dhi[i]);
  for (int r = 0; r < ny; ++r) nanstep = nanstep || std::isnan(t[r]) || std::isnan(ylo[r]) || std::isnan(yhi[r]);
  if (nanstep) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int j = 0; j < p; ++j) u[j] = nan;
    if (zK_out)
      for (int i = 0; i < nt; ++i) zK_out[i] = nan;
    if (info) {
      info[0] = (double)ds.iters;
      info[1] = nan;
    }
    return;
  }
  // rows of s from s_K, z = prox(s + lambda), lambda += s - z (first = true: lambda = 0 and stays), r = max |s - z|
  auto rows = [&](bool first) {
    double r = 0.0;
    for (int i = 0; i < nv; ++i) {
      s2[i] = i >= p ? sK[i] - sK[i - p] : sK[i];
      if (first) lK[i] = l2[i] = 0.0;
      zK[i] = mpc_clip(sK[i] + lK[i], lo[i], hi[i]);
      z2[i] = mpc_clip(s2[i] + l2[i], dlo[i], dhi[i]);
      if (!first) {
        lK[i] = lK[i] + (sK[i] - zK[i]);
        l2[i] = l2[i] + (s2[i] - z2[i]);
      }
      r = std::fmax(r, std::fmax(std::fabs(sK[i] - zK[i]), std::fabs(s2[i] - z2[i])));
    }
    for (int i = nv; i < nt; ++i) {
      if (first) lK[i] = 0.0;
      zK[i] = mpc_out_prox(sK[i] + lK[i], ylo[i - nv], yhi[i - nv], theta);
      if (!first) lK[i] = lK[i] + (sK[i] - zK[i]);
      r = std::fmax(r, std::fabs(sK[i] - zK[i]));
    }
    return r;
  };
  for (int i = 0; i < nt; ++i) {
    double acc = 0.0;
    for (int j = 0; j < nv; ++j) acc += S0t[j * nt + i] * g[j];
    sK[i] = -acc;
  }
  double r = rows(true);
  int k = 0;
  while (k < ds.iters && !(r <= ds.tol && (k == 0 || ds.tol > 0.0))) {
    for (int i = 0; i < nv; ++i) w2[i] = z2[i] - l2[i];
    for (int i = 0; i < nv; ++i) {
      const double dt = i + p < nv ? w2[i] - w2[i + p] : w2[i];
      q[i] = rho * ((zK[i] - lK[i]) + dt) - g[i];
    }
    for (int i = nv; i < nt; ++i) q[i] = rho * (zK[i] - lK[i]);
    for (int i = 0; i < nt; ++i) {
      double acc = 0.0;
      for (int j = 0; j < nt; ++j) acc += Kb[i * nt + j] * q[j];
      sK[i] = acc;
    }
    r = rows(false);
    ++k;
  }
  mpc_saturate(ds, zK, u_prev, u);
  if (zK_out)
    for (int i = 0; i < nt; ++i) zK_out[i] = zK[i];
  if (info) {
    info[0] = (double)k;
    info[1] = r;
  }
}

// nk_mpc_out_qp_host on a pair of descriptions: 0, or -1 with the message in msg.
inline int mpc_out_qp_host(const nk_mpc_desc* ds, const nk_mpc_out* out, const double* e, const double* x_ref,
                           const double* u_prev, double* out_u, double* out_z, double* out_info, char* msg, size_t len) {
  if (!mpc_out_check(ds, out, MPC_OUT_MAX_D, msg, len)) return -1;
  if (!e || !out_u) return snprintf(msg, len, "null argument (e, out_u)"), -1;
  const int nv = ds->N * ds->p, m = ds->m, ny = out->ny, nt = nv + ny;
  std::vector<double> Kb((size_t)nt * nt), S0t((size_t)nv * nt), gt((size_t)nt);
  if (!mpc_out_prepare(*ds, *out, Kb.data(), S0t.data(), msg, len)) return -1;
  for (int i = 0; i < nt; ++i) {
    const double* row = i < nv ? ds->F + (size_t)i * m : out->T + (size_t)(i - nv) * m;
    double acc = 0.0;
    for (int l = 0; l < m; ++l) acc += row[l] * e[l];
    gt[i] = acc;
  }
  mpc_out_qp(*ds, *out, Kb.data(), S0t.data(), gt.data(), gt.data() + nv, x_ref, u_prev, out_u, out_z, out_info);
  return 0;
}

}  // namespace nk
