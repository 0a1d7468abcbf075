// Device-side pieces of the polynomial-plant loops that more than one translation unit instantiates (nk_plant_loop.hip, nk_mpc_loop.hip):
// the kernel value of one landmark, the plant table compiled for the lanes of a wave (PolyProgram, poly_compile) and its
// evaluation (PolyLanes).  Moved here unchanged from nk_plant_loop.hip.
#pragma once
#include "nk_common.h"
#include "nk_plant.h"
#include "nk_poly_plant.h"

#include <algorithm>

namespace nk {

constexpr int PLANT_LOOP_MAX_WAVES = 16;
constexpr int poly_pad_d(int d) { return d <= 2 ? 2 : 4; }

template <int KTYPE, int D>
__device__ __forceinline__ double plant_kval(const double* xs, const double* zs, double sigma0sq) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if (KTYPE == NK_KERNEL_LINEAR) {
      acc = fma(xs[k], zs[k], acc);
    } else {
      const double df = xs[k] - zs[k];
      acc = fma(df, df, acc);
    }
  }
  if (KTYPE == NK_KERNEL_TPS) return tps_value(acc);
  return chain_kfun(KTYPE, acc, sigma0sq);
}

// The plant table as the device loop wants it, compiled on the host from a validated description (poly_compile) and passed
// by value in the kernel arguments.  The terms are sorted by row -- stable, so the terms of a row keep their table order,
// which is all the order of the row sums depends on --; max_e[v] is the largest exponent any term gives variable v (states,
// then inputs).
struct PolyProgram {
  int32_t d, p, n, from_k1;
  double Ts;
  int32_t row_end[NK_POLY_MAX_D];  // row r owns the sorted terms [row_end[r - 1], row_end[r])
  int32_t max_e[NK_POLY_MAX_D + NK_POLY_MAX_P];
  uint32_t word[NK_POLY_MAX_TERMS];  // poly_pack_term of the sorted terms (0 beyond n)
  double coef[NK_POLY_MAX_TERMS];
};
inline PolyProgram poly_compile(const nk_poly_plant& pl) {
  PolyProgram g = {};
  g.d = pl.d; g.p = pl.p; g.n = pl.n_terms; g.from_k1 = pl.k4_at_k1; g.Ts = pl.Ts;
  int at = 0;
  for (int r = 0; r < NK_POLY_MAX_D; ++r) {
    for (int i = 0; i < pl.n_terms; ++i) {
      const nk_poly_term& t = pl.terms[i];
      if (t.row != r) continue;
      g.word[at] = poly_pack_term(t);
      g.coef[at] = t.coef;
      for (int k = 0; k < NK_POLY_MAX_D; ++k) g.max_e[k] = std::max<int32_t>(g.max_e[k], t.ex[k]);
      for (int j = 0; j < NK_POLY_MAX_P; ++j) g.max_e[NK_POLY_MAX_D + j] = std::max<int32_t>(g.max_e[NK_POLY_MAX_D + j], t.eu[j]);
      ++at;
    }
    g.row_end[r] = at;
  }
  return g;
}

// The right-hand side in the lanes of a wave.  The four right-hand sides of a step are on its latency chain, and a single
// wave issues one instruction every few cycles: walking the table term by term costs about 35 instructions per term
// (measured: 2.5 us per step for the five terms of the Duffing table with the terms fetched by v_readlane, 3.5 us with
// the terms fetched from the kernel arguments).  Here lane l holds sorted term l (its word and coefficient,
// loaded once before the loop) and ALL terms are evaluated at once: for every variable, max_e rounds of
// v = v * (e < the lane's exponent ? x_k : 1.0) -- a product with 1.0 changes no bit, so every term sees exactly its own
// multiplications in the order of the interface.  Then the rows are summed in table order, f[r] = f[r] + v of lane i for
// the lanes of row r, v fetched with v_readlane at the uniform index i.  All control flow is uniform.
struct PolyLanes {
  int n, from_k1;
  double ts;
  int row_end[NK_POLY_MAX_D], max_e[NK_POLY_MAX_D + NK_POLY_MAX_P];
  int w;     // per lane
  double c;  // per lane
  __device__ __forceinline__ PolyLanes(const PolyProgram& g, int lane) : n(g.n), from_k1(g.from_k1), ts(g.Ts) {
#pragma unroll
    for (int r = 0; r < NK_POLY_MAX_D; ++r) row_end[r] = g.row_end[r];
#pragma unroll
    for (int v = 0; v < NK_POLY_MAX_D + NK_POLY_MAX_P; ++v) max_e[v] = g.max_e[v];
    const int li = lane & (NK_POLY_MAX_TERMS - 1);
    w = (int)g.word[li];
    c = g.coef[li];
  }
  __device__ __forceinline__ double Ts() const { return ts; }
  __device__ __forceinline__ bool k4_at_k1() const { return from_k1 != 0; }
  template <int D, int P>
  __device__ __forceinline__ void rhs(const double* x, const double* u, double* f) const {
#pragma clang fp contract(off)
    double v = c;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const int ex = (w >> (2 + 3 * k)) & 7;
      for (int e = 0; e < max_e[k]; ++e) v = v * (e < ex ? x[k] : 1.0);
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int eu = (w >> (14 + 3 * j)) & 7;
      for (int e = 0; e < max_e[NK_POLY_MAX_D + j]; ++e) v = v * (e < eu ? u[j] : 1.0);
    }
    const int vlo = __double2loint(v), vhi = __double2hiint(v);
    int i = 0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
      double acc = 0.0;
      for (; i < row_end[r]; ++i)
        acc = acc + __hiloint2double(__builtin_amdgcn_readlane(vhi, i), __builtin_amdgcn_readlane(vlo, i));
      f[r] = acc;
    }
  }
};

}  // namespace nk
