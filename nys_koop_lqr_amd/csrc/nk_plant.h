// The reference's three plants (dynamical_systems.py: Duffing oscillator, double integrator, the HJB tutorial system) as
// closed-form maps x_{t+1} = plant(x_t, u_t): one Runge-Kutta step of length Ts in the reference's order of operations,
// including its quirk that k4 is evaluated at x + k1 Ts (not at x + k3 Ts).  Plain IEEE operations only (no contraction
// into fused multiply-adds, powers written as products), so the host build, the device build and
// nys_koop_lqr_amd/dynamical_systems.py give the same bits: nk_plant_step is the host build, nk_plant_loop the device one.
#pragma once
#include "nyskoop.h"

#if defined(__HIPCC__)
#define NK_PLANT_FN __host__ __device__ __forceinline__
#else
#define NK_PLANT_FN inline
#endif

namespace nk {

constexpr int PLANT_COUNT = 3;
constexpr int PLANT_MAX_D = 2;
// state dimension of a plant (0: unknown id); every plant has one input
inline int plant_dim(int plant) {
  return plant == NK_PLANT_DUFFING || plant == NK_PLANT_DOUBLE_INTEGRATOR ? 2 : (plant == NK_PLANT_HJB ? 1 : 0);
}
inline const char* plant_name(int plant) {
  return plant == NK_PLANT_DUFFING ? "Duffing oscillator"
                                   : (plant == NK_PLANT_DOUBLE_INTEGRATOR ? "double integrator" : "HJB system");
}

template <int PLANT>
struct PlantDim {
  static constexpr int value = PLANT == NK_PLANT_HJB ? 1 : 2;
};

// right-hand side f(x, u), dynamical_systems.py:25-27 / :58-60 / :92-93
template <int PLANT>
NK_PLANT_FN void plant_rhs(const double* x, double u, double* f) {
#pragma clang fp contract(off)
  if (PLANT == NK_PLANT_DUFFING) {
    // -vstack((-x2, 0.5 x2 + x1 (4 x1^2 - 1) - 0.5 u))
    f[0] = -(-x[1]);
    f[1] = -((0.5 * x[1] + x[0] * (4.0 * (x[0] * x[0]) - 1.0)) - 0.5 * u);
  } else if (PLANT == NK_PLANT_DOUBLE_INTEGRATOR) {
    f[0] = x[1];
    f[1] = u;
  } else {
    f[0] = -((x[0] * x[0]) * x[0]) + u;
  }
}

// x + (Ts / 6) (k1 + 2 k2 + 2 k3 + k4) with k2 = f(x + k1 Ts / 2), k3 = f(x + k2 Ts / 2), k4 = f(x + k1 Ts)
// (dynamical_systems.py:29-43)
template <int PLANT>
NK_PLANT_FN void plant_step(double Ts, const double* x, double u, double* x_next) {
#pragma clang fp contract(off)
  constexpr int D = PlantDim<PLANT>::value;
  double k1[D], k2[D], k3[D], k4[D], y[D];
  plant_rhs<PLANT>(x, u, k1);
  for (int i = 0; i < D; ++i) y[i] = x[i] + k1[i] * Ts / 2.0;
  plant_rhs<PLANT>(y, u, k2);
  for (int i = 0; i < D; ++i) y[i] = x[i] + k2[i] * Ts / 2.0;
  plant_rhs<PLANT>(y, u, k3);
  for (int i = 0; i < D; ++i) y[i] = x[i] + k1[i] * Ts;
  plant_rhs<PLANT>(y, u, k4);
  const double h6 = Ts / 6.0;
  for (int i = 0; i < D; ++i) y[i] = x[i] + h6 * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
  for (int i = 0; i < D; ++i) x_next[i] = y[i];
}

}  // namespace nk
