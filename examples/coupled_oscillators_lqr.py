#!/usr/bin/env python3
"""LQR around a plant of your own: two coupled nonlinear oscillators with two inputs (four states), described as a table of
monomials.  Snapshots of the plant -> Nystrom-Koopman fit (m = 200, Matern-5/2) -> LQR gain on the device -> 2000 closed-loop
steps around the TRUE plant in ONE device launch (nk_poly_plant_loop), against the same loop on the host with one lift call
per step.  Needs an MI355X (the library has no CPU path):

    python3 examples/coupled_oscillators_lqr.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

# x1' = x2,  x2' = -x1 - 0.5 x2 - x1^3 + 0.2 x3 + u1,  x3' = x4,  x4' = -x3 - 0.5 x4 - x3^2 x4 + 0.2 x1 + u2
# one term per monomial: (row, coefficient, exponents of x1..x4, exponents of u1, u2)
terms = [(0, 1.0, (0, 1, 0, 0), (0, 0)),
         (1, -1.0, (1, 0, 0, 0), (0, 0)), (1, -0.5, (0, 1, 0, 0), (0, 0)), (1, -1.0, (3, 0, 0, 0), (0, 0)),
         (1, 0.2, (0, 0, 1, 0), (0, 0)), (1, 1.0, (0, 0, 0, 0), (1, 0)),
         (2, 1.0, (0, 0, 0, 1), (0, 0)),
         (3, -1.0, (0, 0, 1, 0), (0, 0)), (3, -0.5, (0, 0, 0, 1), (0, 0)), (3, -1.0, (0, 0, 2, 1), (0, 0)),
         (3, 0.2, (1, 0, 0, 0), (0, 0)), (3, 1.0, (0, 0, 0, 0), (0, 1))]
plant = nk.PolynomialSystem(4, 2, terms, Ts=0.01)                 # classical RK4, one step of 0.01 per call
steps, m = 2000, 200

X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))   # [x | u] -> x', states and inputs in [-1, 1]
reg = nk.KoopmanNystromRegressor(2, kernel=nk.KernelWrapper([1.0] * 4), gamma=1e-6, m=m)
reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(1).choice(X.shape[0], m, False)])
t0 = time.perf_counter()
reg.fit(X, Y)
print(f"fit: n = {X.shape[0]}, m = {m} in {1e3 * (time.perf_counter() - t0):.1f} ms")
K = reg.solve_lqr(c=1.0, device=True)                             # K = dlqr(A, B, sym(C'C), I) on the device, 2 x m
print(f"gain: {K.shape}, |K| = {np.linalg.norm(K):.3f}")

x0, ref = 0.5 * np.ones(4), np.zeros(4)
reg.closed_loop_plant(K, x0, ref, steps, plant)                   # first call of this shape: code-object load
t0 = time.perf_counter()
states, us = reg.closed_loop_plant(K, x0, ref, steps, plant)      # states (4, steps + 1), controls (2, steps)
t_dev = time.perf_counter() - t0
t0 = time.perf_counter()
_, us_h = harness.lqr_control_plant(steps, ref, x0, reg, K, plant.update_SOM)   # the same loop, one lift call per step
t_host = time.perf_counter() - t0
print(f"closed loop, {steps} plant-in-the-loop steps: one launch {1e3 * t_dev:.2f} ms ({1e6 * t_dev / steps:.2f} us per step), "
      f"host loop {1e3 * t_host:.1f} ms; controls differ by {np.linalg.norm(us - us_h) / np.linalg.norm(us_h):.1e}")
sc = harness.control_scores(states, us)
print(f"|x| from {np.linalg.norm(x0):.3f} to {np.linalg.norm(states[:, -1]):.2e}; cost J = {sc['J']:.4f}, max |u| = {sc['u_absmax']:.3f}")
# every state the device returned is the library's host step of the state and control before it, bit for bit
assert all(np.array_equal(states[:, t + 1], plant.step_library(states[:, t], us[:, t])) for t in range(0, steps, 97))
