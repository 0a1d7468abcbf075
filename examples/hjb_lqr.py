#!/usr/bin/env python3
"""The control experiment of the reference's benchmark_lqr_hjb.py (:284-313) on this library, with the reference's own samples
from the committed fixture: fit (N = 1e4, m = 200, Matern-5/2) -> LQR gain (host DARE, Q = C'C, R = 1) -> closed loop around
the TRUE plant x' = -x^3 + u from x = 0.9 to the origin, all steps in one device launch -> relative-% RMSE of the controls
against the analytic optimum u* = x^3 - x sqrt(1 + x^4).  Needs an MI355X (the library has no CPU path):

    python3 examples/hjb_lqr.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
g = np.load(os.path.join(G, "f8_hjb_config2.npz"))
X, Y = g["X"], g["Y"]                                            # 1e4 snapshot pairs: [x | u] -> x'
plant = nk.HJB(Ts=0.01)                                          # dynamical_systems.py:84-112
steps = int(g["cl_steps"])

reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([float(g["ls"])]), gamma=float(g["gamma"]), m=int(g["m"]))
reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, g["idx"]])  # the landmarks the reference drew
t0 = time.perf_counter()
reg.fit(X, Y)
print(f"fit: n = {X.shape[0]}, m = {int(g['m'])} in {1e3 * (time.perf_counter() - t0):.1f} ms")
K = reg.solve_lqr(Q=reg.C.T @ reg.C, R=np.eye(1))                # benchmark_lqr_hjb.py:293

x0, ref = np.array([[0.9]]), np.array([[0.0]])
harness.lqr_control_plant_device(steps, ref, x0, reg, K, plant)  # first call of this shape: code-object load
t0 = time.perf_counter()
xs, us = harness.lqr_control_plant_device(steps, ref, x0, reg, K, plant)
t_dev = time.perf_counter() - t0
t0 = time.perf_counter()
xs_h, us_h = harness.lqr_control_plant(steps, ref, x0, reg, K, plant.update_SOM)  # the same loop, one lift call per step
t_host = time.perf_counter() - t0
print(f"closed loop, {steps} plant-in-the-loop steps: one launch {1e3 * t_dev:.2f} ms, host loop {1e3 * t_host:.1f} ms; "
      f"controls differ by {np.linalg.norm(us - us_h) / np.linalg.norm(us_h):.1e}")

# the analytic optimum rolled through the plant (:302-308) and the figure the reference reports (:313)
x, u_opt = np.array([[0.9]]), []
for _ in range(steps):
    u = x ** 3 - x * np.sqrt(1 + x ** 4)
    u_opt.append(float(u[0, 0]))
    x = plant.update_SOM(x, u)
rmse = harness.control_rmse_percent(us, np.array(u_opt))
print(f"final state {xs[-1]:.4f}; control RMSE against the analytic optimum {rmse:.4f} % "
      f"(the reference's run on the same samples: {float(g['rmse_control']):.4f} %)")
