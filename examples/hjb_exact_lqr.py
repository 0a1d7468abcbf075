#!/usr/bin/env python3
"""The exact-kernel control leg of the reference's benchmark_lqr_hjb.py (:334-381) on this library, with the reference's own
samples from the committed fixture: fit the exact (non-Nystrom) kernel model on the first N samples (lifted dimension N)
-> LQR gain ON THE DEVICE (Q = C'C, R = 1: the launch-chain Riccati solver, the reference calls control.dlqr here and
times it) -> closed loop around the TRUE plant x' = -x^3 + u from x = 0.9 to the origin -> relative-% RMSE of the controls
against the analytic optimum u* = x^3 - x sqrt(1 + x^4).  Needs an MI355X (the library has no CPU path):

    python3 examples/hjb_exact_lqr.py [N]        # N defaults to the fixture's exact_N
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
N = int(sys.argv[1]) if len(sys.argv) > 1 else int(g["exact_N"])
X, Y = np.ascontiguousarray(g["X"][:N]), np.ascontiguousarray(g["Y"][:N])  # snapshot pairs [x | u] -> x'
plant = nk.HJB(Ts=0.01)                                                     # dynamical_systems.py:84-112
steps = int(g["cl_steps"])

reg = nk.KoopmanKernelRegressor(1, kernel=nk.KernelWrapper([float(g["ls"])]), gamma=float(g["gamma"]))
t0 = time.perf_counter()
reg.fit(X, Y)                                                               # :341-343
print(f"exact-kernel fit: N = {N} in {time.perf_counter() - t0:.2f} s")

t0 = time.perf_counter()
K = reg.solve_lqr(c=1.0, device=True)                                       # :351-356, Q = C'C, R = I
t_gain = time.perf_counter() - t0
tm = nk.get_context().dare_large_times()
print(f"device gain: {t_gain:.2f} s ({tm['steps']} doubling steps; the solver alone {tm['ms_total'] / 1e3:.2f} s)")

x0, ref = np.array([[0.9]]), np.array([[0.0]])
t0 = time.perf_counter()
xs, us = harness.lqr_control_plant(steps, ref, x0, reg, K, plant.update_SOM)  # the plant in the loop, one lift per step
print(f"closed loop, {steps} plant-in-the-loop steps: {time.perf_counter() - t0:.2f} s; final state {xs[-1]:.4f}")

u_opt, _ = harness.hjb_optimal_control(x0, steps, plant)                    # :369-377
rmse = harness.control_rmse_percent(us, u_opt)                              # :378-379
print(f"control RMSE against the analytic optimum {rmse:.4f} % "
      f"(the Nystrom model with m = {int(g['m'])} on all samples, examples/hjb_lqr.py: {float(g['rmse_control']):.4f} %)")
