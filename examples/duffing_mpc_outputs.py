#!/usr/bin/env python3
"""Limits on predicted states in the Koopman MPC: the Duffing oscillator from (-0.5, 0) to the equilibrium (0.5, 0) with
|u| <= 2, once with input limits only and once with an overshoot limit on x_1 and a velocity limit on x_2 over the horizon,
hard and soft.  Each closed loop runs around the TRUE plant in ONE device launch (nk_mpc_loop / nk_mpc_out_loop).  No clip of
an LQR control can hold a velocity limit; the QP with output rows does.  Needs an MI355X (the library has no CPU path):

    python3 examples/duffing_mpc_outputs.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

plant = nk.PolynomialSystem.duffing(0.01)
steps, m, N, u_max = 400, 40, 32, 2.0
X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))   # inputs drawn in [-1, 1]
reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6, m=m)
reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(1).choice(X.shape[0], m, False)])
reg.fit(X, Y)

x0, ref = np.array([-0.5, 0.0]), np.array([0.5, 0.0])
# One step moves a velocity by 0.5 Ts u: the output rows are small beside the identity rows of the inputs, and the ADMM step
# has to be far above the default for them to converge in a hundred iterations.
rho = 300.0 * reg.solve_mpc(N, c=1.0).rho
free = reg.solve_mpc(N, c=1.0, u_min=-u_max, u_max=u_max, rho=rho)
S0, U0 = reg.closed_loop_plant_mpc(free, x0, ref, steps, plant, iters=100)
x1_max, v_max = 0.55, 0.6 * float(np.abs(S0[1]).max())
print(f"input limits only: peak x_1 = {S0[0].max():.3f}, peak |x_2| = {np.abs(S0[1]).max():.3f}")
print(f"limits: x_1 <= {x1_max}, |x_2| <= {v_max:.3f} over {N // 2} predicted steps ({N + 2 * (N // 2)} lanes)")
for name, w in (("hard rows", np.inf), ("soft rows, w_y = 10 rho", 10.0 * rho)):
    ctl = reg.solve_mpc(N, c=1.0, u_min=-u_max, u_max=u_max, rho=rho, x_min=[-np.inf, -v_max], x_max=[x1_max, v_max],
                        y_horizon=N // 2, y_weight=w)
    S, U, info = reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=100, return_info=True)
    print(f"{name:24s}: peak x_1 = {S[0].max():.3f}, peak |x_2| = {np.abs(S[1]).max():.3f} "
          f"({np.abs(S[1]).max() / np.abs(S0[1]).max():.2f} of the peak without the rows), final state "
          f"({S[0, -1]:.3f}, {S[1, -1]:.3f}), largest final residual {info[:, 1].max():.1e}")
