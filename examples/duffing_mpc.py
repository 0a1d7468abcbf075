#!/usr/bin/env python3
"""Rate-limited regulation of the Duffing oscillator: LQR, saturated LQR and constrained Koopman MPC on the same
Nystrom-Koopman model, each closed loop around the TRUE plant in ONE device launch.  The actuator gives |u| <= u_max and
moves by at most du_max per step; the LQR loop ignores both, the saturated LQR clips the LQR control (iters = 0), the MPC
solves the condensed QP over a horizon of 16 steps at every step (nk_mpc_loop).  Needs an MI355X (the library has no CPU path):

    python3 examples/duffing_mpc.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

plant = nk.PolynomialSystem.duffing(0.01)
steps, m, N, c = 600, 40, 16, 1e2
X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))   # inputs drawn in [-1, 1]
reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6, m=m)
reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(1).choice(X.shape[0], m, False)])
reg.fit(X, Y)

x0, ref = np.array([-0.5, 0.0]), np.zeros(2)
K = reg.solve_lqr(c=c)
u0 = float(np.abs(K @ (reg.lift(x0.reshape(-1, 1)) - reg.lift(ref.reshape(-1, 1)))).max())
u_max, du_max = 0.3 * u0, 0.015 * u0                          # 30 % of that, reached in 20 steps
print(f"the LQR loop asks for |u| = {u0:.1f} at x0; the actuator gives |u| <= {u_max:.1f}, {du_max:.2f} per step")
ctl = reg.solve_mpc(N, c=c, u_min=-u_max, u_max=u_max, du_min=-du_max, du_max=du_max)
print(f"condensed QP: {ctl.nv} variables, cond(H) = {np.linalg.cond(ctl.H):.1f}, rho = {ctl.rho:.2f}")


def report(name, states, us, t):
    sc = harness.control_scores(states, us)
    du = np.abs(np.diff(np.concatenate([[0.0], us[0]]))).max()
    print(f"{name:14s} {1e6 * t / steps:7.2f} us per step; |x_end| = {np.linalg.norm(states[:, -1]):.2e}, J = {sc['J']:.1f}, "
          f"max |u| = {sc['u_absmax']:.2f}, max |du| = {du:.2f}")


for name, run in (("LQR", lambda: reg.closed_loop_plant(ctl.K, x0, ref, steps, plant)),
                  ("saturated LQR", lambda: reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=0)),
                  ("MPC, 100 it.", lambda: reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=100, tol=1e-6 * u_max))):
    run()  # first call of this shape: code-object load
    t0 = time.perf_counter()
    states, us = run()
    report(name, states, us, time.perf_counter() - t0)
_, _, info = reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=100, tol=1e-6 * u_max, return_info=True)
print(f"MPC iterations per step: mean {info[:, 0].mean():.1f}, {int((info[:, 0] == 0).sum())} steps needed none "
      f"(the unconstrained move was feasible); largest final residual {info[:, 1].max():.1e}")
