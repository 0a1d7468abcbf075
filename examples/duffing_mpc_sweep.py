#!/usr/bin/env python3
"""The seeds x m control table of the Duffing experiments UNDER ACTUATOR LIMITS, on the committed Duffing data (n = 69 900
snapshot pairs, d = 2, p = 1): for seeds 0..23 and m = 20 and 65, draw the landmarks from np.random.RandomState(seed), fit,
build the constrained Koopman MPC of every fit on the host (reg.solve_mpc: horizon 8, Q = 100 C'C, |u| <= 10, at most 1 per
step) beside the fits, and run 600 steps of every unit around the true oscillator from (-0.5, 0) to the origin in ONE device
call (nk_mpc_loop_multi) that returns eight numbers per unit.  The same table without limits (harness.lqr_sweep as before)
stands beside it: the unconstrained loops ask for inputs far outside that range.  Needs an MI355X (the library has no CPU
path):

    python3 examples/duffing_mpc_sweep.py [--build device]

--build device builds the controllers of all fits in ONE device call after the fits (nk_model_mpc_build_batch) instead of on
the host threads.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
g = np.load(os.path.join(G, "f12_duffing_full.npz"))
X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])    # [x | u] -> x'
plant = nk.DuffingOscillator(Ts=0.01)
x0, ref, steps, seeds, ms = np.array([-0.5, 0.0]), np.zeros(2), 600, list(range(24)), [20, 65]
params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))
ap = argparse.ArgumentParser()
ap.add_argument("--build", choices=("host", "device"), default="host")
limits = dict(horizon=8, u_min=-10.0, u_max=10.0, du_min=-1.0, du_max=1.0, build=ap.parse_args().build)

free = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, steps, c=1e2, batch=8)
for label, ctl in (("saturated LQR", dict(limits, iters=0)), ("MPC, 50 iterations", dict(limits, iters=50))):
    res = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, steps, c=1e2, batch=8, controller=ctl)
    tm = res["timing"]
    print(f"{label}: fits {tm['fit_s']:.2f} s, waiting for controllers {tm['gain_wait_s']:.2f} s, all closed loops "
          f"{tm['loop_s'] * 1e3:.1f} ms")
    for k, m in enumerate(ms):
        ok = np.isfinite(res["J"][:, k])
        print(f"  m = {m:3d}: {ok.sum()}/{len(seeds)} units ran; cost J median {np.median(res['J'][ok, k]):.1f} (no limits: "
              f"{np.median(free['J'][ok, k]):.1f}), max |u| {np.max(res['u_absmax'][ok, k]):.2f} (no limits: "
              f"{np.max(free['u_absmax'][ok, k]):.1f}); at a limit on {np.median(res['n_at_limit'][ok, k]):.0f} of {steps} steps, "
              f"{np.median(res['iters_sum'][ok, k]):.0f} iterations in all, largest final residual "
              f"{np.max(res['r_max'][ok, k]):.1e}")
