#!/usr/bin/env python3
"""The seeds x m control table of the Duffing experiments UNDER A VELOCITY LIMIT, on the committed Duffing data (n = 69 900
snapshot pairs, d = 2, p = 1): for seeds 0..7 and m = 20 and 65, draw the landmarks from np.random.RandomState(seed), fit,
build the Koopman MPC with limits on its predicted states on the host (reg.solve_mpc: horizon 8, Q = C'C, |u| <= 2, |x_2| <=
0.6 of the peak velocity of the loop without the limit) beside the fits, and run 300 steps of every unit around the true
oscillator from (-0.5, 0) to (0.5, 0) in ONE device call (nk_mpc_out_loop_multi) that returns ten numbers per unit -- the
last two say how far and how often the PLANT left the limit.  Hard rows and soft rows stand beside the table without the
state limit.  rho is the user's to set: the output rows want about 300 x the default.  Needs an MI355X (the
library has no CPU path):

    python3 examples/duffing_mpc_out_sweep.py
"""
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
x0, ref, steps, seeds, ms = np.array([-0.5, 0.0]), np.array([0.5, 0.0]), 300, list(range(8)), [20, 65]
params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))

# one number for rho, from the first fit of the plan: 300 x what solve_mpc would choose by itself
first = harness.lqr_fit_unit(X, Y, 1, params, harness.lqr_plan(X, Y, 1, params, ms, seeds)[0])
rho = 300.0 * first.solve_mpc(8, c=1.0).rho
base = dict(horizon=8, u_min=-2.0, u_max=2.0, rho=rho, iters=100)

free = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, steps, batch=8, return_trajectories=True, controller=base)
peak = np.nanmax(np.abs(free["states"][..., 1]), axis=-1)            # (seeds, ms): peak |x_2| without the state limit
v = 0.6 * float(np.nanmedian(peak))
print(f"no state limit: peak |x_2| median {np.nanmedian(peak):.3f}; the limit is set at |x_2| <= {v:.3f}")
for label, rows in (("hard rows", dict(y_weight=np.inf)), ("soft rows, weight 10 rho", dict(y_weight=10.0 * rho))):
    ctl = dict(base, x_min=[-np.inf, -v], x_max=[np.inf, v], **rows)
    res = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, steps, batch=8, return_trajectories=True, controller=ctl)
    tm = res["timing"]
    print(f"{label}: fits {tm['fit_s']:.2f} s, waiting for controllers {tm['gain_wait_s']:.2f} s, all closed loops "
          f"{tm['loop_s'] * 1e3:.1f} ms")
    pk = np.nanmax(np.abs(res["states"][..., 1]), axis=-1)
    print("  seed    " + "".join(f"m = {m:<3d}: peak |x_2|  y_viol_max  n_y_viol    " for m in ms))
    for si, seed in enumerate(seeds):
        print(f"  {seed:4d}    " + "".join(f"         {pk[si, k]:10.4f}  {res['y_viol_max'][si, k]:10.2e}  "
                                         f"{res['n_y_viol'][si, k]:8.0f}    " for k in range(len(ms))))
    for k, m in enumerate(ms):
        ok = np.isfinite(res["J"][:, k])
        print(f"  m = {m:3d}: {ok.sum()}/{len(seeds)} units ran; cost J median {np.median(res['J'][ok, k]):.2f} (no state limit: "
              f"{np.median(free['J'][ok, k]):.2f}); {np.median(res['iters_sum'][ok, k]):.0f} iterations in all, largest final "
              f"residual {np.max(res['r_max'][ok, k]):.1e}")
