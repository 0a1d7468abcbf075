#!/usr/bin/env python3
"""The control branch of benchmark_lqr_classic.py:256-299 on this library, on the committed Duffing data (n = 69 900 snapshot
pairs, d = 2, p = 1): for seeds 0..23 and both estimators (Nystrom Matern-5/2 and thin-plate splines, m = 20), draw the
landmarks from np.random.RandomState(seed), fit, solve K = dlqr(A, B, C^T C, I) on the host, run 2000 feedback steps around
the true oscillator from (-0.5, 0) to the origin and score the run -- the fits in lock step, the gains in host threads beside
them, and all closed loops of an estimator in ONE device call (nk_plant_loop_multi) that returns four numbers per unit.
Needs an MI355X (the library has no CPU path):

    python3 examples/duffing_lqr_sweep.py [--gain device]

--gain device solves all gains of an estimator in ONE call of the batched device Riccati solver (nk_model_lqr_gain_batch)
after the fits instead of scipy in host threads (the default, and the choice for replaying the reference's numbers).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

ap = argparse.ArgumentParser()
ap.add_argument("--gain", choices=("host", "device"), default="host")
gain = ap.parse_args().gain

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
g = np.load(os.path.join(G, "f12_duffing_full.npz"))
X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])    # [x | u] -> x'
plant = nk.DuffingOscillator(Ts=0.01)
x0, ref, steps, seeds = np.array([-0.5, 0.0]), np.zeros(2), 2000, list(range(24))
configs = {"nystrom": dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"])),
           "spline": dict(gamma=1e-6, state_bounds_params=(1.0, 2.0))}

for estimator, params in configs.items():
    res = harness.lqr_sweep(X, Y, 1, params, [20], seeds, plant, x0, ref, steps, estimator=estimator, batch=8, gain=gain)
    J, umax, tm = res["J"][:, 0], res["u_absmax"][:, 0], res["timing"]
    ok = np.isfinite(J)
    print(f"{estimator:8s}: {ok.sum()}/{len(seeds)} units ran; cost J median {np.median(J[ok]):.4f} "
          f"[{np.percentile(J[ok], 15):.4f}, {np.percentile(J[ok], 85):.4f}], max |u| {np.max(umax[ok]):.3f}; "
          f"fits {tm['fit_s']:.2f} s, waiting for gains {tm['gain_wait_s']:.2f} s, closed loops {tm['loop_s'] * 1e3:.1f} ms")

# one unit with its trajectory, against the reference's recorded run of seed 0
one = harness.lqr_sweep(X, Y, 1, configs["nystrom"], [20], [0], plant, x0, ref, steps, return_trajectories=True,
                        gain=gain)
us = one["controls"][0, 0]
print("seed 0 controls vs the reference's run:", float(np.linalg.norm(us - g["lqr_us_0"][0]) / np.linalg.norm(g["lqr_us_0"])))
