#!/usr/bin/env python3
"""The multi-seed system-identification sweep of benchmark_lqr_classic.py:211-255 on this library, on the committed Duffing
data (n = 69 900 snapshot pairs, d = 2, p = 1): for seeds 0..2 and the 20 values of m = around(logspace(1, 2.3, 20)), draw the
landmarks from np.random.RandomState(seed), fit KoopmanNystromRegressor (Matern-5/2) and score the seed's 100-step test
trajectory in open loop (relative-% RMSE) -- 60 units in ONE lock-step batched call (nk_sysid_grid): the scores are reduced
on the device, two numbers per trajectory come back.  Needs an MI355X (the library has no CPU path):

    python3 examples/duffing_sysid_sweep.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
g = np.load(os.path.join(G, "f12_duffing_full.npz"))
X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])    # [x | u] -> x'
seeds, ms = [0, 1, 2], g["ms"]
trajs = np.stack([g[f"traj_{s}"] for s in seeds])                    # (3, d, T): the test trajectory of each seed
ctrls = np.stack([g[f"ctrl_{s}"] for s in seeds])                    # (3, p, T - 1)
params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))

for batch in (8, 8, 0):
    t0 = time.perf_counter()
    table = harness.sysid_sweep(X, Y, 1, params, ms, seeds, trajs, ctrls, test_index=[[0], [1], [2]], relative=True,
                                batch=batch)
    dt = time.perf_counter() - t0
    print(f"batch={batch}: {table.size} units in {dt:.2f} s" + (" (first call: pools and workspaces are created)" if batch and dt > 1 else ""))
rmse = table[:, 0, :]                                                # (seed, m)
ref = g["ref_rmse"]
print("   m   median rel-% RMSE over the seeds   (reference)")
for k, m in enumerate(ms):
    print(f"{int(m):4d}   {np.median(rmse[:, k]):12.6f}                  ({np.median(ref[:, k]):.6f})")
