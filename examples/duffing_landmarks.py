#!/usr/bin/env python3
"""Landmark selection against uniform draws on the committed Duffing data (n = 69 900 snapshot pairs, d = 2, p = 1): the
open-loop error (relative-% RMSE of the 100-step test trajectories, harness.sysid_sweep) against m for
  uniform     the reference's draw, np.random.RandomState(seed).choice, seeds 0..2;
  greedy      pivoted-Cholesky landmarks (harness.landmark_centers, rule="greedy"): ONE selection of max(ms) rows on the
              device serves every m and every seed, since the selection is nested;
  rpcholesky  the randomised pick rule, one selection per seed (uniforms from RandomState(seed)).
Also printed: the residual trace tr(K - K_nm K_mm^-1 K_mn) the selection leaves at each m.  Needs an MI355X (the library
has no CPU path):

    python3 examples/duffing_landmarks.py
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
seeds, ms = [0, 1, 2], [int(m) for m in g["ms"][::3]]
trajs = np.stack([g[f"traj_{s}"] for s in seeds])                    # (3, d, T): the test trajectory of each seed
ctrls = np.stack([g[f"ctrl_{s}"] for s in seeds])                    # (3, p, T - 1)
params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))
test_index = [[0], [1], [2]]

tables = {}
for rule in ("uniform", "greedy", "rpcholesky"):
    centers = None if rule == "uniform" else harness.landmark_centers(Y, params["kernel"], ms, seeds, test_index, rule=rule)
    tables[rule] = harness.sysid_sweep(X, Y, 1, params, ms, seeds, trajs, ctrls, test_index=test_index, relative=True,
                                       centers=centers, batch=8)[:, 0, :]        # (seed, m)
_, info = nk.select_landmarks(Y, params["kernel"], max(ms), return_info=True)
print(f"   m   median rel-% RMSE over the seeds: uniform      greedy  rpcholesky   trace left (greedy; of {len(Y)})")
for k, m in enumerate(ms):
    print(f"{m:4d}   {np.median(tables['uniform'][:, k]):40.6f}{np.median(tables['greedy'][:, k]):12.6f}"
          f"{np.median(tables['rpcholesky'][:, k]):12.6f}   {info['trace'][m]:.4g}")
