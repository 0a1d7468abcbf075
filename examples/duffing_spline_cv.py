#!/usr/bin/env python3
"""The spline branch of learn_hyperparams (benchmark_lqr_classic.py:54-60) on this library, on the committed Duffing
validation set (n = 3980 snapshot pairs, d = 2, p = 1): KoopmanSplineRegressor(1, state_bounds) over 16 values of gamma
(10**arange(-6, -2, 0.25)) x m = 500 x 5 folds = 80 units, run as one lock-step batched call (nk_spline_cv_grid).  The centres
are drawn from the global NumPy RNG in GridSearchCV's order after np.random.seed(1).  Needs an MI355X (the library has no
CPU path):

    python3 examples/duffing_spline_cv.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from nys_koop_lqr_amd import harness

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
g = np.load(os.path.join(G, "f13_duffing_cv.npz"))
X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])    # [x | u] -> x'
state_bounds = np.array([1.0, 2])                                    # radius_sampling, angle_sampling of the Duffing plant
candidates = [dict(gamma=float(gm), m=500, state_bounds_params=state_bounds) for gm in np.power(10.0, np.arange(-6, -2, 0.25))]

np.random.seed(1)
t0 = time.perf_counter()
res = harness.grid_search_cv(X, Y, 1, candidates, n_splits=5, batch=32, batch_groups=2, estimator="spline")
dt = time.perf_counter() - t0
print(f"{res['split_scores'].size} units in {dt:.2f} s (first call: pools and workspaces are created)")
for c, mean in zip(candidates, res["mean_test_score"]):
    print(f"  gamma {c['gamma']:.3e}: mean neg-RMSE {mean:.6e}")
print(f"best gamma: {res['best_params']['gamma']:.3e}")
