"""Thin-plate-spline EDMD fits (KoopmanSplineRegressor.fit -> nk_spline_fit): fits/s and the stage times of nk_fit_stats at
three shapes, inputs and centres host arrays as the reference's drivers pass them.

    python3 tools/spline_bench.py [reps]

  duffing   n = 69 900, d = 2, p = 1, m = 200, gamma = 1e-6 (benchmark_lqr_classic.py; f12_duffing_full.npz, disc centres)
  cloth     n = 3 030, d = 192, p = 6, m = 500, gamma = 1e-5 (seed-0 split of benchmark_lqr_cloth.py; data centres)
  headline  n = 1e5, d = 384, p = 6, m = 2000, gamma = 1e-6 (the Nystrom headline's Gram volume; synthetic rows of bench.py)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nys_koop_lqr_amd as nk  # noqa: E402
import bench  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def duffing():
    g = np.load(os.path.join(GOLDEN, "f12_duffing_full.npz"))
    X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])
    np.random.seed(0)
    reg = nk.KoopmanSplineRegressor(1, state_bounds_params=np.array([1.0, 2]), m=200, gamma=1e-6)
    return reg, X, Y


def cloth():
    g = np.load(os.path.join(GOLDEN, "f15_spline_cloth.npz"))
    t = np.load(os.path.join(GOLDEN, "cloth_trajs_all.npz"))
    states, inputs = t["states_e10"] / 1e10, t["inputs"]
    X = np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in g["train"]]).T.copy()
    Y = np.hstack([states[i][:, 1:] for i in g["train"]]).T.copy()
    np.random.seed(0)
    reg = nk.KoopmanSplineRegressor(6, m=500, gamma=1e-5)
    return reg, X, Y


def headline():
    n, m, d, p = 100000, 2000, 384, 6
    X, Y, idx = bench.make_c4(n, d, p, m)
    reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
    reg.centers = np.ascontiguousarray(Y[idx].T)
    return reg, X, Y


def run(name, make, reps):
    reg, X, Y = make()
    reg.fit(X, Y)  # draws the centres (kept by the later fits), warms the workspace
    _ = reg.A
    times, stats = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        reg.fit(X, Y)
        _ = reg.weights  # the operators are on the host
        times.append(time.perf_counter() - t0)
        stats.append(reg.fit_stats_)
    med = float(np.median(times))
    keys = ("ms_total", "ms_upload", "ms_kmat", "ms_gram", "ms_solve", "ms_gram_kernel_avg")
    st = {k: float(np.median([s[k] for s in stats])) for k in keys}
    out = dict(shape=name, n=int(X.shape[0]), d=int(Y.shape[1]), p=int(X.shape[1] - Y.shape[1]),
               m=int(np.asarray(reg.centers).shape[1]), reps=reps, ms_per_fit_wall=med * 1e3, fits_per_s=1.0 / med,
               rank_kept=int(stats[-1]["rank_inner"]), pivot_ratio=float(stats[-1]["pivot_ratio_inner"]),
               gram_launches=int(stats[-1]["gram_kernel_launches"]), **st)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for name, make in (("duffing", duffing), ("cloth", cloth), ("headline", headline)):
        run(name, make, reps)
