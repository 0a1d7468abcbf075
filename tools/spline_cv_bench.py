"""Throughput of the spline hyper-parameter sweep (benchmark_lqr_classic.py:55-60) with and without lock-step batching, at
the reference's shape: n = 3980, d = 2, p = 1, m = 500, 16 gammas 10**arange(-6, -2, 0.25) x 5 folds = 80 units; inputs
generated like those of tools/lockstep_bench.py.  Same process, same inputs: one warm-up sweep, then the median of 5 sweeps,
unbatched (batch=0: per unit exactly the launches of nk_spline_fit + nk_score_neg_rmse on an ordinary context) and batched
(batch=32, batch_groups=2), and -- to separate what the merged launches give from what leaving Python gives -- the same
units through nk_spline_cv_grid on a group of ONE member (one C call, nothing to merge with).  Reports units/s for the
three, the spread (max - min of the 5 sweeps over their median), the share of units that took the pseudo-inverse, whether
the scores are bit-identical, and writes profiles/spline_cv_bench.json.

    python tools/spline_cv_bench.py [--sweeps 5] [--batch 32] [--groups 2] [--out profiles/spline_cv_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import nys_koop_lqr_amd as nk  # noqa: E402
from nys_koop_lqr_amd import harness, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=5)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--groups", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spline_cv_bench.json"))
args = ap.parse_args()

rng = np.random.default_rng(0)
n, d, p, m = 3980, 2, 1, 500
S = rng.standard_normal((n, d)); U = rng.standard_normal((n, p))
Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
X = np.hstack([S, U])
gammas = np.power(10.0, np.arange(-6, -2, 0.25))
cands = [dict(gamma=float(g), m=m) for g in gammas]
folds = harness.kfold_slices(n, 5)
centers = {}
for c in range(len(cands)):  # centres = training states of the unit's fold (regressors.py:195-197), one fixed draw per unit
    for f, (lo, hi) in enumerate(folds):
        centers[(c, f)] = harness.spline_centers_draw(cands[c], np.vstack((S[:lo], S[hi:])), rng=np.random.RandomState(17 * c + f))
n_units = len(centers)

# which side of SPLINE_SVD_WINDOW each unit falls on (nk_fit.hip: pseudo-inverse unless the smallest / largest Cholesky
# pivot exceeds 2 (m+p)^2 eps), read from the statistics of one ordinary fit per unit
pinv_units = 0
for (c, f), Z in centers.items():
    lo, hi = folds[f]
    reg = nk.KoopmanSplineRegressor(p, m=m, gamma=cands[c]["gamma"])
    reg.centers = Z
    reg.fit(X, Y, row_ranges=[(0, lo), (hi, n)], fetch=False)
    st = reg.fit_stats_
    pinv_units += not (st["pivot_ratio_inner"] > 2.0 * (m + p) ** 2 * np.finfo(float).eps)


def timed(**kw):
    harness.grid_search_cv(X, Y, p, cands, centers=centers, estimator="spline", **kw)  # warm-up (workspaces, streams)
    ts, res = [], None
    for _ in range(args.sweeps):
        t0 = time.perf_counter()
        res = harness.grid_search_cv(X, Y, p, cands, centers=centers, estimator="spline", **kw)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts)
    med = float(np.median(ts))
    return res, dict(seconds=[float(t) for t in ts], median_s=med, units_per_s=n_units / med,
                     spread=float((ts.max() - ts.min()) / med))


def timed_one_member():
    """the 80 units in one nk_spline_cv_grid call on a one-member group: no Python per unit, no launch shared"""
    pool = _lib.lockstep_pool(1, index=9)
    units = [(cands[c]["gamma"], m, folds[f], np.ascontiguousarray(centers[(c, f)].T)) for c, f in harness.cv_work_list(len(cands), 5)]
    pool.spline_cv_grid(X, Y, p, units)
    ts, sc = [], None
    for _ in range(args.sweeps):
        t0 = time.perf_counter()
        sc, status = pool.spline_cv_grid(X, Y, p, units)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts)
    med = float(np.median(ts))
    return sc.reshape(len(cands), 5), dict(seconds=[float(t) for t in ts], median_s=med, units_per_s=n_units / med,
                                           spread=float((ts.max() - ts.min()) / med))


base, r0 = timed()
sc1, r_one = timed_one_member()
res, r1 = timed(batch=args.batch, batch_groups=args.groups)
stats = [_lib.lockstep_pool(args.batch, index=gi).stats() for gi in range(args.groups)]
out = dict(shape=dict(n=n, d=d, p=p, m=m, gammas=len(gammas), folds=5, units=n_units), sweeps=args.sweeps,
           unbatched=r0, one_member_call=dict(bit_identical=bool(np.array_equal(sc1, base["split_scores"])), **r_one),
           batched=dict(batch=args.batch, batch_groups=args.groups, **r1),
           speedup=r1["units_per_s"] / r0["units_per_s"], pinv_units=int(pinv_units), pinv_share=pinv_units / n_units,
           bit_identical=bool(np.array_equal(res["split_scores"], base["split_scores"])),
           best_index=int(res["best_index"]), group_stats=stats, runtime_counters=_lib.runtime_counters())
print(f"unbatched: {r0['units_per_s']:.0f} units/s (median {r0['median_s']:.3f} s, spread {r0['spread']:.1%})")
print(f"one-member group, one call: {r_one['units_per_s']:.0f} units/s (median {r_one['median_s']:.3f} s, spread {r_one['spread']:.1%})")
print(f"batch {args.batch} x {args.groups} groups: {r1['units_per_s']:.0f} units/s (median {r1['median_s']:.3f} s, "
      f"spread {r1['spread']:.1%}); x{out['speedup']:.2f}; pseudo-inverse units {pinv_units}/{n_units}; "
      f"bit-identical scores: {out['bit_identical']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
