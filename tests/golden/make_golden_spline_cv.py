#!/usr/bin/env python3
"""Golden vectors for the spline branch of learn_hyperparams (benchmark_lqr_classic.py:54-60), produced by RUNNING THE
REFERENCE in the build container: scikit-learn's real GridSearchCV (n_jobs = 1, so that the centre draws from the global
legacy RNG come in a reproducible order) over the reference's KoopmanSplineRegressor.  Only DATA is written, and the data
set itself is not duplicated: it is X, Y of f13_duffing_cv.npz (make_golden_cv.duffing_dataset after np.random.seed(0),
n = 3980, d = 2, p = 1; checked below).

  f16_spline_cv.npz
    big_*    GridSearchCV(KoopmanSplineRegressor(1, [1.0, 2]), {"gamma": 10**arange(-6, -2, 0.25), "m": [500]}) after
             np.random.seed(1): 16 candidates x 5 folds = 80 units, centres drawn from the state bounds
             (regressors.py:189-193)
    small_*  the same with state_bounds_params = None (centres = columns of the training states, :195-197), m = 50 and
             the gammas 1e-6, 1e-5, 1e-4, 1e-3: 20 units
  per search: split_scores (candidates x folds), mean_test_score, gammas, m, centers (candidates x folds x d x m: what
  compute_centers returned for the unit, recorded by wrapping it; the draw of GridSearchCV's final refit is dropped),
  and per unit the reference's own reproducibility as make_golden_spline.py measures it for the f15 fixtures:
  movement = max(|score(inputs perturbed by one part in 1e15) - score|, |score(pinv through gesvd) - score|) / |score|,
  bar = max(BAR_FACTOR * movement, BAR_FLOOR_RMSE) with make_golden_spline's constants.

    python tests/golden/make_golden_spline_cv.py
"""
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden_cv as MC  # noqa: E402  (imports the reference)
import make_golden_duffing as MD  # noqa: E402
from make_golden_spline import BAR_FACTOR, BAR_FLOOR_RMSE, BOUNDS, Gesvd, fit_with  # noqa: E402

R = MC.R
from sklearn.model_selection import GridSearchCV, KFold  # noqa: E402

SMALL_GAMMAS = np.array([1e-6, 1e-5, 1e-4, 1e-3])


def neg_rmse(reg, X, Y):
    """sklearn's 'neg_root_mean_squared_error' (uniform average over the output columns)."""
    return -float(np.mean(np.sqrt(np.mean(np.square(Y - reg.predict(X)), axis=0))))


def search(X, Y, bounds, gammas, m):
    """split scores of GridSearchCV in its candidate order and the centres every unit drew"""
    drawn = []
    orig = R.KoopmanSplineRegressor.compute_centers

    def spy(self, Xs):
        c = orig(self, Xs)
        drawn.append(np.array(c))
        return c

    R.KoopmanSplineRegressor.compute_centers = spy
    try:
        np.random.seed(1)
        clf = GridSearchCV(R.KoopmanSplineRegressor(1, bounds), {"gamma": gammas, "m": [m]},
                           scoring="neg_root_mean_squared_error", n_jobs=1)
        clf.fit(X, Y)
    finally:
        R.KoopmanSplineRegressor.compute_centers = orig
    res = clf.cv_results_
    sc = np.stack([res[f"split{f}_test_score"] for f in range(5)], axis=1)
    og = np.array([p["gamma"] for p in res["params"]])
    assert np.array_equal(og, gammas) and len(drawn) == sc.size + 1  # (+ 1: the refit of the best candidate)
    centers = np.array(drawn[:sc.size]).reshape(sc.shape + drawn[0].shape)  # unit (c, f) = draw number 5 c + f
    return sc, res["mean_test_score"], centers


def with_bars(tag, X, Y, bounds, gammas, m):
    t0 = time.time()
    sc, mean, centers = search(X, Y, bounds, gammas, m)
    assert np.all(np.isfinite(sc)), "the reference left a unit out (NaN score)"
    rng = np.random.default_rng(7)
    Xp = X * (1 + 1e-15 * rng.standard_normal(X.shape))
    Yp = Y * (1 + 1e-15 * rng.standard_normal(Y.shape))
    move = np.zeros_like(sc)
    for c, gamma in enumerate(gammas):
        for f, (tr, te) in enumerate(KFold(5).split(X)):
            z = centers[c, f]
            base = neg_rmse(fit_with(z, m, gamma, X[tr], Y[tr], bounds), X[te], Y[te])
            assert abs(base - sc[c, f]) <= 1e-12 * abs(sc[c, f]), (c, f, base, sc[c, f])  # the recorded centres are the unit's
            pert = neg_rmse(fit_with(z, m, gamma, Xp[tr], Yp[tr], bounds), Xp[te], Yp[te])
            with Gesvd():
                gesvd = neg_rmse(fit_with(z, m, gamma, X[tr], Y[tr], bounds), X[te], Y[te])
            move[c, f] = max(abs(pert - base), abs(gesvd - base)) / abs(base)
    print(f"{tag}: {sc.size} units in {time.time() - t0:.0f} s; best candidate {int(np.argmax(mean))} "
          f"(gamma {gammas[int(np.argmax(mean))]:.3g}); movement of the reference's scores: median {np.median(move):.2e}, "
          f"max {move.max():.2e} (unit {np.unravel_index(np.argmax(move), move.shape)})", flush=True)
    return {f"{tag}_split_scores": sc, f"{tag}_mean_test_score": mean, f"{tag}_centers": centers, f"{tag}_gammas": gammas,
            f"{tag}_m": m, f"{tag}_movement": move, f"{tag}_bar": np.maximum(BAR_FACTOR * move, BAR_FLOOR_RMSE)}


if __name__ == "__main__":
    ds = MD.duffing_plant()
    np.random.seed(0)
    X, Y = MC.duffing_dataset(ds, 20, int(2 // ds.Ts))
    f13 = np.load(f"{OUT}/f13_duffing_cv.npz")
    assert np.array_equal(X, f13["X"]) and np.array_equal(Y, f13["Y"])
    out = dict(seed=1, bounds=BOUNDS, bar_factor=BAR_FACTOR, bar_floor=BAR_FLOOR_RMSE)
    out.update(with_bars("big", X, Y, BOUNDS, MC.GAMMAS, 500))
    out.update(with_bars("small", X, Y, None, SMALL_GAMMAS, 50))
    np.savez_compressed(f"{OUT}/f16_spline_cv.npz", **out)
    print(f"f16_spline_cv.npz: {os.path.getsize(f'{OUT}/f16_spline_cv.npz')} bytes")
