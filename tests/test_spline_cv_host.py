"""The spline hyper-parameter sweep without a GPU: the centre draws in GridSearchCV's order against the centres the
reference drew (tests/golden/make_golden_spline_cv.py -> f16_spline_cv.npz), the ranking of the recorded scores, the new
entry point in the header, the library and the binding, and the unit lists harness.grid_search_cv hands to the lock-step
pool for either estimator."""
import os

import numpy as np
import pytest

from nys_koop_lqr_amd import _lib, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def duffing_cv_data(golden):
    g = golden("f13_duffing_cv.npz")
    return np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])


def candidates_of(g, tag):
    bounds = g["bounds"] if tag == "big" else None
    return [dict(gamma=float(gm), m=int(g[f"{tag}_m"]), state_bounds_params=bounds) for gm in g[f"{tag}_gammas"]]


def test_centre_draws_follow_gridsearchcv(golden):
    """np.random.seed(1), then one draw per (candidate, fold) unit, candidate-major, from the training states of the fold:
    bit for bit the centres the reference's cloned estimators drew under GridSearchCV(n_jobs=1)."""
    g = golden("f16_spline_cv.npz")
    X, _ = duffing_cv_data(golden)
    folds = harness.kfold_slices(X.shape[0], 5)
    for tag in ("big", "small"):
        cands = candidates_of(g, tag)
        rec = g[f"{tag}_centers"]
        assert rec.shape == (len(cands), 5, 2, cands[0]["m"])
        np.random.seed(int(g["seed"]))
        for c, f in harness.cv_work_list(len(cands), 5):
            lo, hi = folds[f]
            z = harness.spline_centers_draw(cands[c], np.vstack((X[:lo, :2], X[hi:, :2])))
            assert np.array_equal(z, rec[c, f]), (tag, c, f)


def test_centre_draw_from_a_private_rng_leaves_the_global_one_alone():
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    S = np.random.default_rng(0).standard_normal((30, 2))
    z = harness.spline_centers_draw(dict(gamma=1e-3, m=7), S, rng=np.random.RandomState(3))
    assert z.shape == (2, 7) and np.array_equal(np.random.get_state()[1], before)
    idx = np.random.RandomState(3).choice(np.arange(0, 30), size=7, replace=False)
    assert np.array_equal(z, S[idx].T)


def test_ranking_of_the_recorded_scores(golden):
    g = golden("f16_spline_cv.npz")
    for tag in ("big", "small"):
        mean, best = harness._rank_candidates(g[f"{tag}_split_scores"])
        np.testing.assert_allclose(mean, g[f"{tag}_mean_test_score"], rtol=1e-14, atol=0)
        assert best == int(np.argmax(g[f"{tag}_mean_test_score"]))
        assert np.all(np.isfinite(g[f"{tag}_split_scores"]))  # the reference leaves no unit out
        assert np.all(g[f"{tag}_bar"] >= float(g["bar_floor"]))
        np.testing.assert_array_equal(g[f"{tag}_bar"], np.maximum(float(g["bar_factor"]) * g[f"{tag}_movement"],
                                                                  float(g["bar_floor"])))


def test_abi_declares_and_exports_the_spline_sweep():
    assert "nk_spline_cv_grid" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "nyskoop.h")) as f:
        header = f.read()
    assert "int nk_spline_cv_grid(" in header and "} nk_spline_cv_unit;" in header
    assert "#define NK_ABI_VERSION 2" in header
    assert hasattr(_lib.load_library(), "nk_spline_cv_grid")
    fields = [name for name, _ in _lib.SplineCvUnit._fields_]
    assert fields == ["gamma", "m", "reserved", "test_begin", "test_end", "centers"]
    import ctypes as C
    assert C.sizeof(_lib.SplineCvUnit) == 40


class StubPool:
    def __init__(self):
        self.calls = []

    def cv_grid(self, X, Y, n_inputs, units):
        self.calls.append(("nystrom", list(units)))
        return np.zeros(len(units)), np.zeros(len(units), dtype=np.int32)

    def spline_cv_grid(self, X, Y, n_inputs, units):
        self.calls.append(("spline", list(units)))
        return -np.arange(1.0, len(units) + 1), np.zeros(len(units), dtype=np.int32)


def test_default_estimator_hands_the_same_units_to_the_pool(monkeypatch):
    import nys_koop_lqr_amd as nk
    rng = np.random.default_rng(2)
    n, d, p, m = 100, 3, 1, 8
    X, Y = rng.standard_normal((n, d + p)), rng.standard_normal((n, d))
    cands = [dict(kernel=nk.ThreeDimensionalKernel(2.0, 2.0, 2.0, d), gamma=gm, m=m) for gm in (1e-4, 1e-3)]
    pool = StubPool()
    monkeypatch.setattr(_lib, "lockstep_pool", lambda size, device=None, index=0: pool)
    np.random.seed(9)
    harness.grid_search_cv(X, Y, p, cands, batch=4)
    np.random.seed(9)
    harness.grid_search_cv(X, Y, p, cands, batch=4, estimator="nystrom")
    (k0, u0), (k1, u1) = pool.calls
    assert k0 == k1 == "nystrom" and len(u0) == len(u1) == 10
    for a, b in zip(u0, u1):
        assert a[0] is b[0] and a[1:5] == b[1:5] and np.array_equal(a[5], b[5])
    with pytest.raises(ValueError):
        harness.grid_search_cv(X, Y, p, cands, batch=4, estimator="splines")


def test_spline_estimator_hands_centres_folds_and_gammas_to_the_pool(golden, monkeypatch):
    g = golden("f16_spline_cv.npz")
    X, Y = duffing_cv_data(golden)
    cands = candidates_of(g, "small")
    pool = StubPool()
    monkeypatch.setattr(_lib, "lockstep_pool", lambda size, device=None, index=0: pool)
    np.random.seed(int(g["seed"]))
    res = harness.grid_search_cv(X, Y, 1, cands, batch=8, estimator="spline")
    (kind, units), = pool.calls
    assert kind == "spline" and len(units) == 20
    folds = harness.kfold_slices(X.shape[0], 5)
    for k, (c, f) in enumerate(harness.cv_work_list(len(cands), 5)):
        gamma, m, fold, Z = units[k]
        assert gamma == cands[c]["gamma"] and m == 50 and tuple(fold) == folds[f]
        assert Z.shape == (50, 2) and Z.flags["C_CONTIGUOUS"] and np.array_equal(Z, g["small_centers"][c, f].T)
    assert np.array_equal(res["split_scores"], -np.arange(1.0, 21).reshape(4, 5))
    # centres given by the caller are used as they are, and nothing is drawn
    pool.calls.clear()
    state = np.random.get_state()[1].copy()
    centers = {(c, f): g["small_centers"][c, f] for c in range(4) for f in range(5)}
    harness.grid_search_cv(X, Y, 1, cands, batch=8, centers=centers, estimator="spline")
    assert np.array_equal(np.random.get_state()[1], state)
    assert all(np.array_equal(u[3], g["small_centers"][k // 5, k % 5].T) for k, u in enumerate(pool.calls[0][1]))
