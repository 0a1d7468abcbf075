"""CPU: the NumPy reference of the landmark selection (tests/landmark_reference.py) has the properties the device code is
held to -- its factor reproduces K on the selected columns, traces fall, the greedy selection is nested, exact ties go to
the lowest position -- and the host plumbing around the device call: harness.landmark_centers with a stand-in for the
device, the estimator's attributes, and the C-ABI symbol in header and library."""
import os
import pickle

import numpy as np
import pytest

import landmark_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATERN = dict(kind="matern52", length_scale=0.5)
CASES = [(300, 1, 16, MATERN), (257, 2, 24, MATERN), (257, 2, 24, dict(kind="rbf", length_scale=0.3)),
         (120, 40, 24, dict(kind="linear", sigma0=0.5)), (200, 6, 30, dict(kind="rbf", length_scale=[1.0, 10.0, 100.0] * 2))]


def _data(n, d, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, d))


@pytest.mark.parametrize("rule", ["greedy", "rpcholesky"])
@pytest.mark.parametrize("n,d,m,kernel", CASES)
def test_factor_reproduces_the_selected_columns_and_traces_fall(n, d, m, kernel, rule):
    Y = _data(n, d)
    u = np.random.default_rng(7).uniform(size=m)
    for dtype in (np.float64, np.longdouble):
        r = lr.pchol(Y, kernel, m, rule=rule, u=u, dtype=dtype)
        assert r["m_selected"] == m and len(set(r["pivots"].tolist())) == m
        K = lr.kernel_matrix(Y, kernel, dtype=dtype)
        piv = r["pivots"]
        scale = float(np.abs(K).max())
        assert float(np.abs(r["F"] @ r["F"][piv].T - K[:, piv]).max()) <= 1e-12 * scale
        assert np.all(np.diff(r["trace"]) < 0) and r["trace"].shape == (m + 1,)
        # the trace left is the trace of the Nystrom residual K - K_nm K_mm^-1 K_mn
        left = float(np.trace(K) - np.trace(r["F"] @ r["F"].T))
        assert abs(left - float(r["trace"][-1])) <= 1e-10 * scale * n
        # replaying the pivots gives the same residuals
        rp = lr.replay(Y, kernel, piv, dtype=dtype)
        assert np.array_equal(rp["resid"], r["resid"]) and np.array_equal(rp["trace"], r["trace"])
        if rule == "greedy":
            assert np.array_equal(rp["dgmax"], rp["resid"])
        else:
            assert np.all(rp["cum_lo"] <= u * r["trace"][:m]) and np.all(u * r["trace"][:m] < rp["cum_hi"])


@pytest.mark.parametrize("n,d,m,kernel", CASES)
def test_greedy_selection_is_nested(n, d, m, kernel):
    Y = _data(n, d, seed=1)
    a, b = lr.pchol(Y, kernel, m), lr.pchol(Y, kernel, 2 * m)
    assert np.array_equal(b["pivots"][:m], a["pivots"])
    assert np.array_equal(b["resid"][:m], a["resid"])


def test_exact_ties_go_to_the_lowest_position():
    Y = 2.0 * np.eye(600)
    r = lr.pchol(Y, dict(kind="linear", sigma0=0.0), 10)
    assert r["pivots"].tolist() == list(range(10))
    assert np.all(r["resid"] == 4.0) and r["trace"].tolist() == [4.0 * (600 - j) for j in range(11)]
    pos = np.r_[300:600, 0:300]
    r = lr.pchol(Y, dict(kind="linear", sigma0=0.0), 10, positions=pos)
    assert pos[r["pivots"]].tolist() == list(range(300, 310))


def test_stop_rule_and_zero_residuals_are_never_picked():
    pts = _data(7, 2, seed=3)
    Y = pts[np.arange(500) % 7]
    for rule in ("greedy", "rpcholesky"):
        r = lr.pchol(Y, MATERN, 20, rule=rule, u=np.random.default_rng(5).uniform(size=20), tol=1e-8)
        assert r["m_selected"] == 7 and len(r["resid"]) == 8 and len(r["trace"]) == 8
        assert len({tuple(Y[i]) for i in r["pivots"]}) == 7
        assert r["trace"][-1] <= 500 * 1e-8


def test_landmark_centers_with_a_stand_in_for_the_device():
    from nys_koop_lqr_amd import harness
    Y = _data(90, 2, seed=4)
    calls = []

    def select(Y_, kernel, m, rule="greedy", row_ranges=None, tol=0.0, u=None):
        calls.append((m, rule, None if row_ranges is None else np.asarray(row_ranges).tolist(), None if u is None else u.copy()))
        pos = None if row_ranges is None else harness.train_row_map(row_ranges, len(Y_))
        r = lr.pchol(Y_, kernel, m, rule=rule, u=u, tol=tol, positions=pos)
        return r["pivots"] if pos is None else pos[r["pivots"]]  # rows of Y, like select_landmarks

    ms, seeds = (4, 8, 16), [3, 5]
    ranges = {3: [(40, 90), (0, 20)], 5: [(40, 90), (0, 20)]}
    test_index = {3: [0, 1], 5: [2]}
    cen = harness.landmark_centers(Y, MATERN, ms, seeds, test_index, train_ranges=ranges, select_fn=select)
    assert sorted(cen) == sorted([(3, 0, k) for k in range(3)] + [(3, 1, k) for k in range(3)] + [(5, 0, k) for k in range(3)])
    assert len(calls) == 1 and calls[0][0] == 16  # one selection of max(ms) for the one distinct training-row set
    rowmap = harness.train_row_map(ranges[3], 90)
    want = lr.pchol(Y, MATERN, 16, positions=rowmap)["pivots"]
    for (seed, ti, k), idx in cen.items():
        assert idx.shape == (ms[k],) and idx.dtype == np.int64
        assert np.array_equal(idx, want[:ms[k]])  # training-row numbering = candidate positions; every m a prefix
    # sysid_plan accepts the dictionary and maps the indices to data-set rows
    units = harness.sysid_plan(np.zeros((90, 3)), Y, 1, {}, ms, seeds, test_index, train_ranges=ranges, centers=cen)
    assert len(units) == 9 and all(np.array_equal(u["marks"], rowmap[want[:u["m"]]]) for u in units)
    # RPCholesky: one selection per seed, u drawn from RandomState(seed)
    calls.clear()
    cen = harness.landmark_centers(Y, MATERN, ms, seeds, test_index, rule="rpcholesky", select_fn=select)
    assert [c[1] for c in calls] == ["rpcholesky"] * 2 and all(c[2] is None for c in calls)
    for c, seed in zip(calls, seeds):
        assert np.array_equal(c[3], np.random.RandomState(seed).uniform(size=16))
    assert not np.array_equal(cen[(3, 0, 2)], cen[(5, 0, 2)])
    # a tolerance that stops the selection early cannot serve the schedule
    with pytest.raises(ValueError, match="stopped after"):
        harness.landmark_centers(Y[np.arange(90) % 5], MATERN, ms, seeds, test_index, tol=1e-8, select_fn=select)


def test_estimator_attributes_follow_compute_dtype():
    from sklearn.base import clone
    import nys_koop_lqr_amd as nk
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([0.5, 0.5]), gamma=1e-6, m=8)
    assert reg.landmark_rule == "uniform" and reg.landmark_tol == 0.0
    assert set(reg.get_params()) == {"n_inputs", "kernel", "gamma", "m"}
    reg.landmark_rule, reg.landmark_tol = "greedy", 1e-10
    assert clone(reg).landmark_rule == "uniform" and clone(reg).landmark_tol == 0.0
    r2 = pickle.loads(pickle.dumps(reg))
    assert r2.landmark_rule == "greedy" and r2.landmark_tol == 1e-10
    with pytest.raises(ValueError, match="rule must be one of"):
        nk.select_landmarks(np.zeros((4, 2)), nk.KernelWrapper([0.5, 0.5]), 2, rule="nearest")


def test_header_declares_and_library_exports_the_entry():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    assert "int nk_select_landmarks(nk_ctx* ctx, const nk_kernel_desc* kd" in header
    assert "#define NK_LANDMARK_GREEDY 0" in header and "#define NK_LANDMARK_RPCHOLESKY 1" in header
    assert "#define NK_ABI_VERSION 2" in header
    lib = _lib.load_library()
    assert "nk_select_landmarks" in _lib.SIGNATURES and hasattr(lib, "nk_select_landmarks")
    assert (_lib.NK_LANDMARK_GREEDY, _lib.NK_LANDMARK_RPCHOLESKY) == (0, 1)
