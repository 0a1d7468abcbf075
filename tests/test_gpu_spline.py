"""KoopmanSplineRegressor on the MI355X against the reference's own outputs (tests/golden/make_golden_spline.py): the
thin-plate-spline kernel matrices in both kernel-matrix modes, the operators, predictions and rollout errors of the
Duffing and cloth fits within the stored bars (a fixed multiple of the reference's own spread), the four shipped Duffing
rows replayed through the HIP path, the rank the pseudo-inverse keeps, and the device-model surface."""
import ctypes as C
import pickle

import numpy as np
import pytest

from conftest import relf
from spline_fit_reference import tps_bar_direct, tps_bar_gram

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


def tps_matrix(A, B, mode):
    from nys_koop_lqr_amd import _lib
    ctx = _lib.get_context()
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    d = A.shape[1]
    kd = _lib.KernelDesc(_lib.NK_KERNEL_TPS, d, 0, 0, None, 0.0)
    out = np.empty((A.shape[0], B.shape[0]))
    ctx.set_kmat_mode(mode)
    try:
        _lib.check(ctx.lib.nk_kernel_matrix(ctx.handle, C.byref(kd), A.ctypes.data, d, A.shape[0], B.ctypes.data, d,
                                            B.shape[0], out.ctypes.data, B.shape[0]))
    finally:
        ctx.set_kmat_mode(0)
    return out


def duffing_XY(golden):
    g = golden("f12_duffing_full.npz")
    return np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])


def cloth_data(golden):
    g = golden("f15_spline_cloth.npz")
    t = golden("cloth_trajs_all.npz")
    states, inputs = t["states_e10"] / 1e10, t["inputs"]
    X = np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in g["train"]]).T.copy()
    Y = np.hstack([states[i][:, 1:] for i in g["train"]]).T.copy()
    test = int(g["test"][0])
    return g, X, Y, states[test], inputs[test]


def rel_rmse(reg, traj, ctrl):
    from nys_koop_lqr_amd.harness import validate_dyn_sys
    return validate_dyn_sys(reg, traj, ctrl, relative=True)


# ---------------------------------------------------------------------------------------------------- kernel matrices
@pytest.mark.parametrize("case", ["d2", "d192"])
def test_tps_kernel_matrix_direct_exact_zeros(nk, golden, case):
    g = golden("f15_spline_tps.npz")
    P, Z, K = g[f"{case}_points"], g[f"{case}_centers"], g[f"{case}_K"]
    out = tps_matrix(P, Z, 1)
    zero = K == 0.0
    assert zero.sum() >= 10
    assert np.all(out[zero] == 0.0)  # coincident points: exactly 0, like the reference's nan_to_num
    # log within 1 ulp (nk_common.h), r^2 summed in another order than NumPy: a few ulp of r^2 |log r|
    # (spline_fit_reference.tps_bar_direct with u = EPS; K is NumPy's own float64 value, so the term for the kernel function's
    # arithmetic is left out, as it always was here)
    r2 = np.sum((P[:, None, :] - Z[None, :, :]) ** 2, axis=2)
    bar = tps_bar_direct(P.shape[1], r2, np.zeros_like(K), u=EPS)
    assert np.all(np.abs(out - K) <= bar), float(np.max(np.abs(out - K) - bar))


def test_tps_kernel_matrix_gram_form(nk, golden):
    """Gram form (automatic mode at d >= 32) against the direct differences, entry by entry: r^2 = |a|^2 + |b|^2 - 2 a.b
    of rows centred on the mean of the centres carries an error delta <= (d + 8) eps (|a|^2 + |b|^2); the spline
    r^2 log(r) / 1 moves by at most delta (|log max(r^2, delta)| / 2 + 1)."""
    g = golden("f15_spline_tps.npz")
    P, Z = g["d192_points"], g["d192_centers"]
    direct = tps_matrix(P, Z, 1)
    gram = tps_matrix(P, Z, 0)
    r2 = np.sum((P[:, None, :] - Z[None, :, :]) ** 2, axis=2)
    bar = tps_bar_gram(P, Z, Z.mean(axis=0), r2, direct, u=EPS)
    assert np.all(np.abs(gram - direct) <= bar), float(np.max(np.abs(gram - direct) / bar))


# ---------------------------------------------------------------------------------------------------- Duffing
def test_duffing_operators_seed0(nk, golden):
    g = golden("f15_spline_duffing.npz")
    X, Y = duffing_XY(golden)
    ms = list(g["ms"])
    cols = g["centers_0"]
    for m in (10, 48, 200):
        k = ms.index(m)
        o = int(np.sum(g["ms"][:k]))
        reg = nk.KoopmanSplineRegressor(1, state_bounds_params=g["bounds"], m=m, gamma=float(g["gamma"]))
        reg.centers = cols[:, o:o + m]
        reg.fit(X, Y)
        bar = float(g["bar_ops"][k])
        errs = dict(A=relf(reg.A, g[f"A_{m}"]), B=relf(reg.B, g[f"B_{m}"]), C=relf(reg.C, g[f"C_{m}"]))
        assert max(errs.values()) <= bar, (m, errs, bar)
        st = reg.fit_stats_
        assert st["rank_inner"] == m + 1 and st["rank_inner_rec"] == 0
        np.testing.assert_allclose(reg.weights, reg.C @ np.hstack((reg.A, reg.B)), rtol=1e-10, atol=1e-12 * np.abs(reg.weights).max())


def test_duffing_shipped_rows_replayed(nk, golden):
    """The four rows of the authors' duffing/all_rmses_splines_double_dataset.csv (80 fits): np.random.seed(seed) -> test
    trajectory -> 20 sequential fits whose centres the estimator draws itself; each relative-% RMSE within the stored bar
    of the reference's own value, and the reference's value against the shipped one as the fixture recorded it."""
    import random
    g = golden("f15_spline_duffing.npz")
    X, Y = duffing_XY(golden)
    for si, seed in enumerate(g["seeds"]):
        seed = int(seed)
        traj, ctrl = g[f"traj_{seed}"], g[f"ctrl_{seed}"]
        np.random.seed(seed); random.seed(seed)
        o = 0
        for k, m in enumerate(g["ms"]):
            m = int(m)
            reg = nk.KoopmanSplineRegressor(1, state_bounds_params=g["bounds"], m=m, gamma=float(g["gamma"]))
            reg.fit(X, Y)
            np.testing.assert_array_equal(reg.centers, g[f"centers_{seed}"][:, o:o + m])
            o += m
            r = rel_rmse(reg, traj, ctrl)
            ref = g["ref_rmse"][si, k]
            assert abs(r - ref) / ref <= g["bar_rmse"][si, k], (seed, m, r, ref, g["bar_rmse"][si, k])
            shipped = g["shipped_rows"][si, k]
            assert abs(r - shipped) / shipped <= 2e-5 + g["bar_rmse"][si, k], (seed, m, r, shipped)


# ---------------------------------------------------------------------------------------------------- cloth
@pytest.mark.parametrize("k", range(6))
def test_cloth_cases(nk, golden, k):
    g, X, Y, traj, ctrl = cloth_data(golden)
    m, gamma = int(g["ms"][k]), float(g["gammas"][k])
    reg = nk.KoopmanSplineRegressor(6, m=m, gamma=gamma)
    reg.centers = X[:, :192].T[:, g[f"c{k}_centers_idx"]]
    reg.fit(X, Y)
    st = reg.fit_stats_
    golden_rank = int(g[f"c{k}_rank"])
    if golden_rank < m + 6:
        assert st["rank_inner"] == golden_rank, (st["rank_inner"], golden_rank)
    else:
        assert st["rank_inner"] == m + 6
    Xq = np.vstack((traj[:, :-1], ctrl[:, :-1])).T[: int(g["n_predict"])]
    PA = np.random.default_rng(int(g["probe_seeds"][0])).standard_normal((m, 4))
    PC = np.random.default_rng(int(g["probe_seeds"][1])).standard_normal((m, 4))
    from nys_koop_lqr_amd.harness import validate_dyn_sys
    errs = dict(predict=relf(reg.predict(Xq), g[f"c{k}_predict"]), A=relf(reg.A @ PA, g[f"c{k}_A_probe"]),
                C=relf(reg.C @ PC, g[f"c{k}_C_probe"]), B=relf(reg.B, g[f"c{k}_B"]),
                rmse=abs(validate_dyn_sys(reg, traj, ctrl) - float(g[f"c{k}_rmse"])) / float(g[f"c{k}_rmse"]))
    bars = {w: float(g[f"c{k}_bar_{w}"]) for w in errs}
    assert all(errs[w] <= bars[w] for w in errs), (errs, bars, st)


def test_row_ranges_equal_sliced_fit(nk, golden):
    g, X, Y, _, _ = cloth_data(golden)
    cen = X[:, :192].T[:, g["c0_centers_idx"]]
    rr = [[0, 1010], [2020, 3030]]
    a = nk.KoopmanSplineRegressor(6, m=10, gamma=1e-5)
    a.centers = cen
    a.fit(X, Y, row_ranges=rr)
    b = nk.KoopmanSplineRegressor(6, m=10, gamma=1e-5)
    b.centers = cen
    rows = np.r_[0:1010, 2020:3030]
    b.fit(np.ascontiguousarray(X[rows]), np.ascontiguousarray(Y[rows]))
    for w in ("A", "B", "C", "weights"):
        assert relf(getattr(a, w), getattr(b, w)) <= 1e-9, w


# ---------------------------------------------------------------------------------------------------- device model
@pytest.fixture(scope="module")
def duffing_model(nk, golden):
    X, Y = duffing_XY(golden)
    g = golden("f15_spline_duffing.npz")
    reg = nk.KoopmanSplineRegressor(1, state_bounds_params=g["bounds"], m=48, gamma=1e-6)
    np.random.seed(3)
    reg.fit(X, Y)
    return reg, X, Y


def test_lift_predict_score_rollout_closed_loop(nk, duffing_model):
    reg, X, Y = duffing_model
    Z = reg.centers
    Q = X[:64, :2]
    r2 = np.sum((Q[:, None, :] - Z.T[None, :, :]) ** 2, axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi_ref = np.nan_to_num(r2 * np.log(np.sqrt(r2)), nan=0.0).T
    phi = reg.lift(Q.T)
    assert relf(phi, phi_ref) < 1e-13
    pred = reg.predict(X[:64])
    pred_ref = (reg.weights @ np.vstack((phi_ref, X[:64, 2:].T))).T
    assert relf(pred, pred_ref) < 1e-12
    s = reg.score_neg_rmse(X[:500], Y[:500])
    s_ref = -np.mean(np.sqrt(np.mean((Y[:500] - reg.predict(X[:500])) ** 2, axis=0)))
    assert abs(s - s_ref) <= 1e-12 * abs(s_ref)
    U = np.random.default_rng(1).uniform(-1, 1, (1, 30))
    sim = reg.rollout(X[0, :2], U)
    z = reg.lift(X[0, :2].reshape(-1, 1))
    ref = [reg.C @ z]
    for t in range(29):
        z = reg.A @ z + reg.B @ U[:, t:t + 1]
        ref.append(reg.C @ z)
    assert relf(sim, np.hstack(ref)) < 1e-11
    K = reg.solve_lqr(c=1.0)
    phi0, phiref = reg.lift(np.array([[0.5], [0.1]])), reg.lift(np.zeros((2, 1)))
    xs, us = reg.closed_loop(K, phi0, phiref, 20)
    p = phi0
    for t in range(20):
        u = K @ (phiref - p)
        assert abs(us[0, t] - u[0, 0]) <= 1e-9 * (1 + abs(u[0, 0]))
        assert relf(xs[:, t:t + 1], reg.C @ p) < 1e-10
        p = reg.A @ p + reg.B @ u
    from nys_koop_lqr_amd import harness
    v = harness.validate_dyn_sys(reg, np.vstack([sim[:, :]]), U)
    assert np.isfinite(v)
    x_s, u_s = harness.lqr_control_plant(5, np.zeros(2), np.array([0.5, 0.1]), reg, K, lambda x, u: 0.9 * x)
    assert x_s.shape == (5,) and u_s.shape == (1, 5)
    vis, _ = harness.lqr_closed_loop(5, np.zeros(2), np.array([0.5, 0.1]), reg, K)
    assert vis.shape == (2, 6)


def test_model_get_S_I_refused(nk, duffing_model):
    from nys_koop_lqr_amd import _lib
    reg, _, _ = duffing_model
    ctx = _lib.get_context()
    h = reg._ensure_model()
    out = np.empty((48, 48))
    for w in (b"S", b"I"):
        assert ctx.lib.nk_model_get(ctx.handle, h, w, out.ctypes.data, 48) == -1
    assert ctx.lib.nk_model_get(ctx.handle, h, b"A", out.ctypes.data, 48) == 0
    np.testing.assert_array_equal(out, reg.A)


def test_pickle_round_trip(nk, duffing_model):
    reg, X, _ = duffing_model
    r2 = pickle.loads(pickle.dumps(reg))
    assert r2._model is None
    np.testing.assert_array_equal(r2.predict(X[:100]), reg.predict(X[:100]))
    np.testing.assert_array_equal(r2.lift(X[:5, :2].T), reg.lift(X[:5, :2].T))


def test_lift_before_fit_draws_from_query(nk):
    reg = nk.KoopmanSplineRegressor(1, m=4, gamma=1e-6)
    Q = np.random.default_rng(2).standard_normal((2, 9))
    np.random.seed(11)
    phi = reg.lift(Q)
    np.random.seed(11)
    idx = np.random.choice(np.arange(0, 9), size=4, replace=False)
    np.testing.assert_array_equal(reg.centers, Q[:, idx])
    for j, i in enumerate(idx):
        assert phi[j, i] == 0.0


def test_device_tensor_inputs(nk, golden):
    torch = pytest.importorskip("torch")
    X, Y = duffing_XY(golden)
    X, Y = X[:20000], Y[:20000]
    g = golden("f15_spline_duffing.npz")
    a = nk.KoopmanSplineRegressor(1, state_bounds_params=g["bounds"], m=30, gamma=1e-6)
    np.random.seed(5)
    a.fit(X, Y)
    b = nk.KoopmanSplineRegressor(1, state_bounds_params=g["bounds"], m=30, gamma=1e-6)
    b.centers = a.centers
    Xd = torch.tensor(X, dtype=torch.float64, device="cuda")
    Yd = torch.tensor(Y, dtype=torch.float64, device="cuda")
    b.fit(Xd, Yd)
    for w in ("A", "B", "C", "weights"):
        assert relf(getattr(b, w), getattr(a, w)) <= 1e-12, w
    np.testing.assert_allclose(b.predict(Xd[:50]), a.predict(X[:50]), rtol=1e-12, atol=1e-14)
    c = nk.KoopmanSplineRegressor(1, m=8, gamma=1e-6)  # data branch: the centres come from the device tensor's rows
    np.random.seed(9)
    c.fit(Xd, Yd)
    np.random.seed(9)
    idx = np.random.choice(np.arange(0, 20000), size=8, replace=False)
    np.testing.assert_array_equal(c.centers, X[idx, :2].T)
