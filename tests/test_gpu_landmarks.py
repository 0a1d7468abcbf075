"""GPU: landmark selection on the device (nk_select_landmarks, csrc/nk_landmarks.hip) against the NumPy reference of
tests/landmark_reference.py: exact ties across workgroups, exact indices where the reference's gap is decisive, a replay of
the DEVICE's pivots in float64 and long double on data where it is not, the early stop, host / device operands, the
rejections, and the way through the estimator and the sweep.  Shapes cross the 256-row workgroup (257, 1000), the groups of
four of the column sum (m = 65), the 256-entry staging loops (m = 300, d = 300) and the 1024 partial sums the pick stages
per pass (n = 262 444)."""
import ctypes as C
import pickle

import numpy as np
import pytest

import landmark_reference as lr

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
MATERN = dict(kind="matern52", length_scale=0.5)


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


def dev_kernel(kernel):
    from nys_koop_lqr_amd import _lib
    from nys_koop_lqr_amd.kernels import DeviceKernel
    if kernel["kind"] == "linear":
        return DeviceKernel(_lib.NK_KERNEL_LINEAR, None, kernel["sigma0"])
    return DeviceKernel(_lib.NK_KERNEL_RBF if kernel["kind"] == "rbf" else _lib.NK_KERNEL_MATERN52, kernel["length_scale"])


def data(n, d, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, d))


def raw_call(nk, kd, Y, ldy, n, d, ranges, rule, u, m, tol, ctx_handle=None):
    """nk_select_landmarks through ctypes with sentinel-filled outputs: (rc, rows, resid, trace, m_selected)."""
    ctx = nk.get_context()
    rows, resid, trace = np.full(max(m, 1), -7, dtype=np.int64), np.full(max(m, 1), 7.0), np.full(max(m, 1) + 1, 7.0)
    cnt = C.c_int32(-7)
    flat = None if ranges is None else np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1))
    rc = ctx.lib.nk_select_landmarks(ctx.handle if ctx_handle is None else ctx_handle, kd, Y, ldy, n, d,
                                     None if flat is None else flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                     0 if flat is None else flat.size // 2, rule, None if u is None else u.ctypes.data, m,
                                     float(tol), rows.ctypes.data, resid.ctypes.data, trace.ctypes.data, C.byref(cnt))
    return rc, rows, resid, trace, cnt.value


# ---- 1. exact ties and the tie rule across workgroups -------------------------------------------------------------
def test_exact_ties_go_to_the_lowest_position_across_workgroups(nk):
    Y = 2.0 * np.eye(600)
    kern = dev_kernel(dict(kind="linear", sigma0=0.0))
    rows, info = nk.select_landmarks(Y, kern, 10, return_info=True)
    assert rows.tolist() == list(range(10))
    assert np.all(info["resid"] == 4.0) and info["trace"].tolist() == [4.0 * (600 - j) for j in range(11)]
    rows, info = nk.select_landmarks(Y, kern, 10, row_ranges=[(300, 600), (0, 300)], return_info=True)
    assert rows.tolist() == list(range(300, 310))
    assert np.all(info["resid"] == 4.0) and info["trace"].tolist() == [4.0 * (600 - j) for j in range(11)]


# ---- 2. exact indices where the reference is decisive --------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,d,m", [(257, 2, 24), (1000, 3, 65), (1000, 3, 130), (300, 1, 16)])
def test_greedy_rows_equal_the_reference_where_its_gap_is_decisive(nk, n, d, m, seed):
    Y = data(n, d, seed)
    ref = lr.pchol(Y, MATERN, m)
    gap = float(ref["gap"][1:].min())
    print(f"n={n} d={d} m={m} seed={seed}: smallest gap between the two largest residuals after step 0 = {gap:.3e}")
    assert ref["m_selected"] == m and gap >= 1e-9, gap
    rows = nk.select_landmarks(Y, dev_kernel(MATERN), m)
    assert rows.tolist() == ref["pivots"].tolist()


# ---- 3. replay of the device's pivots on any data ------------------------------------------------------------------
ANISO = dict(kind="rbf", length_scale=[1.0, 10.0, 100.0] * 64)
REPLAY = [  # (label, kernel, n, d, m, row ranges)
    ("rbf-1", dict(kind="rbf", length_scale=0.3), 1, 2, 1, None),
    ("rbf-257", dict(kind="rbf", length_scale=0.3), 257, 2, 65, None),
    ("rbf-1000", dict(kind="rbf", length_scale=0.3), 1000, 3, 65, None),
    ("rbf-1000-ranges", dict(kind="rbf", length_scale=0.3), 1000, 3, 65, [(700, 1000), (10, 10), (0, 413)]),
    ("rbf-1000-m300", dict(kind="rbf", length_scale=0.3), 1000, 3, 300, None),
    ("rbf-262444", dict(kind="rbf", length_scale=0.3), 262444, 1, 5, None),
    ("aniso-257", ANISO, 257, 192, 33, None),
    ("aniso-1000", ANISO, 1000, 192, 65, None),
    ("matern-1", MATERN, 1, 3, 1, None),
    ("matern-257", MATERN, 257, 2, 24, None),
    ("matern-1000", MATERN, 1000, 3, 65, None),
    ("linear-1", dict(kind="linear", sigma0=0.5), 1, 5, 1, None),
    ("linear-257", dict(kind="linear", sigma0=0.5), 257, 80, 65, None),
    ("linear-1000", dict(kind="linear", sigma0=0.5), 1000, 300, 65, None),
]


@pytest.mark.parametrize("rule", ["greedy", "rpcholesky"])
@pytest.mark.parametrize("label,kernel,n,d,m,ranges", REPLAY, ids=[c[0] for c in REPLAY])
def test_device_pivots_replayed_in_float64_and_long_double(nk, label, kernel, n, d, m, ranges, rule):
    from nys_koop_lqr_amd import harness
    Y = data(n, d, seed=len(label))
    u = np.random.default_rng(100 + m).uniform(size=m)
    rows, info = nk.select_landmarks(Y, dev_kernel(kernel), m, rule=rule, row_ranges=ranges, u=u, return_info=True)
    rowmap = harness.train_row_map(ranges, n)
    nc = len(rowmap)
    assert len(rows) == m and len(set(rows.tolist())) == m and set(rows.tolist()) <= set(rowmap.tolist())
    inv = np.full(n, -1, dtype=np.int64)
    inv[rowmap] = np.arange(nc)
    piv = inv[rows]
    r64 = lr.replay(Y, kernel, piv, positions=rowmap)
    rld = lr.replay(Y, kernel, piv, positions=rowmap, dtype=np.longdouble)
    move = np.abs(r64["resid"].astype(np.longdouble) - rld["resid"]).astype(np.float64)
    slack = np.maximum(10.0 * move, 64.0 * EPS * float(r64["dg0max"]) * (np.arange(m) + 1))
    T = r64["trace"]
    worst = dict(resid=0.0, trace=0.0, pick=0.0)
    for j in range(m):
        s = slack[j]
        worst["resid"] = max(worst["resid"], abs(info["resid"][j] - r64["resid"][j]) / s)
        worst["trace"] = max(worst["trace"], abs(info["trace"][j] - T[j]) / (nc * s))
        if rule == "greedy":
            worst["pick"] = max(worst["pick"], (r64["dgmax"][j] - r64["resid"][j]) / s)
        else:
            w = nc * EPS * T[j]
            t = u[j] * T[j]
            worst["pick"] = max(worst["pick"], 0.0 if r64["cum_lo"][j] - w <= t <= r64["cum_hi"][j] + w else np.inf)
    worst["trace"] = max(worst["trace"], abs(info["trace"][m] - T[m]) / (nc * slack[m - 1]))
    print(f"{label} {rule}: worst misses in units of the slack: {worst}")
    assert max(worst.values()) <= 1.0, worst


# ---- 4. early stop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["greedy", "rpcholesky"])
def test_early_stop_on_seven_distinct_points(nk, rule):
    rng = np.random.default_rng(11)
    Y = data(7, 2, seed=3)[rng.integers(0, 7, 500)]
    Y[:7] = data(7, 2, seed=3)  # every point is present
    kd, keep = dev_kernel(MATERN).desc(2)
    u = rng.uniform(size=20)
    rc, rows, resid, trace, cnt = raw_call(nk, C.byref(kd), Y.ctypes.data, 2, 500, 2, None, 0 if rule == "greedy" else 1, u, 20,
                                           1e-8)
    assert rc == 0 and cnt == 7
    assert len({tuple(Y[i]) for i in rows[:7]}) == 7
    assert np.all(rows[7:] == -1)
    assert 0.0 <= trace[7] <= 500 * 1e-8 and resid[7] <= 1e-8 and np.all(resid[:7] > 1e-8)
    got, info = nk.select_landmarks(Y, dev_kernel(MATERN), 20, rule=rule, tol=1e-8, u=u, return_info=True)
    assert got.tolist() == rows[:7].tolist() and info["trace"].shape == (8,) and info["stop_resid"] == resid[7]


# ---- 5. pointers and staging ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1000, 40), (200000, 6)])  # page-locked transport / arena transport for the host array
def test_host_and_device_operands_give_the_same_bits(nk, n, m):
    import torch
    d, ld = 3, 5
    big = np.zeros((n, ld))
    big[:, :d] = data(n, d, seed=5)
    big[:, d:] = 1e30  # never read
    u = np.random.default_rng(6).uniform(size=m)
    kern = dev_kernel(dict(kind="rbf", length_scale=0.3))
    outs = []
    for rule in ("greedy", "rpcholesky"):
        dense = nk.select_landmarks(np.ascontiguousarray(big[:, :d]), kern, m, rule=rule, u=u, return_info=True)
        host = nk.select_landmarks(big[:, :d], kern, m, rule=rule, u=u, return_info=True)
        t = torch.from_numpy(big).to("cuda")
        dev = nk.select_landmarks(t[:, :d], kern, m, rule=rule, u=u, return_info=True)
        for other in (host, dev):
            assert np.array_equal(other[0], dense[0])
            for key in ("resid", "trace"):
                assert np.array_equal(other[1][key].view(np.uint64), dense[1][key].view(np.uint64)), (rule, key)
        outs.append(dense[0])
    assert len(outs[0]) == m and len(outs[1]) == m


# ---- 6. rejections ----------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(nk):
    from nys_koop_lqr_amd import _lib
    from nys_koop_lqr_amd.kernels import DeviceKernel
    Y = data(50, 2)
    good, keep = dev_kernel(MATERN).desc(2)
    tps, keep2 = DeviceKernel(_lib.NK_KERNEL_TPS).desc(2)
    wrong_d, keep3 = dev_kernel(MATERN).desc(3)
    u = np.full(8, 0.5)
    u_one = u.copy()
    u_one[3] = 1.0
    lib = _lib.load_library()
    members = (C.c_void_p * 2)()
    _lib.check(lib.nk_group_create(0, 2, members))
    try:
        cases = {
            "tps": dict(kd=tps), "m > n_c": dict(m=51), "m > n_c of the ranges": dict(m=8, ranges=[(0, 4), (10, 13)]),
            "m = 0": dict(m=0), "negative tol": dict(tol=-1e-3), "nan tol": dict(tol=np.nan), "unknown rule": dict(rule=2),
            "u NULL": dict(rule=1, u=None), "u = 1": dict(rule=1, u=u_one), "range outside": dict(ranges=[(0, 51)]),
            "dimension": dict(kd=wrong_d), "lock-step member": dict(ctx_handle=members[0]),
        }
        for name, kw in cases.items():
            a = dict(kd=good, ranges=None, rule=0, u=u, m=8, tol=0.0, ctx_handle=None)
            a.update(kw)
            rc, rows, resid, trace, cnt = raw_call(nk, C.byref(a["kd"]), Y.ctypes.data, 2, 50, 2, a["ranges"], a["rule"], a["u"],
                                                   a["m"], a["tol"], a["ctx_handle"])
            assert rc == -1, name
            assert np.all(rows == -7) and np.all(resid == 7.0) and np.all(trace == 7.0) and cnt == -7, name
            assert lib.nk_last_error(), name
    finally:
        for mb in members:
            lib.nk_destroy(mb)
    rc, rows, resid, trace, cnt = raw_call(nk, C.byref(good), Y.ctypes.data, 2, 50, 2, None, 0, None, 8, 0.0)
    assert rc == 0 and cnt == 8  # the same call without a fault; greedy needs no u


# ---- 7. through the estimator and the sweep ---------------------------------------------------------------------------
def test_fit_with_the_greedy_rule(nk):
    from sklearn.base import clone
    rng = np.random.default_rng(2)
    n, d, p, m = 1000, 2, 1, 40
    S, U = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (n, p))
    Y = np.tanh(S @ np.array([[0.9, 0.2], [-0.3, 0.8]])) + 0.1 * U
    X = np.hstack([S, U])
    kernel = nk.KernelWrapper([0.5, 0.5])
    reg = nk.KoopmanNystromRegressor(p, kernel=kernel, gamma=1e-6, m=m)
    reg.landmark_rule = "greedy"
    ranges = [(500, 1000), (0, 300)]
    reg.fit(X, Y, row_ranges=ranges)
    rows = nk.select_landmarks(Y, kernel, m, row_ranges=ranges)
    assert len(rows) == m and np.all((rows < 300) | (rows >= 500))
    assert np.array_equal(reg.nystrom_centers_output, Y[rows].T)
    assert reg.fit_stats_["rank_inner"] == m + p  # the Cholesky branch, no rank truncation
    assert np.all(np.isfinite(reg.A)) and reg.A.shape == (m, m)
    assert clone(reg).landmark_rule == "uniform"
    r2 = pickle.loads(pickle.dumps(reg))
    assert r2.landmark_rule == "greedy" and np.array_equal(r2.nystrom_centers_output, reg.nystrom_centers_output)
    # a tolerance stops the selection early and the fit takes m from the landmark array
    few = nk.KoopmanNystromRegressor(p, kernel=kernel, gamma=1e-6, m=m)
    few.landmark_rule, few.landmark_tol = "rpcholesky", 0.2
    np.random.seed(4)
    few.fit(X, Y)
    np.random.seed(4)
    want = nk.select_landmarks(Y, kernel, m, rule="rpcholesky", tol=0.2)
    assert 1 <= len(want) < m and np.array_equal(few.nystrom_centers_output, Y[want].T) and few.A.shape == (len(want),) * 2


@pytest.mark.parametrize("rule", ["greedy", "rpcholesky"])
def test_sweep_over_selected_landmarks(nk, golden, rule):
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])
    seeds = [int(s) for s in g["seeds"]]
    params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))
    ms = (8, 16, 32)
    test_index = [[i] for i in range(len(seeds))]
    cen = harness.landmark_centers(Y, params["kernel"], ms, seeds, test_index, rule=rule)
    assert sorted(cen) == sorted((s, 0, k) for s in seeds for k in range(3))
    for s in seeds:
        assert np.array_equal(cen[(s, 0, 0)], cen[(s, 0, 2)][:8]) and len(set(cen[(s, 0, 2)].tolist())) == 32
    assert np.array_equal(cen[(seeds[0], 0, 2)], cen[(seeds[1], 0, 2)]) == (rule == "greedy")
    a = dict(X=X, Y=Y, n_inputs=1, params=params, ms=ms, seeds=seeds, trajs=np.stack([g[f"traj_{s}"] for s in seeds]),
             controls=np.stack([g[f"ctrl_{s}"] for s in seeds]), test_index=test_index, relative=True, centers=cen)
    loop = harness.sysid_sweep(batch=0, **a)
    one = harness.sysid_sweep(batch=8, **a)
    assert loop.shape == (len(seeds), 1, 3) and np.all(np.isfinite(loop))
    assert np.array_equal(one.view(np.uint64), loop.view(np.uint64))
