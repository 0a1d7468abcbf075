"""CPU: the host side of the one-call system-identification sweep -- the C-ABI declares and exports nk_rollout_err and
nk_sysid_grid, the per-seed draw protocols of harness.sysid_plan reproduce the draws the reference made (stored in the
fixtures), the unit ordering / output layout / landmark-row mapping are what nk_sysid_grid expects, and the sharded sweep
assembles the same table at world size 2 (gloo) as at world size 1, with a stub standing in for the GPU."""
import os
import re
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def test_new_entry_points_declared_and_exported(lib):
    from nys_koop_lqr_amd import _lib
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    declared = set(re.findall(r"\b(nk_[a-z_0-9]+)\s*\(", header))
    for name in ("nk_rollout_err", "nk_sysid_grid"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct nk_sysid_unit" in header
    assert re.search(r"#define\s+NK_ABI_VERSION\s+2\b", header) and lib.nk_version() == 2
    # the ctypes mirror of nk_sysid_unit: 8-byte fields first to last, two int32 pairs
    import ctypes as C
    assert C.sizeof(_lib.SysidUnit) == 72
    assert [f[0] for f in _lib.SysidUnit._fields_] == ["kernel", "gamma", "jitter", "m", "n_ranges", "row_ranges",
                                                        "landmark_rows", "centers", "traj", "n_traj", "reserved"]


def test_nystrom_draws_equal_the_stored_reference_draws(golden):
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    ms = g["ms"]
    assert len(ms) == 20
    before = np.random.get_state()
    units = harness.sysid_plan(g["X"], g["Y"], 1, dict(gamma=float(g["gamma"])), ms, [0, 1, 2], {0: [0], 1: [1], 2: [2]})
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert len(units) == 60
    for u in units:
        assert u["ranges"] is None and u["traj"] == u["si"] and u["ti"] == 0
        np.testing.assert_array_equal(u["marks"], g[f"idx_{u['si']}_{u['k']}"])


def test_spline_draws_equal_the_stored_reference_centres(golden):
    from nys_koop_lqr_amd import harness
    g12 = golden("f12_duffing_full.npz")
    f = golden("f15_spline_duffing.npz")
    seeds = [int(s) for s in f["seeds"]]
    assert seeds == [0, 1, 2, 199]
    params = dict(gamma=float(f["gamma"]), state_bounds_params=f["bounds"])
    before = np.random.get_state()
    units = harness.sysid_plan(g12["X"], g12["Y"], 1, params, f["ms"], seeds, [[i] for i in range(4)], estimator="spline")
    assert np.array_equal(before[1], np.random.get_state()[1]) and before[2] == np.random.get_state()[2]
    assert len(units) == 80
    for u in units:
        o = int(np.sum(f["ms"][:u["k"]]))
        np.testing.assert_array_equal(u["marks"], f[f"centers_{seeds[u['si']]}"][:, o:o + u["m"]])


def test_extra_draws_advance_the_stream_by_one_draw_per_fit():
    from nys_koop_lqr_amd import harness
    n, d = 50, 2
    X, Y = np.zeros((n, d + 1)), np.zeros((n, d))
    ms = [3, 5, 4]
    units = harness.sysid_plan(X, Y, 1, {}, ms, [7], {7: [0, 1]}, extra_draws=1)
    rs = np.random.RandomState(7)
    want = {}
    for ti in range(2):
        for k, m in enumerate(ms):
            want[(ti, k)] = rs.choice(np.arange(0, n), size=m, replace=False)
            rs.choice(np.arange(0, n), size=m, replace=False)
    for u in units:
        np.testing.assert_array_equal(u["marks"], want[(u["ti"], u["k"])])
    # and without: consecutive draws
    units0 = harness.sysid_plan(X, Y, 1, {}, ms, [7], {7: [0, 1]})
    rs = np.random.RandomState(7)
    for ti in range(2):
        for k, m in enumerate(ms):
            got = [u for u in units0 if (u["ti"], u["k"]) == (ti, k)][0]["marks"]
            np.testing.assert_array_equal(got, rs.choice(np.arange(0, n), size=m, replace=False))


def test_unit_order_is_m_major_and_outputs_are_prefix_sums():
    from nys_koop_lqr_amd import harness, _lib
    n, d = 40, 2
    X, Y = np.zeros((n, d + 1)), np.zeros((n, d))
    ms, seeds = [3, 6, 4], [5, 9]
    units = harness.sysid_plan(X, Y, 1, {}, ms, seeds, [[2, 0], [1, 3]])
    assert [(u["k"], u["si"], u["ti"]) for u in units] == [(k, s, t) for k in range(3) for s in range(2) for t in range(2)]
    assert [u["m"] for u in units] == [3] * 4 + [6] * 4 + [4] * 4
    assert [u["traj"] for u in units[:4]] == [2, 0, 1, 3]
    vals = np.arange(len(units), dtype=float)
    table = harness.sysid_table(units, vals, len(seeds), len(ms))
    assert table.shape == (2, 2, 3)
    for u, v in zip(units, vals):
        assert table[u["si"], u["ti"], u["k"]] == v
    # the flat unit-major layout of nk_sysid_grid for units with several trajectories each
    tuples = [(None, 1.0, 0.0, 3, None, np.zeros((3, d)), idx) for idx in ([0], [1, 2, 3], [4, 0], [2])]
    _, offs = _lib.sysid_unit_layout(tuples)
    assert offs.tolist() == [0, 1, 4, 6, 7]
    with pytest.raises(ValueError):
        _lib.sysid_unit_layout([(None, 1.0, 0.0, 3, None, np.zeros((3, d)), [])])


def test_landmark_rows_map_through_shuffled_training_ranges():
    """A tiny cloth-shaped example: 5 trajectories of different content, a data set that holds all of them in index order,
    a shuffled training set as ranges.  The rows the plan selects must be the rows the reference's own concatenation
    (create_data_matrices over the shuffled indices) holds at the drawn positions."""
    from nys_koop_lqr_amd import harness
    rng = np.random.default_rng(3)
    d, p, T = 3, 2, 6
    trajs = [rng.standard_normal((d, T)) for _ in range(5)]
    ctrls = [rng.standard_normal((p, T)) for _ in range(5)]
    Xall, Yall = harness.create_data_matrices(trajs, ctrls, range(5))
    Xall, Yall = np.ascontiguousarray(Xall.T), np.ascontiguousarray(Yall.T)
    order = np.array([3, 0, 4])
    ranges = [(int(i) * (T - 1), (int(i) + 1) * (T - 1)) for i in order]
    Xref, Yref = harness.create_data_matrices(trajs, ctrls, order)
    rowmap = harness.train_row_map(ranges, Yall.shape[0])
    np.testing.assert_array_equal(Yall[rowmap], Yref.T)
    np.testing.assert_array_equal(Xall[rowmap], Xref.T)
    units = harness.sysid_plan(Xall, Yall, p, {}, [4, 7], [11], {11: [1, 2]}, train_ranges={11: ranges})
    rs = np.random.RandomState(11)
    for ti in range(2):
        for k, m in enumerate([4, 7]):
            idx = rs.choice(np.arange(0, Yref.shape[1]), size=m, replace=False)
            u = [u for u in units if (u["ti"], u["k"]) == (ti, k)][0]
            np.testing.assert_array_equal(Yall[u["marks"]], Yref.T[idx])
            np.testing.assert_array_equal(u["ranges"], np.asarray(ranges))
    # spline units without state bounds draw their centres from the training states in the same order
    su = harness.sysid_plan(Xall, Yall, p, dict(gamma=1.0), [4], [11], {11: [1]}, train_ranges={11: ranges}, estimator="spline")
    idx = np.random.RandomState(11).choice(np.arange(0, Yref.shape[1]), size=4, replace=False)
    np.testing.assert_array_equal(su[0]["marks"], Xref[:d, idx])
    with pytest.raises(ValueError):
        harness.train_row_map([(0, Yall.shape[0] + 1)], Yall.shape[0])


def test_open_loop_pack_layout():
    from nys_koop_lqr_amd.regressors import open_loop_pack
    rng = np.random.default_rng(0)
    tr, ct = rng.standard_normal((3, 2, 5)), rng.standard_normal((3, 1, 4))
    t, U = open_loop_pack(tr, ct, 2, 1)
    assert t.shape == (3, 5, 2) and U.shape == (3, 5, 1) and t.flags.c_contiguous and U.flags.c_contiguous
    np.testing.assert_array_equal(t[1, :, 0], tr[1, 0])
    np.testing.assert_array_equal(U[2, :4, 0], ct[2, 0])
    assert np.all(U[:, 4] == 0)
    t1, U1 = open_loop_pack(tr[0], ct[0], 2, 1)
    np.testing.assert_array_equal(t1, t[:1])
    np.testing.assert_array_equal(U1, U[:1])
    with pytest.raises(ValueError):
        open_loop_pack(tr, ct[:, :, :3], 2, 1)


# ---------------------------------------------------------------------------------------------------------------
# sharded sweep, world size 2 over gloo, a stub unit in place of the GPU
# ---------------------------------------------------------------------------------------------------------------
COMMON = textwrap.dedent("""
    import numpy as np
    def problem():
        rng = np.random.default_rng(5)
        n, d, p, T = 60, 2, 1, 7
        X, Y = rng.standard_normal((n, d + p)), rng.standard_normal((n, d))
        trajs, ctrls = rng.standard_normal((4, d, T)), rng.standard_normal((4, p, T - 1))
        seeds, ms = [0, 4, 9], [3, 5, 8, 4, 6]
        test_index = {0: [0, 1], 4: [2, 3], 9: [1, 3]}
        ranges = {0: [(30, 60), (0, 10)], 4: [(10, 50)], 9: [(0, 20), (40, 60)]}
        return X, Y, p, trajs, ctrls, seeds, ms, test_index, ranges
    def unit(X, Y, p, params, u, tr, U, estimator, relative):
        # a deterministic stand-in for fit + score: depends on the landmarks, the rows, the trajectory and the controls
        rows = np.concatenate([np.arange(b, e) for b, e in u["ranges"]])
        return float(np.sum(Y[u["marks"]]) + 1e-3 * np.sum(X[rows]) + tr[u["traj"]].sum() * u["m"] + U[u["traj"]].sum()
                     + (100.0 if relative else 0.0))
""")

WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, {root!r})
    sys.path.insert(0, {out!r})
    from nys_koop_lqr_amd import dist as nkd
    from sysid_common import problem, unit
    rank, world = nkd.init_process_group("gloo")
    assert world == 2
    X, Y, p, trajs, ctrls, seeds, ms, test_index, ranges = problem()
    table = nkd.sharded_sysid_sweep(X, Y, p, {{}}, ms, seeds, trajs, ctrls, test_index, train_ranges=ranges, relative=True,
                                    extra_draws=1, unit_fn=unit)
    np.save(os.path.join({out!r}, f"table_{{rank}}.npy"), table)
""")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_sharded_sysid_sweep_world2_gloo(tmp_path):
    (tmp_path / "sysid_common.py").write_text(COMMON)
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    t0, t1 = np.load(tmp_path / "table_0.npy"), np.load(tmp_path / "table_1.npy")
    assert t0.shape == (3, 2, 5) and np.array_equal(t0, t1) and np.all(np.isfinite(t0))
    sys.path.insert(0, str(tmp_path))
    try:
        from sysid_common import problem, unit
    finally:
        sys.path.remove(str(tmp_path))
    from nys_koop_lqr_amd import dist as nkd
    X, Y, p, trajs, ctrls, seeds, ms, test_index, ranges = problem()
    serial = nkd.sharded_sysid_sweep(X, Y, p, {}, ms, seeds, trajs, ctrls, test_index, train_ranges=ranges, relative=True,
                                     extra_draws=1, unit_fn=unit)
    assert np.array_equal(serial, t0)
