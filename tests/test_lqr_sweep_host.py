"""CPU: the host side of the one-call LQR control sweep -- the C-ABI declares and exports nk_plant_loop_multi and its unit
struct, harness.hjb_optimal_control and harness.control_scores reproduce what benchmark_lqr_hjb.py:99-107,304-313 compute (f8
holds the reference's recorded run), the plan of harness.lqr_sweep is sysid_plan's per-seed draw protocol, and the
bookkeeping around a failing gain holds with stubs standing in for the fits and the device loop."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import relf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def test_multi_loop_declared_exported_and_mirrored(lib):
    from nys_koop_lqr_amd import _lib
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    declared = set(re.findall(r"\b(nk_[a-z_0-9]+)\s*\(", header))
    assert "nk_plant_loop_multi" in declared and "nk_plant_loop_multi" in _lib.SIGNATURES
    assert hasattr(lib, "nk_plant_loop_multi")
    assert "typedef struct nk_plant_unit" in header
    assert re.search(r"#define\s+NK_ABI_VERSION\s+2\b", header) and lib.nk_version() == 2  # symbols added, nothing changed
    # the documented layout of nk_plant_unit on an LP64 target: four pointers, then two int32 -- 40 bytes, no padding
    body = re.search(r"typedef struct nk_plant_unit \{(.*?)\} nk_plant_unit;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["model", "K", "x0", "x_ref", "uopt", "reserved"]
    assert [f[0] for f in _lib.PlantUnit._fields_] == fields
    assert C.sizeof(_lib.PlantUnit) == 40
    assert [getattr(_lib.PlantUnit, f).offset for f in fields] == [0, 8, 16, 24, 32, 36]
    assert [getattr(_lib.PlantUnit, f).size for f in fields] == [8, 8, 8, 8, 4, 4]
    # the prototype: ctx, plant, Ts, steps, units, n_units, u_opt, n_uopt, out_x, out_u, scores
    res, args = _lib.SIGNATURES["nk_plant_loop_multi"]
    assert res is C.c_int and len(args) == 11 and args[2] is C.c_double and args[4] is C.POINTER(_lib.PlantUnit)


def test_hjb_optimal_control_reproduces_the_recorded_optimum(golden):
    """f8 records the u_opt of benchmark_lqr_hjb.py:304-311 from x0 = 0.9 over 400 steps.  Bar 1e-12 relative Frobenius: the
    bar the recorded plant replays are held to (tests/test_plants_host.py).  And the sequence is the formula's: replayed
    on the package's plant, every control is x^3 - x sqrt(1 + x^4) of the state it was computed at, exactly."""
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    g = golden("f8_hjb_config2.npz")
    plant = nk.HJB(Ts=0.01)
    u_opt, J_true = harness.hjb_optimal_control(np.array([0.9]), int(g["cl_steps"]), plant)
    e = relf(u_opt, g["u_opt"])
    print(f"\nhjb_optimal_control vs recorded u_opt: {e:.2e}")
    assert u_opt.shape == (400,) and e < 1e-12
    x, J = np.array([[0.9]]), 0.9 * 0.9
    for t in range(400):
        assert u_opt[t] == (x ** 3 - x * np.sqrt(1 + x ** 4)).item()
        x = plant.update_SOM(x, np.array([[u_opt[t]]]))
        J = J + x.item() * x.item() + u_opt[t] * u_opt[t]
    assert J_true == J and np.isfinite(J_true)
    # a prefix of a longer horizon is the same sequence
    assert np.array_equal(harness.hjb_optimal_control(0.9, 50, plant)[0], u_opt[:50])


def test_score_formulas_on_the_recorded_run(golden):
    """harness.control_scores on the reference's recorded closed loop (f8: cl_u, and the states its replay visits) against
    the NumPy expressions of benchmark_lqr_hjb.py:99-107 (open_loop_control's cost) and :313 (control RMSE).  J: the same
    operations in the same order, so equal.  The two sums: NumPy adds pairwise, the scores in step order; both are sums of
    400 non-negative terms, each within 400 eps of the exact sum, so they agree within 2 * 401 eps relative; the RMSE is a
    ratio of their square roots (half the relative error each): the same bound holds for it."""
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    g = golden("f8_hjb_config2.npz")
    plant = nk.HJB(Ts=0.01)
    us, u_opt = g["cl_u"].reshape(1, -1), g["u_opt"]
    x0 = np.array([[0.9]])
    states = harness.open_loop_control(plant.update_SOM, x0, us)  # (1, 401)
    assert relf(states[0, :-1], g["cl_x"]) < 1e-12
    # benchmark_lqr_hjb.py:99-107 on the same states
    Jcurr = x0 ** 2
    for i in range(us.shape[1]):
        Jcurr = Jcurr + states[:, i + 1:i + 2] ** 2 + us[:, i] ** 2
    rmse_ref = np.sqrt(np.sum(np.square(us.squeeze() - u_opt))) / np.sqrt(np.sum(np.square(u_opt))) * 100  # :313
    sc = harness.control_scores(states, us, u_opt)
    bound = 2 * 401 * np.finfo(np.float64).eps
    print(f"\nJ {sc['J']!r} (reference loop {Jcurr.item()!r}); rmse_control {sc['rmse_control']!r} (NumPy {rmse_ref!r}, "
          f"recorded {float(g['rmse_control'])!r})")
    assert sc["J"] == Jcurr.item()
    assert sc["u_absmax"] == np.max(np.abs(us))
    assert abs(sc["sse_u"] - np.sum(np.square(us.squeeze() - u_opt))) <= bound * sc["sse_u"]
    assert abs(sc["ss_opt"] - np.sum(np.square(u_opt))) <= bound * sc["ss_opt"]
    assert abs(sc["rmse_control"] - rmse_ref) <= bound * rmse_ref
    assert abs(sc["rmse_control"] - float(g["rmse_control"])) <= bound * rmse_ref  # the number the reference run printed
    assert harness.control_rmse_percent(us, u_opt) == rmse_ref
    # no u_opt: zeros in the first two slots; a NaN control: u_absmax is NaN whatever follows
    sc0 = harness.control_scores(states, us)
    assert sc0["sse_u"] == 0.0 and sc0["ss_opt"] == 0.0 and sc0["J"] == sc["J"]
    bad = us.copy()
    bad[0, 7] = np.nan
    assert np.isnan(harness.control_scores(states, bad)["u_absmax"])
    # two states: the sum over the coordinates in index order
    xs2 = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 0.125]])
    sc2 = harness.control_scores(xs2, np.array([0.1, -0.2]))
    J2 = 1.0 * 1.0 + 0.5 * 0.5
    J2 = (J2 + (2.0 * 2.0 + 0.25 * 0.25)) + 0.1 * 0.1
    J2 = (J2 + (3.0 * 3.0 + 0.125 * 0.125)) + 0.2 * 0.2
    assert sc2["J"] == J2 and sc2["u_absmax"] == 0.2


def test_plan_is_deterministic_and_uses_the_per_seed_draws(golden):
    """lqr_plan = sysid_plan with one slot per (seed, m): one RandomState(seed) per seed walked m-minor, the global RNG never
    touched; at m = 20 the first draw of seed s is the landmark set the reference's control run recorded (f12, lqr_idx_s)."""
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    X, Y = g["X"], g["Y"]
    n = Y.shape[0]
    params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))
    state = np.random.get_state()[1].copy()
    a = harness.lqr_plan(X, Y, 1, params, [20, 10], [0, 1, 2])
    b = harness.lqr_plan(X, Y, 1, params, [20, 10], [0, 1, 2])
    ref = harness.sysid_plan(X, Y, 1, params, [20, 10], [0, 1, 2], [[0]] * 3)
    assert np.array_equal(np.random.get_state()[1], state)
    assert len(a) == 6 and [(u["k"], u["si"]) for u in a] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]  # m-major
    for ua, ub, ur in zip(a, b, ref):
        assert (ua["si"], ua["ti"], ua["k"], ua["m"]) == (ub["si"], ub["ti"], ub["k"], ub["m"]) == (ur["si"], 0, ur["k"], ur["m"])
        assert np.array_equal(ua["marks"], ub["marks"]) and np.array_equal(ua["marks"], ur["marks"])
    for s in (0, 1, 2):
        rs = np.random.RandomState(s)
        first = rs.choice(np.arange(0, n), size=20, replace=False)
        second = rs.choice(np.arange(0, n), size=10, replace=False)
        assert np.array_equal(a[s]["marks"], first) and np.array_equal(a[3 + s]["marks"], second)
        assert np.array_equal(first, g[f"lqr_idx_{s}"])
    # spline units: centres from the same per-seed stream
    sp = harness.lqr_plan(X[:500], Y[:500], 1, dict(gamma=1e-6), [7], [4], estimator="spline")
    want = harness.spline_centers_draw(dict(m=7), X[:500, :2], rng=np.random.RandomState(4))
    assert sp[0]["marks"].shape == (2, 7) and np.array_equal(sp[0]["marks"], want)
    # given landmarks replace the draws
    given = harness.lqr_plan(X, Y, 1, params, [5], [9], centers={(9, 0): np.arange(5)})
    assert np.array_equal(given[0]["marks"], np.arange(5))


def _stubs(fail=None):
    """Stand-ins for the device: a 'fit' that returns operators tagged with its unit, a gain that raises for the chosen
    (seed position, m position), a 'loop' that scores a unit by its tag and records what it was handed."""
    calls = []

    def fit_fn(X, Y, n_inputs, params, unit, estimator):
        tag = 10.0 * unit["si"] + unit["k"] + 1.0
        return SimpleNamespace(A=np.full((2, 2), tag), B=np.ones((2, 1)), C=np.ones((1, 2)), tag=tag)

    def gain_fn(A, B, C):
        tag = A[0, 0]
        if fail is not None and tag == 10.0 * fail[0] + fail[1] + 1.0:
            raise np.linalg.LinAlgError("no stabilising solution")
        return np.full((1, 2), tag)

    def loop_fn(regs, gains, x0, x_ref, num_steps, plant, u_opt=None, return_trajectories=False):
        calls.append([r.tag for r in regs])
        tags = np.array([r.tag for r in regs])
        assert all(np.all(K == t) for K, t in zip(gains, tags))
        out = dict(sse_u=tags, ss_opt=4.0 * tags, J=tags + 0.5, u_absmax=-tags)
        if return_trajectories:
            out["states"] = np.tile(tags[:, None, None], (1, num_steps + 1, 2))
            out["controls"] = np.tile(tags[:, None], (1, num_steps))
        return out

    return fit_fn, gain_fn, loop_fn, calls


def test_a_failing_gain_is_nan_and_is_not_run():
    from nys_koop_lqr_amd import dist, harness
    X, Y = np.zeros((50, 3)), np.zeros((50, 2))
    args = (X, Y, 1, dict(kernel=None, gamma=1e-6), [4, 6], [0, 1, 2], None, np.zeros(2), np.zeros(2), 5)
    fit_fn, gain_fn, loop_fn, calls = _stubs()
    full = harness.lqr_sweep(*args, gain_fn=gain_fn, fit_fn=fit_fn, loop_fn=loop_fn, return_trajectories=True)
    assert calls == [[1.0, 11.0, 21.0, 2.0, 12.0, 22.0]]  # ONE loop call, every unit, in plan (m-major) order
    tags = np.array([[1.0, 2.0], [11.0, 12.0], [21.0, 22.0]])
    assert np.array_equal(full["sse_u"], tags) and np.array_equal(full["J"], tags + 0.5)
    assert np.array_equal(full["u_absmax"], -tags) and np.array_equal(full["rmse_control"], np.full((3, 2), 50.0))
    assert full["states"].shape == (3, 2, 6, 2) and full["controls"].shape == (3, 2, 5)
    assert np.array_equal(full["controls"][:, :, 0], tags)
    assert set(full["timing"]) >= {"fit_s", "gain_wait_s", "loop_s", "gain_cpu_s"}
    fit_fn, gain_fn, loop_fn, calls = _stubs(fail=(1, 1))
    part = harness.lqr_sweep(*args, gain_fn=gain_fn, fit_fn=fit_fn, loop_fn=loop_fn, return_trajectories=True)
    assert calls == [[1.0, 11.0, 21.0, 2.0, 22.0]]  # the unit without a gain is not submitted
    hole = np.zeros((3, 2), dtype=bool)
    hole[1, 1] = True
    for name in ("sse_u", "ss_opt", "J", "u_absmax", "rmse_control"):
        assert np.all(np.isnan(part[name][hole])) and np.array_equal(part[name][~hole], full[name][~hole]), name
    assert np.all(np.isnan(part["states"][1, 1])) and np.all(np.isnan(part["controls"][1, 1]))
    assert np.array_equal(part["states"][~hole], full["states"][~hole])
    # every gain fails: no loop call at all, an all-NaN table
    fit_fn, _, loop_fn, calls = _stubs()

    def never(A, B, C):
        raise ValueError("no gain")

    none = harness.lqr_sweep(*args, gain_fn=never, fit_fn=fit_fn, loop_fn=loop_fn)
    assert calls == [] and np.all(np.isnan(none["J"])) and "states" not in none
    # a failed fit (None) is a NaN unit too
    fit_fn, gain_fn, loop_fn, calls = _stubs()
    nofit = harness.lqr_sweep(*args, gain_fn=gain_fn, loop_fn=loop_fn,
                              fit_fn=lambda X, Y, p, par, u, est: None if (u["si"], u["k"]) == (0, 0) else fit_fn(X, Y, p, par, u, est))
    assert np.isnan(nofit["J"][0, 0]) and np.array_equal(nofit["J"][~np.isnan(nofit["J"])], (tags + 0.5).reshape(-1)[1:])
    # the sharded sweep at world size 1 assembles the same tables
    fit_fn, gain_fn, loop_fn, calls = _stubs(fail=(1, 1))
    sh = dist.sharded_lqr_sweep(*args, gain_fn=gain_fn, fit_fn=fit_fn, loop_fn=loop_fn)
    for name in ("sse_u", "ss_opt", "J", "u_absmax", "rmse_control"):
        assert np.array_equal(sh[name], part[name], equal_nan=True), name


def test_default_gain_is_solve_lqr():
    """The default gain_fn is regressor.solve_lqr's arithmetic: Q = c C^T C symmetrised, R = I, the host DARE."""
    from nys_koop_lqr_amd import harness
    from nys_koop_lqr_amd.lqr import dlqr
    rng = np.random.default_rng(5)
    A = 0.9 * np.eye(4) + 0.02 * rng.standard_normal((4, 4))
    B, Cm = rng.standard_normal((4, 1)), rng.standard_normal((2, 4))
    Q = 0.3 * Cm.T @ Cm
    K = dlqr(A, B, (Q + Q.T) / 2, np.eye(1))[0]
    assert np.array_equal(harness.lqr_default_gain(0.3)(A, B, Cm), K)
