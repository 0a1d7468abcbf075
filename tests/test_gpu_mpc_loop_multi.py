"""GPU: the multi-model form of the constrained Koopman MPC loop (nk_mpc_loop_multi through Context.mpc_loop_multi,
harness.mpc_loop_multi and harness.lqr_sweep(controller=...)).  Every unit of a call is compared bit for bit with
regressor.closed_loop_plant_mpc of that unit alone (states, controls, out_info), in any order and in any subset; the eight
scores are compared bit for bit with harness.mpc_scores of the returned trajectories; then the limits on m, the argument
checks with canaries, a NaN unit beside healthy ones, and the sweep."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mpc_loop import _limited, _synthetic_controller
from test_gpu_poly_plant_loop import _assert_replay, _limit_model, fits, nk  # noqa: F401  (fits, nk: fixtures)
from test_poly_plant_host import make_plant

pytestmark = pytest.mark.gpu

STEPS = 60
ALL = (True, True, True, True)


def _unit(reg, ctl, iters, x0, tol=0.0, u_init=None):
    return dict(reg=reg, ctl=ctl, iters=iters, tol=tol, x0=np.asarray(x0, dtype=np.float64), u_init=u_init)


def _run(nk, plant, units, steps=STEPS, u_opt=None, rows=None, want=ALL):
    """One nk_mpc_loop_multi call over `units` with reference 0: (scores, states, controls, info), None where not wanted."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    pairs = [_lib.mpc_desc(u["ctl"], u["iters"], u["tol"]) for u in units]
    d = plant.n_states
    out = ctx.mpc_loop_multi(plant.descriptor(), steps, [u["reg"]._ensure_model() for u in units], [ds for ds, _ in pairs],
                             np.stack([u["x0"] for u in units]), np.zeros((len(units), d)),
                             u_inits=[u["u_init"] for u in units], u_opt=u_opt, uopt_rows=rows, want_x=want[0], want_u=want[1],
                             want_info=want[2], want_scores=want[3])
    del pairs
    return out


def _single(plant, u, steps=STEPS):
    """The unit alone: closed_loop_plant_mpc, as (states (steps + 1, d), controls (steps, p), info (steps, 2))."""
    s, c, i = u["reg"].closed_loop_plant_mpc(u["ctl"], u["x0"], np.zeros(plant.n_states), steps, plant, iters=u["iters"],
                                             tol=u["tol"], u_init=u["u_init"], return_info=True)
    return np.ascontiguousarray(s.T), np.ascontiguousarray(c.T), i


def _assert_units_equal_singles(plant, units, res, singles, label):
    _, ox, ou, oi = res
    for k, (u, (s, c, i)) in enumerate(zip(units, singles)):
        assert np.array_equal(ox[k], s), (label, k, "states")
        assert np.array_equal(ou[k], c), (label, k, "controls")
        assert np.array_equal(oi[k], i), (label, k, "info")


def _host_scores(units, res, u_opt, rows):
    from nys_koop_lqr_amd import harness
    _, ox, ou, oi = res
    table = np.empty((len(units), len(harness.MPC_SCORE_NAMES)))
    for k, u in enumerate(units):
        uo = None if rows[k] < 0 else u_opt[rows[k]]
        h = harness.mpc_scores(ox[k].T, ou[k].T, oi[k], u["ctl"], uo, u["u_init"])
        table[k] = [h[name] for name in harness.MPC_SCORE_NAMES]
    return table


def _u_opt(n, steps, p):
    t = np.arange(steps)
    return np.stack([np.stack([0.2 / (r + 1) * np.exp(-t / 40.0) * np.cos(0.1 * (j + 1) * t) for j in range(p)], axis=1)
                     for r in range(n)])


@pytest.fixture(scope="module")
def duffing(nk, fits):
    """The five Duffing units of the issue (Matern fits; box 0.3 |K e_0|, rates 5 %: active limits), their single calls and
    ONE mixed call with everything returned; u_opt: row 0 shared by units 0 and 1, rows 1 and 2 for units 2 and 3, none for 4."""
    x0 = np.array([-0.5, 0.0])
    units = []
    for m, N, iters, tol in ((20, 8, 25, 0.0), (64, 16, 0, 0.0), (65, 17, 100, 1e-9), (130, 33, 10, 0.0)):
        plant, reg, K = fits("duffing", m)
        ctl, _ = _limited(reg, K, plant, x0, N, 1.0, 0.3, 0.05)
        units.append(_unit(reg, ctl, iters, x0, tol))
    b = float(units[0]["ctl"].hi[0])
    units.append(_unit(units[0]["reg"], units[0]["ctl"], 25, np.array([0.4, -0.2]), u_init=np.array([0.5 * b])))
    u_opt, rows = _u_opt(3, STEPS, 1), [0, 0, 1, 2, -1]
    res = _run(nk, plant, units, u_opt=u_opt, rows=rows)
    singles = [_single(plant, u) for u in units]
    return dict(plant=plant, units=units, u_opt=u_opt, rows=rows, res=res, singles=singles)


@pytest.fixture(scope="module")
def p4b(nk, fits):
    """P4b (d = 4, p = 4): m = 300 with N = 16 (nv = 64), m = 40 with N = 8 (nv = 32) and a saturated unit (nv := 4)."""
    x0 = 0.5 * np.ones(4)
    plant, r300, K300 = fits("P4b", 300)
    _, r40, K40 = fits("P4b", 40)
    c300, _ = _limited(r300, K300, plant, x0, 16, 1.0, 0.5)
    c40, _ = _limited(r40, K40, plant, x0, 8, 1.0, 0.5)
    assert c300.nv == 64 and c40.nv == 32
    units = [_unit(r300, c300, 50, x0), _unit(r40, c40, 50, x0), _unit(r40, c40, 0, -x0)]
    u_opt, rows = _u_opt(2, STEPS, 4), [1, -1, 0]
    res = _run(nk, plant, units, u_opt=u_opt, rows=rows)
    singles = [_single(plant, u) for u in units]
    return dict(plant=plant, units=units, u_opt=u_opt, rows=rows, res=res, singles=singles)


def test_mixed_call_equals_single_calls_duffing(nk, duffing):
    """NVP 16 / one wave, nv = 16 at a full wave with iters = 0, NVP 32 with one landmark in the second wave and the early
    stop, NVP 64 with three waves, and the first model again with another x0 and a seed: every unit bit for bit its single
    call; reversed and as a subset every unit keeps its bits, scores included."""
    plant, units, res = duffing["plant"], duffing["units"], duffing["res"]
    assert [u["ctl"].nv for u in units] == [8, 16, 17, 33, 8]
    _assert_units_equal_singles(plant, units, res, duffing["singles"], "mixed")
    assert not np.array_equal(res[2][0], res[2][4])
    _assert_replay(plant, res[1][2].T, res[2][2].T)
    u_opt, rows = duffing["u_opt"], duffing["rows"]
    for label, order in (("reversed", [4, 3, 2, 1, 0]), ("subset", [3, 0, 4])):
        sub = _run(nk, plant, [units[k] for k in order], u_opt=u_opt, rows=[rows[k] for k in order])
        for a in range(4):
            assert np.array_equal(sub[a], res[a][order]), (label, a)
    # through harness.mpc_loop_multi units 0 and 4 (one model, one controller, the same iters and tol) share one description,
    # and with it the prepared constants and the folded W of unit 0: the same bits again
    from nys_koop_lqr_amd import harness
    h = harness.mpc_loop_multi([u["reg"] for u in units], [u["ctl"] for u in units], np.stack([u["x0"] for u in units]),
                               np.zeros(2), STEPS, plant, iters=[u["iters"] for u in units], tol=[u["tol"] for u in units],
                               u_inits=np.stack([np.zeros(1) if u["u_init"] is None else u["u_init"] for u in units]),
                               u_opt=u_opt, uopt_rows=rows, return_trajectories=True, return_info=True)
    assert np.array_equal(h["states"], res[1]) and np.array_equal(h["controls"], res[2]) and np.array_equal(h["info"], res[3])
    assert np.array_equal(np.stack([h[name] for name in harness.MPC_SCORE_NAMES], axis=1), res[0])


def test_kernel_families_in_one_call(nk):
    """P2 at m = 50 with an RBF kernel, a linear kernel and a spline model (no fold: F and K are read transposed), each once
    iterated and once saturated, in one call: bit for bit the single calls.  The controllers come from no Riccati solve
    (_synthetic_controller): the comparison needs none."""
    from nys_koop_lqr_amd import harness
    plant = make_plant("P2")
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    idx = np.random.default_rng(1).choice(2000, 50, False)
    units = []
    for k, kind in enumerate(("rbf", "linear", "spline")):
        if kind == "spline":
            reg = nk.KoopmanSplineRegressor(2, m=50, gamma=1e-6)
            reg.centers = np.ascontiguousarray(Y.T[:, idx])
        else:
            kern = nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2) if kind == "rbf" else nk.LinearKernelWrapper(1.0)
            reg = nk.KoopmanNystromRegressor(2, kernel=kern, gamma=1e-6, m=50)
            reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
        reg.fit(X, Y)
        ctl = _synthetic_controller(np.random.default_rng(40 + k), 50, 2, 8, 0.05)
        units += [_unit(reg, ctl, 20, [0.5, 0.5]), _unit(reg, ctl, 0, [0.3, -0.4])]
    res = _run(nk, plant, units)
    _assert_units_equal_singles(plant, units, res, [_single(plant, u) for u in units], "families")
    assert np.all(res[3][1::2] == 0.0)  # the saturated ones report zeros


def test_several_inputs(nk, p4b):
    """d = 4, p = 4: nv = 64 with five waves, nv = 32 with one, and a saturated unit, in one call."""
    _assert_units_equal_singles(p4b["plant"], p4b["units"], p4b["res"], p4b["singles"], "P4b")
    _assert_replay(p4b["plant"], p4b["res"][1][0].T, p4b["res"][2][0].T)


@pytest.mark.parametrize("which", ["duffing", "p4b"])
def test_scores(nk, fits, duffing, p4b, which):
    """The eight scores against harness.mpc_scores of the returned trajectories, bit for bit; the scores-only call and every
    single-NULL combination give the same scores and the same remaining outputs; a limited unit sits at its limits and
    iterates, a unit with infinite bounds does neither."""
    from nys_koop_lqr_amd import harness
    case = duffing if which == "duffing" else p4b
    plant, units, res, u_opt, rows = case["plant"], case["units"], case["res"], case["u_opt"], case["rows"]
    host = _host_scores(units, res, u_opt, rows)
    names = harness.MPC_SCORE_NAMES
    for k in range(len(units)):
        print(f"\n[{which}] unit {k}: " + ", ".join(f"{n} = {v:.6g}" for n, v in zip(names, res[0][k])))
    assert np.array_equal(res[0], host)
    assert np.all(res[0][np.array(rows) < 0][:, :2] == 0.0) and np.all(res[0][np.array(rows) >= 0][:, 1] > 0.0)
    for want in ((False, False, False, True), (False, True, True, True), (True, False, True, True), (True, True, False, True),
                 (True, True, True, False)):
        part = _run(nk, plant, units, u_opt=u_opt, rows=rows, want=want)
        for a in range(4):
            o = (3, 0, 1, 2)[a]  # `want` is (x, u, info, scores), the result (scores, x, u, info)
            if want[o]:
                assert np.array_equal(part[a], res[a]), (want, a)
            else:
                assert part[a] is None
    lim = names.index("n_at_limit"), names.index("n_iterated")
    assert res[0][0, lim[0]] > 0 and res[0][0, lim[1]] > 0
    if which == "duffing":
        assert res[0][1, lim[1]] == 0 and res[0][1, lim[0]] > 0  # the saturated unit: clipped, never iterated
        _, reg, _ = fits("duffing", 20)
        free = _unit(reg, reg.solve_mpc(8, c=1.0), 25, [-0.5, 0.0])
        fr = _run(nk, plant, [free])
        assert fr[0][0, lim[0]] == 0 and fr[0][0, lim[1]] == 0 and np.all(fr[3] == 0.0)
        assert np.array_equal(fr[0], _host_scores([free], fr, None, [-1]))


def test_limits_on_m(nk):
    """m = 314 at nv = 64 runs (a model without a fit, a synthetic controller); with a second unit at m = 315 the call is a
    ValueError that names unit 1 and the limit."""
    plant = make_plant("P4b")
    reg, _ = _limit_model(nk, 4, 4, 314)
    ctl = _synthetic_controller(np.random.default_rng(5), 314, 4, 16, 0.05)
    unit = _unit(reg, ctl, 30, 0.5 * np.ones(4))
    res = _run(nk, plant, [unit], steps=40)
    _assert_units_equal_singles(plant, [unit], res, [_single(plant, unit, 40)], "m = 314")
    reg1, _ = _limit_model(nk, 4, 4, 315, spline=True)
    ctl1 = _synthetic_controller(np.random.default_rng(5), 315, 4, 16, 0.05)
    with pytest.raises(ValueError, match="unit 1.*at most 314"):
        _run(nk, plant, [unit, _unit(reg1, ctl1, 30, 0.5 * np.ones(4))], steps=40)


def test_rejected_before_any_launch(nk, fits):
    """n_units = 0, all outputs NULL, desc->m != the model's, p mismatch, uopt out of range, reserved != 0, a device pointer
    as x0 and a lock-step member as context: NK_ERR_BAD_ARG, the unit index in the message where a unit is at fault, and
    the canaries in all four outputs untouched."""
    import torch
    from nys_koop_lqr_amd import _lib
    plant, reg, K = fits("duffing", 20)
    _, reg64, K64 = fits("duffing", 64)
    x0 = np.array([-0.5, 0.0])
    ctl, _ = _limited(reg, K, plant, x0, 8, 1.0, 0.3, 0.05)
    ctx = nk.get_context()
    h, h64 = reg._ensure_model(), reg64._ensure_model()
    ds, keep = _lib.mpc_desc(ctl, 20, 0.0)
    xs, xr = np.stack([x0, x0]), np.zeros((2, 2))
    u_opt = np.zeros((1, 10, 1))
    ox, ou, oi, sc = np.full((2, 11, 2), 7.0), np.full((2, 10, 1), 7.0), np.full((2, 10, 2), 7.0), np.full((2, 8), 7.0)

    def call(needle, handle=None, n=2, outs=True, pl=plant, **second):
        """two good units, the second one altered by `second`"""
        arr = (_lib.MpcUnit * 2)()
        for i in range(2):
            arr[i].model, arr[i].desc = h.value if isinstance(h, C.c_void_p) else h, C.pointer(ds)
            arr[i].x0, arr[i].x_ref, arr[i].uopt = xs[i].ctypes.data, xr[i].ctypes.data, 0
        for name, v in second.items():
            setattr(arr[1], name, v)
        ptrs = [a.ctypes.data if outs else None for a in (ox, ou, oi, sc)]
        rc = ctx.lib.nk_mpc_loop_multi(ctx.handle if handle is None else handle, C.byref(pl.descriptor()), 10, arr, n,
                                       u_opt.ctypes.data, 1, *ptrs)
        msg = ctx.lib.nk_last_error().decode()
        assert rc == -1 and all(part in msg for part in needle), (rc, msg, needle)

    call(["n_units = 0"], n=0)
    call(["all null"], outs=False)
    call(["unit 1", "m = 20"], model=h64.value if isinstance(h64, C.c_void_p) else h64)  # the description is for m = 20
    ds1, keep1 = _lib.mpc_desc(_synthetic_controller(np.random.default_rng(3), 20, 2, 4, 0.1), 20, 0.0)
    call(["unit 1", "inputs"], desc=C.pointer(ds1))
    call(["unit 0", "inputs"], pl=make_plant("P2"))  # the plant has two inputs, model and description one
    call(["unit 1", "uopt = 1"], uopt=1)
    call(["unit 1", "uopt = -2"], uopt=-2)
    call(["unit 1", "reserved"], reserved=1)
    dev = torch.zeros(2, dtype=torch.float64, device="cuda")
    call(["unit 1", "host memory"], x0=dev.data_ptr())
    handles = (C.c_void_p * 2)()
    _lib.check(ctx.lib.nk_group_create(ctx.device, 2, handles))
    members = [_lib.Context(ctx.device, C.c_void_p(handles[i])) for i in range(2)]
    try:
        call(["lock-step"], handle=members[0].handle)
    finally:
        for mem in members:
            mem.close()
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(oi == 7.0) and np.all(sc == 7.0)  # nothing ran
    del keep, keep1
    with pytest.raises(ValueError, match="steps"):
        _run(nk, plant, [_unit(reg, ctl, 20, x0)], steps=0)
    res = _run(nk, plant, [_unit(reg, ctl, 20, x0)], steps=10)  # and the call still works
    assert np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[1]))


@pytest.fixture(scope="module")
def nan_call(nk, duffing):
    """The mixed Duffing call with a NaN initial state in unit 2 (m = 65, 100 iterations with the early stop)."""
    units = duffing["units"]
    mixed = [units[0], units[1], dict(units[2], x0=np.array([np.nan, 0.0])), units[3], units[4]]
    return _run(nk, duffing["plant"], mixed, u_opt=duffing["u_opt"], rows=duffing["rows"])


def test_nan_x0_in_one_unit_leaves_the_other_units_their_bits(nk, duffing, nan_call):
    """The other units of the call keep their bits, scores included.  The NaN unit ends: every step runs all its 100 iterations
    (no comparison with a NaN residual is true), as the NumPy statement of the iteration does at a NaN gradient; its states
    from step 1 on, its controls, residuals, J and r_max are NaN; it is its own single call (NaNs at the same places) and its
    scores are those of harness.mpc_scores on what it returned."""
    from nys_koop_lqr_amd import harness
    names, res = harness.MPC_SCORE_NAMES, duffing["res"]
    keep = [0, 1, 3, 4]
    for a in range(4):
        assert np.array_equal(nan_call[a][keep], res[a][keep]), a
    sc = dict(zip(names, nan_call[0][2]))
    print("\n[NaN x0] " + ", ".join(f"{n} = {v!r}" for n, v in sc.items()))
    assert np.all(np.isnan(nan_call[1][2][1:])) and np.all(np.isnan(nan_call[2][2])) and np.isnan(sc["J"]) and np.isnan(sc["r_max"])
    assert np.all(nan_call[3][2][:, 0] == 100.0) and np.all(np.isnan(nan_call[3][2][:, 1]))
    assert sc["iters_sum"] == 100.0 * STEPS and sc["n_iterated"] == STEPS and sc["n_at_limit"] == 0.0
    unit = dict(duffing["units"][2], x0=np.array([np.nan, 0.0]))
    for got, want in zip(nan_call[1:], _single(duffing["plant"], unit)):
        assert np.array_equal(got[2], want, equal_nan=True)
    host = harness.mpc_scores(nan_call[1][2].T, nan_call[2][2].T, nan_call[3][2], unit["ctl"], duffing["u_opt"][1])
    assert np.array_equal(nan_call[0][2], [host[n] for n in names], equal_nan=True)


def test_nan_x0_in_one_unit(nk, nan_call):
    """A NaN initial state in one unit: that unit's u_absmax is NaN (NaN from the first NaN control on).  The clips of the
    loop are fmin / fmax, which alone would drop a NaN and return a bound; a step whose gradient or shifted rate bound holds a
    NaN is therefore decided before the iteration, as the NumPy statement of the interface (np.minimum / np.maximum) decides
    it: NaN controls, all iterations counted, NaN residual."""
    from nys_koop_lqr_amd import harness
    assert np.isnan(nan_call[0][2, harness.MPC_SCORE_NAMES.index("u_absmax")])


def _host_lqr_scores(reg, K, plant, x0, steps):
    """The host LQR loop (one lift per step) from x0 to the origin: control_scores of its states and controls."""
    from nys_koop_lqr_amd import harness
    x = np.asarray(x0, dtype=np.float64).reshape(-1, 1)
    phi_ref = reg.lift(np.zeros_like(x))
    xs, us = [x], []
    for _ in range(steps):
        u = K @ (phi_ref - reg.lift(x))
        us.append(u.reshape(-1, 1))
        x = np.asarray(plant.update_SOM(x, u), dtype=np.float64).reshape(-1, 1)
        xs.append(x)
    return harness.control_scores(np.hstack(xs), np.hstack(us))


def test_sweep(nk):
    """harness.lqr_sweep(controller=dict(horizon=8, ...)) on the Duffing data of `fits`, 3 seeds x ms = (20, 65): every table
    entry equals mpc_scores of its trajectory and every trajectory the unit's own closed_loop_plant_mpc, bit for bit.  With all
    limits infinite u_absmax and J agree with lqr_sweep(controller=None) (dlqr's unrefined gain): per unit the bar is 10 x the
    relative difference of the host LQR loop run with dlqr's gain and with the controller's refined gain, floor 1e-10."""
    from nys_koop_lqr_amd import harness
    plant = nk.PolynomialSystem.duffing(0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    params = dict(kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6)
    ms, seeds = (20, 65), (0, 1, 2)
    x0, ref = np.array([-0.5, 0.0]), np.zeros(2)
    u_opt = _u_opt(1, STEPS, 1)[0]
    box = dict(horizon=8, u_min=-0.1, u_max=0.1, du_min=-0.01, du_max=0.01, iters=20, tol=0.0)
    res = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, STEPS, u_opt=u_opt, batch=4, workers=2,
                            return_trajectories=True, controller=box)
    assert res["J"].shape == (3, 2) and res["states"].shape == (3, 2, STEPS + 1, 2) and res["controls"].shape == (3, 2, STEPS, 1)
    assert np.all(res["n_at_limit"] > 0) and np.all(res["n_iterated"] > 0) and np.all(res["u_absmax"] <= 0.1)
    free = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, STEPS, batch=4, workers=2,
                             controller=dict(horizon=8, iters=20))
    lqr = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, STEPS, batch=4, workers=2)
    assert np.all(free["n_at_limit"] == 0) and np.all(free["n_iterated"] == 0)
    for u in harness.lqr_plan(X, Y, 1, params, ms, seeds, "nystrom"):
        si, k = u["si"], u["k"]
        reg = harness.lqr_fit_unit(X, Y, 1, params, u, "nystrom")
        ctl = reg.solve_mpc(8, c=1.0, u_min=-0.1, u_max=0.1, du_min=-0.01, du_max=0.01)
        s, c, i = reg.closed_loop_plant_mpc(ctl, x0, ref, STEPS, plant, iters=20, return_info=True)
        assert np.array_equal(res["states"][si, k], s.T) and np.array_equal(res["controls"][si, k], c.T), (si, k)
        host = harness.mpc_scores(s, c, i, ctl, u_opt)
        for name in harness.MPC_SCORE_NAMES + ("rmse_control",):
            assert res[name][si, k] == host[name], (name, si, k)
        # inactive limits against the LQR sweep: the bar from the host loop under the two gains
        a = _host_lqr_scores(reg, np.asarray(reg.solve_lqr(c=1.0)), plant, x0, STEPS)
        b = _host_lqr_scores(reg, reg.solve_mpc(8, c=1.0).K, plant, x0, STEPS)
        for name in ("u_absmax", "J"):
            moved = abs(a[name] - b[name]) / abs(a[name])
            bar = max(10.0 * moved, 1e-10)
            err = abs(free[name][si, k] - lqr[name][si, k]) / abs(lqr[name][si, k])
            print(f"\n[sweep, seed {si}, m = {u['m']}] {name}: MPC sweep with infinite limits vs LQR sweep {err:.2e}; the host "
                  f"loop moves {moved:.2e} between dlqr's gain and the refined gain (bar {bar:.2e})")
            assert err <= bar, (name, si, k, err, bar)
