"""GPU: the multi-model form of the MPC loop with limits on predicted states (nk_mpc_out_loop_multi through
Context.mpc_loop_multi(outs=...), harness.mpc_loop_multi and harness.lqr_sweep(controller=dict(..., x_max=...))).  Every unit
of a call -- with rows, without them, saturated -- is compared bit for bit with regressor.closed_loop_plant_mpc of that unit
alone (states, controls, out_info), in any order and in any subset; the ten scores are compared bit for bit with
harness.mpc_out_scores of the returned trajectories; then kernel families and several inputs, absent outputs, a NaN unit
beside healthy ones, the argument checks with guard values, and the sweep."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mpc_loop_multi import _u_opt
from test_gpu_mpc_out_loop import RHO_FACTOR, U_MAX, _synthetic_output_controller, _with_outputs
from test_gpu_poly_plant_loop import _assert_replay, _limit_model, fits, nk  # noqa: F401  (fits, nk: fixtures)
from test_poly_plant_host import make_plant

pytestmark = pytest.mark.gpu

STEPS = 60
X0, REF = np.array([-0.5, 0.0]), np.array([0.5, 0.0])  # a reference off the origin: the shift of the absolute bounds is live
ALL = (True, True, True, True)


def _unit(reg, ctl, iters, x0, ref, tol=0.0, u_init=None):
    return dict(reg=reg, ctl=ctl, iters=iters, tol=tol, x0=np.asarray(x0, dtype=np.float64),
                ref=np.asarray(ref, dtype=np.float64), u_init=u_init)


def _has_rows(u):
    return hasattr(u["ctl"], "ycomp") and u["iters"] != 0


def _run(nk, plant, units, steps=STEPS, u_opt=None, rows=None, want=ALL):
    """One nk_mpc_out_loop_multi call over `units`: (scores, states, controls, info), None where not wanted.  A unit whose
    controller has output rows and iters != 0 gets its nk_mpc_out, every other unit a NULL."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    pairs = [_lib.mpc_desc(u["ctl"], u["iters"], u["tol"]) for u in units]
    opairs = [_lib.mpc_out(u["ctl"]) if _has_rows(u) else (None, None) for u in units]
    out = ctx.mpc_loop_multi(plant.descriptor(), steps, [u["reg"]._ensure_model() for u in units], [ds for ds, _ in pairs],
                             np.stack([u["x0"] for u in units]), np.stack([u["ref"] for u in units]),
                             u_inits=[u["u_init"] for u in units], u_opt=u_opt, uopt_rows=rows, want_x=want[0], want_u=want[1],
                             want_info=want[2], want_scores=want[3], outs=[o for o, _ in opairs])
    del pairs, opairs
    return out


def _single(plant, u, steps=STEPS):
    """The unit alone: closed_loop_plant_mpc, as (states (steps + 1, d), controls (steps, p), info (steps, 2))."""
    s, c, i = u["reg"].closed_loop_plant_mpc(u["ctl"], u["x0"], u["ref"], steps, plant, iters=u["iters"], tol=u["tol"],
                                             u_init=u["u_init"], return_info=True)
    return np.ascontiguousarray(s.T), np.ascontiguousarray(c.T), i


def _assert_units_equal_singles(units, res, singles, label):
    _, ox, ou, oi = res
    for k, (s, c, i) in enumerate(singles):
        assert np.array_equal(ox[k], s, equal_nan=True), (label, k, "states")
        assert np.array_equal(ou[k], c, equal_nan=True), (label, k, "controls")
        assert np.array_equal(oi[k], i, equal_nan=True), (label, k, "info")


def _host_scores(units, res, u_opt, rows):
    from nys_koop_lqr_amd import harness
    _, ox, ou, oi = res
    table = np.empty((len(units), len(harness.MPC_OUT_SCORE_NAMES)))
    for k, u in enumerate(units):
        uo = None if rows[k] < 0 else u_opt[rows[k]]
        ctl = u["ctl"] if _has_rows(u) else (u["ctl"].input_only() if hasattr(u["ctl"], "ycomp") else u["ctl"])
        h = harness.mpc_out_scores(ox[k].T, ou[k].T, oi[k], ctl, uo, u["u_init"])
        table[k] = [h[name] for name in harness.MPC_OUT_SCORE_NAMES]
    return table


def _duffing_controllers(fits, m, N, rows):
    """(plant, reg, the input-only controller, the controller with rows) for the Duffing fit of m landmarks: |u| <= 2, rho =
    300 x the default, the velocity limit at 0.6 of the peak |x_2| of the host loop WITHOUT the rows (60 steps, 100
    iterations), as test_gpu_mpc_out_loop._duffing_case.  rows: "v8" = 8 hard rows on x_2; "mixed9" = the first 9 of the rows
    of x_1 <= 0.55 and the velocity limit over 5 steps, soft; "full32" = x_1 <= 0.55 and the velocity limit over 16 steps, hard."""
    from nys_koop_lqr_amd import harness
    plant, reg, _ = fits("duffing", m)
    rho = RHO_FACTOR * reg.solve_mpc(N, c=1.0).rho
    free = reg.solve_mpc(N, c=1.0, u_min=-U_MAX, u_max=U_MAX, rho=rho)
    S0, _, _ = harness.mpc_control_plant(STEPS, REF, X0, reg, free, plant.update_SOM, iters=100)
    v = 0.6 * float(np.max(np.abs(S0[1])))
    kw = dict(c=1.0, u_min=-U_MAX, u_max=U_MAX, rho=rho)
    if rows == "v8":
        ctl = reg.solve_mpc(N, x_min=[-np.inf, -v], x_max=[np.inf, v], y_horizon=8, **kw)
    elif rows == "mixed9":
        full = reg.solve_mpc(N, x_min=[-np.inf, -v], x_max=[0.55, v], y_horizon=5, y_weight=10.0 * rho, **kw)
        ctl = _with_outputs(full, G=full.G[:9], T=full.T[:9], ylo=full.ylo[:9], yhi=full.yhi[:9], ycomp=full.ycomp[:9])
    else:
        ctl = reg.solve_mpc(N, x_min=[-np.inf, -v], x_max=[0.55, v], y_horizon=16, **kw)
    return plant, reg, free, ctl


@pytest.fixture(scope="module")
def duffing(nk, fits):
    """The units of the issue and ONE mixed call with everything returned.  u_opt: row 0 shared by units 0 and 1, rows 1 and 2
    for units 2 and 3, none for the others."""
    plant, r20, free20, c20 = _duffing_controllers(fits, 20, 8, "v8")
    _, r65, _, c65 = _duffing_controllers(fits, 65, 8, "mixed9")
    _, r130, _, c130 = _duffing_controllers(fits, 130, 32, "full32")
    loose = r20.solve_mpc(8, c=1.0, u_min=-U_MAX, u_max=U_MAX, rho=c20.rho, x_min=-100.0, x_max=100.0)
    units = [_unit(r20, c20, 100, X0, REF),                                         # nt = 16, one wave, hard
             _unit(r65, c65, 100, X0, REF, tol=1e-9),                               # nt = 17, two waves, soft, early stop
             _unit(r130, c130, 100, X0, REF),                                       # nt = 64, three waves, hard
             _unit(r20, c20, 100, [-0.3, 0.1], [0.4, 0.0], u_init=np.array([0.5])),  # shares the pieces of unit 0
             _unit(r20, free20, 25, X0, REF),                                       # input limits only
             _unit(r20, c20, 0, X0, REF),                                           # rows in the controller, saturated LQR
             _unit(r20, loose, 100, X0, REF)]                                       # rows that never bind
    u_opt, rows = _u_opt(3, STEPS, 1), [0, 0, 1, 2, -1, -1, -1]
    res = _run(nk, plant, units, u_opt=u_opt, rows=rows)
    singles = [_single(plant, u) for u in units]
    return dict(plant=plant, units=units, u_opt=u_opt, rows=rows, res=res, singles=singles)


def test_mixed_call_equals_single_calls_duffing(nk, duffing):
    """Lane classes 16 / 32 / 64 at one, two and three waves, hard and soft rows, shared pieces, an input-only unit and a
    saturated one in ONE call: every unit bit for bit its own closed_loop_plant_mpc; reversed and as a subset every unit keeps
    its bits, scores included; harness.mpc_loop_multi returns the bits of the raw context call."""
    from nys_koop_lqr_amd import harness
    plant, units, res = duffing["plant"], duffing["units"], duffing["res"]
    assert [(u["ctl"].nv, getattr(u["ctl"], "ny", 0)) for u in units] == [(8, 8), (8, 9), (32, 32), (8, 8), (8, 0), (8, 8), (8, 16)]
    assert [u["reg"]._landmark_shape()[1] for u in units] == [20, 65, 130, 20, 20, 20, 20]
    _assert_units_equal_singles(units, res, duffing["singles"], "mixed")
    assert not np.array_equal(res[2][0], res[2][3]) and not np.array_equal(res[2][0], res[2][4])
    _assert_replay(plant, res[1][2].T, res[2][2].T)
    u_opt, rows = duffing["u_opt"], duffing["rows"]
    for label, order in (("reversed", [6, 5, 4, 3, 2, 1, 0]), ("subset", [3, 5, 0, 2])):
        sub = _run(nk, plant, [units[k] for k in order], u_opt=u_opt, rows=[rows[k] for k in order])
        for a in range(4):
            assert np.array_equal(sub[a], res[a][order]), (label, a)
    h = harness.mpc_loop_multi([u["reg"] for u in units], [u["ctl"] for u in units], np.stack([u["x0"] for u in units]),
                               np.stack([u["ref"] for u in units]), STEPS, plant, iters=[u["iters"] for u in units],
                               tol=[u["tol"] for u in units],
                               u_inits=np.stack([np.zeros(1) if u["u_init"] is None else u["u_init"] for u in units]),
                               u_opt=u_opt, uopt_rows=rows, return_trajectories=True, return_info=True)
    assert np.array_equal(h["states"], res[1]) and np.array_equal(h["controls"], res[2]) and np.array_equal(h["info"], res[3])
    assert np.array_equal(np.stack([h[name] for name in harness.MPC_OUT_SCORE_NAMES], axis=1), res[0])


def test_scores(nk, duffing):
    """All ten scores against harness.mpc_out_scores of the returned trajectories, bit for bit, u_opt rows shared, distinct and
    absent.  Preconditions on the host loop (no GPU): the soft unit leaves its limits, the unit with bounds of +-100 never does.
    The input-only unit has zeros in the two new scores and its first eight are nk_mpc_loop_multi's."""
    from nys_koop_lqr_amd import harness
    plant, units, res, u_opt, rows = duffing["plant"], duffing["units"], duffing["res"], duffing["u_opt"], duffing["rows"]
    names = harness.MPC_OUT_SCORE_NAMES
    for k in (1, 6):
        u = units[k]
        S, U, I = harness.mpc_control_plant(STEPS, u["ref"], u["x0"], u["reg"], u["ctl"], plant.update_SOM, iters=u["iters"],
                                            tol=u["tol"])
        h = harness.mpc_out_scores(S, U, I, u["ctl"])
        print(f"\n[host loop, unit {k}] y_viol_max = {h['y_viol_max']:.6g}, n_y_viol = {h['n_y_viol']:.0f}")
        if k == 1:
            assert h["y_viol_max"] > 0 and h["n_y_viol"] > 0
        else:
            assert h["y_viol_max"] == 0.0 and h["n_y_viol"] == 0.0
    for k in range(len(units)):
        print(f"[unit {k}] " + ", ".join(f"{n} = {v:.6g}" for n, v in zip(names, res[0][k])))
    assert np.array_equal(res[0], _host_scores(units, res, u_opt, rows))
    assert np.all(res[0][np.array(rows) < 0][:, :2] == 0.0) and np.all(res[0][np.array(rows) >= 0][:, 1] > 0.0)
    yv, ny = names.index("y_viol_max"), names.index("n_y_viol")
    assert res[0][1, yv] > 0 and res[0][1, ny] > 0 and res[0][6, yv] == 0.0 and res[0][6, ny] == 0.0
    assert np.all(res[0][[4, 5], yv:] == 0.0)
    from nys_koop_lqr_amd import _lib
    ds, keep = _lib.mpc_desc(units[4]["ctl"], 25, 0.0)  # the eight scores of nk_mpc_loop_multi for the input-only unit
    sc8 = nk.get_context().mpc_loop_multi(plant.descriptor(), STEPS, [units[4]["reg"]._ensure_model()], [ds], X0.reshape(1, 2),
                                          REF.reshape(1, 2))[0]
    del keep
    assert sc8.shape == (1, 8) and np.array_equal(res[0][4, :8], sc8[0])


def test_absent_outputs(nk, duffing):
    """Each of out_x, out_u, out_info and scores may be absent: the others keep their bits.  All four absent is an error."""
    plant, units, res, u_opt, rows = duffing["plant"], duffing["units"], duffing["res"], duffing["u_opt"], duffing["rows"]
    for want in ((False, False, False, True), (False, True, True, True), (True, False, True, True), (True, True, False, True),
                 (True, True, True, False)):
        part = _run(nk, plant, units, u_opt=u_opt, rows=rows, want=want)
        for a in range(4):
            o = (3, 0, 1, 2)[a]  # `want` is (x, u, info, scores), the result (scores, x, u, info)
            if want[o]:
                assert np.array_equal(part[a], res[a]), (want, a)
            else:
                assert part[a] is None
    with pytest.raises(ValueError, match="all null"):
        _run(nk, plant, units, want=(False, False, False, False))


def test_kernel_families_two_inputs(nk):
    """P2 (d = 2, p = 2: the shifts of D by two lanes among the input lanes, beside output lanes) at m = 50 with an RBF kernel,
    a linear kernel and a spline model (no fold: [F; T] is read transposed), lane classes 16 and 32, rows from no fit
    (_synthetic_output_controller), each beside its input-only controller: bit for bit the single calls."""
    from nys_koop_lqr_amd import harness
    plant = make_plant("P2")
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    idx = np.random.default_rng(1).choice(2000, 50, False)
    units = []
    for k, (kind, N, ny) in enumerate((("rbf", 4, 5), ("linear", 8, 7), ("spline", 8, 16))):
        if kind == "spline":
            reg = nk.KoopmanSplineRegressor(2, m=50, gamma=1e-6)
            reg.centers = np.ascontiguousarray(Y.T[:, idx])
        else:
            kern = nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2) if kind == "rbf" else nk.LinearKernelWrapper(1.0)
            reg = nk.KoopmanNystromRegressor(2, kernel=kern, gamma=1e-6, m=50)
            reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
        reg.fit(X, Y)
        ctl = _synthetic_output_controller(np.random.default_rng(40 + k), 50, 2, 2, N, ny, 0.05)
        units += [_unit(reg, ctl, 20, [0.5, 0.5], [0.1, -0.1]), _unit(reg, ctl.input_only(), 20, [0.3, -0.4], [0.0, 0.0])]
    res = _run(nk, plant, units)
    _assert_units_equal_singles(units, res, [_single(plant, u) for u in units], "families")
    assert np.array_equal(res[0], _host_scores(units, res, None, [-1] * len(units)))


def test_four_inputs_at_the_landmark_limit(nk):
    """P4b (d = 4, p = 4): nt = 64 at m = nk_mpc_loop_max_m(64) = 314 (five waves) beside a small unit (nt = 12, one wave)."""
    plant = make_plant("P4b")
    big, _ = _limit_model(nk, 4, 4, 314)
    small, _ = _limit_model(nk, 4, 4, 40)
    units = [_unit(big, _synthetic_output_controller(np.random.default_rng(5), 314, 4, 4, 8, 32, 0.05), 30, 0.5 * np.ones(4),
                   np.zeros(4)),
             _unit(small, _synthetic_output_controller(np.random.default_rng(6), 40, 4, 4, 2, 4, 0.05), 30, 0.4 * np.ones(4),
                   0.1 * np.ones(4))]
    res = _run(nk, plant, units, steps=40)
    _assert_units_equal_singles(units, res, [_single(plant, u, 40) for u in units], "P4b")
    assert np.array_equal(res[0], _host_scores(units, res, None, [-1, -1]))


def test_nan_x0_in_one_unit(nk, duffing):
    """A NaN x0 in the soft unit: NaN controls, info {iters, NaN}, NaN u_absmax, J, r_max and y_viol_max, n_y_viol = 0; the
    other units keep their bits, scores included."""
    from nys_koop_lqr_amd import harness
    plant, units, res = duffing["plant"], duffing["units"], duffing["res"]
    mixed = list(units)
    mixed[1] = dict(units[1], x0=np.array([np.nan, 0.0]))
    got = _run(nk, plant, mixed, u_opt=duffing["u_opt"], rows=duffing["rows"])
    keep = [0, 2, 3, 4, 5, 6]
    for a in range(4):
        assert np.array_equal(got[a][keep], res[a][keep]), a
    sc = dict(zip(harness.MPC_OUT_SCORE_NAMES, got[0][1]))
    print("\n[NaN x0] " + ", ".join(f"{n} = {v!r}" for n, v in sc.items()))
    assert np.all(np.isnan(got[2][1])) and np.all(got[3][1][:, 0] == 100.0) and np.all(np.isnan(got[3][1][:, 1]))
    for name in ("u_absmax", "J", "r_max", "y_viol_max"):
        assert np.isnan(sc[name]), name
    assert sc["n_y_viol"] == 0.0 and sc["iters_sum"] == 100.0 * STEPS
    assert np.array_equal(got[0][1], _host_scores(mixed, got, duffing["u_opt"], duffing["rows"])[1], equal_nan=True)


def test_rejected_before_any_launch(nk, duffing):
    """A malformed output description, description or unit in a unit that is not the first: NK_ERR_BAD_ARG, the unit index and
    the field in nk_last_error(), and guard values in all four outputs untouched; the call works afterwards."""
    from nys_koop_lqr_amd import _lib
    plant, units = duffing["plant"], duffing["units"]
    reg, ctl = units[0]["reg"], units[0]["ctl"]
    ctx = nk.get_context()
    xs, xr = np.stack([X0, X0]), np.stack([REF, REF])
    ox, ou, oi, sc = np.full((2, 11, 2), 7.0), np.full((2, 10, 1), 7.0), np.full((2, 10, 2), 7.0), np.full((2, 10), 7.0)
    good_ds, keep_ds = _lib.mpc_desc(ctl, 20, 0.0)
    good_out, keep_out = _lib.mpc_out(ctl)

    def call(needle, c=ctl, iters=20, null=(), handle=None, pl=plant, **second):
        """two units on the first model; the second has controller c, `iters`, nulled fields of its nk_mpc_out and `second`"""
        h = reg._ensure_model() if handle is None else handle
        ds, keep = _lib.mpc_desc(c, iters, 0.0)
        out, keep2 = _lib.mpc_out(c)
        for f in null:
            setattr(out, f, None)
        arr = (_lib.MpcUnit * 2)()
        for i, (hh, dd) in enumerate(((reg._ensure_model(), good_ds), (h, ds))):
            arr[i].model, arr[i].desc = hh.value if isinstance(hh, C.c_void_p) else hh, C.pointer(dd)
            arr[i].x0, arr[i].x_ref, arr[i].uopt = xs[i].ctypes.data, xr[i].ctypes.data, -1
        for name, v in second.items():
            setattr(arr[1], name, v)
        oarr = (C.POINTER(_lib.MpcOut) * 2)(C.pointer(good_out), C.pointer(out))
        rc = ctx.lib.nk_mpc_out_loop_multi(ctx.handle, C.byref(pl.descriptor()), 10, arr, oarr, 2, None, 0, ox.ctypes.data,
                                           ou.ctypes.data, oi.ctypes.data, sc.ctypes.data)
        msg = ctx.lib.nk_last_error().decode()
        assert rc == -1 and "nk_mpc_out_loop_multi" in msg and all(part in msg for part in needle), (rc, msg, needle)
        del keep, keep2

    def at(a, i, v):
        b = np.array(a, dtype=np.float64)
        b.flat[i] = v
        return b

    call(["unit 1", "ylo[2]"], _with_outputs(ctl, ylo=at(ctl.ylo, 2, ctl.yhi[2] + 1.0)))
    yc = ctl.ycomp.copy()
    yc[3] = 2  # the plant has two states
    call(["unit 1", "ycomp[3]"], _with_outputs(ctl, ycomp=yc))
    for w in (0.0, float("nan")):
        c = _with_outputs(ctl)
        c.y_weight = w
        call(["unit 1", "y_weight"], c)
    call(["unit 1", "G is null"], null=("G",))
    wide = _with_outputs(ctl, G=np.zeros((57, 8)), T=np.zeros((57, 20)), ylo=np.full(57, -1.0), yhi=np.full(57, 1.0),
                         ycomp=np.zeros(57, dtype=np.int32))
    call(["unit 1", "ny = 57"], wide)
    call(["unit 1", "iters"], iters=0)  # rows with the saturated LQR
    lo = ctl.lo.copy()
    lo[5] = ctl.hi[5] + 1.0
    call(["unit 1", "lo[5]"], _with_outputs(ctl, lo=lo))
    call(["unit 1", "reserved"], reserved=1)
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(oi == 7.0) and np.all(sc == 7.0)  # nothing ran
    del keep_ds, keep_out
    # one landmark past nk_mpc_loop_max_m(nv + ny): four states and inputs, nv = 32 alone would admit m = 315
    p4 = make_plant("P4b")
    assert ctx.lib.nk_mpc_loop_max_m(64) == 314 and ctx.lib.nk_mpc_loop_max_m(32) >= 315
    small, _ = _limit_model(nk, 4, 4, 40)
    over, _ = _limit_model(nk, 4, 4, 315, spline=True)
    pair = [_unit(small, _synthetic_output_controller(np.random.default_rng(6), 40, 4, 4, 2, 4, 0.05), 30, 0.4 * np.ones(4),
                  np.zeros(4)),
            _unit(over, _synthetic_output_controller(np.random.default_rng(5), 315, 4, 4, 8, 32, 0.05), 30, 0.5 * np.ones(4),
                  np.zeros(4))]
    with pytest.raises(ValueError, match="unit 1.*at most 314"):
        _run(nk, p4, pair, steps=10)
    res = _run(nk, plant, units[:2], steps=10)  # and the call still works
    assert np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[1]))


def test_sweep(nk):
    """harness.lqr_sweep(controller=dict(horizon=8, u_min, u_max, x_min, x_max, rho, iters)) on the Duffing data of `fits`,
    2 seeds x ms = (20, 65): the ten tables and the trajectories equal those of the units run one by one (fit -> solve_mpc ->
    closed_loop_plant_mpc -> mpc_out_scores), bit for bit."""
    from nys_koop_lqr_amd import harness
    plant = nk.PolynomialSystem.duffing(0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    params = dict(kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6)
    ms, seeds = (20, 65), (0, 1)
    plan = harness.lqr_plan(X, Y, 1, params, ms, seeds, "nystrom")
    rho = RHO_FACTOR * harness.lqr_fit_unit(X, Y, 1, params, plan[0], "nystrom").solve_mpc(8, c=1.0).rho
    u_opt = _u_opt(1, STEPS, 1)[0]
    spec = dict(horizon=8, u_min=-U_MAX, u_max=U_MAX, x_min=[-np.inf, -0.5], x_max=[np.inf, 0.5], rho=rho, iters=50)
    res = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, X0, REF, STEPS, u_opt=u_opt, batch=4, workers=2,
                            return_trajectories=True, controller=spec)
    assert set(harness.MPC_OUT_SCORE_NAMES) <= set(res) and res["y_viol_max"].shape == (2, 2)
    assert np.all(np.isfinite(res["y_viol_max"])) and np.any(res["n_iterated"] > 0)
    for u in plan:
        si, k = u["si"], u["k"]
        reg = harness.lqr_fit_unit(X, Y, 1, params, u, "nystrom")
        ctl = reg.solve_mpc(8, c=1.0, u_min=-U_MAX, u_max=U_MAX, x_min=[-np.inf, -0.5], x_max=[np.inf, 0.5], rho=rho)
        assert ctl.ny == 8
        s, c, i = reg.closed_loop_plant_mpc(ctl, X0, REF, STEPS, plant, iters=50, return_info=True)
        assert np.array_equal(res["states"][si, k], s.T) and np.array_equal(res["controls"][si, k], c.T), (si, k)
        host = harness.mpc_out_scores(s, c, i, ctl, u_opt)
        print(f"\n[sweep, seed {si}, m = {u['m']}] peak |x_2| {np.max(np.abs(s[1])):.4f}, y_viol_max {host['y_viol_max']:.3e}, "
              f"n_y_viol {host['n_y_viol']:.0f}")
        for name in harness.MPC_OUT_SCORE_NAMES + ("rmse_control",):
            assert res[name][si, k] == host[name], (name, si, k)
