"""GPU: the multi-model plant loop scored on the device (nk_plant_loop_multi, harness.plant_loop_multi): every unit of a
call against the single-model launch it replaces (KoopmanNystromRegressor.closed_loop_plant -> nk_plant_loop) bit for bit --
whatever else the call holds, in whatever order, across kernel families, model kinds and workgroup shapes --, the four
device scores against the host loop over the same states and controls, the reference's recorded HJB run, a diverging
unit among healthy ones, and the argument checks.  300 steps unless stated, at most 7 units per call."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_plant_loop import _duffing_case, _hjb_case, _snapshots

pytestmark = pytest.mark.gpu

STEPS = 300
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def duffing(nk, golden):
    """f12 seeds 0..2 (m = 20) rebuilt from host copies, with their own gains, and the seed-0 model a second time from
    another state towards another reference: units of (regressor, gain, x0, x_ref)."""
    cs = [_duffing_case(nk, golden, s) for s in (0, 1, 2)]
    units = [(c["reg"], c["K"], c["x0"], c["ref"]) for c in cs]
    units.append((cs[0]["reg"], cs[0]["K"], np.array([0.4, -0.3]), np.array([0.05, 0.0])))
    return dict(plant=cs[0]["plant"], units=units)


@pytest.fixture(scope="module")
def hjb(nk, golden):
    c = _hjb_case(nk, golden)
    return dict(case=c, plant=c["plant"], units=[(c["reg"], c["K"], c["x0"], c["ref"]), (c["reg"], 0.5 * c["K"], c["x0"], c["ref"])])


def _alone(unit, steps, plant):
    """The single-model call: states (steps + 1, d), controls (steps,)."""
    reg, K, x0, ref = unit
    states, us = reg.closed_loop_plant(K, x0, ref, steps, plant)
    return np.ascontiguousarray(states.T), np.ascontiguousarray(us[0])


def _multi(units, steps, plant, **kw):
    from nys_koop_lqr_amd import harness
    return harness.plant_loop_multi([u[0] for u in units], [u[1] for u in units], np.stack([u[2] for u in units]),
                                    np.stack([u[3] for u in units]), steps, plant, return_trajectories=True, **kw)


def _assert_units_equal_alone(units, alone, steps, plant):
    res = _multi(units, steps, plant)
    d = units[0][2].size
    assert res["states"].shape == (len(units), steps + 1, d) and res["controls"].shape == (len(units), steps)
    for i, (s, u) in enumerate(alone):
        assert np.array_equal(res["states"][i], s, equal_nan=True), i  # (a unit that diverges does so in both calls)
        assert np.array_equal(res["controls"][i], u, equal_nan=True), i
    return res


@pytest.mark.parametrize("which", ["duffing", "hjb"])
def test_every_unit_is_the_single_call_bit_for_bit(which, duffing, hjb):
    """Duffing: three models with their own gains and one of them twice; HJB (m = 200, one wave at four landmarks per lane):
    one model under the gains K and K / 2.  States and controls of every unit equal closed_loop_plant on that model alone;
    again with the unit order reversed, and with one unit alone in its call."""
    cfg = duffing if which == "duffing" else hjb
    units, plant = cfg["units"], cfg["plant"]
    alone = [_alone(u, STEPS, plant) for u in units]
    assert all(np.all(np.isfinite(s)) and np.all(np.isfinite(u)) for s, u in alone)
    assert not np.array_equal(alone[0][1], alone[-1][1])  # the units differ: equality below is not vacuous
    _assert_units_equal_alone(units, alone, STEPS, plant)
    _assert_units_equal_alone(units[::-1], alone[::-1], STEPS, plant)
    for i in (0, len(units) - 1):
        _assert_units_equal_alone([units[i]], [alone[i]], STEPS, plant)


def test_mixed_classes_in_one_call(nk):
    """Five launch classes in one call on the Duffing plant: Matern m = 20 (one landmark per lane), RBF m = 50, linear
    m = 50, Matern m = 300 (two waves: the LDS reduction) and a thin-plate-spline model at m = 70 (four landmarks per lane,
    no fold).  Fits on 2000 snapshot pairs, gains from solve_lqr.  Each unit is its own closed_loop_plant bit for bit: a
    wrong table index, class sort or output offset shows here."""
    rng = np.random.default_rng(11)
    plant = nk.DuffingOscillator(Ts=0.01)
    X, Y = _snapshots(plant, 2000, rng)
    kinds = [("matern", 20), ("rbf", 50), ("linear", 50), ("matern", 300), ("spline", 70)]
    units = []
    for k, (kind, m) in enumerate(kinds):
        idx = rng.choice(2000, m, replace=False)
        if kind == "spline":
            reg = nk.KoopmanSplineRegressor(1, m=m, gamma=1e-6)
            reg.centers = np.ascontiguousarray(Y.T[:, idx])
        else:
            kern = {"matern": nk.KernelWrapper([1, 1]), "rbf": nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2),
                    "linear": nk.LinearKernelWrapper(1.0)}[kind]
            reg = nk.KoopmanNystromRegressor(1, kernel=kern, gamma=1e-6, m=m)
            reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
        reg.fit(X, Y)
        K = reg.solve_lqr(c=1.0)
        units.append((reg, K, np.array([-0.5 + 0.1 * k, 0.05 * k]), np.array([0.01 * k, 0.0])))
    alone = [_alone(u, STEPS, plant) for u in units]
    for (kind, m), (s, u) in zip(kinds, alone):
        print(f"\n[{kind}, m = {m}] max |u| {np.max(np.abs(u)):.3e}, final state {s[-1]}")
    res = _assert_units_equal_alone(units, alone, STEPS, plant)
    _assert_units_equal_alone(units[::-1], alone[::-1], STEPS, plant)
    assert np.array_equal(res["u_absmax"], [np.max(np.abs(u)) for _, u in alone], equal_nan=True)


def _host_scores(states, us, uo):
    """The four scores from one unit's states (steps + 1, d) and controls on the host: J and u_absmax by the device's own
    operations; the terms of the two sums with the device's subtraction and square, summed exactly (math.fsum)."""
    from nys_koop_lqr_amd import harness
    sc = harness.control_scores(states.T, us, uo)
    if uo is None:
        return sc, 0.0, 0.0
    df = us - uo
    return sc, math.fsum(df * df), math.fsum(uo * uo)


@pytest.mark.parametrize("which", ["duffing", "hjb"])
def test_scores(nk, which, duffing, hjb):
    """J (the running cost of open_loop_control, same operations in the same order) and u_absmax equal the host loop over the
    states and controls of the SAME call; sse_u and ss_opt are sums of `steps` non-negative terms accumulated in step order:
    each partial sum is rounded once, so the result is within steps * eps of the exact sum of the same terms, relative --
    held against math.fsum within 2 (steps + 1) eps.  With out_x = out_u = NULL the scores have the same bits, and a unit
    with uopt = -1 reports zeros in the first two slots."""
    cfg = duffing if which == "duffing" else hjb
    units, plant = cfg["units"], cfg["plant"]
    n = len(units)
    rng = np.random.default_rng(5)
    t = np.arange(STEPS)
    u_opt = np.stack([0.3 * np.exp(-t / 80.0) * np.cos(t / 9.0), 0.05 * rng.standard_normal(STEPS)])
    rows = [0, 1, -1, 0][:n] if n > 2 else [1, -1]
    ctx = nk.get_context()
    args = (plant.plant_id, plant.Ts, STEPS, [u[0]._ensure_model() for u in units], [u[1] for u in units],
            np.stack([u[2] for u in units]), np.stack([u[3] for u in units]))
    sc, ox, ou = ctx.plant_loop_multi(*args, u_opt=u_opt, uopt_rows=rows, want_x=True, want_u=True)
    assert sc.shape == (n, 4) and ox.shape == (n, STEPS + 1, units[0][2].size) and ou.shape == (n, STEPS)
    bound = 2 * (STEPS + 1) * EPS
    for i in range(n):
        uo = None if rows[i] < 0 else u_opt[rows[i]]
        host, sse, sso = _host_scores(ox[i], ou[i], uo)
        print(f"\n[{which} unit {i}, uopt {rows[i]}] device {sc[i].tolist()} host J {host['J']!r} u_absmax {host['u_absmax']!r} "
              f"fsum sse {sse!r} ss_opt {sso!r}")
        assert sc[i, 2] == host["J"] and sc[i, 3] == host["u_absmax"] == np.max(np.abs(ou[i])), i
        if uo is None:
            assert sc[i, 0] == 0.0 and sc[i, 1] == 0.0
        else:
            assert sc[i, 0] > 0 and sc[i, 1] > 0
            assert abs(sc[i, 0] - sse) <= bound * sse and abs(sc[i, 1] - sso) <= bound * sso, i
    # scores only: nothing but 4 numbers per unit leaves the device, and they are the same bits
    sc_only, ox2, ou2 = ctx.plant_loop_multi(*args, u_opt=u_opt, uopt_rows=rows)
    assert ox2 is None and ou2 is None and np.array_equal(sc_only, sc)
    # one of the two trajectories only
    sc_x, ox3, ou3 = ctx.plant_loop_multi(*args, u_opt=u_opt, uopt_rows=rows, want_x=True)
    assert ou3 is None and np.array_equal(ox3, ox) and np.array_equal(sc_x, sc)
    _, ox4, ou4 = ctx.plant_loop_multi(*args, want_u=True, want_scores=False)
    assert ox4 is None and np.array_equal(ou4, ou)
    # no u_opt at all: the cost and the maximum are unchanged
    sc_no, _, _ = ctx.plant_loop_multi(*args)
    assert np.all(sc_no[:, :2] == 0.0) and np.array_equal(sc_no[:, 2:], sc[:, 2:])


def test_hjb_control_rmse_against_the_recorded_run(nk, golden, hjb):
    """f8, 400 steps from 0.9: u_opt from harness.hjb_optimal_control, rmse_control reduced on the device, against the value
    the reference's recorded controls cl_u give.  The existing test holds the device controls to 1e-5 relative (Frobenius)
    of cl_u; by the triangle inequality ||u - u_opt|| then moves by at most 1e-5 ||cl_u||, so the two RMSE values (100 ||u -
    u_opt|| / ||u_opt||) differ by at most 100 * 1e-5 * ||cl_u|| / ||u_opt||."""
    from nys_koop_lqr_amd import harness
    g = golden("f8_hjb_config2.npz")
    c = hjb["case"]
    steps = c["steps"]
    u_opt, J_true = harness.hjb_optimal_control(c["x0"], steps, c["plant"])
    res = harness.plant_loop_multi([c["reg"]], [c["K"]], c["x0"], c["ref"], steps, c["plant"], u_opt=u_opt)
    want = harness.control_rmse_percent(g["cl_u"], u_opt)
    bar = 100.0 * 1e-5 * np.linalg.norm(g["cl_u"]) / np.linalg.norm(u_opt)
    print(f"\nrmse_control: device {res['rmse_control'][0]!r}, from the recorded controls {want!r} (recorded by the reference: "
          f"{float(g['rmse_control'])!r}); bar {bar:.3e}; J {res['J'][0]!r} (optimal {J_true!r})")
    assert "states" not in res and res["rmse_control"].shape == (1,)
    assert abs(res["rmse_control"][0] - want) <= bar
    assert np.isfinite(res["J"][0]) and res["u_absmax"][0] == np.max(np.abs(
        _alone((c["reg"], c["K"], c["x0"], c["ref"]), steps, c["plant"])[1]))


def test_a_diverging_unit_does_not_disturb_the_others(duffing):
    """A gain scaled until the loop leaves the state bounds and goes non-finite (fixed-trip-count arithmetic on inf / NaN):
    its u_absmax is NaN or inf, and its neighbours in the same call keep the bits they have without it."""
    units, plant = duffing["units"][:3], duffing["plant"]
    reg, K, x0, ref = units[1]
    bad = None
    for scale in (1e4, 1e8, 1e12):
        s, u = _alone((reg, scale * K, x0, ref), STEPS, plant)
        if not (np.all(np.isfinite(s)) and np.all(np.isfinite(u))):
            bad = (reg, scale * K, x0, ref)
            print(f"\ngain scale {scale:g}: first non-finite control at step {int(np.argmax(~np.isfinite(u)))}")
            break
    if bad is None:
        bad = (reg, -K, x0, ref)
    mixed = [units[0], bad, units[2]]
    alone = [_alone(u, STEPS, plant) for u in mixed]
    res = _multi(mixed, STEPS, plant)
    assert not np.isfinite(res["u_absmax"][1]), res["u_absmax"]
    for i in (0, 2):
        assert np.array_equal(res["states"][i], alone[i][0]) and np.array_equal(res["controls"][i], alone[i][1])
        assert np.isfinite(res["u_absmax"][i]) and np.isfinite(res["J"][i])
    assert np.array_equal(res["states"][1], alone[1][0], equal_nan=True)
    healthy = _multi([units[0], units[2]], STEPS, plant)
    for name in ("J", "u_absmax"):
        assert np.array_equal(healthy[name], res[name][[0, 2]])


def test_argument_checks(nk, golden, duffing, hjb):
    """Each bad call returns NK_ERR_BAD_ARG, names the unit where there is one, and writes nothing."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    lib = ctx.lib
    plant = duffing["plant"]
    good = duffing["units"][:2]
    rng = np.random.default_rng(3)
    reg2 = nk.KoopmanNystromRegressor(2, kernel=nk.KernelWrapper([1, 1]), gamma=1e-6, m=8)  # two inputs
    reg2.nystrom_centers_output = rng.uniform(-1, 1, size=(2, 8))
    hreg, hK = hjb["units"][0][0], hjb["units"][0][1]  # one state on a two-state plant
    steps = 10
    ox, ou, sc = np.full((2, steps + 1, 2), 7.0), np.full((2, steps), 7.0), np.full((2, 4), 7.0)
    u_opt = np.zeros((1, steps))
    keep = []

    def table(units, uopt=(-1, -1)):
        arr = (_lib.PlantUnit * len(units))()
        for i, (reg, K, x0, ref) in enumerate(units):
            K, x0, ref = (np.ascontiguousarray(a, dtype=np.float64) for a in (K, x0, ref))
            keep.extend((K, x0, ref))
            arr[i].model = reg._ensure_model().value
            arr[i].K, arr[i].x0, arr[i].x_ref, arr[i].uopt = K.ctypes.data, x0.ctypes.data, ref.ctypes.data, uopt[i]
        return arr

    def call(handle, arr, n, n_uopt=1, outs=(ox, ou, sc)):
        px, pu, ps = (None if o is None else o.ctypes.data for o in outs)
        rc = lib.nk_plant_loop_multi(handle, plant.plant_id, plant.Ts, steps, arr, n, u_opt.ctypes.data if n_uopt else None,
                                     n_uopt, px, pu, ps)
        return rc, lib.nk_last_error()

    x0, ref = good[0][2], good[0][3]
    rc, msg = call(ctx.handle, table([good[0], (reg2, np.zeros((2, 8)), x0, ref)]), 2)
    assert rc == -1 and b"unit 1" in msg and b"one input" in msg, (rc, msg)
    rc, msg = call(ctx.handle, table([good[0], (hreg, hK, x0, ref)]), 2)
    assert rc == -1 and b"unit 1" in msg and b"2 states" in msg, (rc, msg)
    rc, msg = call(ctx.handle, table(good, uopt=(0, 1)), 2)
    assert rc == -1 and b"unit 1" in msg and b"uopt" in msg, (rc, msg)
    rc, msg = call(ctx.handle, table(good, uopt=(0, -1)), 2, n_uopt=0)  # a row of a u_opt that is not there
    assert rc == -1 and b"unit 0" in msg, (rc, msg)
    rc, msg = call(ctx.handle, table(good), 2, outs=(None, None, None))
    assert rc == -1 and b"null" in msg, (rc, msg)
    rc, msg = call(ctx.handle, table(good), 0)
    assert rc == -1 and b"n_units" in msg, (rc, msg)
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(sc == 7.0)  # nothing was written by any refused call
    rc, msg = call(ctx.handle, table(good), 2)  # sanity: the same table is accepted ...
    assert rc == 0, (rc, msg)
    assert not np.any(ox == 7.0) and not np.any(ou == 7.0) and not np.any(sc == 7.0)
    ox[:], ou[:], sc[:] = 7.0, 7.0, 7.0
    handles = (C.c_void_p * 2)()
    _lib.check(lib.nk_group_create(ctx.device, 2, handles))
    members = [_lib.Context(ctx.device, C.c_void_p(handles[i])) for i in range(2)]
    try:
        rc, msg = call(members[0].handle, table(good), 2)  # ... but not from a lock-step member
        assert rc == -1 and b"lock-step" in msg, (rc, msg)
    finally:
        for mem in members:
            mem.close()
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(sc == 7.0)
    # the Python layer turns the code into ValueError, and the call still works afterwards
    with pytest.raises(ValueError, match="unit 1"):
        _multi([good[0], (hreg, hK, x0, ref)], steps, plant)
    res = _multi(good, steps, plant)
    assert np.all(np.isfinite(res["states"])) and np.all(np.isfinite(res["J"]))
