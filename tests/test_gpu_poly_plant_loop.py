"""GPU: the plant-in-the-loop closed loop around a polynomial plant the user describes (nk_poly_plant_loop and its multi form;
PolynomialSystem through closed_loop_plant, harness.plant_loop_multi and harness.lqr_sweep).  Every state the device
returns is replayed on the host bit for bit (nk_poly_plant_step); the Duffing and HJB tables run the reference's recorded
configurations; device loops against the host loop (a lift per step) for two to four states, one to four inputs, one and
two waves, every kernel family and the class limits on m; batch invariance; the multi form and its scores; argument checks;
the control sweep."""
import ctypes as C

import numpy as np
import pytest

from conftest import relf
from test_gpu_plant_loop import _cases, _device_vs_host
from test_poly_plant_host import PLANTS, make_plant

pytestmark = pytest.mark.gpu

STEPS = 200
LIMITS = {(1, 1): 4096, (4, 4): 1024}  # include/nyskoop.h: the class limits on m the tests below run at


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def fits(nk):
    """fits(name, m) -> (plant, regressor, gain): Matern-5/2 with length scales 1, gamma = 1e-6, 2000 snapshot pairs from
    default_rng(7) uniform in [-1, 1], landmarks default_rng(1).choice(2000, m, False), Ts = 0.01 with classical RK4, gain
    from Q = sym(C'C), R = I by the host Riccati solve.  Fitted once per (name, m) and left unchanged."""
    from nys_koop_lqr_amd import harness
    cache = {}

    def get(name, m):
        if (name, m) not in cache:
            plant = make_plant(name) if name in PLANTS else nk.PolynomialSystem.duffing(0.01)
            d, p = plant.n_states, plant.n_inputs
            X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
            idx = np.random.default_rng(1).choice(2000, m, False)
            reg = nk.KoopmanNystromRegressor(p, kernel=nk.KernelWrapper([1.0] * d), gamma=1e-6, m=m)
            reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
            reg.fit(X, Y)
            cache[(name, m)] = (plant, reg, np.ascontiguousarray(reg.solve_lqr(c=1.0)))
        return cache[(name, m)]

    return get


def _assert_replay(plant, states, us):
    """states (d, steps + 1), controls (p, steps) of one device loop: x_{t+1} is nk_poly_plant_step(x_t, u_t) on the host, bit
    for bit, at every step (no tolerance: the plant evaluation and the stores)."""
    assert states.shape[1] == us.shape[1] + 1 and np.all(np.isfinite(states)) and np.all(np.isfinite(us))
    for t in range(us.shape[1]):
        want = plant.step_library(states[:, t], us[:, t])
        assert np.array_equal(states[:, t + 1], want), (t, states[:, t + 1], want)


def test_tables_of_the_built_in_plants_vs_reference_and_built_in(nk, golden):
    """f12 (Duffing, seeds 0..2, 2000 steps) and f8 (HJB, 400 steps) with the reference's landmarks, operators and gain, the
    loop around PolynomialSystem.duffing / .hjb: controls and states against the reference's recorded run under the bars of
    the built-in plants' test, every state replayed on the host bit for bit, and the distance to the built-in kernels on the
    same model printed (by the triangle inequality at most the two bars added)."""
    for name, c in _cases(nk, golden):
        poly = nk.PolynomialSystem.duffing(0.01) if c["x0"].size == 2 else nk.PolynomialSystem.hjb(0.01)
        states, us = c["reg"].closed_loop_plant(c["K"], c["x0"], c["ref"], c["steps"], poly)
        d = c["x0"].size
        assert states.shape == (d, c["steps"] + 1) and us.shape == (1, c["steps"]) and np.array_equal(states[:, 0], c["x0"])
        _assert_replay(poly, states, us)
        T = c["states"].shape[1]
        e_u, e_x = relf(us, c["us"]), relf(states[:c["states"].shape[0], :T], c["states"])
        sb, ub = c["reg"].closed_loop_plant(c["K"], c["x0"], c["ref"], c["steps"], c["plant"])
        b_u, b_x = relf(us, ub), relf(states, sb)
        print(f"\n[{name}] polynomial table vs reference: controls {e_u:.2e} (bar {c['bar_u']:.2e}), states {e_x:.2e} "
              f"(bar {c['bar_x']:.2e}); vs the built-in plant: controls {b_u:.2e}, states {b_x:.2e}")
        assert e_u <= c["bar_u"] and e_x <= c["bar_x"], (name, e_u, e_x)
        assert b_u <= 2 * c["bar_u"] and b_x <= 2 * c["bar_x"], (name, b_u, b_x)


def _check_against_host_loop(nk, label, plant, reg, K, x0, steps=STEPS):
    """Device loop against harness.lqr_control_plant with plant.update_SOM from x0 to the origin: bar per quantity 10 x the
    host loop's own movement under a 1e-15 relative perturbation of K, floor 1e-10; and the host replay of every state."""
    ref = np.zeros(plant.n_states)
    states, us = reg.closed_loop_plant(K, x0, ref, steps, plant)
    assert states.shape == (plant.n_states, steps + 1) and us.shape == (plant.n_inputs, steps)
    _assert_replay(plant, states, us)
    (e_u, e_x), (s_u, s_x) = _device_vs_host(nk, reg, K, plant, x0, ref, steps)
    bar_u, bar_x = max(10.0 * s_u, 1e-10), max(10.0 * s_x, 1e-10)
    print(f"\n[{label}] device vs host loop: controls {e_u:.2e} (host loop moves {s_u:.2e}, bar {bar_u:.2e}), states "
          f"{e_x:.2e} (moves {s_x:.2e}, bar {bar_x:.2e}); max |x| {np.max(np.abs(states)):.2f}, max |u| {np.max(np.abs(us)):.2f}")
    assert e_u <= bar_u and e_x <= bar_x, (label, e_u, bar_u, e_x, bar_x)


@pytest.mark.parametrize("m", [40, 300])
@pytest.mark.parametrize("name", ["P2", "P3", "P4", "P4b"])
def test_device_loop_vs_host_loop(nk, fits, name, m):
    """m = 40: one wave, one landmark per lane; m = 300: two waves (P4b: five, at one landmark per lane).  200 steps from
    0.5 * ones to the origin."""
    plant, reg, K = fits(name, m)
    _check_against_host_loop(nk, f"{name}, m = {m}", plant, reg, K, 0.5 * np.ones(plant.n_states))


def test_duffing_table_m200(nk, fits):
    plant, reg, K = fits("duffing", 200)
    _check_against_host_loop(nk, "duffing table, m = 200", plant, reg, K, np.array([-0.5, 0.0]))


@pytest.mark.parametrize("kind", ["rbf", "linear", "spline"])
def test_other_kernel_families(nk, kind):
    """P2 at m = 50 with an RBF kernel, a linear kernel and a spline model (no fold: the gain is read transposed).  No Riccati
    solve in the way: u = G (x_ref - x) read through the model's own output map, K = G C with G = [[4, 2], [1, 0]], which
    stabilises the linearisation of P2 at the origin (x1' = x2 + 0.3 u2, x2' = x1 - 0.5 x2 + 0.5 u1)."""
    from nys_koop_lqr_amd import harness
    plant = make_plant("P2")
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    idx = np.random.default_rng(1).choice(2000, 50, False)
    if kind == "spline":
        reg = nk.KoopmanSplineRegressor(2, m=50, gamma=1e-6)
        reg.centers = np.ascontiguousarray(Y.T[:, idx])
    else:
        kern = nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2) if kind == "rbf" else nk.LinearKernelWrapper(1.0)
        reg = nk.KoopmanNystromRegressor(2, kernel=kern, gamma=1e-6, m=50)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
    reg.fit(X, Y)
    K = np.ascontiguousarray(np.array([[4.0, 2.0], [1.0, 0.0]]) @ np.asarray(reg.C))
    _check_against_host_loop(nk, f"P2 {kind}, m = 50", plant, reg, K, np.array([0.5, 0.5]))


def _limit_model(nk, d, p, m, spline=False):
    """A model of m landmarks without a fit (nk_model_create only recomputes K_mm^{-1/2}).  d = 1: a regular grid on [-1, 1]
    under a Matern kernel of length scale 4 grid steps (4096 random points on a line would nearly coincide); d = 4: uniform
    in [-1, 1]^4, length scales 1."""
    rng = np.random.default_rng(100 * d + p)
    Z = np.linspace(-1.0, 1.0, m).reshape(1, m) if d == 1 else rng.uniform(-1, 1, size=(d, m))
    if spline:
        reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
        reg.centers = np.ascontiguousarray(Z)
    else:
        ls = [8.0 / m] if d == 1 else [1.0] * d
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.KernelWrapper(ls), gamma=1e-6, m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Z)
    return reg, np.ascontiguousarray(1e-2 * rng.standard_normal((p, m)))


@pytest.mark.parametrize("d,p", [(4, 4), (1, 1)])
def test_class_limits(nk, d, p):
    """m at the documented limit of the class (16 waves): 50 steps against the host loop under the same bar; one landmark more
    is a ValueError (NK_ERR_BAD_ARG) that names the limit and leaves nothing running."""
    limit = LIMITS[(d, p)]
    plant = make_plant("P4b") if d == 4 else nk.PolynomialSystem.hjb(0.01)
    reg, K = _limit_model(nk, d, p, limit)
    _check_against_host_loop(nk, f"d = {d}, p = {p}, m = {limit}", plant, reg, K, 0.5 * np.ones(d), steps=50)
    reg1, K1 = _limit_model(nk, d, p, limit + 1, spline=True)
    with pytest.raises(ValueError, match=f"at most {limit}"):
        reg1.closed_loop_plant(K1, 0.5 * np.ones(d), np.zeros(d), 10, plant)


@pytest.mark.parametrize("m", [40, 300])
def test_batch_invariance(nk, fits, m):
    """P4 with 1, 7 and 64 initial states in one call: bit for bit what each state gives in a call of its own; and one
    reference shared by the batch."""
    plant, reg, K = fits("P4", m)
    steps = 100
    rng = np.random.default_rng(2024)
    X0 = rng.uniform(-0.5, 0.5, size=(64, 4))
    ref = rng.uniform(-0.05, 0.05, size=(64, 4))
    alone = [reg.closed_loop_plant(K, X0[i], ref[i], steps, plant) for i in range(64)]
    assert not np.array_equal(alone[0][1], alone[1][1])
    for batch in (1, 7, 64):
        S, U = reg.closed_loop_plant(K, X0[:batch], ref[:batch], steps, plant)
        assert S.shape == (batch, steps + 1, 4) and U.shape == (batch, steps, 2)
        for i in range(batch):
            assert np.array_equal(S[i], alone[i][0].T) and np.array_equal(U[i], alone[i][1].T), (batch, i)
    S, U = reg.closed_loop_plant(K, X0[:7], ref[0], steps, plant)
    S1, U1 = reg.closed_loop_plant(K, X0[3], ref[0], steps, plant)
    assert np.array_equal(S[3], S1.T) and np.array_equal(U[3], U1.T)
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(U))
    _assert_replay(plant, S1, U1)


def _p2_units(fits):
    """6 units over two models (m = 40: one wave; m = 300: two waves) on P2, in shuffled order."""
    plant, r40, K40 = fits("P2", 40)
    _, r300, K300 = fits("P2", 300)
    rng = np.random.default_rng(77)
    units = []
    for k in range(6):
        reg, K = ((r40, K40), (r300, K300))[k % 2]
        units.append((reg, (1.0 - 0.1 * k) * K, rng.uniform(-0.5, 0.5, 2), rng.uniform(-0.05, 0.05, 2)))
    return plant, [units[i] for i in (4, 1, 3, 0, 5, 2)]


def test_multi_form(nk, fits):
    """Every unit of the multi-model call is the single-model call with batch = 1 bit for bit, in either unit order; the four
    scores equal the host loop over the returned states and controls bit for bit (harness.control_scores: the sums over the
    inputs in index order), sse_u against a u_opt with p = 2 columns; with out_x = out_u = NULL the scores keep their bits,
    and with scores = NULL the trajectories keep theirs."""
    from nys_koop_lqr_amd import harness
    plant, units = _p2_units(fits)
    n, steps = len(units), STEPS
    alone = [u[0].closed_loop_plant(u[1], u[2], u[3], steps, plant) for u in units]
    t = np.arange(steps)
    u_opt = np.stack([np.stack([0.3 * np.exp(-t / 80.0) * np.cos(t / 9.0), 0.1 * np.sin(t / 7.0)], axis=1),
                      0.05 * np.random.default_rng(5).standard_normal((steps, 2))])
    rows = [0, 1, -1, 0, 1, 0]
    for order in (list(range(n)), list(range(n))[::-1]):
        us_ = [units[i] for i in order]
        res = harness.plant_loop_multi([u[0] for u in us_], [u[1] for u in us_], np.stack([u[2] for u in us_]),
                                       np.stack([u[3] for u in us_]), steps, plant, u_opt=u_opt,
                                       uopt_rows=[rows[i] for i in order], return_trajectories=True)
        assert res["states"].shape == (n, steps + 1, 2) and res["controls"].shape == (n, steps, 2)
        for k, i in enumerate(order):
            assert np.array_equal(res["states"][k], alone[i][0].T) and np.array_equal(res["controls"][k], alone[i][1].T), i
            host = harness.control_scores(alone[i][0], alone[i][1], None if rows[i] < 0 else u_opt[rows[i]])
            got = {name: res[name][k] for name in ("sse_u", "ss_opt", "J", "u_absmax")}
            print(f"\n[unit {i}, uopt {rows[i]}] sse_u {got['sse_u']!r} ss_opt {got['ss_opt']!r} J {got['J']!r} u_absmax {got['u_absmax']!r}")
            for name in got:
                assert got[name] == host[name], (i, name, got[name], host[name])
            assert (got["sse_u"] > 0 and got["ss_opt"] > 0) if rows[i] >= 0 else (got["sse_u"] == 0 and got["ss_opt"] == 0)
    # the last call (reversed order) again, scores only and trajectories only
    ctx = nk.get_context()
    args = (plant.descriptor(), steps, [u[0]._ensure_model() for u in us_], [u[1] for u in us_],
            np.stack([u[2] for u in us_]), np.stack([u[3] for u in us_]))
    kw = dict(u_opt=u_opt, uopt_rows=[rows[i] for i in order])
    sc, ox, ou = ctx.poly_plant_loop_multi(*args, **kw)
    assert ox is None and ou is None
    for k, name in enumerate(("sse_u", "ss_opt", "J", "u_absmax")):
        assert np.array_equal(sc[:, k], res[name])
    sc2, ox2, ou2 = ctx.poly_plant_loop_multi(*args, want_x=True, want_u=True, want_scores=False, **kw)
    assert sc2 is None and np.array_equal(ox2, res["states"]) and np.array_equal(ou2, res["controls"])


def test_rejected_before_any_launch(nk, fits):
    """Model and plant of different dimensions, a gain of the wrong shape, an invalid table and a lock-step member context:
    NK_ERR_BAD_ARG (ValueError), and the outputs keep their canary value."""
    from nys_koop_lqr_amd import _lib
    plant, reg, K = fits("P2", 40)
    x0, ref = np.array([0.5, 0.5]), np.zeros(2)
    with pytest.raises(ValueError, match="gain"):
        reg.closed_loop_plant(K[:1], x0, ref, 10, plant)
    with pytest.raises(ValueError, match="gain"):
        reg.closed_loop_plant(K[:, :-1], x0, ref, 10, plant)
    with pytest.raises(ValueError, match="steps"):
        reg.closed_loop_plant(K, x0, ref, 0, plant)
    ctx = nk.get_context()
    h = reg._ensure_model()
    Kc = np.ascontiguousarray(K)
    xb, xr = x0.reshape(1, 2).copy(), ref.reshape(1, 2).copy()
    ox, ou = np.full((1, 11, 4), 7.0), np.full((1, 10, 4), 7.0)
    args = (Kc.ctypes.data, xb.ctypes.data, xr.ctypes.data, 10, 1, ox.ctypes.data, ou.ctypes.data)
    sc = np.full((1, 4), 7.0)
    unit = (_lib.PlantUnit * 1)()
    unit[0].model, unit[0].K, unit[0].x0, unit[0].x_ref, unit[0].uopt = h.value if isinstance(h, C.c_void_p) else h, \
        Kc.ctypes.data, xb.ctypes.data, xr.ctypes.data, -1

    def both(desc, handle, needle):
        rc = ctx.lib.nk_poly_plant_loop(handle, h, desc, *args)
        msg = ctx.lib.nk_last_error().decode()
        assert rc == -1 and needle in msg, (rc, msg)
        rc = ctx.lib.nk_poly_plant_loop_multi(handle, desc, 10, unit, 1, None, 0, ox.ctypes.data, ou.ctypes.data, sc.ctypes.data)
        msg = ctx.lib.nk_last_error().decode()
        assert rc == -1 and needle in msg, (rc, msg)

    both(make_plant("P3").descriptor(), ctx.handle, "1 inputs")  # d = 3, p = 1 against the model's 2 and 2
    both(make_plant("P4").descriptor(), ctx.handle, "4 states")  # p = 2 = the model's, d = 4 against 2
    both(nk.PolynomialSystem.duffing(0.01).descriptor(), ctx.handle, "1 inputs")  # d = 2, p = 1 against 2
    bad = _lib.PolyPlant()
    C.memmove(C.byref(bad), C.byref(plant.descriptor()), C.sizeof(bad))
    bad.terms[2].row = 2
    both(bad, ctx.handle, "term 2")
    handles = (C.c_void_p * 2)()
    _lib.check(ctx.lib.nk_group_create(ctx.device, 2, handles))
    members = [_lib.Context(ctx.device, C.c_void_p(handles[i])) for i in range(2)]
    try:
        both(plant.descriptor(), members[0].handle, "lock-step")
    finally:
        for mem in members:
            mem.close()
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(sc == 7.0)  # nothing ran
    # and the call still works afterwards on the ordinary context
    states, us = reg.closed_loop_plant(K, x0, ref, 10, plant)
    assert states.shape == (2, 11) and us.shape == (2, 10) and np.all(np.isfinite(states)) and np.all(np.isfinite(us))


def test_sweep(nk):
    """harness.lqr_sweep on P2, 2 seeds x ms = (20, 40), with the PolynomialSystem: finite tables, and every unit equals fit ->
    solve_lqr -> closed_loop_plant -> host scores with the same draws, bit for bit."""
    from nys_koop_lqr_amd import harness
    plant = make_plant("P2")
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    params = dict(kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6)
    ms, seeds, steps = (20, 40), (0, 1), 150
    x0, ref = np.array([0.5, 0.5]), np.zeros(2)
    t = np.arange(steps)
    u_opt = np.stack([0.2 * np.exp(-t / 100.0), 0.1 * np.cos(t / 11.0)], axis=1)
    res = harness.lqr_sweep(X, Y, 2, params, ms, seeds, plant, x0, ref, steps, u_opt=u_opt, batch=4, workers=2,
                            return_trajectories=True)
    assert res["J"].shape == (2, 2) and res["states"].shape == (2, 2, steps + 1, 2) and res["controls"].shape == (2, 2, steps, 2)
    for name in ("sse_u", "ss_opt", "J", "u_absmax", "rmse_control", "states", "controls"):
        assert np.all(np.isfinite(res[name])), name
    for u in harness.lqr_plan(X, Y, 2, params, ms, seeds, "nystrom"):
        reg = harness.lqr_fit_unit(X, Y, 2, params, u, "nystrom")
        states, us = reg.closed_loop_plant(reg.solve_lqr(c=1.0), x0, ref, steps, plant)
        si, k = u["si"], u["k"]
        assert np.array_equal(res["states"][si, k], states.T) and np.array_equal(res["controls"][si, k], us.T), (si, k)
        host = harness.control_scores(states, us, u_opt)
        for name in ("sse_u", "ss_opt", "J", "u_absmax"):
            assert res[name][si, k] == host[name], (name, si, k)
