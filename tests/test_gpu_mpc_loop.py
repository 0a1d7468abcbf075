"""GPU: the constrained Koopman MPC closed loop around the true plant in one launch (nk_mpc_loop through
regressor.closed_loop_plant_mpc).  Every state the device returns is replayed on the host bit for bit (plant.step_library), and
every control is replayed from the returned x_t and u_{t-1} through the NumPy statement of the iteration (lqr.mpc_solve with the
same iters and tol): bar 10 x the replay's own movement under a 1e-15 relative perturbation of F (K for iters = 0), floor 1e-10.
Inactive limits against the LQR loop, the saturated mode, a rate-limited input, several inputs up to nv = 64, every kernel
family, the limits on m, batch invariance, the early stop and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from conftest import relf
from test_gpu_poly_plant_loop import _assert_replay, _limit_model, fits, nk  # noqa: F401  (fits, nk: fixtures)
from test_poly_plant_host import make_plant

pytestmark = pytest.mark.gpu

STEPS = 150


def _host_controls(reg, ctl, states, us, x_ref, iters, tol, u_init=None):
    """u_t and info_t replayed per step from the returned x_t and u_{t-1}: one lift of all states, then lqr.mpc_solve."""
    Phi = np.asarray(reg.lift(np.ascontiguousarray(states[:, :-1])))
    phi_ref = np.asarray(reg.lift(np.asarray(x_ref, dtype=np.float64).reshape(-1, 1)))
    p, steps = us.shape
    U, info = np.empty((p, steps)), np.empty((steps, 2))
    for t in range(steps):
        u_prev = us[:, t - 1] if t else (np.zeros(p) if u_init is None else np.asarray(u_init, dtype=np.float64).reshape(p))
        U[:, t], info[t] = ctl.control(Phi[:, t] - phi_ref[:, 0], u_prev, iters, tol)
    return U, info


def _perturbed(ctl, seed=99):
    """The controller with F and K moved by 1e-15 relative."""
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(seed)
    return lqr.MPCController(ctl.H, ctl.F * (1 + 1e-15 * rng.standard_normal(ctl.F.shape)), ctl.lo, ctl.hi, ctl.dlo, ctl.dhi,
                             ctl.K * (1 + 1e-15 * rng.standard_normal(ctl.K.shape)), ctl.rho, ctl.horizon)


def _inside(ctl, us, u_init=None):
    """Every control inside its bounds, every change inside the rate limits as the loop forms them (u_prev + dlo in floating
    point), exactly."""
    p = us.shape[0]
    prev = np.column_stack([np.zeros(p) if u_init is None else np.asarray(u_init, dtype=np.float64).reshape(p), us[:, :-1]])
    lo, hi, dlo, dhi = (a[:p, None] for a in (ctl.lo, ctl.hi, ctl.dlo, ctl.dhi))
    return bool(np.all(us >= lo) and np.all(us <= hi) and np.all(us >= prev + dlo) and np.all(us <= prev + dhi))


def _saturated(reg, ctl, states, us, x_ref, u_init=None):
    """The saturated-LQR formula at the returned x_t, u_{t-1}."""
    return _host_controls(reg, ctl, states, us, x_ref, 0, 0.0, u_init)[0]


def _check_case(label, plant, reg, ctl, x0, iters, tol=0.0, u_init=None, steps=STEPS, differs=False):
    """One device loop from x0 to the origin against the per-step host replay; returns (states, us, info)."""
    from nys_koop_lqr_amd import harness
    d, p = plant.n_states, plant.n_inputs
    ref = np.zeros(d)
    bound = float(np.min(ctl.hi[np.isfinite(ctl.hi)])) if np.any(np.isfinite(ctl.hi)) else 1.0
    if differs:  # on the host first: the case must not degenerate into the saturated LQR
        S, U, _ = harness.mpc_control_plant(steps, ref, x0, reg, ctl, plant.update_SOM, iters=iters, tol=tol, u_init=u_init)
        gap = np.max(np.abs(U - _saturated(reg, ctl, S, U, ref, u_init))) / bound
        print(f"\n[{label}] host loop: largest distance of u_t from the saturated-LQR formula {gap:.2e} of the bound")
        assert gap > 1e-6, (label, gap)
    states, us, info = reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=iters, tol=tol, u_init=u_init,
                                                 return_info=True)
    assert states.shape == (d, steps + 1) and us.shape == (p, steps) and info.shape == (steps, 2)
    assert np.array_equal(states[:, 0], x0)
    _assert_replay(plant, states, us)
    assert _inside(ctl, us, u_init), label
    U, I = _host_controls(reg, ctl, states, us, ref, iters, tol, u_init)
    Up, _ = _host_controls(reg, _perturbed(ctl), states, us, ref, iters, tol, u_init)
    e_u, s_u = relf(us, U), relf(Up, U)
    bar = max(10.0 * s_u, 1e-10)
    sat_gap = np.max(np.abs(us - _saturated(reg, ctl, states, us, ref, u_init))) / bound
    print(f"\n[{label}] device vs host replay: controls {e_u:.2e} (replay moves {s_u:.2e}, bar {bar:.2e}); iterations "
          f"{int(info[:, 0].min())} .. {int(info[:, 0].max())}, largest final residual {info[:, 1].max():.2e}; from the saturated "
          f"LQR {sat_gap:.2e} of the bound; max |x| {np.max(np.abs(states)):.2f}, max |u| {np.max(np.abs(us)):.3f}")
    assert e_u <= bar, (label, e_u, bar)
    if tol == 0.0:
        assert np.array_equal(info[:, 0], I[:, 0]), label
    assert np.max(np.abs(info[:, 1] - I[:, 1])) <= max(bar, 1e-10) * max(np.max(np.abs(us)), 1.0) * 10, label
    if differs:
        assert sat_gap > 1e-6, (label, sat_gap)
    return states, us, info


def _limited(reg, K, plant, x0, N, c, frac, rate=None, **kw):
    """solve_mpc with the box at frac |K e_0| (per input: of the largest entry) and rates at `rate` of the box per step."""
    e0 = (reg.lift(x0.reshape(-1, 1)) - reg.lift(np.zeros((x0.size, 1)))).reshape(-1)
    b = frac * float(np.max(np.abs(K @ e0)))
    return reg.solve_mpc(N, c=c, u_min=-b, u_max=b, du_min=None if rate is None else -rate * b,
                         du_max=None if rate is None else rate * b, **kw), b


@pytest.mark.parametrize("m", [40, 300])
def test_inactive_limits_give_the_lqr_loop(nk, fits, m):
    """All bounds +-inf, Duffing table, N = 8: no iteration runs (out_info), and states and controls are those of
    closed_loop_plant(K) within 10 x the host LQR loop's own movement under a 1e-15 perturbation of K, floor 1e-10.  K is the
    controller's gain: solve_mpc refines scipy's Riccati solution by Newton steps, without which the first move of the QP and
    dlqr's gain differ by 5e-9 and the two loops by 1.2e-8 / 2.8e-9 (controls / states at m = 40, measured on the device); the
    distance of the refined gain from solve_lqr's is printed."""
    from test_gpu_plant_loop import _device_vs_host
    plant, reg, K0 = fits("duffing", m)
    ctl = reg.solve_mpc(8, c=1.0)
    x0, ref = np.array([-0.5, 0.0]), np.zeros(2)
    K = ctl.K
    print(f"\n[inactive, m = {m}] the controller's gain against solve_lqr's: {relf(K, K0):.2e}")
    assert relf(K, K0) <= 1e-4
    states, us, info = reg.closed_loop_plant_mpc(ctl, x0, ref, STEPS, plant, iters=50, return_info=True)
    _assert_replay(plant, states, us)
    assert np.all(info == 0.0)
    sl, ul = reg.closed_loop_plant(K, x0, ref, STEPS, plant)
    _, (s_u, s_x) = _device_vs_host(nk, reg, K, plant, x0, ref, STEPS)
    bar_u, bar_x = max(10.0 * s_u, 1e-10), max(10.0 * s_x, 1e-10)
    e_u, e_x = relf(us, ul), relf(states, sl)
    print(f"\n[inactive, m = {m}] MPC loop vs LQR loop: controls {e_u:.2e} (bar {bar_u:.2e}), states {e_x:.2e} (bar {bar_x:.2e})")
    assert e_u <= bar_u and e_x <= bar_x


@pytest.mark.parametrize("name,m", [("duffing", 40), ("P4", 300)])
def test_iters_0_is_the_saturated_lqr(nk, fits, name, m):
    """Per step, from the returned x_t and u_{t-1}: u_t is the clip formula on the host K e (the replay of _check_case with
    iters = 0); every control inside its limits exactly; the limits are active."""
    plant, reg, K = fits(name, m)
    x0 = np.array([-0.5, 0.0]) if name == "duffing" else 0.5 * np.ones(4)
    ctl, b = _limited(reg, K, plant, x0, 8, 1.0, 0.3, 0.05)
    states, us, info = _check_case(f"saturated LQR, {name}, m = {m}", plant, reg, ctl, x0, 0)
    assert np.all(info == 0.0) and np.max(np.abs(us)) <= b
    free = reg.closed_loop_plant(K, x0, np.zeros(x0.size), 1, plant)[1]
    assert np.max(np.abs(free)) > b  # the unconstrained control leaves the box


def test_rate_limited_single_input(nk, fits):
    """Duffing, m = 40, N = 16, |u| <= 0.3 |K e_0|, rate 5 % of that per step, Q = 1e4 C'C (cond(H) = 40), 100 iterations.
    The host loop's controls lie 1.7e-4 of the bound from the saturated-LQR formula at 100 iterations (with the NumPy oracle of
    the fit: 1.8e-4, and 2.1e-7 at 400 iterations: under limits this tight the converged QP is close to a clip as well, so the
    condition "differs from clipping" holds here through unconverged iterates only; the test prints the distance at 400
    iterations beside it.  A one-input case whose CONVERGED solution differs was not found under the limits the case fixes:
    Q = 1e6 C'C differs by the rate step itself, but its residual stays at 0.1 of the bound after 400 iterations).
    Measured on an MI355X: device against the per-step host replay 8.1e-14 (the replay moves 1.9e-14; bar 1e-10)."""
    plant, reg, K = fits("duffing", 40)
    x0 = np.array([-0.5, 0.0])
    Kc = reg.solve_lqr(c=1e4)
    ctl, _ = _limited(reg, Kc, plant, x0, 16, 1e4, 0.3, 0.05)
    assert ctl.nv == 16
    _check_case("rate-limited Duffing, m = 40", plant, reg, ctl, x0, 100, differs=True)
    # what the 1e-6 above rests on: the same host loop with four times the iterations
    from nys_koop_lqr_amd import harness
    S, U, _ = harness.mpc_control_plant(STEPS, np.zeros(2), x0, reg, ctl, plant.update_SOM, iters=400)
    gap400 = np.max(np.abs(U - _saturated(reg, ctl, S, U, np.zeros(2)))) / float(ctl.hi[0])
    print(f"\n[rate-limited Duffing, m = 40] host loop at 400 iterations: {gap400:.2e} of the bound from the saturated LQR -- the "
          f"distance at 100 iterations comes from iterates that have not converged")
    assert np.isfinite(gap400) and gap400 < 1e-3, f"the QP at 400 iterations lies {gap400:.2e} of the bound from the saturated LQR"


def test_built_in_plant_object_runs_as_its_table(nk, fits):
    """A DuffingOscillator passed as the plant is mapped to PolynomialSystem.duffing (the reference's RK4 variant): the same
    bits as the call with the table, in the QP mode and in the saturated mode; a plant that is neither is a ValueError."""
    plant, reg, K = fits("duffing", 40)
    x0, ref = np.array([-0.5, 0.0]), np.zeros(2)
    ctl, _ = _limited(reg, K, plant, x0, 8, 1.0, 0.3, 0.05)
    obj = nk.DuffingOscillator(Ts=0.01)
    for iters in (0, 20):
        a = reg.closed_loop_plant_mpc(ctl, x0, ref, 60, obj, iters=iters, return_info=True)
        b = reg.closed_loop_plant_mpc(ctl, x0, ref, 60, plant, iters=iters, return_info=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), iters
        _assert_replay(plant, a[0], a[1])
    with pytest.raises(ValueError, match="plant"):
        reg.closed_loop_plant_mpc(ctl, x0, ref, 10, object())


@pytest.mark.parametrize("m", [40, 300])
@pytest.mark.parametrize("name,N", [("P4", 8), ("P4b", 16)])
def test_several_inputs(nk, fits, name, N, m):
    """Four states with two inputs (N = 8, nv = 16) and with four (N = 16, nv = 64: the limit), the box at half the largest
    unconstrained control: active on the first part of the horizon.  50 iterations (final residual below 1e-6)."""
    plant, reg, K = fits(name, m)
    x0 = 0.5 * np.ones(4)
    ctl, _ = _limited(reg, K, plant, x0, N, 1.0, 0.5)
    assert ctl.nv == N * plant.n_inputs
    _check_case(f"{name}, N = {N}, m = {m}", plant, reg, ctl, x0, 50, differs=True)


@pytest.mark.parametrize("kind", ["rbf", "linear", "spline"])
def test_other_kernel_families(nk, kind):
    """The rate-limited Duffing case at m = 40 with an RBF kernel, a linear kernel and a spline model (no fold: F is read
    transposed)."""
    from nys_koop_lqr_amd import harness
    plant = nk.PolynomialSystem.duffing(0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    idx = np.random.default_rng(1).choice(2000, 40, False)
    if kind == "spline":
        reg = nk.KoopmanSplineRegressor(1, m=40, gamma=1e-6)
        reg.centers = np.ascontiguousarray(Y.T[:, idx])
    else:
        kern = nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2) if kind == "rbf" else nk.LinearKernelWrapper(1.0)
        reg = nk.KoopmanNystromRegressor(1, kernel=kern, gamma=1e-6, m=40)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
    reg.fit(X, Y)
    x0 = np.array([-0.5, 0.0])
    ctl, _ = _limited(reg, reg.solve_lqr(c=1e2), plant, x0, 16, 1e2, 0.3, 0.05)
    _check_case(f"rate-limited Duffing, {kind}", plant, reg, ctl, x0, 100)


def _synthetic_controller(rng, m, p, N, bound):
    """A controller that comes from no fit (the limit models have no operators): H = I + G G' / nv, small F and K."""
    from nys_koop_lqr_amd import lqr
    nv = N * p
    G = rng.standard_normal((nv, nv))
    H = np.eye(nv) + G @ G.T / nv
    F, K = 0.3 * rng.standard_normal((nv, m)) / np.sqrt(m), 0.3 * rng.standard_normal((p, m)) / np.sqrt(m)
    lo, hi, dlo, dhi = lqr.mpc_bounds(nv, -bound, bound, -0.2 * bound, 0.2 * bound)
    return lqr.MPCController(H, (H + H.T) / 2 @ F, lo, hi, dlo, dhi, K, lqr.mpc_default_rho(H), N)


@pytest.mark.parametrize("d,p,N,limit", [(4, 4, 16, 314), (1, 1, 20, 512)])
def test_limits_on_m(nk, d, p, N, limit):
    """m at the documented limit (nv = 64: 314 by the LDS budget; nv = 20: 512, eight waves): 40 steps against the host replay;
    one landmark more is a ValueError that names the limit."""
    plant = make_plant("P4b") if d == 4 else nk.PolynomialSystem.hjb(0.01)
    assert nk.get_context().lib.nk_mpc_loop_max_m(N * p) == limit
    reg, _ = _limit_model(nk, d, p, limit)
    ctl = _synthetic_controller(np.random.default_rng(5), limit, p, N, 0.05)
    _check_case(f"d = {d}, nv = {N * p}, m = {limit}", plant, reg, ctl, 0.5 * np.ones(d), 30, steps=40)
    reg1, _ = _limit_model(nk, d, p, limit + 1, spline=True)
    ctl1 = _synthetic_controller(np.random.default_rng(5), limit + 1, p, N, 0.05)
    with pytest.raises(ValueError, match=f"at most {limit}"):
        reg1.closed_loop_plant_mpc(ctl1, 0.5 * np.ones(d), np.zeros(d), 10, plant, iters=30)


@pytest.mark.parametrize("m", [40, 300])
def test_batch_invariance(nk, fits, m):
    """P4, N = 8: a trajectory alone and inside a batch of 7 with other x0 and u_init has the same bits, out_info included."""
    plant, reg, K = fits("P4", m)
    ctl, b = _limited(reg, K, plant, 0.5 * np.ones(4), 8, 1.0, 0.5, 0.2)
    rng = np.random.default_rng(2024)
    X0, U0 = rng.uniform(-0.5, 0.5, size=(7, 4)), rng.uniform(-0.3 * b, 0.3 * b, size=(7, 2))
    ref = np.zeros(4)
    S, U, I = reg.closed_loop_plant_mpc(ctl, X0, ref, 100, plant, iters=30, tol=1e-9, u_init=U0, return_info=True)
    assert S.shape == (7, 101, 4) and U.shape == (7, 100, 2) and I.shape == (7, 100, 2)
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(U)) and I[:, :, 0].max() == 30
    for i in (0, 3, 6):
        s, u, info = reg.closed_loop_plant_mpc(ctl, X0[i], ref, 100, plant, iters=30, tol=1e-9, u_init=U0[i], return_info=True)
        assert np.array_equal(S[i], s.T) and np.array_equal(U[i], u.T) and np.array_equal(I[i], info), i
        _assert_replay(plant, s, u)
        assert _inside(ctl, u, U0[i])
    assert not np.array_equal(U[0], U[1])


def test_early_stop(nk, fits):
    """tol > 0: at most `iters` iterations per step, the final residual at most tol wherever the stop was taken, fewer
    iterations than the cap on most steps, and the controls agree with the host iteration run with the same tol."""
    plant, reg, K = fits("P4", 40)
    x0 = 0.5 * np.ones(4)
    ctl, b = _limited(reg, K, plant, x0, 8, 1.0, 0.5)
    tol = 1e-7 * b
    states, us, info = _check_case("early stop, P4", plant, reg, ctl, x0, 200, tol=tol)
    stopped = info[:, 0] < 200
    assert np.all(info[:, 0] <= 200) and np.all(info[stopped, 1] <= tol) and stopped.sum() > STEPS // 2
    assert info[:, 0].max() > 0 and info[:, 0].min() == 0  # active at the start, the LQR control at the end


def test_rejected_before_any_launch(nk, fits):
    """nv = 65, lo > hi, H not positive definite, m past the limit, p mismatch and a lock-step member context:
    NK_ERR_BAD_ARG with the reason in nk_last_error(), and no output buffer is touched (canaries)."""
    from nys_koop_lqr_amd import _lib, lqr
    plant, reg, K = fits("P4", 40)
    x0 = 0.5 * np.ones(4)
    ctl, b = _limited(reg, K, plant, x0, 8, 1.0, 0.5)
    ctx = nk.get_context()
    h = reg._ensure_model()
    xb, xr = x0.reshape(1, 4).copy(), np.zeros((1, 4))
    ox, ou, oi = np.full((1, 11, 4), 7.0), np.full((1, 10, 2), 7.0), np.full((1, 10, 2), 7.0)

    def call(c, needle, handle=None, model=h, pl=plant):
        ds, keep = _lib.mpc_desc(c, 20, 0.0)
        rc = ctx.lib.nk_mpc_loop(ctx.handle if handle is None else handle, model, pl.descriptor(), C.byref(ds), xb.ctypes.data,
                                 xr.ctypes.data, None, 10, 1, ox.ctypes.data, ou.ctypes.data, oi.ctypes.data)
        msg = ctx.lib.nk_last_error().decode()
        assert rc == -1 and needle in msg, (rc, msg, needle)

    def variant(**kw):
        f = dict(H=ctl.H, F=ctl.F, lo=ctl.lo, hi=ctl.hi, dlo=ctl.dlo, dhi=ctl.dhi, K=ctl.K, rho=ctl.rho, horizon=ctl.horizon)
        f.update(kw)
        return lqr.MPCController(**f)

    big = variant(H=np.eye(66), F=np.zeros((66, 40)), lo=np.full(66, -1.0), hi=np.full(66, 1.0), dlo=np.full(66, -1.0),
                  dhi=np.full(66, 1.0), horizon=33)
    call(big, "nv")
    lo = ctl.lo.copy()
    lo[5] = ctl.hi[5] + 1.0
    call(variant(lo=lo), "lo[5]")
    call(variant(H=ctl.H - 2 * np.max(np.linalg.eigvalsh(ctl.H)) * np.eye(16)), "not positive definite")
    call(variant(rho=0.0), "rho")
    # p mismatch: the description of a one-input problem against the two-input plant and model
    one = variant(H=np.eye(8), F=np.zeros((8, 40)), lo=ctl.lo[:8], hi=ctl.hi[:8], dlo=ctl.dlo[:8], dhi=ctl.dhi[:8], K=ctl.K[:1])
    call(one, "inputs")
    call(ctl, "1 inputs", pl=make_plant("P3"))  # the plant has d = 3, p = 1
    # m past the limit for nv = 64 (and a description for another m)
    reg_big, _ = _limit_model(nk, 4, 2, 400)
    call(ctl, "m = 40", model=reg_big._ensure_model())
    wide = _synthetic_controller(np.random.default_rng(1), 400, 2, 32, 0.1)
    call(wide, "at most 314", model=reg_big._ensure_model())
    handles = (C.c_void_p * 2)()
    _lib.check(ctx.lib.nk_group_create(ctx.device, 2, handles))
    members = [_lib.Context(ctx.device, C.c_void_p(handles[i])) for i in range(2)]
    try:
        call(ctl, "lock-step", handle=members[0].handle)
    finally:
        for mem in members:
            mem.close()
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(oi == 7.0)  # nothing ran
    with pytest.raises(ValueError, match="steps"):
        reg.closed_loop_plant_mpc(ctl, x0, np.zeros(4), 0, plant)
    states, us = reg.closed_loop_plant_mpc(ctl, x0, np.zeros(4), 10, plant, iters=20)  # and the call still works
    assert states.shape == (4, 11) and us.shape == (2, 10) and np.all(np.isfinite(states)) and np.all(np.isfinite(us))
