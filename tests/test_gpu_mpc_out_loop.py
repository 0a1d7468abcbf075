"""GPU: the constrained Koopman MPC loop with limits on predicted states in one launch (nk_mpc_out_loop through
regressor.closed_loop_plant_mpc with an lqr.MPCOutputController).  The method of test_gpu_mpc_loop.py: every state the device
returns is replayed on the host bit for bit, and every control is replayed from the returned x_t and u_{t-1} through the NumPy
statement of the folded iteration (lqr.mpc_out_solve, same iters and tol): bar 10 x the replay's own movement under a 1e-15
relative perturbation of F, T and G, floor 1e-10; equal iteration counts at tol = 0; residuals within that file's bar.
Duffing from (-0.5, 0) to the equilibrium (0.5, 0) under a velocity limit (and an overshoot limit), hard and soft, at one and
five waves and in the lane classes 16 and 64; two inputs; other kernel families; inactive rows against nk_mpc_loop; batch
invariance; a NaN trajectory in a batch; the limits and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from conftest import relf
from test_gpu_mpc_loop import _inside, _synthetic_controller
from test_gpu_poly_plant_loop import _assert_replay, _limit_model, fits, nk  # noqa: F401  (fits, nk: fixtures)
from test_poly_plant_host import make_plant

pytestmark = pytest.mark.gpu

STEPS = 150
X0, REF = np.array([-0.5, 0.0]), np.array([0.5, 0.0])
# The output rows are small beside the identity rows of the inputs (one step moves a velocity by 0.5 Ts u): with the default
# rho the ADMM iteration on them stands nearly still.  300 x the default reached the hard velocity limit within 2 % in 100
# iterations on the host loop (NumPy fit of the same model, m = 40), the default left the control unchanged.
RHO_FACTOR = 300.0
U_MAX = 2.0


def _with_outputs(ctl, **kw):
    from nys_koop_lqr_amd import lqr
    f = dict(H=ctl.H, F=ctl.F, lo=ctl.lo, hi=ctl.hi, dlo=ctl.dlo, dhi=ctl.dhi, K=ctl.K, rho=ctl.rho, horizon=ctl.horizon, G=ctl.G,
             T=ctl.T, ylo=ctl.ylo, yhi=ctl.yhi, ycomp=ctl.ycomp, y_weight=ctl.y_weight)
    f.update(kw)
    return lqr.MPCOutputController(**f)


def _perturbed(ctl, seed=99):
    """The controller with F, T and G moved by 1e-15 relative."""
    rng = np.random.default_rng(seed)
    mv = lambda a: a * (1 + 1e-15 * rng.standard_normal(a.shape))
    return _with_outputs(ctl, F=mv(ctl.F), T=mv(ctl.T), G=mv(ctl.G))


def _host_controls(reg, ctl, states, us, x_ref, iters, tol, u_init=None):
    """u_t and info_t replayed per step from the returned x_t and u_{t-1}: one lift of all states, then the NumPy statement."""
    Phi = np.asarray(reg.lift(np.ascontiguousarray(states[:, :-1])))
    x_ref = np.asarray(x_ref, dtype=np.float64).reshape(-1)
    phi_ref = np.asarray(reg.lift(x_ref.reshape(-1, 1)))
    p, steps = us.shape
    U, info = np.empty((p, steps)), np.empty((steps, 2))
    kw = dict(x_ref=x_ref) if hasattr(ctl, "ycomp") else {}
    for t in range(steps):
        u_prev = us[:, t - 1] if t else (np.zeros(p) if u_init is None else np.asarray(u_init, dtype=np.float64).reshape(p))
        U[:, t], info[t] = ctl.control(Phi[:, t] - phi_ref[:, 0], u_prev, iters, tol, **kw)
    return U, info


def _check_replay(label, plant, reg, ctl, x0, ref, states, us, info, iters, tol=0.0, u_init=None):
    """One returned device loop against the per-step host replay."""
    _assert_replay(plant, states, us)
    assert _inside(ctl, us, u_init), label
    U, I = _host_controls(reg, ctl, states, us, ref, iters, tol, u_init)
    Up, _ = _host_controls(reg, _perturbed(ctl), states, us, ref, iters, tol, u_init)
    e_u, s_u = relf(us, U), relf(Up, U)
    bar = max(10.0 * s_u, 1e-10)
    print(f"\n[{label}] device vs host replay: controls {e_u:.2e} (replay moves {s_u:.2e}, bar {bar:.2e}); iterations "
          f"{int(info[:, 0].min())} .. {int(info[:, 0].max())}, largest final residual {info[:, 1].max():.2e}; max |x| "
          f"{np.max(np.abs(states)):.2f}, max |u| {np.max(np.abs(us)):.3f}")
    assert e_u <= bar, (label, e_u, bar)
    if tol == 0.0:
        assert np.array_equal(info[:, 0], I[:, 0]), label
    assert np.max(np.abs(info[:, 1] - I[:, 1])) <= max(bar, 1e-10) * max(np.max(np.abs(us)), 1.0) * 10, label


def _run(label, plant, reg, ctl, x0, ref, iters, tol=0.0, u_init=None, steps=STEPS):
    d, p = plant.n_states, plant.n_inputs
    states, us, info = reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=iters, tol=tol, u_init=u_init,
                                                 return_info=True)
    assert states.shape == (d, steps + 1) and us.shape == (p, steps) and info.shape == (steps, 2)
    assert np.array_equal(states[:, 0], x0)
    _check_replay(label, plant, reg, ctl, x0, ref, states, us, info, iters, tol, u_init)
    return states, us, info


_duffing_cache = {}


def _duffing_case(fits, m, N, soft):
    """(plant, reg, input-only controller, controller with rows, free peak of |x_2| on the host loop, host loops).  The
    velocity limit is 0.6 of the peak |x_2| of the host loop WITHOUT the rows (|u| <= 2, 100 iterations); N = 8: 8 rows on
    x_2; N = 32: x_1 <= 0.55 (the overshoot limit) and the velocity limit over 16 steps, 32 rows.  Computed once per case."""
    from nys_koop_lqr_amd import harness
    key = (m, N, soft)
    if key not in _duffing_cache:
        plant, reg, _ = fits("duffing", m)
        rho = RHO_FACTOR * reg.solve_mpc(N, c=1.0).rho
        if (m, N) not in _duffing_cache:
            free = reg.solve_mpc(N, c=1.0, u_min=-U_MAX, u_max=U_MAX, rho=rho)
            S0, U0, _ = harness.mpc_control_plant(STEPS, REF, X0, reg, free, plant.update_SOM, iters=100)
            _duffing_cache[(m, N)] = (free, S0, U0)
        free, S0, U0 = _duffing_cache[(m, N)]
        v = 0.6 * float(np.max(np.abs(S0[1])))
        ctl = reg.solve_mpc(N, c=1.0, u_min=-U_MAX, u_max=U_MAX, rho=rho, x_min=[-np.inf, -v],
                            x_max=[np.inf if N == 8 else 0.55, v], y_horizon=8 if N == 8 else 16,
                            y_weight=10.0 * rho if soft else np.inf)
        _duffing_cache[key] = (plant, reg, free, ctl, S0, U0)
    return _duffing_cache[key]


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("N", [8, 32])
@pytest.mark.parametrize("m", [40, 300])
def test_duffing_velocity_and_overshoot_limits(nk, fits, m, N, soft):
    """Duffing, Matern model, (-0.5, 0) -> (0.5, 0), 100 iterations.  On the host loop first: the controls differ from the
    input-only controller's by more than 1e-6 of the bound at some step, and the peak of |x_2| is strictly below the peak
    without the rows (the ratio is printed).  Then the device loop against the per-step replay."""
    from nys_koop_lqr_amd import harness
    plant, reg, free, ctl, S0, _ = _duffing_case(fits, m, N, soft)
    label = f"Duffing, m = {m}, N = {N}, {'soft' if soft else 'hard'}"
    assert ctl.nv == N and ctl.ny == (8 if N == 8 else 32) and ctl.nv + ctl.ny == (16 if N == 8 else 64)
    S, U, _ = harness.mpc_control_plant(STEPS, REF, X0, reg, ctl, plant.update_SOM, iters=100)
    gap = np.max(np.abs(U - _host_controls(reg, free, S, U, REF, 100, 0.0)[0])) / U_MAX
    pk0, pk = float(np.max(np.abs(S0[1]))), float(np.max(np.abs(S[1])))
    print(f"\n[{label}] host loop: largest distance of u_t from the input-only controller's {gap:.2e} of the bound; peak |x_2| "
          f"{pk:.4f} with the rows, {pk0:.4f} without: ratio {pk / pk0:.3f} (limit at 0.600)")
    assert gap > 1e-6, (label, gap)
    assert pk < pk0, (label, pk, pk0)
    states, us, info = _run(label, plant, reg, ctl, X0, REF, 100)
    assert info[:, 0].max() == 100
    pkd = float(np.max(np.abs(states[1])))
    print(f"[{label}] device loop: peak |x_2| {pkd:.4f}, ratio {pkd / pk0:.3f}")
    assert pkd < pk0


@pytest.mark.parametrize("m", [40, 300])
def test_two_inputs_four_states(nk, fits, m):
    """P4 (four states, two inputs), N = 8 (nv = 16), soft limits |x_1|, |x_2| <= 0.3 over 8 steps (16 rows, nt = 32) from
    0.5 * ones: outside the limits at the start, which the soft rows allow; the box at half the largest unconstrained control."""
    plant, reg, K = fits("P4", m)
    x0, ref = 0.5 * np.ones(4), np.zeros(4)
    e0 = (reg.lift(x0.reshape(-1, 1)) - reg.lift(np.zeros((4, 1)))).reshape(-1)
    b = 0.5 * float(np.max(np.abs(K @ e0)))
    rho = RHO_FACTOR * reg.solve_mpc(8, c=1.0).rho
    lim = [0.3, 0.3, np.inf, np.inf]
    ctl = reg.solve_mpc(8, c=1.0, u_min=-b, u_max=b, rho=rho, x_min=[-v for v in lim], x_max=lim, y_weight=10.0 * rho)
    assert ctl.nv == 16 and ctl.ny == 16
    _, _, info = _run(f"P4, m = {m}", plant, reg, ctl, x0, ref, 50)
    assert info[:, 0].max() == 50


@pytest.mark.parametrize("kind", ["rbf", "spline"])
def test_other_kernel_families(nk, kind):
    """The Duffing velocity limit at m = 40 with an RBF kernel and with a spline model (no fold: [F; T] is read transposed)."""
    from nys_koop_lqr_amd import harness
    plant = nk.PolynomialSystem.duffing(0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    idx = np.random.default_rng(1).choice(2000, 40, False)
    if kind == "spline":
        reg = nk.KoopmanSplineRegressor(1, m=40, gamma=1e-6)
        reg.centers = np.ascontiguousarray(Y.T[:, idx])
    else:
        reg = nk.KoopmanNystromRegressor(1, kernel=nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2), gamma=1e-6, m=40)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
    reg.fit(X, Y)
    rho = RHO_FACTOR * reg.solve_mpc(8, c=1e2).rho
    ctl = reg.solve_mpc(8, c=1e2, u_min=-U_MAX, u_max=U_MAX, rho=rho, x_min=[-np.inf, -0.3], x_max=[np.inf, 0.3], y_weight=10.0 * rho)
    _run(f"Duffing velocity limit, {kind}", plant, reg, ctl, X0, np.zeros(2), 60)


@pytest.mark.parametrize("m", [40, 300])
def test_inactive_rows_give_the_loop_without_them(nk, fits, m):
    """Output bounds of +-100 and no input limits, to the origin: no iteration at any step, and the controls and states are
    those of nk_mpc_loop with the same controller without the rows, within 10 x the host LQR loop's own movement under a
    1e-15 perturbation of K, floor 1e-10 (to rounding; the fold has another shape, so the bits may differ)."""
    from test_gpu_plant_loop import _device_vs_host
    plant, reg, _ = fits("duffing", m)
    ctl = reg.solve_mpc(8, c=1.0, x_min=-100.0, x_max=100.0)
    assert ctl.ny == 16
    x0, ref = X0, np.zeros(2)
    states, us, info = reg.closed_loop_plant_mpc(ctl, x0, ref, STEPS, plant, iters=50, return_info=True)
    _assert_replay(plant, states, us)
    assert np.all(info == 0.0)
    s2, u2 = reg.closed_loop_plant_mpc(ctl.input_only(), x0, ref, STEPS, plant, iters=50)
    _, (s_u, s_x) = _device_vs_host(nk, reg, ctl.K, plant, x0, ref, STEPS)
    bar_u, bar_x = max(10.0 * s_u, 1e-10), max(10.0 * s_x, 1e-10)
    e_u, e_x = relf(us, u2), relf(states, s2)
    print(f"\n[inactive rows, m = {m}] against nk_mpc_loop: controls {e_u:.2e} (bar {bar_u:.2e}), states {e_x:.2e} (bar {bar_x:.2e})")
    assert e_u <= bar_u and e_x <= bar_x


def _batch_case(fits, m):
    plant, reg, free, ctl, _, _ = _duffing_case(fits, m, 8, True)
    rng = np.random.default_rng(2024)
    X0s = np.column_stack([rng.uniform(-0.6, -0.3, 8), rng.uniform(-0.2, 0.2, 8)])
    refs = np.column_stack([rng.uniform(0.4, 0.5, 8), np.zeros(8)])
    U0 = rng.uniform(-0.5, 0.5, size=(8, 1))
    return plant, reg, ctl, X0s, refs, U0


@pytest.mark.parametrize("m", [40, 300])
def test_batch_invariance(nk, fits, m):
    """A trajectory alone and among 7 others with other x0, x_ref and u_init has the same bits in out_x, out_u and out_info."""
    plant, reg, ctl, X0s, refs, U0 = _batch_case(fits, m)
    S, U, I = reg.closed_loop_plant_mpc(ctl, X0s, refs, 100, plant, iters=30, tol=1e-9, u_init=U0, return_info=True)
    assert S.shape == (8, 101, 2) and U.shape == (8, 100, 1) and I.shape == (8, 100, 2)
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(U)) and I[:, :, 0].max() == 30
    for i in (0, 3, 7):
        s, u, info = reg.closed_loop_plant_mpc(ctl, X0s[i], refs[i], 100, plant, iters=30, tol=1e-9, u_init=U0[i], return_info=True)
        assert np.array_equal(S[i], s.T) and np.array_equal(U[i], u.T) and np.array_equal(I[i], info), i
        _check_replay(f"batch member {i}, m = {m}", plant, reg, ctl, X0s[i], refs[i], s, u, info, 30, 1e-9, U0[i])
    assert not np.array_equal(U[0], U[1])


def test_nan_state_in_one_trajectory(nk, fits):
    """A NaN x0 in one trajectory of a batch: its controls are NaN and its info {iters, NaN} at every step; the others keep
    the bits they have without it."""
    plant, reg, ctl, X0s, refs, U0 = _batch_case(fits, 40)
    S, U, I = reg.closed_loop_plant_mpc(ctl, X0s, refs, 40, plant, iters=30, u_init=U0, return_info=True)
    bad = X0s.copy()
    bad[2, 1] = np.nan
    Sb, Ub, Ib = reg.closed_loop_plant_mpc(ctl, bad, refs, 40, plant, iters=30, u_init=U0, return_info=True)
    assert np.all(np.isnan(Ub[2])) and np.all(Ib[2, :, 0] == 30) and np.all(np.isnan(Ib[2, :, 1]))
    keep = [i for i in range(8) if i != 2]
    assert np.array_equal(Sb[keep], S[keep]) and np.array_equal(Ub[keep], U[keep]) and np.array_equal(Ib[keep], I[keep])


def _synthetic_output_controller(rng, m, d, p, N, ny, bound):
    """_synthetic_controller with ny soft output rows that come from no fit."""
    from nys_koop_lqr_amd import lqr
    c = _synthetic_controller(rng, m, p, N, bound)
    G, T = 0.1 * rng.standard_normal((ny, N * p)), 0.3 * rng.standard_normal((ny, m)) / np.sqrt(m)
    return lqr.MPCOutputController(c.H, c.F, c.lo, c.hi, c.dlo, c.dhi, c.K, c.rho, N, G, T, np.full(ny, -0.02), np.full(ny, 0.02),
                                   np.arange(ny) % d, 10.0 * c.rho)


def test_limits_on_lanes_and_landmarks(nk, fits):
    """nv + ny = 64 runs (the Duffing cases above, and here at m = nk_mpc_loop_max_m(64) = 314 on a synthetic controller, four
    states and four inputs: 40 steps against the host replay); one landmark more and one row more are ValueErrors that name
    the limit."""
    from nys_koop_lqr_amd import lqr
    plant = make_plant("P4b")
    limit = nk.get_context().lib.nk_mpc_loop_max_m(64)
    assert limit == 314
    reg, _ = _limit_model(nk, 4, 4, limit)
    ctl = _synthetic_output_controller(np.random.default_rng(5), limit, 4, 4, 8, 32, 0.05)
    _run(f"d = 4, nv + ny = 64, m = {limit}", plant, reg, ctl, 0.5 * np.ones(4), np.zeros(4), 30, steps=40)
    reg1, _ = _limit_model(nk, 4, 4, limit + 1, spline=True)
    ctl1 = _synthetic_output_controller(np.random.default_rng(5), limit + 1, 4, 4, 8, 32, 0.05)
    with pytest.raises(ValueError, match=f"at most {limit}"):
        reg1.closed_loop_plant_mpc(ctl1, 0.5 * np.ones(4), np.zeros(4), 10, plant, iters=30)
    ctl65 = _synthetic_output_controller(np.random.default_rng(5), limit, 4, 4, 8, 33, 0.05)
    with pytest.raises(ValueError, match="ny = 33"):
        reg.closed_loop_plant_mpc(ctl65, 0.5 * np.ones(4), np.zeros(4), 10, plant, iters=30)


def test_rejected_before_any_launch(nk, fits):
    """Every malformed field of the output description, iters = 0 and a malformed nk_mpc_desc: NK_ERR_BAD_ARG with the field
    in nk_last_error(), and no output buffer is touched (guard values); the call still works afterwards."""
    from nys_koop_lqr_amd import _lib
    plant, reg, free, ctl, _, _ = _duffing_case(fits, 40, 8, True)
    ctx = nk.get_context()
    h = reg._ensure_model()
    xb, xr = X0.reshape(1, 2).copy(), REF.reshape(1, 2).copy()
    ox, ou, oi = np.full((1, 11, 2), 7.0), np.full((1, 10, 1), 7.0), np.full((1, 10, 2), 7.0)

    def call(c, needle, iters=20, null=()):
        ds, keep = _lib.mpc_desc(c, iters, 0.0)
        out, keep2 = _lib.mpc_out(c)
        for f in null:
            setattr(out, f, None)
        rc = ctx.lib.nk_mpc_out_loop(ctx.handle, h, plant.descriptor(), C.byref(ds), C.byref(out), xb.ctypes.data, xr.ctypes.data,
                                     None, 10, 1, ox.ctypes.data, ou.ctypes.data, oi.ctypes.data)
        msg = ctx.lib.nk_last_error().decode()
        assert rc == -1 and needle in msg and "nk_mpc_out_loop" in msg, (rc, msg, needle)

    def at(a, i, v):
        b = np.array(a, dtype=np.float64)
        b.flat[i] = v
        return b

    yc = ctl.ycomp.copy()
    yc[3] = 2  # the plant has two states
    call(_with_outputs(ctl, ylo=at(ctl.ylo, 2, ctl.yhi[2] + 1.0)), "ylo[2]")
    call(_with_outputs(ctl, ycomp=yc), "ycomp[3]")
    ycm = ctl.ycomp.copy()
    ycm[0] = -2
    call(_with_outputs(ctl, ycomp=ycm), "ycomp[0]")
    for w in (0.0, -1.0):
        c = _with_outputs(ctl)
        c.y_weight = w
        call(c, "y_weight")
    c = _with_outputs(ctl)
    c.y_weight = float("nan")
    call(c, "y_weight")
    call(_with_outputs(ctl, G=at(ctl.G, 3, np.nan)), "G is not finite")
    call(_with_outputs(ctl, T=at(ctl.T, 3, np.inf)), "T is not finite")
    call(ctl, "G is null", null=("G",))
    call(ctl, "T is null", null=("T",))
    call(_with_outputs(ctl, G=1e160 * np.ones_like(ctl.G)), "not positive definite")
    call(ctl, "iters", iters=0)
    wide = _with_outputs(ctl, G=np.zeros((57, 8)), T=np.zeros((57, 40)), ylo=np.full(57, -1.0), yhi=np.full(57, 1.0),
                         ycomp=np.zeros(57, dtype=np.int32))
    call(wide, "ny = 57")
    lo = ctl.lo.copy()
    lo[5] = ctl.hi[5] + 1.0
    call(_with_outputs(ctl, lo=lo), "lo[5]")
    assert np.all(ox == 7.0) and np.all(ou == 7.0) and np.all(oi == 7.0)  # nothing ran
    states, us = reg.closed_loop_plant_mpc(ctl, X0, REF, 10, plant, iters=20)  # and the call still works
    assert states.shape == (2, 11) and us.shape == (1, 10) and np.all(np.isfinite(states)) and np.all(np.isfinite(us))
