"""GPU: the plant-in-the-loop LQR closed loop as one device launch (nk_plant_loop, KoopmanNystromRegressor.closed_loop_plant,
harness.lqr_control_plant_device) against the reference's recorded runs, against the host loop it replaces
(harness.lqr_control_plant: one lift per step), across batches, kernels, model kinds and landmark counts."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import relf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


# ---------------------------------------------------------------------------------------------------------------
# the two reference configurations, rebuilt from host copies (no fit in the way: nk_model_create only recomputes K_mm^{-1/2})
# ---------------------------------------------------------------------------------------------------------------
def _duffing_case(nk, golden, seed):
    g = golden("f12_duffing_full.npz")
    env = golden("f12b_duffing_envelope.npz")
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]), m=20)
    reg.nystrom_centers_output = np.ascontiguousarray(g["Y"].T[:, g[f"lqr_idx_{seed}"]])
    reg.A, reg.B, reg.C = g[f"lqr_A_{seed}"], g[f"lqr_B_{seed}"], g[f"lqr_C_{seed}"]
    # the bars of test_duffing_plant_in_the_loop_lqr_vs_reference (tests/test_gpu_configs.py): [2] controls, [3] states
    bars = np.maximum(np.maximum(10.0 * np.maximum(g[f"lqr_sens_{seed}"], env[f"lqr_roworder_{seed}"]),
                                 3.0 * env[f"lqr_envelope_{seed}"]), 1e-8)
    return dict(reg=reg, K=g[f"lqr_K_{seed}"], steps=int(g["lqr_steps"]), plant=nk.DuffingOscillator(Ts=0.01),
                x0=np.array([-0.5, 0.0]), ref=np.zeros(2), us=g[f"lqr_us_{seed}"], states=g[f"lqr_states_{seed}"],
                bar_u=float(bars[2]), bar_x=float(bars[3]))


def _hjb_case(nk, golden):
    g = golden("f8_hjb_config2.npz")
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([float(g["ls"])]), gamma=float(g["gamma"]), m=int(g["m"]))
    reg.nystrom_centers_output = np.ascontiguousarray(g["Y"].T[:, g["idx"]])
    reg.A, reg.B, reg.C = g["A"], g["B"], g["C"]
    # the bars of test_hjb_config2_nystrom_vs_exact_kernel: 1e-5 on the controls, 1e-6 on the visited states
    return dict(reg=reg, K=g["K"], steps=int(g["cl_steps"]), plant=nk.HJB(Ts=0.01), x0=np.array([0.9]), ref=np.zeros(1),
                us=g["cl_u"].reshape(1, -1), states=g["cl_x"].reshape(1, -1), bar_u=1e-5, bar_x=1e-6)


def _cases(nk, golden):
    return [("duffing seed %d" % s, _duffing_case(nk, golden, s)) for s in (0, 1, 2)] + [("hjb", _hjb_case(nk, golden))]


def test_device_loop_vs_reference_runs(nk, golden):
    """The REFERENCE's landmarks, operators and gain (f12: Matern [1, 1], m = 20, seeds 0..2, 2000 steps; f8: Matern [ls], m = 200,
    400 steps), the loop on the device: controls and states against the reference's own run under the bars the host-loop tests
    use for the same quantities (the reference's reproducibility, tests/test_gpu_configs.py)."""
    for name, c in _cases(nk, golden):
        t0 = time.perf_counter()
        states, us = c["reg"].closed_loop_plant(c["K"], c["x0"], c["ref"], c["steps"], c["plant"])
        dt = time.perf_counter() - t0
        d = c["x0"].size
        assert states.shape == (d, c["steps"] + 1) and us.shape == (1, c["steps"])
        assert np.array_equal(states[:, 0], c["x0"])
        T = c["states"].shape[1]  # f12 records steps + 1 states, f8 the `steps` states the controls were computed at
        e_u, e_x = relf(us, c["us"]), relf(states[:c["states"].shape[0], :T], c["states"])
        print(f"\n[{name}] device loop vs reference: controls {e_u:.2e} (bar {c['bar_u']:.2e}), states {e_x:.2e} "
              f"(bar {c['bar_x']:.2e}); {c['steps']} steps in {dt * 1e3:.2f} ms (first call: includes the model rebuild)")
        assert e_u <= c["bar_u"] and e_x <= c["bar_x"], (name, e_u, e_x)


def test_device_loop_vs_host_loop(nk, golden):
    """Same regressor, same gain, the package's plant: the device launch against harness.lqr_control_plant (a lift per step),
    under the same bars as against the reference.  The measured distance is printed: the CPU emulation of the folded gain
    gave 1e-13..2e-12, but with SciPy's square root, not the device's."""
    from nys_koop_lqr_amd import harness
    for name, c in _cases(nk, golden):
        xs_d, us_d = harness.lqr_control_plant_device(c["steps"], c["ref"], c["x0"], c["reg"], c["K"], c["plant"])
        t0 = time.perf_counter()
        xs_d, us_d = harness.lqr_control_plant_device(c["steps"], c["ref"], c["x0"], c["reg"], c["K"], c["plant"])
        t1 = time.perf_counter()
        xs_h, us_h = harness.lqr_control_plant(c["steps"], c["ref"], c["x0"], c["reg"], c["K"], c["plant"].update_SOM)
        t2 = time.perf_counter()
        assert xs_d.shape == xs_h.shape == (c["steps"],) and us_d.shape == us_h.shape == (1, c["steps"])
        e_u, e_x = relf(us_d, us_h), relf(xs_d, xs_h)
        print(f"\n[{name}] device loop vs host loop: controls {e_u:.2e}, first state coordinate {e_x:.2e}; device "
              f"{(t1 - t0) * 1e3:.2f} ms, host loop {(t2 - t1) * 1e3:.1f} ms")
        assert e_u <= c["bar_u"] and e_x <= c["bar_x"], (name, e_u, e_x)


@pytest.mark.parametrize("which", ["duffing", "hjb"])
def test_batch_invariance(nk, golden, which):
    """Trajectories never interact: 1, 7 and 64 initial states (inside the plants' state bounds) in one call give, bit for
    bit, what each state gives in a call of its own."""
    c = _duffing_case(nk, golden, 0) if which == "duffing" else _hjb_case(nk, golden)
    d, steps = c["x0"].size, 300
    rng = np.random.default_rng(2024)
    X0 = rng.uniform(-0.9, 0.9, size=(64, d))
    ref = rng.uniform(-0.1, 0.1, size=(64, d))
    alone = [c["reg"].closed_loop_plant(c["K"], X0[i], ref[i], steps, c["plant"]) for i in range(64)]
    for batch in (1, 7, 64):
        S, U = c["reg"].closed_loop_plant(c["K"], X0[:batch], ref[:batch], steps, c["plant"])
        if batch == 1 and d == 1:  # a (1, 1) array is the (d, 1) column of ONE state: the single-trajectory shapes
            assert S.shape == (1, steps + 1) and U.shape == (1, steps)
            S, U = S.T[None], U.T[None]
        assert S.shape == (batch, steps + 1, d) and U.shape == (batch, steps, 1)
        for i in range(batch):
            assert np.array_equal(S[i], alone[i][0].T) and np.array_equal(U[i], alone[i][1].T), (batch, i)
    # one reference shared by the batch
    S, U = c["reg"].closed_loop_plant(c["K"], X0[:7], ref[0], steps, c["plant"])
    S1, U1 = c["reg"].closed_loop_plant(c["K"], X0[3], ref[0], steps, c["plant"])
    assert np.array_equal(S[3], S1.T) and np.array_equal(U[3], U1.T)
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(U))


# ---------------------------------------------------------------------------------------------------------------
# other kernels, spline models, landmark counts: device loop against host loop
# ---------------------------------------------------------------------------------------------------------------
def _snapshots(plant, n, rng, bound=1.0, u_bound=1.0):
    """n snapshot pairs of the package's plant: states uniform in the box, inputs uniform; X = [state | input], Y = next state."""
    d = plant.n_states
    S = rng.uniform(-bound, bound, size=(d, n))
    U = rng.uniform(-u_bound, u_bound, size=(1, n))
    Y = plant.update_SOM(S, U)
    return np.ascontiguousarray(np.vstack((S, U)).T), np.ascontiguousarray(Y.T)


def _proportional_gain(reg, gain=2.0):
    """u = gain (x1_ref - x1) read through the model's own output map: K = gain C[0].  No Riccati solve in the way, and the
    loop is stable for the Duffing oscillator and the HJB system."""
    return gain * np.asarray(reg.C)[0:1, :]


def _device_vs_host(nk, reg, K, plant, x0, ref, steps):
    """Distances (controls, first state coordinate) between the device loop and the host loop, and the host loop's own
    movement when the gain is perturbed by 1e-15 relative (the sensitivity protocol of tests/golden/make_golden_duffing.py)."""
    from nys_koop_lqr_amd import harness
    xs_d, us_d = harness.lqr_control_plant_device(steps, ref, x0, reg, K, plant)
    xs_h, us_h = harness.lqr_control_plant(steps, ref, x0, reg, K, plant.update_SOM)
    prng = np.random.default_rng(99)
    Kp = K * (1 + 1e-15 * prng.standard_normal(K.shape))
    xs_p, us_p = harness.lqr_control_plant(steps, ref, x0, reg, Kp, plant.update_SOM)
    return (relf(us_d, us_h), relf(xs_d, xs_h)), (relf(us_p, us_h), relf(xs_p, xs_h))


@pytest.mark.parametrize("kind", ["rbf", "linear", "spline"])
def test_other_kernels_and_spline_models(nk, kind):
    """A small Duffing fit (n = 2000 snapshot pairs of the package's plant, m = 50), device loop against host loop over 200
    steps from (-0.5, 0) to the origin, gain K = 2 C[0].  Bar, per quantity: 10 x the host loop's own movement under a
    1e-15 relative perturbation of K, floor 1e-10.
    Measured on an MI355X (controls / first state coordinate; device-vs-host, then the host loop's movement):
    rbf 1.9e-13 / 9.8e-14 (host loop: 1.8e-13 / 1.5e-14); linear 3.5e-13 / 1.6e-14 (5.0e-13 / 2.0e-14); spline 1.4e-15 /
    1.5e-16 (2.0e-15 / 4.9e-16).  Ten times the host loop's movement is below the floor everywhere: the bars are 1e-10."""
    rng = np.random.default_rng(7)
    plant = nk.DuffingOscillator(Ts=0.01)
    X, Y = _snapshots(plant, 2000, rng)
    idx = rng.choice(2000, 50, replace=False)
    if kind == "spline":
        reg = nk.KoopmanSplineRegressor(1, m=50, gamma=1e-6)
        reg.centers = np.ascontiguousarray(Y.T[:, idx])
    else:
        kern = nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, 2) if kind == "rbf" else nk.LinearKernelWrapper(1.0)
        reg = nk.KoopmanNystromRegressor(1, kernel=kern, gamma=1e-6, m=50)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
    reg.fit(X, Y)
    K = _proportional_gain(reg)
    (e_u, e_x), (s_u, s_x) = _device_vs_host(nk, reg, K, plant, np.array([-0.5, 0.0]), np.zeros(2), 200)
    bar_u, bar_x = max(10.0 * s_u, 1e-10), max(10.0 * s_x, 1e-10)
    print(f"\n[{kind}, m = 50] device vs host loop: controls {e_u:.2e} (host loop moves {s_u:.2e}, bar {bar_u:.2e}), "
          f"states {e_x:.2e} (moves {s_x:.2e}, bar {bar_x:.2e})")
    assert e_u <= bar_u and e_x <= bar_x, (kind, e_u, bar_u, e_x, bar_x)


@pytest.mark.parametrize("m", [10, 200, 500, 2048])
def test_landmark_counts(nk, golden, m):
    """One wave (m = 10, 200), two (500) and eight (2048) per workgroup: HJB data of f8 (n = 1e4, Matern [ls]), landmarks drawn
    from its Y, gain K = 2 C[0], device loop against host loop over 200 steps from 0.9 to 0.  Bars as for the other kernels:
    10 x the host loop's own movement under a 1e-15 relative perturbation of K, floor 1e-10.
    Measured on an MI355X (controls / first state coordinate; device-vs-host, then the host loop's movement):
    m = 10: 2.6e-13 / 2.6e-14 (host loop: 2.4e-13 / 2.8e-14); 200: 6.4e-13 / 7.1e-13 (3.2e-13 / 3.6e-14); 500: 1.0e-12 /
    8.5e-13 (3.5e-13 / 1.3e-14); 2048: 1.2e-12 / 4.7e-13 (8.7e-17 / 0).  The bars are the 1e-10 floor everywhere."""
    g = golden("f8_hjb_config2.npz")
    X, Y = g["X"], g["Y"]
    rng = np.random.default_rng(31 + m)
    idx = rng.choice(X.shape[0], m, replace=False)
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([float(g["ls"])]), gamma=float(g["gamma"]), m=m)
    reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
    reg.fit(X, Y)
    K = _proportional_gain(reg)
    (e_u, e_x), (s_u, s_x) = _device_vs_host(nk, reg, K, nk.HJB(Ts=0.01), np.array([0.9]), np.zeros(1), 200)
    bar_u, bar_x = max(10.0 * s_u, 1e-10), max(10.0 * s_x, 1e-10)
    print(f"\n[hjb, m = {m}] device vs host loop: controls {e_u:.2e} (host loop moves {s_u:.2e}, bar {bar_u:.2e}), "
          f"states {e_x:.2e} (moves {s_x:.2e}, bar {bar_x:.2e})")
    assert e_u <= bar_u and e_x <= bar_x, (m, e_u, bar_u, e_x, bar_x)


# ---------------------------------------------------------------------------------------------------------------
# argument checks: the library's message, no launch
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks(nk, golden):
    from nys_koop_lqr_amd import _lib
    c = _hjb_case(nk, golden)
    reg, K = c["reg"], c["K"]
    with pytest.raises(ValueError, match="steps"):
        reg.closed_loop_plant(K, c["x0"], c["ref"], 0, c["plant"])
    with pytest.raises(ValueError, match="steps"):
        reg.closed_loop_plant(K, c["x0"], c["ref"], -3, c["plant"])
    with pytest.raises(ValueError, match="2 states"):  # a two-state plant on a one-state model
        reg.closed_loop_plant(K, c["x0"], c["ref"], 10, nk.DuffingOscillator(Ts=0.01))
    with pytest.raises(ValueError, match="plant"):
        reg.closed_loop_plant(K, c["x0"], c["ref"], 10, lambda x, u: x)
    with pytest.raises(ValueError, match="gain"):
        reg.closed_loop_plant(K[:, :-1], c["x0"], c["ref"], 10, c["plant"])
    # a model with two inputs
    rng = np.random.default_rng(3)
    reg2 = nk.KoopmanNystromRegressor(2, kernel=nk.KernelWrapper([1.0]), gamma=1e-6, m=8)
    reg2.nystrom_centers_output = rng.uniform(-1, 1, size=(1, 8))
    with pytest.raises(ValueError, match="one input"):
        reg2.closed_loop_plant(np.zeros((2, 8)), c["x0"], c["ref"], 10, c["plant"])
    # the raw entry point: unknown plant id, null pointer, a lock-step member context
    ctx = nk.get_context()
    h = reg._ensure_model()
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    x0, xr = np.array([[0.9]]), np.zeros((1, 1))
    ox, ou = np.full((1, 11, 1), 7.0), np.full((1, 10, 1), 7.0)
    args = (Kc.ctypes.data, x0.ctypes.data, xr.ctypes.data, 10, 1, ox.ctypes.data, ou.ctypes.data)
    assert ctx.lib.nk_plant_loop(ctx.handle, h, 5, 0.01, *args) == -1 and b"unknown plant" in ctx.lib.nk_last_error()
    assert ctx.lib.nk_plant_loop(ctx.handle, h, 2, 0.01, None, *args[1:]) == -1
    handles = (C.c_void_p * 2)()
    _lib.check(ctx.lib.nk_group_create(ctx.device, 2, handles))
    members = [_lib.Context(ctx.device, C.c_void_p(handles[i])) for i in range(2)]
    try:
        rc = ctx.lib.nk_plant_loop(members[0].handle, h, 2, 0.01, *args)
        msg = ctx.lib.nk_last_error()
        assert rc == -1 and b"lock-step" in msg, (rc, msg)
    finally:
        for mem in members:
            mem.close()
    assert np.all(ox == 7.0) and np.all(ou == 7.0)  # nothing ran
    # and the call still works afterwards on the ordinary context
    states, us = reg.closed_loop_plant(K, c["x0"], c["ref"], 10, c["plant"])
    assert states.shape == (1, 11) and np.all(np.isfinite(states)) and np.all(np.isfinite(us))
