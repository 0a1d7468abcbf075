"""CPU: the package's plants (nys_koop_lqr_amd/dynamical_systems.py) and the library's host build of the same maps
(nk_plant_step, csrc/nk_plant.h) against trajectories the reference recorded, and the double integrator against its closed
form."""
import numpy as np
import pytest

from conftest import relf


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def _replay(step, x0, controls):
    """x_{t+1} = step(x_t, u_t) over the columns of `controls` (1 x T); returns the states (d x (T + 1))."""
    x = np.asarray(x0, dtype=np.float64).reshape(-1, 1)
    out = [x]
    for t in range(controls.shape[1]):
        x = np.asarray(step(x, controls[:, t].reshape(-1, 1)), dtype=np.float64).reshape(-1, 1)
        out.append(x)
    return np.hstack(out)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_duffing_replays_the_reference_trajectory(lib, golden, seed):
    """f12: `lqr_states_{seed}` is the reference's open-loop replay of `lqr_us_{seed}` from (-0.5, 0) with Ts = 0.01
    (benchmark_lqr_classic.py:91-97), 2000 steps.  Bar 1e-12 relative Frobenius: a restatement in the reference's order of
    operations reproduces it to 0, a reordered evaluation to 1e-13..1e-12, a wrong k4 or sign misses by many orders."""
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    us, ref = g[f"lqr_us_{seed}"], g[f"lqr_states_{seed}"]
    assert us.shape == (1, 2000) and ref.shape == (2, 2001)
    plant = nk.DuffingOscillator(Ts=0.01)
    assert plant.Ts == 0.01 and plant.plant_id == 0 and plant.n_states == 2
    x0 = np.array([[-0.5], [0.0]])
    e_np = relf(_replay(plant.update_SOM, x0, us), ref)
    e_lib = relf(_replay(plant.step_library, x0, us), ref)
    e_harness = relf(harness.open_loop_control(plant.update_SOM, x0, us), ref)
    print(f"\nduffing seed {seed}: update_SOM {e_np:.2e}, nk_plant_step {e_lib:.2e} from the reference's states")
    assert e_np < 1e-12 and e_lib < 1e-12 and e_harness < 1e-12


def test_hjb_replays_the_reference_trajectory(lib, golden):
    """f8: `cl_x` are the states the reference's plant-in-the-loop run visited from 0.9 under `cl_u` (benchmark_lqr_hjb.py:73-97),
    Ts = 0.01.  Bar 1e-12 relative Frobenius, as for the Duffing oscillator."""
    import nys_koop_lqr_amd as nk
    g = golden("f8_hjb_config2.npz")
    us, ref = g["cl_u"].reshape(1, -1), g["cl_x"]
    plant = nk.HJB(Ts=0.01)
    assert plant.plant_id == 2 and plant.n_states == 1
    x0 = np.array([[0.9]])
    e_np = relf(_replay(plant.update_SOM, x0, us)[0, :-1], ref)
    e_lib = relf(_replay(plant.step_library, x0, us)[0, :-1], ref)
    print(f"\nhjb: update_SOM {e_np:.2e}, nk_plant_step {e_lib:.2e} from the reference's states")
    assert e_np < 1e-12 and e_lib < 1e-12


def test_double_integrator_closed_form(lib):
    """No recorded trajectory exists for the double integrator.  For a constant input this Runge-Kutta variant is exact:
    x2' = x2 + Ts u, x1' = x1 + Ts x2 + Ts^2 u / 2.  Bar 1e-14 relative (rounding only), 300 steps chained."""
    import nys_koop_lqr_amd as nk
    rng = np.random.default_rng(5)
    for Ts in (0.01, 0.05):
        plant = nk.DoubleIntegrator(Ts=Ts)
        assert plant.plant_id == 1 and plant.n_states == 2
        for _ in range(5):
            x = rng.uniform(-1.0, 1.0, size=(2, 1))
            u = float(rng.uniform(-2.0, 2.0))
            xa, xb, xc = x.copy(), x.copy(), x.copy()
            for _ in range(300):
                xa = plant.update_SOM(xa, np.array([[u]]))
                xb = plant.step_library(xb, u).reshape(2, 1)
                xc = np.array([[xc[0, 0] + Ts * xc[1, 0] + Ts * Ts * u / 2], [xc[1, 0] + Ts * u]])
            assert relf(xa, xc) < 1e-14 and relf(xb, xc) < 1e-14, (relf(xa, xc), relf(xb, xc))


def test_package_plants_and_library_plants_agree_bit_for_bit(lib):
    """update_SOM (NumPy) and nk_plant_step (the host build of the function the device loop inlines) are the same IEEE
    operations in the same order: identical bits, also for a batch of states in the columns."""
    import nys_koop_lqr_amd as nk
    rng = np.random.default_rng(11)
    for plant in (nk.DuffingOscillator(Ts=0.01), nk.DoubleIntegrator(Ts=0.02), nk.HJB(Ts=0.01)):
        d = plant.n_states
        X = rng.uniform(-1.0, 1.0, size=(d, 40))
        U = rng.uniform(-3.0, 3.0, size=(1, 40))
        batched = plant.update_SOM(X, U)
        assert batched.shape == (d, 40)
        for i in range(40):
            one = plant.update_SOM(X[:, i], U[:, i:i + 1])
            lib_one = plant.step_library(X[:, i], U[0, i])
            assert np.array_equal(one.reshape(-1), lib_one) and np.array_equal(batched[:, i], lib_one)


def test_plant_step_rejects_bad_arguments(lib):
    from nys_koop_lqr_amd import _lib
    x, u, out = np.zeros(2), np.zeros(1), np.zeros(2)
    assert lib.nk_plant_step(7, 0.01, x.ctypes.data, u.ctypes.data, out.ctypes.data) == -1
    assert b"unknown plant" in lib.nk_last_error()
    assert lib.nk_plant_step(0, 0.01, None, u.ctypes.data, out.ctypes.data) == -1
    assert (_lib.NK_PLANT_DUFFING, _lib.NK_PLANT_DOUBLE_INTEGRATOR, _lib.NK_PLANT_HJB) == (0, 1, 2)
