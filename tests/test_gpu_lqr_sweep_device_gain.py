"""GPU: the control sweep with the gains from the batched device Riccati solver (harness.lqr_sweep(gain="device"): lock-step
fits, ONE nk_model_lqr_gain_batch call, ONE nk_plant_loop_multi call) against the plain loop it replaces -- reg.fit,
reg.solve_lqr(c, device=True), reg.closed_loop_plant -- bit for bit, for both estimators and with and without the lock-step
pool; and the reference's recorded Duffing control runs (f12) under the fixture's own bars, which
tests/test_gpu_lqr_sweep.py applies to the host gain."""
import numpy as np
import pytest

from conftest import relf
from test_gpu_plant_loop import _duffing_case

pytestmark = pytest.mark.gpu

STEPS = 200
MS, SEEDS = [5, 20], [0, 1]
X0, REF = np.array([-0.5, 0.0]), np.zeros(2)
U_OPT = 0.2 * np.exp(-np.arange(STEPS) / 100.0) * np.cos(np.arange(STEPS) / 11.0)
SCORES = ("sse_u", "ss_opt", "J", "u_absmax")


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def data(golden):
    g = golden("f12_duffing_full.npz")
    return np.ascontiguousarray(g["X"][:2000]), np.ascontiguousarray(g["Y"][:2000]), float(g["gamma"])


def _params(nk, data, estimator):
    if estimator == "spline":
        return dict(gamma=1e-3, state_bounds_params=(1.0, 2.0))
    return dict(kernel=nk.KernelWrapper([1, 1]), gamma=data[2])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("estimator", ["nystrom", "spline"])
def test_device_gain_sweep_equals_the_plain_loop(nk, data, estimator):
    from nys_koop_lqr_amd import harness
    X, Y, _ = data
    plant = nk.DuffingOscillator(Ts=0.01)
    params = _params(nk, data, estimator)
    units = harness.lqr_plan(X, Y, 1, params, MS, SEEDS, estimator)
    rows = []
    for u in units:  # the plain loop, one unit at a time
        reg = harness.lqr_fit_unit(X, Y, 1, params, u, estimator)
        try:
            K = reg.solve_lqr(c=1.0, device=True)
        except np.linalg.LinAlgError:
            rows.append(None)
            continue
        states, us = reg.closed_loop_plant(K, X0, REF, STEPS, plant)
        rows.append(dict(reg=reg, K=K, states=np.array(states.T), controls=np.array(us[0])))
    live = [r for r in rows if r is not None]
    assert len(live) >= 3  # the comparison is about numbers, not about NaN
    # the scores of the plain loop's gains by the device's own scoring: the sweep must reproduce them bit for bit
    want = harness.plant_loop_multi([r["reg"] for r in live], [r["K"] for r in live], X0, REF, STEPS, plant, u_opt=U_OPT)
    for batch in (4, 0):
        res = harness.lqr_sweep(X, Y, 1, params, MS, SEEDS, plant, X0, REF, STEPS, estimator=estimator, c=1.0, u_opt=U_OPT,
                                batch=batch, workers=2, return_trajectories=True, gain="device")
        assert set(res["timing"]) == {"fit_s", "gain_wait_s", "loop_s", "gain_cpu_s", "total_s"} and res["timing"]["gain_cpu_s"] == 0.0
        print(f"\n[{estimator}, batch = {batch}] timing {res['timing']}")
        k = 0
        for u, r in zip(units, rows):
            si, kk = u["si"], u["k"]
            if r is None:
                assert all(np.isnan(res[name][si, kk]) for name in SCORES) and np.all(np.isnan(res["states"][si, kk]))
                continue
            assert _same_bits(res["states"][si, kk], r["states"]), (si, kk)
            assert _same_bits(res["controls"][si, kk], r["controls"]), (si, kk)
            for name in SCORES:
                assert _same_bits(res[name][si, kk], want[name][k]), (name, si, kk)
            k += 1


def test_device_gain_sweep_meets_the_bars_of_the_recorded_duffing_runs(nk, golden):
    """The full f12 inputs, seeds 0..2 at m = 20, 2000 steps, gains from the device solver: controls and states of every
    seed against the reference's own run under the bars of tests/test_gpu_lqr_sweep.py (f12b lqr_envelope_*).
    Measured ratios error / bar are printed; gain="host" stays the documented choice for replaying the reference."""
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    seeds = [0, 1, 2]
    cases = [_duffing_case(nk, golden, s) for s in seeds]
    steps = cases[0]["steps"]
    res = harness.lqr_sweep(np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"]), 1,
                            dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"])), [20], seeds, cases[0]["plant"],
                            cases[0]["x0"], cases[0]["ref"], steps, batch=3, workers=2, return_trajectories=True,
                            gain="device")
    assert steps == 2000 and res["controls"].shape == (3, 1, steps) and not np.any(np.isnan(res["J"]))
    misses = []
    for s, c in zip(seeds, cases):
        e_u = relf(res["controls"][s, 0][None], c["us"])
        e_x = relf(res["states"][s, 0].T, c["states"])
        print(f"\n[duffing seed {s}] device-gain sweep vs reference: controls {e_u:.2e} = {e_u / c['bar_u']:.2f} x bar, states "
              f"{e_x:.2e} = {e_x / c['bar_x']:.2f} x bar")
        if not (e_u <= c["bar_u"] and e_x <= c["bar_x"]):
            misses.append((s, e_u, c["bar_u"], e_x, c["bar_x"]))
    assert not misses, misses
