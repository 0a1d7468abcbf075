"""GPU: the control sweep as one call (harness.lqr_sweep: lock-step fits, host gains in worker threads, ONE nk_plant_loop_multi
call scored on the device) against the plain loop it replaces -- reg.fit, reg.solve_lqr, reg.closed_loop_plant, host scores
-- with the same draws, for both estimators; a failing gain; and the reference's recorded Duffing control runs (f12)."""
import numpy as np
import pytest

from conftest import relf
from test_gpu_plant_loop import _duffing_case

pytestmark = pytest.mark.gpu

STEPS = 300
MS, SEEDS = [10, 20], [0, 1, 2]
X0, REF = np.array([-0.5, 0.0]), np.zeros(2)
U_OPT = 0.2 * np.exp(-np.arange(STEPS) / 100.0) * np.cos(np.arange(STEPS) / 11.0)  # something to score against
SCORES = ("sse_u", "ss_opt", "J", "u_absmax")


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def data(golden):
    g = golden("f12_duffing_full.npz")
    return np.ascontiguousarray(g["X"][:4000]), np.ascontiguousarray(g["Y"][:4000]), float(g["gamma"])


def _params(nk, data, estimator):
    if estimator == "spline":
        # the state bounds of the Duffing spline configuration (f15); its gamma = 1e-6 is for n = 69 900: on 4000 rows it
        # gives gains of order 1e2..1e3 under which the plain loop itself leaves the state bounds for some seeds
        return dict(gamma=1e-3, state_bounds_params=(1.0, 2.0))
    return dict(kernel=nk.KernelWrapper([1, 1]), gamma=data[2])


@pytest.fixture(scope="module")
def plain(nk, data):
    """The loop the sweep replaces, once per estimator: per planned unit fit, solve_lqr, closed_loop_plant, host scores."""
    from nys_koop_lqr_amd import harness
    X, Y, _ = data
    plant = nk.DuffingOscillator(Ts=0.01)
    out = {}
    for estimator in ("nystrom", "spline"):
        params = _params(nk, data, estimator)
        units = harness.lqr_plan(X, Y, 1, params, MS, SEEDS, estimator)
        rows = []
        for u in units:
            reg = harness.lqr_fit_unit(X, Y, 1, params, u, estimator)
            K = reg.solve_lqr(c=1.0)
            states, us = reg.closed_loop_plant(K, X0, REF, STEPS, plant)
            rows.append(dict(unit=u, A=np.array(reg.A), states=np.array(states.T), controls=np.array(us[0]),
                             scores=harness.control_scores(states, us, U_OPT)))
        out[estimator] = rows
    return out


def _same_bits(a, b):
    """Bit for bit, NaN included (a loop that leaves the state bounds does so in both runs, with the same bits)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _compare(res, rows, skip=()):
    bound = 2 * (STEPS + 1) * np.finfo(np.float64).eps
    for r in rows:
        si, k = r["unit"]["si"], r["unit"]["k"]
        if (si, k) in skip:
            continue
        assert _same_bits(res["states"][si, k], r["states"]), (si, k)
        assert _same_bits(res["controls"][si, k], r["controls"]), (si, k)
        for name in ("J", "u_absmax"):  # equal; a NaN of the host loop is a NaN of the device (the sign of a NaN is the machine's)
            assert np.array_equal(res[name][si, k], r["scores"][name], equal_nan=True), (name, si, k)
        for name in ("sse_u", "ss_opt", "rmse_control"):
            got, want = res[name][si, k], r["scores"][name]
            if np.isfinite(want):
                assert abs(got - want) <= bound * want, (name, si, k, got, want)
            else:  # a diverged loop: the sum is inf or NaN on both sides
                assert np.array_equal(got, want, equal_nan=True), (name, si, k, got, want)


@pytest.mark.parametrize("estimator", ["nystrom", "spline"])
def test_sweep_equals_the_plain_loop(nk, data, plain, estimator):
    """Duffing data cut to 4000 rows, ms = [10, 20], seeds 0..2, 300 steps.  Trajectories bit for bit; J and u_absmax equal;
    sse_u, ss_opt (and the RMSE formed from them) within 2 (steps + 1) eps relative of the host's step-order sums -- sums of
    non-negative terms, each side within steps * eps of the exact sum.  The same for batch = 0 (no lock-step pool)."""
    from nys_koop_lqr_amd import harness
    X, Y, _ = data
    plant = nk.DuffingOscillator(Ts=0.01)
    rows = plain[estimator]
    finite = [bool(np.all(np.isfinite(r["states"]))) for r in rows]
    print(f"\n[{estimator}] plain loop: units with finite states {finite}")
    assert sum(finite) >= 4  # most loops of the plain run stay inside the state bounds: the comparison is about numbers
    for batch in (4, 0):
        res = harness.lqr_sweep(X, Y, 1, _params(nk, data, estimator), MS, SEEDS, plant, X0, REF, STEPS, estimator=estimator,
                                u_opt=U_OPT, batch=batch, workers=2, return_trajectories=True)
        assert res["J"].shape == (3, 2) and res["states"].shape == (3, 2, STEPS + 1, 2) and res["controls"].shape == (3, 2, STEPS)
        assert not np.any(np.isnan(res["ss_opt"])) and np.all(res["ss_opt"] > 0)  # every unit ran
        print(f"\n[{estimator}, batch = {batch}] rmse_control\n{res['rmse_control']}\ntiming {res['timing']}")
        _compare(res, rows)
    # scores only: the same tables
    only = harness.lqr_sweep(X, Y, 1, _params(nk, data, estimator), MS, SEEDS, plant, X0, REF, STEPS, estimator=estimator,
                             u_opt=U_OPT, batch=4, workers=2)
    assert "states" not in only and all(_same_bits(only[name], res[name]) for name in SCORES)  # device against device


def test_a_failing_gain_is_nan_and_the_rest_is_unchanged(nk, data, plain):
    from nys_koop_lqr_amd import harness
    X, Y, _ = data
    plant = nk.DuffingOscillator(Ts=0.01)
    rows = plain["nystrom"]
    victim = next(r for r in rows if (r["unit"]["si"], r["unit"]["k"]) == (1, 1))
    default = harness.lqr_default_gain(1.0)

    def gain_fn(A, B, C):
        if A.shape == victim["A"].shape and np.array_equal(A, victim["A"]):
            raise np.linalg.LinAlgError("no stabilising solution")
        return default(A, B, C)

    res = harness.lqr_sweep(X, Y, 1, _params(nk, data, "nystrom"), MS, SEEDS, plant, X0, REF, STEPS, gain_fn=gain_fn,
                            u_opt=U_OPT, batch=4, workers=2, return_trajectories=True)
    for name in SCORES + ("rmse_control",):
        assert np.isnan(res[name][1, 1]) and np.sum(np.isnan(res[name])) == 1, name
    assert np.all(np.isnan(res["states"][1, 1])) and np.all(np.isnan(res["controls"][1, 1]))
    _compare(res, rows, skip={(1, 1)})


def test_sweep_meets_the_bars_of_the_recorded_duffing_runs(nk, golden):
    """The full f12 inputs (n = 69 900), seeds 0..2 at m = 20, 2000 steps: the sweep draws the reference's landmarks, fits,
    solves K = dlqr(A, B, C^T C, I) and runs the three loops in one call; controls and states of every seed against the
    reference's own run under the bars of the single-launch test (tests/test_gpu_plant_loop.py, _duffing_case)."""
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    cases = [_duffing_case(nk, golden, s) for s in SEEDS]
    steps = cases[0]["steps"]
    res = harness.lqr_sweep(np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"]), 1,
                            dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"])), [20], SEEDS, cases[0]["plant"],
                            cases[0]["x0"], cases[0]["ref"], steps, batch=3, workers=2, return_trajectories=True)
    assert steps == 2000 and res["controls"].shape == (3, 1, steps) and not np.any(np.isnan(res["J"]))
    for s, c in zip(SEEDS, cases):
        assert np.array_equal(res["units"][s]["marks"], g[f"lqr_idx_{s}"])
        e_u = relf(res["controls"][s, 0][None], c["us"])
        e_x = relf(res["states"][s, 0].T, c["states"])
        print(f"\n[duffing seed {s}] sweep vs reference: controls {e_u:.2e} (bar {c['bar_u']:.2e}), states {e_x:.2e} "
              f"(bar {c['bar_x']:.2e}); J {res['J'][s, 0]!r}, max |u| {res['u_absmax'][s, 0]!r}")
        assert e_u <= c["bar_u"] and e_x <= c["bar_x"], (s, e_u, e_x)
