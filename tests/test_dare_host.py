"""CPU: the NumPy statement of the batched Riccati solver (lqr.dare_doubling) against scipy on every fixture that stores
A, B, C, under the two bars of tests/dare_reference.py (built from scipy's own residual and its own movement under 1e-15
perturbations); the unstabilisable pair; and the host plumbing of the device gain (solve_lqr(device=True),
lqr_run_units(gain="device")) with stubbed device calls."""
import numpy as np
import pytest

import dare_reference as dr
from nys_koop_lqr_amd import harness, lqr, regressors


@pytest.mark.parametrize("name,c", dr.HOST_CASES, ids=[f"{n}-c{c}" for n, c in dr.HOST_CASES])
def test_doubling_meets_scipy_bars(name, c):
    A, B, Q, R = dr.fixture_problem(name, c)
    ref = dr.fixture_reference(name, c)
    P, K, iters, status = lqr.dare_doubling(A, B, Q, R)
    m = A.shape[0]
    r_bar, k_bar = dr.bars(ref, m)
    r, dk = dr.residual(A, B, Q, P, K), dr.relk(K, ref["K"])
    print(f"{name} c={c} m={m}: iterations {iters}, r {r:.3e} (scipy {ref['r']:.3e}, bar {r_bar:.3e}), "
          f"|K - K_scipy| {dk:.3e} = {dk / ref['movement']:.2f} x scipy's movement {ref['movement']:.3e}")
    assert status == 0 and 1 <= iters <= 40
    assert np.array_equal(P, P.T)
    assert r <= r_bar
    assert dk <= k_bar


def test_defaults_and_max_iter():
    A, B, Q, R = dr.fixture_problem("f12_m10")
    P, K, iters, status = lqr.dare_doubling(A, B, Q, R)
    P2, K2, iters2, status2 = lqr.dare_doubling(A, B, Q, R, tol=1e-13, max_iter=40)
    assert status == status2 == 0 and iters == iters2 and np.array_equal(K, K2) and np.array_equal(P, P2)
    P3, K3, iters3, status3 = lqr.dare_doubling(A, B, Q, R, max_iter=3)
    assert status3 == 1 and iters3 == 3 and np.all(np.isnan(K3)) and np.all(np.isnan(P3))


def test_unstabilisable_pair():
    A, B, Q, R = dr.UNSTABILISABLE
    with pytest.raises(np.linalg.LinAlgError):
        lqr.dlqr(A, B, Q, R)
    P, K, iters, status = lqr.dare_doubling(A, B, Q, R)
    assert status != 0 and iters <= 40
    assert K.shape == (1, 3) and np.all(np.isnan(K)) and np.all(np.isnan(P))


def test_indefinite_R_is_status_2():
    A, B, Q, _ = dr.fixture_problem("f12_m10")
    assert lqr.dare_doubling(A, B, Q, -np.eye(1))[3] == 2


class _Reg:
    """A fitted regressor as the gain plumbing sees it."""

    def __init__(self, tag, m=3):
        self.tag, self.n_inputs = tag, 1
        self.A, self.B, self.C = np.eye(m) * 0.5, np.ones((m, 1)), np.ones((1, m))


def test_solve_lqr_device_maps_status_to_linalgerror(monkeypatch):
    reg = regressors.KoopmanNystromRegressor(1)
    seen = []

    def stub(regs, c, R=None, tol=1e-13, max_iter=40):
        seen.append((list(regs), c, R))
        return [np.full((1, 3), 7.0)], np.array([stub.status], dtype=np.int32), np.array([5], dtype=np.int32)

    monkeypatch.setattr(regressors, "_lqr_gain_batch", stub)
    stub.status = 0
    K = reg.solve_lqr(c=0.25, device=True)
    assert np.array_equal(K, np.full((1, 3), 7.0)) and seen[0][0] == [reg] and seen[0][1] == 0.25 and seen[0][2] is None
    for status in (1, 2):
        stub.status = status
        with pytest.raises(np.linalg.LinAlgError):
            reg.solve_lqr(c=0.25, device=True)
    with pytest.raises(ValueError):
        reg.solve_lqr(Q=np.eye(3), device=True)


def _run(gain, **kw):
    units = [dict(m=3, tag=i) for i in range(6)]
    fit_fn = lambda X, Y, n_inputs, params, u, estimator: None if u["tag"] == 1 else _Reg(u["tag"])
    submitted = {}

    def loop_fn(regs, gains, x0, x_ref, num_steps, plant, u_opt=None, return_trajectories=False):
        submitted["tags"] = [r.tag for r in regs]
        submitted["gains"] = [np.array(g) for g in gains]
        n = len(regs)
        out = {name: np.array([10.0 * r.tag + k for r in regs]) for k, name in enumerate(harness.SCORE_NAMES)}
        if return_trajectories:
            out["states"] = np.stack([np.full((num_steps + 1, 2), float(r.tag)) for r in regs]) if n else np.zeros((0, num_steps + 1, 2))
            out["controls"] = np.stack([np.full(num_steps, float(r.tag)) for r in regs]) if n else np.zeros((0, num_steps))
        return out

    res = harness.lqr_run_units(np.zeros((4, 3)), np.zeros((4, 2)), 1, {}, units, None, np.zeros(2), np.zeros(2), 5,
                                fit_fn=fit_fn, loop_fn=loop_fn, gain=gain, return_trajectories=True, **kw)
    return res, submitted


def test_run_units_device_gain_with_stubbed_batch_call():
    calls = []

    def gain_batch_fn(regs, c):
        calls.append(([r.tag for r in regs], c))
        status = np.array([2 if r.tag == 3 else (1 if r.tag == 4 else 0) for r in regs], dtype=np.int32)
        Ks = [np.full((1, 3), np.nan if s else float(r.tag)) for r, s in zip(regs, status)]
        return Ks, status, np.full(len(regs), 9, dtype=np.int32)

    (scores, states, controls, timing), sub = _run("device", gain_batch_fn=gain_batch_fn, c=0.5)
    # one batch call for every fitted unit, in plan order; failed units (status 1 and 2) are not submitted to the loops
    assert calls == [([0, 2, 3, 4, 5], 0.5)]
    assert sub["tags"] == [0, 2, 5]
    assert [float(g[0, 0]) for g in sub["gains"]] == [0.0, 2.0, 5.0]
    for i in (1, 3, 4):
        assert np.all(np.isnan(scores[i])) and np.all(np.isnan(states[i])) and np.all(np.isnan(controls[i]))
    for i in (0, 2, 5):
        assert np.array_equal(scores[i], 10.0 * i + np.arange(4)) and np.all(states[i] == i) and np.all(controls[i] == i)
    assert set(timing) == {"fit_s", "gain_wait_s", "loop_s", "gain_cpu_s", "total_s"}
    assert timing["gain_cpu_s"] == 0.0 and timing["gain_wait_s"] >= 0.0


def test_run_units_host_gain_is_unchanged_and_arguments_checked():
    (scores, _, _, timing), sub = _run("host", gain_fn=lambda A, B, C: np.full((1, 3), 1.0))
    assert sub["tags"] == [0, 2, 3, 4, 5] and np.all(np.isnan(scores[1]))
    assert set(timing) == {"fit_s", "gain_wait_s", "loop_s", "gain_cpu_s", "total_s"}
    with pytest.raises(ValueError):
        _run("gpu")
    with pytest.raises(ValueError):
        _run("device", gain_fn=lambda A, B, C: None)
