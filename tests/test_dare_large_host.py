"""CPU: what the launch-chain Riccati solver's GPU tests stand on, and its Python plumbing with the device calls stubbed.
The admission rule of tests/dare_large_reference.py (the mirror at or below 0.5 of both scipy bars on every scipy-referenced
problem), the mirror's convergence and movement on the mirror-referenced ones, the host form of
KoopmanKernelRegressor.solve_lqr, the routing of regressors._lqr_gain_batch between the batched and the single-model call,
and the status mapping of lqr.dlqr_device.  The scipy and mirror solves (up to m = 1025) are the cost of this module."""
import numpy as np
import pytest

import dare_reference as dr
import dare_large_reference as dl


@pytest.mark.parametrize("case", dl.SCIPY_CHEAP + dl.SCIPY_FIXTURES + dl.SCIPY_PAST_LIMIT, ids=dl.label)
def test_mirror_is_admitted_on_the_scipy_referenced_problems(case):
    A, B, Q, R = dl.problem(case)
    ref = dl.scipy_ref(case)
    P, K, iters, status = dl.mirror_solution(case)
    assert status == 0 and 1 <= iters <= 40
    r_bar, k_bar = dr.bars(ref, A.shape[0])
    r, dk = dr.residual(A, B, Q, P, K), dr.relk(K, ref["K"])
    print(f"\n[{dl.label(case)}] mirror: {iters} steps, residual {r / r_bar:.2f} of its bar, gain {dk / k_bar:.2f} of its bar")
    assert r <= dl.ADMISSION * r_bar and dk <= dl.ADMISSION * k_bar, (r / r_bar, dk / k_bar)


@pytest.mark.parametrize("case", dl.MIRROR, ids=dl.label)
def test_mirror_converges_and_moves_on_the_mirror_referenced_problems(case):
    ref = dl.mirror_ref(case)
    print(f"\n[{dl.label(case)}] mirror: {ref['iters']} steps, residual {ref['r']:.2e}, movement {ref['movement']:.2e}")
    assert ref["status"] == 0 and 1 <= ref["iters"] <= 40
    assert np.isfinite(ref["movement"]) and ref["movement"] > 0.0 and np.isfinite(ref["r"])


def test_mirror_reference_draws_the_perturbations_of_the_scipy_reference():
    """Same generator, same order of draws: with the solver replaced by one that returns its perturbed A, both references see
    the same matrices."""
    A, B, Q, R = dr.random_problem(5, 1, 1.1, 5)
    rng = np.random.default_rng(1000 + 5)
    want = []
    for _ in range(3):
        want.append(A * (1.0 + 1e-15 * rng.standard_normal(A.shape)))
        rng.standard_normal(B.shape)
    seen = []
    from nys_koop_lqr_amd import lqr
    orig = lqr.dare_doubling

    def spy(Ap, Bp, Qp, Rp, **kw):
        seen.append(np.array(Ap))
        return orig(Ap, Bp, Qp, Rp, **kw)

    lqr.dare_doubling = spy
    try:
        dl.mirror_reference(A, B, Q, R, seed=5)
    finally:
        lqr.dare_doubling = orig
    assert len(seen) == 4 and np.array_equal(seen[0], A)
    for got, exp in zip(seen[1:], want):
        assert np.array_equal(got, exp)


def test_exact_regressor_host_solve_lqr_is_dlqr_on_its_operators():
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import lqr
    A, B, _, _ = dr.random_problem(12, 2, 0.9, 3)
    Cm = np.random.default_rng(4).standard_normal((3, 12))
    reg = nk.KoopmanKernelRegressor(2, kernel=None, gamma=1e-3)
    reg.A, reg.B, reg.C = A, B, Cm  # the fit, by hand
    c = 0.3
    K_ref, _ = lqr.dlqr(A, B, c * dr.sym(Cm.T @ Cm), np.eye(2))
    assert np.array_equal(reg.solve_lqr(c=c), K_ref)
    Q, R = np.eye(12) * 0.5, np.array([[2.0, 0.1], [0.1, 1.0]])
    assert np.array_equal(reg.solve_lqr(Q=Q, R=R), lqr.dlqr(A, B, Q, R)[0])
    K1, _ = lqr.dlqr(A, B, 1.0 * dr.sym(Cm.T @ Cm), np.eye(2))
    assert np.array_equal(reg.solve_lqr(), K1)  # c defaults to 1


class _Reg:
    def __init__(self, m, p):
        self.m, self.n_inputs = m, p

    def _ensure_model(self):
        return ("handle", self.m, self.n_inputs)

    def _landmark_shape(self):
        return (2, self.m)


class _Ctx:
    def __init__(self):
        self.batch_calls, self.single_calls = [], []

    def model_lqr_gain_batch(self, models, c, R=None, tol=1e-13, max_iter=40, dims=None):
        self.batch_calls.append((list(models), list(dims)))
        Ks = [np.full((p, m), 100.0 * m + p) for m, p in dims]
        return Ks, np.zeros(len(models), dtype=np.int32), np.full(len(models), 7, dtype=np.int32)

    def model_lqr_gain(self, model, m, p, c, R=None, tol=1e-13, max_iter=40):
        self.single_calls.append((model, m, p))
        return np.full((p, m), -(100.0 * m + p)), 0, 9


def test_gain_batch_routes_by_the_batched_solvers_limits(monkeypatch):
    from nys_koop_lqr_amd import regressors, _lib
    ctx = _Ctx()
    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: ctx)
    dims = [(257, 1), (200, 1), (100, 9), (256, 8)]
    regs = [_Reg(m, p) for m, p in dims]
    Ks, status, iters = regressors._lqr_gain_batch(regs, 1.0)
    assert len(ctx.batch_calls) == 1 and ctx.batch_calls[0][1] == [(200, 1), (256, 8)]
    assert [h[1:] for h in ctx.batch_calls[0][0]] == [(200, 1), (256, 8)]
    assert [s[1:] for s in ctx.single_calls] == [(257, 1), (100, 9)]
    for (m, p), K, it in zip(dims, Ks, iters):  # results in the callers' order
        small = m <= 256 and p <= 8
        assert K.shape == (p, m) and np.all(K == (100.0 * m + p) * (1 if small else -1)) and it == (7 if small else 9)
    assert np.all(status == 0)
    # nothing past the limits: the one batch call, as before
    ctx2 = _Ctx()
    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: ctx2)
    regressors._lqr_gain_batch([_Reg(20, 1), _Reg(256, 8)], 1.0)
    assert len(ctx2.batch_calls) == 1 and not ctx2.single_calls


@pytest.mark.parametrize("status", [1, 2])
def test_dlqr_device_raises_on_a_non_zero_status(monkeypatch, status):
    from nys_koop_lqr_amd import lqr, _lib

    class Ctx:
        def dare_large(self, A, B, Q, R, tol=1e-13, max_iter=40, want_P=True):
            return np.full((1, 3), np.nan), np.full((3, 3), np.nan), status, 3, np.nan

    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: Ctx())
    with pytest.raises(np.linalg.LinAlgError):
        lqr.dlqr_device(*dr.UNSTABILISABLE)


def test_dlqr_device_returns_gain_and_solution(monkeypatch):
    from nys_koop_lqr_amd import lqr, _lib
    K, P = np.ones((1, 3)), np.eye(3)

    class Ctx:
        def dare_large(self, A, B, Q, R, tol=1e-13, max_iter=40, want_P=True):
            assert want_P
            return K, P, 0, 5, 1e-14

    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: Ctx())
    Kd, Pd = lqr.dlqr_device(*dr.UNSTABILISABLE)
    assert Kd is K and Pd is P
