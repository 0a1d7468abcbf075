"""The tile-dataflow blocked Cholesky (nk_chol_flow.hip) computes the same bits as the launch-per-step chain it replaces
(NYSKOOP_CHOL_FLOW=0, read per call): whole fits, the matrix square root, an ill-conditioned system whose diagonal blocks
take the correction step, and a non-positive-definite input that takes the fallback."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    return nk


def _flow_launches():
    """Dataflow Cholesky launches issued so far (nk_runtime_counters slot 6)."""
    from nys_koop_lqr_amd import _lib
    v = (C.c_uint64 * 7)()
    _lib.check(_lib.load_library().nk_runtime_counters(v, 7))
    return int(v[6])


def _both(monkeypatch, run, uses_flow=True):
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "1")
    n0 = _flow_launches()
    flow = run()
    n1 = _flow_launches()
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "0")
    chain = run()
    n2 = _flow_launches()
    monkeypatch.delenv("NYSKOOP_CHOL_FLOW")
    # the switch really selects the path: dataflow launches with 1 (where the shape takes it), none with 0
    assert (n1 > n0) == uses_flow
    assert n2 == n1
    assert len(flow) == len(chain)
    for a, b in zip(flow, chain):
        assert a.shape == b.shape
        assert np.array_equal(a, b)
    return flow


def _fit_data(n, d, p, seed):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, d))
    U = rng.standard_normal((n, p))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
    return np.hstack([S, U]), Y


# m = 700: eleven blocks, a short last one, 703 rows in the paired system and 700 + 3 / 40 right-hand-side rows;
# m = 40: a single block (below the dataflow's size threshold: both settings take the chain);
# m = 2000, d = 384: the headline's shape on fewer rows
@pytest.mark.parametrize("n,d,p,m,ls", [(3000, 40, 3, 700, 6.0), (600, 24, 3, 40, 5.0), (20000, 384, 6, 2000, 20.0)])
def test_fit_same_bits(nk, monkeypatch, n, d, p, m, ls):
    X, Y = _fit_data(n, d, p, seed=m)

    def run():
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(ls, ls, ls, d), gamma=1e-5, m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y[:m].T)
        reg.fit(X, Y)
        W = np.array(reg.C) @ np.hstack([np.array(reg.A), np.array(reg.B)])
        return [np.array(reg.A), np.array(reg.B), np.array(reg.C), W]

    A = _both(monkeypatch, run, uses_flow=m >= 256)[0]
    assert np.isfinite(A).all()


def _sqrtm(nk, P):
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    m = P.shape[0]
    P = np.ascontiguousarray(P)
    S, Si = np.empty((m, m)), np.empty((m, m))
    it, res = C.c_int32(), C.c_double()
    _lib.check(ctx.lib.nk_sqrtm_spd(ctx.handle, P.ctypes.data, m, m, S.ctypes.data, Si.ctypes.data, C.byref(it), C.byref(res)))
    return [S, Si, np.array([it.value], dtype=np.float64)]


def test_sqrtm_same_bits(nk, monkeypatch):
    rng = np.random.default_rng(5)
    m = 2000
    Q = rng.standard_normal((m, 2 * m))
    P = Q @ Q.T / (2 * m) + 1e-3 * np.eye(m)
    S, Si, _ = _both(monkeypatch, lambda: _sqrtm(nk, P))
    assert np.linalg.norm(S @ Si - np.eye(m)) / np.sqrt(m) < 1e-8


def test_illconditioned_sqrtm_same_bits(nk, monkeypatch):
    # eigenvalues from 1 down to 1e-11: the first diagonal blocks exceed the correction step's condition bound
    rng = np.random.default_rng(6)
    m = 300
    Qo, _ = np.linalg.qr(rng.standard_normal((m, m)))
    P = (Qo * np.logspace(0, -11, m)) @ Qo.T
    P = (P + P.T) / 2
    # the correction step of the diagonal-block products fires: some diagonal block of the factor has
    # ||L_jj||_F ||L_jj^-1||_F above CHOL_FIX_KAPPA = 8 * 64 (the verdict potrf_diag_kernel_body writes), some not
    L = np.linalg.cholesky(P)
    kappa = [np.linalg.norm(L[j:j + 64, j:j + 64]) * np.linalg.norm(np.linalg.inv(L[j:j + 64, j:j + 64]))
             for j in range(0, m, 64)]
    assert max(kappa) > 8 * 64 and min(kappa) < 8 * 64
    _both(monkeypatch, lambda: _sqrtm(nk, P))


def test_not_positive_definite_same_fallback(nk, monkeypatch):
    # one negative eigenvalue: the factorisation flags a non-positive pivot (same info word in both forms) and the square root
    # takes the coupled iteration, which then meets the negative eigenvalue -- same outcome either way
    rng = np.random.default_rng(7)
    m = 320
    Qo, _ = np.linalg.qr(rng.standard_normal((m, m)))
    ev = np.linspace(1.0, 2.0, m)
    ev[m // 2] = -0.5
    P = (Qo * ev) @ Qo.T
    P = (P + P.T) / 2

    def run():
        from nys_koop_lqr_amd import _lib
        try:
            return _sqrtm(nk, P)
        except _lib.NyskoopError as e:
            return [np.frombuffer(str(e).encode(), dtype=np.uint8).astype(np.float64)]

    _both(monkeypatch, run)
