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


# ------------------------------------------------------------------------------------------------------------------------
# The give-up, end to end.  NYSKOOP_CHOL_FLOW_TEST_GIVEUP=<ticket>[,<nsys>[,<extra>]] makes the workgroup that draws that work
# item of a dataflow launch take the give-up branch at once (nobody waits); every recovery site of the host then runs for real.
# Each case is compared bit for bit with the same call on the chain, the counters (slot 5 give-ups, slot 6 dataflow launches,
# slot 3 coupled-iteration retries) say which launches were hit and that the re-run never took the dataflow launch, and an
# unhooked repeat on the same context shows that flag slots, arena and saved systems were left usable.
# ------------------------------------------------------------------------------------------------------------------------
HOOK = "NYSKOOP_CHOL_FLOW_TEST_GIVEUP"


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)


def _recovered(monkeypatch, run, hook, giveups, launches):
    import chol_reference as cr
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "0")
    chain = run()
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "1")
    monkeypatch.setenv(HOOK, hook)
    c0 = cr.counters()
    hooked = run()
    c1 = cr.counters()
    monkeypatch.delenv(HOOK)
    after = run()
    c2 = cr.counters()
    monkeypatch.delenv("NYSKOOP_CHOL_FLOW")
    # exactly the launches aimed at gave up; the re-runs took the chain (no further dataflow launch, so no second give-up)
    assert c1[5] - c0[5] == giveups and c1[6] - c0[6] == launches, (c0, c1)
    assert c1[3] == c0[3], "a give-up must not be counted (or handled) as a coupled-iteration retry"
    assert c2[5] == c1[5] and c2[6] - c1[6] == launches and c2[3] == c1[3], (c1, c2)
    _same(hooked, chain)
    _same(after, chain)
    return chain


def test_giveup_word_reaches_every_system(nk, monkeypatch):
    """nk_chol_aug does no recovery: the word comes back as it is, for BOTH systems, also when one of them had already recorded
    a non-positive pivot (first tile: long before the last ticket is drawn); the chain then finds that pivot again."""
    import chol_reference as cr
    ctx = nk.get_context()
    m, j = 321, 5
    bad = (cr.indefinite(m, j, seed=11), cr.rhs(64, m, 11), m)
    good = (cr.matrix("rbf", 256, 5), cr.rhs(40, 256, 5), 256)
    total = cr.flow_items([(m, 64), (256, 40)])
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "1")
    for systems in ([bad, good], [good, bad]):
        for ticket in (0, total // 2, total - 1):
            monkeypatch.setenv(HOOK, str(ticket))
            c0 = cr.counters()
            out = cr.chol_aug(ctx, systems)
            c1 = cr.counters()
            assert [o[2] for o in out] == [cr.CHOL_FLOW_GIVEUP] * 2 and [o[3] for o in out] == [0.0, 0.0], (ticket, out)
            assert c1[5] == c0[5] + 1 and c1[6] == c0[6] + 1
    # filters that do not match, and tickets outside the launch, leave the launch alone
    for hook in (str(total), "-1", "0,1", f"0,2,{m + 1}", "x"):
        monkeypatch.setenv(HOOK, hook)
        c0 = cr.counters()
        out = cr.chol_aug(ctx, [bad, good])
        c1 = cr.counters()
        assert out[0][2] == j + 1 and out[1][2] == 0, (hook, out[0][2], out[1][2])
        assert c1[5] == c0[5] and c1[6] == c0[6] + 1
    # ... and one that does match on all three
    monkeypatch.setenv(HOOK, "3,2,64")
    assert [o[2] for o in cr.chol_aug(ctx, [bad, good])] == [cr.CHOL_FLOW_GIVEUP] * 2
    monkeypatch.delenv(HOOK)
    flow = cr.chol_aug(ctx, [bad, good])
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "0")
    chain = cr.chol_aug(ctx, [bad, good])
    assert flow[0][2] == chain[0][2] == j + 1 and chain[1][2] == 0
    assert np.array_equal(np.tril(flow[1][0]), np.tril(chain[1][0])) and np.array_equal(flow[1][1], chain[1][1])


def _nystrom_run(nk, X, Y, d, p, m, ls):
    def run():
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(ls, ls, ls, d), gamma=1e-5, m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y[:m].T)
        reg.fit(X, Y)
        W = np.array(reg.C) @ np.hstack([np.array(reg.A), np.array(reg.B)])
        return [np.array(reg.A), np.array(reg.B), np.array(reg.C), W, np.array(reg.lift(X[:40, :d].T)),
                np.array(reg.predict(X[:40]))]
    return run


# m = 700 (not the early square-root form): the K_mm launch has one system, the regularised pair two
@pytest.mark.parametrize("hook,giveups", [("0,2", 1), ("9,2", 1), ("0,1", 1), ("30,1", 1), ("0", 2)],
                         ids=["pair", "pair_mid", "kmm", "kmm_mid", "both"])
def test_giveup_nystrom_fit_recovers(nk, monkeypatch, hook, giveups):
    n, d, p, m = 3000, 40, 3, 700
    X, Y = _fit_data(n, d, p, seed=m)
    out = _recovered(monkeypatch, _nystrom_run(nk, X, Y, d, p, m, 6.0), hook, giveups, launches=2)
    assert all(np.isfinite(a).all() for a in out)


def test_giveup_nystrom_fit_early_square_root(nk, monkeypatch):
    """m = 1024, even: the iteration is queued before the factorisation's verdict (NK_SQRT_RETRY + flow_gave_up)."""
    n, d, p, m = 20000, 384, 6, 1024
    X, Y = _fit_data(n, d, p, seed=2000)
    out = _recovered(monkeypatch, _nystrom_run(nk, X, Y, d, p, m, 20.0), "0,1", giveups=1, launches=2)
    assert all(np.isfinite(a).all() for a in out)


@pytest.mark.parametrize("m", [300, 2000])
def test_giveup_sqrtm_recovers(nk, monkeypatch, m):
    rng = np.random.default_rng(50 + m)
    Q = rng.standard_normal((m, 2 * m))
    P = Q @ Q.T / (2 * m) + 1e-3 * np.eye(m)
    S, Si, _ = _recovered(monkeypatch, lambda: _sqrtm(nk, P), "3", giveups=1, launches=1)
    assert np.linalg.norm(S @ Si - np.eye(m)) / np.sqrt(m) < 1e-8


@pytest.mark.parametrize("strict", [False, True])
def test_giveup_spline_fit_recovers(nk, monkeypatch, golden, strict):
    """Cloth case c3 (m = 500, full rank: ends in the Cholesky solve).  With strict mode on, a give-up is not a rank verdict."""
    from test_gpu_spline import cloth_data
    g, X, Y, traj, ctrl = cloth_data(golden)
    k = 3
    m, gamma = int(g["ms"][k]), float(g["gammas"][k])
    assert m == 500

    def run():
        reg = nk.KoopmanSplineRegressor(6, m=m, gamma=gamma)
        reg.centers = X[:, :192].T[:, g[f"c{k}_centers_idx"]]
        reg.fit(X, Y)
        assert reg.fit_stats_["rank_inner"] == m + 6
        return [np.array(reg.A), np.array(reg.B), np.array(reg.C), np.array(reg.predict(X[:30]))]

    ctx = nk.get_context()
    ctx.set_strict_spd(strict)
    try:
        _recovered(monkeypatch, run, "0", giveups=1, launches=1)
        _recovered(monkeypatch, run, "40", giveups=1, launches=1)
    finally:
        ctx.set_strict_spd(False)


def test_giveup_spline_fit_that_ends_in_the_svd(nk, monkeypatch, golden):
    """Cloth case c5 (m = 500, gamma = 1e-7): the pivots send it to the pseudo-inverse, which starts from the saved system."""
    from test_gpu_spline import cloth_data
    g, X, Y, traj, ctrl = cloth_data(golden)
    k = 5
    m, gamma = int(g["ms"][k]), float(g["gammas"][k])

    def run():
        reg = nk.KoopmanSplineRegressor(6, m=m, gamma=gamma)
        reg.centers = X[:, :192].T[:, g[f"c{k}_centers_idx"]]
        reg.fit(X, Y)
        assert reg.fit_stats_["rank_inner"] == int(g[f"c{k}_rank"])
        return [np.array(reg.A), np.array(reg.B), np.array(reg.C), np.array(reg.predict(X[:30]))]

    _recovered(monkeypatch, run, "0", giveups=1, launches=1)


def test_giveup_sharded_solve_recovers(nk, monkeypatch):
    """nk_nystrom_gram + nk_nystrom_solve (two shards), the pair launch of the solve hit."""
    n, d, p, m = 3000, 40, 3, 700
    X, Y = _fit_data(n, d, p, seed=m)

    def run():
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(6.0, 6.0, 6.0, d), gamma=1e-5, m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y[:m].T)
        gram = reg.gram_partial(X[:1700], Y[:1700]) + reg.gram_partial(X[1700:], Y[1700:])
        reg.fit_from_gram(gram, n, d)
        return [np.array(reg.A), np.array(reg.B), np.array(reg.C), np.array(reg.predict(X[:40]))]

    _recovered(monkeypatch, run, "5,2", giveups=1, launches=2)
