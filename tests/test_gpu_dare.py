"""GPU: the batched Riccati solver (nk_dare_batch, nk_model_lqr_gain_batch; csrc/nk_dare.hip, one workgroup per problem)
at the smallest shapes at which the kernel can go wrong -- below, at and one row past an MFMA tile, several inputs, the
fixture operators at m = 50, 100, 200 and the limits m = 256, p = 8 -- against scipy under the two bars of
tests/dare_reference.py (10 x scipy's own residual / 10 x scipy's own movement under 1e-15 perturbations), against the NumPy
statement of the same iteration (lqr.dare_doubling) under the same gain bar, and bit for bit against itself: alone, in
batches of different order, next to a failing problem.  The random problems at m = 256 are the unstable ones only (rho =
1.1): four scipy solves of that size per problem are the cost of this module."""
import ctypes as C

import numpy as np
import pytest

import dare_reference as dr

pytestmark = pytest.mark.gpu

# (label, m, p, what it probes)
SHAPES = [("r1", 1, 1), ("r5", 5, 1), ("r16", 16, 1), ("r17", 17, 6), ("r33", 33, 1), ("f3", 50, 1), ("f10", 100, 6),
          ("f8", 200, 1), ("r256", 256, 8)]


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def problems():
    """label -> dict(A, B, Q, R, ref): the nine shapes (random ones at rho = 1.1), the stable twins of the small random
    shapes and the second m = 200 fixture.  References are computed once and never modified."""
    out = {}
    for label, m, p in SHAPES:
        if label.startswith("r"):
            A, B, Q, R = dr.random_problem(m, p, 1.1, seed=m)
            out[label] = dict(A=A, B=B, Q=Q, R=R, ref=dr.reference(A, B, Q, R, seed=m))
            if m < 256:
                A, B, Q, R = dr.random_problem(m, p, 0.9, seed=1000 + m)
                out[label + "s"] = dict(A=A, B=B, Q=Q, R=R, ref=dr.reference(A, B, Q, R, seed=1000 + m))
        else:
            A, B, Q, R = dr.fixture_problem(label)
            assert A.shape == (m, m) and B.shape == (m, p)
            out[label] = dict(A=A, B=B, Q=Q, R=R, ref=dr.fixture_reference(label))
    A, B, Q, R = dr.fixture_problem("f12_m200")
    out["f12_m200"] = dict(A=A, B=B, Q=Q, R=R, ref=dr.fixture_reference("f12_m200"))
    return out


def _solve(nk, probs, **kw):
    ctx = nk.get_context()
    return ctx.dare_batch([q["A"] for q in probs], [q["B"] for q in probs], [q["Q"] for q in probs],
                          [q["R"] for q in probs], **kw)


@pytest.fixture(scope="module")
def solo(nk, problems):
    """Every problem solved alone: label -> (K, P, status, iterations, delta)."""
    out = {}
    for label, q in problems.items():
        Ks, Ps, st, it, dl = _solve(nk, [q])
        out[label] = (Ks[0], Ps[0], int(st[0]), int(it[0]), float(dl[0]))
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_every_shape_meets_the_scipy_bars(nk, problems, solo):
    from nys_koop_lqr_amd import lqr
    misses = []
    for label, q in problems.items():
        K, P, status, iters, delta = solo[label]
        m, ref = q["A"].shape[0], q["ref"]
        r_bar, k_bar = dr.bars(ref, m)
        Pm, Km, itm, stm = lqr.dare_doubling(q["A"], q["B"], q["Q"], q["R"])
        assert status == 0 and stm == 0 and 1 <= iters <= 40, (label, status, iters)
        r, dk, dm = dr.residual(q["A"], q["B"], q["Q"], P, K), dr.relk(K, ref["K"]), dr.relk(K, Km)
        print(f"\n[{label}] m = {m}, p = {q['B'].shape[1]}: {iters} steps (mirror {itm}), last step {delta:.1e}; residual {r:.2e} "
              f"(scipy {ref['r']:.2e}, bar {r_bar:.2e}); |K - K_scipy| = {dk / ref['movement']:.2f} x, |K - K_mirror| = "
              f"{dm / ref['movement']:.2f} x scipy's movement {ref['movement']:.2e}")
        assert np.array_equal(P, P.T), label
        if not (r <= r_bar and dk <= k_bar and dm <= k_bar):
            misses.append((label, r, r_bar, dk, dm, k_bar))
    assert not misses, misses


def test_batch_invariance(nk, problems, solo):
    """A problem's K, P and iteration count have the same bits alone, in a batch of the nine shapes in two orders, and
    next to a failing problem."""
    labels = [s[0] for s in SHAPES]
    bad = dict(zip("ABQR", dr.UNSTABILISABLE))
    for order in (labels, labels[::-1][3:] + labels[::-1][:3]):
        for with_bad in (False, True):
            seq = [problems[l] for l in order]
            if with_bad:
                seq = seq[:4] + [bad] + seq[4:]
            Ks, Ps, st, it, _ = _solve(nk, seq)
            if with_bad:
                assert st[4] != 0 and np.all(np.isnan(Ks[4])) and np.all(np.isnan(Ps[4]))
                Ks, Ps, st, it = Ks[:4] + Ks[5:], Ps[:4] + Ps[5:], np.delete(st, 4), np.delete(it, 4)
            for l, K, P, s, i in zip(order, Ks, Ps, st, it):
                assert int(s) == 0 and int(i) == solo[l][3], (l, s, i)
                assert _bits(K, solo[l][0]) and _bits(P, solo[l][1]), l


def test_status_of_a_failing_problem_in_a_batch_of_three(nk, problems, solo):
    bad = dict(zip("ABQR", dr.UNSTABILISABLE))
    Ks, Ps, st, it, _ = _solve(nk, [problems["r17"], bad, problems["f3"]])
    assert st[1] != 0 and it[1] <= 40 and Ks[1].shape == (1, 3) and np.all(np.isnan(Ks[1])) and np.all(np.isnan(Ps[1]))
    for k, l in ((0, "r17"), (2, "f3")):
        assert st[k] == 0 and _bits(Ks[k], solo[l][0]) and _bits(Ps[k], solo[l][1]) and it[k] == solo[l][3]
    # max_iter reached is status 1, outputs NaN; P may be skipped
    Ks, Ps, st, it, _ = _solve(nk, [problems["f3"]], max_iter=3, want_P=False)
    assert Ps is None and st[0] == 1 and it[0] == 3 and np.all(np.isnan(Ks[0]))


@pytest.mark.parametrize("m,p", [(257, 1), (4, 9)])
def test_sizes_past_the_limits_are_refused(nk, m, p):
    """NK_ERR_BAD_ARG naming the problem, before anything is queued: the outputs of EVERY problem of the call are untouched."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    ok = dict(A=np.eye(3) * 0.5, B=np.ones((3, 1)), Q=np.eye(3), R=np.eye(1), K=np.full((1, 3), 7.0), P=np.full((3, 3), 7.0))
    bad = dict(A=np.eye(m) * 0.5, B=np.ones((m, p)), Q=np.eye(m), R=np.eye(p), K=np.full((p, m), 7.0), P=np.full((m, m), 7.0))
    arr = (_lib.DareProblem * 2)()
    for a, q in zip(arr, (ok, bad)):
        a.m, a.p = q["B"].shape
        a.A, a.lda, a.B, a.ldb = q["A"].ctypes.data, a.m, q["B"].ctypes.data, a.p
        a.Q, a.ldq, a.R, a.ldr = q["Q"].ctypes.data, a.m, q["R"].ctypes.data, a.p
        a.out_K, a.out_P, a.out_delta = q["K"].ctypes.data, q["P"].ctypes.data, None
    status = np.full(2, -7, dtype=np.int32)
    iters = np.full(2, -7, dtype=np.int32)
    rc = ctx.lib.nk_dare_batch(ctx.handle, arr, 2, 1e-13, 40, status.ctypes.data_as(C.POINTER(C.c_int32)),
                               iters.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == -1 and b"problem 1" in ctx.lib.nk_last_error()
    for q in (ok, bad):
        assert np.all(q["K"] == 7.0) and np.all(q["P"] == 7.0)
    assert np.all(status == -7) and np.all(iters == -7)
    with pytest.raises(ValueError):
        ctx.dare_batch([bad["A"]], [bad["B"]], [bad["Q"]], [bad["R"]])


@pytest.fixture(scope="module")
def duffing_models(nk, golden):
    """Duffing subset (2000 rows), m in {5, 20}, Nystrom and spline: fitted regressors."""
    from nys_koop_lqr_amd import harness
    g = golden("f12_duffing_full.npz")
    X, Y = np.ascontiguousarray(g["X"][:2000]), np.ascontiguousarray(g["Y"][:2000])
    regs = []
    for estimator, params in (("nystrom", dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))),
                              ("spline", dict(gamma=1e-3, state_bounds_params=(1.0, 2.0)))):
        for u in harness.lqr_plan(X, Y, 1, params, [5, 20], [0], estimator):
            reg = harness.lqr_fit_unit(X, Y, 1, params, u, estimator)
            assert reg is not None
            regs.append(reg)
    return regs


def test_model_entry_equals_the_batch_entry_and_meets_the_bars(nk, duffing_models):
    from nys_koop_lqr_amd import regressors
    ctx = nk.get_context()
    c = 1.0
    Ks, status, iters = regressors._lqr_gain_batch(duffing_models, c)
    assert np.all(status == 0), status
    As = [np.array(r.A) for r in duffing_models]
    Bs = [np.array(r.B) for r in duffing_models]
    Qs = [ctx.model_lqr_cost(r._ensure_model(), r.A.shape[0], c) for r in duffing_models]
    Kb, Pb, sb, ib, _ = ctx.dare_batch(As, Bs, Qs, [np.eye(1)] * len(As))
    for k, reg in enumerate(duffing_models):
        m = As[k].shape[0]
        Qh = c * dr.sym(np.array(reg.C).T @ np.array(reg.C))
        assert np.array_equal(Qs[k], Qs[k].T) and np.allclose(Qs[k], Qh, rtol=0, atol=8 * np.finfo(float).eps * np.abs(Qh).max())
        assert sb[k] == 0 and ib[k] == iters[k] and _bits(Kb[k], Ks[k]), k
        assert _bits(reg.solve_lqr(c=c, device=True), Ks[k]), k  # one model through the same entry
        ref = dr.reference(As[k], Bs[k], Qh, np.eye(1), seed=k)
        K_host = reg.solve_lqr(c=c)
        r_bar, k_bar = dr.bars(ref, m)
        dk, r = dr.relk(Ks[k], K_host), dr.residual(As[k], Bs[k], Qh, Pb[k], Kb[k])
        print(f"\n[{type(reg).__name__}, m = {m}] {iters[k]} steps; residual {r:.2e} (scipy {ref['r']:.2e}, bar {r_bar:.2e}); "
              f"|K_dev - K_host| = {dk / ref['movement']:.2f} x scipy's movement {ref['movement']:.2e}")
        assert r <= r_bar and dk <= k_bar, (k, r, r_bar, dk, k_bar)


def test_model_entry_is_refused_inside_a_lockstep_group(nk, duffing_models):
    from nys_koop_lqr_amd import _lib
    lib = _lib.load_library()
    members = (C.c_void_p * 2)()
    _lib.check(lib.nk_group_create(0, 2, members))
    try:
        h0 = duffing_models[0]._ensure_model()
        h = (C.c_void_p * 1)(h0.value if isinstance(h0, C.c_void_p) else h0)
        out = np.full(5, 7.0)
        st = np.full(1, -7, dtype=np.int32)
        rc = lib.nk_model_lqr_gain_batch(members[0], h, 1, 1.0, None, 1e-13, 40, out.ctypes.data,
                                         st.ctypes.data_as(C.POINTER(C.c_int32)), None)
        assert rc == -1 and np.all(out == 7.0) and st[0] == -7
    finally:
        for mb in members:
            lib.nk_destroy(mb)
