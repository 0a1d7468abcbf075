"""GPU: the launch-chain Riccati solver (nk_dare_large, nk_model_lqr_gain; csrc/nk_dare_large.hip) at the smallest shapes at
which it can go wrong -- below, at and one past the LU's column block of 64, p up to the limit of 32, odd sizes, exact
multiples of 16 and 64, one past 256, 512 and 1024 -- under the two bars of tests/dare_reference.py on scipy's solution where
scipy is affordable and on the NumPy statement of the same iteration (lqr.dare_doubling, tests/dare_large_reference.py)
beyond; bit for bit against itself; its statuses and refusals; the model entry and the exact-kernel comparator.
Every device call runs a few seconds at the most.  The references are host work and the cost of this module: four scipy
solves at m = 257 (about 9 s) and four mirror solves per mirror-referenced problem (1 to 6 s each at m = 272 .. 1025)."""
import ctypes as C

import numpy as np
import pytest

import dare_reference as dr
import dare_large_reference as dl

pytestmark = pytest.mark.gpu

SCIPY_CASES = dl.SCIPY_CHEAP + dl.SCIPY_FIXTURES + dl.SCIPY_PAST_LIMIT
CASES = SCIPY_CASES + dl.MIRROR


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


_solved = {}


def _solve(nk, case):
    """(K, P, status, iterations, delta) of nk_dare_large on one case, solved once per process."""
    if case not in _solved:
        _solved[case] = nk.get_context().dare_large(*dl.problem(case))
    return _solved[case]


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case", CASES, ids=dl.label)
def test_case_meets_its_bars(nk, case):
    A, B, Q, R = dl.problem(case)
    m = A.shape[0]
    K, P, status, iters, delta = _solve(nk, case)
    scipy_referenced = case in SCIPY_CASES
    ref = dl.scipy_ref(case) if scipy_referenced else dl.mirror_ref(case)
    Pm, Km, itm, stm = dl.mirror_solution(case)
    r_bar, k_bar = dr.bars(ref, m)
    assert status == 0 and stm == 0 and 1 <= iters <= 40, (status, iters)
    r, dk, dm = dr.residual(A, B, Q, P, K), dr.relk(K, ref["K"]), dr.relk(K, Km)
    print(f"\n[{dl.label(case)}] m = {m}, p = {B.shape[1]}: {iters} steps (mirror {itm}), last step {delta:.1e}; residual {r:.2e} "
          f"({'scipy' if scipy_referenced else 'mirror'} {ref['r']:.2e}, bar {r_bar:.2e}) = {r / r_bar:.2f} of the bar; "
          f"|K - K_ref| = {dk / ref['movement']:.2f} x, |K - K_mirror| = {dm / ref['movement']:.2f} x the reference's movement "
          f"{ref['movement']:.2e}")
    assert np.array_equal(P, P.T)
    assert r <= r_bar and dk <= k_bar and dm <= k_bar, (r, r_bar, dk, dm, k_bar)


@pytest.mark.parametrize("case", [(17, 6, 1.1, 17), (129, 8, 1.1, 129), (272, 8, 1.1, 272)], ids=dl.label)
def test_same_bits_from_call_to_call_and_after_a_failing_call(nk, case):
    ctx = nk.get_context()
    K0, P0, st0, it0, d0 = _solve(nk, case)
    K1, P1, st1, it1, d1 = ctx.dare_large(*dl.problem(case))
    assert st0 == st1 == 0 and it0 == it1 and d0 == d1 and _bits(K0, K1) and _bits(P0, P1)
    Kb, Pb, stb, itb, _ = ctx.dare_large(*dr.UNSTABILISABLE)
    assert stb != 0 and np.all(np.isnan(Kb))
    K2, P2, st2, it2, _ = ctx.dare_large(*dl.problem(case))
    assert st2 == 0 and it2 == it0 and _bits(K0, K2) and _bits(P0, P2)


def test_device_operands_give_the_bits_of_host_operands(nk):
    import torch
    case = (129, 8, 1.1, 129)
    ctx = nk.get_context()
    K0, P0, st0, it0, _ = _solve(nk, case)
    dev = torch.device("cuda", ctx.device)
    ops = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in dl.problem(case)]
    torch.cuda.synchronize(dev)
    K1, P1, st1, it1, _ = ctx.dare_large(*ops)
    assert st1 == 0 and it1 == it0 and _bits(K0, K1) and _bits(P0, P1)
    # a padded device operand (leading dimension past the width), and a mix of host and device memory
    wide = torch.zeros((129, 200), dtype=torch.float64, device=dev)
    wide[:, :129] = ops[0]
    torch.cuda.synchronize(dev)
    A, B, Q, R = dl.problem(case)
    K2, P2, st2, it2, _ = ctx.dare_large(wide[:, :129], B, ops[2], R)
    assert st2 == 0 and it2 == it0 and _bits(K0, K2) and _bits(P0, P2)


def test_statuses(nk):
    ctx = nk.get_context()
    K, P, st, it, _ = ctx.dare_large(*dr.UNSTABILISABLE)
    assert st != 0 and it <= 40 and K.shape == (1, 3) and np.all(np.isnan(K)) and np.all(np.isnan(P))
    A, B, Q, R = dl.problem("f3")
    K, P, st, it, _ = ctx.dare_large(A, B, Q, R, max_iter=3, want_P=False)  # out_P = NULL
    assert P is None and st == 1 and it == 3 and np.all(np.isnan(K))
    K, P, st, it, _ = ctx.dare_large(A, B, Q, -np.eye(1))
    assert st == 2 and np.all(np.isnan(K)) and np.all(np.isnan(P))
    A, B, Q, R = dl.problem((17, 6, 1.1, 17))
    K, P, st, it, _ = ctx.dare_large(A, B, Q, -np.eye(6))
    assert st == 2 and np.all(np.isnan(K)) and np.all(np.isnan(P))


def _raw_call(lib, handle, m, p, A, lda, B, ldb, Q, ldq, R, ldr, K, P, status, iters):
    return lib.nk_dare_large(handle, m, p, A.ctypes.data, lda, B.ctypes.data, ldb, Q.ctypes.data, ldq, R.ctypes.data, ldr,
                             1e-13, 40, K.ctypes.data, P.ctypes.data, None, C.byref(status), C.byref(iters))


@pytest.mark.parametrize("what", ["m0", "m10241", "p33", "lda", "ldb", "ldq", "ldr", "lockstep"])
def test_refusals_touch_nothing(nk, what):
    """NK_ERR_BAD_ARG before anything is read, queued or allocated: small buffers stand in for the operands of a size past
    the limit; outputs and status keep their sentinels."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    m, p = 4, 2
    A, B, Q, R = np.eye(m) * 0.5, np.ones((m, p)), np.eye(m), np.eye(p)
    K, P = np.full((p, m), 7.0), np.full((m, m), 7.0)
    status, iters = C.c_int32(-7), C.c_int32(-7)
    args = dict(m=m, p=p, lda=m, ldb=p, ldq=m, ldr=p)
    args.update({"m0": dict(m=0), "m10241": dict(m=10241, lda=10241, ldq=10241), "p33": dict(p=33, ldb=33, ldr=33),
                 "lda": dict(lda=m - 1), "ldb": dict(ldb=p - 1), "ldq": dict(ldq=m - 1), "ldr": dict(ldr=p - 1),
                 "lockstep": {}}[what])
    handle, members = ctx.handle, None
    if what == "lockstep":
        members = (C.c_void_p * 2)()
        _lib.check(ctx.lib.nk_group_create(0, 2, members))
        handle = members[0]
    try:
        rc = _raw_call(ctx.lib, handle, args["m"], args["p"], A, args["lda"], B, args["ldb"], Q, args["ldq"], R, args["ldr"], K, P,
                       status, iters)
    finally:
        if members is not None:
            for mb in members:
                ctx.lib.nk_destroy(mb)
    assert rc == -1, (what, rc)
    assert np.all(K == 7.0) and np.all(P == 7.0) and status.value == -7 and iters.value == -7
    # the batched solver keeps its own limits
    if what == "p33":
        with pytest.raises(ValueError):
            ctx.dare_batch([np.eye(4) * 0.5], [np.ones((4, 9))], [np.eye(4)], [np.eye(9)])


@pytest.fixture(scope="module")
def hjb_model(nk, golden):
    """KoopmanNystromRegressor with m = 300 landmarks on the 800 rows of the HJB fixture."""
    g = golden("f4_hjb_matern.npz")
    np.random.seed(0)
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper(g["ls"]), gamma=float(g["gamma"]), m=300)
    reg.fit(g["X"].astype(np.float64), g["Y"].astype(np.float64))
    return reg


def _check_against_mirror(tag, A, B, Qh, K, P, extra=()):
    m = A.shape[0]
    ref = dl.mirror_reference(A, B, Qh, np.eye(B.shape[1]), seed=0)
    assert ref["status"] == 0
    r_bar, k_bar = dr.bars(ref, m)
    r, dk = dr.residual(A, B, Qh, P, K), dr.relk(K, ref["K"])
    rho = float(np.abs(np.linalg.eigvals(A)).max())
    print(f"\n[{tag}] m = {m}, spectral radius {rho:.5f}: mirror {ref['iters']} steps, movement {ref['movement']:.2e}; residual "
          f"{r:.2e} (mirror {ref['r']:.2e}, bar {r_bar:.2e}); |K - K_mirror| = {dk / k_bar:.2f} of the bar"
          + "".join(f"; {name} = {v / k_bar:.2f} of the bar" for name, v in extra))
    assert r <= r_bar and dk <= k_bar, (r, r_bar, dk, k_bar)
    for name, v in extra:
        assert v <= k_bar, (name, v, k_bar)
    return ref


def test_model_entry_past_the_batched_limit(nk, hjb_model):
    ctx = nk.get_context()
    reg = hjb_model
    A, B, Cm = np.array(reg.A), np.array(reg.B).reshape(300, 1), np.array(reg.C)
    Qh = 1.0 * dr.sym(Cm.T @ Cm)
    K = reg.solve_lqr(c=1.0, device=True)
    assert K.shape == (1, 300) and np.all(np.isfinite(K))
    Kd, Pd, st, it, _ = ctx.dare_large(A, B, Qh, np.eye(1))
    assert st == 0 and np.array_equal(Pd, Pd.T)
    _check_against_mirror("nystrom m = 300", A, B, Qh, K, Pd, extra=[("|K_model - K_large|", dr.relk(K, Kd))])
    # the seam gives the same gain, and reports the steps
    from nys_koop_lqr_amd import regressors
    Ks, status, iters = regressors._lqr_gain_batch([reg], 1.0)
    assert status[0] == 0 and iters[0] == it and _bits(Ks[0], K)
    with pytest.raises(ValueError):  # the batched entry still refuses the size
        ctx.dare_batch([A], [B], [Qh], [np.eye(1)])


def test_small_model_keeps_the_batched_solvers_bits(nk, golden):
    g = golden("f4_hjb_matern.npz")
    np.random.seed(1)
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper(g["ls"]), gamma=float(g["gamma"]), m=20)
    reg.fit(g["X"].astype(np.float64), g["Y"].astype(np.float64))
    ctx = nk.get_context()
    Kb, sb, ib = ctx.model_lqr_gain_batch([reg._ensure_model()], 1.0, dims=[(20, 1)])
    assert sb[0] == 0 and _bits(reg.solve_lqr(c=1.0, device=True), Kb[0])
    # the single-model entry takes the new path whatever m is: same problem, gain under the mirror's bars
    A, B, Cm = np.array(reg.A), np.array(reg.B).reshape(20, 1), np.array(reg.C)
    Qh = dr.sym(Cm.T @ Cm)
    Kl, sl, il = ctx.model_lqr_gain(reg._ensure_model(), 20, 1, 1.0)
    _, Pl, st, _, _ = ctx.dare_large(A, B, Qh, np.eye(1))
    assert sl == 0 and st == 0
    _check_against_mirror("nystrom m = 20", A, B, Qh, Kl, Pl, extra=[("|K_large - K_batch|", dr.relk(Kl, Kb[0]))])


def test_exact_comparator_gain_on_the_device(nk, golden):
    g = golden("f4c_hjb_exact_kernel.npz")
    reg = nk.KoopmanKernelRegressor(1, kernel=nk.KernelWrapper(g["ls"]), gamma=float(g["gamma"]))
    reg.fit(g["X"], g["Y"])
    N = g["X"].shape[0]
    K = reg.solve_lqr(c=1.0, device=True)
    assert K.shape == (1, N)
    A, B, Cm = np.array(reg.A), np.array(reg.B).reshape(N, 1), np.array(reg.C)
    Qh = dr.sym(Cm.T @ Cm)
    _, Pd, st, _, _ = nk.get_context().dare_large(A, B, Qh, np.eye(1))
    assert st == 0
    ref = _check_against_mirror("exact N = 300", A, B, Qh, K, Pd)
    assert float(np.abs(np.linalg.eigvals(A - B @ K)).max()) < 1.0
    # an un-pickled regressor (no device tensors) passes NumPy operators
    import pickle
    reg2 = pickle.loads(pickle.dumps(reg))
    assert "_dev_cache" not in reg2.__dict__
    K2 = reg2.solve_lqr(c=1.0, device=True)
    assert dr.relk(K2, K) <= dr.MULTIPLIER * ref["movement"]
