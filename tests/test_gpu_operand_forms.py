"""The dense building blocks of the C-ABI (nk_gemm, nk_gemm_f32, nk_solve_spd, nk_sqrtm_spd, nk_kernel_matrix) on padded,
odd and unaligned operands (tests/operand_forms.py): host arrays with ld > cols at a column offset, device tensors used in
place with an even or odd leading dimension, 16-byte aligned or 8 bytes past a 16-byte boundary, and host and device operands
mixed in one call.  Every operand lies in a sentinel-filled parent; after every call all guards of all operands are intact
(compared as bit patterns), the inputs are unchanged, the result is within a derived bar of a longdouble reference, and it has
the BITS of the baseline call (host, tight), because a form changes which load instruction a kernel uses, never its
arithmetic.  The one exception is stated in test_gemm.

Routes (launch_gemm, launch_kmat; tests/test_operand_forms_host.py asserts them through operand_forms.gemm_route / kmat_route):
  nk_gemm  (7,5,3) (33,17,130) (9,6,0), every form         gemm_small_kernel (strided scalar loads)
           (130,257,37|300|0) H0 H1 D0                      gemm_f64_kernel, vecA = vecB = 1; for (transA, transB) = (1, 0) and
                                                             K = 300 the LDS-DMA engine (tn_fast_ok true)
           the same, D1 D2 D3 on A, B, C                    gemm_f64_kernel, vecA = vecB = 0 (tn_fast_ok false at K = 300)
           the same, D3 on A only / B only / C only         vecA = 0, vecB = 1 / vecA = 1, vecB = 0 / both 1 (C is stored
                                                             by scalar stores on every engine)
  nk_kernel_matrix (9,7,5) every form                       kmat_small_kernel
           (70,64,3)  H0 H1 D0 / D1 D2 D3 / D3 on out        kmat_flat_kernel (gate true) / kmat_small_kernel (gate false)
           (130,66,2) H0 H1 D0 / D1 D2 D3 / D3 on out        kmat_flat_kernel / kmat_kernel with vecA = vecB = vecO = 0 / vecO = 0
           (130,67,19) H0 H1 D0 / D1 D2 D3 / D3 on one       kmat_kernel, all vec = 1 / all 0 / that one 0 (flat gate false: odd nB)
Figures (worst error / bar of each call family) are printed and, with NYSKOOP_OPERAND_FORMS_LOG set, appended to that file.

Measured on one MI355X, worst error / bar over all forms (the bars are derived in operand_forms.py / gram_reference.py and were
not touched afterwards): nk_gemm 0.22 at K = 3, 0.009 .. 0.11 at K = 37 .. 300, 0.33 at K = 0 (the one rounding of beta C against
gamma_3); nk_gemm_f32 0.02 / 0.11 / 0.008; nk_solve_spd relf 8.1e-16 (Cholesky) and 2.2e-14 (SVD branch, cap 5.6e-11);
nk_kernel_matrix 0.07 .. 0.30 for RBF, Matern and the spline, 0.16 .. 0.87 for the linear kernel (largest at d = 2, where
sigma0^2 dominates the entries); nk_sqrtm_spd at most 0.49 of a bar of sqrtm_reference.  Every bit comparison held, the
exception of test_gemm included; no form faulted."""
import ctypes as C
import os

import numpy as np
import pytest

import chol_reference as cr
import gram_reference as gr
import operand_forms as of
import pinv_reference as pr
import sqrtm_reference as sr
from conftest import relf

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not of.HAVE_LONGDOUBLE, reason=of.LONGDOUBLE_SKIP)]

ALL_FORMS = [("H1",) * 3, ("D0",) * 3, ("D1",) * 3, ("D2",) * 3, ("D3",) * 3,
             ("D3", "H0", "H0"), ("H0", "D3", "H0"), ("H0", "H0", "D3")]


@pytest.fixture(scope="module")
def ctx():
    import nys_koop_lqr_amd as nk
    return nk.get_context()


def _log(line):
    print(line)
    path = os.environ.get("NYSKOOP_OPERAND_FORMS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _last_error(ctx):
    return ctx.lib.nk_last_error().decode("utf-8", "replace")


# ---------------------------------------------------------------------------------------------------------------------
# nk_gemm
# ---------------------------------------------------------------------------------------------------------------------
def _gemm(ctx, tA, tB, M, N, K, alpha, beta, forms, As, Bs, C0):
    fa, fb, fc = forms
    a = of.Operand(fa, *As.shape, As)
    b = of.Operand(fb, *Bs.shape, Bs)
    c = of.Operand(fc, M, N, C0 if beta != 0.0 else None)  # beta == 0: C starts as the sentinel NaN and must not be read
    rc = of.call((a, b, c), lambda: ctx.lib.nk_gemm(ctx.handle, tA, tB, M, N, K, alpha, a.ptr, a.ld, b.ptr, b.ld, beta,
                                                    c.ptr, c.ld))
    assert rc == 0, (forms, rc, _last_error(ctx))
    of.check_inputs_and_guards(dict(A=(a, As), B=(b, Bs)), dict(C=c), tag=forms)
    return c.block()


@pytest.mark.parametrize("tA,tB", of.TRANSPOSITIONS)
@pytest.mark.parametrize("M,N,K", of.GEMM_SHAPES)
def test_gemm(ctx, M, N, K, tA, tB):
    """Bit equality with the baseline holds whenever the same kernel runs.  The exception, from launch_gemm
    (nk_gemm.hip: `if (transA && !transB && ... && K >= 128)` ... `if (tn_fast_ok(tp) && ...) return launch_gemm_tn_multi`):
    for (transA, transB) = (1, 0), K >= 128 and a product beyond the small bound -- here (130, 257, 300) -- the baseline runs on
    the LDS-DMA engine, and a call whose A or B is in D1, D2 or D3 breaks tn_fast_ok (odd leading dimension or a base 8 bytes
    past a 16-byte boundary) and runs on the generic engine with two K slices: another summation order.  Those calls must
    equal each other's bits and meet the bar; C's form never matters."""
    A, B, C0, P, S = of.gemm_problem(M, N, K)
    As = np.ascontiguousarray(A.T if tA else A)
    Bs = np.ascontiguousarray(B.T if tB else B)
    base_route = of.gemm_route(M, N, K, tA, tB)[0]
    worst = 0.0
    for alpha, beta in of.ALPHA_BETA:
        ref, bar = of.gemm_ref(tA, tB, alpha, As, Bs, beta, C0, product=P, scale=S)
        base = _gemm(ctx, tA, tB, M, N, K, alpha, beta, ("H0",) * 3, As, Bs, C0)
        assert not np.isnan(base).any(), (alpha, beta)
        worst = max(worst, gr.worst_ratio(base, ref, bar))
        other_engine = {}
        for forms in ALL_FORMS:
            got = _gemm(ctx, tA, tB, M, N, K, alpha, beta, forms, As, Bs, C0)
            assert not np.isnan(got).any(), (forms, alpha, beta)
            r = gr.worst_ratio(got, ref, bar)
            worst = max(worst, r)
            assert r <= 1.0, (forms, alpha, beta, r)
            if base_route == "tn" and of.gemm_route(M, N, K, tA, tB, forms[0], forms[1])[0] == "tile":
                other_engine[forms] = got
            else:
                assert of.same_bits(got, base), (forms, alpha, beta, float(np.abs(got - base).max()))
        if base_route == "tn":
            assert sorted(other_engine) == sorted(f for f in ALL_FORMS if f[0] in ("D1", "D2", "D3") or f[1] in ("D1", "D2", "D3"))
            first = other_engine[("D1",) * 3]
            for forms, got in other_engine.items():
                assert of.same_bits(got, first), (forms, alpha, beta, float(np.abs(got - first).max()))
        else:
            assert not other_engine
        if K == 0:
            assert np.array_equal(base, beta * C0 if beta != 0.0 else np.zeros((M, N)))
    _log(f"nk_gemm ({M}, {N}, {K}) trans ({tA}, {tB}) [{base_route}]: worst error / bar {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# nk_gemm_f32
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_f32(ctx, M, N, K, forms, A, B, expect_rc=0):
    fa, fb, fc = forms
    a = of.Operand(fa, K, M, A, dtype=np.float32)
    b = of.Operand(fb, K, N, B, dtype=np.float32)
    c = of.Operand(fc, M, N)
    rc = of.call((a, b, c), lambda: ctx.lib.nk_gemm_f32(ctx.handle, M, N, K, a.ptr, a.ld, b.ptr, b.ld, c.ptr, c.ld))
    assert rc == expect_rc, (forms, rc, _last_error(ctx))
    of.check_inputs_and_guards(dict(A=(a, A), B=(b, B)), dict(C=c), tag=forms)
    return c.block()


F32_FORMS = [("F1", "F1", "H0"), ("F2", "F2", "H0"),                     # padded host A and B, tight C
             ("F0", "F0", "H1"),                                            # padded host C at a column offset
             ("G0", "G0", "D0"), ("G0", "G0", "D1"), ("G0", "G0", "D2"), ("G0", "G0", "D3"),
             ("F1", "G0", "H1"), ("G0", "F2", "D3"), ("F0", "G0", "H0"), ("G0", "G0", "H1")]  # host and device mixed


@pytest.mark.parametrize("M,N,K", of.GEMM_F32_SHAPES)
def test_gemm_f32(ctx, M, N, K):
    """(F0, F0, H1) -- tight operands, a padded host C at a column offset -- is the case that the flat write-back of M * ldc
    doubles failed: test_operand_forms_host.py shows on this parent layout that it overwrites the pad columns and trips the
    guard check.  Host operands need lda >= M, ldb >= N, ldc >= N only; the engine's contract (16-byte aligned, leading
    dimension a multiple of 4) binds device A and B, and a device operand that breaks it is NK_ERR_BAD_ARG with nothing
    written and the context usable."""
    rng = np.random.default_rng(M + 3 * N + 11 * K)
    A = rng.standard_normal((K, M)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    ref = gr._tn(A.astype(of.LD), B.astype(of.LD))
    bar = gr.contraction_bar(K, np.abs(A.astype(np.float64)).T @ np.abs(B.astype(np.float64)), flush_len=gr.F32_FLUSH_ROWS)
    base = _gemm_f32(ctx, M, N, K, ("F0", "F0", "H0"), A, B)
    assert not np.isnan(base).any()
    worst = gr.worst_ratio(base, ref, bar)
    _log(f"nk_gemm_f32 ({M}, {N}, {K}): worst error / bar {worst:.3f}")
    assert worst <= 1.0
    for forms in F32_FORMS:
        got = _gemm_f32(ctx, M, N, K, forms, A, B)
        assert of.same_bits(got, base), (forms, float(np.nanmax(np.abs(got - base))))
    for bad in of.CONTRACT_BREAKING32:
        for forms in [(bad, "G0", "D0"), ("F0", bad, "H1"), (bad, bad, "H0")]:
            got = _gemm_f32(ctx, M, N, K, forms, A, B, expect_rc=of.NK_ERR_BAD_ARG)
            msg = _last_error(ctx)
            assert "nk_gemm_f32" in msg and "16-byte aligned" in msg, msg
            assert (of.bits(got) == of.SENTINEL_BITS64).all(), forms  # C untouched
    again = _gemm_f32(ctx, M, N, K, ("F0", "F0", "H0"), A, B)
    assert of.same_bits(again, base)


# ---------------------------------------------------------------------------------------------------------------------
# nk_solve_spd
# ---------------------------------------------------------------------------------------------------------------------
SOLVE_M, SOLVE_NRHS = 70, 5  # two Cholesky blocks of 64, an odd right-hand-side count


def _solve(ctx, forms, P, R):
    m, nrhs = R.shape
    fp, fr, fx = forms
    p, r, x = of.Operand(fp, m, m, P), of.Operand(fr, m, nrhs, R), of.Operand(fx, m, nrhs)
    rc = of.call((p, r, x), lambda: ctx.lib.nk_solve_spd(ctx.handle, p.ptr, p.ld, m, r.ptr, r.ld, nrhs, x.ptr, x.ld))
    assert rc == 0, (forms, rc, _last_error(ctx))
    of.check_inputs_and_guards(dict(P=(p, P), R=(r, R)), dict(X=x), tag=forms)
    return x.block()


@pytest.mark.parametrize("force_pinv", [False, True], ids=["cholesky", "pinv"])
def test_solve_spd(ctx, monkeypatch, force_pinv):
    """The Cholesky branch copies P and R out of the caller's arrays with elementwise kernels (launch_copy2d) and works on
    arena blocks from there on; the SVD branch (NYSKOOP_FORCE_PINV=1) receives the caller's leading dimension and reads P
    through launch_copy2d and sumsq_all_kernel, whose summation runs over (row, column) indices in an order that does not
    depend on it, and R through launch_transpose.  So every form gives the bits of its mode's baseline.  The baselines:
    relf < 1e-10 against numpy.linalg.solve, and for the SVD branch pinv_reference's full-rank cap 2 cond(P) cap_ls(m)."""
    m, nrhs = SOLVE_M, SOLVE_NRHS
    P = np.array(cr.matrix("random", m, m))
    R = np.random.default_rng(7070).standard_normal((m, nrhs))
    want = np.linalg.solve(P, R)
    if force_pinv:
        monkeypatch.setenv("NYSKOOP_FORCE_PINV", "1")
    base = _solve(ctx, ("H0",) * 3, P, R)
    assert not np.isnan(base).any()
    err = relf(base, want)
    bar = pr.cap_forward(m, float(np.linalg.cond(P))) if force_pinv else 1e-10
    _log(f"nk_solve_spd m={m} nrhs={nrhs} {'pinv' if force_pinv else 'cholesky'}: relf {err:.3e} (bar {bar:.3e})")
    assert err < bar
    for forms in ALL_FORMS:
        got = _solve(ctx, forms, P, R)
        assert of.same_bits(got, base), (forms, float(np.nanmax(np.abs(got - base))))


# ---------------------------------------------------------------------------------------------------------------------
# nk_sqrtm_spd
# ---------------------------------------------------------------------------------------------------------------------
SQRT_M = 130


def _sqrtm(ctx, form_p, form_out, P):
    m = P.shape[0]
    p, s, si = of.Operand(form_p, m, m, P), of.Operand(form_out, m, m), of.Operand(form_out, m, m)
    assert s.ld == m and si.ld == m  # S and Sinv are tight: the call takes no leading dimension for them
    it, res = C.c_int32(-1), C.c_double(np.nan)
    rc = of.call((p, s, si), lambda: ctx.lib.nk_sqrtm_spd(ctx.handle, p.ptr, p.ld, m, s.ptr, si.ptr, C.byref(it), C.byref(res)))
    assert rc == 0, (form_p, form_out, rc, _last_error(ctx))
    of.check_inputs_and_guards(dict(P=(p, P)), dict(S=s, Sinv=si), tag=(form_p, form_out))
    return s.block(), si.block(), it.value, res.value


def test_sqrtm_spd(ctx):
    """m = 130 (graded family: the case of test_gpu_sqrtm.py, whose cached reference and bars grade the baseline).  P is read
    through elementwise kernels that take its leading dimension (launch_max_abs_rowsum, launch_sumsq_trace, launch_copy2d,
    launch_transpose, launch_axpby2d); everything after works on arena blocks.  Same iterations, residual, S and Sinv bits for
    every form of P, with S and Sinv on the host and on the device."""
    from test_gpu_sqrtm import _grade
    m = SQRT_M
    c = sr.case("graded", m, sr.seed_of(m), "host")
    P = np.array(c.P)
    S, Si, iters, resid = _sqrtm(ctx, "H0", "H0", P)
    assert resid < 1e-7 and abs(iters - c.steps[0]) <= 1, (iters, c.steps, resid)
    _grade(f"operand forms m={m} graded", c.P, S, Si, c.vals, c.bars, c.caps, c.ref, c.rows)
    for form_out in ("H0", "DT"):
        for form_p in ("H0", "H1", "D0", "D1", "D2", "D3"):
            S2, Si2, it2, res2 = _sqrtm(ctx, form_p, form_out, P)
            assert (it2, res2) == (iters, resid), (form_p, form_out, it2, res2, iters, resid)
            assert of.same_bits(S2, S) and of.same_bits(Si2, Si), (form_p, form_out)


# ---------------------------------------------------------------------------------------------------------------------
# nk_kernel_matrix
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = {"rbf": 0, "matern": 1, "linear": 2, "tps": 3}


def _kernel_matrix(ctx, family, par, forms, A, B):
    from nys_koop_lqr_amd import _lib
    fa, fb, fo = forms
    nA, d = A.shape
    nB = B.shape[0]
    ls = np.ascontiguousarray(par if family in ("rbf", "matern") else [1.0], dtype=np.float64)
    kd = _lib.KernelDesc(FAMILIES[family], d, ls.size, 0, ls.ctypes.data_as(C.POINTER(C.c_double)),
                         float(par) if family == "linear" else 0.0)
    a, b, o = of.Operand(fa, nA, d, A), of.Operand(fb, nB, d, B), of.Operand(fo, nA, nB)
    rc = of.call((a, b, o), lambda: ctx.lib.nk_kernel_matrix(ctx.handle, C.byref(kd), a.ptr, a.ld, nA, b.ptr, b.ld, nB,
                                                             o.ptr, o.ld))
    assert rc == 0, (forms, rc, _last_error(ctx))
    of.check_inputs_and_guards(dict(A=(a, A), B=(b, B)), dict(out=o), tag=forms)
    return o.block()


@pytest.mark.parametrize("nA,nB,d", of.KMAT_SHAPES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernel_matrix(ctx, family, nA, nB, d):
    """The three kernel-matrix kernels give the same bits (test_kernel_matrix_bits_do_not_depend_on_the_shape), so every form
    reproduces the baseline bit for bit whichever kernel it selects.  d < 32: the spline takes direct differences in the
    automatic mode.  Rows 0 coincide: r^2 = 0 exactly."""
    rng = np.random.default_rng(100 * nA + 10 * nB + d)
    A, B = rng.standard_normal((nA, d)), rng.standard_normal((nB, d))
    B[0] = A[0]
    if family == "tps":
        par = None
        ref, r2 = of.tps_ld(A, B)
        bar = of.tps_bar_direct(d, r2)
    else:
        _, par = gr.kernel_spec({"rbf": gr.RBF, "matern": gr.MATERN, "linear": gr.LINEAR}[family], d)
        ref, r2 = gr.kernel_ld(A, B, par, family)
        bar = gr.kblock_bar_direct(A, B, par, family, k=ref, r2=r2)
    base = _kernel_matrix(ctx, family, par, ("H0",) * 3, A, B)
    assert not np.isnan(base).any()
    worst = gr.worst_ratio(base, ref, bar)
    _log(f"nk_kernel_matrix {family} ({nA}, {nB}, {d}) [{of.kmat_route(nA, nB, d)[0]}]: worst error / bar {worst:.3f}")
    assert worst <= 1.0
    if family in ("rbf", "matern", "tps"):
        assert base[0, 0] == (0.0 if family == "tps" else 1.0)
    for forms in ALL_FORMS:
        got = _kernel_matrix(ctx, family, par, forms, A, B)
        assert of.same_bits(got, base), (forms, of.kmat_route(nA, nB, d, *forms), float(np.nanmax(np.abs(got - base))))
