"""CPU: the extended-precision reference of tests/test_gpu_chol_accuracy.py is itself sound before the GPU is asked to meet
it -- LAPACK's factor and solve stay under the derived cap m eps for every matrix family, the bar relative to LAPACK is what
its definition says, the residuals notice the mistakes a tiled kernel makes, and the diagnostic export is declared."""
import os

import numpy as np
import pytest

import chol_reference as cr
from nys_koop_lqr_amd import _lib

needs_longdouble = pytest.mark.skipif(not cr.HAVE_LONGDOUBLE, reason=cr.LONGDOUBLE_SKIP)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_longdouble_is_extended():
    # x87 extended precision on the platforms the suite runs on; elsewhere the GPU accuracy file skips with a message
    if cr.HAVE_LONGDOUBLE:
        assert cr.LD_EPS < 1.1e-19


@needs_longdouble
@pytest.mark.parametrize("family", sorted(cr.FAMILIES))
@pytest.mark.parametrize("m,extra", [(257, 63), (705, 65)])
def test_lapack_meets_the_cap(family, m, extra):
    fr, be = cr.lapack_reference(family, m, m, extra)
    assert len(fr) == len(be) == cr.N_PERM + 1
    assert max(fr) <= cr.cap(m) and max(be) <= cr.cap(m), (np.array(fr) / cr.EPS, np.array(be) / cr.EPS)
    # the bar relative to LAPACK is far inside the cap, and LAPACK itself meets it with a factor 2 to spare
    assert cr.lapack_bar(fr) < cr.cap(m) / 20 and cr.lapack_bar(be) < cr.cap(m) / 20
    assert fr[0] <= cr.lapack_bar(fr) / 2 and max(cr.EPS, be[0]) <= cr.lapack_bar(be) / 2


@needs_longdouble
def test_residuals_agree_with_the_plain_formulas():
    m, extra = 150, 7
    P, R = cr.matrix("rbf", m, 3), cr.rhs(extra, m, 3)
    L, X = cr.lapack_factor_solve(np.array(P), R)
    Ll, Pl = np.tril(L).astype(cr.LD), P.astype(cr.LD)
    want = float(np.sqrt(((Ll @ Ll.T - Pl) ** 2).sum()) / np.sqrt((Pl ** 2).sum()))
    assert abs(cr.factor_residual(L, P, blk=64) - want) <= 1e-3 * want
    assert abs(cr.factor_residual(L, P, blk=47) - want) <= 1e-3 * want
    # the strict upper triangle of L is not part of the factor
    junk = L + np.triu(np.ones((m, m)), 1)
    assert cr.factor_residual(junk, P) == cr.factor_residual(L, P)
    Xl = X.astype(cr.LD)
    want = float(np.sqrt(((Xl @ Pl - R) ** 2).sum()) / (np.sqrt((Pl ** 2).sum()) * np.sqrt((Xl ** 2).sum())))
    assert abs(cr.solve_backward_error(X, P, R) - want) <= 1e-3 * want


@needs_longdouble
def test_residuals_catch_what_a_tiled_kernel_gets_wrong():
    m, extra = 321, 65
    P, R = cr.matrix("random", m, 9), cr.rhs(extra, m, 9)
    L, X = cr.lapack_factor_solve(np.array(P), R)
    lfr, lbe = cr.lapack_reference("random", m, 9, extra)
    # one left-looking update of one tile lost: tile (4, 3) misses the contribution of block column 2
    lost = L.copy()
    T = P[256:320, 192:256] - L[256:320, :128] @ L[192:256, :128].T
    lost[256:320, 192:256] = np.linalg.solve(L[192:256, 192:256], T.T).T
    assert cr.factor_residual(lost, P) > cr.cap(m) > cr.lapack_bar(lfr)
    # a relative error of 256 roundings on one tile of the factor: under the cap, over the bar relative to LAPACK
    bent = L.copy()
    bent[256:320, 192:256] *= 1.0 + 256 * cr.EPS
    assert cr.lapack_bar(lfr) < cr.factor_residual(bent, P) < cr.cap(m)
    # a block of solution columns off by 1e-9
    Xb = X.copy()
    Xb[:, 300:] *= 1.0 + 1e-9
    assert cr.solve_backward_error(Xb, P, R) > cr.cap(m) > cr.lapack_bar(lbe)


def test_indefinite_matrix_fails_where_it_is_told_to():
    import scipy.linalg as sla
    for j in (5, 320):
        P = cr.indefinite(321, j, seed=11)
        assert (np.linalg.eigvalsh(P) < 0).sum() == 1
        assert sla.lapack.dpotrf(P, lower=1)[1] == j + 1


def test_flow_items_counts_the_tiles():
    # m = 256: 4 diagonal items + tiles (2,0) (3,0) (3,1) + one extra tile row under each of the 4 columns
    assert cr.flow_items([(256, 1)]) == 4 + 3 + 4
    assert cr.flow_items([(262, 256), (256, 40)]) == (5 + 6 + 5 * 4) + (4 + 3 + 4)


def test_abi_declares_the_cholesky_diagnostic():
    assert "nk_chol_aug" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nk_chol_aug"][1]) == 11
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    assert "int nk_chol_aug(nk_ctx* ctx, int32_t nsys," in header
    assert "#define NK_CHOL_FLOW_GIVEUP (-0x40000000)" in header and cr.CHOL_FLOW_GIVEUP == -0x40000000
