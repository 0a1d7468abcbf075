"""CPU: the extended-precision reference of tests/test_gpu_chol_accuracy.py is itself sound before the GPU is asked to meet
it -- LAPACK's factor and solve stay under the derived cap m eps for every matrix family, the bar relative to LAPACK is what
its definition says, the residuals notice the mistakes a tiled kernel makes, and the diagnostic export is declared.  The same
for tests/test_gpu_chol_small.py: every shape below 256 it uses, with the m < 5 form of the cap."""
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


def _small_systems():
    """(family, m, seed, extra) of every system test_gpu_chol_small.py factors: singles, both systems of the pairs, nk_solve_spd."""
    out = [(fam, m, m, extra) for m, extra, fam, _ in cr.SMALL_SINGLE]
    for pair in cr.SMALL_PAIRS:
        out += [(fam, m, seed, extra) for fam, m, seed, extra in cr.small_pair_systems(*pair)]
    out += [(fam, m, m, nrhs) for m, nrhs, fam in cr.SOLVE_SPD]
    return sorted(set(out), key=lambda t: (t[1], t[0], t[3]))


def test_small_caps_are_highams_constants_below_five_and_the_cap_from_there():
    assert cr.caps(1) == (2 * cr.EPS, 4 * cr.EPS) and cr.caps(2) == (3 * cr.EPS, 7 * cr.EPS)
    assert cr.caps(4) == (5 * cr.EPS, 13 * cr.EPS)
    for m in (5, 17, 255, 321):
        assert cr.caps(m) == (cr.cap(m), cr.cap(m))


@needs_longdouble
@pytest.mark.parametrize("family,m,seed,extra", _small_systems())
def test_lapack_meets_the_small_bars(family, m, seed, extra):
    fr, be = cr.lapack_reference(family, m, seed, extra)
    cap_f, cap_s = cr.caps(m)
    assert max(fr) <= cap_f and max(be) <= cap_s, (np.array(fr) / cr.EPS, np.array(be) / cr.EPS)
    if m >= 5:
        assert fr[0] <= cr.lapack_bar(fr) / 2 and max(cr.EPS, be[0]) <= cr.lapack_bar(be) / 2
        assert cr.lapack_bar(fr) <= cap_f and cr.lapack_bar(be) <= cap_s  # (the bar relative to LAPACK is the tighter one)


def test_small_graded_systems_make_the_correction_step_fire():
    systems = [(m, m) for m, _, fam, _ in cr.SMALL_SINGLE if fam == "graded"]
    for pair in cr.SMALL_PAIRS:
        systems += [(m, seed) for fam, m, seed, _ in cr.small_pair_systems(*pair) if fam == "graded"]
    systems += [(m, m) for m, _, fam in cr.SOLVE_SPD if fam == "graded"]
    assert len(systems) >= 9
    for m, seed in systems:
        kappa = cr.diag_block_kappa(cr.matrix("graded", m, seed))
        assert max(kappa) > cr.CHOL_FIX_KAPPA, (m, seed, kappa)
    # up to m = 192 every full block of a graded system is above the threshold; m = 255 has blocks on both sides of it
    kappa = cr.diag_block_kappa(cr.matrix("graded", 255, 255))
    assert min(kappa) < cr.CHOL_FIX_KAPPA < max(kappa), kappa


@needs_longdouble
def test_residuals_catch_what_the_chain_gets_wrong_at_a_one_row_block():
    m, extra, seed = 65, 64, 65
    P, R = cr.matrix("random", m, seed), cr.rhs(extra, m, seed)
    L, X = cr.lapack_factor_solve(np.array(P), R)
    lfr, lbe = cr.lapack_reference("random", m, seed, extra)
    cap_f, cap_s = cr.caps(m)
    assert cr.factor_residual(L, P) <= cr.lapack_bar(lfr) and cr.solve_backward_error(X, P, R) <= cr.lapack_bar(lbe)
    # the one-row last block factored without its row's update (the trailing step before it skipped)
    lost = L.copy()
    lost[64, 64] = np.sqrt(P[64, 64])
    assert cr.factor_residual(lost, P) > cap_f > cr.lapack_bar(lfr)
    # a stale last column of X: the backward substitution did not reach the one-column block of this right-hand side set
    other = cr.lapack_factor_solve(np.array(P), cr.rhs(extra, m, seed + 1))[1]
    stale = X.copy()
    stale[:, 64] = other[:, 64]
    assert cr.solve_backward_error(stale, P, R) > cap_s > cr.lapack_bar(lbe)
    # a relative error of 64 roundings on the (64:65, 0:64) panel (a product with the inverted block that lost its correction)
    bent = L.copy()
    bent[64:65, 0:64] *= 1.0 + 64 * cr.EPS
    assert cr.lapack_bar(lfr) < cr.factor_residual(bent, P) < cap_f


def test_singular_psd_matrix_has_one_zero_eigenvalue_and_lapack_stops_at_the_copy():
    import scipy.linalg as sla
    P = cr.singular_psd()
    assert P.shape == (130, 130) and np.array_equal(P, P.T)
    assert np.array_equal(P[100], P[7]) and P[100, 100] == P[7, 7]
    w = np.linalg.eigvalsh(P)
    # PSD to rounding with exactly one zero eigenvalue: the next one is the smallest of the kernel matrix itself
    assert abs(w[0]) <= 130 * cr.EPS * w[-1] and w[1] > 1e6 * 130 * cr.EPS * w[-1], w[:3]
    # LAPACK either stops at the duplicated row (index + 1) or rounding leaves that pivot barely positive
    info = sla.lapack.dpotrf(P, lower=1)[1]
    assert info in (0, 101), info
    assert info == SINGULAR_LAPACK_INFO


SINGULAR_LAPACK_INFO = 101  # recorded: OpenBLAS / reference LAPACK dpotrf on cr.singular_psd()


def test_small_indefinite_matrices_fail_where_they_are_told_to():
    import scipy.linalg as sla
    for m, j in ((65, 3), (65, 64), (40, 39)):
        P = cr.indefinite(m, j, seed=11)
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
