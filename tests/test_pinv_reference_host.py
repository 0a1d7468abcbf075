"""CPU: the reference of tests/test_gpu_pinv.py is itself sound before the GPU is asked to meet it -- LAPACK's truncated SVD
solve stays under every derived cap on every system the GPU file runs, the diagonal cut-off cases have the ranks they claim,
the three measures notice a planted error of the kind each is there for, and nk_solve_spd is declared as the header has it.

LAPACK's own figures depend on the BLAS build; profiles/pinv_accuracy.log records one run of them (units of eps = 2^-52, the
matrix and two symmetric permutations of it): integer family e_ls up to 1.55, e_null up to 13.3 kappa_r; full-rank families,
backward error of the SVD solve up to 0.50.  The caps are m max(m, 64) eps; the assertions here leave a factor 10 to them."""
import os

import numpy as np
import pytest

import pinv_reference as pr
from nys_koop_lqr_amd import _lib

needs_longdouble = pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason=pr.LONGDOUBLE_SKIP)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every (m, rank, nrhs) of the GPU file, and m = 7 (odd, below one block)
INT_SYSTEMS = sorted({c[:3] for c in pr.INT_CASES + pr.SCALAR_CASES} | {(7, r, 3) for r in pr.ranks(7)})
FULL_SYSTEMS = sorted({c[:3] for c in pr.FULL_CASES} | {("graded", 513, 3)})


@needs_longdouble
@pytest.mark.parametrize("m,rank,nrhs", INT_SYSTEMS)
def test_lapack_meets_the_caps_on_the_integer_family(m, rank, nrhs):
    P, B, kappa = pr.int_lowrank(m, rank, m)
    assert P.shape == (m, m) and B.shape == (m, rank) and np.linalg.matrix_rank(B) == rank and kappa >= 1.0
    X, els, enull = pr.lapack_reference(m, rank, m, nrhs)
    assert X.shape == (m, nrhs) and len(els) == len(enull) == pr.N_PERM + 1 == 3
    e = pr.EPS
    assert max(els) <= pr.cap_ls(m) / 10, (np.array(els) / e, pr.cap_ls(m) / e)
    assert max(enull) <= pr.cap_null(m, kappa) / 10, (np.array(enull) / e / kappa, pr.cap_ls(m) / e)
    assert pr.cap_forward(m, kappa) < 1e-4  # the forward bound still says something at the largest size


@needs_longdouble
@pytest.mark.parametrize("family,m,nrhs", FULL_SYSTEMS)
def test_lapack_meets_the_cap_on_the_full_rank_families(family, m, nrhs):
    X, cond, be = pr.lapack_reference_full(family, m, m, nrhs)
    assert len(be) == 3 and max(be) <= pr.cap_ls(m) / 10, (np.array(be) / pr.EPS, pr.cap_ls(m) / pr.EPS)
    if family == "graded":
        assert 1e9 < cond < 1e11  # nothing is truncated at rcond = eps


@pytest.mark.parametrize("name", pr.DIAG_CASES)
def test_diag_cases_have_the_ranks_they_claim(name):
    P, s, rcond, keep, rank, oracle_rcond = pr.diag_case(name)  # (its own assertions: margins, the rule's decision)
    m = pr.DIAG_M
    assert np.array_equal(P, np.diag(s)) and keep.sum() == rank
    want = {"clean": 60, "decay": 32, "cluster": 60, "cluster_not_isolated": 63, "rcond": 40}[name]
    assert rank == want
    R = np.ones((m, 2))
    X, rk = pr.O.truncated_solve(P, R, rcond=oracle_rcond)
    assert rk == rank
    assert np.array_equal(X[~keep], np.zeros((m - rank, 2)))
    assert np.abs(X[keep] * s[keep, None] - 1.0).max() <= 5 * pr.EPS
    # gelsd's rule alone: what the isolated-cluster rule changes
    gelsd = pr.O.truncated_solve(P, R, rcond=rcond)[1]
    assert gelsd == (62 if name == "cluster" else rank)


def test_diag_dropped_values_are_the_ones_the_issue_names():
    _, s, _, keep, _, _ = pr.diag_case("decay")
    assert np.isclose(s[keep].min(), 10 ** -15.5) and np.isclose(s[~keep].max(), 1e-16)
    _, s, _, keep, _, _ = pr.diag_case("cluster_not_isolated")
    assert np.isclose(np.sort(s[keep])[:3], [5e-15, 4e-14, 1e-12]).all() and np.isclose(s[~keep].max(), 1e-16)
    _, s, _, keep, _, _ = pr.diag_case("cluster")
    assert np.isclose(s[keep].min(), 1e-2) and np.isclose(s[~keep].max(), 4e-14)
    _, s, _, keep, _, _ = pr.diag_case("rcond")
    assert s[keep].min() > 1e-2 > s[~keep].max() > 9e-3


@needs_longdouble
def test_measures_agree_with_the_plain_formulas():
    m, rank, nrhs = 130, 43, 3
    P, B, _ = pr.int_lowrank(m, rank, m)
    R = pr.int_rhs(m, nrhs, m)
    X = pr.lapack_reference(m, rank, m, nrhs)[0] + 1e-9  # (a residual large enough to compare in float64)
    nP = np.linalg.norm(P)
    want = np.linalg.norm(P @ (P @ X - R)) / (nP * (nP * np.linalg.norm(X) + np.linalg.norm(R)))
    assert abs(pr.e_ls(X, P, R) - want) <= 1e-6 * want
    U = np.linalg.svd(B)[0]
    want = np.linalg.norm(U[:, rank:].T @ X) / np.linalg.norm(X)  # the null space from the other side
    assert abs(pr.e_null(X, B) - want) <= 1e-6 * want
    Pf = pr.matrix("rbf", m, m)
    Xf = np.linalg.solve(Pf, R)
    want = np.linalg.norm(Pf @ (Xf * (1 + 1e-9)) - R) / (np.linalg.norm(Pf) * np.linalg.norm(Xf))
    assert abs(pr.backward_error(Xf * (1 + 1e-9), Pf, R) - want) <= 1e-3 * want


@needs_longdouble
@pytest.mark.parametrize("m,rank", [(130, 43), (513, 384)])
def test_measures_catch_a_planted_error(m, rank):
    nrhs = 3
    P, B, kappa = pr.int_lowrank(m, rank, m)
    R = pr.int_rhs(m, nrhs, m)
    X = np.array(pr.lapack_reference(m, rank, m, nrhs)[0])
    U, s, _ = np.linalg.svd(P)
    assert pr.e_ls(X, P, R) < pr.cap_ls(m) and pr.e_null(X, B) < pr.cap_null(m, kappa)
    # (i) one kept direction removed (the leading one): still minimum norm, no longer a least-squares solution
    lost = X - np.outer(U[:, 0], U[:, 0] @ X)
    assert pr.e_ls(lost, P, R) > pr.cap_ls(m)
    assert pr.e_null(lost, B) < pr.cap_null(m, kappa)
    # (ii) 1e-6 ||X|| of a null vector added: still a least-squares solution, no longer the minimum-norm one
    tilted = X + 1e-6 * np.linalg.norm(X) * np.outer(U[:, -1], np.ones(nrhs) / np.sqrt(nrhs))
    assert pr.e_null(tilted, B) > pr.cap_null(m, kappa)
    assert pr.e_ls(tilted, P, R) < pr.cap_ls(m)


@needs_longdouble
def test_forward_bound_catches_a_scaled_row():
    # (iii) one row of X scaled by 1 + 1e-6, on a case whose forward bound is below 1e-7
    m, rank, nrhs = 7, 5, 3
    P, B, kappa = pr.int_lowrank(m, rank, m)
    assert pr.cap_forward(m, kappa) < 1e-7
    X = pr.lapack_reference(m, rank, m, nrhs)[0]
    bent = np.array(X)
    bent[np.argmax(np.abs(X).sum(1))] *= 1.0 + 1e-6
    assert pr.relf(bent, X) > pr.cap_forward(m, kappa)
    # and an independent evaluation of the same answer is far inside it
    assert pr.relf(np.linalg.pinv(P, rcond=pr.GAP_RCOND) @ pr.int_rhs(m, nrhs, m), X) < pr.cap_forward(m, kappa) / 100


def test_kernel_of_follows_the_dispatch():
    got = [pr.kernel_of(m) for m in (1, 2, 3, 4, 512, 513, 1024, 1025, 2048, 2049)]
    assert got == ["none", "round_wave", "round_wave", "block8", "block8", "block4", "block4", "block2", "block2", "round"]
    assert [pr.kernel_of(m, block=False) for m in (130, 512, 513, 520)] == ["round_wave", "round_wave", "round", "round"]
    assert {pr.kernel_of(c[0]) for c in pr.INT_CASES} == {"none", "round_wave", "block8", "block4", "block2"}
    for kernel in ("round_wave", "block8", "block4", "block2"):  # NaN padding columns at least once per kernel
        assert any(pad for m, _, _, pad in pr.INT_CASES if pr.kernel_of(m) == kernel), kernel
    assert {pr.kernel_of(c[0], block=False) for c in pr.SCALAR_CASES} == {"round_wave", "round"}


def test_abi_declares_the_solve():
    assert "nk_solve_spd" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nk_solve_spd"][1]) == 9
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    want = ("int nk_solve_spd(nk_ctx* ctx, const double* P, int64_t ldp, int32_t m, const double* R, int64_t ldr,\n"
            "                 int32_t nrhs, double* X, int64_t ldxo);")
    assert want in header
    import ctypes as C
    assert _lib.SIGNATURES["nk_solve_spd"][1][2:4] == [C.c_int64, C.c_int32]
    assert _lib.SIGNATURES["nk_solve_spd"][1][5:7] == [C.c_int64, C.c_int32] and _lib.SIGNATURES["nk_solve_spd"][1][8] == C.c_int64
