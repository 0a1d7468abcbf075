"""Shared reference data of the launch-chain Riccati solver's tests (test_dare_large_host.py, test_gpu_dare_large.py): the
problems, and a second reference beside scipy's (dare_reference, imported unchanged) for the sizes at which four scipy solves
per problem cost too much -- lqr.dare_doubling, the NumPy statement of the iteration the device runs (LAPACK getrf + dgemm),
with its own movement under the perturbations dare_reference.reference draws.  The bars are dare_reference.bars on either
reference: residual <= max(10 r_ref, 64 m eps), gain <= 10 x the reference's movement.

A problem is admitted as scipy-referenced only if the mirror itself sits at or below ADMISSION = 0.5 of both scipy bars there
(test_dare_large_host.py asserts it): the device solver runs the mirror's steps in another summation order, so a problem on
which the mirror is at the bar says nothing about the kernels.  Everything is computed once per process and never modified."""
import functools

import numpy as np

import dare_reference as dr
from nys_koop_lqr_amd import lqr

ADMISSION = 0.5

# dr.random_problem(m, p, rho, seed), scipy-referenced: below, at and one past the LU's column block of 64 (and of 32), odd
# sizes, p = 32, one past an MFMA tile and the batched solver's 128 x 128 GEMM tile
SCIPY_CHEAP = [(1, 1, 1.1, 1), (5, 1, 1.1, 5), (17, 6, 1.1, 17), (33, 1, 1.1, 33), (63, 2, 1.1, 63), (64, 6, 1.1, 64),
               (65, 2, 0.9, 1065), (48, 32, 1.1, 48), (129, 8, 1.1, 129)]
SCIPY_FIXTURES = ["f3", "f10", "f12_m200"]
# one past the batched solver's limit: four scipy solves of this size are about 9 s of host time
SCIPY_PAST_LIMIT = [(257, 6, 0.9, 1257)]
# mirror-referenced (no scipy): one past 256, exact multiples of 16 and 64, one past 512 and 1024
MIRROR = [(272, 8, 1.1, 272), (320, 6, 1.1, 320), (513, 6, 1.1, 513), (1025, 6, 0.9, 2025)]


def label(case):
    return case if isinstance(case, str) else "r%d_p%d_rho%g_s%d" % case


@functools.lru_cache(maxsize=None)
def problem(case):
    """(A, B, Q, R) of a fixture name or an (m, p, rho, seed) tuple."""
    return dr.fixture_problem(case) if isinstance(case, str) else dr.random_problem(*case)


def case_seed(case):
    return 0 if isinstance(case, str) else int(case[3])


def mirror_reference(A, B, Q, R, seed=0):
    """dict(P, K, r, movement, iters, status) of lqr.dare_doubling on one problem; movement = the largest relative change of
    the mirror's K over three perturbations of A and B of relative size 1e-15, drawn exactly as dare_reference.reference
    draws them."""
    P, K, iters, status = lqr.dare_doubling(A, B, Q, R)
    out = dict(P=P, K=K, iters=iters, status=status, r=np.nan, movement=np.nan)
    if status != 0:
        return out
    rng = np.random.default_rng(1000 + seed)
    move = 0.0
    for _ in range(3):
        Ap = A * (1.0 + 1e-15 * rng.standard_normal(A.shape))
        Bp = B * (1.0 + 1e-15 * rng.standard_normal(B.shape))
        move = max(move, dr.relk(lqr.dare_doubling(Ap, Bp, Q, R)[1], K))
    out.update(r=dr.residual(A, B, Q, P, K), movement=move)
    return out


@functools.lru_cache(maxsize=None)
def scipy_ref(case):
    if isinstance(case, str):
        return dr.fixture_reference(case)
    return dr.reference(*problem(case), seed=case_seed(case))


@functools.lru_cache(maxsize=None)
def mirror_ref(case):
    return mirror_reference(*problem(case), seed=case_seed(case))


@functools.lru_cache(maxsize=None)
def mirror_solution(case):
    """(P, K, iterations, status) of the mirror alone (no perturbed solves)."""
    return lqr.dare_doubling(*problem(case))
