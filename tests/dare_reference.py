"""Shared reference data of the Riccati-solver tests (test_dare_host.py, test_gpu_dare.py): the problems, scipy's
solution of each, scipy's own movement under rounding-level perturbations of the operators, and the two bars built on them.

The stabilising gain of the fixture operators is ill-determined (closed-loop spectral radius up to 0.99999), so no fixed
tolerance against scipy's K can hold.  The bars are therefore relative to the reference's own error:
  residual  r(P) = ||A'PA - P - A'PBK + Q||_F / ||P||_F  <=  max(10 r(P_scipy), 64 m eps)
            (the second term is the rounding of evaluating the residual itself);
  gain      ||K - K_scipy||_F / ||K_scipy||_F  <=  10 x movement, movement = the largest relative change of scipy's K over
            three seeded perturbations of A and B of relative size 1e-15.
Everything is computed once per process and never modified."""
import functools
import os

import numpy as np
import scipy.linalg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps
MULTIPLIER = 10.0

# fixture operators: name -> (file, key of A, key of B, key of C)
FIXTURE_OPS = {
    "f1_wellcond": ("f1_cloth_rbf_wellcond.npz", "A", "B", "C"),
    "f1_illcond": ("f1_cloth_rbf_illcond.npz", "A", "B", "C"),
    "f2": ("f2_synth_rbf_d384.npz", "A", "B", "C"),
    "f3": ("f3_duffing_matern.npz", "A", "B", "C"),
    "f4": ("f4_hjb_matern.npz", "A", "B", "C"),
    "f8": ("f8_hjb_config2.npz", "A", "B", "C"),
    "f10": ("f10_lqr_control.npz", "A", "B", "C"),
    "f12_m10": ("f12_duffing_full.npz", "A_m10", "B_m10", "C_m10"),
    "f12_m48": ("f12_duffing_full.npz", "A_m48", "B_m48", "C_m48"),
    "f12_m200": ("f12_duffing_full.npz", "A_m200", "B_m200", "C_m200"),
    "f15_m10": ("f15_spline_duffing.npz", "A_10", "B_10", "C_10"),
    "f15_m48": ("f15_spline_duffing.npz", "A_48", "B_48", "C_48"),
    "f15_m200": ("f15_spline_duffing.npz", "A_200", "B_200", "C_200"),
}
# the fixtures that store A, B, C directly are also run with the small cost weight
SMALL_C = ("f1_wellcond", "f1_illcond", "f2", "f3", "f4", "f8", "f10")
HOST_CASES = [(name, 1.0) for name in FIXTURE_OPS] + [(name, 0.005) for name in SMALL_C]


def sym(M):
    return (M + M.T) / 2


@functools.lru_cache(maxsize=None)
def _npz(fname):
    return dict(np.load(os.path.join(GOLDEN, fname), allow_pickle=False))


def fixture_problem(name, c=1.0):
    """(A, B, Q, R) with Q = c sym(C'C), R = I."""
    fname, ka, kb, kc = FIXTURE_OPS[name]
    g = _npz(fname)
    A = np.array(g[ka], dtype=np.float64)
    B = np.array(g[kb], dtype=np.float64).reshape(A.shape[0], -1)
    C = np.array(g[kc], dtype=np.float64)
    return A, B, c * sym(C.T @ C), np.eye(B.shape[1])


def random_problem(m, p, rho, seed, rank=None):
    """Seeded random pair with spectral radius rho (stable below one, unstable above), Q = C'C of rank d < m (d = 1 at
    m = 1), R = I + a small seeded SPD part."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, m))
    A *= rho / max(np.abs(np.linalg.eigvals(A)).max(), 1e-300)
    B = rng.standard_normal((m, p))
    d = rank if rank is not None else max(1, min(m - 1, 3))
    C = rng.standard_normal((d, m))
    Rh = rng.standard_normal((p, p)) * 0.1
    return A, B, sym(C.T @ C), np.eye(p) + Rh @ Rh.T


def scipy_gain(A, B, Q, R):
    P = scipy.linalg.solve_discrete_are(A, B, Q, R)
    return P, np.linalg.solve(B.T @ P @ B + R, B.T @ P @ A)


def residual(A, B, Q, P, K):
    return float(np.linalg.norm(A.T @ P @ A - P - A.T @ P @ B @ K + Q) / np.linalg.norm(P))


def relk(K, Kref):
    return float(np.linalg.norm(K - Kref) / np.linalg.norm(Kref))


def reference(A, B, Q, R, seed=0):
    """dict(P, K, r, movement) of scipy on one problem."""
    P, K = scipy_gain(A, B, Q, R)
    rng = np.random.default_rng(1000 + seed)
    move = 0.0
    for _ in range(3):
        Ap = A * (1.0 + 1e-15 * rng.standard_normal(A.shape))
        Bp = B * (1.0 + 1e-15 * rng.standard_normal(B.shape))
        move = max(move, relk(scipy_gain(Ap, Bp, Q, R)[1], K))
    return dict(P=P, K=K, r=residual(A, B, Q, P, K), movement=move)


@functools.lru_cache(maxsize=None)
def fixture_reference(name, c=1.0):
    return reference(*fixture_problem(name, c))


def bars(ref, m):
    """(residual bar, gain bar) of a problem with reference `ref`."""
    return max(MULTIPLIER * ref["r"], 64 * m * EPS), MULTIPLIER * ref["movement"]


UNSTABILISABLE = (np.diag([1.2, 0.5, 0.3]), np.array([[0.0], [1.0], [1.0]]), np.eye(3), np.eye(1))
