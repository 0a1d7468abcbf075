"""Extended-precision reference for the Jacobi pseudo-inverse (nk_pinv.hip, reached through nk_solve_spd): exactly singular
integer matrices, diagonal matrices that pin every decision of the singular-value cut-off, the least-squares and minimum-norm
measures formed in NumPy longdouble, LAPACK's SVD (oracle.nk_oracle.truncated_solve) as the comparison solver, and the derived
caps of tests/test_gpu_pinv.py.  Nothing here touches the GPU except solve(), the ctypes call.

Convention: nk_solve_spd solves P X = R with R and X of shape (m, nrhs); chol_reference carries right-hand sides as rows, so
its rhs() and solve_backward_error() are used through a transpose."""
import functools

import numpy as np

from chol_reference import EPS, HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP, _fro, matrix, rhs, solve_backward_error  # noqa: F401
from oracle import nk_oracle as O

MAX_SWEEPS = 150  # pinv_right_divide's limit
GAP_RCOND = 1e-10  # truncated_solve's cut-off for the integer family: inside the gap (int_lowrank asserts it)


# ---------------------------------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_lowrank(m, rank, seed):
    """P = B B^T with B (m x rank) of integer entries in [-3, 3] and full column rank: every entry of P is a small integer,
    formed without rounding, so the rank is exact (as test_pinv_fallback_shapes builds it).  Returns P, B and
    kappa_r = s_1 / s_rank of B^T B, the condition of P on its range."""
    rng = np.random.default_rng(seed)
    B = rng.integers(-3, 4, size=(m, rank)).astype(np.float64)
    while np.linalg.matrix_rank(B) < rank:
        B = rng.integers(-3, 4, size=(m, rank)).astype(np.float64)
    P = B @ B.T
    assert np.array_equal(P, np.rint(P)) and np.abs(P).max() < 2.0 ** 40
    s = np.linalg.svd(B.T @ B, compute_uv=False)
    kappa_r = float(s[0] / s[-1])
    assert kappa_r * GAP_RCOND < 1e-2  # the smallest kept singular value is 100 x above truncated_solve's cut-off
    P.setflags(write=False)
    B.setflags(write=False)
    return P, B, kappa_r


def int_rhs(m, nrhs, seed):
    return rhs(nrhs, m, seed).T  # (m, nrhs), a view of chol_reference's cached rows


def ranks(m):
    """The ranks of test_pinv_fallback_shapes: 1, m // 3, 3 m // 4 (at least 1, duplicates merged)."""
    return sorted({1, max(1, m // 3), max(1, (3 * m) // 4)})


# (m, rank, nrhs, padding columns of P's buffer) of tests/test_gpu_pinv.py, seed = m.  The smallest sizes that reach each
# kernel of pinv_right_divide's dispatch and each of its edges:
#   no sweep       m = 1
#   round_wave     m = 2, 3 (m < 4 takes the scalar rounds; 3 is odd: the pairing has a dummy player)
#   block8         m = 4 (one real block beside a padding block), 9, 17 (odd block count, padded to even), 64, 511 and 512 (the
#                  last 64-entry chunk of a row partial, then full)
#   block4         m = 513 (first size: one row into a new block, block count padded), 520 (even block count)
#   block2         m = 1025, 1028; ranks 1 and m // 3 only, to hold the time
# nrhs is 1 or 3, and m + 3 once; the buffer of P has 5 NaN columns at least once per kernel.
INT_CASES = [
    (1, 1, 1, 0),
    (2, 1, 3, 5), (3, 1, 1, 0), (3, 2, 3, 5),
    (4, 1, 1, 0), (4, 3, 3, 5),
    (9, 1, 3, 0), (9, 3, 1, 0), (9, 6, 12, 0),
    (17, 1, 1, 0), (17, 5, 3, 5), (17, 12, 1, 0),
    (64, 1, 3, 0), (64, 21, 1, 0), (64, 48, 3, 0),
    (511, 1, 1, 0), (511, 170, 3, 0), (511, 383, 1, 5),
    (512, 1, 3, 0), (512, 170, 1, 0), (512, 384, 3, 0),
    (513, 1, 1, 0), (513, 171, 3, 5), (513, 384, 1, 0),
    (520, 1, 3, 0), (520, 173, 1, 0), (520, 390, 3, 0),
    (1025, 1, 1, 0), (1025, 341, 3, 5),
    (1028, 1, 3, 0), (1028, 342, 1, 0),
]
# the scalar rounds (NYSKOOP_PINV_BLOCK=0, a launch per round): m <= 512 runs jacobi_round_wave_kernel, m > 512
# jacobi_round_kernel, which is what every m > 2048 runs by default
SCALAR_CASES = [
    (130, 1, 1, 0), (130, 43, 3, 5), (130, 97, 1, 0),
    (520, 1, 3, 0), (520, 173, 1, 5), (520, 390, 3, 0),
]
# (family, m, nrhs, padding): full rank through the SVD path.  graded (cond 1e10, nothing truncated, the most sweeps) at the
# small size only.
FULL_CASES = [("random", 130, 3, 0), ("rbf", 130, 1, 5), ("graded", 130, 3, 0), ("random", 513, 1, 0), ("rbf", 513, 3, 5)]
assert all(r in ranks(m) for m, r, _, _ in INT_CASES + SCALAR_CASES)


# the pseudo-inverse of a diagonal matrix: nothing to rotate, so pinv_scale_kernel sees the prescribed values themselves
DIAG_M = 70
DIAG_WINDOW = 8 * DIAG_M * EPS  # pinv_right_divide's window, 1.24e-13
DIAG_GAP = 1000.0               # pinv_scale_kernel's isolation factor
DIAG_MARGIN = 1.4
_CLUSTER = [1e-16, 5e-15, 4e-14]
# name -> (non-zero values, rcond, expected rank as the issue states it or None = count of values above rcond, isolated?)
_DIAG = {
    "clean": (np.logspace(0, -3, 60), EPS, 60, False),
    "decay": (10.0 ** (-np.arange(40) / 2.0), EPS, 32, False),
    "cluster": (np.concatenate([np.logspace(0, -2, 60), _CLUSTER]), EPS, 60, True),
    "cluster_not_isolated": (np.concatenate([np.logspace(0, -2, 60), _CLUSTER, [1e-12]]), EPS, 63, False),
    "rcond": (np.logspace(0, -3, 60), 1e-2, None, False),
}
DIAG_CASES = sorted(_DIAG)
# Two comparisons that the prescribed spectra themselves place nearer than DIAG_MARGIN:
#   decay, window: 1e-13 against the window 1.24e-13.  The window only feeds the isolation test, and the neighbour ratio of
#                  this spectrum is 3.16 whichever side the value falls on: diag_case asserts that the rank does not move when
#                  the window is scaled by DIAG_MARGIN either way.
#   rcond, cut:    logspace(0, -3, 60) steps by a factor 1.124, so its neighbours of 1e-2 are 1.04e-2 and 9.25e-3.  sqrt(fl(s^2))
#                  is s itself in binary floating point and sigma_max is 1.0, so the comparison is still with the stored value.
_MARGIN = {("decay", "window"): 1.2, ("rcond", "cut"): 1.03}


def _rule(s, rcond, window):
    """pinv_scale_kernel's decision on singular values s: (cut, whether the isolated-cluster rule fired).  A transcription of
    the kernel, so no oracle for it: the specification is the literal ranks and fired flags of _DIAG and the kept / dropped
    values named in test_pinv_reference_host.py, which diag_case holds this function to; it serves to find the margins."""
    smax = s.max()
    wtop = window * smax
    above, inside = s[s > wtop], s[s <= wtop]
    cut = rcond * smax
    cmax = inside.max() if inside.size else 0.0
    fired = bool(cmax > cut and above.size and above.min() >= DIAG_GAP * cmax)
    return (wtop if fired else cut), fired


def _apart(a, b):
    return max(a, b) / min(a, b) if min(a, b) > 0 else np.inf


@functools.lru_cache(maxsize=None)
def diag_case(name, m=DIAG_M):
    """Diagonal P (m x m) with a prescribed spectrum, its entries shuffled by one fixed permutation so that kept and dropped
    rows interleave.  Returns (P, sigma, rcond, keep, rank, oracle_rcond): sigma the diagonal, rcond what NYSKOOP_PINV_RCOND has
    to be (EPS = the default, leave it unset), keep the mask of the rows that survive, oracle_rcond a cut-off that gives
    truncated_solve, which knows gelsd's rule only, the same rank."""
    assert m == DIAG_M
    vals, rcond, want_rank, want_fired = _DIAG[name]
    s = np.zeros(m)
    s[:len(vals)] = vals
    window = 8 * m * EPS
    cut, fired = _rule(s, rcond, window)
    assert fired == want_fired, (name, fired)
    keep = s > cut
    rank = int(keep.sum())
    if want_rank is None:
        want_rank = int((vals > rcond).sum())
    assert rank == want_rank, (name, rank, want_rank)
    # every prescribed value is a factor DIAG_MARGIN away from every threshold it is compared with
    nz = s[s > 0]
    wtop = window * s.max()
    for v in nz:
        assert _apart(v, cut) >= _MARGIN.get((name, "cut"), DIAG_MARGIN), (name, "cut", v, cut)
        assert _apart(v, wtop) >= _MARGIN.get((name, "window"), DIAG_MARGIN), (name, "window", v, wtop)
    inside, above = nz[nz <= wtop], nz[nz > wtop]
    if inside.size and inside.max() > rcond * s.max():  # the isolation test is evaluated: its ratio is clear of the factor
        assert _apart(above.min() / inside.max(), DIAG_GAP) >= DIAG_MARGIN, (name, above.min() / inside.max())
    for f in (1.0 / DIAG_MARGIN, DIAG_MARGIN):  # no decision hangs on where exactly the window ends
        cut_f, fired_f = _rule(s, rcond, window * f)
        assert fired_f == fired and int((s > cut_f).sum()) == rank, (name, f)
    perm = np.random.default_rng(4242).permutation(m)
    s, keep = s[perm], keep[perm]
    assert np.count_nonzero(np.diff(keep.astype(int))) >= 8  # kept and dropped rows interleave
    P = np.diag(s)
    for a in (P, s, keep):
        a.setflags(write=False)
    return P, s, rcond, keep, rank, (float(wtop) if fired else rcond)


# ---------------------------------------------------------------------------------------------------------------------
# measures, products in longdouble
# ---------------------------------------------------------------------------------------------------------------------
def e_ls(X, P, R):
    """||P (P X - R)||_F / (||P||_F (||P||_F ||X||_F + ||R||_F)): the residual of the normal equations, zero for every
    least-squares solution of P X = R."""
    Xl, Pl, Rl = np.asarray(X).astype(LD), np.asarray(P).astype(LD), np.asarray(R).astype(LD)
    nP = _fro(Pl)
    return float(_fro(Pl @ (Pl @ Xl - Rl)) / (nP * (nP * _fro(Xl) + _fro(Rl))))


def e_null(X, B):
    """||X - Q Q^T X||_F / ||X||_F with Q an orthonormal basis of range(B) = range(P): the part of X in the null space of P,
    zero for the minimum-norm solution."""
    Q, _ = np.linalg.qr(np.asarray(B, dtype=np.float64))  # orthonormal to a few eps, which is this measure's floor
    Xl, Ql = np.asarray(X).astype(LD), Q.astype(LD)
    return float(_fro(Xl - Ql @ (Ql.T @ Xl)) / _fro(Xl))


def backward_error(X, P, R):
    """Full rank: chol_reference's ||X P - R||_F / (||P||_F ||X||_F) on the transposed (row) system."""
    return solve_backward_error(np.asarray(X).T, P, np.asarray(R).T)


def relf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


N_PERM = 2  # the matrix itself and two symmetric permutations of it: three orderings


def _orderings(m, seed):
    rng = np.random.default_rng(777 + seed)
    return [np.arange(m)] + [rng.permutation(m) for _ in range(N_PERM)]


@functools.lru_cache(maxsize=None)
def lapack_reference(m, rank, seed, nrhs):
    """LAPACK's SVD solve of the integer system (truncated_solve, cut-off inside the gap) on the matrix and on N_PERM symmetric
    permutations of it: (X of the unpermuted system, [e_ls], [e_null]), entry 0 the unpermuted one.  Cached."""
    P, B, _ = int_lowrank(m, rank, seed)
    R = int_rhs(m, nrhs, seed)
    els, enull, X0 = [], [], None
    for perm in _orderings(m, seed):
        Pp, Rp, Bp = np.ascontiguousarray(P[perm][:, perm]), np.ascontiguousarray(R[perm]), B[perm]
        X, rk = O.truncated_solve(Pp, Rp, rcond=GAP_RCOND)
        assert rk == rank, (m, rank, rk)
        els.append(e_ls(X, Pp, Rp))
        enull.append(e_null(X, Bp))
        if X0 is None:
            X0 = X
    X0.setflags(write=False)
    return X0, els, enull


@functools.lru_cache(maxsize=None)
def lapack_reference_full(family, m, seed, nrhs):
    """The same for a full-rank family: (numpy.linalg.solve's X, cond(P), [backward errors of the SVD solve])."""
    P, R = matrix(family, m, seed), int_rhs(m, nrhs, seed)
    be = []
    for perm in _orderings(m, seed):
        Pp, Rp = np.ascontiguousarray(P[perm][:, perm]), np.ascontiguousarray(R[perm])
        X, rk = O.truncated_solve(Pp, Rp)
        assert rk == m
        be.append(backward_error(X, Pp, Rp))
    X0 = np.linalg.solve(P, R)
    X0.setflags(write=False)
    return X0, float(np.linalg.cond(P)), be


# ---------------------------------------------------------------------------------------------------------------------
# caps: derived, not measured
# ---------------------------------------------------------------------------------------------------------------------
def jacobi_tol(m):
    """pinv_right_divide's stopping criterion: every pair of columns orthogonal to max(m, 64) eps."""
    return max(m, 64) * EPS


def cap_ls(m):
    """With every pair of columns of W orthogonal to tol, W^T W = S^2 + E with |E_jk| <= tol s_j s_k, so the computed
    U = S^-1 W departs from orthogonality by ||S^-1 E S^-1||_F <= m tol, and so does P P^+ from the projector on range(P).
    Worst case; also the cap of the full-rank backward error."""
    return m * jacobi_tol(m)


def cap_null(m, kappa_r):
    """A kept singular vector tilts into the null space by its backward error over its singular value."""
    return kappa_r * cap_ls(m)


def cap_forward(m, kappa_r):
    """Two solutions that are each within kappa_r x their backward error of the exact one."""
    return 2.0 * kappa_r * cap_ls(m)


# ---------------------------------------------------------------------------------------------------------------------
# the device call
# ---------------------------------------------------------------------------------------------------------------------
def kernel_of(m, block=True):
    """The Jacobi kernel pinv_right_divide launches for a single solve outside a lock-step group (NYSKOOP_PINV_SWEEP_LAUNCH
    unset or 0); block=False is NYSKOOP_PINV_BLOCK=0."""
    if m == 1:
        return "none"
    if block and m >= 4:
        if m <= 2048:
            return "block8" if m <= 512 else ("block4" if m <= 1024 else "block2")
    return "round_wave" if m <= 512 else "round"


def solve(ctx, P, R, ldp=None):
    """nk_solve_spd: X (m x nrhs) with P X = R.  P sits in a buffer of row length ldp whose padding columns are NaN."""
    from nys_koop_lqr_amd import _lib
    m, nrhs = P.shape[0], R.shape[1]
    ldp = m if ldp is None else ldp
    assert P.shape == (m, m) and R.shape == (m, nrhs) and ldp >= m
    Pb = np.full((m, ldp), np.nan)  # (the padding columns are not part of the matrix: nothing may read them)
    Pb[:, :m] = P
    Rb = np.ascontiguousarray(R, dtype=np.float64)
    X = np.full((m, nrhs), np.nan)
    _lib.check(ctx.lib.nk_solve_spd(ctx.handle, Pb.ctypes.data, ldp, m, Rb.ctypes.data, nrhs, nrhs, X.ctypes.data, nrhs))
    return X
