"""Extended-precision reference for the augmented blocked Cholesky (nk_chol_aug): test matrices, residuals formed in NumPy
longdouble, LAPACK potrf / cho_solve as the comparison solver, and the two kinds of bars of tests/test_gpu_chol_accuracy.py.
Nothing here touches the GPU except chol_aug(), the ctypes call."""
import ctypes as C
import functools

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
EPS = 2.0 ** -52
LD_EPS = float(np.finfo(LD).eps)
# every residual below is formed in longdouble: it has to resolve a small multiple of EPS times the norm of the data
HAVE_LONGDOUBLE = LD_EPS < 1e-18
LONGDOUBLE_SKIP = f"numpy.longdouble is no wider than float64 here (eps {LD_EPS:.3g}): no extended-precision reference"

CHOL_FLOW_GIVEUP = -0x40000000
NB = 64  # tile size of the factorisation


# ---------------------------------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------------------------------
def random_spd(m, seed):
    """Q Q^T / k + 1e-3 I with k = 2 m standard-normal columns: cond about 1e3."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((m, 2 * m))
    P = Q @ Q.T / (2 * m) + 1e-3 * np.eye(m)
    return (P + P.T) / 2


def graded_spd(m, seed):
    """Eigenvalues logspace(0, -10) under a random orthogonal basis: the leading diagonal blocks of the factor are
    conditioned beyond CHOL_FIX_KAPPA, so the correction step of the products with the inverted blocks fires."""
    rng = np.random.default_rng(seed)
    Qo, _ = np.linalg.qr(rng.standard_normal((m, m)))
    P = (Qo * np.logspace(0, -10, m)) @ Qo.T
    return (P + P.T) / 2


def rbf_kernel(m, seed):
    """RBF kernel matrix of clustered points, without jitter."""
    rng = np.random.default_rng(seed)
    nc, d = 8, 6
    centres = rng.standard_normal((nc, d)) * 2.0
    pts = centres[rng.integers(0, nc, m)] + 0.3 * rng.standard_normal((m, d))
    sq = (pts * pts).sum(1)
    r2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * pts @ pts.T, 0.0)
    K = np.exp(-r2 / (2.0 * 1.5 ** 2))
    return (K + K.T) / 2


def rbf_spd(m, seed):
    """RBF kernel matrix of clustered points plus 1e-6 I: what the fits factor (K_mm + jitter)."""
    return rbf_kernel(m, seed) + 1e-6 * np.eye(m)


FAMILIES = {"random": random_spd, "graded": graded_spd, "rbf": rbf_spd}


@functools.lru_cache(maxsize=None)
def matrix(family, m, seed):
    P = FAMILIES[family](m, seed)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def rhs(extra, m, seed):
    R = np.random.default_rng(10_000 + seed).standard_normal((extra, m))
    R.setflags(write=False)
    return R


def indefinite(m, j, seed):
    """A random SPD matrix with its (j, j) entry lowered so that the elimination meets its FIRST non-positive pivot exactly at
    row j (the pivots before it are those of the SPD matrix; pivot j becomes -L_jj^2).  A rank-one change of an SPD matrix: one
    negative eigenvalue."""
    P = np.array(matrix("random", m, seed))
    L = np.linalg.cholesky(P)
    P[j, j] -= 2.0 * L[j, j] ** 2
    return P


def singular_psd(m=130, seed=130, src=7, dst=100):
    """An exactly singular PSD matrix: the RBF kernel matrix without its jitter, row and column `src` copied onto row and column
    `dst` (a duplicated landmark): e_src - e_dst spans its null space."""
    P = np.array(rbf_kernel(m, seed))
    P[dst, :] = P[src, :]
    P[:, dst] = P[:, src]
    return P


def diag_block_kappa(P):
    """||L_jj||_F ||L_jj^-1||_F of every 64 x 64 diagonal block of the factor (the quantity potrf_diag_kernel_body compares
    with CHOL_FIX_KAPPA = 8 * 64)."""
    L = np.linalg.cholesky(P)
    return [float(np.linalg.norm(L[j:j + NB, j:j + NB]) * np.linalg.norm(np.linalg.inv(L[j:j + NB, j:j + NB])))
            for j in range(0, P.shape[0], NB)]


# ---------------------------------------------------------------------------------------------------------------------
# residuals, products in longdouble
# ---------------------------------------------------------------------------------------------------------------------
def _fro(a):
    return np.sqrt((a * a).sum(dtype=LD))


def factor_residual(L, P, blk=128):
    """||tril(L) tril(L)^T - P||_F / ||P||_F.  The product is formed block by block over the lower triangle with the
    contraction cut at the triangle's edge (a third of the full product's work), then mirrored."""
    m = P.shape[0]
    Ll = np.tril(np.asarray(L)).astype(LD)
    Pl = np.asarray(P).astype(LD)
    tot = LD(0)
    for i0 in range(0, m, blk):
        i1 = min(i0 + blk, m)
        for j0 in range(0, i1, blk):
            j1 = min(j0 + blk, m)
            D = Ll[i0:i1, :j1] @ Ll[j0:j1, :j1].T - Pl[i0:i1, j0:j1]
            s = (D * D).sum(dtype=LD)
            if j0 == i0:  # diagonal block: count the strictly lower part twice, the diagonal once
                Dl = np.tril(D, -1)
                s = 2 * (Dl * Dl).sum(dtype=LD) + (np.diag(D) ** 2).sum(dtype=LD)
            else:
                s = 2 * s
            tot += s
    return float(np.sqrt(tot) / _fro(Pl))


def solve_backward_error(X, P, R):
    """||X P - R||_F / (||P||_F ||X||_F) for X = R P^-1 (rows of right-hand sides, as the fits carry them)."""
    Xl, Pl, Rl = np.asarray(X).astype(LD), np.asarray(P).astype(LD), np.asarray(R).astype(LD)
    return float(_fro(Xl @ Pl - Rl) / (_fro(Pl) * _fro(Xl)))


def lapack_factor_solve(P, R):
    L, info = sla.lapack.dpotrf(P, lower=1, clean=1)
    assert info == 0, info
    X = sla.cho_solve((L, True), R.T, check_finite=False).T
    return L, X


N_PERM = 4


@functools.lru_cache(maxsize=None)
def lapack_reference(family, m, seed, extra):
    """LAPACK on the matrix itself and on N_PERM random symmetric permutations of it: (factor residuals, solve backward
    errors), entry 0 the unpermuted problem.  Cached: a matrix is shared by the dataflow and the chain run of a case."""
    P, R = matrix(family, m, seed), rhs(extra, m, seed)
    rng = np.random.default_rng(777 + seed)
    fr, be = [], []
    for k in range(N_PERM + 1):
        perm = np.arange(m) if k == 0 else rng.permutation(m)
        Pp = np.ascontiguousarray(P[perm][:, perm])
        Rp = np.ascontiguousarray(R[:, perm])
        L, X = lapack_factor_solve(Pp, Rp)
        fr.append(factor_residual(L, Pp))
        be.append(solve_backward_error(X, Pp, Rp))
    return fr, be


def cap(m):
    """Derived, not measured: blocked Cholesky and the solve with its factor are normwise backward stable with a constant of
    order m (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3 / 10.4): at most m eps."""
    return m * EPS


def caps(m):
    """(cap of the factor residual, cap of the solve backward error).  From m = 5 both are cap(m).  Below that m eps drops the
    lower-order terms of the theorems it cites (at m = 1 LAPACK itself sits at 0.90 of it), so the constants themselves stand:
    ||L L^T - P|| <= gamma_(m+1) || |L| |L^T| || (Higham, 2nd ed., Thm 10.3) and (P + dP) x = b with |dP| <= gamma_(3m+1) |L| |L^T|
    (Thm 10.4), normwise and to first order: (m + 1) eps and (3 m + 1) eps."""
    if m >= 5:
        return cap(m), cap(m)
    return (m + 1) * EPS, (3 * m + 1) * EPS


def lapack_bar(values):
    """2 x the worst of LAPACK's own values over the permutations, floored at one rounding (LAPACK's solve backward error is
    about 0.1 eps, below one rounding of X: a ratio to that means nothing).  The factor 2 is the project's existing bar
    (test_blocked_solve_is_backward_stable_...); the permutations stand for an equally valid elimination and summation order."""
    return 2.0 * max(EPS, max(values))


# ---------------------------------------------------------------------------------------------------------------------
# the cases below m = 256 (tests/test_gpu_chol_small.py; test_chol_reference_host.py holds LAPACK to the same bars first)
# ---------------------------------------------------------------------------------------------------------------------
CHOL_FIX_KAPPA = 8 * NB

# (m, extra, family, ld), seed = m: the smallest shapes at which each piece of the launch-per-step chain changes behaviour
SMALL_SINGLE = [
    (1, 1, "rbf", 1),            # order-1 block
    (2, 3, "graded", 2),
    (5, 1, "random", 8),         # ld > m
    (17, 63, "rbf", 17),
    (40, 7, "graded", 40),       # one partial block, kappa 2e5
    (63, 64, "random", 63),
    (64, 1, "rbf", 64),          # exactly one block
    (64, 65, "graded", 72),
    (65, 64, "random", 65),      # second block of order 1: fused trailing + next diagonal with nb = 1
    (66, 2, "rbf", 66),
    (127, 130, "graded", 127),
    (128, 63, "rbf", 128),       # trailing matrix exactly one 128-tile wide after step 0
    (129, 1, "random", 136),
    (191, 65, "rbf", 191),
    (192, 192, "graded", 192),
    (193, 3, "random", 193),     # four blocks, the last a single row
    (200, 203, "rbf", 200),      # extra = m + 3
    (255, 64, "graded", 264),    # last size under the threshold of the dataflow launch
]
# (m, p, d, fam0, fam1): system 0 is (m + p) with m extra rows (seed 1000 + m + p), system 1 is m with d extra rows (seed 2000 + m)
SMALL_PAIRS = [
    (64, 1, 2, "rbf", "random"),       # 65 beside 64: system 1 has no step 1 (order 0, empty calls)
    (62, 3, 1, "graded", "rbf"),       # 65 beside 62
    (128, 6, 40, "random", "graded"),  # three blocks beside two
    (200, 1, 2, "rbf", "rbf"),         # the Duffing sweeps' shape
    (250, 6, 7, "random", "rbf"),      # 256 beside 250: the rule is "every m_q >= 256", so this pair takes the chain
]
# (m, nrhs, family), seed = m: nk_solve_spd (plain factor + forward and backward substitution)
SOLVE_SPD = [
    (1, 1, "rbf"),
    (5, 3, "random"),
    (64, 5, "graded"),
    (65, 64, "rbf"),
    (129, 1, "graded"),
    (200, 130, "random"),
    (321, 65, "rbf"),
]


def small_pair_systems(m, p, d, fam0, fam1):
    """[(family, order, seed, extra), ...] of a pair of SMALL_PAIRS."""
    return [(fam0, m + p, 1000 + m + p, m), (fam1, m, 2000 + m, d)]


# ---------------------------------------------------------------------------------------------------------------------
# the device call
# ---------------------------------------------------------------------------------------------------------------------
def counters():
    from nys_koop_lqr_amd import _lib
    v = (C.c_uint64 * 8)()
    _lib.check(_lib.load_library().nk_runtime_counters(v, 8))
    return [int(x) for x in v]


def flow_items(systems):
    """Work items (tickets) of the dataflow launch for systems [(m, extra), ...].  Mirrors chol_flow_counts / chol_flow_items
    of csrc/nk_chol_plan.h, which the library takes its count from (tests/test_chol_plan_host.py holds the two together)."""
    total = 0
    for m, extra in systems:
        nblk, nex = -(-m // NB), -(-extra // NB)
        total += sum(1 + max(0, nblk - c - 2) + nex for c in range(nblk))
    return total


def chol_aug(ctx, systems):
    """nk_chol_aug on [(P, R, ld), ...] (one or two systems): [(L, X, failed, piv_ratio), ...]."""
    from nys_koop_lqr_amd import _lib
    n = len(systems)
    keep, Pp, Rp, Lp, Xp = [], (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    ld, ms, ex = (C.c_int64 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    failed, ratio = (C.c_int32 * n)(), (C.c_double * n)()
    out = []
    for q, (P, R, ldq) in enumerate(systems):
        m, extra = P.shape[0], R.shape[0]
        assert P.shape == (m, m) and R.shape == (extra, m) and ldq >= m
        Pb = np.full((m, ldq), np.nan)  # (the padding columns are not part of the matrix: nothing may read them)
        Pb[:, :m] = P
        Rb = np.ascontiguousarray(R, dtype=np.float64)
        L, X = np.empty((m, m)), np.empty((extra, m))
        keep += [Pb, Rb]
        Pp[q], Rp[q], Lp[q], Xp[q] = Pb.ctypes.data, Rb.ctypes.data, L.ctypes.data, X.ctypes.data
        ld[q], ms[q], ex[q] = ldq, m, extra
        out.append((L, X))
    _lib.check(ctx.lib.nk_chol_aug(ctx.handle, n, Pp, ld, ms, Rp, ex, Lp, Xp, failed, ratio))
    return [(L, X, int(failed[q]), float(ratio[q])) for q, (L, X) in enumerate(out)]


def upper_tiles_untouched(L, P):
    """The contract of nk_chol_aug's L (include/nyskoop.h): 64 x 64 tiles strictly above the block diagonal return the input."""
    m = P.shape[0]
    for i0 in range(0, m, NB):
        if not np.array_equal(L[i0:i0 + NB, i0 + NB:], P[i0:i0 + NB, i0 + NB:]):
            return False
    return True
