"""Discrete LQR.  dlqr is the host Riccati solve (scipy) and the default everywhere; dare_doubling is the NumPy statement
of the structure-preserving doubling iteration that the batched device solver runs (csrc/nk_dare.hip, one workgroup per
problem), and dlqr_batch hands a list of problems to that solver in one call.  dlqr_device solves one problem of any
size with the launch-chain form of the same iteration (csrc/nk_dare_large.hip).

Stands in for `control.dlqr(A, B, Q, R)` used at benchmark_lqr_cloth.py:262, benchmark_lqr_classic.py:288 and
benchmark_lqr_hjb.py:293,356 (python-control is not a dependency here): K = (B'PB + R)^-1 B'PA with P the
stabilising solution of the discrete algebraic Riccati equation.
"""
import numpy as np
import scipy.linalg


def dlqr(A, B, Q, R):
    """Returns (K, P).  control.dlqr returns (K, S, E); K and S(=P) are the same quantities."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    P = scipy.linalg.solve_discrete_are(A, B, Q, R)
    K = np.linalg.solve(B.T @ P @ B + R, B.T @ P @ A)
    return K, P


def _sym(M):
    return (M + M.T) / 2


def dare_doubling(A, B, Q, R, tol=1e-13, max_iter=40):
    """Structure-preserving doubling for A'PA - P - A'PB (R + B'PB)^-1 B'PA + Q = 0:
        A_0 = A, G_0 = B R^-1 B', H_0 = Q;   W = I + G H,   [X_A | X_G] = W^-1 [A_k | G],
        A+ = A_k X_A,   G+ = sym(G + A_k X_G A_k'),   H+ = H + sym(A_k' H X_A),
    stopped when |H+ - H|_1 <= tol |H+|_1 or after max_iter steps; P = H, K = (R + B'PB)^-1 B'PA.
    Returns (P, K, iterations, status): status 0 = converged, 1 = max_iter reached, 2 = non-finite values or a singular
    W / R; P and K are NaN for a status other than 0.  The device kernel computes the same steps."""
    A = np.array(A, dtype=np.float64)
    B = np.array(B, dtype=np.float64).reshape(A.shape[0], -1)
    Q = np.array(Q, dtype=np.float64)
    R = np.array(R, dtype=np.float64).reshape(B.shape[1], B.shape[1])
    m, p = B.shape
    nanP, nanK = np.full((m, m), np.nan), np.full((p, m), np.nan)
    status, it = 0, 0
    with np.errstate(all="ignore"):
        try:
            L = np.linalg.cholesky(R)
            Y = scipy.linalg.solve_triangular(L, B.T, lower=True)
        except (np.linalg.LinAlgError, ValueError):
            return nanP, nanK, 0, 2
        Ak, G, H = A.copy(), Y.T @ Y, Q.copy()
        converged = False
        while it < max_iter:
            W = np.eye(m) + G @ H
            if not np.all(np.isfinite(W)):
                status = 2
                break
            try:
                X = np.linalg.solve(W, np.hstack([Ak, G]))
            except np.linalg.LinAlgError:
                status = 2
                break
            XA, XG = X[:, :m], X[:, m:]
            G = _sym(G + Ak @ XG @ Ak.T)
            dH = _sym(Ak.T @ H @ XA)
            H = H + dH
            it += 1
            nd, nh = np.abs(dH).sum(axis=0).max(), np.abs(H).sum(axis=0).max()
            if not (np.isfinite(nd) and np.isfinite(nh)):
                status = 2
                break
            if nd <= tol * nh:
                converged = True
                break
            Ak = Ak @ XA
        if status == 0 and not converged:
            status = 1
        if status != 0:
            return nanP, nanK, it, status
        S = R + _sym(B.T @ H @ B)
        try:
            K = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S, lower=True), B.T @ H @ A)
        except (np.linalg.LinAlgError, ValueError):
            return nanP, nanK, it, 2
        if not np.all(np.isfinite(K)):
            return nanP, nanK, it, 2
    return H, K, it, 0


def dlqr_batch(As, Bs, Qs, Rs, tol=1e-13, max_iter=40):
    """K_u = dlqr(A_u, B_u, Q_u, R_u) for a list of problems in ONE device call (nk_dare_batch; m <= 256, p <= 8).
    Returns (Ks, Ps, status, iterations); a problem with status != 0 (1: max_iter reached, 2: non-finite / singular) has
    NaN outputs and leaves the others untouched."""
    from . import _lib
    Ks, Ps, status, iters, _ = _lib.get_context().dare_batch(As, Bs, Qs, Rs, tol=tol, max_iter=max_iter)
    return Ks, Ps, status, iters


def dlqr_device(A, B, Q, R, tol=1e-13, max_iter=40):
    """(K, P) = dlqr(A, B, Q, R) on the device for ONE problem of any size (nk_dare_large: the steps of dare_doubling as a
    chain of launches, products on the fp64 GEMM engine, W solved by a blocked pivoted LU; m <= 10240, p <= 32).  The
    operands are NumPy arrays or float64 device tensors.  Raises np.linalg.LinAlgError when the iteration does not
    converge or breaks down, as scipy does."""
    from . import _lib
    K, P, status, _, _ = _lib.get_context().dare_large(A, B, Q, R, tol=tol, max_iter=max_iter, want_P=True)
    if status != 0:
        raise np.linalg.LinAlgError(f"device Riccati solve failed with status {status} "
                                    "(1: max_iter reached, 2: non-finite values or a singular pivot)")
    return K, P


def cloth_gain_for_simulator(K):
    """Row permutation expected by the MATLAB cloth simulator (benchmark_lqr_cloth.py:263)."""
    return K[[0, 3, 1, 4, 2, 5], :]
