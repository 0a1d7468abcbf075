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


# ---------------------------------------------------------------------------------------------------------------------------
# Constrained Koopman MPC: the condensed QP of the lifted model under box and rate limits on the inputs, and the fixed-step
# ADMM iteration that the device loop runs (csrc/nk_mpc_loop.hip) and the host build states (csrc/nk_mpc.h, nk_mpc_qp_host).
# ---------------------------------------------------------------------------------------------------------------------------
def mpc_condense(A, B, Q, R, P, N):
    """(H, F) of  sum_{k<N} (e_k'Q e_k + u_k'R u_k) + e_N'P e_N  under  e_{k+1} = A e_k + B u_k  as a function of
    U = (u_0, ..., u_{N-1}) (nv = N p entries) and e_0: the cost is 1/2 U'HU + (F e_0)'U + const, H (nv x nv) symmetrised,
    F (nv x m).  With P the Riccati solution the first p rows of H^-1 F are the dlqr gain for every N.
    Only thin products: G_k = A^k B (m x p) and, per block column j, the Horner recursion
        W_l = T_l + A' W_{l+1},  l = N .. 0,  T_l = Q_l G_{l-1-j} for l > j (Q_N = P), 0 otherwise,
    which gives H_ij = 2 B'W_{i+1} (i >= j) and F_j = 2 W_0'; no power of A is formed.  O(N^2 m^2 p) operations."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(m, -1)
    p = B.shape[1]
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(p, p)
    N = int(N)
    if N < 1:
        raise ValueError("the horizon N must be at least 1")
    G = [B]
    for _ in range(N - 1):
        G.append(A @ G[-1])
    nv = N * p
    H, F = np.zeros((nv, nv)), np.zeros((nv, m))
    for j in range(N):
        W = np.zeros((m, p))
        for l in range(N, -1, -1):
            W = A.T @ W
            if l > j:
                W = W + (P if l == N else Q) @ G[l - 1 - j]
            if j + 1 <= l <= N:  # W_l = W_{i+1} with i = l - 1 >= j
                H[(l - 1) * p:l * p, j * p:(j + 1) * p] = 2.0 * (B.T @ W)
        F[j * p:(j + 1) * p, :] = 2.0 * W.T
    low = np.tril(H, -1)
    H = low + low.T + np.diag(np.diag(H))
    for j in range(N):  # the diagonal blocks are symmetric up to rounding
        blk = H[j * p:(j + 1) * p, j * p:(j + 1) * p]
        H[j * p:(j + 1) * p, j * p:(j + 1) * p] = (blk + blk.T) / 2 + 2.0 * _sym(R)
    return _sym(H), F


def dare_refine(A, B, Q, R, K, steps=2):
    """Newton (Hewer) steps on a stabilising gain: P = (A - BK)'P(A - BK) + Q + K'RK by a Lyapunov solve, then
    K = (R + B'PB)^-1 B'PA.  Returns (K, P).  scipy's Riccati solution of the lifted models (spectral radius of A just above 1,
    of the closed loop just below) leaves a relative Riccati residual of 1e-9 .. 1e-10, and dlqr's gain then differs from the
    first move of the condensed problem by 2e-9 .. 1e-8; one step brings the residual to 1e-14 and the two to 1e-13."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64).reshape(np.shape(A)[0], -1)
    R = np.asarray(R, dtype=np.float64).reshape(B.shape[1], B.shape[1])
    K, P = np.asarray(K, dtype=np.float64), None
    for _ in range(int(steps)):
        Ac = A - B @ K
        P = _sym(scipy.linalg.solve_discrete_lyapunov(Ac.T, Q + K.T @ R @ K))
        K = np.linalg.solve(B.T @ P @ B + R, B.T @ P @ A)
    return K, P


def mpc_condense_blocked(A, B, Q, R, P, N):
    """The (H, F) of mpc_condense with the Horner recursion run for all block columns at once on one m x nv matrix W -- the
    NumPy statement of what the device build computes (csrc/nk_mpc_build.hip).  G_k = A^k B; for l = N .. 0:
        W = A' W;  block column j of W += (P if l == N else Q) G_{l-1-j} for every j < min(l, N);
        for l >= 1: block row l-1 of H, columns 0 .. l-1, = 2 B' W[:, :l p];
    at the end F = 2 W'.  The symmetrisation and + 2 sym(R) are those of mpc_condense.  N + 1 products of m x m by m x nv
    instead of O(N^2) thin ones."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(m, -1)
    p = B.shape[1]
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(p, p)
    N = int(N)
    if N < 1:
        raise ValueError("the horizon N must be at least 1")
    nv = N * p
    Gs = np.zeros((m, nv))  # [G_0 | G_1 | ... | G_{N-1}]
    Gs[:, :p] = B
    for k in range(1, N):
        Gs[:, k * p:(k + 1) * p] = A @ Gs[:, (k - 1) * p:k * p]
    QG, PG = Q @ Gs, P @ Gs
    W, H = np.zeros((m, nv)), np.zeros((nv, nv))
    for l in range(N, -1, -1):
        W = A.T @ W
        src = PG if l == N else QG
        for j in range(min(l, N)):
            W[:, j * p:(j + 1) * p] += src[:, (l - 1 - j) * p:(l - j) * p]
        if l >= 1:
            H[(l - 1) * p:l * p, :l * p] = 2.0 * (B.T @ W[:, :l * p])
    F = 2.0 * W.T
    low = np.tril(H, -1)
    H = low + low.T + np.diag(np.diag(H))
    for j in range(N):
        blk = H[j * p:(j + 1) * p, j * p:(j + 1) * p]
        H[j * p:(j + 1) * p, j * p:(j + 1) * p] = (blk + blk.T) / 2 + 2.0 * _sym(R)
    return _sym(H), F


def lyap_smith(Ac, X0, tol=1e-15, max_iter=60):
    """The squared Smith iteration for X = Ac' X Ac + X0:  X = sym(X0); repeat  D = sym(Ac' X Ac), X += D, stop when
    |D|_1 <= tol |X|_1, otherwise Ac = Ac Ac.  Returns (X, iterations, status): status 0 = converged, 3 = max_iter reached,
    2 = non-finite values.  The device build runs the same steps."""
    Ac = np.array(Ac, dtype=np.float64)
    X = _sym(np.array(X0, dtype=np.float64))
    it = 0
    with np.errstate(all="ignore"):
        while it < max_iter:
            D = _sym(Ac.T @ X @ Ac)
            X = X + D
            it += 1
            nd, nx = np.abs(D).sum(axis=0).max(), np.abs(X).sum(axis=0).max()
            if not (np.isfinite(nd) and np.isfinite(nx)):
                return X, it, 2
            if nd <= tol * nx:
                return X, it, 0
            Ac = Ac @ Ac
    return X, it, 3


def dare_newton_smith(A, B, Q, R, K, steps=1, tol=1e-15, max_iter=60, P=None):
    """Newton (Hewer) steps on a stabilising gain, each as a correction of the current P (zeros when P is None) by lyap_smith:
        Ac = A - BK,  Res = sym((Ac'P Ac - P) + (Q + K'RK)),  P += lyap_smith(Ac, Res),  K = (R + sym(B'PB))^-1 B'PA.
    P + the correction solves X = Ac'X Ac + Q + K'RK, the Lyapunov equation of the step; from P = 0 the first step is that
    solve itself.  From the doubling iteration's P the Smith iteration carries only the correction, so its rounding (which
    grows with the squarings when the closed-loop radius is near one) is relative to the correction and not to P: on the
    Duffing fixtures with radius 0.99999 the full solve left a Riccati residual of 3e-13, the correction leaves 4e-16.
    Returns (K, P, iterations, status): the squarings summed over the steps; status 0, or the first non-zero one of lyap_smith
    (2 also when R + B'PB is not positive definite), with K and P then NaN.  steps = 0 returns K and P as given."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(m, -1)
    p = B.shape[1]
    Q = np.asarray(Q, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(p, p)
    K, total = np.array(K, dtype=np.float64).reshape(p, m), 0
    nan = (np.full((p, m), np.nan), np.full((m, m), np.nan))
    if int(steps) > 0:
        P = np.zeros((m, m)) if P is None else np.array(P, dtype=np.float64)
    for _ in range(int(steps)):
        Ac = A - B @ K
        with np.errstate(all="ignore"):
            res = (Ac.T @ P @ Ac - P) + (Q + K.T @ R @ K)
        dP, it, status = lyap_smith(Ac, res, tol=tol, max_iter=max_iter)
        total += it
        if status != 0:
            return nan[0], nan[1], total, status
        P = P + dP
        try:
            K = scipy.linalg.cho_solve(scipy.linalg.cho_factor(R + _sym(B.T @ P @ B), lower=True), B.T @ P @ A)
        except (np.linalg.LinAlgError, ValueError):
            return nan[0], nan[1], total, 2
    return K, P, total, 0


def mpc_build_batch(As, Bs, Qs, Rs, Ns, Ps=None, C_rows=None, Nys=None, tol=1e-13, max_iter=40, newton_steps=1,
                    newton_tol=1e-15, newton_max_iter=60):
    """The controllers of a list of problems in ONE device call (nk_mpc_build_batch; m <= 512, p <= 4, N p <= 64): per problem
    the Riccati solution by the doubling iteration (tol, max_iter), newton_steps steps of dare_newton_smith (newton_tol,
    newton_max_iter), (H, F) of mpc_condense_blocked for the horizon Ns[i] and, with C_rows[i] (nc <= 4 rows) and Nys[i]
    (default N), (G, T) of mpc_condense_outputs.  A terminal cost Ps[i] skips the Riccati and Newton stages: pure condensing,
    K = (R + B'PB)^-1 B'PA.  Returns a dict of lists H, F, K, P, G, T (G, T None without rows) and the arrays status (0 =
    success, 1 = doubling cap, 2 = non-finite / not positive definite, 3 = Smith cap: NaN outputs, the other problems
    untouched) and iters (n, 2) = {doubling steps, Smith squarings}."""
    from . import _lib
    return _lib.get_context().mpc_build_batch(As, Bs, Qs, Rs, Ns, Ps=Ps, C_rows=C_rows, Nys=Nys, tol=tol, max_iter=max_iter,
                                              newton_steps=newton_steps, newton_tol=newton_tol,
                                              newton_max_iter=newton_max_iter)


def mpc_diff(U, p):
    """D U: the block first difference, (D U)_k = u_k - u_{k-1}, (D U)_0 = u_0."""
    s = np.array(U, dtype=np.float64)
    s[p:] -= U[:-p]
    return s


def mpc_diff_t(w, p):
    """D'w: (D'w)_k = w_k - w_{k+1}, the last block w_{N-1}."""
    r = np.array(w, dtype=np.float64)
    r[:-p] -= w[p:]
    return r


def mpc_matrices(H, rho, p):
    """(M, Hinv) = ((H + rho (I + D'D))^-1, H^-1): what a call forms once.  Raises np.linalg.LinAlgError when H is not
    positive definite."""
    H = np.asarray(H, dtype=np.float64)
    nv = H.shape[0]
    D = np.eye(nv) - np.eye(nv, k=-p)
    eye = np.eye(nv)
    Hinv = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, lower=True), eye)
    M = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H + rho * (eye + D.T @ D), lower=True), eye)
    return _sym(M), _sym(Hinv)


def mpc_default_rho(H):
    """sqrt(lambda_min(H) lambda_max(H)): the fixed step that reached 1e-9 of the bound in at most 26 / 52 / 242 iterations at
    N = 32 for Q = c C'C, c = 1 / 1e2 / 1e4 on the Duffing models."""
    ev = np.linalg.eigvalsh(np.asarray(H, dtype=np.float64))
    if not ev[0] > 0:
        raise np.linalg.LinAlgError("H is not positive definite")
    return float(np.sqrt(ev[0] * ev[-1]))


def mpc_admm_step(M, rho, g, lo_c, hi_c, z, lam, p):
    """One iteration on the constraint rows A_c = [I; D] (2 nv rows; lo_c, hi_c their bounds, the first p rate rows already
    shifted by the control applied last):  w = z - lambda;  U = M (rho (w_1 + D'w_2) - g);  s = A_c U;
    z = clip(s + lambda);  lambda += s - z.  Returns (U, z, lambda, max |s - z|)."""
    nv = g.size
    w = z - lam
    U = M @ (rho * (w[:nv] + mpc_diff_t(w[nv:], p)) - g)
    s = np.concatenate([U, mpc_diff(U, p)])
    z = np.minimum(np.maximum(s + lam, lo_c), hi_c)
    lam = lam + (s - z)
    return U, z, lam, float(np.max(np.abs(s - z)))


def mpc_saturate(v, lo, hi, dlo, dhi, u_prev):
    """clip(clip(v, lo, hi), u_prev + dlo, u_prev + dhi) on the p entries of one move: the rate clip last."""
    p = np.size(v)
    a = np.minimum(np.maximum(np.asarray(v, dtype=np.float64).reshape(p), lo[:p]), hi[:p])
    return np.minimum(np.maximum(a, u_prev + dlo[:p]), u_prev + dhi[:p])


def mpc_bounds(nv, lo=None, hi=None, dlo=None, dhi=None):
    """The four bound vectors of nv entries; None is the infinite bound, a scalar or one move (p entries) is repeated."""
    def full(a, missing):
        if a is None:
            return np.full(nv, missing)
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        if nv % a.size:
            raise ValueError(f"a bound of {a.size} entries does not tile {nv} decision variables")
        return np.ascontiguousarray(np.tile(a, nv // a.size))
    return full(lo, -np.inf), full(hi, np.inf), full(dlo, -np.inf), full(dhi, np.inf)


def mpc_solve(H, g, lo, hi, dlo, dhi, u_prev, rho, iters, tol=0.0, p=1, M=None, Hinv=None, K_e=None):
    """One solve of  min 1/2 U'HU + g'U,  lo <= U <= hi,  dlo <= u_k - u_{k-1} <= dhi  (u_{-1} = u_prev) by the iteration of
    include/nyskoop.h -- the NumPy statement the device kernel follows:
        U_unc = -H^-1 g;  s = A_c U_unc;  z = clip(s);  lambda = 0;  r = max |s - z|;  k = 0
        while k < iters and not (r <= tol and (k == 0 or tol > 0)):  mpc_admm_step;  k += 1
        u = clip(clip(z[:p], lo, hi), u_prev + dlo, u_prev + dhi)
    Returns (u (p,), z_1 (nv,), (k, r)).  iters = 0 is the saturated LQR: u from v = -K_e (the caller's K e), z_1 = None.
    lo, hi, dlo, dhi: nv entries each (mpc_bounds); M, Hinv: mpc_matrices(H, rho, p) when the caller keeps them."""
    u_prev = np.zeros(p) if u_prev is None else np.asarray(u_prev, dtype=np.float64).reshape(p)
    if iters == 0:
        return mpc_saturate(-np.asarray(K_e, dtype=np.float64).reshape(p), lo, hi, dlo, dhi, u_prev), None, (0, 0.0)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    nv = g.size
    if M is None or Hinv is None:
        M, Hinv = mpc_matrices(H, rho, p)
    shift = np.zeros(nv)
    shift[:p] = u_prev
    lo_c, hi_c = np.concatenate([lo, dlo + shift]), np.concatenate([hi, dhi + shift])
    U = -(Hinv @ g)
    s = np.concatenate([U, mpc_diff(U, p)])
    z = np.minimum(np.maximum(s, lo_c), hi_c)
    lam = np.zeros(2 * nv)
    r, k = float(np.max(np.abs(s - z))), 0
    while k < iters and not (r <= tol and (k == 0 or tol > 0)):
        U, z, lam, r = mpc_admm_step(M, rho, g, lo_c, hi_c, z, lam, p)
        k += 1
    return mpc_saturate(z[:p], lo, hi, dlo, dhi, u_prev), z[:nv].copy(), (k, r)


class MPCController:
    """What reg.solve_mpc returns: the condensed QP (H, F), the bounds lo, hi, dlo, dhi (nv entries each, +-inf where
    absent), the LQR gain K of the same cost (the saturated-LQR mode, iters = 0), rho and the horizon.  Plain arrays: picklable."""

    def __init__(self, H, F, lo, hi, dlo, dhi, K, rho, horizon):
        self.H, self.F = np.ascontiguousarray(H, dtype=np.float64), np.ascontiguousarray(F, dtype=np.float64)
        self.K = np.ascontiguousarray(K, dtype=np.float64)
        self.lo, self.hi, self.dlo, self.dhi = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi, dlo, dhi))
        self.rho, self.horizon = float(rho), int(horizon)
        self._mats = None

    n_inputs = property(lambda self: self.K.shape[0])
    nv = property(lambda self: self.H.shape[0])

    def matrices(self):
        if self.__dict__.get("_mats") is None:
            self._mats = mpc_matrices(self.H, self.rho, self.n_inputs)
        return self._mats

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_mats"] = None
        return st

    def control(self, e, u_prev=None, iters=50, tol=0.0):
        """The control for the lifted error e = phi(x) - phi(x_ref) (m,): (u (p,), (iterations, residual)) by mpc_solve."""
        e = np.asarray(e, dtype=np.float64).reshape(-1)
        if iters == 0:
            u, _, info = mpc_solve(None, None, self.lo, self.hi, self.dlo, self.dhi, u_prev, self.rho, 0, p=self.n_inputs,
                                   K_e=self.K @ e)
            return u, info
        M, Hinv = self.matrices()
        u, _, info = mpc_solve(self.H, self.F @ e, self.lo, self.hi, self.dlo, self.dhi, u_prev, self.rho, iters, tol,
                               self.n_inputs, M, Hinv)
        return u, info


# ---------------------------------------------------------------------------------------------------------------------------
# Limits on predicted states, hard or soft (nk_mpc_out_loop, nk_mpc_out_qp_host; csrc/nk_mpc_out.h, nk_mpc_loop.hip): ny
# output rows G U + T e with their own bounds join the constraint rows, A_c = [I; D; G].
# ---------------------------------------------------------------------------------------------------------------------------
def mpc_condense_outputs(A, B, C_rows, N, Ny=None):
    """(G, T) of the predicted outputs y_k = C_rows e_k, k = 1 .. Ny (Ny <= N, default N), under e_{k+1} = A e_k + B u_k as a
    function of U (nv = N p entries) and e_0: the stacked outputs are G U + T e_0, row (k, c) at (k - 1) nc + c.  Row (k, c) of T
    is C_c A^k, block (k, j) of G is C_c A^(k-1-j) B for j < k and 0 otherwise.  Only thin products: R_k = R_{k-1} A (nc x m)
    from R_0 = C_rows, and R_i B; no power of A is formed."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(m, -1)
    p = B.shape[1]
    R = np.asarray(C_rows, dtype=np.float64).reshape(-1, m)
    nc = R.shape[0]
    N = int(N)
    Ny = N if Ny is None else int(Ny)
    if N < 1 or not 1 <= Ny <= N:
        raise ValueError("the horizons must satisfy 1 <= Ny <= N")
    G, T = np.zeros((Ny * nc, N * p)), np.zeros((Ny * nc, m))
    RB = []
    for k in range(1, Ny + 1):
        RB.append(R @ B)  # C A^(k-1) B
        R = R @ A         # C A^k
        T[(k - 1) * nc:k * nc] = R
        for j in range(k):
            G[(k - 1) * nc:k * nc, j * p:(j + 1) * p] = RB[k - 1 - j]
    return G, T


def mpc_out_matrices(H, rho, p, G):
    """(Kb, S0, M) of a call with output rows G (ny x nv): M = (H + rho (I + D'D + G'G))^-1 by Cholesky, symmetrised;
    Kb = [[M, M G'], [G M, G M G']] (nt x nt, nt = nv + ny) by plain products from M, symmetrised; S0 = [H^-1; G H^-1] (nt x nv).
    Raises np.linalg.LinAlgError when a matrix is not positive definite."""
    H, G = np.asarray(H, dtype=np.float64), np.asarray(G, dtype=np.float64)
    nv = H.shape[0]
    G = G.reshape(-1, nv)
    D = np.eye(nv) - np.eye(nv, k=-p)
    eye = np.eye(nv)
    Hinv = _sym(scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, lower=True), eye))
    M = _sym(scipy.linalg.cho_solve(scipy.linalg.cho_factor(H + rho * (eye + D.T @ D + G.T @ G), lower=True), eye))
    MG = M @ G.T
    Kb = np.block([[M, MG], [G @ M, G @ MG]])
    return _sym(Kb), np.vstack([Hinv, G @ Hinv]), M


def mpc_out_theta(rho, y_weight):
    """rho / (rho + w_y), and 0 for w_y = inf (hard rows)."""
    return 0.0 if np.isinf(y_weight) else float(rho / (rho + y_weight))


def mpc_out_shift(ylo, yhi, ycomp, x_ref=None):
    """The bounds of the output rows in error coordinates, b = ylo_r - x_ref[ycomp_r] (one rounded subtraction per row; a row
    with ycomp = -1, or x_ref = None, keeps its bound)."""
    ylo, yhi = np.array(ylo, dtype=np.float64).reshape(-1), np.array(yhi, dtype=np.float64).reshape(-1)
    if x_ref is not None:
        yc = np.asarray(ycomp, dtype=np.int64).reshape(-1)
        xr = np.asarray(x_ref, dtype=np.float64).reshape(-1)
        sel = yc >= 0
        ylo[sel] = ylo[sel] - xr[yc[sel]]
        yhi[sel] = yhi[sel] - xr[yc[sel]]
    return ylo, yhi


def mpc_out_prox(v, lo_c, hi_c, nrows_in, theta):
    """clip on the box and rate rows (the first nrows_in); on the output rows c = clip(v), z = c + theta (v - c)."""
    c = np.minimum(np.maximum(v, lo_c), hi_c)
    if theta != 0.0:
        c[nrows_in:] = c[nrows_in:] + theta * (v[nrows_in:] - c[nrows_in:])
    return c


def mpc_out_solve(g, t, lo, hi, dlo, dhi, ylo_b, yhi_b, u_prev, rho, theta, iters, tol, p, Kb, S0):
    """One solve of  min 1/2 U'HU + g'U + (w_y / 2) dist^2(G U + t, [ylo_b, yhi_b])  under the box and rate limits of mpc_solve,
    by the folded iteration of include/nyskoop.h -- the NumPy statement the device kernel follows.  Rows of a stacked vector:
    (nv box, nv rate, ny output); s_K = (s_1, s_3) has nt = nv + ny entries.
        bounds of the output rows: ylo_b - t, yhi_b - t  (ylo_b, yhi_b: mpc_out_shift)
        s_K = -(S0 g);  s = (s_K[:nv], D s_K[:nv], s_K[nv:]);  z = prox(s);  lambda = 0;  r = max |s - z|;  k = 0
        while k < iters and not (r <= tol and (k == 0 or tol > 0)):
            w = z - lambda;  q = [rho (w_1 + D'w_2) - g; rho w_3];  s_K = Kb q;  z = prox(s + lambda);  lambda += s - z
            r = max |s - z|;  k += 1
        u = clip(clip(z[:p], lo, hi), u_prev + dlo, u_prev + dhi)
    Returns (u (p,), z_K = (z_1, z_3) (nt,), (k, r)).  iters >= 1."""
    g, t = np.asarray(g, dtype=np.float64).reshape(-1), np.asarray(t, dtype=np.float64).reshape(-1)
    nv, ny = g.size, t.size
    u_prev = np.zeros(p) if u_prev is None else np.asarray(u_prev, dtype=np.float64).reshape(p)
    shift = np.zeros(nv)
    shift[:p] = u_prev
    lo_c = np.concatenate([lo, dlo + shift, np.asarray(ylo_b, dtype=np.float64) - t])
    hi_c = np.concatenate([hi, dhi + shift, np.asarray(yhi_b, dtype=np.float64) - t])

    def rows(sK):
        return np.concatenate([sK[:nv], mpc_diff(sK[:nv], p), sK[nv:]])

    s = rows(-(S0 @ g))
    z = mpc_out_prox(s, lo_c, hi_c, 2 * nv, theta)
    lam = np.zeros(2 * nv + ny)
    r, k = float(np.max(np.abs(s - z))), 0
    while k < iters and not (r <= tol and (k == 0 or tol > 0)):
        w = z - lam
        q = np.concatenate([rho * (w[:nv] + mpc_diff_t(w[nv:2 * nv], p)) - g, rho * w[2 * nv:]])
        s = rows(Kb @ q)
        z = mpc_out_prox(s + lam, lo_c, hi_c, 2 * nv, theta)
        lam = lam + (s - z)
        r = float(np.max(np.abs(s - z)))
        k += 1
    return mpc_saturate(z[:p], lo, hi, dlo, dhi, u_prev), np.concatenate([z[:nv], z[2 * nv:]]), (k, r)


class MPCOutputController(MPCController):
    """MPCController with ny output rows: G (ny x nv), T (ny x m) (mpc_condense_outputs), the absolute state bounds ylo, yhi
    of the rows (+-inf where absent), ycomp (the state component of a row, -1 for a row without a reference shift) and
    y_weight (np.inf: hard rows; finite > 0: the squared violation is penalised).  Plain arrays: picklable."""

    def __init__(self, H, F, lo, hi, dlo, dhi, K, rho, horizon, G, T, ylo, yhi, ycomp, y_weight=np.inf):
        super().__init__(H, F, lo, hi, dlo, dhi, K, rho, horizon)
        self.G, self.T = np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(T, dtype=np.float64)
        self.ylo, self.yhi = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (ylo, yhi))
        self.ycomp = np.ascontiguousarray(ycomp, dtype=np.int32).reshape(-1)
        self.y_weight = float(y_weight)
        ny = self.ylo.size
        if self.G.shape != (ny, self.nv) or self.T.shape != (ny, self.F.shape[1]) or self.yhi.size != ny or self.ycomp.size != ny:
            raise ValueError(f"G {self.G.shape}, T {self.T.shape}, ylo, yhi and ycomp must describe the same {ny} output rows")
        if not self.y_weight > 0:
            raise ValueError("y_weight must be positive (np.inf: hard rows)")
        self._omats = None

    ny = property(lambda self: self.G.shape[0])

    def out_matrices(self):
        if self.__dict__.get("_omats") is None:
            self._omats = mpc_out_matrices(self.H, self.rho, self.n_inputs, self.G)
        return self._omats

    def __getstate__(self):
        st = super().__getstate__()
        st["_omats"] = None
        return st

    def input_only(self):
        """The MPCController of the same problem without the output rows."""
        return MPCController(self.H, self.F, self.lo, self.hi, self.dlo, self.dhi, self.K, self.rho, self.horizon)

    def control(self, e, u_prev=None, iters=50, tol=0.0, x_ref=None):
        """The control for the lifted error e = phi(x) - phi(x_ref) (m,) and the reference state x_ref (None: no shift of the
        output bounds): (u (p,), (iterations, residual)) by mpc_out_solve; iters = 0 is the saturated LQR of MPCController."""
        if iters == 0:
            return super().control(e, u_prev, 0, tol)
        e = np.asarray(e, dtype=np.float64).reshape(-1)
        Kb, S0, _ = self.out_matrices()
        yl, yh = mpc_out_shift(self.ylo, self.yhi, self.ycomp, x_ref)
        u, _, info = mpc_out_solve(self.F @ e, self.T @ e, self.lo, self.hi, self.dlo, self.dhi, yl, yh, u_prev, self.rho,
                                   mpc_out_theta(self.rho, self.y_weight), iters, tol, self.n_inputs, Kb, S0)
        return u, info
