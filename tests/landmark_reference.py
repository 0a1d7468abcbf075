"""NumPy reference of the landmark selection (nk_select_landmarks): partial pivoted Cholesky of K(Y, Y) over candidate
rows with the greedy or the RPCholesky pick rule, in float64 or np.longdouble.  No GPU, no project code.

A kernel is a dict: {"kind": "rbf" | "matern52", "length_scale": scalar or d values} or {"kind": "linear", "sigma0": s}.
Kernel values come from direct differences (dot products for the linear kernel) of coordinates divided by the length
scale, like the device code."""
import numpy as np


def _scaled(Y, kernel, positions, dtype):
    Y = np.asarray(Y, dtype=np.float64)
    if positions is not None:
        Y = Y[np.asarray(positions, dtype=np.int64)]
    Ys = Y.astype(dtype)
    if kernel["kind"] != "linear":
        w = dtype(1.0) / np.atleast_1d(np.asarray(kernel["length_scale"], dtype=np.float64)).astype(dtype)
        Ys = Ys * w
    return Ys


def _column(Ys, kernel, i):
    """k(y_r, y_i) for every candidate r."""
    dtype = Ys.dtype.type
    if kernel["kind"] == "linear":
        return Ys @ Ys[i] + dtype(kernel.get("sigma0", 0.0)) ** 2
    r2 = ((Ys - Ys[i]) ** 2).sum(axis=1)
    if kernel["kind"] == "rbf":
        return np.exp(dtype(-0.5) * r2)
    if kernel["kind"] == "matern52":
        t = np.sqrt(dtype(5.0) * r2)
        return (dtype(1.0) + t + t * t / dtype(3.0)) * np.exp(-t)
    raise ValueError(kernel["kind"])


def _diagonal(Ys, kernel):
    dtype = Ys.dtype.type
    if kernel["kind"] == "linear":
        return (Ys * Ys).sum(axis=1) + dtype(kernel.get("sigma0", 0.0)) ** 2
    return np.ones(len(Ys), dtype=Ys.dtype)


def _step(Ys, kernel, F, dg, j, piv):
    c = _column(Ys, kernel, piv) - F[:, :j] @ F[piv, :j]
    F[:, j] = c / np.sqrt(dg[piv])
    dg[:] = np.maximum(dg - F[:, j] ** 2, 0)
    dg[piv] = 0


def pchol(Y, kernel, m, rule="greedy", u=None, tol=0.0, positions=None, dtype=np.float64):
    """m steps over the candidates Y[positions] (all rows when None).  Greedy: the largest residual, ties to the LOWEST
    candidate position.  RPCholesky: the smallest position whose inclusive prefix sum of the residual diagonal exceeds
    u[j] * T; entries with a zero residual are never picked.  Stop (m_selected = j) when dg[piv] <= tol * dg0max or
    dg[piv] <= 0.  Returns a dict: pivots (candidate positions, m_selected of them), resid (one per step taken, plus the
    one that fired the stop rule), trace (sum of dg before each step taken; last entry = the trace left), F (the factor,
    n_c x m_selected), m_selected, gap (largest minus second-largest residual at every step taken)."""
    Ys = _scaled(Y, kernel, positions, dtype)
    nc = len(Ys)
    dg = _diagonal(Ys, kernel)
    dg0max = dg.max()
    F = np.zeros((nc, m), dtype=Ys.dtype)
    pivots, resid, trace, gap = [], [], [], []
    for j in range(m):
        T = dg.sum()
        if rule == "greedy":
            piv = int(np.argmax(dg))  # the first of equal maxima
        else:
            cs = np.cumsum(dg)
            hit = np.nonzero((cs > dtype(u[j]) * T) & (dg > 0))[0]
            pos = np.nonzero(dg > 0)[0]
            piv = int(hit[0]) if len(hit) else (int(pos[-1]) if len(pos) else 0)
        trace.append(T)
        resid.append(dg[piv])
        if dg[piv] <= dtype(tol) * dg0max or dg[piv] <= 0:
            break
        top = np.sort(dg)[-2:] if nc > 1 else np.array([0, dg[piv]], dtype=Ys.dtype)
        gap.append(top[1] - top[0])
        pivots.append(piv)
        _step(Ys, kernel, F, dg, j, piv)
    else:
        trace.append(dg.sum())
    k = len(pivots)
    return dict(pivots=np.array(pivots, dtype=np.int64), resid=np.array(resid, dtype=Ys.dtype),
                trace=np.array(trace, dtype=Ys.dtype), F=F[:, :k], m_selected=k, gap=np.array(gap, dtype=Ys.dtype))


def replay(Y, kernel, pivots, positions=None, dtype=np.float64):
    """Residual diagonals and traces for a GIVEN pivot sequence (candidate positions).  Per step j, before the step:
    resid[j] = dg[pivots[j]], trace[j] = sum dg, dgmax[j] = max dg, cum_lo[j] / cum_hi[j] = the exclusive / inclusive
    prefix sum of dg at the pivot; trace has one more entry, the trace left.  A pivot whose replayed residual is not
    positive cannot be eliminated: ValueError."""
    Ys = _scaled(Y, kernel, positions, dtype)
    nc, m = len(Ys), len(pivots)
    dg = _diagonal(Ys, kernel)
    F = np.zeros((nc, m), dtype=Ys.dtype)
    out = {k: np.zeros(m, dtype=Ys.dtype) for k in ("resid", "dgmax", "cum_lo", "cum_hi")}
    trace = np.zeros(m + 1, dtype=Ys.dtype)
    for j, piv in enumerate(int(p) for p in pivots):
        cs = np.cumsum(dg)
        trace[j], out["resid"][j], out["dgmax"][j] = dg.sum(), dg[piv], dg.max()
        out["cum_hi"][j], out["cum_lo"][j] = cs[piv], (cs[piv - 1] if piv > 0 else 0)
        if not dg[piv] > 0:
            raise ValueError(f"step {j}: the replayed residual of pivot {piv} is {dg[piv]}")
        _step(Ys, kernel, F, dg, j, piv)
    trace[m] = dg.sum()
    return dict(out, trace=trace, dg0max=_diagonal(Ys, kernel).max())


def kernel_matrix(Y, kernel, positions=None, dtype=np.float64):
    Ys = _scaled(Y, kernel, positions, dtype)
    return np.stack([_column(Ys, kernel, i) for i in range(len(Ys))], axis=1)
