"""Landmark selection on the device (nk_select_landmarks, include/nyskoop.h): partial pivoted Cholesky of K(Y, Y) with a
greedy or a randomised (RPCholesky) pick rule.  An extension beyond the reference, which draws landmarks uniformly at
random (regressors.py:129-132)."""
import ctypes as C

import numpy as np

from . import _lib

RULES = {"greedy": _lib.NK_LANDMARK_GREEDY, "rpcholesky": _lib.NK_LANDMARK_RPCHOLESKY}


def select_landmarks(Y, kernel, m, rule="greedy", row_ranges=None, tol=0.0, u=None, return_info=False):
    """Rows of Y chosen as Nystrom landmarks for `kernel` (a KernelWrapper / ThreeDimensionalKernel / LinearKernelWrapper,
    or its DeviceKernel), in pick order.

    Y: n x d, a NumPy array or a float64 device tensor.  row_ranges: [begin, end) pairs; the candidates are their rows
    concatenated in the order given (None: all rows), exactly the training rows of a fit with the same `row_ranges`.
    rule: "greedy" (largest residual diagonal entry, ties to the lowest candidate position) or "rpcholesky" (a row drawn
    in proportion to the residual diagonal; `u`: m uniforms in [0, 1), by default np.random.uniform(size=m) from the
    global legacy RNG in one call).  tol: stop once the picked residual is <= tol times the largest initial diagonal
    entry, so fewer than m rows may come back.  The selection is nested: the result for m is a prefix of the result for
    any larger m (with the same leading u).

    Returns the int64 row indices (length m_selected <= m); with return_info=True also a dict with `resid` (the
    residual at which each row was picked: the squared Cholesky pivot of K_mm at that landmark), `trace` (m_selected + 1
    entries: the sum of the residual diagonal before each step and, last, the trace left) and `stop_resid` (the
    residual that fired the stop rule, or None)."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)}, got {rule!r}")
    ctx = _lib.get_context()
    Ym = _lib.Mat(Y)
    n, d = Ym.shape
    m = int(m)
    kern = getattr(kernel, "kernel", kernel)
    kd, keep = kern.desc(d)
    up = None
    if rule == "rpcholesky":
        u = np.random.uniform(size=max(m, 0)) if u is None else np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.size < m:
            raise ValueError(f"u has {u.size} entries, m = {m} are needed")
        up = u.ctypes.data
    flat = None if row_ranges is None else np.ascontiguousarray(np.asarray(row_ranges, dtype=np.int64).reshape(-1))
    rr = None if flat is None else flat.ctypes.data_as(C.POINTER(C.c_int64))
    rows = np.full(max(m, 1), -1, dtype=np.int64)
    resid = np.zeros(max(m, 1))
    trace = np.zeros(max(m, 1) + 1)
    count = C.c_int32(0)
    ctx.wait_for(Y)
    rc = ctx.lib.nk_select_landmarks(ctx.handle, C.byref(kd), Ym.ptr, Ym.ld, n, d, rr, 0 if flat is None else flat.size // 2,
                                     RULES[rule], up, m, float(tol), rows.ctypes.data, resid.ctypes.data, trace.ctypes.data,
                                     C.byref(count))
    _lib.check_mapped(rc)
    k = int(count.value)
    if not return_info:
        return rows[:k].copy()
    return rows[:k].copy(), dict(resid=resid[:k].copy(), trace=trace[:k + 1].copy(),
                                 stop_resid=float(resid[k]) if k < m else None)
