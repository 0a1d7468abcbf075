"""Extended-precision reference for the QP iteration of the MPC loops (mpc_loop_body<KTYPE, D, NP, OUT, SCORED>,
csrc/nk_mpc_loop.hip: nk_mpc_loop, nk_mpc_out_loop and their _multi forms), with an entry-wise bar propagated alongside the
iteration, a float64 emulation of the device's order with planted faults, and the cases tests/test_gpu_mpc_qp_steps.py runs.
NumPy only; nothing here touches the GPU, and nothing of the library stands on the reference side (no lqr.mpc_solve, no
MPCController method, no nk_mpc_qp_host).

The check is open loop per step.  For step t of a trajectory the control u_t and the pair info_t = {iterations, final
max |s - z|} are recomputed in longdouble from the state x_t and the control u_{t-1} the device stored (u_init for t = 0):
  gradient   gt = [F; T] (phi(x_t) - phi(x_ref)) = -plant_loop_reference.control_reference(...)["u"] with w = S^-1 [F; T]'
             folded in longdouble from the model's own K_mm^-1/2 (spline models: no fold); its bar there, with the reduction
             count mpc_reduction_c(m), is the input error dg (nv entries) and dt (ny entries) below.
  matrices   H^-1, M = (H + rho (I + D'D [+ G'G]))^-1, Kb = [[M, M G'], [G M, G M G']], S0 = [H^-1; G H^-1] in longdouble from
             the H, G, rho passed: a Cholesky factor, its inverse by substitution, one product (spd_inverse_ld).
  bounds     u_prev + dlo, ylo - x_ref[c]: one IEEE operation each, formed in float64 as the interface states them (they are
             bit-determined); (ylo - x_ref[c]) - t_r carries dt and one rounding.
  iteration  the order of include/nyskoop.h as mpc_qp / mpc_out_qp (csrc/nk_mpc.h:143-215, nk_mpc_out.h:123-207) write it out.

The bar.  u = 2^-53, gamma_k = k u / (1 - k u).  All bars are entry-wise, float64, and carried beside the longdouble values;
|x| in a rounding term stands for |x_ref| + dx, so the second-order terms are inside.  No tolerance and no factor is chosen.
  inverses   mpc_spd_inverse (nk_mpc.h:77-106) forms A = L L' (Higham, Accuracy and Stability, 2nd ed., Theorem 10.3:
             L^ L^' = A + dA, |dA| <= gamma_{n+1} |L^| |L^'|), X = L^-1 column by column by substitution (Theorem 8.5:
             (L^ + dL_c) x^_c = e_c, |dL_c| <= gamma_n |L^|, so |X^ - L^^-1| <= gamma_n |L^-1| |L| |X|) and inv = X'X
             (3.1: gamma_n |X'| |X|), so to first order in u, with the longdouble L and X,
               dInv(A) = gamma_{n+1} |A^-1| (|L| |L'|) |A^-1| + gamma_n (|X'| Y + Y' |X|) + gamma_n |X'| |X|,  Y = |X| |L| |X|
             (the terms of second order are below cond(A) u ~ 1e-15 of it: H is designed with cond of order 10).  The
             argument of the second inverse is rounded when it is formed (nk_mpc.h:113-120, nk_mpc_out.h:53-66: at most ny + 4
             roundings on an entry): dA_in = gamma_{ny+4} (|H| + rho (|I + D'D| + |G|'|G|)), and dM = dInv + |M| dA_in |M|.
  products   mpc_out_prepare (nk_mpc_out.h:69-101): M G' and G M are nv-term sums, their mean one more rounding; G (M G') is an
             nv-term sum of that, symmetrised with one more; G H^-1 an nv-term sum: dKb, dS0 by gamma_nv |.||.| on top of
             what dM and dH^-1 hand on.
  start      s = -S0 g, nv FMAs in index order (nk_mpc_loop.hip:171-173): ds = |dS0| |g| + |S0| dg + gamma_nv |S0| |g|.
             s2 = s_i - s_{i-p}: one rounding (:149-153).  z = prox(s): clip is 1-Lipschitz in (v, lo, hi) jointly, and so is
             the soft prox c + theta (v - c) = (1 - theta) c + theta v: dz = max(dv, db), db the bar of the lane's bound (zero
             for an input lane); the soft form adds gamma_2 theta |v - c| + u |z| (:154-159).
  iteration  (:181-196) w2 = z2 - l2, dt = w2 - w2n, (z1 - l1) + dt: one rounding each; rhs = rho (.) - g: two (one as an
             FMA); U: a chain of NP FMAs over Krow of which nt are non-zero (a zero row entry adds exactly):
             dU = |dKb| |rhs| + |Kb| drhs + gamma_nt |Kb| |rhs|; the shift subtraction; v = s + l one rounding; the prox; the
             dual l' = l + (s - z), two roundings.  With v = s + l the exact new dual N(v) = v - prox(v) is 1-Lipschitz in v (and
             in the bound), so dl' = (ds + dl) + db + u |v| + (soft) + u |s - z| + u |l'|: the dual's bar grows additively.
  control    clip(clip(z1, lo, hi), dlo, dhi) is 1-Lipschitz and its bounds are exact: du = dz1.  A disagreement about the
             side of a bound is covered by the same fact; no step is left out for it.
  residual   r = max of |s - z| over lanes and slots: d|s - z| = ds + dz + u |s - z| per entry, dr the largest entry bar.
The bar grows with the iteration count: a lane's right-hand side collects rho (dz1 + dl1 + dz2 + dl2 of two lanes), at most
rho (5 ds + 6 dl) with dz = ds + dl and ds2 <= 2 ds, so with f = 6 rho || |Kb| ||_inf the pair obeys ds' <= f (5 ds / 6 + dl) + c,
dl' = dl + ds': the dual's bar is additive in itself but feeds the next product, a factor near 1 + f per iteration on top of
the linear growth.  At the default rho = sqrt(lambda_min lambda_max) f is of order 10 (ladder 1, 2, 3 only); the 30-iteration
cases run at the designed rho = 1 / (96 || |Kb_0| ||_inf), Kb_0 the matrix at rho = 0: f = 1 / 16, (1 + f)^30 = 6.2.

Decisions.  Two comparisons decide the iteration count: r_0 <= tol before the first iteration, and r_k <= tol after one when
tol > 0.  A step is AMBIGUOUS when |r_k - tol| <= dr_k at a comparison the reference makes, or, for tol = 0, when r_0 <= dr_0
without every start iterate lying farther than its bar inside its bounds (then r_0 = 0 on both sides).  Ambiguous steps
are left out of the control and info comparison and counted; at most 2 % of a case's steps may be (AMBIGUITY_CAP).

Reference and emulation share one statement of the iteration (qp_core), in two number formats, on two sets of matrices
(longdouble inverse / float64 mirror of mpc_spd_inverse and mpc_out_prepare), two gradients (longdouble sum / the wave
chains of plant_loop_reference.emulate) and two product orders (a longdouble matrix product / the index-order chains).  The
planted faults change the emulation alone.  The ladder's runs do not share a reference run: the check is per step on the
states of each run, which differ with `iters`.

Measured (profiles/README.md, "MPC QP steps"; profiles/mpc_qp_steps.log): the float64 emulation stays at 2.9e-3 of the bar or
below, the weakest planted fault exceeds it by 232 bars, the least visible lane moves a control by 2.9e5 bars, and the bar grows
by a factor of 131 at most over 30 iterations; the device's worst ratios are in the docstring of tests/test_gpu_mpc_qp_steps.py."""
import collections
import functools
import types

import numpy as np

import plant_loop_reference as P
from plant_loop_reference import HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP, U64, gamma  # noqa: F401

STEPS, BATCH = 8, P.BATCH
AMBIGUITY_CAP = 0.02
INF = np.inf


def ab(x, dx=0.0):
    """|x| + dx in float64: what a rounding term multiplies."""
    return np.abs(x).astype(np.float64) + dx


# ---------------------------------------------------------------------------------------------------------------------
# matrices: longdouble with bars, and the float64 mirror of the library's prepare code
# ---------------------------------------------------------------------------------------------------------------------
def spd_inverse_ld(A):
    """(A^-1, L, X = L^-1) in longdouble."""
    A = np.asarray(A).astype(LD)
    n = A.shape[0]
    L, X = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    for i in range(n):
        X[i, i] = 1 / L[i, i]
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X.T @ X, L, X


def inverse_bar(Ainv, L, X):
    """dInv(A) of the module docstring."""
    n = L.shape[0]
    aL, aX, aI = ab(L), ab(X), ab(Ainv)
    Y = aX @ aL @ aX
    return gamma(n + 1) * (aI @ (aL @ aL.T) @ aI) + gamma(n) * (aX.T @ Y + Y.T @ aX) + gamma(n) * (aX.T @ aX)


def idd(nv, p):
    """I + D'D: 3 I (the last block 2 I) on the diagonal, -I beside it."""
    D = np.eye(nv) - np.eye(nv, k=-p)
    return np.eye(nv) + D.T @ D


def matrices_ld(H, G, rho, p):
    """Namespace(Kb (nt x nt), S0 (nt x nv) longdouble, dKb, dS0 float64) from the H, G (ny x nv, ny may be 0), rho passed."""
    H = np.asarray(H, dtype=np.float64)
    nv = H.shape[0]
    G = np.asarray(G, dtype=np.float64).reshape(-1, nv)
    ny = G.shape[0]
    Gl, aG = G.astype(LD), np.abs(G)
    Hinv, L, X = spd_inverse_ld(H)
    dH = inverse_bar(Hinv, L, X)
    A = H.astype(LD) + LD(rho) * (idd(nv, p).astype(LD) + Gl.T @ Gl)
    M, L, X = spd_inverse_ld(A)
    aM = ab(M)
    dM = inverse_bar(M, L, X) + aM @ (gamma(ny + 4) * (np.abs(H) + rho * (np.abs(idd(nv, p)) + aG.T @ aG))) @ aM
    MG = M @ Gl.T
    dMG = dM @ aG.T + gamma(nv) * ((aM + dM) @ aG.T)
    dMGs = dMG + U64 * ab(MG, dMG)  # the mean of M G' and (G M)': one more rounding
    GMG = Gl @ MG
    dGMG = aG @ dMG + gamma(nv) * (aG @ ab(MG, dMG))
    dGMG = (dGMG + dGMG.T) / 2 + U64 * ab(GMG, dGMG)
    Kb = np.block([[M, MG], [MG.T, GMG]])
    dKb = np.block([[dM, dMGs], [dMGs.T, dGMG]])
    GH = Gl @ Hinv
    dGH = aG @ dH + gamma(nv) * (aG @ ab(Hinv, dH))
    return types.SimpleNamespace(Kb=Kb, dKb=dKb, S0=np.vstack([Hinv, GH]), dS0=np.vstack([dH, dGH]), rho=float(rho))


def spd_inverse64(A):
    """mpc_spd_inverse (nk_mpc.h:77-106) in float64, its sums in the library's index order."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        s = A[j:, j].copy()
        for k in range(j):
            s -= L[j:, k] * L[j, k]
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    X = np.zeros((n, n))
    for i in range(n):  # row i of L^-1, all columns at once; the sum over k in index order
        s = np.zeros(n)
        for k in range(i):
            s -= L[i, k] * X[k]
        s[i] = 1.0
        X[i] = s / L[i, i]
    inv = np.zeros((n, n))
    for k in range(n):
        inv += np.outer(X[k], X[k])
    return inv


def _dot_chain(A, B):
    """A @ B with the inner sum in index order."""
    out = np.zeros((A.shape[0], B.shape[1]))
    for k in range(A.shape[1]):
        out += np.outer(A[:, k], B[k])
    return out


def matrices64(H, G, rho, p, fault=None):
    """mpc_prepare / mpc_out_prepare (nk_mpc.h:110-123, nk_mpc_out.h:48-103) in float64: Namespace(Kb, S0 (nt x nv)).
    Faults: last_block_3I, no_rhoGG, kb_offdiag_GM."""
    H = np.asarray(H, dtype=np.float64)
    nv = H.shape[0]
    G = np.asarray(G, dtype=np.float64).reshape(-1, nv)
    ny = G.shape[0]
    Hinv = spd_inverse64(H)
    A = H.copy()
    for i in range(nv):
        A[i, i] += rho * (3.0 if (i + p < nv or fault == "last_block_3I") else 2.0)
        if i + p < nv:
            A[i, i + p] -= rho
            A[i + p, i] -= rho
    if ny and fault != "no_rhoGG":
        A += rho * _dot_chain(G.T, G)
    M = spd_inverse64(A)
    if not ny:
        return types.SimpleNamespace(Kb=M, S0=Hinv, rho=float(rho))
    MG, GM = _dot_chain(M, G.T), _dot_chain(G, M)
    off = (MG + GM.T) / 2
    GMG = _dot_chain(G, MG)
    GMG = (GMG + GMG.T) / 2
    off_rows = off.T
    if fault == "kb_offdiag_GM":
        off = GM.reshape(nv, ny)
    Kb = np.block([[M, off], [off_rows, GMG]])
    return types.SimpleNamespace(Kb=Kb, S0=np.vstack([Hinv, _dot_chain(G, Hinv)]), rho=float(rho))


def default_rho(H):
    """The formula of lqr.mpc_default_rho, copied: sqrt(lambda_min(H) lambda_max(H))."""
    ev = np.linalg.eigvalsh(np.asarray(H, dtype=np.float64))
    return float(np.sqrt(ev[0] * ev[-1]))


def small_rho(H, G):
    """1 / (96 || |Kb_0| ||_inf), Kb_0 = [[H^-1, H^-1 G'], [G H^-1, G H^-1 G']] (module docstring: f = 1 / 16)."""
    Hi = np.linalg.inv(np.asarray(H, dtype=np.float64))
    G = np.asarray(G, dtype=np.float64).reshape(-1, Hi.shape[0])
    Kb0 = np.block([[Hi, Hi @ G.T], [G @ Hi, G @ Hi @ G.T]])
    return float(1.0 / (96.0 * np.max(np.sum(np.abs(Kb0), axis=1))))


# ---------------------------------------------------------------------------------------------------------------------
# the iteration: one statement, two number formats
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("up_lane_p_plain", "up_lane_pm1_diff", "dt_le_nv", "dt_lt_nv_m1", "dn_wrap", "krow_truncated", "s0_untransposed",
          "kb_offdiag_GM", "last_block_3I", "no_rhoGG", "theta_dropped", "theta_on_input", "bound_plus_t", "xref_wrong_comp",
          "out_rate_slot", "no_rho_out_q", "dual_sign", "l2_not_reset", "uprev_t2", "max_half", "stop_per_lane",
          "rate_before_box")
MATRIX_FAULTS = ("kb_offdiag_GM", "last_block_3I", "no_rhoGG")
# dn_wrap is a name only: qp_core has no branch for it.  The guard lane + p < nv <= 64 never lets a lane read a wrapped
# neighbour, so no result can depend on how `dn` treats lane + p >= 64; fault_applies is False everywhere and the host
# test counts no case for it.


def fault_applies(fault, c, run):
    """Whether the fault can change a result of the run (the host test asserts that it then does, by twice the bar)."""
    nv, nt = c.p * c.N, c.p * c.N + c.ny
    if run.regime == "inactive" or fault == "dn_wrap":
        return False
    if fault in ("up_lane_pm1_diff", "last_block_3I", "dual_sign"):
        return True
    if fault in ("l2_not_reset", "uprev_t2"):
        return run.limits != "no_rate"
    if fault == "rate_before_box":
        return run.limits == "all"
    if fault in ("up_lane_p_plain", "dt_lt_nv_m1"):
        return nv > c.p
    if fault == "dt_le_nv":
        return c.ny == 0
    if fault == "krow_truncated":
        return nt > 16
    if fault in ("no_rhoGG", "bound_plus_t", "out_rate_slot", "no_rho_out_q"):
        return c.ny > 0
    if fault == "s0_untransposed":  # (nv = 1: both readings of the buffer are the same words)
        return c.ny > 0 and nv > 1
    if fault == "kb_offdiag_GM":
        return c.ny > 1 and nv > 1
    if fault in ("theta_dropped", "theta_on_input"):
        return c.ny > 0 and c.soft
    if fault == "xref_wrong_comp":
        return c.ny > 0 and c.d > 1
    if fault == "max_half":  # (nt = 33: lane 32 alone is lost, and no case is designed to hold its largest residual there)
        return nt >= 48
    if fault == "stop_per_lane":
        return nt > 1
    raise ValueError(fault)


def _clip(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def qp_core(c, ctl, A, gt, dgt, uprev, xref, iters, tol, dtype, fault=None, l2_init=None):
    """The step of nk_mpc_loop.hip:127-203 on R rows at once.  c: the case (p, N, ny, d); ctl: the controller's arrays (lo,
    hi, dlo, dhi (nv), ylo, yhi, ycomp (ny), theta); A: matrices_ld / matrices64; gt (R, nt) in `dtype`: g in the input
    lanes, t in the output lanes, dgt its bar; uprev (R, p), xref (R, d) float64.  dtype = LD: the reference (a matrix
    product); float64: the emulation (index-order chains) with `fault`.  Returns a dict: u (R, p), du, it (R,), r, dr, amb
    (R,) bool, margin (R,) = r_0 / dr_0, vis (nt,), growth (list of the largest du-like bar per iteration), l2 (R, nt)."""
    p, nv, ny = c.p, c.p * c.N, c.ny
    nt = nv + ny
    R = gt.shape[0]
    emul = dtype is not LD
    cast = lambda a: np.asarray(a).astype(dtype)
    rho, theta = dtype(A.rho), float(ctl.theta)
    TH = np.zeros(nt)
    TH[nv:] = theta
    if fault == "theta_dropped":
        TH[:] = 0.0
    if fault == "theta_on_input":
        TH[:] = theta
    soft = TH != 0.0
    THd = cast(TH)
    var = np.arange(nt) < nv
    Kb, S0 = cast(A.Kb), cast(A.S0)
    dKb, dS0 = (np.zeros(Kb.shape), np.zeros(S0.shape)) if emul else (A.dKb, A.dS0)
    aKb, aS0 = ab(Kb, dKb), ab(S0, dS0)
    # bounds: the box slot (input lanes: lo / hi; output lanes: (ylo - x_ref[c]) - t) and the rate slot
    LO, HI = np.full((R, nt), -INF, dtype=dtype), np.full((R, nt), INF, dtype=dtype)
    LO[:, :nv], HI[:, :nv] = ctl.lo, ctl.hi
    DB = np.zeros((R, nt))
    g = gt.copy()
    g[:, nv:] = 0
    dg = np.array(dgt, dtype=np.float64)
    dg[:, nv:] = 0.0
    for r_ in range(ny):
        cc = int(ctl.ycomp[r_])
        if fault == "xref_wrong_comp" and cc >= 0:
            cc = (cc + 1) % c.d
        sh = xref[:, cc] if cc >= 0 else 0.0
        for B_, bnd in ((LO, ctl.ylo[r_]), (HI, ctl.yhi[r_])):
            b64 = bnd - sh  # float64: bit-determined
            t_r = gt[:, nv + r_]
            B_[:, nv + r_] = cast(b64) + t_r if fault == "bound_plus_t" else cast(b64) - t_r
            fin = np.isfinite(b64) & np.ones(R, dtype=bool)
            DB[:, nv + r_] = np.maximum(DB[:, nv + r_], np.where(fin, dgt[:, nv + r_] + U64 * ab(np.where(fin, B_[:, nv + r_], 0), dgt[:, nv + r_]), 0.0))
    DLO, DHI = np.full((R, nt), -INF), np.full((R, nt), INF)
    DLO[:, :nv], DHI[:, :nv] = ctl.dlo, ctl.dhi
    DLO[:, :p] = uprev + ctl.dlo[:p]
    DHI[:, :p] = uprev + ctl.dhi[:p]
    DLO, DHI = cast(DLO), cast(DHI)

    def product(K, x, terms):
        if not emul:
            return x @ K.T
        out = np.zeros((R, K.shape[0]))
        for j in range(terms):
            out = K[:, j] * x[:, j:j + 1] + out
        return out

    def rate_slot(s, ds):
        s2, d2 = s.copy(), ds.copy()
        s2[:, p:nv] = s[:, p:nv] - s[:, :nv - p]
        hi_ = nv  # lanes from hi_ on keep zeros in the rate slot: the output lanes
        if fault == "out_rate_slot":  # the `var ? ds : 0.0` of rate_slot dropped: an output lane is differenced p lanes down too
            s2[:, nv:] = s[:, nv:] - s[:, nv - p:nt - p]
            hi_ = nt
        if fault == "up_lane_p_plain" and nv > p:
            s2[:, p] = s[:, p]
        if fault == "up_lane_pm1_diff":
            s2[:, p - 1] = s[:, p - 1] - s[:, 0]
        d2[:, p:nv] = ds[:, p:nv] + ds[:, :nv - p]
        d2[:, p:nv] += U64 * ab(s2[:, p:nv], d2[:, p:nv])
        s2[:, hi_:] = 0
        d2[:, nv:] = 0.0
        return s2, d2

    def prox(v, dv):
        c1 = _clip(v, LO, HI)
        z = np.where(soft, c1 + THd * (v - c1), c1)
        sig = np.where(soft, gamma(2) * TH * ab(v - c1, 2 * dv) + U64 * ab(z, dv), 0.0)  # the soft form's own roundings
        return z, np.maximum(dv, DB) + sig, sig

    def residual(e1, de1, e2, de2):
        both, dboth = np.maximum(np.abs(e1), np.abs(e2)), np.maximum(de1, de2)
        if fault == "max_half":
            both, dboth = both[:, :32], dboth[:, :32]
        return np.max(both, axis=1), np.max(dboth, axis=1), np.maximum(np.abs(e1), np.abs(e2))

    # the start: s = -S0 g
    s_chain = S0
    if fault == "s0_untransposed":  # word lane nv + j of the buffer S0t (nv x nt), as if it were stored nt x nv
        s_chain = np.ascontiguousarray(S0.T).reshape(-1)[:nt * nv].reshape(nt, nv)
    s1 = -product(s_chain, g[:, :nv], nv)
    ds1 = ab(g[:, :nv], dg[:, :nv]) @ dS0.T + dg[:, :nv] @ aS0.T + gamma(nv) * (ab(g[:, :nv], dg[:, :nv]) @ aS0.T)
    s2, ds2 = rate_slot(s1, ds1)
    z1, dz1, sig = prox(s1, ds1)
    z2, dz2 = _clip(s2, DLO, DHI), ds2
    l1, l2 = np.zeros((R, nt), dtype=dtype), np.zeros((R, nt), dtype=dtype)
    if l2_init is not None:
        l2 = cast(l2_init)
    dl1, dl2 = np.zeros((R, nt)), np.zeros((R, nt))
    e1, e2 = s1 - z1, s2 - z2
    de1 = ds1 + DB + sig + U64 * ab(e1, ds1 + DB)  # (s - z = N(v) at the start: 1-Lipschitz in v and in the bound)
    de2 = ds2 + U64 * ab(e2, ds2)
    r, dr, elane = residual(e1, de1, e2, de2)
    margin = np.where(dr > 0, r.astype(np.float64) / np.where(dr > 0, dr, 1.0), INF)
    far = ds1 + DB
    inside = np.all((s1 - LO > far) & (HI - s1 > far) & (s2 - DLO > ds2) & (DHI - s2 > ds2), axis=1)
    tol_ = dtype(tol)

    def goes_on(r_, it_):
        return ~((r_ <= tol_) & ((it_ == 0) | (tol > 0.0)))

    amb = (np.abs(r - tol_).astype(np.float64) <= dr) & ~(inside if tol == 0.0 else False)
    it = np.zeros(R, dtype=np.int64)
    per_lane = fault == "stop_per_lane"
    act = (goes_on(elane, 0) if per_lane else np.repeat(goes_on(r, it)[:, None], nt, axis=1)) & (iters > 0)
    vis, growth = np.zeros(nt), []
    for k in range(int(iters)):
        if not act.any():
            break
        w2 = z2 - l2
        dw2 = dz2 + dl2 + U64 * ab(w2, dz2 + dl2)
        dtv, ddt = w2.copy(), dw2.copy()
        dtv[:, :nv - p] = w2[:, :nv - p] - w2[:, p:nv]
        ddt[:, :nv - p] = dw2[:, :nv - p] + dw2[:, p:nv]
        ddt[:, :nv - p] += U64 * ab(dtv[:, :nv - p], ddt[:, :nv - p])
        if fault == "dt_lt_nv_m1" and nv > p:
            dtv[:, nv - p - 1] = w2[:, nv - p - 1]
        if fault == "dt_le_nv":  # lane nv - p differenced against what lane nv holds (no row: w2 = -s1 of lane nv - p)
            dtv[:, nv - p] = w2[:, nv - p] + s1[:, nv - p] if nv < 64 else 0.0
        a_ = z1 - l1
        da = dz1 + dl1 + U64 * ab(a_, dz1 + dl1)
        b_ = a_ + dtv
        db_ = np.where(var, da + ddt + U64 * ab(b_, da + ddt), da)
        rb = rho * b_
        if fault == "no_rho_out_q":
            rb = np.where(var, rb, b_)
        rhs = rb - g
        drhs = float(A.rho) * db_ + dg + U64 * ab(rb, float(A.rho) * db_) + np.where(var, U64 * ab(rhs, float(A.rho) * db_ + dg), 0.0)
        terms = nt if fault != "krow_truncated" else (16 if nt <= 32 else 32)
        s1n = product(Kb, rhs, terms)
        ds1n = ab(rhs, drhs) @ dKb.T + drhs @ aKb.T + gamma(nt) * (ab(rhs, drhs) @ aKb.T)
        s2n, ds2n = rate_slot(s1n, ds1n)
        v1 = s1n + l1
        dv1 = ds1n + dl1 + U64 * ab(v1, ds1n + dl1)
        z1n, dz1n, sig = prox(v1, dv1)
        v2 = s2n + l2
        dv2 = ds2n + dl2 + U64 * ab(v2, ds2n + dl2)
        z2n, dz2n = _clip(v2, DLO, DHI), dv2
        e1, e2 = s1n - z1n, s2n - z2n
        if fault == "dual_sign":
            l1n, l2n = l1 + (z1n - s1n), l2 + (z2n - s2n)
        else:
            l1n, l2n = l1 + e1, l2 + e2
        de1, de2 = ds1n + dz1n + U64 * ab(e1, ds1n + dz1n), ds2n + dz2n + U64 * ab(e2, ds2n + dz2n)
        dl1n = dv1 + DB + sig + U64 * ab(e1, ds1n + dz1n) + U64 * ab(l1n, dv1 + DB)
        dl2n = dv2 + U64 * ab(e2, ds2n + dz2n) + U64 * ab(l2n, dv2)
        rn, drn, elane = residual(e1, de1, e2, de2)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.max(ab(Kb[:p])[None, :, :] * ab(rhs)[:, None, :] / dz1n[:, :p, None], axis=1)
        rows_on = act.any(axis=1)
        if rows_on.any():
            vis = np.maximum(vis, np.max(np.where(np.isfinite(share[rows_on]), share[rows_on], 0.0), axis=0))
            growth.append(float(np.max(dz1n[rows_on][:, :p])))
        s1, ds1, s2, ds2 = np.where(act, s1n, s1), np.where(act, ds1n, ds1), np.where(act, s2n, s2), np.where(act, ds2n, ds2)
        z1, dz1, z2, dz2 = np.where(act, z1n, z1), np.where(act, dz1n, dz1), np.where(act, z2n, z2), np.where(act, dz2n, dz2)
        l1, dl1, l2, dl2 = np.where(act, l1n, l1), np.where(act, dl1n, dl1), np.where(act, l2n, l2), np.where(act, dl2n, dl2)
        r, dr = np.where(rows_on, rn, r), np.where(rows_on, drn, dr)
        it = it + rows_on
        if k + 1 < iters and tol > 0.0:
            amb = amb | (rows_on & (np.abs(rn - tol_).astype(np.float64) <= drn))
        act = act & (goes_on(elane, 1) if per_lane else goes_on(rn, it)[:, None])
    if fault == "rate_before_box":
        u = _clip(_clip(z1[:, :p], DLO[:, :p], DHI[:, :p]), LO[:, :p], HI[:, :p])
    else:
        u = _clip(_clip(z1[:, :p], LO[:, :p], HI[:, :p]), DLO[:, :p], DHI[:, :p])
    return dict(u=u, du=dz1[:, :p], it=it, r=r, dr=dr, amb=amb, margin=margin, vis=vis, growth=growth, l2=l2)


# ---------------------------------------------------------------------------------------------------------------------
# the cases and their designed problems
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "section plant fam d p N ny m soft")
Run = collections.namedtuple("Run", "tag regime limits rho iters tol")  # rho: "default" / "small"; tol: 0.0 or "median5"
PLANT_OF_P = {1: ("duffing", 2), 2: ("P2", 2), 3: ("P23", 2), 4: ("P4b", 4)}
# section A: (nv, p, N) -> plant override (the padded-D classes: d = 1 (hjb), d = 3 (P3), d = 4 (P4, P4b))
A_SHAPES = [(1, 1), (2, 1), (3, 1), (4, 1), (3, 5), (1, 16), (4, 4), (1, 17), (1, 31), (2, 16), (3, 11), (3, 21), (1, 64), (2, 32),
            (4, 16)]
A_PLANT = {(1, 1): ("hjb", 1), (1, 17): ("P3", 3), (2, 16): ("P4", 4)}
B_SHAPES = [(1, 1, 1), (12, 4, 1), (13, 4, 1), (28, 4, 2), (30, 3, 3), (48, 16, 4), (63, 1, 3), (1, 63, 1)]  # (nv, ny, p)
M_LADDER = (1, 63, 64, 128, 129)  # beside 65 and nk_mpc_loop_max_m
ONE_SIDED = {(4, 4): "lo_only", (2, 16): "no_rate", (1, 64): "no_box"}  # one shape per NP class


def _a_cases():
    out = []
    for p, N in A_SHAPES:
        plant, d = A_PLANT.get((p, N), PLANT_OF_P[p])
        out.append(Case("A", plant, "matern", d, p, N, 0, 65, False))
    for p, N in ((1, 16), (4, 16)):
        plant, d = PLANT_OF_P[p]
        out += [Case("A", plant, "matern", d, p, N, 0, m, False) for m in M_LADDER + (P.mpc_loop_max_m(p * N),)]
    out += [Case("A", "duffing", fam, 2, 1, 17, 0, 65, False) for fam in ("rbf", "linear", "spline")]  # (matern: P3 above)
    return out


def _b_cases():
    out = []
    for nv, ny, p in B_SHAPES:
        plant, d = PLANT_OF_P[p]
        for m in (65, P.mpc_loop_max_m(nv + ny)):
            out += [Case("B", plant, "matern", d, p, nv // p, ny, m, soft) for soft in (False, True)]
    return out


A_CASES, B_CASES = _a_cases(), _b_cases()
ALL_CASES = A_CASES + B_CASES


def name(c):
    return f"{c.section}-{c.plant}-{c.fam}-p{c.p}N{c.N}" + (f"ny{c.ny}{'soft' if c.soft else 'hard'}" if c.ny else "") + f"-m{c.m}"


def full_ladder(c):
    return c.m == 65 and c.fam == "matern"


def runs_of(c):
    """The runs of a case: the regimes and the iteration ladder at m = 65; the active regime at 3 and 30 iterations elsewhere."""
    out = [Run("it3", "active", "all", "default", 3, 0.0), Run("it30", "active", "all", "small", 30, 0.0)]
    if full_ladder(c):
        out += [Run("it1", "active", "all", "default", 1, 0.0), Run("it2", "active", "all", "default", 2, 0.0),
                Run("inactive", "inactive", "all", "default", 3, 0.0), Run("early", "active", "all", "small", 30, "median5")]
        if c.section == "A" and (c.p, c.N) in ONE_SIDED:
            out.append(Run(ONE_SIDED[(c.p, c.N)], "active", ONE_SIDED[(c.p, c.N)], "default", 3, 0.0))
    return out


def case_seed(c):
    return [c.p, c.N, c.ny, c.m, c.d, int(c.soft), list(P.FAMILIES).index(c.fam)]


# The active regime asks for r_0 > 0 at every step of every trajectory.  With one or two lanes, or one landmark, a start
# whose |H^-1 g| is small or changes sign on the way settles inside its limits for a step, so the starts and [F; T] of these
# cases are the first draw (seed offset) for which the float64 emulation's closed loops stay active at every step of every
# run; tests/test_mpc_qp_reference_host.py asserts the condition for every case, the GPU test again on the device's states.
DESIGN_DRAW = {"A-hjb-matern-p1N1-m65": 9, "A-P2-matern-p2N1-m65": 1, "A-P4b-matern-p4N16-m1": 1}


@functools.lru_cache(maxsize=None)
def _design(c, draw=0):
    """What does not depend on S^-1: H, G, ycomp, the starts, the sign pattern of u_init."""
    nv = c.p * c.N
    rng = np.random.default_rng(case_seed(c) + [3])
    Gm = rng.standard_normal((nv, nv))
    H = np.eye(nv) + Gm @ Gm.T / nv
    H = (H + H.T) / 2
    G = rng.standard_normal((c.ny, nv)) / np.sqrt(nv)
    ycomp = np.array([(-1 if r % 2 == 0 else (r // 2) % c.d) for r in range(c.ny)], dtype=np.int32)
    if c.ny == 1:
        ycomp[:] = c.d - 1  # a single row: with a component
    x0, xref = P.starts(c.d, sum(case_seed(c)) + draw)
    usign = rng.choice([-1.0, 1.0], (BATCH, c.p))
    usign[1::2] = 0.0  # half the batch starts from u_init = 0
    return H, G, ycomp, x0, xref, usign


def problem(c, Sinv, draw=None):
    """The designed problem of case c (draw: DESIGN_DRAW's unless given) around the S^-1 handed in: a namespace with spec, FT ([F; T], nt x m), w, Fbar, w64, H, G,
    ycomp, x0, xref, u_init, waves, cc, scale (the median start |H^-1 g|), yscale, and controller(run) / matrices(run)."""
    nv, nt = c.p * c.N, c.p * c.N + c.ny
    spec = P.model_spec(c.fam, c.d, c.m)
    draw = DESIGN_DRAW.get(name(c), 0) if draw is None else draw
    H, G, ycomp, x0, xref, usign = _design(c, draw)
    cc = P.mpc_reduction_c(c.m)
    FT = P.design_gain(spec, nt, Sinv, seed=sum(case_seed(c)) + 7919 * draw)
    w, Fbar = P.fold_ld(spec, FT, Sinv)
    ref0 = P.control_reference(spec, w, Fbar, x0[:, None, :], xref, cc)
    gt0 = -ref0["u"][:, 0].astype(np.float64)
    U0 = -(gt0[:, :nv] @ np.linalg.inv(H).T)
    scale = float(np.median(np.abs(U0)))
    yscale = float(np.median(np.abs(U0 @ G.T + gt0[:, nv:]))) if c.ny else 0.0
    q = types.SimpleNamespace(c=c, spec=spec, FT=FT, w=w, Fbar=Fbar, w64=P.fold64(spec, FT, Sinv), H=H, G=G, ycomp=ycomp, x0=x0,
                              xref=xref, u_init=usign * (0.3 + 0.2) * scale, waves=P.mpc_class(c.m, nt)[1], cc=cc, scale=scale,
                              yscale=yscale, draw=draw, gt0=gt0, dgt0=ref0["bar"][:, 0], rhos={"default": default_rho(H), "small": small_rho(H, G)})
    q.cache = {}
    return q


def controller(q, run):
    """The controller of a run as closed_loop_plant_mpc reads it (K is never used: iters >= 1)."""
    c = q.c
    nv = c.p * c.N
    box, rate = 0.3 * q.scale, 0.1 * q.scale
    if run.regime == "inactive":
        box, rate = 1e6, INF
    lo, hi, dlo, dhi = (np.full(nv, v) for v in (-box, box, -rate, rate))
    if run.limits == "lo_only":
        hi[:] = INF
        dhi[:] = INF
    if run.limits == "no_rate":
        dlo[:], dhi[:] = -INF, INF
    if run.limits == "no_box":
        lo[:], hi[:] = -INF, INF
    rho = q.rhos[run.rho]
    ctl = types.SimpleNamespace(K=np.zeros((c.p, c.m)), F=np.ascontiguousarray(q.FT[:nv]), H=q.H, horizon=c.N, lo=lo, hi=hi, dlo=dlo,
                                dhi=dhi, rho=rho, theta=0.0, ylo=np.zeros(0), yhi=np.zeros(0))
    if c.ny:
        yb = 1e6 if run.regime == "inactive" else 0.3 * q.yscale
        ctl.G, ctl.T = q.G, np.ascontiguousarray(q.FT[nv:])
        ctl.ylo, ctl.yhi, ctl.ycomp, ctl.ny = np.full(c.ny, -yb), np.full(c.ny, yb), q.ycomp, c.ny
        ctl.y_weight = 3.0 * rho if c.soft else INF
        ctl.theta = 0.0 if np.isinf(ctl.y_weight) else float(rho / (rho + ctl.y_weight))  # mpc_out_theta, nk_mpc_out.h:105
    return ctl


def matrices(q, run, fault=None, emul=False):
    key = (run.rho, fault if fault in MATRIX_FAULTS else None, emul)
    if key not in q.cache:
        rho = q.rhos[run.rho]
        q.cache[key] = matrices64(q.H, q.G, rho, q.c.p, key[1]) if emul else matrices_ld(q.H, q.G, rho, q.c.p)
    return q.cache[key]


def run_tol(q, run):
    """tol of a run: 0, or the reference's median r at iteration 5 over the 16 starts at step 0 (fixed by the design)."""
    if run.tol != "median5":
        return float(run.tol)
    if ("tol", run.rho) not in q.cache:
        ctl = controller(q, run)
        out = qp_core(q.c, ctl, matrices(q, run), q.gt0.astype(LD), q.dgt0, q.u_init, q.xref, 5, 0.0, LD)
        q.cache[("tol", run.rho)] = float(np.median(out["r"].astype(np.float64)))
    return q.cache[("tol", run.rho)]


def uprev_of(q, U, fault=None):
    """(B, T, p): the control applied before each step, from the stored controls."""
    up = np.concatenate([q.u_init[:, None, :], U[:, :-1]], axis=1)
    if fault == "uprev_t2":
        up = np.concatenate([q.u_init[:, None, :], q.u_init[:, None, :], U[:, :-2]], axis=1)
    return up


def reference(q, run, X, U):
    """The open-loop reference of a run on the stored states X (B, T + 1, d) and controls U (B, T, p): dict of u (B, T, p)
    longdouble, du, it (B, T), r, dr, amb, margin, vis (nt,), growth, share (landmarks through g)."""
    B, T = U.shape[:2]
    gref = P.control_reference(q.spec, q.w, q.Fbar, X[:, :-1], q.xref, q.cc)
    gt = (-gref["u"]).reshape(B * T, -1)
    out = qp_core(q.c, controller(q, run), matrices(q, run), gt, gref["bar"].reshape(B * T, -1), uprev_of(q, U).reshape(B * T, -1),
                  np.repeat(q.xref, T, axis=0), run.iters, run_tol(q, run), LD)
    out = {k: (v.reshape((B, T) + v.shape[1:]) if isinstance(v, np.ndarray) and v.shape[:1] == (B * T,) else v) for k, v in out.items()}
    out["share"] = gref["share"]
    return out


def emulate(q, run, X, U, fault=None):
    """The float64 emulation of the same steps: dict of u (B, T, p), it, r.  l2_not_reset walks the steps in order."""
    B, T = U.shape[:2]
    ctl, A = controller(q, run), matrices(q, run, fault, emul=True)
    gt = -P.emulate(q.spec, q.w64, X[:, :-1], q.xref, 1, q.waves, mpc=True)
    up = uprev_of(q, U, fault)
    z = np.zeros(gt.shape)
    if fault == "l2_not_reset":
        l2, parts = None, []
        for t in range(T):
            o = qp_core(q.c, ctl, A, gt[:, t], z[:, t], up[:, t], q.xref, run.iters, run_tol(q, run), np.float64, fault, l2)
            l2 = o["l2"]
            parts.append(o)
        return {k: np.stack([o[k] for o in parts], axis=1) for k in ("u", "it", "r")}
    o = qp_core(q.c, ctl, A, gt.reshape(B * T, -1), z.reshape(B * T, -1), up.reshape(B * T, -1), np.repeat(q.xref, T, axis=0),
                run.iters, run_tol(q, run), np.float64, fault)
    return {k: o[k].reshape((B, T) + o[k].shape[1:]) for k in ("u", "it", "r")}


def emulate_step(q, run, x, uprev):
    """One closed-loop step of the emulation on the states x (B, d): u (B, p), info (B, 2)."""
    gt = -P.emulate(q.spec, q.w64, x[:, None, :], q.xref, 1, q.waves, mpc=True)[:, 0]
    o = qp_core(q.c, controller(q, run), matrices(q, run, emul=True), gt, np.zeros(gt.shape), uprev, q.xref, run.iters,
                run_tol(q, run), np.float64)
    return o["u"], np.stack([o["it"].astype(np.float64), o["r"]], axis=1)


def compare(ref, U, info):
    """Worst err / bar of the controls and of the residual over the steps that are not ambiguous, the count of ambiguous
    steps, and whether every unambiguous step has the reference's iteration count."""
    keep = ~ref["amb"]
    ru, at_u = P.worst(np.where(keep[..., None], U, 0.0), np.where(keep[..., None], ref["u"], 0.0), ref["du"])
    rr, at_r = P.worst(np.where(keep, info[..., 1], 0.0), np.where(keep, ref["r"], 0.0), ref["dr"])
    same_it = bool(np.all((info[..., 0] == ref["it"]) | ~keep))
    return dict(u=ru, at_u=at_u, r=rr, at_r=at_r, n_amb=int(np.sum(~keep)), same_it=same_it)
