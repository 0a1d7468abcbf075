"""Extended-precision reference for the tail of a Nystrom fit, from GIVEN Gram accumulators to the operators A, B, C, W
(nk_nystrom_solve / KoopmanNystromRegressor.fit_from_gram: assemble_and_factor, sqrt_products, operator_products and the
optional refinement of csrc/nk_fit.hip):

    inner     = G1 + gamma n blkdiag(K_in + jitter I, I_p)          V = G2 inner^-1
    inner_rec = G3 + gamma n (K_mm + jitter I)                      Y = G4 inner_rec^-1
    A = S^-1 V[:, :m] (K_xo S^-1)    B = S^-1 V[:, m:]    C = Y S    W = C [A B]          S = (K_mm + jitter I)^(1/2)

tail_ld forms this in NumPy longdouble (the solves: an fp64 factor and longdouble residuals), tail_f64 is the comparison solver
in float64 NumPy / LAPACK with the device's shortcut K_xo S^-1 = S - jitter S^-1 and with switches that plant the faults the
GPU test has to be able to see.  The accumulators are gram_reference's, rounded to fp64 once: the reference, the comparison
solver and the device start from the same bits, so the Gram stage is no part of what is measured.  The bars are measured on
tail_f64 against tail_ld (bars), the caps are derived (caps).  NumPy only; nothing here touches the GPU."""
import functools
import math
import types

import numpy as np
import scipy.linalg as sla

import gram_reference as R
from chol_reference import EPS, HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP, N_PERM  # noqa: F401  (re-exported for the tests)
from gram_reference import LINEAR, MATERN, RBF
from sqrtm_reference import _fro, _mm, sqrt_ld

MARGIN = 4.0        # the products sum in MFMA k order, not NumPy's: the project's margin where the summation differs
N_SIGN_DRAWS = 4    # sign draws of the kernel term
JITTER = 1e-6       # KoopmanNystromRegressor.jitter


# ---------------------------------------------------------------------------------------------------------------------
# cases: name -> n_total, d, m, p, kernel family, anisotropic, separate input landmarks, gamma, ls (the length scale is
# ls sqrt(d); anisotropic: spread over a factor 4 across the coordinates).  gamma and ls: the operators must stay sensitive to
# the regulariser and the jitter (a fault in gamma n or a dropped jitter has to show 100 x above the bar), so gamma n K must
# matter beside G and K_mm must have small eigenvalues for the jitter to act on, while cond(inner) stays at 1e2 .. 1e5:
# gamma = 0.1 and kernels half a data spread wide (the host test checks the 100 x on every case).
# ---------------------------------------------------------------------------------------------------------------------
def _c(n, d, m, p, family=RBF, aniso=False, sep=False, gamma=1e-1, ls=0.5):
    return types.SimpleNamespace(n=n, d=d, m=m, p=p, family=family, aniso=aniso, sep=sep, gamma=gamma, ls=ls, jitter=JITTER)


CASES = {
    "n50_d1_m5_p0_rbf": _c(50, 1, 5, 0, ls=0.1),                                   # p = 0: no B, no add_diag; m + p odd
    "n400_d3_m64_p1_matern": _c(400, 3, 64, 1, MATERN),                            # one Cholesky block; G3 at the padded offset
    "n400_d5_m33_p2_rbf": _c(400, 5, 33, 2),                                       # odd m, odd m + p, odd d
    "n2100_d7_m65_p6_aniso_sep": _c(2100, 7, 65, 6, RBF, True, True, ls=0.9),      # the real K_xo S^-1 product, second landmark pair
    "n300_d50_m20_p2_linear": _c(300, 50, 20, 2, LINEAR),                          # d > m
    "n900_d40_m130_p3_matern": _c(900, 40, 130, 3, MATERN, ls=0.9),
    "n900_d4_m257_p2_rbf": _c(900, 4, 257, 2, ls=0.2),                             # both factorisations take the dataflow launch
    # the refinement's systems: the two shapes above with smoother kernels (longer length scales) and gamma lowered until
    # cond(inner) is in REFINE_COND -- and cond(inner_rec) as well: both systems are refined, and right_divide_ld resolves a
    # solution to cond x 1e-19 only (test_fit_tail_reference_host.py checks the range)
    # (m = 65: on the MI355X the unrefined solve of inner_rec's d = 7 right-hand sides sits at the floor left by the rounding of
    # the assembled fp64 system on every one of fifteen systems in the range, ls 2 .. 6 and gamma 1e-4 .. 1e-2: refined C is
    # 0.98 .. 1.08 x nearer tail_ld.  This one is among those where every block is strictly nearer, and its refined C and last
    # row of C are 2.7 x and 8.5 x nearer the fp64 system's own solution, where that floor does not enter.)
    "refine_n2100_d7_m65_p6_aniso_sep": _c(2100, 7, 65, 6, RBF, True, True, gamma=1e-3, ls=5.0),
    "refine_n900_d40_m130_p3_matern": _c(900, 40, 130, 3, MATERN, gamma=1e-6, ls=3.0),
}
DEFAULT_CASES = tuple(k for k in CASES if not k.startswith("refine_"))
# the three smallest by the order of the systems (m = 5, 20, 33), the one-block m = 64 and (900, 40, 130, 3); the linear case
# sends more right-hand sides than unknowns (d = 50 > m = 20) through the pseudo-inverse and the second pass of the products
SVD_CASES = ("n50_d1_m5_p0_rbf", "n300_d50_m20_p2_linear", "n400_d5_m33_p2_rbf", "n400_d3_m64_p1_matern",
             "n900_d40_m130_p3_matern")
FLOW_CASE = "n900_d4_m257_p2_rbf"
LOCKSTEP_CASE = "n400_d5_m33_p2_rbf"
REFINE_CASES = ("refine_n2100_d7_m65_p6_aniso_sep", "refine_n900_d40_m130_p3_matern")
REFINE_SMALL = "n50_d1_m5_p0_rbf"   # well conditioned: the refinement must leave it where it is
REFINE_COND = (1e9, 1e11)


def variant(name, gamma=None, n_total=None):
    """The case `name` with another gamma and / or another n_total handed to the tail (the accumulator stays the case's)."""
    c = CASES[name]
    return (name, c.gamma if gamma is None else gamma, c.n if n_total is None else n_total)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_spec(c):
    if c.family == LINEAR:
        return (LINEAR, 0.7)
    if c.aniso:  # length scales spread over a factor 4 across the coordinates
        return (c.family, tuple(c.ls * math.sqrt(c.d) * np.geomspace(0.5, 2.0, c.d)))
    return (c.family, (c.ls * math.sqrt(c.d),))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Everything the tail of case `name` starts from, as fp64 arrays the reference and the device share: the data and
    landmarks (a seeded synthetic system as gram_reference.problem draws them, with p inputs), G = {G1..G4} = gram_ld rounded to
    fp64, its packed form, K_mm / K_in / K_xo = kernel_ld rounded to fp64 and their entry-wise bars kblock_bar_direct (what the
    device's own landmark matrices may differ by).  Read-only."""
    c = CASES[name]
    n, d, m, p = c.n, c.d, c.m, c.p
    pool = max(n, m)
    rng = np.random.default_rng(104729 * d + 31 * pool + m)
    St = rng.standard_normal((pool, d))
    U = rng.standard_normal((pool, max(p, 1)))
    Y = np.tanh(St @ (rng.standard_normal((d, d)) * 0.9 / math.sqrt(d))) + U @ (rng.standard_normal((max(p, 1), d)) * 0.1)
    Zout = np.ascontiguousarray(Y[rng.permutation(pool)[:m]])
    Zin = np.ascontiguousarray(St[rng.permutation(pool)[:m]]) if c.sep else Zout
    X = np.ascontiguousarray(np.hstack([St[:n], U[:n, :p]]))
    Yn = np.ascontiguousarray(Y[:n])
    kernel = _kernel_spec(c)
    family, par = kernel
    Gl, _ = R.gram_ld(X, Yn, Zin, Zout, p, kernel)
    G = {k: np.ascontiguousarray(v.astype(np.float64)) for k, v in Gl.items()}

    def kmat(A, B):
        k, r2 = R.kernel_ld(A, B, par, family)
        return np.ascontiguousarray(k.astype(np.float64)), R.kblock_bar_direct(A, B, par, family, k=k, r2=r2)

    K_mm, E_mm = kmat(Zout, Zout)
    K_in, E_in = kmat(Zin, Zin) if c.sep else (K_mm, E_mm)
    K_xo, E_xo = kmat(Zin, Zout) if c.sep else (K_mm, E_mm)
    packed = R.pack(G["G1"], G["G2"], G["G3"], G["G4"])
    out = types.SimpleNamespace(name=name, case=c, n=n, d=d, m=m, p=p, sep=c.sep, kernel=kernel, X=X, Y=Yn, Zin=Zin, Zout=Zout,
                                G=G, packed=packed, K_mm=K_mm, K_in=K_in, K_xo=K_xo, E_mm=E_mm, E_in=E_in, E_xo=E_xo)
    for a in (X, Yn, Zin, Zout, packed, K_mm, K_in, K_xo, E_mm, E_in, E_xo, *G.values()):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the longdouble tail
# ---------------------------------------------------------------------------------------------------------------------
def _blkdiag_reg(K_in_j, p, dtype, pp_regulariser=True):
    m = K_in_j.shape[0]
    out = np.zeros((m + p, m + p), dtype=dtype)
    out[:m, :m] = K_in_j
    if pp_regulariser:
        out[m:, m:] = np.eye(p, dtype=dtype)
    return out


def right_divide_ld(P, Rhs, max_rounds=40):
    """X = Rhs P^-1 for the symmetric positive definite longdouble P: LAPACK's fp64 factor of P rounded to fp64, then
    corrections from residuals formed in longdouble, repeated until the correction stops shrinking (each round contracts the
    error by cond(P) m eps, so this needs cond(P) well below 1e15).  Returns (X, rounds, last accepted |dX| / |X|)."""
    c = sla.cho_factor(np.asarray(P, dtype=np.float64), lower=True, check_finite=False)
    solve = lambda B: sla.cho_solve(c, np.asarray(B, dtype=np.float64).T, check_finite=False).T.astype(LD)
    X = solve(Rhs)
    prev, rounds, last = np.inf, 0, np.inf
    for rounds in range(1, max_rounds + 1):
        dX = solve(Rhs - _mm(X, P))
        nd = float(_fro(dX))
        if not nd < 0.5 * prev:
            break
        X, prev, last = X + dX, nd, nd / float(_fro(X))
        if nd == 0.0:
            break
    return X, rounds, last


def _as_ld(a):
    return np.asarray(a).astype(LD)


def tail_ld(G, K_mm, K_in, K_xo, n_total, gamma, jitter, S=None, Sinv=None):
    """The tail in longdouble.  G: the four accumulators; K_mm (output landmarks), K_in (input landmarks), K_xo (input x output
    landmarks), all without jitter.  S, Sinv: taken as given when passed (the device's own square root: what it differs by from
    the true one is test_gpu_sqrtm.py's business and stays out of the operators' distances), else sqrt_ld of K_mm + jitter I.
    Returns a namespace with A, B, C, W, the solutions V, Y, the systems inner, inner_rec and S, Sinv, all longdouble."""
    G1, G2, G3, G4 = (_as_ld(G[k]) for k in ("G1", "G2", "G3", "G4"))
    m = G3.shape[0]
    p = G1.shape[0] - m
    gn = LD(gamma) * LD(n_total)
    Im = np.eye(m, dtype=LD)
    Kj = _as_ld(K_mm) + LD(jitter) * Im
    inner = G1 + gn * _blkdiag_reg(_as_ld(K_in) + LD(jitter) * Im, p, LD)
    inner_rec = G3 + gn * Kj
    if S is None:
        S, Sinv = sqrt_ld(np.asarray(K_mm, dtype=np.float64) + jitter * np.eye(m))  # the fp64 matrix the device takes the root of
    S, Sinv = _as_ld(S), _as_ld(Sinv)
    V, rounds_v, last_v = right_divide_ld(inner, G2)
    Ysol, rounds_y, last_y = right_divide_ld(inner_rec, G4)
    T = _mm(_as_ld(K_xo), Sinv)
    A = _mm(Sinv, _mm(V[:, :m], T))
    B = _mm(Sinv, V[:, m:])
    C = _mm(Ysol, S)
    W = _mm(C, np.hstack([A, B]))
    return types.SimpleNamespace(A=A, B=B, C=C, W=W, V=V, Y=Ysol, inner=inner, inner_rec=inner_rec, S=S, Sinv=Sinv, T=T, Kj=Kj,
                                 rounds=(rounds_v, rounds_y), last=(last_v, last_y), m=m, p=p)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison solver, float64, with fault switches
# ---------------------------------------------------------------------------------------------------------------------
# fault -> the block it must show on
FAULTS = {
    "n_total_plus_1": "A",
    "no_jitter_in_K_in": "A",
    "no_jitter_in_shortcut": "A",
    "no_regulariser_on_pp_block": "B",
    "V1_transposed": "A",
    "B_one_column_early": "B",
    "C_last_row_zero": "C_last",
    "W_last_column_zero": "W_last",
    "G3_G4_from_unpadded_offset": "C",
    "K_in_in_inner_rec": "C",
    "K_xo_transposed": "A",
}


def faults_of(c):
    """The faults that apply to case c."""
    out = ["n_total_plus_1", "no_jitter_in_K_in", "V1_transposed", "C_last_row_zero", "W_last_column_zero"]
    if not c.sep:
        out.append("no_jitter_in_shortcut")
    if c.p > 0:
        out += ["no_regulariser_on_pp_block", "B_one_column_early"]
    if ((2 * c.m + c.p) * (c.m + c.p)) % 2 == 1:
        out.append("G3_G4_from_unpadded_offset")
    if c.sep:
        out += ["K_in_in_inner_rec", "K_xo_transposed"]
    return out


ASSEMBLIES = 3


def _assemble(Gq, K, gn, jitter, p, how, pp_regulariser=True):
    """Gq + gn blkdiag(K + jitter I, I_p) in fp64, in one of ASSEMBLIES equally valid ways: 0 = the formula as written, 1 = the
    jitter's share added last, 2 = the longdouble sum rounded once (what a fused multiply-add per entry comes close to).  A
    rounding of the assembled system is a backward error the solve carries forward cond-fold, and a relabelling of the
    landmarks does not draw it anew: the ways stand for the draws."""
    m = K.shape[0]
    if how == 0:
        return Gq + gn * _blkdiag_reg(K + jitter * np.eye(m), p, np.float64, pp_regulariser)
    if how == 1:
        return (Gq + gn * _blkdiag_reg(K, p, np.float64, pp_regulariser)) + _blkdiag_reg((gn * jitter) * np.eye(m), p, np.float64, False)
    out = _as_ld(Gq) + LD(gn) * _blkdiag_reg(_as_ld(K) + LD(jitter) * np.eye(m, dtype=LD), p, LD, pp_regulariser)
    return out.astype(np.float64)


def tail_f64(G, K_mm, K_in, K_xo, n_total, gamma, jitter, S, Sinv, shared, lstsq=False, fault=None, solves=None, assembly=0):
    """The same formula in float64 NumPy: LAPACK potrf / potrs for the two systems (numpy.linalg.lstsq, i.e. gelsd, with
    lstsq=True: the SVD route), K_xo S^-1 = S - jitter S^-1 when the landmarks are shared (sqrt_products) and the product
    otherwise.  S, Sinv: fp64, as given.  solves = (V, Y): the two solutions taken as given (the longdouble ones rounded to
    fp64), or solves = "ld": the solutions of THIS function's own fp64 systems by right_divide_ld, rounded to fp64 -- what a
    converged refinement returns.  assembly: see _assemble.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    G1, G2, G3, G4 = (np.asarray(G[k], dtype=np.float64) for k in ("G1", "G2", "G3", "G4"))
    m = G3.shape[0]
    p = G1.shape[0] - m
    d = G4.shape[0]
    if fault == "G3_G4_from_unpadded_offset":
        flat = R.pack(G1, G2, G3, G4)
        bot = flat[(2 * m + p) * (m + p):(2 * m + p) * (m + p) + (m + d) * m].reshape(m + d, m)
        G3, G4 = bot[:m], bot[m:]
    gn = gamma * float(n_total + 1 if fault == "n_total_plus_1" else n_total)
    inner = _assemble(G1, K_in, gn, 0.0 if fault == "no_jitter_in_K_in" else jitter, p, assembly,
                      fault != "no_regulariser_on_pp_block")
    inner_rec = _assemble(G3, K_in if fault == "K_in_in_inner_rec" else K_mm, gn, jitter, 0, assembly)
    if isinstance(solves, str):
        assert solves == "ld", solves
        V = right_divide_ld(_as_ld(inner), _as_ld(G2))[0].astype(np.float64)
        Ysol = right_divide_ld(_as_ld(inner_rec), _as_ld(G4))[0].astype(np.float64)
    elif solves is not None:
        V, Ysol = (np.asarray(s, dtype=np.float64) for s in solves)
    elif fault == "G3_G4_from_unpadded_offset":  # (the shifted "G3" is not symmetric: no Cholesky)
        V = sla.cho_solve(sla.cho_factor(inner, lower=True), G2.T).T
        Ysol = np.linalg.solve(inner_rec.T, G4.T).T
    elif lstsq:
        V = np.linalg.lstsq(inner, G2.T, rcond=None)[0].T
        Ysol = np.linalg.lstsq(inner_rec, G4.T, rcond=None)[0].T
    else:
        V = sla.cho_solve(sla.cho_factor(inner, lower=True), G2.T).T
        Ysol = sla.cho_solve(sla.cho_factor(inner_rec, lower=True), G4.T).T
    if shared:
        T = np.array(S) if fault == "no_jitter_in_shortcut" else S - jitter * Sinv
    else:
        T = (K_xo.T if fault == "K_xo_transposed" else K_xo) @ Sinv
    V1 = V[:, :m].T if fault == "V1_transposed" else V[:, :m]
    V2 = V[:, m - 1:m + p - 1] if fault == "B_one_column_early" else V[:, m:]
    A = Sinv @ (V1 @ T)
    B = Sinv @ V2
    C = Ysol @ S
    if fault == "C_last_row_zero":
        C[-1] = 0.0
    W = C @ np.hstack([A, B])
    if fault == "W_last_column_zero":
        W[:, -1] = 0.0
    return types.SimpleNamespace(A=A, B=B, C=C, W=W, V=V, Y=Ysol, inner=inner, inner_rec=inner_rec, m=m, p=p)


# ---------------------------------------------------------------------------------------------------------------------
# distances, block by block
# ---------------------------------------------------------------------------------------------------------------------
def blocks_of(t):
    """The six graded blocks of a tail's operators (empty ones left out): a small block is measured on its own, so that it
    cannot hide in a large one.  (W_last, the last column of W, is graded by the host test's fault check only.)"""
    m = t.A.shape[0]
    out = {"A": t.A, "C": t.C, "C_last": t.C[-1:], "W_state": t.W[:, :m]}
    if t.B.shape[1]:
        out["B"], out["W_input"] = t.B, t.W[:, m:]
    return out


def distances(got, ref, extra=()):
    """{block: ||got - ref||_F / ||ref||_F}, the differences formed in longdouble."""
    g, r = blocks_of(got), blocks_of(ref)
    if "W_last" in extra:
        g["W_last"], r["W_last"] = got.W[:, -1:], ref.W[:, -1:]
    return {k: float(_fro(_as_ld(g[k]) - _as_ld(r[k])) / _fro(_as_ld(r[k]))) for k in r}


def relabel(v, G, perm_in, perm_out):
    """(G, K_mm, K_in, K_xo) of inputs v with the input landmarks renumbered by perm_in and the output landmarks by perm_out
    (one and the same permutation when they are shared), the accumulators G permuted to match."""
    m, p = v.m, v.p
    cols = np.concatenate([perm_in, m + np.arange(p)])
    Gp = dict(G1=G["G1"][cols][:, cols], G2=G["G2"][perm_out][:, cols], G3=G["G3"][perm_out][:, perm_out],
              G4=G["G4"][:, perm_out])
    return ({k: np.ascontiguousarray(a) for k, a in Gp.items()}, np.ascontiguousarray(v.K_mm[perm_out][:, perm_out]),
            np.ascontiguousarray(v.K_in[perm_in][:, perm_in]), np.ascontiguousarray(v.K_xo[perm_in][:, perm_out]))


def relabelled(t, perm_out):
    """The operators of the relabelled problem from those of the problem itself: A lives in the whitened coordinates of the
    output landmarks (S -> P S P^T), B's rows, C's columns and W's state columns follow them; the inputs keep their place."""
    return types.SimpleNamespace(A=t.A[perm_out][:, perm_out], B=t.B[perm_out], C=t.C[:, perm_out],
                                 W=np.hstack([t.W[:, :t.A.shape[0]][:, perm_out], t.W[:, t.A.shape[0]:]]))


def _perms(v, k, seed=0):
    if k == 0:
        return np.arange(v.m), np.arange(v.m)
    rng = np.random.default_rng(4001 + 17 * seed + k)
    po = rng.permutation(v.m)
    return (rng.permutation(v.m) if v.sep else po), po


# ---------------------------------------------------------------------------------------------------------------------
# references and bars of a case
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrt_f64(name):
    """(S, Sinv) = sqrt_ld(K_mm + jitter I) of the case rounded to fp64: the square root the bars are measured with."""
    v = inputs(name)
    S, Si = sqrt_ld(v.K_mm + v.case.jitter * np.eye(v.m))
    out = np.ascontiguousarray(S.astype(np.float64)), np.ascontiguousarray(Si.astype(np.float64))
    for a in out:
        a.setflags(write=False)
    return out


def reference(key, S=None, Sinv=None):
    """tail_ld of key = variant(...) (a case, the gamma and the n_total handed to the tail) with the square root given, else
    sqrt_f64's."""
    name, gamma, n_total = key
    v = inputs(name)
    if S is None:
        S, Sinv = sqrt_f64(name)
    return tail_ld(v.G, v.K_mm, v.K_in, v.K_xo, n_total, gamma, v.case.jitter, S, Sinv)


@functools.lru_cache(maxsize=None)
def _reference_own(key):
    return reference(key)


def floor_of(m):
    return m * EPS


@functools.lru_cache(maxsize=None)
def measured(key, lstsq=False, converged_solves=False):
    """What the comparison solver itself differs by, on key = variant(...): a namespace with
      spread: {block: worst distance of tail_f64 from tail_ld over the problem and N_PERM relabellings of its landmarks}
      kernel: {block: worst movement of tail_f64 when K_mm, K_in, K_xo move by +- kblock_bar_direct, N_SIGN_DRAWS sign draws}
    both with the square root of sqrt_f64; every labelling is run with each of the ASSEMBLIES ways of assembling the systems (way
    0 is the formula as written: the worst over the ways is at or above the worst of that way alone).  converged_solves: tail_f64's own
    systems solved in longdouble and the solutions rounded to fp64 (the bar of the refined operators: a converged refinement
    returns the system's own solution to working precision)."""
    name, gamma, n_total = key
    v = inputs(name)
    c = v.case
    S, Si = sqrt_f64(name)
    ref = _reference_own(key)
    spread = {}
    for k in range(N_PERM + 1):
        pi, po = _perms(v, k)
        Gp, Kmm, Kin, Kxo = relabel(v, v.G, pi, po)
        Sp, Sip = S[po][:, po], Si[po][:, po]
        ref_k = relabelled(ref, po)
        for how in range(ASSEMBLIES):
            got = tail_f64(Gp, Kmm, Kin, Kxo, n_total, gamma, c.jitter, Sp, Sip, not v.sep, lstsq=lstsq,
                           solves="ld" if converged_solves else None, assembly=how)
            for b, x in distances(got, ref_k).items():
                spread[b] = max(spread.get(b, 0.0), x)
    solves = "ld" if converged_solves else None
    base = tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, n_total, gamma, c.jitter, S, Si, not v.sep, lstsq=lstsq, solves=solves)
    kernel = {}
    rng = np.random.default_rng(9001)
    for _ in range(N_SIGN_DRAWS):
        def moved(K, E, symmetric):
            sg = rng.choice([-1.0, 1.0], size=K.shape)
            if symmetric:
                sg = np.triu(sg) + np.triu(sg, 1).T
            return K + sg * E
        Kmm = moved(v.K_mm, v.E_mm, True)
        Kin = moved(v.K_in, v.E_in, True) if v.sep else Kmm
        Kxo = moved(v.K_xo, v.E_xo, False) if v.sep else Kmm
        got = tail_f64(v.G, Kmm, Kin, Kxo, n_total, gamma, c.jitter, S, Si, not v.sep, lstsq=lstsq, solves=solves)
        for b, x in distances(got, base).items():
            kernel[b] = max(kernel.get(b, 0.0), x)
    return types.SimpleNamespace(spread=spread, kernel=kernel)


@functools.lru_cache(maxsize=None)
def resolution(key):
    """{block: what the reference itself is known to}: the worst distance of tail_ld of the N_PERM relabelled problems from
    the relabelled tail_ld of the problem (exact algebra commutes with the relabelling; the fp64 factor and the summation
    orders inside right_divide_ld do not).  right_divide_ld resolves a solution to cond x 1e-19: at cond 1e10 two distances
    from tail_ld that differ by less than this are not told apart."""
    name, gamma, n_total = key
    v = inputs(name)
    S, Si = sqrt_f64(name)
    ref = _reference_own(key)
    out = {}
    for k in range(1, N_PERM + 1):
        pi, po = _perms(v, k)
        Gp, Kmm, Kin, Kxo = relabel(v, v.G, pi, po)
        again = tail_ld(Gp, Kmm, Kin, Kxo, n_total, gamma, v.case.jitter, S[po][:, po], Si[po][:, po])
        for b, x in distances(again, relabelled(ref, po)).items():
            out[b] = max(out.get(b, 0.0), x)
    return out


def shortcut_term(S, Sinv, Kj):
    """||S^2 - K_j||_F ||S^-1||_F / ||S||_F in longdouble: what S - jitter S^-1 may differ by from the product K_xo S^-1 =
    (K_j - jitter I) S^-1, relative to ||S||, for the S and S^-1 at hand."""
    Sl, Il = _as_ld(S), _as_ld(Sinv)
    return float(_fro(_mm(Sl, Sl) - _as_ld(Kj)) * _fro(Il) / _fro(Sl))


def bars(key, S=None, Sinv=None, lstsq=False, converged_solves=False):
    """{block: bar} = max(m eps, MARGIN x spread) + kernel term + shortcut term (shared landmarks; blocks that hold K_xo S^-1:
    A and W's state columns) for the square root at hand (default: sqrt_f64's)."""
    name = key[0]
    v = inputs(name)
    ms = measured(key, lstsq, converged_solves)
    if S is None:
        S, Sinv = sqrt_f64(name)
    sc = 0.0 if v.sep else shortcut_term(S, Sinv, v.K_mm + v.case.jitter * np.eye(v.m))
    return {b: max(floor_of(v.m), MARGIN * ms.spread[b]) + ms.kernel[b] + (sc if b in ("A", "W_state") else 0.0)
            for b in ms.spread}


def gamma_k(k):
    return k * EPS / (1.0 - k * EPS)


def caps(key):
    """Derived, kept apart from the bars (as chol_reference.caps): the first-order composition of the stage bounds.  A solve
    with a backward-stable factor has forward error cond_2 x order x eps, a product of inner dimension m has error gamma_m times
    the norms of its factors; each operator's cap is the sum over its stages, every term carried to the operator by the norms
    of the factors that follow it, relative to the operator's norm."""
    ref = _reference_own(key)
    m, p = ref.m, ref.p
    f = lambda a: float(_fro(a))
    k1 = float(np.linalg.cond(ref.inner.astype(np.float64))) * (m + p) * EPS
    k2 = float(np.linalg.cond(ref.inner_rec.astype(np.float64))) * m * EPS
    g = gamma_k(m)
    V1, V2 = ref.V[:, :m], ref.V[:, m:]
    amp_a = f(ref.Sinv) * f(V1) * f(ref.T) / f(ref.A)
    out = {"A": (k1 + 3 * g) * amp_a,
           "C": (k2 + g) * f(ref.Y) * f(ref.S) / f(ref.C),
           "C_last": (k2 + g) * f(ref.Y[-1:]) * f(ref.S) / f(ref.C[-1:])}
    if p:
        out["B"] = (k1 + g) * f(ref.Sinv) * f(V2) / f(ref.B)
    out["W_state"] = (out["C"] + out["A"] + g) * f(ref.C) * f(ref.A) / f(ref.W[:, :m])
    if p:
        out["W_input"] = (out["C"] + out["B"] + g) * f(ref.C) * f(ref.B) / f(ref.W[:, m:])
    return out


def refine_emulate(key, steps=2):
    """The device's refinement in NumPy, for the host test: LAPACK's fp64 solve, then `steps` corrections from residuals
    formed in longdouble and rounded to fp64 (the device forms them in doubled precision), with the device's gate (step 0 is
    taken when |dX| <= |X| / 4, a later one when its correction is at most half the one before).  Returns (tail_f64 of the refined
    solutions, accepted steps per system, |dX_0| / |X| per system)."""
    name, gamma, n_total = key
    v = inputs(name)
    S, Si = sqrt_f64(name)
    base = tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, n_total, gamma, v.case.jitter, S, Si, not v.sep)
    sols, accepted, ratio0 = [], [], []
    for P, Rhs, X in ((base.inner, v.G["G2"], base.V), (base.inner_rec, v.G["G4"], base.Y)):
        c = sla.cho_factor(P, lower=True)
        X, alive, prev, acc, r0 = np.array(X), True, 0.0, 0, 0.0
        for step in range(steps):
            res = (_as_ld(Rhs) - _mm(_as_ld(X), _as_ld(P))).astype(np.float64)
            dX = sla.cho_solve(c, res.T).T
            dx2, x2 = float((dX * dX).sum()), float((X * X).sum())
            if step == 0:
                r0 = math.sqrt(dx2 / x2)
            alive = alive and dx2 <= (0.0625 * x2 if step == 0 else 0.25 * prev)
            if alive:
                X, prev, acc = X + dX, dx2, acc + 1
        sols.append(X)
        accepted.append(acc)
        ratio0.append(r0)
    out = tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, n_total, gamma, v.case.jitter, S, Si, not v.sep, solves=tuple(sols))
    return out, accepted, ratio0


def conds(key):
    ref = _reference_own(key)
    return (float(np.linalg.cond(ref.inner.astype(np.float64))), float(np.linalg.cond(ref.inner_rec.astype(np.float64))))


def ratios(got, ref, bar):
    """{block: distance / bar}"""
    return {b: x / bar[b] for b, x in distances(got, ref).items()}
