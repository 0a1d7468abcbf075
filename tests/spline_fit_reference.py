"""Extended-precision reference for the thin-plate-spline EDMD fit (nk_spline_fit / KoopmanSplineRegressor.fit), stage by
stage: the two n x m spline blocks, the three Gram products

    cov = [Phi_x U]^T [Phi_x U]      top = Phi_y^T [Phi_x U]      bot = X_state^T [Phi_x U]

the regularised system P = cov + fl(gamma n_eff) I, M_ls = [top; bot] P^-1 (fit_tail_reference.right_divide_ld), the slices
A | B = M_ls[:m], C = M_ls[m:, :m] and W = C [A B]; entry-wise bars that come from error analysis; and a float64 NumPy emulation
of the fit's own assembly (feature layout, pass loop, pieces, mirror, tiles, solve branch, slicing) with switches that plant the
faults the GPU test has to be able to see.  NumPy / SciPy only; nothing here touches the GPU.

What the GPU test can see.  Only A, B, C, W and the statistics leave a fit.  With fl(gamma n_eff) = gn = 2^100 and |cov| below
2^46, fl(cov_ii + gn) = gn, so P = gn (I + E / gn) with E the off-diagonal part of cov and

    gn M_ls = [top; bot] (I + E / gn)^-1 = [top; bot] - [top; bot] E / gn + O(2^-140):

the operators hand back top and the first m columns of bot, scaled by a power of two, to the first-order term and the
roundings it causes, which readout_bar bounds by 2.02 |[top; bot]| |E| / gn (2^-70 of the scale; it is what stands where an
entry of top is exactly zero; every entry larger than 2^-17 of the scale comes back bit for bit).  With p = n and U = I_n, top[:, m:] = Phi_y^T is a sum with one non-zero term per entry, and
with the first n state coordinates a diagonal of powers of two so is bot[:n, :m] = diag(2^e) Phi_x: the device's own spline
blocks, through the kernels a fit uses.

Bars.  Spline blocks: tps_bar_direct and tps_bar_gram (the two rules tests/test_gpu_spline.py states).  Products: for any
summation order, passes and pieces included, gram_reference.contraction_bar (gamma_(K+2) |F|^T |F|) plus the block bars
propagated to first order with their square (products).  Solve: M = R P^-1 moves by (dR - M dP) P^-1 to first order, so

    |dM| <= (E_R + |M| (E_P + E_solver)) |P^-1|

with E_R, E_P the product bars (and u |P_ii| for the rounding of the added regulariser) and E_solver the backward error of the
solver: Cholesky, |dP| <= gamma_(3 (m+p) + 1) |L| |L|^T <= gamma_(3 (m+p) + 1) sqrt(p_ii p_jj) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., theorem 10.4 and (10.7)); Jacobi pseudo-inverse, ||dP||_F <= pinv_reference.cap_ls(m+p) ||P||_F,
carried to an entry by the 2-norms of the row of M and the column of P^-1.  These are worst-case bounds, so the project's
MARGIN for a summation order that differs from NumPy's has nothing to widen here and is not applied.  W from the fit's own
C and [A B]: gamma_(m+2) |C| |[A B]|."""
import functools
import math
import types

import numpy as np
import scipy.linalg as sla

import gram_reference as R
import pinv_reference as PR
from chol_reference import EPS, HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP  # noqa: F401  (re-exported for the tests)
from fit_tail_reference import right_divide_ld
from gram_reference import U64, contraction_bar, gamma, worst_ratio  # noqa: F401

GN_READOUT = 2.0 ** 100   # fl(gamma n_eff) of the read-out sections
READOUT_ULPS = 0          # ulp the solve leaves on an entry that is a power of two times top: none (readout_bar; the MI355X gives 0)
TILE = R.TILE
PASS_ROWS = 1024          # rows per pass under NYSKOOP_F_BUDGET_GB = BUDGET
BUDGET = "1e-6"
GATHER_BYTES = 256e6      # nk_fit.hip, gather_ranges


# ---------------------------------------------------------------------------------------------------------------------
# the spline block and its two bars
# ---------------------------------------------------------------------------------------------------------------------
def tps_ld(A, Z):
    """(k, r2) in longdouble: r2 by direct differences, coordinate by coordinate; k = r2 log(sqrt(r2)), exactly 0 at r2 = 0."""
    A, Z = np.atleast_2d(np.asarray(A)).astype(LD), np.atleast_2d(np.asarray(Z)).astype(LD)
    r2 = np.zeros((A.shape[0], Z.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        diff = A[:, k][:, None] - Z[:, k][None, :]
        r2 += diff * diff
    safe = np.where(r2 > 0, r2, LD(1))
    return np.where(r2 > 0, r2 * np.log(np.sqrt(safe)), LD(0)), r2


def _f(a):
    return np.asarray(a, dtype=np.float64)


def tps_bar_direct(d, r2, k, u=U64):
    """Direct differences: r^2 carries (d + 8) u r^2 (no cancellation), d(r^2 log r) / d(r^2) = log(r^2) / 2 + 1 / 2, the log
    is good to an ulp: (d + 8) u r2 (|log r2| / 2 + 1) + 8 u |k|.  Zero where r2 is zero."""
    r2 = _f(r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.where(r2 > 0, np.abs(np.log(np.where(r2 > 0, r2, 1.0))), 0.0)
    return (d + 8) * u * r2 * (lg / 2 + 1) + 8 * u * np.abs(_f(k))


def tps_bar_gram(A, Z, mu, r2, k, u=U64):
    """Gram form, r^2 = |a|^2 + |b|^2 - 2 a.b of rows centred on mu: delta = (d + 8) u (|a - mu|^2 + |b - mu|^2), and the spline
    moves by at most delta (|log max(r2, delta)| / 2 + 1), plus 8 u |k|."""
    A, Z = np.atleast_2d(_f(A)), np.atleast_2d(_f(Z))
    na, nb = np.sum((A - mu) ** 2, 1), np.sum((Z - mu) ** 2, 1)
    delta = (A.shape[1] + 8) * u * (na[:, None] + nb[None, :])
    with np.errstate(divide="ignore"):
        lg = np.abs(np.log(np.maximum(_f(r2), delta)))
    lg = np.where(delta > 0, lg, 0.0)
    return delta * (lg / 2 + 1) + 8 * u * np.abs(_f(k))


def tps_f64(A, Z, mu=None):
    """The block in float64 NumPy: direct differences (mu None) or Gram form on rows centred on mu, clamped at 0."""
    A, Z = np.atleast_2d(_f(A)), np.atleast_2d(_f(Z))
    if mu is None:
        r2 = ((A[:, None, :] - Z[None, :, :]) ** 2).sum(axis=2)
    else:
        a, b = A - mu, Z - mu
        r2 = np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0)
    return np.where(r2 > 0, 0.5 * r2 * np.log(np.where(r2 > 0, r2, 1.0)), 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(n, d, m, p, identity=False, diag=False, dup=False, seed=0):
    """X = [state | input] (n x (d + p)) uniform in [-1, 1], Y (n x d) a smooth map of it, centres (m x d): the first half rows
    of Y (row 0 always), the rest rows of the state, so that exact zeros occur in both blocks.  identity: p = n, U = I_n.
    diag: n <= d and the first n state coordinates are diag(2^e) with distinct e.  dup: centre 1 repeats centre 0."""
    rng = np.random.default_rng(15485863 * d + 31 * n + 7 * m + seed)
    S = rng.uniform(-1.0, 1.0, (n, d))
    if diag:
        assert n <= d
        S[:, :n] = np.diag(2.0 ** (np.arange(n) - n // 2))
    if identity:
        assert p == n
        U = np.eye(n)
    else:
        U = rng.uniform(-1.0, 1.0, (n, p))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / math.sqrt(d)))
    if p and not identity:
        Y = Y + U @ (rng.standard_normal((p, d)) * 0.1)
    assert m <= n or n == 1
    my = (m + 1) // 2
    iy = np.concatenate([[0], 1 + rng.permutation(n - 1)[:my - 1]]) if n > 1 else np.zeros(1, dtype=int)
    ix = rng.permutation(n)[:m - my]
    Z = np.vstack([Y[iy[:my]], S[ix]]) if m > my else Y[iy[:my]]
    Z = np.ascontiguousarray(Z[:m])
    if dup:
        Z[1] = Z[0]
    X = np.ascontiguousarray(np.hstack([S, U]))
    Y = np.ascontiguousarray(Y)
    mu = Z.mean(axis=0)
    for a in (X, Y, Z, mu):
        a.setflags(write=False)
    return types.SimpleNamespace(key=(n, d, m, p, identity, diag, dup, seed), n=n, d=d, m=m, p=p, X=X, Y=Y, Z=Z, mu=mu,
                                 identity=identity, diag=diag, dup=dup)


@functools.lru_cache(maxsize=None)
def _blocks(key):
    q = problem(*key)
    return tps_ld(q.X[:, :q.d], q.Z) + tps_ld(q.Y, q.Z)


def blocks(q):
    """(Phi_x, r2_x, Phi_y, r2_y) of problem q in longdouble, cached."""
    return _blocks(q.key)


def block_bars(q, gram_form, rows, direct_pos=()):
    """(E_x, E_y) over the selected rows: the entry-wise bars of the two blocks as the fit builds them.  gram_form: the
    Gram-form rule, except at the positions direct_pos (one-row pieces), which the fit builds by direct differences also in
    that mode."""
    kx, r2x, ky, r2y = (a[rows] for a in blocks(q))
    Dx, Dy = tps_bar_direct(q.d, r2x, kx), tps_bar_direct(q.d, r2y, ky)
    if not gram_form:
        return Dx, Dy
    Gx, Gy = tps_bar_gram(q.X[rows, :q.d], q.Z, q.mu, r2x, kx), tps_bar_gram(q.Y[rows], q.Z, q.mu, r2y, ky)
    if len(direct_pos):
        Gx[direct_pos], Gy[direct_pos] = Dx[direct_pos], Dy[direct_pos]
    return Gx, Gy


# ---------------------------------------------------------------------------------------------------------------------
# the fit's plan: rows, gathering, passes, pieces (nk_fit.hip: select_rows, gather_ranges, pass_rows_for, plan_passes)
# ---------------------------------------------------------------------------------------------------------------------
def plan(n, d, p, row_ranges=None, pass_rows=None):
    """(rows, passes, gathered): the selected row indices in order; passes = lists of (offset into rows, length) pieces; whether
    the ranges are gathered into one piece.  pass_rows None: one pass."""
    rng = [(0, n)] if row_ranges is None else [(b, e) for b, e in row_ranges if e > b]
    rows = np.concatenate([np.arange(b, e) for b, e in rng])
    n_eff = len(rows)
    gathered = len(rng) > 1 and n_eff * (2.0 * d + p) * 8.0 <= GATHER_BYTES
    lens = [n_eff] if gathered else [e - b for b, e in rng]
    pr = n_eff if pass_rows is None else pass_rows
    passes, used, o = [[]], 0, 0
    for ln in lens:
        while ln > 0:
            if used == pr:
                passes.append([])
                used = 0
            take = min(ln, pr - used)
            passes[-1].append((o, take))
            used, o, ln = used + take, o + take, ln - take
    return rows, passes, gathered


def layout(m, p):
    """(off_out, ldf) of the feature rows F = [Phi_x | U | pad | Phi_y]."""
    off_out = (m + p + 1) & ~1
    return off_out, (off_out + m + 1) & ~1


# ---------------------------------------------------------------------------------------------------------------------
# cases of tests/test_gpu_spline_stages.py.  section "A": identity read-out; "B": products at gn = 2^100; "C": the solve at
# gamma; "D": the rank-deficient system.  form: how X, Y reach the fit ("host", "odd_ld", "offset8", "nan_pad").
# ---------------------------------------------------------------------------------------------------------------------
def _case(section, n, d, m, p, mode=0, gamma=None, ranges=None, budget=False, form="host", launches=None, **kw):
    gram_form = mode == 0 and d >= 32 and m >= 2
    rows, passes, gathered = plan(n, d, p, ranges, PASS_ROWS if budget else None)
    fused = m >= 2  # (top has M = m rows of operand columns: one landmark is below the fused engine's two, whatever p is)
    if launches is None:
        launches = len(passes) * (1 if fused else 2)
    return types.SimpleNamespace(section=section, n=n, d=d, m=m, p=p, mode=mode, gamma=gamma, ranges=ranges, budget=budget, form=form,
                                 gram_form=gram_form, launches=launches, n_eff=len(rows), passes=passes, gathered=gathered,
                                 key=(n, d, m, p, kw.get("identity", False), kw.get("diag", False), kw.get("dup", False), 0))


A_SHAPES = list(R.A_SHAPES) + [(5, 1), (300, 1)]
A_DIMS = [(1, 0), (2, 0), (7, 0), (40, 1), (32, 0), (33, 0), (40, 0), (64, 0)]   # (d, kmat mode)


def a_case(n, m, d, mode):
    return _case("A", n, d, m, n, mode, identity=True, diag=n <= d)


BIG = dict(n=15750, d=1024, m=4, p=0, ranges=((0, 7850), (7900, 15750)))  # n_eff = 15 700: 15 700 x 2048 x 8 = 257 MB
B_CASES = {
    # fused three-problem launch, host arrays
    "fused_d40_m130_p6": _case("B", 2100, 40, 130, 6),
    "fused_d7_m20_p1": _case("B", 300, 7, 20, 1),
    "fused_d33_m65_p0": _case("B", 400, 33, 65, 0),
    "fused_d2_m12_p1": _case("B", 400, 2, 12, 1),
    "fused_d40_direct_m20_p6": _case("B", 300, 40, 20, 6, mode=1),
    "fused_d3_m20_p0": _case("B", 300, 3, 20, 0),  # (the shape of the NaN pad-column test)
    # generic engine
    "generic_m1_p0": _case("B", 300, 7, 1, 0),
    # bot apart
    "bot_apart_d1": _case("B", 300, 1, 8, 1),
    "bot_apart_odd_ld": _case("B", 400, 2, 12, 1, form="odd_ld"),
    "bot_apart_odd_ld_d40": _case("B", 2100, 40, 130, 1, form="odd_ld"),
    "bot_apart_offset8": _case("B", 300, 7, 20, 1, form="offset8"),
    # several passes
    "passes_n2100_d2": _case("B", 2100, 2, 12, 1, budget=True),
    "passes_n2100_d2_odd_ld": _case("B", 2100, 2, 12, 1, budget=True, form="odd_ld"),
    "passes_n1025_d40": _case("B", 1025, 40, 65, 1, budget=True),
    "passes_n1025_d40_odd_ld": _case("B", 1025, 40, 65, 1, budget=True, form="odd_ld"),
    "passes_n2048_d7": _case("B", 2048, 7, 20, 2, budget=True),
    "passes_n2048_d7_odd_ld": _case("B", 2048, 7, 20, 2, budget=True, form="odd_ld"),
    # row ranges
    "two_ranges": _case("B", 2100, 40, 65, 2, ranges=((0, 700), (1100, 2100))),
    "two_ranges_and_an_empty_one": _case("B", 2100, 40, 65, 2, ranges=((0, 700), (900, 900), (1100, 2100))),
    "two_ranges_two_passes": _case("B", 2100, 7, 20, 1, ranges=((0, 700), (1100, 2100)), budget=True),
    "two_pieces_past_256MB": _case("B", **BIG),
}
C_SHAPES = [(300, 1, 8, 1), (400, 2, 12, 1), (300, 7, 20, 2), (2100, 2, 65, 1), (2100, 40, 130, 2), (900, 2, 255, 2)]
C_GAMMAS = (1.0, 1e-2)
C_CASES = {f"n{n}_d{d}_m{m}_p{p}_gamma{g:g}": _case("C", n, d, m, p, gamma=g) for n, d, m, p in C_SHAPES for g in C_GAMMAS}
FLOW_CASES = tuple(k for k in C_CASES if k.startswith("n900_d2_m255_p2"))
D_CASE = _case("D", 400, 2, 12, 1, gamma=0.0, dup=True)
CASES = dict(B_CASES, **C_CASES)


def readout_gamma(n_eff):
    """gamma with fl(gamma n_eff) = 2^100 exactly where a neighbour of 2^100 / n_eff gives that (every case but n_eff = 15 700,
    where the products of the three neighbours step over 2^100: there fl(gamma n_eff) is 2^100 (1 + 3.7e-16), see readout_bar)."""
    g = GN_READOUT / n_eff
    for cand in (g, np.nextafter(g, 0.0), np.nextafter(g, np.inf)):
        if float(cand) * float(n_eff) == GN_READOUT:
            return float(cand)
    return float(g)


def gamma_of(c):
    return readout_gamma(c.n_eff) if c.section in ("A", "B") else c.gamma


def gn_of(c):
    """fl(gamma n_eff), the regulariser the fit adds (nk_fit.hip: gamma * (double)n_eff)."""
    return float(gamma_of(c)) * float(c.n_eff)


# ---------------------------------------------------------------------------------------------------------------------
# longdouble products and their bars
# ---------------------------------------------------------------------------------------------------------------------
def _direct_rows(c):
    """Positions (in the selected order) of the rows that sit in one-row pieces."""
    return np.array([o for ps in c.passes for o, ln in ps if ln == 1], dtype=int)


_PRODUCTS = {}


def products(c):
    """({cov, top, bot} longdouble over the selected rows, {cov, top, bot} entry-wise bars: contraction + propagated blocks),
    cached."""
    k = (c.key, c.ranges, c.budget, c.mode)
    if k not in _PRODUCTS:
        q = problem(*c.key)
        rows, _, _ = plan(q.n, q.d, q.p, c.ranges, PASS_ROWS if c.budget else None)
        kx, _, ky, _ = blocks(q)
        kx, ky = kx[rows], ky[rows]
        Xs = q.X[rows, :q.d].astype(LD)
        Fin = np.hstack([kx, q.X[rows, q.d:].astype(LD)])
        ref = dict(cov=R._tn(Fin, Fin), top=R._tn(ky, Fin), bot=R._tn(Xs, Fin))
        aF, aY, aX = np.abs(_f(Fin)), np.abs(_f(ky)), np.abs(_f(Xs))
        scale = dict(cov=aF.T @ aF, top=aY.T @ aF, bot=aX.T @ aF)
        Ex, Ey = block_bars(q, c.gram_form, rows, _direct_rows(c))
        Ein = np.hstack([Ex, np.zeros((len(rows), q.p))])
        prop = dict(cov=Ein.T @ aF + aF.T @ Ein + Ein.T @ Ein, top=Ey.T @ aF + aY.T @ Ein + Ey.T @ Ein, bot=aX.T @ Ein)
        _PRODUCTS[k] = (ref, {w: contraction_bar(len(rows), scale[w]) + prop[w] for w in ref})
    return _PRODUCTS[k]


def readout_bar(c, Rl, cov):
    """What the solve at gn = fl(gamma n_eff) ~ 2^100 may leave between gn M_ls and R = [top; bot]: 2.02 |R| |E| / gn, E the
    off-diagonal part of cov.  Half of it is the first-order term of the exact solution.  The other half is rounding: with
    gn = 2^100 the factor's diagonal is 2^50 exactly, so every scaling of an entry r of R is exact, and a rounding happens only
    where a sum of terms r_j e_jk / gn (2^-70 of the scale) is added to r: it is at most half an ulp of r and at most that sum
    itself.  So no multiple of an ulp is needed (READOUT_ULPS = 0): where the sum is below half an ulp the entry comes back
    bit for bit, which is what the MI355X gives on every entry of the spline blocks read out this way.  Where gn is no power
    of two, three ulp: L_ii = fl(sqrt(gn)) has L_ii^2 = gn (1 + 2 delta), |delta| <= u, and each of the two sweeps then rounds a
    reciprocal and a product that are exact scalings otherwise: 2 u + 4 u = 3 ulp."""
    E = np.abs(_f(cov))
    np.fill_diagonal(E, 0.0)
    gn = gn_of(c)
    assert np.abs(_f(cov)).max() < 2.0 ** 46 and abs(gn / GN_READOUT - 1.0) < 1e-15  # fl(cov_ii + gn) = gn
    ulps = READOUT_ULPS + (0 if gn == GN_READOUT else 3)
    return ulps * EPS * np.abs(_f(Rl)) + 2.02 * (np.abs(_f(Rl)) @ E) / gn


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_of the case CASES[name], cached: the tests of a case share it."""
    return reference_of(CASES[name])


def solve_ld(cov, top, bot, gn):
    """(P, M_ls) in longdouble: P = cov + gn I, M_ls = [top; bot] P^-1 by right_divide_ld, whose residual must be at the
    longdouble level (measured: 6e-20 .. 1e-18 of the right-hand side on the section C systems)."""
    P = np.array(cov, dtype=LD)
    P[np.diag_indices_from(P)] += LD(gn)
    Rhs = np.vstack([top, bot])
    M, _, _ = right_divide_ld(P, Rhs)
    assert float(np.abs(Rhs - R._tn(M.T, P)).max()) <= 1e-17 * float(np.abs(Rhs).max())
    return P, M


def solve_bars(P, M, E_R, E_P, solver):
    """|dM| <= (E_R + |M| (E_P + E_solver)) |P^-1| (module docstring).  solver: "chol" or "svd"."""
    P64, aM = _f(P), np.abs(_f(M))
    mp = P64.shape[0]
    Pinv = np.abs(np.linalg.inv(P64))
    dg = np.sqrt(np.abs(np.diag(P64)))
    E_P = E_P + np.diag(U64 * np.abs(np.diag(P64)))  # the rounding of cov_ii + gn
    bar = (E_R + aM @ E_P) @ Pinv + U64 * aM
    if solver == "chol":
        return bar + (aM @ (gamma(3 * mp + 1) * np.outer(dg, dg))) @ Pinv
    assert solver == "svd", solver
    back = PR.cap_ls(mp) * float(np.linalg.norm(P64))
    return bar + back * np.outer(np.linalg.norm(_f(M), axis=1), np.linalg.norm(np.linalg.inv(P64), axis=0))


def w_bars(AB, C, dAB, dC, m):
    aC, aAB = np.abs(_f(C)), np.abs(_f(AB))
    return dC @ aAB + aC @ dAB + dC @ dAB + gamma(m + 2) * (aC @ aAB)


def reference_of(c):
    """Everything a case is graded against.  Sections A, B: top, botm = bot[:, :m] and their bars (products + read-out).
    Sections C: AB, C, W and their bars for both solvers."""
    q = problem(*c.key)
    ref, bar = products(c)
    m = c.m
    out = types.SimpleNamespace(case=c, q=q, products=ref, product_bars=bar)
    if c.section in ("A", "B"):
        rb = readout_bar(c, np.vstack([ref["top"], ref["bot"]]), ref["cov"])
        out.top, out.botm = ref["top"], ref["bot"][:, :m]
        out.bar_top, out.bar_botm = bar["top"] + rb[:m], (bar["bot"] + rb[m:])[:, :m]
        return out
    gn = gn_of(c)
    P, M = solve_ld(ref["cov"], ref["top"], ref["bot"], gn)
    out.P, out.M, out.AB, out.C = P, M, M[:m], M[m:, :m]
    out.W = out.C @ out.AB
    E_R = np.vstack([bar["top"], bar["bot"]])
    out.bars = {}
    for solver in ("chol", "svd"):
        bM = solve_bars(P, M, E_R, bar["cov"], solver)
        out.bars[solver] = dict(AB=bM[:m], C=bM[m:, :m], W=w_bars(out.AB, out.C, bM[:m], bM[m:, :m], m))
    s = np.linalg.svd(_f(P), compute_uv=False)
    out.cond = float(s[0] / s[-1])
    return out


def grade(ref, AB, C, W, solver="chol"):
    """{quantity: worst err / bar} of a fit's operators (the device's or the emulation's) against reference `ref`."""
    c = ref.case
    AB, C, W = _f(AB), _f(C), _f(W)
    out = {}
    if c.section in ("A", "B"):
        gn = LD(gn_of(c))
        out["top"] = worst_ratio(AB.astype(LD) * gn, ref.top, ref.bar_top)
        out["bot"] = worst_ratio(C.astype(LD) * gn, ref.botm, ref.bar_botm)
    else:
        b = ref.bars[solver]
        out["AB"] = worst_ratio(AB, ref.AB, b["AB"])
        out["C"] = worst_ratio(C, ref.C, b["C"])
        out["W"] = worst_ratio(W, ref.W, b["W"])
    out["W_own"] = worst_ratio(W, C.astype(LD) @ AB.astype(LD), gamma(c.m + 2) * (np.abs(C) @ np.abs(AB)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the rank-deficient system of section D: centre 1 repeats centre 0, gamma = 0
# ---------------------------------------------------------------------------------------------------------------------
def collapse_matrix(mp):
    """T (mp x (mp - 1)): columns 0 and 1 rotated into their normalised sum (kept) and difference (dropped)."""
    T = np.zeros((mp, mp - 1))
    T[0, 0] = T[1, 0] = math.sqrt(0.5)
    T[np.arange(2, mp), np.arange(1, mp - 1)] = 1.0
    return T


@functools.lru_cache(maxsize=None)
def reference_d():
    """The minimum-norm solution of the system whose columns 0 and 1 coincide, from the collapsed (full-rank) system, with
    the solve bars of the pseudo-inverse evaluated on the collapsed system and rotated back."""
    c = D_CASE
    q = problem(*c.key)
    ref, bar = products(c)
    m, mp = c.m, c.m + c.p
    assert np.array_equal(ref["cov"][0], ref["cov"][1]) and np.array_equal(ref["top"][0], ref["top"][1])
    T = collapse_matrix(mp)
    Tl = T.astype(LD)
    Pc = Tl.T @ ref["cov"] @ Tl
    Rc = np.vstack([ref["top"], ref["bot"]]) @ Tl
    Mc, _, _ = right_divide_ld(Pc, Rc)
    M = Mc @ Tl.T
    bMc = solve_bars(Pc, Mc, np.vstack([bar["top"], bar["bot"]]) @ T, T.T @ bar["cov"] @ T, "svd")
    bM = bMc @ T.T
    s = np.linalg.svd(_f(ref["cov"]), compute_uv=False)
    sc = np.linalg.svd(_f(Pc), compute_uv=False)
    out = types.SimpleNamespace(case=c, q=q, AB=M[:m], C=M[m:, :m], M=M, cov=ref["cov"], s=s, cond_collapsed=float(sc[0] / sc[-1]),
                                bars=dict(AB=bM[:m], C=bM[m:, :m]))
    out.W = out.C @ out.AB
    out.bars["W"] = w_bars(out.AB, out.C, bM[:m], bM[m:, :m], m)
    return out


def grade_d(ref, AB, C, W):
    AB, C, W = _f(AB), _f(C), _f(W)
    return dict(AB=worst_ratio(AB, ref.AB, ref.bars["AB"]), C=worst_ratio(C, ref.C, ref.bars["C"]),
                W=worst_ratio(W, ref.W, ref.bars["W"]),
                W_own=worst_ratio(W, C.astype(LD) @ AB.astype(LD), gamma(ref.case.m + 2) * (np.abs(C) @ np.abs(AB))))


# the window of nk_spline_fit: pivot ratio at or below 2 (m+p)^2 eps takes the pseudo-inverse
def window(mp):
    return 2.0 * mp * mp * EPS


def pivot_ratio_ld(P):
    """min / max Cholesky pivot (Schur-complement diagonal) of P, the factorisation run in longdouble."""
    A = np.array(P, dtype=LD)
    n = A.shape[0]
    piv = []
    for k in range(n):
        piv.append(A[k, k])
        if k + 1 < n:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / A[k, k]
    piv = np.array(piv, dtype=LD)
    return float(piv.min() / piv.max()), bool(np.all(piv > 0))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 emulation of the fit, with fault switches
# ---------------------------------------------------------------------------------------------------------------------
# fault -> (what it is, predicate on the case: does the code the fault lives in run / can its effect leave the fit)
def _multi_pass(c):
    return len(c.passes) > 1


def _several_pieces(c):
    return sum(len(ps) for ps in c.passes) > 1


def _solve_visible(c):
    return c.section == "C"


FAULTS = {
    "dropped_row_at_pass_boundary": lambda c: True,          # the last row of the first pass (of the only pass: the last row)
    "beta0_on_later_pass": _multi_pass,
    "beta0_on_later_pass_bot_only": _multi_pass,
    "cov_without_mirror": _solve_visible,                    # cov leaves a fit only through the solve
    "stale_tile": lambda c: True,                            # the last 128 x 128 tile of every product misses the last pass
    "phi_y_read_one_column_early": lambda c: True,
    "bot_from_wrong_piece": _several_pieces,
    "AB_sliced_with_ld_m": lambda c: c.p > 0,
    "Gtop_left_unsolved": lambda c: True,
    "W_from_stale_A": lambda c: True,
}


def faults_of(c):
    return [f for f, on in FAULTS.items() if on(c)]


def emulate(c, fault=None, lstsq=False):
    """The fit of case c in float64 NumPy, assembled the way nk_spline_fit assembles it.  Returns (AB, C, W)."""
    assert fault is None or fault in FAULTS, fault
    q = problem(*c.key)
    m, p, d = c.m, c.p, c.d
    mp = m + p
    off_out, ldf = layout(m, p)
    rows, passes, _ = plan(q.n, d, p, c.ranges, PASS_ROWS if c.budget else None)
    Xs, Ys = q.X[rows], q.Y[rows]
    G = {k: np.zeros(s) for k, s in (("cov", (mp, mp)), ("top", (m, mp)), ("bot", (d, mp)))}
    off_y = off_out - 1 if fault == "phi_y_read_one_column_early" else off_out
    for ip, ps in enumerate(passes):
        n_rows = sum(ln for _, ln in ps)
        F = np.zeros((n_rows, ldf))
        o = 0
        for b, ln in ps:
            mu = q.mu if c.gram_form and ln >= 2 else None
            F[o:o + ln, :m] = tps_f64(Xs[b:b + ln, :d], q.Z, mu)
            F[o:o + ln, m:mp] = Xs[b:b + ln, d:]
            F[o:o + ln, off_out:off_out + m] = tps_f64(Ys[b:b + ln], q.Z, mu)
            o += ln
        keep = np.ones(n_rows, dtype=bool)
        if fault == "dropped_row_at_pass_boundary" and ip == 0:
            keep[-1] = False
        Fk = F[keep]
        beta = 0.0 if ip == 0 or fault == "beta0_on_later_pass" else 1.0
        beta_bot = 0.0 if fault == "beta0_on_later_pass_bot_only" and ip > 0 else beta
        new = dict(cov=Fk[:, :mp].T @ Fk[:, :mp], top=Fk[:, off_y:off_y + m].T @ Fk[:, :mp])
        b0 = passes[0][0][0]  # (the wrong piece: the rows of the fit's first piece, for every piece)
        xb = np.vstack([Xs[b0:b0 + ln, :d] if fault == "bot_from_wrong_piece" else Xs[b:b + ln, :d] for b, ln in ps])
        new["bot"] = xb[keep].T @ Fk[:, :mp]
        if fault == "cov_without_mirror":
            new["cov"] = np.triu(new["cov"])
        else:
            new["cov"] = np.triu(new["cov"]) + np.triu(new["cov"], 1).T  # TRI_UPPER_MIRROR: the same bits
        for k, b_k in (("cov", beta), ("top", beta), ("bot", beta_bot)):
            upd = b_k * G[k] + new[k]
            if fault == "stale_tile" and ip == len(passes) - 1:
                r0, c0 = ((G[k].shape[0] - 1) // TILE) * TILE, ((mp - 1) // TILE) * TILE
                upd[r0:, c0:] = G[k][r0:, c0:]
            G[k] = upd
    gn = gn_of(c)
    P = G["cov"] + gn * np.eye(mp)
    Rhs = np.vstack([G["top"], G["bot"]])
    if fault in ("cov_without_mirror", "stale_tile"):  # (the planted system is not symmetric positive definite: plain LU)
        M = np.linalg.solve(P.T, Rhs.T).T
    elif lstsq:
        M = np.linalg.lstsq(P, Rhs.T, rcond=mp * EPS)[0].T  # gelsd: singular values <= (m+p) eps sigma_max dropped
    else:
        M = sla.cho_solve(sla.cho_factor(P, lower=True), Rhs.T).T
    AB = np.array(M[:m])
    if fault == "Gtop_left_unsolved":
        AB = np.array(G["top"])
    if fault == "AB_sliced_with_ld_m":
        flat = np.concatenate([M[:m].ravel(), np.zeros(mp)])
        AB = np.array([flat[i * m:i * m + mp] for i in range(m)])
    C = np.array(M[m:, :m])
    if fault == "W_from_stale_A":  # the A of a fit with twice the regulariser
        stale = sla.cho_solve(sla.cho_factor(G["cov"] + 2.0 * gn * np.eye(mp), lower=True), G["top"].T).T
        W = C @ np.hstack([stale[:, :m], AB[:, m:]])
    else:
        W = C @ AB
    return AB, C, W


# ---------------------------------------------------------------------------------------------------------------------
# section A: the device's own spline blocks, read out of B (p = n, U = I_n) and of C (diagonal state coordinates)
# ---------------------------------------------------------------------------------------------------------------------
def grade_blocks(ref, AB, C):
    """({phi_y, phi_y_at_zero, phi_x (diag cases)}: worst err / bar of the blocks read out of the operators, phi_y apart
    where the reference is exactly zero; the number of such entries; the largest magnitude the fit returned there).  Where
    Phi_y is exactly 0 the operator is not: gn B = top (I + E / gn)^-1 has the first-order term -(top E) / gn there, about
    2^-70 of the scale.  In direct mode the block bar is 0 at such an entry, so the first-order bound is the whole bar and a
    block value of one rounding (2^-53 of the scale) would stand 2^17 above it: the check is as sharp as an exact zero."""
    c, q = ref.case, ref.q
    m, n = c.m, c.n
    assert q.identity
    gn = LD(gn_of(c))
    kx, r2x, ky, r2y = blocks(q)
    Ex, Ey = block_bars(q, c.gram_form, np.arange(n), _direct_rows(c))
    rb = readout_bar(c, np.vstack([ref.products["top"], ref.products["bot"]]), ref.products["cov"])
    phi_y = (_f(AB)[:, m:].astype(LD) * gn).T
    zero = _f(r2y) == 0
    bar_y = Ey + rb[:m, m:].T
    out = dict(phi_y=worst_ratio(phi_y[~zero], ky[~zero], bar_y[~zero]), phi_y_at_zero=worst_ratio(phi_y[zero], ky[zero], bar_y[zero]))
    at_zero = float(np.abs(_f(phi_y))[zero].max()) if zero.any() else 0.0
    if q.diag:
        scale = (2.0 ** (np.arange(n) - n // 2))[:, None]
        phi_x = _f(C)[:n].astype(LD) * gn / scale.astype(LD)
        out["phi_x"] = worst_ratio(phi_x, kx, Ex + rb[m:m + n, :m] / scale)
    return out, int(zero.sum()), at_zero


# ---------------------------------------------------------------------------------------------------------------------
# section D: a system inside the window.  Of the section C shapes only (900, 2, 255, 2) has a cov so ill conditioned that a
# small regulariser brings the pivot ratio under the window 2 (m+p)^2 eps at all (the others stay 400 x and more above it at
# gamma = 0).  There, a pivot ratio between 1/30 and 1/3 of the window (gn = 10^-14.5 .. 10^-13.5 sigma_max) comes with
# sigma_min / sigma_max = 0.055 .. 0.55 (m+p) eps, below scipy.linalg.pinv's cut-off instead of 10 x above it: no listed case is
# inside the window at full rank, and the GPU file has no such test.  The same system at gn = 1e-14 sigma_max is what the
# statistics test uses: the factorisation succeeds (smallest pivot 40 x above its rounding) and the window sends it on.
# ---------------------------------------------------------------------------------------------------------------------
WINDOW_SHAPE = (900, 2, 255, 2)
WINDOW_GN_OVER_SMAX = 1e-14


@functools.lru_cache(maxsize=None)
def window_case(gn_over_smax=WINDOW_GN_OVER_SMAX):
    """(case, P longdouble, pivot ratio in longdouble, sigma_min / sigma_max) of WINDOW_SHAPE with gn = gn_over_smax sigma_max."""
    n, d, m, p = WINDOW_SHAPE
    ref, _ = products(_case("C", n, d, m, p, gamma=1.0))
    s = np.linalg.svd(_f(ref["cov"]), compute_uv=False)
    c = _case("C", n, d, m, p, gamma=float(gn_over_smax * s[0] / n))
    P = np.array(ref["cov"], dtype=LD)
    P[np.diag_indices_from(P)] += LD(gn_of(c))
    ratio, positive = pivot_ratio_ld(P)
    assert positive
    return c, P, ratio, float((s[-1] + gn_of(c)) / (s[0] + gn_of(c)))
