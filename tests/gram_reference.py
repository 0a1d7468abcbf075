"""Extended-precision reference for the part of a Nystrom fit in front of the m x m algebra: the two n x m kernel blocks and
the four Gram accumulators G1..G4 (nk_nystrom_gram / KoopmanNystromRegressor.gram_partial), with the packed layout of
include/nyskoop.h and bars that come from error analysis, each returned as a full matrix so that a test can report the worst
ratio err / bar.  NumPy only; nothing here touches the GPU.

Two facts the tests rest on.  (1) With p = n input columns U = I_n, G1[m:, :m] = U^T Phi_in = Phi_in and G2[:, m:] =
Phi_out^T U = Phi_out^T, and every such entry is a sum with ONE non-zero term (1.0 x value): exact in any summation order, with
or without split-K, in fp64 and on the fp32 engine (1.0f x v is exact, the flush to fp64 is exact).  The accumulators then
hand back the device's own kernel-block entries bit for bit, through the kernels a fit uses.  (2) For any summation order
|fl(x^T y) - x^T y| <= gamma_K |x|^T |y| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1): at
K = 2100 that is 2.3e-13 of the scale |F|^T |F|, while one dropped row moves an entry by about 1 / K of it."""
import functools
import types

import numpy as np

from chol_reference import EPS, HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP  # noqa: F401  (re-exported for the tests)

U64 = 2.0 ** -53  # unit roundoff, fp64 (EPS of chol_reference is the machine epsilon 2^-52)
U32 = 2.0 ** -24  # unit roundoff, fp32
# Rows an fp32 partial sum of the fp32 engine runs over before it is added to its fp64 shadow: one k-step of FBK = 32 rows
# (nk_gemm_tn_f32.hip: `constexpr int FBK = 32`, and `P.flush_steps = epi ? 1 << 30 : env.flush < 1 ? 1 : env.flush` with the
# default NYSKOOP_F32_FLUSH = 1 in launch_tnf).  include/nyskoop.h says the same (32 rows).
F32_FLUSH_ROWS = 32
TILE = 128  # output tile of every engine (nk_gemm_plan.h: TBM)
RBF, MATERN, LINEAR = "rbf", "matern", "linear"
SQRT5 = 2.23606797749978969641


def gamma(k, u=U64):
    """gamma_k = k u / (1 - k u)."""
    return k * u / (1.0 - k * u)


# ---------------------------------------------------------------------------------------------------------------------
# kernels and features, longdouble
# ---------------------------------------------------------------------------------------------------------------------
def kernel_ld(A, B, ls_or_sigma0, family):
    """(k, r2) in longdouble.  r2: squared distance from direct differences of the scaled coordinates, accumulated coordinate by
    coordinate (unscaled for the linear kernel, whose value a.b + sigma0^2 is accumulated the same way)."""
    A, B = np.atleast_2d(np.asarray(A)).astype(LD), np.atleast_2d(np.asarray(B)).astype(LD)
    d = A.shape[1]
    assert B.shape[1] == d
    if family == LINEAR:
        ls = np.ones(d, dtype=LD)
    else:
        ls = np.broadcast_to(np.asarray(ls_or_sigma0, dtype=np.float64).astype(LD).reshape(-1), (d,))
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    dot = np.zeros_like(r2)
    for k in range(d):
        a, b = A[:, k] / ls[k], B[:, k] / ls[k]
        diff = a[:, None] - b[None, :]
        r2 += diff * diff
        if family == LINEAR:
            dot += a[:, None] * b[None, :]
    if family == RBF:
        return np.exp(-r2 / 2), r2
    if family == MATERN:
        t = np.sqrt(LD(5)) * np.sqrt(r2)
        return (1 + t + t * t / 3) * np.exp(-t), r2
    assert family == LINEAR, family
    s0 = LD(float(ls_or_sigma0))
    return dot + s0 * s0, r2


def features_ld(X, Y, Zin, Zout, p, kernel):
    """(Phi_in, U, Phi_out) in longdouble for X = [state | input] (n x (d + p)), Y (n x d); kernel = (family, ls_or_sigma0)."""
    family, par = kernel
    d = np.asarray(Y).shape[1]
    X = np.asarray(X)
    assert X.shape[1] == d + p
    phi_in, _ = kernel_ld(X[:, :d], Zin, par, family)
    phi_out, _ = kernel_ld(Y, Zout, par, family)
    return phi_in, X[:, d:].astype(LD), phi_out


def select_rows(n, row_ranges):
    """Row indices of [begin, end) pairs, concatenated in the order given (None = all rows)."""
    if row_ranges is None:
        return np.arange(n)
    parts = [np.arange(b, e) for b, e in row_ranges]
    return np.concatenate(parts) if parts else np.arange(0)


def _tn(A, B, blk=64):
    """A^T B in longdouble, summed in row blocks of 64 (sqrtm_reference._mm: NumPy's longdouble product adds its terms one
    after the other, and the rounding of that running sum is what limits a longdouble reference; two levels leave ~1/30 of it)."""
    K = A.shape[0]
    out = np.zeros((A.shape[1], B.shape[1]), dtype=LD)
    for i in range(0, K, blk):
        out += A[i:i + blk].T @ B[i:i + blk]
    return out


def gram_from_features(phi_in, U, phi_out, Y, rows=None):
    """({G1..G4} longdouble, {G1..G4} scales |.|^T |.| in fp64) over the given rows."""
    if rows is not None:
        phi_in, U, phi_out, Y = phi_in[rows], U[rows], phi_out[rows], np.asarray(Y)[rows]
    Fin = np.hstack([phi_in, U])
    Yl = np.asarray(Y).astype(LD)
    G = dict(G1=_tn(Fin, Fin), G2=_tn(phi_out, Fin), G3=_tn(phi_out, phi_out), G4=_tn(Yl, phi_out))
    a_in, a_out, a_y = (np.abs(np.asarray(v, dtype=np.float64)) for v in (Fin, phi_out, Yl))
    S = dict(G1=a_in.T @ a_in, G2=a_out.T @ a_in, G3=a_out.T @ a_out, G4=a_y.T @ a_out)
    return G, S


def gram_ld(X, Y, Zin, Zout, p, kernel, row_ranges=None):
    """The four Gram blocks of regressors.py:151,153,162,164 without the regularisers, G1 = [Phi_in | U]^T [Phi_in | U],
    G2 = Phi_out^T [Phi_in | U], G3 = Phi_out^T Phi_out, G4 = Y^T Phi_out over the rows of row_ranges, and their scales."""
    phi_in, U, phi_out = features_ld(X, Y, Zin, Zout, p, kernel)
    return gram_from_features(phi_in, U, phi_out, Y, select_rows(np.asarray(Y).shape[0], row_ranges))


# ---------------------------------------------------------------------------------------------------------------------
# the packed layout (include/nyskoop.h, nk_nystrom_gram): [G1 (m+p)x(m+p) ; G2 m x (m+p)] row-major, leading dimension m+p,
# then at the next even offset [G3 m x m ; G4 d x m], leading dimension m
# ---------------------------------------------------------------------------------------------------------------------
def gram_block1(m, p):
    return ((2 * m + p) * (m + p) + 1) & ~1


def gram_doubles(m, d, p):
    return gram_block1(m, p) + (m + d) * m


def pack(G1, G2, G3, G4, fill=0.0):
    mp, m, d = G1.shape[0], G3.shape[0], G4.shape[0]
    p = mp - m
    assert G1.shape == (mp, mp) and G2.shape == (m, mp) and G3.shape == (m, m) and G4.shape == (d, m)
    out = np.full(gram_doubles(m, d, p), fill, dtype=np.result_type(G1, G2, G3, G4))
    out[:(2 * m + p) * mp] = np.vstack([G1, G2]).ravel()
    out[gram_block1(m, p):] = np.vstack([G3, G4]).ravel()
    return out


def unpack(gram, m, d, p):
    gram = np.asarray(gram)
    mp = m + p
    assert gram.shape == (gram_doubles(m, d, p),), (gram.shape, gram_doubles(m, d, p))
    top = gram[:(2 * m + p) * mp].reshape(2 * m + p, mp)
    bot = gram[gram_block1(m, p):].reshape(m + d, m)
    return dict(G1=top[:mp], G2=top[mp:], G3=bot[:m], G4=bot[m:])


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def _slope(family):
    """sup |dk / d(r^2)|: 1/2 for exp(-r^2 / 2); 5/6 for Matern-5/2, whose derivative is -(5/6)(1 + sqrt5 r) e^(-sqrt5 r)."""
    return {RBF: 0.5, MATERN: 5.0 / 6.0}[family]


def _linear_bar(A, Z, sigma0, u):
    d = np.asarray(A).shape[1]
    return gamma(d + 2, u) * (np.abs(A) @ np.abs(Z).T) + u * float(sigma0) ** 2


def kblock_bar_gram_form(A, Z, center, ls_or_sigma0, family, u=U64, k=None):
    """Entry-wise bar of a kernel block built in Gram form, r^2 = |a|^2 + |b|^2 - 2 a.b of the rows centred on `center` and
    scaled by 1 / l: r^2 carries delta = (d + 8) u (|a|^2 + |b|^2) (the rule of test_tps_kernel_matrix_gram_form: d products
    and sums in each of the three terms, the centring and the scaling), the kernel moves by at most sup|dk/dr^2| delta, and
    8 u |k| stands for the kernel function's own arithmetic.  Linear: a dot product of d terms of the uncentred rows,
    gamma_(d+2) |a|^T |b| + u sigma0^2.  u = 2^-53, or 2^-24 for the fp32 engine.  k: kernel_ld's values, if at hand."""
    A, Z = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    if family == LINEAR:
        return _linear_bar(A, Z, ls_or_sigma0, u)
    d = A.shape[1]
    ls = np.broadcast_to(np.asarray(ls_or_sigma0, dtype=np.float64).reshape(-1), (d,))
    na, nb = (((A - center) / ls) ** 2).sum(1), (((Z - center) / ls) ** 2).sum(1)
    if k is None:
        k, _ = kernel_ld(A, Z, ls_or_sigma0, family)
    return _slope(family) * (d + 8) * u * (na[:, None] + nb[None, :]) + 8 * u * np.abs(k.astype(np.float64))


def kblock_bar_direct(A, Z, ls_or_sigma0, family, u=U64, k=None, r2=None):
    """Entry-wise bar of a kernel block from direct differences: no cancellation, so r^2 carries (d + 8) u r^2 only."""
    A, Z = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    if family == LINEAR:
        return _linear_bar(A, Z, ls_or_sigma0, u)
    if k is None or r2 is None:
        k, r2 = kernel_ld(A, Z, ls_or_sigma0, family)
    return _slope(family) * (A.shape[1] + 8) * u * r2.astype(np.float64) + 8 * u * np.abs(k.astype(np.float64))


def contraction_bar(K, scale, u_operand=0.0, flush_len=0):
    """(2 u_operand + gamma32_flush_len + gamma_(K+2)) scale for a contraction over K rows in any summation order.  fp64:
    u_operand = 0 and no fp32 term.  fp32 engine: u_operand = 2^-24 (U and Y are rounded to fp32; the kernel-block operands are
    fp32 values already, their error is the kernel-block bar) and fp32 partial sums over flush_len rows."""
    g32 = gamma(flush_len, U32) if flush_len else 0.0
    return (2.0 * u_operand + g32 + gamma(K + 2, U64)) * np.asarray(scale, dtype=np.float64)


def propagated_bar(E_in, E_out, phi_in, U, phi_out, Y, rows=None):
    """What entry-wise errors |F^ - F| <= E of the kernel blocks add to the four Gram blocks: E^T |F| + |F|^T E (+ E^T E)."""
    f = lambda v: np.abs(np.asarray(v, dtype=np.float64))
    if rows is not None:
        E_in, E_out, phi_in, U, phi_out, Y = (np.asarray(v)[rows] for v in (E_in, E_out, phi_in, U, phi_out, Y))
    Fin, Ein = np.hstack([f(phi_in), f(U)]), np.hstack([E_in, np.zeros(np.asarray(U).shape)])
    Fo, Eo, Ya = f(phi_out), E_out, f(Y)
    return dict(G1=Ein.T @ Fin + Fin.T @ Ein + Ein.T @ Ein, G2=Eo.T @ Fin + Fo.T @ Ein + Eo.T @ Ein,
                G3=Eo.T @ Fo + Fo.T @ Eo + Eo.T @ Eo, G4=Ya.T @ Eo)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar, the difference formed in longdouble."""
    err = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), err.shape)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(np.max(r))


# ---------------------------------------------------------------------------------------------------------------------
# plain NumPy emulations of what the device does (the host tests hold the bars against them; the fp32 one also measures what
# float32 exp / sqrt add to the fp32 kernel-block bar, which the project's text does not let one derive)
# ---------------------------------------------------------------------------------------------------------------------
def kblock_emulate(A, Z, center, ls_or_sigma0, family, dtype=np.float64):
    """Gram-form kernel block in `dtype` arithmetic: rows centred and scaled in fp64 and rounded to dtype (prep_rows /
    prep_rows_f32), squared norms, dot products, clamp at 0 and the kernel function in dtype."""
    A, Z = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    if family == LINEAR:
        a, b = A.astype(dtype), Z.astype(dtype)
        return a @ b.T + dtype(float(ls_or_sigma0) ** 2)
    w = 1.0 / np.broadcast_to(np.asarray(ls_or_sigma0, dtype=np.float64).reshape(-1), (A.shape[1],))
    a, b = ((A - center) * w).astype(dtype), ((Z - center) * w).astype(dtype)
    D = np.maximum((a * a).sum(1, dtype=dtype)[:, None] + (b * b).sum(1, dtype=dtype)[None, :] - dtype(2) * (a @ b.T), dtype(0))
    if family == RBF:
        return np.exp(dtype(-0.5) * D)
    t = np.sqrt(D) * dtype(SQRT5)
    return (dtype(1) + t + t * t * dtype(1.0 / 3.0)) * np.exp(-t)


def contraction_emulate(A, B, f32=False, flush_len=F32_FLUSH_ROWS):
    """A^T B as the engines form it: fp64 throughout, or (fp32 engine) float32 operands, float32 partial sums over flush_len
    rows, the partial sums added in fp64."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if not f32:
        return A.T @ B
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    out = np.zeros((A.shape[1], B.shape[1]))
    for i in range(0, A.shape[0], flush_len):
        out += (A32[i:i + flush_len].T @ B32[i:i + flush_len]).astype(np.float64)
    return out


def f32_kblock_allowance(A, Z, center, ls_or_sigma0, family, k=None):
    """(allowed ratio, emulation's ratio) for a kernel block of the fp32 engine against kblock_bar_gram_form(u = 2^-24): the
    float32 NumPy emulation of the same formula is measured against kernel_ld, and the device -- another exp, another summation
    order, the same class of arithmetic -- is allowed 4 x the emulation's worst ratio."""
    if k is None:
        k, _ = kernel_ld(A, Z, ls_or_sigma0, family)
    bar = kblock_bar_gram_form(A, Z, center, ls_or_sigma0, family, U32, k=k)
    r = worst_ratio(kblock_emulate(A, Z, center, ls_or_sigma0, family, np.float32), k, bar)
    return 4.0 * r, r


# ---------------------------------------------------------------------------------------------------------------------
# problems: data as _synth of test_gpu_parity.py; the output landmarks are rows of Y and separate input landmarks are rows of
# the state, so coincident points (r^2 = 0 exactly, where the Gram form clamps a negative r^2) occur in both blocks
# ---------------------------------------------------------------------------------------------------------------------
def kernel_spec(family, d, aniso=False):
    if family == LINEAR:
        return (LINEAR, 0.7)
    if aniso:  # l from 1 to 100: coordinates with a short length scale give large scaled norms
        return (family, tuple(np.geomspace(1.0, 100.0, d)))
    return (family, (0.9 * np.sqrt(d),))


@functools.lru_cache(maxsize=None)
def problem(n, d, m, p, family=RBF, aniso=False, sep=False, identity=False, seed=0):
    """X (n x (d + p)), Y (n x d), landmarks Zout (rows of Y; row 0 is always one) and Zin (rows of the state when sep, else
    Zout), kernel spec and the library's centre.  identity: the p = n input columns are I_n.  Data and landmarks are drawn from
    a pool of max(n, m) rows, of which the first n are the data."""
    pool = max(n, m)
    rng = np.random.default_rng(7919 * d + 31 * pool + seed)
    pin = 3
    S = rng.standard_normal((pool, d))
    Uall = rng.standard_normal((pool, pin))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / np.sqrt(d))) + Uall @ (rng.standard_normal((pin, d)) * 0.1)
    idx = rng.permutation(pool)[:m]
    if 0 not in idx:
        idx[0] = 0
    idx_in = rng.permutation(pool)[:m]
    if 0 not in idx_in:
        idx_in[0] = 0
    if identity:
        assert p == n
        U = np.eye(n)
    else:
        assert p <= pin
        U = Uall[:n, :p]
    X = np.ascontiguousarray(np.hstack([S[:n], U]))
    Yn = np.ascontiguousarray(Y[:n])
    Zout = np.ascontiguousarray(Y[idx])
    Zin = np.ascontiguousarray(S[idx_in]) if sep else Zout
    kernel = kernel_spec(family, d, aniso)
    center = np.zeros(d) if family == LINEAR else Zout.mean(axis=0)
    for a in (X, Yn, Zout, Zin, center):
        a.setflags(write=False)
    return types.SimpleNamespace(key=(n, d, m, p, family, aniso, sep, identity, seed), n=n, d=d, m=m, p=p, family=family, X=X,
                                 Y=Yn, Zout=Zout, Zin=Zin, sep=sep, kernel=kernel, par=kernel[1], center=center)


@functools.lru_cache(maxsize=None)
def _problem_kernels(n, d, m, family, aniso, sep, seed):
    q = problem(n, d, m, 0, family, aniso, sep, False, seed)  # (the kernel blocks do not depend on the input columns)
    return kernel_ld(q.X[:, :d], q.Zin, q.par, family) + kernel_ld(q.Y, q.Zout, q.par, family)


def problem_kernels(q_key):
    """(Phi_in, r2_in, Phi_out, r2_out) of problem(*q_key) in longdouble, cached: the cases of a shape share them."""
    n, d, m, p, family, aniso, sep, identity, seed = q_key
    return _problem_kernels(n, d, m, family, aniso, sep, seed)


def problem_features(*key):
    """(Phi_in, U, Phi_out) of problem(*key) in longdouble (features_ld of its data, from the cached kernel blocks)."""
    q = problem(*key)
    k_in, _, k_out, _ = problem_kernels(key)
    return k_in, q.X[:, q.d:].astype(LD), k_out


@functools.lru_cache(maxsize=None)
def problem_gram(key, row_ranges=None):
    """(G, scales) of problem(*key) over row_ranges (a tuple of (begin, end) pairs or None), cached."""
    q = problem(*key)
    phi_in, U, phi_out = problem_features(*key)
    return gram_from_features(phi_in, U, phi_out, q.Y, select_rows(q.n, row_ranges))


@functools.lru_cache(maxsize=None)
def problem_f32_allowance(q_key):
    """f32_kblock_allowance of the two kernel blocks of problem(*q_key): ((allowed, emulated) input block, (..) output block)."""
    q = problem(*q_key)
    k_in, _, k_out, _ = problem_kernels(q_key)
    return (f32_kblock_allowance(q.X[:, :q.d], q.Zin, q.center, q.par, q.family, k=k_in),
            f32_kblock_allowance(q.Y, q.Zout, q.center, q.par, q.family, k=k_out))


def kblock_bars_f32(q):
    """(E_in, E_out) of the fp32 engine for the propagation into the Gram blocks: the fp32 Gram-form bars, widened to the
    allowance of Section A where that exceeds 1 (linear: no exp, the bar stands as it is)."""
    E_in, E_out = kblock_bars(q, "gram", U32)
    if q.family == LINEAR:
        return E_in, E_out
    (a_in, _), (a_out, _) = problem_f32_allowance(q.key)
    return max(1.0, a_in) * E_in, max(1.0, a_out) * E_out


def kblock_bars(q, form, u=U64):
    """(E_in, E_out): the kernel-block bars of problem q; form = "gram" (Gram form, the library's centre) or "direct"."""
    d = q.d
    k_in, r2_in, k_out, r2_out = problem_kernels(q.key)
    if form == "gram":
        return (kblock_bar_gram_form(q.X[:, :d], q.Zin, q.center, q.par, q.family, u, k=k_in),
                kblock_bar_gram_form(q.Y, q.Zout, q.center, q.par, q.family, u, k=k_out))
    return (kblock_bar_direct(q.X[:, :d], q.Zin, q.par, q.family, u, k=k_in, r2=r2_in),
            kblock_bar_direct(q.Y, q.Zout, q.par, q.family, u, k=k_out, r2=r2_out))


# Section A of tests/test_gpu_gram_entries.py: (n, m) with p = n identity inputs.  Edge tiles in both directions of the
# 128 x 128 kernel-matrix tiles; exactly one tile; a handful of rows.
A_SHAPES = [(300, 130), (128, 128), (5, 4)]

# Section B: name -> (problem key fields, options).  Base shape d = 40, m = 130, n = 2100 (132 k-steps of 16 rows: split-K and
# the reduce kernel run).  launches = Gram kernel launches per pass (1 fused, 3 generic).  The generic route is taken at m = 1
# only: the feature matrix is padded to even columns, so an odd m + p meets the fused engine's operand contract as well.
def _b(n=2100, d=40, m=130, p=2, family=RBF, sep=False, **opt):
    opt.setdefault("launches", 1)
    opt.setdefault("passes", 1)
    return dict(key=(n, d, m, p, family, False, sep, False, 0), **opt)


B_CASES = {
    "fused_p2": _b(),
    "fused_p0": _b(p=0),
    "one_tile_m126_p2": _b(m=126),
    "fused_odd_p3": _b(p=3),
    "generic_m1_p2": _b(m=1, launches=3),
    "n1": _b(n=1),
    "n17": _b(n=17),
    "n100": _b(n=100),
    "matern_p2": _b(family=MATERN),
    "linear_p2": _b(family=LINEAR),
    "separate_input_landmarks": _b(sep=True),
    "two_ranges": _b(row_ranges=((0, 700), (1100, 2100))),
    "two_ranges_and_an_empty_one": _b(row_ranges=((0, 700), (900, 900), (1100, 2100))),
    "three_passes": _b(budget="1e-6", passes=3),
    "two_passes_two_ranges": _b(budget="1e-6", passes=2, row_ranges=((0, 700), (1100, 2100))),
    "three_passes_odd_p3": _b(p=3, budget="1e-6", passes=3),
    "three_passes_generic_m1_p2": _b(m=1, budget="1e-6", passes=3, launches=3),
    "device_inputs_odd_ldy": _b(d=33, m=131, p=1, device=True),
    "f32_d40_p2": _b(f32=True),
    "f32_d64_p3": _b(d=64, p=3, f32=True),
    "f32_d40_p2_three_passes": _b(f32=True, budget="1e-6", passes=3),
}


def all_shapes():
    """Every (problem key, row_ranges) the GPU tests contract over: the mutation checks of the host tests run on each."""
    out = [((n, d, m, n, RBF, False, False, True, 0), None) for n, m in A_SHAPES for d in (40,)]
    seen = set()
    for c in B_CASES.values():
        k = (c["key"], c.get("row_ranges"))
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out
