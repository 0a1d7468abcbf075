"""Extended-precision reference for the control law of the plant-in-the-loop family (nk_plant_loop, nk_poly_plant_loop, their
_multi forms and the lift / gradient pass of nk_mpc_loop with iters = 0; csrc/nk_plant_loop.hip, nk_loop_lanes.h,
nk_poly_lanes.h), with an entry-wise bar that comes from error analysis, Python mirrors of the workgroup classes, a float64
emulation of the device's summation order with planted faults, and the cases tests/test_gpu_plant_loop_steps.py runs.
NumPy only; nothing here touches the GPU.

The check is open loop per step: the control the device returned for step t is recomputed from the state the device stored
for step t,
    u_ref[t, j] = sum_l w[l, j] (k(z_l, x_ref) - k(z_l, x_t)),      w = S^-1 K^T  (spline models: w = K^T),
in longdouble, with S^-1 the model's own K_mm^-1/2 (read back from the model; the square root has its own test).  Step 31
weighs as much as step 0, and nothing of the library stands on the reference side.

The bar.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).
The device holds w^_l, forms dk^_l = fl(kref^_l - k^_l) and sums the products w^_l dk^_l.
  fold          w^ is one fp64 product of m terms per entry (nk_api_loops.hip: launch_gemm(S^-1, K^T)), in any order:
                |w^ - w| <= F := gamma_m (|S^-1| |K^T|) entry-wise; zero for a spline model, which reads K^T as it is.
  kernel value  |k^_l(x) - k_l(x)| <= E_l(x).  plant_kval (nk_poly_lanes.h:17-31) is the arithmetic of the chain kernel's
                lift: the coordinates are SCALED FIRST, xs = fl(x w), zs = fl(z w) with w = fl(1 / l), and subtracted then.
                The issue behind this module names gram_reference.kblock_bar_direct for E; that rule ((d + 8) u r^2 on r^2)
                assumes differences of the unscaled coordinates and is not a bound for this arithmetic: the roundings of the
                two products are relative to |x| / l and |z| / l, not to their difference.  E is therefore
                rollout_reference.chain_lift_kernel_bar, the direct bar plus slope * 4 u sum_k |t_k| (|a_k| + |b_k|) (derived
                there for the same code); it was fixed before the first device run, and the host test prints the float64
                emulation's worst ratio against the direct bar alone beside the asserted one (0.213 against 0.209 on these
                cases: the term matters where |x| / l is large beside the distance).  Linear kernel: gram_reference's
                dot-product rule.  Thin-plate
                spline: unscaled coordinates (w = 1 exactly), spline_fit_reference.tps_bar_direct.
                Both rows count, E_l := E_l(x_t) + E_l(x_ref): |dk' - dk| <= E_l for dk' = kref^_l - k^_l before its rounding.
  subtraction   one rounding, dk^ = dk' (1 + delta), |delta| <= u.
  reduction     sum_l w^_l dk^_l with at most c roundings on any path from a product to the result, so that
                |fl(sum) - sum| <= gamma_c sum |w^_l| |dk^_l| whatever the shape of the tree (Higham 3.1 / 4.2).  c is read
                off the code.  Plant loops (plant_feedback, nk_plant_loop.hip:43-53; poly_feedback :253-273): a chain of LPT
                fused multiply-adds per lane (one rounding each), the six levels of wave_sum64_dpp (nk_common.h:782-793: four
                DPP levels, permlane16 and permlane32 swaps), and with several waves the four levels of row_sum16_dpp
                (nk_loop_lanes.h:18-24) over the 16 words, absent waves contributing exact zeros: c = LPT + 6 (+ 4).
                MPC loop (mpc_w_pass, nk_loop_lanes.h:165-183; nk_mpc_loop.hip:128-129): a chain of fused multiply-adds over
                the wave's up to 64 landmarks, then the waves' words added in wave order onto 0.0 (the first addition is
                exact): c = min(m, 64) + ceil(m / 64) - 1; the sign of dk is reversed and u = -g, both exact.
With W~ := |w| + F (a bound of |w^|) and D~_l := |dk_l| + E_l (a bound of |dk'_l|),
    |u^ - u_ref| <= sum_l ( F_l |dk_l| + W~_l E_l + gamma_{c+1} W~_l D~_l ),
where gamma_{c+1} takes the subtraction and the reduction together.  Every second-order term is inside W~ and D~: no safety
factor is needed and none is applied.  The reference's own error (longdouble, running sums of m terms: m 2^-64 of the same
scales) is below 2^-11 of the fold and reduction terms and is not added.

Designed problems.  Landmarks lie on a jittered grid in the plants' state box [-1, 1]^d in an order drawn by a generator
seeded by (d, m); the length scale is a multiple of the grid step that lets 16 starts spread over the box reach every
landmark (reach: 5 length scales for the RBF, 8 for Matern-5/2: kernel values of 1e-6 and more), and K_mm + jitter I with
jitter = 1e-2 keeps cond(S) near 1e2 however wide the kernel is, so that nk_model_create has an easy square root and the fold
term stays small beside a single landmark's share.  The gain is designed for folded entries of comparable size, K^T = (K_mm
+ jitter I) (S^-1 w_target) = S w_target with |w_target| in [0.5, 1] / sqrt(m) and random signs (splines: K^T = w_target), so
that no landmark hides behind the rounding of the others and |u| stays of order one.  The reference always folds the K that
was really passed with the S^-1 that was really read back.

Measured (profiles/plant_loop_steps.log): the float64 emulation stays at 0.21 of the bar or below (m = 1), every planted fault
exceeds it by 4.8e5 or more on every case where it can occur, and the least visible landmark moves a control by 367 bars; the
device's worst ratios are in the docstring of tests/test_gpu_plant_loop_steps.py."""
import collections
import functools
import types

import numpy as np

import gram_reference as G
import rollout_reference as R
import spline_fit_reference as SF
from chol_reference import HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP  # noqa: F401  (re-exported for the tests)
from gram_reference import LINEAR, MATERN, RBF, U64, gamma  # noqa: F401

SPLINE = "spline"
STEPS, TS, BATCH, JITTER, SIGMA0 = 32, 0.01, 16, 1e-2, 0.7
REACH = {RBF: 5.0, MATERN: 8.0}  # length scales within which a kernel value is 1e-6 or more

# ---------------------------------------------------------------------------------------------------------------------
# the workgroup classes, mirrored from the source
# ---------------------------------------------------------------------------------------------------------------------
PLANT_LOOP_LPT = 4          # nk_plant_loop.hip:29
PLANT_LOOP_MAX_WAVES = 16   # nk_poly_lanes.h:13
PLANT_LOOP_MAX_M = 64 * PLANT_LOOP_LPT * PLANT_LOOP_MAX_WAVES  # nk_plant_loop.hip:30
NK_POLY_MAX_D = NK_POLY_MAX_P = 4
MPC_MAX_WAVES, MPC_LDS_DOUBLES, NK_MPC_MAX_NV = 8, 160 * 1024 // 8, 64  # nk_mpc.h:18-19


def plant_loop_class(m):
    """(landmarks per lane, waves) of nk_plant_loop.hip:146-154: one landmark per lane up to 64, four beyond."""
    if m <= 64:
        return 1, 1
    return PLANT_LOOP_LPT, (m + 64 * PLANT_LOOP_LPT - 1) // (64 * PLANT_LOOP_LPT)


def poly_pad_d(d):
    return 2 if d <= 2 else 4  # nk_poly_lanes.h:14


def poly_pad_p(p):
    return 4 if p == 3 else p  # nk_plant_loop.hip:235


def poly_lpt(D, P):
    """nk_plant_loop.hip:239, of the padded (D, P)."""
    if D == 2:
        return 4 if P <= 2 else 2
    return 2 if P <= 2 else 1


def poly_loop_max_m(d, p):
    """nk_plant_loop.hip:370-373."""
    if not (1 <= d <= NK_POLY_MAX_D and 1 <= p <= NK_POLY_MAX_P):
        return 0
    return 64 * poly_lpt(poly_pad_d(d), poly_pad_p(p)) * PLANT_LOOP_MAX_WAVES


def poly_loop_class(m, d, p):
    """(landmarks per lane, waves) of nk_plant_loop.hip:377-385 in the class of a plant with d states and p inputs."""
    if m <= 64:
        return 1, 1
    lpt = poly_lpt(poly_pad_d(d), poly_pad_p(p))
    return lpt, (m + 64 * lpt - 1) // (64 * lpt)


def mpc_lds_doubles(m, nv):
    return m * nv + 64 * ((m + 63) // 64) + 16  # nk_mpc.h:22


def mpc_loop_max_m(nv):
    """nk_mpc.h:23-28."""
    if nv < 1 or nv > NK_MPC_MAX_NV:
        return 0
    m = 64 * MPC_MAX_WAVES
    while m > 0 and mpc_lds_doubles(m, nv) > MPC_LDS_DOUBLES:
        m -= 1
    return m


def mpc_class(m, nv):
    """(padded QP lanes NP, waves): nk_loop_lanes.h:201-211 and nk_mpc_loop.hip:330 -- one landmark per lane."""
    return (16 if nv <= 16 else 32 if nv <= 32 else 64), (m + 63) // 64


def reduction_c(lpt, waves):
    """Roundings on the longest path of the plant loops' reduction (module docstring)."""
    return lpt + 6 + (4 if waves > 1 else 0)


def mpc_reduction_c(m):
    return min(m, 64) + (m + 63) // 64 - 1


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def kernel_ld(X, Z, par, family):
    """(k, r2) in longdouble: gram_reference.kernel_ld, or the thin-plate spline of spline_fit_reference."""
    if family == SPLINE:
        return SF.tps_ld(X, Z)
    return G.kernel_ld(X, Z, par, family)


def kernel_bar(X, Z, par, family, k, r2):
    """Entry-wise bar E of the kernel values plant_kval forms (module docstring)."""
    if family == SPLINE:
        return SF.tps_bar_direct(np.atleast_2d(X).shape[1], r2, k)
    return R.chain_lift_kernel_bar(X, Z, par, family, k, r2)


def kernel_bar_direct_only(X, Z, par, family, k, r2):
    """The bar of gram_reference.kblock_bar_direct alone (what the scaled products add is left out): printed, never asserted."""
    if family == SPLINE:
        return SF.tps_bar_direct(np.atleast_2d(X).shape[1], r2, k)
    return G.kblock_bar_direct(X, Z, par, family, k=k, r2=r2)


def _scales(par, family, d):
    """Inverse length scales as the device holds them, fl(1 / l); ones for the linear kernel and the spline."""
    if family in (LINEAR, SPLINE):
        return np.ones(d)
    return 1.0 / np.broadcast_to(np.asarray(par, dtype=np.float64).reshape(-1), (d,))


def _kfun64(acc, family, sigma0sq):
    """chain_kfun / tps_value (nk_common.h:814-821, :299-302) in float64 NumPy."""
    if family == RBF:
        return np.exp(-0.5 * acc)
    if family == MATERN:
        t = np.sqrt(acc) * G.SQRT5
        return (1.0 + t + t * t / 3.0) * np.exp(-t)
    if family == LINEAR:
        return acc + sigma0sq
    safe = np.where(acc > 0.0, acc, 1.0)
    return np.where(acc > 0.0, acc * np.log(np.sqrt(safe)), 0.0)


def kval64(xs, zs, family, sigma0sq):
    """plant_kval in float64: xs (..., d) scaled states against zs (m, d) scaled landmarks, coordinates in index order."""
    acc = np.zeros(xs.shape[:-1] + (zs.shape[0],))
    for k in range(zs.shape[1]):
        if family == LINEAR:
            acc = acc + xs[..., k, None] * zs[:, k]
        else:
            df = xs[..., k, None] - zs[:, k]
            acc = acc + df * df
    return _kfun64(acc, family, sigma0sq)


def kmm64(Z, par, family):
    """K_mm + jitter I in float64 (the design of the gain and the host stand-in of S^-1; not a reference)."""
    d = Z.shape[1]
    wi = _scales(par, family, d)
    return kval64(Z * wi, Z * wi, family, SIGMA0 ** 2 if family == LINEAR else 0.0) + JITTER * np.eye(Z.shape[0])


# ---------------------------------------------------------------------------------------------------------------------
# models, gains, starts
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = {"rbf": (RBF, False), "aniso": (RBF, True), "matern": (MATERN, False), "linear": (LINEAR, False),
            "spline": (SPLINE, False)}
_STARTS_PER_AXIS = {1: 16, 2: 4, 3: 2, 4: 2}


@functools.lru_cache(maxsize=None)
def model_spec(fam, d, m):
    """Landmarks Z (m x d, read-only), the kernel parameter (length scales, sigma_0 or None) and the grid step of the model
    every case of (family tag, d, m) shares."""
    family, aniso = FAMILIES[fam]
    n1 = 1
    while n1 ** d < m:
        n1 += 1
    h = 2.0 / n1
    rng = np.random.default_rng([d, m, 20261])
    cells = rng.permutation(n1 ** d)[:m]
    idx = np.stack(np.unravel_index(cells, (n1,) * d), axis=1)
    Z = -1.0 + (idx + 0.5) * h + rng.uniform(-0.3, 0.3, (m, d)) * h
    if family in REACH:
        c = max(1.0, np.sqrt(d) * 0.75 * (n1 / _STARTS_PER_AXIS[d]) / REACH[family])
        par = tuple(c * h * (1.5 if aniso and k == 1 else 1.0) for k in range(d))
    else:
        par = SIGMA0 if family == LINEAR else None
    Z = np.ascontiguousarray(Z)
    Z.setflags(write=False)
    return types.SimpleNamespace(fam=fam, family=family, d=d, m=m, Z=Z, par=par, h=h, jitter=JITTER)


@functools.lru_cache(maxsize=None)
def host_sinv(fam, d, m):
    """(K_mm + jitter I)^-1/2 by a symmetric eigendecomposition in float64: what the host tests put where the GPU test reads
    the model's own S^-1 back.  None for a spline model."""
    s = model_spec(fam, d, m)
    if s.family == SPLINE:
        return None
    lam, V = np.linalg.eigh(kmm64(s.Z, s.par, s.family))
    Si = (V / np.sqrt(lam)) @ V.T
    Si.setflags(write=False)
    return Si


def starts(d, seed):
    """(x0 (BATCH, d), x_ref (BATCH, d)): the starts sit one per cell of a grid over the box (d <= 2; a 2^d grid and uniform
    draws beyond), within a quarter cell of its centre; the references are uniform in 0.9 of the box."""
    rng = np.random.default_rng([d, seed, 7])
    npa = _STARTS_PER_AXIS[d]
    cells = np.stack(np.unravel_index(np.arange(npa ** d), (npa,) * d), axis=1)[:BATCH]
    side = 2.0 / npa
    x0 = -1.0 + (cells + 0.5) * side + rng.uniform(-0.25, 0.25, cells.shape) * side
    if x0.shape[0] < BATCH:
        x0 = np.vstack([x0, rng.uniform(-0.9, 0.9, (BATCH - x0.shape[0], d))])
    x0 = x0[rng.permutation(BATCH)]
    return np.ascontiguousarray(x0), np.ascontiguousarray(rng.uniform(-0.9, 0.9, (BATCH, d)))


def w_target(m, p, seed=0):
    rng = np.random.default_rng([m, p, seed, 11])
    return rng.uniform(0.5, 1.0, (m, p)) * rng.choice([-1.0, 1.0], (m, p)) / np.sqrt(m)


def design_gain(spec, p, Sinv, seed=0):
    """K (p x m, C-contiguous) with S^-1 K^T close to w_target: K^T = (K_mm + jitter I) (S^-1 w_target); splines: w_target."""
    wt = w_target(spec.m, p, seed)
    if spec.family == SPLINE:
        return np.ascontiguousarray(wt.T)
    return np.ascontiguousarray((kmm64(spec.Z, spec.par, spec.family) @ (np.asarray(Sinv) @ wt)).T)


def fold_ld(spec, K, Sinv):
    """(w (m x p) longdouble, F (m x p) float64): the folded gain and its bar gamma_m |S^-1| |K^T| (zero for a spline model)."""
    K = np.asarray(K, dtype=np.float64)
    if spec.family == SPLINE:
        return K.T.astype(LD), np.zeros(K.T.shape)
    Si = np.asarray(Sinv, dtype=np.float64)
    w = np.zeros(K.T.shape, dtype=LD)
    Kt = K.T.astype(LD)
    for i in range(0, spec.m, 512):  # in column blocks: NumPy's longdouble product adds its terms one after the other
        w += Si[:, i:i + 512].astype(LD) @ Kt[i:i + 512]
    return w, gamma(spec.m) * (np.abs(Si) @ np.abs(K.T))


def fold64(spec, K, Sinv):
    """The fold as the device forms it: one float64 product."""
    K = np.asarray(K, dtype=np.float64)
    return K.T.copy() if spec.family == SPLINE else np.asarray(Sinv) @ K.T


# ---------------------------------------------------------------------------------------------------------------------
# the reference and its bar
# ---------------------------------------------------------------------------------------------------------------------
def control_reference(spec, w, F, X, xref, c):
    """X (B, T, d): the states the controls were formed at, xref (B, d) or (1, d) (shared).  Returns dict(u (B, T, p)
    longdouble, bar (B, T, p) float64, share (B, T, m): max_j |w[l, j] dk_l| / bar_j, a landmark's weight against the bar,
    bar_direct: the bar with kblock_bar_direct alone for the kernel values -- printed by the host test, never asserted)."""
    X = np.asarray(X, dtype=np.float64)
    B, T, d = X.shape
    xref = np.broadcast_to(np.asarray(xref, dtype=np.float64).reshape(-1, d), (B, d))
    kr, r2r = kernel_ld(xref, spec.Z, spec.par, spec.family)
    Xf = X.reshape(B * T, d)
    k, r2 = kernel_ld(Xf, spec.Z, spec.par, spec.family)
    dk = kr[:, None, :] - k.reshape(B, T, -1)
    adk = np.abs(dk).astype(np.float64)
    aw = np.abs(w).astype(np.float64)
    Wt = aw + F

    def bar_with(ebar):
        E = (ebar(Xf, spec.Z, spec.par, spec.family, k, r2).reshape(B, T, -1)
             + ebar(xref, spec.Z, spec.par, spec.family, kr, r2r)[:, None, :])
        return adk @ F + E @ Wt + gamma(c + 1) * ((adk + E) @ Wt)

    bar = bar_with(kernel_bar)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.max(adk[..., None] * aw / bar[:, :, None, :], axis=3)
    return dict(u=dk @ w, bar=bar, share=share, bar_direct=bar_with(kernel_bar_direct_only))


def visible(share):
    """Per landmark: dropping it moves some control of the case by more than twice its bar -- a device result that lacks the
    landmark then misses the bar wherever the rest of its error lies inside it."""
    return np.max(share, axis=(0, 1)) > 2.0


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulation of the device's order, with planted faults
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("drop_last", "drop_wave2_first", "drop_slot1_first", "swap_w", "word_missing", "word_stale", "kref_shift",
          "w_column", "scale_off", "exchange")


def fault_applies(fault, spec, p, lpt, waves, mpc=False):
    m = spec.m
    if fault == "drop_last" or fault == "exchange" or fault is None:
        return True
    if fault == "drop_wave2_first":
        return m > 64 and waves > 1
    if fault == "drop_slot1_first":
        return not mpc and lpt > 1 and m > 64 * waves
    if fault in ("swap_w", "kref_shift"):
        return m > 1
    if fault == "word_missing":
        return waves > 1
    if fault == "word_stale":
        return waves > 1 and not mpc
    if fault == "w_column":
        return p > 1
    if fault == "scale_off":
        return spec.family in REACH
    raise ValueError(fault)


def _tree(a):
    """Butterfly over the last axis (a power of two): lanes i and i ^ 1, then pairs of pairs, ... -- the DPP levels and the
    two permlane swaps of wave_sum64_dpp add neighbours of growing blocks, and every lane ends with the same bits."""
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def emulate(spec, w64, X, xref, lpt, waves, fault=None, mpc=False):
    """u (B, T, p) in float64 in the device's order.  Plant loops: lane tid of 64 * waves owns landmarks tid + l * nthreads, a
    chain over l, the wave butterfly, the row sum of the 16 words (absent waves: zeros).  mpc: one landmark per lane, a chain
    over the wave's landmarks in index order, the words added in wave order, u = -g.  Faults: FAULTS (the stale word is the
    second wave's word of step t - 2, the other parity buffer)."""
    X = np.asarray(X, dtype=np.float64)
    B, T, d = X.shape
    m, p = w64.shape
    xref = np.broadcast_to(np.asarray(xref, dtype=np.float64).reshape(-1, d), (B, d))
    wi = _scales(spec.par, spec.family, d)
    s0 = SIGMA0 ** 2 if spec.family == LINEAR else 0.0
    w = np.array(w64, dtype=np.float64)
    if fault == "exchange":
        X, xref = np.broadcast_to(xref[:, None, :], X.shape), X  # (kref then depends on the step)
    zs = spec.Z * wi
    wx = wi.copy()
    if fault == "scale_off":
        wx[0] = 1.0
    kref = kval64((xref * wi), zs, spec.family, s0)
    if kref.ndim == 2:
        kref = kref[:, None, :]
    k = kval64(X * wx, zs, spec.family, s0)
    if fault == "kref_shift":
        kref = np.roll(kref, -1, axis=-1)
    dk = (k - kref) if mpc else (kref - k)
    dk = np.broadcast_to(dk, (B, T, m))
    nthreads = 64 * waves
    drop = {"drop_last": m - 1, "drop_wave2_first": 64, "drop_slot1_first": nthreads}.get(fault)
    if drop is not None:
        w[drop] = 0.0
    if fault == "swap_w":
        w[[0, m - 1]] = w[[m - 1, 0]]
    if fault == "w_column":
        w[:, 0] = w64[:, 1]
    slots = nthreads * lpt
    wp = np.zeros((slots, p))
    wp[:m] = w
    dp = np.zeros((B, T, slots))
    dp[..., :m] = dk
    if mpc:
        wv = wp.reshape(waves, 64, p)
        dv = dp.reshape(B, T, waves, 64)
        words = np.zeros((B, T, waves, p))
        for l in range(64):
            words = wv[:, l, :] * dv[..., l, None] + words
    else:
        wl = wp.reshape(lpt, nthreads, p)
        dl = dp.reshape(B, T, lpt, nthreads)
        part = np.zeros((B, T, nthreads, p))
        for l in range(lpt):
            part = wl[l] * dl[:, :, l, :, None] + part
        words = _tree(np.moveaxis(part.reshape(B, T, waves, 64, p), 3, -1))  # (B, T, waves, p)
    if fault == "word_missing":
        words = words.copy()
        words[:, :, 1] = 0.0
    if fault == "word_stale":
        words = words.copy()
        words[:, 2:, 1] = words[:, :-2, 1].copy()
    if mpc:
        g = np.zeros((B, T, p))
        for wv_ in range(waves):
            g = g + words[:, :, wv_]
        return -g
    if waves == 1:
        return words[:, :, 0]
    pad = np.zeros((B, T, 16, p))
    pad[:, :, :waves] = words
    return _tree(np.moveaxis(pad, 2, -1))


def worst(got, ref, bar):
    return R.worst(got, ref, bar)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "section plant fam d p m")
LADDER = (1, 63, 64, 65, 255, 256, 257, 1025, 4095, 4096)
# what the ladder is for, written out (landmarks per lane, waves): one, two, five and sixteen waves
LADDER_CLASS = {1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (4, 1), 255: (4, 1), 256: (4, 1), 257: (4, 2), 1025: (4, 5),
                4095: (4, 16), 4096: (4, 16)}
EDGES = (64, 65, 257)
BUILTIN = {"duffing": 2, "double_integrator": 2, "hjb": 1}
LADDER_PAIRS = {("duffing", "matern"), ("hjb", "rbf")}
# a plant with two states and three inputs (padded to four) in the format of dynamical_systems.PolynomialSystem
P23 = (2, 3, [(0, 1.0, (0, 1), (0, 0, 0)), (0, 0.3, (0, 0), (0, 1, 0)), (1, 1.0, (1, 0), (0, 0, 0)),
              (1, -0.5, (0, 1), (0, 0, 0)), (1, -1.0, (3, 0), (0, 0, 0)), (1, 0.5, (0, 0), (1, 0, 0)),
              (1, 0.2, (0, 0), (0, 0, 1))])
# polynomial plants: name -> (d, p, family tag); the padded classes are d = 1 (hjb), d = 3 (P3) and p = 3 (P23)
POLY = {"hjb": (1, 1, "rbf"), "duffing": (2, 1, "matern"), "P2": (2, 2, "matern"), "P23": (2, 3, "spline"),
        "P3": (3, 1, "matern"), "P4": (4, 2, "rbf"), "P4b": (4, 4, "matern")}
MPC_PLANTS = {1: ("duffing", 2), 2: ("P2", 2), 4: ("P4b", 4)}


def _a_cases():
    out = []
    for plant, d in BUILTIN.items():
        for fam in FAMILIES:
            if fam == "aniso" and d != 2:
                continue
            ms = LADDER if (plant, fam) in LADDER_PAIRS else EDGES + ((4096,) if (plant, fam) == ("duffing", "spline") else ())
            out += [Case("A", plant, fam, d, 1, m) for m in ms]
    return out


def _b_cases():
    out = []
    for plant, (d, p, fam) in POLY.items():
        lpt = poly_lpt(poly_pad_d(d), poly_pad_p(p))
        for m in sorted({64, 65, 64 * lpt, 64 * lpt + 1, poly_loop_max_m(d, p)}):
            out.append(Case("B", plant, fam, d, p, m))
    return out


def _d_cases():
    return [Case("D", MPC_PLANTS[p][0], "matern", MPC_PLANTS[p][1], p, m)
            for p in (1, 2, 4) for m in (1, 64, 65, 128, 129, mpc_loop_max_m(p))]


A_CASES, B_CASES, D_CASES = _a_cases(), _b_cases(), _d_cases()
ALL_CASES = A_CASES + B_CASES + D_CASES


def name(c):
    return f"{c.section}-{c.plant}-{c.fam}-m{c.m}"


def case_class(c):
    """(landmarks per lane, waves, roundings c of the reduction) the mirror predicts for the case."""
    if c.section == "A":
        lpt, waves = plant_loop_class(c.m)
    elif c.section == "B":
        lpt, waves = poly_loop_class(c.m, c.d, c.p)
    else:
        return 1, mpc_class(c.m, c.p)[1], mpc_reduction_c(c.m)
    return lpt, waves, reduction_c(lpt, waves)


def case_seed(c):
    return list(FAMILIES).index(c.fam) * 100003 + c.m * 7 + c.p


def problem(c, Sinv):
    """The designed problem of case c around the S^-1 handed in (the model's own on the device, host_sinv without one):
    dict(spec, K, w, F, w64, x0, xref, lpt, waves, c)."""
    spec = model_spec(c.fam, c.d, c.m)
    K = design_gain(spec, c.p, Sinv, seed=case_seed(c))
    w, F = fold_ld(spec, K, Sinv)
    x0, xref = starts(c.d, case_seed(c))
    lpt, waves, cc = case_class(c)
    return dict(spec=spec, K=K, w=w, F=F, w64=fold64(spec, K, Sinv), x0=x0, xref=xref, lpt=lpt, waves=waves, c=cc)
