"""Extended-precision reference for the lifted recursion z_{t+1} = A z_t + B u_t (+ bias) of nk_rollout.hip / nk_control.hip,
the lifted closed loop, the lift in front of it and the fused open-loop score, with entry-wise bars that come from error
analysis, a Python mirror of the route decision (csrc/nk_chain_plan.h), a float64 emulation of the recursion with planted
faults, and the list of cases tests/test_gpu_rollout_steps.py runs.  NumPy only; nothing here touches the GPU.

u = 2^-53 is the unit roundoff, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
section 3.1): a dot product of k terms, in ANY summation order, with or without fused multiply-adds, has
|fl(x^T y) - x^T y| <= gamma_k |x|^T |y|.

The recursion.  A step forms, per row, a dot product of m + p terms and adds the bias: z^_{t+1} = (A z^_t + B u_t + bias)
(1 + delta), |delta| <= gamma_{m+p+1} on the sum of absolute values.  With e_t = |z^_t - z_t| entry-wise,
    e_{t+1} <= |A| e_t + gamma_{m+p+1} (|A| |z^_t| + |B| |u_t| + |bias|),   |z^_t| <= |z_t| + e_t.
The bar carried along with the reference is
    b_0 = 0 (or the bar of the lift),   b_{t+1} = |A| b_t + gamma_{m+p+3} (|A| |z_t| + |B| |u_t| + |bias|):
the two extra units of gamma pay for the second-order term gamma |A| e_t.  It holds for the register chain (32 parts x 5
columns, DPP reduction), the multi-workgroup chain (64 lanes x KPT chunks, controls in the first partial sum), the
matrix-vector step and the GEMM per step (bias copied, then two products with beta = 1): they differ in summation order
only.  No tolerance is chosen.  With || |A| ||_inf <= 1 the bar grows linearly in t.  x_t = C z_t is one more dot product of
m terms of the device's own z^_t: |x^_t - x_t| <= |C| b_t + gamma_{m+2} |C| |z_t|.

The closed loop.  phi_{t+1} = A phi_t + B K (phi_ref - phi_t), u_t = K (phi_ref - phi_t), x_t = C phi_t.  The device forms
    Acl^ = fl(A - B K)          one product of p terms on top of A:  |Acl^ - Acl| <= gamma_{p+1} (|A| + |B| |K|) =: gamma_{p+1} M,
    kr^  = fl(K phi_ref)        |kr^ - kr| <= gamma_m |K| |phi_ref|,
    c^   = fl(B kr^)            |c^ - c| <= (gamma_m + gamma_p + gamma_m gamma_p) |B| |K| |phi_ref| <= gamma_{m+p+1} s,  s := |B| |K| |phi_ref|,
and then iterates phi^_{t+1} = fl(Acl^ phi^_t + c^), a dot product of m terms plus one addition (gamma_{m+1}).  With
|Acl^| <= (1 + gamma_{p+1}) M and |c^| <= (1 + gamma_{m+p+1}) s,
    e_{t+1} <= M e_t + gamma_{p+1} M |phi_t| + gamma_{m+p+1} s + gamma_{m+1} (M |phi_t| + s)   + second-order terms,
so the bar is  b_0 = 0,  b_{t+1} = M b_t + gamma_{m+p+5} M |phi_t| + gamma_{2m+p+5} s  (three units of gamma for the second-order
terms).  The reference runs the loop as written, in longdouble; M has || M ||_inf <= 1 by design (rows of |A| <= 0.8, rows of
|B| |K| <= 0.2).  The controls are recovered as D = fl(phi_ref - phi^_t), u^ = fl(D K^T):
|u^_t - u_t| <= |K| b_t + gamma_{m+3} |K| |phi_ref - phi_t|   (one rounding for D, m terms, second order), and x as above.

The lift of the chain kernel.  z_0 = k(x_0, Z) S^-1.  The kernel forms, per coordinate, t = z w - fl(x w) with w = fl(1 / l)
(one fused multiply-add, or a product and a difference), and r^2 = sum t^2.  The rounding of fl(x w) does not shrink with t:
|t^ - t| <= 2 u (|a| + |b|) + u |t| for the scaled coordinates a, b, so
    |r^2^ - r^2| <= (d + 8) u r^2 + 4 u sum_k |t_k| (|a_k| + |b_k|),
the first term being the direct-difference rule of gram_reference.kblock_bar_direct.  The kernel value moves by at most
sup |dk / dr^2| times that, plus 8 u |k| for the kernel function's own arithmetic (gram_reference); the linear kernel is a
dot product, gamma_{d+2} |x|^T |z| + u sigma_0^2.  The product with S^-1 (the model's own, nk_model_get 'I') adds
gamma_{m+2} |k| |S^-1|.  Everything is derived: no constant is taken from a measurement.

The fused score: the bound of tests/test_gpu_sysid.py::check_fused, moved here unchanged (score_reference)."""
import collections
import functools

import numpy as np

import gram_reference as G
from chol_reference import EPS, HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP  # noqa: F401  (re-exported for the tests)
from gram_reference import LINEAR, MATERN, RBF, U64, gamma  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------------
# the plan: csrc/nk_chain_plan.h, line by line
# ---------------------------------------------------------------------------------------------------------------------
CHAIN, MW, STEP, GEMM = "CHAIN", "MW", "STEP", "GEMM"
ROUTES = (CHAIN, MW, STEP, GEMM)
CHAIN_ZU, CHAIN_MAX_M, CHAIN_BIAS_DOUBLES, CHAIN_TB_MAX, CHAIN_LDS_MAX = 160, 128, 128, 1024, 64 * 1024
MW_KPT, MW_ROWS, MW_MAX_PU, MW_FEW_GROUPS = 32, 16, 64, 16
STEP_MAX_BATCH, STEP_GEMV_BATCH, STEP_INVARIANT_CHUNK = 8, 16, 16
TERR_TT, TERR_LDS_DOUBLES = 8, 4096

Plan = collections.namedtuple("Plan", "route lift_in_kernel tb blocks kpt nt groups launches launches_per_step")


def chain_d_pad(d_lift):
    return d_lift + (d_lift & 1) if d_lift > 0 else 0


def chain_fixed_doubles(d_lift):
    return 3 * CHAIN_ZU + CHAIN_BIAS_DOUBLES + chain_d_pad(d_lift) + 2


def lifted_chain_ok(m, pu, d_lift):
    if not (1 <= m <= CHAIN_MAX_M and pu >= 0 and m + pu <= CHAIN_ZU):
        return False
    return (chain_fixed_doubles(d_lift) + pu * 16) * 8 <= CHAIN_LDS_MAX


def chain_tb(pu, d_lift, T):
    tb = T - 1 if T > 1 else 1
    if pu > 0:
        room = (CHAIN_LDS_MAX - chain_fixed_doubles(d_lift) * 8) // (8 * pu)
        tb = min(tb, room, CHAIN_TB_MAX)
    return tb


def chain_lds_bytes(pu, d_lift, tb):
    return chain_fixed_doubles(d_lift) * 8 + tb * pu * 8


def chain_control_blocks(T, tb):
    return (T - 1 + tb - 1) // tb if T > 1 else 0


def chain_mw_kpt_class(kpt):
    return 4 if kpt <= 4 else 8 if kpt <= 8 else 16 if kpt <= 16 else 32


def chain_mw_group(m, batch):
    kpt = (m + 63) // 64
    nt = 1
    while nt < 4 and 2 * nt * chain_mw_kpt_class(kpt) <= 32 and 2 * nt <= batch:
        nt *= 2
    return nt


def chain_mw_workgroups(m):
    return (m + MW_ROWS - 1) // MW_ROWS


def chain_mw_fits(m, pu, num_cu):
    return 1 <= m <= 64 * MW_KPT and 0 <= pu <= MW_MAX_PU and chain_mw_workgroups(m) <= num_cu


def chain_mw_wanted(m, pu, pu_read, d_lift, T, batch, num_cu, allowed):
    if not allowed or T < 3:
        return False
    if lifted_chain_ok(m, pu, d_lift):
        return False
    if not chain_mw_fits(m, pu_read, num_cu):
        return False
    nt = chain_mw_group(m, batch)
    groups = (batch + nt - 1) // nt
    return groups <= MW_FEW_GROUPS or groups * chain_mw_workgroups(m) <= num_cu


def chain_mw_chunk(m, batch, num_cu):
    return max(num_cu // chain_mw_workgroups(m), 1) * chain_mw_group(m, batch)


def step_launches(batch, per_trajectory_bias):
    return batch if per_trajectory_bias else (batch + STEP_MAX_BATCH - 1) // STEP_MAX_BATCH


def traj_err_tile(m):
    if m < 1 or m > TERR_LDS_DOUBLES:
        return 0
    return min(TERR_LDS_DOUBLES // m, TERR_TT)


def chain_plan(m, p, d_lift, T, batch, num_cu, batch_invariant=False, per_trajectory_bias=False, mw_allowed=True):
    pu = p if T > 1 else 0
    lift = d_lift > 0 and lifted_chain_ok(m, pu, d_lift)
    dl = d_lift if lift else 0
    z = dict(route=STEP, lift_in_kernel=lift, tb=0, blocks=0, kpt=0, nt=0, groups=0, launches=0, launches_per_step=0)
    if lifted_chain_ok(m, pu, dl):
        tb = chain_tb(pu, dl, T)
        z.update(route=CHAIN, tb=tb, blocks=chain_control_blocks(T, tb))
    elif not batch_invariant and chain_mw_wanted(m, pu, pu, dl, T, batch, num_cu, mw_allowed):
        nb = chain_mw_chunk(m, batch, num_cu)
        first = min(batch, nb)
        nt = chain_mw_group(m, first)
        z.update(route=MW, kpt=chain_mw_kpt_class((m + 63) // 64), nt=nt, groups=(first + nt - 1) // nt,
                 launches=(batch + nb - 1) // nb)
    elif batch_invariant:
        z.update(route=STEP, launches_per_step=sum(step_launches(min(batch - b0, STEP_INVARIANT_CHUNK), per_trajectory_bias)
                                                   for b0 in range(0, batch, STEP_INVARIANT_CHUNK)))
    elif batch <= STEP_GEMV_BATCH:
        z.update(route=STEP, launches_per_step=step_launches(batch, per_trajectory_bias))
    else:
        z.update(route=GEMM, launches_per_step=(1 if per_trajectory_bias else 0) + 1 + (1 if pu > 0 else 0))
    return Plan(**z)


def mw_instantiations(m, batch, num_cu):
    """The (KPT, NT) of every launch of a multi-workgroup call, in launch order."""
    nb = chain_mw_chunk(m, batch, num_cu)
    k = chain_mw_kpt_class((m + 63) // 64)
    return [(k, chain_mw_group(m, min(batch - b0, nb))) for b0 in range(0, batch, nb)]


# ---------------------------------------------------------------------------------------------------------------------
# designed operators and inputs
# ---------------------------------------------------------------------------------------------------------------------
def design(m, p, d, seed=0, a=0.9, row=1.0, brow=None):
    """A = row (a Pi + (1 - a) R): Pi the cyclic shift (Pi z)[i] = z[i + 1], R dense with mixed signs and rows of L1 norm 1,
    so the rows of |A| sum to `row` and A is far from symmetric; B dense (rows of L1 norm `brow` if given); C dense d x m."""
    rng = np.random.default_rng([m, p, d, seed, 20261])
    R = rng.standard_normal((m, m))
    R /= np.abs(R).sum(axis=1, keepdims=True)
    A = row * (a * np.roll(np.eye(m), 1, axis=1) + (1.0 - a) * R)
    B = rng.standard_normal((m, p)) * 0.25
    if brow is not None and p > 0:
        B *= brow / np.abs(B).sum(axis=1, keepdims=True)
    C = rng.standard_normal((d, m)) / np.sqrt(m)
    return np.ascontiguousarray(A), np.ascontiguousarray(B), np.ascontiguousarray(C)


def inputs(m, p, T, batch, seed=0):
    rng = np.random.default_rng([m, p, T, batch, seed, 7])
    return rng.standard_normal((batch, m)), rng.standard_normal((batch, T, p))


def gain(m, p, seed=0, krow=1.0):
    """K (p x m) dense, every row of L1 norm krow: with rows of |B| of L1 norm brow the rows of |B| |K| have L1 norm brow krow."""
    rng = np.random.default_rng([m, p, seed, 99])
    K = rng.standard_normal((p, m))
    K *= krow / np.abs(K).sum(axis=1, keepdims=True)
    return np.ascontiguousarray(K)


# ---------------------------------------------------------------------------------------------------------------------
# references and bars
# ---------------------------------------------------------------------------------------------------------------------
def _f(v):
    return np.abs(np.asarray(v, dtype=np.float64))


def recursion_ld(A, B, z0, U, bias=None, b0=None, T=None):
    """(Z, bar), both (batch, T, m): the recursion in longdouble and its entry-wise bar.  z0 may be longdouble (a lifted
    state); U is (batch, T, p) (row T - 1 is not used); bias (batch, m) or None; b0: bar of z0."""
    A, B = np.asarray(A), np.asarray(B)
    m, p = A.shape[0], B.shape[1] if B.ndim == 2 else 0
    z0 = np.atleast_2d(z0)
    batch = z0.shape[0]
    T = (U.shape[1] if T is None else T)
    Al, Bl, aA, aB = A.astype(LD), B.astype(LD).reshape(m, p), np.abs(A), np.abs(B).reshape(m, p)
    Z, bar = np.empty((batch, T, m), dtype=LD), np.zeros((batch, T, m))
    Z[:, 0] = z0
    if b0 is not None:
        bar[:, 0] = b0
    g = gamma(m + p + 3)
    for t in range(T - 1):
        z = Z[:, t]
        nxt, s = z @ Al.T, _f(z) @ aA.T
        if p > 0:
            nxt = nxt + U[:, t].astype(LD) @ Bl.T
            s += np.abs(U[:, t]) @ aB.T
        if bias is not None:
            nxt = nxt + np.asarray(bias).astype(LD)
            s += np.abs(bias)
        Z[:, t + 1] = nxt
        bar[:, t + 1] = bar[:, t] @ aA.T + g * s
    return Z, bar


def output_ld(C, Z, bar):
    """(x, bar_x) for x_t = C z_t of the device's own lifted states."""
    C = np.asarray(C)
    m = C.shape[1]
    return Z @ C.astype(LD).T, bar @ np.abs(C).T + gamma(m + 2) * (_f(Z) @ np.abs(C).T)


def closed_loop_ld(A, B, C, K, phi0, phi_ref, steps):
    """dict(Phi, bar, x, bar_x, u, bar_u) of the lifted closed loop (module docstring); phi0, phi_ref (batch, m)."""
    m, p = B.shape
    phi0, phi_ref = np.atleast_2d(phi0), np.atleast_2d(phi_ref)
    batch = phi0.shape[0]
    phi_ref = np.broadcast_to(phi_ref, (batch, m))
    Al, Bl, Kl, rl = A.astype(LD), B.astype(LD), K.astype(LD), phi_ref.astype(LD)
    M = np.abs(A) + np.abs(B) @ np.abs(K)
    s = (np.abs(phi_ref) @ np.abs(K).T) @ np.abs(B).T
    Phi, bar = np.empty((batch, steps, m), dtype=LD), np.zeros((batch, steps, m))
    Phi[:, 0] = phi0
    g1, g2 = gamma(m + p + 5), gamma(2 * m + p + 5)
    for t in range(steps - 1):
        f = Phi[:, t]
        Phi[:, t + 1] = f @ Al.T + ((rl - f) @ Kl.T) @ Bl.T
        bar[:, t + 1] = bar[:, t] @ M.T + g1 * (_f(f) @ M.T) + g2 * s
    D = rl[:, None, :] - Phi
    x, bar_x = output_ld(C, Phi, bar)
    return dict(Phi=Phi, bar=bar, x=x, bar_x=bar_x, u=D @ Kl.T, bar_u=bar @ np.abs(K).T + gamma(m + 3) * (_f(D) @ np.abs(K).T), M=M)


def chain_lift_kernel_bar(x0, Zl, par, family, k, r2):
    """Entry-wise bar of the kernel values the chain kernel forms from scaled-then-subtracted coordinates (module docstring)."""
    x0, Zl = np.atleast_2d(np.asarray(x0, dtype=np.float64)), np.atleast_2d(np.asarray(Zl, dtype=np.float64))
    if family == LINEAR:
        return G.kblock_bar_direct(x0, Zl, par, family, k=k, r2=r2)
    d = x0.shape[1]
    ls = np.broadcast_to(np.asarray(par, dtype=np.float64).reshape(-1), (d,))
    a, b = x0 / ls, Zl / ls
    cross = np.zeros((a.shape[0], b.shape[0]))
    for c in range(d):
        cross += np.abs(a[:, c, None] - b[None, :, c]) * (np.abs(a[:, c, None]) + np.abs(b[None, :, c]))
    return G.kblock_bar_direct(x0, Zl, par, family, k=k, r2=r2) + G._slope(family) * 4.0 * U64 * cross


def lift_ld(x0, Zl, par, family, Sinv, center=None):
    """dict(z0, bar, k, bar_api): z_0 = k(x_0, Z) S^-1 in longdouble with the bar of the chain kernel's lift; bar_api is the
    bar of the same product behind nk_lift, whose kernel block may be built in either form (the sum of both bars)."""
    x0, Zl, Sinv = np.atleast_2d(x0), np.atleast_2d(Zl), np.asarray(Sinv)
    m = Zl.shape[0]
    k, r2 = G.kernel_ld(x0, Zl, par, family)
    Ek = chain_lift_kernel_bar(x0, Zl, par, family, k, r2)
    aS = np.abs(Sinv)
    prod = gamma(m + 2) * (_f(k) @ aS)
    out = dict(z0=k @ Sinv.astype(LD), bar=Ek @ aS + prod, k=k, Ek=Ek)
    if center is not None:
        out["bar_api"] = (Ek + G.kblock_bar_gram_form(x0, Zl, center, par, family, k=k)) @ aS + prod
    return out


def gamma_eps(k):
    """gamma with the machine epsilon 2^-52, as the bound of the fused score was written."""
    return k * EPS / (1.0 - k * EPS)


def score_reference(Z, C, true):
    """(sse, ssim, bound_sse, bound_ssim) per trajectory.  |d sse| <= 2 sqrt(sse) |e| + |e|^2 + gamma_{dT} sse with
    e = gamma_{m+2} (|C| |z|) entry by entry: the device forms each entry of C z as a sum of m products (any order: at most
    m + 2 roundings on a path with the final subtraction), squares and adds dT of them (any order: at most dT roundings on a
    path).  Same for ssim with sqrt(ssim).  The device hands back sqrt(sse / dT) and 100 sqrt(sse) / sqrt(ssim): recovering
    the two sums from them costs a square root, a division, a square and a product each (gamma_8 on sse; ssim is recovered
    from both numbers: gamma_16).  Z: (k, T, m) the device's lifted states, true: (k, T, d)."""
    k, T, m = Z.shape
    d = C.shape[0]
    true = np.asarray(true).astype(LD)
    sim = Z.astype(LD) @ C.T.astype(LD)
    sse = np.sum((true - sim) ** 2, axis=(1, 2))
    ssim = np.sum(sim ** 2, axis=(1, 2))
    e = gamma_eps(m + 2) * (np.abs(Z) @ np.abs(C).T)
    e_norm = np.sqrt(np.sum(e.astype(LD) ** 2, axis=(1, 2)))
    bound_sse = 2 * np.sqrt(sse) * e_norm + e_norm ** 2 + gamma_eps(d * T) * sse + gamma_eps(8) * sse
    bound_ssim = 2 * np.sqrt(ssim) * e_norm + e_norm ** 2 + gamma_eps(d * T) * ssim + gamma_eps(16) * ssim
    return sse, ssim, bound_sse, bound_ssim


def score_sums(err_abs, err_rel, d, T):
    """(sse, ssim) in longdouble from the two numbers the device hands back."""
    sse = np.asarray(err_abs).astype(LD) ** 2 * (d * T)
    return sse, sse * (LD(100.0) / np.asarray(err_rel).astype(LD)) ** 2


def worst(got, ref, bar):
    """(max err / bar, index of it): the difference formed in longdouble; an entry with err = 0 counts 0, err > 0 = bar inf."""
    err = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), err.shape)
    if err.size == 0:
        return 0.0, ()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    r = np.where(np.isnan(r), np.inf, r)  # a NaN from the device is a miss
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulation of the recursion, with planted faults
# ---------------------------------------------------------------------------------------------------------------------
ORDERS = ("chunks", "chunks_reversed", "lanes")


def _dot_rows(Gm, v, order):
    """Gm v in float64, summed in chunks of 64 as the kernels do: per chunk then chunk by chunk (either direction), or per lane
    (stride 64) and then over the 64 lanes in a tree."""
    n = Gm.shape[1]
    if order == "lanes":
        part = np.stack([Gm[:, l::64] @ v[l::64] if l < n else np.zeros(Gm.shape[0]) for l in range(64)], axis=1)
        w = 32
        while w >= 1:
            part = part[:, :w] + part[:, w:2 * w]
            w //= 2
        return part[:, 0]
    starts = list(range(0, n, 64))
    if order == "chunks_reversed":
        starts.reverse()
    acc = np.zeros(Gm.shape[0])
    for s in starts:
        acc = acc + Gm[:, s:s + 64] @ v[s:s + 64]
    return acc


FAULTS = ("dropped_term", "stale_state_word", "next_control_row", "last_control_column", "neighbour_inputs",
          "second_block_first_control", "unpadded_leading_dimension", "padding_lane")


def fault_applies(fault, m, p, T, batch, has_bias=False, blocks=1):
    """Can this fault occur, and change anything, at this shape?"""
    if T < 2:
        return False
    # (m = 1 without controls: A is the scalar 0.9 +- 0.1, and with A = 1 the state never changes -- a stale word is the word)
    return {"dropped_term": True, "stale_state_word": T >= 3 and (m > 1 or p > 0), "next_control_row": p > 0 and T >= 3,
            "last_control_column": p > 0, "neighbour_inputs": batch > 1 and (p > 0 or has_bias),
            "second_block_first_control": p > 0 and blocks > 1, "unpadded_leading_dimension": (m + p) % 2 == 1 and m > 1,
            "padding_lane": (m % 64 != 0) or (m + p < CHAIN_ZU)}[fault]


def emulate(A, B, z0, U, bias=None, order="chunks", fault=None, tb=None, T=None):
    """The recursion in float64, (batch, T, m).  fault: one of FAULTS, planted at every step it can occur at (row m // 2,
    column m // 3 where one is meant); tb: steps per control block (second_block_first_control)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    m = A.shape[0]
    p = B.size // m
    B = B.reshape(m, p)
    z0 = np.atleast_2d(np.asarray(z0, dtype=np.float64))
    batch = z0.shape[0]
    T = U.shape[1] if T is None else T
    Gm = np.hstack([A, B])
    r, c = m // 2, m // 3
    if fault == "dropped_term":
        Gm[r, c] = 0.0
    elif fault == "last_control_column":
        Gm[:, m + p - 1] = 0.0
    elif fault == "unpadded_leading_dimension":  # row i read at i * (m + p) of the padded image
        flat = np.hstack([Gm, np.zeros((m, 1))]).ravel()
        Gm = np.stack([flat[i * (m + p):i * (m + p) + m + p] for i in range(m)])
    elif fault == "padding_lane":  # one more lane per row, holding G[i][m - 1] z[m - 1]
        Gm = np.hstack([Gm, A[:, m - 1:m]])
    Z = np.empty((batch, T, m))
    Z[:, 0] = z0
    for b in range(batch):
        src = (b + 1) % batch if fault == "neighbour_inputs" else b
        for t in range(T - 1):
            z = Z[b, t].copy()
            if fault == "stale_state_word" and t >= 1:
                z[c] = Z[b, t - 1, c]
            tu = t
            if fault == "next_control_row" and t + 1 < T:
                tu = t + 1
            if fault == "second_block_first_control" and tb and t > 0 and t % tb == 0:
                tu = t - 1
            v = np.concatenate([z, U[src, tu, :p]])
            if fault == "padding_lane":
                v = np.concatenate([v, z[m - 1:m]])
            acc = _dot_rows(Gm, v, order)
            if bias is not None:
                acc = acc + bias[src]
            Z[b, t + 1] = acc
    return Z


def emulate_closed_loop(A, B, C, K, phi0, phi_ref, steps, order="chunks", fault=None):
    """The device's sequence in float64: Acl = A - B K, c = B (K phi_ref), the recursion with c as bias, u = (phi_ref - phi) K^T,
    x = C phi.  fault: one of the recursion's, planted in the iteration."""
    phi0 = np.atleast_2d(phi0)
    batch, m = phi0.shape
    phi_ref = np.ascontiguousarray(np.broadcast_to(np.atleast_2d(phi_ref), (batch, m)))
    Acl = A - B @ K
    c = (phi_ref @ K.T) @ B.T
    Phi = emulate(Acl, np.zeros((m, 0)), phi0, np.zeros((batch, steps, 0)), bias=c, order=order, fault=fault, T=steps)
    return dict(Phi=Phi, u=(phi_ref[:, None, :] - Phi) @ K.T, x=Phi @ C.T)


def emulate_lift(x0, Zl, par, family, Sinv, fault=None):
    """The chain kernel's lift in float64: scaled coordinates, differences, sum of squares, kernel function, product with S^-1.
    fault: "dropped_landmark" (one kernel value missing from the product), "dropped_coordinate" (the last coordinate left out
    of r^2) or "neighbour_state"."""
    x0, Zl = np.atleast_2d(np.asarray(x0, dtype=np.float64)), np.atleast_2d(np.asarray(Zl, dtype=np.float64))
    if fault == "neighbour_state":
        x0 = np.roll(x0, -1, axis=0)
    d = x0.shape[1]
    if family == LINEAR:
        dd = d - 1 if fault == "dropped_coordinate" else d
        k = x0[:, :dd] @ Zl[:, :dd].T + float(par) ** 2
    else:
        w = 1.0 / np.broadcast_to(np.asarray(par, dtype=np.float64).reshape(-1), (d,))
        if fault == "dropped_coordinate":
            w = w.copy()
            w[-1] = 0.0
        t = (Zl * w)[None, :, :] - (x0 * w)[:, None, :]
        acc = np.sum(t * t, axis=2)
        if family == RBF:
            k = np.exp(-0.5 * acc)
        else:
            s = np.sqrt(acc) * G.SQRT5
            k = (1.0 + s + s * s / 3.0) * np.exp(-s)
    if fault == "dropped_landmark":
        k = k.copy()
        k[:, Zl.shape[0] // 2] = 0.0
    return k @ Sinv


def emulate_score(Z, C, true, tile, fault=None):
    """(sse, ssim) per trajectory in float64, tile by tile as traj_err_partial_kernel adds them.  fault: "dropped_tail" (the
    steps of the last, partial tile left out) or "dropped_row" (the last row of C left out)."""
    k, T, m = Z.shape
    d = C.shape[0]
    rows = d - 1 if fault == "dropped_row" else d
    sse, ssim = np.zeros(k), np.zeros(k)
    for t0 in range(0, T, tile):
        t1 = min(t0 + tile, T)
        if fault == "dropped_tail" and t1 - t0 < tile:
            continue
        y = Z[:, t0:t1] @ C[:rows].T
        sse += np.sum((true[:, t0:t1, :rows] - y) ** 2, axis=(1, 2))
        ssim += np.sum(y * y, axis=(1, 2))
    return sse, ssim


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_rollout_steps.py.  route / kpt / nt / blocks / launches: what the case's name claims on 256 CUs
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name m p T batch route kpt nt blocks launches hook", defaults=(0, 0, 0, 0, False))
D_OUT = 3  # rows of C in the recursion cases


def _name(c):
    return c.name


CHAIN_SHAPES = [(m, p) for m in (1, 3, 5, 64, 127, 128) for p in (0, 1, 7)] + [(128, 32), (101, 59)]
CHAIN_T = (1, 2, 3, 40)
CHAIN_BATCH = (1, 3)
CHAIN_CASES = [Case(f"chain-m{m}-p{p}-T{T}-b{b}", m, p, T, b, CHAIN, blocks=1 if (T > 1) else 0)
               for m, p in CHAIN_SHAPES for T in CHAIN_T for b in CHAIN_BATCH]
BLOCK_CASES = [Case("chain-blocks-m128-p32-T238-second-block-one-step", 128, 32, 238, 2, CHAIN, blocks=2),
               Case("chain-blocks-m128-p32-T240", 128, 32, 240, 1, CHAIN, blocks=2),
               Case("chain-blocks-m8-p1-T1030-cap-1024", 8, 1, 1030, 1, CHAIN, blocks=2)]

MW_T = (3, 20)
_MW = [  # (m, p, batch, kpt, nt, launches)
    (129, 3, 1, 4, 1, 1), (129, 3, 3, 4, 2, 1), (129, 3, 5, 4, 4, 1), (144, 0, 2, 4, 2, 1), (145, 1, 4, 4, 4, 1),
    (256, 2, 1, 4, 1, 1), (257, 2, 1, 8, 1, 1), (257, 2, 2, 8, 2, 1), (512, 1, 3, 8, 2, 1), (512, 1, 4, 8, 4, 1),
    (512, 1, 5, 8, 4, 1), (513, 1, 1, 16, 1, 1), (513, 1, 2, 16, 2, 1), (513, 1, 3, 16, 2, 1), (1024, 2, 1, 16, 1, 1),
    (1024, 2, 2, 16, 2, 1), (1025, 2, 1, 32, 1, 1), (2048, 2, 1, 32, 1, 1), (2048, 2, 3, 32, 1, 2),
    (100, 61, 1, 4, 1, 1), (100, 61, 5, 4, 4, 1), (128, 33, 2, 4, 2, 1), (200, 64, 1, 4, 1, 1), (200, 64, 4, 4, 4, 1)]
MW_CASES = [Case(f"mw-m{m}-p{p}-T{T}-b{b}-kpt{k}-nt{nt}" + ("-two-launches" if L > 1 else ""), m, p, T, b, MW, k, nt, 0, L)
            for (m, p, b, k, nt, L) in _MW for T in MW_T]
# 33 trajectories at m = 512: one launch of 32 (eight groups of four) and a second of one trajectory, <8, 1> in a batch > 1
MW_CASES.append(Case("mw-m512-p1-T3-b33-kpt8-nt4-then-nt1-two-launches", 512, 1, 3, 33, MW, 8, 4, 0, 2))

STEP_CASES = [Case(f"step-m2049-p2-T4-b{b}", 2049, 2, 4, b, STEP) for b in (1, 8, 9, 16)] + \
             [Case(f"step-m129-p65-T20-b{b}", 129, 65, 20, b, STEP) for b in (1, 9)] + \
             [Case(f"step-m300-p2-T2-b{b}", 300, 2, 2, b, STEP) for b in (1, 3)] + \
             [Case(f"step-hook-m129-p3-T20-b{b}", 129, 3, 20, b, STEP, hook=True) for b in (1, 8, 9, 16)]
GEMM_CASES = [Case("gemm-m2049-p2-T4-b17", 2049, 2, 4, 17, GEMM), Case("gemm-m129-p65-T20-b17", 129, 65, 20, 17, GEMM),
              Case("gemm-hook-m129-p3-T20-b17", 129, 3, 20, 17, GEMM, hook=True)]
RECURSION_CASES = CHAIN_CASES + BLOCK_CASES + MW_CASES + STEP_CASES + GEMM_CASES

# closed loop: (name, m, steps, batch, route, hook); p = 2, d = 3; the chain has no controls and a bias per trajectory
LoopCase = collections.namedtuple("LoopCase", "name m steps batch route hook")
LOOP_P, LOOP_D = 2, 3
LOOP_CASES = [LoopCase("loop-chain-m5", 5, 30, 3, CHAIN, False), LoopCase("loop-chain-m128", 128, 30, 3, CHAIN, False),
              LoopCase("loop-mw-m129", 129, 20, 3, MW, False), LoopCase("loop-mw-m513", 513, 20, 3, MW, False),
              LoopCase("loop-step-m129-two-steps", 129, 2, 3, STEP, False),
              LoopCase("loop-step-hook-m129", 129, 20, 3, STEP, True), LoopCase("loop-step-hook-m513", 513, 12, 3, STEP, True),
              LoopCase("loop-gemm-hook-m129", 129, 20, 17, GEMM, True)]

# in-kernel lift: family tag -> (family, anisotropic)
LIFT_FAMILIES = {"rbf": (RBF, False), "rbf-aniso": (RBF, True), "matern": (MATERN, False), "linear": (LINEAR, False)}
LIFT_D = (1, 9, 63, 64, 65, 192)
LIFT_M = (1, 5, 128)
LIFT_T = (1, 5)
LIFT_P, LIFT_BATCH = 1, 3

# fused score: m -> tile
SCORE_M = {512: 8, 513: 7, 2048: 2}
SCORE_D = (1, 3, 5)
SCORE_T = 11  # 11 = 8 + 3 = 7 + 4 = 5 * 2 + 1: a partial last tile at every tile size
SCORE_BATCH = (1, 17)
SCORE_P = 2


def claimed_plan_matches(case, plan):
    """Does the plan agree with what the case's name claims?"""
    if plan.route != case.route:
        return False
    if case.route == CHAIN:
        return plan.blocks == case.blocks
    if case.route == MW:
        return (plan.kpt, plan.nt, plan.launches) == (case.kpt, case.nt, case.launches)
    return True


def case_plans(case, num_cu):
    """(first attempt, the repeat after a give-up or None) of a recursion case through nk_linear_rollout."""
    first = chain_plan(case.m, case.p, 0, case.T, case.batch, num_cu)
    if not case.hook:
        return first, None
    return first, chain_plan(case.m, case.p, 0, case.T, case.batch, num_cu, mw_allowed=False)


@functools.lru_cache(maxsize=None)
def recursion_problem(m, p, T, batch):
    """Operators, inputs, reference and bars of a recursion shape, computed once: a case with fewer trajectories or steps uses
    the leading part (the recursion is causal and the trajectories are independent)."""
    A, B, C = design(m, p, D_OUT)
    z0, U = inputs(m, p, T, batch)
    Z, bar = recursion_ld(A, B, z0, U)
    x, bar_x = output_ld(C, Z, bar)
    for a in (A, B, C, z0, U, Z, bar, x, bar_x):
        a.setflags(write=False)
    return dict(A=A, B=B, C=C, z0=z0, U=U, Z=Z, bar=bar, x=x, bar_x=bar_x)


def lattice_landmarks(m, d, seed=0):
    """m points near the integer lattice of R^d (distinct cells, a tenth of a cell of noise): with a length scale of 0.35
    their RBF kernel matrix is close to the identity, so a Nystrom model of any m is well conditioned in any d."""
    side = 1
    while side ** d < m:
        side += 1
    rng = np.random.default_rng([m, d, seed, 5])
    cells = rng.permutation(side ** d)[:m]
    pts = np.stack([(cells // side ** c) % side for c in range(d)], axis=1).astype(np.float64)
    return pts + 0.1 * rng.standard_normal((m, d))


LATTICE_LS = 0.35
