#!/usr/bin/env python3
"""SHA-256 of the operators of a few fits, of square roots and SPD solves through the C-ABI, and of one lock-step round of
small fits, and of the unit-table calls (plant loops, lifted loops, Riccati gains) on models rebuilt from host copies
(library given by NYSKOOP_LIB), then every single-launch closed loop and its multi form (the cases of ops_hash_loops.py, beside
this file): two builds that compute the same bits print the same lines."""
import ctypes as C, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import _lib
h = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()[:16]
rng = np.random.default_rng(5)


def data(n, d, p):
    S = rng.standard_normal((n, d)); U = rng.standard_normal((n, p))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
    return np.hstack([S, U]), Y


for (n, d, p, m, fam) in ((30000, 384, 6, 1100, "rbf"), (25000, 64, 2, 1030, "matern"), (3000, 40, 3, 700, "rbf")):
    X, Y = data(n, d, p)
    kern = nk.ThreeDimensionalKernel(6., 7., 8., d) if fam == "rbf" and d % 3 == 0 else nk.KernelWrapper([6.0] * d)
    reg = nk.KoopmanNystromRegressor(p, kernel=kern, gamma=1e-5, m=m)
    reg.nystrom_centers_output = np.ascontiguousarray(Y[:m].T)
    reg.fit(X, Y)
    print(n, d, p, m, fam, h(reg.A, reg.B, reg.C), "finite", bool(np.all(np.isfinite(reg.A))), flush=True)

ctx = nk.get_context()


def well_conditioned(m):  # the family of test_sqrtm_same_bits
    Q = np.random.default_rng(m).standard_normal((m, 2 * m))
    return Q @ Q.T / (2 * m) + 1e-3 * np.eye(m)


def kernel_matrix(m):  # cond ~ 1e8, the family of test_sqrtm_fast_path_vs_scipy
    pts = np.random.default_rng(m).standard_normal((m, 6))
    D2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * D2 / 9.0) + 1e-6 * np.eye(m)


def singular(m):  # test_sqrtm_numerically_singular_input_is_handled
    t = np.linspace(0.0, 1.0, m)
    return np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.5 ** 2)


def sqrtm(name, P):
    m = P.shape[0]
    P = np.ascontiguousarray(P)
    S, Si = np.zeros((m, m)), np.zeros((m, m))
    it, res = C.c_int32(), C.c_double()
    rc = ctx.lib.nk_sqrtm_spd(ctx.handle, P.ctypes.data, m, m, S.ctypes.data, Si.ctypes.data, C.byref(it), C.byref(res))
    print("sqrtm", name, m, "rc", rc, "iters", it.value, "S", h(S) if rc == 0 else "-", "Sinv", h(Si) if rc == 0 else "-", flush=True)


for m in (5, 100, 333, 500, 1022, 1024, 2000):
    sqrtm("well", well_conditioned(m))
for m in (500, 1024):
    sqrtm("kmat", kernel_matrix(m))
sqrtm("singular", singular(192))

for m in (100, 333, 700):
    r = np.random.default_rng(m)
    Q = r.standard_normal((m, 3 * m))
    P = Q @ Q.T / (3 * m) + 1e-3 * np.eye(m)
    R = r.standard_normal((m, m + 3))
    Xs = np.zeros_like(R)
    rc = ctx.lib.nk_solve_spd(ctx.handle, P.ctypes.data, m, m, R.ctypes.data, m + 3, m + 3, Xs.ctypes.data, m + 3)
    print("solve_spd", m, "rc", rc, "X", h(Xs), flush=True)

# one lock-step round of four small fits: the kernels run through their batched twins
Xl, Yl = data(1200, 12, 2)


def unit(k):
    reg = nk.KoopmanNystromRegressor(2, kernel=nk.KernelWrapper([4.0 + k] * 12), gamma=1e-5, m=100)
    reg.nystrom_centers_output = np.ascontiguousarray(Yl[:100].T)
    reg.fit(Xl, Yl)
    return h(np.array(reg.A), np.array(reg.B), np.array(reg.C))


pool = _lib.lockstep_pool(4, index=31)
before = pool.stats()
hashes = pool.run_round(unit, range(4))
after = pool.stats()
print("lockstep round of 4, m = 100:", *hashes, flush=True)
# how the round's launches were grouped, beside the hashes: where members diverge (their square roots take different numbers
# of steps) the merge breaks ties between kernels by address, so the grouping may differ between two builds; the number of
# launches the members recorded may not
delta = {k: after[k] - before[k] for k in after}
print("lockstep grouping:", delta, "member launches", delta["member_launches_merged"] + delta["single_launches"],
      file=sys.stderr, flush=True)
pool.close()


# ---- models rebuilt from host copies (nk_model_create, nk_spline_model_create) and the unit-table calls on them
def rebuilt(kind, m, p, d, seed, scale=1.0):
    """Random stable operators on random landmarks: A = 0.9 x orthogonal, B and C of order one."""
    r = np.random.default_rng(seed)
    if kind == "spline":
        reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
        reg.centers = scale * r.standard_normal((d, m))
    else:
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.KernelWrapper(np.ones(d)), gamma=1e-6, m=m)
        reg.nystrom_centers_output = scale * r.standard_normal((d, m))
    Q, _ = np.linalg.qr(r.standard_normal((m, m)))
    reg.A, reg.B, reg.C = 0.9 * Q, 0.3 * r.standard_normal((m, p)) / np.sqrt(m), r.standard_normal((d, m))
    return reg, r


for kind in ("nystrom", "spline"):
    reg, r = rebuilt(kind, 50, 2, 3, 11)
    print("rebuilt", kind, "lift of 5 points", h(reg.lift(r.standard_normal((3, 5)))), flush=True)

plant = nk.DuffingOscillator(Ts=0.01)
units = [rebuilt("nystrom", 40, 1, 2, 21), rebuilt("spline", 64, 1, 2, 22), rebuilt("nystrom", 300, 1, 2, 23)]
gains = [0.1 * r.standard_normal(reg._landmark_shape()[1]) for reg, r in units]
x0s = np.array([[0.5, -0.2], [0.1, 0.3], [-0.4, 0.2]])
sc, ox, ou = ctx.plant_loop_multi(plant.plant_id, plant.Ts, 20, [reg._ensure_model() for reg, _ in units], gains, x0s,
                                  np.zeros((3, 2)), u_opt=np.linspace(-1.0, 1.0, 20), want_x=True, want_u=True)
print("plant_loop_multi m = 40, 64, 300, 20 steps: states", h(ox), "controls", h(ou), "scores", h(sc),
      "finite", bool(np.all(np.isfinite(ox))), flush=True)

for steps in (16, 17):
    units = [rebuilt("nystrom", 20, 1, 2, 31), rebuilt("nystrom", 100, 6, 192, 32), rebuilt("spline", 128, 8, 5, 33)]
    dims = [(20, 1, 2), (100, 6, 192), (128, 8, 5)]
    K = [0.2 * r.standard_normal((p, m)) / np.sqrt(m) for (reg, r), (m, p, d) in zip(units, dims)]
    vec = lambda k: [r.standard_normal(dm[k]) for (reg, r), dm in zip(units, dims)]
    phi0, phi_ref, target, u_init = vec(0), vec(0), vec(2), vec(1)
    sc, err, ox, ou, oc = ctx.closed_loop_multi(steps, 0.0075, [reg._ensure_model() for reg, _ in units], dims, K, phi0, phi_ref,
                                                target, u_init, want_x=True, want_u=True, want_ucum=True)
    print("closed_loop_multi", steps, "steps: x", h(*ox), "u", h(*ou), "ucum", h(*oc), "err", h(err), "scores", h(sc),
          "finite", bool(np.all(np.isfinite(sc))), flush=True)

As, Bs, Qs, Rs = [], [], [], []
for m, p in ((3, 1), (64, 2), (100, 6)):
    r = np.random.default_rng(40 + m)
    Q, _ = np.linalg.qr(r.standard_normal((m, m)))
    Cm = r.standard_normal((p + 1, m))
    As.append(0.95 * Q); Bs.append(r.standard_normal((m, p)) / np.sqrt(m)); Qs.append(Cm.T @ Cm); Rs.append(np.eye(p))
Ks, Ps, status, iters, deltas = ctx.dare_batch(As, Bs, Qs, Rs)
print("dare_batch m = 3, 64, 100: status", list(status), "iters", list(iters), "K", h(*Ks), "P", h(*Ps), "delta", h(deltas),
      flush=True)
regs = [rebuilt("nystrom", 40, 2, 3, 51)[0], rebuilt("spline", 64, 2, 4, 52)[0]]
Ks, status, iters = ctx.model_lqr_gain_batch([reg._ensure_model() for reg in regs], 0.5)
print("model_lqr_gain_batch m = 40, 64: status", list(status), "iters", list(iters), "K", h(*Ks), flush=True)

# ---- the matrix-product engines on their own: the fp64 TN engine through nk_gemm(transA = 1) (one slice, edge tiles with a
# K tail, less than a k-step, one tile in 16 slices), the fp32 engine through nk_gemm_f32, a fit on the fp32 engine, and the
# Gram-form kernel matrix (thin-plate spline, d >= 32)
for (M, N, K) in ((128, 128, 64), (130, 258, 17), (2, 2, 3), (128, 128, 2048)):
    r = np.random.default_rng(M + 7 * N + 13 * K)
    A, B, Cm = r.standard_normal((K, M)), r.standard_normal((K, N)), np.empty((M, N))
    _lib.check(ctx.lib.nk_gemm(ctx.handle, 1, 0, M, N, K, 1.0, A.ctypes.data, M, B.ctypes.data, N, 0.0, Cm.ctypes.data, N))
    print("nk_gemm transA", M, N, K, h(Cm), flush=True)
for (M, N, K) in ((132, 260, 96), (128, 128, 2048)):
    r = np.random.default_rng(M + 3 * N + 11 * K)
    A, B, Cm = r.standard_normal((K, M)).astype(np.float32), r.standard_normal((K, N)).astype(np.float32), np.empty((M, N))
    _lib.check(ctx.lib.nk_gemm_f32(ctx.handle, M, N, K, A.ctypes.data, M, B.ctypes.data, N, Cm.ctypes.data, N))
    print("nk_gemm_f32", M, N, K, h(Cm), flush=True)
X, Y = data(4096, 64, 3)
reg = nk.KoopmanNystromRegressor(3, kernel=nk.ThreeDimensionalKernel(6., 6., 6., 64), gamma=1e-4, m=256)
reg.compute_dtype = "f32"
reg.nystrom_centers_output = np.ascontiguousarray(Y[:256].T)
reg.fit(X, Y)
print("fp32 fit 4096 64 3 256", h(reg.A, reg.B, reg.C), "finite", bool(np.all(np.isfinite(reg.A))), flush=True)
r = np.random.default_rng(77)
Kt = nk.kernels.DeviceKernel(_lib.NK_KERNEL_TPS)(r.standard_normal((300, 40)), r.standard_normal((260, 40)))
print("nk_kernel_matrix tps 300 260 40", h(Kt), "finite", bool(np.all(np.isfinite(Kt))), flush=True)

# ---- the single-launch closed loops (plant, polynomial plant, MPC, MPC with output rows) and their multi forms
import ops_hash_loops  # noqa: E402  (beside this file)
ops_hash_loops.main()
