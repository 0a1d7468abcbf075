#!/usr/bin/env python3
"""SHA-256 of the operators of a few fits, of square roots and SPD solves through the C-ABI, and of one lock-step round of
small fits (library given by NYSKOOP_LIB): two builds that compute the same bits print the same lines."""
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
