"""CPU: limits on predicted states in the constrained Koopman MPC -- lqr.mpc_condense_outputs against the dense construction,
the folded ADMM iteration (lqr.mpc_out_solve, the NumPy statement of the interface) against scipy's exact solver (hard rows,
and soft rows on the slack formulation) and against the plain iteration with separate products by G and G', the limiting
cases, the library's host build (nk_mpc_out_qp_host) against the NumPy statement, every validation rule, a stand-alone program
(tests/mpc_out_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan, and reg.solve_mpc with and without
the new arguments."""
import ctypes as C
import os
import pickle
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.optimize

from conftest import relf
from test_mpc_host import _stable, lib  # noqa: F401  (lib: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")
ITERS = 800  # see test_folded_iteration_against_the_exact_solver
X_REF = np.array([0.3, -0.2])


def _dense_outputs(A, B, Cr, N, Ny):
    m, p = B.shape
    nc = Cr.shape[0]
    G, T = np.zeros((Ny * nc, N * p)), np.zeros((Ny * nc, m))
    for k in range(1, Ny + 1):
        T[(k - 1) * nc:k * nc] = Cr @ np.linalg.matrix_power(A, k)
        for j in range(k):
            G[(k - 1) * nc:k * nc, j * p:(j + 1) * p] = Cr @ np.linalg.matrix_power(A, k - 1 - j) @ B
    return G, T


@pytest.mark.parametrize("N,Ny", [(7, 7), (7, 3), (1, 1)])
@pytest.mark.parametrize("p", [1, 2])
def test_condense_outputs_against_the_dense_construction(p, N, Ny):
    """Random stable (A, B), m = 12, two output components: G and T to 1e-12 relative against explicit powers of A."""
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(300 * p + 10 * N + Ny)
    A, B = _stable(rng, 12, p)
    Cr = rng.standard_normal((2, 12))
    G, T = lqr.mpc_condense_outputs(A, B, Cr, N, Ny)
    G2, T2 = _dense_outputs(A, B, Cr, N, Ny)
    assert G.shape == (2 * Ny, N * p) and T.shape == (2 * Ny, 12)
    e_g, e_t = relf(G, G2), relf(T, T2)
    print(f"\np = {p}, N = {N}, Ny = {Ny}: G {e_g:.2e}, T {e_t:.2e}")
    assert e_g <= 1e-12 and e_t <= 1e-12
    with pytest.raises(ValueError):
        lqr.mpc_condense_outputs(A, B, Cr, N, N + 1)


def problems():
    """name -> the two problems: 12 states, one input, N = 8, 8 output rows (one component over 8 steps).
    'hard': y_weight = inf, inputs practically free, the output bound at 0.7 of the largest free prediction (and above the
    first one, which one move cannot bring back): 2 output rows active.  'soft': y_weight = 10 rho, the box at 0.6 of the
    largest unconstrained move, the output bound at 0.6 of the largest free prediction: input and output rows active.
    The bounds are absolute, around the reference state X_REF with ycomp = 0 in every row."""
    from nys_koop_lqr_amd import lqr
    out = {}
    for name, seed in (("hard", 22), ("soft", 25)):
        rng = np.random.default_rng(seed)
        m, p, N = 12, 1, 8
        A, B = _stable(rng, m, p, 0.95)
        Cm = rng.standard_normal((2, m))
        Q, R = 100 * Cm.T @ Cm, np.eye(p)
        K, P = lqr.dlqr(A, B, Q, R)
        H, F = lqr.mpc_condense(A, B, Q, R, P, N)
        G, T = lqr.mpc_condense_outputs(A, B, Cm[:1], N, N)
        e = rng.standard_normal(m)
        rho = lqr.mpc_default_rho(H)
        free = -np.linalg.solve(H, F @ e)
        y = G @ free + T @ e
        if name == "hard":
            bound, yw = 10 * np.max(np.abs(free)), np.inf
            ylim = max(0.7 * np.max(np.abs(y[1:])), 1.05 * abs(y[0]))
        else:
            bound, yw = 0.6 * np.max(np.abs(free)), 10 * rho
            ylim = 0.6 * np.max(np.abs(y))
        ycomp = np.zeros(N, dtype=np.int32)
        out[name] = dict(H=H, F=F, K=K, G=G, T=T, e=e, p=p, N=N, ny=N, bnd=lqr.mpc_bounds(N * p, -bound, bound), bound=bound,
                         ylo=np.full(N, -ylim) + X_REF[0], yhi=np.full(N, ylim) + X_REF[0], ycomp=ycomp, y_weight=yw,
                         u_prev=np.zeros(p), rho=rho, x_ref=X_REF)
    return out


def _numpy(pr, iters, tol=0.0, x_ref=X_REF, **over):
    """lqr.mpc_out_solve on a problem -> (u, z_K, (k, r))."""
    from nys_koop_lqr_amd import lqr
    f = dict(pr)
    f.update(over)
    Kb, S0, _ = lqr.mpc_out_matrices(f["H"], f["rho"], f["p"], f["G"])
    yl, yh = lqr.mpc_out_shift(f["ylo"], f["yhi"], f["ycomp"], x_ref)
    return lqr.mpc_out_solve(f["F"] @ f["e"], f["T"] @ f["e"], *f["bnd"], yl, yh, f["u_prev"], f["rho"],
                             lqr.mpc_out_theta(f["rho"], f["y_weight"]), iters, tol, f["p"], Kb, S0)


def _exact(pr):
    """trust-constr: the hard rows as a LinearConstraint; the soft rows on the slack formulation,
    min 1/2 U'HU + g'U + w_y/2 |sl|^2  with  ylo' <= G U + t - sl <= yhi'."""
    from nys_koop_lqr_amd import lqr
    H, g, G, t = pr["H"], pr["F"] @ pr["e"], pr["G"], pr["T"] @ pr["e"]
    lo, hi, _, _ = pr["bnd"]
    yl, yh = lqr.mpc_out_shift(pr["ylo"], pr["yhi"], pr["ycomp"], pr["x_ref"])
    nv, ny = g.size, t.size
    opts = dict(gtol=1e-13, xtol=1e-14, barrier_tol=1e-14, maxiter=5000)
    if np.isinf(pr["y_weight"]):
        Hs, gs, A_c, blo, bhi = H, g, G, lo, hi
    else:
        Hs = np.block([[H, np.zeros((nv, ny))], [np.zeros((ny, nv)), pr["y_weight"] * np.eye(ny)]])
        gs, A_c = np.concatenate([g, np.zeros(ny)]), np.hstack([G, -np.eye(ny)])
        blo, bhi = np.concatenate([lo, np.full(ny, -np.inf)]), np.concatenate([hi, np.full(ny, np.inf)])
    res = scipy.optimize.minimize(lambda v: 0.5 * v @ Hs @ v + gs @ v, np.zeros(gs.size), jac=lambda v: Hs @ v + gs,
                                  hess=lambda v: Hs, method="trust-constr", bounds=scipy.optimize.Bounds(blo, bhi),
                                  constraints=[scipy.optimize.LinearConstraint(A_c, yl - t, yh - t)], options=opts)
    return res.x[:nv]


def _plain(pr, iters):
    """The iteration on A_c = [I; D; G] with M alone and separate products by G and G' -> (z_1, z_3)."""
    from nys_koop_lqr_amd import lqr
    H, g, G, t, p, rho = pr["H"], pr["F"] @ pr["e"], pr["G"], pr["T"] @ pr["e"], pr["p"], pr["rho"]
    lo, hi, dlo, dhi = pr["bnd"]
    nv = g.size
    _, _, M = lqr.mpc_out_matrices(H, rho, p, G)
    yl, yh = lqr.mpc_out_shift(pr["ylo"], pr["yhi"], pr["ycomp"], pr["x_ref"])
    shift = np.zeros(nv)
    shift[:p] = pr["u_prev"]
    lo_c, hi_c = np.concatenate([lo, dlo + shift, yl - t]), np.concatenate([hi, dhi + shift, yh - t])
    theta = lqr.mpc_out_theta(rho, pr["y_weight"])
    U = -np.linalg.solve(H, g)
    s = np.concatenate([U, lqr.mpc_diff(U, p), G @ U])
    z = lqr.mpc_out_prox(s, lo_c, hi_c, 2 * nv, theta)
    lam = np.zeros(s.size)
    for _ in range(iters):
        w = z - lam
        U = M @ (rho * (w[:nv] + lqr.mpc_diff_t(w[nv:2 * nv], p) + G.T @ w[2 * nv:]) - g)
        s = np.concatenate([U, lqr.mpc_diff(U, p), G @ U])
        z = lqr.mpc_out_prox(s + lam, lo_c, hi_c, 2 * nv, theta)
        lam = lam + (s - z)
    return np.concatenate([z[:nv], z[2 * nv:]])


@pytest.mark.parametrize("name", ["hard", "soft"])
def test_folded_iteration_against_the_exact_solver(name):
    """lqr.mpc_out_solve against trust-constr.  iters = 800, chosen on the CPU so that the NumPy statement is within 1e-8 of
    the input bound: measured 2.8e-12 on 'hard' (6.8e-8 after 400 iterations) and 1.1e-9 on 'soft' (the same after 400:
    trust-constr's own accuracy).  At least one output row is active.  The folded iteration against the plain one: 1e-12
    relative on z after the same count."""
    from nys_koop_lqr_amd import lqr
    pr = problems()[name]
    want = _exact(pr)
    u, z, (k, r) = _numpy(pr, ITERS)
    nv = pr["N"] * pr["p"]
    lo, hi, _, _ = pr["bnd"]
    yl, yh = lqr.mpc_out_shift(pr["ylo"], pr["yhi"], pr["ycomp"], pr["x_ref"])
    yv = pr["G"] @ want + pr["T"] @ pr["e"]
    ylim = float(yh[0])
    act_in = int(np.sum(np.abs(want - lo) < 1e-7 * pr["bound"]) + np.sum(np.abs(want - hi) < 1e-7 * pr["bound"]))
    act_out = int(np.sum(yv >= yh - 1e-7 * ylim) + np.sum(yv <= yl + 1e-7 * ylim))  # at the bound, or (soft) beyond it
    dist = np.max(np.abs(z[:nv] - want)) / pr["bound"]
    e_gu = np.max(np.abs(pr["G"] @ z[:nv] - z[nv:])) / ylim
    print(f"\n[{name}] {k} iterations, residual {r:.2e}: distance {dist:.2e} of the bound; active rows: {act_in} input, "
          f"{act_out} output; z_3 against G z_1 {e_gu:.2e}")
    assert k == ITERS and dist <= 1e-8
    assert act_out >= 1
    assert np.max(np.abs(u - want[:pr["p"]])) <= 1e-8 * pr["bound"]
    e_plain = relf(z, _plain(pr, ITERS))
    print(f"[{name}] folded against plain iteration: {e_plain:.2e}")
    assert e_plain <= 1e-12


def test_limiting_cases():
    """y_weight = inf is the hard clip (theta = 0: z_3 inside the bounds exactly); output bounds all infinite and inactive
    input limits: no iteration at tol = 0 and at tol > 0, z_1 is U_unc; a finite y_weight leaves r > 0 at a start outside the
    output bounds, and z_3 between the bound and s_3."""
    from nys_koop_lqr_amd import lqr
    pr = problems()["hard"]
    yl, yh = lqr.mpc_out_shift(pr["ylo"], pr["yhi"], pr["ycomp"], pr["x_ref"])
    t = pr["T"] @ pr["e"]
    assert lqr.mpc_out_theta(pr["rho"], np.inf) == 0.0 and lqr.mpc_out_theta(2.0, 6.0) == 0.25
    _, z, (k, r) = _numpy(pr, 5)
    assert k == 5 and np.all(z[8:] >= yl - t) and np.all(z[8:] <= yh - t)
    free = -np.linalg.solve(pr["H"], pr["F"] @ pr["e"])
    inf = np.full(8, np.inf)
    for tol in (0.0, 1e-12):
        u, z, (k, r) = _numpy(pr, 50, tol, ylo=-inf, yhi=inf)
        assert k == 0 and r == 0.0 and relf(z[:8], free) <= 1e-13 and u[0] == z[0]
        assert relf(z[8:], pr["G"] @ free) <= 1e-13
    s3 = pr["G"] @ free
    outside = (s3 > yh - t) | (s3 < yl - t)
    assert outside.any()  # the start violates an output bound
    theta = lqr.mpc_out_theta(pr["rho"], 3.0 * pr["rho"])
    Kb, S0, _ = lqr.mpc_out_matrices(pr["H"], pr["rho"], 1, pr["G"])
    # iters = 1 with a huge tol stops at k = 0 only if r <= tol there: r is the residual of the START
    _, _, (k0, r0) = lqr.mpc_out_solve(pr["F"] @ pr["e"], t, *pr["bnd"], yl, yh, None, pr["rho"], theta, 1, 1e300, 1, Kb, S0)
    want = (1 - theta) * np.max(np.maximum(s3 - (yh - t), (yl - t) - s3))  # |s - z| = (1 - theta) x the violation
    assert k0 == 0 and r0 > 0.0 and abs(r0 - want) <= 1e-12 * want
    _, _, (k1, r1) = _numpy(pr, 1, 0.0, y_weight=3.0 * pr["rho"])
    assert k1 == 1 and r1 > 0.0


# ---- the library's host build ---------------------------------------------------------------------------------------------
def _descs(pr, iters, tol_=0.0, **over):
    """(MpcDesc, MpcOut, keep-alive, fields) of a problem; over: fields to replace (arrays, scalars or None)."""
    from nys_koop_lqr_amd import _lib
    lo, hi, dlo, dhi = pr["bnd"]
    f = dict(N=pr["N"], p=pr["p"], m=pr["e"].size, iters=iters, H=pr["H"], F=pr["F"], lo=lo, hi=hi, dlo=dlo, dhi=dhi, K=pr["K"],
             rho=pr["rho"], tol=tol_, ny=pr["ny"], G=pr["G"], T=pr["T"], ylo=pr["ylo"], yhi=pr["yhi"], ycomp=pr["ycomp"],
             y_weight=pr["y_weight"])
    f.update(over)
    ds, out, keep = _lib.MpcDesc(), _lib.MpcOut(), []
    for k, v in f.items():
        tgt = out if k in ("ny", "G", "T", "ylo", "yhi", "ycomp", "y_weight") else ds
        if k in ("N", "p", "m", "iters", "rho", "tol", "ny", "y_weight"):
            setattr(tgt, k, v)
        elif v is None:
            setattr(tgt, k, None)
        else:
            a = np.ascontiguousarray(v, dtype=np.int32 if k == "ycomp" else np.float64)
            keep.append(a)
            setattr(tgt, k, a.ctypes.data)
    return ds, out, keep, f


def _qp_host(lib, pr, iters, tol_=0.0, x_ref=X_REF, **over):
    ds, out, keep, f = _descs(pr, iters, tol_, **over)
    nt, p = pr["N"] * pr["p"] + pr["ny"], pr["p"]
    u, z, info = np.full(p, 7.0), np.full(nt, 7.0), np.full(2, 7.0)
    e, up = np.ascontiguousarray(pr["e"]), np.ascontiguousarray(pr["u_prev"])
    xr = None if x_ref is None else np.ascontiguousarray(x_ref, dtype=np.float64)
    rc = lib.nk_mpc_out_qp_host(C.byref(ds), C.byref(out), e.ctypes.data, None if xr is None else xr.ctypes.data, up.ctypes.data,
                                u.ctypes.data, z.ctypes.data, info.ctypes.data)
    return rc, u, z, info


@pytest.mark.parametrize("name", ["hard", "soft"])
def test_library_host_build_against_the_numpy_statement(lib, name):
    """nk_mpc_out_qp_host against lqr.mpc_out_solve, with the non-zero reference state and ycomp of the problems: 1e-13
    relative on z and u at the full count and after 7 iterations, the same iteration count, the residual within 1e-13 of the
    bound; tol > 0 stops both at the same iteration.  Without x_ref, and with ycomp = -1, the bounds are not shifted."""
    pr = problems()[name]
    for iters, tol in ((ITERS, 0.0), (7, 0.0), (ITERS, 1e-6 * pr["bound"])):
        rc, u, z, info = _qp_host(lib, pr, iters, tol)
        assert rc == 0, lib.nk_last_error().decode()
        u2, z2, (k, r) = _numpy(pr, iters, tol)
        e_z, e_u = relf(z, z2), relf(u, u2)
        print(f"\n[{name}] iters {iters}, tol {tol:.1e}: {int(info[0])} iterations, z {e_z:.2e}, u {e_u:.2e}, residual "
              f"{info[1]:.2e} / {r:.2e}")
        assert e_z <= 1e-13 and e_u <= 1e-13 and info[0] == k
        assert abs(info[1] - r) <= 1e-13 * pr["bound"]
        if tol > 0:
            assert 0 < k < iters and r <= tol
    ref = _numpy(pr, 7, x_ref=None)
    assert relf(ref[1], _numpy(pr, 7)[1]) > 1e-6  # the shift matters
    for kw in (dict(x_ref=None), dict(ycomp=np.full(pr["ny"], -1)), dict(ycomp=None)):
        rc, u, z, info = _qp_host(lib, pr, 7, **kw)
        assert rc == 0 and relf(z, ref[1]) <= 1e-13 and info[0] == 7, kw


def _malformed(pr):
    """(label, fields to replace, iters, what the message must name): the rules of nk_mpc_out, and one of nk_mpc_desc"""
    nv, ny = pr["N"] * pr["p"], pr["ny"]

    def at(a, i, v):
        b = np.array(a, dtype=np.float64)
        b.flat[i] = v
        return b

    yc = np.array(pr["ycomp"])
    yc5, ycm = yc.copy(), yc.copy()
    yc5[2], ycm[1] = 4, -2
    big = 64 - nv + 1
    Gbig = 1e160 * np.ones_like(pr["G"])  # G'G overflows: the Cholesky factorisation of M^-1 meets a non-finite pivot
    return [("ny = 0", dict(ny=0), 5, "ny ="), ("ny = -1", dict(ny=-1), 5, "ny ="),
            ("nv + ny = 65", dict(ny=big, G=np.zeros((big, nv)), T=np.zeros((big, 12)), ylo=None, yhi=None, ycomp=None), 5, "ny ="),
            ("ylo > yhi", dict(ylo=at(pr["ylo"], 3, pr["yhi"][3] + 1.0)), 5, "ylo[3]"),
            ("ylo nan", dict(ylo=at(pr["ylo"], 2, np.nan)), 5, "ylo[2]"), ("yhi = -inf", dict(yhi=at(pr["yhi"], 0, -np.inf)), 5, "yhi[0]"),
            ("ycomp = 4", dict(ycomp=yc5), 5, "ycomp[2]"), ("ycomp = -2", dict(ycomp=ycm), 5, "ycomp[1]"),
            ("y_weight = 0", dict(y_weight=0.0), 5, "y_weight"), ("y_weight < 0", dict(y_weight=-1.0), 5, "y_weight"),
            ("y_weight nan", dict(y_weight=float("nan")), 5, "y_weight"),
            ("G nan", dict(G=at(pr["G"], 5, np.nan)), 5, "G is not finite"), ("T inf", dict(T=at(pr["T"], 7, np.inf)), 5, "T is not finite"),
            ("G null", dict(G=None), 5, "G is null"), ("T null", dict(T=None), 5, "T is null"),
            ("M not positive definite", dict(G=Gbig), 5, "not positive definite"),
            ("iters = 0", dict(), 0, "iters"), ("rho = 0", dict(rho=0.0), 5, "rho"),
            ("lo > hi", dict(lo=at(pr["bnd"][0], 3, pr["bnd"][1][3] + 1.0)), 5, "lo[3]"),
            ("H not positive definite", dict(H=pr["H"] - 2 * np.max(np.linalg.eigvalsh(pr["H"])) * np.eye(nv)), 5,
             "H is not positive definite")]


def test_every_validation_rule(lib):
    """Each malformed pair is NK_ERR_BAD_ARG with the field in nk_last_error(), the outputs keep their canary, and the valid
    pair still solves afterwards."""
    pr = problems()["soft"]
    for label, over, iters, names in _malformed(pr):
        rc, u, z, info = _qp_host(lib, pr, iters, **over)
        msg = lib.nk_last_error().decode()
        assert rc == -1 and names in msg and "nk_mpc_out_qp_host" in msg, (label, rc, msg)
        assert np.all(u == 7.0) and np.all(z == 7.0) and np.all(info == 7.0), label
    ds, out, keep, _ = _descs(pr, 5)
    e = pr["e"]
    assert lib.nk_mpc_out_qp_host(C.byref(ds), None, e.ctypes.data, None, None, e.ctypes.data, None, None) == -1
    assert "output description is null" in lib.nk_last_error().decode()
    assert lib.nk_mpc_out_qp_host(None, C.byref(out), e.ctypes.data, None, None, e.ctypes.data, None, None) == -1
    assert lib.nk_mpc_out_qp_host(C.byref(ds), C.byref(out), None, None, None, e.ctypes.data, None, None) == -1
    rc, u, z, info = _qp_host(lib, pr, 5)
    assert rc == 0 and info[0] == 5 and np.all(np.abs(u) <= pr["bound"])
    # nv + ny = 64 is accepted
    ny = 64 - 8
    rc, *_ = _qp_host(lib, dict(pr, ny=ny), 3, ny=ny, G=np.tile(pr["G"], (7, 1)), T=np.tile(pr["T"], (7, 1)), ylo=None, yhi=None,
                      ycomp=None)
    assert rc == 0, lib.nk_last_error().decode()


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mpc_out_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("mpc_out") / "mpc_out_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mpc_out_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(cases):
        """cases: (problem, iters, tol, replaced fields) -> one output line per case"""
        def num(v):
            v = float(v)
            return v.hex() if np.isfinite(v) else repr(v)

        lines = []
        for pr, iters, tol, over in cases:
            _, _, _, f = _descs(pr, iters, tol, **over)
            arrays = [f[k] for k in ("H", "F", "lo", "hi", "dlo", "dhi", "K", "G", "T", "ylo", "yhi", "ycomp")]
            arrays += [pr["e"], pr["x_ref"], pr["u_prev"]]
            arrays = [np.zeros(0) if a is None else np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]
            lines.append(f"{f['N']} {f['p']} {f['m']} {f['iters']} {num(f['rho'])} {num(f['tol'])} {f['ny']} {num(f['y_weight'])}")
            lines.append(" ".join(str(a.size) for a in arrays))
            lines += [" ".join(num(v) for v in a) for a in arrays if a.size]
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = res.stdout.splitlines()
        assert len(out) == len(cases), out
        return out

    return run


def test_sanitized_program_solves_and_rejects_every_malformed_description(lib, mpc_out_program):
    """The header alone, compiled by the host compiler with -fsanitize=address,undefined: the two problems (800 iterations, 7,
    an early stop) give the library's bits, every malformed pair is rejected with the library's field, and nothing is read or
    written out of bounds on the way."""
    prs = problems()
    good = [(prs[n], iters, tol, {}) for n in ("hard", "soft") for iters, tol in ((ITERS, 0.0), (7, 0.0), (ITERS, 1e-6))]
    bad = _malformed(prs["soft"])
    out = mpc_out_program(good + [(prs["soft"], iters, 0.0, over) for _, over, iters, _ in bad])
    for line, (pr, iters, tol, _) in zip(out, good):
        rc, u, z, info = _qp_host(lib, pr, iters, tol)
        assert rc == 0 and line.startswith("ok "), line
        got = [np.array([float.fromhex(t) for t in part.split()]) for part in line[3:].split("|")]
        assert np.array_equal(got[0], u) and np.array_equal(got[1], z) and np.array_equal(got[2], info), (line, u, info)
    for line, (label, _, _, names) in zip(out[len(good):], bad):
        assert line.startswith("bad ") and names in line, (label, line)


# ---- reg.solve_mpc and the controller object -------------------------------------------------------------------------------
def _fake_regressor(seed=5):
    rng = np.random.default_rng(seed)
    A, B = _stable(rng, 12, 1, 0.95)
    return SimpleNamespace(A=A, B=B, C=rng.standard_normal((2, 12)), n_inputs=1)


def test_solve_mpc_without_and_with_state_limits():
    """Without the new arguments solve_mpc returns the arrays it always returned (the same calls, np.array_equal) in a plain
    MPCController; with x_max on one component it returns an MPCOutputController whose rows are mpc_condense_outputs of that
    component over y_horizon steps; only components with a finite bound get rows; the controller pickles and gives the same
    controls; iters = 0 is the saturated LQR of the plain controller."""
    from nys_koop_lqr_amd import lqr
    from nys_koop_lqr_amd.regressors import KoopmanRegressor, _DeviceModelRegressor
    solve = _DeviceModelRegressor.solve_mpc if hasattr(_DeviceModelRegressor, "solve_mpc") else KoopmanRegressor.solve_mpc
    reg = _fake_regressor()
    ctl = solve(reg, 8, c=100.0, u_min=-0.5, u_max=0.5, du_max=0.1)
    Q = 100.0 * reg.C.T @ reg.C
    Q = (Q + Q.T) / 2
    K, P = lqr.dare_refine(reg.A, reg.B, Q, np.eye(1), lqr.dlqr(reg.A, reg.B, Q, np.eye(1))[0])
    H, F = lqr.mpc_condense(reg.A, reg.B, Q, np.eye(1), P, 8)
    assert type(ctl) is lqr.MPCController
    assert np.array_equal(ctl.H, H) and np.array_equal(ctl.F, F) and np.array_equal(ctl.K, K) and ctl.rho == lqr.mpc_default_rho(H)
    assert np.array_equal(ctl.hi, np.full(8, 0.5)) and np.array_equal(ctl.dlo, np.full(8, -np.inf))
    assert type(solve(reg, 8, c=100.0, x_min=-np.inf, x_max=[np.inf, np.inf])) is lqr.MPCController
    out = solve(reg, 8, c=100.0, u_min=-0.5, u_max=0.5, du_max=0.1, x_max=[np.inf, 0.2], y_horizon=5, y_weight=3.0)
    assert isinstance(out, lqr.MPCOutputController) and out.ny == 5 and out.nv == 8 and out.y_weight == 3.0
    G, T = lqr.mpc_condense_outputs(reg.A, reg.B, reg.C[1:], 8, 5)
    assert np.array_equal(out.G, G) and np.array_equal(out.T, T) and np.array_equal(out.ycomp, np.ones(5, dtype=np.int32))
    assert np.array_equal(out.yhi, np.full(5, 0.2)) and np.all(out.ylo == -np.inf)
    assert np.array_equal(out.H, ctl.H) and np.array_equal(out.F, ctl.F) and np.array_equal(out.lo, ctl.lo)
    both = solve(reg, 8, c=100.0, x_min=-1.0, x_max=1.0)
    assert both.ny == 16 and np.array_equal(both.ycomp, np.tile([0, 1], 8)) and np.isinf(both.y_weight)
    with pytest.raises(ValueError, match="x_min"):
        solve(reg, 8, x_min=1.0, x_max=0.0)
    e = np.random.default_rng(1).standard_normal(12)
    x_ref = np.array([0.1, -0.1])
    u1, info1 = out.control(e, np.array([0.1]), iters=60, x_ref=x_ref)
    other = pickle.loads(pickle.dumps(out))
    assert other._mats is None and other._omats is None and other.ny == 5 and other.horizon == 8
    u2, info2 = other.control(e, np.array([0.1]), iters=60, x_ref=x_ref)
    assert np.array_equal(u1, u2) and info1 == info2 and info1[0] == 60
    u0, info0 = out.control(e, np.array([0.1]), iters=0, x_ref=x_ref)
    assert np.array_equal(u0, ctl.control(e, np.array([0.1]), iters=0)[0]) and info0 == (0, 0.0)


def test_host_loop_passes_the_reference_to_the_output_controller():
    """harness.mpc_control_plant hands x_ref to a controller with output rows and calls a plain controller as before."""
    from nys_koop_lqr_amd import harness
    seen = []

    class Plain:
        n_inputs = 1

        def control(self, e, u_prev, iters, tol):
            seen.append(None)
            return np.zeros(1), (0, 0.0)

    class WithRows(Plain):
        ycomp = np.zeros(1, dtype=np.int32)

        def control(self, e, u_prev, iters, tol, x_ref=None):
            seen.append(np.array(x_ref))
            return np.zeros(1), (0, 0.0)

    reg = SimpleNamespace(lift=lambda x: np.vstack([x, x]))
    step = lambda x, u: 0.5 * x
    harness.mpc_control_plant(2, [0.5, 0.0], [1.0, 1.0], reg, Plain(), step)
    harness.mpc_control_plant(2, [0.5, 0.0], [1.0, 1.0], reg, WithRows(), step)
    assert seen[:2] == [None, None] and all(np.array_equal(s, [0.5, 0.0]) for s in seen[2:]) and len(seen) == 4
