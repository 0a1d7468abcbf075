"""CPU: the constrained Koopman MPC on the host -- lqr.mpc_condense against the dense block construction, the first move of the
unconstrained QP against the Riccati gain, the ADMM iteration (lqr.mpc_solve, the NumPy statement of the interface) against
independent exact solvers, the library's host build (nk_mpc_qp_host) against the NumPy statement, every validation rule of the
description, and a stand-alone program (tests/mpc_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan
that sends the same problems and every malformed description through csrc/nk_mpc.h."""
import ctypes as C
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize

from conftest import relf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")
ITERS = 200  # test 3: see test_admm_against_exact_solvers


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def _stable(rng, m, p, radius=0.9):
    A = rng.standard_normal((m, m))
    A *= radius / np.max(np.abs(np.linalg.eigvals(A)))
    return A, rng.standard_normal((m, p))


def _dense(A, B, Q, R, P, N):
    """H = 2 (Gamma' Qbar Gamma + Rbar), F = 2 Gamma' Qbar Phi from the stacked prediction e = Phi e_0 + Gamma U."""
    m, p = B.shape
    Gam, Phi = np.zeros((N * m, N * p)), np.zeros((N * m, m))
    for k in range(1, N + 1):
        Phi[(k - 1) * m:k * m] = np.linalg.matrix_power(A, k)
        for j in range(k):
            Gam[(k - 1) * m:k * m, j * p:(j + 1) * p] = np.linalg.matrix_power(A, k - 1 - j) @ B
    Qb = np.kron(np.eye(N), Q)
    Qb[-m:, -m:] = P
    return 2 * (Gam.T @ Qb @ Gam + np.kron(np.eye(N), R)), 2 * Gam.T @ Qb @ Phi


@pytest.mark.parametrize("N", [1, 2, 7])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_condense_against_the_dense_construction(p, N):
    """Random stable (A, B), m = 12: H and F to 1e-12 relative; H exactly symmetric."""
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(100 * p + N)
    A, B = _stable(rng, 12, p)
    Cm = rng.standard_normal((3, 12))
    Q, R = Cm.T @ Cm, np.eye(p) + 0.1 * np.ones((p, p))
    _, P = lqr.dlqr(A, B, Q, R)
    H, F = lqr.mpc_condense(A, B, Q, R, P, N)
    H2, F2 = _dense(A, B, Q, R, P, N)
    assert H.shape == (N * p, N * p) and F.shape == (N * p, 12) and np.array_equal(H, H.T)
    e_h, e_f = relf(H, H2), relf(F, F2)
    print(f"\np = {p}, N = {N}: H {e_h:.2e}, F {e_f:.2e}")
    assert e_h <= 1e-12 and e_f <= 1e-12


@pytest.mark.parametrize("N", [1, 2, 7, 20])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_first_move_is_the_riccati_gain(p, N):
    """The first p rows of H^-1 F equal dlqr's K when P is the Riccati solution.  Bar: 10 x the movement of that quantity
    under a 1e-15 relative perturbation of A, floor 1e-10."""
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(200 * p + N)
    A, B = _stable(rng, 12, p)
    Cm = rng.standard_normal((3, 12))
    Q, R = Cm.T @ Cm, np.eye(p)
    K, P = lqr.dlqr(A, B, Q, R)

    def first(Am):
        H, F = lqr.mpc_condense(Am, B, Q, R, P, N)
        return np.linalg.solve(H, F)[:p]

    K1 = first(A)
    move = relf(first(A * (1 + 1e-15 * rng.standard_normal(A.shape))), K1)
    bar = max(10 * move, 1e-10)
    err = relf(K1, K)
    print(f"\np = {p}, N = {N}: first move vs K {err:.2e} (moves {move:.2e}, bar {bar:.2e})")
    assert err <= bar


def test_newton_refinement_of_the_riccati_solution():
    """lqr.dare_refine on a problem like the lifted models (spectral radius of A just above 1): the relative Riccati residual
    falls to 1e-12 or below and does not grow with further steps, and the first move of the condensed problem is the refined
    gain to 1e-11."""
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(3)
    A, B = _stable(rng, 30, 1, 1.005)
    Cm = rng.standard_normal((2, 30))
    Q, R = Cm.T @ Cm, np.eye(1)
    K0, P0 = lqr.dlqr(A, B, Q, R)

    def residual(P):
        return relf(A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A) + Q, P)

    K, P = lqr.dare_refine(A, B, Q, R, K0)
    H, F = lqr.mpc_condense(A, B, Q, R, P, 12)
    first = relf(np.linalg.solve(H, F)[:1], K)
    print(f"\nRiccati residual {residual(P0):.2e} -> {residual(P):.2e}; first move vs refined gain {first:.2e}; gain moved {relf(K, K0):.2e}")
    assert residual(P) <= max(1e-12, residual(P0)) and first <= 1e-11 and relf(K, K0) <= 1e-6
    assert np.max(np.abs(np.linalg.eigvals(A - B @ K))) < 1.0


def problems():
    """name -> the two problems of tests 3 and 5.  'two': two inputs, N = 8 (nv = 16), the box at 0.4 of the largest
    unconstrained move: 3 bounds active at the solution.  'rate': one input, N = 20 (nv = 20), the box at 0.5 of the largest
    unconstrained move, rates at 15 % of the box per step, u_prev = 0.3 of the box."""
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(11)
    out = {}
    for name, p, N, nc in (("two", 2, 8, 3), ("rate", 1, 20, 2)):
        A, B = _stable(rng, 12, p, 0.95)
        Cm = rng.standard_normal((nc, 12))
        Q, R = 100 * Cm.T @ Cm, np.eye(p)
        K, P = lqr.dlqr(A, B, Q, R)
        H, F = lqr.mpc_condense(A, B, Q, R, P, N)
        e = rng.standard_normal(12)
        free = -np.linalg.solve(H, F @ e)
        if name == "two":
            bound = 0.4 * np.max(np.abs(free))
            bnd, u_prev = lqr.mpc_bounds(N * p, -bound, bound), np.zeros(p)
        else:
            bound = 0.5 * np.max(np.abs(free))
            bnd, u_prev = lqr.mpc_bounds(N * p, -bound, bound, -0.15 * bound, 0.15 * bound), np.array([0.3 * bound])
        out[name] = dict(H=H, F=F, K=K, e=e, p=p, N=N, bnd=bnd, bound=bound, u_prev=u_prev, rho=lqr.mpc_default_rho(H))
    return out


def _exact(pr):
    """bvls on the Cholesky factor (bounds only) or trust-constr with a LinearConstraint (bounds and rates)."""
    H, g, p = pr["H"], pr["F"] @ pr["e"], pr["p"]
    lo, hi, dlo, dhi = pr["bnd"]
    nv = g.size
    L = np.linalg.cholesky(H)
    if np.all(np.isinf(dlo)):
        return scipy.optimize.lsq_linear(L.T, -scipy.linalg.solve_triangular(L, g, lower=True), bounds=(lo, hi), method="bvls",
                                         tol=1e-15).x
    D = np.eye(nv) - np.eye(nv, k=-p)
    sh = np.zeros(nv)
    sh[:p] = pr["u_prev"]
    res = scipy.optimize.minimize(lambda U: 0.5 * U @ H @ U + g @ U, np.zeros(nv), jac=lambda U: H @ U + g, hess=lambda U: H,
                                  method="trust-constr", bounds=scipy.optimize.Bounds(lo, hi),
                                  constraints=[scipy.optimize.LinearConstraint(D, dlo + sh, dhi + sh)],
                                  options=dict(gtol=1e-13, xtol=1e-14, barrier_tol=1e-14, maxiter=5000))
    return res.x


@pytest.mark.parametrize("name", ["two", "rate"])
def test_admm_against_exact_solvers(name):
    """lqr.mpc_solve against scipy's exact solvers.  iters = 200, chosen on the CPU so that the NumPy iteration is within 1e-8
    of the bound: it reached 1.6e-9 of the bound on 'two' (cond(H) = 21.7; 1.3e-7 after 150 iterations) and 1.2e-11 on 'rate'
    (cond(H) = 4.6; trust-constr's own accuracy -- the iteration stands still from 150 iterations on)."""
    from nys_koop_lqr_amd import lqr
    pr = problems()[name]
    want = _exact(pr)
    u, z, (k, r) = lqr.mpc_solve(pr["H"], pr["F"] @ pr["e"], *pr["bnd"], pr["u_prev"], pr["rho"], ITERS, p=pr["p"])
    lo, hi, dlo, dhi = pr["bnd"]
    active = int(np.sum(np.abs(want - lo) < 1e-9 * pr["bound"]) + np.sum(np.abs(want - hi) < 1e-9 * pr["bound"]))
    dist = np.max(np.abs(z - want)) / pr["bound"]
    print(f"\n[{name}] {k} iterations, residual {r:.2e}: distance {dist:.2e} of the bound; {active} bounds active")
    assert k == ITERS and dist <= 1e-8
    assert active >= 1 or name == "rate"
    p = pr["p"]
    assert np.all(u >= lo[:p]) and np.all(u <= hi[:p])
    assert np.all(u >= pr["u_prev"] + dlo[:p]) and np.all(u <= pr["u_prev"] + dhi[:p])
    assert np.max(np.abs(u - want[:p])) <= 1e-8 * pr["bound"]


def test_feasible_start_is_returned_after_no_iteration():
    """Bounds wider than the unconstrained solution: 0 iterations at tol = 1e-12 (and at tol = 0), z is U_unc, the control its
    first move."""
    from nys_koop_lqr_amd import lqr
    pr = problems()["rate"]
    g = pr["F"] @ pr["e"]
    free = -np.linalg.solve(pr["H"], g)
    big = 10 * np.max(np.abs(free))
    bnd = lqr.mpc_bounds(g.size, -big, big, -2 * big, 2 * big)
    for tol in (1e-12, 0.0):
        u, z, (k, r) = lqr.mpc_solve(pr["H"], g, *bnd, None, pr["rho"], 50, tol, p=1)
        assert k == 0 and r == 0.0 and relf(z, free) <= 1e-13 and u[0] == z[0]
    inf = lqr.mpc_bounds(g.size)
    u, z, (k, r) = lqr.mpc_solve(pr["H"], g, *inf, None, pr["rho"], 50, p=1)
    assert k == 0 and r == 0.0 and u[0] == z[0]


def test_saturated_mode_and_controller_object():
    """iters = 0 is the clip formula on -K e; MPCController pickles and gives the same controls."""
    from nys_koop_lqr_amd import lqr
    pr = problems()["rate"]
    lo, hi, dlo, dhi = pr["bnd"]
    ctl = lqr.MPCController(pr["H"], pr["F"], lo, hi, dlo, dhi, pr["K"], pr["rho"], pr["N"])
    u, info = ctl.control(pr["e"], pr["u_prev"], iters=0)
    v = -(pr["K"] @ pr["e"])
    want = np.clip(np.clip(v, lo[:1], hi[:1]), pr["u_prev"] + dlo[:1], pr["u_prev"] + dhi[:1])
    assert np.array_equal(u, want) and info == (0, 0.0)
    u1, info1 = ctl.control(pr["e"], pr["u_prev"], iters=ITERS)
    other = pickle.loads(pickle.dumps(ctl))
    assert other._mats is None and other.horizon == pr["N"] and other.nv == 20 and other.n_inputs == 1
    u2, info2 = other.control(pr["e"], pr["u_prev"], iters=ITERS)
    assert np.array_equal(u1, u2) and info1 == info2


# ---- the library's host build ---------------------------------------------------------------------------------------------
def _desc(pr, iters, tol_=0.0, **over):
    """(MpcDesc, keep-alive) of a problem; over: fields to replace (arrays or scalars)."""
    from nys_koop_lqr_amd import _lib
    lo, hi, dlo, dhi = pr["bnd"]
    f = dict(N=pr["N"], p=pr["p"], m=pr["e"].size, iters=iters, H=pr["H"], F=pr["F"], lo=lo, hi=hi, dlo=dlo, dhi=dhi, K=pr["K"],
             rho=pr["rho"], tol=tol_)
    f.update(over)
    ds, keep = _lib.MpcDesc(), []
    for k, v in f.items():
        if k in ("N", "p", "m", "iters", "rho", "tol"):
            setattr(ds, k, v)
        elif v is None:
            setattr(ds, k, None)
        else:
            a = np.ascontiguousarray(v, dtype=np.float64)
            keep.append(a)
            setattr(ds, k, a.ctypes.data)
    return ds, keep, f


def _qp_host(lib, pr, iters, tol_=0.0, **over):
    ds, keep, f = _desc(pr, iters, tol_, **over)
    nv, p = pr["N"] * pr["p"], pr["p"]
    u, z, info = np.full(p, 7.0), np.full(nv, 7.0), np.full(2, 7.0)
    e, up = np.ascontiguousarray(pr["e"]), np.ascontiguousarray(pr["u_prev"])
    rc = lib.nk_mpc_qp_host(C.byref(ds), e.ctypes.data, up.ctypes.data, u.ctypes.data, z.ctypes.data, info.ctypes.data)
    return rc, u, z, info


@pytest.mark.parametrize("name", ["two", "rate"])
def test_library_host_build_against_the_numpy_statement(lib, name):
    """nk_mpc_qp_host against lqr.mpc_solve on the problems of the exact-solver test: 1e-13 relative on z and u after 200
    iterations and after 7, the same iteration count and residual; tol > 0 stops both at the same iteration; iters = 0 gives the
    clip formula."""
    from nys_koop_lqr_amd import lqr
    pr = problems()[name]
    g = pr["F"] @ pr["e"]
    for iters, tol in ((ITERS, 0.0), (7, 0.0), (ITERS, 1e-6 * pr["bound"])):
        rc, u, z, info = _qp_host(lib, pr, iters, tol)
        assert rc == 0, lib.nk_last_error().decode()
        u2, z2, (k, r) = lqr.mpc_solve(pr["H"], g, *pr["bnd"], pr["u_prev"], pr["rho"], iters, tol, p=pr["p"])
        e_z, e_u = relf(z, z2), relf(u, u2)
        print(f"\n[{name}] iters {iters}, tol {tol:.1e}: {int(info[0])} iterations, z {e_z:.2e}, u {e_u:.2e}, residual {info[1]:.2e} / {r:.2e}")
        assert e_z <= 1e-13 and e_u <= 1e-13 and info[0] == k
        assert abs(info[1] - r) <= 1e-13 * pr["bound"]
        if tol > 0:
            assert 0 < k < iters and r <= tol
    rc, u, z, info = _qp_host(lib, pr, 0)
    u2, _, _ = lqr.mpc_solve(None, None, *pr["bnd"], pr["u_prev"], pr["rho"], 0, p=pr["p"], K_e=pr["K"] @ pr["e"])
    assert rc == 0 and relf(u, u2) <= 1e-13 and np.all(z == 7.0) and np.all(info == 0.0)


def _malformed(pr):
    """(label, fields to replace, iters, what the message must name)"""
    nv = pr["N"] * pr["p"]
    lo, hi, dlo, dhi = pr["bnd"]

    def at(a, i, v):
        b = np.array(a, dtype=np.float64)
        b.flat[i] = v
        return b

    Hns = at(pr["H"], 1, pr["H"].flat[1] * 1.5)
    Hneg = pr["H"] - 2 * np.max(np.linalg.eigvalsh(pr["H"])) * np.eye(nv)
    return [("p = 0", dict(p=0), 5, "p ="), ("p = 5", dict(p=5), 5, "p ="), ("N = 0", dict(N=0), 5, "N ="),
            ("nv = 65", dict(N=65, p=1), 5, "nv"), ("nv = 68", dict(N=17, p=4), 5, "nv"), ("m = 0", dict(m=0), 5, "m ="),
            ("iters = -1", dict(), -1, "iters"), ("rho = 0", dict(rho=0.0), 5, "rho"), ("rho < 0", dict(rho=-1.0), 5, "rho"),
            ("rho nan", dict(rho=float("nan")), 5, "rho"), ("rho inf", dict(rho=float("inf")), 5, "rho"),
            ("tol < 0", dict(tol=-1e-3), 5, "tol"), ("tol nan", dict(tol=float("nan")), 5, "tol"),
            ("lo > hi", dict(lo=at(lo, 3, hi[3] + 1.0)), 5, "lo[3]"), ("lo nan", dict(lo=at(lo, 2, np.nan)), 5, "lo[2]"),
            ("hi = -inf", dict(hi=at(hi, 0, -np.inf)), 5, "hi[0]"),
            ("dlo > dhi", dict(dlo=np.full(nv, 1.0), dhi=np.full(nv, 0.5)), 5, "dlo[0]"),
            ("dhi nan", dict(dhi=at(np.full(nv, 1.0), 4, np.nan)), 5, "dhi[4]"),
            ("H null", dict(H=None), 5, "H is null"), ("F null", dict(F=None), 5, "F is null"),
            ("K null, iters = 0", dict(K=None), 0, "K is null"), ("H nan", dict(H=at(pr["H"], 5, np.nan)), 5, "H is not finite"),
            ("F inf", dict(F=at(pr["F"], 5, np.inf)), 5, "F is not finite"),
            ("K nan, iters = 0", dict(K=at(pr["K"], 1, np.nan)), 0, "K is not finite"),
            ("H not symmetric", dict(H=Hns), 5, "H is not symmetric"), ("H not positive definite", dict(H=Hneg), 5, "H is not positive definite")]


def test_every_validation_rule(lib):
    """Each malformed description is NK_ERR_BAD_ARG with the field in nk_last_error(), the outputs keep their canary, and the
    valid description still solves afterwards."""
    pr = problems()["two"]
    for label, over, iters, names in _malformed(pr):
        rc, u, z, info = _qp_host(lib, pr, iters, **over)
        msg = lib.nk_last_error().decode()
        assert rc == -1 and names in msg and "nk_mpc_qp_host" in msg, (label, rc, msg)
        assert np.all(u == 7.0) and np.all(z == 7.0) and np.all(info == 7.0), label
    assert lib.nk_mpc_qp_host(None, pr["e"].ctypes.data, None, pr["e"].ctypes.data, None, None) == -1
    ds, keep, _ = _desc(pr, 5)
    assert lib.nk_mpc_qp_host(C.byref(ds), None, None, pr["e"].ctypes.data, None, None) == -1
    rc, u, z, info = _qp_host(lib, pr, 5)
    assert rc == 0 and info[0] == 5 and np.all(np.abs(u) <= pr["bound"])
    assert lib.nk_mpc_loop_max_m(64) == 314 and lib.nk_mpc_loop_max_m(38) == 512 and lib.nk_mpc_loop_max_m(39) == 511
    assert lib.nk_mpc_loop_max_m(65) == 0 and lib.nk_mpc_loop_max_m(0) == 0


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mpc_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("mpc") / "mpc_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mpc_main.cpp"), "-o", exe]
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
            _, _, f = _desc(pr, iters, tol, **over)
            arrays = [f[k] for k in ("H", "F", "lo", "hi", "dlo", "dhi", "K")] + [pr["e"], pr["u_prev"]]
            arrays = [np.zeros(0) if a is None else np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]
            lines.append(f"{f['N']} {f['p']} {f['m']} {f['iters']} {num(f['rho'])} {num(f['tol'])}")
            lines.append(" ".join(str(a.size) for a in arrays))
            lines += [" ".join(num(v) for v in a) for a in arrays if a.size]
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = res.stdout.splitlines()
        assert len(out) == len(cases), out
        return out

    return run


def test_sanitized_program_solves_and_rejects_every_malformed_description(lib, mpc_program):
    """The header alone, compiled by the host compiler with -fsanitize=address,undefined: the problems of the exact-solver
    test (200 iterations, 7, an early stop, the saturated mode) give the library's bits, every malformed description is
    rejected with the library's message, and nothing is read or written out of bounds on the way."""
    prs = problems()
    good = [(prs[n], iters, tol, {}) for n in ("two", "rate") for iters, tol in ((ITERS, 0.0), (7, 0.0), (ITERS, 1e-6), (0, 0.0))]
    bad = _malformed(prs["two"])
    out = mpc_program(good + [(prs["two"], iters, 0.0, over) for _, over, iters, _ in bad])
    for line, (pr, iters, tol, _) in zip(out, good):
        rc, u, z, info = _qp_host(lib, pr, iters, tol)
        assert rc == 0 and line.startswith("ok "), line
        got = [np.array([float.fromhex(t) for t in part.split()]) for part in line[3:].split("|")]
        assert np.array_equal(got[0], u) and np.array_equal(got[2], info), (line, u, info)
        assert np.array_equal(got[1], z) if iters > 0 else got[1].size == 0
    for line, (label, _, _, names) in zip(out[len(good):], bad):
        assert line.startswith("bad ") and names in line, (label, line)
