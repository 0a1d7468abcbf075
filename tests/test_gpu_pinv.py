"""The Jacobi pseudo-inverse (nk_pinv.hip, entered through nk_solve_spd with NYSKOOP_FORCE_PINV=1) against an outside answer,
on every kernel of pinv_right_divide's dispatch and on every branch of the singular-value cut-off.  Measures formed in NumPy
longdouble and LAPACK's SVD as the comparison solver: tests/pinv_reference.py; test_pinv_reference_host.py holds LAPACK to the
same caps on the CPU first.

Which sizes reach which kernel (pinv_reference.INT_CASES / SCALAR_CASES / FULL_CASES):
  no sweep                  m = 1
  jacobi_round_wave_kernel  m = 2, 3 by default; m = 130 with NYSKOOP_PINV_BLOCK=0
  jacobi_block8_kernel      m = 4, 9, 17, 64, 511, 512; 70 (cut-off cases); 130 (full rank, and beside the scalar run)
  jacobi_block4_kernel      m = 513, 520
  jacobi_block2_kernel      m = 1025, 1028
  jacobi_round_kernel       m = 520 with NYSKOOP_PINV_BLOCK=0 (what every m > 2048 runs by default)
  jacobi_sweep_kernel       not run here: with the block kernels as default nothing outside a lock-step group reaches it

Caps, derived from the stopping criterion (every pair of columns orthogonal to tol = max(m, 64) eps), never from the GPU:
  e_ls, full-rank backward error   <= cap_ls = m tol
  e_null                           <= kappa_r cap_ls
  relf(X, LAPACK's X)              <= 2 kappa_r cap_ls     (full rank: 2 cond(P) cap_ls against numpy.linalg.solve)
Cut-off cases (diagonal P, so every decision is deterministic): dropped rows are exactly 0.0, kept rows R / sigma to 5 eps.

Every case logs its figures in units of eps = 2^-52 (stdout, and the file named by NYSKOOP_PINV_ACC_LOG): family, m, rank,
kernel, sweeps, the GPU's measures, LAPACK's over three orderings, the caps, and -- not asserted -- the expectation
(tol / eps) x chol_reference.lapack_bar(LAPACK's values).  lapack_bar already holds the project's factor 2 over LAPACK's worst
ordering; it is taken once, the stricter reading of "2 (tol / eps) times lapack_bar".  A line ends with
ABOVE-EXPECTATION(<measure>) where the GPU lies between the expectation and the cap.

Measured on one MI355X (profiles/pinv_accuracy.log, 58 lines, units of eps; LAPACK on the same systems in brackets):
  e_ls                     round_wave 0.04 .. 4.93, block8 0.00 .. 17.06, block4 0.12 .. 13.64, block2 0.07 .. 15.25,
                           round 0.09 .. 9.54                                      (LAPACK 0.00 .. 1.55)
  e_null / kappa_r         0.00 .. 2.32 over all kernels                           (LAPACK 0.00 .. 13.28)
  forward / kappa_r        0.00 .. 297.7, largest at m = 1028, rank 342; its cap there is 2.1e6
  full-rank backward error 22.5 .. 44.3 at m = 130, 126.9 .. 247.6 at m = 513      (LAPACK 0.15 .. 0.50)
  sweeps                   at most 32 (m = 512), 29 for the graded family at m = 130
  cut-off cases            ranks 60 / 60 / 63 / 32 / 40 as prescribed, kept rows within 1.000 eps of R / sigma
No line carries ABOVE-EXPECTATION: no case lies between the expectation and the cap.  Nearest to its expectation are the
full-rank backward errors (rbf at m = 513: 248 of 1026; graded at m = 130: 44 of 260); e_ls stays below 1/60 of it from
m = 511 on.  At m = 1 and 2 the expectation's floor (128 eps) is not below the cap (64 and 128 eps), so there the cap is the
tighter of the two.  The longest case takes 1.3 s (m = 1028, rank 342), so both m >= 1025 sizes are kept."""
import os
import re

import numpy as np
import pytest

import pinv_reference as pr
from chol_reference import lapack_bar

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason=pr.LONGDOUBLE_SKIP)]

SCALAR_ENV = {"NYSKOOP_PINV_BLOCK": "0", "NYSKOOP_PINV_SWEEP_LAUNCH": "0"}
_RANK_LINE = re.compile(r"\[nk pinv\] rank (\d+) of (\d+), .* (\d+) sweeps")
_SWEEP_LINE = re.compile(r"\[nk pinv\] m=(\d+) sweep (\d+): (\d+) rotations")


@pytest.fixture(scope="module")
def ctx():
    import nys_koop_lqr_amd as nk
    return nk.get_context()


def _log(line):
    print(line)
    path = os.environ.get("NYSKOOP_PINV_ACC_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _solve(ctx, monkeypatch, capfd, P, R, pad=0, env=None):
    """X through the SVD path, the sweep count and the rank of the trace.  The switches are read per call."""
    m = P.shape[0]
    monkeypatch.setenv("NYSKOOP_FORCE_PINV", "1")
    monkeypatch.setenv("NYSKOOP_PINV_TRACE", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    X = pr.solve(ctx, P, R, ldp=m + pad)
    err = capfd.readouterr().err
    for k in ["NYSKOOP_FORCE_PINV", "NYSKOOP_PINV_TRACE"] + list(env or {}):
        monkeypatch.delenv(k)
    (rank, of, sweeps), = _RANK_LINE.findall(err)
    assert int(of) == m
    per_sweep = _SWEEP_LINE.findall(err)
    assert len(per_sweep) == int(sweeps) and all(int(mm) == m for mm, _, _ in per_sweep)
    if m > 1:
        assert int(per_sweep[-1][2]) == 0  # the last sweep found nothing left to rotate
    assert int(sweeps) < pr.MAX_SWEEPS
    return X, int(sweeps), int(rank)


def _expect(m, values):
    """Not asserted: LAPACK's bar (2 x its worst ordering, floored at 1 eps) scaled by tol / eps, how much looser the Jacobi
    stopping criterion is than LAPACK's.  The factor 2 is the one inside lapack_bar, taken once: the stricter reading."""
    return pr.jacobi_tol(m) / pr.EPS * lapack_bar(values)


def _mark(measure, value, expect):
    return f"  ABOVE-EXPECTATION({measure})" if value > expect else ""


def _check_int(kernel, m, rank, nrhs, pad, X, sweeps, traced_rank):
    P, B, kappa = pr.int_lowrank(m, rank, m)
    R = pr.int_rhs(m, nrhs, m)
    Xl, lls, lnull = pr.lapack_reference(m, rank, m, nrhs)
    assert X.shape == (m, nrhs) and np.isfinite(X).all()
    assert traced_rank == rank
    els, enull, fwd = pr.e_ls(X, P, R), pr.e_null(X, B), pr.relf(X, Xl)
    e = pr.EPS
    x_ls, x_null = _expect(m, lls), _expect(m, lnull)
    _log(f"int m={m} rank={rank} nrhs={nrhs} pad={pad} kernel={kernel} sweeps={sweeps} kappa_r={kappa:.3g} | "
         f"e_ls: gpu {els / e:.3f} lapack {min(lls) / e:.3f}..{max(lls) / e:.3f} expect {x_ls / e:.0f} cap {pr.cap_ls(m) / e:.0f} | "
         f"e_null/kappa_r: gpu {enull / e / kappa:.3f} lapack {min(lnull) / e / kappa:.3f}..{max(lnull) / e / kappa:.3f} "
         f"expect/kappa_r {x_null / e / kappa:.0f} cap/kappa_r {pr.cap_null(m, kappa) / e / kappa:.0f} | "
         f"forward/kappa_r: gpu {fwd / e / kappa:.3f} cap/kappa_r {pr.cap_forward(m, kappa) / e / kappa:.0f} (no expectation)"
         f"{_mark('e_ls', els, x_ls)}{_mark('e_null', enull, x_null)}")
    assert els <= pr.cap_ls(m), (els / e, pr.cap_ls(m) / e)
    assert enull <= pr.cap_null(m, kappa), (enull / e, pr.cap_null(m, kappa) / e)
    assert fwd <= pr.cap_forward(m, kappa), (fwd / e, pr.cap_forward(m, kappa) / e)
    return fwd


# ---- a. integer low-rank, default dispatch
@pytest.mark.parametrize("m,rank,nrhs,pad", pr.INT_CASES)
def test_integer_lowrank(ctx, monkeypatch, capfd, m, rank, nrhs, pad):
    P, _, _ = pr.int_lowrank(m, rank, m)
    X, sweeps, traced = _solve(ctx, monkeypatch, capfd, P, pr.int_rhs(m, nrhs, m), pad)
    assert sweeps == 0 if m == 1 else sweeps >= 1
    _check_int(pr.kernel_of(m), m, rank, nrhs, pad, X, sweeps, traced)


# ---- b. full rank through the SVD path
@pytest.mark.parametrize("family,m,nrhs,pad", pr.FULL_CASES)
def test_full_rank(ctx, monkeypatch, capfd, family, m, nrhs, pad):
    P, R = pr.matrix(family, m, m), pr.int_rhs(m, nrhs, m)
    Xs, cond, lbe = pr.lapack_reference_full(family, m, m, nrhs)
    X, sweeps, traced = _solve(ctx, monkeypatch, capfd, P, R, pad)
    assert np.isfinite(X).all() and traced == m
    be, fwd = pr.backward_error(X, P, R), pr.relf(X, Xs)
    e, x_be = pr.EPS, _expect(m, lbe)
    _log(f"full family={family} m={m} nrhs={nrhs} pad={pad} kernel={pr.kernel_of(m)} sweeps={sweeps} cond={cond:.3g} | "
         f"backward: gpu {be / e:.3f} lapack {min(lbe) / e:.3f}..{max(lbe) / e:.3f} expect {x_be / e:.0f} cap {pr.cap_ls(m) / e:.0f} | "
         f"forward/cond: gpu {fwd / e / cond:.4f} cap/cond {2 * pr.cap_ls(m) / e:.0f} (no expectation){_mark('backward', be, x_be)}")
    assert be <= pr.cap_ls(m), (be / e, pr.cap_ls(m) / e)
    assert fwd <= 2.0 * cond * pr.cap_ls(m), (fwd, 2.0 * cond * pr.cap_ls(m))


# ---- c. the scalar rounds, and block against scalar on the same system
@pytest.mark.parametrize("m,rank,nrhs,pad", pr.SCALAR_CASES)
def test_scalar_kernels(ctx, monkeypatch, capfd, m, rank, nrhs, pad):
    P, _, kappa = pr.int_lowrank(m, rank, m)
    R = pr.int_rhs(m, nrhs, m)
    kernel = pr.kernel_of(m, block=False)
    assert kernel == ("round_wave" if m == 130 else "round")
    Xs, sweeps, traced = _solve(ctx, monkeypatch, capfd, P, R, pad, SCALAR_ENV)
    _check_int(kernel, m, rank, nrhs, pad, Xs, sweeps, traced)
    Xb, sweeps_b, traced_b = _solve(ctx, monkeypatch, capfd, P, R, pad)
    _check_int(pr.kernel_of(m), m, rank, nrhs, pad, Xb, sweeps_b, traced_b)
    assert pr.relf(Xs, Xb) <= 2 * pr.cap_forward(m, kappa)  # the sum of their forward bounds


# ---- d. the cut-off rule
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("name", pr.DIAG_CASES)
def test_cutoff_rule(ctx, monkeypatch, capfd, name, pad):
    P, s, rcond, keep, rank, _ = pr.diag_case(name)
    m = pr.DIAG_M
    R = np.ones((m, 2))
    env = {"NYSKOOP_PINV_RCOND": "1e-2"} if name == "rcond" else {}
    assert (rcond == 1e-2) == bool(env) and (env or rcond == pr.EPS)
    X, sweeps, traced = _solve(ctx, monkeypatch, capfd, P, R, pad, env)
    nonzero = (X != 0.0).any(axis=1)
    _log(f"diag case={name} m={m} pad={pad} kernel={pr.kernel_of(m)} sweeps={sweeps} rank: want {rank} trace {traced} "
         f"non-zero rows {int(nonzero.sum())} | kept rows: max |X sigma - 1| {np.abs(X[keep] * s[keep, None] - 1.0).max() / pr.EPS:.3f} cap 5")
    assert np.isfinite(X).all()
    assert (X[~keep] == 0.0).all()  # a dropped direction contributes exactly nothing
    # at most four roundings on the way: sigma^2, its reciprocal, two products
    assert (np.abs(X[keep] - 1.0 / s[keep, None]) <= 5 * pr.EPS / s[keep, None]).all()
    assert int(nonzero.sum()) == rank and np.array_equal(nonzero, keep)
    assert traced == rank
    assert sweeps == 1  # a diagonal matrix has nothing to rotate
