"""The augmented blocked Cholesky (nk_chol_aug = cholesky_aug_pair_async + cholesky_fail_flags, as every fit calls them)
against an outside answer: residuals formed in NumPy longdouble, LAPACK potrf / cho_solve as the comparison solver
(tests/chol_reference.py).  Every case runs the tile-dataflow launch and the launch-per-step chain, checks through the
runtime counters that the launch was / was not taken, and requires the same bits from both.

Two bars, kept apart:
  cap  -- derived: factor residual ||L L^T - P||_F / ||P||_F and solve backward error ||X P - R||_F / (||P||_F ||X||_F) at
          most m eps (Higham, Thm 10.3 / 10.4, normwise).  test_chol_reference_host.py holds LAPACK to it on the CPU first.
  bar  -- relative to LAPACK, from the reference alone: 2 x the worst of LAPACK's own values over the matrix and 4 random
          symmetric permutations of it, floored at 1 eps.

Measured on one MI355X (profiles/r05_chol_accuracy.log, 23 systems, units of eps = 2^-52; LAPACK's spread over the
permutations is at most 0.08 eps):
  factor residual        GPU 0.83 .. 1.54     LAPACK 0.55 .. 2.80    (GPU / LAPACK 0.41 .. 1.67; the random family, where LAPACK
                                                                      sits at 0.55 .. 0.76, is the one above 1: GPU 0.83 .. 0.94,
                                                                      under the bar's 1 eps floor x 2)
  solve backward error   GPU 0.07 .. 0.14     LAPACK 0.06 .. 0.14    (all far below the 1 eps floor of the bar)
No case lies between the bar and the cap.

This file starts where the dataflow launch starts (m >= 256) and runs the chain there only under NYSKOOP_CHOL_FLOW=0.  Where
the chain runs in production -- every system below 256, every call of a lock-step member at any size -- and the plain factor
with its two-sided substitution (nk_solve_spd) are held to the same two bars in tests/test_gpu_chol_small.py."""
import os

import numpy as np
import pytest

import chol_reference as cr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not cr.HAVE_LONGDOUBLE, reason=cr.LONGDOUBLE_SKIP)]

CHOL_FIX_KAPPA = cr.CHOL_FIX_KAPPA

# (m, extra, family, ld).  Every m of {256, 257, 319, 320, 321, 384, 705, 1025} (the first size that takes the launch, one row
# into a new tile, an exact tile multiple, ...) and every extra of {1, 63, 64, 65, m, m + 3} appears; ld > m three times.
SINGLE = [
    (256, 1, "random", 256),
    (256, 259, "graded", 256),
    (257, 63, "graded", 264),
    (257, 64, "rbf", 257),
    (319, 64, "random", 319),
    (320, 65, "rbf", 320),
    (320, 320, "graded", 320),
    (321, 1, "rbf", 328),
    (321, 324, "random", 321),
    (384, 63, "rbf", 384),
    (384, 65, "graded", 384),
    (705, 65, "random", 705),
    (705, 63, "graded", 712),
    (1025, 64, "rbf", 1025),
]
# graded spectra whose leading diagonal blocks exceed CHOL_FIX_KAPPA (the correction step of the products with the inverted
# blocks fires); under a random basis a 64 x 64 block of a larger matrix is conditioned better, so not the larger ones
GRADED_FIRES = {256, 257}

# two systems in one launch, sized as the fits pair them: (m + p, extra m) beside (m, extra d)
PAIRS = [
    (256, 6, 40, "rbf", "random"),   # 5 tile columns beside 4
    (256, 1, 3, "graded", "rbf"),
    (320, 0, 24, "random", "graded"),
    (700, 3, 384, "rbf", "random"),
]


@pytest.fixture(scope="module")
def ctx():
    import nys_koop_lqr_amd as nk
    return nk.get_context()


def _log(line):
    print(line)
    path = os.environ.get("NYSKOOP_CHOL_ACC_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _both_paths(ctx, monkeypatch, systems):
    """nk_chol_aug with the dataflow launch and with the chain: same bits; the counters prove which ran."""
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "1")
    c0 = cr.counters()
    flow = cr.chol_aug(ctx, systems)
    c1 = cr.counters()
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "0")
    chain = cr.chol_aug(ctx, systems)
    c2 = cr.counters()
    monkeypatch.delenv("NYSKOOP_CHOL_FLOW")
    assert c1[6] == c0[6] + 1 and c2[6] == c1[6], (c0, c1, c2)  # one dataflow launch, then none
    assert c2[5] == c0[5]                                       # nobody gave up
    for (L1, X1, f1, r1), (L0, X0, f0, r0) in zip(flow, chain):
        assert f1 == f0 and r1 == r0
        # (the strict upper triangle inside a diagonal tile is scratch, see include/nyskoop.h: the factor is the lower triangle)
        assert np.array_equal(np.tril(L1), np.tril(L0)) and np.array_equal(X1, X0)
    for (P, _, _), (L0, _, _, _) in zip(systems, chain):  # (_check holds the dataflow launch's L to the same)
        assert cr.upper_tiles_untouched(L0, P)
    return flow


def _check(tag, m, extra, family, seed, P, R, L, X, failed):
    """Both bars on one factored and solved system.  cr.caps(m) is (cap(m), cap(m)) from m = 5 up, and the bar relative to
    LAPACK applies from there (tests/test_gpu_chol_small.py goes below)."""
    assert failed == 0, failed
    assert np.isfinite(np.tril(L)).all() and np.isfinite(X).all()
    # the contract of the returned L: tiles above the block diagonal are never written
    assert cr.upper_tiles_untouched(L, P)
    fr, be = cr.factor_residual(L, P), cr.solve_backward_error(X, P, R)
    lfr, lbe = cr.lapack_reference(family, m, seed, extra)
    cap_f, cap_s = cr.caps(m)
    e = cr.EPS
    _log(f"{tag} m={m} extra={extra} family={family} factor: gpu {fr / e:.3f} lapack {lfr[0] / e:.3f} "
         f"(perms {min(lfr) / e:.3f}..{max(lfr) / e:.3f}) bar {cr.lapack_bar(lfr) / e:.3f} | solve: gpu {be / e:.3f} "
         f"lapack {lbe[0] / e:.3f} (perms {min(lbe) / e:.3f}..{max(lbe) / e:.3f}) bar {cr.lapack_bar(lbe) / e:.3f} | cap "
         + (f"{m}" if m >= 5 else f"{cap_f / e:.0f} factor, {cap_s / e:.0f} solve (m < 5: no bar relative to LAPACK)"))
    assert fr <= cap_f and be <= cap_s, (fr / e, be / e, m)
    if m >= 5:
        assert fr <= cr.lapack_bar(lfr), (fr / e, [v / e for v in lfr])
        assert be <= cr.lapack_bar(lbe), (be / e, [v / e for v in lbe])


@pytest.mark.parametrize("m,extra,family,ld", SINGLE)
def test_single_system(ctx, monkeypatch, m, extra, family, ld):
    seed = m
    P, R = cr.matrix(family, m, seed), cr.rhs(extra, m, seed)
    if family == "graded" and m in GRADED_FIRES:
        kappa = cr.diag_block_kappa(P)
        assert max(kappa) > CHOL_FIX_KAPPA and min(kappa) < CHOL_FIX_KAPPA
    (L, X, failed, ratio), = _both_paths(ctx, monkeypatch, [(P, R, ld)])
    assert 0.0 < ratio <= 1.0
    _check("single", m, extra, family, seed, P, R, L, X, failed)


@pytest.mark.parametrize("m,p,d,fam0,fam1", PAIRS)
def test_paired_systems(ctx, monkeypatch, m, p, d, fam0, fam1):
    s0, s1 = 1000 + m + p, 2000 + m
    P0, R0 = cr.matrix(fam0, m + p, s0), cr.rhs(m, m + p, s0)
    P1, R1 = cr.matrix(fam1, m, s1), cr.rhs(d, m, s1)
    out = _both_paths(ctx, monkeypatch, [(P0, R0, m + p), (P1, R1, m)])
    _check("pair0", m + p, m, fam0, s0, P0, R0, *out[0][:3])
    _check("pair1", m, d, fam1, s1, P1, R1, *out[1][:3])


# m = 321: six tile columns, the last one a single row.  The failure word is LAPACK potrf's `info`: index + 1 of the first
# non-positive pivot.
@pytest.mark.parametrize("j", [5, 320], ids=["first_tile", "last_tile"])
def test_first_nonpositive_pivot_is_lapack_info(ctx, monkeypatch, j):
    import scipy.linalg as sla
    m = 321
    P = cr.indefinite(m, j, seed=11)
    assert (np.linalg.eigvalsh(P) < 0).sum() == 1
    _, info = sla.lapack.dpotrf(P, lower=1)
    assert info == j + 1
    (_, _, failed, ratio), = _both_paths(ctx, monkeypatch, [(P, cr.rhs(64, m, 11), m)])
    assert failed == info and ratio == 0.0


def test_indefinite_system_beside_a_good_one(ctx, monkeypatch):
    """The failure word belongs to its own system: the other system of the pair factors and solves as if alone."""
    m = 321
    bad = cr.indefinite(m, 320, seed=11)
    P1, R1 = cr.matrix("rbf", 256, 5), cr.rhs(40, 256, 5)
    out = _both_paths(ctx, monkeypatch, [(bad, cr.rhs(64, m, 11), m), (P1, R1, 256)])
    assert out[0][2] == 321
    _check("beside-indefinite", 256, 40, "rbf", 5, P1, R1, *out[1][:3])
