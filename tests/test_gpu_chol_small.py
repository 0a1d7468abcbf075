"""The launch-per-step chain of the augmented blocked Cholesky where it runs in production -- every system below m = 256 on an
ordinary context, every call of a lock-step member at any size (the `_batched` twins of its kernels) -- and the plain factor
with its two-sided substitution (nk_solve_spd), against the outside answer of tests/chol_reference.py: residuals formed in
NumPy longdouble, LAPACK potrf / cho_solve as the comparison solver.  tests/test_gpu_chol_accuracy.py covers m >= 256.

The two bars of that file, unchanged:
  cap  -- derived: factor residual and solve backward error at most m eps (Higham, Thm 10.3 / 10.4, normwise).  For m < 5,
          m eps drops the lower-order terms of the theorems (at m = 1 LAPACK itself sits at 0.90 of it), so the constants
          themselves stand there: (m + 1) eps for the factor, (3 m + 1) eps for the solve (cr.caps).
  bar  -- relative to LAPACK: 2 x the worst of LAPACK's own values over the matrix and 4 random symmetric permutations of it,
          floored at 1 eps.  Applied from m = 5: below that the cap alone holds (inverting a 1 x 1 or 2 x 2 block and
          correcting takes more roundings than LAPACK's division, and a ratio to 0.0 eps means nothing).
test_chol_reference_host.py holds LAPACK to both on the CPU first, at every shape used here.

Every nk_chol_aug case runs with NYSKOOP_CHOL_FUSE unset and set to 0 (separate trailing and diagonal launches) and requires
the same bits, and proves through the runtime counters that no dataflow launch was issued and nobody gave up.

Measured on one MI355X (profiles/chol_small.log, 29 systems through nk_chol_aug and 7 through nk_solve_spd, units of
eps = 2^-52):
  factor residual        graded GPU 0.13 .. 1.53 (LAPACK 0.18 .. 1.59)   random 0.30 .. 0.97 (0.25 .. 0.57)   rbf 0.39 .. 1.36 (0.34 .. 1.39)
  solve backward error   graded GPU 0.09 .. 0.18 (LAPACK 0.09 .. 0.22)   random 0.11 .. 0.21 (0.07 .. 0.45)   rbf 0.10 .. 0.77 (0.07 .. 0.77)
  nk_solve_spd           graded GPU 0.07 .. 0.10 (LAPACK 0.08 .. 0.12)   random 0.10 .. 0.19 (0.08 .. 0.35)   rbf 0.08 .. 0.77 (0.09 .. 0.77)
No case lies between the bar and the cap: the nearest is the factor of (128, 63, rbf) at 0.59 of its bar.  (0.77 is m = 1, where
the GPU and LAPACK return the same bits.)"""
import numpy as np
import pytest

import chol_reference as cr
import pinv_reference as pr
from test_gpu_chol_accuracy import _check, _log

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not cr.HAVE_LONGDOUBLE, reason=cr.LONGDOUBLE_SKIP)]


@pytest.fixture(scope="module")
def ctx():
    import nys_koop_lqr_amd as nk
    return nk.get_context()


def _same_bits(a, b):
    for (L1, X1, f1, r1), (L0, X0, f0, r0) in zip(a, b):
        assert f1 == f0 and r1 == r0, (f1, f0, r1, r0)
        # (the strict upper triangle inside a diagonal tile is scratch, see include/nyskoop.h: the factor is the lower triangle)
        assert np.array_equal(np.tril(L1), np.tril(L0)) and np.array_equal(X1, X0)


def _chain(ctx, monkeypatch, systems):
    """nk_chol_aug on the ordinary context with the fused trailing + diagonal launch and without it: same bits, no dataflow
    launch, no give-up."""
    monkeypatch.delenv("NYSKOOP_CHOL_FUSE", raising=False)
    c0 = cr.counters()
    fused = cr.chol_aug(ctx, systems)
    monkeypatch.setenv("NYSKOOP_CHOL_FUSE", "0")
    apart = cr.chol_aug(ctx, systems)
    monkeypatch.delenv("NYSKOOP_CHOL_FUSE")
    c1 = cr.counters()
    assert c1[6] == c0[6], (c0, c1)  # no dataflow launch
    assert c1[5] == c0[5], (c0, c1)  # nobody gave up
    _same_bits(fused, apart)
    for (P, _, _), (L1, _, _, _), (L0, _, _, _) in zip(systems, fused, apart):  # also where a system failed
        assert cr.upper_tiles_untouched(L1, P) and cr.upper_tiles_untouched(L0, P)
    return fused


def _pair(m, p, d, fam0, fam1):
    """[(family, order, seed, extra, P, R), ...] of a pair of cr.SMALL_PAIRS."""
    return [(fam, mq, seed, extra, cr.matrix(fam, mq, seed), cr.rhs(extra, mq, seed))
            for fam, mq, seed, extra in cr.small_pair_systems(m, p, d, fam0, fam1)]


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the chain below the threshold of the dataflow launch, ordinary context
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,extra,family,ld", cr.SMALL_SINGLE)
def test_single_system(ctx, monkeypatch, m, extra, family, ld):
    seed = m
    P, R = cr.matrix(family, m, seed), cr.rhs(extra, m, seed)
    if family == "graded":  # the correction step of the products with the inverted blocks fires
        assert max(cr.diag_block_kappa(P)) > cr.CHOL_FIX_KAPPA
    (L, X, failed, ratio), = _chain(ctx, monkeypatch, [(P, R, ld)])
    assert 0.0 < ratio <= 1.0
    _check("small", m, extra, family, seed, P, R, L, X, failed)


@pytest.mark.parametrize("m,p,d,fam0,fam1", cr.SMALL_PAIRS)
def test_paired_systems(ctx, monkeypatch, m, p, d, fam0, fam1):
    systems = _pair(m, p, d, fam0, fam1)
    for fam, mq, seed, _, P, _ in systems:
        if fam == "graded":
            assert max(cr.diag_block_kappa(P)) > cr.CHOL_FIX_KAPPA
    out = _chain(ctx, monkeypatch, [(P, R, mq) for _, mq, _, _, P, R in systems])
    for q, ((fam, mq, seed, extra, P, R), (L, X, failed, ratio)) in enumerate(zip(systems, out)):
        assert 0.0 < ratio <= 1.0
        _check(f"small-pair{q}", mq, extra, fam, seed, P, R, L, X, failed)


# The failure word is LAPACK potrf's `info`: index + 1 of the first non-positive pivot -- in the first block, in a second block
# of order 1 (factored by the fused launch), in the last row of a partial block.
@pytest.mark.parametrize("m,j", [(65, 3), (65, 64), (40, 39)])
def test_first_nonpositive_pivot_is_lapack_info(ctx, monkeypatch, m, j):
    import scipy.linalg as sla
    P = cr.indefinite(m, j, seed=11)
    assert (np.linalg.eigvalsh(P) < 0).sum() == 1
    _, info = sla.lapack.dpotrf(P, lower=1)
    assert info == j + 1
    (_, _, failed, ratio), = _chain(ctx, monkeypatch, [(P, cr.rhs(64, m, 11), m)])
    assert failed == info and ratio == 0.0


def test_indefinite_system_beside_a_good_one(ctx, monkeypatch):
    """The failure word belongs to its own system: the other system of the pair factors and solves as if alone."""
    bad = cr.indefinite(65, 64, seed=11)
    P1, R1 = cr.matrix("rbf", 64, 5), cr.rhs(40, 64, 5)
    out = _chain(ctx, monkeypatch, [(bad, cr.rhs(64, 65, 11), 65), (P1, R1, 64)])
    assert out[0][2] == 65 and out[0][3] == 0.0
    assert 0.0 < out[1][3] <= 1.0
    _check("small-beside-indefinite", 64, 40, "rbf", 5, P1, R1, *out[1][:3])


def test_exactly_singular_psd_system_is_flagged(ctx, monkeypatch):
    """A duplicated landmark (row and column 7 of the jitter-free kernel matrix copied onto 100): either the pivot at 100 comes
    out non-positive, as in LAPACK (index + 1), or rounding leaves it positive and the isolated rounding-level pivot is
    reported as an exact null space (-1); then the factor and the solution are still finite."""
    import scipy.linalg as sla
    P = cr.singular_psd()
    m = P.shape[0]
    info = sla.lapack.dpotrf(P, lower=1)[1]
    (L, X, failed, ratio), = _chain(ctx, monkeypatch, [(P, cr.rhs(3, m, m), m)])
    _log(f"small-singular m={m}: failed {failed} (LAPACK info {info}) piv_ratio {ratio:.3e}")
    assert failed != 0
    assert failed == -1 or failed == 101, failed
    if failed == -1:
        assert np.isfinite(np.tril(L)).all() and np.isfinite(X).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  lock-step members: the chain recorded and replayed through the _batched twins of its kernels
# ---------------------------------------------------------------------------------------------------------------------
def _member_rounds(ctx, rounds_of_systems):
    """One round of a three-member pool, member k solving rounds_of_systems[k]; every result must have the bits of the same
    call on the ordinary context.  Returns the growth of the group's merged-launch count over the round."""
    from nys_koop_lqr_amd import _lib
    pool = _lib.lockstep_pool(3, index=11)
    s0 = pool.stats()
    got = pool.run_round(lambda systems: cr.chol_aug(_lib.get_context(), systems), rounds_of_systems)
    s1 = pool.stats()
    for systems, member in zip(rounds_of_systems, got):
        _same_bits(member, cr.chol_aug(ctx, systems))
        for (P, _, _), (L, _, _, _) in zip(systems, member):
            assert cr.upper_tiles_untouched(L, P)
    return s1["merged_launches"] - s0["merged_launches"], s1["single_launches"] - s0["single_launches"]


def _single(m, extra, family, seed):
    return [(cr.matrix(family, m, seed), cr.rhs(extra, m, seed), m)]


def test_members_with_one_shape_merge_their_launches_and_keep_the_bits(ctx):
    m, extra = 65, 64
    merged, single = _member_rounds(ctx, [_single(m, extra, "random", m + k) for k in range(3)])
    _log(f"small-members merged round (65, 64, random) x 3: merged launches {merged}, single launches {single}")
    assert merged > 0


def test_members_with_one_pair_shape_merge_their_launches_and_keep_the_bits(ctx):
    m, p, d, fam0, fam1 = cr.SMALL_PAIRS[0]
    assert (m, p, d) == (64, 1, 2)
    rounds = []
    for k in range(3):  # three different matrices of the pair's shape
        rounds.append([(cr.matrix(fam0, m + p, 1000 + m + p + k), cr.rhs(m, m + p, 1000 + m + p + k), m + p),
                       (cr.matrix(fam1, m, 2000 + m + k), cr.rhs(d, m, 2000 + m + k), m)])
    merged, single = _member_rounds(ctx, rounds)
    _log(f"small-members merged round pair (64, 1, 2) x 3: merged launches {merged}, single launches {single}")
    assert merged > 0


def test_members_with_different_shapes_keep_the_bits(ctx):
    """(321, 65, rbf) is above the threshold: the member records the chain while the ordinary context, which the member's bits
    are compared with, takes the dataflow launch."""
    c0 = cr.counters()
    merged, single = _member_rounds(ctx, [_single(65, 64, "random", 65), _single(129, 1, "random", 129),
                                          _single(321, 65, "rbf", 321)])
    c1 = cr.counters()
    _log(f"small-members unmerged round 65 / 129 / 321: merged launches {merged}, single launches {single}")
    assert c1[6] == c0[6] + 1 and c1[5] == c0[5], (c0, c1)  # the one dataflow launch is the ordinary context's, at m = 321


# ---------------------------------------------------------------------------------------------------------------------
# 3.  nk_solve_spd: the plain factor, then forward and backward substitution with their own diagonal-block correction
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def strict(ctx):
    ctx.set_strict_spd(1)  # the pseudo-inverse branch cannot stand in for the Cholesky: a flagged pivot is an error
    try:
        yield ctx
    finally:
        ctx.set_strict_spd(0)


@pytest.mark.parametrize("m,nrhs,family", cr.SOLVE_SPD)
def test_solve_spd_is_backward_stable(strict, monkeypatch, m, nrhs, family):
    seed = m
    P, Rrows = cr.matrix(family, m, seed), cr.rhs(nrhs, m, seed)
    if family == "graded":
        assert max(cr.diag_block_kappa(P)) > cr.CHOL_FIX_KAPPA
    monkeypatch.delenv("NYSKOOP_CHOL_FUSE", raising=False)
    c0 = cr.counters()
    X = pr.solve(strict, P, np.ascontiguousarray(Rrows.T))
    if (m, nrhs) in ((65, 64), (321, 65)):
        monkeypatch.setenv("NYSKOOP_CHOL_FUSE", "0")
        apart = pr.solve(strict, P, np.ascontiguousarray(Rrows.T))
        monkeypatch.delenv("NYSKOOP_CHOL_FUSE")
        assert np.array_equal(X, apart)
    c1 = cr.counters()
    assert c1[6] == c0[6] and c1[5] == c0[5], (c0, c1)  # the plain factor never takes the dataflow launch
    assert np.isfinite(X).all()
    be = cr.solve_backward_error(X.T, P, Rrows)
    lbe = cr.lapack_reference(family, m, seed, nrhs)[1]
    cap_s = cr.caps(m)[1]
    e = cr.EPS
    _log(f"small-solve_spd m={m} nrhs={nrhs} family={family} solve: gpu {be / e:.3f} lapack {lbe[0] / e:.3f} "
         f"(perms {min(lbe) / e:.3f}..{max(lbe) / e:.3f}) bar {cr.lapack_bar(lbe) / e:.3f} | cap {cap_s / e:.0f}")
    assert be <= cap_s, (be / e, m)
    if m >= 5:
        assert be <= cr.lapack_bar(lbe), (be / e, [v / e for v in lbe])
