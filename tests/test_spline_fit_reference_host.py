"""Host checks of tests/spline_fit_reference.py, which tests/test_gpu_spline_stages.py grades the device with: the
fault-free float64 emulation of the fit stays under every bar on every case the GPU file uses, every planted fault exceeds a
bar on every case where that fault's code runs, the plan (passes, pieces, gathering) of each case is the one its name says,
and the systems of sections C and D have the condition, rank and pivot ratios the GPU tests rely on.  No GPU."""
import numpy as np
import pytest

import spline_fit_reference as S

pytestmark = pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason=S.LONGDOUBLE_SKIP)


def test_tps_reference_and_bars():
    """The spline value: exactly 0 at coincident points, r^2 log(r) elsewhere; the float64
    NumPy block stays under its bar in both forms, and the Gram-form bar is the wider one where the rows are far from mu."""
    q = S.problem(300, 40, 20, 2)
    kx, r2x, ky, r2y = S.blocks(q)
    assert (r2x == 0).sum() >= 5 and (r2y == 0).sum() >= 5
    assert np.all(kx[r2x == 0] == 0) and np.all(ky[r2y == 0] == 0)
    nz = r2y > 0
    assert np.allclose(S._f(ky[nz]), 0.5 * S._f(r2y[nz]) * np.log(S._f(r2y[nz])), rtol=1e-14)
    rows = np.arange(q.n)
    Dx, Dy = S.block_bars(q, False, rows)
    Gx, Gy = S.block_bars(q, True, rows)
    assert S.worst_ratio(S.tps_f64(q.X[:, :q.d], q.Z), kx, Dx) <= 1.0
    assert S.worst_ratio(S.tps_f64(q.Y, q.Z), ky, Dy) <= 1.0
    assert S.worst_ratio(S.tps_f64(q.X[:, :q.d], q.Z, q.mu), kx, Gx) <= 1.0
    assert S.worst_ratio(S.tps_f64(q.Y, q.Z, q.mu), ky, Gy) <= 1.0
    assert np.all(Dy[r2y == 0] == 0) and np.all(Gy[r2y == 0] > 0)


def test_plans_are_what_the_names_say():
    B = S.B_CASES
    lens = lambda c: [[ln for _, ln in ps] for ps in c.passes]
    assert lens(B["passes_n2100_d2"]) == [[1024], [1024], [52]]
    assert lens(B["passes_n1025_d40"]) == [[1024], [1]] and B["passes_n1025_d40"].gram_form
    assert lens(B["passes_n2048_d7"]) == [[1024], [1024]]
    assert lens(B["two_ranges"]) == [[1700]] and B["two_ranges"].gathered
    assert lens(B["two_ranges_and_an_empty_one"]) == [[1700]]
    assert lens(B["two_ranges_two_passes"]) == [[1024], [676]]
    big = B["two_pieces_past_256MB"]
    assert lens(big) == [[7850, 7850]] and not big.gathered and big.n_eff == 15700
    assert big.n_eff * 2.0 * big.d * 8.0 > S.GATHER_BYTES > (big.n_eff - 80) * 2.0 * big.d * 8.0  # just past the rule
    assert B["generic_m1_p0"].launches == 2 and B["fused_d7_m20_p1"].launches == 1 and B["passes_n2100_d2"].launches == 3
    assert S.layout(20, 1) == (22, 42) and S.layout(12, 2) == (14, 26)
    for n in {c.n_eff for c in S.B_CASES.values()} | {n for n, _ in S.A_SHAPES}:
        assert (S.readout_gamma(n) * float(n) == 2.0 ** 100) == (n != 15700), n  # see readout_bar


@pytest.mark.parametrize("name", list(S.CASES))
def test_emulation_under_the_bars_and_every_fault_over_one(name):
    c = S.CASES[name]
    ref = S.reference(name)
    solvers = ("chol", "svd") if c.section == "C" else ("chol",)
    for solver in solvers:
        clean = S.grade(ref, *S.emulate(c, lstsq=solver == "svd"), solver=solver)
        assert max(clean.values()) <= 1.0, (solver, clean)
    faults = S.faults_of(c)
    assert len(faults) >= 5
    for fault in faults:
        for solver in solvers:  # (the faults are graded against the bars of both solvers: the wider one has to see them too)
            got = S.grade(ref, *S.emulate(c, fault), solver=solver)
            assert max(got.values()) > 100.0, (fault, solver, got)


def test_every_fault_has_a_route_among_the_cases():
    seen = {f for c in S.CASES.values() for f in S.faults_of(c)}
    assert seen == set(S.FAULTS)


@pytest.mark.parametrize("n,m", S.A_SHAPES)
def test_identity_cases_emulate_under_the_bars(n, m):
    for d, mode in S.A_DIMS:
        c = S.a_case(n, m, d, mode)
        ref = S.reference_of(c)
        got = S.grade(ref, *S.emulate(c))
        assert max(got.values()) <= 1.0, (d, mode, got)
        assert c.gram_form == (mode == 0 and d >= 32 and m >= 2)


def test_section_c_systems():
    """cond(P) and the pivot ratio of every section C system: far above the window, so the default path is the Cholesky, and
    cond(P) times a product bar of 1e-12 stays far below 1, which is what the first-order solve bars need."""
    for name, c in S.C_CASES.items():
        ref = S.reference(name)
        mp = c.m + c.p
        ratio, pos = S.pivot_ratio_ld(ref.P)
        assert pos and ratio > 1e4 * S.window(mp), (name, ratio, S.window(mp))
        assert 1.5 <= ref.cond <= 1e8, (name, ref.cond)


def test_section_d_known_rank():
    """One centre repeated, gamma = 0: cov has two equal rows bit for bit, rank m + p - 1 with a clear gap on both sides of
    scipy.linalg.pinv's cut-off (the zero singular value is rounding noise of LAPACK's fp64 SVD here, a tenth of eps), and
    the collapsed system is well conditioned."""
    ref = S.reference_d()
    mp = ref.case.m + ref.case.p
    s = ref.s
    cut = mp * S.EPS * s[0]
    assert int((s > cut).sum()) == mp - 1
    assert s[-2] > 1e6 * cut and s[-1] < 0.1 * cut, (s[-2] / s[0], s[-1] / s[0], cut / s[0])
    assert ref.cond_collapsed < 1e8, ref.cond_collapsed
    # the minimum-norm solution: equal columns 0 and 1, and it solves the normal equations of the singular system
    assert np.array_equal(ref.M[:, 0], ref.M[:, 1])
    Rl = np.vstack([S.products(ref.case)[0]["top"], S.products(ref.case)[0]["bot"]])
    res = ref.M @ ref.cov - Rl
    assert float(np.abs(res).max()) <= 1e-12 * float(np.abs(Rl).max())
    # the float64 emulation through gelsd stays under the bars of the collapsed system; a stale top (the pseudo-inverse's result
    # not written over the Cholesky's rows), the wrong leading dimension and a dropped row do not
    c = ref.case
    clean = S.grade_d(ref, *S.emulate(c, lstsq=True))
    assert max(clean.values()) <= 1.0, clean
    for fault in ("Gtop_left_unsolved", "AB_sliced_with_ld_m", "dropped_row_at_pass_boundary"):
        got = S.grade_d(ref, *S.emulate(c, fault, lstsq=True))
        assert max(got.values()) > 100.0, (fault, got)


def test_section_d_no_listed_case_is_inside_the_window_at_full_rank():
    """The two conditions of the issue on a full-rank system inside the window exclude each other on the listed shapes (see
    spline_fit_reference.window_case): where the pivot ratio is 1/30 .. 1/3 of the window, sigma_min / sigma_max is below
    (m+p) eps, not 10 x above it.  And the system the statistics test uses sits inside the window with positive pivots."""
    mp = S.WINDOW_SHAPE[2] + S.WINDOW_SHAPE[3]
    for g in (10.0 ** -14.5, 1e-14, 10.0 ** -13.5):
        _, _, ratio, srat = S.window_case(g)
        assert S.window(mp) / 40 <= ratio <= S.window(mp) / 2.5, (g, ratio / S.window(mp))
        assert srat < mp * S.EPS, (g, srat / (mp * S.EPS))
    _, _, ratio, _ = S.window_case()
    assert 40 * mp * S.EPS < ratio < S.window(mp) / 3  # 40 x the rounding (m+p) eps p_kk of a pivot
    for n, d, m, p in S.C_SHAPES:  # every other shape: the pivot ratio at gamma = 0 is far above the window
        if (n, d, m, p) != S.WINDOW_SHAPE:
            ref, _ = S.products(S._case("C", n, d, m, p, gamma=1.0))
            ratio, pos = S.pivot_ratio_ld(ref["cov"])
            assert pos and ratio > 100 * S.window(m + p), ((n, d, m, p), ratio / S.window(m + p))
