"""The thin-plate-spline EDMD fit (nk_spline_fit) stage by stage on the MI355X, entry by entry against the longdouble
reference of tests/spline_fit_reference.py: the two spline blocks as the fit builds them, the products top and bot on every
route of the pass loop, cov and the solve on the Cholesky and the pseudo-inverse path, the slicing into A | B and C, W, and the
branch between the two solvers.  Everything goes through nk_spline_fit / nk_model_get and the statistics; the bars are derived
in the reference module, the host tests (tests/test_spline_fit_reference_host.py) hold them against a NumPy emulation and show
that every planted fault exceeds them on each of the cases used here.  Each case prints its worst err / bar
("spline-stages: ..." lines, pytest -s); profiles/spline_stages.log holds the figures of one MI355X run.

A. gamma n_eff = 2^100: the operators are [top; bot] / 2^100 to a rounding.  p = n, U = I_n hands back Phi_y, a diagonal of
   powers of two in the state hands back Phi_x: the device's own blocks under the block bars.
B. top and bot (its first m columns: C) entry by entry at 2^100 on every route.
C. A, B, C, W under the solve bars at gamma = 1 and 1e-2, Cholesky and strict_spd = 2.
D. The branch: an exactly singular cov, and what the statistics say about the window.

Measured on an MI355X (worst err / bar, profiles/spline_stages.log; 61 passed in 12 s): A, spline blocks 0.24 (direct) and 0.08
(Gram form), read-out 0 ulp from nk_kernel_matrix; B, top 0.016 and bot 0.011 over all routes (0.00025 and 0.00001 on the two
pieces past 256 MB, where the propagated Gram-form bar of d = 1024 dominates); C, Cholesky A | B 0.0050, C 0.0065, W 0.0029,
pseudo-inverse 0.012, 0.0038, 0.0015, without the dataflow launch the same figures as with it; W against the fit's own C [A B]
at most 0.37 of gamma_(m+2) |C| |[A B]|; D, known rank 0.0002 (the factorisation fails: strict = 1 is NK_ERR_NOT_SPD), window
case pivot ratio 2.83e-12 as in longdouble, rank 237 of 257, e_ls 0.0018 of cap_ls.  The solve ratios are small because the bars
are worst-case bounds; the host test holds every planted fault 100 x and more above them."""
import ctypes as C
import types

import numpy as np
import pytest

import pinv_reference as PR
import spline_fit_reference as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason=S.LONGDOUBLE_SKIP)]


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()  # fails loudly without a gfx950 device / built library
    return nk


def _report(what, ratios):
    print("spline-stages: " + what + ": " + ", ".join(f"{k} {v:.4g}" for k, v in ratios.items()))


def _device(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(torch.device("cuda", 0))  # (a copy: the problems are read-only)


def _operands(q, form):
    """X, Y of problem q in the form the case asks for (module docstring of spline_fit_reference, _case)."""
    import torch
    if form == "host":
        return q.X, q.Y
    if form == "odd_ld":
        X, Y = _device(q.X), _device(q.Y)
        assert X.stride(0) % 2 == 1  # stage_in leaves device inputs where they are: X misses the operand contract
        return X, Y
    assert form == "offset8", form
    ld = (q.d + q.p + 2) & ~1
    flat = torch.zeros(q.n * ld + 2, dtype=torch.float64, device=torch.device("cuda", 0))
    k = 0 if flat.data_ptr() % 16 == 8 else 1
    X = torch.as_strided(flat, (q.n, q.d + q.p), (ld, 1), storage_offset=k)
    X.copy_(torch.from_numpy(np.array(q.X)))
    assert X.data_ptr() % 16 == 8 and X.stride(0) % 2 == 0
    return X, _device(q.Y)


def _fit(nk, X, Y, Z, p, gamma, ranges=None, ldc=None, mode=0, strict=0, expect=0):
    """nk_spline_fit and nk_model_get: a namespace with AB (m x (m+p)), C, W, Z and the statistics (None and the return code
    when the call fails with the code `expect`)."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    Xm, Ym = _lib.Mat(X), _lib.Mat(Y)
    n, d = Ym.shape
    Zb = np.asarray(Z)
    m = Zb.shape[0]
    ldc = Zb.strides[0] // 8 if ldc is None else ldc
    rr, n_rr = None, 0
    if ranges is not None:
        flat = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1))
        rr, n_rr = flat.ctypes.data_as(C.POINTER(C.c_int64)), flat.size // 2
    stats, h = _lib.FitStats(), C.c_void_p()
    ctx.wait_for(X, Y)
    ctx.set_kmat_mode(mode)
    ctx.set_strict_spd(strict)
    try:
        rc = ctx.lib.nk_spline_fit(ctx.handle, Xm.ptr, Xm.ld, Ym.ptr, Ym.ld, n, d, p, rr, n_rr, Zb.ctypes.data, ldc, m, float(gamma),
                                   C.byref(h), C.byref(stats))
    finally:
        ctx.set_kmat_mode(0)
        ctx.set_strict_spd(0)
    if expect != 0 and rc == expect:
        return None
    _lib.check(rc)
    try:
        out = types.SimpleNamespace(AB=np.full((m, m + p), np.nan), C=np.full((d, m), np.nan), W=np.full((d, m + p), np.nan),
                                    Z=np.full((m, d), np.nan), stats=stats.as_dict())
        get = lambda w, a, ld: _lib.check(ctx.lib.nk_model_get(ctx.handle, h, w, a.ctypes.data, ld))
        get(b"A", out.AB, m + p)
        if p:
            get(b"B", out.AB[:, m:], m + p)
        get(b"C", out.C, m)
        get(b"W", out.W, m + p)
        get(b"Z", out.Z, d)
    finally:
        _lib.check(ctx.lib.nk_model_destroy(h))
    assert all(np.all(np.isfinite(a)) for a in (out.AB, out.C, out.W))
    return out


def _kernel_matrix(nk, A, Z, mode):
    """nk_kernel_matrix of the spline kernel (mode 1: direct differences, 0: automatic, Gram form at d >= 32)."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    A, Z = np.ascontiguousarray(A), np.ascontiguousarray(Z)
    d = A.shape[1]
    kd = _lib.KernelDesc(_lib.NK_KERNEL_TPS, d, 0, 0, None, 0.0)
    out = np.empty((A.shape[0], Z.shape[0]))
    ctx.set_kmat_mode(mode)
    try:
        _lib.check(ctx.lib.nk_kernel_matrix(ctx.handle, C.byref(kd), A.ctypes.data, d, A.shape[0], Z.ctypes.data, d, Z.shape[0],
                                            out.ctypes.data, Z.shape[0]))
    finally:
        ctx.set_kmat_mode(0)
    return out


def _run(nk, monkeypatch, c, **kw):
    q = S.problem(*c.key)
    if c.budget:
        monkeypatch.setenv("NYSKOOP_F_BUDGET_GB", S.BUDGET)  # read per fit
    X, Y = _operands(q, c.form)
    kw.setdefault("mode", c.mode)
    return _fit(nk, X, Y, q.Z, q.p, S.gamma_of(c), ranges=None if c.ranges is None else [list(r) for r in c.ranges], **kw)


# =====================================================================================================================
# A. the spline blocks, read out at gamma n = 2^100
# =====================================================================================================================
@pytest.mark.parametrize("d,mode", S.A_DIMS)
def test_spline_blocks_read_out_of_the_operators(nk, monkeypatch, d, mode):
    """Direct differences at d = 1, 2, 7 and at d = 40 under nk_set_kmat_mode(1); Gram form at d = 32, 33, 40, 64 (m = 1 stays
    direct).  Shapes: gram_reference.A_SHAPES and m = 1.  B 2^100 = Phi_y^T with identity inputs; where n <= d the first n rows of
    C 2^100 are 2^e Phi_x.  The bar of an entry is its block bar plus the read-out term (spline_fit_reference.readout_bar: no
    ulp, only the first-order term |top| |cov| / 2^100 and its rounding, which is all that stands where Phi_y is exactly 0 --
    the operator is not zero there, see grade_blocks).  An allowance of 2 ulp for the read-out is not needed: wherever the
    reference is not exactly zero the read-out is asserted equal, bit for bit, to the block nk_kernel_matrix computes in the
    same mode (at the coincident points the Gram form leaves noise of 1e-13, to which the first-order term adds).
    Measured on an MI355X (profiles/spline_stages.log): direct blocks at most 0.24 of the bar, Gram-form blocks at most 0.08
    (0.10 at the coincident points), the first-order term at the exact zeros 0.49 of its bound, 0 ulp from nk_kernel_matrix."""
    for n, m in S.A_SHAPES:
        c = S.a_case(n, m, d, mode)
        ref = S.reference_of(c)
        got = _run(nk, monkeypatch, c)
        assert got.stats["gram_kernel_launches"] == c.launches and got.stats["rank_inner"] == m + n
        ratios, n_zero, at_zero = S.grade_blocks(ref, got.AB, got.C)
        own = _kernel_matrix(nk, ref.q.Y, ref.q.Z, 0 if c.gram_form else 1)  # the device's block by nk_kernel_matrix
        read = (got.AB[:, m:] * S.gn_of(c)).T
        nz = (S._f(S.blocks(ref.q)[3]) > 0) & (own != 0)
        ratios["ulps_from_nk_kernel_matrix"] = float(np.max(np.abs(read[nz] - own[nz]) / np.spacing(np.abs(own[nz])))) if nz.any() else 0.0
        assert np.array_equal(read[nz], own[nz])  # one entry, one fixed contraction over d: nk_kernel_matrix's bits come back
        ratios.update(S.grade(ref, got.AB, got.C, got.W))
        _report(f"A {'gram form' if c.gram_form else 'direct'} d={d} n={n} m={m} (zeros {n_zero}, largest there {at_zero:.3g})", ratios)
        assert n_zero >= 1 and max(v for k, v in ratios.items() if not k.startswith("ulps")) <= 1.0, ratios
        assert ("phi_x" in ratios) == (n <= d)


# =====================================================================================================================
# B. top and bot on every route
# =====================================================================================================================
@pytest.mark.parametrize("name", list(S.B_CASES))
def test_top_and_bot_entry_by_entry(nk, monkeypatch, name):
    """Routes (spline_fit_reference.B_CASES), asserted from gram_kernel_launches where they show (1 per pass fused, 2 per pass
    on the generic engine, which m = 1 takes whatever p is; bot apart does not show): the fused three-problem launch from host arrays with d even
    and odd, p = 0, 1, 6 and m + p odd, Gram form and direct; the generic engine; bot by launch_gemm at d = 1, from a device
    tensor of odd leading dimension and from a device view 8 bytes off a 16-byte boundary; passes of 1024 rows (1024 / 1024 / 52,
    1024 / 1 -- at d = 40 the one-row piece is built by direct differences inside Gram-form mode --, 1024 / 1024), each also from
    an odd-ld device tensor so that the piecewise bot accumulates across passes; two row ranges gathered, with an empty one, over
    two passes, and un-gathered just past the 256 MB rule (two pieces in one pass)."""
    c = S.B_CASES[name]
    ref = S.reference(name)
    got = _run(nk, monkeypatch, c)
    assert got.stats["gram_kernel_launches"] == c.launches, got.stats["gram_kernel_launches"]
    assert got.stats["rank_inner"] == c.m + c.p
    ratios = S.grade(ref, got.AB, got.C, got.W)
    _report(f"B {name} (launches {c.launches})", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", ["two_ranges", "two_ranges_and_an_empty_one", "two_ranges_two_passes"])
def test_row_ranges_equal_the_sliced_copy_bit_for_bit(nk, monkeypatch, name):
    """Gathered ranges are one piece of n_eff rows: the same launches as the fit on the sliced copy, so the same bits."""
    c = S.B_CASES[name]
    q = S.problem(*c.key)
    a = _run(nk, monkeypatch, c)
    rows, _, gathered = S.plan(q.n, q.d, q.p, c.ranges)
    assert gathered
    b = _fit(nk, np.ascontiguousarray(q.X[rows]), np.ascontiguousarray(q.Y[rows]), q.Z, q.p, S.gamma_of(c))
    for w in ("AB", "C", "W"):
        assert np.array_equal(getattr(a, w), getattr(b, w)), w


def test_nan_pad_columns_are_never_read(nk):
    """d = 3, p = 0: device views X[:, :3] and Y[:, :3] of n x 4 tensors whose fourth column is NaN (the engine's operand A of
    bot spans an even number of columns: beside an odd d it reads the pad column and must not let it into the result), and
    centres with ldc = 4 > d.  Every result is finite, under the bars, and bit for bit the result of the same call with zeros in
    the pad column; A (top does not depend on X's layout) is the dense host call's bit for bit in every form, C and W as well
    where bot takes the same route as there (host arrays are staged with an even leading dimension: the fused launch)."""
    ref = S.reference("fused_d3_m20_p0")
    q = ref.q
    gam = S.readout_gamma(q.n)
    dense = _fit(nk, q.X, q.Y, q.Z, 0, gam)
    pad = lambda a, v: np.hstack([a, np.full((a.shape[0], 1), v)])
    forms = {"X": lambda v: (_device(pad(q.X, v))[:, :3], _device(q.Y), q.Z),
             "Y": lambda v: (_device(q.X), _device(pad(q.Y, v))[:, :3], q.Z),
             "X and Y": lambda v: (_device(pad(q.X, v))[:, :3], _device(pad(q.Y, v))[:, :3], q.Z),
             "centres": lambda v: (q.X, q.Y, pad(q.Z, v)[:, :3])}
    for what, make in forms.items():
        got, twin = (_fit(nk, *make(v), 0, gam) for v in (np.nan, 0.0))
        assert got.stats["gram_kernel_launches"] == 1 and np.array_equal(got.Z, q.Z), what
        for w in ("AB", "C", "W"):
            assert np.array_equal(getattr(got, w), getattr(twin, w)), (what, w)
        assert np.array_equal(got.AB, dense.AB), what
        if what != "Y":  # (there X is a dense n x 3 device tensor: odd leading dimension, bot apart)
            assert np.array_equal(got.C, dense.C) and np.array_equal(got.W, dense.W), what
        ratios = S.grade(ref, got.AB, got.C, got.W)
        _report(f"B nan pad d=3 p=0, NaN beside {what}", ratios)
        assert max(ratios.values()) <= 1.0, ratios


# =====================================================================================================================
# C. cov and the solve
# =====================================================================================================================
@pytest.mark.parametrize("strict", [0, 2])
@pytest.mark.parametrize("name", list(S.C_CASES))
def test_operators_under_the_solve_bars(nk, monkeypatch, name, strict):
    """A | B, C, W against the longdouble solution under spline_fit_reference.solve_bars, on the default path (the augmented
    Cholesky with extra = m + d rows; m + p = 257 takes the dataflow launch) and under nk_set_strict_spd(2) (the Jacobi
    pseudo-inverse on the saved system, written over the top rows); W also against the fit's own C [A B].  Both report the full
    rank; the default path reports a pivot ratio far above the window, strict = 2 none."""
    c = S.C_CASES[name]
    ref = S.reference(name)
    got = _run(nk, monkeypatch, c, strict=strict)
    mp = c.m + c.p
    assert got.stats["rank_inner"] == mp and got.stats["gram_kernel_launches"] == c.launches
    if strict == 0:
        assert got.stats["pivot_ratio_inner"] > 1e4 * S.window(mp)
    else:
        assert got.stats["pivot_ratio_inner"] == 0.0
    ratios = S.grade(ref, got.AB, got.C, got.W, solver="svd" if strict else "chol")
    _report(f"C {name} strict={strict} cond {ref.cond:.3g}", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", S.FLOW_CASES)
def test_operators_under_the_solve_bars_without_the_dataflow_launch(nk, monkeypatch, name):
    """m + p = 257 again with NYSKOOP_CHOL_FLOW=0 (read per call): the launch-per-step chain, the same bars."""
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "0")
    c = S.C_CASES[name]
    ref = S.reference(name)
    got = _run(nk, monkeypatch, c)
    assert got.stats["rank_inner"] == c.m + c.p
    ratios = S.grade(ref, got.AB, got.C, got.W)
    _report(f"C {name} NYSKOOP_CHOL_FLOW=0", ratios)
    assert max(ratios.values()) <= 1.0, ratios


# =====================================================================================================================
# D. the branch
# =====================================================================================================================
def test_known_rank_takes_the_pseudo_inverse(nk, monkeypatch):
    """(400, 2, 12, 1) with centre 1 a copy of centre 0 and gamma = 0: cov is exactly singular, rank m + p - 1, the rest well
    conditioned.  rank_inner says so, the rank-truncation counter moves, and A | B, C, W are the minimum-norm solution: the
    longdouble solution of the collapsed system (the two equal columns rotated into sum and difference, the difference dropped),
    under the solve bars evaluated on the collapsed system.  nk_set_strict_spd(1): NK_ERR_NOT_SPD if the factorisation met a
    non-positive pivot, else the same bits; which of the two is printed."""
    from nys_koop_lqr_amd import _lib
    c = S.D_CASE
    ref = S.reference_d()
    mp = c.m + c.p
    before = _lib.runtime_counters()["rank_truncated_fits"]
    got = _run(nk, monkeypatch, c)
    assert _lib.runtime_counters()["rank_truncated_fits"] == before + 1
    assert got.stats["rank_inner"] == mp - 1
    ratios = S.grade_d(ref, got.AB, got.C, got.W)
    failed = got.stats["pivot_ratio_inner"] == 0.0
    strict = _run(nk, monkeypatch, c, strict=1, expect=-3)
    assert (strict is None) == failed  # NK_ERR_NOT_SPD exactly when the factorisation failed
    if strict is not None:
        for w in ("AB", "C", "W"):
            assert np.array_equal(getattr(strict, w), getattr(got, w)), w
    _report(f"D known rank (factorisation {'failed: strict = 1 is NK_ERR_NOT_SPD' if failed else 'succeeded: strict = 1 gives the same bits'},"
            f" pivot ratio {got.stats['pivot_ratio_inner']:.3g}, cond collapsed {ref.cond_collapsed:.3g})", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_pivot_ratio_is_reported_when_the_window_sends_the_system_on(nk, monkeypatch):
    """include/nyskoop.h: pivot_ratio_inner is the ratio whenever the factorisation succeeded, also when it then sent the
    system to the pseudo-inverse -- it is what lets a caller see the window decision.  (900, 2, 255, 2) with gamma n = 1e-14
    sigma_max: in longdouble the pivot ratio is a tenth of the window 2 (m+p)^2 eps and 40 x above a pivot's rounding, so the
    factorisation succeeds and the pseudo-inverse solves: the reported ratio is positive, inside the window and within a factor
    2 of the longdouble one, the rank is what the cut-off (m+p) eps leaves (below m + p here: sigma_min / sigma_max is a fifth of
    it), and the solution meets pinv_reference's least-squares criterion e_ls <= cap_ls on the reference's system.
    No case is inside the window at FULL rank: spline_fit_reference.window_case says why, the host test checks it."""
    from nys_koop_lqr_amd import _lib
    c, P, ratio_ld, srat = S.window_case()
    mp = c.m + c.p
    before = _lib.runtime_counters()["rank_truncated_fits"]
    got = _run(nk, monkeypatch, c)
    r = got.stats["pivot_ratio_inner"]
    assert 0.0 < r <= S.window(mp) and ratio_ld / 2 <= r <= 2 * ratio_ld, (r, ratio_ld, S.window(mp))
    assert srat < mp * S.EPS and got.stats["rank_inner"] < mp
    assert _lib.runtime_counters()["rank_truncated_fits"] == before + 1
    ref, _ = S.products(c)
    Rhs = np.vstack([ref["top"], ref["bot"]]).astype(np.float64)
    e = PR.e_ls(got.AB.T, P.astype(np.float64), Rhs[:c.m].T)  # the rows the fit returns whole: A | B = top pinv(P)
    _report(f"D window (pivot ratio {r:.3g}, longdouble {ratio_ld:.3g}, window {S.window(mp):.3g}, rank {got.stats['rank_inner']} of {mp})",
            dict(e_ls_over_cap=e / PR.cap_ls(mp)))
    assert e <= PR.cap_ls(mp), (e, PR.cap_ls(mp))
