"""The part of a Nystrom fit in front of the m x m algebra, entry by entry against the longdouble reference of
tests/gram_reference.py: the two n x m kernel blocks as the fit builds them (Gram form on the MFMA engine at d >= 32, on the fp64
and the fp32 engine; direct differences otherwise) and the four Gram accumulators on every route of pass_f64 / pass_f32 (one
fused four-problem launch, three problems with G4 apart, the generic three-launch route of an odd m + p, several passes with
beta = 1, gathered row ranges, device-resident inputs, the fp32 engine).  Everything goes through
KoopmanNystromRegressor.gram_partial, i.e. nk_nystrom_gram and the packed layout include/nyskoop.h documents.

Section A reads the kernel blocks out of the accumulators with identity inputs (p = n, U = I_n: every entry of G1[m:, :m] and
G2[:, m:] is a sum with one non-zero term, exact in any order), so the device's own kernel values come back bit for bit through
the kernels a fit uses.  Section B holds every accumulator entry against contraction_bar + the propagated kernel-block bar.
Section C ties the checked accumulator to `fit`.  The bars come from error analysis (gram_reference.py), the host tests hold
them against NumPy emulations and show that a dropped row, a stale tile, a missing mirror or a wrong leading dimension exceeds
them on every shape used here.  Each test prints its worst err / bar ("gram-entries: ..." lines, pytest -s);
profiles/README.md records the figures of one MI355X run.

Measured there (worst err / bar, profiles/gram_entries.log): Gram-form blocks fp64 0.08 (RBF), 0.21 (anisotropic RBF), 0.13
(Matern), 0.21 (linear); direct differences 0.16 / 0.29 / 0.36; fp32 engine 0.08 (RBF) and 0.11 (Matern) of the fp32 bar where
the float32 NumPy emulation has 0.09 and 0.11 (allowed: 4 x the emulation); accumulators at n = 2100 at most 0.0033 (fp64) and
0.0071 (fp32 engine), 0.09 at n = 1; contraction alone 0.003 (fp64) and 0.023 (fp32 engine) of gamma_(n+2) |F|^T |F|; fit and
gram + solve: the same bits."""
import types

import numpy as np
import pytest

import gram_reference as R
from gram_reference import LINEAR, MATERN, RBF, U32, U64

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.LONGDOUBLE_SKIP)]

D0 = 40


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()  # fails loudly without a gfx950 device / built library
    return nk


def _regressor(nk, q, f32=False):
    from nys_koop_lqr_amd import _lib
    code = {RBF: _lib.NK_KERNEL_RBF, MATERN: _lib.NK_KERNEL_MATERN52, LINEAR: _lib.NK_KERNEL_LINEAR}[q.family]
    if q.family == LINEAR:
        kern = nk.kernels.DeviceKernel(code, None, q.par)
    else:
        kern = nk.kernels.DeviceKernel(code, np.asarray(q.par))
    reg = nk.KoopmanNystromRegressor(q.p, kernel=types.SimpleNamespace(kernel=kern), gamma=1e-3, m=q.m)
    reg.nystrom_centers_output = np.ascontiguousarray(q.Zout.T)
    if q.sep:
        reg.nystrom_centers_input = np.ascontiguousarray(q.Zin.T)
    if f32:
        reg.compute_dtype = "f32"
    return reg


def _gram(nk, q, f32=False, kmat_mode=0, **kw):
    """(the four blocks, Gram kernel launches, the flat accumulator) of gram_partial on problem q."""
    reg = _regressor(nk, q, f32)
    ctx = nk.get_context()
    X, Y = kw.pop("X", q.X), kw.pop("Y", q.Y)
    ctx.set_kmat_mode(kmat_mode)
    try:
        flat = reg.gram_partial(X, Y, **kw)
    finally:
        ctx.set_kmat_mode(0)
    host = flat if isinstance(flat, np.ndarray) else flat.cpu().numpy()
    assert host.shape == (reg.gram_size(q.d),) == (R.gram_doubles(q.m, q.d, q.p),)
    return R.unpack(host, q.m, q.d, q.p), int(reg._gram_stats["gram_kernel_launches"]), flat


def _symmetric_and_finite(G):
    assert all(np.all(np.isfinite(G[k])) for k in G)
    assert np.array_equal(G["G1"], G["G1"].T) and np.array_equal(G["G3"], G["G3"].T)  # TRI_UPPER_MIRROR: the same bits


def _report(what, ratios):
    print("gram-entries: " + what + ": " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


# =====================================================================================================================
# A. kernel blocks by identity inputs
# =====================================================================================================================
KINDS = {"rbf": (RBF, False, False), "rbf_aniso": (RBF, True, False), "matern": (MATERN, False, False),
         "linear": (LINEAR, False, False), "rbf_separate_input_landmarks": (RBF, False, True)}


def _identity_problem(n, m, d, kind):
    family, aniso, sep = KINDS[kind]
    return R.problem(n, d, m, n, family, aniso, sep, True, 0)


def _extract(nk, q, expect_f32, **kw):
    """The device's two kernel blocks, read out of G1 and G2; the invariants of every Section A case."""
    n, m = q.n, q.m
    G, launches, _ = _gram(nk, q, **kw)
    _symmetric_and_finite(G)
    assert np.array_equal(G["G1"][m:, m:], np.eye(n))  # U^T U
    assert launches == 1, launches  # fused, also at the odd m + p = 9 of the smallest shape (the feature matrix is padded)
    phi_in, phi_out = G["G1"][m:, :m], G["G2"][:, m:].T
    assert np.array_equal(G["G1"][:m, m:].T, phi_in)
    is_f32 = lambda a: np.array_equal(a.astype(np.float32).astype(np.float64), a)
    if expect_f32:
        assert is_f32(phi_in) and is_f32(phi_out)  # the fp32 engine's kernel values, handed back exactly
    elif q.family != LINEAR:
        assert not is_f32(phi_in) and not is_f32(phi_out)  # and the fp64 engine's are not fp32 numbers
    return phi_in, phi_out


def _kblock_ratios(q, phi_in, phi_out, E_in, E_out):
    k_in, _, k_out, _ = R.problem_kernels(q.key)
    return dict(input=R.worst_ratio(phi_in, k_in, E_in), output=R.worst_ratio(phi_out, k_out, E_out))


@pytest.mark.parametrize("d", [33, 40, 64])
@pytest.mark.parametrize("kind", ["rbf", "rbf_aniso", "matern", "linear"])
def test_gram_form_kernel_blocks_entry_by_entry(nk, kind, d):
    """Automatic mode at d >= 32 (odd d, d no multiple of the k-step, whole k-steps): gemm_tn_f64_kernel<EPI> behind prep_rows,
    colsq and colmean, against kernel_ld under kblock_bar_gram_form with the centre the library uses (the mean of the output
    landmarks; zero for linear).  Shapes: edge tiles in both directions, exactly one tile, a handful of rows."""
    for n, m in R.A_SHAPES:
        q = _identity_problem(n, m, d, kind)
        phi_in, phi_out = _extract(nk, q, False)
        ratios = _kblock_ratios(q, phi_in, phi_out, *R.kblock_bars(q, "gram"))
        _report(f"A gram-form fp64 {kind} d={d} n={n} m={m}", ratios)
        assert max(ratios.values()) <= 1.0, ratios


def test_gram_form_kernel_blocks_separate_input_landmarks(nk):
    """Input landmarks that are rows of the state (coincident points in the input block as well), prepared with the centre
    of the output landmarks."""
    q = _identity_problem(300, 130, D0, "rbf_separate_input_landmarks")
    phi_in, phi_out = _extract(nk, q, False)
    assert (R.problem_kernels(q.key)[1] == 0).any()
    ratios = _kblock_ratios(q, phi_in, phi_out, *R.kblock_bars(q, "gram"))
    _report("A gram-form fp64 separate input landmarks d=40 n=300 m=130", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("d,mode", [(D0, 1), (7, 0)])
@pytest.mark.parametrize("kind", ["rbf", "matern", "linear"])
def test_direct_difference_kernel_blocks_entry_by_entry(nk, kind, d, mode):
    """nk_set_kmat_mode(1) at d = 40 and the automatic mode at d = 7: no cancellation, kblock_bar_direct, and coincident points
    give exactly 1.0 for RBF and Matern."""
    for n, m in R.A_SHAPES:
        q = _identity_problem(n, m, d, kind)
        phi_in, phi_out = _extract(nk, q, False, kmat_mode=mode)
        ratios = _kblock_ratios(q, phi_in, phi_out, *R.kblock_bars(q, "direct"))
        _report(f"A direct {kind} d={d} n={n} m={m}", ratios)
        assert max(ratios.values()) <= 1.0, ratios
        if q.family != LINEAR:
            zero = R.problem_kernels(q.key)[3] == 0
            assert zero.any() and np.all(phi_out[zero] == 1.0)


@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_fp32_engine_kernel_blocks_entry_by_entry(nk, kind, d):
    """kmat_f32_asm_kernel<EPI> (d = 64: whole k-steps of 32) and gemm_tn_f32_kernel<EPI> (d = 40) behind prep_rows_f32.  The
    bar is kblock_bar_gram_form with u = 2^-24; what a float32 exp adds to it cannot be derived from the project's text, so the
    float32 NumPy emulation of the same formula is measured against kernel_ld and the device is allowed 4 x its worst ratio.
    Measured on an MI355X, worst over the shapes: RBF device 0.082 / emulation 0.094, Matern device 0.108 / emulation 0.109 of
    the bar (per shape the device is at 0.5 .. 2.5 x its emulation; profiles/README.md)."""
    for n, m in R.A_SHAPES:
        q = _identity_problem(n, m, d, kind)
        phi_in, phi_out = _extract(nk, q, True, f32=True)
        ratios = _kblock_ratios(q, phi_in, phi_out, *R.kblock_bars(q, "gram", U32))
        (allow_in, emu_in), (allow_out, emu_out) = R.problem_f32_allowance(q.key)
        _report(f"A gram-form fp32 {kind} d={d} n={n} m={m}",
                dict(ratios, emulation_input=emu_in, emulation_output=emu_out))
        assert ratios["input"] <= allow_in and ratios["output"] <= allow_out, (ratios, allow_in, allow_out)


# =====================================================================================================================
# B. accumulators on every route
# =====================================================================================================================
def _bars(q, case, rows):
    """Per block: contraction_bar over the rows + the kernel-block bars of the route, propagated."""
    f32 = case.get("f32", False)
    phi_in, U, phi_out = R.problem_features(*q.key)
    if f32:
        E_in, E_out = R.kblock_bars_f32(q)
    else:  # (a one-row piece and a single landmark are built by direct differences: nk_fit.hip, KernelBlocks)
        E_in, E_out = R.kblock_bars(q, "direct" if len(rows) < 2 or q.m < 2 else "gram", U64)
    E = R.propagated_bar(E_in[rows], E_out[rows], phi_in[rows], U[rows], phi_out[rows], q.Y[rows])
    _, S = R.problem_gram(q.key, case.get("row_ranges"))
    return {k: R.contraction_bar(len(rows), S[k], U32 if f32 else 0.0, R.F32_FLUSH_ROWS if f32 else 0) + E[k] for k in S}


@pytest.mark.parametrize("name", list(R.B_CASES))
def test_gram_accumulators_entry_by_entry(nk, monkeypatch, name):
    """Routes, as asserted from gram_kernel_launches (1 per pass fused, 3 per pass generic): p = 2 and p = 0 fused four-problem
    launch; m + p = 128 exactly one tile; p = 3: an odd m + p is ALSO one fused launch (the feature matrix is padded to even
    columns, off_out and ldf are even, so the operands meet the contract and only ldc is odd); the generic three-launch route
    with G4 by launch_gemm is reached at m = 1 alone, below the contract's two columns (kernel blocks by direct differences
    there); n = 1 (shorter than a k-step; its one-row piece takes direct differences), 17 (one step and a one-row tail), 100 (no
    split-K); Matern, linear; separate input landmarks; two row ranges gathered into one piece, also with an empty range;
    NYSKOOP_F_BUDGET_GB=1e-6: passes of 1024 rows, beta = 1 from the second (three passes with a 52-row tail; two with the row
    ranges; odd m + p and the generic route too); device-resident X, Y with d = 33, m = 131, p = 1: stage_in leaves device
    inputs where they are, so Y keeps its odd leading dimension, misses the alignment contract and the fused launch takes
    three problems, G4 by launch_gemm (the statistics count one launch either way; with four problems launch_gemm_tn_multi
    would refuse the operand); the fp32 engine (one fused launch per pass)."""
    case = R.B_CASES[name]
    q = R.problem(*case["key"])
    rr = case.get("row_ranges")
    rows = R.select_rows(q.n, rr)
    kw = {}
    if rr is not None:
        kw["row_ranges"] = [list(r) for r in rr]
    if "budget" in case:
        monkeypatch.setenv("NYSKOOP_F_BUDGET_GB", case["budget"])  # read per fit
    if case.get("device"):
        import torch
        dev = torch.device("cuda", 0)
        kw["X"], kw["Y"] = torch.from_numpy(q.X.copy()).to(dev), torch.from_numpy(q.Y.copy()).to(dev)
        assert kw["Y"].stride(0) % 2 == 1
    f32 = case.get("f32", False)
    G, launches, _ = _gram(nk, q, f32=f32, **kw)
    assert launches == case["passes"] * (1 if f32 else case["launches"]), launches
    _symmetric_and_finite(G)
    ref, _ = R.problem_gram(q.key, rr)
    bars = _bars(q, case, rows)
    ratios = {k: R.worst_ratio(G[k], ref[k], bars[k]) for k in ref}
    _report(f"B {name} (launches {launches})", ratios)
    assert max(ratios.values()) <= 1.0, ratios


_DEVICE_BLOCKS = {}


def _device_kernel_blocks(nk, q, f32):
    """The device's own kernel blocks of problem q, read out with identity inputs as in Section A (cached per shape)."""
    k = (q.key, f32)
    if k not in _DEVICE_BLOCKS:
        n, d, m, p, family, aniso, sep, _, seed = q.key
        qi = R.problem(n, d, m, n, family, aniso, sep, True, seed)  # the same states, outputs and landmarks, U = I_n
        assert np.array_equal(qi.Y, q.Y) and np.array_equal(qi.X[:, :d], q.X[:, :d]) and np.array_equal(qi.Zout, q.Zout)
        _DEVICE_BLOCKS[k] = _extract(nk, qi, f32, f32=f32)
    return _DEVICE_BLOCKS[k]


@pytest.mark.parametrize("name", ["fused_p2", "fused_odd_p3", "two_ranges", "three_passes", "device_inputs_odd_ldy",
                                  "f32_d40_p2", "f32_d40_p2_three_passes"])
def test_contraction_alone_from_the_devices_own_kernel_blocks(nk, monkeypatch, name):
    """The sharpest look at the Gram launches: the reference contracts, in longdouble, the kernel blocks the DEVICE computed
    (read out bit for bit with identity inputs; an entry of a kernel block is one contraction over d and does not depend on p,
    on the pass or on its tile), so no kernel-block bar is needed and contraction_bar alone must hold: gamma_(n+2) |F|^T |F|, on
    the fp32 engine plus the rounding of U and Y and the fp32 partial sums over 32 rows."""
    case = R.B_CASES[name]
    q = R.problem(*case["key"])
    f32 = case.get("f32", False)
    phi_in, phi_out = _device_kernel_blocks(nk, q, f32)
    rr = case.get("row_ranges")
    rows = R.select_rows(q.n, rr)
    kw = {}
    if rr is not None:
        kw["row_ranges"] = [list(r) for r in rr]
    if "budget" in case:
        monkeypatch.setenv("NYSKOOP_F_BUDGET_GB", case["budget"])
    if case.get("device"):
        import torch
        dev = torch.device("cuda", 0)
        kw["X"], kw["Y"] = torch.from_numpy(q.X.copy()).to(dev), torch.from_numpy(q.Y.copy()).to(dev)
    G, launches, _ = _gram(nk, q, f32=f32, **kw)
    assert launches == case["passes"] * case["launches"]
    ref, S = R.gram_from_features(phi_in.astype(R.LD), q.X[:, q.d:].astype(R.LD), phi_out.astype(R.LD), q.Y, rows)
    ratios = {k: R.worst_ratio(G[k], ref[k], R.contraction_bar(len(rows), S[k], U32 if f32 else 0.0,
                                                               R.F32_FLUSH_ROWS if f32 else 0)) for k in ref}
    _report(f"B contraction alone {name}", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def _base():
    case = R.B_CASES["fused_p2"]
    return case, R.problem(*case["key"])


def test_gram_accumulators_are_additive_over_rows(nk):
    """gram_partial(rows A) + gram_partial(rows B) against gram_partial(all): the kernel-block entries are the same bits in
    both (one entry, one fixed-length contraction over d), so the three contraction bars are all that may separate them."""
    case, q = _base()
    cut = 900
    Ga, _, _ = _gram(nk, q, X=q.X[:cut], Y=q.Y[:cut])
    Gb, _, _ = _gram(nk, q, row_ranges=[[cut, q.n]])
    Gall, _, _ = _gram(nk, q)
    _, Sa = R.problem_gram(q.key, ((0, cut),))
    _, Sb = R.problem_gram(q.key, ((cut, q.n),))
    _, Sall = R.problem_gram(q.key, None)
    ratios = {}
    for k in Gall:
        bar = R.contraction_bar(cut, Sa[k]) + R.contraction_bar(q.n - cut, Sb[k]) + R.contraction_bar(q.n, Sall[k])
        ratios[k] = R.worst_ratio(Ga[k] + Gb[k], Gall[k], bar)
    _report("B additivity", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_device_accumulator_equals_host_accumulator(nk):
    """out = a 1-D device tensor: filled in place, the bits of the host-array result."""
    import torch
    case, q = _base()
    _, _, host = _gram(nk, q)
    acc = torch.full((R.gram_doubles(q.m, q.d, q.p),), float("nan"), dtype=torch.float64, device=torch.device("cuda", 0))
    _, _, dev = _gram(nk, q, out=acc)
    assert dev is acc
    got = acc.cpu().numpy()
    first = (2 * q.m + q.p) * (q.m + q.p)
    pad = np.zeros(got.size, dtype=bool)
    pad[first:R.gram_block1(q.m, q.p)] = True  # (the padding entry of an odd first block belongs to nobody)
    assert np.array_equal(got[~pad], host[~pad])


# =====================================================================================================================
# C. the checked accumulator is the fit's
# =====================================================================================================================
def test_fit_from_checked_gram_reproduces_fit(nk):
    """include/nyskoop.h: "nk_nystrom_gram followed by nk_nystrom_solve on one rank equals nk_nystrom_fit" -- the operators of
    fit_from_gram(gram_partial(all rows)) are the bits of fit on the same rows (same kernels, same launches, same order)."""
    case, q = _base()
    a = _regressor(nk, q)
    a.fit(q.X, q.Y)
    b = _regressor(nk, q)
    gram = b.gram_partial(q.X, q.Y)
    ref, _ = R.problem_gram(q.key, None)
    G = R.unpack(gram, q.m, q.d, q.p)
    bars = _bars(q, case, np.arange(q.n))
    assert max(R.worst_ratio(G[k], ref[k], bars[k]) for k in ref) <= 1.0
    b.fit_from_gram(gram, q.n, q.d)
    diff = {k: float(np.max(np.abs(getattr(a, k) - getattr(b, k))) / np.max(np.abs(getattr(a, k)))) for k in ("A", "B", "C")}
    _report("C fit vs gram + solve, max difference / max entry", diff)
    for k in ("A", "B", "C", "weights"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (k, diff)
