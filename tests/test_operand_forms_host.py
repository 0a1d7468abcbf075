"""tests/operand_forms.py without a GPU: the views land where the forms say, the guard check is silent after a correct
write-back and names the position of each planted fault, the flat write-back that nk_gemm_f32 used to make trips it on the
parent layout of the GPU test without leaving the parent, the derived bar of a product holds for float64 `@` and is not
vacuous, and the routes the GPU cases rely on are those of csrc/nk_gemm_plan.h and of the gates in nk_gemm.hip / nk_kmat.hip."""
import os
import re

import numpy as np
import pytest

import operand_forms as of
from gram_reference import worst_ratio
from test_gemm_plan_host import CSRC, plan_program  # noqa: F401  (the fixture that builds tests/gemm_plan_main.cpp)

needs_ld = pytest.mark.skipif(not of.HAVE_LONGDOUBLE, reason=of.LONGDOUBLE_SKIP)
SHAPES = [(5, 4), (3, 7), (1, 6), (6, 1), (0, 5), (5, 0), (130, 257)]


def _block(rows, cols, dtype, seed=0):
    return np.random.default_rng(seed).standard_normal((rows, cols)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("form", ["H0", "H1", "F0", "F1", "F2"])
def test_host_views_land_where_the_form_says(form, rows, cols):
    dtype = np.float32 if form in of.FORMS32 else np.float64
    size = np.dtype(dtype).itemsize
    blk = _block(rows, cols, dtype)
    op = of.Operand(form, rows, cols, blk, dtype=dtype)
    want_ld = {"H0": max(cols, 1), "H1": cols + 3, "F0": max(cols, 1), "F1": cols + 4}.get(form)
    if form == "F2":
        assert op.ld % 2 == 1 and op.ld >= cols + 2
    else:
        assert op.ld == want_ld
    col0 = {"H0": 0, "H1": 1, "F0": 0, "F1": 4, "F2": 1}[form]
    assert op.offset == op.ld + col0 and op.ptr == op.parent.ctypes.data + op.offset * size
    assert op.parent.shape == (rows + 2, op.ld) and not op.is_device
    # the block read through the pointer arithmetic of the C-ABI: element (i, j) at ptr + (i ld + j) size
    flat = op.parent.reshape(-1)
    for i, j in [(0, 0), (rows - 1, cols - 1), (rows // 2, cols // 2)]:
        if rows and cols:
            assert of.same_bits(flat[op.offset + i * op.ld + j], blk[i, j])
    assert of.same_bits(op.block(), blk) and op.guards() is None
    # at least one guard row before and after, guard columns on both sides with a column offset
    pb = op.parent_bits()
    sent = of._BITS[size]
    assert (pb[0] == sent).all() and (pb[-1] == sent).all()
    if col0 and rows:
        assert (pb[1:-1, :col0] == sent).all() and (flat.view(pb.dtype)[op.offset + cols:op.offset + cols + 1] == sent).all()


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("form", ["D0", "D1", "D2", "D3", "G0", "X0", "X1", "X2"])
def test_device_views_land_where_the_form_says(form, rows, cols):
    """The device forms on torch's CPU allocator (the same as_strided views of a 1-D tensor; Operand asserts data_ptr() % 16
    and the parity of the stride itself)."""
    torch = pytest.importorskip("torch")
    dtype = np.float32 if form in of.FORMS32 else np.float64
    size = np.dtype(dtype).itemsize
    blk = _block(rows, cols, dtype, 1)
    op = of.Operand(form, rows, cols, blk, dtype=dtype, device="cpu")
    base = op.storage.data_ptr()
    assert op.is_device and op.storage.dim() == 1 and base % 16 == 0
    want = {"D0": (0, 2, 0), "D1": (0, 2, 1), "D2": (8, 2, 0), "D3": (8, 2, 1), "G0": (0, 4, 0), "X0": (0, 4, 2), "X1": (4, 4, 0),
            "X2": (8, 4, 0)}[form]
    assert (op.ptr % 16, op.ld % want[1]) == (want[0], want[2]) and op.ld > cols
    assert op.view.storage_offset() == op.offset and tuple(op.view.shape) == (rows, cols)
    if rows and cols:
        assert op.view.stride() == (op.ld, 1) and op.view.data_ptr() == op.ptr == base + op.offset * size
        assert of.same_bits(op.view.contiguous().numpy(), blk)
    assert of.same_bits(op.block(), blk) and op.guards() is None
    pb = op.parent_bits()
    g = op.form.guard_rows
    assert pb.shape == (rows + 2 * g, op.ld) and (pb[:g] == of._BITS[size]).all() and (pb[-g:] == of._BITS[size]).all()
    # a write through the view lands in the block and nowhere else
    if rows and cols:
        op.view.copy_(torch.from_numpy(blk + 1))
        assert of.same_bits(op.block(), blk + 1) and op.guards() is None


def test_an_output_block_starts_as_the_sentinel():
    op = of.Operand("H1", 4, 3)
    assert (of.bits(op.block()) == of.SENTINEL_BITS64).all() and np.isnan(op.block()).all()
    assert of.bits(np.array([of.sentinel()]))[0] == of.SENTINEL_BITS64
    assert of.bits(np.array([of.sentinel(np.float32)]))[0] == of.SENTINEL_BITS32
    # quiet NaNs with a payload: a float comparison could not tell them from any other NaN, the bit patterns can
    other = np.array([np.nan])
    assert np.isnan(of.sentinel()) and of.bits(other)[0] != of.SENTINEL_BITS64


# ---------------------------------------------------------------------------------------------------------------------
# the guard check
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["H0", "H1"])
def test_guards_are_intact_after_a_2d_write_back(form):
    """hipMemcpy2D's shape: `cols` elements per row, rows `ld` apart"""
    M, N = 6, 9
    op = of.Operand(form, M, N)
    res = _block(M, N, np.float64, 2)
    flat = op.parent.reshape(-1)
    for i in range(M):
        flat[op.offset + i * op.ld:op.offset + i * op.ld + N] = res[i]
    assert op.guards() is None and of.guards_intact(op.parent, op.block_slice) is None
    assert of.same_bits(op.block(), res)


def test_guard_check_names_each_planted_fault():
    M, N = 6, 9  # not square
    res = _block(M, N, np.float64, 3)

    def fresh():
        op = of.Operand("H1", M, N)
        op.parent[op.block_slice] = res
        return op, op.parent.reshape(-1)

    op, flat = fresh()  # one pad column written, in the third row of the block
    flat[op.offset + 2 * op.ld + N] = 1.0
    assert op.guards() == (1 + 2, 1 + N)
    op, flat = fresh()  # one element before the block
    flat[op.offset - 1] = 1.0
    assert op.guards() == (1, 0)
    op, flat = fresh()  # one past the last row: the first element of what would be row M
    flat[op.offset + M * op.ld] = 1.0
    assert op.guards() == (1 + M, 1)
    op, flat = fresh()  # a transposed write: N rows of M elements at the block's leading dimension
    for j in range(M + 1):  # (rows M + 1 .. N - 1 of the transposed block would lie below the parent: not simulated)
        flat[op.offset + j * op.ld:op.offset + j * op.ld + M] = res[:, j]
    assert op.guards() == (1 + M, 1)  # row M of the transposed block lies below the block
    op, flat = fresh()  # ... and with M > N it is the columns to the right that give it away
    wide = of.Operand("H1", N, M)
    wf = wide.parent.reshape(-1)
    for j in range(M):
        wf[wide.offset + j * wide.ld:wide.offset + j * wide.ld + N] = res[j]
    assert wide.guards() == (1, 1 + M)
    # a NaN written over a guard is a change too, unless it is the sentinel itself
    op, flat = fresh()
    flat[0] = np.nan
    assert op.guards() == (0, 0)
    op, flat = fresh()
    flat[0] = of.sentinel()
    assert op.guards() is None
    # tight parent: only the guard rows can tell
    tight = of.Operand("H0", M, N, res)
    tight.parent.reshape(-1)[tight.offset + M * tight.ld] = 0.0
    assert tight.guards() == (1 + M, 0)


@pytest.mark.parametrize("M,N,K", of.GEMM_F32_SHAPES)
def test_flat_write_back_of_the_old_nk_gemm_f32_trips_the_guards_inside_the_parent(M, N, K):
    """The write-back nk_gemm_f32 made before it became a 2-D copy -- M * ldc doubles from C's first element -- on the very
    parent the GPU test hands in for `padded host C at a column offset` (form H1): it overwrites the pad columns of every
    row and runs col0 doubles past the last row, the guard check names the first pad column, and the last element written
    still lies inside the parent (whose last guard row is ld >= col0 + 1 long), so the GPU test cannot corrupt the heap even
    against a library that still has the fault."""
    op = of.Operand("H1", M, N)
    flat_size = op.parent.size
    end = of.flat_writeback(op)
    assert end == op.offset + M * op.ld and end <= flat_size
    assert end - 1 >= (1 + M) * op.ld  # it did run past the block's last row ...
    assert end <= (2 + M) * op.ld      # ... into the guard row below, no further
    assert op.guards() == (1, 1 + N)
    # the same on the operands: K * lda floats read from A's first element stay inside A's parent for every host form
    for form in ("F0", "F1", "F2"):
        a = of.Operand(form, K, M, dtype=np.float32)
        assert a.offset + K * a.ld <= a.parent.size, form


# ---------------------------------------------------------------------------------------------------------------------
# the reference and its bar
# ---------------------------------------------------------------------------------------------------------------------
@needs_ld
def test_float64_matmul_is_inside_the_derived_bar():
    worst = 0.0
    for M, N, K in of.GEMM_SHAPES:
        A, B, C0, P, S = of.gemm_problem(M, N, K)
        for tA, tB in of.TRANSPOSITIONS:
            As, Bs = (A.T if tA else A), (B.T if tB else B)
            for alpha, beta in of.ALPHA_BETA:
                C = of.sentinel_filled((M, N)) if beta == 0.0 else C0
                ref, bar = of.gemm_ref(tA, tB, alpha, As, Bs, beta, C, product=P, scale=S)
                assert np.isfinite(ref.astype(np.float64)).all() and np.isfinite(bar).all()
                got = alpha * (A @ B) + (beta * C0 if beta != 0.0 else 0.0)
                r = worst_ratio(got, ref, bar)
                worst = max(worst, r)
                if K == 0:
                    assert np.array_equal(got, (beta * C0 if beta != 0.0 else np.zeros((M, N)))) and r <= 1.0
        # the cached product is the one gemm_ref forms itself
        ref2, bar2 = of.gemm_ref(1, 1, 0.5, A.T, B.T, -1.5, C0)
        ref1, bar1 = of.gemm_ref(0, 0, 0.5, A, B, -1.5, C0, product=P, scale=S)
        assert np.array_equal(ref1, ref2) and np.allclose(bar1, bar2, rtol=1e-14, atol=0)
    print(f"float64 @ against gemm_ref: worst error / bar {worst:.3f}")
    assert worst < 1.0


@needs_ld
def test_the_bar_is_not_vacuous():
    """K = 3: the bar is gamma_6 = 3 eps of each entry's own |A| |B|.  One entry whose operands are 16 times smaller than the
    rest gets an error of one ulp of the product's scale (its largest |A| |B|): a normwise check would pass it, the
    componentwise bar does not.  Without the planted error the same product is inside the bar."""
    rng = np.random.default_rng(33)
    A, B = rng.uniform(0.5, 1.0, (7, 3)), rng.uniform(0.5, 1.0, (3, 5))
    A[2] /= 16.0
    ref, bar = of.gemm_ref(0, 0, 1.0, A, B, 0.0, None)
    got = A @ B
    assert worst_ratio(got, ref, bar) < 1.0
    scale = float((np.abs(A) @ np.abs(B)).max())
    got[2, 3] += np.spacing(scale)
    r = worst_ratio(got, ref, bar)
    print(f"one ulp of the scale in a small entry: error / bar {r:.2f}")
    assert r > 1.0
    assert np.abs(got - ref.astype(np.float64)).max() / scale < 4 * 2.0 ** -52  # invisible normwise
    assert of.gemm_bar_factor(0) == of.gamma(3, of.U64) >= 2.0 ** -52 and of.gemm_bar_factor(300) == of.gamma(303, of.U64)


@needs_ld
def test_tps_reference():
    A = np.array([[0.0, 0.0], [3.0, 4.0], [1.0, 0.0]])
    k, r2 = of.tps_ld(A, A[:2])
    assert k[0, 0] == 0 and k[1, 1] == 0 and float(r2[1, 0]) == 25.0
    assert abs(float(k[1, 0]) - 25.0 * np.log(5.0)) < 1e-13 and float(k[2, 0]) == 0.0  # r = 1: log 1 = 0
    assert of.tps_bar_direct(2, r2)[0, 0] == 0.0 and of.tps_bar_direct(2, r2)[1, 0] > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_routes_through_the_plan(plan_program):
    """At 256 compute units (MI355X), through csrc/nk_gemm_plan.h: (130, 257, 300) is 2 x 3 tiles and 19 k-steps of 16 rows,
    which the generic engine cuts into 2 slices of 160 rows (the second: 140 rows, ending in a 12-row step), so the reduce
    kernel runs; (130, 257, 37) is 3 k-steps in one slice."""
    tiles = plan_program("tiles", [(0, 2, 3)])[0][0]
    assert tiles == 6 == -(-130 // 128) * -(-257 // 128)
    (kt300, klen1), (kt37, _), (kt0, klen0) = plan_program("slice", [(300, 16, 1), (37, 16, 1), (0, 16, 1)])
    assert (kt300, kt37, kt0, klen0) == (19, 3, 0, 16)
    s300, s37, s0 = (r[0] for r in plan_program("splitk", [(tiles, kt300, 256), (tiles, kt37, 256), (tiles, kt0, 256)]))
    assert s300 >= 2 and s300 == 2 and s37 == 1 and s0 == 1
    assert plan_program("slice", [(300, 16, s300)]) == [[19, 160]]
    assert 300 - 160 == 140 and 140 % 16 == 12
    # the LDS-DMA engine's choice for the same shape does not depend on the form either (it is a function of these three)
    assert plan_program("splitk", [(tiles, kt300, 256)])[0][1] >= 1


def test_small_product_bound_and_engine_gate_are_the_sources():
    """The bound and the gates that gemm_route / kmat_route mirror, read from the sources they mirror."""
    gemm = open(os.path.join(CSRC, "nk_gemm.hip")).read()
    assert "M * N <= 32768 && K <= 1024" in gemm and (of.SMALL_MN, of.SMALL_K) == (32768, 1024)
    assert "transA && !transB && opts.tri != TRI_LOWER && opts.splitk == 0 && K >= 128" in gemm and of.TN_MIN_K == 128
    assert "if (tn_fast_ok(tp) && (opts.tri == TRI_FULL || M == N)) return launch_gemm_tn_multi" in gemm
    assert "p.vecA = aligned16(A) && (lda % 2 == 0);" in gemm and "p.vecB = aligned16(B) && (ldb % 2 == 0);" in gemm
    kmat = open(os.path.join(CSRC, "nk_kmat.hip")).read()
    assert re.search(r"constexpr int KFLAT_DMAX = 8;", kmat) and re.search(r"KSMALL_MAX_ENTRIES = 8192;", kmat)
    assert ("if (d <= KFLAT_DMAX && ldo % 2 == 0 && nB % 2 == 0 && aligned16(out) && (size_t)(nB * d + d) * 8 <= 60 * 1024 &&\n"
            "      nA * nB >= 4096 &&") in kmat
    assert "const int vecO = aligned16(out) && ldo % 2 == 0;" in kmat
    plan = open(os.path.join(CSRC, "nk_gemm_plan.h")).read()
    assert "return M >= per16 && N >= per16 && aligned16(A) && aligned16(B) && lda % per16 == 0 && ldb % per16 == 0 &&" in plan


def test_gemm_cases_reach_every_side_of_every_gate():
    small = [(7, 5, 3), (33, 17, 130), (9, 6, 0)]
    tile = [(130, 257, 37), (130, 257, 300), (130, 257, 0)]
    assert sorted(small + tile) == sorted(of.GEMM_SHAPES)
    for tA, tB in of.TRANSPOSITIONS:
        for s in small:
            assert of.gemm_route(*s, tA, tB)[0] == "small" and of.gemm_route(*s, tA, tB, "D3", "D3")[0] == "small"
        for s in tile:
            want = "tn" if (tA, tB) == (1, 0) and s[2] >= 128 else "tile"
            assert of.gemm_route(*s, tA, tB)[0] == want, (s, tA, tB)
    M, N, K = 130, 257, 300
    # the LDS-DMA engine for host operands and for aligned device operands with even leading dimensions ...
    for fa, fb in [("H0", "H0"), ("H1", "H1"), ("D0", "D0"), ("H0", "D0")]:
        assert of.gemm_route(M, N, K, 1, 0, fa, fb) == ("tn", True, True, True)
    # ... the generic engine when tn_fast_ok fails, with every combination of scalar and double2 loads
    assert of.gemm_route(M, N, K, 1, 0, "D1", "D1") == ("tile", False, False, False)
    assert of.gemm_route(M, N, K, 1, 0, "D2", "D2") == ("tile", False, False, False)
    assert of.gemm_route(M, N, K, 1, 0, "D3", "D3") == ("tile", False, False, False)
    assert of.gemm_route(M, N, K, 1, 0, "D3", "H0") == ("tile", False, True, False)
    assert of.gemm_route(M, N, K, 1, 0, "H0", "D3") == ("tile", True, False, False)
    for tA, tB in of.TRANSPOSITIONS:  # both load helpers (direct and transposing) of both operands, vector and scalar
        for K2 in (37, 300):
            assert of.gemm_route(M, N, K2, tA, tB, "D0", "D0")[1:3] == (True, True)
            for f in ("D1", "D2", "D3"):
                assert of.gemm_route(M, N, K2, tA, tB, f, f)[1:3] == (False, False)


def test_kernel_matrix_cases_reach_every_side_of_every_gate():
    r = of.kmat_route
    assert [r(*s)[0] for s in of.KMAT_SHAPES] == ["small", "flat", "flat", "tiled"]
    assert r(70, 64, 3, "D0", "D0", "D0")[0] == "flat"
    assert [r(70, 64, 3, f, f, f)[0] for f in ("D1", "D2", "D3")] == ["small"] * 3
    assert [r(130, 66, 2, f, f, f)[0] for f in ("D1", "D2", "D3")] == ["tiled"] * 3
    assert r(130, 66, 2, "H0", "H0", "D3") == ("tiled", True, True, False, False)
    assert r(130, 67, 19, "D0", "D0", "D0") == ("tiled", True, True, True, False)  # odd nB: the flat gate is false anyway
    assert r(130, 67, 19, "D3", "D3", "D3") == ("tiled", False, False, False, False)
    assert r(130, 67, 19, "D3", "H0", "H0")[1:4] == (False, True, True)
    assert r(130, 67, 19, "H0", "D3", "H0")[1:4] == (True, False, True)
    assert r(130, 67, 19, "H0", "H0", "D3")[1:4] == (True, True, False)
