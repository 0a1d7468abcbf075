"""Operand forms for the dense building blocks of the C-ABI (nk_gemm, nk_gemm_f32, nk_solve_spd, nk_sqrtm_spd,
nk_kernel_matrix): every operand, input or output, lives inside a larger parent allocation filled with one sentinel (a quiet
NaN with a fixed payload), as a host array or as a torch.as_strided view of a 1-D device tensor, tight or padded, 16-byte
aligned or 8 bytes past a 16-byte boundary, with an even or an odd leading dimension.  After a call the guards (everything of
the parent that is not the block) are compared as integer bit patterns.  Also here: the longdouble reference of a product with
its derived componentwise bar, the thin-plate-spline reference, and Python mirrors of the route decisions of launch_gemm
(nk_gemm.hip) and launch_kmat (nk_kmat.hip).  Importing this module needs neither a GPU nor torch.

Layout of a parent: a 2-D array of (guard_rows + rows + guard_rows) x ld elements at a 16-byte aligned base; the block starts
at row guard_rows, column col0.  The element offset of the block, guard_rows * ld + col0, decides the alignment of its first
element, so the forms choose guard_rows (1 or 2) and col0 to land where they say, and Operand asserts that they did."""
import functools

import numpy as np

from chol_reference import HAVE_LONGDOUBLE, LD, LONGDOUBLE_SKIP  # noqa: F401  (re-exported for the tests)
from gram_reference import gamma
from sqrtm_reference import _mm

SENTINEL_BITS64 = 0x7FF8_0BAD_C0DE_F00D  # quiet NaN, payload 0xBADC0DEF00D
SENTINEL_BITS32 = 0x7FC5_A5A5            # quiet NaN (fp32)
_INT = {8: np.int64, 4: np.int32}
_BITS = {8: SENTINEL_BITS64, 4: SENTINEL_BITS32}
NK_ERR_BAD_ARG = -1


def sentinel(dtype=np.float64):
    size = np.dtype(dtype).itemsize
    return np.array([_BITS[size]], dtype=_INT[size]).view(dtype)[0]


def bits(a):
    """the elements of a float array as integers of the same width"""
    a = np.ascontiguousarray(a)
    return a.view(_INT[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def sentinel_filled(shape, dtype=np.float64):
    size = np.dtype(dtype).itemsize
    return np.full(shape, _BITS[size], dtype=_INT[size]).view(dtype)


def guards_intact(parent, block_slice):
    """parent: 2-D array (floats, or their bit patterns as integers); block_slice: (row slice, column slice) of the block.
    Returns None when every element outside the block still holds the sentinel's bits, else the (row, column) of the first
    one, in row-major order, that does not."""
    parent = np.asarray(parent)
    ib = parent if parent.dtype.kind in "iu" else bits(parent)
    ok = ib == ib.dtype.type(_BITS[ib.dtype.itemsize])
    ok[block_slice] = True
    bad = np.flatnonzero(~ok.ravel())
    if bad.size == 0:
        return None
    return (int(bad[0] // parent.shape[1]), int(bad[0] % parent.shape[1]))


# ---------------------------------------------------------------------------------------------------------------------
# forms.  name -> (device, ld(cols), col0, guard_rows, first element's address mod 16 or None (host), ld modulus, ld residue)
# ---------------------------------------------------------------------------------------------------------------------
def _ld_above(cols, at_least, modulus, residue):
    """the smallest ld >= at_least with ld % modulus == residue"""
    ld = max(at_least, 1)
    while ld % modulus != residue:
        ld += 1
    return ld


class Form:
    def __init__(self, name, device, pad, col0, guard_rows, mod16, ld_mod, ld_res):
        self.name, self.device, self.pad, self.col0, self.guard_rows = name, device, pad, col0, guard_rows
        self.mod16, self.ld_mod, self.ld_res = mod16, ld_mod, ld_res

    def ld(self, cols):
        if self.ld_mod is None:  # exactly cols + pad
            return max(cols + self.pad, 1)
        return _ld_above(cols, cols + self.col0 + self.pad, self.ld_mod, self.ld_res)


# fp64 (issue table): H0 host tight; H1 host ld = cols + 3 at column 1; D0 aligned, even ld; D1 aligned, odd ld; D2 and D3
# 8 bytes past a 16-byte boundary with an even and an odd ld.  Offset of the block in elements = guard_rows * ld + col0:
#   D0: 1 * even + 0 (even);  D1: 2 * odd + 0 (even);  D2: 1 * even + 1 (odd);  D3: 2 * odd + 1 (odd).
FORMS = {f.name: f for f in (
    Form("H0", False, 0, 0, 1, None, None, None),
    Form("H1", False, 3, 1, 1, None, None, None),
    Form("D0", True, 1, 0, 1, 0, 2, 0),
    Form("D1", True, 1, 0, 2, 0, 2, 1),
    Form("D2", True, 1, 1, 1, 8, 2, 0),
    Form("D3", True, 1, 1, 2, 8, 2, 1),
    Form("DT", True, 0, 0, 1, None, None, None),  # device, tight (for outputs the C-ABI takes without a leading dimension)
)}
# fp32 operands of nk_gemm_f32 (K x M / K x N): F0 host tight; F1 host ld = cols + 4 at a 4-float offset; F2 host odd ld at a
# 1-float offset; G0 device, aligned, ld % 4 == 0; and three that break the engine's contract for device operands:
# X0 ld % 4 == 2 (aligned: 2 guard rows), X1 base + 4 bytes, X2 base + 8 bytes (both with ld % 4 == 0).
FORMS32 = {f.name: f for f in (
    Form("F0", False, 0, 0, 1, None, None, None),
    Form("F1", False, 4, 4, 1, None, None, None),
    Form("F2", False, 1, 1, 1, None, 2, 1),
    Form("G0", True, 1, 0, 1, 0, 4, 0),
    Form("X0", True, 1, 0, 2, 0, 4, 2),
    Form("X1", True, 1, 1, 1, 4, 4, 0),
    Form("X2", True, 1, 2, 1, 8, 4, 0),
)}
DEVICE_FORMS = ("D0", "D1", "D2", "D3")
CONTRACT_BREAKING32 = ("X0", "X1", "X2")


def form_of(name):
    return FORMS[name] if name in FORMS else FORMS32[name]


class Operand:
    """A rows x cols block inside a sentinel-filled parent, on the host or the device.  block: the contents (None: the block
    itself starts as the sentinel, for outputs that must be overwritten)."""

    def __init__(self, form, rows, cols, block=None, dtype=np.float64, device="cuda"):
        f = form_of(form) if isinstance(form, str) else form
        self.form, self.rows, self.cols, self.dtype = f, int(rows), int(cols), np.dtype(dtype)
        self.is_device = f.device
        self.ld = f.ld(cols)
        g, c0 = f.guard_rows, f.col0
        # (F1 is ld = cols + 4 at column 4 by definition: the guard to the right of a row is the left guard of the next one)
        assert self.ld >= c0 + cols and (c0 == 0 or self.ld > c0 + cols or f.name == "F1"), (f.name, self.ld, c0, cols)
        self.parent_shape = (g + self.rows + g, self.ld)
        self.block_slice = (slice(g, g + self.rows), slice(c0, c0 + self.cols))
        self.offset = g * self.ld + c0
        size = self.dtype.itemsize
        host = sentinel_filled(self.parent_shape, self.dtype)
        if block is not None:
            block = np.asarray(block, dtype=self.dtype)
            assert block.shape == (self.rows, self.cols), (block.shape, self.rows, self.cols)
            host[self.block_slice] = block
        if self.is_device:
            import torch
            tdt, idt = {8: (torch.float64, torch.int64), 4: (torch.float32, torch.int32)}[size]
            self._torch = torch
            # 1-D, in the allocator's own (at least 16-byte aligned) memory; copied as integers, so every bit is kept
            flat = torch.from_numpy(bits(host).reshape(-1)).to(device, copy=True).view(tdt)
            assert flat.dim() == 1 and flat.data_ptr() % 16 == 0
            self.storage = flat
            self.view = torch.as_strided(flat, (self.rows, self.cols), (self.ld, 1), storage_offset=self.offset)
            self.ptr = flat.data_ptr() + self.offset * size
            assert self.view.numel() == 0 or (self.view.data_ptr() == self.ptr and self.view.stride(0) == self.ld)
            assert f.mod16 is None or self.ptr % 16 == f.mod16, (f.name, self.ptr % 16)
            self._idt = idt
        else:
            self.parent = host
            self.ptr = host.ctypes.data + self.offset * size
            v = host[self.block_slice]
            assert v.size == 0 or (v.ctypes.data == self.ptr and (self.rows == 1 or v.strides[0] == self.ld * size))
        if f.ld_mod is not None:
            assert self.ld % f.ld_mod == f.ld_res, (f.name, self.ld)

    def parent_bits(self):
        """the whole parent as a host array of integers"""
        if self.is_device:
            return self.storage.view(self._idt).cpu().numpy().reshape(self.parent_shape)
        return bits(self.parent).reshape(self.parent_shape)

    def block(self):
        """a host copy of the block as it is now"""
        pb = self.parent_bits()[self.block_slice]
        return np.ascontiguousarray(pb).view(self.dtype)

    def guards(self):
        return guards_intact(self.parent_bits(), self.block_slice)


def call(operands, fn):
    """fn() between two torch.cuda.synchronize() when an operand is on the device: the library's streams do not wait for
    torch's, and the read-back must not overtake the call."""
    torch = next((o._torch for o in operands if o.is_device), None)
    if torch is not None:
        torch.cuda.synchronize()
    rc = fn()
    if torch is not None:
        torch.cuda.synchronize()
    return rc


def check_inputs_and_guards(inputs, outputs, tag=""):
    """inputs: [(Operand, contents)] that a call must leave unchanged; outputs: [Operand].  Every guard intact."""
    for name, (op, want) in inputs.items():
        assert op.guards() is None, (tag, name, "guard changed at", op.guards())
        assert same_bits(op.block(), np.asarray(want, dtype=op.dtype)), (tag, name, "input changed")
    for name, op in outputs.items():
        assert op.guards() is None, (tag, name, "guard changed at", op.guards())


# ---------------------------------------------------------------------------------------------------------------------
# the faults the guards are there for, as NumPy writes into a parent (tests/test_operand_forms_host.py)
# ---------------------------------------------------------------------------------------------------------------------
def flat_writeback(op, result_ld=None):
    """What nk_gemm_f32 did with a host C before its write-back became a 2-D copy: M * ldc consecutive doubles from the
    block's first element on, columns N .. ldc-1 of every row from a device buffer that nothing had written.  Returns the
    index one past the last element written, in elements of the flattened parent; the write itself stays inside it (asserted
    by the caller)."""
    flat = op.parent.reshape(-1)
    n = op.rows * op.ld
    end = op.offset + n
    assert end <= flat.size, "the simulated write would leave the parent"
    flat[op.offset:end] = np.arange(n, dtype=np.float64) + 0.5
    return end


# ---------------------------------------------------------------------------------------------------------------------
# references and bars
# ---------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(7, 5, 3), (33, 17, 130), (130, 257, 37), (130, 257, 300), (9, 6, 0), (130, 257, 0)]
ALPHA_BETA = [(1.0, 0.0), (0.5, -1.5), (-1.0, 1.0)]
TRANSPOSITIONS = [(0, 0), (0, 1), (1, 0), (1, 1)]
GEMM_F32_SHAPES = [(6, 10, 70), (132, 260, 33), (128, 128, 2048)]
KMAT_SHAPES = [(9, 7, 5), (70, 64, 3), (130, 66, 2), (130, 67, 19)]
U64 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def gemm_problem(M, N, K):
    """op(A) (M x K), op(B) (K x N), C0 (M x N) and, when longdouble is wider than fp64, the longdouble product and the
    scale |op(A)| |op(B)|; cached and read-only."""
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    A, B, C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
    P = _mm(A.astype(LD), B.astype(LD)) if K > 0 else np.zeros((M, N), dtype=LD)
    S = np.abs(A) @ np.abs(B)
    for a in (A, B, C0, P, S):
        a.setflags(write=False)
    return A, B, C0, P, S


def gemm_bar_factor(K):
    """gamma_(K+3): any summation order of correctly rounded fma / add stays within gamma_K, three more roundings for alpha,
    beta and the final sum; never below one machine epsilon."""
    return max(gamma(K + 3, U64), 2.0 ** -52)


def gemm_ref(tA, tB, alpha, A, B, beta, C, product=None, scale=None):
    """(alpha op(A) op(B) + beta C in longdouble, componentwise bar gamma_(K+3) (|alpha| |op(A)| |op(B)| + |beta| |C|)).
    A and B as stored (K x M when tA, N x K when tB).  beta == 0: C is not read (it may hold NaN).  product / scale: the
    longdouble op(A) op(B) and |op(A)| |op(B)|, if at hand."""
    opA = np.asarray(A).T if tA else np.asarray(A)
    opB = np.asarray(B).T if tB else np.asarray(B)
    M, K = opA.shape
    N = opB.shape[1]
    if product is None:
        product = _mm(opA.astype(LD), opB.astype(LD)) if K > 0 else np.zeros((M, N), dtype=LD)
    if scale is None:
        scale = np.abs(opA) @ np.abs(opB)
    ref = LD(alpha) * product
    mag = abs(alpha) * np.asarray(scale, dtype=np.float64)
    if beta != 0.0:
        ref = ref + LD(beta) * np.asarray(C).astype(LD)
        mag = mag + abs(beta) * np.abs(np.asarray(C, dtype=np.float64))
    return ref, gemm_bar_factor(K) * mag


def tps_ld(A, B):
    """(k, r2) of the thin-plate spline r^2 log(r) from direct differences, longdouble; exactly 0 at coincident points"""
    A, B = np.atleast_2d(np.asarray(A)).astype(LD), np.atleast_2d(np.asarray(B)).astype(LD)
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        diff = A[:, k][:, None] - B[:, k][None, :]
        r2 += diff * diff
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(r2 > 0, r2 * np.log(np.sqrt(np.where(r2 > 0, r2, 1))), LD(0))
    return k, r2


def tps_bar_direct(d, r2):
    """the project's bar for the spline at direct differences (tests/test_gpu_spline.py): r^2 carries (d + 8) eps r^2, and
    r^2 log(r) moves by at most that times (|log r^2| / 2 + 1)"""
    r2 = np.asarray(r2, dtype=np.float64)
    return (d + 8) * 2.0 ** -52 * r2 * (np.abs(np.log(np.maximum(r2, 1e-300))) / 2 + 1)


# ---------------------------------------------------------------------------------------------------------------------
# routes: launch_gemm (nk_gemm.hip) and launch_kmat (nk_kmat.hip) as predicates of what the forms change
# ---------------------------------------------------------------------------------------------------------------------
SMALL_MN, SMALL_K, TN_MIN_K = 32768, 1024, 128
KFLAT_DMAX, KFLAT_MIN_ENTRIES, KSMALL_MAX_ENTRIES = 8, 4096, 8192


def staged(form, cols):
    """(16-byte aligned, even leading dimension) of an fp64 operand as the kernel sees it: a host operand is repacked into
    the arena (aligned, cols rounded up to even), a device operand is used in place"""
    f = form_of(form)
    if not f.device:
        return True, True
    return f.mod16 == 0, f.ld(cols) % 2 == 0


def gemm_route(M, N, K, tA, tB, form_a="H0", form_b="H0"):
    """-> (kernel, vecA, vecB, tn_fast_ok).  kernel: 'small', 'tn' (LDS-DMA engine) or 'tile' (generic engine)."""
    a_rows, a_cols = (K, M) if tA else (M, K)
    b_rows, b_cols = (N, K) if tB else (K, N)
    al_a, ev_a = staged(form_a, a_cols)
    al_b, ev_b = staged(form_b, b_cols)
    vec_a, vec_b = al_a and ev_a, al_b and ev_b
    fast = bool(tA and not tB and M >= 2 and N >= 2 and vec_a and vec_b)  # (ld >= cols rounded up holds for every form)
    if M * N <= SMALL_MN and K <= SMALL_K:
        return "small", vec_a, vec_b, fast
    if tA and not tB and K >= TN_MIN_K and fast:
        return "tn", vec_a, vec_b, fast
    return "tile", vec_a, vec_b, fast


def kmat_route(nA, nB, d, form_a="H0", form_b="H0", form_o="H0"):
    """-> (kernel, vecA, vecB, vecO, flat gate).  kernel: 'flat', 'small' (one wave per entry) or 'tiled'."""
    vec = [al and ev for al, ev in (staged(form_a, d), staged(form_b, d), staged(form_o, nB))]
    gate = bool(vec[2] and nB % 2 == 0)  # ldo % 2 == 0 && nB % 2 == 0 && aligned16(out)
    if d <= KFLAT_DMAX and gate and (nB * d + d) * 8 <= 60 * 1024 and nA * nB >= KFLAT_MIN_ENTRIES:
        return "flat", vec[0], vec[1], vec[2], gate
    if nA * nB <= KSMALL_MAX_ENTRIES:
        return "small", vec[0], vec[1], vec[2], gate
    return "tiled", vec[0], vec[1], vec[2], gate
