"""The launch plan of the matrix-product engines (csrc/nk_gemm_plan.h) without a GPU: a stand-alone program
(tests/gemm_plan_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan prints what the header
computes, and the expected values are computed here a second time -- the three split-K choosers as transcriptions of the
launchers they were taken out of (the commit before the header existed, cited per function), run over all cases at once
with NumPy's IEEE doubles and 64-bit integers, one array entry per case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")

NUM_CU = [256, 304, 64]
NTILES = list(range(1, 701))
KTILES = list(range(0, 80)) + list(range(79 + 37, 1301, 37))
TRI_FULL, TRI_UPPER_MIRROR, TRI_LOWER = 0, 1, 2
TBM, TN_MAXP, TILE_UNUSED = 128, 4, 1 << 30


# ---- the three choosers as they stood inline in the launchers -------------------------------------------------------
def generic_splitk(ntiles, kt, num_cu):
    """nk_gemm.hip:306-314 (gemm_prepare)"""
    target = 4 * num_cu
    splitk = np.where(ntiles >= target // 2, 1, (target + ntiles - 1) // ntiles)
    splitk = np.where(splitk >= 6, ((splitk + 7) // 8) * 8, splitk)
    max_split = np.where(kt // 8 > 0, kt // 8, 1)
    splitk = np.where(splitk > max_split, max_split, splitk)
    splitk = np.where(splitk > 64, 64, splitk)
    return np.where(splitk < 1, 1, splitk)


def tn_f64_splitk(ntiles, kt, num_cu, bonus=True):
    """nk_gemm_tn.hip:561-583 (launch_gemm_tn_multi); bonus=False drops the line `if (c % 8 == 0) t *= 0.97`"""
    slots = 2 * num_cu
    max_split = np.where(kt // 8 > 1, kt // 8, 1)
    best = np.full(ntiles.shape, 1e300)
    splitk = np.ones(ntiles.shape, dtype=np.int64)
    for c in range(1, 65):
        live = c <= max_split
        wgs = ntiles * c
        steps = ((kt + c - 1) // c).astype(np.float64)
        full, rem = wgs // slots, wgs % slots
        t = full * 2.44 * steps
        t = np.where(rem > 0, t + np.where(rem <= num_cu, 2.35, 2.44) * steps, t)
        t = t * 4096.0
        if c > 1:
            t = t + wgs.astype(np.float64) * (TBM * TBM * 8.0 * 2.0) / 4.0e12 * 2.4e9
        t = t + 2000.0 * c / 8.0
        if bonus and c % 8 == 0:
            t = t * 0.97
        better = live & (t < best)
        best = np.where(better, t, best)
        splitk = np.where(better, c, splitk)
    return splitk


def tn_f32_splitk(ntiles, kt, num_cu):
    """nk_gemm_tn_f32.hip:501-515 (launch_gemm_tn_f32_multi)"""
    slots = 2 * num_cu
    splitk = np.ones(ntiles.shape, dtype=np.int64)
    best_eff = np.zeros(ntiles.shape)
    live = np.ones(ntiles.shape, dtype=bool)
    for c in (1, 2, 4, 8, 16, 24, 32, 40, 48, 56, 64):
        if c > 1:
            live = live & ~(kt // c < 8)  # break
        wgs = ntiles * c
        rounds = (wgs + slots - 1) // slots
        eff = wgs.astype(np.float64) / (rounds * slots).astype(np.float64)
        better = live & (eff > best_eff + 1e-9)
        best_eff = np.where(better, eff, best_eff)
        splitk = np.where(better, c, splitk)
        live = live & ~(eff >= 0.95)  # break
    return splitk


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "gemm_plan_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(what, records=()):
        """records (tuples of integers) -> one list of integers per record"""
        text = "".join(" ".join(str(int(v)) for v in r) + "\n" for r in records)
        res = subprocess.run([exe, what], input=text, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = [[int(t) for t in l.split()] for l in res.stdout.splitlines()]
        assert len(out) == max(len(records), 1)
        return out

    return run


@pytest.fixture(scope="module")
def chooser_grid(plan_program):
    cu, nt, kt = (a.ravel() for a in np.meshgrid(np.array(NUM_CU, dtype=np.int64), np.array(NTILES, dtype=np.int64),
                                                 np.array(KTILES, dtype=np.int64), indexing="ij"))
    got = np.array(plan_program("splitk", list(zip(nt, kt, cu))), dtype=np.int64)
    return cu, nt, kt, got


def per_cu(fn, cu, nt, kt, **kw):
    out = np.empty(nt.shape, dtype=np.int64)
    for c in NUM_CU:
        sel = cu == c
        out[sel] = fn(nt[sel], kt[sel], c, **kw)
    return out


def test_the_grid_is_the_237300_cases():
    assert len(KTILES) == 113 and KTILES[79] == 79 and KTILES[80] == 116 and KTILES[-1] == 1300
    assert len(NUM_CU) * len(NTILES) * len(KTILES) == 237300


@pytest.mark.parametrize("column,port", [(0, generic_splitk), (1, tn_f64_splitk), (2, tn_f32_splitk)],
                         ids=["generic", "tn_f64", "tn_f32"])
def test_chooser_agrees_with_the_launcher_it_came_from(chooser_grid, column, port):
    cu, nt, kt, got = chooser_grid
    want = per_cu(port, cu, nt, kt)
    bad = np.flatnonzero(got[:, column] != want)
    assert bad.size == 0, [(int(cu[i]), int(nt[i]), int(kt[i]), int(got[i, column]), int(want[i])) for i in bad[:10]]
    assert got[:, column].min() >= 1 and got[:, column].max() <= 64


def test_the_grid_sees_the_policy(chooser_grid):
    """Negative control: the fp64 cost model without its bonus for multiples of 8 disagrees with the header somewhere."""
    cu, nt, kt, got = chooser_grid
    without = per_cu(tn_f64_splitk, cu, nt, kt, bonus=False)
    differ = int(np.count_nonzero(got[:, 1] != without))
    print(f"fp64 chooser without the c % 8 bonus: {differ} of {nt.size} cases differ")
    assert differ > 0


def test_residual_partials_need_two_slices(plan_program):
    got = plan_program("resid", [(1, 0), (1, 1), (2, 1), (16, 1), (16, 0)])
    assert [g[0] for g in got] == [1, 2, 2, 16, 16]


def tiles(n):
    return (n + TBM - 1) // TBM


def tile_count(tri, tm, tn):
    """full: every tile; mirrored: the upper triangle of a square tile grid; lower (tm >= tn): the lower triangle of the
    top tn x tn grid and the full rows below it"""
    if tri == TRI_UPPER_MIRROR:
        return sum(tm - r for r in range(tm))
    if tri == TRI_LOWER:
        return sum(min(r + 1, tn) for r in range(tm))
    return tm * tn


def test_constants_and_tile_counts(plan_program):
    assert plan_program("constants") == [[TBM, TN_MAXP, TILE_UNUSED]]
    recs = [(tri, tm, tn) for tm in (1, 2, 7, 16, 17) for tn in (1, 2, 7, 16, 17) for tri in (TRI_FULL, TRI_UPPER_MIRROR, TRI_LOWER)
            if (tri == TRI_FULL) or (tri == TRI_UPPER_MIRROR and tm == tn) or (tri == TRI_LOWER and tm >= tn)]
    got = plan_program("tiles", recs)
    assert [g[0] for g in got] == [tile_count(*r) for r in recs]


LAYOUTS = [
    [(1, 1, TRI_FULL)],                                    # one tile
    [(128, 128, TRI_UPPER_MIRROR)],
    [(17 * 128, 16 * 128, TRI_FULL)],                      # 17 x 16 tiles
    [(2049, 1921, TRI_FULL)],                              # 17 x 16 tiles with edges
    [(2000, 2000, TRI_UPPER_MIRROR), (2000, 3, TRI_FULL)],
    [(2000, 2000, TRI_UPPER_MIRROR), (2000, 3, TRI_FULL), (3, 3, TRI_UPPER_MIRROR)],
    [(2000, 2000, TRI_UPPER_MIRROR), (2000, 3, TRI_FULL), (2000, 2000, TRI_FULL), (3, 2000, TRI_FULL)],  # a fit's four
    [(129, 129, TRI_FULL), (129, 129, TRI_UPPER_MIRROR), (129, 129, TRI_FULL), (129, 129, TRI_UPPER_MIRROR)],
]


def test_layout_of_one_to_four_problems(plan_program):
    got = plan_program("layout", [(len(ps),) + tuple(v for p in ps for v in p) for ps in LAYOUTS])
    for ps, g in zip(LAYOUTS, got):
        begins, tiles_n, total = g[:TN_MAXP], g[TN_MAXP:-1], g[-1]
        at = 0
        for q, (M, N, tri) in enumerate(ps):
            assert begins[q] == at and tiles_n[q] == tiles(N), (ps, g)
            at += tile_count(tri, tiles(M), tiles(N))
        assert total == at and begins[len(ps):] == [TILE_UNUSED] * (TN_MAXP - len(ps)), (ps, g)
        assert total < TILE_UNUSED


@pytest.mark.parametrize("bk", [16, 32])
def test_slice_length(plan_program, bk):
    recs = [(K, bk, s) for s in (1, 2, 8, 64) for K in (0, 1, bk - 1, bk, bk + 1, bk * s, bk * s + 1, 12288)]
    got = plan_program("slice", recs)
    for (K, _, s), (kt, klen) in zip(recs, got):
        assert kt == -(-K // bk)
        assert klen % bk == 0 and klen >= bk          # whole k-steps, never an empty slice
        assert klen * s >= K                          # the slices cover K ...
        assert klen == bk or (klen - bk) * s < kt * bk  # ... with the fewest steps per slice that do
    assert got[recs.index((bk * 8 + 1, bk, 8))] == [9, 2 * bk]
    assert got[recs.index((0, bk, 1))] == [0, bk]


def test_slab_size_and_kernel_matrix_grid(plan_program):
    recs = [(1, 2), (256, 2), (136, 16), (700, 64), (70000, 64)]
    assert [g[0] for g in plan_program("slab", recs)] == [n * s * TBM * TBM for n, s in recs]
    recs = [(tm, tn) for tm in (1, 3, 16) for tn in (1, 7, 8, 9, 16)]
    got = [g[0] for g in plan_program("kmat", recs)]
    for (tm, tn), grid in zip(recs, got):
        # workgroup b serves XCD b & 7, which owns the tile columns xcd, xcd + 8, ...: the grid holds the XCD with the most
        assert grid == 8 * tm * max(len(range(x, tn, 8)) for x in range(8))
    assert got[:4] == [8, 8, 8, 16]


def fast_ok(per16, offa, offb, lda, ldb, M, N):
    """nk_gemm_tn.hip:509-512 (tn_fast_ok, per16 = 2) and nk_gemm_tn_f32.hip:446-450 (tnf_fast_ok, per16 = 4)"""
    r = per16 - 1
    return (M >= per16 and N >= per16 and offa % 16 == 0 and offb % 16 == 0 and lda % per16 == 0 and ldb % per16 == 0
            and lda >= ((M + r) & ~r) and ldb >= ((N + r) & ~r))


@pytest.mark.parametrize("per16", [2, 4])
def test_operand_contract(plan_program, per16):
    good = (per16, 0, 0, 136, 264, 130, 258)
    recs = [good,
            (per16, 0, 0, 136, 264, per16 - 1, 258), (per16, 0, 0, 136, 264, 130, per16 - 1),  # too narrow
            (per16, 0, 0, per16, per16, per16, per16),                                          # the narrowest
            (per16, 0, 0, 137, 264, 130, 258), (per16, 0, 0, 136, 265, 130, 258),              # odd leading dimension
            (per16, 0, 0, 136 - per16, 264, 135, 258), (per16, 0, 0, 136, 264 - per16, 130, 263),  # below the rounded columns
            (per16, 0, 0, 132, 260, 129, 257),
            (per16, 8, 0, 136, 264, 130, 258), (per16, 0, 8, 136, 264, 130, 258),              # pointer offset by 8 bytes
            (per16, 16, 32, 136, 264, 130, 258)]
    if per16 == 4:
        recs += [(4, 0, 0, 134, 264, 130, 258), (4, 0, 0, 136, 262, 130, 258)]  # even, but no multiple of four
    got = [g[0] for g in plan_program("contract", recs)]
    want = [int(fast_ok(*r)) for r in recs]
    assert got == want, list(zip(recs, got, want))
    assert got[0] == 1 and got[1] == got[2] == 0 and got[3] == 1 and got[4] == got[5] == 0 and got[6] == got[7] == 0
    assert got[8] == 1 and got[9] == got[10] == 0 and got[11] == 1
