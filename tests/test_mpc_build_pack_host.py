"""The staging layout of the controller build (pack_mpc_build_unit, csrc/nk_mpc_build_pack.h) without a GPU and without
Python in the program under test: a stand-alone program (tests/mpc_build_pack_main.cpp) built with the host C++ compiler under
AddressSanitizer and UBSan packs units the way nk_mpc_build_batch and nk_model_mpc_build_batch do and prints the offsets and
the block; the layout is computed here a second time from its rules:

  slot(n) = n rounded up to 32 doubles (256 bytes); every piece is dense, starts on a slot boundary, zero beyond its doubles
  in:   A (m m) | B (m p) | Q (m m) with host operands | R (p p) when given | P (m m) when given | C_rows (nc m) with rows
  out:  H (nv nv) | F (nv m) | K (p m) | P (m m) when wanted | G (Ny nc nv) | T (Ny nc m) with rows
  ws:   the Riccati stage's K (p m) | P (m m) unless P is given | 6 M M | 5 M NVP + 48 M + 16 NVP + slot(Ny nc p),
        M, NVP = m, nv rounded up to 16
"""
import os
import shutil
import subprocess

import pytest

from test_unit_pack_host import check_block, slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")


def pad16(n):
    return (n + 15) // 16 * 16


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("mpc_build_pack") / "mpc_build_pack_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "mpc_build_pack_main.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(units):
        text = "".join(" ".join(str(int(v)) for v in u) + "\n" for u in units)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = res.stdout.splitlines()
        assert len(out) == len(units) + 2
        offsets = [[int(t) for t in l.split()] for l in out[:len(units)]]
        totals = [int(t) for t in out[len(units)].split()]
        block = [float.fromhex(t) for t in out[len(units) + 1].split()]
        return offsets, totals, block

    return run


def build_case(run, units):
    offsets, (n_in, n_out, n_ws), block = run(units)
    at_in = at_out = at_ws = 0
    copied = []
    for u, (m, p, N, nc, Ny, host_ops, have_R, have_P, want_P, host_C, extra) in enumerate(units):
        A, B, Q, R, P, Cr, H, F, K, oP, G, T, rK, rP, sq, wide = offsets[u]
        nv, ny = N * p, nc * Ny

        def piece(got, present, count, at, k=None):
            if not present:
                assert got == -1
                return at
            assert got == at and got % 32 == 0
            if k is not None:
                copied.append((got, u, k, count))
            return at + slot(count)
        at_in = piece(A, host_ops, m * m, at_in, 0)
        at_in = piece(B, host_ops, m * p, at_in, 1)
        at_in = piece(Q, host_ops, m * m, at_in, 2)
        at_in = piece(R, have_R, p * p, at_in, 3)
        at_in = piece(P, have_P, m * m, at_in, 4)
        at_in = piece(Cr, host_C and nc, nc * m, at_in, 5)
        at_out = piece(H, True, nv * nv, at_out)
        at_out = piece(F, True, nv * m, at_out)
        at_out = piece(K, True, p * m, at_out)
        at_out = piece(oP, want_P, m * m, at_out)
        at_out = piece(G, ny, ny * nv, at_out)
        at_out = piece(T, ny, ny * m, at_out)
        at_ws = piece(rK, not have_P, p * m, at_ws)
        at_ws = piece(rP, not have_P, m * m, at_ws)
        M, NVP = pad16(m), pad16(nv)
        at_ws = piece(sq, True, 6 * M * M, at_ws)
        at_ws = piece(wide, True, 5 * M * NVP + 48 * M + 16 * NVP + slot((Ny if nc else 0) * nc * p), at_ws)
    assert (n_in, n_out, n_ws) == (at_in, at_out, at_ws)
    check_block(block, n_in, copied)


# m p N nc Ny host_ops have_R have_P want_P host_C extra_ld
HOST = [(1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 0), (5, 1, 1, 1, 1, 1, 1, 1, 0, 1, 3), (17, 3, 5, 2, 3, 1, 1, 0, 1, 1, 0),
        (33, 4, 16, 4, 16, 1, 1, 0, 0, 1, 2), (64, 2, 8, 0, 0, 1, 1, 1, 1, 0, 1)]
MODEL = [(20, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0), (40, 1, 8, 2, 8, 0, 1, 0, 0, 0, 0), (31, 2, 4, 1, 2, 0, 1, 0, 0, 0, 5)]


@pytest.mark.parametrize("unit", HOST + MODEL, ids=str)
def test_one_unit_is_laid_out_by_the_rules(pack_program, unit):
    build_case(pack_program, [unit])


def test_a_mixed_group_is_laid_out_by_the_rules(pack_program):
    build_case(pack_program, HOST + MODEL)
    build_case(pack_program, MODEL + HOST[::-1])


def test_a_group_of_models_without_r_has_no_staging_block(pack_program):
    offsets, (n_in, n_out, n_ws), block = pack_program([MODEL[0], MODEL[0]])
    assert n_in == 0 and block == [] and n_out > 0 and n_ws > 0
    assert offsets[1][6] == offsets[0][6] + slot(8 * 8) + slot(8 * 20) + slot(20)  # the second unit's H follows the first's K
