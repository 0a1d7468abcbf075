"""The staging layout of the unit-table calls (csrc/nk_unit_pack.h) without a GPU: a stand-alone program
(tests/unit_pack_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan packs units the way
nk_plant_loop_multi and nk_closed_loop_multi do and prints the offsets and the block; the layout is computed here a second
time from its rules:

  slot(n) = n rounded up to 32 doubles (256 bytes); a piece copies `count` doubles and reserves slot(reserve), zero filled
  plant unit, staging block:  K reserved as m + (m & 1) | x0 and x_ref together in slot(2 d);  folded gain: slot(m + 2)
  loop unit, staging block:   K (p m) | phi0 (m) | phi_ref (m) | target (d) | u_init (p);  workspace: phi_t (steps m) | usq | sse
"""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")

PLANT_SHAPES = [(m, d) for m in (1, 2, 63, 64, 65) for d in (1, 2)]
LOOP_SHAPES = [(1, 1, 1), (31, 6, 192), (32, 1, 33), (128, 8, 1)]
STEPS = 17


def slot(n):
    return (n + 31) // 32 * 32


def value(unit, piece, i):
    return 1.0 + 100000.0 * unit + 10000.0 * piece + i


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("unit_pack") / "unit_pack_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "unit_pack_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(lines):
        """unit lines -> (offsets per unit, staging doubles, device-only doubles, block)"""
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = res.stdout.splitlines()
        assert len(out) == len(lines) + 2
        offsets = [[int(t) for t in l.split()] for l in out[:len(lines)]]
        total, dev_total = (int(t) for t in out[len(lines)].split())
        block = [float.fromhex(t) for t in out[len(lines) + 1].split()]
        return offsets, total, dev_total, block

    return run


def check_block(block, total, copied):
    """copied: [(offset, unit, piece, count)]: those ranges hold the source, every other double is +0.0"""
    assert len(block) == total
    want = [None] * total
    for off, unit, piece, count in copied:
        for i in range(count):
            assert want[off + i] is None  # ranges are disjoint
            want[off + i] = value(unit, piece, i)
    for i, (got, w) in enumerate(zip(block, want)):
        if w is None:
            assert got == 0.0 and math.copysign(1.0, got) == 1.0, (i, got)
        else:
            assert got == w, (i, got, w)


def plant_case(run, shapes, folds):
    offsets, total, dev_total, block = run([f"plant {m} {d} {int(f)}" for (m, d), f in zip(shapes, folds)])
    at, w_at, copied = 0, 0, []
    for u, ((m, d), fold) in enumerate(zip(shapes, folds)):
        k, x0, xr, w, reserve = offsets[u]
        assert reserve == m + (m & 1)
        assert all(o % 32 == 0 for o in (k, x0, w))
        assert k == at and x0 == k + slot(m + (m & 1)) and xr == x0 + d  # K | x0, x_ref, in this order
        at = x0 + slot(2 * d)
        if fold:
            assert w == w_at
            w_at += slot(m + 2)
        copied += [(k, u, 0, m), (x0, u, 1, d), (xr, u, 2, d)]
    assert total == at == sum(slot(m + (m & 1)) + slot(2 * d) for m, d in shapes)
    assert dev_total == w_at == sum(slot(m + 2) for (m, _), f in zip(shapes, folds) if f)
    check_block(block, total, copied)


def loop_case(run, shapes, nulls):
    lines = [f"loop {m} {p} {d} {STEPS} {int(not nt)} {int(not nu)}" for (m, p, d), (nt, nu) in zip(shapes, nulls)]
    offsets, total, dev_total, block = run(lines)
    at, ws_at, copied = 0, 0, []
    for u, ((m, p, d), (null_target, null_u)) in enumerate(zip(shapes, nulls)):
        assert all(o % 32 == 0 for o in offsets[u])
        k, f0, fr, tg, ui, phi, usq, sse = offsets[u]
        sizes = [p * m, m, m, d, p]
        for off, n in zip((k, f0, fr, tg, ui), sizes):  # K | phi0 | phi_ref | target | u_init
            assert off == at
            at += slot(n)
        for off, n in zip((phi, usq, sse), (STEPS * m, STEPS, STEPS)):  # phi_t | usq | sse
            assert off == ws_at
            ws_at += slot(n)
        copied += [(k, u, 0, p * m), (f0, u, 1, m), (fr, u, 2, m)]
        if not null_target:
            copied.append((tg, u, 3, d))
        if not null_u:
            copied.append((ui, u, 4, p))
    assert total == at == sum(slot(p * m) + 2 * slot(m) + slot(d) + slot(p) for m, p, d in shapes)
    assert dev_total == ws_at == sum(slot(STEPS * m) + 2 * slot(STEPS) for m, _, _ in shapes)
    check_block(block, total, copied)


@pytest.mark.parametrize("shape", PLANT_SHAPES)
def test_one_plant_unit(pack_program, shape):
    plant_case(pack_program, [shape], [True])
    plant_case(pack_program, [shape], [False])  # a spline model: no folded gain


def test_three_plant_units_of_mixed_shapes(pack_program):
    plant_case(pack_program, [(65, 2), (1, 1), (64, 2)], [True, False, True])
    plant_case(pack_program, [(63, 1), (2, 2), (65, 1)], [False, True, True])


@pytest.mark.parametrize("shape", LOOP_SHAPES)
def test_one_loop_unit(pack_program, shape):
    loop_case(pack_program, [shape], [(False, False)])


@pytest.mark.parametrize("shape", LOOP_SHAPES)
def test_loop_unit_with_null_target_and_null_u_init(pack_program, shape):
    loop_case(pack_program, [shape], [(True, True)])


def test_three_loop_units_of_mixed_shapes(pack_program):
    loop_case(pack_program, [(31, 6, 192), (1, 1, 1), (128, 8, 1)], [(False, False), (True, True), (False, True)])
    loop_case(pack_program, [(32, 1, 33), (128, 8, 1), (31, 6, 192)], [(True, False), (False, False), (False, False)])
