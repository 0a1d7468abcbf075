"""The staging layout of an MPC unit with output rows (pack_mpc_out_unit, csrc/nk_unit_pack.h) without a GPU and without Python
in the program under test: a stand-alone program (tests/mpc_out_unit_pack_main.cpp) built with the host C++ compiler under
AddressSanitizer and UBSan packs units the way nk_mpc_out_loop_multi does and prints the offsets and the block; the layout is
computed here a second time from its rules:

  slot(n) = n rounded up to 32 doubles (256 bytes); a piece copies `count` doubles and reserves slot(reserve), zero filled
  nt = nv + ny
  staging block:  [Kb | S0' | lo hi dlo dhi ycomp] in slot(nt^2 + nv nt + 5 nt)
                  | [F; T]: nt rows of m with the leading dimension m + (m & 1) (a spline model: m nt dense)
                  | x0, x_ref, u_init together in slot(2 d + p) (a null u_init leaves zeros)
  device only:    the folded W, slot(m nt + 2), for a unit that has one
  a unit that shares model and descriptions with the one before it: its own slot(2 d + p) alone, every other offset shared
"""
import os
import shutil
import subprocess

import pytest

from test_unit_pack_host import check_block, slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")

LANES = {2: (1, 1), 16: (8, 8), 17: (8, 9), 64: (32, 32)}  # nt -> (nv, ny)
SHAPES = [(m, nt) for m in (1, 63, 64, 65) for nt in (2, 16, 17, 64)]


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("mpc_out_unit_pack") / "mpc_out_unit_pack_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "mpc_out_unit_pack_main.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(units):
        """units: (m, nv, ny, d, p, fold, has_u) -> (offsets per unit, staging doubles, device-only doubles, block)"""
        text = "".join(" ".join(str(int(v)) for v in u) + "\n" for u in units)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = res.stdout.splitlines()
        assert len(out) == len(units) + 2
        offsets = [[int(t) for t in l.split()] for l in out[:len(units)]]
        total, dev_total = (int(t) for t in out[len(units)].split())
        block = [float.fromhex(t) for t in out[len(units) + 1].split()]
        return offsets, total, dev_total, block

    return run


def out_case(run, units):
    offsets, total, dev_total, block = run(units)
    at, w_at, copied, ft_rows = 0, 0, [], []
    for u, (m, nv, ny, d, p, fold, has_u) in enumerate(units):
        Kb, S0t, bnd, FT, x0, xr, ui, w, ldg = offsets[u]
        if m == 0:  # shares the pieces of the unit before it: those offsets again, and its own state piece
            assert offsets[u][:4] == offsets[u - 1][:4] and w == offsets[u - 1][7]
            assert x0 == at and x0 % 32 == 0 and xr == x0 + d and ui == xr + d
            at += slot(2 * d + p)
            copied += [(x0, u, 2, d), (xr, u, 3, d)] + ([(ui, u, 4, p)] if has_u else [])
            continue
        nt = nv + ny
        consts = nt * nt + nv * nt + 5 * nt
        assert ldg == m + (m & 1)
        assert all(o % 32 == 0 for o in (Kb, FT, x0, w))
        assert Kb == at and S0t == Kb + nt * nt and bnd == S0t + nv * nt  # the constants in one piece
        at += slot(consts)
        copied.append((Kb, u, 0, consts))
        assert FT == at
        if fold:  # the rows of [F; T] with the leading dimension of a staged nt x m matrix
            at += slot(nt * ldg)
            rows = [(FT + i * ldg, i * m) for i in range(nt)]
        else:
            at += slot(m * nt)
            rows = [(FT, 0)]
        assert x0 == at and xr == x0 + d and ui == xr + d  # x0, x_ref, u_init in this order in one piece
        at += slot(2 * d + p)
        if fold:
            assert w == w_at
            w_at += slot(m * nt + 2)
        copied += [(x0, u, 2, d), (xr, u, 3, d)] + ([(ui, u, 4, p)] if has_u else [])
        ft_rows.append((u, rows, m if fold else m * nt))
    assert total == at and dev_total == w_at
    # the rows of [F; T] start inside piece 1 at i m: check them by hand, the rest with check_block's rule
    want = {}
    for u, rows, count in ft_rows:
        for off, first in rows:
            for i in range(count):
                assert off + i not in want
                want[off + i] = 1.0 + 100000.0 * u + 10000.0 * 1 + first + i
    for i, v in want.items():
        assert block[i] == v, (i, block[i], v)
    rest = [0.0 if i in want else b for i, b in enumerate(block)]
    covered = set(want)
    for off, _, _, count in copied:
        assert covered.isdisjoint(range(off, off + count))
    check_block(rest, total, copied)


@pytest.mark.parametrize("m,nt", SHAPES)
@pytest.mark.parametrize("has_u", [True, False])
def test_one_unit_with_rows(pack_program, m, nt, has_u):
    nv, ny = LANES[nt]
    for d, p in ((2, 1), (4, 4)):
        if nv % p:
            continue
        out_case(pack_program, [(m, nv, ny, d, p, True, has_u)])
        out_case(pack_program, [(m, nv, ny, d, p, False, has_u)])  # a spline model: no fold, [F; T] dense


def test_units_that_share_prepared_pieces(pack_program):
    """Two units behind a full one reuse its constants, [F; T] and fold and add 2 d + p doubles each."""
    out_case(pack_program, [(65, 8, 9, 2, 1, True, True), (0, 8, 9, 2, 1, True, False), (0, 8, 9, 2, 1, True, True),
                            (63, 4, 4, 4, 4, False, True), (0, 4, 4, 4, 4, False, True)])


def test_mixed_units_in_one_pack(pack_program):
    out_case(pack_program, [(65, 8, 9, 2, 1, True, False), (1, 1, 1, 2, 1, True, True), (64, 32, 32, 2, 1, False, True),
                            (63, 8, 8, 2, 1, True, True), (64, 1, 1, 2, 1, False, False)])
