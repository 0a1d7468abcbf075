"""The block plan of the blocked Cholesky (csrc/nk_chol_plan.h) without a GPU: a stand-alone program
(tests/chol_plan_main.cpp, which includes nothing but that header) built with the host C++ compiler under AddressSanitizer and
UBSan prints the plan of every (m, extra) below, and everything it prints is computed here a second time from the plain
formulas, by brute force over tiles, or by a model of how the trailing-update kernel walks its tiles.

The launchers of the chain take the plan's shapes as they are: nk_chol.hip has no other engine to fall back on.  What licenses
that is test_step_shapes: every panel has at most 64 columns, every trailing update contracts over exactly 64 and has
rows >= rem, and a next diagonal block exists only behind a trailing update."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chol_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")

NB, TILE, PANEL_ROWS, TRSM_ROWS, FLOW_HDR, FLOW_MIN_M = 64, 128, 64, 16, 16, 256
ORDERS = list(range(1, 331)) + [511, 512, 513, 700, 2000]
SYSTEMS = [(m, e) for m in ORDERS for e in sorted({0, 1, 63, 64, 65, 130, m})]
PARTNERS = [(1, 0), (64, 65), (200, 2), (256, 250), (700, 130)]  # second systems of the two-system launches
ROUTE_PAIRS = [(256, 250), (256, 256), (255, 255), (250, 256), (2000, 256), (257, 1)]


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """{(m, extra): {"blocks", "flow", "trsm", "steps": [tuple of ints per step, one past the last included]}} and
    {(systems, allowed): (words, items, route)}, from ONE run of the program."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("chol_plan") / "chol_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "chol_plan_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    launches = [((s,), a) for s in SYSTEMS for a in (0, 1)]
    launches += [((s, p), a) for s in SYSTEMS for p in PARTNERS for a in (0, 1)]
    launches += [(((a_, 3), (b_, 5)), a) for a_, b_ in ROUTE_PAIRS for a in (0, 1)]
    text = "".join(f"sys {m} {e}\n" for m, e in SYSTEMS)
    for systems, allowed in launches:
        (m0, e0), (m1, e1) = systems[0], (systems[1] if len(systems) > 1 else (0, 0))
        text += f"pair {len(systems)} {m0} {e0} {m1} {e1} {allowed}\n"
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
    lines = iter(res.stdout.splitlines())
    per_system = {}
    for key in SYSTEMS:
        blocks, flow, trsm = next(lines).split(), next(lines).split(), next(lines).split()
        assert (blocks[0], flow[0], trsm[0]) == ("blocks", "flow", "trsm")
        steps = []
        for line in lines:
            if line == "end":
                break
            tok = line.split()
            assert tok[0] == "step"
            steps.append(tuple(int(t) for t in tok[1:] if t != "|"))
        per_system[key] = dict(blocks=int(blocks[1]), flow=tuple(int(t) for t in flow[1:]), trsm=int(trsm[1]), steps=steps)
    per_launch = {}
    for key in launches:
        tok = next(lines).split()
        assert tok[0] == "launch"
        per_launch[key] = tuple(int(t) for t in tok[1:])
    assert next(lines, None) is None
    return per_system, per_launch


def step_fields(step):
    """A printed step as a dict (the order of chol_plan_main.cpp)."""
    names = ("jb j0 nbj rem rows panel trail nb_next panel_wgs tiles_n tiles_m trail_wgs "
             "n_row0 n_col0 n_rows n_cols r_row0 r_col0 r_rows r_cols f_row0 f_rows f_k b_row0 b_rows b_k").split()
    assert len(step) == len(names)
    return dict(zip(names, step))


def test_blocks_and_step_shapes(plan):
    """The plain formulas, and the preconditions of the kernels that the launchers no longer test."""
    per_system, _ = plan
    for (m, extra), got in per_system.items():
        nblk = cdiv(m, NB)
        assert got["blocks"] == nblk and len(got["steps"]) == nblk + 1
        for jb, step in enumerate(got["steps"]):
            s = step_fields(step)
            assert s["jb"] == jb
            if jb == nblk:  # one past the last block: an empty step
                assert not any(step[1:]), (m, extra, step)
                continue
            j0 = NB * jb
            nbj = min(NB, m - j0)
            rem = m - j0 - nbj
            rows = rem + extra
            assert (s["j0"], s["nbj"], s["rem"], s["rows"]) == (j0, nbj, rem, rows), (m, extra, step)
            assert 1 <= nbj <= NB                                   # a panel has N = K = nbj <= 64 columns
            assert s["panel"] == int(rows > 0)
            assert s["trail"] == int(rem > 0)
            if s["trail"]:
                assert nbj == NB and rows >= rem and s["panel"]     # K = 64 exactly, M >= N, and its panel was solved
            assert s["nb_next"] == (min(NB, rem) if rem > 0 else 0)
            assert s["nb_next"] == (min(NB, m - NB * (jb + 1)) if jb + 1 < nblk else 0)
            if s["nb_next"]:
                assert s["trail"]                                   # no next diagonal block without a trailing update before it
            assert s["panel_wgs"] == (cdiv(rows, PANEL_ROWS) if rows > 0 else 0)
            # substitutions with the finished factor
            assert (s["f_row0"], s["f_rows"], s["f_k"]) == ((j0 + nbj, rem, nbj) if rem > 0 else (0, 0, 0))
            assert (s["b_row0"], s["b_rows"], s["b_k"]) == ((0, j0, nbj) if j0 > 0 else (0, 0, 0))
        assert got["trsm"] == cdiv(extra, TRSM_ROWS)


def brute_force_trail_tiles(rows, rem):
    """128 x 128 tiles of the rows x rem trailing matrix that hold an element of the lower triangle (diagonal included) of its
    leading rem x rem part or of the rows below it, element by element."""
    r, c = np.arange(rows)[:, None], np.arange(rem)[None, :]
    wanted = (r >= rem) | (c <= r)
    return sum(bool(wanted[r0:r0 + TILE, c0:c0 + TILE].any()) for r0 in range(0, rows, TILE) for c0 in range(0, rem, TILE))


def test_trailing_update_workgroups(plan):
    per_system, _ = plan
    counted = {}
    for (m, extra), got in per_system.items():
        for step in got["steps"]:
            s = step_fields(step)
            if not s["trail"]:
                assert (s["tiles_n"], s["tiles_m"], s["trail_wgs"]) == (0, 0, 0)
                continue
            key = (s["rows"], s["rem"])
            if key not in counted:
                counted[key] = brute_force_trail_tiles(*key)
            assert (s["tiles_n"], s["tiles_m"]) == (cdiv(s["rem"], TILE), cdiv(s["rows"], TILE))
            assert s["trail_wgs"] == counted[key], (m, extra, step)


def kernel_tiles64(rows, cols, tiles_n, workgroups, row0=0, col0=0):
    """The 64 x 64 sub-tiles that chol_trail_kernel_body writes for a (rows x cols) update launched with `workgroups`
    workgroups, as {(tile row, tile column): (first row, end row, first column, end column)} in the coordinates of the
    matrix the part was cut from (row0 / col0: the part's offsets).  Workgroup w owns 128-tile (tm, tn): tile row r of the
    lower set holds min(r + 1, tiles_n) tiles; each of its four waves owns one 64 x 64 quarter, and the quarter above the
    diagonal of a diagonal tile is left alone."""
    assert row0 % NB == 0 and col0 % NB == 0
    out = {}
    for w in range(workgroups):
        tm, left = 0, w
        while left >= min(tm + 1, tiles_n):
            left -= min(tm + 1, tiles_n)
            tm += 1
        tn = left
        for wm in (0, 1):
            for wn in (0, 1):
                if tm == tn and (wm, wn) == (0, 1):
                    continue
                r0, c0 = TILE * tm + NB * wm, TILE * tn + NB * wn
                if r0 >= rows or c0 >= cols:
                    continue
                key = ((r0 + row0) // NB, (c0 + col0) // NB)
                assert key not in out
                out[key] = (r0 + row0, min(r0 + NB, rows) + row0, c0 + col0, min(c0 + NB, cols) + col0)
    return out


def test_lookahead_split_partitions_the_trailing_update(plan):
    """Next block column and rest: disjoint, and together exactly what the unsplit update writes (as 64 x 64 sub-tiles with
    their clipped extents: all offsets are multiples of 64, so elements and sub-tiles say the same)."""
    per_system, _ = plan
    seen = set()
    for (m, extra), got in per_system.items():
        for step in got["steps"]:
            s = step_fields(step)
            rows, rem = s["rows"], s["rem"]
            nxt = (s["n_row0"], s["n_col0"], s["n_rows"], s["n_cols"])
            rest = (s["r_row0"], s["r_col0"], s["r_rows"], s["r_cols"])
            if not s["trail"]:
                assert nxt == rest == (0, 0, 0, 0)
                continue
            nbn = min(NB, rem)
            assert nxt == (0, 0, rows, nbn), (m, extra, step)
            assert rest == ((nbn, nbn, rows - nbn, rem - nbn) if rem > nbn else (0, 0, 0, 0)), (m, extra, step)
            if (rows, rem) in seen:
                continue
            seen.add((rows, rem))
            whole = kernel_tiles64(rows, rem, s["tiles_n"], s["trail_wgs"])
            # the unsplit update itself: every sub-tile on or below the block diagonal, none above
            assert set(whole) == {(a, b) for a in range(cdiv(rows, NB)) for b in range(cdiv(rem, NB)) if b <= a}
            parts = []
            for row0, col0, prow, pcol in (nxt, rest):
                if pcol == 0:
                    continue
                assert prow >= pcol  # each part is a trailing update in its own right
                n = cdiv(pcol, TILE)
                wgs = n * (n + 1) // 2 + (cdiv(prow, TILE) - n) * n
                parts.append(kernel_tiles64(prow, pcol, n, wgs, row0, col0))
            assert len(parts) == 1 or not set(parts[0]) & set(parts[1]), (rows, rem)
            union = {}
            for p in parts:
                union.update(p)
            assert union == whole, (rows, rem)


def test_flow_counts_and_route(plan):
    per_system, per_launch = plan
    for (m, extra), got in per_system.items():
        nblk, nex = cdiv(m, NB), cdiv(extra, NB)
        assert got["flow"] == (nblk, nex, (nblk + nex) * nblk, cr.flow_items([(m, extra)])), (m, extra)
    for (systems, allowed), (words, items, route) in per_launch.items():
        assert items == cr.flow_items(list(systems)), systems
        assert words == FLOW_HDR + sum((cdiv(m, NB) + cdiv(e, NB)) * cdiv(m, NB) for m, e in systems), systems
        assert route == int(bool(allowed) and all(m >= FLOW_MIN_M for m, _ in systems)), (systems, allowed)
    # the pairs at the threshold: the rule is "every m_q >= 256"
    for pair, want in (((256, 250), 0), ((256, 256), 1), ((255, 255), 0)):
        key = tuple((m, e) for m, e in zip(pair, (3, 5)))
        assert per_launch[(key, 1)][2] == want and per_launch[(key, 0)][2] == 0, pair
