"""The launch classes of the multi-model closed loops (csrc/nk_loop_classes.h) without a GPU: a stand-alone program
(tests/loop_classes_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan prints the stable permutation
and the runs of equal keys the header computes, and the expected values are computed here a second time with sorted(), which
is stable, and itertools.groupby."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")


@pytest.fixture(scope="module")
def classes_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("loop_classes") / "loop_classes_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "loop_classes_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(keys, lds=None):
        """keys: (ktype, shape, waves) per unit; lds: a need per unit or None -> (perm, [(begin, end, key, lds)])"""
        rows = [k + ((lds[u],) if lds is not None else ()) for u, k in enumerate(keys)]
        text = f"{len(keys)} {int(lds is not None)}\n" + "".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        lines = [l.split() for l in res.stdout.splitlines()]
        assert lines[0][0] == "perm" and lines[-1] == ["end"] and all(l[0] == "run" for l in lines[1:-1])
        perm = [int(t) for t in lines[0][1:]]
        runs = [(int(l[1]), int(l[2]), (int(l[3]), int(l[4]), int(l[5])), int(l[6])) for l in lines[1:-1]]
        return perm, runs

    return run


def expected(keys, lds=None):
    perm = sorted(range(len(keys)), key=lambda u: keys[u])  # stable: equal keys keep the caller's order
    runs, begin = [], 0
    for key, grp in itertools.groupby(perm, key=lambda u: keys[u]):
        grp = list(grp)
        runs.append((begin, begin + len(grp), key, max(lds[u] for u in grp) if lds is not None else 0))
        begin += len(grp)
    return perm, runs


def check(classes_program, keys, lds=None):
    got, want = classes_program(keys, lds), expected(keys, lds)
    assert got == want, (keys, lds, got, want)
    perm, runs = got
    assert sorted(perm) == list(range(len(keys)))
    assert runs[0][0] == 0 and runs[-1][1] == len(keys) and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    return got


def test_one_unit(classes_program):
    assert check(classes_program, [(1, 4, 2)]) == ([0], [(0, 1, (1, 4, 2), 0)])
    assert check(classes_program, [(1, 4, 2)], [77]) == ([0], [(0, 1, (1, 4, 2), 77)])


def test_all_units_in_one_class(classes_program):
    perm, runs = check(classes_program, [(2, 1, 1)] * 7)
    assert perm == list(range(7)) and runs == [(0, 7, (2, 1, 1), 0)]


def test_all_classes_distinct(classes_program):
    """Every field decides in turn: kernel family first, then the shape, then the waves."""
    keys = [(k, s, w) for k in (3, 0, 1) for s in (4, 1) for w in (2, 16, 1)]
    perm, runs = check(classes_program, keys)
    assert len(runs) == len(keys) and [r[2] for r in runs] == sorted(keys)
    assert [keys[u] for u in perm] == sorted(keys)


def test_shuffled_mix_keeps_the_callers_order_inside_a_class(classes_program):
    rng = random.Random(5)
    classes = [(0, 1, 1), (0, 4, 1), (0, 4, 3), (1, 1, 1), (3, 4, 16), (3, 16, 2)]
    keys = [rng.choice(classes) for _ in range(50)]
    assert len(set(keys)) == len(classes)
    lds = [rng.randrange(1, 20000) for _ in keys]
    for needs in (None, lds):
        perm, runs = check(classes_program, keys, needs)
        for begin, end, key, _ in runs:
            members = perm[begin:end]
            assert members == sorted(members) and all(keys[u] == key for u in members)
            assert members == [u for u in range(50) if keys[u] == key]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_lds_maximum_of_a_run(classes_program, where):
    """Two runs of five; the largest need of each is its first, a middle or its last member."""
    keys = [(0, 16, 1), (1, 32, 2)] * 5
    at = {"first": 0, "middle": 2, "last": 4}[where]
    lds = [100 + u for u in range(10)]
    lds[2 * at] = 5000      # run of (0, 16, 1): the callers' units 0, 2, 4, 6, 8
    lds[2 * at + 1] = 7000  # run of (1, 32, 2): units 1, 3, 5, 7, 9
    perm, runs = check(classes_program, keys, lds)
    assert perm == [0, 2, 4, 6, 8, 1, 3, 5, 7, 9]
    assert runs == [(0, 5, (0, 16, 1), 5000), (5, 10, (1, 32, 2), 7000)]
