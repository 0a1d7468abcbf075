"""The step schedule of the queued square-root iteration (csrc/nk_sqrt_schedule.h) without a GPU: a stand-alone program
(tests/sqrt_schedule_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan prints the schedule, and
the scalar model of the iteration -- a step maps every eigenvalue x of M to p(s2_k x), p(x) = x (3 - x)^2 / 4 -- is run
through it."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")
LAM_MINS = [1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 1e-12]
BOUND_FACTORS = [0.9, 0.5, 1e-2, 1e-4]
M = 500


def spectrum(lam_min):
    """500 eigenvalues: lam_min, 1 and the rest log-uniform between them (fixed seed)."""
    rng = np.random.default_rng(int(round(-math.log10(lam_min))))
    mid = 10.0 ** rng.uniform(math.log10(lam_min), 0.0, M - 2)
    return np.concatenate(([lam_min], mid, [1.0]))


def trace_frobenius_estimate(lam):
    """ns_interval_estimate for a spectrum whose largest eigenvalue is 1 (c = 1)."""
    fro, tr, m = math.sqrt(float(np.sum(lam * lam))), float(np.sum(lam)), lam.size
    lam1 = min(fro, 1.0)
    a = (tr - lam1) / (m - 1) if (m > 1 and tr > lam1) else tr / m * 1e-2
    if not (a > 0.0) or not math.isfinite(a):
        a = 1e-12
    return min(a, 1.0)


def cases():
    out = []
    for lam_min in LAM_MINS:
        lam = spectrum(lam_min)
        for a in (lam_min, 10.0 * lam_min, min(1000.0 * lam_min, 1.0), trace_frobenius_estimate(lam)):
            for f in BOUND_FACTORS:
                out.append((lam_min, a, f * lam_min))
    return out


@pytest.fixture(scope="module")
def schedule_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("sqrt_schedule") / "sqrt_schedule_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "sqrt_schedule_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(pairs):
        """[(estimate, true_lower)] -> [(kmax, s2, check)]"""
        text = "".join(f"{a!r} {lo!r}\n" for a, lo in pairs)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        lines = res.stdout.splitlines()
        assert len(lines) == 3 * len(pairs)
        out = []
        for i in range(len(pairs)):
            kmax = int(lines[3 * i])
            s2 = [float.fromhex(t) for t in lines[3 * i + 1].split()]
            check = [t == "1" for t in lines[3 * i + 2].split()]
            assert len(s2) == kmax and len(check) == kmax
            out.append((kmax, s2, check))
        return out

    run.exe = exe  # (tests/test_sqrtm_reference_host.py runs the program's other modes)
    return run


@pytest.fixture(scope="module")
def schedules(schedule_program):
    cs = cases()
    return dict(zip(cs, schedule_program([(a, lo) for _, a, lo in cs])))


def test_the_case_list_is_the_96_of_the_issue():
    assert len(cases()) == 96 and len(set(cases())) == 96


@pytest.mark.parametrize("lam_min", LAM_MINS)
def test_schedule_carries_the_scalar_model_to_convergence(schedules, lam_min):
    """For every (estimate, true lower bound): the budget stays below the cap of 100, every scaled eigenvalue stays strictly
    inside (0, 3) at every step, and some checked step k <= kmax - 1 sees sqrt(mean((lambda - 1)^2)) < 1e-7, the device's
    own bar (ns_flag_kernel)."""
    mine = [(c, s) for c, s in schedules.items() if c[0] == lam_min]
    assert len(mine) == 16
    for (_, a, lower), (kmax, s2, check) in mine:
        lam = spectrum(lam_min)
        assert lam.min() >= lower  # the bound is one
        first_pass = None
        for k in range(kmax):
            resid = math.sqrt(float(np.mean((lam - 1.0) ** 2)))
            if first_pass is None and check[k] and resid < 1e-7:
                first_pass = k
            x = s2[k] * lam
            assert x.min() > 0.0 and x.max() < 3.0, (lam_min, a, lower, k, x.min(), x.max())
            lam = x * (3.0 - x) ** 2 / 4.0
        print(f"lam_min {lam_min:g} estimate {a:.3e} bound {lower:.3e}: kmax {kmax}, first passing checked step {first_pass}")
        assert kmax < 100, (lam_min, a, lower, kmax)
        assert first_pass is not None and first_pass <= kmax - 1, (lam_min, a, lower, kmax, first_pass)


def test_first_scale_is_the_weighted_geometric_mean(schedule_program):
    """s2[0] = 3 / (a_s + sqrt(a_s) + 1) with a_s = a^0.8 bound^0.2; one unit in the last place for pow."""
    (kmax, s2, check), = schedule_program([(1e-6, 5e-7)])
    a_s = 1e-6 ** 0.8 * 5e-7 ** 0.2
    want = 3.0 / (a_s + math.sqrt(a_s) + 1.0)
    assert abs(s2[0] - want) <= math.ulp(want), (s2[0], want)
    assert not check[0] and kmax < 100
