"""The lifted recursion's route decision and error bars without a GPU.

1. csrc/nk_chain_plan.h: a stand-alone program (tests/chain_plan_main.cpp) built with the host C++ compiler under
   AddressSanitizer and UBSan prints the plan for a grid of arguments that holds every size-class boundary; the Python mirror
   (tests/rollout_reference.py) must agree everywhere, and every case of tests/test_gpu_rollout_steps.py must, on 256 compute
   units, take the route and the template instantiation its name claims.
2. the bars of tests/rollout_reference.py: a float64 NumPy emulation of the recursion (sums in chunks of 64, three orders)
   stays under the bar on every shape the GPU test runs, and every planted fault exceeds it at the last step, on every shape
   where the fault can occur.  The same for the closed loop, the lift and the fused score."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import rollout_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")
needs_ld = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.LONGDOUBLE_SKIP)

# every boundary of a size class: the register chain (m 128 / 129, m + p 160 / 161), the workgroup count (144 / 145), the KPT
# classes (256 / 257, 512 / 513, 1024 / 1025, 2048 / 2049), the controls of the multi-workgroup chain (p 64 / 65), the score
# tile (512 / 513, 4096 / 4097), the control blocks (T 237 / 238, 1025 / 1026), the batch classes (8 / 9, 16 / 17)
GRID_M = (1, 8, 64, 100, 101, 127, 128, 129, 144, 145, 200, 256, 257, 300, 512, 513, 585, 586, 1024, 1025, 2048, 2049, 4096, 4097)
GRID_P = (0, 1, 3, 7, 32, 33, 59, 60, 61, 64, 65)
GRID_T = (1, 2, 3, 20, 237, 238, 240, 1025, 1026, 1030)
GRID_BATCH = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 70)
GRID_CU = (104, 256, 304)


def grid():
    core = [(m, p, 0, T, b, cu, 0, 0, 1) for m, p, T, b, cu in itertools.product(GRID_M, GRID_P, GRID_T, GRID_BATCH, GRID_CU)]
    flags = [(m, p, dl, T, b, cu, inv, ptb, allowed)
             for m, p, dl, T, b, cu, inv, ptb, allowed in itertools.product(
                 (5, 128, 129, 513, 2049), (0, 2, 33, 65), (0, 9, 192, 5032, 5033, 7000), (1, 3, 40), (1, 3, 17, 33), GRID_CU,
                 (0, 1), (0, 1), (0, 1))]
    return core + flags


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("chain_plan") / "chain_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "chain_plan_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(rows):
        text = "".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        lines = res.stdout.splitlines()
        assert len(lines) == len(rows)
        return [tuple(int(t) for t in ln.split()) for ln in lines]
    return run


def mirror_row(m, p, dl, T, b, cu, inv, ptb, allowed):
    pl = R.chain_plan(m, p, dl, T, b, cu, bool(inv), bool(ptb), bool(allowed))
    pu = p if T > 1 else 0
    lds = R.chain_lds_bytes(pu, dl if pl.lift_in_kernel else 0, pl.tb) if pl.route == R.CHAIN else 0
    return (R.ROUTES.index(pl.route), int(pl.lift_in_kernel), pl.tb, pl.blocks, pl.kpt, pl.nt, pl.groups, pl.launches,
            pl.launches_per_step, R.traj_err_tile(m), int(R.lifted_chain_ok(m, pu, dl)), int(R.chain_mw_fits(m, pu, cu)), lds)


def test_plan_program_equals_the_mirror_on_the_grid(plan_program):
    rows = grid()
    got = plan_program(rows)
    routes = set()
    for r, g in zip(rows, got):
        assert g == mirror_row(*r), (r, g, mirror_row(*r))
        routes.add(g[0])
        if g[0] == 0:  # the chain's LDS image fits and a block holds at least one step
            assert g[12] <= R.CHAIN_LDS_MAX and g[2] >= 1
        if g[0] == 1:  # no launch of the multi-workgroup chain has more workgroups than the device has compute units
            assert g[6] * R.chain_mw_workgroups(r[0]) <= r[5]
    assert routes == {0, 1, 2, 3}


def test_plan_boundaries():
    """The classes on both sides of every boundary the issue names, on 256 compute units."""
    P = lambda m, p, T=20, b=1, **k: R.chain_plan(m, p, 0, T, b, 256, **k)
    assert P(128, 0).route == R.CHAIN and P(129, 0).route == R.MW
    assert P(128, 32).route == R.CHAIN and P(128, 33).route == R.MW and P(101, 59).route == R.CHAIN and P(100, 61).route == R.MW
    assert [P(m, 1).kpt for m in (256, 257, 512, 513, 1024, 1025, 2048)] == [4, 8, 8, 16, 16, 32, 32]
    assert P(2049, 1).route == R.STEP and P(2049, 1, b=17).route == R.GEMM
    assert P(129, 64).route == R.MW and P(129, 65).route == R.STEP
    assert P(300, 2, T=2).route == R.STEP and P(300, 2, T=3).route == R.MW
    assert (P(128, 32, T=237).blocks, P(128, 32, T=238).blocks, P(128, 32, T=238).tb) == (1, 2, 236)
    assert (P(8, 1, T=1025).blocks, P(8, 1, T=1026).blocks, P(8, 1, T=1030).tb) == (1, 2, 1024)
    assert (R.chain_mw_workgroups(144), R.chain_mw_workgroups(145)) == (9, 10)
    assert [R.traj_err_tile(m) for m in (512, 513, 585, 586, 2048, 2049, 4096, 4097)] == [8, 7, 7, 6, 2, 1, 1, 0]
    # what test_gpu_round2.py used to call "one GEMM per step" and "stepwise path" on 256 compute units
    assert P(129, 3, T=12, b=70).route == R.MW and P(200, 1, T=12, b=70).route == R.MW
    assert P(150, 0, T=12, b=3, per_trajectory_bias=True).route == R.MW
    assert P(129, 3, T=12, b=70).launches == 1 and P(129, 3, T=12, b=70, mw_allowed=False).route == R.GEMM


def test_gpu_cases_take_the_route_their_names_claim():
    seen, blocks, step_batches = set(), set(), set()
    for c in R.RECURSION_CASES:
        first, repeat = R.case_plans(c, 256)
        if c.hook:
            assert first.route == R.MW and repeat.route == c.route, (c, first, repeat)
        else:
            assert R.claimed_plan_matches(c, first), (c, first)
        if first.route == R.MW:
            seen.update(R.mw_instantiations(c.m, c.batch, 256))
        if first.route == R.CHAIN:
            blocks.add((c.m, c.p, c.T, first.tb, first.blocks))
        if c.route == R.STEP:
            step_batches.add(c.batch)
    assert seen == {(4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4), (16, 1), (16, 2), (32, 1)}
    assert (128, 32, 238, 236, 2) in blocks and (128, 32, 240, 236, 2) in blocks and (8, 1, 1030, 1024, 2) in blocks
    assert {1, 8, 9, 16} <= step_batches
    assert {c.route for c in R.RECURSION_CASES} == set(R.ROUTES)
    assert len({c.name for c in R.RECURSION_CASES}) == len(R.RECURSION_CASES)
    for c in R.LOOP_CASES:
        first = R.chain_plan(c.m, 0, 0, c.steps, c.batch, 256, per_trajectory_bias=True)
        last = R.chain_plan(c.m, 0, 0, c.steps, c.batch, 256, per_trajectory_bias=True, mw_allowed=False) if c.hook else first
        assert last.route == c.route and (not c.hook or first.route == R.MW), (c, first, last)
    assert {c.route for c in R.LOOP_CASES} == set(R.ROUTES)
    for m in R.LIFT_M:
        for d in R.LIFT_D:
            for T in R.LIFT_T:
                pl = R.chain_plan(m, R.LIFT_P, d, T, R.LIFT_BATCH, 256)
                assert pl.route == R.CHAIN and pl.lift_in_kernel, (m, d, T, pl)
    for m, tile in R.SCORE_M.items():
        assert R.traj_err_tile(m) == tile and R.SCORE_T % tile != 0
        for b in R.SCORE_BATCH:
            pl = R.chain_plan(m, R.SCORE_P, 0, R.SCORE_T, b, 256, batch_invariant=True)
            assert pl.route == R.STEP and pl.launches_per_step == {1: 1, 17: 3}[b], (m, b, pl)


# ---------------------------------------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------------------------------------
def recursion_shapes():
    """(m, p, T) of every recursion case, each once, with its control-block length."""
    out = {}
    for c in R.RECURSION_CASES:
        out.setdefault((c.m, c.p, c.T), R.chain_plan(c.m, c.p, 0, c.T, 1, 256))
    return sorted(out.items())


def test_the_issues_trial_shapes_are_among_the_cases():
    have = {k for k, _ in recursion_shapes()}
    m_p = {(m, p) for m, p, _ in have}
    assert {(128, 32, 240), (129, 3, 20), (100, 61, 20)} <= have and {(1, 0), (513, 1), (2049, 2), (128, 33), (200, 64)} <= m_p


@needs_ld
@pytest.mark.parametrize("shape,plan", recursion_shapes(), ids=lambda v: "m%d-p%d-T%d" % v if isinstance(v, tuple) and len(v) == 3 else None)
def test_recursion_bar_passes_the_emulation_and_catches_every_fault(shape, plan):
    m, p, T = shape
    batch = 2
    q = R.recursion_problem(m, p, T, batch)
    lines = []
    for order in R.ORDERS:
        Z = R.emulate(q["A"], q["B"], q["z0"], q["U"], order=order)
        rz, iz = R.worst(Z, q["Z"], q["bar"])
        rx, _ = R.worst(Z @ q["C"].T, q["x"], q["bar_x"])
        lines.append(f"{order} {rz:.3g}/{rx:.3g}")
        assert rz <= 1.0 and rx <= 1.0, (shape, order, rz, iz, rx)
    tb = plan.tb if plan.route == R.CHAIN else None
    blocks = plan.blocks if plan.route == R.CHAIN else 1
    for fault in R.FAULTS:
        if not R.fault_applies(fault, m, p, T, batch, blocks=blocks):
            continue
        Z = R.emulate(q["A"], q["B"], q["z0"], q["U"], fault=fault, tb=tb)
        rz, _ = R.worst(Z[:, -1], q["Z"][:, -1], q["bar"][:, -1])
        rx, _ = R.worst(Z[:, -1] @ q["C"].T, q["x"][:, -1], q["bar_x"][:, -1])
        lines.append(f"{fault} {rz:.3g}/{rx:.3g}")
        assert rz > 1.0, (shape, fault, rz)
        assert rx > 1.0, (shape, fault, rx)
    print(f"\n[m {m} p {p} T {T}] err / bar (Z / x): " + "; ".join(lines))


def loop_problem(m, batch, steps, shared=False):
    A, B, C = R.design(m, R.LOOP_P, R.LOOP_D, row=0.8, brow=0.2)
    K = R.gain(m, R.LOOP_P)
    phi0, _ = R.inputs(m, 0, steps, batch, seed=1)
    ref, _ = R.inputs(m, 0, steps, 1 if shared else batch, seed=2)
    return A, B, C, K, phi0, ref


@needs_ld
@pytest.mark.parametrize("m", sorted({c.m for c in R.LOOP_CASES}))
@pytest.mark.parametrize("shared", [False, True])
def test_closed_loop_bar_passes_the_emulation_and_catches_faults(m, shared):
    steps, batch = 20, 3
    A, B, C, K, phi0, ref = loop_problem(m, batch, steps, shared)
    want = R.closed_loop_ld(A, B, C, K, phi0, ref, steps)
    assert np.max(np.sum(want["M"], axis=1)) <= 1.0 + 1e-12
    for order in R.ORDERS:
        got = R.emulate_closed_loop(A, B, C, K, phi0, ref, steps, order=order)
        r = [R.worst(got[k], want[k], want[b])[0] for k, b in (("Phi", "bar"), ("x", "bar_x"), ("u", "bar_u"))]
        print(f"\n[closed loop m {m} shared {shared} {order}] err / bar (phi, x, u) {r[0]:.3g} {r[1]:.3g} {r[2]:.3g}")
        assert max(r) <= 1.0, (m, order, r)
    for fault in ("dropped_term", "stale_state_word", "neighbour_inputs", "padding_lane"):
        if fault == "neighbour_inputs" and shared:
            continue  # one reference: every trajectory has the same bias
        if fault == "padding_lane" and m % 64 == 0 and m >= R.CHAIN_ZU:
            continue
        got = R.emulate_closed_loop(A, B, C, K, phi0, ref, steps, fault=fault)
        rx = R.worst(got["x"][:, -1], want["x"][:, -1], want["bar_x"][:, -1])[0]
        ru = R.worst(got["u"][:, -1], want["u"][:, -1], want["bar_u"][:, -1])[0]
        print(f"[closed loop m {m} {fault}] err / bar (x, u) {rx:.3g} {ru:.3g}")
        assert rx > 1.0 and ru > 1.0, (m, fault, rx, ru)


def lift_problem(tag, d, m):
    family, aniso = R.LIFT_FAMILIES[tag]
    fam, par = R.G.kernel_spec(family, d, aniso)
    rng = np.random.default_rng([d, m, len(tag)])
    Zl = rng.standard_normal((m, d))
    x0 = np.vstack([Zl[:1] + 0.05 * rng.standard_normal((1, d)), rng.standard_normal((R.LIFT_BATCH - 1, d))])
    return fam, par, Zl, x0


@needs_ld
@pytest.mark.parametrize("tag", sorted(R.LIFT_FAMILIES))
@pytest.mark.parametrize("d", R.LIFT_D)
def test_lift_bar_passes_the_emulation_and_catches_faults(tag, d):
    for m in R.LIFT_M:
        fam, par, Zl, x0 = lift_problem(tag, d, m)
        K = np.asarray(R.G.kernel_ld(Zl, Zl, par, fam)[0], dtype=np.float64) + 1e-6 * np.eye(m)
        w, V = np.linalg.eigh(K)
        Sinv = (V / np.sqrt(np.maximum(w, 1e-6))) @ V.T
        want = R.lift_ld(x0, Zl, par, fam, Sinv, center=np.zeros(d) if fam == R.LINEAR else Zl.mean(axis=0))
        r = R.worst(R.emulate_lift(x0, Zl, par, fam, Sinv), want["z0"], want["bar"])[0]
        line = f"clean {r:.3g}"
        assert r <= 1.0, (tag, d, m, r)
        assert np.all(want["bar_api"] >= want["bar"])
        for fault in ("dropped_landmark", "dropped_coordinate", "neighbour_state"):
            r = R.worst(R.emulate_lift(x0, Zl, par, fam, Sinv, fault=fault), want["z0"], want["bar"])[0]
            line += f"; {fault} {r:.3g}"
            assert r > 1.0, (tag, d, m, fault, r)
        print(f"\n[lift {tag} d {d} m {m}] err / bar: {line}")


@needs_ld
@pytest.mark.parametrize("m", sorted(R.SCORE_M))
@pytest.mark.parametrize("d", R.SCORE_D)
def test_score_bound_passes_the_emulation_and_catches_faults(m, d):
    T, k = R.SCORE_T, 3
    A, B, C = R.design(m, R.SCORE_P, d)
    z0, U = R.inputs(m, R.SCORE_P, T, k)
    Z = R.emulate(A, B, z0, U)
    true = np.random.default_rng([m, d]).standard_normal((k, T, d)) * 0.5
    sse, ssim, b_sse, b_ssim = R.score_reference(Z, C, true)
    tile = R.SCORE_M[m]
    got = R.emulate_score(Z, C, true, tile)
    r = (np.abs(got[0] - sse) / b_sse).max(), (np.abs(got[1] - ssim) / b_ssim).max()
    line = f"clean {float(r[0]):.3g} {float(r[1]):.3g}"
    assert r[0] <= 1.0 and r[1] <= 1.0, (m, d, r)
    for fault in ("dropped_tail", "dropped_row"):
        got = R.emulate_score(Z, C, true, tile, fault=fault)
        r = (np.abs(got[0] - sse) / b_sse).min(), (np.abs(got[1] - ssim) / b_ssim).min()
        line += f"; {fault} {float(r[0]):.3g} {float(r[1]):.3g}"
        assert r[0] > 1.0 and r[1] > 1.0, (m, d, fault, r)
    print(f"\n[score m {m} d {d} tile {tile}] |d sse| / bound, |d ssim| / bound: {line}")
