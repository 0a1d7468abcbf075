"""CPU: polynomial plants a user describes as a table of monomials (nk.PolynomialSystem; csrc/nk_poly_plant.h behind
nk_poly_plant_step): the reference's recorded Duffing and HJB runs replayed through the tables, the Python arithmetic against
the library's host build bit for bit, the double integrator against its closed form, every validation rule, pickling, and a
stand-alone program (tests/poly_plant_main.cpp) built with the host C++ compiler under AddressSanitizer and UBSan that sends
the tables and every malformed description through the header."""
import copy
import ctypes as C
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

from conftest import relf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")

# ---- the test plants as (row, coef, state exponents, input exponents) ------------------------------------------------------
# P2: Duffing with a second input in the first row; the origin is an unstable equilibrium
P2 = [(0, 1.0, (0, 1), (0, 0)), (1, -0.5, (0, 1), (0, 0)), (1, -4.0, (3, 0), (0, 0)), (1, 1.0, (1, 0), (0, 0)),
      (1, 0.5, (0, 0), (1, 0)), (0, 0.3, (0, 0), (0, 1))]
# P3: x1' = x2, x2' = x3, x3' = -x1 - 2 x2 - 2 x3 - x1^3 + u
P3 = [(0, 1.0, (0, 1, 0), (0,)), (1, 1.0, (0, 0, 1), (0,)), (2, -1.0, (1, 0, 0), (0,)), (2, -2.0, (0, 1, 0), (0,)),
      (2, -2.0, (0, 0, 1), (0,)), (2, -1.0, (3, 0, 0), (0,)), (2, 1.0, (0, 0, 0), (1,))]
# P4: x1' = x2, x2' = -x1 - 0.5 x2 - x1^3 + 0.2 x3 + u1, x3' = x4, x4' = -x3 - 0.5 x4 - x3^2 x4 + 0.2 x1 + u2
P4 = [(0, 1.0, (0, 1, 0, 0), (0, 0)), (1, -1.0, (1, 0, 0, 0), (0, 0)), (1, -0.5, (0, 1, 0, 0), (0, 0)),
      (1, -1.0, (3, 0, 0, 0), (0, 0)), (1, 0.2, (0, 0, 1, 0), (0, 0)), (1, 1.0, (0, 0, 0, 0), (1, 0)),
      (2, 1.0, (0, 0, 0, 1), (0, 0)), (3, -1.0, (0, 0, 1, 0), (0, 0)), (3, -0.5, (0, 0, 0, 1), (0, 0)),
      (3, -1.0, (0, 0, 2, 1), (0, 0)), (3, 0.2, (1, 0, 0, 0), (0, 0)), (3, 1.0, (0, 0, 0, 0), (0, 1))]
# P4b: P4 with four inputs, 0.3 u3 in the first row and 0.3 u4 in the third
P4B = [(r, c, ex, tuple(eu) + (0, 0)) for r, c, ex, eu in P4] + [(0, 0.3, (0, 0, 0, 0), (0, 0, 1, 0)),
                                                                   (2, 0.3, (0, 0, 0, 0), (0, 0, 0, 1))]
PLANTS = {"P2": (2, 2, P2), "P3": (3, 1, P3), "P4": (4, 2, P4), "P4b": (4, 4, P4B)}


def make_plant(name, rk4="classic", Ts=0.01):
    import nys_koop_lqr_amd as nk
    d, p, terms = PLANTS[name]
    return nk.PolynomialSystem(d, p, terms, Ts, rk4=rk4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def _replay_both(plant, x0, controls):
    """x_{t+1} = step(x_t, u_t) over the columns of `controls` through update_SOM and through nk_poly_plant_step, each on its
    own states; returns the two state arrays (d x (T + 1)) and whether they agreed bit for bit at every step."""
    xa = np.asarray(x0, dtype=np.float64).reshape(-1)
    xb = xa.copy()
    A, B, same = [xa], [xb], True
    for t in range(controls.shape[1]):
        xa = plant.update_SOM(xa, controls[:, t]).reshape(-1)
        xb = plant.step_library(xb, controls[:, t])
        same = same and np.array_equal(xa, xb)
        A.append(xa)
        B.append(xb)
    return np.array(A).T, np.array(B).T, same


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_duffing_table_replays_the_reference_trajectory(lib, golden, seed):
    """f12: the reference's open-loop replay of `lqr_us_{seed}` from (-0.5, 0), Ts = 0.01, 2000 steps, through the Duffing
    TABLE (products multiplied out: a reordered evaluation of the reference's nested form).  Host arithmetic in the
    specified order gives 9.4e-16 / 9.9e-13 / 2.6e-17 relative Frobenius for seeds 0 / 1 / 2; the bar is 1e-11, ten times the
    largest.  update_SOM and nk_poly_plant_step agree bit for bit at every step."""
    import nys_koop_lqr_amd as nk
    g = golden("f12_duffing_full.npz")
    us, ref = g[f"lqr_us_{seed}"], g[f"lqr_states_{seed}"]
    plant = nk.PolynomialSystem.duffing(0.01)
    assert plant.rk4 == "reference" and plant.n_states == 2 and plant.n_inputs == 1 and plant.terms[2][:2] == (1, -4.0)
    A, B, same = _replay_both(plant, [-0.5, 0.0], us)
    e_np, e_lib = relf(A, ref), relf(B, ref)
    print(f"\nduffing table seed {seed}: update_SOM {e_np:.2e}, nk_poly_plant_step {e_lib:.2e} from the reference's states")
    assert same and e_np < 1e-11 and e_lib < 1e-11


def test_hjb_table_replays_the_reference_trajectory(lib, golden):
    """f8: the states the reference's plant-in-the-loop run visited from 0.9 under `cl_u`, Ts = 0.01, through the HJB table:
    distance exactly 0 in the specified order; bar 1e-11 as for the Duffing table."""
    import nys_koop_lqr_amd as nk
    g = golden("f8_hjb_config2.npz")
    us, ref = g["cl_u"].reshape(1, -1), g["cl_x"]
    plant = nk.PolynomialSystem.hjb(0.01)
    A, B, same = _replay_both(plant, [0.9], us)
    e_np, e_lib = relf(A[0, :-1], ref), relf(B[0, :-1], ref)
    print(f"\nhjb table: update_SOM {e_np:.2e}, nk_poly_plant_step {e_lib:.2e} from the reference's states")
    assert same and e_np < 1e-11 and e_lib < 1e-11


@pytest.mark.parametrize("rk4", ["classic", "reference"])
@pytest.mark.parametrize("name", ["P2", "P3", "P4", "P4b"])
def test_python_and_library_steps_agree_bit_for_bit(lib, name, rk4):
    """200 random (x, u) in [-1, 1]: update_SOM on one state, update_SOM on all states at once (NumPy rows) and
    nk_poly_plant_step give identical bits; the two Runge-Kutta variants differ from each other."""
    plant = make_plant(name, rk4)
    d, p = plant.n_states, plant.n_inputs
    rng = np.random.default_rng(17)
    X, U = rng.uniform(-1, 1, size=(d, 200)), rng.uniform(-1, 1, size=(p, 200))
    batched = plant.update_SOM(X, U)
    assert batched.shape == (d, 200)
    other = make_plant(name, "reference" if rk4 == "classic" else "classic")
    differ = False
    for i in range(200):
        one = plant.update_SOM(X[:, i], U[:, i])
        lib_one = plant.step_library(X[:, i], U[:, i])
        assert one.shape == (d, 1)
        assert np.array_equal(one.reshape(-1), lib_one) and np.array_equal(batched[:, i], lib_one), i
        differ = differ or not np.array_equal(other.step_library(X[:, i], U[:, i]), lib_one)
    assert differ


def test_double_integrator_table_closed_form(lib):
    """For a constant input both Runge-Kutta variants are exact on the double integrator: x2' = x2 + Ts u, x1' = x1 + Ts x2 +
    Ts^2 u / 2.  Bar 1e-14 relative (rounding only), 300 steps chained, as for the built-in plant."""
    import nys_koop_lqr_amd as nk
    rng = np.random.default_rng(5)
    for Ts in (0.01, 0.05):
        plant = nk.PolynomialSystem.double_integrator(Ts)
        for _ in range(5):
            x = rng.uniform(-1.0, 1.0, size=2)
            u = float(rng.uniform(-2.0, 2.0))
            xa, xb, xc = x.copy(), x.copy(), x.copy()
            for _ in range(300):
                xa = plant.update_SOM(xa, u).reshape(-1)
                xb = plant.step_library(xb, [u])
                xc = np.array([xc[0] + Ts * xc[1] + Ts * Ts * u / 2, xc[1] + Ts * u])
            assert relf(xa, xc) < 1e-14 and relf(xb, xc) < 1e-14, (relf(xa, xc), relf(xb, xc))


def test_van_der_pol_table(lib):
    """x1' = x2, x2' = mu (1 - x1^2) x2 - x1 + u under classical RK4 against the same step written out with NumPy scalars
    in another order: 1e-13 relative over 500 chained steps (rounding only; one step's error is a few eps)."""
    import nys_koop_lqr_amd as nk
    mu, Ts = 1.5, 0.01
    plant = nk.PolynomialSystem.van_der_pol(mu, Ts)
    assert plant.rk4 == "classic"
    f = lambda x, u: np.array([x[1], mu * (1 - x[0] ** 2) * x[1] - x[0] + u])
    xa = xb = np.array([0.5, -0.2])
    for t in range(500):
        u = 0.3 * np.cos(0.05 * t)
        xa = plant.step_library(xa, [u])
        k1 = f(xb, u); k2 = f(xb + Ts / 2 * k1, u); k3 = f(xb + Ts / 2 * k2, u); k4 = f(xb + Ts * k3, u)
        xb = xb + Ts / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    assert relf(xa, xb) < 1e-13, relf(xa, xb)


# ---- validation -----------------------------------------------------------------------------------------------------------
def _malformed():
    """(label, mutation of a valid P4 description, what the message must name).  With d = 3 the first offending term is
    term 6 (x3' = x4), which uses the fourth state."""
    def term(i, **kw):
        def f(ds):
            for k, v in kw.items():
                if k in ("ex", "eu"):
                    getattr(ds.terms[i], k)[v[0]] = v[1]
                else:
                    setattr(ds.terms[i], k, v)
        return f

    def field(**kw):
        return lambda ds: [setattr(ds, k, v) for k, v in kw.items()]

    return [("d = 0", field(d=0), "d ="), ("d = 5", field(d=5), "d ="), ("p = 0", field(p=0), "p ="),
            ("p = 5", field(p=5), "p ="), ("n_terms = 0", field(n_terms=0), "n_terms"),
            ("n_terms = 33", field(n_terms=33), "n_terms"), ("row = -1", term(3, row=-1), "term 3"),
            ("row = d", term(5, row=4), "term 5"), ("ex beyond d", field(d=3), "term 6"),
            ("eu beyond p", term(2, eu=(2, 1)), "term 2"), ("degree 6", term(9, ex=(0, 3)), "term 9"),
            ("coef nan", term(1, coef=float("nan")), "term 1"), ("coef inf", term(11, coef=float("inf")), "term 11"),
            ("Ts nan", field(Ts=float("nan")), "Ts"), ("Ts = 0", field(Ts=0.0), "Ts"), ("Ts < 0", field(Ts=-0.01), "Ts"),
            ("Ts inf", field(Ts=float("inf")), "Ts"), ("k4_at_k1 = 2", field(k4_at_k1=2), "k4_at_k1"),
            ("k4_at_k1 = -1", field(k4_at_k1=-1), "k4_at_k1")]


def _mutated(mutate):
    from nys_koop_lqr_amd import _lib
    ds = _lib.PolyPlant()
    C.memmove(C.byref(ds), C.byref(make_plant("P4").descriptor()), C.sizeof(ds))
    mutate(ds)
    return ds


def test_every_validation_rule(lib):
    """Each rule of the description (include/nyskoop.h) is NK_ERR_BAD_ARG with the field or the term index in the message, the
    output is left alone, and the valid description still steps afterwards."""
    x, u = np.full(4, 0.1), np.full(4, 0.2)
    for label, mutate, names in _malformed():
        ds = _mutated(mutate)
        out = np.full(4, 7.0)
        rc = lib.nk_poly_plant_step(ds, x.ctypes.data, u.ctypes.data, out.ctypes.data)
        msg = lib.nk_last_error().decode()
        assert rc == -1 and names in msg and "nk_poly_plant_step" in msg, (label, rc, msg)
        assert np.all(out == 7.0), label
    assert lib.nk_poly_plant_step(None, x.ctypes.data, u.ctypes.data, x.ctypes.data) == -1
    ok = _mutated(lambda ds: None)
    assert lib.nk_poly_plant_step(ok, None, u.ctypes.data, x.ctypes.data) == -1
    out = np.zeros(4)
    assert lib.nk_poly_plant_step(ok, x.ctypes.data, u.ctypes.data, out.ctypes.data) == 0
    assert np.array_equal(out, make_plant("P4").update_SOM(x, u[:2]).reshape(-1))


def test_python_class_reports_bad_tables_as_value_errors(lib):
    import nys_koop_lqr_amd as nk
    with pytest.raises(ValueError, match="term 0"):
        nk.PolynomialSystem(2, 1, [(2, 1.0, (1, 0), (0,))], 0.01)
    with pytest.raises(ValueError, match="term 1"):
        nk.PolynomialSystem(2, 1, [(0, 1.0, (1, 0), (0,)), (1, 1.0, (3, 3), (0,))], 0.01)
    with pytest.raises(ValueError, match="n_terms"):
        nk.PolynomialSystem(2, 1, [], 0.01)
    with pytest.raises(ValueError, match="n_terms"):
        nk.PolynomialSystem(1, 1, [(0, 1.0, (1,), (0,))] * 33, 0.01)
    with pytest.raises(ValueError, match="Ts"):
        nk.PolynomialSystem(1, 1, [(0, 1.0, (1,), (0,))], 0.0)
    with pytest.raises(ValueError, match="d ="):
        nk.PolynomialSystem(5, 1, [(0, 1.0, (1,), (0,))], 0.01)
    with pytest.raises(ValueError, match="rk4"):
        nk.PolynomialSystem(1, 1, [(0, 1.0, (1,), (0,))], 0.01, rk4="heun")


def test_pickle_and_deepcopy_keep_the_descriptor(lib):
    plant = make_plant("P4b", "reference", Ts=0.02)
    want = bytes(plant.descriptor())
    x, u = np.linspace(-0.4, 0.5, 4), np.linspace(0.3, -0.2, 4)
    for other in (pickle.loads(pickle.dumps(plant)), copy.deepcopy(plant)):
        assert other is not plant and other._desc is None  # built on demand
        assert bytes(other.descriptor()) == want
        assert other.terms == plant.terms and other.rk4 == "reference" and other.Ts == 0.02
        assert np.array_equal(other.step_library(x, u), plant.step_library(x, u))


def test_plant_snapshots_for_any_plant(lib):
    """harness.plant_snapshots: X = [state | input], Y = next state, for a polynomial plant with four inputs and for a
    built-in plant with one; the draws are states first, then inputs."""
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    for plant, d, p in ((make_plant("P4b"), 4, 4), (nk.DuffingOscillator(Ts=0.01), 2, 1)):
        X, Y = harness.plant_snapshots(plant, 30, np.random.default_rng(3), bound=0.8, u_bound=2.0)
        assert X.shape == (30, d + p) and Y.shape == (30, d) and X.flags.c_contiguous and Y.flags.c_contiguous
        rng = np.random.default_rng(3)
        assert np.array_equal(X[:, :d], rng.uniform(-0.8, 0.8, size=(d, 30)).T)
        assert np.array_equal(X[:, d:], rng.uniform(-2.0, 2.0, size=(p, 30)).T)
        for i in (0, 29):
            assert np.array_equal(Y[i], plant.update_SOM(X[i, :d], X[i, d:]).reshape(-1))


def test_control_scores_with_several_inputs():
    """harness.control_scores over p = 2 inputs against the definition written out with exact sums (math.fsum) of the same
    rounded terms: every partial sum is rounded once, so 2 (n + 1) eps relative for a sum of n non-negative terms."""
    import math
    from nys_koop_lqr_amd import harness
    rng = np.random.default_rng(9)
    steps = 50
    xs, us, uo = rng.standard_normal((3, steps + 1)), rng.standard_normal((2, steps)), rng.standard_normal((steps, 2))
    sc = harness.control_scores(xs, us, uo)
    assert sc == harness.control_scores(xs, np.ascontiguousarray(us.T), uo)  # (steps, p) controls
    eps = np.finfo(np.float64).eps
    sse, sso = math.fsum(((us.T - uo) ** 2).ravel()), math.fsum((uo ** 2).ravel())
    J = math.fsum((xs ** 2).ravel()) + math.fsum((us ** 2).ravel())
    assert abs(sc["sse_u"] - sse) <= 2 * (2 * steps + 1) * eps * sse and abs(sc["ss_opt"] - sso) <= 2 * (2 * steps + 1) * eps * sso
    assert abs(sc["J"] - J) <= 2 * (5 * steps + 4) * eps * J and sc["u_absmax"] == np.max(np.abs(us))
    us[1, 7] = np.nan
    assert math.isnan(harness.control_scores(xs, us)["u_absmax"])


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plant_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path_factory.mktemp("poly_plant") / "poly_plant_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "poly_plant_main.cpp"), "-o", exe]
    # the sanitizer runtimes inside the program where the compiler has them as archives (GCC's flags; Clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        res = subprocess.run(cmd + static, capture_output=True, text=True, timeout=300)
        if res.returncode == 0:
            break
    assert res.returncode == 0, res.stderr[-3000:]

    def run(cases):
        """cases: (descriptor, x (4,), u (4,)) -> one output line per case"""
        lines = []
        for ds, x, u in cases:
            n_lines = min(max(int(ds.n_terms), 0), 32)
            if int(ds.n_terms) > 32 or int(ds.n_terms) < 1:
                n_lines = 12  # the term lines of P4, with a count that is out of range
            lines.append(f"{ds.d} {ds.p} {ds.n_terms} {ds.k4_at_k1} {float(ds.Ts).hex() if np.isfinite(ds.Ts) else ds.Ts} {n_lines}")
            for i in range(n_lines):
                t = ds.terms[i]
                coef = float(t.coef).hex() if np.isfinite(t.coef) else repr(float(t.coef))
                lines.append(f"{t.row} {' '.join(str(v) for v in t.ex)} {' '.join(str(v) for v in t.eu)} {coef}")
            lines.append(" ".join(float(v).hex() for v in list(x) + list(u)))
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
        out = res.stdout.splitlines()
        assert len(out) == len(cases), out
        return out

    return run


def test_sanitized_program_steps_the_tables_and_rejects_every_malformed_one(lib, plant_program):
    """The header alone, compiled by the host compiler with -fsanitize=address,undefined: the valid tables (the four test
    plants and the three built-in plants as tables, both Runge-Kutta variants) give the bits of update_SOM; every malformed
    description is rejected with the message of the library, and nothing is read or written out of bounds on the way."""
    import nys_koop_lqr_amd as nk
    rng = np.random.default_rng(23)
    plants = [make_plant(n, r) for n in PLANTS for r in ("classic", "reference")]
    plants += [nk.PolynomialSystem.duffing(0.01), nk.PolynomialSystem.hjb(0.01), nk.PolynomialSystem.double_integrator(0.05),
               nk.PolynomialSystem.van_der_pol(2.0, 0.02)]
    cases, want = [], []
    for pl in plants:
        x, u = np.zeros(4), np.zeros(4)
        x[:pl.n_states], u[:pl.n_inputs] = rng.uniform(-1, 1, pl.n_states), rng.uniform(-1, 1, pl.n_inputs)
        cases.append((pl.descriptor(), x, u))
        want.append(pl.update_SOM(x[:pl.n_states], u[:pl.n_inputs]).reshape(-1))
    bad = _malformed()
    cases += [(_mutated(mutate), np.full(4, 0.1), np.full(4, 0.2)) for _, mutate, _ in bad]
    out = plant_program(cases)
    for line, w in zip(out, want):
        tok = line.split()
        assert tok[0] == "ok" and len(tok) == 1 + w.size, line
        assert np.array_equal(np.array([float.fromhex(t) for t in tok[1:]]), w), (line, w)
    for line, (label, _, names) in zip(out[len(want):], bad):
        assert line.startswith("bad ") and names in line, (label, line)
