"""Where a large fit queues the factorisation of K_mm + jitter I -- beside the kernel blocks and fenced from the Gram launch
(the default), or behind the Gram launch (NYSKOOP_PREP_PAUSE=0, the schedule before it; read per fit) -- changes when the
work runs and how many workgroups the dataflow factorisations take, never what is computed: operators, iteration count and
residual are the same bits.  Shape: the smallest that takes the early schedule (n_eff >= 20000, m >= 1024, Gram-form kernel
blocks from d = 32)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, D, P, LS = 20480, 1024, 32, 2, 6.0
SWITCH = "NYSKOOP_PREP_PAUSE"
HOOK = "NYSKOOP_CHOL_FLOW_TEST_GIVEUP"


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    return nk


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20480)
    S = rng.standard_normal((N + 512, D))
    U = rng.standard_normal((N + 512, P))
    Y = np.tanh(S @ (rng.standard_normal((D, D)) * 0.9 / np.sqrt(D))) + U @ (rng.standard_normal((P, D)) * 0.1)
    return np.hstack([S, U]), Y


def _fit(nk, X, Y, centers_input=None, row_ranges=None):
    reg = nk.KoopmanNystromRegressor(P, kernel=nk.ThreeDimensionalKernel(LS, LS, LS, D), gamma=1e-5, m=M)
    reg.nystrom_centers_output = np.ascontiguousarray(Y[:M].T)
    if centers_input is not None:
        reg.nystrom_centers_input = centers_input
    reg.fit(X, Y, row_ranges=row_ranges)
    st = reg.fit_stats_
    out = [np.array(reg.A), np.array(reg.B), np.array(reg.C), np.array(reg.weights),
           np.array([st["sqrt_iters"]], dtype=np.float64), np.array([st["sqrt_residual"]])]
    assert all(np.isfinite(a).all() for a in out)
    return out


def _both_schedules(monkeypatch, run):
    """run() under the default schedule, under the old one, and under the default again (one process, one context)."""
    import chol_reference as cr
    monkeypatch.delenv(SWITCH, raising=False)
    c0 = cr.counters()
    early = run()
    c1 = cr.counters()
    monkeypatch.setenv(SWITCH, "0")
    late = run()
    c2 = cr.counters()
    monkeypatch.delenv(SWITCH)
    again = run()
    for other in (late, again):
        assert len(early) == len(other)
        for a, b in zip(early, other):
            assert a.shape == b.shape and np.array_equal(a, b)
    return early, (c0, c1, c2)


def _plain(c):
    """Both factorisations of each fit were dataflow launches, nothing gave up, no retry of the square root."""
    c0, c1, c2 = c
    assert c1[6] - c0[6] == 2 and c2[6] - c1[6] == 2, c
    assert c2[5] == c0[5] and c2[3] == c0[3], c


def test_same_bits_under_both_schedules(nk, monkeypatch, data):
    X, Y = data
    out, c = _both_schedules(monkeypatch, lambda: _fit(nk, X[:N], Y[:N]))
    _plain(c)
    assert 1 <= out[4][0] <= 40 and out[5][0] < 1e-7


def test_separate_input_landmarks(nk, monkeypatch, data):
    X, Y = data
    Zin = np.ascontiguousarray(X[M:2 * M, :D].T)
    out, c = _both_schedules(monkeypatch, lambda: _fit(nk, X[:N], Y[:N], centers_input=Zin))
    _plain(c)
    # the input landmarks are really in use: another A than with the output landmarks on both sides
    assert not np.array_equal(out[0], _fit(nk, X[:N], Y[:N])[0])


def test_two_row_ranges(nk, monkeypatch, data):
    """Two pieces of training rows with a gap between them (a fit this small gathers them into one block first; the
    ungathered route, several pieces per pass, starts at 256 MB of rows)."""
    X, Y = data
    ranges = [(0, 10000), (10512, N + 512)]
    out, c = _both_schedules(monkeypatch, lambda: _fit(nk, X, Y, row_ranges=ranges))
    _plain(c)
    # the ranges are really in use: another A than from the first N rows
    assert not np.array_equal(out[0], _fit(nk, X[:N], Y[:N])[0])


def test_two_passes(nk, monkeypatch, data):
    """A workspace budget of two passes: the Y rows are not prepared beside the X rows' kernel block (overlap_prep off), and
    only the first pass's Gram launch waits for the factorisation."""
    X, Y = data
    monkeypatch.setenv("NYSKOOP_F_BUDGET_GB", "0.16")  # 10 240 rows of the 2050-column feature matrix per pass
    out, c = _both_schedules(monkeypatch, lambda: _fit(nk, X[:N], Y[:N]))
    _plain(c)
    monkeypatch.delenv("NYSKOOP_F_BUDGET_GB")
    one_pass = _fit(nk, X[:N], Y[:N])
    # (two passes add the Gram blocks in another order than one: close, not equal)
    assert np.linalg.norm(out[0] - one_pass[0]) <= 1e-6 * np.linalg.norm(one_pass[0])
    assert not np.array_equal(out[0], one_pass[0])


def test_giveup_of_the_early_factorisation(nk, monkeypatch, data):
    """The workgroup that draws ticket 0 of the K_mm launch (one system, m extra rows) gives up: the fit returns, through the
    same recovery (square root once more on the launch-per-step chain) and with the same operators as under the old schedule,
    which are those of an undisturbed fit."""
    import chol_reference as cr
    X, Y = data
    plain = _fit(nk, X[:N], Y[:N])
    monkeypatch.setenv(HOOK, f"0,1,{M}")
    c0 = cr.counters()
    out, c = _both_schedules(monkeypatch, lambda: _fit(nk, X[:N], Y[:N]))
    monkeypatch.delenv(HOOK)
    # per fit: two dataflow launches, one of them gave up; never counted or handled as a coupled-iteration retry
    assert c[1][6] - c[0][6] == 2 and c[2][6] - c[1][6] == 2, c
    assert c[1][5] - c[0][5] == 1 and c[2][5] - c[1][5] == 1, c
    assert c[2][3] == c0[3], c
    for a, b in zip(out[:4], plain[:4]):
        assert np.array_equal(a, b)
    # flag slots, arenas and events are left usable
    for a, b in zip(_fit(nk, X[:N], Y[:N]), plain):
        assert np.array_equal(a, b)
