"""The spline hyper-parameter sweep on the MI355X (tests/golden/make_golden_spline_cv.py -> f16_spline_cv.npz):
nk_spline_fit on the members of a lock-step group, nk_spline_cv_grid through harness.grid_search_cv(estimator="spline"),
bit for bit against the unbatched path and, unit by unit, against scikit-learn's GridSearchCV over the reference's
KoopmanSplineRegressor within the stored bars (a fixed multiple of the reference's own movement, with a floor)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
NK_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def cv(golden):
    g = golden("f16_spline_cv.npz")
    d = golden("f13_duffing_cv.npz")
    return g, np.ascontiguousarray(d["X"]), np.ascontiguousarray(d["Y"])


def candidates_of(g, tag):
    bounds = g["bounds"] if tag == "big" else None
    return [dict(gamma=float(gm), m=int(g[f"{tag}_m"]), state_bounds_params=bounds) for gm in g[f"{tag}_gammas"]]


def centers_of(g, tag):
    rec = g[f"{tag}_centers"]
    return {(c, f): rec[c, f] for c in range(rec.shape[0]) for f in range(rec.shape[1])}


def small_units(g, X):
    """the 20 units of the small search in the form LockstepPool.spline_cv_grid takes"""
    from nys_koop_lqr_amd import harness
    folds = harness.kfold_slices(X.shape[0], 5)
    return [(float(g["small_gammas"][c]), 50, folds[f], np.ascontiguousarray(g["small_centers"][c, f].T))
            for c, f in harness.cv_work_list(4, 5)]


# --------------------------------------------------------------------------- 1. the fit on members of a group
@pytest.mark.parametrize("k,side", [(0, "cholesky"), (4, "svd")])
def test_spline_fit_on_group_members_equals_ordinary_context(nk, golden, k, side):
    """Four members of a group fit the same cloth system (f15_spline_cloth case k) inside a unit of work, each from its own
    thread: A, B, C, W are the bits of the fit on an ordinary context.  Case 0 (m = 10, gamma = 1e-5) is solved by the
    blocked Cholesky, case 4 (m = 398, gamma = 1e-7) lies inside the SVD window and pinv drops two singular values."""
    from nys_koop_lqr_amd import _lib
    g = golden("f15_spline_cloth.npz")
    t = golden("cloth_trajs_all.npz")
    states, inputs = t["states_e10"] / 1e10, t["inputs"]
    X = np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in g["train"]]).T.copy()
    Y = np.hstack([states[i][:, 1:] for i in g["train"]]).T.copy()
    m, gamma = int(g["ms"][k]), float(g["gammas"][k])
    centers = X[:, :192].T[:, g[f"c{k}_centers_idx"]]

    def unit(_):
        reg = nk.KoopmanSplineRegressor(6, m=m, gamma=gamma)
        reg.centers = centers
        reg.fit(X, Y)
        return np.array(reg.A), np.array(reg.B), np.array(reg.C), np.array(reg.weights), dict(reg.fit_stats_)

    want = unit(0)
    mp = m + 6
    if side == "cholesky":
        assert want[4]["rank_inner"] == mp and want[4]["pivot_ratio_inner"] > 2.0 * mp * mp * EPS
    else:
        assert want[4]["rank_inner"] == int(g[f"c{k}_rank"]) < mp
    pool = _lib.lockstep_pool(4, index=21)
    for got in pool.run_round(unit, range(4)):
        assert got[4]["rank_inner"] == want[4]["rank_inner"]
        assert got[4]["pivot_ratio_inner"] == want[4]["pivot_ratio_inner"]
        for name, a, b in zip("ABCW", got, want):
            assert np.array_equal(a, b), (name, float(np.max(np.abs(a - b))))
    one = pool.run_round(unit, [0])[0]  # a round of one member: nobody to merge with
    assert all(np.array_equal(a, b) for a, b in zip(one[:4], want[:4]))


# --------------------------------------------------------------------------- 2. batched sweep == unbatched sweep
def test_batched_spline_sweep_is_bit_identical(nk, cv):
    from nys_koop_lqr_amd import harness
    g, X, Y = cv
    cands, centers = candidates_of(g, "small"), centers_of(g, "small")
    base = harness.grid_search_cv(X, Y, 1, cands, centers=centers, estimator="spline")
    assert np.all(np.isfinite(base["split_scores"]))
    one = harness.grid_search_cv(X, Y, 1, cands, centers=centers, estimator="spline", batch=8)
    two = harness.grid_search_cv(X, Y, 1, cands, centers=centers, estimator="spline", batch=8, batch_groups=2)
    assert np.array_equal(one["split_scores"], base["split_scores"])
    assert np.array_equal(two["split_scores"], base["split_scores"])
    assert one["best_index"] == two["best_index"] == base["best_index"]


# --------------------------------------------------------------------------- 3. parity with the reference's GridSearchCV
@pytest.mark.parametrize("tag", ["small", "big"])
def test_sweep_against_gridsearchcv_unit_by_unit(nk, cv, tag):
    """Every unit within its stored bar max(BAR_FACTOR x movement of the reference's own score, BAR_FLOOR_RMSE), relative;
    no unit left out (the reference scores all of them); the same best candidate."""
    from nys_koop_lqr_amd import harness
    g, X, Y = cv
    cands, centers = candidates_of(g, tag), centers_of(g, tag)
    res = harness.grid_search_cv(X, Y, 1, cands, centers=centers, estimator="spline", batch=32)
    ref, bar = g[f"{tag}_split_scores"], g[f"{tag}_bar"]
    sc = res["split_scores"]
    err = np.abs(sc - ref) / np.abs(ref)
    worst = np.unravel_index(np.argmax(np.where(np.isfinite(err), err / bar, np.inf)), err.shape)
    print(f"[{tag}] max relative error {np.nanmax(err):.3e}, worst unit {worst}: {err[worst]:.3e} against bar {bar[worst]:.3e}; "
          f"median error {np.nanmedian(err):.3e}, median bar {np.median(bar):.3e}; best {res['best_index']}")
    skipped = int(np.count_nonzero(~np.isfinite(ref)))
    assert skipped == 0
    assert np.all(np.isfinite(sc))
    assert np.all(err <= bar), (worst, float(err[worst]), float(bar[worst]))
    assert res["best_index"] == int(np.argmax(g[f"{tag}_mean_test_score"]))


# --------------------------------------------------------------------------- 4. schedule independence, real batching
def test_scores_do_not_depend_on_the_schedule_and_launches_merge(nk, cv):
    from nys_koop_lqr_amd import _lib
    g, X, Y = cv
    units = small_units(g, X)
    pool = _lib.lockstep_pool(8, index=22)
    s0 = pool.stats()
    fwd, st_f = pool.spline_cv_grid(X, Y, 1, units)
    s1 = pool.stats()
    rev, st_r = pool.spline_cv_grid(X, Y, 1, units[::-1])
    assert not st_f.any() and not st_r.any()
    assert np.array_equal(fwd, rev[::-1])
    merged = s1["merged_launches"] - s0["merged_launches"]
    covered = s1["member_launches_merged"] - s0["member_launches_merged"]
    single = s1["single_launches"] - s0["single_launches"]
    print(f"small search, 8 members: {merged} merged launches cover {covered} member launches, {single} single launches; "
          f"single-launch Jacobi sweeps that gave up: {_lib.runtime_counters()['jacobi_giveups']}")
    assert merged > 0
    assert 2 * covered >= covered + single  # at least half of all member launches went out in merged launches


# --------------------------------------------------------------------------- 5. a unit that is refused
def test_bad_gamma_fails_its_unit_only(nk, cv):
    from nys_koop_lqr_amd import _lib
    g, X, Y = cv
    units = small_units(g, X)[:10]
    pool = _lib.lockstep_pool(8, index=22)
    clean, st_c = pool.spline_cv_grid(X, Y, 1, units)
    bad = list(units)
    bad.insert(3, (float("nan"),) + units[3][1:])
    got, st = pool.spline_cv_grid(X, Y, 1, bad)
    assert st[3] == NK_ERR_BAD_ARG and np.isnan(got[3])
    assert not st_c.any() and not np.delete(st, 3).any()
    assert np.array_equal(np.delete(got, 3), clean)
    # what is checked before any unit runs raises instead: a fold outside the data set
    with pytest.raises(ValueError):
        pool.spline_cv_grid(X, Y, 1, [units[0][:2] + ((0, X.shape[0] + 1),) + units[0][3:]])


# --------------------------------------------------------------------------- 7. the second phase of nk_spline_cv_grid
def test_units_inside_the_svd_window_are_deferred_and_keep_their_bits(nk, golden, capfd, monkeypatch):
    """No unit of the f16 searches falls inside the SVD window (their pivot ratios are 1.6e-6 and above), so the deferral and
    the second phase get units of their own: the cloth system of f15 case 4 (n = 3030, d = 192, p = 6, its 398 recorded
    centres) over 5 folds at gamma = 1e-7 (pivot ratio 2.2e-12..2.7e-12 against a window of 7.2e-11: pseudo-inverse, pinv
    keeps 395-396 of 404 singular values) and at gamma = 1e-5 (2.2e-10..2.7e-10: Cholesky), and the m = 10 centres of case 0 at
    gamma = 1e-5, interleaved so that every round of the 8-member group holds units of all three kinds.  Every unit must
    score the bits of nk_spline_fit + nk_score_neg_rmse on an ordinary context, forwards and reversed; the five window
    units must be the ones that are run again (the sweep's own trace line and the rank-truncation counter say so), and the
    members must come back without the deferral flag."""
    from nys_koop_lqr_amd import _lib, harness
    g = golden("f15_spline_cloth.npz")
    t = golden("cloth_trajs_all.npz")
    states, inputs = t["states_e10"] / 1e10, t["inputs"]
    X = np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in g["train"]]).T.copy()
    Y = np.hstack([states[i][:, 1:] for i in g["train"]]).T.copy()
    n, d, p = X.shape[0], 192, 6
    Zbig = np.ascontiguousarray(X[g["c4_centers_idx"], :d])    # m x d
    Zsmall = np.ascontiguousarray(X[g["c0_centers_idx"], :d])
    folds = harness.kfold_slices(n, 5)
    units, kinds = [], []
    for f in range(5):
        units += [(1e-7, 398, folds[f], Zbig), (1e-5, 398, folds[f], Zbig), (1e-5, 10, folds[f], Zsmall)]
        kinds += ["svd", "cholesky", "cholesky"]

    def ordinary(unit):
        gamma, m, (lo, hi), Z = unit
        reg = nk.KoopmanSplineRegressor(p, m=m, gamma=gamma)
        reg.centers = Z.T
        reg.fit(X, Y, row_ranges=[(0, lo), (hi, n)], fetch=False)
        return reg.score_neg_rmse(X[lo:hi], Y[lo:hi]), dict(reg.fit_stats_)

    want = []
    for unit, kind in zip(units, kinds):
        sc, st = ordinary(unit)
        mp = unit[1] + p
        window = 2.0 * mp * mp * EPS
        print(f"{kind}: gamma {unit[0]:g} m {unit[1]} fold {unit[2]}: rank {st['rank_inner']}/{mp}, pivot ratio "
              f"{st['pivot_ratio_inner']:.3e} (window {window:.3e}), score {sc:.17g}")
        if kind == "svd":
            assert 0.0 < st["pivot_ratio_inner"] <= window and st["rank_inner"] < mp
        else:
            assert st["pivot_ratio_inner"] > window and st["rank_inner"] == mp
        want.append(sc)
    want = np.array(want)
    assert np.all(np.isfinite(want))

    pool = _lib.lockstep_pool(8, index=23)
    monkeypatch.setenv("NYSKOOP_CV_TRACE", "1")
    capfd.readouterr()
    for order in (slice(None), slice(None, None, -1)):
        before = _lib.runtime_counters()["rank_truncated_fits"]
        got, status = pool.spline_cv_grid(X, Y, p, units[order])
        err = capfd.readouterr().err
        assert not status.any(), status
        assert np.array_equal(got, want[order]), (got, want[order])
        assert "spline_cv_grid: 15 units" in err and " 5 rank-deficient units again" in err, err
        assert _lib.runtime_counters()["rank_truncated_fits"] - before == 5  # counted once each: in the second phase
    monkeypatch.delenv("NYSKOOP_CV_TRACE")
    # the members are left as they were: a window unit through the ordinary API on a member takes the pseudo-inverse again
    for (sc, st) in pool.run_round(ordinary, [units[0]] * 3):
        assert sc == want[0] and st["rank_inner"] < 404
    # fewer units than members, all of them deferred: the second phase runs with idle members
    got, status = pool.spline_cv_grid(X, Y, p, units[0:6:3])
    assert not status.any() and np.array_equal(got, want[0:6:3])
