"""Counterparts of the callers either side of the fit in the reference's benchmark drivers
(benchmark_lqr_cloth.py / _classic.py / _hjb.py): open-loop validation, the (kernel, gamma, m) x K-fold
hyper-parameter sweep, the lifted closed loop, and the cloth data-matrix assembly.  Heavy loops run on the device
through the estimator's C-ABI calls; bookkeeping stays in Python.
"""
import itertools

import numpy as np

from . import _lib
from .regressors import KoopmanNystromRegressor, KoopmanSplineRegressor


def open_loop_forecast(regressor, true_trajectory, test_controls):
    """The simulated trajectory of validate_dyn_sys (benchmark_lqr_cloth.py:23-32): lift the first state, then
    z <- A z + B u_i for i < T-1, x = C z; T = number of columns of the true trajectory.  Only the first T-1 control
    columns are used, so `test_controls` may have T-1 columns (benchmark_lqr_hjb.py:129-139 builds them that way) or more."""
    T = true_trajectory.shape[1]
    U = np.asarray(test_controls, dtype=np.float64)[:, :T]
    if U.shape[1] < T - 1:
        raise ValueError(f"{T - 1} control columns needed, got {U.shape[1]}")
    if U.shape[1] == T - 1:  # the rollout call takes one column per state; the last one is never read
        U = np.hstack((U, np.zeros((U.shape[0], 1))))
    return regressor.rollout(true_trajectory[:, 0], U)


def validate_dyn_sys(regressor, true_trajectory, test_controls, relative=False):
    """benchmark_lqr_cloth.py:18-36 (absolute RMSE, :34); relative=True gives the %-form of
    benchmark_lqr_classic.py:39 / benchmark_lqr_hjb.py:42."""
    sim = open_loop_forecast(regressor, true_trajectory, test_controls)
    if relative:
        return np.sqrt(np.sum(np.square(true_trajectory - sim))) / np.sqrt(np.sum(np.square(sim))) * 100
    return np.sqrt(np.mean(np.square(true_trajectory - sim)))


def validate_dyn_sys_all(regressor, true_trajectories, test_controls, relative=False):
    """validate_dyn_sys for ALL test trajectories in one device call (the reference loops over them,
    benchmark_lqr_cloth.py:171-176, benchmark_lqr_hjb.py:296-305): trajectories (k, d, T) with controls (k, p, T) or
    (k, p, T-1) -> k errors.  The trajectories of a batch do not influence each other (same bits as one call each)."""
    trajs = np.asarray(true_trajectories, dtype=np.float64)
    ctrl = np.asarray(test_controls, dtype=np.float64)
    k, d, T = trajs.shape
    if ctrl.shape[0] != k or ctrl.shape[2] < T - 1:
        raise ValueError(f"controls have shape {ctrl.shape}, expected ({k}, p, >= {T - 1})")
    U = np.zeros((k, T, ctrl.shape[1]))
    U[:, : min(T, ctrl.shape[2]), :] = np.transpose(ctrl[:, :, :T], (0, 2, 1))
    if not hasattr(regressor, "_ensure_model"):  # an estimator without a device model (the exact-kernel comparator)
        return np.array([validate_dyn_sys(regressor, trajs[i], ctrl[i], relative) for i in range(k)])
    sims = np.transpose(regressor.rollout(np.ascontiguousarray(trajs[:, :, 0]), U), (0, 2, 1))  # (k, d, T)
    if relative:
        return np.sqrt(np.sum(np.square(trajs - sims), axis=(1, 2))) / np.sqrt(np.sum(np.square(sims), axis=(1, 2))) * 100
    return np.sqrt(np.mean(np.square(trajs - sims), axis=(1, 2)))


def kfold_slices(n, n_splits=5):
    """sklearn KFold(n_splits) without shuffling (GridSearchCV's default cv): contiguous test folds, the first
    n % n_splits folds one element longer."""
    sizes = np.full(n_splits, n // n_splits, dtype=int)
    sizes[: n % n_splits] += 1
    out, cur = [], 0
    for s in sizes:
        out.append((cur, cur + int(s)))
        cur += int(s)
    return out


def parameter_grid(grid):
    """Candidates in sklearn ParameterGrid order: keys sorted, last key fastest."""
    keys = sorted(grid)
    return [dict(zip(keys, vals)) for vals in itertools.product(*(grid[k] for k in keys))]


def cv_work_list(n_candidates, n_splits):
    """(candidate, fold) units in GridSearchCV's evaluation order (candidate-major)."""
    return [(c, f) for c in range(n_candidates) for f in range(n_splits)]


def spline_centers_draw(params, train_states, rng=None):
    """The centres a cloned KoopmanSplineRegressor draws at the first `lift` of its `fit` (regressors.py:187-197,
    compute_centers on the training states), draw for draw from the global legacy RNG: two np.random.uniform calls when
    the candidate has `state_bounds_params`, one np.random.choice over the training rows otherwise.  train_states:
    n_train x d rows.  rng: a np.random.RandomState to draw from instead of the global one.  Returns the reference's
    `centers` attribute, d x m.  Needs no GPU."""
    rng = np.random if rng is None else rng
    m = int(params["m"])
    bounds = params.get("state_bounds_params")
    if bounds is not None:
        length = np.sqrt(rng.uniform(0, bounds[0], size=(1, m)))
        angle = np.pi * rng.uniform(0, bounds[1], size=(1, m))
        return np.vstack((length * np.cos(angle), length * np.sin(angle)))
    train_states = np.asarray(train_states)
    idx = rng.choice(np.arange(0, train_states.shape[0]), size=m, replace=False)
    return train_states[idx].T


def _check_estimator(estimator):
    if estimator not in ("nystrom", "spline"):
        raise ValueError(f"estimator must be 'nystrom' or 'spline', got {estimator!r}")


def cv_unit_score(X, Y, n_inputs, params, fold, centers_idx=None, error_score=np.nan, estimator="nystrom"):
    """One (candidate, fold) unit: fit on the training rows (two contiguous ranges, no copy), score the held-out
    rows with sklearn's 'neg_root_mean_squared_error' reduced on the device.  A fit that fails numerically
    (LinAlgError: only possible in strict mode, or when the square-root iteration diverges) scores `error_score`,
    like GridSearchCV's default error_score=nan; error_score='raise' re-raises.
    estimator='spline': `params` has gamma, m and optionally state_bounds_params, and `centers_idx` is the unit's d x m
    centre array (None: drawn by the fit from the training states, as the reference does)."""
    _check_estimator(estimator)
    n = X.shape[0]
    lo, hi = fold
    n_train = n - (hi - lo)
    if estimator == "spline":
        reg = KoopmanSplineRegressor(n_inputs, state_bounds_params=params.get("state_bounds_params"), m=params["m"],
                                     gamma=params["gamma"])
        if centers_idx is not None:
            reg.centers = np.asarray(centers_idx, dtype=np.float64)
    else:
        reg = KoopmanNystromRegressor(n_inputs, **params)
        if centers_idx is None:  # what clone()+fit does in the reference: fresh draw from the global legacy RNG
            centers_idx = np.random.choice(np.arange(0, n_train), size=reg.m, replace=False)
        centers_idx = np.asarray(centers_idx)
        rows = np.where(centers_idx < lo, centers_idx, centers_idx + (hi - lo))  # training-row index -> dataset row
        reg.nystrom_centers_output = np.asarray(Y)[rows].T
    try:
        reg.fit(X, Y, row_ranges=[(0, lo), (hi, n)], fetch=False)  # the sweep only scores: A, B, C stay on the device
        return reg.score_neg_rmse(X[lo:hi], Y[lo:hi])
    except (np.linalg.LinAlgError, _lib.NyskoopError) as e:
        if isinstance(error_score, str) and error_score == "raise":
            raise
        if isinstance(e, _lib.NyskoopError) and e.code != -5:  # only numerical failures are scored; the rest is a bug
            raise
        return float(error_score)


def _rank_candidates(scores):
    """mean_test_score, best_index as GridSearchCV computes them: a candidate with a failed (NaN) fold has a NaN mean and
    ranks last; best = first candidate with the highest finite mean (-1 if every candidate failed)."""
    mean = scores.mean(axis=1)
    finite = np.isfinite(mean)
    best = int(np.argmax(np.where(finite, mean, -np.inf))) if finite.any() else -1
    return mean, best


def grid_search_cv(X, Y, n_inputs, candidates, n_splits=5, centers=None, work=None, workers=1, error_score=np.nan,
                   batch=0, batch_groups=1, estimator="nystrom"):
    """learn_hyperparams (benchmark_lqr_cloth.py:39-66 and the classic/hjb twins) without sklearn's process pool.

    candidates: list of dicts with keys kernel / gamma / m.  centers: optional {(c, f): landmark indices into the
    training rows}; otherwise indices are drawn from the global NumPy RNG in GridSearchCV's order, which reproduces
    sklearn with n_jobs=1 exactly.  work: optional subset of (candidate, fold) units (for sharding over GPUs); units
    not evaluated are NaN.  workers: host threads issuing units concurrently on this GPU (each thread has its own
    context and streams; small fits are latency bound, so several in flight fill the chip).  The landmark draws happen
    up front in GridSearchCV's order, so the scores do not depend on `workers`.  error_score: score of a unit whose fit
    fails numerically (GridSearchCV's default: nan; such a candidate ranks last), or 'raise'.  batch: run that many
    units in lock step (include/nyskoop.h, nk_group_create): small fits are chains of launch-bound kernels, a batch shares
    every launch; scores are bit-identical to batch=0.
    estimator: 'nystrom' (default) or 'spline' (the thin-plate-spline branch of learn_hyperparams,
    benchmark_lqr_classic.py:54-60).  Spline candidates are dicts with gamma, m and optionally state_bounds_params;
    `centers` then maps (c, f) to the unit's d x m centre array (the reference's `centers` attribute), and without it the
    centres are drawn by spline_centers_draw in GridSearchCV's order (n_jobs=1).  Everything else behaves the same.
    Returns split_scores (n_cand x n_splits), mean_test_score, best_index.
    """
    _check_estimator(estimator)
    spline = estimator == "spline"
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    folds = kfold_slices(X.shape[0], n_splits)
    scores = np.full((len(candidates), n_splits), np.nan)
    units = cv_work_list(len(candidates), n_splits)
    mine = set(units if work is None else work)
    todo = []
    for (c, f) in units:
        if centers is not None:
            idx = centers.get((c, f)) if (c, f) not in mine else centers[(c, f)]
        elif spline:  # (drawn for every unit, evaluated or not, like the landmark indices below)
            lo, hi = folds[f]  # (the training states are only read by candidates without state bounds)
            bounded = candidates[c].get("state_bounds_params") is not None
            idx = spline_centers_draw(candidates[c], None if bounded else np.vstack((X[:lo, :Y.shape[1]], X[hi:, :Y.shape[1]])))
        else:  # drawn for every unit, evaluated or not: keeps the RNG stream aligned with the serial sweep
            n_train = X.shape[0] - (folds[f][1] - folds[f][0])
            idx = np.random.choice(np.arange(0, n_train), size=candidates[c]["m"], replace=False)
        if (c, f) in mine:
            todo.append((c, f, idx))

    def run(item):
        c, f, idx = item
        if spline:
            return c, f, cv_unit_score(X, Y, n_inputs, candidates[c], folds[f], idx, error_score, estimator)
        return c, f, cv_unit_score(X, Y, n_inputs, candidates[c], folds[f], idx, error_score)

    if batch > 1 and len(todo) > 1:
        # lock-step batching (nk_cv_grid): `batch` units per round, one library thread each, kernel launches merged
        units = []
        for (c, f, idx) in todo:
            lo, hi = folds[f]
            if spline:  # (nk_spline_cv_grid: the centres as m x d rows)
                units.append((candidates[c]["gamma"], candidates[c]["m"], (lo, hi),
                              np.ascontiguousarray(np.asarray(idx, dtype=np.float64).T)))
                continue
            idx = np.asarray(idx)
            rows = np.where(idx < lo, idx, idx + (hi - lo))  # training-row index -> dataset row
            kern = candidates[c]["kernel"].kernel
            units.append((kern, candidates[c]["gamma"], 1e-6, candidates[c]["m"], (lo, hi), rows))

        def sweep(pool, sub):
            return pool.spline_cv_grid(X, Y, n_inputs, sub) if spline else pool.cv_grid(X, Y, n_inputs, sub)

        if batch_groups > 1 and len(units) >= 2 * batch:
            # several independent lock-step groups, each on its own stream and driven from its own host thread: the
            # latency-bound factorisation chains of one group overlap with the GEMM-bound stages of another
            from concurrent.futures import ThreadPoolExecutor
            shares = [list(range(gi, len(units), batch_groups)) for gi in range(batch_groups)]
            sc, status = np.full(len(units), np.nan), np.zeros(len(units), dtype=np.int32)

            def run_share(gi):
                sub = [units[i] for i in shares[gi]]
                return sweep(_lib.lockstep_pool(batch, index=gi), sub)

            with ThreadPoolExecutor(max_workers=batch_groups) as ex:
                for gi, (s_g, st_g) in enumerate(ex.map(run_share, range(batch_groups))):
                    sc[shares[gi]], status[shares[gi]] = s_g, st_g
        else:
            sc, status = sweep(_lib.lockstep_pool(batch), units)
        bad = [int(st) for st in status if st not in (0, -3, -5)]
        if bad:
            raise _lib.NyskoopError(bad[0], "a unit of the batched sweep failed")
        if isinstance(error_score, str) and error_score == "raise" and np.any(status != 0):
            raise np.linalg.LinAlgError("a unit of the batched sweep failed numerically")
        sc = np.where(status == 0, sc, float("nan") if isinstance(error_score, str) else float(error_score))
        results = [(c, f, float(s)) for (c, f, _), s in zip(todo, sc)]
    elif workers > 1 and len(todo) > 1:
        results = list(_lib.worker_pool(workers).map(run, todo))
    else:
        results = [run(item) for item in todo]
    for c, f, sc in results:
        scores[c, f] = sc
    if work is None:
        mean, best = _rank_candidates(scores)
    else:  # a shard: the caller assembles the full table
        mean, best = scores.mean(axis=1), -1
    return dict(split_scores=scores, mean_test_score=mean, best_index=best,
                best_params=candidates[best] if best >= 0 else None)


# ---------------------------------------------------------------------------------------------------------------
# the multi-seed system-identification sweep (benchmark_lqr_classic.py:211-255, benchmark_lqr_cloth.py:163-211)
# ---------------------------------------------------------------------------------------------------------------
def _per_seed(table, si, seed):
    """Entry of a per-seed argument: a dict is keyed by the seed, anything else is indexed by the seed's position."""
    if table is None:
        return None
    return table[seed] if isinstance(table, dict) else table[si]


def train_row_map(ranges, n):
    """Data-set row of every training row, in the reference's concatenation order: `ranges` = [begin, end) pairs in the
    order the reference stacks them (benchmark_lqr_cloth.py:117-130 over the shuffled training trajectories); None = all
    n rows.  A landmark index i the reference drew over its own X refers to data-set row train_row_map(...)[i]."""
    if ranges is None:
        return np.arange(n, dtype=np.int64)
    rr = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if rr.size and (rr.min() < 0 or rr.max() > n or np.any(rr[:, 1] < rr[:, 0])):
        raise ValueError(f"training ranges must lie in [0, {n}]")
    return np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in rr]) if len(rr) else np.zeros(0, dtype=np.int64)


def sysid_plan(X, Y, n_inputs, params, ms, seeds, test_index, train_ranges=None, estimator="nystrom", extra_draws=0,
               centers=None, streams=None):
    """The units of sysid_sweep and their random draws, made up front (needs no GPU).  For every seed one stream
    np.random.RandomState(seed) (or `streams`' entry for the seed: a RandomState the caller has already advanced, e.g. by
    the trajectory shuffle of benchmark_lqr_cloth.py:171-172) is walked in the reference's order -- test trajectory major,
    m minor, one fit each.  The global NumPy RNG is never touched.
      nystrom: one choice(arange(n_train), m, replace=False) per fit (regressors.py:130), followed by `extra_draws`
               discarded draws of the same size; the indices count rows of the reference's concatenated training set and
               are mapped to rows of the data set (train_row_map);
      spline:  spline_centers_draw(..., rng=stream) per fit (regressors.py:187-197).
    centers: {(seed, test, k): landmark indices (nystrom, in the reference's row numbering) or d x m centres (spline)}
    replaces the draws.  Returns the units in m-major order (k, then seed, then test trajectory), so that a lock-step
    round holds fits of one shape: dicts with si, ti, k (position in the result table), m, traj (index of the test
    trajectory), ranges (the seed's training ranges or None) and marks (data-set rows, or the d x m centres)."""
    _check_estimator(estimator)
    spline = estimator == "spline"
    n, d = np.shape(Y)
    units = []
    for si, seed in enumerate(seeds):
        seed = int(seed)
        rs = _per_seed(streams, si, seed) if streams is not None else np.random.RandomState(seed)
        ranges = _per_seed(train_ranges, si, seed)
        rowmap = train_row_map(ranges, n)
        n_train = len(rowmap)
        states = None
        for ti, traj in enumerate(_per_seed(test_index, si, seed)):
            for k, m in enumerate(ms):
                m = int(m)
                if centers is not None:
                    marks = np.asarray(centers[(seed, ti, k)])
                    marks = np.asarray(marks, dtype=np.float64) if spline else rowmap[marks.astype(np.int64)]
                elif spline:
                    par = dict(params, m=m)
                    if par.get("state_bounds_params") is None and states is None:
                        states = np.asarray(X)[rowmap, :d]
                    marks = spline_centers_draw(par, states, rng=rs)
                else:
                    idx = rs.choice(np.arange(0, n_train), size=m, replace=False)
                    for _ in range(int(extra_draws)):
                        rs.choice(np.arange(0, n_train), size=m, replace=False)
                    marks = rowmap[idx]
                if marks.shape != ((d, m) if spline else (m,)):
                    raise ValueError(f"unit (seed {seed}, test {ti}, m {m}): landmarks have shape {marks.shape}")
                units.append(dict(si=si, ti=ti, k=k, m=m, traj=int(traj), marks=marks,
                                  ranges=None if ranges is None else np.asarray(ranges, dtype=np.int64).reshape(-1, 2)))
    units.sort(key=lambda u: (u["k"], u["si"], u["ti"]))  # (a stable sort of an already seed-major list)
    return units


def landmark_centers(Y, kernel, ms, seeds, test_index, train_ranges=None, rule="greedy", tol=0.0, select_fn=None):
    """The `centers=` dictionary of sysid_plan / sysid_sweep from pivoted-Cholesky landmark selection on the device
    (landmarks.select_landmarks) instead of uniform draws: {(seed, test, k): the first ms[k] selected landmarks, as
    indices in the reference's training-row numbering}.  The selection is nested, so ONE selection of max(ms) per distinct
    training-row set serves every m.  rule="greedy": all seeds with the same training rows share it; "rpcholesky": every
    seed draws its own max(ms) uniforms from np.random.RandomState(seed).  A tolerance that stops the selection before
    max(ms) landmarks is an error (sysid_plan wants ms[k] landmarks per unit).  select_fn: stands in for
    select_landmarks (tests without a GPU)."""
    if select_fn is None:
        from .landmarks import select_landmarks as select_fn
    n = np.shape(Y)[0]
    m_max = max(int(m) for m in ms)
    shared, out = {}, {}
    for si, seed in enumerate(seeds):
        seed = int(seed)
        ranges = _per_seed(train_ranges, si, seed)
        key = None if ranges is None else tuple(np.asarray(ranges, dtype=np.int64).reshape(-1).tolist())
        if rule != "greedy":
            key = (seed, key)
        if key not in shared:
            u = None if rule == "greedy" else np.random.RandomState(seed).uniform(size=m_max)
            rows = np.asarray(select_fn(Y, kernel, m_max, rule=rule, row_ranges=ranges, tol=tol, u=u), dtype=np.int64)
            if len(rows) < m_max:
                raise ValueError(f"the selection stopped after {len(rows)} landmarks (tol = {tol}), ms asks for {m_max}")
            rowmap = train_row_map(ranges, n)
            position = np.full(n, -1, dtype=np.int64)
            position[rowmap[::-1]] = np.arange(len(rowmap) - 1, -1, -1)  # data-set row -> its first training-row index
            shared[key] = position[rows]
        for ti, _ in enumerate(_per_seed(test_index, si, seed)):
            for k, m in enumerate(ms):
                out[(seed, ti, k)] = shared[key][:int(m)].copy()
    return out


def sysid_unit_error(X, Y, n_inputs, params, unit, tr, U, estimator="nystrom", relative=False):
    """One unit of the sweep on the calling thread's context: fit on the unit's rows with its landmarks, operators left on
    the device, then the open-loop error of its test trajectory reduced on the device (reg.open_loop_errors).
    tr: (n_trajs, T, d), U: (n_trajs, T, p) or None, as open_loop_pack lays them out."""
    m = unit["m"]
    if estimator == "spline":
        reg = KoopmanSplineRegressor(n_inputs, state_bounds_params=params.get("state_bounds_params"), m=m,
                                     gamma=params["gamma"])
        reg.centers = np.asarray(unit["marks"], dtype=np.float64)
    else:
        reg = KoopmanNystromRegressor(n_inputs, **dict(params, m=m))
        reg.nystrom_centers_output = np.ascontiguousarray(np.asarray(Y)[unit["marks"]].T)
    reg.fit(X, Y, row_ranges=unit["ranges"], fetch=False)
    t = unit["traj"]
    return float(reg.open_loop_errors(tr[t].T[None], None if U is None else U[t].T[None], relative)[0])


def sysid_grid_units(params, units, estimator="nystrom"):
    """The argument tuples of LockstepPool.sysid_grid for planned units (one test trajectory per unit)."""
    if estimator == "spline":
        return [(None, params["gamma"], 0.0, u["m"], u["ranges"], np.ascontiguousarray(u["marks"].T), [u["traj"]])
                for u in units]
    kern = params["kernel"].kernel
    jitter = KoopmanNystromRegressor(1, **dict(params, m=1)).jitter
    return [(kern, params["gamma"], jitter, u["m"], u["ranges"], u["marks"], [u["traj"]]) for u in units]


def sysid_run_units(X, Y, n_inputs, params, units, trajs, controls, estimator="nystrom", relative=False, batch=0,
                    batch_groups=1, unit_fn=None):
    """Errors of planned units, in their order.  batch=0 (or a `unit_fn` standing in for the device): the plain loop of
    sysid_unit_error; batch>1: one nk_sysid_grid call per lock-step group (bit-identical numbers).  A unit whose fit fails
    numerically is NaN; any other failure raises."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    from .regressors import open_loop_pack
    tr, U = open_loop_pack(np.asarray(trajs, dtype=np.float64), controls, Y.shape[1], int(n_inputs))
    if unit_fn is not None or batch <= 1 or len(units) <= 1:
        fn = unit_fn or sysid_unit_error
        return np.array([fn(X, Y, n_inputs, params, u, tr, U, estimator, relative) for u in units], dtype=np.float64)
    tuples = sysid_grid_units(params, units, estimator)

    def sweep(pool, sub):
        ea, er, st, _ = pool.sysid_grid(X, Y, n_inputs, tr, U, sub)  # one trajectory per unit: offsets = 0, 1, 2, ...
        return (er if relative else ea), st

    if batch_groups > 1 and len(tuples) >= 2 * batch:  # independent groups on their own streams, as in grid_search_cv
        from concurrent.futures import ThreadPoolExecutor
        shares = [list(range(gi, len(tuples), batch_groups)) for gi in range(batch_groups)]
        err, status = np.full(len(tuples), np.nan), np.zeros(len(tuples), dtype=np.int32)
        with ThreadPoolExecutor(max_workers=batch_groups) as ex:
            runs = ex.map(lambda gi: sweep(_lib.lockstep_pool(batch, index=gi), [tuples[i] for i in shares[gi]]),
                          range(batch_groups))
            for gi, (e_g, st_g) in enumerate(runs):
                err[shares[gi]], status[shares[gi]] = e_g, st_g
    else:
        err, status = sweep(_lib.lockstep_pool(batch), tuples)
    bad = [int(st) for st in status if st not in (0, -3, -5)]
    if bad:
        raise _lib.NyskoopError(bad[0], "a unit of the batched sweep failed")
    return np.where(status == 0, err, np.nan)


def sysid_table(units, values, n_seeds, n_ms):
    """(seed, test trajectory, m) table from per-unit values in plan order; entries without a unit are NaN."""
    n_test = 1 + max((u["ti"] for u in units), default=0)
    out = np.full((n_seeds, n_test, n_ms), np.nan)
    for u, v in zip(units, values):
        out[u["si"], u["ti"], u["k"]] = v
    return out


def sysid_sweep(X, Y, n_inputs, params, ms, seeds, trajs, controls, test_index, train_ranges=None, estimator="nystrom",
                relative=False, extra_draws=0, centers=None, batch=0, batch_groups=1, streams=None):
    """The multi-seed system-identification sweep of benchmark_lqr_classic.py:211-255 and benchmark_lqr_cloth.py:163-211:
    for every seed, every test trajectory of the seed and every m in `ms`: draw landmarks, fit, validate_dyn_sys.
    Returns the open-loop errors (absolute RMSE, or the relative-% form with relative=True) as an array of shape
    (len(seeds), n_test_per_seed, len(ms)).

    X: n x (d+p), Y: n x d: ONE data set holding every row any seed trains on; train_ranges[seed] = the [begin, end) row
    ranges the seed trains on, in the order the reference concatenates them (cloth: one range per training trajectory of
    the seed's shuffle; the fit accepts them in any order and gathers them in that order, so its training matrix is the
    reference's, row for row); None = all rows.  trajs: (k, d, T) test trajectories, controls: (k, p, T or T-1);
    test_index[seed] = the trajectories the seed is tested on.  Per-seed arguments are dicts keyed by the seed or sequences
    in the order of `seeds`.  params: kernel and gamma (nystrom), or gamma and optionally state_bounds_params (spline); m
    comes from `ms`.  Draws, `extra_draws`, `centers` and `streams`: see sysid_plan (the shipped cloth CSV needs
    extra_draws=1 and streams advanced by the seed's shuffle).
    batch=0: the plain loop of reg.fit(row_ranges=..., fetch=False) + reg.open_loop_errors.  batch>1: the units are
    ordered m-major and run `batch` at a time in lock step by ONE library call (nk_sysid_grid): same bits, merged launches;
    batch_groups>1: that many independent groups side by side, as in grid_search_cv."""
    units = sysid_plan(X, Y, n_inputs, params, ms, seeds, test_index, train_ranges, estimator, extra_draws, centers, streams)
    vals = sysid_run_units(X, Y, n_inputs, params, units, trajs, controls, estimator, relative, batch, batch_groups)
    return sysid_table(units, vals, len(seeds), len(ms))


def lqr_closed_loop(num_steps, reference, initial_state, regressor, K):
    """The loop of benchmark_lqr_cloth.py:73-84 alone: returns (visited_states (d, 1+num_steps) starting with the initial
    state, u_ops (p, num_steps)).  One device call (lifts of both states + the whole lifted recursion)."""
    initial_state = np.asarray(initial_state, dtype=np.float64).reshape(-1, 1)
    reference = np.asarray(reference, dtype=np.float64).reshape(-1, 1)
    phi = regressor.lift(np.hstack((initial_state, reference)))  # one call for both lifts
    xs, us = regressor.closed_loop(K, phi[:, 0], phi[:, 1], num_steps)
    return np.hstack((initial_state, xs)), us


def lqr_control(num_steps, reference, initial_state, regressor, K, control_nodes=(168, 169, 170, 189, 190, 191),
                simulator_order=(0, 3, 1, 4, 2, 5)):
    """benchmark_lqr_cloth.py:69-104 in full: the lifted closed loop, the CUMULATIVE input sequence seeded with the
    positions of the two controlled corner nodes (`u_s[:, 0] = initial_state[control_nodes]`, every later column adds
    the step's u_op, :76-81), the per-axis split of the visited states (x = rows 0,3,6.., y = 1,4,.., z = 2,5,..; :85-101)
    and the input rows permuted for the MATLAB simulator (:102).  Returns (x_s, y_s, z_s, final_us) with
    x_s, y_s, z_s: (d/3, 1+num_steps), final_us: (p, 1+num_steps)."""
    initial_state = np.asarray(initial_state, dtype=np.float64).reshape(-1, 1)
    visited, u_ops = lqr_closed_loop(num_steps, reference, initial_state, regressor, K)
    u0 = initial_state[list(control_nodes), :]
    u_s = np.hstack((u0, u0 + np.cumsum(u_ops, axis=1)))
    x_s, y_s, z_s = visited[0::3], visited[1::3], visited[2::3]
    final_us = u_s[list(simulator_order), :]
    return x_s, y_s, z_s, final_us


def plant_snapshots(plant, n, rng, bound=1.0, u_bound=1.0):
    """n snapshot pairs of a plant object (n_states, update_SOM; n_inputs when it has more than one input): states uniform in
    [-bound, bound]^d, inputs uniform in [-u_bound, u_bound]^p, drawn from `rng` (a numpy Generator) states first.  Returns
    X = [state | input] (n, d + p) and Y = the next states (n, d)."""
    d, p = int(plant.n_states), int(getattr(plant, "n_inputs", 1))
    S = rng.uniform(-bound, bound, size=(d, n))
    U = rng.uniform(-u_bound, u_bound, size=(p, n))
    Y = np.asarray(plant.update_SOM(S, U), dtype=np.float64)
    return np.ascontiguousarray(np.vstack((S, U)).T), np.ascontiguousarray(Y.T)


def lqr_control_plant(num_steps, reference, initial_state, regressor, K, plant_step):
    """The plant-in-the-loop variant of benchmark_lqr_hjb.py:73-97 (and _classic.py:67-89): u = K (phi(ref) - phi(x)),
    x <- plant_step(x, u), phi re-lifted from the true state every step (one cached-square-root lift per step instead of
    the reference's O(m^3) sqrtm).  plant_step(x (d,1), u (p,1)) -> x_next.  Returns (x_s (num_steps,), u_s (p, num_steps))
    like the reference: x_s is the first state coordinate of the visited states."""
    x = np.asarray(initial_state, dtype=np.float64).reshape(-1, 1)
    phi_ref = regressor.lift(np.asarray(reference, dtype=np.float64).reshape(-1, 1))
    phi = regressor.lift(x)
    xs, us = [], []
    for _ in range(num_steps):
        u = K @ (phi_ref - phi)
        us.append(u.reshape(-1, 1))
        xs.append(x[0, 0])
        x = np.asarray(plant_step(x, u), dtype=np.float64).reshape(-1, 1)
        phi = regressor.lift(x)
    return np.array(xs), np.hstack(us)


def lqr_control_plant_device(num_steps, reference, initial_state, regressor, K, plant):
    """lqr_control_plant with the whole loop in ONE device launch (regressor.closed_loop_plant -> nk_plant_loop): `plant` is one
    of dynamical_systems.DuffingOscillator / DoubleIntegrator / HJB or a PolynomialSystem instead of a callable.  Returns (x_s (num_steps,),
    u_s (p, num_steps)) like lqr_control_plant: x_s is the first coordinate of the states the controls were computed at."""
    x0 = np.asarray(initial_state, dtype=np.float64).reshape(-1)
    ref = np.asarray(reference, dtype=np.float64).reshape(-1)
    states, us = regressor.closed_loop_plant(K, x0, ref, num_steps, plant)
    return np.array(states[0, :num_steps]), us


def mpc_control_plant(num_steps, reference, initial_state, regressor, controller, plant_step, iters=50, tol=0.0,
                      u_init=None):
    """The host loop of the constrained MPC (regressor.closed_loop_plant_mpc is the same loop in one device launch): one
    lift per step, e = phi(x) - phi(ref), the control from lqr.mpc_solve (controller.control) with u_{-1} = the control
    applied last (u_init, zeros by default, before the first step), x <- plant_step(x (d, 1), u (p, 1)).  iters = 0: the
    saturated LQR.  Returns (states (d, num_steps + 1) with the initial state first, u_s (p, num_steps), info (num_steps, 2)
    = {iterations run, final max |s - z|}).  A controller with output rows (lqr.MPCOutputController) is given the reference
    state as well: its state bounds are absolute."""
    x = np.asarray(initial_state, dtype=np.float64).reshape(-1, 1)
    x_ref = np.asarray(reference, dtype=np.float64).reshape(-1)
    phi_ref = regressor.lift(x_ref.reshape(-1, 1))
    p = controller.n_inputs
    u_prev = np.zeros(p) if u_init is None else np.asarray(u_init, dtype=np.float64).reshape(p)
    kw = dict(x_ref=x_ref) if hasattr(controller, "ycomp") else {}
    xs, us, info = [x], [], []
    for _ in range(num_steps):
        u_prev, it = controller.control((regressor.lift(x) - phi_ref).reshape(-1), u_prev, iters, tol, **kw)
        us.append(u_prev.reshape(-1, 1))
        info.append(it)
        x = np.asarray(plant_step(x, u_prev.reshape(-1, 1)), dtype=np.float64).reshape(-1, 1)
        xs.append(x)
    return np.hstack(xs), np.hstack(us), np.array(info, dtype=np.float64).reshape(num_steps, 2)


def open_loop_control(plant_step, initial_state, controls):
    """benchmark_lqr_classic.py:91-97: replay a control sequence (p x T) on the true plant; returns the visited states
    (d x (T + 1)), the initial state first."""
    state = np.asarray(initial_state, dtype=np.float64).reshape(-1, 1)
    controls = np.asarray(controls, dtype=np.float64)
    states = [state]
    for i in range(controls.shape[1]):
        state = np.asarray(plant_step(state, controls[:, i].reshape(-1, 1)), dtype=np.float64).reshape(-1, 1)
        states.append(state)
    return np.hstack(states)


def control_rmse_percent(us, u_opt):
    """benchmark_lqr_hjb.py:313 / :378."""
    us, u_opt = np.asarray(us).squeeze(), np.asarray(u_opt).squeeze()
    return np.sqrt(np.sum(np.square(us - u_opt))) / np.sqrt(np.sum(np.square(u_opt))) * 100


# ---------------------------------------------------------------------------------------------------------------
# the multi-seed CONTROL sweep (benchmark_lqr_classic.py:256-299, benchmark_lqr_hjb.py:265-333)
# ---------------------------------------------------------------------------------------------------------------
SCORE_NAMES = ("sse_u", "ss_opt", "J", "u_absmax")


def rmse_control_percent(sse_u, ss_opt):
    """benchmark_lqr_hjb.py:313 from the two sums: 100 sqrt(sum (u - u_opt)^2) / sqrt(sum u_opt^2)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return 100.0 * np.sqrt(np.asarray(sse_u, dtype=np.float64)) / np.sqrt(np.asarray(ss_opt, dtype=np.float64))


def control_scores(states, controls, u_opt=None):
    """The four scores of nk_plant_loop_multi / nk_poly_plant_loop_multi on the host, in the device's order of operations, from
    one loop's visited states (d, steps + 1) (x0 first) and controls (steps,) / (p, steps) / (steps, p): sse_u and ss_opt (sums over the
    steps and, within a step, over the inputs in index order; 0 without u_opt; u_opt: (steps,) or (steps, p)),
    J = the cost of open_loop_control (benchmark_lqr_hjb.py:99-107: J = sum_k x0_k^2, then (J + sum_k x_{t+1,k}^2) +
    sum_j u_{t,j}^2) and u_absmax (over steps and inputs, NaN from the first NaN control on); plus rmse_control
    (benchmark_lqr_hjb.py:313).  Returns a dict of floats.  Needs no GPU."""
    xs = np.asarray(states, dtype=np.float64)
    xs = xs.reshape(1, -1) if xs.ndim == 1 else xs
    us = np.asarray(controls, dtype=np.float64)
    us = us.reshape(1, -1) if us.ndim < 2 else us
    if us.shape[1] != xs.shape[1] - 1 and us.shape[0] == xs.shape[1] - 1:
        us = us.T  # (steps, p), as the multi-model call returns a unit's controls
    p, steps = us.shape
    if xs.shape[1] != steps + 1:
        raise ValueError(f"states have shape {xs.shape}, expected (d, {steps + 1})")
    uo = None if u_opt is None else np.asarray(u_opt, dtype=np.float64)
    if uo is not None and uo.size != steps * p:
        raise ValueError(f"u_opt has {uo.size} entries, the loop has {steps} steps of {p} inputs")
    uo = None if uo is None else uo.reshape(steps, p)

    def sumsq(col):
        acc = float(col[0]) * float(col[0])
        for v in col[1:]:
            acc = acc + float(v) * float(v)
        return acc

    J, sse, sso, umax = sumsq(xs[:, 0]), 0.0, 0.0, 0.0
    for t in range(steps):
        J = (J + sumsq(xs[:, t + 1])) + sumsq(us[:, t])
        for j in range(p):
            u = float(us[j, t])
            au = abs(u)
            if au > umax or au != au:
                umax = au
            if uo is not None:
                df = u - float(uo[t, j])
                sse = sse + df * df
                sso = sso + float(uo[t, j]) * float(uo[t, j])
    return dict(sse_u=sse, ss_opt=sso, J=J, u_absmax=umax, rmse_control=float(rmse_control_percent(sse, sso)))


def hjb_optimal_control(x0, num_steps, plant):
    """The analytic optimum the HJB driver compares against (benchmark_lqr_hjb.py:304-311), on the host: from x0,
    u = x^3 - x sqrt(1 + x^4), x <- plant(x, u), J <- J + x^2 + u^2 starting at x0^2.  Returns (u_opt (num_steps,), J_true)."""
    x = np.asarray(x0, dtype=np.float64).reshape(-1, 1)
    J = x ** 2
    u_opt = np.empty(int(num_steps))
    for i in range(int(num_steps)):
        u = x ** 3 - x * np.sqrt(1 + x ** 4)
        u_opt[i] = u.squeeze()
        x = np.asarray(plant.update_SOM(x, u), dtype=np.float64).reshape(-1, 1)
        J = J + x ** 2 + u ** 2
    return u_opt, float(np.squeeze(J))


def _broadcast_states(x, n, d, what, one=None):
    """(n, d) states of the plant loops, whose units share d: x holds d numbers (one state for all units) or n d (one per unit,
    row after row).  The count decides, where _per_unit, whose units may differ in d, goes by the shape."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == d:
        return np.ascontiguousarray(np.broadcast_to(x.reshape(1, d), (n, d)))
    if x.size != n * d:
        raise ValueError(f"{what} has shape {x.shape}, expected {one or f'one state of dimension {d}'} or {(n, d)}")
    return np.ascontiguousarray(x.reshape(n, d))


def _uopt_rows(u_opt, width, n, rows):
    """(u_opt as a (k, width) table or None, the row of each of n units: `rows` if given, else u when k = n > 1, else 0)."""
    if u_opt is None:
        return None, rows
    uo = np.asarray(u_opt, dtype=np.float64).reshape(-1, width)
    if rows is None:
        rows = list(range(n)) if uo.shape[0] == n and n > 1 else [0] * n
    return uo, rows


def _score_dict(names, sc, trajectories=False, states=None, controls=None, with_info=False, info=None):
    """What the multi loops return: the score columns by name, rmse_control, and the trajectories / info that were asked for."""
    out = {name: sc[:, i].copy() for i, name in enumerate(names)}
    out["rmse_control"] = rmse_control_percent(out["sse_u"], out["ss_opt"])
    if trajectories:
        out["states"], out["controls"] = states, controls
    if with_info:
        out["info"] = info
    return out


def plant_loop_multi(regressors, gains, x0s, x_refs, num_steps, plant, u_opt=None, return_trajectories=False,
                     uopt_rows=None):
    """One closed loop around the TRUE plant per (regressor, gain, x0, x_ref) unit -- lqr_control, open_loop_control and
    the control RMSE of benchmark_lqr_hjb.py:73-107,313 -- for all units in ONE device call (nk_plant_loop_multi).  Unit u
    is bit for bit regressors[u].closed_loop_plant(gains[u], x0s[u], x_refs[u], num_steps, plant); the units may mix model
    kinds, kernels and landmark counts.  x0s, x_refs: (n_units, d) or one state for all.  u_opt: (num_steps,) scored
    against by every unit, or (k, num_steps) with uopt_rows[u] = the row of unit u (-1: none; default: row u when
    k = n_units > 1, else row 0).
    Returns a dict of (n_units,) arrays sse_u, ss_opt, J, u_absmax (see include/nyskoop.h) and rmse_control =
    100 sqrt(sse_u) / sqrt(ss_opt); with return_trajectories also states (n_units, num_steps + 1, d) and controls
    (n_units, num_steps).  Without them nothing but the scores leaves the device.
    A dynamical_systems.PolynomialSystem as `plant` runs nk_poly_plant_loop_multi: gains (p, m), u_opt (num_steps, p) or
    (k, num_steps, p), controls (n_units, num_steps, p), the scores summed over the inputs (control_scores)."""
    regs = list(regressors)
    n = len(regs)
    from .regressors import _check_plant
    plant_id, Ts, poly = _check_plant(plant)
    d = int(plant.n_states)
    p = int(plant.n_inputs) if poly else 1
    ctx = _lib.get_context()
    handles = [r._ensure_model() for r in regs]
    Ks = []
    for r, K in zip(regs, gains):
        K = np.ascontiguousarray(K, dtype=np.float64)
        m = r._landmark_shape()[1]
        if K.size != p * m or (poly and K.shape != (p, m)):
            raise ValueError(f"gain has shape {K.shape}, expected {(p, m)}")
        Ks.append(K)
    if len(Ks) != n:
        raise ValueError(f"{len(Ks)} gains for {n} regressors")
    uo, rows = _uopt_rows(u_opt, int(num_steps) * p, n, uopt_rows)
    x0b, xrb = _broadcast_states(x0s, n, d, "x0s"), _broadcast_states(x_refs, n, d, "x_refs")
    if poly:
        sc, ox, ou = ctx.poly_plant_loop_multi(plant.descriptor(), num_steps, handles, Ks, x0b, xrb, u_opt=uo, uopt_rows=rows,
                                               want_x=return_trajectories, want_u=return_trajectories)
    else:
        sc, ox, ou = ctx.plant_loop_multi(plant_id, Ts, num_steps, handles, Ks, x0b, xrb, u_opt=uo, uopt_rows=rows,
                                          want_x=return_trajectories, want_u=return_trajectories)
    return _score_dict(SCORE_NAMES, sc, return_trajectories, ox, ou)


MPC_SCORE_NAMES = SCORE_NAMES + ("iters_sum", "r_max", "n_at_limit", "n_iterated")


def mpc_scores(states, controls, info, controller, u_opt=None, u_init=None):
    """The eight scores of nk_mpc_loop_multi on the host, in the device's order of operations, from one loop's visited states
    (d, steps + 1), controls (p, steps) / (steps, p), info (steps, 2) = {iterations run, final max |s - z|} and the bounds of
    `controller` (lo, hi, dlo, dhi; the first p entries are the applied move's): control_scores' four, then iters_sum (sum
    of the iterations in step order), r_max (the largest final residual, NaN from the first NaN on), n_at_limit (the (t, j) at
    which u_tj equals lo_j, hi_j, fl(u_{t-1,j} + dlo_j) or fl(u_{t-1,j} + dhi_j), u_{-1} = u_init or zeros; counted once
    each) and n_iterated (steps with at least one iteration); plus rmse_control.  Returns a dict of floats.  Needs no GPU."""
    out = control_scores(states, controls, u_opt)
    xs = np.asarray(states, dtype=np.float64)
    steps = (xs.reshape(1, -1) if xs.ndim == 1 else xs).shape[1] - 1
    us = np.asarray(controls, dtype=np.float64)
    us = us.reshape(1, -1) if us.ndim < 2 else us
    if us.shape[1] != steps and us.shape[0] == steps:
        us = us.T
    p = us.shape[0]
    info = np.asarray(info, dtype=np.float64).reshape(steps, 2)
    lo, hi, dlo, dhi = (np.asarray(a, dtype=np.float64).reshape(-1)[:p] for a in
                        (controller.lo, controller.hi, controller.dlo, controller.dhi))
    prev = np.zeros(p) if u_init is None else np.asarray(u_init, dtype=np.float64).reshape(p).copy()
    it_sum, r_max, n_lim, n_it = 0.0, 0.0, 0, 0
    for t in range(steps):
        it, r = float(info[t, 0]), float(info[t, 1])
        it_sum = it_sum + it
        n_it += it > 0
        if r > r_max or r != r:
            r_max = r
        with np.errstate(invalid="ignore"):  # inf - inf of an absent rate limit: NaN, equal to nothing
            rl, rh = prev + dlo, prev + dhi
        for j in range(p):
            u = us[j, t]
            n_lim += bool(u == lo[j] or u == hi[j] or u == rl[j] or u == rh[j])
        prev = us[:, t]
    out.update(iters_sum=it_sum, r_max=r_max, n_at_limit=float(n_lim), n_iterated=float(n_it))
    return out


MPC_OUT_SCORE_NAMES = MPC_SCORE_NAMES + ("y_viol_max", "n_y_viol")


def mpc_out_scores(states, controls, info, controller, u_opt=None, u_init=None):
    """The ten scores of nk_mpc_out_loop_multi on the host, in the device's order of operations: mpc_scores' eight, then
    y_viol_max = the maximum over the steps t and the output rows r of `controller` with ycomp[r] = c >= 0 of
    max(ylo_r - x_{t+1}[c], x_{t+1}[c] - yhi_r, 0) -- one rounded subtraction each, on the ABSOLUTE bounds and the realised
    next state; a step with a NaN difference has a NaN maximum, which enters once and stays (the rule of u_absmax) -- and
    n_y_viol = the number of steps whose maximum is > 0 (a NaN step does not count).  A controller without output rows (an
    lqr.MPCController) has 0 and 0.  Returns a dict of floats.  Needs no GPU."""
    out = mpc_scores(states, controls, info, controller, u_opt, u_init)
    xs = np.asarray(states, dtype=np.float64)
    xs = xs.reshape(1, -1) if xs.ndim == 1 else xs
    steps = xs.shape[1] - 1
    y_max, n_viol = 0.0, 0
    if hasattr(controller, "ycomp"):
        yc = np.asarray(controller.ycomp, dtype=np.int64).reshape(-1)
        rows = np.flatnonzero(yc >= 0)
        ylo = np.asarray(controller.ylo, dtype=np.float64).reshape(-1)[rows]
        yhi = np.asarray(controller.yhi, dtype=np.float64).reshape(-1)[rows]
        comp = yc[rows]
        for t in range(steps if rows.size else 0):
            xc = xs[comp, t + 1]
            with np.errstate(invalid="ignore"):  # inf - inf: NaN, which the rule below hands on
                below, above = ylo - xc, xc - yhi
            if np.any(below != below) or np.any(above != above):
                v = float("nan")
            else:
                v = float(max(np.max(below), np.max(above), 0.0))
            n_viol += v > 0
            if v > y_max or v != v:
                y_max = v
    out.update(y_viol_max=y_max, n_y_viol=float(n_viol))
    return out


def mpc_loop_multi(regressors, controllers, x0s, x_refs, num_steps, plant, iters=50, tol=0.0, u_inits=None, u_opt=None,
                   uopt_rows=None, return_trajectories=False, return_info=False):
    """One constrained MPC loop around the TRUE plant per (regressor, controller, x0, x_ref) unit, all units in ONE device call
    (nk_mpc_loop_multi), scored on the device.  Unit u is bit for bit regressors[u].closed_loop_plant_mpc(controllers[u],
    x0s[u], x_refs[u], num_steps, plant, iters[u], tol[u], u_inits[u]); the units may mix model kinds, kernels, landmark
    counts, horizons, limits and iteration counts (iters = 0: the saturated LQR).  iters, tol: scalars or one per unit.
    x0s, x_refs: (n_units, d) or one state for all; u_inits: (n_units, p), one (p,) for all, or None = zeros.  plant: what
    closed_loop_plant_mpc accepts.  u_opt: (num_steps, p) scored against by every unit, or (k, num_steps, p) with
    uopt_rows[u] = the row of unit u (-1: none; default: row u when k = n_units > 1, else row 0).
    Returns a dict of (n_units,) arrays, the eight MPC_SCORE_NAMES (see include/nyskoop.h) and rmse_control; with
    return_trajectories also states (n_units, num_steps + 1, d) and controls (n_units, num_steps, p), with return_info info
    (n_units, num_steps, 2).  Without them nothing but the scores leaves the device.
    A controller with output rows (lqr.MPCOutputController, solve_mpc(x_min=, x_max=)) runs WITH its rows: when at least one
    unit has one and iters != 0 the call is nk_mpc_out_loop_multi, such a unit is bit for bit its closed_loop_plant_mpc
    (nk_mpc_out_loop), the others stay what they were, and the dict holds the ten MPC_OUT_SCORE_NAMES (y_viol_max and n_y_viol
    are 0 for a unit without rows).  An MPCOutputController at iters = 0 runs as the saturated LQR, as in
    closed_loop_plant_mpc.  (Before, the rows of such a controller were dropped without a word and the unit ran as the
    input-only MPC; that no longer happens.)  Without any such unit the call and its eight scores are what they were."""
    from .regressors import _as_polynomial_plant
    regs, ctls = list(regressors), list(controllers)
    n = len(regs)
    if len(ctls) != n:
        raise ValueError(f"{len(ctls)} controllers for {n} regressors")
    plant = _as_polynomial_plant(plant)
    d, p = int(plant.n_states), int(plant.n_inputs)
    num_steps = int(num_steps)

    def per_unit(v, what):
        a = np.asarray(v)
        if a.ndim == 0:
            return [a.item()] * n
        if a.size != n:
            raise ValueError(f"{what} has {a.size} entries for {n} units")
        return [x.item() for x in a.reshape(-1)]

    its, tols = per_unit(iters, "iters"), per_unit(tol, "tol")
    ctx = _lib.get_context()
    handles = [r._ensure_model() for r in regs]
    descs, keep, shared = [], [], {}
    outs, shared_out = [], {}
    for r, c, it, tl in zip(regs, ctls, its, tols):
        m = r._landmark_shape()[1]
        if c.K.shape != (p, m) or c.F.shape[1] != m:
            raise ValueError(f"the controller is for a model with K of shape {c.K.shape}, expected {(p, m)}")
        key = (id(c), int(it), float(tl))
        if key not in shared:  # units with the same controller, iters and tol share one description
            shared[key] = _lib.mpc_desc(c, it, tl)
            keep.append(shared[key][1])
        descs.append(shared[key][0])
        if hasattr(c, "ycomp") and int(it) != 0:  # an lqr.MPCOutputController (iters = 0: the saturated LQR, no rows)
            if id(c) not in shared_out:
                shared_out[id(c)] = _lib.mpc_out(c)
                keep.append(shared_out[id(c)][1])
            outs.append(shared_out[id(c)][0])
        else:
            outs.append(None)
    with_rows = any(o is not None for o in outs)
    uo, rows = _uopt_rows(u_opt, num_steps * p, n, uopt_rows)
    uis = None if u_inits is None else list(_broadcast_states(u_inits, n, p, "u_inits", f"{p} entries"))
    x0b, xrb = _broadcast_states(x0s, n, d, "x0s"), _broadcast_states(x_refs, n, d, "x_refs")
    sc, ox, ou, oi = ctx.mpc_loop_multi(plant.descriptor(), num_steps, handles, descs, x0b, xrb, u_inits=uis, u_opt=uo,
                                        uopt_rows=rows, want_x=return_trajectories, want_u=return_trajectories,
                                        want_info=return_info, outs=outs if with_rows else None)
    del keep
    return _score_dict(MPC_OUT_SCORE_NAMES if with_rows else MPC_SCORE_NAMES, sc, return_trajectories, ox, ou, return_info, oi)


def lqr_default_gain(c=1.0):
    """gain_fn of lqr_sweep: K = dlqr(A, B, c C^T C symmetrised, I), the arithmetic of regressor.solve_lqr(c=c)."""
    from .lqr import dlqr

    def gain(A, B, C):
        Q = c * C.T @ C
        Q = (Q + Q.T) / 2
        return dlqr(A, B, Q, np.eye(np.shape(B)[1]))[0]

    return gain


def lqr_plan(X, Y, n_inputs, params, ms, seeds, estimator="nystrom", centers=None):
    """The units of lqr_sweep: sysid_plan's per-seed protocol (one np.random.RandomState(seed) per seed walked in the
    reference's order, m minor; all rows train) with one slot per (seed, m).  Needs no GPU."""
    return sysid_plan(X, Y, n_inputs, params, ms, seeds, [[0]] * len(seeds), None, estimator, 0,
                      None if centers is None else {(int(s), 0, k): v for (s, k), v in centers.items()})


def lqr_fit_unit(X, Y, n_inputs, params, unit, estimator="nystrom"):
    """The fit of one planned unit on the calling thread's context, operators fetched; returns the fitted regressor, or
    None when the fit fails numerically."""
    m = unit["m"]
    if estimator == "spline":
        reg = KoopmanSplineRegressor(n_inputs, state_bounds_params=params.get("state_bounds_params"), m=m,
                                     gamma=params["gamma"])
        reg.centers = np.asarray(unit["marks"], dtype=np.float64)
    else:
        reg = KoopmanNystromRegressor(n_inputs, **dict(params, m=m))
        reg.nystrom_centers_output = np.ascontiguousarray(np.asarray(Y)[unit["marks"]].T)
    try:
        reg.fit(X, Y, row_ranges=unit["ranges"])
    except np.linalg.LinAlgError:
        return None
    except _lib.NyskoopError as e:
        if e.code != -5:
            raise
        return None
    return reg


def lqr_fit_and_gain(X, Y, n_inputs, params, units, estimator="nystrom", gain_fn=None, c=1.0, batch=32, workers=4,
                     fit_fn=None, gain="host", gain_batch_fn=None, after_fit=None, controller=None, controller_batch_fn=None):
    """The fits and gains of planned units -- what lqr_run_units and cloth_lqr_sweep share.  Fits: `batch` at a time through
    the lock-step pool (a plain loop with batch <= 1 or a fit_fn); a unit may carry its own "estimator" and "params".
    after_fit(reg, unit): called on the fitting thread right after a successful fit, inside the lock-step round (its result
    is kept per unit).  Gains: gain="host": gain_fn(A, B, C) in `workers` host threads while later rounds fit;
    gain="device": ONE nk_model_lqr_gain_batch call after the fits (gain_batch_fn(regs, c) stands in for it).
    controller (the checked dict of lqr_sweep): instead of a gain, reg.solve_mpc(horizon, c=c, limits, rho) is built per
    unit on the same host threads, and gains[i] is that lqr.MPCController (None when it raises); with x_min / x_max (and
    y_horizon, y_weight) in the dict it is an lqr.MPCOutputController.  With controller["build"] == "device" the controllers of
    all fitted units come from ONE nk_model_mpc_build_batch call after the fits instead (regressors._mpc_controller_batch;
    controller_batch_fn(regs, c, controller) -> (controllers, status) stands in for it): a unit with a non-zero status, or
    whose limits solve_mpc refuses, has gains[i] None; gain_wait_s is that call and gain_cpu_s is 0.
    Returns (regs, gains, extras, timing): a unit whose fit failed has regs[i] None, one without a gain gains[i] None;
    timing = dict(fit_s, gain_wait_s, gain_cpu_s)."""
    import time
    if gain not in ("host", "device"):
        raise ValueError(f"gain must be 'host' or 'device', got {gain!r}")
    if controller is not None and gain == "device":
        raise ValueError("controller needs gain='host': the terminal cost of the MPC is the host Riccati solution")
    if gain == "device" and gain_fn is not None:
        raise ValueError("gain='device' solves K = dlqr(A, B, c C'C, I) on the device: gain_fn cannot be combined with it")
    device_gain = gain == "device"
    device_build = controller is not None and controller.get("build", "host") == "device"
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    gain_fn = gain_fn or lqr_default_gain(c)
    n = len(units)
    gain_s = [0.0] * n

    def gain_of(i, reg):
        t0 = time.perf_counter()
        try:
            if controller is not None:
                rows = {}  # the state limits travel only when the dict holds one: without them the call is what it was
                if controller.get("x_min") is not None or controller.get("x_max") is not None:
                    rows = dict(x_min=controller["x_min"], x_max=controller["x_max"], y_horizon=controller.get("y_horizon"),
                                y_weight=controller.get("y_weight", np.inf))
                return reg.solve_mpc(controller["horizon"], c=c, u_min=controller["u_min"], u_max=controller["u_max"],
                                     du_min=controller["du_min"], du_max=controller["du_max"], rho=controller["rho"], **rows)
            return np.asarray(gain_fn(np.asarray(reg.A), np.asarray(reg.B), np.asarray(reg.C)), dtype=np.float64)
        finally:
            gain_s[i] = time.perf_counter() - t0

    pool = _lib.worker_pool(max(1, int(workers)))
    regs, futures, extras = [None] * n, [None] * n, [None] * n
    t0 = time.perf_counter()
    lockstep = fit_fn is None and batch > 1 and n > 1

    def fit(u):
        reg = (fit_fn or lqr_fit_unit)(X, Y, n_inputs, u.get("params", params), u, u.get("estimator", estimator))
        if after_fit is None:
            return reg
        return reg, (None if reg is None else after_fit(reg, u))

    step = int(batch) if lockstep else 1
    lpool = _lib.lockstep_pool(step) if lockstep else None
    for r in range(0, n, step):
        idx = list(range(r, min(r + step, n)))
        fitted = lpool.run_round(fit, [units[i] for i in idx]) if lockstep else [fit(units[i]) for i in idx]
        for i, reg in zip(idx, fitted):  # the gains of this round are solved on the host while the next round fits
            if after_fit is not None:
                reg, extras[i] = reg
            regs[i] = reg
            if reg is not None and not device_gain and not device_build:
                futures[i] = pool.submit(gain_of, i, reg)
    t1 = time.perf_counter()
    gains = [None] * n
    if device_gain:
        fitted_idx = [i for i in range(n) if regs[i] is not None]
        if fitted_idx:
            from .regressors import _lqr_gain_batch
            Ks, status, _ = (gain_batch_fn or _lqr_gain_batch)([regs[i] for i in fitted_idx], c)
            for i, K, st in zip(fitted_idx, Ks, status):
                if int(st) == 0:
                    gains[i] = np.asarray(K, dtype=np.float64)
    if device_build:
        fitted_idx = [i for i in range(n) if regs[i] is not None]
        if fitted_idx:
            from .regressors import _mpc_controller_batch
            ctrls, status = (controller_batch_fn or _mpc_controller_batch)([regs[i] for i in fitted_idx], c, controller)
            for i, ctrl, st in zip(fitted_idx, ctrls, status):
                if int(st) == 0:
                    gains[i] = ctrl
    for i, f in enumerate(futures):
        if f is not None:
            try:
                gains[i] = f.result()  # (an lqr.MPCController with `controller`)
            except Exception:  # noqa: BLE001 -- a unit without a gain scores NaN, like GridSearchCV's error_score=nan
                gains[i] = None
    t2 = time.perf_counter()
    return regs, gains, extras, dict(fit_s=t1 - t0, gain_wait_s=t2 - t1, gain_cpu_s=float(sum(gain_s)))


CONTROLLER_KEYS = ("horizon", "u_min", "u_max", "du_min", "du_max", "iters", "tol", "rho", "build", "x_min", "x_max",
                   "y_horizon", "y_weight")


def lqr_controller_spec(controller):
    """The `controller` dict of lqr_sweep with its defaults filled in (limits None = absent, iters = 50, tol = 0.0, rho None
    = lqr.mpc_default_rho; the state limits x_min, x_max None = absent, y_horizon None = the horizon, y_weight = inf = hard
    rows; build = "host", or "device": the controllers of all units in one device call); `horizon` is required and an unknown
    key or build value is a ValueError.  None stays None."""
    if controller is None:
        return None
    spec = dict(u_min=None, u_max=None, du_min=None, du_max=None, iters=50, tol=0.0, rho=None, build="host", x_min=None,
                x_max=None, y_horizon=None, y_weight=np.inf)
    unknown = sorted(set(controller) - set(CONTROLLER_KEYS))
    if unknown:
        raise ValueError(f"controller has unknown keys {unknown}; known: {CONTROLLER_KEYS}")
    if "horizon" not in controller:
        raise ValueError("controller needs a 'horizon'")
    spec.update(controller)
    if spec["build"] not in ("host", "device"):
        raise ValueError(f"controller['build'] must be 'host' or 'device', got {spec['build']!r}")
    return spec


def lqr_controller_has_rows(spec):
    """Whether the units of a checked controller dict run with output rows and carry the ten MPC_OUT_SCORE_NAMES: x_min or
    x_max has a finite entry (what makes solve_mpc return an lqr.MPCOutputController) and iters != 0 (the saturated LQR has
    no rows)."""
    if spec is None or int(spec["iters"]) == 0:
        return False
    given = [np.asarray(spec[k], dtype=np.float64) for k in ("x_min", "x_max") if spec[k] is not None]
    return any(np.any(np.isfinite(a)) for a in given)


def _run_live_units(gains, names, tm, loop, extras):
    """The tail of lqr_run_units and cloth_lqr_run_units after lqr_fit_and_gain (timing `tm`): res = loop(live) over the units
    with a gain; its columns `names` and the arrays res[key] of `extras` go into NaN-filled arrays over all units (extras:
    key -> trailing shape, or None: res decides, None when no unit is live).  Returns (scores, extras, res, live, timing)."""
    import time
    t2 = time.perf_counter()
    n = len(gains)
    live = [i for i in range(n) if gains[i] is not None]
    scores = np.full((n, len(names)), np.nan)
    more = {key: None if tail is None else np.full((n,) + tail, np.nan) for key, tail in extras.items()}
    res = None
    if live:
        res = loop(live)
        for k, name in enumerate(names):
            scores[live, k] = res[name]
        for key in extras:
            if more[key] is None:
                more[key] = np.full((n,) + np.shape(res[key])[1:], np.nan)
            more[key][live] = res[key]
    loop_s = time.perf_counter() - t2
    timing = dict(fit_s=tm["fit_s"], gain_wait_s=tm["gain_wait_s"], loop_s=loop_s, gain_cpu_s=tm["gain_cpu_s"],
                  total_s=tm["fit_s"] + tm["gain_wait_s"] + loop_s)
    return scores, more, res, live, timing


def lqr_run_units(X, Y, n_inputs, params, units, plant, x0, x_ref, num_steps, estimator="nystrom", gain_fn=None, c=1.0,
                  u_opt=None, batch=32, workers=4, return_trajectories=False, fit_fn=None, loop_fn=None, gain="host",
                  gain_batch_fn=None, controller=None, controller_batch_fn=None):
    """Scores of planned units, in their order: an (n_units, 4) array (SCORE_NAMES; NaN for a unit whose fit or gain
    failed), the trajectories (or None, None) and the wall-clock split.  fit_fn / loop_fn stand in for lqr_fit_unit /
    plant_loop_multi (rehearsals without a GPU; with a fit_fn the fits run as a plain loop).
    gain="device": the gains of all fitted units come from ONE nk_model_lqr_gain_batch call after the fits (K =
    dlqr(A, B, c sym(C'C), I) by the batched doubling solver; gain_fn is not used); a unit whose solve reports a non-zero
    status gets NaN scores and is not run.  timing keeps its keys: gain_wait_s is that call, gain_cpu_s is 0.
    gain_batch_fn(regs, c) -> (Ks, status, iterations) stands in for the device call.
    controller (lqr_sweep's dict): the units run the constrained MPC instead -- reg.solve_mpc per fitted unit where the
    gains are built, ONE mpc_loop_multi call (loop_fn stands in for it, with its signature), eight scores per unit
    (MPC_SCORE_NAMES); a unit whose controller raises scores NaN and is not run.  gain="device" with it is a ValueError.
    With a state limit in the dict (lqr_controller_has_rows) the units run with their output rows and carry the ten
    MPC_OUT_SCORE_NAMES.  build="device" in the dict: the controllers of all fitted units from ONE nk_model_mpc_build_batch call
    after the fits (lqr_fit_and_gain; controller_batch_fn stands in for it); a unit with a non-zero status scores NaN."""
    controller = lqr_controller_spec(controller)
    if controller is not None and gain == "device":
        raise ValueError("controller needs gain='host': the terminal cost of the MPC is the host Riccati solution")
    names = SCORE_NAMES if controller is None else MPC_OUT_SCORE_NAMES if lqr_controller_has_rows(controller) else MPC_SCORE_NAMES
    loop_fn = loop_fn or (plant_loop_multi if controller is None else mpc_loop_multi)
    regs, gains, _, tm = lqr_fit_and_gain(X, Y, n_inputs, params, units, estimator, gain_fn, c, batch, workers, fit_fn, gain,
                                          gain_batch_fn, controller=controller, controller_batch_fn=controller_batch_fn)
    kw = {} if controller is None else dict(iters=controller["iters"], tol=controller["tol"])

    def loop(live):
        return loop_fn([regs[i] for i in live], [gains[i] for i in live], x0, x_ref, num_steps, plant, u_opt=u_opt,
                       return_trajectories=return_trajectories, **kw)

    scores, more, _, _, timing = _run_live_units(gains, names, tm, loop,
                                                 dict(states=None, controls=None) if return_trajectories else {})
    return scores, more.get("states"), more.get("controls"), timing


def lqr_table(units, values, n_seeds, n_ms):
    """(seed, m) table from per-unit values in plan order: sysid_table with its single test slot dropped; per-unit arrays
    (trajectories) keep their trailing axes."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1:
        return sysid_table(units, values, n_seeds, n_ms)[:, 0, :]
    out = np.full((n_seeds, n_ms) + values.shape[1:], np.nan)
    for u, v in zip(units, values):
        out[u["si"], u["k"]] = v
    return out


def lqr_sweep(X, Y, n_inputs, params, ms, seeds, plant, x0, x_ref, num_steps, estimator="nystrom", gain_fn=None, c=1.0,
              u_opt=None, batch=32, workers=4, return_trajectories=False, centers=None, fit_fn=None, loop_fn=None,
              gain="host", gain_batch_fn=None, controller=None, controller_batch_fn=None):
    """The control branch of the reference's one-input drivers (benchmark_lqr_classic.py:256-299: seeds x {Nystrom,
    splines}; benchmark_lqr_hjb.py:265-333: seeds x m) as one call: for every seed and every m in `ms`
    fit -> K = dlqr(A, B, c C^T C, I) -> `num_steps` feedback steps around the true plant -> replay cost and control scores.
      draws:  sysid_plan's per-seed protocol (lqr_plan): one RandomState(seed) per seed, reference order; `centers`
              {(seed, k): landmarks} replaces them;
      fits:   `batch` at a time through the lock-step pool (batch <= 1: a plain loop; same bits);
      gains:  gain_fn(A, B, C) -> K (1 x m) (default lqr_default_gain(c): the host Riccati solve), computed in `workers`
              host threads while later rounds fit; a unit whose gain raises gets NaN scores and is not run;
              gain="device": all gains in ONE nk_model_lqr_gain_batch call after the fits instead (see lqr_run_units;
              gain="host" stays the choice for replaying the reference's numbers);
      loops:  ONE plant_loop_multi call over all surviving units, scored on the device (u_opt: (num_steps,) or None).
    x0, x_ref: one state each, shared by the units.  Returns a dict of (len(seeds), len(ms)) tables sse_u, ss_opt, J,
    u_absmax, rmse_control, the planned `units`, the wall-clock split `timing` (fit_s, gain_wait_s, loop_s; gain_cpu_s =
    host seconds summed over the gain solves, which overlap the fits) and, with return_trajectories, states
    (len(seeds), len(ms), num_steps + 1, d) and controls (len(seeds), len(ms), num_steps).
    controller: None, or a dict (horizon, and optionally u_min, u_max, du_min, du_max, iters = 50, tol = 0, rho) -- the
    sweep under actuator limits: every fitted unit gets reg.solve_mpc(horizon, c=c, limits) where the gains are built (host
    threads, while later rounds fit), all surviving units run in ONE mpc_loop_multi call, the tables gain iters_sum, r_max,
    n_at_limit and n_iterated (MPC_SCORE_NAMES), the plant may have several inputs (controls: (.., num_steps, p)) and must be
    one closed_loop_plant_mpc accepts.  gain_fn is not used; gain="device" is a ValueError.
    The dict may also hold x_min, x_max (scalars or d entries), y_horizon and y_weight, passed to reg.solve_mpc: limits on the
    PREDICTED states, hard (y_weight = inf, the default) or soft.  The units then run with their output rows in ONE
    nk_mpc_out_loop_multi call and the tables gain y_viol_max (the largest excursion of the plant past its state limits) and
    n_y_viol (the steps with one): the ten MPC_OUT_SCORE_NAMES.  rho stays the user's to set: the rows of a sampled plant are
    small beside the identity rows of the inputs, so the output rows want a rho far above the default (300 x the default
    reached a hard velocity limit within 2 % in 100 iterations on the Duffing models; with the default the controls did not
    move).  build="device" in the dict builds the controllers of all fitted units in ONE device call after the fits
    (nk_model_mpc_build_batch: Riccati, one Newton step and the condensing on the device; controller_batch_fn(regs, c,
    controller) stands in for it) instead of reg.solve_mpc per unit on host threads; the default "host" is what it was."""
    _check_estimator(estimator)
    units = lqr_plan(X, Y, n_inputs, params, ms, seeds, estimator, centers)
    scores, states, controls, timing = lqr_run_units(X, Y, n_inputs, params, units, plant, x0, x_ref, num_steps, estimator,
                                                     gain_fn, c, u_opt, batch, workers, return_trajectories, fit_fn, loop_fn,
                                                     gain, gain_batch_fn, controller, controller_batch_fn)
    return lqr_result(units, scores, states, controls, len(seeds), len(ms), timing)


def lqr_result(units, scores, states, controls, n_seeds, n_ms, timing=None):
    """The dict lqr_sweep returns, from per-unit values in plan order (four score columns, the eight of the MPC sweep, or the
    ten of the MPC sweep under state limits)."""
    names = {len(MPC_SCORE_NAMES): MPC_SCORE_NAMES, len(MPC_OUT_SCORE_NAMES): MPC_OUT_SCORE_NAMES}.get(np.shape(scores)[1],
                                                                                                      SCORE_NAMES)
    out = {name: lqr_table(units, scores[:, k], n_seeds, n_ms) for k, name in enumerate(names)}
    out["rmse_control"] = rmse_control_percent(out["sse_u"], out["ss_opt"])
    out["units"], out["timing"] = units, timing
    if states is not None:
        out["states"], out["controls"] = lqr_table(units, states, n_seeds, n_ms), lqr_table(units, controls, n_seeds, n_ms)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the CLOTH control sweep (benchmark_lqr_cloth.py:213-270): seeds x {Nystrom, splines}, lifted closed loop
# ---------------------------------------------------------------------------------------------------------------
LOOP_SCORE_NAMES = ("J", "err_final", "u_sumsq", "u_absmax")
LOOP_MULTI_MAX_M = 128  # nk_closed_loop_multi keeps [A B] in the registers of one workgroup


def closed_loop_scores(states, controls, target, c=0.0075, u_init=None):
    """What nk_closed_loop_multi reduces on the device, on the host by the same formulas, from one loop's states
    (steps, d), controls (steps, p) and the target (d,): e_t = sqrt(sum_k (x_{t,k} - target_k)^2 / d),
    J = sum_t (c sum_k (x_{t,k} - target_k)^2 + sum_j u_{t,j}^2), err_final = e_{steps-1}, u_sumsq, u_absmax (NaN from the
    first NaN control on) and the cumulative inputs s_0 = u_init (zeros), s_{t+1} = s_t + u_t.  Returns a dict.  Needs no GPU."""
    xs = np.asarray(states, dtype=np.float64)
    us = np.asarray(controls, dtype=np.float64)
    steps, d = xs.shape
    with np.errstate(all="ignore"):
        sse = np.sum(np.square(xs - np.asarray(target, dtype=np.float64).reshape(1, d)), axis=1)
        usq = np.sum(np.square(us), axis=1)
        J = 0.0
        for t in range(steps):
            J = J + (c * sse[t] + usq[t])
        au = np.abs(us)
        cum = np.empty((steps + 1, us.shape[1]))
        cum[0] = 0.0 if u_init is None else np.asarray(u_init, dtype=np.float64).reshape(-1)
        for t in range(steps):
            cum[t + 1] = cum[t] + us[t]
        err = np.sqrt(sse / d)
    return dict(J=float(J), err_final=float(err[-1]), u_sumsq=float(np.sum(usq)),
                u_absmax=float("nan") if np.any(np.isnan(au)) else float(np.max(au)), err=err, cum_controls=cum)


def closed_loop_multi_lifted(regressors, gains, lifts, targets, num_steps, c=0.0075, u_inits=None,
                             return_trajectories=False):
    """closed_loop_multi after the lifts: lifts[u] = (phi0, phi_ref), two (m,) vectors."""
    regs = list(regressors)
    n = len(regs)
    num_steps = int(num_steps)
    if not (len(gains) == len(lifts) == len(targets) == n):
        raise ValueError("regressors, gains, lifts and targets must have the same length")
    u_inits = [None] * n if u_inits is None else list(u_inits)
    dims = []
    for r, K in zip(regs, gains):
        d, m = r._landmark_shape()
        p = int(r.n_inputs)
        if np.shape(K) != (p, m):
            raise ValueError(f"gain has shape {np.shape(K)}, expected {(p, m)}")
        dims.append((int(m), p, int(d)))
    out = {name: np.full(n, np.nan) for name in LOOP_SCORE_NAMES}
    out["err"] = np.full((n, num_steps), np.nan)
    out["path"] = ["device" if dm[0] <= LOOP_MULTI_MAX_M else "single" for dm in dims]
    states, controls, cums = [None] * n, [None] * n, [None] * n
    dev = [i for i in range(n) if out["path"][i] == "device"]
    if dev:
        sc, err, ox, ou, oc = _lib.get_context().closed_loop_multi(
            num_steps, c, [regs[i]._ensure_model() for i in dev], [dims[i] for i in dev], [gains[i] for i in dev],
            [lifts[i][0] for i in dev], [lifts[i][1] for i in dev], [targets[i] for i in dev], [u_inits[i] for i in dev],
            want_x=return_trajectories, want_u=return_trajectories, want_ucum=return_trajectories)
        for k, name in enumerate(LOOP_SCORE_NAMES):
            out[name][dev] = sc[:, k]
        out["err"][dev] = err
        if return_trajectories:
            for k, i in enumerate(dev):
                states[i], controls[i], cums[i] = ox[k], ou[k], oc[k]
    for i in range(n):  # a model beyond one workgroup's registers: the single-model call, scored on the host
        if out["path"][i] == "device":
            continue
        xs, us = regs[i].closed_loop(np.asarray(gains[i], dtype=np.float64), lifts[i][0], lifts[i][1], num_steps)
        sc = closed_loop_scores(xs.T, us.T, targets[i], c, u_inits[i])
        for name in LOOP_SCORE_NAMES:
            out[name][i] = sc[name]
        out["err"][i] = sc["err"]
        states[i], controls[i], cums[i] = np.ascontiguousarray(xs.T), np.ascontiguousarray(us.T), sc["cum_controls"]
    if return_trajectories:
        same = len({dm[1:] for dm in dims}) == 1  # equal (p, d): plain 3-D arrays, otherwise lists of per-unit arrays
        out["states"] = np.stack(states) if same else states
        out["controls"] = np.stack(controls) if same else controls
        out["cum_controls"] = np.stack(cums) if same else cums
    return out


def _per_unit(x, n, what):
    """One state for all n units (a vector / column) or one per unit (a sequence of n, or an (n, d) array), as n vectors: the
    rule of closed_loop_multi, whose units may differ in d.  The shape decides: a flat array of any length is ONE state and a
    sequence of n numbers is n states -- _broadcast_states reads n d numbers as rows and d = n numbers as one state."""
    if isinstance(x, np.ndarray) and (x.ndim == 1 or (x.ndim == 2 and x.shape[1] == 1)):
        return [x.reshape(-1)] * n
    x = list(x)
    if len(x) != n:
        if all(np.ndim(v) == 0 for v in x):
            return [np.asarray(x, dtype=np.float64)] * n
        raise ValueError(f"{what}: {len(x)} entries for {n} units")
    return [np.asarray(v, dtype=np.float64).reshape(-1) for v in x]


def closed_loop_multi(regressors, gains, x0s, x_refs, num_steps, c=0.0075, u_inits=None, targets=None,
                      return_trajectories=False):
    """The lifted closed loop of lqr_control (benchmark_lqr_cloth.py:73-84) for every (regressor, gain, x0, x_ref) unit in
    ONE device call (nk_closed_loop_multi), scored on the device: per step u_t = K (phi_ref - phi_t), x_t = C phi_t,
    phi_{t+1} = A phi_t + B u_t.  The units may mix model kinds, m, p and d.  x0s, x_refs: one state for all units or one
    per unit; each regressor lifts its [x0, x_ref] with one `lift` call.  targets: the state each loop is scored against
    (default: its x_ref).  u_inits: per unit, the seed of the cumulative input sequence (None: zeros).
    Returns a dict of (n_units,) arrays J, err_final, u_sumsq, u_absmax (include/nyskoop.h), err (n_units, num_steps) =
    RMSE per step (plot_reg_error_cloth.py:24), and path: per unit "device" or "single" -- a regressor with m > 128 runs
    through its own closed_loop call and is scored on the host by the same formulas.  With return_trajectories also states
    (n_units, num_steps, d), controls (n_units, num_steps, p) and cum_controls (n_units, num_steps + 1, p) (lists of
    per-unit arrays when the units differ in p or d).  Without them nothing but the scores and errors leaves the device."""
    regs = list(regressors)
    n = len(regs)
    x0s, x_refs = _per_unit(x0s, n, "x0s"), _per_unit(x_refs, n, "x_refs")
    targets = x_refs if targets is None else _per_unit(targets, n, "targets")
    lifts = []
    for r, x0, xr in zip(regs, x0s, x_refs):
        phi = r.lift(np.stack((x0, xr), axis=1))  # one call for both lifts
        lifts.append((np.ascontiguousarray(phi[:, 0]), np.ascontiguousarray(phi[:, 1])))
    return closed_loop_multi_lifted(regs, list(gains), lifts, targets, num_steps, c, u_inits, return_trajectories)


def cloth_control_layout(initial_state, states, cum_controls, simulator_order=(0, 3, 1, 4, 2, 5)):
    """What lqr_control returns (benchmark_lqr_cloth.py:85-104), from one unit of closed_loop_multi: states (steps, d) and
    cum_controls (steps + 1, p).  Returns (x_s, y_s, z_s, final_us) in the layout of harness.lqr_control."""
    x0 = np.asarray(initial_state, dtype=np.float64).reshape(-1, 1)
    visited = np.hstack((x0, np.asarray(states, dtype=np.float64).T))
    final_us = np.asarray(cum_controls, dtype=np.float64).T[list(simulator_order), :]
    return visited[0::3], visited[1::3], visited[2::3], final_us


def cloth_lqr_plan(X, Y, n_inputs, params, m, seeds, estimator="nystrom", centers=None):
    """The units of cloth_lqr_sweep: per estimator lqr_plan with the one landmark count `m` (np.random.seed(seed) in front
    of every fit, benchmark_lqr_cloth.py:216-233), estimator-major; each unit carries its "estimator", "params" and "ei"
    (position of the estimator).  estimator: a name or a sequence of names; with a sequence `params` (and `centers`) are
    dicts keyed by the name.  Needs no GPU."""
    names = [estimator] if isinstance(estimator, str) else list(estimator)
    units = []
    for ei, name in enumerate(names):
        _check_estimator(name)
        par = params if isinstance(estimator, str) else params[name]
        cen = centers if isinstance(estimator, str) or centers is None else centers.get(name)
        cen = None if cen is None else {(s, 0): v for s, v in cen.items()}
        for u in lqr_plan(X, Y, n_inputs, par, [int(m)], seeds, name, cen):
            units.append(dict(u, estimator=name, params=par, ei=ei))
    return names, units


def cloth_lqr_run_units(X, Y, n_inputs, units, x0, x_ref, num_steps=60, c=0.0075, gain="host", batch=32, workers=4,
                        control_nodes=(168, 169, 170, 189, 190, 191), return_trajectories=False, fit_fn=None, loop_fn=None,
                        gain_batch_fn=None):
    """Planned units of the cloth sweep: fits (the lifts of x0 / x_ref inside the lock-step round, right after each
    member's fit), gains (lqr_fit_and_gain) and ONE closed_loop_multi call over the units that have a gain.  Returns
    (scores (n_units, 4) in LOOP_SCORE_NAMES order, err (n_units, num_steps), gains, result of the loop call or None,
    indices of the units it held, timing); a unit whose fit or gain failed is NaN and is not submitted."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    x_ref = np.asarray(x_ref, dtype=np.float64).reshape(-1)
    both = np.stack((x0, x_ref), axis=1)
    u_init = None if control_nodes is None else np.ascontiguousarray(x0[list(control_nodes)])
    loop_fn = loop_fn or closed_loop_multi_lifted

    def lifted(reg, unit):
        phi = reg.lift(both)
        return np.ascontiguousarray(phi[:, 0]), np.ascontiguousarray(phi[:, 1])

    regs, gains, lifts, tm = lqr_fit_and_gain(X, Y, n_inputs, None, units, "nystrom", None, c, batch, workers, fit_fn, gain,
                                              gain_batch_fn, after_fit=lifted)

    def loop(live):
        return loop_fn([regs[i] for i in live], [gains[i] for i in live], [lifts[i] for i in live], [x_ref] * len(live),
                       num_steps, c, [u_init] * len(live), return_trajectories)

    scores, more, res, live, timing = _run_live_units(gains, LOOP_SCORE_NAMES, tm, loop, dict(err=(int(num_steps),)))
    return scores, more["err"], gains, res, live, timing


def cloth_lqr_result(names, units, scores, err, n_seeds, single, timing=None):
    """The tables of cloth_lqr_sweep from per-unit values in plan order: (n_seeds,) for one estimator name, else
    (len(names), n_seeds)."""
    def table(values):
        values = np.asarray(values, dtype=np.float64)
        out = np.full((len(names), n_seeds) + values.shape[1:], np.nan)
        for u, v in zip(units, values):
            out[u["ei"], u["si"]] = v
        return out[0] if single else out

    out = {name: table(scores[:, k]) for k, name in enumerate(LOOP_SCORE_NAMES)}
    out["err"] = table(err)
    out["estimators"], out["units"], out["timing"] = names, units, timing
    return out


def cloth_lqr_sweep(X, Y, n_inputs, params, m, seeds, x0, x_ref, num_steps=60, estimator="nystrom", c=0.0075, gain="host",
                    batch=32, workers=4, control_nodes=(168, 169, 170, 189, 190, 191), return_trajectories=False,
                    centers=None, fit_fn=None, loop_fn=None, gain_batch_fn=None):
    """The control branch of benchmark_lqr_cloth.py:213-270 as one call: for every seed (and every estimator) fit at `m`
    landmarks -> K = dlqr(A, B, c C'C, I) -> `num_steps` steps of the lifted closed loop of lqr_control from x0 towards
    x_ref, with its cumulative input sequence seeded by x0[control_nodes].
      draws:  lqr_plan's per-seed protocol (one RandomState(seed) per seed and estimator); `centers` {seed: landmarks}
              replaces them.  estimator: "nystrom", "spline", or a sequence of both with params = {name: params}: then
              every table gets a leading estimator axis and all units still share the ONE loop call;
      fits:   `batch` at a time through the lock-step pool (batch <= 1: a plain loop; same bits); each member lifts
              [x0, x_ref] right after its fit, inside the round;
      gains:  gain="host": regressor.solve_lqr's arithmetic in `workers` host threads while later rounds fit;
              gain="device": ONE nk_model_lqr_gain_batch call after the fits; a unit without a gain is NaN and is not run;
      loops:  ONE closed_loop_multi call over all surviving units, scored on the device against x_ref.
    Returns a dict of per-seed tables J, err_final, u_sumsq, u_absmax (len(seeds),) and err (len(seeds), num_steps), the
    planned `units`, `estimators` and the wall-clock split `timing` (fit_s, gain_wait_s, loop_s, gain_cpu_s, total_s).
    With return_trajectories also x_s, y_s, z_s (len(seeds), d / 3, num_steps + 1) and final_us (len(seeds), p,
    num_steps + 1) in the layout of harness.lqr_control, the raw states (len(seeds), num_steps, d) and controls
    (len(seeds), num_steps, p) of the loop call, K (len(seeds), p, m) and K_sim, the gains with the rows in the
    simulator's order (lqr.cloth_gain_for_simulator, benchmark_lqr_cloth.py:263); failed units are NaN.
    fit_fn / loop_fn / gain_batch_fn stand in for lqr_fit_unit / closed_loop_multi_lifted / the device gain call."""
    single = isinstance(estimator, str)
    names, units = cloth_lqr_plan(X, Y, n_inputs, params, m, seeds, estimator, centers)
    scores, err, gains, res, live, timing = cloth_lqr_run_units(X, Y, n_inputs, units, x0, x_ref, num_steps, c, gain, batch,
                                                                workers, control_nodes, return_trajectories, fit_fn,
                                                                loop_fn, gain_batch_fn)
    out = cloth_lqr_result(names, units, scores, err, len(seeds), single, timing)
    if return_trajectories:
        from .lqr import cloth_gain_for_simulator
        n_seeds, p, steps = len(seeds), int(n_inputs), int(num_steps)
        d = np.asarray(x0).size
        shape = (len(names), n_seeds)
        tabs = dict(x_s=np.full(shape + (d // 3, steps + 1), np.nan), y_s=np.full(shape + (d // 3, steps + 1), np.nan),
                    z_s=np.full(shape + (d // 3, steps + 1), np.nan), final_us=np.full(shape + (p, steps + 1), np.nan),
                    K=np.full(shape + (p, int(m)), np.nan), K_sim=np.full(shape + (p, int(m)), np.nan),
                    states=np.full(shape + (steps, d), np.nan), controls=np.full(shape + (steps, p), np.nan))
        for k, i in enumerate(live):
            at = (units[i]["ei"], units[i]["si"])
            xs, ys, zs, fu = cloth_control_layout(x0, res["states"][k], res["cum_controls"][k])
            tabs["x_s"][at], tabs["y_s"][at], tabs["z_s"][at], tabs["final_us"][at] = xs, ys, zs, fu
            tabs["K"][at], tabs["states"][at] = gains[i], res["states"][k]
            if "controls" in res:
                tabs["controls"][at] = res["controls"][k]
            tabs["K_sim"][at] = cloth_gain_for_simulator(np.asarray(gains[i])) if p == 6 else gains[i]
        out.update({k: (v[0] if single else v) for k, v in tabs.items()})
    return out


def create_data_matrices(trajs, controls, indices):
    """benchmark_lqr_cloth.py:117-130: snapshot pairs from trajectories (d x T) and controls (p x T)."""
    states = np.hstack([trajs[i][:, :-1] for i in indices])
    next_states = np.hstack([trajs[i][:, 1:] for i in indices])
    inputs = np.hstack([controls[i][:, :-1] for i in indices])
    return np.vstack((states, inputs)), next_states
