"""What the Python bindings of the loop and batch entry points hand to the library, without a GPU and without the
library: a recording stand-in takes the place of libnyskoop.so, reads the unit tables and every pointer argument back from
memory (after a garbage collection, so an array that nothing keeps alive shows) and fills every output buffer with a
counting pattern.  The tests compare what it read with values computed here, and what the bindings return with the
pattern.  Covers _lib.Context (the nine packing methods and the four single-call loops), the single / batch rule of
regressors.closed_loop_plant / closed_loop_plant_mpc and the per-unit defaults of harness.plant_loop_multi /
mpc_loop_multi."""
import ctypes as C
import gc
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import _lib, harness

CTX_HANDLE = 7
PLANT_MSG = ("plant must be one of the package's dynamical systems (plant_id) or a PolynomialSystem, with its step length "
             "Ts set")


# ------------------------------------------------------------------------------------------------- the stand-in library
def _addr(a):
    """The address behind whatever a binding may hand to a pointer parameter; None for a null pointer."""
    if a is None:
        return None
    if isinstance(a, int):
        return a or None
    if hasattr(a, "_obj"):  # ctypes.byref(x)
        return C.addressof(a._obj)
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value
    return C.addressof(a)  # a structure or an array, passed as it is


def _view(a, shape, ctype=C.c_double):
    shape = tuple(int(s) for s in shape)
    addr = _addr(a)
    if addr is None:
        return None
    if int(np.prod(shape)) == 0:
        return np.zeros(shape, dtype=np.dtype(ctype))
    return np.ctypeslib.as_array(C.cast(addr, C.POINTER(ctype)), shape)


def _read(a, shape, ctype=C.c_double):
    v = _view(a, shape, ctype)
    return None if v is None else v.copy()


def _fill(a, count, base):
    """base, base + 1, ... into a non-null buffer of `count` numbers; returns whether the pointer was null."""
    v = _view(a, (count,))
    if v is not None and count:
        v[:] = base + np.arange(count)
    return v is None


def _pattern(base, shape):
    return base + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


X_BASE, U_BASE, I_BASE, S_BASE, E_BASE, C_BASE = 1000.0, 2000.0, 3000.0, 4000.0, 5000.0, 6000.0


class FakeLib:
    """nk_* entry points as Python functions.  `hint` carries what a unit table does not say (landmark counts, d, p)."""

    def __init__(self, decode=True):
        self.calls, self.hint, self.decode = [], {}, decode

    def _rec(self, name, **kw):
        kw["name"] = name
        self.calls.append(kw)
        return 0

    @property
    def last(self):
        return self.calls[-1]

    # --- unit-table loops
    def _loop_units(self, arr, n, d, p, mpc):
        units = []
        for i in range(n):
            a, m = arr[i], self.hint["ms"][i]
            u = dict(model=a.model, x0=_read(a.x0, (d,)), x_ref=_read(a.x_ref, (d,)), uopt=a.uopt, reserved=a.reserved)
            if mpc:
                u["desc"] = C.addressof(a.desc.contents)
                u["u_init"] = _read(a.u_init, (p,))
            else:
                u["K"] = _read(a.K, (p * m,))
            units.append(u)
        return units

    def _loop_multi(self, name, ctx, steps, arr, n, uo, n_uopt, ox, ou, oi, sc, ncol, mpc, **extra):
        gc.collect()
        if not self.decode:
            return 0
        d, p, T = self.hint["d"], self.hint["p"], max(steps, 0)
        nulls = dict(x=_fill(ox, n * (T + 1) * d, X_BASE), u=_fill(ou, n * T * p, U_BASE), sc=_fill(sc, n * ncol, S_BASE))
        if mpc:
            nulls["info"] = _fill(oi, n * T * 2, I_BASE)
        return self._rec(name, ctx=ctx.value, steps=steps, n=n, n_uopt=n_uopt, table_len=len(arr),
                         units=self._loop_units(arr, n, d, p, mpc), uo=_read(uo, (n_uopt, max(steps, 1) * p)), nulls=nulls,
                         **extra)

    def nk_plant_loop_multi(self, ctx, plant_id, Ts, steps, arr, n, uo, n_uopt, ox, ou, sc):
        return self._loop_multi("nk_plant_loop_multi", ctx, steps, arr, n, uo, n_uopt, ox, ou, None, sc, 4, False,
                                plant_id=plant_id, Ts=Ts)

    def nk_poly_plant_loop_multi(self, ctx, desc, steps, arr, n, uo, n_uopt, ox, ou, sc):
        return self._loop_multi("nk_poly_plant_loop_multi", ctx, steps, arr, n, uo, n_uopt, ox, ou, None, sc, 4, False,
                                plant=_addr(desc))

    def nk_mpc_loop_multi(self, ctx, desc, steps, arr, n, uo, n_uopt, ox, ou, oi, sc):
        return self._loop_multi("nk_mpc_loop_multi", ctx, steps, arr, n, uo, n_uopt, ox, ou, oi, sc, 8, True, plant=_addr(desc))

    def nk_mpc_out_loop_multi(self, ctx, desc, steps, arr, oarr, n, uo, n_uopt, ox, ou, oi, sc):
        outs = [C.addressof(oarr[i].contents) if oarr[i] else None for i in range(n)]
        return self._loop_multi("nk_mpc_out_loop_multi", ctx, steps, arr, n, uo, n_uopt, ox, ou, oi, sc, 10, True,
                                plant=_addr(desc), outs=outs, out_len=len(oarr))

    def nk_closed_loop_multi(self, ctx, steps, c, arr, n, ox, ou, oc, oe, sc):
        gc.collect()
        if not self.decode:
            return 0
        dims, T = self.hint["dims"], max(steps, 0)
        units = []
        for i in range(n):
            a, (m, p, d) = arr[i], dims[i]
            units.append(dict(model=a.model, K=_read(a.K, (p * m,)), phi0=_read(a.phi0, (m,)), phi_ref=_read(a.phi_ref, (m,)),
                              target=_read(a.target, (d,)), u_init=_read(a.u_init, (p,))))
        nulls = dict(x=_fill(ox, sum(T * dm[2] for dm in dims), X_BASE), u=_fill(ou, sum(T * dm[1] for dm in dims), U_BASE),
                     ucum=_fill(oc, sum((T + 1) * dm[1] for dm in dims), C_BASE), err=_fill(oe, n * T, E_BASE),
                     sc=_fill(sc, n * 4, S_BASE))
        return self._rec("nk_closed_loop_multi", ctx=ctx.value, steps=steps, c=c, n=n, units=units, nulls=nulls)

    # --- batched solvers and builds
    @staticmethod
    def _status(status, iters, n, per=1):
        _view(status, (n,), C.c_int32)[:] = np.arange(n) % 3
        _view(iters, (n * per,), C.c_int32)[:] = 10 + np.arange(n * per)

    @staticmethod
    def _abqr(a):
        m, p = a.m, a.p
        return dict(m=m, p=p, lda=a.lda, ldb=a.ldb, ldq=a.ldq, ldr=a.ldr, A=_read(a.A, (m, m)), B=_read(a.B, (m, p)),
                    Q=_read(a.Q, (m, m)), R=_read(a.R, (p, p)))

    def nk_dare_batch(self, ctx, arr, n, tol, max_iter, status, iters):
        gc.collect()
        if not self.decode:
            return 0
        probs = []
        for i in range(n):
            a = arr[i]
            pr = self._abqr(a)
            pr["P_null"] = _fill(a.out_P, a.m * a.m, 200.0 * (i + 1))
            _fill(a.out_K, a.p * a.m, 100.0 * (i + 1))
            _fill(a.out_delta, 1, 0.5 + i)
            probs.append(pr)
        self._status(status, iters, n)
        return self._rec("nk_dare_batch", ctx=ctx.value, n=n, tol=tol, max_iter=max_iter, probs=probs)

    def nk_mpc_build_batch(self, ctx, arr, n, tol, max_iter, newton_steps, newton_tol, newton_max_iter, status, iters):
        gc.collect()
        if not self.decode:
            return 0
        probs = []
        for i in range(n):
            a = arr[i]
            pr = self._abqr(a)
            m, p, nv, ny = a.m, a.p, max(a.N, 0) * a.p, a.nc * max(a.Ny, 0)
            pr.update(N=a.N, nc=a.nc, Ny=a.Ny, ldp=a.ldp, ldc=a.ldc, P=_read(a.P, (m, m)), C_rows=_read(a.C_rows, (a.nc, m)))
            b = 1000.0 * (i + 1)
            pr["nulls"] = dict(H=_fill(a.out_H, nv * nv, b + 100), F=_fill(a.out_F, nv * m, b + 200), K=_fill(a.out_K, p * m, b + 300),
                               P=_fill(a.out_P, m * m, b + 400), G=_fill(a.out_G, ny * nv, b + 500), T=_fill(a.out_T, ny * m, b + 600))
            probs.append(pr)
        self._status(status, iters, n, 2)
        return self._rec("nk_mpc_build_batch", ctx=ctx.value, n=n, solver=(tol, max_iter, newton_steps, newton_tol, newton_max_iter),
                         probs=probs)

    def nk_model_lqr_gain_batch(self, ctx, hs, n, c, R, tol, max_iter, out, status, iters):
        gc.collect()
        if not self.decode:
            return 0
        dims = self.hint["dims"]
        p0 = dims[0][1] if dims else 1
        _fill(out, sum(m * p for m, p in dims), 100.0)
        self._status(status, iters, n)
        return self._rec("nk_model_lqr_gain_batch", ctx=ctx.value, n=n, c=c, tol=tol, max_iter=max_iter, hs_len=len(hs),
                         models=[hs[i] for i in range(n)], R=_read(R, (p0, p0)))

    def nk_model_mpc_build_batch(self, ctx, hs, n, c, R, sp, tol, max_iter, newton_steps, newton_tol, newton_max_iter, ou, status,
                                 iters):
        gc.collect()
        if not self.decode:
            return 0
        dims = self.hint["dims"]
        specs, nulls = [], []
        for i in range(n):
            (m, p), s, o = dims[i], sp[i], ou[i]
            nv, ny = max(s.N, 0) * p, s.nc * max(s.Ny, 0)
            specs.append((s.N, s.nc, list(s.comps), s.Ny))
            b = 1000.0 * (i + 1)
            nulls.append(dict(H=_fill(o.H, nv * nv, b + 100), F=_fill(o.F, nv * m, b + 200), K=_fill(o.K, p * m, b + 300),
                              G=_fill(o.G, ny * nv, b + 500), T=_fill(o.T, ny * m, b + 600)))
        self._status(status, iters, n, 2)
        p0 = dims[0][1] if dims else 1
        return self._rec("nk_model_mpc_build_batch", ctx=ctx.value, n=n, c=c, models=[hs[i] for i in range(n)], specs=specs,
                         nulls=nulls, solver=(tol, max_iter, newton_steps, newton_tol, newton_max_iter), R=_read(R, (p0, p0)))

    def nk_model_lqr_gain(self, ctx, h, c, R, tol, max_iter, K, status, iters):
        gc.collect()
        if not self.decode:
            return 0
        m, p = self.hint["dims"][0]
        _fill(K, p * m, 100.0)
        status._obj.value, iters._obj.value = 1, 17
        return self._rec("nk_model_lqr_gain", ctx=ctx.value, model=_addr(h), c=c, tol=tol, max_iter=max_iter, R=_read(R, (p, p)))

    def nk_poly_plant_step(self, desc, x, u, out):
        return 0

    # --- single-model loops
    def _loop(self, name, ctx, h, K, x0, xr, steps, batch, ox, ou, oi=None, mpc=False, lifted=False, **extra):
        gc.collect()
        if not self.decode:
            return 0
        d, p, m, T = self.hint["d"], self.hint["p"], self.hint["m"], max(steps, 0)
        w = m if lifted else d
        pu = p if self.hint.get("pu") is None else self.hint["pu"]
        nulls = dict(x=_fill(ox, batch * (T + (0 if lifted else 1)) * d, X_BASE), u=_fill(ou, batch * T * pu, U_BASE))
        if mpc:
            nulls["info"] = _fill(oi, batch * T * 2, I_BASE)
        return self._rec(name, ctx=ctx.value, model=_addr(h), K=_read(K, (p, m)), x0=_read(x0, (batch, w)), x_ref=_read(xr, (batch, w)),
                         steps=steps, batch=batch, nulls=nulls, **extra)

    def nk_closed_loop_batch(self, ctx, h, K, f0, fr, steps, batch, ox, ou):
        return self._loop("nk_closed_loop_batch", ctx, h, K, f0, fr, steps, batch, ox, ou, lifted=True)

    def nk_plant_loop(self, ctx, h, plant_id, Ts, K, x0, xr, steps, batch, ox, ou):
        return self._loop("nk_plant_loop", ctx, h, K, x0, xr, steps, batch, ox, ou, plant_id=plant_id, Ts=Ts)

    def nk_poly_plant_loop(self, ctx, h, desc, K, x0, xr, steps, batch, ox, ou):
        return self._loop("nk_poly_plant_loop", ctx, h, K, x0, xr, steps, batch, ox, ou, plant=_addr(desc))

    def _desc(self, ds):
        ds = ds._obj if hasattr(ds, "_obj") else ds
        return dict(N=ds.N, p=ds.p, m=ds.m, iters=ds.iters, tol=ds.tol, K=_read(ds.K, (ds.p, ds.m)))

    def nk_mpc_loop(self, ctx, h, desc, ds, x0, xr, ui, steps, batch, ox, ou, oi):
        return self._loop("nk_mpc_loop", ctx, h, None, x0, xr, steps, batch, ox, ou, oi, mpc=True, plant=_addr(desc),
                          desc=self._desc(ds), u_init=_read(ui, (batch, self.hint["p"])))

    def nk_mpc_out_loop(self, ctx, h, desc, ds, out, x0, xr, ui, steps, batch, ox, ou, oi):
        o = out._obj if hasattr(out, "_obj") else out
        return self._loop("nk_mpc_out_loop", ctx, h, None, x0, xr, steps, batch, ox, ou, oi, mpc=True, plant=_addr(desc),
                          desc=self._desc(ds), u_init=_read(ui, (batch, self.hint["p"])), ny=o.ny,
                          ycomp=_read(o.ycomp, (o.ny,), C.c_int32))


def make_context(lib=None):
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.handle, ctx.lib, ctx.device = C.c_void_p(CTX_HANDLE), lib or FakeLib(), 0
    return ctx


@pytest.fixture
def ctx():
    c = make_context()
    gc.collect()
    gc.freeze()  # what is alive now is not the bindings': the stand-in's collections then walk the new objects only
    yield c
    gc.unfreeze()
    c.handle = None  # (nothing to destroy)


@pytest.fixture
def patched(ctx, monkeypatch):
    """The stand-in context behind _lib.get_context, for the regressors / harness levels."""
    monkeypatch.setattr(_lib, "get_context", lambda device=None: ctx)
    monkeypatch.setattr(_lib, "load_library", lambda: ctx.lib)  # a PolynomialSystem has the library check its table
    return ctx


class FakeReg(nk.KoopmanNystromRegressor):
    """A regressor whose device model is a made-up handle."""

    def __init__(self, p, d, m, handle):
        super().__init__(p)
        self._shape, self._handle = (d, m), handle

    def _ensure_model(self):
        return self._handle

    def _landmark_shape(self):
        return self._shape


def _handles(n, kind):
    hs = [0x1000 + 16 * i for i in range(n)]
    return hs, [C.c_void_p(h) if kind == "void_p" or (kind == "mixed" and i % 2) else h for i, h in enumerate(hs)]


def _gain(rng, p, m, kind):
    """((p, m) values, the array handed in): contiguous, a slice of a wider array, or Fortran-ordered."""
    K = rng.standard_normal((p, m))
    if kind == "sliced":
        wide = np.zeros((p, 2 * m))
        wide[:, ::2] = K
        arg = wide[:, ::2]
        assert not arg.flags.c_contiguous or p * m == 1
    elif kind == "fortran":
        arg = np.asfortranarray(K)
    else:
        arg = K
    return K, arg


def _desc_struct(rng, p, m):
    ds = _lib.MpcDesc()
    ds.N, ds.p, ds.m, ds.iters = 2, p, m, 5
    return ds


# ------------------------------------------------------------------------------------- the three plant / MPC multi calls
MS = (3, 4, 3)


def _multi_case(ctx, kind, n, steps, handle_kind="int", gain_kind="plain", uopt_kind=None, rows_given=False,
                want=(True, True, True, True), u_inits_kind=None, outs_kind=None):
    rng = np.random.default_rng(n * 100 + steps)
    d, p = (2, 1) if kind == "plant" else (2, 2)
    ms = list(MS[:n])
    T, Tu = max(steps, 0), max(steps, 1)
    hs, models = _handles(n, handle_kind)
    x0s, x_refs = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    Ks, gains = zip(*[_gain(rng, p, m, gain_kind) for m in ms]) if n else ((), ())
    descs = [_desc_struct(rng, p, m) for m in ms]
    if uopt_kind is None:
        u_opt, n_uopt = None, 0
    elif uopt_kind == "one":
        u_opt, n_uopt = rng.standard_normal(Tu * p), 1
    else:
        u_opt, n_uopt = rng.standard_normal((n, Tu, p) if kind != "plant" else (n, Tu)), n
    rows = [(-1, 0, n_uopt - 1)[i % 3] for i in range(n)] if rows_given else None
    want_x, want_u, want_info, want_sc = want
    plant = _lib.PolyPlant()
    plant.d, plant.p = d, p
    ctx.lib.hint = dict(ms=ms, d=d, p=p)
    kw = dict(u_opt=u_opt, uopt_rows=rows, want_x=want_x, want_u=want_u, want_scores=want_sc)
    ncol, oi, outs, u_inits = 4, None, None, None
    if kind == "plant":
        sc, ox, ou = ctx.plant_loop_multi(2, 0.25, steps, models, list(gains), x0s, x_refs, **kw)
        name = "nk_plant_loop_multi"
    elif kind == "poly":
        sc, ox, ou = ctx.poly_plant_loop_multi(plant, steps, models, list(gains), x0s, x_refs, **kw)
        name = "nk_poly_plant_loop_multi"
    else:
        if u_inits_kind == "some":
            u_inits = [None if i % 2 == 0 else rng.standard_normal(p) for i in range(n)]
        if outs_kind == "some":
            shared = _lib.MpcOut()
            outs = [None if i == min(1, n - 1) else shared for i in range(n)]
        ncol = 8 if outs is None else 10
        sc, ox, ou, oi = ctx.mpc_loop_multi(plant, steps, models, descs, x0s, x_refs, u_inits=u_inits, want_info=want_info,
                                            outs=outs, **kw)
        name = "nk_mpc_loop_multi" if outs is None else "nk_mpc_out_loop_multi"
    call = ctx.lib.last
    assert call["name"] == name and call["ctx"] == CTX_HANDLE and call["n"] == n and call["steps"] == steps
    assert call["table_len"] == max(n, 1) and call["n_uopt"] == n_uopt
    if kind == "plant":
        assert (call["plant_id"], call["Ts"]) == (2, 0.25) and type(call["plant_id"]) is int and type(call["Ts"]) is float
    else:
        assert call["plant"] == C.addressof(plant)
    exp_rows = rows if rows is not None else [0 if n_uopt else -1] * n
    for i, u in enumerate(call["units"]):
        assert u["model"] == hs[i] and u["uopt"] == exp_rows[i] and u["reserved"] == 0
        np.testing.assert_array_equal(u["x0"], x0s[i])
        np.testing.assert_array_equal(u["x_ref"], x_refs[i])
        if kind == "mpc":
            assert u["desc"] == C.addressof(descs[i])
            if u_inits is None or u_inits[i] is None:
                assert u["u_init"] is None
            else:
                np.testing.assert_array_equal(u["u_init"], u_inits[i])
        else:
            np.testing.assert_array_equal(u["K"], Ks[i].reshape(-1))  # row-major values, whatever the layout handed in
    if u_opt is None:
        assert call["uo"] is None
    else:
        np.testing.assert_array_equal(call["uo"], np.asarray(u_opt).reshape(n_uopt, Tu * p))
    if outs is not None:
        assert call["out_len"] == max(n, 1)
        assert call["outs"] == [None if o is None else C.addressof(o) for o in outs]
    nulls = call["nulls"]
    assert (nulls["x"], nulls["u"], nulls["sc"]) == (not want_x, not want_u, not want_sc)
    dd = 1 if (kind == "plant" and n == 0) else d  # nk_plant_loop_multi takes d from x0s: nothing says it without a unit
    for got, on, base, shape in ((ox, want_x, X_BASE, (n, T + 1, dd)), (ou, want_u, U_BASE, (n, T) if kind == "plant" else (n, T, p)),
                                 (sc, want_sc, S_BASE, (n, ncol))):
        if on:
            assert got.shape == shape and got.dtype == np.float64
            np.testing.assert_array_equal(got, _pattern(base, shape))
        else:
            assert got is None
    if kind == "mpc":
        assert nulls["info"] == (not want_info)
        if want_info:
            np.testing.assert_array_equal(oi, _pattern(I_BASE, (n, T, 2)))
        else:
            assert oi is None


@pytest.mark.parametrize("kind", ["plant", "poly", "mpc"])
@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("steps", [0, 5])
def test_multi_calls_pack_units_tables_and_outputs(ctx, kind, n, steps):
    variants = ((None, False), ("one", False), ("n", False), ("n", True), (None, True))
    kinds = (("int", "plain"), ("void_p", "sliced"), ("mixed", "fortran"), ("int", "fortran"), ("void_p", "plain"))
    for (handle_kind, gain_kind), (uopt_kind, rows_given) in zip(kinds, variants):
        _multi_case(ctx, kind, n, steps, handle_kind, gain_kind, uopt_kind, rows_given)


@pytest.mark.parametrize("kind", ["plant", "poly", "mpc"])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_multi_calls_an_output_not_wanted_is_a_null_pointer_and_none(ctx, kind, off):
    want = tuple(i != off for i in range(4))
    for n, steps in itertools.product((0, 3), (0, 5)):
        _multi_case(ctx, kind, n, steps, uopt_kind="one", want=want)


@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("steps", [0, 5])
def test_mpc_multi_seed_controls_and_output_rows(ctx, n, steps):
    for u_inits_kind, outs_kind in ((None, None), ("some", None), (None, "some"), ("some", "some")):
        _multi_case(ctx, "mpc", n, steps, "mixed", uopt_kind="n", rows_given=True, u_inits_kind=u_inits_kind, outs_kind=outs_kind)


def test_multi_calls_wrong_counts_raise(ctx):
    x = np.zeros((2, 2))
    plant = _lib.PolyPlant()
    plant.d, plant.p = 2, 2
    with pytest.raises(ValueError, match="^1 gains for 2 models$"):
        ctx.plant_loop_multi(0, 0.1, 3, [1, 2], [np.zeros(3)], x, x)
    with pytest.raises(ValueError, match="^3 gains for 2 models$"):
        ctx.poly_plant_loop_multi(plant, 3, [1, 2], [np.zeros((2, 3))] * 3, x, x)
    descs = [_lib.MpcDesc(), _lib.MpcDesc()]
    with pytest.raises(ValueError, match="^1 descriptions for 2 models$"):
        ctx.mpc_loop_multi(plant, 3, [1, 2], descs[:1], x, x)
    with pytest.raises(ValueError, match="^3 u_inits for 2 models$"):
        ctx.mpc_loop_multi(plant, 3, [1, 2], descs, x, x, u_inits=[None] * 3)
    with pytest.raises(ValueError, match="^1 output descriptions for 2 models$"):
        ctx.mpc_loop_multi(plant, 3, [1, 2], descs, x, x, outs=[None])
    assert ctx.lib.calls == []


# ------------------------------------------------------------------------------------------------- closed_loop_multi
def test_closed_loop_multi_splits_flat_outputs_per_unit(ctx):
    rng = np.random.default_rng(3)
    dims, T = [(3, 1, 2), (4, 2, 3)], 4
    hs, models = _handles(2, "mixed")
    Ks, gains = zip(*[_gain(rng, p, m, kind) for (m, p, d), kind in zip(dims, ("sliced", "fortran"))])
    phi0s, phi_refs = [rng.standard_normal(m) for m, _, _ in dims], [rng.standard_normal((m, 1)) for m, _, _ in dims]
    targets, u_inits = [rng.standard_normal(d) for _, _, d in dims], [None, rng.standard_normal(2)]
    ctx.lib.hint = dict(dims=dims)
    sc, err, xs, us, cs = ctx.closed_loop_multi(T, 0.5, models, dims, list(gains), phi0s, phi_refs, targets, u_inits, want_x=True,
                                                want_u=True, want_ucum=True)
    call = ctx.lib.last
    assert (call["name"], call["ctx"], call["steps"], call["c"], call["n"]) == ("nk_closed_loop_multi", CTX_HANDLE, T, 0.5, 2)
    for i, u in enumerate(call["units"]):
        assert u["model"] == hs[i]
        np.testing.assert_array_equal(u["K"], Ks[i].reshape(-1))
        np.testing.assert_array_equal(u["phi0"], phi0s[i])
        np.testing.assert_array_equal(u["phi_ref"], phi_refs[i].reshape(-1))
        np.testing.assert_array_equal(u["target"], targets[i])
    assert call["units"][0]["u_init"] is None
    np.testing.assert_array_equal(call["units"][1]["u_init"], u_inits[1])
    assert not any(call["nulls"].values())
    np.testing.assert_array_equal(sc, _pattern(S_BASE, (2, 4)))
    np.testing.assert_array_equal(err, _pattern(E_BASE, (2, T)))
    for got, base, rows, col in ((xs, X_BASE, T, 2), (us, U_BASE, T, 1), (cs, C_BASE, T + 1, 1)):
        off = 0
        for i, dm in enumerate(dims):
            assert got[i].shape == (rows, dm[col])
            np.testing.assert_array_equal(got[i], off + _pattern(base, (rows, dm[col])))
            off += rows * dm[col]
    # nothing wanted but the scores: null pointers, None
    sc, err, xs, us, cs = ctx.closed_loop_multi(T, 0.5, models, dims, list(gains), phi0s, phi_refs, targets, want_err=False)
    assert ctx.lib.last["nulls"] == dict(x=True, u=True, ucum=True, err=True, sc=False)
    assert err is None and xs is None and us is None and cs is None and sc.shape == (2, 4)
    assert all(u["u_init"] is None for u in ctx.lib.last["units"])
    # no targets: nothing scored
    out = ctx.closed_loop_multi(T, 0.5, models, dims, list(gains), phi0s, phi_refs, want_err=False, want_scores=False, want_x=True)
    assert out[0] is None and out[1] is None and all(u["target"] is None for u in ctx.lib.last["units"])
    n_calls = len(ctx.lib.calls)
    with pytest.raises(ValueError, match="^scores and errors need a target per unit$"):
        ctx.closed_loop_multi(T, 0.5, models, dims, list(gains), phi0s, phi_refs, targets=None, want_err=True, want_scores=False)
    with pytest.raises(ValueError, match="^unit 1: phi0 has 3 entries, expected 4$"):
        ctx.closed_loop_multi(T, 0.5, models, dims, list(gains), [phi0s[0], phi0s[0]], phi_refs, targets)
    with pytest.raises(ValueError, match="^unit 0: the gain has 4 entries, expected 3$"):
        ctx.closed_loop_multi(T, 0.5, models, dims, [np.zeros((1, 4)), gains[1]], phi0s, phi_refs, targets)
    with pytest.raises(ValueError, match="^models, dims, gains, phi0s and phi_refs must have the same length$"):
        ctx.closed_loop_multi(T, 0.5, models, dims, list(gains), phi0s[:1], phi_refs, targets)
    assert len(ctx.lib.calls) == n_calls


# ------------------------------------------------------------------------------------- dare_batch / mpc_build_batch
def _problems(rng, kinds=("sliced", "fortran")):
    out = []
    for (m, p), kind in zip(((2, 1), (3, 2)), kinds):
        A, Aa = _gain(rng, m, m, kind)
        B, Ba = _gain(rng, m, p, kind)
        Q, Qa = _gain(rng, m, m, kind)
        R, Ra = _gain(rng, p, p, "plain")
        out.append(dict(m=m, p=p, vals=(A, B, Q, R), args=(Aa, Ba if p > 1 else Ba.reshape(-1), Qa, Ra)))
    return out


def _check_abqr(pr, prob):
    m, p = prob["m"], prob["p"]
    assert (pr["m"], pr["p"], pr["lda"], pr["ldb"], pr["ldq"], pr["ldr"]) == (m, p, m, p, m, p)
    for name, v in zip("ABQR", prob["vals"]):
        np.testing.assert_array_equal(pr[name], v)


@pytest.mark.parametrize("want_P", [True, False])
def test_dare_batch_packs_problems_and_returns_each_output(ctx, want_P):
    probs = _problems(np.random.default_rng(5))
    As, Bs, Qs, Rs = (list(a) for a in zip(*[pr["args"] for pr in probs]))
    Ks, Ps, status, iters, delta = ctx.dare_batch(As, Bs, Qs, Rs, tol=1e-9, max_iter=7, want_P=want_P)
    call = ctx.lib.last
    assert (call["name"], call["ctx"], call["n"], call["tol"], call["max_iter"]) == ("nk_dare_batch", CTX_HANDLE, 2, 1e-9, 7)
    for i, (pr, prob) in enumerate(zip(call["probs"], probs)):
        _check_abqr(pr, prob)
        m, p = prob["m"], prob["p"]
        assert pr["P_null"] == (not want_P)
        np.testing.assert_array_equal(Ks[i], _pattern(100.0 * (i + 1), (p, m)))
        if want_P:
            np.testing.assert_array_equal(Ps[i], _pattern(200.0 * (i + 1), (m, m)))
    assert (Ps is None) == (not want_P)
    np.testing.assert_array_equal(delta, [0.5, 1.5])
    np.testing.assert_array_equal(status, [0, 1])
    np.testing.assert_array_equal(iters, [10, 11])
    assert status.dtype == np.int32 and iters.dtype == np.int32 and status.shape == (2,) and iters.shape == (2,)


def test_dare_batch_empty_and_bad_input(ctx):
    Ks, Ps, status, iters, delta = ctx.dare_batch([], [], [], [])
    assert Ks == [] and Ps == [] and status.shape == iters.shape == delta.shape == (0,) and ctx.lib.last["n"] == 0
    with pytest.raises(ValueError, match=r"^problem 0: A must be square, got \(2, 3\)$"):
        ctx.dare_batch([np.zeros((2, 3))], [np.zeros(2)], [np.eye(2)], [np.eye(1)])
    with pytest.raises(ValueError, match="^As, Bs, Qs, Rs must have the same length$"):
        ctx.dare_batch([np.eye(2)], [], [np.eye(2)], [np.eye(1)])


@pytest.mark.parametrize("want_P", [True, False])
def test_mpc_build_batch_packs_problems_and_returns_each_output(ctx, want_P):
    rng = np.random.default_rng(6)
    probs = _problems(rng)
    As, Bs, Qs, Rs = (list(a) for a in zip(*[pr["args"] for pr in probs]))
    P1, P1a = _gain(rng, 3, 3, "fortran")
    Cr, Cra = _gain(rng, 1, 3, "sliced")
    res = ctx.mpc_build_batch(As, Bs, Qs, Rs, [2, 3], Ps=[None, P1a], C_rows=[None, Cra], Nys=None, tol=1e-9, max_iter=7,
                              newton_steps=2, newton_tol=1e-12, newton_max_iter=9, want_P=want_P)
    call = ctx.lib.last
    assert (call["name"], call["ctx"], call["n"]) == ("nk_mpc_build_batch", CTX_HANDLE, 2)
    assert call["solver"] == (1e-9, 7, 2, 1e-12, 9)
    for i, (pr, prob) in enumerate(zip(call["probs"], probs)):
        _check_abqr(pr, prob)
        m, p = prob["m"], prob["p"]
        N, nc = (2, 3)[i], (0, 1)[i]
        Ny = N if nc else 0  # C_rows without Nys: the rows run over the whole horizon
        assert (pr["N"], pr["nc"], pr["Ny"], pr["ldp"], pr["ldc"]) == (N, nc, Ny, m, m)
        nv, ny, b = N * p, nc * Ny, 1000.0 * (i + 1)
        assert pr["nulls"] == dict(H=False, F=False, K=False, P=not want_P, G=not nc, T=not nc)
        np.testing.assert_array_equal(res["H"][i], _pattern(b + 100, (nv, nv)))
        np.testing.assert_array_equal(res["F"][i], _pattern(b + 200, (nv, m)))
        np.testing.assert_array_equal(res["K"][i], _pattern(b + 300, (p, m)))
        if want_P:
            np.testing.assert_array_equal(res["P"][i], _pattern(b + 400, (m, m)))
        else:
            assert res["P"][i] is None
        if nc:
            np.testing.assert_array_equal(res["G"][i], _pattern(b + 500, (ny, nv)))
            np.testing.assert_array_equal(res["T"][i], _pattern(b + 600, (ny, m)))
        else:
            assert res["G"][i] is None and res["T"][i] is None
    assert call["probs"][0]["P"] is None and call["probs"][0]["C_rows"] is None
    np.testing.assert_array_equal(call["probs"][1]["P"], P1)
    np.testing.assert_array_equal(call["probs"][1]["C_rows"], Cr)
    np.testing.assert_array_equal(res["status"], [0, 1])
    np.testing.assert_array_equal(res["iters"], [[10, 11], [12, 13]])
    assert sorted(res) == ["F", "G", "H", "K", "P", "T", "iters", "status"]
    # horizons of the rows given
    ctx.mpc_build_batch(As, Bs, Qs, Rs, [2, 3], C_rows=[None, Cra], Nys=[1, 2])
    assert [pr["Ny"] for pr in ctx.lib.last["probs"]] == [0, 2] and ctx.lib.last["solver"] == (1e-13, 40, 1, 1e-15, 60)
    with pytest.raises(ValueError, match=r"^problem 1: A must be square, got \(2, 3\)$"):
        ctx.mpc_build_batch([As[0], np.zeros((2, 3))], Bs, Qs, Rs, [2, 3])
    with pytest.raises(ValueError, match="^As, Bs, Qs, Rs, Ns must have the same length$"):
        ctx.mpc_build_batch(As, Bs, Qs, Rs, [2])


# ------------------------------------------------------------------- model_lqr_gain(_batch) / model_mpc_build_batch
def test_model_lqr_gain_batch_splits_the_flat_gains_into_copies(ctx):
    dims = [(3, 1), (4, 2)]
    hs, models = _handles(2, "mixed")
    ctx.lib.hint = dict(dims=dims)
    Ks, status, iters = ctx.model_lqr_gain_batch(models, 0.5, None, tol=1e-9, max_iter=7, dims=dims)
    call = ctx.lib.last
    assert (call["name"], call["ctx"], call["n"], call["c"], call["tol"], call["max_iter"]) == \
        ("nk_model_lqr_gain_batch", CTX_HANDLE, 2, 0.5, 1e-9, 7)
    assert call["models"] == hs and call["R"] is None and call["hs_len"] == 2
    np.testing.assert_array_equal(Ks[0], _pattern(100.0, (1, 3)))
    np.testing.assert_array_equal(Ks[1], _pattern(103.0, (2, 4)))
    assert all(K.flags.owndata or K.base is not None and K.base.flags.owndata and K.base.size == K.size for K in Ks)
    assert not np.shares_memory(Ks[0], Ks[1])
    np.testing.assert_array_equal(status, [0, 1])
    np.testing.assert_array_equal(iters, [10, 11])
    R = np.asfortranarray(np.array([[2.0, 0.5], [0.25, 3.0]]))
    ctx.lib.hint = dict(dims=[(4, 2)])
    Ks, status, iters = ctx.model_lqr_gain_batch([models[1]], 0.5, R, dims=[(4, 2)])
    np.testing.assert_array_equal(ctx.lib.last["R"], R)
    assert (ctx.lib.last["tol"], ctx.lib.last["max_iter"]) == (1e-13, 40) and len(Ks) == 1 and status.shape == (1,)
    ctx.lib.hint = dict(dims=[])
    Ks, status, iters = ctx.model_lqr_gain_batch([], 0.5, dims=[])
    assert Ks == [] and status.shape == (0,) and iters.shape == (0,) and ctx.lib.last["hs_len"] == 1


def test_model_lqr_gain_one_model(ctx):
    ctx.lib.hint = dict(dims=[(4, 2)])
    R = np.array([2.0, 0.5, 0.25, 3.0])
    for model in (0x1230, C.c_void_p(0x1230)):
        K, status, iters = ctx.model_lqr_gain(model, 4, 2, 0.5, R, tol=1e-9, max_iter=7)
        call = ctx.lib.last
        assert (call["ctx"], call["model"], call["c"], call["tol"], call["max_iter"]) == (CTX_HANDLE, 0x1230, 0.5, 1e-9, 7)
        np.testing.assert_array_equal(call["R"], R.reshape(2, 2))
        np.testing.assert_array_equal(K, _pattern(100.0, (2, 4)))
        assert (status, iters) == (1, 17) and type(status) is int and type(iters) is int
    ctx.model_lqr_gain(0x1230, 4, 2, 0.5)
    assert ctx.lib.last["R"] is None


def test_model_mpc_build_batch_specs_and_outputs(ctx):
    dims = [(3, 1), (4, 2)]
    hs, models = _handles(2, "mixed")
    ctx.lib.hint = dict(dims=dims)
    specs = [(2, [], None), (3, np.array([0, 2]), None)]
    units, status, iters = ctx.model_mpc_build_batch(models, dims, 0.5, None, specs, tol=1e-9, max_iter=7, newton_steps=2,
                                                     newton_tol=1e-12, newton_max_iter=9)
    call = ctx.lib.last
    assert (call["name"], call["ctx"], call["n"], call["c"]) == ("nk_model_mpc_build_batch", CTX_HANDLE, 2, 0.5)
    assert call["models"] == hs and call["R"] is None and call["solver"] == (1e-9, 7, 2, 1e-12, 9)
    assert call["specs"] == [(2, 0, [0, 0, 0, 0], 0), (3, 2, [0, 2, 0, 0], 3)]
    assert call["nulls"] == [dict(H=False, F=False, K=False, G=True, T=True), dict(H=False, F=False, K=False, G=False, T=False)]
    for i, ((m, p), (N, nc, _, Ny)) in enumerate(zip(dims, call["specs"])):
        nv, ny, b, u = N * p, nc * Ny, 1000.0 * (i + 1), units[i]
        assert sorted(u) == ["F", "G", "H", "K", "T"]
        np.testing.assert_array_equal(u["H"], _pattern(b + 100, (nv, nv)))
        np.testing.assert_array_equal(u["F"], _pattern(b + 200, (nv, m)))
        np.testing.assert_array_equal(u["K"], _pattern(b + 300, (p, m)))
        if nc:
            np.testing.assert_array_equal(u["G"], _pattern(b + 500, (ny, nv)))
            np.testing.assert_array_equal(u["T"], _pattern(b + 600, (ny, m)))
        else:
            assert u["G"] is None and u["T"] is None
    np.testing.assert_array_equal(status, [0, 1])
    np.testing.assert_array_equal(iters, [[10, 11], [12, 13]])
    R = np.asfortranarray(np.array([[2.0, 0.5], [0.25, 3.0]]))
    ctx.lib.hint = dict(dims=[(4, 2)])
    ctx.model_mpc_build_batch([models[1]], [(4, 2)], 0.5, R, [(3, [1], 2)])
    assert ctx.lib.last["specs"] == [(3, 1, [1, 0, 0, 0], 2)] and ctx.lib.last["solver"] == (1e-13, 40, 1, 1e-15, 60)
    np.testing.assert_array_equal(ctx.lib.last["R"], R)
    n_calls = len(ctx.lib.calls)
    with pytest.raises(ValueError, match="^unit 0: 5 output rows per step, at most 4$"):
        ctx.model_mpc_build_batch([models[1]], [(4, 2)], 0.5, None, [(3, [0, 1, 2, 3, 0], None)])
    assert len(ctx.lib.calls) == n_calls


# ----------------------------------------------------------------------------- the single-call loops of Context itself
NEW_METHODS = ("plant_loop", "poly_plant_loop", "mpc_loop", "closed_loop_batch")


@pytest.mark.skipif(not all(hasattr(_lib.Context, k) for k in NEW_METHODS), reason="Context has no single-call loop methods yet")
def test_context_single_call_loops(ctx):
    rng = np.random.default_rng(8)
    d, p, m, batch, T = 2, 2, 3, 3, 4
    K, xb, xr = rng.standard_normal((p, m)), rng.standard_normal((batch, d)), rng.standard_normal((batch, d))
    plant = _lib.PolyPlant()
    plant.d, plant.p = d, p
    ctx.lib.hint = dict(d=d, p=1, m=m)
    K1 = K[:1].copy()
    ox, ou = ctx.plant_loop(0x50, 1, 0.25, K1, xb, xr, T)
    call = ctx.lib.last
    assert (call["name"], call["ctx"], call["model"], call["plant_id"], call["Ts"], call["steps"], call["batch"]) == \
        ("nk_plant_loop", CTX_HANDLE, 0x50, 1, 0.25, T, batch)
    np.testing.assert_array_equal(call["K"], K1)
    np.testing.assert_array_equal(call["x0"], xb)
    np.testing.assert_array_equal(call["x_ref"], xr)
    np.testing.assert_array_equal(ox, _pattern(X_BASE, (batch, T + 1, d)))
    np.testing.assert_array_equal(ou, _pattern(U_BASE, (batch, T, 1)))
    ctx.lib.hint = dict(d=d, p=p, m=m)
    ox, ou = ctx.poly_plant_loop(C.c_void_p(0x50), plant, K, xb, xr, T)
    call = ctx.lib.last
    assert (call["name"], call["model"], call["plant"], call["batch"]) == ("nk_poly_plant_loop", 0x50, C.addressof(plant), batch)
    np.testing.assert_array_equal(call["K"], K)
    np.testing.assert_array_equal(ou, _pattern(U_BASE, (batch, T, p)))
    ds = _lib.MpcDesc()
    ds.N, ds.p, ds.m, ds.iters = 2, p, m, 5
    ui = rng.standard_normal((batch, p))
    ox, ou, oi = ctx.mpc_loop(0x50, plant, ds, xb, xr, T, u_init=ui, want_info=True)
    call = ctx.lib.last
    assert (call["name"], call["model"], call["plant"], call["steps"]) == ("nk_mpc_loop", 0x50, C.addressof(plant), T)
    np.testing.assert_array_equal(call["u_init"], ui)
    np.testing.assert_array_equal(oi, _pattern(I_BASE, (batch, T, 2)))
    out = _lib.MpcOut()
    ox, ou, oi = ctx.mpc_loop(0x50, plant, ds, xb, xr, T, out=out)
    assert ctx.lib.last["name"] == "nk_mpc_out_loop" and ctx.lib.last["u_init"] is None and oi is None
    assert ctx.lib.last["nulls"]["info"] and ox.shape == (batch, T + 1, d) and ou.shape == (batch, T, p)
    f0, fr = rng.standard_normal((batch, m)), rng.standard_normal((batch, m))
    ox, ou = ctx.closed_loop_batch(0x50, K, f0, fr, T, d)
    call = ctx.lib.last
    assert (call["name"], call["model"], call["steps"], call["batch"]) == ("nk_closed_loop_batch", 0x50, T, batch)
    np.testing.assert_array_equal(call["x0"], f0)
    np.testing.assert_array_equal(call["x_ref"], fr)
    np.testing.assert_array_equal(ox, _pattern(X_BASE, (batch, T, d)))
    np.testing.assert_array_equal(ou, _pattern(U_BASE, (batch, T, p)))


# ------------------------------------------------------------------- closed_loop_plant / closed_loop_plant_mpc / closed_loop
def _poly_plant(d, p):
    return nk.PolynomialSystem(d, p, [(0, 1.0, (1,) + (0,) * (d - 1), (0,) * p)], 0.05)


def _controller(rng, p, m, N=2, rows=False):
    nv = N * p
    c = SimpleNamespace(H=np.eye(nv), F=rng.standard_normal((nv, m)), K=rng.standard_normal((p, m)), lo=np.full(nv, -1.0),
                        hi=np.full(nv, 1.0), dlo=np.full(nv, -np.inf), dhi=np.full(nv, np.inf), rho=1.5, horizon=N)
    if rows:
        c.ny, c.G, c.T = 2, rng.standard_normal((2, nv)), rng.standard_normal((2, m))
        c.ylo, c.yhi, c.ycomp, c.y_weight = np.full(2, -0.5), np.full(2, np.inf), np.array([1, 1]), np.inf
    return c


X0_FORMS = ("vector", "column", "batch")


def _x0_forms(rng, d, batch=3):
    v = rng.standard_normal(d)
    return {"vector": (v, v.reshape(1, d), True), "column": (v.reshape(d, 1), v.reshape(1, d), True),
            "batch": (rng.standard_normal((batch, d)),) * 2 + (False,)}


@pytest.mark.parametrize("poly", [False, True])
def test_closed_loop_plant_single_and_batch(patched, poly):
    rng = np.random.default_rng(11)
    d, m, T = 2, 3, 4
    p = 2 if poly else 1
    plant = _poly_plant(d, p) if poly else nk.DuffingOscillator(Ts=0.05)
    reg = FakeReg(p, d, m, C.c_void_p(0x70))
    Kv, K = _gain(rng, p, m, "fortran" if poly else "sliced")
    patched.lib.hint = dict(d=d, p=p, m=m)
    for form, (x0, xb, single) in _x0_forms(rng, d).items():
        batch = xb.shape[0]
        refs = [rng.standard_normal(d), rng.standard_normal((d, 1))] + ([] if single else [rng.standard_normal((batch, d))])
        for x_ref in refs:
            ox, ou = reg.closed_loop_plant(K, x0, x_ref, T, plant)
            call = patched.lib.last
            assert call["name"] == ("nk_poly_plant_loop" if poly else "nk_plant_loop")
            assert (call["ctx"], call["model"], call["steps"], call["batch"]) == (CTX_HANDLE, 0x70, T, batch)
            if poly:
                assert call["plant"] == C.addressof(plant.descriptor())
            else:
                assert (call["plant_id"], call["Ts"]) == (_lib.NK_PLANT_DUFFING, 0.05)
            np.testing.assert_array_equal(call["K"], Kv)
            np.testing.assert_array_equal(call["x0"], xb)
            np.testing.assert_array_equal(call["x_ref"], np.broadcast_to(np.reshape(x_ref, (-1, d)), (batch, d)))
            X, U = _pattern(X_BASE, (batch, T + 1, d)), _pattern(U_BASE, (batch, T, p))
            if single:
                assert ox.shape == (d, T + 1) and ou.shape == (p, T)
                np.testing.assert_array_equal(ox, X[0].T)
                np.testing.assert_array_equal(ou, U[0].T)
            else:
                np.testing.assert_array_equal(ox, X)
                np.testing.assert_array_equal(ou, U)
    ox, ou = reg.closed_loop_plant(K, np.zeros(d), np.zeros(d), -1, plant)  # (a negative step count reaches the library as it is)
    assert patched.lib.last["steps"] == -1 and ox.shape == (d, 1) and ou.shape == (p, 0)


def test_closed_loop_plant_one_state_model_takes_a_1x1_array_as_single(patched):
    reg = FakeReg(1, 1, 3, 0x70)
    patched.lib.hint = dict(d=1, p=1, m=3)
    K = np.arange(3.0).reshape(1, 3)
    ox, ou = reg.closed_loop_plant(K, np.array([[0.25]]), np.array([[0.5]]), 4, nk.HJB(Ts=0.05))
    assert patched.lib.last["batch"] == 1 and patched.lib.last["plant_id"] == _lib.NK_PLANT_HJB
    assert ox.shape == (1, 5) and ou.shape == (1, 4)
    np.testing.assert_array_equal(ox, _pattern(X_BASE, (1, 5, 1))[0].T)
    ox, ou = reg.closed_loop_plant(K, np.array([[0.25], [0.5]]), np.array([0.5]), 4, nk.HJB(Ts=0.05))
    assert patched.lib.last["batch"] == 2 and ox.shape == (2, 5, 1) and ou.shape == (2, 4, 1)
    c = _controller(np.random.default_rng(0), 1, 3)
    ox, ou = reg.closed_loop_plant_mpc(c, np.array([[0.25]]), np.array([[0.5]]), 4, nk.HJB(Ts=0.05))
    assert patched.lib.last["batch"] == 1 and ox.shape == (1, 5) and ou.shape == (1, 4)


def test_closed_loop_plant_errors_keep_their_text(patched):
    reg = FakeReg(1, 2, 3, 0x70)
    K, x, plant = np.zeros((1, 3)), np.zeros(2), nk.DuffingOscillator(Ts=0.05)
    c = _controller(np.random.default_rng(0), 1, 3)

    def raises(text, fn, *a, **kw):
        with pytest.raises(ValueError) as e:
            fn(*a, **kw)
        assert str(e.value) == text

    raises(PLANT_MSG, reg.closed_loop_plant, K, x, x, 4, SimpleNamespace(plant_id=None, Ts=0.1))
    raises(PLANT_MSG, reg.closed_loop_plant, K, x, x, 4, nk.DuffingOscillator())
    raises(PLANT_MSG, reg.closed_loop_plant_mpc, c, x, x, 4, SimpleNamespace(plant_id=None, Ts=0.1))
    raises(PLANT_MSG, reg.closed_loop_plant_mpc, c, x, x, 4, nk.DuffingOscillator())
    raises(PLANT_MSG, harness.plant_loop_multi, [reg], [K], x, x, 4, SimpleNamespace(plant_id=None, Ts=0.1, n_states=2))
    raises("gain has shape (3,), expected (1, 3)", reg.closed_loop_plant, np.zeros(3), x, x, 4, plant)
    raises("the controller is for a model with K of shape (1, 4), expected (1, 3)", reg.closed_loop_plant_mpc,
           _controller(np.random.default_rng(0), 1, 4), x, x, 4, plant)
    for fn, first in ((reg.closed_loop_plant, K), (reg.closed_loop_plant_mpc, c)):
        raises("initial states have shape (3,), the model has 2 states", fn, first, np.zeros(3), x, 4, plant)
        raises("reference has shape (3,), expected one state of dimension 2 or (1, 2)", fn, first, x, np.zeros(3), 4, plant)
        raises("reference has shape (2, 2), expected one state of dimension 2 or (3, 2)", fn, first, np.zeros((3, 2)),
               np.zeros((2, 2)), 4, plant)
    raises("u_init has shape (2,), expected 1 entries or (3, 1)", reg.closed_loop_plant_mpc, c, np.zeros((3, 2)), x, 4, plant,
           u_init=np.zeros(2))
    assert patched.lib.calls == []


@pytest.mark.parametrize("poly", [False, True])
def test_closed_loop_plant_mpc_single_and_batch(patched, poly):
    rng = np.random.default_rng(12)
    d, m, T = 2, 3, 4
    p = 2 if poly else 1
    plant = _poly_plant(d, p) if poly else nk.DuffingOscillator(Ts=0.05)
    reg = FakeReg(p, d, m, 0x70)
    patched.lib.hint = dict(d=d, p=p, m=m)
    for rows, iters, entry in ((False, 6, "nk_mpc_loop"), (True, 6, "nk_mpc_out_loop"), (True, 0, "nk_mpc_loop")):
        c = _controller(rng, p, m, rows=rows)
        for form, (x0, xb, single) in _x0_forms(rng, d).items():
            batch = xb.shape[0]
            x_ref = rng.standard_normal(d) if form != "batch" else rng.standard_normal((batch, d))
            for k, u_init in enumerate((None, rng.standard_normal(p), rng.standard_normal((batch, p)))):
                for info in ((False, True) if k == 1 else (k == 2,)):
                    res = reg.closed_loop_plant_mpc(c, x0, x_ref, T, plant, iters, 1e-7, u_init, info)
                    call = patched.lib.last
                    assert call["name"] == entry and len(res) == (3 if info else 2)
                    assert (call["ctx"], call["model"], call["steps"], call["batch"]) == (CTX_HANDLE, 0x70, T, batch)
                    if poly:
                        assert call["plant"] == C.addressof(plant.descriptor())
                    ds = call["desc"]
                    assert (ds["N"], ds["p"], ds["m"], ds["iters"], ds["tol"]) == (2, p, m, iters, 1e-7)
                    np.testing.assert_array_equal(ds["K"], c.K)
                    if entry == "nk_mpc_out_loop":
                        assert call["ny"] == 2
                        np.testing.assert_array_equal(call["ycomp"], [1, 1])
                    np.testing.assert_array_equal(call["x0"], xb)
                    np.testing.assert_array_equal(call["x_ref"], np.broadcast_to(x_ref.reshape(-1, d), (batch, d)))
                    if u_init is None:
                        assert call["u_init"] is None
                    else:
                        np.testing.assert_array_equal(call["u_init"], np.broadcast_to(u_init.reshape(-1, p), (batch, p)))
                    assert call["nulls"] == dict(x=False, u=False, info=not info)
                    X, U, I = _pattern(X_BASE, (batch, T + 1, d)), _pattern(U_BASE, (batch, T, p)), _pattern(I_BASE, (batch, T, 2))
                    if single:
                        np.testing.assert_array_equal(res[0], X[0].T)
                        np.testing.assert_array_equal(res[1], U[0].T)
                    else:
                        np.testing.assert_array_equal(res[0], X)
                        np.testing.assert_array_equal(res[1], U)
                    if info:
                        np.testing.assert_array_equal(res[2], I[0] if single else I)


def test_closed_loop_keeps_its_own_single_rule(patched):
    rng = np.random.default_rng(13)
    d, p, m, T = 2, 2, 3, 4
    reg = FakeReg(p, d, m, C.c_void_p(0x70))
    patched.lib.hint = dict(d=d, p=p, m=m)
    Kv, K = _gain(rng, p, m, "fortran")
    f = rng.standard_normal(m)
    for phi0, fb, single in ((f, f.reshape(1, m), True), (f.reshape(m, 1), f.reshape(1, m), True),
                             (rng.standard_normal((2, m)),) * 2 + (False,)):
        phi_ref = rng.standard_normal(phi0.shape) if single else rng.standard_normal(m)
        ox, ou = reg.closed_loop(K, phi0, phi_ref, T)
        call = patched.lib.last
        batch = fb.shape[0]
        assert (call["name"], call["ctx"], call["model"], call["steps"], call["batch"]) == \
            ("nk_closed_loop_batch", CTX_HANDLE, 0x70, T, batch)
        np.testing.assert_array_equal(call["K"], Kv)
        np.testing.assert_array_equal(call["x0"], fb)
        np.testing.assert_array_equal(call["x_ref"], np.broadcast_to(phi_ref.reshape(-1, m), (batch, m)))
        X, U = _pattern(X_BASE, (batch, T, d)), _pattern(U_BASE, (batch, T, p))
        np.testing.assert_array_equal(ox, X[0].T if single else X)
        np.testing.assert_array_equal(ou, U[0].T if single else U)
    with pytest.raises(ValueError, match=r"^gain has shape \(3, 2\), expected \(2, 3\)$"):
        reg.closed_loop(Kv.T, f, f, T)


# ------------------------------------------------------------------------- harness.plant_loop_multi / mpc_loop_multi
@pytest.mark.parametrize("poly", [False, True])
def test_harness_plant_loop_multi_broadcasts_and_defaults(patched, poly):
    rng = np.random.default_rng(14)
    n, d, T = 3, 2, 5
    p = 2 if poly else 1
    plant = _poly_plant(d, p) if poly else nk.DuffingOscillator(Ts=0.05)
    regs = [FakeReg(p, d, m, 0x100 + i) for i, m in enumerate(MS)]
    Ks = [rng.standard_normal((p, m)) for m in MS]
    patched.lib.hint = dict(ms=list(MS), d=d, p=p)
    one, per = rng.standard_normal(d), rng.standard_normal((n, d))
    for x0s, x_refs in ((one, per), (per, one.reshape(d, 1))):
        for u_opt, rows, exp_rows in ((None, None, [-1] * n), (rng.standard_normal((T, p)), None, [0] * n),
                                      (rng.standard_normal((n, T, p)), None, [0, 1, 2]),
                                      (rng.standard_normal((2, T, p)), None, [0] * n),
                                      (rng.standard_normal((n, T, p)), [2, -1, 0], [2, -1, 0])):
            for traj in ((False, True) if rows is None and u_opt is not None and len(u_opt) == n else (u_opt is None,)):
                out = harness.plant_loop_multi(regs, Ks, x0s, x_refs, T, plant, u_opt, traj, rows)
                call = patched.lib.last
                assert call["name"] == ("nk_poly_plant_loop_multi" if poly else "nk_plant_loop_multi") and call["n"] == n
                assert [u["uopt"] for u in call["units"]] == exp_rows
                assert [u["model"] for u in call["units"]] == [0x100, 0x101, 0x102]
                for i, u in enumerate(call["units"]):
                    np.testing.assert_array_equal(u["x0"], np.broadcast_to(np.reshape(x0s, (-1, d)), (n, d))[i])
                    np.testing.assert_array_equal(u["x_ref"], np.broadcast_to(np.reshape(x_refs, (-1, d)), (n, d))[i])
                    np.testing.assert_array_equal(u["K"], Ks[i].reshape(-1))
                if u_opt is None:
                    assert call["uo"] is None
                else:
                    np.testing.assert_array_equal(call["uo"], u_opt.reshape(-1, T * p))
                assert call["nulls"] == dict(x=not traj, u=not traj, sc=False)
                keys = list(harness.SCORE_NAMES) + ["rmse_control"] + (["states", "controls"] if traj else [])
                assert list(out) == keys
                S = _pattern(S_BASE, (n, 4))
                for k, name in enumerate(harness.SCORE_NAMES):
                    np.testing.assert_array_equal(out[name], S[:, k])
                    assert out[name].flags.owndata
                np.testing.assert_array_equal(out["rmse_control"], harness.rmse_control_percent(S[:, 0], S[:, 1]))
                if traj:
                    np.testing.assert_array_equal(out["states"], _pattern(X_BASE, (n, T + 1, d)))
                    np.testing.assert_array_equal(out["controls"], _pattern(U_BASE, (n, T, p) if poly else (n, T)))
    n_calls = len(patched.lib.calls)
    with pytest.raises(ValueError, match=r"^x0s has shape \(3,\), expected one state of dimension 2 or \(3, 2\)$"):
        harness.plant_loop_multi(regs, Ks, np.zeros(3), one, T, plant)
    with pytest.raises(ValueError, match=r"^x_refs has shape \(2, 2\), expected one state of dimension 2 or \(3, 2\)$"):
        harness.plant_loop_multi(regs, Ks, one, np.zeros((2, 2)), T, plant)
    with pytest.raises(ValueError, match="^2 gains for 3 regressors$"):
        harness.plant_loop_multi(regs, Ks[:2], one, one, T, plant)
    with pytest.raises(ValueError, match=r"^gain has shape \(.*\), expected \(.*, 3\)$"):
        harness.plant_loop_multi(regs, [np.zeros((p, 5))] + Ks[1:], one, one, T, plant)
    assert len(patched.lib.calls) == n_calls


def test_harness_mpc_loop_multi_shares_descriptions_and_names_the_scores(patched):
    rng = np.random.default_rng(15)
    n, d, p, T = 3, 2, 1, 5
    plant = nk.DuffingOscillator(Ts=0.05)  # runs as its table
    regs = [FakeReg(p, d, m, 0x100 + i) for i, m in enumerate(MS)]
    c3, c4, c3rows = _controller(rng, p, 3), _controller(rng, p, 4), _controller(rng, p, 3, rows=True)
    patched.lib.hint = dict(ms=list(MS), d=d, p=p)
    one, per = rng.standard_normal(d), rng.standard_normal((n, d))
    # units 0 and 2 share a controller: one description; a per-unit iteration count splits it
    out = harness.mpc_loop_multi(regs, [c3, c4, c3], one, per, T, plant, 7, 1e-6)
    call = patched.lib.last
    assert call["name"] == "nk_mpc_loop_multi" and call["n"] == n
    descs = [u["desc"] for u in call["units"]]
    assert descs[0] == descs[2] != descs[1]
    assert [u["uopt"] for u in call["units"]] == [-1] * n and all(u["u_init"] is None for u in call["units"])
    for i, u in enumerate(call["units"]):
        np.testing.assert_array_equal(u["x0"], one)
        np.testing.assert_array_equal(u["x_ref"], per[i])
    assert list(out) == list(harness.MPC_SCORE_NAMES) + ["rmse_control"]
    S = _pattern(S_BASE, (n, 8))
    for k, name in enumerate(harness.MPC_SCORE_NAMES):
        np.testing.assert_array_equal(out[name], S[:, k])
    np.testing.assert_array_equal(out["rmse_control"], harness.rmse_control_percent(S[:, 0], S[:, 1]))
    harness.mpc_loop_multi(regs, [c3, c4, c3], one, per, T, plant, [7, 7, 8], 1e-6)
    descs = [u["desc"] for u in patched.lib.last["units"]]
    assert len(set(descs)) == 3
    # u_opt rows, seed controls, trajectories and info
    for u_opt, rows, exp_rows in ((rng.standard_normal((T, p)), None, [0] * n), (rng.standard_normal((n, T, p)), None, [0, 1, 2]),
                                  (rng.standard_normal((2, T, p)), None, [0] * n),
                                  (rng.standard_normal((2, T, p)), [1, -1, 0], [1, -1, 0])):
        for u_inits in (None, rng.standard_normal(p), rng.standard_normal((n, p))):
            out = harness.mpc_loop_multi(regs, [c3, c4, c3], per, one, T, plant, 7, 0.0, u_inits, u_opt, rows, True, True)
            call = patched.lib.last
            assert [u["uopt"] for u in call["units"]] == exp_rows
            np.testing.assert_array_equal(call["uo"], u_opt.reshape(-1, T * p))
            for i, u in enumerate(call["units"]):
                np.testing.assert_array_equal(u["x0"], per[i])
                np.testing.assert_array_equal(u["x_ref"], one)
                if u_inits is None:
                    assert u["u_init"] is None
                else:
                    np.testing.assert_array_equal(u["u_init"], np.broadcast_to(u_inits.reshape(-1, p), (n, p))[i])
            assert list(out) == list(harness.MPC_SCORE_NAMES) + ["rmse_control", "states", "controls", "info"]
            np.testing.assert_array_equal(out["states"], _pattern(X_BASE, (n, T + 1, d)))
            np.testing.assert_array_equal(out["controls"], _pattern(U_BASE, (n, T, p)))
            np.testing.assert_array_equal(out["info"], _pattern(I_BASE, (n, T, 2)))
    # a controller with rows: the other entry point, ten columns, a null pointer for the units without rows
    out = harness.mpc_loop_multi(regs, [c3rows, c4, c3rows], one, one, T, plant, 7)
    call = patched.lib.last
    assert call["name"] == "nk_mpc_out_loop_multi"
    assert call["outs"][1] is None and call["outs"][0] is not None and call["outs"][0] == call["outs"][2]
    assert list(out) == list(harness.MPC_OUT_SCORE_NAMES) + ["rmse_control"]
    np.testing.assert_array_equal(out["n_y_viol"], _pattern(S_BASE, (n, 10))[:, 9])
    harness.mpc_loop_multi(regs, [c3rows, c4, c3rows], one, one, T, plant, 0)  # the saturated LQR runs without rows
    assert patched.lib.last["name"] == "nk_mpc_loop_multi"
    n_calls = len(patched.lib.calls)
    with pytest.raises(ValueError, match="^2 controllers for 3 regressors$"):
        harness.mpc_loop_multi(regs, [c3, c4], one, one, T, plant)
    with pytest.raises(ValueError, match="^iters has 2 entries for 3 units$"):
        harness.mpc_loop_multi(regs, [c3, c4, c3], one, one, T, plant, [1, 2])
    with pytest.raises(ValueError, match=r"^u_inits has shape \(2,\), expected 1 entries or \(3, 1\)$"):
        harness.mpc_loop_multi(regs, [c3, c4, c3], one, one, T, plant, u_inits=np.zeros(2))
    with pytest.raises(ValueError, match=r"^the controller is for a model with K of shape \(1, 4\), expected \(1, 3\)$"):
        harness.mpc_loop_multi(regs, [c4, c4, c3], one, one, T, plant)
    assert len(patched.lib.calls) == n_calls


def test_the_two_per_unit_rules_differ_where_their_docstrings_say():
    """_broadcast_states (plant loops, one d) counts; _per_unit (closed_loop_multi, d per unit) goes by the shape."""
    flat = np.arange(6.0)  # n d numbers in a flat array: rows per unit for one, ONE state for the other
    np.testing.assert_array_equal(harness._broadcast_states(flat, 3, 2, "x0s"), flat.reshape(3, 2))
    got = harness._per_unit(flat, 3, "x0s")
    assert len(got) == 3 and all(np.array_equal(v, flat) for v in got)
    pair = [1.0, 2.0]  # n = d numbers in a sequence: one state for both units, or a one-entry state each
    np.testing.assert_array_equal(harness._broadcast_states(pair, 2, 2, "x0s"), [[1.0, 2.0], [1.0, 2.0]])
    got = harness._per_unit(pair, 2, "x0s")
    assert [v.tolist() for v in got] == [[1.0], [2.0]]
    # where the tests and tools call them they agree: one vector for all units, or an (n, d) array
    for x in (np.array([0.5, -1.0]), np.arange(6.0).reshape(3, 2)):
        np.testing.assert_array_equal(np.stack(harness._per_unit(x, 3, "x0s")), harness._broadcast_states(x, 3, 2, "x0s"))
    with pytest.raises(ValueError, match="^x0s: 2 entries for 3 units$"):
        harness._per_unit([np.zeros(2), np.zeros(2)], 3, "x0s")
