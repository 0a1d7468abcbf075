"""The reference's three plants (dynamical_systems.py: Duffing oscillator, double integrator, the HJB tutorial system of
Guo et al. 2022), each one Runge-Kutta step of length `Ts` per call.  Same constructor (keyword arguments become
attributes; `Ts` is the one the arithmetic needs) and the same `update_SOM(x, u)` as the reference, including its quirk
that k4 is evaluated at x + k1 Ts instead of x + k3 Ts, so trajectories recorded from the reference are reproduced.

The arithmetic is restated operation by operation, in the reference's order, with the cube of the HJB system written
as a product: it is then, bit for bit, the arithmetic of the library's own plants (csrc/nk_plant.h: `nk_plant_step` on
the host, the single-launch closed loop `nk_plant_loop` on the device), which `plant_id` selects.

`PolynomialSystem` is a plant the user describes as a table of monomials, with up to four states and four inputs; the
library runs the same single-launch loops around it (csrc/nk_poly_plant.h: `nk_poly_plant_step`, `nk_poly_plant_loop`)."""
import numpy as np

from . import _lib


class DynamicalSystem:
    """A plant with one input.  Subclasses give `plant_id`, `n_states` and the right-hand side `_f_u(x, u)` for states
    x (n_states, n) and an input u that broadcasts against a row of x."""

    plant_id = None
    n_states = None

    def __init__(self, **kwargs):
        for key in kwargs:
            setattr(self, key, kwargs[key])

    def _f_u(self, x, u):
        raise NotImplementedError

    def _f_ud(self, x, u):
        k1 = self._f_u(x, u)
        k2 = self._f_u(x + k1 * self.Ts / 2, u)
        k3 = self._f_u(x + k2 * self.Ts / 2, u)
        k4 = self._f_u(x + k1 * self.Ts, u)  # the reference's k4: from k1, not from k3
        return x + (self.Ts / 6) * (k1 + 2 * k2 + 2 * k3 + k4)

    def update_SOM(self, xbef, u):
        xbef = np.asarray(xbef, dtype=np.float64)
        if xbef.ndim == 1:
            xbef = xbef.reshape([-1, 1])
        return self._f_ud(xbef, np.asarray(u, dtype=np.float64))

    def step_library(self, x, u):
        """One step through the library's host build of the same map (nk_plant_step): x (n_states,), u scalar."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.n_states))
        uu = np.array([float(np.asarray(u, dtype=np.float64).reshape(-1)[0])])
        out = np.empty(self.n_states)
        _lib.check(_lib.load_library().nk_plant_step(int(self.plant_id), float(self.Ts), x.ctypes.data, uu.ctypes.data,
                                                     out.ctypes.data))
        return out


def _row(u):
    """The input as a row that stacks under a row of states."""
    return np.asarray(u, dtype=np.float64).reshape(1, -1)


class DuffingOscillator(DynamicalSystem):
    """x1' = x2, x2' = -0.5 x2 - x1 (4 x1^2 - 1) + 0.5 u."""

    plant_id = _lib.NK_PLANT_DUFFING
    n_states = 2

    def _f_u(self, x, u):
        x1, x2 = x[0:1, :], x[1:2, :]
        return -np.vstack((-x2, 0.5 * x2 + x1 * (4 * (x1 * x1) - 1) - 0.5 * _row(u)))


class DoubleIntegrator(DynamicalSystem):
    """x1' = x2, x2' = u."""

    plant_id = _lib.NK_PLANT_DOUBLE_INTEGRATOR
    n_states = 2

    def _f_u(self, x, u):
        x2 = x[1:2, :]
        return np.vstack((x2, np.broadcast_to(_row(u), x2.shape)))


class HJB(DynamicalSystem):
    """x' = -x^3 + u."""

    plant_id = _lib.NK_PLANT_HJB
    n_states = 1

    def _f_u(self, x, u):
        return -((x * x) * x) + u


class PolynomialSystem:
    """A plant the user describes: a polynomial vector field with up to four states and four inputs as a table of
    monomials, one Runge-Kutta step of length `Ts` per call (nk_poly_plant of include/nyskoop.h; csrc/nk_poly_plant.h).

    terms: a list of (row, coef, state_exponents, input_exponents):
        f_row(x, u) = sum over the row's terms of coef * prod_k x_k^ex[k] * prod_j u_j^eu[j]
    (exponent tuples may be shorter than n_states / n_inputs: missing entries are 0; a scalar stands for a 1-tuple).
    rk4="classic": k4 = f(x + k3 Ts); rk4="reference": k4 = f(x + k1 Ts), the variant of the three plants above, which
    the constructors duffing / double_integrator / hjb restate as tables.

    The order of operations is the library's (term: v = coef, times x_k ex[k] times for k = 0.., then times u_j eu[j] times;
    row: f = 0.0, then f = f + v in table order; step: y = x + k Ts / 2, h6 = Ts / 6, x + h6 (((k1 + 2 k2) + 2 k3) + k4)):
    `update_SOM` (Python / NumPy scalars), `step_library` (nk_poly_plant_step, the host build) and the single-launch closed
    loops on the device (nk_poly_plant_loop) give the same bits.  The table is validated by the library (ValueError)."""

    plant_id = None  # not one of the library's built-in plants

    def __init__(self, n_states, n_inputs, terms, Ts, rk4="classic"):
        if rk4 not in ("classic", "reference"):
            raise ValueError(f"rk4 must be 'classic' or 'reference', got {rk4!r}")
        self.n_states, self.n_inputs, self.Ts, self.rk4 = int(n_states), int(n_inputs), float(Ts), rk4

        def exps(e, n, what, i):
            e = tuple(int(v) for v in (e if np.ndim(e) else (e,)))
            if len(e) > 4 or any(v < 0 or v > 255 for v in e):
                raise ValueError(f"term {i}: {what} exponents {e} must be at most four numbers in 0 .. 255")
            return e + (0,) * (4 - len(e))

        self.terms = []
        for i, (row, coef, ex, eu) in enumerate(terms):
            self.terms.append((int(row), float(coef), exps(ex, self.n_states, "state", i), exps(eu, self.n_inputs, "input", i)))
        if len(self.terms) > 32:
            raise ValueError(f"n_terms = {len(self.terms)} must lie in 1 .. 32")
        self._desc = None
        # the library's validation (a host function; needs no GPU)
        x, u = np.zeros(4), np.zeros(4)
        _lib.check_mapped(_lib.load_library().nk_poly_plant_step(self.descriptor(), x.ctypes.data, u.ctypes.data,
                                                                 x.ctypes.data))

    # ---- the ctypes descriptor: built on demand and left out of a pickle, rebuilt from the terms afterwards
    def descriptor(self):
        """The nk_poly_plant of this system (a _lib.PolyPlant; pass it with ctypes.byref)."""
        if self._desc is None:
            ds = _lib.PolyPlant()
            ds.d, ds.p, ds.n_terms, ds.k4_at_k1, ds.Ts = self.n_states, self.n_inputs, len(self.terms), int(self.rk4 == "reference"), self.Ts
            for i, (row, coef, ex, eu) in enumerate(self.terms):
                t = ds.terms[i]
                t.row, t.coef = row, coef
                for k in range(4):
                    t.ex[k], t.eu[k] = ex[k], eu[k]
            self._desc = ds
        return self._desc

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_desc"] = None
        return state

    # ---- the arithmetic, on Python floats (one state) or NumPy rows (states in the columns): the same IEEE operations
    def _f(self, x, u):
        f = [0.0] * self.n_states
        for row, coef, ex, eu in self.terms:
            v = coef
            for k in range(self.n_states):
                for _ in range(ex[k]):
                    v = v * x[k]
            for j in range(self.n_inputs):
                for _ in range(eu[j]):
                    v = v * u[j]
            f[row] = f[row] + v
        return f

    def _step(self, x, u):
        Ts, d = self.Ts, self.n_states
        k1 = self._f(x, u)
        k2 = self._f([x[i] + k1[i] * Ts / 2.0 for i in range(d)], u)
        k3 = self._f([x[i] + k2[i] * Ts / 2.0 for i in range(d)], u)
        kq = k1 if self.rk4 == "reference" else k3
        k4 = self._f([x[i] + kq[i] * Ts for i in range(d)], u)
        h6 = Ts / 6.0
        return [x[i] + h6 * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]) for i in range(d)]

    def update_SOM(self, xbef, u):
        """x (n_states,) / (n_states, n) and u (n_inputs,) / (n_inputs, n) (a scalar or a row with one input; one input
        column broadcasts over the states) -> the next states (n_states, n)."""
        d, p = self.n_states, self.n_inputs
        x = np.asarray(xbef, dtype=np.float64)
        x = x.reshape(d, -1)
        u = np.asarray(u, dtype=np.float64)
        u = u.reshape(p, -1)
        n = max(x.shape[1], u.shape[1])
        if n == 1:
            out = self._step([float(v) for v in x[:, 0]], [float(v) for v in u[:, 0]])
            return np.array(out, dtype=np.float64).reshape(d, 1)
        x, u = np.broadcast_to(x, (d, n)), np.broadcast_to(u, (p, n))
        out = self._step([x[k] for k in range(d)], [u[j] for j in range(p)])
        return np.vstack([np.broadcast_to(np.asarray(r, dtype=np.float64), (n,)) for r in out])

    def step_library(self, x, u):
        """One step through the library's host build of the same map (nk_poly_plant_step): x (n_states,), u (n_inputs,)."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.n_states))
        uu = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(self.n_inputs))
        out = np.empty(self.n_states)
        _lib.check_mapped(_lib.load_library().nk_poly_plant_step(self.descriptor(), x.ctypes.data, uu.ctypes.data,
                                                                 out.ctypes.data))
        return out

    # ---- the reference's three plants as tables, and Van der Pol
    @classmethod
    def duffing(cls, Ts):
        """x1' = x2, x2' = -0.5 x2 - 4 x1^3 + x1 + 0.5 u (DuffingOscillator with its products multiplied out)."""
        return cls(2, 1, [(0, 1.0, (0, 1), (0,)), (1, -0.5, (0, 1), (0,)), (1, -4.0, (3, 0), (0,)), (1, 1.0, (1, 0), (0,)),
                          (1, 0.5, (0, 0), (1,))], Ts, rk4="reference")

    @classmethod
    def double_integrator(cls, Ts):
        """x1' = x2, x2' = u."""
        return cls(2, 1, [(0, 1.0, (0, 1), (0,)), (1, 1.0, (0, 0), (1,))], Ts, rk4="reference")

    @classmethod
    def hjb(cls, Ts):
        """x' = -x^3 + u."""
        return cls(1, 1, [(0, -1.0, (3,), (0,)), (0, 1.0, (0,), (1,))], Ts, rk4="reference")

    @classmethod
    def van_der_pol(cls, mu, Ts):
        """x1' = x2, x2' = mu (1 - x1^2) x2 - x1 + u, classical RK4."""
        mu = float(mu)
        return cls(2, 1, [(0, 1.0, (0, 1), (0,)), (1, mu, (0, 1), (0,)), (1, -mu, (2, 1), (0,)), (1, -1.0, (1, 0), (0,)),
                          (1, 1.0, (0, 0), (1,))], Ts)
