"""The reference's three plants (dynamical_systems.py: Duffing oscillator, double integrator, the HJB tutorial system of
Guo et al. 2022), each one Runge-Kutta step of length `Ts` per call.  Same constructor (keyword arguments become
attributes; `Ts` is the one the arithmetic needs) and the same `update_SOM(x, u)` as the reference, including its quirk
that k4 is evaluated at x + k1 Ts instead of x + k3 Ts, so trajectories recorded from the reference are reproduced.

The arithmetic is restated operation by operation, in the reference's order, with the cube of the HJB system written
as a product: it is then, bit for bit, the arithmetic of the library's own plants (csrc/nk_plant.h: `nk_plant_step` on
the host, the single-launch closed loop `nk_plant_loop` on the device), which `plant_id` selects."""
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
