"""nys_koop_lqr_amd -- MI355X (gfx950) drop-in for the Nystrom-Koopman (and thin-plate-spline) fit / lift / predict /
rollout surface of LCSL/nys-koop-lqr's regressors.py.  Python host classes call hand-written HIP kernels through the C-ABI of
libnyskoop.so (include/nyskoop.h) with ctypes.  There is no CPU fallback: importing works anywhere, but any
compute call without the built library and a gfx950 device raises.
"""
from .kernels import KernelWrapper, LinearKernelWrapper, ThreeDimensionalKernel  # noqa: F401
from .regressors import (KoopmanKernelRegressor, KoopmanNystromRegressor, KoopmanRegressor,  # noqa: F401
                         KoopmanSplineRegressor, linear_rollout)
from .dynamical_systems import DoubleIntegrator, DuffingOscillator, HJB, PolynomialSystem  # noqa: F401
from .landmarks import select_landmarks  # noqa: F401
from ._lib import NyskoopError, get_context, library_path, shutdown  # noqa: F401

__all__ = [
    "KoopmanRegressor", "KoopmanNystromRegressor", "KoopmanKernelRegressor", "KoopmanSplineRegressor",
    "ThreeDimensionalKernel", "KernelWrapper", "LinearKernelWrapper", "NyskoopError", "get_context", "library_path", "linear_rollout", "select_landmarks", "shutdown",
    "DuffingOscillator", "DoubleIntegrator", "HJB", "PolynomialSystem",
]
