"""ctypes binding of libnyskoop.so (include/nyskoop.h).  Fails loudly: no library or no GPU => exception."""
import atexit
import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

NK_KERNEL_RBF, NK_KERNEL_MATERN52, NK_KERNEL_LINEAR, NK_KERNEL_TPS = 0, 1, 2, 3
NK_PLANT_DUFFING, NK_PLANT_DOUBLE_INTEGRATOR, NK_PLANT_HJB = 0, 1, 2
NK_LANDMARK_GREEDY, NK_LANDMARK_RPCHOLESKY = 0, 1
NK_OK = 0
_ERR_NAMES = {-1: "NK_ERR_BAD_ARG", -2: "NK_ERR_HIP", -3: "NK_ERR_NOT_SPD", -4: "NK_ERR_OOM",
              -5: "NK_ERR_NO_CONVERGENCE", -6: "NK_ERR_NO_DEVICE"}


class NyskoopError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class KernelDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("d", C.c_int32), ("n_lengthscale", C.c_int32), ("reserved", C.c_int32),
                ("lengthscale", C.POINTER(C.c_double)), ("sigma0", C.c_double)]


class CvUnit(C.Structure):
    _fields_ = [("kernel", C.POINTER(KernelDesc)), ("gamma", C.c_double), ("jitter", C.c_double), ("m", C.c_int32),
                ("reserved", C.c_int32), ("test_begin", C.c_int64), ("test_end", C.c_int64),
                ("landmark_rows", C.POINTER(C.c_int64))]


class SplineCvUnit(C.Structure):
    _fields_ = [("gamma", C.c_double), ("m", C.c_int32), ("reserved", C.c_int32), ("test_begin", C.c_int64),
                ("test_end", C.c_int64), ("centers", C.POINTER(C.c_double))]


class SysidUnit(C.Structure):
    _fields_ = [("kernel", C.POINTER(KernelDesc)), ("gamma", C.c_double), ("jitter", C.c_double), ("m", C.c_int32),
                ("n_ranges", C.c_int32), ("row_ranges", C.POINTER(C.c_int64)), ("landmark_rows", C.POINTER(C.c_int64)),
                ("centers", C.POINTER(C.c_double)), ("traj", C.POINTER(C.c_int32)), ("n_traj", C.c_int32),
                ("reserved", C.c_int32)]


class PlantUnit(C.Structure):
    """nk_plant_unit (include/nyskoop.h), one unit of nk_plant_loop_multi: four pointers (model, K, x0, x_ref) and two
    int32 (uopt, reserved): 40 bytes, no padding."""
    _fields_ = [("model", C.c_void_p), ("K", C.c_void_p), ("x0", C.c_void_p), ("x_ref", C.c_void_p),
                ("uopt", C.c_int32), ("reserved", C.c_int32)]


class PolyTerm(C.Structure):
    """nk_poly_term (include/nyskoop.h): one monomial of a polynomial plant, 24 bytes."""
    _fields_ = [("row", C.c_int32), ("ex", C.c_uint8 * 4), ("eu", C.c_uint8 * 4), ("coef", C.c_double)]


class PolyPlant(C.Structure):
    """nk_poly_plant (include/nyskoop.h): the table of a polynomial plant."""
    _fields_ = [("d", C.c_int32), ("p", C.c_int32), ("n_terms", C.c_int32), ("k4_at_k1", C.c_int32), ("Ts", C.c_double),
                ("terms", PolyTerm * 32)]


class MpcDesc(C.Structure):
    """nk_mpc_desc (include/nyskoop.h): the condensed QP of the constrained MPC loop.  The arrays are host memory the
    caller keeps alive for the call."""
    _fields_ = [("N", C.c_int32), ("p", C.c_int32), ("m", C.c_int32), ("iters", C.c_int32), ("H", C.c_void_p),
                ("F", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p), ("dlo", C.c_void_p), ("dhi", C.c_void_p),
                ("K", C.c_void_p), ("rho", C.c_double), ("tol", C.c_double)]


def mpc_desc(controller, iters, tol):
    """(MpcDesc, keep-alive list) of an lqr.MPCController: infinite bounds travel as NULL only when a whole vector is
    infinite."""
    ds, keep = MpcDesc(), []

    def ptr(a, skip=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if skip is not None and np.all(a == skip):
            return None
        keep.append(a)
        return a.ctypes.data

    p, m = controller.K.shape
    ds.N, ds.p, ds.m, ds.iters = int(controller.horizon), p, m, int(iters)
    ds.H, ds.F, ds.K = ptr(controller.H), ptr(controller.F), ptr(controller.K)
    ds.lo, ds.hi = ptr(controller.lo, -np.inf), ptr(controller.hi, np.inf)
    ds.dlo, ds.dhi = ptr(controller.dlo, -np.inf), ptr(controller.dhi, np.inf)
    ds.rho, ds.tol = float(controller.rho), float(tol)
    return ds, keep


class MpcOut(C.Structure):
    """nk_mpc_out (include/nyskoop.h): the output rows of nk_mpc_out_loop beside an MpcDesc.  Host arrays the caller keeps
    alive for the call."""
    _fields_ = [("ny", C.c_int32), ("reserved", C.c_int32), ("G", C.c_void_p), ("T", C.c_void_p), ("ylo", C.c_void_p),
                ("yhi", C.c_void_p), ("ycomp", C.c_void_p), ("y_weight", C.c_double)]


def mpc_out(controller):
    """(MpcOut, keep-alive list) of an lqr.MPCOutputController: infinite bounds travel as NULL only when a whole vector is
    infinite."""
    out = MpcOut()
    G, T = (np.ascontiguousarray(a, dtype=np.float64) for a in (controller.G, controller.T))
    ylo, yhi = (np.ascontiguousarray(a, dtype=np.float64) for a in (controller.ylo, controller.yhi))
    yc = np.ascontiguousarray(controller.ycomp, dtype=np.int32)
    out.ny, out.reserved, out.G, out.T, out.ycomp = int(controller.ny), 0, G.ctypes.data, T.ctypes.data, yc.ctypes.data
    out.ylo = None if np.all(ylo == -np.inf) else ylo.ctypes.data
    out.yhi = None if np.all(yhi == np.inf) else yhi.ctypes.data
    out.y_weight = float(controller.y_weight)
    return out, [G, T, ylo, yhi, yc]


class MpcUnit(C.Structure):
    """nk_mpc_unit (include/nyskoop.h), one unit of nk_mpc_loop_multi: five pointers (model, desc, x0, x_ref, u_init) and
    two int32 (uopt, reserved): 48 bytes, no padding."""
    _fields_ = [("model", C.c_void_p), ("desc", C.POINTER(MpcDesc)), ("x0", C.c_void_p), ("x_ref", C.c_void_p),
                ("u_init", C.c_void_p), ("uopt", C.c_int32), ("reserved", C.c_int32)]


MPC_N_SCORES = 8  # NK_MPC_N_SCORES
MPC_OUT_N_SCORES = 10  # NK_MPC_OUT_N_SCORES


class LoopUnit(C.Structure):
    """nk_loop_unit (include/nyskoop.h), one unit of nk_closed_loop_multi: six pointers (model, K, phi0, phi_ref, target,
    u_init): 48 bytes, no padding."""
    _fields_ = [("model", C.c_void_p), ("K", C.c_void_p), ("phi0", C.c_void_p), ("phi_ref", C.c_void_p),
                ("target", C.c_void_p), ("u_init", C.c_void_p)]


class DareProblem(C.Structure):
    """nk_dare_problem (include/nyskoop.h), one problem of nk_dare_batch."""
    _fields_ = [("m", C.c_int32), ("p", C.c_int32), ("A", C.c_void_p), ("lda", C.c_int64), ("B", C.c_void_p),
                ("ldb", C.c_int64), ("Q", C.c_void_p), ("ldq", C.c_int64), ("R", C.c_void_p), ("ldr", C.c_int64),
                ("out_K", C.c_void_p), ("out_P", C.c_void_p), ("out_delta", C.c_void_p)]


class MpcBuildProblem(C.Structure):
    """nk_mpc_build_problem (include/nyskoop.h), one problem of nk_mpc_build_batch."""
    _fields_ = [("m", C.c_int32), ("p", C.c_int32), ("N", C.c_int32), ("nc", C.c_int32), ("Ny", C.c_int32),
                ("reserved", C.c_int32), ("A", C.c_void_p), ("lda", C.c_int64), ("B", C.c_void_p), ("ldb", C.c_int64),
                ("Q", C.c_void_p), ("ldq", C.c_int64), ("R", C.c_void_p), ("ldr", C.c_int64), ("P", C.c_void_p),
                ("ldp", C.c_int64), ("C_rows", C.c_void_p), ("ldc", C.c_int64), ("out_H", C.c_void_p),
                ("out_F", C.c_void_p), ("out_K", C.c_void_p), ("out_P", C.c_void_p), ("out_G", C.c_void_p),
                ("out_T", C.c_void_p)]


class MpcBuildSpec(C.Structure):
    """nk_mpc_build_spec (include/nyskoop.h): the horizon and the output rows of one unit of nk_model_mpc_build_batch."""
    _fields_ = [("N", C.c_int32), ("nc", C.c_int32), ("comps", C.c_int32 * 4), ("Ny", C.c_int32), ("reserved", C.c_int32)]


class MpcBuildOut(C.Structure):
    """nk_mpc_build_out (include/nyskoop.h): where the results of one unit of nk_model_mpc_build_batch go."""
    _fields_ = [("H", C.c_void_p), ("F", C.c_void_p), ("K", C.c_void_p), ("G", C.c_void_p), ("T", C.c_void_p)]


class FitStats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_upload", C.c_double), ("ms_kmat", C.c_double),
                ("ms_gram", C.c_double), ("ms_sqrt", C.c_double), ("ms_solve", C.c_double),
                ("ms_gram_kernel_avg", C.c_double), ("gram_kernel_launches", C.c_int32),
                ("sqrt_iters", C.c_int32), ("sqrt_residual", C.c_double), ("gram_flops", C.c_double),
                ("kmat_pairs", C.c_double), ("rank_inner", C.c_int32), ("rank_inner_rec", C.c_int32),
                ("pivot_ratio_inner", C.c_double), ("pivot_ratio_inner_rec", C.c_double), ("refined", C.c_int32),
                ("reserved_", C.c_int32), ("refine_ratio_inner", C.c_double), ("refine_ratio_inner_rec", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_P = C.c_void_p
_I64 = C.c_int64
_I32 = C.c_int32
_D = C.c_double

# name -> (restype, argtypes); every symbol declared in include/nyskoop.h
SIGNATURES = {
    "nk_version": (C.c_int, []),
    "nk_last_error": (C.c_char_p, []),
    "nk_device_count": (C.c_int, []),
    "nk_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "nk_destroy": (C.c_int, [_P]),
    "nk_synchronize": (C.c_int, [_P]),
    "nk_stream": (_P, [_P]),
    "nk_set_kmat_mode": (C.c_int, [_P, C.c_int]),
    "nk_set_strict_spd": (C.c_int, [_P, C.c_int]),
    "nk_set_refine": (C.c_int, [_P, C.c_double, C.c_int32]),
    "nk_wait_stream": (C.c_int, [_P, _P]),
    "nk_shutdown": (C.c_int, []),
    "nk_group_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "nk_group_enter": (C.c_int, [_P]),
    "nk_group_leave": (C.c_int, [_P]),
    "nk_set_compute_dtype": (C.c_int, [_P, C.c_int]),
    "nk_group_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "nk_runtime_counters": (C.c_int, [C.POINTER(C.c_uint64), C.c_int32]),
    "nk_cv_grid": (C.c_int, [C.POINTER(_P), _I32, _P, _I64, _P, _I64, _I64, _I32, _I32, C.POINTER(CvUnit), _I32,
                             C.POINTER(_D), C.POINTER(_I32)]),
    "nk_spline_cv_grid": (C.c_int, [C.POINTER(_P), _I32, _P, _I64, _P, _I64, _I64, _I32, _I32, C.POINTER(SplineCvUnit),
                                    _I32, C.POINTER(_D), C.POINTER(_I32)]),
    "nk_sysid_grid": (C.c_int, [C.POINTER(_P), _I32, _P, _I64, _P, _I64, _I64, _I32, _I32, _P, _P, _I32, _I32,
                                C.POINTER(SysidUnit), _I32, C.POINTER(_D), C.POINTER(_D), C.POINTER(_I32)]),
    "nk_host_alloc": (_P, [C.c_uint64]),
    "nk_host_free": (None, [_P]),
    "nk_kernel_matrix": (C.c_int, [_P, C.POINTER(KernelDesc), _P, _I64, _I64, _P, _I64, _I64, _P, _I64]),
    "nk_select_landmarks": (C.c_int, [_P, C.POINTER(KernelDesc), _P, _I64, _I64, _I32, C.POINTER(_I64), _I32, _I32, _P,
                                      _I32, _D, _P, _P, _P, C.POINTER(_I32)]),
    "nk_nystrom_fit": (C.c_int, [_P, C.POINTER(KernelDesc), _P, _I64, _P, _I64, _I64, _I32, _I32,
                                 C.POINTER(_I64), _I32, _P, _I64, _P, _I64, _I32, _D, _D,
                                 C.POINTER(_P), C.POINTER(FitStats)]),
    "nk_gram_doubles": (C.c_int, [_I32, _I32, _I32, C.POINTER(_I64)]),
    "nk_nystrom_gram": (C.c_int, [_P, C.POINTER(KernelDesc), _P, _I64, _P, _I64, _I64, _I32, _I32,
                                  C.POINTER(_I64), _I32, _P, _I64, _P, _I64, _I32, _P, C.POINTER(FitStats)]),
    "nk_nystrom_solve": (C.c_int, [_P, C.POINTER(KernelDesc), _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I64, _D, _D,
                                   C.POINTER(_P), C.POINTER(FitStats)]),
    "nk_model_create": (C.c_int, [_P, C.POINTER(KernelDesc), _P, _I64, _I32, _I32, _I32, _D, _P, _P, _P, _P,
                                  C.POINTER(_P)]),
    "nk_spline_fit": (C.c_int, [_P, _P, _I64, _P, _I64, _I64, _I32, _I32, C.POINTER(_I64), _I32, _P, _I64, _I32, _D,
                                C.POINTER(_P), C.POINTER(FitStats)]),
    "nk_spline_model_create": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _P, C.POINTER(_P)]),
    "nk_model_destroy": (C.c_int, [_P]),
    "nk_model_get": (C.c_int, [_P, _P, C.c_char, _P, _I64]),
    "nk_model_dims": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32)]),
    "nk_model_get_ops": (C.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I64]),
    "nk_model_get_ops_async": (C.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I64]),
    "nk_model_wait": (C.c_int, [_P]),
    "nk_lift": (C.c_int, [_P, _P, _P, _I64, _I64, _P, _I64]),
    "nk_predict": (C.c_int, [_P, _P, _P, _I64, _I64, _P, _I64]),
    "nk_score_neg_rmse": (C.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, C.POINTER(_D)]),
    "nk_rollout": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _I32, _P, _P]),
    "nk_rollout_err": (C.c_int, [_P, _P, _P, _P, _I32, _I32, C.POINTER(_D), C.POINTER(_D)]),
    "nk_closed_loop": (C.c_int, [_P, _P, _P, _P, _P, _I32, _P, _P]),
    "nk_closed_loop_batch": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "nk_plant_step": (C.c_int, [C.c_int, _D, _P, _P, _P]),
    "nk_plant_loop": (C.c_int, [_P, _P, C.c_int, _D, _P, _P, _P, _I32, _I32, _P, _P]),
    "nk_plant_loop_multi": (C.c_int, [_P, C.c_int, _D, _I32, C.POINTER(PlantUnit), _I32, _P, _I32, _P, _P, _P]),
    "nk_poly_plant_step": (C.c_int, [C.POINTER(PolyPlant), _P, _P, _P]),
    "nk_poly_plant_loop": (C.c_int, [_P, _P, C.POINTER(PolyPlant), _P, _P, _P, _I32, _I32, _P, _P]),
    "nk_poly_plant_loop_multi": (C.c_int, [_P, C.POINTER(PolyPlant), _I32, C.POINTER(PlantUnit), _I32, _P, _I32, _P, _P,
                                           _P]),
    "nk_mpc_loop": (C.c_int, [_P, _P, C.POINTER(PolyPlant), C.POINTER(MpcDesc), _P, _P, _P, _I32, _I32, _P, _P, _P]),
    "nk_mpc_loop_multi": (C.c_int, [_P, C.POINTER(PolyPlant), _I32, C.POINTER(MpcUnit), _I32, _P, _I32, _P, _P, _P, _P]),
    "nk_mpc_out_loop_multi": (C.c_int, [_P, C.POINTER(PolyPlant), _I32, C.POINTER(MpcUnit), C.POINTER(C.POINTER(MpcOut)), _I32,
                                        _P, _I32, _P, _P, _P, _P]),
    "nk_mpc_qp_host": (C.c_int, [C.POINTER(MpcDesc), _P, _P, _P, _P, _P]),
    "nk_mpc_loop_max_m": (C.c_int, [_I32]),
    "nk_mpc_out_loop": (C.c_int, [_P, _P, C.POINTER(PolyPlant), C.POINTER(MpcDesc), C.POINTER(MpcOut), _P, _P, _P, _I32,
                                  _I32, _P, _P, _P]),
    "nk_mpc_out_qp_host": (C.c_int, [C.POINTER(MpcDesc), C.POINTER(MpcOut), _P, _P, _P, _P, _P, _P]),
    "nk_closed_loop_multi": (C.c_int, [_P, _I32, _D, C.POINTER(LoopUnit), _I32, _P, _P, _P, _P, _P]),
    "nk_dare_batch": (C.c_int, [_P, C.POINTER(DareProblem), _I32, _D, _I32, C.POINTER(_I32), C.POINTER(_I32)]),
    "nk_model_lqr_gain_batch": (C.c_int, [_P, C.POINTER(_P), _I32, _D, _P, _D, _I32, _P, C.POINTER(_I32),
                                          C.POINTER(_I32)]),
    "nk_model_lqr_cost": (C.c_int, [_P, _P, _D, _P, _I64]),
    "nk_dare_large": (C.c_int, [_P, _I32, _I32, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _D, _I32, _P, _P, C.POINTER(_D),
                                C.POINTER(_I32), C.POINTER(_I32)]),
    "nk_model_lqr_gain": (C.c_int, [_P, _P, _D, _P, _D, _I32, _P, C.POINTER(_I32), C.POINTER(_I32)]),
    "nk_dare_large_times": (C.c_int, [C.POINTER(_D)]),
    "nk_mpc_build_batch": (C.c_int, [_P, C.POINTER(MpcBuildProblem), _I32, _D, _I32, _I32, _D, _I32, C.POINTER(_I32),
                                     C.POINTER(_I32)]),
    "nk_model_mpc_build_batch": (C.c_int, [_P, C.POINTER(_P), _I32, _D, _P, C.POINTER(MpcBuildSpec), _D, _I32, _I32, _D,
                                           _I32, C.POINTER(MpcBuildOut), C.POINTER(_I32), C.POINTER(_I32)]),
    "nk_mpc_build_times": (C.c_int, [C.POINTER(_D)]),
    "nk_linear_rollout": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P]),
    "nk_gemm_f32": (C.c_int, [_P, _I64, _I64, _I64, _P, _I64, _P, _I64, _P, _I64]),
    "nk_gemm": (C.c_int, [_P, C.c_int, C.c_int, _I64, _I64, _I64, _D, _P, _I64, _P, _I64, _D, _P, _I64]),
    "nk_sqrtm_spd": (C.c_int, [_P, _P, _I64, _I32, _P, _P, C.POINTER(_I32), C.POINTER(_D)]),
    "nk_solve_spd": (C.c_int, [_P, _P, _I64, _I32, _P, _I64, _I32, _P, _I64]),
    "nk_bench_gram": (C.c_int, [_P, _I64, _I32, _I32, _I32, _I32, C.POINTER(_D), C.POINTER(_D)]),
    "nk_chol_aug": (C.c_int, [_P, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

_lib = None
_lib_lock = threading.Lock()


def library_path():
    return os.environ.get("NYSKOOP_LIB", os.path.join(_HERE, "libnyskoop.so"))


def load_library():
    """dlopen libnyskoop.so and declare every prototype.  Raises if the library has not been built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            path = library_path()
            if not os.path.exists(path):
                raise NyskoopError(-6, f"{path} not found: build it with `python -c 'import __graft_entry__ as g; "
                                       f"g.build()'` or `make -C nys_koop_lqr_amd/csrc` (there is no CPU fallback)")
            # torch wheels bundle their own HIP runtime (same SONAME as /opt/rocm's): if this library pulled in the system
            # runtime first, a later `import torch` in the same process would find no GPUs.  When torch is installed,
            # let it load its runtime first (plumbing only: nothing here calls into torch).
            if os.environ.get("NYSKOOP_PRELOAD_TORCH", "1") == "1" and "torch" not in sys.modules:
                try:
                    import torch  # noqa: F401
                except Exception:
                    pass
            lib = C.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
            # Deterministic teardown: release every stream, event, workspace, model buffer and page-locked block while
            # the HIP runtime (and a profiler's tool library, if one is attached) is still fully alive.  atexit hooks of
            # the interpreter run before Py_Finalize and before the C runtime's exit handlers / static destructors;
            # afterwards the finalisers of Context / regressor / pinned-array objects find their handles already
            # released (nk_destroy, nk_model_destroy and nk_host_free are no-ops for handles the library no longer knows).
            atexit.register(shutdown)
    return _lib


def shutdown():
    """nk_shutdown(): wait for pending work and release everything the library holds.  Idempotent; contexts, device
    models and pinned result arrays that are still referenced become invalid (operators already fetched stay valid only
    if they were copied: `np.array(reg.A)`)."""
    lib = _lib
    if lib is None:
        return
    with _pools_lock:
        pools = list(_pools.values())
        _pools.clear()
        lpools = list(_lockstep_pools.values())
        _lockstep_pools.clear()
    for pool in pools:  # worker threads hold contexts in thread-local storage; stop them before their streams go away
        pool.shutdown(wait=True)
    for pool in lpools:
        pool.close()
    _PinnedBlock.drain()
    lib.nk_shutdown()


def check(rc):
    if rc != NK_OK:
        raise NyskoopError(rc, load_library().nk_last_error().decode("utf-8", "replace"))


def check_mapped(rc):
    """check() for the calls whose failures have Python equivalents: NK_ERR_BAD_ARG raises ValueError and NK_ERR_NOT_SPD
    np.linalg.LinAlgError, as NumPy / SciPy / sklearn would for the same input."""
    if rc == -1:
        raise ValueError(load_library().nk_last_error().decode())
    if rc == -3:
        raise np.linalg.LinAlgError(load_library().nk_last_error().decode())
    check(rc)


def runtime_counters():
    """Process-wide counts of the library's silent slow paths (nk_runtime_counters): single-launch recursions and Jacobi
    sweeps that gave up waiting for non-resident workgroups, fits that took the rank-truncating branch of the
    reference's lstsq (regressors.py:155,165), fits that repeated the matrix square root."""
    v = (C.c_uint64 * 5)()
    check(load_library().nk_runtime_counters(v, 5))
    return dict(chain_giveups=int(v[0]), jacobi_giveups=int(v[1]), rank_truncated_fits=int(v[2]), sqrt_retries=int(v[3]),
                refined_fits=int(v[4]))


def torch_if_cuda():
    """torch if it is importable and sees a HIP device (it is the allocator of device-resident intermediates where a
    caller-side composition wants them, e.g. KoopmanKernelRegressor.fit), else None."""
    try:
        import torch
    except Exception:  # noqa: BLE001 -- optional dependency
        return None
    try:
        return torch if torch.cuda.is_available() else None
    except Exception:  # noqa: BLE001
        return None


class Mat:
    """A row-major float64 matrix view handed to the C-ABI: host (numpy) or device (anything with
    data_ptr()/stride()/shape such as a torch.cuda tensor).  Keeps the owner alive for the call."""

    def __init__(self, obj, rows=None, cols=None):
        if hasattr(obj, "data_ptr") and hasattr(obj, "stride"):  # device tensor (duck-typed torch)
            if str(getattr(obj, "dtype", "")).split(".")[-1] not in ("float64", "double"):
                raise TypeError("device tensors must be float64")
            if obj.dim() != 2 or (obj.shape[1] > 1 and obj.stride(1) != 1):  # (a size-1 dimension may carry any stride)
                raise ValueError("device tensors must be 2-D with unit inner stride")
            self.owner, self.ptr, self.ld = obj, obj.data_ptr(), int(obj.stride(0))
            self.shape = (int(obj.shape[0]), int(obj.shape[1]))
        else:
            a = np.asarray(obj, dtype=np.float64)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim != 2:
                raise ValueError("expected a 2-D array")
            if a.shape[1] > 0 and a.shape[0] > 0 and (a.strides[1] != 8 or a.strides[0] % 8 or a.strides[0] < 8 * a.shape[1]):
                a = np.ascontiguousarray(a)
            self.owner, self.ptr = a, a.ctypes.data
            self.ld = a.strides[0] // 8 if a.shape[0] > 1 else max(a.shape[1], 1)
            self.shape = a.shape
        if self.shape[0] <= 1:
            self.ld = max(self.ld, self.shape[1], 1)
        if rows is not None and self.shape[0] != rows or cols is not None and self.shape[1] != cols:
            raise ValueError(f"expected a {rows} x {cols} matrix, got {self.shape}")


# Packing helpers of the unit-table and batch calls.  A helper that hands out an address appends the array behind it to
# the `keep` list of the calling method, which lives until the native call has returned.
def _handle(h):
    """A model handle as an address: an int as it is, a c_void_p unwrapped."""
    return h.value if isinstance(h, C.c_void_p) else h


def _handle_array(models):
    hs = (_P * max(len(models), 1))()
    for i, h in enumerate(models):
        hs[i] = _handle(h)
    return hs


def _ptr(a):
    return None if a is None else a.ctypes.data


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(_I32))


def _f64(a, shape, keep, unit=None, what=None):
    """`a` as a C-contiguous float64 array of `shape` in `keep`; with `what`, a vector of `shape` entries or a ValueError."""
    if what is None:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    else:
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if a.size != shape:
            raise ValueError(f"unit {unit}: {what} has {a.size} entries, expected {shape}")
    keep.append(a)
    return a


def _uopt_table(u_opt, steps, p, n, uopt_rows, keep):
    """(table (n_uopt, max(steps, 1) * p) or None, n_uopt, the row of each unit: 0 with a table, else -1, unless given)."""
    uo, n_uopt = None, 0
    if u_opt is not None:
        uo = _f64(u_opt, (-1, max(steps, 1) * p), keep)
        n_uopt = uo.shape[0]
    if uopt_rows is None:
        uopt_rows = [0 if n_uopt else -1] * n
    return uo, n_uopt, uopt_rows


def _status_iters(n, per=None):
    """The int32 status (-1) and iteration (0) arrays of a batch call: n entries, `per` iteration counts each."""
    n1 = max(n, 1)
    return np.full(n1, -1, dtype=np.int32), np.zeros(n1 if per is None else (n1, per), dtype=np.int32)


def _pack_abqr(a, i, A, B, Q, R, keep):
    """The A, B, Q, R block of a DareProblem / MpcBuildProblem; returns (m, p)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"problem {i}: A must be square, got {A.shape}")
    keep.append(A)
    m = A.shape[0]
    B = _f64(B, (m, -1), keep)
    p = B.shape[1]
    Q, R = _f64(Q, (m, m), keep), _f64(R, (p, p), keep)
    a.m, a.p = m, p
    a.A, a.lda, a.B, a.ldb = A.ctypes.data, max(m, 1), B.ctypes.data, max(p, 1)
    a.Q, a.ldq, a.R, a.ldr = Q.ctypes.data, max(m, 1), R.ctypes.data, max(p, 1)
    return m, p


def _build_outputs(s, prefix, m, p, N, nc, Ny, want_P=None):
    """NaN-filled H, F, K, (P,) G, T of one controller build, their addresses in the fields prefix + name of `s`.  G and T
    are None without output rows, P is None unless wanted (want_P = None: the structure has no such field)."""
    nv, ny = max(N, 0) * p, nc * max(Ny, 0)
    o = dict(H=np.full((nv, nv), np.nan), F=np.full((nv, m), np.nan), K=np.full((p, m), np.nan))
    if want_P is not None:
        o["P"] = np.full((m, m), np.nan) if want_P else None
    o["G"] = np.full((ny, nv), np.nan) if nc else None
    o["T"] = np.full((ny, m), np.nan) if nc else None
    for k, v in o.items():
        setattr(s, prefix + k, _ptr(v))
    return o


class Context:
    """One nk_ctx (HIP stream + HBM workspace) on one device.  Not thread-safe; one per process and device."""

    def __init__(self, device=0, handle=None):
        self.lib = load_library()
        if handle is None:
            handle = _P()
            check(self.lib.nk_create(int(device), C.byref(handle)))
        self.handle = handle
        self.device = int(device)

    def enter(self):
        """Lock-step group member: start of a unit of work (nk_group_enter)."""
        check(self.lib.nk_group_enter(self.handle))

    def leave(self):
        check(self.lib.nk_group_leave(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.nk_synchronize(self.handle))

    @property
    def stream(self):
        return self.lib.nk_stream(self.handle)

    def set_strict_spd(self, strict):
        """True: a numerically rank-deficient regularised system raises LinAlgError (NK_ERR_NOT_SPD) instead of being
        solved like scipy.linalg.lstsq does (minimum-norm solution, singular values <= eps * sigma_max dropped).
        2 / "lstsq": every regularised system goes through the SVD with gelsd's cut-off, ill-conditioned or not."""
        check(self.lib.nk_set_strict_spd(self.handle, 2 if strict in (2, "lstsq") else (1 if strict else 0)))

    def set_refine(self, pivot_ratio=1e-9, steps=2):
        """Refine the regularised solves of fits whose smallest / largest Cholesky pivot is below `pivot_ratio` with
        doubled-precision residuals (nk_set_refine); pivot_ratio = 0 switches it off (the default)."""
        check(self.lib.nk_set_refine(self.handle, float(pivot_ratio), int(steps)))

    def wait_for(self, *objs):
        """Order the context's streams after the work queued on torch's current stream whenever one of `objs` is a
        device tensor: the library's streams are non-blocking, so nothing else makes them wait for, say, a pending
        all-reduce that produces the tensor (nk_wait_stream; the host does not block)."""
        torch = sys.modules.get("torch")
        if torch is None:
            return
        for o in objs:
            if hasattr(o, "data_ptr") and hasattr(o, "stride") and getattr(o, "is_cuda", False):
                stream = torch.cuda.current_stream(o.device)
                check(self.lib.nk_wait_stream(self.handle, C.c_void_p(stream.cuda_stream)))
                return

    def set_compute_dtype(self, dtype):
        """'f64' (default) or 'f32': arithmetic of the kernel blocks and Gram contractions of fits on this context
        (nk_set_compute_dtype: the stress configuration's fp32 engine; everything m x m stays fp64)."""
        code = {"f64": 0, "f32": 1}.get(str(dtype))
        if code is None:
            raise ValueError("dtype must be 'f64' or 'f32'")
        check(self.lib.nk_set_compute_dtype(self.handle, code))

    def _loop_multi(self, fn, head, d, p, steps, models, x0s, x_refs, u_opt, uopt_rows, want_x, want_u, want_scores, gains=None,
                    fill=None, keep=None, n_scores=4, want_info=None, mid=(), ou_flat=False):
        """plant_loop_multi, poly_plant_loop_multi and mpc_loop_multi: fn(ctx, *head, steps, unit table, *mid, n, u_opt table,
        n_uopt, states, controls, (info,) scores).  Normalises the states ((n, d); d = None: the width of x0s), fills model /
        x0 / x_ref / uopt of every unit and K from `gains` (PlantUnit) or what fill(unit, i) sets (MpcUnit), allocates the
        outputs that are wanted (want_info = None: no info argument).  Returns (scores, states, controls, info)."""
        n, steps, keep = len(models), int(steps), [] if keep is None else keep
        if gains is not None:
            if len(gains) != n:
                raise ValueError(f"{len(gains)} gains for {n} models")
            Ks = [_f64(K, -1, keep).ctypes.data for K in gains]

            def fill(u, i):
                u.K = Ks[i]
        if d is None:
            x0s = _f64(x0s, (n, -1), keep) if n else np.zeros((0, 1))
            d = x0s.shape[1]
            x_refs = _f64(x_refs, (n, d), keep) if n else np.zeros((0, d))
        else:
            x0s, x_refs = _f64(x0s, (n, d), keep), _f64(x_refs, (n, d), keep)
        uo, n_uopt, uopt_rows = _uopt_table(u_opt, steps, p, n, uopt_rows, keep)
        arr = ((MpcUnit if gains is None else PlantUnit) * max(n, 1))()
        x0, xr, row = x0s.ctypes.data, x_refs.ctypes.data, 8 * d
        for i in range(n):
            u = arr[i]
            u.model, u.x0, u.x_ref, u.uopt = _handle(models[i]), x0 + i * row, xr + i * row, int(uopt_rows[i])
            fill(u, i)
        T = max(steps, 0)
        sc = np.full((n, n_scores), np.nan) if want_scores else None
        ox = np.empty((n, T + 1, d)) if want_x else None
        ou = np.empty((n, T) if ou_flat else (n, T, p)) if want_u else None
        oi = np.empty((n, T, 2)) if want_info else None
        info = () if want_info is None else (_ptr(oi),)
        check_mapped(fn(self.handle, *head, steps, arr, *mid, n, _ptr(uo), n_uopt, _ptr(ox), _ptr(ou), *info, _ptr(sc)))
        return sc, ox, ou, oi

    def plant_loop_multi(self, plant_id, Ts, steps, models, gains, x0s, x_refs, u_opt=None, uopt_rows=None,
                         want_x=False, want_u=False, want_scores=True):
        """nk_plant_loop_multi: one closed loop around the true plant per unit, all units in one call, scored on the device.
        models: device-model handles (one per unit); gains: one (1, m) / (m,) array per unit; x0s, x_refs: (n_units, d);
        u_opt: (n_uopt, steps) reference controls or None; uopt_rows: the row each unit is scored against (-1: none;
        default: row 0 for every unit when u_opt is given).  Returns (scores (n_units, 4) or None, states
        (n_units, steps + 1, d) or None, controls (n_units, steps) or None); scores[u] = sse_u, ss_opt, J, u_absmax."""
        return self._loop_multi(self.lib.nk_plant_loop_multi, (int(plant_id), float(Ts)), None, 1, steps, models, x0s, x_refs,
                                u_opt, uopt_rows, want_x, want_u, want_scores, gains, ou_flat=True)[:3]

    def poly_plant_loop_multi(self, descriptor, steps, models, gains, x0s, x_refs, u_opt=None, uopt_rows=None, want_x=False,
                              want_u=False, want_scores=True):
        """nk_poly_plant_loop_multi: plant_loop_multi around a polynomial plant (descriptor: a PolyPlant) with p inputs.
        gains: one (p, m) array per unit; u_opt: (n_uopt, steps, p) or None.  Returns (scores (n_units, 4) or None, states
        (n_units, steps + 1, d) or None, controls (n_units, steps, p) or None)."""
        return self._loop_multi(self.lib.nk_poly_plant_loop_multi, (C.byref(descriptor),), int(descriptor.d), int(descriptor.p),
                                steps, models, x0s, x_refs, u_opt, uopt_rows, want_x, want_u, want_scores, gains)[:3]

    def mpc_loop_multi(self, descriptor, steps, models, descs, x0s, x_refs, u_inits=None, u_opt=None, uopt_rows=None,
                       want_x=False, want_u=False, want_info=False, want_scores=True, outs=None):
        """nk_mpc_loop_multi: one constrained MPC loop around a polynomial plant (descriptor: a PolyPlant) per unit, all units
        in one call, scored on the device.  models: device-model handles; descs: one MpcDesc per unit (units may share one;
        the caller keeps their arrays alive); x0s, x_refs: (n_units, d); u_inits: (n_units, p), a list with None entries, or
        None = zeros; u_opt: (n_uopt, steps, p) or None; uopt_rows as in poly_plant_loop_multi.  Returns (scores
        (n_units, 8) or None, states (n_units, steps + 1, d) or None, controls (n_units, steps, p) or None, info
        (n_units, steps, 2) or None).
        outs: None, or one entry per unit, an MpcOut (units may share one; the caller keeps their arrays alive) or None for a
        unit without rows -- the call is then nk_mpc_out_loop_multi and the scores are (n_units, 10)."""
        n, keep = len(models), []
        d, p = int(descriptor.d), int(descriptor.p)
        if len(descs) != n:
            raise ValueError(f"{len(descs)} descriptions for {n} models")
        uis = [None] * n
        if u_inits is not None:
            if len(u_inits) != n:
                raise ValueError(f"{len(u_inits)} u_inits for {n} models")
            uis = [None if ui is None else _f64(ui, p, keep).ctypes.data for ui in u_inits]
        if outs is not None and len(outs) != n:
            raise ValueError(f"{len(outs)} output descriptions for {n} models")

        def fill(u, i):
            u.desc, u.u_init = C.pointer(descs[i]), uis[i]

        if outs is None:
            fn, mid, n_scores = self.lib.nk_mpc_loop_multi, (), MPC_N_SCORES
        else:
            oarr = (C.POINTER(MpcOut) * max(n, 1))()  # (null pointers; `outs` keeps the structures alive through the call)
            for i, o in enumerate(outs):
                if o is not None:
                    oarr[i] = C.pointer(o)
            fn, mid, n_scores = self.lib.nk_mpc_out_loop_multi, (oarr,), MPC_OUT_N_SCORES
        return self._loop_multi(fn, (C.byref(descriptor),), d, p, steps, models, x0s, x_refs, u_opt, uopt_rows, want_x, want_u,
                                want_scores, None, fill, keep, n_scores, bool(want_info), mid)

    def _single_loop(self, fn, head, K, xb, xr, u_init, steps, p, want_info=None):
        """fn(ctx, *head, (K,) x0, x_ref, (u_init,) steps, batch, states, controls, (info)): the single-model plant loops on
        C-contiguous (batch, d) states.  want_info = None: the call has neither u_init nor info."""
        batch, d = xb.shape
        T = max(steps, 0)
        ox, ou = np.empty((batch, T + 1, d)), np.empty((batch, T, p))
        oi = np.empty((batch, T, 2)) if want_info else None
        gain = () if K is None else (K.ctypes.data,)
        seed, info = ((), ()) if want_info is None else ((_ptr(u_init),), (_ptr(oi),))
        check_mapped(fn(self.handle, *head, *gain, xb.ctypes.data, xr.ctypes.data, *seed, steps, batch, ox.ctypes.data,
                        ou.ctypes.data, *info))
        return ox, ou, oi

    def plant_loop(self, model, plant_id, Ts, K, xb, xr, steps):
        """nk_plant_loop: LQR loops around a built-in plant that share the gain K (1, m).  xb, xr: C-contiguous (batch, d).
        Returns (states (batch, steps + 1, d), controls (batch, steps, 1))."""
        return self._single_loop(self.lib.nk_plant_loop, (model, int(plant_id), float(Ts)), K, xb, xr, None, steps, 1)[:2]

    def poly_plant_loop(self, model, descriptor, K, xb, xr, steps):
        """nk_poly_plant_loop: plant_loop around a polynomial plant (descriptor: a PolyPlant), K (p, m).  Returns (states
        (batch, steps + 1, d), controls (batch, steps, p))."""
        return self._single_loop(self.lib.nk_poly_plant_loop, (model, descriptor), K, xb, xr, None, steps, K.shape[0])[:2]

    def mpc_loop(self, model, descriptor, desc, xb, xr, steps, u_init=None, want_info=False, out=None):
        """nk_mpc_loop, or nk_mpc_out_loop with an MpcOut as `out`: constrained MPC loops around a polynomial plant that share
        the controller (desc: an MpcDesc; the caller keeps its arrays, and those of `out`, alive).  u_init: C-contiguous
        (batch, p) or None = zeros.  Returns (states, controls (batch, steps, p), info (batch, steps, 2) or None)."""
        if out is None:
            fn, head = self.lib.nk_mpc_loop, (model, descriptor, C.byref(desc))
        else:
            fn, head = self.lib.nk_mpc_out_loop, (model, descriptor, C.byref(desc), C.byref(out))
        return self._single_loop(fn, head, None, xb, xr, u_init, steps, int(desc.p), bool(want_info))

    def closed_loop_batch(self, model, K, f0, fr, steps, d):
        """nk_closed_loop_batch: lifted closed loops that share the gain K (p, m).  f0, fr: C-contiguous (batch, m); d: the
        model's state dimension.  Returns (states (batch, steps, d), controls (batch, steps, p))."""
        batch = f0.shape[0]
        ox, ou = np.empty((batch, steps, d)), np.empty((batch, steps, K.shape[0]))
        check(self.lib.nk_closed_loop_batch(self.handle, model, K.ctypes.data, f0.ctypes.data, fr.ctypes.data, int(steps), batch,
                                            ox.ctypes.data, ou.ctypes.data))
        return ox, ou

    def closed_loop_multi(self, steps, c, models, dims, gains, phi0s, phi_refs, targets=None, u_inits=None, want_x=False,
                          want_u=False, want_ucum=False, want_err=True, want_scores=True):
        """nk_closed_loop_multi: one lifted closed loop per unit (u_t = K (phi_ref - phi_t), x_t = C phi_t, phi_{t+1} =
        A phi_t + B u_t), all units in one call and one launch, scored on the device.  models: device-model handles; dims:
        their (m, p, d); gains: one (p, m) array per unit; phi0s, phi_refs: one (m,) array per unit; targets: one (d,) array
        per unit (None: nothing is scored); u_inits: one (p,) array per unit, None entries (or None) = zeros.
        Returns (scores (n_units, 4) = J, err_final, u_sumsq, u_absmax or None, err (n_units, steps) or None, and three lists
        of per-unit arrays or None: states (steps, d), controls (steps, p), cum_controls (steps + 1, p))."""
        n = len(models)
        steps = int(steps)
        if not (len(dims) == len(gains) == len(phi0s) == len(phi_refs) == n):
            raise ValueError("models, dims, gains, phi0s and phi_refs must have the same length")
        if targets is None and (want_err or want_scores):
            raise ValueError("scores and errors need a target per unit")
        arr = (LoopUnit * max(n, 1))()
        keep = []
        for i in range(n):
            m, p, d = (int(v) for v in dims[i])
            u = arr[i]
            u.model = _handle(models[i])
            u.K = _f64(gains[i], p * m, keep, i, "the gain").ctypes.data
            u.phi0 = _f64(phi0s[i], m, keep, i, "phi0").ctypes.data
            u.phi_ref = _f64(phi_refs[i], m, keep, i, "phi_ref").ctypes.data
            if targets is not None:
                u.target = _f64(targets[i], d, keep, i, "the target").ctypes.data
            if u_inits is not None and u_inits[i] is not None:
                u.u_init = _f64(u_inits[i], p, keep, i, "u_init").ctypes.data
        T = max(steps, 0)
        nx, nu, nc = (sum(rows * int(dm[col]) for dm in dims) for rows, col in ((T, 2), (T, 1), (T + 1, 1)))
        ox = np.empty(max(nx, 1)) if want_x else None
        ou = np.empty(max(nu, 1)) if want_u else None
        oc = np.empty(max(nc, 1)) if want_ucum else None
        oe = np.full((n, T), np.nan) if want_err else None
        sc = np.full((n, 4), np.nan) if want_scores else None
        check_mapped(self.lib.nk_closed_loop_multi(self.handle, steps, float(c), arr, n, _ptr(ox), _ptr(ou), _ptr(oc), _ptr(oe),
                                                   _ptr(sc)))

        def split(flat, rows, col):
            if flat is None:
                return None
            out, off = [], 0
            for dm in dims:
                w = int(dm[col])
                out.append(flat[off:off + rows * w].reshape(rows, w))
                off += rows * w
            return out

        return sc, oe, split(ox, T, 2), split(ou, T, 1), split(oc, T + 1, 1)

    def dare_batch(self, As, Bs, Qs, Rs, tol=1e-13, max_iter=40, want_P=True):
        """nk_dare_batch: K = dlqr(A, B, Q, R) for every problem of the lists in one call, one workgroup per problem.
        Returns (Ks, Ps or None, status, iterations, deltas): lists of (p, m) and (m, m) arrays and int32 / float64
        arrays of length n; status 0 = converged, 1 = max_iter reached, 2 = non-finite / singular (outputs NaN)."""
        n = len(As)
        if not (len(Bs) == len(Qs) == len(Rs) == n):
            raise ValueError("As, Bs, Qs, Rs must have the same length")
        arr = (DareProblem * max(n, 1))()
        keep, Ks, Ps = [], [], []
        delta = np.full(max(n, 1), np.nan)
        for i in range(n):
            a = arr[i]
            m, p = _pack_abqr(a, i, As[i], Bs[i], Qs[i], Rs[i], keep)
            Ks.append(np.full((p, m), np.nan))
            Ps.append(np.full((m, m), np.nan) if want_P else None)
            a.out_K, a.out_P, a.out_delta = Ks[i].ctypes.data, _ptr(Ps[i]), delta.ctypes.data + 8 * i
        status, iters = _status_iters(n)
        check_mapped(self.lib.nk_dare_batch(self.handle, arr, n, float(tol), int(max_iter), _i32p(status), _i32p(iters)))
        return Ks, (Ps if want_P else None), status[:n], iters[:n], delta[:n]

    def model_lqr_gain_batch(self, models, c, R=None, tol=1e-13, max_iter=40, dims=None):
        """nk_model_lqr_gain_batch: K_u = dlqr(A_u, B_u, c sym(C_u'C_u), R) for n device models in one call (R = None: the
        identity).  models: device-model handles; dims: their (m, p) pairs (queried with nk_model_dims when None).
        Returns (Ks, status, iterations); a unit with status != 0 has a NaN gain."""
        n = len(models)
        hs = _handle_array(models)
        if dims is None:
            dims = []
            for i in range(n):
                m, d, p = _I32(), _I32(), _I32()
                check(self.lib.nk_model_dims(hs[i], C.byref(m), C.byref(d), C.byref(p)))
                dims.append((m.value, p.value))
        sizes = [int(m) * int(p) for m, p in dims]
        out = np.full(max(sum(sizes), 1), np.nan)
        Rm = None if R is None else np.ascontiguousarray(R, dtype=np.float64)
        status, iters = _status_iters(n)
        check_mapped(self.lib.nk_model_lqr_gain_batch(self.handle, hs, n, float(c), _ptr(Rm), float(tol), int(max_iter),
                                                      out.ctypes.data, _i32p(status), _i32p(iters)))
        Ks, off = [], 0
        for (m, p), sz in zip(dims, sizes):
            Ks.append(out[off:off + sz].reshape(int(p), int(m)).copy())
            off += sz
        return Ks, status[:n], iters[:n]

    def mpc_build_batch(self, As, Bs, Qs, Rs, Ns, Ps=None, C_rows=None, Nys=None, tol=1e-13, max_iter=40, newton_steps=1,
                        newton_tol=1e-15, newton_max_iter=60, want_P=True):
        """nk_mpc_build_batch: the controllers of a list of problems in one call, one workgroup per problem.  Ps: terminal
        costs (a None entry, or Ps = None: the Riccati solution with newton_steps Newton steps); C_rows: (nc, m) output rows
        per problem or None, with the horizons Nys (default N).  Returns a dict of lists H, F, K, P, G, T (G, T None for a
        problem without rows; P None unless want_P) and the arrays status (n,), iters (n, 2) = {doubling steps, Smith
        squarings}; status 0 = success, 1 = doubling cap, 2 = non-finite / not positive definite, 3 = Smith cap (NaN outputs)."""
        n = len(As)
        if not (len(Bs) == len(Qs) == len(Rs) == len(Ns) == n):
            raise ValueError("As, Bs, Qs, Rs, Ns must have the same length")
        arr = (MpcBuildProblem * max(n, 1))()
        keep = []
        res = dict(H=[], F=[], K=[], P=[], G=[], T=[])
        for i in range(n):
            a = arr[i]
            m, p = _pack_abqr(a, i, As[i], Bs[i], Qs[i], Rs[i], keep)
            N = int(Ns[i])
            P = None if Ps is None or Ps[i] is None else _f64(Ps[i], (m, m), keep)
            Cr = None if C_rows is None or C_rows[i] is None else _f64(C_rows[i], (-1, m), keep)
            nc = 0 if Cr is None else Cr.shape[0]
            Ny = 0 if nc == 0 else (N if Nys is None or Nys[i] is None else int(Nys[i]))
            a.N, a.nc, a.Ny = N, nc, Ny
            a.P, a.ldp, a.C_rows, a.ldc = _ptr(P), max(m, 1), _ptr(Cr), max(m, 1)
            for k, v in _build_outputs(a, "out_", m, p, N, nc, Ny, bool(want_P)).items():
                res[k].append(v)
        status, iters = _status_iters(n, 2)
        check_mapped(self.lib.nk_mpc_build_batch(self.handle, arr, n, float(tol), int(max_iter), int(newton_steps),
                                                 float(newton_tol), int(newton_max_iter), _i32p(status), _i32p(iters)))
        res["status"], res["iters"] = status[:n], iters[:n]
        return res

    def model_mpc_build_batch(self, models, dims, c, R, specs, tol=1e-13, max_iter=40, newton_steps=1, newton_tol=1e-15,
                              newton_max_iter=60):
        """nk_model_mpc_build_batch: the controllers of n device models in one call.  models: device-model handles; dims:
        their (m, p) pairs; R: (p, p) or None for the identity; specs: per unit (N, comps, Ny) with comps the state components
        of the output rows (empty: none).  Returns (units, status (n,), iters (n, 2)); units[u] = dict(H, F, K, G, T) (G, T
        None without rows); a unit with status != 0 has NaN arrays."""
        n = len(models)
        hs = _handle_array(models)
        sp = (MpcBuildSpec * max(n, 1))()
        ou = (MpcBuildOut * max(n, 1))()
        units = []
        for i in range(n):
            m, p = int(dims[i][0]), int(dims[i][1])
            N, comps, Ny = specs[i]
            N, comps = int(N), [int(v) for v in comps]
            if len(comps) > 4:
                raise ValueError(f"unit {i}: {len(comps)} output rows per step, at most 4")
            nc = len(comps)
            Ny = 0 if nc == 0 else (N if Ny is None else int(Ny))
            sp[i].N, sp[i].nc, sp[i].Ny = N, nc, Ny
            for k, v in enumerate(comps):
                sp[i].comps[k] = v
            units.append(_build_outputs(ou[i], "", m, p, N, nc, Ny))
        Rm = None if R is None else np.ascontiguousarray(R, dtype=np.float64)
        status, iters = _status_iters(n, 2)
        check_mapped(self.lib.nk_model_mpc_build_batch(self.handle, hs, n, float(c), _ptr(Rm), sp, float(tol), int(max_iter),
                                                       int(newton_steps), float(newton_tol), int(newton_max_iter), ou,
                                                       _i32p(status), _i32p(iters)))
        return units, status[:n], iters[:n]

    def mpc_build_times(self):
        """nk_mpc_build_times: dict(ms_riccati, ms_build, groups) of this thread's last build call: device time by events."""
        v = (_D * 3)()
        check(self.lib.nk_mpc_build_times(v))
        return dict(ms_riccati=v[0], ms_build=v[1], groups=int(v[2]))

    def dare_large(self, A, B, Q, R, tol=1e-13, max_iter=40, want_P=True):
        """nk_dare_large: K = dlqr(A, B, Q, R) for ONE problem of any size (m <= 10240, p <= 32) by the launch-chain solver.
        A, B, Q, R: NumPy arrays or float64 device tensors (2-D, unit inner stride), each on its own.  Returns
        (K (p, m), P (m, m) or None, status, iterations, delta) with host arrays; status 0 = converged, 1 = max_iter
        reached, 2 = non-finite / singular (outputs NaN)."""
        a = Mat(A)
        m = a.shape[0]
        if a.shape != (m, m):
            raise ValueError(f"A must be square, got {a.shape}")
        if not (hasattr(B, "data_ptr") and hasattr(B, "stride")):
            B = np.asarray(B, dtype=np.float64).reshape(m, -1) if m else np.zeros((0, 1))
        b = Mat(B)
        p = b.shape[1]
        q, r = Mat(Q, m, m), Mat(R, p, p)
        if b.shape[0] != m:
            raise ValueError(f"B has {b.shape[0]} rows, A {m}")
        K = np.full((p, m), np.nan)
        P = np.full((m, m), np.nan) if want_P else None
        status, iters, delta = _I32(-1), _I32(0), _D(np.nan)
        self.wait_for(A, B, Q, R)
        rc = self.lib.nk_dare_large(self.handle, m, p, a.ptr, a.ld, b.ptr, b.ld, q.ptr, q.ld, r.ptr, r.ld, float(tol),
                                    int(max_iter), K.ctypes.data, P.ctypes.data if want_P else None, C.byref(delta),
                                    C.byref(status), C.byref(iters))
        check_mapped(rc)
        return K, P, int(status.value), int(iters.value), float(delta.value)

    def model_lqr_gain(self, model, m, p, c, R=None, tol=1e-13, max_iter=40):
        """nk_model_lqr_gain: K = dlqr(A, B, c sym(C'C), R) of one device model by the launch-chain solver, whatever m is
        (R = None: the identity).  Returns (K (p, m), status, iterations); a status other than 0 has a NaN gain."""
        keep = []
        K = np.full((int(p), int(m)), np.nan)
        Rm = None if R is None else _f64(R, (int(p), int(p)), keep)
        status, iters = _I32(-1), _I32(0)
        check_mapped(self.lib.nk_model_lqr_gain(self.handle, _handle(model), float(c), _ptr(Rm), float(tol), int(max_iter),
                                                K.ctypes.data, C.byref(status), C.byref(iters)))
        return K, int(status.value), int(iters.value)

    def dare_large_times(self):
        """nk_dare_large_times: dict(ms_total, ms_lu, ms_products, ms_sync, steps) of this thread's last nk_dare_large /
        nk_model_lqr_gain; the split is taken only with NYSKOOP_DARE_TIMING set in the environment."""
        v = (_D * 5)()
        check(self.lib.nk_dare_large_times(v))
        return dict(ms_total=v[0], ms_lu=v[1], ms_products=v[2], ms_sync=v[3], steps=int(v[4]))

    def model_lqr_cost(self, model, m, c):
        """nk_model_lqr_cost: the cost matrix c sym(C'C) (m x m) exactly as nk_model_lqr_gain_batch forms it."""
        Q = np.empty((int(m), int(m)))
        rc = self.lib.nk_model_lqr_cost(self.handle, _handle(model), float(c), Q.ctypes.data, int(m))
        check_mapped(rc)
        return Q

    def set_kmat_mode(self, mode):
        """0 = automatic (Gram form on the MFMA engine for d >= 32), 1 = always direct differences."""
        check(self.lib.nk_set_kmat_mode(self.handle, int(mode)))


class _PinnedBlock:
    """A page-locked host block that returns to a small pool when its last array view dies."""
    _pool = {}
    _lock = threading.Lock()
    _closed = False

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = None
        with _PinnedBlock._lock:
            free = _PinnedBlock._pool.get(self.nbytes)
            if free:
                self.ptr = free.pop()
        if self.ptr is None:
            self.ptr = load_library().nk_host_alloc(self.nbytes)
            if not self.ptr:
                raise MemoryError(f"nk_host_alloc({self.nbytes}) failed")

    def __del__(self):
        try:
            with _PinnedBlock._lock:
                free = _PinnedBlock._pool.setdefault(self.nbytes, [])
                if not _PinnedBlock._closed and len(free) < 8:
                    free.append(self.ptr)
                    return
            load_library().nk_host_free(self.ptr)  # a no-op after nk_shutdown
        except Exception:
            pass

    @classmethod
    def drain(cls):
        """Free the pooled blocks and stop pooling (blocks still referenced by arrays are released by nk_shutdown)."""
        with cls._lock:
            ptrs = [p for free in cls._pool.values() for p in free]
            cls._pool.clear()
            cls._closed = True
        lib = load_library()
        for p in ptrs:
            lib.nk_host_free(p)


def pinned_empty(shape):
    """float64 C-contiguous ndarray backed by page-locked memory (results of fit land here)."""
    n = int(np.prod(shape))
    if n == 0:
        return np.empty(shape)
    block = _PinnedBlock(n * 8)
    buf = (C.c_double * n).from_address(block.ptr)
    buf._nk_owner = block  # the ctypes array is the ndarray's base and keeps the block alive
    return np.frombuffer(buf, dtype=np.float64).reshape(shape)


_tls = threading.local()


def default_device():
    return int(os.environ.get("NYSKOOP_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def get_context(device=None):
    """The calling thread's context on `device` (a context is not thread-safe: one per thread and device; independent
    fits issued from several threads overlap on the GPU).  Contexts live in thread-local storage, so a worker thread's
    streams and workspace are released when the thread ends."""
    device = default_device() if device is None else int(device)
    ctxs = getattr(_tls, "ctxs", None)
    if ctxs is None:
        ctxs = _tls.ctxs = {}
    key = (os.getpid(), device)
    ctx = ctxs.get(key)
    if ctx is None:
        ctx = ctxs[key] = Context(device)
    return ctx


class LockstepPool:
    """`size` host threads, thread i permanently bound to member i of a lock-step group (nk_group_create): the units of a
    round run through the ordinary API, one per thread, and the library merges their kernel launches (see
    include/nyskoop.h).  run_round(fn, items) runs fn(item) for up to `size` items, one per member, and returns the results
    in order; an exception in a unit is re-raised after the round."""

    def __init__(self, size, device=None):
        import queue
        self.size = int(size)
        self.device = default_device() if device is None else int(device)
        lib = load_library()
        handles = (_P * self.size)()
        check(lib.nk_group_create(self.device, self.size, handles))
        self.members = [Context(self.device, _P(handles[i])) for i in range(self.size)]
        self._queues = [queue.Queue() for _ in range(self.size)]
        self._done = queue.Queue()
        self._threads = [threading.Thread(target=self._worker, args=(i,), daemon=True, name=f"nyskoop-lockstep-{i}")
                         for i in range(self.size)]
        for t in self._threads:
            t.start()

    def _worker(self, i):
        member = self.members[i]
        _tls.ctxs = {(os.getpid(), self.device): member}
        while True:
            task = self._queues[i].get()
            if task is None:
                return
            fn, item, k = task
            try:
                out = (k, fn(item), None)
            except BaseException as e:  # noqa: BLE001 -- reported to the caller of run_round
                out = (k, None, e)
            finally:
                try:
                    member.leave()
                except Exception:
                    pass
            self._done.put(out)

    def run_round(self, fn, items):
        items = list(items)
        if len(items) > self.size:
            raise ValueError("more items than members")
        for k in range(len(items)):  # all members of the round are inside their unit before any of them starts
            self.members[k].enter()
        for k, item in enumerate(items):
            self._queues[k].put((fn, item, k))
        results, err = [None] * len(items), None
        for _ in items:
            k, out, e = self._done.get()
            results[k] = out
            err = err or e
        if err is not None:
            raise err
        return results

    def map(self, fn, items):
        items = list(items)
        out = []
        for r in range(0, len(items), self.size):
            out.extend(self.run_round(fn, items[r:r + self.size]))
        return out

    @staticmethod
    def _grid_data(X, Y, n_inputs):
        """The shared data set of a grid call, checked: (Xm, Ym, n, d, p)."""
        Xm, Ym = Mat(X), Mat(Y)
        n, d = Ym.shape
        p = int(n_inputs)
        if Xm.shape != (n, d + p):
            raise ValueError(f"X has shape {Xm.shape}, expected {(n, d + p)}")
        return Xm, Ym, n, d, p

    def _grid_call(self, name, data, extra, arr, n_scores, n_score_arrays=1):
        """The grid entry point `name` on the members' contexts: data set, the call's own arguments `extra`, the units
        `arr`, then `n_score_arrays` NaN-filled float64 outputs of n_scores entries and one int32 status per unit.
        Returns (*scores, status)."""
        Xm, Ym, n, d, p = data
        handles = (_P * self.size)(*[m_.handle for m_ in self.members])
        scores = [np.full(n_scores, np.nan) for _ in range(n_score_arrays)]
        status = np.zeros(len(arr), dtype=np.int32)
        rc = getattr(self.members[0].lib, name)(handles, self.size, Xm.ptr, Xm.ld, Ym.ptr, Ym.ld, n, d, p, *extra, arr,
                                                len(arr), *[a.ctypes.data_as(C.POINTER(_D)) for a in scores],
                                                status.ctypes.data_as(C.POINTER(_I32)))
        check_mapped(rc)
        return (*scores, status)

    def cv_grid(self, X, Y, n_inputs, units):
        """nk_cv_grid: `units` = list of (DeviceKernel, gamma, jitter, m, (test_begin, test_end), landmark_rows) run in
        lock step, len(members) at a time, entirely inside the library (no Python per unit).  Returns (scores, status)."""
        data = self._grid_data(X, Y, n_inputs)
        d = data[3]
        arr = (CvUnit * len(units))()
        keep = []
        descs = {}
        for i, (kern, gamma, jitter, m, (lo, hi), rows) in enumerate(units):
            if id(kern) not in descs:
                descs[id(kern)] = kern.desc(d)
            kd, ls = descs[id(kern)]
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.shape != (int(m),):
                raise ValueError("landmark_rows must hold m row indices")
            keep.append(rows)
            arr[i].kernel = C.pointer(kd)
            arr[i].gamma, arr[i].jitter, arr[i].m = float(gamma), float(jitter), int(m)
            arr[i].test_begin, arr[i].test_end = int(lo), int(hi)
            arr[i].landmark_rows = rows.ctypes.data_as(C.POINTER(C.c_int64))
        return self._grid_call("nk_cv_grid", data, (), arr, len(units))

    def spline_cv_grid(self, X, Y, n_inputs, units):
        """nk_spline_cv_grid: `units` = list of (gamma, m, (test_begin, test_end), centers (m x d)) of the thin-plate-spline
        estimator, run in lock step like cv_grid.  Returns (scores, status)."""
        data = self._grid_data(X, Y, n_inputs)
        d = data[3]
        arr = (SplineCvUnit * len(units))()
        keep = []
        for i, (gamma, m, (lo, hi), centers) in enumerate(units):
            Z = np.ascontiguousarray(centers, dtype=np.float64)
            if Z.shape != (int(m), d):
                raise ValueError(f"centers must be an m x d = {(int(m), d)} array, got {Z.shape}")
            keep.append(Z)
            arr[i].gamma, arr[i].m = float(gamma), int(m)
            arr[i].test_begin, arr[i].test_end = int(lo), int(hi)
            arr[i].centers = Z.ctypes.data_as(C.POINTER(C.c_double))
        return self._grid_call("nk_spline_cv_grid", data, (), arr, len(units))

    def sysid_grid(self, X, Y, n_inputs, trajs, controls, units):
        """nk_sysid_grid: the multi-seed system-identification sweep in one call.  X: n x (d+p), Y: n x d (the shared data
        set); trajs: (n_trajs, T, d) test trajectories, controls: (n_trajs, T, p) (row T-1 never read; None when p = 0).
        `units` = list of (kernel, gamma, jitter, m, row_ranges, landmarks, traj_indices): kernel = a DeviceKernel for a
        Nystrom unit, whose `landmarks` are m row indices into Y, or None for a thin-plate-spline unit, whose `landmarks`
        are its centres (m x d); row_ranges = [begin, end) pairs of training rows or None (all rows); traj_indices = the
        unit's test trajectories.  Returns (err_abs, err_rel, status, offsets): flat unit-major arrays, unit u owning
        [offsets[u], offsets[u + 1]); a failed unit holds NaN and its code in status[u]."""
        units, offsets = sysid_unit_layout(units)
        data = self._grid_data(X, Y, n_inputs)
        d, p = data[3:]
        tr = np.ascontiguousarray(trajs, dtype=np.float64)
        if tr.ndim != 3 or tr.shape[2] != d:
            raise ValueError(f"trajs must be (n_trajs, T, {d}), got {tr.shape}")
        n_trajs, T = tr.shape[0], tr.shape[1]
        U = None
        if p > 0 and T > 1:
            U = np.ascontiguousarray(controls, dtype=np.float64)
            if U.shape != (n_trajs, T, p):
                raise ValueError(f"controls must be {(n_trajs, T, p)}, got {U.shape}")
        arr = (SysidUnit * len(units))()
        keep, descs = [], {}
        for i, (kern, gamma, jitter, m, ranges, marks, tidx) in enumerate(units):
            arr[i].gamma, arr[i].jitter, arr[i].m = float(gamma), float(jitter), int(m)
            if kern is not None:
                if id(kern) not in descs:
                    descs[id(kern)] = kern.desc(d)
                arr[i].kernel = C.pointer(descs[id(kern)][0])
                rows = np.ascontiguousarray(marks, dtype=np.int64)
                if rows.shape != (int(m),):
                    raise ValueError("a Nystrom unit's landmarks must be m row indices")
                keep.append(rows)
                arr[i].landmark_rows = rows.ctypes.data_as(C.POINTER(C.c_int64))
            else:
                Z = np.ascontiguousarray(marks, dtype=np.float64)
                if Z.shape != (int(m), d):
                    raise ValueError(f"a spline unit's centres must be m x d = {(int(m), d)}, got {Z.shape}")
                keep.append(Z)
                arr[i].centers = Z.ctypes.data_as(C.POINTER(C.c_double))
            if ranges is not None:
                rr = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1))
                keep.append(rr)
                arr[i].row_ranges, arr[i].n_ranges = rr.ctypes.data_as(C.POINTER(C.c_int64)), rr.size // 2
            ti = np.ascontiguousarray(tidx, dtype=np.int32).reshape(-1)
            keep.append(ti)
            arr[i].traj, arr[i].n_traj = ti.ctypes.data_as(C.POINTER(C.c_int32)), ti.size
        extra = (tr.ctypes.data, None if U is None else U.ctypes.data, n_trajs, T)
        err_abs, err_rel, status = self._grid_call("nk_sysid_grid", data, extra, arr, int(offsets[-1]), 2)
        return err_abs, err_rel, status, offsets

    def stats(self):
        v = (C.c_uint64 * 4)()
        check(self.members[0].lib.nk_group_stats(self.members[0].handle, v))
        return dict(flushes=int(v[0]), merged_launches=int(v[1]), single_launches=int(v[2]), member_launches_merged=int(v[3]))

    def close(self):
        for q in self._queues:
            q.put(None)
        for t in self._threads:
            t.join(timeout=5)
        for m in self.members:
            m.close()


def sysid_unit_layout(units):
    """The flat unit-major layout of nk_sysid_grid's outputs: returns (units as a list, offsets) where unit u owns the
    entries [offsets[u], offsets[u + 1]) -- the prefix sums of the units' numbers of test trajectories.  Needs no GPU."""
    units = list(units)
    counts = [int(np.asarray(u[6]).size) for u in units]
    if any(c < 1 for c in counts):
        raise ValueError("every unit needs at least one test trajectory")
    return units, np.concatenate(([0], np.cumsum(counts, dtype=np.int64))).astype(np.int64)


_lockstep_pools = {}


def lockstep_pool(size, device=None, index=0):
    """A persistent LockstepPool of `size` members on `device` (created on first use); `index` distinguishes several
    pools of the same size (independent groups whose work overlaps on the GPU)."""
    device = default_device() if device is None else int(device)
    with _pools_lock:
        key = (os.getpid(), device, int(size), int(index))
        pool = _lockstep_pools.get(key)
        if pool is None:
            pool = _lockstep_pools[key] = LockstepPool(size, device)
        return pool


_pools = {}
_pools_lock = threading.Lock()


def worker_pool(workers):
    """A persistent pool of `workers` host threads (their contexts, streams and workspaces are reused across calls)."""
    from concurrent.futures import ThreadPoolExecutor
    with _pools_lock:
        key = (os.getpid(), int(workers))
        pool = _pools.get(key)
        if pool is None:
            pool = _pools[key] = ThreadPoolExecutor(max_workers=int(workers), thread_name_prefix="nyskoop")
        return pool
