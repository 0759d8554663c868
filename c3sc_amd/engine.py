"""ctypes binding of libc3sc_hip.so (include/c3sc_hip.h) + a thin host-side engine object.

PyTorch is used only as plumbing: device buffers (torch tensors' data_ptr()), streams and
torch.distributed.  The compute path is the HIP library; if it is missing this module raises --
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libc3sc_hip.so")
_LIB = None

c_double_p = C.POINTER(C.c_double)
c_size_p = C.POINTER(C.c_size_t)
c_int_p = C.POINTER(C.c_int)
c_i32_p = C.POINTER(C.c_int32)

# every symbol include/c3sc_hip.h declares (the CPU test-suite checks they are all exported)
EXPORTS = [
    "c3sc_hip_ctx_create", "c3sc_hip_ctx_destroy", "c3sc_hip_last_error", "c3sc_hip_device_count", "c3sc_hip_max_rank",
    "c3sc_hip_set_grid", "c3sc_hip_set_boundary", "c3sc_hip_set_consistent_ends", "c3sc_hip_get_consistent_ends", "c3sc_hip_cross_setup", "c3sc_hip_cross_iteration", "c3sc_hip_cross_iteration_streamed", "c3sc_hip_cross_wait_core", "c3sc_hip_cross_iteration_pi", "c3sc_hip_cross_confirm", "c3sc_hip_bellman_fibers_all", "c3sc_hip_policy_fibers_all", "c3sc_hip_cross_speculate", "c3sc_hip_comm_unique_id", "c3sc_hip_comm_create", "c3sc_hip_comm_destroy", "c3sc_hip_comm_world", "c3sc_hip_comm_rank", "c3sc_hip_comm_allgather", "c3sc_hip_cross_set_comm", "c3sc_hip_comm_exchange", "c3sc_hip_cross_options", "c3sc_hip_cross_grow_memo", "c3sc_hip_cross_fetch", "c3sc_hip_cross_free", "c3sc_hip_set_mca", "c3sc_hip_set_model",
    "c3sc_hip_set_controls", "c3sc_hip_upload_value", "c3sc_hip_upload_value_device", "c3sc_hip_set_variant",
    "c3sc_hip_bellman_fibers", "c3sc_hip_bellman_fibers_tables", "c3sc_hip_bellman_fibers_tables_host", "c3sc_hip_stencil_fibers", "c3sc_hip_bellman_fibers_host",
    "c3sc_hip_policy_fibers", "c3sc_hip_policy_fibers_host", "c3sc_hip_policy_fibers_tables", "c3sc_hip_policy_fibers_tables_host",
    "c3sc_hip_set_control_box", "c3sc_hip_bellman_fibers_box", "c3sc_hip_bellman_fibers_box_host", "c3sc_hip_policy_fibers_box",
    "c3sc_hip_policy_fibers_box_host",
    "c3sc_hip_stencil_fibers_host", "c3sc_hip_stencil_fibers_nb", "c3sc_hip_stencil_fibers_nb_host", "c3sc_hip_sync", "c3sc_hip_get_status", "c3sc_hip_last_kernel",
    "c3sc_hip_debug_read", "c3sc_hip_launch_count", "c3sc_hip_table3_launch_count", "c3sc_hip_last_partition", "c3sc_hip_timer_start", "c3sc_hip_timer_stop", "c3sc_hip_peak_fma_f64", "c3sc_hip_peak_mfma_f64",
    "c3sc_hip_set_interp", "c3sc_hip_stencil_points", "c3sc_hip_simulate", "c3sc_hip_simulate_host", "c3sc_hip_normals",
    "c3sc_hip_integrate", "c3sc_hip_integrate_host",
    "c3sc_hip_model_compile", "c3sc_hip_model_code_object", "c3sc_hip_model_log",
    "c3sc_hip_set_game", "c3sc_hip_model_compile_ex", "c3sc_hip_model_code_object_ex",
    "c3sc_hip_model_compile_fh", "c3sc_hip_model_code_object_fh", "c3sc_hip_set_horizon_step", "c3sc_hip_upload_value_stack",
    "c3sc_hip_model_compile_os", "c3sc_hip_model_code_object_os", "c3sc_hip_set_stopping",
    "c3sc_hip_model_compile_jd", "c3sc_hip_model_code_object_jd", "c3sc_hip_set_jumps", "c3sc_hip_jump_uniforms",
    "c3sc_hip_model_compile_ic", "c3sc_hip_model_code_object_ic", "c3sc_hip_set_impulses",
    "c3sc_hip_model_compile_cd", "c3sc_hip_model_code_object_cd", "c3sc_hip_set_correlation",
    "c3sc_hip_chain_transitions", "c3sc_hip_chain_transitions_host", "c3sc_hip_simulate_chain", "c3sc_hip_simulate_chain_host",
    "c3sc_hip_model_compile_mc", "c3sc_hip_model_code_object_mc", "c3sc_hip_chain_outcomes", "c3sc_hip_chain_outcomes_host",
    "c3sc_hip_model_has_chain",
]

class SimArgs(C.Structure):
    """struct c3sc_hip_sim_args (include/c3sc_hip.h)"""
    _fields_ = [("n", C.c_size_t), ("d_x0", C.c_void_p), ("dt", C.c_double), ("nsteps", C.c_size_t),
                ("traj_offset", C.c_uint64), ("seed", C.c_uint64), ("d_noise", C.c_void_p), ("wrap_periodic", C.c_int),
                ("box", C.c_int), ("steps_per_launch", C.c_int), ("save_every", C.c_size_t), ("d_traj", C.c_void_p),
                ("d_u", C.c_void_p), ("d_cost", C.c_void_p), ("d_exit", C.c_void_p), ("d_vend", C.c_void_p),
                ("d_xfinal", C.c_void_p)]


class ChainArgs(C.Structure):
    """struct c3sc_hip_chain_args (include/c3sc_hip.h)"""
    _fields_ = [("n", C.c_size_t), ("d_node0", C.c_void_p), ("nsteps", C.c_size_t), ("traj_offset", C.c_uint64),
                ("seed", C.c_uint64), ("d_uniform", C.c_void_p), ("steps_per_launch", C.c_int), ("save_every", C.c_size_t),
                ("d_cost", C.c_void_p), ("d_disc", C.c_void_p), ("d_time", C.c_void_p), ("d_vend", C.c_void_p),
                ("d_node", C.c_void_p), ("d_exit", C.c_void_p), ("d_traj", C.c_void_p), ("d_uidx", C.c_void_p)]


ODE_FORWARD_EULER, ODE_RK4 = 0, 1  # C3SC_ODE_*
_ODE_METHODS = {"forward-euler": ODE_FORWARD_EULER, "euler": ODE_FORWARD_EULER, "rk4": ODE_RK4}


class OdeArgs(C.Structure):
    """struct c3sc_hip_ode_args (include/c3sc_hip.h)"""
    _fields_ = [("n", C.c_size_t), ("d_x0", C.c_void_p), ("dt_out", C.c_double), ("dt_int", C.c_double), ("nout", C.c_size_t),
                ("method", C.c_int), ("wrap_periodic", C.c_int), ("box", C.c_int), ("evals_per_launch", C.c_int),
                ("goal", C.c_void_p), ("keep", C.c_void_p), ("save_every", C.c_size_t), ("d_traj", C.c_void_p),
                ("d_u", C.c_void_p), ("d_cost", C.c_void_p), ("d_stop_step", C.c_void_p), ("d_stop_reason", C.c_void_p),
                ("d_vend", C.c_void_p), ("d_xfinal", C.c_void_p)]


class ModelSpec(C.Structure):
    """struct c3sc_hip_model_spec (include/c3sc_hip.h)"""
    _fields_ = [("source", C.c_char_p), ("name", C.c_char_p), ("d", C.c_int), ("du", C.c_int), ("udep_mask", C.c_uint),
                ("uconst_mask", C.c_uint), ("stage_udep", C.c_int), ("box", C.c_int), ("nranks", C.c_int),
                ("ranks", C.POINTER(C.c_int))]


class ModelSpecEx(C.Structure):
    """struct c3sc_hip_model_spec_ex (include/c3sc_hip.h): the spec plus the game flag"""
    _fields_ = [("base", ModelSpec), ("game", C.c_int)]


class ModelSpecFh(C.Structure):
    """struct c3sc_hip_model_spec_fh (include/c3sc_hip.h): the _ex spec plus the horizon flag"""
    _fields_ = [("ex", ModelSpecEx), ("horizon", C.c_int)]


class ModelSpecOs(C.Structure):
    """struct c3sc_hip_model_spec_os (include/c3sc_hip.h): the _fh spec plus the stop flag"""
    _fields_ = [("fh", ModelSpecFh), ("stop", C.c_int)]


class ModelSpecJd(C.Structure):
    """struct c3sc_hip_model_spec_jd (include/c3sc_hip.h): the _os spec plus the number of jump marks"""
    _fields_ = [("os", ModelSpecOs), ("njump", C.c_int)]


JUMP_MAX = 8  # C3SC_JUMP_MAX: most atoms of a discretised mark distribution


class ModelSpecIc(C.Structure):
    """struct c3sc_hip_model_spec_ic (include/c3sc_hip.h): the _jd spec plus the number of interventions"""
    _fields_ = [("jd", ModelSpecJd), ("nimpulse", C.c_int)]


IMPULSE_MAX = 8  # C3SC_IMPULSE_MAX: most interventions of an impulse-control model

CORR_MAX = 8  # C3SC_CORR_MAX: most pairs of dimensions with a cross-diffusion term


class ModelSpecCd(C.Structure):
    """struct c3sc_hip_model_spec_cd (include/c3sc_hip.h): the _ic spec plus the pairs of correlated dimensions"""
    _fields_ = [("ic", ModelSpecIc), ("ncorr", C.c_int), ("corr_dims", C.c_int * (2 * CORR_MAX))]


class ModelSpecMc(C.Structure):
    """struct c3sc_hip_model_spec_mc (include/c3sc_hip.h): the _cd spec plus the chain flag"""
    _fields_ = [("cd", ModelSpecCd), ("chain", C.c_int)]


STATUS_STATIONARY, STATUS_CFL, STATUS_DOMINANCE = 1, 2, 4  # C3SC_STATUS_*


MODEL_USER = 1000  # C3SC_MODEL_USER: first id of the run-time compiled models
GAME_MINMAX, GAME_MAXMIN = 0, 1  # C3SC_GAME_*: upper value (min over u of max over w), lower value (max over w of min over u)
_GAME_ORDERS = {"minmax": GAME_MINMAX, "upper": GAME_MINMAX, "maxmin": GAME_MAXMIN, "lower": GAME_MAXMIN}

VARIANT_AUTO, VARIANT_FIBER_PER_WAVE, VARIANT_FIBER_PER_LANE, VARIANT_FIBER_PAIR, VARIANT_FIBER_QUAD = 0, 1, 2, 3, 4


class C3scHipError(RuntimeError):
    pass


def load_library():
    """Load libc3sc_hip.so or fail loudly (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise C3scHipError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C c3sc_amd/csrc`.  There is no CPU fallback.")
        # PyTorch bundles its own libamdhip64.so.7; load it FIRST so that this library binds to the same
        # HIP runtime instance (two runtimes in one process cannot both own the GPU).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.c3sc_hip_last_error.restype = C.c_char_p
        L.c3sc_hip_last_error.argtypes = [C.c_void_p]
        L.c3sc_hip_last_kernel.restype = C.c_char_p
        L.c3sc_hip_last_kernel.argtypes = [C.c_void_p]
        L.c3sc_hip_ctx_destroy.restype = None
        L.c3sc_hip_ctx_destroy.argtypes = [C.c_void_p]
        L.c3sc_hip_bellman_fibers.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.c3sc_hip_stencil_fibers.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        L.c3sc_hip_bellman_fibers_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        L.c3sc_hip_stencil_fibers_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.c3sc_hip_policy_fibers.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
        L.c3sc_hip_policy_fibers_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        L.c3sc_hip_stencil_fibers_nb_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]
        L.c3sc_hip_bellman_fibers_tables_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 6
        L.c3sc_hip_policy_fibers_tables_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 6
        L.c3sc_hip_launch_count.restype = C.c_ulonglong
        L.c3sc_hip_table3_launch_count.restype = C.c_ulonglong
        L.c3sc_hip_last_partition.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.c3sc_hip_sync.argtypes = [C.c_void_p, C.c_void_p]
        L.c3sc_hip_timer_start.argtypes = [C.c_void_p, C.c_void_p]
        L.c3sc_hip_timer_stop.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.c3sc_hip_upload_value_device.argtypes = [C.c_void_p, c_size_p, C.POINTER(C.c_void_p), C.c_void_p]
        # device-resident cross (include/c3sc_hip.h); index sets are int32 tuple arrays, one pointer per core step
        L.c3sc_hip_cross_setup.argtypes = [C.c_void_p, c_size_p, C.POINTER(c_i32_p), C.POINTER(c_i32_p), C.c_int]
        L.c3sc_hip_cross_iteration.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.c3sc_hip_cross_confirm.argtypes = [C.c_void_p, c_int_p, C.c_void_p]
        L.c3sc_hip_cross_options.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.c3sc_hip_cross_iteration_pi.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.c3sc_hip_cross_grow_memo.argtypes = [C.c_void_p]
        L.c3sc_hip_cross_fetch.argtypes = [C.c_void_p, C.POINTER(c_double_p), C.POINTER(c_i32_p), C.POINTER(c_i32_p),
                                           C.POINTER(C.c_ulonglong), C.c_void_p]
        L.c3sc_hip_set_interp.argtypes = [C.c_void_p, C.c_int]
        L.c3sc_hip_stencil_points.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.c3sc_hip_simulate.argtypes = [C.c_void_p, C.POINTER(SimArgs), C.c_void_p]
        L.c3sc_hip_integrate.argtypes = [C.c_void_p, C.POINTER(OdeArgs), C.c_void_p]
        L.c3sc_hip_chain_transitions.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 8
        L.c3sc_hip_chain_transitions_host.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 7
        L.c3sc_hip_simulate_chain.argtypes = [C.c_void_p, C.POINTER(ChainArgs), C.c_void_p]
        L.c3sc_hip_simulate_chain_host.argtypes = [C.c_void_p, C.POINTER(ChainArgs)]
        L.c3sc_hip_integrate_host.argtypes = [C.c_void_p, C.POINTER(OdeArgs)]
        L.c3sc_hip_normals.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t, C.c_uint64, C.c_size_t, C.c_int, c_double_p]
        L.c3sc_hip_model_compile.argtypes = [C.POINTER(ModelSpec), c_int_p]
        L.c3sc_hip_model_code_object.argtypes = [C.POINTER(ModelSpec), C.c_void_p, c_size_p]
        L.c3sc_hip_model_log.restype = C.c_char_p
        L.c3sc_hip_model_log.argtypes = []
        L.c3sc_hip_model_compile_ex.argtypes = [C.POINTER(ModelSpecEx), c_int_p]
        L.c3sc_hip_model_code_object_ex.argtypes = [C.POINTER(ModelSpecEx), C.c_void_p, c_size_p]
        L.c3sc_hip_set_game.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, C.c_int, c_double_p, C.c_int]
        L.c3sc_hip_model_compile_fh.argtypes = [C.POINTER(ModelSpecFh), c_int_p]
        L.c3sc_hip_model_code_object_fh.argtypes = [C.POINTER(ModelSpecFh), C.c_void_p, c_size_p]
        L.c3sc_hip_set_horizon_step.argtypes = [C.c_void_p, C.c_double]
        L.c3sc_hip_upload_value_stack.argtypes = [C.c_void_p, C.c_int, c_size_p, C.POINTER(c_double_p)]
        L.c3sc_hip_model_compile_os.argtypes = [C.POINTER(ModelSpecOs), c_int_p]
        L.c3sc_hip_model_code_object_os.argtypes = [C.POINTER(ModelSpecOs), C.c_void_p, c_size_p]
        L.c3sc_hip_set_stopping.argtypes = [C.c_void_p, C.c_int]
        L.c3sc_hip_model_compile_jd.argtypes = [C.POINTER(ModelSpecJd), c_int_p]
        L.c3sc_hip_model_code_object_jd.argtypes = [C.POINTER(ModelSpecJd), C.c_void_p, c_size_p]
        L.c3sc_hip_set_jumps.argtypes = [C.c_void_p, C.c_int]
        L.c3sc_hip_jump_uniforms.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, c_double_p]
        L.c3sc_hip_model_compile_ic.argtypes = [C.POINTER(ModelSpecIc), c_int_p]
        L.c3sc_hip_model_code_object_ic.argtypes = [C.POINTER(ModelSpecIc), C.c_void_p, c_size_p]
        L.c3sc_hip_set_impulses.argtypes = [C.c_void_p, C.c_int]
        L.c3sc_hip_model_compile_cd.argtypes = [C.POINTER(ModelSpecCd), c_int_p]
        L.c3sc_hip_model_code_object_cd.argtypes = [C.POINTER(ModelSpecCd), C.c_void_p, c_size_p]
        L.c3sc_hip_set_correlation.argtypes = [C.c_void_p, C.c_int]
        L.c3sc_hip_model_compile_mc.argtypes = [C.POINTER(ModelSpecMc), c_int_p]
        L.c3sc_hip_model_code_object_mc.argtypes = [C.POINTER(ModelSpecMc), C.c_void_p, c_size_p]
        L.c3sc_hip_chain_outcomes.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 11
        L.c3sc_hip_chain_outcomes_host.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 10
        _LIB = L
    return _LIB


def normals(seed: int, traj0: int, ntraj: int, step0: int, nsteps: int, dw: int) -> np.ndarray:
    """Host twin of the rollouts' noise (c3sc_hip_normals): (ntraj, nsteps, dw) standard normals, the device's bits."""
    L = load_library()
    out = np.empty((ntraj, nsteps, dw), dtype=np.float64)
    rc = L.c3sc_hip_normals(C.c_uint64(seed), C.c_uint64(traj0), C.c_size_t(ntraj), C.c_uint64(step0), C.c_size_t(nsteps),
                            C.c_int(dw), out.ctypes.data_as(c_double_p))
    if rc != 0:
        raise C3scHipError(f"c3sc_hip_normals failed (code {rc})")
    return out


def _model_spec(source, d, du, ranks, box, udep_mask, uconst_mask, stage_udep, name):
    rk = (C.c_int * max(1, len(ranks)))(*ranks)
    spec = ModelSpec(source.encode(), name.encode() if name is not None else None, int(d), int(du), int(udep_mask),
                     int(uconst_mask), 1 if stage_udep else 0, 1 if box else 0, len(ranks), rk if len(ranks) else None)
    spec._keep = rk
    return spec


def _form_spec(spec, game, horizon, stop, njump, nimpulse, corr_pairs, chain=0):
    """The shallowest of the nested spec structs that carries the request, and the suffix of the entry points that take it
    ("", "_ex", "_fh", "_os", "_jd", "_ic", "_cd": c3sc_hip_model_compile<suffix>, c3sc_hip_model_code_object<suffix>).  The
    pair list is passed as given (the library validates it), cut at CORR_MAX + 1 pairs' count."""
    pairs = [(int(i), int(j)) for i, j in corr_pairs]
    levels = [(ModelSpecEx, "_ex", 1 if game else 0), (ModelSpecFh, "_fh", 1 if horizon else 0), (ModelSpecOs, "_os", 1 if stop else 0),
              (ModelSpecJd, "_jd", int(njump)), (ModelSpecIc, "_ic", int(nimpulse)), (ModelSpecCd, "_cd", len(pairs)),
              (ModelSpecMc, "_mc", int(chain))]
    depth = max((q + 1 for q, (_, _, v) in enumerate(levels) if v), default=0)
    suffix = ""
    for struct, suffix, v in levels[:depth]:
        spec = struct(spec, v)
        if struct is ModelSpecCd:
            for p, (i, j) in enumerate(pairs[:CORR_MAX]):
                spec.corr_dims[2 * p], spec.corr_dims[2 * p + 1] = i, j
    return spec, suffix


def _model_fail(rc, what):
    log = load_library().c3sc_hip_model_log().decode(errors="replace")
    raise C3scHipError(f"{what} failed (code {rc}): {log}", rc)


def compile_model(source: str, d: int, du: int, ranks=(4, 8), box: bool = False, udep_mask: int = 0, uconst_mask: int = 0,
                  stage_udep: bool = True, name: Optional[str] = None, game: bool = False, horizon: bool = False,
                  stop: bool = False, njump: int = 0, nimpulse: int = 0, corr_pairs=(), chain=False) -> int:
    """Compile a device model from source (c3sc_hip_model_compile, include/c3sc_hip.h states the source contract) and return
    its model id (>= MODEL_USER), usable wherever a built-in model id is.  No GPU is needed.  Raises C3scHipError with the
    compiler's log on failure; the error code is args[1].  game=True (c3sc_hip_model_compile_ex) adds the game kernels that
    BellmanEngine.set_game needs: the control vector is then (u, w) of the two players.  horizon=True
    (c3sc_hip_model_compile_fh) adds the finite-horizon kernels that BellmanEngine.set_horizon_step needs.  stop=True
    (c3sc_hip_model_compile_os) adds the stop kernels that BellmanEngine.set_stopping needs: the source then defines stopcost.
    njump=M > 0 (c3sc_hip_model_compile_jd) adds the jump kernels that BellmanEngine.set_jumps needs: the source then defines
    jumprate and jump for M marks.  nimpulse=M > 0 (c3sc_hip_model_compile_ic) adds the impulse kernels that
    BellmanEngine.set_impulses needs: the source then defines impulse for M interventions.  corr_pairs=[(i, j), ...]
    (c3sc_hip_model_compile_cd) adds the corr kernels that BellmanEngine.set_correlation needs: the source then defines covar for
    these pairs of dimensions, i < j.  chain=True (c3sc_hip_model_compile_mc) adds the Markov-chain kernels that
    BellmanEngine.simulate_chain, chain_transitions and chain_outcomes need, in the plain form and in every combination of the
    horizon, stop and jump features asked for here; chain=False is the model without the flag."""
    L = load_library()
    base = _model_spec(source, d, du, tuple(ranks), box, udep_mask, uconst_mask, stage_udep, name)
    spec, suffix = _form_spec(base, game, horizon, stop, njump, nimpulse, corr_pairs, chain)
    mid = C.c_int(0)
    rc = getattr(L, "c3sc_hip_model_compile" + suffix)(C.byref(spec), C.byref(mid))
    if rc != 0:
        _model_fail(rc, "c3sc_hip_model_compile")
    return mid.value


def code_object(source: str, d: int, du: int, ranks=(4, 8), box: bool = False, udep_mask: int = 0, uconst_mask: int = 0,
                stage_udep: bool = True, name: Optional[str] = None, game: bool = False, horizon: bool = False,
                stop: bool = False, njump: int = 0, nimpulse: int = 0, corr_pairs=(), chain=False) -> bytes:
    """The gfx950 code object of this spec (c3sc_hip_model_code_object): the loaded one if compile_model already compiled the
    spec, otherwise what compile_model would build now (its id and default name are in the kernel names), compiled and not
    registered.  game, horizon, stop, njump and nimpulse select the spec as in compile_model (stop: c3sc_hip_model_code_object_os,
    njump: c3sc_hip_model_code_object_jd, nimpulse: c3sc_hip_model_code_object_ic, corr_pairs: c3sc_hip_model_code_object_cd,
    chain: c3sc_hip_model_code_object_mc)."""
    L = load_library()
    base = _model_spec(source, d, du, tuple(ranks), box, udep_mask, uconst_mask, stage_udep, name)
    spec, suffix = _form_spec(base, game, horizon, stop, njump, nimpulse, corr_pairs, chain)
    cap = 16 << 20  # one compile when the code object fits; a larger one is compiled again into a buffer of its size
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        size = C.c_size_t(cap)
        rc = getattr(L, "c3sc_hip_model_code_object" + suffix)(C.byref(spec), buf, C.byref(size))
        if rc == 0:
            return buf.raw[:size.value]
        if size.value <= cap:
            break
        cap = size.value
    _model_fail(rc, "c3sc_hip_model_code_object")


def game_split(index, nw: int):
    """A reported game index (iu * nw + iw; -1 on absorbed nodes) as (iu, iw); works elementwise on arrays (-1 -> (-1, -1))."""
    i = np.asarray(index)
    iu = np.where(i < 0, -1, i // nw)
    iw = np.where(i < 0, -1, i % nw)
    if np.ndim(index) == 0:
        return int(iu), int(iw)
    return iu, iw


def decode_exit(exit_step):
    """d_exit of a rollout with stopping on (c3sc_hip_set_stopping) as (step, stopped): an exit at step k >= 0 is (k, 0), a
    voluntary stop stored as -(k + 2) is (k, 1), never (-1) is (-1, 0); works elementwise on arrays."""
    e = np.asarray(exit_step)
    stopped = e <= -2
    step = np.where(stopped, -e - 2, e)
    if np.ndim(exit_step) == 0:
        return int(step), int(stopped)
    return step, stopped.astype(np.int32)


def decode_action(uidx, ncand: int):
    """A reported action index as (kind, index): 0 .. ncand-1 is ("control", i), ncand ("stop", 0), ncand + 1 + m
    ("impulse", m) (c3sc_hip_set_impulses), -1 on absorbed nodes ("absorbed", -1).  On arrays: kind as an array of strings."""
    i = np.asarray(uidx)
    kind = np.where(i < 0, "absorbed", np.where(i < ncand, "control", np.where(i == ncand, "stop", "impulse")))
    idx = np.where(i < 0, -1, np.where(i < ncand, i, np.where(i == ncand, 0, i - ncand - 1)))
    if np.ndim(uidx) == 0:
        return str(kind), int(idx)
    return kind, idx


def decode_chain_exit(exit_step):
    """d_exit of a chain walk (c3sc_hip_simulate_chain) as (step, kind): -1 is (-1, "running"), s >= 0 is (s, "exit") -- an absorbed
    or obstacle node at step s, or with jumps on a jump out at step s - 1 -- -(s + 2) is (s, "stuck") and -(s + 2) - 2^32
    (C3SC_CHAIN_STOPPED) is (s, "stopped"); works elementwise on arrays."""
    e = np.asarray(exit_step)
    stopped = e <= -2 - (1 << 32)
    stuck = (e <= -2) & ~stopped
    step = np.where(stopped, -e - 2 - (1 << 32), np.where(stuck, -e - 2, e))
    kind = np.where(stopped, "stopped", np.where(stuck, "stuck", np.where(e >= 0, "exit", "running")))
    if np.ndim(exit_step) == 0:
        return int(step), str(kind)
    return step, kind


def jump_uniforms(seed: int, traj: int, step: int):
    """(u0, u1) of c3sc_hip_jump_uniforms: the event and mark uniforms of one rollout step (no GPU needed)"""
    out = (C.c_double * 2)()
    rc = load_library().c3sc_hip_jump_uniforms(C.c_uint64(seed), C.c_uint64(traj), C.c_uint64(step), out)
    if rc != 0:
        raise C3scHipError(f"jump_uniforms failed (code {rc})")
    return float(out[0]), float(out[1])


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr_array(arrs):
    arr = (c_double_p * len(arrs))(*[a.ctypes.data_as(c_double_p) for a in arrs])
    arr._keep = arrs
    return arr


class BellmanEngine:
    """Device-resident Bellman-backup problem: the HIP counterpart of C3Control + VIparam
    (src/bellman.c:1942-1999, 1132-1180) for one GPU."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.c3sc_hip_ctx_create(C.c_int(device), C.byref(h))
        if rc != 0:
            raise C3scHipError(f"c3sc_hip_ctx_create(device={device}) failed with code {rc} (no usable HIP device?)")
        self.h = h
        self.device = device
        self.w = None
        self.stopping = False
        self.jumps = False
        self.impulses = False
        self.correlation = False

    def close(self):
        if getattr(self, "h", None):
            self.L.c3sc_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.L.c3sc_hip_last_error(self.h)
            raise C3scHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    # ------------------------------------------------------------------ problem description
    def set_grid(self, ngrid: Sequence[int], xgrid: Sequence[np.ndarray]):
        ng = np.ascontiguousarray(ngrid, dtype=np.uintp)
        xs = [_f64(g) for g in xgrid]
        self._chk(self.L.c3sc_hip_set_grid(self.h, C.c_int(len(ng)), ng.ctypes.data_as(c_size_p), _ptr_array(xs)),
                  "set_grid")
        self.ngrid = [int(n) for n in ngrid]
        self.d = len(self.ngrid)

    def set_boundary(self, bctype: Sequence[int], obstacles=()):
        bc = np.ascontiguousarray(bctype, dtype=np.int32)
        lb = _f64([[c - wd / 2.0 for c, wd in zip(cen, wid)] for cen, wid in obstacles]).reshape(-1)
        ub = _f64([[c + wd / 2.0 for c, wd in zip(cen, wid)] for cen, wid in obstacles]).reshape(-1)
        self._chk(self.L.c3sc_hip_set_boundary(self.h, bc.ctypes.data_as(c_int_p), C.c_int(len(obstacles)),
                                               lb.ctypes.data_as(c_double_p), ub.ctypes.data_as(c_double_p)),
                  "set_boundary")

    def set_mca(self, h2: float, t: Sequence[float], discount: float):
        tv = _f64(t)
        self._chk(self.L.c3sc_hip_set_mca(self.h, C.c_double(h2), tv.ctypes.data_as(c_double_p), C.c_double(discount)),
                  "set_mca")

    def set_model(self, model: int, params: Sequence[float] = ()):
        p = _f64(list(params) if len(params) else [0.0])
        self._chk(self.L.c3sc_hip_set_model(self.h, C.c_int(model), p.ctypes.data_as(c_double_p), C.c_int(len(params))),
                  "set_model")

    def set_controls(self, cands: np.ndarray):
        cd = _f64(cands)
        self._chk(self.L.c3sc_hip_set_controls(self.h, C.c_int(cd.shape[0]), C.c_int(cd.shape[1]),
                                               cd.ctypes.data_as(c_double_p)), "set_controls")

    def set_game(self, U: np.ndarray, W: np.ndarray, order="minmax"):
        """Zero-sum game over the product of the minimiser's list U (nu, du_min) and the maximiser's W (nw, du_max)
        (c3sc_hip_set_game): order "minmax" (upper value) or "maxmin" (lower value).  The model must be compiled with game=True
        and du = du_min + du_max.  Reported indices are iu * nw + iw (game_split).  set_controls ends game mode."""
        u, w = _f64(np.atleast_2d(U)), _f64(np.atleast_2d(W))
        o = _GAME_ORDERS[order] if isinstance(order, str) else int(order)
        self._chk(self.L.c3sc_hip_set_game(self.h, C.c_int(u.shape[1]), C.c_int(u.shape[0]), u.ctypes.data_as(c_double_p),
                                           C.c_int(w.shape[0]), w.ctypes.data_as(c_double_p), C.c_int(o)), "set_game")
        self.game_nw = w.shape[0]

    def clear_game(self):
        self._chk(self.L.c3sc_hip_set_game(self.h, 0, 0, None, 0, None, 0), "set_game")

    def set_horizon_step(self, dt: float):
        """Finite-horizon mode (c3sc_hip_set_horizon_step): the Bellman calls apply Kushner's explicit scheme with the fixed step
        dt, one stage back from the uploaded value; dt = 0 ends it.  The model must be compiled with horizon=True."""
        self._chk(self.L.c3sc_hip_set_horizon_step(self.h, C.c_double(dt)), "set_horizon_step")
        self.horizon_dt = float(dt)

    def set_stopping(self, on: bool = True):
        """Optimal stopping (c3sc_hip_set_stopping): the Bellman calls add the stop action (index ncand, cost stopcost(x)) to
        the scan, and simulate stops a trajectory where the controller picks it (decode_exit).  The model must be compiled with
        stop=True, and with horizon=True as well to combine it with set_horizon_step."""
        self._chk(self.L.c3sc_hip_set_stopping(self.h, C.c_int(1 if on else 0)), "set_stopping")
        self.stopping = bool(on)

    def set_jumps(self, on: bool = True):
        """Jump diffusions (c3sc_hip_set_jumps): the Bellman calls add the Poisson jump term h^2 lambda(x) (J(x) - V) to the
        backup, J the mark average of the value at the jump targets, and simulate adds a compound-Poisson increment to every
        step (jump_uniforms is the host twin of its two uniforms).  The model must be compiled with njump=M > 0, and with
        horizon / stop as well to combine it with set_horizon_step / set_stopping."""
        self._chk(self.L.c3sc_hip_set_jumps(self.h, C.c_int(1 if on else 0)), "set_jumps")
        self.jumps = bool(on)

    def set_correlation(self, on: bool = True):
        """Correlated noise (c3sc_hip_set_correlation): the Bellman calls add the cross-diffusion terms of the model's pairs, two
        diagonal neighbours per pair, to the backup; status() may then carry STATUS_DOMINANCE.  The model must be compiled with
        corr_pairs, and with horizon / stop / njump as well to combine it with those switches.  simulate and integrate are
        refused while it is on."""
        self._chk(self.L.c3sc_hip_set_correlation(self.h, C.c_int(1 if on else 0)), "set_correlation")
        self.correlation = bool(on)

    def set_impulses(self, on: bool = True):
        """Impulse control (c3sc_hip_set_impulses): the Bellman calls compare the candidates' result with the best intervention
        min_m [k_m(x) + V(y_m(x))], reported as the index ncand + 1 + m (decode_action), and simulate moves a trajectory whose
        controller intervenes to y_m in one step slot.  The model must be compiled with nimpulse=M > 0, and with njump as well
        to combine it with set_jumps; not offered with games, the horizon step or stopping."""
        self._chk(self.L.c3sc_hip_set_impulses(self.h, C.c_int(1 if on else 0)), "set_impulses")
        self.impulses = bool(on)

    def upload_value_stack(self, ranks, cores):
        """V_0 .. V_N for simulate in horizon mode (c3sc_hip_upload_value_stack): ranks[s] is stage s's rank list (d + 1 entries),
        cores[s] its d cores in upload_value's layout.  An empty list frees the stack."""
        ns = len(ranks)
        if ns == 0:
            self._chk(self.L.c3sc_hip_upload_value_stack(self.h, 0, None, None), "upload_value_stack")
            return
        rk = np.ascontiguousarray(np.asarray(ranks).reshape(ns, -1), dtype=np.uintp)
        cs = [_f64(c) for stage in cores for c in stage]
        self._chk(self.L.c3sc_hip_upload_value_stack(self.h, C.c_int(ns), rk.ctypes.data_as(c_size_p), _ptr_array(cs)),
                  "upload_value_stack")

    def set_variant(self, variant: int):
        self._chk(self.L.c3sc_hip_set_variant(self.h, C.c_int(variant)), "set_variant")

    def set_consistent_ends(self, on: bool):
        """Not the reference's rule (default off): end points of reflecting / periodic fibers keep their absorbed flags."""
        self._chk(self.L.c3sc_hip_set_consistent_ends(self.h, C.c_int(1 if on else 0)), "set_consistent_ends")

    def upload_value(self, ranks: Sequence[int], cores: Sequence[np.ndarray]):
        rk = np.ascontiguousarray(ranks, dtype=np.uintp)
        cs = [_f64(c) for c in cores]
        self._chk(self.L.c3sc_hip_upload_value(self.h, rk.ctypes.data_as(c_size_p), _ptr_array(cs)), "upload_value")
        self.ranks = [int(r) for r in ranks]

    def upload_value_device(self, ranks: Sequence[int], core_tensors, stream_ptr: int = 0):
        """cores already on this GPU (torch float64 tensors in the reference layout)."""
        rk = np.ascontiguousarray(ranks, dtype=np.uintp)
        ptrs = (C.c_void_p * len(core_tensors))(*[C.c_void_p(t.data_ptr()) for t in core_tensors])
        self._chk(self.L.c3sc_hip_upload_value_device(self.h, rk.ctypes.data_as(c_size_p), ptrs, C.c_void_p(stream_ptr)),
                  "upload_value_device")
        self.ranks = [int(r) for r in ranks]

    def configure(self, w, cores=None):
        """Everything from a c3sc_amd.workloads.Workload.  Grid constants follow c3control_create /
        mca_add_grid_refs (src/bellman.c:1972-1986, 171-188)."""
        xg = w.xgrid()
        self.set_grid(w.ngrid, xg)
        self.set_boundary(w.bc, w.obstacles)
        hs = [g[1] - g[0] for g in xg]
        hmin = w.ub[0] - w.lb[0]
        for h in hs:
            if h < hmin:
                hmin = h
        h2 = hmin * hmin
        t = []
        for h in hs:
            t0 = h2 / h
            t += [t0, t0 / h]
        self.set_mca(h2, t, w.discount)
        self.set_model(w.model, w.params)
        self.set_controls(w.cands)
        self.w = w
        if cores is not None:
            self.upload_value(w.ranks, cores)

    # ------------------------------------------------------------------ the hot path
    def bellman_fibers(self, k: int, idx_t, out_t=None, uidx_t=None, absorbed_t=None, stream_ptr: Optional[int] = None):
        """Device API: idx_t int32 CUDA tensor (F, d); returns/reuses float64 CUDA tensor (F, N_k)."""
        import torch

        assert idx_t.is_cuda and idx_t.dtype == torch.int32 and idx_t.is_contiguous()
        F = idx_t.shape[0]
        N = self.ngrid[k]
        if out_t is None:
            out_t = torch.empty((F, N), dtype=torch.float64, device=idx_t.device)
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(idx_t.device).cuda_stream
        self._chk(self.L.c3sc_hip_bellman_fibers(self.h, k, F, idx_t.data_ptr(), out_t.data_ptr(),
                                                 uidx_t.data_ptr() if uidx_t is not None else None,
                                                 absorbed_t.data_ptr() if absorbed_t is not None else None,
                                                 stream_ptr), "bellman_fibers")
        return out_t

    def bellman_fibers_all(self, ks, idx_ts, out_ts, stream_ptr: Optional[int] = None, policy_ts=None):
        """Device API, several varying dimensions of one batch in one call (c3sc_hip_bellman_fibers_all / _policy_fibers_all): one
        launch where a fused instantiation exists.  idx_ts[s]: int32 CUDA tensor (F_s, d); out_ts[s]: float64 (F_s, N_ks[s])."""
        import torch

        nk = len(ks)
        KS = (C.c_int * nk)(*[int(k) for k in ks])
        FS = (C.c_size_t * nk)(*[int(t.shape[0]) for t in idx_ts])
        IDX = (C.c_void_p * nk)(*[t.data_ptr() for t in idx_ts])
        OUT = (C.c_void_p * nk)(*[t.data_ptr() for t in out_ts])
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(idx_ts[0].device).cuda_stream
        if policy_ts is None:
            self._chk(self.L.c3sc_hip_bellman_fibers_all(self.h, nk, KS, FS, IDX, OUT, None, None, C.c_void_p(stream_ptr)), "bellman_fibers_all")
        else:
            POL = (C.c_void_p * nk)(*[t.data_ptr() for t in policy_ts])
            self._chk(self.L.c3sc_hip_policy_fibers_all(self.h, nk, KS, FS, IDX, POL, OUT, None, C.c_void_p(stream_ptr)), "policy_fibers_all")
        return out_ts

    def stencil_fibers(self, k: int, idx_t, costs_t=None, absorbed_t=None, stream_ptr: Optional[int] = None):
        import torch

        assert idx_t.is_cuda and idx_t.dtype == torch.int32 and idx_t.is_contiguous()
        F = idx_t.shape[0]
        N = self.ngrid[k]
        if costs_t is None:
            costs_t = torch.empty((F, N, 2 * self.d + 1), dtype=torch.float64, device=idx_t.device)
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(idx_t.device).cuda_stream
        self._chk(self.L.c3sc_hip_stencil_fibers(self.h, k, F, idx_t.data_ptr(), costs_t.data_ptr(),
                                                 absorbed_t.data_ptr() if absorbed_t is not None else None,
                                                 stream_ptr), "stencil_fibers")
        return costs_t

    # ------------------------------------------------------------------ closed-loop rollouts of the implicit policy
    def set_interp(self, constelm: bool):
        """Off-grid evaluation as a CONSTELM value function (nearest node per dimension) instead of multilinear."""
        self._chk(self.L.c3sc_hip_set_interp(self.h, C.c_int(1 if constelm else 0)), "set_interp")

    def stencil_points(self, x_t, out_t=None, absorbed_t=None, stream_ptr: Optional[int] = None):
        """Device API (c3sc_hip_stencil_points): x_t float64 CUDA tensor (n, d) of arbitrary states; returns
        (values (n, 2d+1), absorbed int32 (n,)) -- mca_get_neighbor_node_costs per state."""
        import torch

        assert x_t.is_cuda and x_t.dtype == torch.float64 and x_t.is_contiguous() and x_t.shape[1] == self.d
        n = x_t.shape[0]
        if out_t is None:
            out_t = torch.empty((n, 2 * self.d + 1), dtype=torch.float64, device=x_t.device)
        if absorbed_t is None:
            absorbed_t = torch.empty((n,), dtype=torch.int32, device=x_t.device)
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(x_t.device).cuda_stream
        self._chk(self.L.c3sc_hip_stencil_points(self.h, n, x_t.data_ptr(), out_t.data_ptr(), absorbed_t.data_ptr(),
                                                 C.c_void_p(stream_ptr)), "stencil_points")
        return out_t, absorbed_t

    def simulate(self, x0_t, dt: float, nsteps: int, seed: int = 0, noise_t=None, wrap_periodic: bool = False,
                 save_every: int = 0, traj_offset: int = 0, box: bool = False, steps_per_launch: int = 0,
                 stream_ptr: Optional[int] = None):
        """Device API (c3sc_hip_simulate): x0_t float64 CUDA tensor (n, d).  Returns a dict of CUDA tensors: cost (n,),
        exit (int64, -1 = never), vend (n,), xfinal (n, d) and, with save_every > 0, traj (n, nsteps//save_every + 1, d)
        and u (n, ceil(nsteps/save_every), du).  noise_t: float64 (n, nsteps, d) standard normals, else Philox(seed).
        In horizon mode (set_horizon_step, upload_value_stack) dt must be the horizon step, step k's controller uses V_{k+1},
        and cost includes the discounted terminal value V_nsteps(x_nsteps) of the trajectories still alive."""
        import torch

        assert x0_t.is_cuda and x0_t.dtype == torch.float64 and x0_t.is_contiguous() and x0_t.shape[1] == self.d
        n, d, dev = x0_t.shape[0], self.d, x0_t.device
        du = getattr(self, "box_du", self.w.du) if box else self.w.du
        res = {"cost": torch.empty((n,), dtype=torch.float64, device=dev),
               "exit": torch.empty((n,), dtype=torch.int64, device=dev),
               "vend": torch.empty((n,), dtype=torch.float64, device=dev),
               "xfinal": torch.empty((n, d), dtype=torch.float64, device=dev)}
        a = SimArgs()
        a.n, a.d_x0, a.dt, a.nsteps = n, x0_t.data_ptr(), float(dt), int(nsteps)
        a.traj_offset, a.seed, a.wrap_periodic, a.box = int(traj_offset), int(seed), int(bool(wrap_periodic)), int(bool(box))
        a.steps_per_launch, a.save_every = int(steps_per_launch), int(save_every)
        if noise_t is not None:
            assert noise_t.is_cuda and noise_t.dtype == torch.float64 and noise_t.is_contiguous()
            assert tuple(noise_t.shape) == (n, nsteps, d)
            a.d_noise = noise_t.data_ptr()
        if save_every > 0:
            res["traj"] = torch.empty((n, nsteps // save_every + 1, d), dtype=torch.float64, device=dev)
            res["u"] = torch.empty((n, (nsteps + save_every - 1) // save_every, du), dtype=torch.float64, device=dev)
            a.d_traj, a.d_u = res["traj"].data_ptr(), res["u"].data_ptr()
        a.d_cost, a.d_exit, a.d_vend, a.d_xfinal = (res["cost"].data_ptr(), res["exit"].data_ptr(), res["vend"].data_ptr(),
                                                    res["xfinal"].data_ptr())
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        self._chk(self.L.c3sc_hip_simulate(self.h, C.byref(a), C.c_void_p(stream_ptr)), "simulate")
        return res

    def simulate_rc(self, args: "SimArgs", stream_ptr: int = 0) -> int:
        """c3sc_hip_simulate's return code as is (for callers that check the error codes)."""
        return int(self.L.c3sc_hip_simulate(self.h, C.byref(args), C.c_void_p(stream_ptr)))

    # ------------------------------------------------------------------ the approximating Markov chain
    def chain_transitions(self, nodes_t, stream_ptr: Optional[int] = None):
        """Device API (c3sc_hip_chain_transitions): nodes_t int32 CUDA tensor (n, d) of multi-indices.  Returns a dict of CUDA
        tensors: uidx int32 (n,) the greedy candidate (-1 on absorbed, obstacle and stuck nodes), value, stage, dt (n,),
        P (n, 2d) the transition probabilities in stencil order (lo, hi per dimension) and flag int32 (n,): 1 absorbing face,
        -1 obstacle, 0 live."""
        import torch

        assert nodes_t.is_cuda and nodes_t.dtype == torch.int32 and nodes_t.is_contiguous() and nodes_t.shape[1] == self.d
        n, d, dev = nodes_t.shape[0], self.d, nodes_t.device
        f64 = dict(dtype=torch.float64, device=dev)
        res = {"uidx": torch.empty((n,), dtype=torch.int32, device=dev), "value": torch.empty((n,), **f64),
               "stage": torch.empty((n,), **f64), "dt": torch.empty((n,), **f64), "P": torch.empty((n, 2 * d), **f64),
               "flag": torch.empty((n,), dtype=torch.int32, device=dev)}
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        self._chk(self.L.c3sc_hip_chain_transitions(self.h, n, nodes_t.data_ptr(), res["uidx"].data_ptr(), res["value"].data_ptr(),
                                                    res["stage"].data_ptr(), res["dt"].data_ptr(), res["P"].data_ptr(),
                                                    res["flag"].data_ptr(), C.c_void_p(stream_ptr)), "chain_transitions")
        return res

    def chain_transitions_host(self, nodes: np.ndarray):
        """c3sc_hip_chain_transitions_host: the same on numpy arrays (nodes int32 (n, d)), staged through device memory."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        n, d = nodes.shape[0], self.d
        res = {"uidx": np.empty((n,), np.int32), "value": np.empty((n,)), "stage": np.empty((n,)), "dt": np.empty((n,)),
               "P": np.empty((n, 2 * d)), "flag": np.empty((n,), np.int32)}
        self._chk(self.L.c3sc_hip_chain_transitions_host(self.h, n, nodes.ctypes.data, *[res[k].ctypes.data for k in
                                                                                          ("uidx", "value", "stage", "dt", "P", "flag")]),
                  "chain_transitions_host")
        return res

    def chain_outcomes(self, nodes_t, njump: int = 0, stream_ptr: Optional[int] = None):
        """Device API (c3sc_hip_chain_outcomes; models compiled with chain=True): chain_transitions' dict plus pself (n,), the
        self-loop's probability (horizon mode, else 0), and with njump = M > 0 (jumps on) pmark (n, M), the marks' probabilities,
        and markval (n, M), what a jump to each mark's target pays.  P, pmark and pself of a moving node sum to one."""
        import torch

        assert nodes_t.is_cuda and nodes_t.dtype == torch.int32 and nodes_t.is_contiguous() and nodes_t.shape[1] == self.d
        n, d, dev = nodes_t.shape[0], self.d, nodes_t.device
        f64 = dict(dtype=torch.float64, device=dev)
        res = {"uidx": torch.empty((n,), dtype=torch.int32, device=dev), "value": torch.empty((n,), **f64),
               "stage": torch.empty((n,), **f64), "dt": torch.empty((n,), **f64), "P": torch.empty((n, 2 * d), **f64),
               "flag": torch.empty((n,), dtype=torch.int32, device=dev), "pself": torch.empty((n,), **f64)}
        if njump > 0:
            res["pmark"], res["markval"] = torch.empty((n, njump), **f64), torch.empty((n, njump), **f64)
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        ptr = [res[k].data_ptr() if k in res else None for k in ("uidx", "value", "stage", "dt", "P", "flag", "pself", "pmark", "markval")]
        self._chk(self.L.c3sc_hip_chain_outcomes(self.h, n, nodes_t.data_ptr(), *ptr, C.c_void_p(stream_ptr)), "chain_outcomes")
        return res

    def chain_outcomes_host(self, nodes: np.ndarray, njump: int = 0):
        """c3sc_hip_chain_outcomes_host: the same on numpy arrays (nodes int32 (n, d)), staged through device memory."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        n, d = nodes.shape[0], self.d
        res = {"uidx": np.empty((n,), np.int32), "value": np.empty((n,)), "stage": np.empty((n,)), "dt": np.empty((n,)),
               "P": np.empty((n, 2 * d)), "flag": np.empty((n,), np.int32), "pself": np.empty((n,))}
        if njump > 0:
            res["pmark"], res["markval"] = np.empty((n, njump)), np.empty((n, njump))
        ptr = [res[k].ctypes.data if k in res else None for k in ("uidx", "value", "stage", "dt", "P", "flag", "pself", "pmark", "markval")]
        self._chk(self.L.c3sc_hip_chain_outcomes_host(self.h, n, nodes.ctypes.data, *ptr), "chain_outcomes_host")
        return res

    def simulate_chain(self, node0_t, nsteps: int, seed: int = 0, uniform_t=None, save_every: int = 0, traj_offset: int = 0,
                       steps_per_launch: int = 0, stream_ptr: Optional[int] = None):
        """Device API (c3sc_hip_simulate_chain): node0_t int32 CUDA tensor (n, d) of start nodes.  Returns a dict of CUDA tensors:
        cost J, disc D, time T, vend V(xi_nsteps) (n,), node int32 (n, d), exit int64 (n,) (decode_chain_exit) and, with
        save_every > 0, traj int32 (n, nsteps//save_every + 1, d) and uidx int32 (n, ceil(nsteps/save_every)).  uniform_t:
        float64 (n, nsteps) uniforms in [0, 1), else Philox(seed).  cost + disc * J(node) estimates the greedy policy's exact cost
        in the discrete problem without bias."""
        import torch

        assert node0_t.is_cuda and node0_t.dtype == torch.int32 and node0_t.is_contiguous() and node0_t.shape[1] == self.d
        n, d, dev = node0_t.shape[0], self.d, node0_t.device
        f64 = dict(dtype=torch.float64, device=dev)
        res = {"cost": torch.empty((n,), **f64), "disc": torch.empty((n,), **f64), "time": torch.empty((n,), **f64),
               "vend": torch.empty((n,), **f64), "node": torch.empty((n, d), dtype=torch.int32, device=dev),
               "exit": torch.empty((n,), dtype=torch.int64, device=dev)}
        a = ChainArgs()
        a.n, a.d_node0, a.nsteps, a.traj_offset, a.seed = n, node0_t.data_ptr(), int(nsteps), int(traj_offset), int(seed)
        a.steps_per_launch, a.save_every = int(steps_per_launch), int(save_every)
        if uniform_t is not None:
            assert uniform_t.is_cuda and uniform_t.dtype == torch.float64 and uniform_t.is_contiguous()
            assert tuple(uniform_t.shape) in ((n, nsteps), (n, nsteps, 2))  # (v, u1) pairs with jumps on
            a.d_uniform = uniform_t.data_ptr()
        if save_every > 0:
            res["traj"] = torch.empty((n, nsteps // save_every + 1, d), dtype=torch.int32, device=dev)
            res["uidx"] = torch.empty((n, (nsteps + save_every - 1) // save_every), dtype=torch.int32, device=dev)
            a.d_traj, a.d_uidx = res["traj"].data_ptr(), res["uidx"].data_ptr()
        a.d_cost, a.d_disc, a.d_time, a.d_vend = (res["cost"].data_ptr(), res["disc"].data_ptr(), res["time"].data_ptr(),
                                                  res["vend"].data_ptr())
        a.d_node, a.d_exit = res["node"].data_ptr(), res["exit"].data_ptr()
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        self._chk(self.L.c3sc_hip_simulate_chain(self.h, C.byref(a), C.c_void_p(stream_ptr)), "simulate_chain")
        return res

    def simulate_chain_host(self, node0: np.ndarray, nsteps: int, seed: int = 0, uniform=None, save_every: int = 0,
                            traj_offset: int = 0, steps_per_launch: int = 0):
        """c3sc_hip_simulate_chain_host: simulate_chain on numpy arrays, staged through device memory."""
        node0 = np.ascontiguousarray(node0, dtype=np.int32)
        n, d = node0.shape[0], self.d
        res = {"cost": np.empty((n,)), "disc": np.empty((n,)), "time": np.empty((n,)), "vend": np.empty((n,)),
               "node": np.empty((n, d), np.int32), "exit": np.empty((n,), np.int64)}
        a = ChainArgs()
        a.n, a.d_node0, a.nsteps, a.traj_offset, a.seed = n, node0.ctypes.data, int(nsteps), int(traj_offset), int(seed)
        a.steps_per_launch, a.save_every = int(steps_per_launch), int(save_every)
        if uniform is not None:
            uniform = _f64(uniform)
            assert uniform.shape in ((n, nsteps), (n, nsteps, 2))  # (v, u1) pairs with jumps on
            a.d_uniform = uniform.ctypes.data
        if save_every > 0:
            res["traj"] = np.empty((n, nsteps // save_every + 1, d), np.int32)
            res["uidx"] = np.empty((n, (nsteps + save_every - 1) // save_every), np.int32)
            a.d_traj, a.d_uidx = res["traj"].ctypes.data, res["uidx"].ctypes.data
        a.d_cost, a.d_disc, a.d_time, a.d_vend = (res["cost"].ctypes.data, res["disc"].ctypes.data, res["time"].ctypes.data,
                                                  res["vend"].ctypes.data)
        a.d_node, a.d_exit = res["node"].ctypes.data, res["exit"].ctypes.data
        self._chk(self.L.c3sc_hip_simulate_chain_host(self.h, C.byref(a)), "simulate_chain_host")
        return res

    def simulate_chain_rc(self, args: "ChainArgs", stream_ptr: int = 0) -> int:
        """c3sc_hip_simulate_chain's return code as is (for callers that check the error codes)."""
        return int(self.L.c3sc_hip_simulate_chain(self.h, C.byref(args), C.c_void_p(stream_ptr)))

    def integrate(self, x0_t, dt_out: float, nout: int, method: str = "rk4", dt_int: Optional[float] = None, goal=None,
                  keep_in=None, wrap_periodic: bool = False, box: bool = False, save_every: int = 0, evals_per_launch: int = 0,
                  stream_ptr: Optional[int] = None):
        """Device API (c3sc_hip_integrate): deterministic closed loops of the implicit policy, nout outer steps of dt_out, each
        dt_out / dt_int substeps of "forward-euler" or "rk4" (dt_int None: one substep).  goal / keep_in: (lo, hi) sequences of
        d values (+-inf allowed) or None.  x0_t float64 CUDA tensor (n, d).  Returns a dict of CUDA tensors: cost (n,),
        stop_step (int64, -1 = never), stop_reason (int32: 0 running, 1 absorbing face, 2 obstacle, 3 goal, 4 keep-in left),
        vend (n,), xfinal (n, d) and, with save_every > 0, traj (n, nout//save_every + 1, d) and u (n, ceil(nout/save_every), du)."""
        import torch

        assert x0_t.is_cuda and x0_t.dtype == torch.float64 and x0_t.is_contiguous() and x0_t.shape[1] == self.d
        if method not in _ODE_METHODS:
            raise ValueError(f"integrate: unknown method {method!r} (forward-euler, rk4)")
        n, d, dev = x0_t.shape[0], self.d, x0_t.device
        du = getattr(self, "box_du", self.w.du) if box else self.w.du
        res = {"cost": torch.empty((n,), dtype=torch.float64, device=dev),
               "stop_step": torch.empty((n,), dtype=torch.int64, device=dev),
               "stop_reason": torch.empty((n,), dtype=torch.int32, device=dev),
               "vend": torch.empty((n,), dtype=torch.float64, device=dev),
               "xfinal": torch.empty((n, d), dtype=torch.float64, device=dev)}
        a = OdeArgs()
        a.n, a.d_x0, a.dt_out, a.nout = n, x0_t.data_ptr(), float(dt_out), int(nout)
        a.dt_int = 0.0 if dt_int is None else float(dt_int)
        a.method, a.wrap_periodic, a.box = _ODE_METHODS[method], int(bool(wrap_periodic)), int(bool(box))
        a.evals_per_launch, a.save_every = int(evals_per_launch), int(save_every)
        boxes = {}
        for key, b in (("goal", goal), ("keep", keep_in)):
            if b is not None:
                arr = np.ascontiguousarray(np.concatenate([np.asarray(b[0], dtype=np.float64).reshape(-1),
                                                           np.asarray(b[1], dtype=np.float64).reshape(-1)]))
                if arr.shape[0] != 2 * d:
                    raise ValueError(f"integrate: {key} needs (lo, hi) of {d} values each")
                boxes[key] = arr
                setattr(a, key, arr.ctypes.data)
        if save_every > 0:
            res["traj"] = torch.empty((n, nout // save_every + 1, d), dtype=torch.float64, device=dev)
            res["u"] = torch.empty((n, (nout + save_every - 1) // save_every, du), dtype=torch.float64, device=dev)
            a.d_traj, a.d_u = res["traj"].data_ptr(), res["u"].data_ptr()
        a.d_cost, a.d_stop_step, a.d_stop_reason = res["cost"].data_ptr(), res["stop_step"].data_ptr(), res["stop_reason"].data_ptr()
        a.d_vend, a.d_xfinal = res["vend"].data_ptr(), res["xfinal"].data_ptr()
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        self._chk(self.L.c3sc_hip_integrate(self.h, C.byref(a), C.c_void_p(stream_ptr)), "integrate")
        return res

    def integrate_rc(self, args: "OdeArgs", stream_ptr: int = 0) -> int:
        """c3sc_hip_integrate's return code as is (for callers that check the error codes)."""
        return int(self.L.c3sc_hip_integrate(self.h, C.byref(args), C.c_void_p(stream_ptr)))

    def bellman_fibers_host(self, k: int, idx: np.ndarray, want_uidx=True, want_absorbed=True):
        """Host-buffer API (what the C facade's bellman_vi uses): numpy in, numpy out, synchronous."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        F, N = idx.shape[0], self.ngrid[k]
        out = np.empty((F, N))
        ui = np.empty((F, N), dtype=np.int32) if want_uidx else None
        ab = np.empty((F, N), dtype=np.int32) if want_absorbed else None
        self._chk(self.L.c3sc_hip_bellman_fibers_host(self.h, k, F, idx.ctypes.data, out.ctypes.data,
                                                      ui.ctypes.data if ui is not None else None,
                                                      ab.ctypes.data if ab is not None else None), "bellman_fibers_host")
        return out, ui, ab

    def policy_fibers_host(self, k: int, idx: np.ndarray, policy: np.ndarray):
        """Policy evaluation (batched bellman_pi): apply candidate policy[f, j] at every node."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        policy = np.ascontiguousarray(policy, dtype=np.int32)
        F, N = idx.shape[0], self.ngrid[k]
        assert policy.shape == (F, N)
        out = np.empty((F, N))
        ab = np.empty((F, N), dtype=np.int32)
        self._chk(self.L.c3sc_hip_policy_fibers_host(self.h, k, F, idx.ctypes.data, policy.ctypes.data, out.ctypes.data,
                                                     ab.ctypes.data), "policy_fibers_host")
        return out, ab

    # ---- continuous controls in a box
    def set_control_box(self, lb, ub, grid=33, polish=2):
        lb, ub = _f64(lb), _f64(ub)
        self.box_du = len(lb)
        self._chk(self.L.c3sc_hip_set_control_box(self.h, len(lb), lb.ctypes.data_as(c_double_p), ub.ctypes.data_as(c_double_p),
                                                  int(grid), int(polish)), "set_control_box")

    def bellman_fibers_box_host(self, k: int, idx: np.ndarray):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        F, N = idx.shape[0], self.ngrid[k]
        out, uo, ab = np.empty((F, N)), np.empty((F, N, self.box_du)), np.empty((F, N), dtype=np.int32)
        self._chk(self.L.c3sc_hip_bellman_fibers_box_host(self.h, k, C.c_size_t(F), C.c_void_p(idx.ctypes.data), C.c_void_p(out.ctypes.data),
                                                          C.c_void_p(uo.ctypes.data), C.c_void_p(ab.ctypes.data)), "bellman_fibers_box_host")
        return out, uo, ab

    def policy_fibers_box_host(self, k: int, idx: np.ndarray, policy_u: np.ndarray):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        pu = _f64(policy_u)
        F, N = idx.shape[0], self.ngrid[k]
        out, ab = np.empty((F, N)), np.empty((F, N), dtype=np.int32)
        self._chk(self.L.c3sc_hip_policy_fibers_box_host(self.h, k, C.c_size_t(F), C.c_void_p(idx.ctypes.data), C.c_void_p(pu.ctypes.data),
                                                         C.c_void_p(out.ctypes.data), C.c_void_p(ab.ctypes.data)), "policy_fibers_box_host")
        return out, ab

    def bellman_fibers_tables_host(self, k: int, idx: np.ndarray, tables: np.ndarray, costs2: np.ndarray):
        """Universal path: tables (F, N, U, 2d+1) = host-evaluated (drift, diag sigma, stage), costs2 (F, N, 2)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        tables = _f64(tables)
        costs2 = _f64(costs2)
        F, N = idx.shape[0], self.ngrid[k]
        out = np.empty((F, N))
        ui = np.empty((F, N), dtype=np.int32)
        ab = np.empty((F, N), dtype=np.int32)
        self._chk(self.L.c3sc_hip_bellman_fibers_tables_host(self.h, k, F, idx.ctypes.data, tables.ctypes.data,
                                                             costs2.ctypes.data, out.ctypes.data, ui.ctypes.data,
                                                             ab.ctypes.data), "bellman_fibers_tables_host")
        return out, ui, ab

    def policy_fibers_tables_host(self, k: int, idx: np.ndarray, tables: np.ndarray, costs2: np.ndarray, policy: np.ndarray):
        """Policy evaluation on the universal path (c3sc_hip_policy_fibers_tables_host): apply candidate policy[f, j] of the
        tables at every node.  Returns (values (F, N), absorbed (F, N))."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        tables = _f64(tables)
        costs2 = _f64(costs2)
        policy = np.ascontiguousarray(policy, dtype=np.int32)
        F, N = idx.shape[0], self.ngrid[k]
        assert policy.shape == (F, N)
        out = np.empty((F, N))
        ab = np.empty((F, N), dtype=np.int32)
        self._chk(self.L.c3sc_hip_policy_fibers_tables_host(self.h, k, F, idx.ctypes.data, tables.ctypes.data, costs2.ctypes.data,
                                                            policy.ctypes.data, out.ctypes.data, ab.ctypes.data),
                  "policy_fibers_tables_host")
        return out, ab

    def stencil_fibers_host(self, k: int, idx: np.ndarray, nb_fixed=None, nb_vary=None):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        F, N = idx.shape[0], self.ngrid[k]
        costs = np.empty((F, N, 2 * self.d + 1))
        ab = np.empty((F, N), dtype=np.int32)
        nf = np.ascontiguousarray(nb_fixed, dtype=np.int32) if nb_fixed is not None else None
        nv = np.ascontiguousarray(nb_vary, dtype=np.int32) if nb_vary is not None else None
        self._chk(self.L.c3sc_hip_stencil_fibers_nb_host(self.h, k, F, idx.ctypes.data,
                                                         nf.ctypes.data if nf is not None else None,
                                                         nv.ctypes.data if nv is not None else None,
                                                         costs.ctypes.data, ab.ctypes.data), "stencil_fibers_nb_host")
        return costs, ab

    # ------------------------------------------------------------------ misc
    def sync(self, stream_ptr: int = 0):
        self._chk(self.L.c3sc_hip_sync(self.h, C.c_void_p(stream_ptr)), "sync")

    def status(self, clear=True) -> int:
        fl = C.c_uint(0)
        self._chk(self.L.c3sc_hip_get_status(self.h, C.byref(fl), C.c_int(1 if clear else 0)), "get_status")
        return fl.value

    def last_kernel(self) -> str:
        return self.L.c3sc_hip_last_kernel(self.h).decode()

    def last_partition(self, slot: int = 0):
        """(perm, nlive) of the last partition a fiber-pair launch ran in scratch block `slot`; waits for that launch (tests)"""
        F, nl = C.c_size_t(0), C.c_int(0)
        self._chk(self.L.c3sc_hip_last_partition(self.h, slot, None, 0, C.byref(F), C.byref(nl)), "last_partition")
        perm = np.empty(F.value, dtype=np.int32)
        self._chk(self.L.c3sc_hip_last_partition(self.h, slot, perm.ctypes.data_as(C.c_void_p), perm.size, C.byref(F), C.byref(nl)),
                  "last_partition")
        return perm, nl.value

    def timer_start(self, stream_ptr: int = 0):
        self._chk(self.L.c3sc_hip_timer_start(self.h, C.c_void_p(stream_ptr)), "timer_start")

    def timer_stop(self, stream_ptr: int = 0) -> float:
        ms = C.c_float(0)
        self._chk(self.L.c3sc_hip_timer_stop(self.h, C.c_void_p(stream_ptr), C.byref(ms)), "timer_stop")
        return ms.value

    def debug_read(self, n: int) -> np.ndarray:
        buf = np.zeros(n, dtype=np.uint64)
        self._chk(self.L.c3sc_hip_debug_read(self.h, C.c_void_p(buf.ctypes.data), C.c_size_t(n)), "debug_read")
        return buf

    def peak_fma_f64(self) -> float:
        v = C.c_double(0)
        self._chk(self.L.c3sc_hip_peak_fma_f64(self.h, C.byref(v)), "peak_fma_f64")
        return v.value

    def peak_mfma_f64(self) -> float:
        v = C.c_double(0)
        self._chk(self.L.c3sc_hip_peak_mfma_f64(self.h, C.byref(v)), "peak_mfma_f64")
        return v.value
