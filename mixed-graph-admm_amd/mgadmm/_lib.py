"""ctypes binding of libmgadmm.so (C ABI declared in include/mgadmm.h).

The product path has no CPU fallback: importing this module fails loudly when the HIP library has
not been built (run ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C mixed-graph-admm_amd/csrc``).
"""
import ctypes as C
import os

# torch first: it bundles its own libamdhip64.so.7; loading it before libmgadmm.so makes both share ONE
# HIP runtime (device pointers, streams and events are exchanged between them).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# MGADMM_LIB selects another build of the same library (kernel experiments with different compiler flags)
LIB_PATH = os.environ.get("MGADMM_LIB") or os.path.join(_HERE, "libmgadmm.so")

OK, ERR_INVALID, ERR_HIP, ERR_NONFINITE, ERR_UNSUPPORTED, ERR_NOMEM = 0, -1, -2, -3, -4, -5
F32, F64 = 0, 1
TEMPORAL_SPATIAL, TEMPORAL_BAND = 0, 1
OP_LU, OP_LDR, OP_LDRT, OP_CLDR, OP_LN = 0, 1, 2, 3, 4
CG_PER_SAMPLE, CG_BATCH_MAX = 0, 1
ADMM_WHOLE_BATCH, ADMM_PER_SAMPLE = 0, 1
LHS_X, LHS_ZU, LHS_ZD = 0, 1, 2
ABLATIONS = {"None": 0, "DGTV": 1, "DGLR": 2, "UT": 3}
PATH_AUTO, PATH_STREAM, PATH_LDS = 0, 1, 2
NMETRIC = 11
(M_XSHIFT, M_PRI_ZU, M_DUAL_ZU, M_PRI_PHI, M_DUAL_PHI, M_PRI_ZD, M_DUAL_ZD, M_GLR, M_DGTV, M_DGLR,
 M_RECOVER) = range(11)
NPROF = 4
(Q_LDS_OK, Q_LDS_TPG, Q_LDS_THREADS, Q_LDS_BYTES, Q_LDS_ROW_STRIDE, Q_NNZ_U, Q_NNZ_D, Q_NNZ_DT, Q_TILE_ROWS, Q_LDS_UNIFORM,
 Q_LDS_TAIL_PAIRS, Q_LDS_LEAD, Q_LDS_SLOTS, Q_LDS_CHUNK, Q_LDS_ROWS, Q_CLDR_SLOTS, Q_LDS_INSTANCE, Q_LDS_CG_BARRIERS,
 Q_LDS_UNIT) = range(19)
Q_STREAM_KEYS, Q_STREAM_KEY0 = 19, 1000
LDS_UNITS = ("k_admm_lds", "k_admm_lds_ps", "k_admm_lds_pp")      # values of Q_LDS_UNIT (-1: no LDS launch yet)

_i32p = C.POINTER(C.c_int32)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)


class GraphDesc(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32), ("T", C.c_int32), ("temporal_mode", C.c_int32),
        ("u_rowptr", _i32p), ("u_col", _i32p), ("u_val", _f32p),
        ("d_rowptr", _i32p), ("d_col", _i32p), ("d_val", _f32p),
        ("transpose_by_gather", C.c_int32), ("q1_identity_t0", C.c_int32),
        ("skip", C.c_int32), ("band_w", _f32p),
        ("reorder", C.c_int32), ("device", C.c_int32),
    ]


class Params(C.Structure):
    _fields_ = [
        ("rho", C.c_double), ("rho_u", C.c_double), ("rho_d", C.c_double),
        ("mu_u", C.c_double), ("mu_d1", C.c_double), ("mu_d2", C.c_double),
        ("t_in", C.c_int32), ("ablation", C.c_int32),
        ("cg_tol", C.c_double), ("max_cg_iter", C.c_int32),
        ("admm_tol", C.c_double), ("max_admm_iter", C.c_int32),
        ("dtype", C.c_int32), ("check_stop", C.c_int32), ("path", C.c_int32),
        ("record_cg_coeffs", C.c_int32), ("cg_convergence", C.c_int32), ("max_inner_iter", C.c_int32),
        ("admm_convergence", C.c_int32),
    ]


class History(C.Structure):
    _fields_ = [
        ("n_iters", C.c_int32),
        ("metrics", _f64p), ("delta_x_per_step", _f64p), ("cg_iters", _i32p),
        ("metrics_per_sample", _f64p), ("cg_alpha", _f64p), ("cg_beta", _f64p),
        ("n_iters_per_sample", _i32p),
    ]


class State(C.Structure):
    _fields_ = [("zu", C.c_void_p), ("zd", C.c_void_p), ("phi", C.c_void_p), ("gamma", C.c_void_p),
                ("gamma_u", C.c_void_p), ("gamma_d", C.c_void_p)]


class SampleParams(C.Structure):
    _fields_ = [("rho", _f64p), ("rho_u", _f64p), ("rho_d", _f64p), ("mu_u", _f64p), ("mu_d1", _f64p), ("mu_d2", _f64p)]


ParamSchedule = SampleParams       # mgadmm_param_schedule: the same six pointers, arrays of [n_rows][B] / [n_rows]


class AdaptiveRho(C.Structure):    # mgadmm_adaptive_rho; rho_min / rho_max in the order rho, rho_u, rho_d
    _fields_ = [("every", C.c_int32), ("until", C.c_int32), ("mu", C.c_double), ("tau", C.c_double),
                ("rho_min", C.c_double * 3), ("rho_max", C.c_double * 3)]


# every symbol include/mgadmm.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
SYMBOLS = {
    "mgadmm_version": (C.c_char_p, []),
    "mgadmm_last_error": (C.c_char_p, []),
    "mgadmm_graph_create": (C.c_int, [C.POINTER(GraphDesc), C.POINTER(_vp)]),
    "mgadmm_graph_destroy": (C.c_int, [_vp]),
    "mgadmm_graph_transpose_nnz": (C.c_int, [_vp, _i32p]),
    "mgadmm_graph_get_transpose": (C.c_int, [_vp, _i32p, _i32p, _f32p]),
    "mgadmm_graph_get_perm": (C.c_int, [_vp, _i32p]),
    "mgadmm_graph_set_time_weights": (C.c_int, [_vp, _f32p, C.c_int32, _f32p, C.c_int32]),
    "mgadmm_solver_create": (C.c_int, [_vp, C.POINTER(Params), C.c_int32, C.POINTER(_vp)]),
    "mgadmm_solver_destroy": (C.c_int, [_vp]),
    "mgadmm_solver_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "mgadmm_solver_set_sample_params": (C.c_int, [_vp, C.POINTER(SampleParams), C.c_int32]),
    "mgadmm_solver_set_sample_graphs": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.c_int32]),
    "mgadmm_solver_set_param_schedule": (C.c_int, [_vp, C.POINTER(SampleParams), C.c_int32, C.c_int32, C.c_int32]),
    "mgadmm_solver_set_adaptive_rho": (C.c_int, [_vp, C.POINTER(AdaptiveRho), C.c_int32]),
    "mgadmm_solver_get_adaptive_history": (C.c_int, [_vp, C.c_int32, _f64p, C.c_int32, _i32p]),
    "mgadmm_solver_set_sample_bands": (C.c_int, [_vp, C.c_int32, _f32p, _i32p, C.c_int32]),
    "mgadmm_solver_workspace_bytes": (C.c_int64, [_vp]),
    "mgadmm_solver_path": (C.c_int, [_vp, C.c_int32]),
    "mgadmm_solver_query": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64)]),
    "mgadmm_apply": (C.c_int, [_vp, C.c_int32, _vp, _vp, C.c_int32, _vp]),
    "mgadmm_lhs": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp]),
    "mgadmm_phi_direct": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _vp]),
    "mgadmm_initial_guess": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp]),
    "mgadmm_initial_interpolation": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp]),
    "mgadmm_cg": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _i32p, _f64p, _f64p, C.c_int32, _vp]),
    "mgadmm_solve": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, C.POINTER(State), C.POINTER(History), _vp]),
    "mgadmm_solve_from": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, C.POINTER(State), _vp, C.POINTER(State), C.POINTER(History), _vp]),
    "mgadmm_two_loops": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, C.POINTER(State), C.POINTER(History), _vp]),
    "mgadmm_knn_graph": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int64), _f64p, C.c_int32, _i32p, _f32p, C.c_int32]),
    "mgadmm_weight_tables": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64), _f32p, C.c_double, C.c_double, C.c_int32,
                                       _f32p, _f32p, _f64p, C.c_int32]),
    "mgadmm_series_stats": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "mgadmm_series_affine": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp]),
    "mgadmm_gather_windows": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "mgadmm_prof_begin": (C.c_int, [_vp]),
    "mgadmm_prof_end": (C.c_int, [_vp, C.POINTER(C.c_int64), _f64p, _f64p]),
}


class MgadmmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmgadmm error {code}: {msg}")
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise OSError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. mgadmm has no CPU fallback; "
            "build it with `make -C mixed-graph-admm_amd/csrc` (needs hipcc, --offload-arch=gfx950).")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)       # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc):
    if rc != OK:
        raise MgadmmError(rc, lib.mgadmm_last_error().decode("utf-8", "replace"))
    return rc


def version():
    return lib.mgadmm_version().decode()


def query(handle, what):
    out = C.c_int64()
    check(lib.mgadmm_solver_query(handle, what, C.byref(out)))
    return int(out.value)


def decode_lds_instance(v):
    """Packed MGADMM_Q_LDS_INSTANCE value -> the instance name as `nm -C` prints it, e.g.
    'k_admm_lds<12, false, 640, false, 4, 5, true, 2>'; None for -1 (no launch yet)."""
    if v < 0:
        return None
    b = lambda bit: "true" if (v >> bit) & 1 else "false"
    args = [v & 0xFF, b(8), (v >> 21) & 0x7FF, b(9), (v >> 11) & 0x1F, (v >> 16) & 0x1F, b(10), ((v >> 32) & 0xFF) - 1]
    return "k_admm_lds<" + ", ".join(str(a) for a in args) + ">"


def lds_instance(handle):
    """Name of the k_admm_lds instance the solver's last LDS launch ran (None before the first launch)."""
    return decode_lds_instance(query(handle, Q_LDS_INSTANCE))


# csrc/stream_keys.h: epilogue functors by ID, and the integer template arguments that follow the functor(s) per kernel
STREAM_EPILOGUES = ("EpiStore", "EpiLhs", "EpiCgInit", "EpiCgUpdate", "EpiPUpdate", "EpiXFinal", "EpiLin2", "EpiRhsX", "EpiDual",
                    "EpiPhi", "EpiPhiDirect", "EpiDot", "EpiLnLine", "EpiAddTo")
STREAM_KERNELS = ("k_rows", "k_tile", "k_cldr")
_STREAM_NARGS = (1, 2, 7)


def decode_stream_key(v):
    """Packed MGADMM_Q_STREAM_KEY0 + i value -> the instance name as `nm -C` prints it, e.g.
    'k_tile<float, 4, EpiLhs<float, 4>, 4, 2, TileSrcFold<float, 4> >' or
    'k_cldr<double, 1, EpiStore<double, 1>, CldrSrcPlain<double, 1>, 8, 8, 11, 15, 6, 12, 2>'."""
    kern, s, vec = v & 3, "double" if (v >> 2) & 1 else "float", (v >> 3) & 7
    epi, fold = STREAM_EPILOGUES[(v >> 6) & 31], (v >> 11) & 1
    args = [str((v >> (12 + 6 * i)) & 63) for i in range(_STREAM_NARGS[kern])]
    e = f"{epi}<{s}, {vec}>"
    src = f"{'Fold' if fold else 'Plain'}<{s}, {vec}>"
    if kern == 0:
        assert not fold
        return f"k_rows<{s}, {vec}, {e}, {args[0]}>"
    if kern == 1:
        return f"k_tile<{s}, {vec}, {e}, {args[0]}, {args[1]}, TileSrc{src} >"
    return f"k_cldr<{s}, {vec}, {e}, CldrSrc{src}, " + ", ".join(args) + ">"


def stream_keys(handle):
    return [query(handle, Q_STREAM_KEY0 + i) for i in range(query(handle, Q_STREAM_KEYS))]


def stream_instances(handle):
    """Names of the distinct k_rows / k_tile / k_cldr instances the solver has launched since it was created."""
    return {decode_stream_key(v) for v in stream_keys(handle)}
