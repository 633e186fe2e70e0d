"""ctypes binding of libspx.so (include/spx.h).  There is NO fallback: if the HIP library is missing
or no GPU is visible, the product path raises -- it never computes on the CPU."""
import ctypes
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("SPX_LIB_NAME", "libspx.so"))  # SPX_LIB_NAME: A/B builds (tools/)

c_double_p = ctypes.c_void_p  # device pointers are passed as plain addresses
_i64, _d, _p, _int = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
_f = ctypes.c_float

# name -> argtypes; must list every symbol declared in include/spx.h (tests/test_abi.py checks this)
SIGNATURES = {
    "spx_abi_version": [],
    "spx_last_error": [],
    "spx_ctx_create": [_int, ctypes.POINTER(_p)],
    "spx_ctx_create_on_stream": [_int, _p, ctypes.POINTER(_p)],
    "spx_ctx_destroy": [_p],
    "spx_sync": [_p],
    "spx_timer_start": [_p],
    "spx_timer_stop": [_p, ctypes.POINTER(ctypes.c_float)],
    "spx_ctx_set_tuning": [_p, _int, _int],
    "spx_ctx_set_value_target": [_p, _p],
    "spx_copy_strided": [_p, _p, _i64, _p, _i64, _i64, _int],
    "spx_synth_fill": [_p, _p, _i64, ctypes.c_uint64, ctypes.c_uint64, _int, _d],
    "spx_check_bounds": [_p, _p, _p, _d, _d, _i64, ctypes.POINTER(_int)],
    "spx_build_mask": [_p, _p, _i64, _p, _i64],
    "spx_prox_l1": [_p, _p, _p, _p, _p, _i64, _d, _d],
    "spx_prox_l0": [_p, _p, _p, _p, _p, _i64, _d, _d],
    "spx_prox_lhalf": [_p, _p, _p, _p, _p, _i64, _d, _d],
    "spx_prox_l1_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p],
    "spx_prox_l0_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p],
    "spx_prox_lhalf_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p],
    "spx_prox_l1_f32": [_p, _p, _p, _p, _p, _i64, _f, _f],
    "spx_prox_l0_f32": [_p, _p, _p, _p, _p, _i64, _f, _f],
    "spx_prox_l1_box_f32": [_p, _p, _p, _p, _p, _i64, _f, _f, _p, _p, _f, _f, _p],
    "spx_prox_l0_box_f32": [_p, _p, _p, _p, _p, _i64, _f, _f, _p, _p, _f, _f, _p],
    "spx_iprox_l1_f32": [_p, _p, _p, _p, _p, _p, _i64, _f, _int],
    "spx_iprox_l0_f32": [_p, _p, _p, _p, _p, _p, _i64, _f, _int],
    "spx_iprox_l1_box_f32": [_p, _p, _p, _p, _p, _p, _i64, _f, _p, _p, _f, _f, _p],
    "spx_iprox_l0_box_f32": [_p, _p, _p, _p, _p, _p, _i64, _f, _p, _p, _f, _f, _p],
    "spx_proxval_l1": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, ctypes.POINTER(_d)],
    "spx_proxval_l0": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, ctypes.POINTER(_d)],
    "spx_proxval_lhalf": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, ctypes.POINTER(_d)],
    "spx_proxval_l1_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p, _d, ctypes.POINTER(_d)],
    "spx_proxval_l0_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p, _d, ctypes.POINTER(_d)],
    "spx_proxval_lhalf_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p, _d, ctypes.POINTER(_d)],
    "spx_proxstep_l1": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxstep_l0": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxstep_lhalf": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxstep_l1_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxstep_l0_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxstep_lhalf_box": [_p, _p, _p, _p, _p, _i64, _d, _d, _p, _p, _d, _d, _p, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxval_group_l2": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d, _d, ctypes.POINTER(_d)],
    "spx_proxval_group_l2_binf": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d, _d, _d, ctypes.POINTER(_d)],
    "spx_proxstep_group_l2": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxstep_group_l2_binf": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d, _d, _d, _p, ctypes.POINTER(_d), _p],
    "spx_proxval_l1_b2": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, _d, _d, ctypes.POINTER(_d)],
    "spx_proxstep_l1_b2": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, _d, _d, _p, ctypes.POINTER(_d), _p],
    "spx_iprox_l1": [_p, _p, _p, _p, _p, _p, _i64, _d, _int],
    "spx_iprox_l0": [_p, _p, _p, _p, _p, _p, _i64, _d, _int],
    "spx_iprox_l1_box": [_p, _p, _p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p],
    "spx_iprox_l0_box": [_p, _p, _p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p],
    "spx_iproxstep_l1": [_p, _p, _p, _p, _p, _p, _i64, _d, _int, _p, ctypes.POINTER(_d), _p],
    "spx_iproxstep_l0": [_p, _p, _p, _p, _p, _p, _i64, _d, _int, _p, ctypes.POINTER(_d), _p],
    "spx_iproxstep_l1_box": [_p, _p, _p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p, _p, ctypes.POINTER(_d), _p],
    "spx_iproxstep_l0_box": [_p, _p, _p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p, _p, ctypes.POINTER(_d), _p],
    "spx_obj_l1": [_p, _p, _p, _p, _i64, _d, ctypes.POINTER(_d)],
    "spx_obj_l0": [_p, _p, _p, _p, _i64, _d, ctypes.POINTER(_d)],
    "spx_obj_lhalf": [_p, _p, _p, _p, _i64, _d, ctypes.POINTER(_d)],
    "spx_obj_l1_box": [_p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p, ctypes.POINTER(_d)],
    "spx_obj_l0_box": [_p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p, ctypes.POINTER(_d)],
    "spx_obj_lhalf_box": [_p, _p, _p, _p, _i64, _d, _p, _p, _d, _d, _p, ctypes.POINTER(_d)],
    "spx_obj_indball_l0": [_p, _p, _p, _p, _i64, _i64, ctypes.POINTER(_d)],
    "spx_obj_indball_l0_binf": [_p, _p, _p, _p, _i64, _i64, _d, ctypes.POINTER(_d)],
    "spx_obj_group_l2": [_p, _p, _p, _p, _i64, _p, _i64, _i64, _p, ctypes.POINTER(_d)],
    "spx_obj_group_l2_binf": [_p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d, ctypes.POINTER(_d)],
    "spx_obj_l1_f32": [_p, _p, _p, _p, _i64, _f, ctypes.POINTER(_d)],
    "spx_obj_l0_f32": [_p, _p, _p, _p, _i64, _f, ctypes.POINTER(_d)],
    "spx_obj_lhalf_f32": [_p, _p, _p, _p, _i64, _f, ctypes.POINTER(_d)],
    "spx_obj_l1_box_f32": [_p, _p, _p, _p, _i64, _f, _p, _p, _f, _f, _p, ctypes.POINTER(_d)],
    "spx_obj_l0_box_f32": [_p, _p, _p, _p, _i64, _f, _p, _p, _f, _f, _p, ctypes.POINTER(_d)],
    "spx_obj_lhalf_box_f32": [_p, _p, _p, _p, _i64, _f, _p, _p, _f, _f, _p, ctypes.POINTER(_d)],
    "spx_obj_indball_l0_f32": [_p, _p, _p, _p, _i64, _i64, ctypes.POINTER(_d)],
    "spx_obj_indball_l0_binf_f32": [_p, _p, _p, _p, _i64, _i64, _f, ctypes.POINTER(_d)],
    "spx_obj_group_l2_f32": [_p, _p, _p, _p, _i64, _p, _i64, _i64, _p, ctypes.POINTER(_d)],
    "spx_obj_group_l2_binf_f32": [_p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _f, ctypes.POINTER(_d)],
    "spx_prox_indball_l0": [_p, _p, _p, _p, _p, _i64, _i64],
    "spx_prox_indball_l0_binf": [_p, _p, _p, _p, _p, _i64, _i64, _d],
    "spx_prox_indball_l0_f32": [_p, _p, _p, _p, _p, _i64, _i64],
    "spx_prox_indball_l0_binf_f32": [_p, _p, _p, _p, _p, _i64, _i64, _f],
    "spx_prox_l1_b2": [_p, _p, _p, _p, _p, _i64, _d, _d, _d, _d],
    "spx_obj_l1_b2": [_p, _p, _p, _p, _i64, _d, _d, ctypes.POINTER(_d)],
    "spx_prox_group_l2": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d],
    "spx_prox_group_l2_f32": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _f],
    "spx_prox_group_l2_binf": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _d, _d],
    "spx_prox_group_l2_gather": [_p, _p, _p, _p, _p, _i64, _p, _p, _i64, _i64, _p, _d],
    "spx_prox_group_l2_binf_gather": [_p, _p, _p, _p, _p, _i64, _p, _p, _i64, _i64, _p, _d, _d],
    "spx_obj_group_l2_gather": [_p, _p, _p, _p, _i64, _p, _p, _i64, _i64, _p, ctypes.POINTER(_d)],
    "spx_obj_group_l2_binf_gather": [_p, _p, _p, _p, _i64, _p, _p, _i64, _i64, _p, _d, ctypes.POINTER(_d)],
}
# host-pointer forms: spx_host_X has the argument list of spx_X (include/spx.h, "host-pointer forms")
SIGNATURES.update({"spx_host_" + k[4:]: list(v) for k, v in list(SIGNATURES.items())
                   if k.startswith(("spx_prox_", "spx_iprox_", "spx_obj_")) and not k.endswith("_f32")})

# include/spx_batch.h: the batched separable call
BATCH_SIGNATURES = {
    "spx_proxstep_l1_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "spx_proxstep_l0_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "spx_proxstep_l1_box_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p],
    "spx_proxstep_l0_box_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p],
}

# include/spx_ibatch.h: the batched iprox! call
IBATCH_SIGNATURES = {
    "spx_iproxstep_l1_batch": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "spx_iproxstep_l0_batch": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "spx_iproxstep_l1_box_batch": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p],
    "spx_iproxstep_l0_box_batch": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p],
}

# include/spx_gbatch.h: the batched group call
GBATCH_SIGNATURES = {
    "spx_proxstep_group_l2_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p],
}

# include/spx_gbinf_batch.h: the batched Binf group call
GBINF_BATCH_SIGNATURES = {
    "spx_proxstep_group_l2_binf_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p, _p],
}

# include/spx_b2_batch.h: the batched ShiftedNormL1B2 call
B2_BATCH_SIGNATURES = {
    "spx_proxstep_l1_b2_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _d, _p, _p],
}

# include/spx_topr_batch.h: the batched top-r calls
TOPR_BATCH_SIGNATURES = {
    "spx_proxstep_indball_l0_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p],
    "spx_proxstep_indball_l0_binf_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p],
}

# include/spx_lhalf_batch.h: the batched RootNormLhalf(Box) calls
LHALF_BATCH_SIGNATURES = {
    "spx_proxstep_lhalf_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "spx_proxstep_lhalf_box_batch": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p],
    "spx_lhalf_threshold_batch": [_p, _p, _p, _i64, _p],
}


class SpxError(RuntimeError):
    """A libspx call returned a non-zero spx_status."""

    def __init__(self, status, message):
        super().__init__("libspx status %d: %s" % (status, message))
        self.status = status


_lib = None


def load():
    """Load libspx.so (built by csrc/build.sh / __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libspx.so not found at %s -- build it with shiftedproximaloperators.jl_amd/csrc/build.sh "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
            fn.argtypes = args
            fn.restype = ctypes.c_char_p if name == "spx_last_error" else _int
        _lib = L
    return _lib


# The batched libraries, in build order: file-name suffix -> ctypes table.  Each is a library of its own that links against
# libspx.so ("A library of its own, and why"); everything else about one follows from its key: include/spx_<key>.h,
# csrc/spx_<key>.hip, lib/libspx_<key>.so.  csrc/build.sh's BATCH_LIBS array names the same keys (tests/test_batch_libraries.py).
BATCH_LIBRARIES = {
    "batch": BATCH_SIGNATURES,
    "ibatch": IBATCH_SIGNATURES,
    "gbatch": GBATCH_SIGNATURES,
    "gbinf_batch": GBINF_BATCH_SIGNATURES,
    "b2_batch": B2_BATCH_SIGNATURES,
    "topr_batch": TOPR_BATCH_SIGNATURES,
    "lhalf_batch": LHALF_BATCH_SIGNATURES,
}


def batch_lib_path(key):
    """lib/libspx_<key>.so -- for SPX_LIB_NAME=X.so: X_<key>.so"""
    return LIB_PATH[:-3] + "_" + key + ".so"


_batch_libs = {}


def load_batch_library(key):
    """Load libspx_<key>.so (after libspx.so, whose contexts and error text it shares).  Raises if it is missing."""
    if key not in _batch_libs:
        signatures, path = BATCH_LIBRARIES[key], batch_lib_path(key)  # KeyError for a library the table does not know
        load()
        if not os.path.exists(path):
            raise ImportError("libspx_%s.so not found at %s -- build it with shiftedproximaloperators.jl_amd/csrc/build.sh; "
                              "there is no CPU fallback" % (key, path))
        L = ctypes.CDLL(path)
        for name, args in signatures.items():
            fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
            fn.argtypes = args
            fn.restype = _int
        _batch_libs[key] = L
    return _batch_libs[key]


# the names shifted.py, tests/ and tools/ use: one line each, defined from the table
BATCH_LIB_PATH = batch_lib_path("batch")
IBATCH_LIB_PATH = batch_lib_path("ibatch")
GBATCH_LIB_PATH = batch_lib_path("gbatch")
GBINF_BATCH_LIB_PATH = batch_lib_path("gbinf_batch")
B2_BATCH_LIB_PATH = batch_lib_path("b2_batch")
TOPR_BATCH_LIB_PATH = batch_lib_path("topr_batch")
LHALF_BATCH_LIB_PATH = batch_lib_path("lhalf_batch")


load_batch = functools.partial(load_batch_library, "batch")
load_ibatch = functools.partial(load_batch_library, "ibatch")
load_gbatch = functools.partial(load_batch_library, "gbatch")
load_gbinf_batch = functools.partial(load_batch_library, "gbinf_batch")
load_b2_batch = functools.partial(load_batch_library, "b2_batch")
load_topr_batch = functools.partial(load_batch_library, "topr_batch")
load_lhalf_batch = functools.partial(load_batch_library, "lhalf_batch")


def check(status):
    if status != 0:
        msg = load().spx_last_error()
        raise SpxError(status, msg.decode() if msg else "")
