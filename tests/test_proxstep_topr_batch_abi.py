"""CPU: what is specific to the batched top-r prox! + step statistics entry points (spx_proxstep_indball_l0_batch,
spx_proxstep_indball_l0_binf_batch, include/spx_topr_batch.h, libspx_topr_batch.so): the header declares the calls and states
their contract, the library takes spx_set_error and spx_zero_async from libspx.so and does not ask for spx_ws_reserve, the ctypes
table (TOPR_BATCH_SIGNATURES) binds the calls with the three integers by value and pointers elsewhere, and the mirror takes r as
an int64 device tensor and delta and q_scale as float64 device tensors: anything else is refused.

What holds for every batched library alike -- the header compiles alone as C99 and C++11, includes spx.h and declares exactly
the ctypes table's names; the library exports them and no other library does; no host-pointer twin; NEEDED libspx.so found by
$ORIGIN; the loader's argtypes; the ABI version; the build -- is in tests/test_batch_libraries.py, for all seven."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from batch_libs import header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, BINF = "spx_proxstep_indball_l0_batch", "spx_proxstep_indball_l0_binf_batch"
HEAD = ["spx_ctx* ctx", "double* y", "const double* q", "const double* xk", "const double* sj", "int64_t n", "int64_t batch",
        "int64_t ld", "const int64_t* r"]
ARGS = {PLAIN: HEAD + ["const double* q_scale", "double* xkn", "double* stats_dev"],
        BINF: HEAD + ["const double* delta", "const double* q_scale", "double* xkn", "double* stats_dev"]}
I64_BY_VALUE = [5, 6, 7]
HEADER = os.path.join(ROOT, "include", "spx_topr_batch.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_text():
    return open(HEADER).read()


@pytest.mark.parametrize("name", [PLAIN, BINF])
def test_header_declares_the_calls(name):
    args = [" ".join(a.split()) for a in header_declarations(HEADER)[name].split(",")]
    assert args == ARGS[name], args
    # the single call's vectors under their names, r and delta as device arrays, plus batch, ld, q_scale, xkn and stats_dev
    single = header_declarations(os.path.join(ROOT, "include", "spx.h"))[name.replace("proxstep", "prox").replace("_batch", "")]
    names = lambda decl: [a.split()[-1].lstrip("*") for a in decl.split(",")]
    batched = names(header_declarations(HEADER)[name])
    assert sorted(batched) == sorted(names(single) + ["batch", "ld", "q_scale", "xkn", "stats_dev"])
    assert batched[:6] == names(single)[:6]


def test_header_states_the_contract():
    txt = " ".join(re.sub(r"\n \*", "\n", _header_text()).split())   # (the comment's line breaks and their stars dropped)
    for word in ("ALIGNMENT CLASS", "16-byte pairs form when ld is even", "element-wise form for EVERY row", "ONE rounded multiply",
                 "r, delta, q_scale : DEVICE int64_t[batch], double[batch], double[batch]", "r[b] <= 0 keeps nothing",
                 "r[b] >= n keeps everything", "has the BITS of spx_prox_indball_l0[_binf]", "ties to the lowest index first",
                 "all NaNs one key above Inf", "exact (a NaN counts as nonzero)", "0 iff stats_dev[3 b] <= r[b]",
                 "the count is what the caller cannot recover from h", "q AS PASSED", "fixed order", "batch-of-1",
                 "workspace: NONE", "capturable cold", "n > 2^20", "spx_prox_indball_l0[_binf] spreads such a problem",
                 "2^31 - 1", "no memset node", "fixed cap of passes", "y equal to q, xk or sj",
                 "a NULL r, delta, q_scale or stats_dev", "only its stores drop to 8 bytes", "touches that row's y and sums only"):
        assert word in txt, word
    # the sentence of spx.h about the missing single step form stays as it is
    spx_h = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "spx.h")).read()).split())
    assert "no top-r form (its h is 0 at any prox result)" in spx_h


def test_library_links_against_libspx_and_reserves_no_workspace(built):
    if not shutil.which("nm"):
        pytest.skip("no binutils")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", built._lib.TOPR_BATCH_LIB_PATH], check=True, capture_output=True,
                               text=True).stdout
    assert "spx_set_error" in undefined and "spx_zero_async" in undefined   # what it takes from libspx.so ...
    assert "spx_ws_reserve" not in undefined                                # ... and what it does not: workspace NONE
    for name in ("spx_topr_batch.hip", "spx_row_batch.hpp"):     # the call's own file and the row-owner site it shares
        src = open(os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc", name)).read()
        assert "spx_ws_reserve(" not in src and "hipMemsetAsync" not in src and "ctx->sync" not in src, name


def test_ctypes_table_binds_the_calls(built):
    sig = built._lib.TOPR_BATCH_SIGNATURES
    for name, args in ARGS.items():
        assert len(sig[name]) == len(args), sig[name]
        for k, t in enumerate(sig[name]):
            assert t is (ctypes.c_int64 if k in I64_BY_VALUE else ctypes.c_void_p), (name, k, t)
        assert [k for k, a in enumerate(args) if a.startswith("int64_t")] == I64_BY_VALUE
        fn = getattr(built._lib.load_topr_batch(), name)
        assert list(fn.argtypes) == sig[name] and fn.restype is ctypes.c_int


def test_mirror_takes_the_parameters_per_problem_on_the_device(built):
    import torch
    for f in (built.prox_step_topr_batch_bang, built.prox_step_topr_batch):
        names = list(inspect.signature(f).parameters)
        assert names[-5:] == ["r", "q_scale", "delta", "xkn", "out"], names
        assert inspect.signature(f).parameters["delta"].default is None
    assert list(inspect.signature(built.prox_step_topr_batch_bang).parameters)[:4] == ["Y", "Q", "XK", "SJ"]
    src = inspect.getsource(built.prox_step_topr_batch_bang)
    assert "_batch_matrix(" in src and "_batch_params(" in src and "torch.int64" in src
    like = torch.zeros(3, 8, dtype=torch.float64)
    # the call itself refuses what it can see before it looks for a device: host tensors, Y among the inputs
    with pytest.raises(TypeError):
        built.prox_step_topr_batch_bang(like.clone(), like, like, like, torch.ones(3, dtype=torch.int64),
                                        torch.ones(3, dtype=torch.float64))
    doc = built.prox_step_topr_batch_bang.__doc__
    for word in ("delta", "ShiftedIndBallL0BInf", "spx_proxstep_indball_l0_binf_batch", "alignment class", "DEVICE", "int64", "BITS",
                 "2^20"):
        assert word in doc, word
    assert "prox_step_topr_batch" in built.__all__ and "prox_step_topr_batch_bang" in built.__all__
