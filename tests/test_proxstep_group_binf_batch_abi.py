"""CPU: what is specific to the batched Binf group prox! + step statistics entry point (spx_proxstep_group_l2_binf_batch,
include/spx_gbinf_batch.h, libspx_gbinf_batch.so): the header declares the call as spx_proxstep_group_l2_batch's with
`const double* delta` between sigma and q_scale and states its contract, the ctypes table (GBINF_BATCH_SIGNATURES) binds it with
the five integers by value and pointers elsewhere, and the mirror takes delta as a per-problem device tensor: anything else is
refused.

What holds for every batched library alike -- the header compiles alone as C99 and C++11, includes spx.h and declares exactly
the ctypes table's names; the library exports them and no other library does; no host-pointer twin; NEEDED libspx.so found by
$ORIGIN; the loader's argtypes; the ABI version; the build -- is in tests/test_batch_libraries.py, for all seven."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from batch_libs import header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "spx_proxstep_group_l2_binf_batch"
ARGS = ["spx_ctx* ctx", "double* y", "const double* q", "const double* xk", "const double* sj", "int64_t group_size",
        "int64_t ngroups", "int64_t batch", "int64_t ld", "const double* lambda_vec", "int64_t ldl", "const double* lambda_scale",
        "const double* sigma", "const double* delta", "const double* q_scale", "double* xkn", "double* stats_dev"]
BY_VALUE = [5, 6, 7, 8, 10]
HEADER = os.path.join(ROOT, "include", "spx_gbinf_batch.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_text():
    return open(HEADER).read()


def test_header_declares_the_call_as_the_plain_one_plus_delta():
    args = [" ".join(a.split()) for a in header_declarations(HEADER)[NAME].split(",")]
    assert args == ARGS, args
    plain = header_declarations(os.path.join(ROOT, "include", "spx_gbatch.h"))["spx_proxstep_group_l2_batch"]
    assert [a for a in args if a != "const double* delta"] == [" ".join(a.split()) for a in plain.split(",")]


def test_header_states_the_contract():
    txt = " ".join(re.sub(r"\n \*", "\n", _header_text()).split())   # (the comment's line breaks and their stars dropped)
    for word in ("ALIGNMENT CLASS", "16-byte pairs form when group_size is even, ld is even", "element-wise form for EVERY row",
                 "ldl == 0", "ONE rounded multiply", "group_size < 1 or > 512", "spx_proxstep_group_l2_binf serves larger groups",
                 "no memset node", "2^31 - 1", "sigma, delta, q_scale : DEVICE double[batch]", "tuning key 9",
                 "a NULL lambda_vec, sigma, delta, q_scale or stats_dev", "literal"):
        assert word in txt, word


def test_ctypes_table_binds_the_call(built):
    sig = built._lib.GBINF_BATCH_SIGNATURES
    assert len(sig[NAME]) == len(ARGS), sig[NAME]
    for k, t in enumerate(sig[NAME]):
        assert t is (ctypes.c_int64 if k in BY_VALUE else ctypes.c_void_p), (k, t)
    assert [k for k, a in enumerate(ARGS) if a.startswith("int64_t")] == BY_VALUE
    fn = getattr(built._lib.load_gbinf_batch(), NAME)
    assert list(fn.argtypes) == sig[NAME] and fn.restype is ctypes.c_int


def test_mirror_takes_delta_per_problem_on_the_device(built):
    import torch
    shifted = sys.modules[built.prox_step_group_binf_batch_bang.__module__]   # (the package's `shifted` is the function)
    for f in (built.prox_step_group_binf_batch_bang, built.prox_step_group_binf_batch):
        names = list(inspect.signature(f).parameters)
        assert names[names.index("sigma"):names.index("sigma") + 3] == ["sigma", "delta", "q_scale"], names
    assert '(delta, "delta")' in inspect.getsource(built.prox_step_group_binf_batch_bang)   # checked like sigma and q_scale
    like = torch.zeros(3, 8, dtype=torch.float64)
    for bad in (0.3, [0.3, 0.3, 0.3], torch.full((3,), 0.3, dtype=torch.float64), torch.full((3,), 0.3, dtype=torch.float32),
                torch.full((3, 1), 0.3, dtype=torch.float64)):
        with pytest.raises(TypeError, match="delta must be a contiguous 1-D float64 device tensor"):
            shifted._batch_params(bad, "delta", 3, like)
    # the call itself refuses what it can see before it looks for a device: host tensors
    with pytest.raises(TypeError):
        built.prox_step_group_binf_batch_bang(like.clone(), like, like, like, 8, torch.ones(1, dtype=torch.float64),
                                              torch.ones(3, dtype=torch.float64), torch.full((3,), 0.3, dtype=torch.float64),
                                              torch.ones(3, dtype=torch.float64))
    doc = built.prox_step_group_binf_batch_bang.__doc__
    for word in ("delta", "ShiftedGroupNormL2Binf", "tuning key 9", "alignment class", "device"):
        assert word in doc, word
