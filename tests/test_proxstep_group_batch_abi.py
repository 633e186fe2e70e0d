"""CPU: what is specific to the batched group prox! + step statistics entry point (spx_proxstep_group_l2_batch,
include/spx_gbatch.h, libspx_gbatch.so): the header declares it with `int64_t group_size, int64_t ngroups, int64_t batch,
int64_t ld`, the weights as `lambda_vec, ldl, lambda_scale` and the device parameter arrays, the ctypes table (GBATCH_SIGNATURES)
binds it with the five integers by value and pointers elsewhere, the header states the alignment classes, and the mirror's
docstring names the three sums and the weights' layout.

What holds for every batched library alike -- the header compiles alone as C99 and C++11, includes spx.h and declares exactly
the ctypes table's names; the library exports them and no other library does; no host-pointer twin; NEEDED libspx.so found by
$ORIGIN; the loader's argtypes; the ABI version; the build -- is in tests/test_batch_libraries.py, for all seven."""
import ctypes
import os
import re

import pytest

from batch_libs import header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spx_gbatch.h")
NAME = "spx_proxstep_group_l2_batch"
ARGS = ["spx_ctx* ctx", "double* y", "const double* q", "const double* xk", "const double* sj", "int64_t group_size",
        "int64_t ngroups", "int64_t batch", "int64_t ld", "const double* lambda_vec", "int64_t ldl", "const double* lambda_scale",
        "const double* sigma", "const double* q_scale", "double* xkn", "double* stats_dev"]
BY_VALUE = [5, 6, 7, 8, 10]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_text():
    return open(os.path.join(ROOT, "include", "spx_gbatch.h")).read()


def test_header_declares_the_call():
    args = [" ".join(a.split()) for a in header_declarations(HEADER)[NAME].split(",")]
    assert args == ARGS, args


def test_header_states_the_alignment_classes_and_the_refusals():
    txt = " ".join(re.sub(r"\n \*", "\n", _header_text()).split())   # (the comment's line breaks and their stars dropped)
    for word in ("ALIGNMENT CLASS", "16-byte pairs form when group_size is even, ld is even", "element-wise form for EVERY row",
                 "ldl == 0", "ONE rounded multiply", "group_size < 1 or > 512", "spx_proxstep_group_l2 serves larger groups",
                 "no memset node", "2^31 - 1"):
        assert word in txt, word


def test_ctypes_table_binds_the_call(built):
    sig = built._lib.GBATCH_SIGNATURES
    assert len(sig[NAME]) == len(ARGS), sig[NAME]
    for k, t in enumerate(sig[NAME]):
        assert t is (ctypes.c_int64 if k in BY_VALUE else ctypes.c_void_p), (k, t)
    assert [k for k, a in enumerate(ARGS) if a.startswith("int64_t")] == BY_VALUE


def test_mirror_documents_the_sums_and_the_weights(built):
    doc = built.prox_step_group_batch_bang.__doc__
    for word in ("h ", "qy", "yy", "xkn", "lam_scale", "ONE rounded multiply", "ldl", "UNSCALED", "DEVICE", "row stride",
                 "alignment class", "1 .. 512"):
        assert word in doc, word
    assert built.prox_step_group_batch.__doc__
