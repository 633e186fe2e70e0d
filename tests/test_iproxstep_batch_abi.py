"""CPU: the batched iprox! + step statistics entry points (spx_iproxstep_{l1,l0}[_box]_batch) exist at every layer that can be
looked at without a GPU -- include/spx_ibatch.h (a header of its own: the call lives in libspx_ibatch.so, next to libspx.so and
libspx_batch.so) declares the four with `int64_t n, int64_t batch, int64_t ld` followed by the device parameter arrays and
`double* xkn, double* stats_dev`, libspx_ibatch.so exports them, the ctypes table (IBATCH_SIGNATURES) binds exactly the declared
set with n, batch and ld by value and pointers elsewhere, there is no host-pointer twin, the ABI version is unchanged, and the
mirror's docstring names the four sums and d_shift."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"l1": 14, "l0": 14, "l1_box": 16, "l0_box": 16}   # operator -> argument count
HEAD = ["spx_ctx* ctx", "double* y", "const double* g", "const double* d", "const double* xk", "const double* sj", "int64_t n",
        "int64_t batch", "int64_t ld", "const double* lambda", "const double* d_shift"]
TAIL = ["double* xkn", "double* stats_dev"]
FLAG = ["int32_t* d_flag"]
BOX = ["const double* l", "const double* u", "const uint8_t* sel_mask"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_declarations():
    txt = open(os.path.join(ROOT, "include", "spx_ibatch.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(spx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


def test_header_is_additive_and_includes_spx_h():
    txt = open(os.path.join(ROOT, "include", "spx_ibatch.h")).read()
    assert '#include "spx.h"' in txt
    assert sorted(_header_declarations()) == sorted("spx_iproxstep_%s_batch" % op for op in OPS)


@pytest.mark.parametrize("op", sorted(OPS))
def test_header_declares_iproxstep_batch(op):
    decl = _header_declarations()
    name = "spx_iproxstep_%s_batch" % op
    assert name in decl
    args = [" ".join(a.split()) for a in decl[name].split(",")]
    assert len(args) == OPS[op], args
    assert args == HEAD + (BOX if op.endswith("_box") else FLAG) + TAIL, args


@pytest.mark.parametrize("op", sorted(OPS))
def test_library_exports_iproxstep_batch(built, op):
    lib = built._lib.load_ibatch()
    assert os.path.basename(built._lib.IBATCH_LIB_PATH) == "libspx_ibatch.so"
    assert hasattr(lib, "spx_iproxstep_%s_batch" % op), "libspx_ibatch.so lacks spx_iproxstep_%s_batch" % op


@pytest.mark.parametrize("op", sorted(OPS))
def test_ctypes_table_binds_iproxstep_batch(built, op):
    sig = built._lib.IBATCH_SIGNATURES
    assert sorted(sig) == sorted(_header_declarations())      # the table binds exactly the declared set
    name = "spx_iproxstep_%s_batch" % op
    assert name in sig
    assert len(sig[name]) == OPS[op], sig[name]
    # n, batch, ld by value; everything else -- the per-problem scalars, d_shift and d_flag included -- is a pointer
    assert sig[name][6:9] == [ctypes.c_int64] * 3
    assert all(t is ctypes.c_void_p for t in sig[name][:6] + sig[name][9:]), sig[name]
    assert "spx_host_iproxstep_%s_batch" % op not in sig      # device pointers only: no host-pointer twin


def test_no_host_twin_and_the_abi_version_stays(built):
    for table in (built._lib.SIGNATURES, built._lib.BATCH_SIGNATURES, built._lib.IBATCH_SIGNATURES, _header_declarations()):
        assert not [k for k in table if k.startswith("spx_host_") and k.endswith("_batch")]
    lib, ilib = ctypes.CDLL(built._lib.LIB_PATH), built._lib.load_ibatch()
    for op in OPS:
        assert not hasattr(lib, "spx_host_iproxstep_%s_batch" % op) and not hasattr(ilib, "spx_host_iproxstep_%s_batch" % op)
        assert not hasattr(lib, "spx_iproxstep_%s_batch" % op)       # the new entry points live in the third library only
    lib.spx_abi_version.restype = ctypes.c_int
    assert lib.spx_abi_version() == 1                        # the change is additive


def test_mirror_documents_the_four_sums_and_d_shift(built):
    doc = built.iprox_step_batch_bang.__doc__
    for word in ("h ", "gy", "ydy", "yy", "xkn", "d_shift", "d_flag", "SELECTED", "ALL", "DEVICE", "row stride", "ONE rounded add"):
        assert word in doc, word
    assert built.iprox_step_batch.__doc__
