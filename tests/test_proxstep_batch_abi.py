"""CPU: what is specific to the batched prox! + step statistics entry points (spx_proxstep_{l1,l0}[_box]_batch, include/spx_batch.h,
libspx_batch.so): the header declares the four with `int64_t n, int64_t batch, int64_t ld` followed by the device parameter arrays
and `double* xkn, double* stats_dev`, the library has them, the ctypes table (BATCH_SIGNATURES) binds them with the header's
argument count, n, batch and ld by value and pointers elsewhere, and the mirror's docstring names the three sums.

What holds for every batched library alike -- the header compiles alone as C99 and C++11, includes spx.h and declares exactly
the ctypes table's names; the library exports them and no other library does; no host-pointer twin; NEEDED libspx.so found by
$ORIGIN; the loader's argtypes; the ABI version; the build -- is in tests/test_batch_libraries.py, for all seven."""
import ctypes
import os

import pytest

from batch_libs import header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spx_batch.h")
OPS = {"l1": 13, "l0": 13, "l1_box": 16, "l0_box": 16}   # operator -> argument count
HEAD = ["spx_ctx* ctx", "double* y", "const double* q", "const double* xk", "const double* sj", "int64_t n", "int64_t batch",
        "int64_t ld", "const double* lambda", "const double* sigma"]
TAIL = ["const double* q_scale", "double* xkn", "double* stats_dev"]
BOX = ["const double* l", "const double* u", "const uint8_t* sel_mask"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


@pytest.mark.parametrize("op", sorted(OPS))
def test_header_declares_proxstep_batch(op):
    decl = header_declarations(HEADER)
    name = "spx_proxstep_%s_batch" % op
    assert name in decl
    args = [" ".join(a.split()) for a in decl[name].split(",")]
    assert len(args) == OPS[op], args
    assert args == HEAD + (BOX if op.endswith("_box") else []) + TAIL, args


@pytest.mark.parametrize("op", sorted(OPS))
def test_library_exports_proxstep_batch(built, op):
    lib = built._lib.load_batch()
    assert hasattr(lib, "spx_proxstep_%s_batch" % op), "libspx_batch.so lacks spx_proxstep_%s_batch" % op


@pytest.mark.parametrize("op", sorted(OPS))
def test_ctypes_table_binds_proxstep_batch(built, op):
    sig = built._lib.BATCH_SIGNATURES
    name = "spx_proxstep_%s_batch" % op
    assert name in sig
    assert len(sig[name]) == OPS[op], sig[name]
    # n, batch, ld by value; everything else -- the per-problem scalars included -- is a pointer
    assert sig[name][5:8] == [ctypes.c_int64] * 3
    assert all(t is ctypes.c_void_p for t in sig[name][:5] + sig[name][8:]), sig[name]
    assert "spx_host_proxstep_%s_batch" % op not in sig      # device pointers only: no host-pointer twin


def test_mirror_documents_the_three_sums(built):
    doc = built.prox_step_batch_bang.__doc__
    for word in ("h ", "qy", "yy", "xkn", "UNSCALED", "SELECTED", "ALL", "DEVICE", "row stride"):
        assert word in doc, word
    assert built.prox_step_batch.__doc__
