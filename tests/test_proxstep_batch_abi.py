"""CPU: the batched prox! + step statistics entry points (spx_proxstep_{l1,l0}[_box]_batch) exist at every layer that can be
looked at without a GPU -- include/spx_batch.h (a header of its own: the call lives in libspx_batch.so, next to libspx.so) declares the four with `int64_t n, int64_t batch, int64_t ld` followed by the device
parameter arrays and `double* xkn, double* stats_dev`, libspx_batch.so exports them, the ctypes table (BATCH_SIGNATURES) binds them with the header's
argument count, there is no host-pointer twin, the ABI version is unchanged, and the mirror's docstring names the three sums."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _header_declarations():
    txt = open(os.path.join(ROOT, "include", "spx_batch.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(spx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


@pytest.mark.parametrize("op", sorted(OPS))
def test_header_declares_proxstep_batch(op):
    decl = _header_declarations()
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
    assert sorted(sig) == sorted(_header_declarations())      # the table binds exactly the declared set
    name = "spx_proxstep_%s_batch" % op
    assert name in sig
    assert len(sig[name]) == OPS[op], sig[name]
    # n, batch, ld by value; everything else -- the per-problem scalars included -- is a pointer
    assert sig[name][5:8] == [ctypes.c_int64] * 3
    assert all(t is ctypes.c_void_p for t in sig[name][:5] + sig[name][8:]), sig[name]
    assert "spx_host_proxstep_%s_batch" % op not in sig      # device pointers only: no host-pointer twin


def test_no_host_twin_and_the_abi_version_stays(built):
    for table in (built._lib.SIGNATURES, built._lib.BATCH_SIGNATURES, _header_declarations()):
        assert not [k for k in table if k.startswith("spx_host_") and k.endswith("_batch")]
    lib, blib = ctypes.CDLL(built._lib.LIB_PATH), built._lib.load_batch()
    for op in OPS:
        assert not hasattr(lib, "spx_host_proxstep_%s_batch" % op) and not hasattr(blib, "spx_host_proxstep_%s_batch" % op)
    lib.spx_abi_version.restype = ctypes.c_int
    assert lib.spx_abi_version() == 1                        # the change is additive


def test_mirror_documents_the_three_sums(built):
    doc = built.prox_step_batch_bang.__doc__
    for word in ("h ", "qy", "yy", "xkn", "UNSCALED", "SELECTED", "ALL", "DEVICE", "row stride"):
        assert word in doc, word
    assert built.prox_step_batch.__doc__
