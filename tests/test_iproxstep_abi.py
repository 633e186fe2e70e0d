"""CPU: the fused iprox! + step statistics entry points (spx_iproxstep_*) exist at every layer that can be looked at without
a GPU -- include/spx.h declares the four with the argument list of the matching spx_iprox_X followed by
`double* xkn, double* stats, double* stats_dev`, libspx.so exports them, the ctypes table binds them with the header's
argument count, there is no host-pointer twin, and the mirror's docstring names the four sums."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"l1": 12, "l0": 12, "l1_box": 16, "l0_box": 16}   # operator -> argument count
TAIL = ["double* xkn", "double* stats", "double* stats_dev"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_declarations():
    txt = open(os.path.join(ROOT, "include", "spx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(spx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


@pytest.mark.parametrize("op", sorted(OPS))
def test_header_declares_iproxstep(op):
    decl = _header_declarations()
    name = "spx_iproxstep_" + op
    assert name in decl
    args = [" ".join(a.split()) for a in decl[name].split(",")]
    assert len(args) == OPS[op], args
    assert args[-3:] == TAIL, args
    plain = [" ".join(a.split()) for a in decl["spx_iprox_" + op].split(",")]
    assert args[:-3] == plain, (args, plain)          # the argument list of spx_iprox_X in front: no q_scale


@pytest.mark.parametrize("op", sorted(OPS))
def test_library_exports_iproxstep(built, op):
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    assert hasattr(lib, "spx_iproxstep_" + op), "libspx.so lacks spx_iproxstep_" + op


@pytest.mark.parametrize("op", sorted(OPS))
def test_ctypes_table_binds_iproxstep(built, op):
    sig = built._lib.SIGNATURES
    name = "spx_iproxstep_" + op
    assert name in sig
    assert len(sig[name]) == OPS[op], sig[name]
    assert sig[name][:-3] == sig["spx_iprox_" + op]
    assert sig[name][-3] is ctypes.c_void_p and sig[name][-1] is ctypes.c_void_p
    assert "spx_host_iproxstep_" + op not in sig      # device pointers only: no host-pointer twin


def test_no_host_twin_and_no_f32_form_anywhere(built):
    assert not [k for k in built._lib.SIGNATURES if k.startswith("spx_host_iproxstep")]
    decl = _header_declarations()
    assert not [k for k in decl if k.startswith("spx_host_iproxstep")]
    assert sorted(k for k in decl if k.startswith("spx_iproxstep")) == sorted("spx_iproxstep_" + op for op in OPS)
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    for op in OPS:
        assert not hasattr(lib, "spx_host_iproxstep_" + op)
        assert not hasattr(lib, "spx_iproxstep_" + op + "_f32")


def test_mirror_documents_the_four_sums(built):
    doc = built.iprox_step_bang.__doc__
    for word in ("h ", "gy", "ydy", "yy", "xkn", "SELECTED", "ALL"):
        assert word in doc, word
    assert built.iprox_step.__doc__
    assert "iprox_step" in built.__all__ and "iprox_step_bang" in built.__all__
