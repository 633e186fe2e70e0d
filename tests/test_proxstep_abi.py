"""CPU: the fused prox! + step statistics entry points (spx_proxstep_*) exist at every layer that can be looked at without
a GPU -- include/spx.h declares the six with the arguments of the matching spx_proxval_X up to q_scale followed by
`double* xkn, double* stats, double* stats_dev`, libspx.so exports them, the ctypes table binds them with the header's
argument count, there is no host-pointer twin, and the mirror's docstring names the three sums."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"l1": 12, "l0": 12, "lhalf": 12, "l1_box": 17, "l0_box": 17, "lhalf_box": 17}   # operator -> argument count
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
def test_header_declares_proxstep(op):
    decl = _header_declarations()
    name = "spx_proxstep_" + op
    assert name in decl
    args = [" ".join(a.split()) for a in decl[name].split(",")]
    assert len(args) == OPS[op], args
    assert args[-3:] == TAIL and args[-4] == "double q_scale", args
    # ... in front of them the arguments of spx_proxval_X up to and including q_scale
    val = [" ".join(a.split()) for a in decl["spx_proxval_" + op].split(",")]
    assert val[-1] == "double* value" and args[:-3] == val[:-1], (args, val)


@pytest.mark.parametrize("op", sorted(OPS))
def test_library_exports_proxstep(built, op):
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    assert hasattr(lib, "spx_proxstep_" + op), "libspx.so lacks spx_proxstep_" + op


@pytest.mark.parametrize("op", sorted(OPS))
def test_ctypes_table_binds_proxstep(built, op):
    sig = built._lib.SIGNATURES
    name = "spx_proxstep_" + op
    assert name in sig
    assert len(sig[name]) == OPS[op], sig[name]
    assert sig[name][:-3] == sig["spx_proxval_" + op][:-1] and sig[name][-4] is ctypes.c_double
    assert "spx_host_proxstep_" + op not in sig      # device pointers only: no host-pointer twin


def test_no_host_twin_anywhere(built):
    assert not [k for k in built._lib.SIGNATURES if k.startswith("spx_host_proxstep")]
    assert not [k for k in _header_declarations() if k.startswith("spx_host_proxstep")]
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    for op in OPS:
        assert not hasattr(lib, "spx_host_proxstep_" + op)


def test_mirror_documents_the_three_sums(built):
    doc = built.prox_step_bang.__doc__
    for word in ("h ", "qy", "yy", "xkn", "UNSCALED", "SELECTED", "ALL"):
        assert word in doc, word
    assert built.prox_step.__doc__
