"""CPU: the fused prox! + value entry point of ShiftedNormL1B2 exists at every layer that can be looked at without a GPU --
include/spx.h declares it, libspx.so exports it, the ctypes table binds it with the header's argument count, the mirror's
docstring names the operator."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "spx_proxval_l1_b2", 12


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


def test_header_declares_b2_proxval():
    decl = _header_declarations()
    assert NAME in decl
    args = [" ".join(a.split()) for a in decl[NAME].split(",")]
    assert len(args) == NARGS, args
    assert args[0] == "spx_ctx* ctx" and args[-2] == "double q_scale" and args[-1] == "double* value", args
    # ... and the plain prox's arguments in between, in its order
    plain = [" ".join(a.split()) for a in decl["spx_prox_l1_b2"].split(",")]
    assert args[:-2] == plain, (args, plain)


def test_library_exports_b2_proxval(built):
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    assert hasattr(lib, NAME), "libspx.so lacks " + NAME


def test_ctypes_table_binds_b2_proxval(built):
    sig = built._lib.SIGNATURES
    assert NAME in sig
    assert len(sig[NAME]) == NARGS, sig[NAME]
    assert sig[NAME][:-2] == sig["spx_prox_l1_b2"] and sig[NAME][-2] is ctypes.c_double
    assert "spx_host_" + NAME[4:] not in sig   # device pointers only: no host-pointer twin


def test_mirror_documents_b2(built):
    assert "ShiftedNormL1B2" in built.prox_value_bang.__doc__
