"""CPU: the fused prox! + step statistics entry point of ShiftedNormL1B2 exists at every layer that can be looked at without a
GPU -- include/spx.h declares it, libspx.so exports it, the ctypes table binds it with the header's argument count, there is no
host-pointer twin, the mirror's docstring names the operator."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "spx_proxstep_l1_b2", 14


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


def test_header_declares_b2_proxstep():
    decl = _header_declarations()
    assert NAME in decl
    args = [" ".join(a.split()) for a in decl[NAME].split(",")]
    assert len(args) == NARGS, args
    # the first 11: spx_proxval_l1_b2's without `value`; then the tail of spx_proxstep_*
    val = [" ".join(a.split()) for a in decl["spx_proxval_l1_b2"].split(",")]
    assert val[-1] == "double* value" and args[:11] == val[:-1], (args, val)
    assert args[11:] == ["double* xkn", "double* stats", "double* stats_dev"], args
    sep = [" ".join(a.split()) for a in decl["spx_proxstep_l1"].split(",")]
    assert args[10:] == sep[-4:], (args, sep)


def test_library_exports_b2_proxstep(built):
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    assert hasattr(lib, NAME), "libspx.so lacks " + NAME


def test_ctypes_table_binds_b2_proxstep(built):
    sig = built._lib.SIGNATURES
    assert NAME in sig
    assert len(sig[NAME]) == NARGS, sig[NAME]
    assert sig[NAME][:11] == sig["spx_proxval_l1_b2"][:-1]
    assert sig[NAME][10:] == sig["spx_proxstep_l1"][-4:]
    assert "spx_host_" + NAME[4:] not in sig   # device pointers only: no host-pointer twin
    assert "spx_host_" + NAME[4:] not in _header_declarations()


def test_mirror_documents_b2_step(built):
    assert "ShiftedNormL1B2" in built.b2_prox_step_bang.__doc__
    assert built.b2_prox_step is not None and "b2_prox_step" in built.__all__
