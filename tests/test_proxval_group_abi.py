"""CPU: the fused prox! + value entry points of the group operators exist at every layer that can be looked at without a GPU
-- include/spx.h declares them, libspx.so exports them, the ctypes table binds them with the header's argument counts."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"spx_proxval_group_l2": 13, "spx_proxval_group_l2_binf": 14}


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


def test_header_declares_group_proxval():
    decl = _header_declarations()
    for name, nargs in SYMBOLS.items():
        assert name in decl, name
        args = [a.strip() for a in decl[name].split(",")]
        assert len(args) == nargs, (name, args)
        assert args[0] == "spx_ctx* ctx" and args[-1] == "double* value" and args[-2] == "double q_scale", (name, args)


def test_library_exports_group_proxval(built):
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), "libspx.so lacks " + name


def test_ctypes_table_binds_group_proxval(built):
    for name, nargs in SYMBOLS.items():
        assert name in built._lib.SIGNATURES, name
        assert len(built._lib.SIGNATURES[name]) == nargs, (name, built._lib.SIGNATURES[name])
        assert not ("spx_host_" + name[4:]) in built._lib.SIGNATURES   # device pointers only: no host-pointer twin


def test_mirror_documents_group_forms(built):
    doc = built.prox_value_bang.__doc__
    assert "ShiftedGroupNormL2" in doc and "ShiftedGroupNormL2Binf" in doc
