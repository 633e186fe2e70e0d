"""CPU: the fused prox! + step statistics entry points of the group operators (spx_proxstep_group_l2[_binf]) exist at every
layer that can be looked at without a GPU -- include/spx.h declares them with the arguments of spx_proxval_group_l2[_binf] up
to q_scale followed by `double* xkn, double* stats, double* stats_dev`, libspx.so exports them, the ctypes table binds them
with the header's argument counts, there is no host-pointer twin, and the mirror's docstring names both operators."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"spx_proxstep_group_l2": 15, "spx_proxstep_group_l2_binf": 16}
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


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_header_declares_group_proxstep(name):
    decl = _header_declarations()
    assert name in decl
    args = [" ".join(a.split()) for a in decl[name].split(",")]
    assert len(args) == SYMBOLS[name], args
    assert args[0] == "spx_ctx* ctx" and args[-3:] == TAIL and args[-4] == "double q_scale", args
    # ... in front of them the arguments of spx_proxval_group_* up to and including q_scale
    val = [" ".join(a.split()) for a in decl[name.replace("proxstep", "proxval")].split(",")]
    assert val[-1] == "double* value" and args[:-3] == val[:-1], (args, val)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_library_exports_group_proxstep(built, name):
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    assert hasattr(lib, name), "libspx.so lacks " + name


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_ctypes_table_binds_group_proxstep(built, name):
    sig = built._lib.SIGNATURES
    assert name in sig
    assert len(sig[name]) == SYMBOLS[name], sig[name]
    assert sig[name][:-3] == sig[name.replace("proxstep", "proxval")][:-1] and sig[name][-4] is ctypes.c_double


def test_no_host_twin_anywhere(built):
    assert not [k for k in built._lib.SIGNATURES if k.startswith("spx_host_proxstep")]
    assert not [k for k in _header_declarations() if k.startswith("spx_host_proxstep")]
    lib = ctypes.CDLL(built._lib.LIB_PATH)
    for name in SYMBOLS:
        assert not hasattr(lib, "spx_host_" + name[4:])


def test_mirror_documents_both_operators(built):
    doc = built.group_prox_step_bang.__doc__
    assert "ShiftedGroupNormL2" in doc.replace("ShiftedGroupNormL2Binf", "") and "ShiftedGroupNormL2Binf" in doc
    for word in ("h ", "qy", "yy", "xkn", "UNSCALED", "ALL"):
        assert word in doc, word
    assert built.group_prox_step.__doc__
    # the separable call keeps refusing the group operators and says where to go
    assert "group_prox_step_bang" in built.prox_step_bang.__doc__
