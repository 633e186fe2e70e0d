"""CPU: what is specific to the batched ShiftedNormL1B2 prox! + step statistics entry point (spx_proxstep_l1_b2_batch,
include/spx_b2_batch.h, libspx_b2_batch.so): the header declares the call as the single one's with the per-problem scalars as
device arrays and states its contract, the ctypes table (B2_BATCH_SIGNATURES) binds it with the three integers and chi_lambda by
value and pointers elsewhere, and the mirror takes lambda, sigma, delta and q_scale as per-problem device tensors: anything else
is refused.

What holds for every batched library alike -- the header compiles alone as C99 and C++11, includes spx.h and declares exactly
the ctypes table's names; the library exports them and no other library does; no host-pointer twin; NEEDED libspx.so found by
$ORIGIN; the loader's argtypes; the ABI version; the build -- is in tests/test_batch_libraries.py, for all seven."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from batch_libs import header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "spx_proxstep_l1_b2_batch"
ARGS = ["spx_ctx* ctx", "double* y", "const double* q", "const double* xk", "const double* sj", "int64_t n", "int64_t batch",
        "int64_t ld", "const double* lambda", "const double* sigma", "const double* delta", "const double* q_scale",
        "double chi_lambda", "double* xkn", "double* stats_dev"]
I64_BY_VALUE = [5, 6, 7]
F64_BY_VALUE = [12]
HEADER = os.path.join(ROOT, "include", "spx_b2_batch.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_text():
    return open(HEADER).read()


def test_header_declares_the_call():
    args = [" ".join(a.split()) for a in header_declarations(HEADER)[NAME].split(",")]
    assert args == ARGS, args
    # the single call's vectors and scalars under their names (the per-problem ones as device arrays), plus batch and ld; no
    # host destination
    single = header_declarations(os.path.join(ROOT, "include", "spx.h"))["spx_proxstep_l1_b2"]
    names = lambda decl: [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert sorted(names(header_declarations(HEADER)[NAME])) == sorted([a for a in names(single) if a != "stats"] + ["batch", "ld"])
    assert names(header_declarations(HEADER)[NAME])[:6] == names(single)[:6]


def test_header_states_the_contract():
    txt = " ".join(re.sub(r"\n \*", "\n", _header_text()).split())   # (the comment's line breaks and their stars dropped)
    for word in ("ALIGNMENT CLASS", "16-byte pairs form when ld is even", "element-wise form for EVERY row", "ONE rounded multiply",
                 "lambda, sigma, delta, q_scale : DEVICE double[batch]", "chi_lambda : one host double", "NOT promised",
                 "inactive", "1e-12", "q AS PASSED", "fixed order", "batch-of-1", "workspace: NONE", "n > 2^20",
                 "spx_proxstep_l1_b2 holds such a problem", "2^31 - 1", "no memset node", "fixed cap of reductions",
                 "a NULL lambda, sigma, delta, q_scale or stats_dev", "NON-FINITE DATA", "only its stores drop to 8 bytes"):
        assert word in txt, word


def test_ctypes_table_binds_the_call(built):
    sig = built._lib.B2_BATCH_SIGNATURES
    assert len(sig[NAME]) == len(ARGS), sig[NAME]
    for k, t in enumerate(sig[NAME]):
        want = ctypes.c_int64 if k in I64_BY_VALUE else ctypes.c_double if k in F64_BY_VALUE else ctypes.c_void_p
        assert t is want, (k, t)
    assert [k for k, a in enumerate(ARGS) if a.startswith("int64_t")] == I64_BY_VALUE
    assert [k for k, a in enumerate(ARGS) if a.startswith("double ")] == F64_BY_VALUE
    fn = getattr(built._lib.load_b2_batch(), NAME)
    assert list(fn.argtypes) == sig[NAME] and fn.restype is ctypes.c_int


def test_mirror_takes_the_scalars_per_problem_on_the_device(built):
    import torch
    shifted = sys.modules[built.prox_step_b2_batch_bang.__module__]   # (the package's `shifted` is the function)
    for f in (built.prox_step_b2_batch_bang, built.prox_step_b2_batch):
        names = list(inspect.signature(f).parameters)
        assert names[names.index("lam"):names.index("lam") + 5] == ["lam", "sigma", "delta", "q_scale", "chi_lambda"], names
        assert inspect.signature(f).parameters["chi_lambda"].default == 1.0
        assert names[-2:] == ["xkn", "out"]
    src = inspect.getsource(built.prox_step_b2_batch_bang)
    assert "_batch_matrix(" in src and "_batch_params(" in src
    for name in ("lam", "sigma", "delta", "q_scale"):
        assert '(%s, "%s")' % (name, name) in src, name                # checked through _batch_params
    like = torch.zeros(3, 8, dtype=torch.float64)
    for bad in (0.3, [0.3, 0.3, 0.3], torch.full((3,), 0.3, dtype=torch.float64), torch.full((3,), 0.3, dtype=torch.float32),
                torch.full((3, 1), 0.3, dtype=torch.float64)):
        with pytest.raises(TypeError, match="delta must be a contiguous 1-D float64 device tensor"):
            shifted._batch_params(bad, "delta", 3, like)
    # the call itself refuses what it can see before it looks for a device: host tensors
    with pytest.raises(TypeError):
        built.prox_step_b2_batch_bang(like.clone(), like, like, like, torch.ones(3, dtype=torch.float64),
                                      torch.ones(3, dtype=torch.float64), torch.full((3,), 0.3, dtype=torch.float64),
                                      torch.ones(3, dtype=torch.float64))
    doc = built.prox_step_b2_batch_bang.__doc__
    for word in ("delta", "ShiftedNormL1B2", "spx_proxstep_l1_b2_batch", "alignment class", "DEVICE", "inactive", "2^20"):
        assert word in doc, word
    assert "prox_step_b2_batch" in built.__all__ and "prox_step_b2_batch_bang" in built.__all__
