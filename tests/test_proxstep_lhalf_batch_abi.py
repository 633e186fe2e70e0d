"""CPU: what is specific to the batched RootNormLhalf(Box) prox! + step statistics entry points (spx_proxstep_lhalf_batch,
spx_proxstep_lhalf_box_batch) and the threshold call (spx_lhalf_threshold_batch), include/spx_lhalf_batch.h,
libspx_lhalf_batch.so: the header declares exactly the three calls, word for word the NormL1 calls' argument lists, and states
their contract, the ctypes table (LHALF_BATCH_SIGNATURES) binds them with the integers by value and pointers elsewhere, and the
mirror has the new names (prox_step_batch_bang keeps refusing "lhalf").

What holds for every batched library alike -- the header compiles alone as C99 and C++11, includes spx.h and declares exactly
the ctypes table's names; the library exports them and no other library does; no host-pointer twin; NEEDED libspx.so found by
$ORIGIN; the loader's argtypes; the ABI version; the build -- is in tests/test_batch_libraries.py, for all seven.

The host side of the device threshold (csrc/spx_lhalf_threshold.hpp is __host__ __device__) is held to glibc's pow here too:
tests/c/lhalf_threshold_driver.cpp runs the header's statements on the host."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from batch_libs import header_declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spx_lhalf_batch.h")
PLAIN = ["spx_ctx* ctx", "double* y", "const double* q", "const double* xk", "const double* sj", "int64_t n", "int64_t batch",
         "int64_t ld", "const double* lambda", "const double* sigma", "const double* q_scale", "double* xkn", "double* stats_dev"]
BOX = PLAIN[:10] + ["const double* l", "const double* u", "const uint8_t* sel_mask"] + PLAIN[10:]
THRESHOLD = ["spx_ctx* ctx", "const double* lambda", "const double* sigma", "int64_t batch", "double* p_dev"]
DECLS = {"spx_proxstep_lhalf_batch": PLAIN, "spx_proxstep_lhalf_box_batch": BOX, "spx_lhalf_threshold_batch": THRESHOLD}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd


def _header_text():
    return open(HEADER).read()


def test_header_declares_exactly_the_three_calls():
    assert '#include "spx.h"' in _header_text()
    decl = header_declarations(HEADER)
    assert sorted(decl) == sorted(DECLS)
    for name, want in DECLS.items():
        args = [" ".join(a.split()) for a in decl[name].split(",")]
        assert args == want, (name, args)
    # word for word the argument lists of the NormL1 calls of spx_batch.h
    l1 = header_declarations(os.path.join(ROOT, "include", "spx_batch.h"))
    flat = lambda d: [" ".join(a.split()) for a in d.split(",")]
    assert flat(decl["spx_proxstep_lhalf_batch"]) == flat(l1["spx_proxstep_l1_batch"])
    assert flat(decl["spx_proxstep_lhalf_box_batch"]) == flat(l1["spx_proxstep_l1_box_batch"])


def test_header_states_the_contract():
    txt = " ".join(re.sub(r"\n \*", "\n", _header_text()).split())   # (the comment's line breaks and their stars dropped)
    for word in ("BOX FORM: row b has the bits of spx_proxstep_lhalf_box", "UNBOXED FORM", "<= 4 ulp(p_host)",
                 "(a <= p_host) == (a <= p_dev)", "strictly between the two thresholds, or equals the larger one",
                 "exactly 0.0 - (xk + sj) where a <= p_dev", "1e-12 * max(|y|, |xk + sj|, |q|)",
                 "always bit for bit (xk + sj) + y of the stored y", "always of the stored y", "q AS PASSED", "fixed order",
                 "never read or written", "ONE byte mask", "no host destination", "n > 12288 needs workspace", "2^31 - 1",
                 "no memset node", "batch == 0: SPX_OK", "a NULL parameter array", "stats_dev == NULL",
                 "spx_lhalf_threshold_batch stores p_dev itself", "a NULL lambda, sigma or p_dev", "touches that row's y and sums only"):
        assert word in txt, word


def test_ctypes_table_binds_the_calls(built):
    sig = built._lib.LHALF_BATCH_SIGNATURES
    for name, args in DECLS.items():
        assert len(sig[name]) == len(args), name
        for k, (t, a) in enumerate(zip(sig[name], args)):
            assert t is (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_void_p), (name, k, t)
        fn = getattr(built._lib.load_lhalf_batch(), name)
        assert list(fn.argtypes) == sig[name] and fn.restype is ctypes.c_int
    assert sig["spx_proxstep_lhalf_batch"] == built._lib.BATCH_SIGNATURES["spx_proxstep_l1_batch"]
    assert sig["spx_proxstep_lhalf_box_batch"] == built._lib.BATCH_SIGNATURES["spx_proxstep_l1_box_batch"]


def test_mirror_has_the_new_names(built):
    import torch
    for name in ("prox_step_lhalf_batch", "prox_step_lhalf_batch_bang", "lhalf_threshold_batch"):
        assert name in built.__all__, name
    for f in (built.prox_step_lhalf_batch_bang, built.prox_step_lhalf_batch):
        names = list(inspect.signature(f).parameters)
        assert names[-8:] == ["lam", "sigma", "q_scale", "l", "u", "selected", "xkn", "out"], names
        assert "kind" not in names
    assert list(inspect.signature(built.lhalf_threshold_batch).parameters) == ["lam", "sigma", "out"]
    src = inspect.getsource(built.prox_step_lhalf_batch_bang)
    assert "_batch_matrix(" in src and "_batch_params(" in src and "load_lhalf_batch()" in src
    like = torch.zeros(3, 8, dtype=torch.float64)
    ones = torch.ones(3, dtype=torch.float64)
    with pytest.raises(TypeError):      # host tensors: refused before a device is looked for
        built.prox_step_lhalf_batch_bang(like.clone(), like, like, like, ones, ones, ones)
    with pytest.raises(TypeError):
        built.lhalf_threshold_batch(ones, ones)
    with pytest.raises(TypeError):      # the old name keeps refusing the new operator
        built.prox_step_batch_bang(like.clone(), "lhalf", like, like, like, ones, ones, ones)
    doc = built.prox_step_lhalf_batch_bang.__doc__
    for word in ("RootNormLhalf", "spx_proxstep_lhalf[_box]_batch", "DEVICE", "4 ulps", "lhalf_threshold_batch", "UNSCALED Q"):
        assert word in doc, word


def test_threshold_routine_on_the_host_is_within_4_ulps_of_glibc_pow(tmp_path):
    """csrc/spx_lhalf_threshold.hpp compiled for the host (-ffp-contract=off, as the library): over sigma lambda = m 2^k, k from
    -500 to 500 in steps of 20 and three m in [1, 2) per k -- the sweep of the GPU test -- and 20000 more random ones, the routine
    is within 4 ulps of 54.0 ** (1/3) * (2 nl) ** (2/3) / 4 (Python's pow is glibc's, the one libspx.so's host code calls)."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "lhalf_threshold_driver")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "lhalf_threshold_driver.cpp"), "-o", exe])
    rng = np.random.default_rng(20260)
    nl = [m * 2.0 ** k for k in range(-500, 501, 20) for m in (1.0, 1.0 + float(rng.random()), 2.0 - 2.0 ** -52)]
    nl += [float(np.ldexp(1.0 + rng.random(), int(rng.integers(-1000, 1000)))) for _ in range(20000)]
    out = subprocess.run([exe], input="\n".join(v.hex() for v in nl) + "\n", check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(nl)
    worst = 0.0
    for v, line in zip(nl, out):
        p_host = 54.0 ** (1 / 3) * (2 * v) ** (2 / 3) / 4
        worst = max(worst, abs(float.fromhex(line) - p_host) / float(np.spacing(p_host)))
    assert worst <= 4.0, worst
