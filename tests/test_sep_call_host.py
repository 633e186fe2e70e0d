"""CPU: the members of SepCall (csrc/spx_common.hpp) that state "every vector of a separable call" -- the head shift, the Float64
and the Float32 alignment predicates, the list xkn must not be in -- against the hand-written enumerations they replaced, in a
stand-alone program (tests/c/sep_call_driver.hip, its own main) built with AddressSanitizer + UBSan on the host side and run as
a child.  Nothing is put into LD_PRELOAD and the library is not loaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_sep_call_members_sanitized(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "sep_call_driver")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "sep_call_driver.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
