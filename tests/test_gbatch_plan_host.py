"""CPU: the device-free plan of the batched group call (csrc/spx_plan.hpp: gbatch_plan and the tile -> groups mapping that
k_group_batch walks, on the tile table of csrc/spx_group_common.hpp) -- every group in exactly one (problem, tile), tiles of
whole groups, every row element touched exactly once and no padding, the form as a function of (group_size, ngroups) alone,
grid and workspace, the refusal of a grid beyond 2^31 - 1 workgroups -- in a stand-alone program
(tests/c/gbatch_plan_driver.hip, its own main) built with AddressSanitizer + UBSan on the host side and run as a child.
Nothing is put into LD_PRELOAD and the library is not loaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gbatch_plan_covers_every_group_exactly_once_sanitized(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "gbatch_plan_driver")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "gbatch_plan_driver.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    lines = r.stdout.split()
    assert r.returncode == 0 and lines[-1:] == ["ok"], r.stdout[-2000:] + r.stderr[-4000:]
    # the grid of cases is there: 512 sizes x 21 counts x 8 batches x 4 paddings x 4 alignments, several checks each
    assert lines[1] == "checks" and int(lines[0]) > 5_000_000, r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
