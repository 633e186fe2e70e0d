"""CPU: the device-free plan of the batched Binf group call (csrc/spx_plan.hpp: gbatch_plan with the lanes per group of
GroupTilesBinf, and the bit walk of the literal phase -- binf_bitmap_words, binf_walk_passes, binf_walk_bit -- that k_binf_batch
of csrc/spx_gbinf_batch.hip uses) -- every group in exactly one (problem, tile), tiles of whole groups, a group's bitmap index
below the bitmap's capacity, every set bit visited exactly once and in ascending group order per wave (empty, full, single-bit,
alternating and random bitmaps), the form as a function of (group_size, ngroups) alone, the refusal of a grid beyond 2^31 - 1
workgroups -- in a stand-alone program (tests/c/gbinf_batch_plan_driver.hip, its own main) built with AddressSanitizer + UBSan
on the host side and run as a child.  Nothing is put into LD_PRELOAD and the library is not loaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gbinf_batch_plan_and_bit_walk_sanitized(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "gbinf_batch_plan_driver")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "gbinf_batch_plan_driver.hip"), "-o", exe]
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
