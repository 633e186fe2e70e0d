"""CPU: the device-free parts of the batched top-r calls (spx_proxstep_indball_l0[_binf]_batch) in a stand-alone program
(tests/c/topr_batch_plan_driver.hip, its own main) built with AddressSanitizer + UBSan on the host side and run as a child.
Nothing is put into LD_PRELOAD and the library is not loaded.

(a) row_batch_plan on kToprBatchShape (csrc/spx_plan.hpp; tests/c/row_batch_plan_checks.hpp) at n = 0, 1, 2, every tile edge +-1, 8192, 8193, 2^20 and 2^20 + 1, over all 32 alignment
    classes, even and odd ld and seven batch sizes: every element of every row is visited by exactly one lane slot, form and
    tile are functions of n alone, refusals come at the grid and n bounds.
(b) the selection of csrc/spx_topr_row.hpp -- the one k_topr_batch runs -- on host arrays with histograms built by a plain loop:
    the kept set against a stable descending sort by |v| for EVERY r in {-1, 0, ..., n + 1}, on random values, a constant with
    alternating sign, a 2^-8 lattice, values over 2^+-500, two keys that differ in the last bit, NaNs and +-Inf mixed in, and all
    zeros; n = 1, 2, 3, 64, 65, 1000 need one index digit, n = 4097 (13 index bits) and n = 8193 two."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("topr_batch_plan") / "topr_batch_plan_driver")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "topr_batch_plan_driver.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    return subprocess.run([exe], env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=600)


def test_topr_batch_plan_and_selection_sanitized(run):
    lines = run.stdout.split("\n")
    assert run.returncode == 0 and lines[-2:] == ["ok", ""], run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert "FAILED" not in run.stdout
    # the grid of cases is there: ~40 sizes x 7 batches x 4 paddings x 32 alignments, ten checks each, and the selections
    checks = int(re.search(r"^(\d+) checks$", run.stdout, flags=re.M).group(1))
    assert checks > 300_000, checks


def test_topr_digit_counts(run):
    passes = {int(n): (int(k), int(i)) for n, k, i in re.findall(r"^n (\d+) key_passes (\d+) index_passes (\d+)$", run.stdout, flags=re.M)}
    assert sorted(passes) == [1, 2, 3, 64, 65, 1000, 4097, 8193], run.stdout[-2000:]
    assert passes[1] == (0, 0)                                  # r <= 0 or r >= n: nothing to select
    for n in (2, 3, 64, 65, 1000):
        assert passes[n][1] == 1, (n, passes[n])                # one index digit
    for n in (4097, 8193):
        assert passes[n][1] == 2, (n, passes[n])                # two
    assert all(1 <= k <= 6 for n, (k, _) in passes.items() if n > 1), passes   # 63 key bits in 12-bit digits at most
