"""The CPU oracle under AddressSanitizer + UBSan (CPU build only; GPU sanitizers are not available on this pool):
the golden-vector suite is re-run in a child process against oracle/_asan/libspx_oracle_asan.so."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_golden_suite_under_asan_ubsan():
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    libasan = subprocess.run([gcc, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "asan"])
    env = dict(os.environ)
    preload = " ".join(p for p in (libasan, env.get("LD_PRELOAD", "")) if p)  # the runtime first; keep what was preloaded already
    env.update(SPX_ORACLE_SO=os.path.join(ROOT, "oracle", "_asan", "libspx_oracle_asan.so"), LD_PRELOAD=preload,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_oracle_golden.py"), "-q", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "passed" in r.stdout and "runtime error" not in (r.stdout + r.stderr)
