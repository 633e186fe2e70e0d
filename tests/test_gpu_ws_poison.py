"""A call's results do not depend on what the library's scratch held on entry.

spx_ctx::ws (spx_ws_reserve, about twenty call sites) and the staging block of the spx_host_* forms are bare hipMalloc blocks,
freed and allocated anew when they grow.  Fresh device memory arrives zeroed and a zero is exactly the value that makes a
forgotten zero-fill harmless (a partial-sum slot no workgroup wrote, a count word atomicAdd adds onto, a flag that is polled), so
the rest of the suite cannot see such a mistake.  Here the hooks build (libspx_hooks.so and its batched siblings,
-DSPX_TEST_HOOKS) fills both blocks before every call -- tuning key 103: 1 zero bytes, 2 the 32-bit word 0x00000001 (a count,
flag or index off by one and in range; a subnormal double), 3 0xFF bytes (NaN, a non-zero mask byte, -1) -- and names every
reserving site it passes (key 104).

One child process per family (tests/ws_poison.py, the pattern of tests/test_gpu_robustness.py).  Each call of a case runs three
times on one context, all of pattern 1 first, then 2, then 3 -- a stale integer shows as a wrong result under pattern 2 before
pattern 3 could turn it into an index of -1 -- and the child stops at the first mismatch:
  (a) pattern 1: the bar of the entry point's neighbouring test against the CPU oracle (NormL1 / NormL0 / top-r bit for bit,
      the arbiter at 1e-12 for RootNormLhalf, the group operators and B2, sums within 1e-12 of the sum of |term| of math.fsum, the
      NormL0 count exactly);
  (b) patterns 2 and 3: every output has the bits of pattern 1;
  (c) every return code is 0, spx_sync included.
Then the growth step on a fresh context per pattern: the smallest call, the largest, the smallest again.

Every form that reserves scratch adds its sums in a fixed order (include/spx.h), so none is held to (a) in place of (b) -- but in
the growth step ShiftedNormL1B2, whose speculative pass follows the regime of the context's previous call, is held to (a).

The batched libraries that promise to reserve nothing (ShiftedNormL1B2, top-r) have a test of their own: the same three patterns
on a workspace another call has grown, and no site named.

The last test holds the union of the traced sites to the ledger tests/ws_sites.json: a site no case reached is a failure."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "lib", "libspx_hooks.so")
CASES = ("separable", "topr", "group", "b2", "host", "batch", "ibatch", "gbatch", "gbinf_batch", "lhalf_batch")
_RESULTS = {}
_OUTPUT = {}


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _child(case):
    """the case in a child process on the hooks build: (result line, set of traced (file, function, line), tail of the output)"""
    if case not in _RESULTS:
        env = dict(os.environ, SPX_LIB_NAME="libspx_hooks.so", SPX_NO_BUILD="1")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ws_poison.py"), case], env=env, capture_output=True,
                             text=True, timeout=600, cwd=ROOT)
        lines = out.stdout.splitlines()
        _OUTPUT[case] = lines
        result = [ln for ln in lines if ln.startswith("RESULT")]
        traced = set()
        for ln in lines:
            if ln.startswith("SPX_WS_SITE "):
                _, f, fn, line, _bytes = ln.split()
                traced.add((f, fn, int(line)))
        tail = "\n".join([ln for ln in lines if not ln.startswith("SPX_WS_SITE ")][-40:]) + "\n" + out.stderr[-3000:]
        _RESULTS[case] = (result[-1] if result else "", traced, tail)
    return _RESULTS[case]


@pytest.mark.parametrize("case", CASES)
def test_results_do_not_depend_on_the_scratch(s, case):
    if not os.path.exists(LIB):
        pytest.skip("libspx_hooks.so not built")
    result, traced, tail = _child(case)
    assert result.startswith("RESULT ok"), (case, result, tail)
    assert int(result.split()[2]) > 0 and traced, (case, result)


def test_row_batched_calls_reserve_nothing_and_do_not_read_the_scratch(s):
    """spx_proxstep_l1_b2_batch and spx_proxstep_indball_l0[_binf]_batch promise "workspace: NONE" (include/spx_b2_batch.h,
    include/spx_topr_batch.h).  The case `row_batch` of tests/ws_poison.py, in a child on the hooks build: a tiled
    spx_proxstep_l1_batch call grows the context's workspace and names its site (key 104 is live); then the three calls at
    n = 1000 and n = 8200 (the row in registers, the row walk), rows = 3, ld = n and n + 1, under patterns 1, 2, 3 of key 103 on
    that block: pattern 1 meets the oracle at the batched files' bars, patterns 2 and 3 have its bits, every return code is 0
    -- and between the child's two markers NO site is named."""
    if not os.path.exists(LIB):
        pytest.skip("libspx_hooks.so not built")
    result, traced, tail = _child("row_batch")
    assert result.startswith("RESULT ok"), (result, tail)
    assert int(result.split()[2]) == 3 * 12, result                    # three patterns of 2 sizes x 2 row strides x 3 calls
    lines = _OUTPUT["row_batch"]
    assert lines.count("NO_WS_BEGIN") == 1 and lines.count("NO_WS_END") == 1, tail
    a, b = lines.index("NO_WS_BEGIN"), lines.index("NO_WS_END")
    before = [ln for ln in lines[:a] if ln.startswith("SPX_WS_SITE ")]
    assert before and all(ln.split()[1:3] == ["spx_batch_device.hpp", "run_batch"] for ln in before), before
    assert int(before[-1].split()[4]) > 0                              # there is a block to fill
    inside = [ln for ln in lines[a:b] if ln.startswith("SPX_WS_SITE ")]
    assert inside == [], inside
    assert not [ln for ln in lines[b:] if ln.startswith("SPX_WS_SITE ")]


def test_every_ledger_site_was_traced(s):
    """key 104: the union of the traced sites over all cases equals the ledger, function by function and site by site"""
    if not os.path.exists(LIB):
        pytest.skip("libspx_hooks.so not built")
    with open(os.path.join(ROOT, "tests", "ws_sites.json")) as f:
        ledger = json.load(f)["sites"]
    by_case = {case: _child(case)[1] for case in CASES}
    union = set().union(*by_case.values())
    seen = {}
    for f, fn, line in union:
        seen.setdefault((f, fn), set()).add(line)
    listed = {(e["file"], e["function"]): e for e in ledger}
    assert sorted(k for k in seen if k not in listed) == [], "traced sites the ledger does not list"
    for key, e in listed.items():
        assert len(seen.get(key, ())) == e["sites"], "%s %s: %d of %d sites traced (lines %r)" % (
            key[0], key[1], len(seen.get(key, ())), e["sites"], sorted(seen.get(key, ())))
        for case in e["cases"]:
            assert any((f, fn) == key for f, fn, _ in by_case[case]), "%s %s: not reached by the case %r the ledger names" % (key[0], key[1], case)
