"""CPU: every kernel instantiation of libspx_gbatch.so (the batched group call, csrc/spx_gbatch.hip) is accounted for in
tests/kernel_census_gbatch.json -- the ledger of tests/test_kernel_census.py for the fourth library, in the same form: one entry
per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches it, a full
pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_gbatch.txt: one profiler run
per test file); this test checks that the ledger and the library agree and that each id names an existing test function.

A pull request that adds (or removes) an instantiation of k_group_batch or k_gbatch_reduce fails here until it says which test
launches the new one.  libspx.so, libspx_batch.so and libspx_ibatch.so must not gain a kernel from the batched group call: their
ledgers are unchanged."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_census.py")
# GroupTilesPlain (csrc/spx_group_common.hpp): lanes per group x elements per lane of the nine rows
TILES = [(1, 2), (2, 4), (4, 4), (16, 2), (16, 4), (16, 8), (32, 8), (64, 6), (64, 8)]


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd._lib.LIB_PATH, spx_amd._lib.BATCH_LIB_PATH, spx_amd._lib.IBATCH_LIB_PATH, spx_amd._lib.GBATCH_LIB_PATH


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_gbatch.json")) as f:
        return json.load(f)


def _normalised(lib):
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        import kernel_census as kc
    finally:
        sys.path.pop(0)
    out = subprocess.run([sys.executable, TOOL, "symbols", lib], check=True, capture_output=True, text=True).stdout
    names = [l for l in out.splitlines() if l.strip()]
    norm = [kc.normalise(n)[0] for n in names]
    assert len(set(norm)) == len(names)                  # the normalised spelling keeps the instantiations apart
    return set(norm)


def test_every_gbatch_instantiation_is_in_the_census(libs, census):
    built = _normalised(libs[3])
    assert built and all(n.startswith(("k_group_batch<", "k_gbatch_reduce")) for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_gbatch.json is out of step with libspx_gbatch.so: %d instantiations without an entry %s; %d entries "
        "for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # the nine tiles x {row, tiled} x {element-wise, pairs} + the per-problem reduce
    want = {"k_group_batch<%d,%d,%s,%s>" % (l, e, t, p) for l, e in TILES for t in ("false", "true") for p in ("false", "true")}
    assert built == want | {"k_gbatch_reduce"}, sorted(built ^ (want | {"k_gbatch_reduce"}))
    assert len(built) == 37, len(built)


def test_the_other_libraries_gained_no_kernel_of_the_new_names(libs):
    for lib in libs[:3]:
        assert not [n for n in _normalised(lib) if "k_group_batch" in n or "k_gbatch" in n], lib
    # the first library holds no batched kernel at all; the second and the third still hold their own 25
    assert not [n for n in _normalised(libs[0]) if "batch" in n]
    assert len(_normalised(libs[1])) == 25 and len(_normalised(libs[2])) == 25


def test_gbatch_census_entries_name_existing_tests(census):
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)) and rest, (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        assert rest.split("[", 1)[0] in funcs[path], (norm, e)
