"""CPU: every kernel instantiation of libspx_gbinf_batch.so (the batched Binf group call, csrc/spx_gbinf_batch.hip) is accounted
for in tests/kernel_census_gbinf_batch.json -- the ledger of tests/test_kernel_census_gbatch.py for the fifth library, in the same
form: one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches
it, a full pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_gbinf_batch.txt: one
profiler run per test file); this test checks that the ledger and the library agree and that each id names an existing test
function.

A pull request that adds (or removes) an instantiation of k_binf_batch or k_binf_batch_reduce fails here until it says which test
launches the new one.  libspx.so, libspx_batch.so, libspx_ibatch.so and libspx_gbatch.so must not gain a kernel from the batched
Binf call: their ledgers are unchanged."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_census.py")
# GroupTilesBinf (csrc/spx_group_common.hpp): lanes per group x elements per lane of the nine rows
TILES = [(1, 2), (1, 4), (1, 8), (2, 8), (4, 8), (8, 8), (8, 16), (16, 16), (32, 16)]


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    L = spx_amd._lib
    return L.LIB_PATH, L.BATCH_LIB_PATH, L.IBATCH_LIB_PATH, L.GBATCH_LIB_PATH, L.GBINF_BATCH_LIB_PATH


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_gbinf_batch.json")) as f:
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


def test_every_gbinf_batch_instantiation_is_in_the_census(libs, census):
    built = _normalised(libs[4])
    assert built and all(n.startswith(("k_binf_batch<", "k_binf_batch_reduce")) for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_gbinf_batch.json is out of step with libspx_gbinf_batch.so: %d instantiations without an entry %s; %d "
        "entries for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # the nine tiles x {row, tiled} x {element-wise, pairs} + the per-problem reduce
    want = {"k_binf_batch<%d,%d,%s,%s>" % (l, e, t, p) for l, e in TILES for t in ("false", "true") for p in ("false", "true")}
    assert built == want | {"k_binf_batch_reduce"}, sorted(built ^ (want | {"k_binf_batch_reduce"}))
    assert len(built) == 37, len(built)


def test_the_other_libraries_gained_no_kernel_of_the_new_names(libs):
    for lib in libs[:4]:
        assert not [n for n in _normalised(lib) if "k_binf_batch" in n], lib
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in _normalised(libs[4]) if "k_group_batch" in n or "k_gbatch" in n]
    # the first library holds no batched kernel at all; the others still hold their own
    assert not [n for n in _normalised(libs[0]) if "batch" in n]
    assert [len(_normalised(lib)) for lib in libs[1:4]] == [25, 25, 37]


def test_gbinf_batch_census_entries_name_existing_tests(census):
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)) and rest, (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        assert rest.split("[", 1)[0] in funcs[path], (norm, e)
