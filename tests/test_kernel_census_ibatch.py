"""CPU: every kernel instantiation of libspx_ibatch.so (the batched iprox! call, csrc/spx_ibatch.hip) is accounted for in
tests/kernel_census_ibatch.json -- the ledger of tests/test_kernel_census.py for the third library, in the same form: one entry
per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches it, a full
pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_ibatch.txt: one profiler run
per test file); this test checks that the ledger and the library agree and that each id names an existing test function.

A pull request that adds (or removes) an instantiation of k_isep_batch or k_ibatch_reduce fails here until it says which test
launches the new one.  libspx.so and libspx_batch.so must not gain a kernel from the batched iprox! call: their ledgers are
unchanged."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_census.py")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd._lib.LIB_PATH, spx_amd._lib.BATCH_LIB_PATH, spx_amd._lib.IBATCH_LIB_PATH


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_ibatch.json")) as f:
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


def test_every_ibatch_instantiation_is_in_the_census(libs, census):
    built = _normalised(libs[2])
    assert built and all(n.startswith(("k_isep_batch<", "k_ibatch_reduce")) for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_ibatch.json is out of step with libspx_ibatch.so: %d instantiations without an entry %s; %d entries "
        "for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # {row, tiled} x {L1, L0, L1Box, L1Box + mask, L0Box, L0Box + mask} x {pairs, element-wise} + the per-problem reduce
    assert len(built) == 25, len(built)


def test_the_other_libraries_gained_no_kernel_of_the_new_names(libs):
    for lib in libs[:2]:
        assert not [n for n in _normalised(lib) if "k_isep_batch" in n or "k_ibatch" in n], lib
    # and the second library still holds its own 25
    assert len(_normalised(libs[1])) == 25


def test_ibatch_census_entries_name_existing_tests(census):
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)) and rest, (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        assert rest.split("[", 1)[0] in funcs[path], (norm, e)
