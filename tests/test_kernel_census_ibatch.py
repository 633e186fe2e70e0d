"""CPU: every kernel instantiation of libspx_ibatch.so (the batched iprox! call, csrc/spx_ibatch.hip) is accounted for in
tests/kernel_census_ibatch.json -- the ledger of tests/test_kernel_census.py for the third library, in the same form: one entry
per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches it, a full
pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_ibatch.txt: one profiler run
per test file); this test checks that the ledger and the library agree and that each id names an existing test function.

A pull request that adds (or removes) an instantiation of k_isep_batch or k_ibatch_reduce fails here until it says which test
launches the new one.  No other library may gain a kernel from the batched iprox! call: their ledgers are unchanged."""
import json
import os

import pytest

import batch_libs
from batch_libs import normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    return batch_libs.library_paths()


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_ibatch.json")) as f:
        return json.load(f)


def test_every_ibatch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["ibatch"])
    assert built and all(n.startswith(("k_isep_batch<", "k_ibatch_reduce")) for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_ibatch.json is out of step with libspx_ibatch.so: %d instantiations without an entry %s; %d entries "
        "for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # {row, tiled} x {L1, L0, L1Box, L1Box + mask, L0Box, L0Box + mask} x {pairs, element-wise} + the per-problem reduce
    assert len(built) == 25, len(built)


def test_the_other_libraries_gained_no_kernel_of_the_new_names(libs):
    for key, lib in batch_libs.others("ibatch").items():
        assert not [n for n in normalised(lib) if "k_isep_batch" in n or "k_ibatch" in n], key
    # and the second library still holds its own 25
    assert len(normalised(libs["batch"])) == 25


def test_ibatch_census_entries_name_existing_tests(census):
    batch_libs.census_entries_name_existing_tests(census)
