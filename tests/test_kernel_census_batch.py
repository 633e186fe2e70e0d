"""CPU: every kernel instantiation of libspx_batch.so (the batched separable call, csrc/spx_batch.hip) is accounted for in
tests/kernel_census_batch.json -- the ledger of tests/test_kernel_census.py for the second library, in the same form: one entry
per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches it, a full
pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census.txt: one profiler run per test
file); this test checks that the ledger and the library agree and that each id names an existing test function.

A pull request that adds (or removes) an instantiation of k_sep_batch or k_batch_reduce fails here until it says which test
launches the new one.  No other library may gain a kernel from the batched call, and libspx.so holds no batched kernel at all:
its ledger is unchanged."""
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
    with open(os.path.join(ROOT, "tests", "kernel_census_batch.json")) as f:
        return json.load(f)


def test_every_batch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["batch"])
    # {row, tiled} x {L1, L0, L1Box, L1Box + mask, L0Box, L0Box + mask} x {pairs, element-wise} + the per-problem reduce
    assert len(built) == 25 and all(n.startswith(("k_sep_batch<", "k_batch_reduce")) for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_batch.json is out of step with libspx_batch.so: %d instantiations without an entry %s; %d entries "
        "for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # the batched kernels live in this library only, and libspx.so holds no batched kernel at all
    for key, lib in batch_libs.others("batch").items():
        assert not [n for n in normalised(lib) if n.startswith(("k_sep_batch<", "k_batch_reduce"))], key
    assert not [n for n in normalised(libs[batch_libs.CORE]) if "batch" in n]


def test_batch_census_entries_name_existing_tests(census):
    batch_libs.census_entries_name_existing_tests(census)
