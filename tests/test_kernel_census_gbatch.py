"""CPU: every kernel instantiation of libspx_gbatch.so (the batched group call, csrc/spx_gbatch.hip) is accounted for in
tests/kernel_census_gbatch.json -- the ledger of tests/test_kernel_census.py for the fourth library, in the same form: one entry
per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches it, a full
pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_gbatch.txt: one profiler run
per test file); this test checks that the ledger and the library agree and that each id names an existing test function.

A pull request that adds (or removes) an instantiation of k_group_batch or k_gbatch_reduce fails here until it says which test
launches the new one.  No other library may gain a kernel from the batched group call: their ledgers are unchanged."""
import json
import os

import pytest

import batch_libs
from batch_libs import normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# GroupTilesPlain (csrc/spx_group_common.hpp): lanes per group x elements per lane of the nine rows
TILES = [(1, 2), (2, 4), (4, 4), (16, 2), (16, 4), (16, 8), (32, 8), (64, 6), (64, 8)]


@pytest.fixture(scope="module")
def libs():
    return batch_libs.library_paths()


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_gbatch.json")) as f:
        return json.load(f)


def test_every_gbatch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["gbatch"])
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
    for key, lib in batch_libs.others("gbatch").items():
        assert not [n for n in normalised(lib) if "k_group_batch" in n or "k_gbatch" in n], key
    # the first library holds no batched kernel at all; the second and the third still hold their own 25
    assert not [n for n in normalised(libs[batch_libs.CORE]) if "batch" in n]
    assert len(normalised(libs["batch"])) == 25 and len(normalised(libs["ibatch"])) == 25


def test_gbatch_census_entries_name_existing_tests(census):
    batch_libs.census_entries_name_existing_tests(census)
