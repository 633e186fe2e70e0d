"""CPU: every kernel instantiation of libspx_gbinf_batch.so (the batched Binf group call, csrc/spx_gbinf_batch.hip) is accounted
for in tests/kernel_census_gbinf_batch.json -- the ledger of tests/test_kernel_census_gbatch.py for the fifth library, in the same
form: one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches
it, a full pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_gbinf_batch.txt: one
profiler run per test file); this test checks that the ledger and the library agree and that each id names an existing test
function.

A pull request that adds (or removes) an instantiation of k_binf_batch or k_binf_batch_reduce fails here until it says which test
launches the new one.  No other library may gain a kernel from the batched Binf call: their ledgers are unchanged."""
import json
import os

import pytest

import batch_libs
from batch_libs import normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# GroupTilesBinf (csrc/spx_group_common.hpp): lanes per group x elements per lane of the nine rows
TILES = [(1, 2), (1, 4), (1, 8), (2, 8), (4, 8), (8, 8), (8, 16), (16, 16), (32, 16)]


@pytest.fixture(scope="module")
def libs():
    return batch_libs.library_paths()


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_gbinf_batch.json")) as f:
        return json.load(f)


def test_every_gbinf_batch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["gbinf_batch"])
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
    for key, lib in batch_libs.others("gbinf_batch").items():
        assert not [n for n in normalised(lib) if "k_binf_batch" in n], key
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in normalised(libs["gbinf_batch"]) if "k_group_batch" in n or "k_gbatch" in n]
    # the first library holds no batched kernel at all; the others still hold their own
    assert not [n for n in normalised(libs[batch_libs.CORE]) if "batch" in n]
    assert [len(normalised(libs[key])) for key in ("batch", "ibatch", "gbatch")] == [25, 25, 37]


def test_gbinf_batch_census_entries_name_existing_tests(census):
    batch_libs.census_entries_name_existing_tests(census)
