"""CPU: every kernel instantiation of libspx_lhalf_batch.so (the batched RootNormLhalf(Box) calls, csrc/spx_lhalf_batch.hip) is
accounted for in tests/kernel_census_lhalf_batch.json -- the ledger of tests/test_kernel_census_batch.py for the eighth library, in
the same form: one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that
launches it, a full pytest id `file::function[case]`.  The ids are the measurement's evidence
(profiles/kernel_census_lhalf_batch.txt: one profiler run per new test file); this test checks that the ledger and the library
agree and that each id names an existing test function.

A pull request that adds (or removes) an instantiation of k_lhalf_batch fails here until it says which test launches the new one.
The other libraries must not gain a kernel from these calls."""
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
    with open(os.path.join(ROOT, "tests", "kernel_census_lhalf_batch.json")) as f:
        return json.load(f)


def test_every_lhalf_batch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["lhalf_batch"])
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_lhalf_batch.json is out of step with libspx_lhalf_batch.so: %d instantiations without an entry %s; %d "
        "entries for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # {row, tiled} x {Lhalf, LhalfBox, LhalfBox + mask} x {pairs, element-wise}, the per-problem reduce and the threshold kernel
    want = {"k_lhalf_batch<%s,%s,%s,%s>" % (row, t, p, m) for row, masks in (("BatchRowLhalf", ("false",)), ("BatchRowLhalfBox", ("false", "true")))
            for t in ("false", "true") for p in ("false", "true") for m in masks}
    want |= {"k_lhalf_batch_reduce", "k_lhalf_threshold_batch"}
    assert built == want, sorted(built ^ want)
    assert len(built) == 14


def test_the_other_libraries_gained_no_kernel_of_the_new_names(libs):
    for key, lib in batch_libs.others("lhalf_batch").items():
        assert not [n for n in normalised(lib) if "lhalf_batch" in n or "lhalf_threshold" in n or "BatchRowLhalf" in n], key
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in normalised(libs["lhalf_batch"]) if n.startswith(("k_sep_batch", "k_batch_reduce")) or "k_b2_batch" in n
                or "k_binf_batch" in n or "k_group_batch" in n or "k_gbatch" in n or "topr" in n]
    assert not [n for n in normalised(libs[batch_libs.CORE]) if "batch" in n]   # the first library holds no batched kernel at all
    assert len(normalised(libs["batch"])) == 25                                 # libspx_batch.so is what it was


def test_lhalf_batch_census_entries_name_existing_tests(census):
    batch_libs.census_entries_name_existing_tests(census)
