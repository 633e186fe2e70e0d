"""CPU: every kernel instantiation of libspx_b2_batch.so (the batched ShiftedNormL1B2 call, csrc/spx_b2_batch.hip) is accounted for
in tests/kernel_census_b2_batch.json -- the ledger of tests/test_kernel_census_gbinf_batch.py for the sixth library, in the same
form: one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches
it, a full pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_b2_batch.txt: one
profiler run of the test file); this test checks that the ledger and the library agree and that each id names an existing test
function.

A pull request that adds (or removes) an instantiation of k_b2_batch fails here until it says which test launches the new one.
No other library may gain a kernel from the batched ShiftedNormL1B2 call: their counts are unchanged."""
import json
import os

import pytest

import batch_libs
from batch_libs import normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kB2BatchTiles (csrc/spx_plan.hpp): lanes x elements per lane of the row-resident form; the row walk: kB2BatchWalkLanes x 0
TILES = [(64, 4), (256, 4), (256, 16), (512, 16)]
WALK = (1024, 0)


@pytest.fixture(scope="module")
def libs():
    return batch_libs.library_paths()


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_b2_batch.json")) as f:
        return json.load(f)


def test_every_b2_batch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["b2_batch"])
    assert built and all(n.startswith("k_b2_batch<") for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_b2_batch.json is out of step with libspx_b2_batch.so: %d instantiations without an entry %s; %d "
        "entries for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # the four tiles of the row-resident form and the row walk x {element-wise, pairs}
    want = {"k_b2_batch<%d,%d,true,%s>" % (l, e, p) for l, e in TILES for p in ("false", "true")}
    want |= {"k_b2_batch<%d,%d,false,%s>" % (WALK + (p,)) for p in ("false", "true")}
    assert built == want, sorted(built ^ want)
    assert len(built) == 10, len(built)


def test_the_other_libraries_gained_no_kernel_of_the_new_names(libs):
    for key, lib in batch_libs.others("b2_batch").items():
        assert not [n for n in normalised(lib) if "k_b2_batch" in n], key
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in normalised(libs["b2_batch"]) if "k_binf_batch" in n or "k_group_batch" in n or "k_gbatch" in n]
    # the first library holds no batched kernel at all; the others still hold their own
    assert not [n for n in normalised(libs[batch_libs.CORE]) if "batch" in n]
    assert [len(normalised(libs[key])) for key in ("batch", "ibatch", "gbatch", "gbinf_batch")] == [25, 25, 37, 37]


def test_b2_batch_census_entries_name_existing_tests(census):
    batch_libs.census_entries_name_existing_tests(census)
    for norm, e in census.items():
        path, _, rest = e["test"].partition("::")
        # the case named is one the test file generates: n among its SIZES
        case = int(rest.split("[", 1)[1].rstrip("]"))
        with open(os.path.join(ROOT, path)) as f:
            assert "SIZES" in f.read() and case in _sizes(), (norm, case)


def _sizes():
    caps = [l * e for l, e in TILES]
    return sorted({1, 2, 3, 7, 63, 64, 65} | {c + d for c in caps for d in (-1, 0, 1)} | {caps[-1] + 2, 2 * caps[-1] + 3})
