"""CPU: every kernel instantiation of libspx_topr_batch.so (the batched top-r calls, csrc/spx_topr_batch.hip) is accounted for in
tests/kernel_census_topr_batch.json -- the ledger of tests/test_kernel_census_b2_batch.py for the seventh library, in the same
form: one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that
launches it, a full pytest id `file::function[case]`.  This test checks kernel names: that the ledger and the library agree,
and that each id names an existing test function and a size the test file generates.

A pull request that adds (or removes) an instantiation of k_topr_batch fails here until it says which test launches the new
one.  The other seven libraries must not gain a kernel from the batched top-r calls."""
import json
import os
import re

import pytest

import batch_libs
from batch_libs import normalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kToprBatchTiles (csrc/spx_plan.hpp): lanes x elements per lane of the row-resident form; the row walk: kToprBatchWalkLanes x 0
TILES = [(64, 4), (256, 4), (256, 16), (512, 16)]
WALK = (1024, 0)
BOOL = ("false", "true")


@pytest.fixture(scope="module")
def libs():
    return batch_libs.library_paths()


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_topr_batch.json")) as f:
        return json.load(f)


def test_every_topr_batch_instantiation_is_in_the_census(libs, census):
    built = normalised(libs["topr_batch"])
    assert built and all(n.startswith("k_topr_batch<") for n in built), sorted(built)[:5]
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census_topr_batch.json is out of step with libspx_topr_batch.so: %d instantiations without an entry %s; %d "
        "entries for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))
    # the four tiles of the row-resident form and the row walk x {element-wise, pairs} x {plain, BInf}
    want = {"k_topr_batch<%d,%d,true,%s,%s>" % (l, e, p, b) for l, e in TILES for p in BOOL for b in BOOL}
    want |= {"k_topr_batch<%d,%d,false,%s,%s>" % (WALK + (p, b)) for p in BOOL for b in BOOL}
    assert built == want, sorted(built ^ want)
    assert len(built) == 20, len(built)


def test_the_other_libraries_gained_no_kernel_of_the_new_name(libs):
    for key, lib in batch_libs.others("topr_batch").items():
        assert not [n for n in normalised(lib) if "topr" in n], key
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in normalised(libs["topr_batch"]) if "k_b2_batch" in n or "k_binf_batch" in n or "k_group_batch" in n or "k_gbatch" in n]


def test_topr_batch_census_entries_name_existing_tests(census):
    path = "tests/test_gpu_proxstep_topr_batch.py"
    with open(os.path.join(ROOT, path)) as f:
        src = f.read()
    funcs = set(re.findall(r"^def (test_\w+)\(", src, flags=re.M))
    sizes = [int(v) if v.isdigit() else 2 * 8192 + 3 for v in
             re.search(r"^SIZES = \[(.*)\]$", src, flags=re.M).group(1).replace("2 * ROW_MAX + 3", "x").split(", ")]
    caps = [l * e for l, e in TILES]
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        file, _, rest = e["test"].partition("::")
        assert file == path and rest.split("[", 1)[0] in funcs, (norm, e)
        n, form = rest.split("[", 1)[1].rstrip("]").split("-")
        lanes, epl, reg, pairs, binf = norm[len("k_topr_batch<"):-1].split(",")
        assert form == ("binf" if binf == "true" else "plain"), (norm, e)
        # the size named is one the test generates, and one the plan sends to this tile (odd and even ld, aligned and not, are
        # all in that test: both alignment classes run at every size)
        n = int(n)
        assert n in sizes, (norm, n)
        if reg == "true":
            tile = TILES.index((int(lanes), int(epl)))
            assert (caps[tile - 1] if tile else 0) < n <= caps[tile], (norm, n)
        else:
            assert (int(lanes), int(epl)) == WALK and n > caps[-1], (norm, n)
