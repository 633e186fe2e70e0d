"""CPU: every kernel instantiation of libspx_b2_batch.so (the batched ShiftedNormL1B2 call, csrc/spx_b2_batch.hip) is accounted for
in tests/kernel_census_b2_batch.json -- the ledger of tests/test_kernel_census_gbinf_batch.py for the sixth library, in the same
form: one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub) naming the test that launches
it, a full pytest id `file::function[case]`.  The ids are the measurement's evidence (profiles/kernel_census_b2_batch.txt: one
profiler run of the test file); this test checks that the ledger and the library agree and that each id names an existing test
function.

A pull request that adds (or removes) an instantiation of k_b2_batch fails here until it says which test launches the new one.
libspx.so, libspx_batch.so, libspx_ibatch.so, libspx_gbatch.so and libspx_gbinf_batch.so must not gain a kernel from the batched
ShiftedNormL1B2 call: their counts are unchanged."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_census.py")
# kB2BatchTiles (csrc/spx_plan.hpp): lanes x elements per lane of the row-resident form; the row walk: kB2BatchWalkLanes x 0
TILES = [(64, 4), (256, 4), (256, 16), (512, 16)]
WALK = (1024, 0)


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    L = spx_amd._lib
    return L.LIB_PATH, L.BATCH_LIB_PATH, L.IBATCH_LIB_PATH, L.GBATCH_LIB_PATH, L.GBINF_BATCH_LIB_PATH, L.B2_BATCH_LIB_PATH


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_b2_batch.json")) as f:
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


def test_every_b2_batch_instantiation_is_in_the_census(libs, census):
    built = _normalised(libs[5])
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
    for lib in libs[:5]:
        assert not [n for n in _normalised(lib) if "k_b2_batch" in n], lib
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in _normalised(libs[5]) if "k_binf_batch" in n or "k_group_batch" in n or "k_gbatch" in n]
    # the first library holds no batched kernel at all; the others still hold their own
    assert not [n for n in _normalised(libs[0]) if "batch" in n]
    assert [len(_normalised(lib)) for lib in libs[1:5]] == [25, 25, 37, 37]


def test_b2_batch_census_entries_name_existing_tests(census):
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)) and rest, (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        assert rest.split("[", 1)[0] in funcs[path], (norm, e)
        # the case named is one the test file generates: n among its SIZES
        case = int(rest.split("[", 1)[1].rstrip("]"))
        with open(os.path.join(ROOT, path)) as f:
            assert "SIZES" in f.read() and case in _sizes(), (norm, case)


def _sizes():
    caps = [l * e for l, e in TILES]
    return sorted({1, 2, 3, 7, 63, 64, 65} | {c + d for c in caps for d in (-1, 0, 1)} | {caps[-1] + 2, 2 * caps[-1] + 3})
