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
    L = spx_amd._lib
    return (L.LHALF_BATCH_LIB_PATH, L.LIB_PATH, L.BATCH_LIB_PATH, L.IBATCH_LIB_PATH, L.GBATCH_LIB_PATH, L.GBINF_BATCH_LIB_PATH,
            L.B2_BATCH_LIB_PATH, L.TOPR_BATCH_LIB_PATH)


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census_lhalf_batch.json")) as f:
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


def test_every_lhalf_batch_instantiation_is_in_the_census(libs, census):
    built = _normalised(libs[0])
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
    for lib in libs[1:]:
        assert not [n for n in _normalised(lib) if "lhalf_batch" in n or "lhalf_threshold" in n or "BatchRowLhalf" in n], lib
    # the new names stay clear of the strings the other ledgers search for
    assert not [n for n in _normalised(libs[0]) if n.startswith(("k_sep_batch", "k_batch_reduce")) or "k_b2_batch" in n
                or "k_binf_batch" in n or "k_group_batch" in n or "k_gbatch" in n or "topr" in n]
    assert not [n for n in _normalised(libs[1]) if "batch" in n]      # the first library holds no batched kernel at all
    assert len(_normalised(libs[2])) == 25                            # libspx_batch.so is what it was


def test_lhalf_batch_census_entries_name_existing_tests(census):
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)) and rest, (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        assert rest.split("[", 1)[0] in funcs[path], (norm, e)
