"""CPU: every kernel instantiation of libspx.so is accounted for in tests/kernel_census.json.

The file has one entry per instantiation (tools/kernel_census.py's normalised spelling of the launch stub): either
"test": the test that launches it -- a test file (the census traces one profiler run per test file, so that is what it
measures: profiles/kernel_census.txt) or a full pytest id `file::function[case]` where a case was written to reach it -- or
"unreachable": the `file:line` of the dispatch code that shows no argument combination selects it.

A pull request that adds (or removes) an instantiation fails here until it says which test launches the new one.  The ids are
the measurement's evidence; this test only checks that each names an existing test file and, where given, test function."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_census.py")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as ge
    ge.build()
    import spx_amd
    return spx_amd._lib.LIB_PATH


@pytest.fixture(scope="module")
def census():
    with open(os.path.join(ROOT, "tests", "kernel_census.json")) as f:
        return json.load(f)


def _tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        import kernel_census
    finally:
        sys.path.pop(0)
    return kernel_census


def test_every_instantiation_is_in_the_census(lib_path, census):
    out = subprocess.run([sys.executable, TOOL, "symbols", lib_path], check=True, capture_output=True, text=True).stdout
    names = [l for l in out.splitlines() if l.strip()]
    assert len(names) == len(set(names)) and len(names) >= 600, len(names)
    kc = _tool()
    built = {kc.normalise(n)[0] for n in names}
    assert len(built) == len(names)                      # the normalised spelling keeps the instantiations apart
    listed = set(census)
    missing, stale = sorted(built - listed), sorted(listed - built)
    assert not missing and not stale, (
        "tests/kernel_census.json is out of step with libspx.so: %d instantiations without an entry (say which test launches "
        "each) %s; %d entries for instantiations that no longer exist %s" % (len(missing), missing[:5], len(stale), stale[:5]))


def test_census_entries_name_existing_tests(census):
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and (set(e) == {"test"} or set(e) == {"unreachable"}), (norm, e)
        if "unreachable" in e:
            m = re.fullmatch(r"([\w./]+):(\d+)(?::.*)?", e["unreachable"], flags=re.S)
            assert m, (norm, e)
            path = os.path.join(ROOT, m.group(1))
            assert os.path.isfile(path), (norm, e)
            with open(path) as f:
                assert int(m.group(2)) <= sum(1 for _ in f), (norm, e)
            continue
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)), (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        if rest:
            assert rest.split("[", 1)[0] in funcs[path], (norm, e)


def test_the_join_refuses_a_traced_kernel_it_cannot_match(tmp_path, lib_path):
    """`diff` is sound: a traced k_... name that matches no symbol ends it with a non-zero status; names from elsewhere are
    ignored"""
    d = tmp_path / "trace"
    d.mkdir()
    kc = _tool()
    real = kc.symbols(lib_path)[0].replace("__device_stub__", "")
    (d / "1_kernel_stats.csv").write_text('Name,Calls\n"%s [clone .kd]",3\n"void at::native::fill<double>(double*)",2\n' % real)
    ok = subprocess.run([sys.executable, TOOL, "diff", lib_path, str(d)], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert re.search(r"^total\s+%d\s+1\s+%d$" % (len(kc.symbols(lib_path)), len(kc.symbols(lib_path)) - 1), ok.stdout, re.M), ok.stdout[-400:]
    (d / "2_kernel_stats.csv").write_text('Name,Calls\n"void k_sep_lds<NoSuchOp, 6, false, false>(double*)",1\n')
    bad = subprocess.run([sys.executable, TOOL, "diff", lib_path, str(d)], capture_output=True, text=True)
    assert bad.returncode != 0 and "NoSuchOp" in bad.stderr, (bad.returncode, bad.stderr)
