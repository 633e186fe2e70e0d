"""What the CPU tests of the batched libraries share (a plain module, as arbiter.py and redzone.py are): the libraries by the
keys of _lib.BATCH_LIBRARIES, a header's declarations, a library's kernel names in the census's spelling, and the check that a
census ledger's entries name existing tests."""
import functools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_census.py")
CORE = "core"      # libspx.so's place among the keys of library_paths()


def header(key):
    return os.path.join(ROOT, "include", "spx_%s.h" % key)


def header_declarations(path):
    """{name: argument text} of the `int spx_*(...);` declarations of a header, comments dropped"""
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(spx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


def library_paths():
    """{CORE: libspx.so, key: libspx_<key>.so for every key of the table}, built"""
    import __graft_entry__ as ge
    L = ge.build()._lib
    return dict({CORE: L.LIB_PATH}, **{key: L.batch_lib_path(key) for key in L.BATCH_LIBRARIES})


def others(key):
    """every library of the eight but `key`'s: {key: path}"""
    return {k: p for k, p in library_paths().items() if k != key}


@functools.lru_cache(maxsize=None)
def normalised(lib):
    """the kernel instantiations of a built library, in tools/kernel_census.py's normalised spelling"""
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        import kernel_census as kc
    finally:
        sys.path.pop(0)
    out = subprocess.run([sys.executable, TOOL, "symbols", lib], check=True, capture_output=True, text=True).stdout
    names = [l for l in out.splitlines() if l.strip()]
    norm = [kc.normalise(n)[0] for n in names]
    assert len(set(norm)) == len(names)                  # the normalised spelling keeps the instantiations apart
    return frozenset(norm)


def census_entries_name_existing_tests(census):
    """every entry of a ledger is {"test": "tests/test_X.py::test_function[case]"} of an existing file and function"""
    funcs = {}
    for norm, e in census.items():
        assert isinstance(e, dict) and set(e) == {"test"}, (norm, e)     # none is unreachable
        path, _, rest = e["test"].partition("::")
        assert re.fullmatch(r"tests/test_\w+\.py", path) and os.path.isfile(os.path.join(ROOT, path)) and rest, (norm, e)
        if path not in funcs:
            with open(os.path.join(ROOT, path)) as f:
                funcs[path] = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
        assert rest.split("[", 1)[0] in funcs[path], (norm, e)
