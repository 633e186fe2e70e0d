"""CPU: the eight libraries as one set.  _lib.BATCH_LIBRARIES is the table of the seven batched ones (file-name suffix ->
ctypes table); csrc/build.sh's BATCH_LIBS array, the headers include/spx_*batch.h, the sources csrc/spx_*batch.hip and the Julia
shim must name the same seven, and for each of them the header, the exported names, the dynamic section, the loader, the build
and the kernel ledger must agree with its row: every entry point and every kernel lives in exactly one library of the eight and
has a table or ledger entry.  What is specific to one call (its argument list, its contract's words, its mirror) is in that
call's own test file; a ninth library fails here until its row, its array entry, its header, its source and its ledger agree."""
import ctypes
import glob
import json
import os
import re
import shutil
import subprocess

import pytest

import batch_libs
import spx_amd

ROOT = batch_libs.ROOT
CSRC = os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc")
TABLE = spx_amd._lib.BATCH_LIBRARIES
KEYS = list(TABLE)
EIGHT = [batch_libs.CORE] + KEYS


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def libs(built):
    return batch_libs.library_paths()


@pytest.fixture(scope="module")
def exported(libs):
    """{key: the spx_* names the library defines}: nm -D, or without binutils what ctypes finds of every table's names and twins"""
    known = set(spx_amd._lib.SIGNATURES).union(*TABLE.values())
    known |= {"spx_host_" + n[4:] for n in known}
    out = {}
    for key, path in libs.items():
        if shutil.which("nm"):
            txt = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
            out[key] = {l.split()[-1] for l in txt.splitlines() if " T " in l and l.split()[-1].startswith("spx_")}
        else:
            lib = ctypes.CDLL(path)
            out[key] = {n for n in known if hasattr(lib, n)}
    return out


def _stems(pattern):
    return sorted(os.path.splitext(os.path.basename(p))[0][len("spx_"):] for p in glob.glob(os.path.join(ROOT, pattern)))


def test_table_is_the_build_array():
    with open(os.path.join(CSRC, "build.sh")) as f:
        (line,) = re.findall(r"^BATCH_LIBS=\((.*)\)$", f.read(), flags=re.M)
    assert line.split() == KEYS


def test_table_is_the_headers_the_sources_and_the_shim():
    assert len(KEYS) == len(set(KEYS)) and all(re.fullmatch(r"[a-z0-9_]*batch", k) for k in KEYS), KEYS
    assert _stems("include/spx_*batch.h") == sorted(KEYS)
    assert _stems("shiftedproximaloperators.jl_amd/csrc/spx_*batch.hip") == sorted(KEYS)
    with open(os.path.join(ROOT, "julia", "SPXShim.jl")) as f:
        shim = f.read()
    assert [k for k in KEYS if '"libspx_%s.so"' % k not in shim] == []


def test_no_table_and_no_header_has_a_host_twin():
    tables = [spx_amd._lib.SIGNATURES] + list(TABLE.values()) + [batch_libs.header_declarations(batch_libs.header(k)) for k in KEYS]
    for table in tables:
        assert not [k for k in table if k.startswith("spx_host_") and k.endswith("_batch")]


@pytest.mark.parametrize("key", KEYS)
def test_header_compiles_alone_includes_spx_h_and_declares_the_table(key):
    header = batch_libs.header(key)
    if shutil.which("gcc"):
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", header])
    if shutil.which("g++"):
        subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", header])
    with open(header) as f:
        assert '#include "spx.h"' in f.read()
    assert sorted(batch_libs.header_declarations(header)) == sorted(TABLE[key])      # the table binds exactly the declared set


@pytest.mark.parametrize("key", KEYS)
def test_library_exports_its_table_and_no_other_library_does(exported, key):
    names = set(TABLE[key])
    assert names and all(n.endswith("_batch") for n in names), names
    assert {n for n in exported[key] if n.endswith("_batch")} == names     # nothing else of that form is exported ...
    assert exported[key] == names, exported[key] ^ names                   # ... and nothing else at all
    for other in EIGHT:
        if other != key:
            assert not exported[other] & names, (other, exported[other] & names)     # ... here and nowhere else
    assert not [n for n in exported[batch_libs.CORE] if n.endswith("_batch")]
    for lib in EIGHT:
        assert not [n for n in exported[lib] if n.startswith("spx_host_") and n.endswith("_batch")], lib     # no host-pointer twin


@pytest.mark.parametrize("key", KEYS)
def test_library_links_against_libspx_by_rpath_origin(libs, key):
    if not shutil.which("readelf"):
        pytest.skip("no readelf")
    dyn = subprocess.run(["readelf", "-d", libs[key]], check=True, capture_output=True, text=True).stdout
    assert re.search(r"NEEDED.*\[%s\]" % re.escape(os.path.basename(libs[batch_libs.CORE])), dyn), dyn
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn


@pytest.mark.parametrize("key", KEYS)
def test_loader_binds_the_table(built, key):
    L = built._lib
    # named after libspx.so and found next to it; the per-library names are the table's
    assert L.batch_lib_path(key) == L.LIB_PATH[:-3] + "_%s.so" % key == getattr(L, key.upper() + "_LIB_PATH")
    if os.path.basename(L.LIB_PATH) == "libspx.so":
        assert os.path.basename(L.batch_lib_path(key)) == "libspx_%s.so" % key
    assert getattr(L, key.upper() + "_SIGNATURES") is TABLE[key]
    lib = L.load_batch_library(key)
    assert getattr(L, "load_" + key)() is lib and L.load_batch_library(key) is lib     # one handle per key
    for name, args in TABLE[key].items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int, name
    assert L.load().spx_abi_version() == 1                       # the batched libraries are additive
    with pytest.raises(KeyError):
        L.load_batch_library("no_such_batch")


@pytest.mark.parametrize("key", KEYS)
def test_build_leaves_the_library_no_older_than_its_sources(libs, key):
    assert os.path.isfile(libs[key])
    for src in (os.path.join(CSRC, "spx_%s.hip" % key), batch_libs.header(key), os.path.join(CSRC, "build.sh")):
        assert os.path.getmtime(libs[key]) >= os.path.getmtime(src), src


@pytest.mark.parametrize("key", KEYS)
def test_library_kernels_are_its_ledger(libs, key):
    with open(os.path.join(ROOT, "tests", "kernel_census_%s.json" % key)) as f:
        census = json.load(f)
    assert set(census) == batch_libs.normalised(libs[key])
    batch_libs.census_entries_name_existing_tests(census)


def test_no_kernel_lives_in_two_libraries(libs):
    kernels = {key: batch_libs.normalised(libs[key]) for key in EIGHT}
    assert all(kernels.values())
    for k, a in enumerate(EIGHT):
        for b in EIGHT[k + 1:]:
            assert not kernels[a] & kernels[b], (a, b, sorted(kernels[a] & kernels[b])[:5])


@pytest.mark.parametrize("key", KEYS)
def test_a_newer_header_makes_every_library_stale(tmp_path, key):
    """build()'s predicate on a copy of the tree: sources copied with their times, stand-ins for the libraries newer than all"""
    import __graft_entry__ as ge
    root = str(tmp_path)
    pkg = os.path.join(root, "shiftedproximaloperators.jl_amd")
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(root, "include"))
    shutil.copytree(CSRC, os.path.join(pkg, "csrc"))
    os.makedirs(os.path.join(pkg, "lib"))
    srcs, libs = ge._build_files(root)
    newest = max(os.path.getmtime(s) for s in srcs)
    for lib in libs:
        with open(lib, "w"):
            pass
        os.utime(lib, (newest, newest))
    assert [os.path.basename(b) for b in libs] == [os.path.basename(p) for p in batch_libs.library_paths().values()]
    assert ge._stale_libraries(root) == []
    header = os.path.join(root, "include", "spx_%s.h" % key)
    assert header in srcs
    os.utime(header, (newest + 10, newest + 10))
    assert ge._stale_libraries(root) == libs       # everything is rebuilt, as build() does
    os.remove(libs[-1])
    os.utime(header, (newest, newest))
    assert ge._stale_libraries(root) == libs[-1:]  # and a missing library is a stale one
