"""The ledger of the call sites that reserve library-owned scratch (tests/ws_sites.json) against the sources, read as text.

Every spx_ws_reserve(...) call in csrc/*.hip and *.hpp and the staging allocation of the spx_host_* forms is listed by file and
enclosing function, with the number of sites in that function and the case of tests/ws_poison.py that reaches it.  A site that is
missing from the ledger, or a ledger entry whose site is gone, fails here: a new reserving site cannot be added without a case of
tests/test_gpu_ws_poison.py that runs it on filled scratch."""
import glob
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shiftedproximaloperators.jl_amd", "csrc")
LEDGER = os.path.join(ROOT, "tests", "ws_sites.json")

_CALL = re.compile(r"\bspx_ws_reserve\(|\bstage_reserve\(")
_NAME = re.compile(r"\b(\w+)\(")


def ledger():
    with open(LEDGER) as f:
        return json.load(f)["sites"]


def scan(text):
    """[(enclosing function, line number)] of the reserving calls in one source text.  The enclosing function: the name in front
    of the first parenthesis of the nearest line above that starts in column 0 and is neither a closing brace, a preprocessor line
    nor a comment -- the definitions of this code base start there, their bodies are indented."""
    lines = text.split("\n")
    out = []
    for i, line in enumerate(lines):
        code = line.split("//")[0]
        if not _CALL.search(code) or code.lstrip().startswith("#define"):
            continue
        if re.match(r"^(SPX_SHARED |static |inline )*int \(?(spx_ws_reserve|stage_reserve)\)?\(", code):   # the declaration / definition
            continue
        for j in range(i, -1, -1):
            head = lines[j]
            if head and not head[0].isspace() and head[0] not in "}#/" and "(" in head:
                out.append((_NAME.search(head).group(1), i + 1))
                break
        else:
            raise AssertionError("no enclosing function for line %d: %s" % (i + 1, line))
    return out


def sites_in_sources():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        with open(path) as f:
            for fn, _ in scan(f.read()):
                key = (os.path.basename(path), fn)
                found[key] = found.get(key, 0) + 1
    return found


def test_scan_finds_the_enclosing_function():
    text = "\n".join([
        "// spx_ws_reserve(ctx, 1) in a comment",
        "SPX_SHARED int spx_ws_reserve(spx_ctx* ctx, size_t bytes);",
        "#define spx_ws_reserve(ctx, bytes) spx_ws_reserve_at((ctx), (bytes), __FILE__, __func__, __LINE__)",
        "template <class Op>",
        "static int run_thing(const Call<double>& c, Op op,",
        "                     double scale = 1.0) {",
        "  if constexpr (NS > 0) {",
        "    int rc = spx_ws_reserve(ctx, bytes(n));",
        "  }",
        "  rc = spx_ws_reserve(ctx, 256);  // twice",
        "}",
        "int (spx_ws_reserve)(spx_ctx* ctx, size_t bytes) {",
        "  return 0;",
        "}",
        "SPX_EXPORT int spx_entry(spx_ctx* ctx) {",
        "  rc = stage_reserve(ctx, total ? total : kAlign);",
        "}",
    ])
    assert scan(text) == [("run_thing", 8), ("run_thing", 10), ("spx_entry", 16)]


def test_every_reserving_site_is_in_the_ledger_and_every_entry_has_its_site():
    found = sites_in_sources()
    listed = {(e["file"], e["function"]): e["sites"] for e in ledger()}
    assert len(listed) == len(ledger()), "a (file, function) pair is listed twice"
    missing = sorted(k for k in found if k not in listed)
    gone = sorted(k for k in listed if k not in found)
    assert not missing, "reserving sites without a ledger entry (add the entry and a case of tests/ws_poison.py): %r" % (missing,)
    assert not gone, "ledger entries whose site is gone: %r" % (gone,)
    wrong = {k: (found[k], listed[k]) for k in found if found[k] != listed[k]}
    assert not wrong, "sites per function (sources, ledger): %r" % (wrong,)
    assert found[("spx_host.hip", "stage_in")] == 1          # the staging allocation


def test_every_entry_names_a_case_of_the_poison_test():
    import ast
    with open(os.path.join(ROOT, "tests", "ws_poison.py")) as f:
        tree = ast.parse(f.read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "CASES")
    for e in ledger():
        assert e["cases"] and set(e["cases"]) <= set(cases), e
        assert e["sites"] >= 1 and e["what"], e
    assert set(c for e in ledger() for c in e["cases"]) == set(cases), "a case that reaches no site, or none for a site"
