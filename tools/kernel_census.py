#!/usr/bin/env python3
"""Which kernel instantiations of libspx.so does a test run launch?

  kernel_census.py symbols LIB              (no GPU) the kernel instantiations of a built library, demangled, one per line
  kernel_census.py launched DIR...          Calls per kernel name, summed over every *kernel_stats.csv (Name, Calls) below
                                            the directories: the files `rocprofv3 --kernel-trace --stats --output-format csv`
                                            writes.  *.calls.csv (the output of this command, redirected) is read the same way
  kernel_census.py diff LIB DIR...          the join of the two: per kernel template instantiations / launched / never
                                            launched, then the never-launched instantiations in full
                                            (--only-in DIR2...: also list what DIR... alone does not launch but DIR2 does)

The join is on one normalised spelling: return type, parameter list, whitespace, `(anonymous namespace)::` and a `[clone ...]`
suffix removed.  It must be sound: a traced name that starts with k_ and matches no symbol, or more than one, ends `diff`
with exit status 2.  Names from elsewhere (at::..., rocBLAS, copy and fill kernels) are ignored.

The symbols are the host launch stubs (`__device_stub__...` in `nm -C`): the library is linked with hidden visibility but
is not stripped."""
import collections
import csv
import glob
import os
import shutil
import subprocess
import sys

STUB = "__device_stub__"


def _cut_params(name):
    """the name up to the '(' of the parameter list: the first one outside every <...>"""
    depth = 0
    for k, c in enumerate(name):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return name[:k], True
    return name, False


def normalise(name):
    """-> (normalised spelling, complete?)  complete is False for a name the profiler cut short inside its template list"""
    name = name.strip()
    k = name.find(" [clone")
    if k >= 0:
        name = name[:k]
    name = name.replace("(anonymous namespace)::", "").replace(STUB, "")
    if name.startswith("void "):
        name = name[5:]
    head, had_params = _cut_params(name)
    complete = had_params or not name.endswith("...")
    return "".join(head.split()), complete


def template_of(norm):
    return norm.split("<", 1)[0]


def _nm():
    for cand in ("nm", "llvm-nm", "/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm"):
        p = shutil.which(cand) if os.sep not in cand else (cand if os.path.exists(cand) else None)
        if p:
            return p
    raise SystemExit("kernel_census: no nm / llvm-nm found")


def symbols(lib):
    """the demangled host stubs of LIB, sorted: one per kernel instantiation"""
    out = subprocess.run([_nm(), "-C", lib], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        k = line.find(STUB)
        if k < 0:
            continue
        parts = line.split(None, 2)   # address, type letter, demangled name
        if len(parts) == 3:
            names.add(parts[2].strip())
    return sorted(names)


def symbol_table(lib):
    """{normalised spelling: demangled symbol}; two symbols with one spelling would make the join ambiguous"""
    table = {}
    for full in symbols(lib):
        norm, _ = normalise(full)
        if norm in table:
            raise SystemExit("kernel_census: two symbols normalise to %s:\n  %s\n  %s" % (norm, table[norm], full))
        table[norm] = full
    return table


def launched(dirs):
    """{traced name: Calls} summed over the *kernel_stats.csv / *.calls.csv files below dirs"""
    calls = collections.Counter()
    files = []
    for d in dirs:
        if os.path.isfile(d):
            files.append(d)
            continue
        for pat in ("*kernel_stats.csv", "*.calls.csv"):
            files += glob.glob(os.path.join(d, "**", pat), recursive=True)
    for f in sorted(set(files)):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if row.get("Name"):
                    calls[row["Name"]] += int(row["Calls"])
    return calls, sorted(set(files))


def join(table, calls):
    """-> ({normalised symbol: calls}, [unmatched k_ names])"""
    per = collections.Counter()
    bad = []
    for name, c in calls.items():
        norm, complete = normalise(name)
        if not norm.startswith("k_"):
            continue
        if complete and norm in table:
            per[norm] += c
            continue
        # a name cut short by the profiler: sound only when it is the prefix of exactly one symbol
        stem = norm[:-3] if norm.endswith("...") else norm
        hits = [s for s in table if s.startswith(stem)] if not complete else []
        if len(hits) == 1:
            per[hits[0]] += c
        else:
            bad.append((name, len(hits)))
    return per, bad


def report(table, per, title, out=sys.stdout):
    tmpl = collections.defaultdict(list)
    for norm in table:
        tmpl[template_of(norm)].append(norm)
    print(title, file=out)
    print("%-28s %14s %9s %15s" % ("kernel template", "instantiations", "launched", "never launched"), file=out)
    tot = [0, 0]
    for t in sorted(tmpl, key=lambda t: (-len(tmpl[t]), t)):
        hit = sum(1 for s in tmpl[t] if per.get(s, 0) > 0)
        tot[0] += len(tmpl[t]); tot[1] += hit
        print("%-28s %14d %9d %15d" % (t, len(tmpl[t]), hit, len(tmpl[t]) - hit), file=out)
    print("%-28s %14d %9d %15d" % ("total", tot[0], tot[1], tot[0] - tot[1]), file=out)
    never = sorted(s for s in table if per.get(s, 0) == 0)
    if never:
        print("never launched:", file=out)
        for s in never:
            print("  " + s, file=out)
    return never


def main(argv):
    if len(argv) >= 2 and argv[0] == "symbols":
        for s in symbols(argv[1]):
            print(s)
        return 0
    if len(argv) >= 2 and argv[0] == "launched":
        calls, files = launched(argv[1:])
        w = csv.writer(sys.stdout)
        w.writerow(["Name", "Calls"])
        for name in sorted(calls):
            w.writerow([name, calls[name]])
        print("kernel_census: %d names from %d files" % (len(calls), len(files)), file=sys.stderr)
        return 0
    if len(argv) >= 3 and argv[0] == "diff":
        args = argv[2:]
        extra = []
        if "--only-in" in args:
            k = args.index("--only-in")
            args, extra = args[:k], args[k + 1:]
        table = symbol_table(argv[1])
        calls, files = launched(args)
        per, bad = join(table, calls)
        never = report(table, per, "%d instantiations in %s; %d trace files" % (len(table), os.path.basename(argv[1]), len(files)))
        if extra:
            per2, bad2 = join(table, launched(extra)[0])
            bad += bad2
            only = [s for s in never if per2.get(s, 0) > 0]
            print("launched only by the second set (%d):" % len(only))
            for s in only:
                print("  " + s)
        if bad:
            for name, hits in bad:
                print("kernel_census: traced kernel matches %d symbols: %s" % (hits, name), file=sys.stderr)
            return 2
        return 0
    print(__doc__, file=sys.stderr)
    return 64


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
