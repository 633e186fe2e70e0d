#!/usr/bin/env python3
"""Is the device code of two builds the same?  tools/asm_diff.py DIR_A DIR_B

DIR_A and DIR_B hold one .s per csrc/*.hip, compiled with the flags of csrc/build.sh plus `--cuda-device-only -S`.  Comments,
.file / .ident / .loc lines and the position of a function in its file (the number in local labels such as .LBB12_3, which
changes when the host code instantiates the kernels in another order) are dropped; then every function's instructions and
every kernel descriptor (.amdhsa_* lines: registers, LDS, scratch) are compared by symbol.  One summary line per file, then
the symbols that differ; a kernel whose descriptor differs is listed with the keys that moved (`key a -> b`).  Exit status 1
on any difference.  profiles/result_dest_asm_diff.txt and profiles/batch_shared_asm_diff.txt are its output."""
import hashlib
import os
import re
import sys


def parse(path):
    funcs, kds = {}, {}
    cur, body, kcur = None, [], None
    for line in open(path, errors="replace"):
        st = re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", line.split(";")[0]).strip()
        if not st or st.startswith((".loc", ".file", ".ident", ".cfi")):
            continue
        m = re.match(r"^\.amdhsa_kernel\s+(\S+)", st)
        if m:
            kcur = m.group(1)
            kds[kcur] = []
        elif st == ".end_amdhsa_kernel":
            kcur = None
        elif kcur is not None:
            kds[kcur].append(st)
        elif cur is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):$", st)
            if m and not st.startswith(".L") and not st.endswith(".kd:"):
                cur, body = m.group(1), []
        elif st.startswith(".Lfunc_end"):
            funcs[cur] = body
            cur = None
        else:
            body.append(st)
    return funcs, kds


def worst(kds, key):
    return max([int(l.split()[1]) for k in kds.values() for l in k if l.startswith(key)] or [0])


def main(a, b):
    differing = 0
    nf = nk = 0
    for f in sorted(x for x in os.listdir(a) if x.endswith(".s")):
        fa, ka = parse(os.path.join(a, f))
        fb, kb = parse(os.path.join(b, f))
        sets = set(fa) == set(fb) and set(ka) == set(kb)
        df = [n for n in fa if n in fb and fa[n] != fb[n]]
        dk = [n for n in ka if n in kb and ka[n] != kb[n]]
        digest = hashlib.sha256("\n".join(n + "\n" + "\n".join(fa[n]) for n in sorted(fa)).encode()).hexdigest()[:16]
        print("%-18s functions %4d  kernels %4d  lines %7d  max vgpr %3d  max LDS %6d  max scratch %4d  sha256/16 %s  symbols %s  "
              "functions differing %d  descriptors differing %d"
              % (f, len(fa), len(ka), sum(len(v) for v in fa.values()), worst(ka, ".amdhsa_next_free_vgpr"),
                 worst(ka, ".amdhsa_group_segment_fixed_size"), worst(ka, ".amdhsa_private_segment_fixed_size"), digest,
                 "equal" if sets else "DIFFER", len(df), len(dk)))
        for n in sorted(set(fa) ^ set(fb))[:8] + df[:8]:
            print("    differs: " + n)
        for n in dk:
            da, db = (dict(l.split(None, 1) for l in k[n]) for k in (ka, kb))
            print("    descriptor differs: %s  %s" % (n, ", ".join(
                "%s %s -> %s" % (key, da.get(key, "-"), db.get(key, "-")) for key in sorted(set(da) | set(db)) if da.get(key) != db.get(key))))
        differing += (not sets) or bool(df) or bool(dk)
        nf += len(fa)
        nk += len(ka)
    print("total: %d functions, %d kernels; files with any difference: %d" % (nf, nk, differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
