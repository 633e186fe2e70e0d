"""Inputs, exact references and bars for the Float32 psi(y) entry points and spx_prox_group_l2_f32.

Plain helper module (like tests/arbiter.py and tests/nonfinite.py): numpy, fractions and the CPU oracle only, no torch, no GPU.
tests/test_oracle_f32_forms.py checks it against the oracle alone (the wrong-answer inequality, the ambiguity census);
tests/test_gpu_f32_exact.py runs the same inputs through the C ABI.

The arithmetic under test is the one include/spx.h states: every element operation in Float32, `1.1 * Delta` and its
comparison in Float64, squares of group elements as exact Float64 products, every sum in Float64, the group norm rounded to
Float32 once.  So
  * psi(y) is a sum of terms that the oracle states exactly: the bar is nonfinite.check_sum at 1e-12 of sum |term|, times
    (double)lambda; counts and the 0 / +Inf decisions are exact;
  * the group prox is determined to the bit -- except in a group whose EXACT norm lies within AMBIGUOUS_REL = 1e-12 (the
    project's bar for the device's own Float64 sum of non-negative terms) of the midpoint of two adjacent Float32 values: such
    a group must equal, bit for bit, the restatement evaluated with one of the two neighbours.  `census` finds those groups
    from the exact sum of the exact squares (rational arithmetic), and gives every other group its correctly rounded norm.
"""
import zlib
from fractions import Fraction

import numpy as np

import nonfinite

F32 = np.float32
EPS32 = F32(np.finfo(np.float32).eps)
SLACK32 = np.sqrt(EPS32)                      # sqrt(eps(Float32)) formed in Float32
assert SLACK32.dtype == np.float32
AMBIGUOUS_REL = Fraction(1, 10 ** 12)
LAM = F32(1.2)
INF32 = F32(np.inf)


def rng_of(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def up(v):
    return np.nextafter(F32(v), INF32)


def down(v):
    return np.nextafter(F32(v), -INF32)


def binf_edge(start=1.5):
    """(Delta, t_in, t_out), all Float32: t_in is the largest Float32 <= 1.1 * (double)Delta (feasible), t_out the next one up --
    outside the ball, yet <= 1.1f * Delta formed in Float32: a kernel that forms the radius in Float32 calls it feasible."""
    d = F32(start)
    for _ in range(100000):
        rad = 1.1 * float(d)
        t_in = F32(rad)
        if float(t_in) > rad:
            t_in = down(t_in)
        t_out = up(t_in)
        if float(t_out) > rad and t_out <= F32(F32(1.1) * d):
            return d, t_in, t_out
        d = up(d)
    raise AssertionError("no Delta found")


DELTA, T_IN, T_OUT = binf_edge()
L_EDGE, U_EDGE = F32(-1.5), F32(1.5)
T_LOW = F32(L_EDGE - SLACK32)                 # sj + y exactly at l - sqrt(eps32): feasible; down(T_LOW): +Inf
T_HIGH = F32(U_EDGE + SLACK32)


# ====================================================================================================== separable psi(y)
SEP_ENTRIES = ("l1", "l0", "lhalf", "l1_box", "l0_box", "lhalf_box", "indball_l0", "indball_l0_binf")
SEP_SIZES = (1, 2, 63, 64, 65, 255, 257, 2047, 2049, 300_001, 4_196_353)   # the last: past the 2048-workgroup cap of run_obj
OBJ_BLOCK = 256 * 8
OBJ_BLOCKS_CAP = 2048


def family_of(entry):
    return "box" if entry.endswith("_box") else "binf" if entry.endswith("_binf") else "plain"


def kind_of(entry):
    return "l0" if entry.startswith("indball") else entry.split("_")[0]


def last_trip_index(n):
    """an index in the last, partial trip of k_obj's grid-stride loop (n - 1 where there is one trip only)"""
    blocks = min((n + OBJ_BLOCK - 1) // OBJ_BLOCK, OBJ_BLOCKS_CAP)
    stride = blocks * 256
    first = (n - 1) // stride * stride
    return first + (n - 1 - first) // 2


def _set_t(d, p, t, side):
    """sj[p] + y[p] == t exactly in Float32 (t in [1, 2) by magnitude, sj[p] = -+0.25: every operand on t's grid)"""
    s = F32(0.25) if side < 0 else F32(-0.25)
    d["sj"][p] = s
    d["y"][p] = F32(F32(t) - s)
    assert F32(d["sj"][p] + d["y"][p]) == F32(t)


def sep_data(n, family, flavour="plain"):
    """Float32 (x, sj, y [, l, u, mask]) of one size and family, seeded by both.  flavours of the L-half cases: "subnormal" (every
    |v| subnormal), "huge" (every |v| ~ 1e38), "mixed" (a few of both among N(0, 1) data), "overflow" ((xk + sj) + y = +Inf)."""
    rng = rng_of("sep-%d-%s-%s" % (n, family, flavour))
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    y = np.clip(0.3 * rng.normal(size=n), -0.8, 0.8)
    if flavour == "subnormal":
        x, sj, y = 1e-40 * x, 1e-41 * sj, 1e-40 * y
    elif flavour == "huge":
        x, sj, y = 1e38 * np.clip(x, -2, 2), 1e37 * sj, 1e37 * y
    d = {"n": n, "x": x.astype(F32), "sj": sj.astype(F32), "y": y.astype(F32), "pokes": []}
    if flavour == "mixed":
        d["x"][0::5] = F32(1e38) * np.sign(d["x"][0::5])
        d["x"][1::5] = F32(1e-40)
        d["sj"][1::5] = F32(3e-41)
        d["y"][1::5] = F32(-7e-42)
    elif flavour == "overflow":
        d["x"][n // 2] = F32(3e38)
        d["sj"][n // 2] = F32(3e38)
        d["y"][n // 2] = F32(-3e38)          # (3e38 + 3e38) + -3e38: +Inf in Float32, 3e38 in Float64
    if flavour != "plain":
        if family == "box":
            big = F32(3e38) if flavour in ("huge", "mixed") else F32(2.0)
            d.update(l=-big, u=big, mask=(rng.random(n) < 0.6).astype(np.uint8))
        return d
    # exact zeros of v in Float32 that are not zero in Float64 (NormL0 / IndBallL0 count them out)
    if family == "binf":                      # v = (sj + y) + xk
        a32 = d["sj"] + d["y"]
        inexact = a32.astype(np.float64) != d["sj"].astype(np.float64) + d["y"].astype(np.float64)
        idx = np.flatnonzero(inexact)[::5]
        d["x"][idx] = -a32[idx]
    else:                                     # v = (xk + sj) + y
        a32 = d["x"] + d["sj"]
        inexact = a32.astype(np.float64) != d["x"].astype(np.float64) + d["sj"].astype(np.float64)
        if family == "box":                   # (sj + y stays well inside the box)
            inexact &= np.abs(d["sj"].astype(np.float64) - a32) <= 1.3
        idx = np.flatnonzero(inexact)[::5]
        d["y"][idx] = -a32[idx]
    assert len(idx) > 0 or n < 63, "no exact Float32 zero planted: the NormL0 / IndBallL0 cases would be vacuous"
    if family == "box":
        d["l"] = rng.uniform(-3.0, -1.6, size=n).astype(F32)
        d["u"] = rng.uniform(1.6, 3.0, size=n).astype(F32)
        d["mask"] = (rng.random(n) < 0.6).astype(np.uint8)
        # one element exactly at l - sqrt(eps32) and (n >= 3) one exactly at u + sqrt(eps32): feasible
        pl = n // 2
        _set_t(d, pl, T_LOW, -1)
        d["l"][pl] = L_EDGE
        if n >= 6:
            _set_t(d, n // 3, T_HIGH, +1)
            d["u"][n // 3] = U_EDGE
        # the only infeasible element, one Float32 ulp outside: at 0, at n - 1, in the last partial trip; and at the upper end
        for p in sorted({0, n - 1, last_trip_index(n)}):
            d["pokes"].append(("low@%d" % p, p, {"sj": F32(0.25), "y": F32(down(T_LOW) - F32(0.25)), "l": L_EDGE}))
        p = n - 1
        d["pokes"].append(("high@%d" % p, p, {"sj": F32(-0.25), "y": F32(up(T_HIGH) + F32(0.25)), "u": U_EDGE}))
    elif family == "binf":
        # one element exactly at the largest Float32 inside 1.1 Delta: feasible; one ulp up: +Inf
        _set_t(d, n // 2, T_IN, -1)
        for p in sorted({0, n - 1, last_trip_index(n)}):
            d["pokes"].append(("out@%d" % p, p, {"sj": F32(0.25), "y": F32(T_OUT - F32(0.25))}))
        d["pokes"].append(("out-@%d" % (n // 2), n // 2, {"sj": F32(-0.25), "y": F32(-T_OUT + F32(0.25))}))
    return d


def poked(d, poke):
    """a copy of the vectors of `d` with one poke applied"""
    _, p, vals = poke
    out = dict(d)
    for k, v in vals.items():
        out[k] = d[k].copy()
        out[k][p] = v
    return out


BOX_VARIANTS = ("vec-vec-mask", "vec-vec", "scal-scal", "vec-scal-mask", "scal-vec")


def box_args(d, variant):
    """(l, u, mask) of a Box variant: scalar bounds are the edge values (every other element lies well inside)"""
    if "l" in d and np.ndim(d["l"]) == 0:
        return d["l"], d["u"], d["mask"] if variant.endswith("mask") else None
    lk, uk = variant.split("-")[:2]
    return (d["l"] if lk == "vec" else L_EDGE), (d["u"] if uk == "vec" else U_EDGE), (d["mask"] if variant.endswith("mask") else None)


def sep_terms(orc, entry, d, variant=None):
    """(terms without lambda, infeasible) of one entry point on the vectors of `d`"""
    fam, kind = family_of(entry), kind_of(entry)
    if fam == "box":
        l, u, m = box_args(d, variant)
        return orc.obj_f32(kind, d["y"], d["x"], d["sj"], l=l, u=u, mask=m)
    if fam == "binf":
        return orc.obj_f32(kind, d["y"], d["x"], d["sj"], delta=DELTA)
    return orc.obj_f32(kind, d["y"], d["x"], d["sj"])


def check_value(got, entry, terms, infeasible, what, r=None):
    """the bar of one psi(y) value.  Returns the relative deviation from the exact sum (0.0 for the exact rules)."""
    import math
    kind = kind_of(entry)
    if entry.startswith("indball"):
        want = np.inf if (infeasible or int(terms.sum()) > r) else 0.0
        assert got == want, (what, got, want)
        return 0.0
    if infeasible:
        assert got == np.inf, (what, got)
        return 0.0
    if kind == "l0":                                          # lambda * count: one rounded product of exact operands
        want = float(LAM) * float(int(terms.sum()))
        assert got == want, (what, got, want)
        return 0.0
    cls = nonfinite.check_sum(got, terms, what, factor=float(LAM))
    if cls != "finite":
        return 0.0
    ref = float(LAM) * math.fsum(terms.tolist())
    return abs(got - ref) / (float(LAM) * nonfinite.magnitude(terms)) if ref else 0.0


# ====================================================================================================== groups
SIGMA = F32(0.8)
UNIFORM_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 300, 5000)


def lanes_by_typical(typical):
    lanes = 1
    while lanes < 64 and lanes * 4 < typical:
        lanes *= 2
    return lanes


def group_layouts(which):
    """[(name, n, offsets or None, gsize, ngroups, scale)] for which = "prox" (spx_prox_group_l2_f32) or "obj" (the two
    spx_obj_group_l2*_f32): every lane-count step, a last wavefront that is half live, the second trip of the grid-stride loop
    (prox: 16 workgroups per CU on 256 CUs; obj: 2048 workgroups), the CSR layouts."""
    out = []
    for gs in UNIFORM_SIZES:
        ng = 1001 if gs <= 129 else 301 if gs == 300 else 41
        assert ng % (4 * (64 // lanes_by_typical(gs))) != 0
        out.append(("uniform%d" % gs, gs * ng, None, gs, ng, 1.0))
    big = ((129, 16_400), (3, 1_050_000)) if which == "prox" else ((129, 8_200), (3, 530_000))
    for gs, ng in big:
        out.append(("trip2-gs%d" % gs, gs * ng, None, gs, ng, 1.0))
    rng = rng_of("layouts")
    n = 60_001
    cuts = np.sort(rng.integers(0, n + 1, size=2999))
    cuts[100:140] = cuts[100]                                   # a run of empty groups (and whatever the draw repeats)
    ragged = np.concatenate([[0], np.sort(cuts), [n]]).astype(np.int64)
    out.append(("ragged-empty", n, ragged, 0, len(ragged) - 1, 1.0))
    n = 40_009
    cuts = np.sort(rng.integers(37, n - 41, size=1499))
    unc = np.concatenate([[37], cuts, [n - 41]]).astype(np.int64)   # head [0, 37) and tail [n - 41, n) in no group
    out.append(("uncovered", n, unc, 0, len(unc) - 1, 1.0))
    out.append(("one-group", 100_003, np.array([0, 100_003], dtype=np.int64), 0, 1, 1.0))
    out.append(("no-groups", 5_003, np.array([11], dtype=np.int64), 0, 0, 1.0))
    out.append(("all-1e30", 5 * 37, None, 5, 37, 1e30))
    out.append(("all-1e-30", 5 * 37, None, 5, 37, 1e-30))
    return out


def offsets_of(lay):
    name, n, offsets, gs, ng, scale = lay
    return offsets if offsets is not None else np.arange(0, n + 1, gs, dtype=np.int64)


def group_data(lay):
    """Float32 (x, sj, q, y, y0, lam) of a layout.  lambda: close neighbours (steps of 2^-20 around 0.7) -- a lambda indexed one
    group off moves psi(y) by ~1e-7 relative.  Planted where the layout has the groups for it: a group whose S is all zero,
    a group thresholded to zero, and a group of |S| = 1e-30 with a lambda of its own size (a norm that is zero if the squares are
    Float32).  scale != 1: every vector and lambda times that (|S| = 1e30: the squares overflow Float32)."""
    name, n, offsets, gs, ng, scale = lay
    rng = rng_of("group-" + name)
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    q = rng.normal(size=n)
    y = np.clip(0.3 * rng.normal(size=n), -0.8, 0.8)
    y0 = rng.normal(size=n)                                       # y on entry: the uncovered indices keep y0 - (xk + sj)
    lam = 0.7 + 2.0 ** -20 * ((np.arange(ng) * 5) % 11)
    d = {"n": n, "lam": lam.astype(F32)}
    offs = offsets_of(lay)
    sizes = np.diff(offs)
    full = np.flatnonzero(sizes > 0)
    if scale == 1.0 and len(full) >= 8:
        gz, gt, ge = (int(full[k]) for k in (1, len(full) // 2, len(full) - 2))
        a, b = offs[gz], offs[gz + 1]
        sj[a:b] = 0.0
        q[a:b] = -x[a:b].astype(F32)                               # (q + xk) + 0 == 0
        a, b = offs[gt], offs[gt + 1]
        for v in (x, sj, q):
            v[a:b] *= 2.0 ** -12                                   # ||S|| << sigma lambda: alpha = 0
        a, b = offs[ge], offs[ge + 1]
        x[a:b] = 0.0
        sj[a:b] = 0.0
        q[a:b] = 1e-30 * np.sign(q[a:b])
        y[a:b] = 1e-30 * np.sign(y[a:b])
        d["lam"][ge] = F32(1e-31)
        d["planted"] = (gz, gt, ge)
    d["pokes"] = []
    if scale == 1.0 and n >= 8:
        # psi(y) of the Binf form: sj + y exactly at the largest Float32 inside 1.1 Delta (feasible) at n - 1; one ulp outside, at
        # 0 or at n - 1 (in no group where the layout leaves head and tail uncovered): +Inf
        sj[n - 1], y[n - 1] = 0.25, float(F32(T_IN - F32(0.25)))
        for p in (0, n - 1):
            d["pokes"].append(("out@%d" % p, p, {"sj": F32(0.25), "y": F32(T_OUT - F32(0.25))}))
    if scale != 1.0:
        x, sj, q, y, y0 = (scale * v for v in (x, sj, q, y, y0))
        d["lam"] = (d["lam"].astype(np.float64) * scale).astype(F32)
    d.update(x=x.astype(F32), sj=sj.astype(F32), q=q.astype(F32), y=y.astype(F32), y0=y0.astype(F32))
    return d


# The Float32 group cases of two older files, seeded here so that their census runs on the CPU (tests/test_oracle_f32_forms.py)
API_GROUP_SIZES = (1, 2, 3, 4, 7, 9, 16, 33, 64, 128, 1000)     # tests/test_gpu_f32.py::test_f32_group_l2
REDZONE_GROUP_LAYOUTS = ("uniform", "ragged")                   # tests/test_gpu_redzone.py: grp-f32-*


def _plain_group_data(tag, n, ng, lam_lo, lam_hi):
    rng = rng_of(tag)
    return {"x": rng.normal(size=n).astype(F32), "sj": rng.uniform(-0.5, 0.5, size=n).astype(F32),
            "q": rng.normal(size=n).astype(F32), "lam": rng.uniform(lam_lo, lam_hi, size=ng).astype(F32),
            "y0": np.zeros(n, dtype=F32)}


def api_group_case(gs):
    """(layout, data, sigma): 3000 uniform groups of gs"""
    ng = 3000
    lay = ("api-uniform%d" % gs, ng * gs, None, gs, ng, 1.0)
    return lay, _plain_group_data(lay[0], ng * gs, ng, 0.2, 3.0), F32(0.8)


def redzone_group_case(name):
    """(layout, data, sigma): 2001 uniform groups of 16, or 3001 ragged groups over 200 003 elements"""
    if name == "uniform":
        lay = ("redzone-uniform", 16 * 2001, None, 16, 2001, 1.0)
    else:
        n = 200_003
        cuts = np.sort(rng_of("redzone-ragged-cuts").choice(np.arange(1, n), size=3000, replace=False))
        lay = ("redzone-ragged", n, np.concatenate([[0], cuts, [n]]).astype(np.int64), 0, 3001, 1.0)
    return lay, _plain_group_data(lay[0], lay[1], lay[4], 0.3, 1.5), F32(0.9)


def _exact_square_sum(v):
    """sum of v[i]^2 as a Fraction (v Float32)"""
    tot = Fraction(0)
    for f in v.astype(np.float64).tolist():
        a, b = f.as_integer_ratio()
        tot += Fraction(a * a, b * b)
    return tot


def census(S, offs):
    """S = sol = (q + xk) + sj in Float32; offs = CSR offsets.  Returns (snorm, ambiguous):
    snorm[g] = the EXACT norm of group g rounded to Float32 once (what the restatement must use);
    ambiguous = {g: (lower neighbour, upper neighbour)} for the groups whose exact norm lies within 1e-12 relative of the
    midpoint of two adjacent Float32 values.  Groups whose Float64 norm is far from every midpoint are settled in Float64 (its
    error is below 1e-15 per element of the group); the others with the exact sum of the exact squares."""
    offs = np.asarray(offs, dtype=np.int64)
    ng = len(offs) - 1
    sq = S.astype(np.float64) ** 2                                 # exact: 48 significant bits at most
    ss = np.zeros(ng)
    full = np.flatnonzero(np.diff(offs) > 0)
    if len(full):
        # reduceat runs each segment to the next start: the groups are contiguous, so that is the group's end -- except for the
        # last one, which reduceat runs to the end of S
        red = np.add.reduceat(sq, offs[full])
        last = int(full[-1])
        red[-1] = sq[offs[last]:offs[last + 1]].sum()
        ss[full] = red
    nrm = np.sqrt(ss)
    with np.errstate(over="ignore"):
        f = nrm.astype(F32)
    lo = np.where(f.astype(np.float64) <= nrm, f, np.nextafter(f, -INF32)).astype(F32)    # lo <= nrm < hi
    hi = np.nextafter(lo, INF32)
    mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))   # exact in Float64
    window = max(1e-11, 1e-15 * float(np.diff(offs).max() if ng else 1))
    snorm = f.copy()
    ambiguous = {}
    finite = np.isfinite(hi) & (nrm > 0)
    near = np.flatnonzero(finite & (np.abs(nrm - mid) <= window * mid))
    for g in near.tolist():
        exact = _exact_square_sum(S[offs[g]:offs[g + 1]])
        m = Fraction(float(mid[g]))
        snorm[g] = hi[g] if exact >= m * m else lo[g]            # (an exact tie rounds to even: ambiguous below anyway)
        if (m * (1 - AMBIGUOUS_REL)) ** 2 <= exact <= (m * (1 + AMBIGUOUS_REL)) ** 2:
            ambiguous[g] = (lo[g], hi[g])
    return snorm, ambiguous


def ambiguity_cap(ngroups):
    return max(1, ngroups // 1000)


def sol_of(d):
    return ((d["q"] + d["x"]).astype(F32) + d["sj"]).astype(F32)


def prox_reference(orc, lay, d, sigma=None):
    """(ref, ambiguous, alternatives): ref = the restatement with every group's exact norm rounded once; alternatives[g] = the
    two results an ambiguous group may take (its rows of the restatement with the lower / the upper neighbour)"""
    name, n, offsets, gs, ng, scale = lay
    offs = offsets_of(lay)
    sigma = SIGMA if sigma is None else F32(sigma)
    snorm, amb = census(sol_of(d), offs)
    kw = dict(offsets=offsets, gsize=gs if offsets is None else 0, y0=d["y0"])
    ref = orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], sigma, snorm=snorm, **kw)
    alts = {}
    if amb:
        lo, hi = snorm.copy(), snorm.copy()
        for g, (a, b) in amb.items():
            lo[g], hi[g] = a, b
        rl = orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], sigma, snorm=lo, **kw)
        rh = orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], sigma, snorm=hi, **kw)
        for g in amb:
            alts[g] = (rl[offs[g]:offs[g + 1]].copy(), rh[offs[g]:offs[g + 1]].copy())
    return ref, amb, alts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_prox(got, lay, ref, amb, alts, what):
    """the bit rule.  Returns the number of ambiguous groups that took the neighbour the correctly rounded norm does not."""
    offs = offsets_of(lay)
    got = np.ascontiguousarray(got, dtype=F32)
    bad = np.flatnonzero(got.view(np.int32) != ref.view(np.int32))
    if not len(bad):
        return 0
    gi = np.searchsorted(offs, bad, side="right") - 1             # (the last group that starts at or before the index)
    assert gi.min() >= 0 and bad.max() < offs[-1], "%s: an index in no group differs from y0 - (xk + sj) (first %d)" % (what, int(bad[0]))
    other = 0
    for g in np.unique(gi).tolist():
        assert g in amb, "%s: group %d differs from the restatement (first index %d, %d elements in all) and is not ambiguous" % (
            what, g, int(bad[gi == g][0]), len(bad))
        row = got[offs[g]:offs[g + 1]]
        assert same_bits(row, alts[g][0]) or same_bits(row, alts[g][1]), "%s: ambiguous group %d equals neither neighbour's result" % (what, g)
        other += 1
    return other


def obj_group_terms(orc, lay, d, binf):
    name, n, offsets, gs, ng, scale = lay
    return orc.obj_group_f32(d["y"], d["x"], d["sj"], d["lam"], offsets=offsets, gsize=gs if offsets is None else 0,
                             delta=(DELTA * F32(scale) if binf else None))


def check_group_value(got, terms, outside, what):
    import math
    if outside:
        assert got == np.inf, (what, got)
        return 0.0
    nonfinite.check_sum(got, terms, what)
    ref = math.fsum(terms.tolist())
    return abs(got - ref) / nonfinite.magnitude(terms) if ref else 0.0
