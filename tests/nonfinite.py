"""Non-finite and extreme data for the fused and reduction kernels: plant sets, the IEEE class rules and the nan-aware bars.

Plain helper module (like tests/arbiter.py): numpy and the CPU oracle only, no torch, no GPU.  tests/test_nonfinite_helpers.py
checks it against the oracle alone; tests/test_gpu_nonfinite.py uses it on the device results.

A plant set overwrites a handful of positions of the clean, seeded vectors (q, xk, sj) of the neighbouring tests.  The positions
always hold element 0, the last element and whatever the caller adds (an element of another workgroup / tile / group).

Magnitudes: the `huge` set is +-1e150 in xk.  There y = prox - (xk + sj) stays of the size of q for every separable operator,
the terms q y and y^2 stay small and the terms of h stay near 1e150: sum |term| < 1e300, the condition check_sum asserts on
its inputs.  1e150 in q or sj gives |y| ~ 1e150 on the unboxed / boxed operators and y^2 ~ 1e300: outside that condition, as are
1e200 and 1e308, whose squares overflow.  So that a large y does travel through <q, y> and <y, y>, the `large` set plants
+-1e148 in q and in sj: |y| ~ 1e148, q y and y^2 ~ 1e296, a handful of them below 1e300.
"""
import math
import zlib

import numpy as np

TOL = 1e-12
MAG_LIMIT = 1e300
HUGE = 1e150
LARGE = 1e148
TINY = (0.0, -0.0, 5e-324, -5e-324, 1e-150, -1e-150)

PLANTS = ("none", "nan-q", "nan-xk", "nan-sj", "pinf-q", "ninf-q", "pminf-q", "pinf-xk", "pinf-sj", "tiny")
PLANTS_SEPARABLE = PLANTS + ("huge", "large")
INF_PLANTS = ("pinf-q", "ninf-q", "pminf-q", "pinf-xk", "pinf-sj")
_SINGLE = {"nan-q": (0, np.nan), "nan-xk": (1, np.nan), "nan-sj": (2, np.nan), "pinf-q": (0, np.inf), "ninf-q": (0, -np.inf),
           "pinf-xk": (1, np.inf), "pinf-sj": (2, np.inf)}


# ---------------------------------------------------------------- plants
def positions(n, extra=()):
    """element 0, the last element, then `extra`; duplicates dropped, order kept"""
    out = []
    for p in [0, n - 1] + [int(e) for e in extra]:
        assert 0 <= p < n, (p, n)
        if p not in out:
            out.append(p)
    return out


def plant(name, q, xk, sj, pos):
    """copies of (q, xk, sj) with the plant set `name` written at the positions `pos`"""
    vs = [np.array(v, dtype=np.float64) for v in (q, xk, sj)]
    pos = list(pos)
    if name == "none":
        pass
    elif name in _SINGLE:
        which, value = _SINGLE[name]
        vs[which][pos] = value
    elif name == "pminf-q":                       # +Inf and -Inf at different positions
        assert len(pos) >= 2
        vs[0][pos[0::2]] = np.inf
        vs[0][pos[1::2]] = -np.inf
    elif name == "tiny":                          # +-0, +-5e-324, +-1e-150 spread over q, xk, sj
        for k, p in enumerate(pos):
            for j in range(3):
                vs[j][p] = TINY[(k + 2 * j) % 6]
    elif name == "huge":
        for k, p in enumerate(pos):
            vs[1][p] = HUGE if k % 2 == 0 else -HUGE
    elif name == "large":                         # q at the even plants, sj at the odd ones, alternating signs
        for k, p in enumerate(pos):
            vs[0 if k % 2 == 0 else 2][p] = LARGE if k % 4 < 2 else -LARGE
    else:
        raise ValueError(name)
    for v in vs:
        v.setflags(write=False)
    return vs


# ---------------------------------------------------------------- the class rules
FINITE, PINF, NINF, NANC = 0, 1, 2, 3


def classes(a):
    """per element: 0 finite, 1 +Inf, 2 -Inf, 3 NaN"""
    a = np.asarray(a, dtype=np.float64)
    c = np.zeros(a.shape, dtype=np.int8)
    c[a == np.inf] = PINF
    c[a == -np.inf] = NINF
    c[np.isnan(a)] = NANC
    return c


def same_bits_or_both_nan(a, b):
    """per element: equal int64 bits, or both NaN (any payload)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def scalar_same(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


def triple_same(a, b):
    return len(a) == len(b) and all(scalar_same(u, v) for u, v in zip(a, b))


def sum_class(terms):
    """what IEEE addition gives for these terms in ANY order, overflow apart: "nan" (a NaN term, or both signs of Inf), "+inf",
    "-inf", or "finite" """
    t = np.asarray(terms, dtype=np.float64)
    p, m = bool(np.any(t == np.inf)), bool(np.any(t == -np.inf))
    if bool(np.any(np.isnan(t))) or (p and m):
        return "nan"
    return "+inf" if p else "-inf" if m else "finite"


def scalar_class(v):
    v = float(v)
    return "nan" if math.isnan(v) else "+inf" if v == math.inf else "-inf" if v == -math.inf else "finite"


def magnitude(terms):
    """sum of the magnitudes of the finite terms: the input condition of check_sum"""
    t = np.asarray(terms, dtype=np.float64)
    return math.fsum(np.abs(t[np.isfinite(t)]).tolist())


def check_sum(got, terms, what, factor=1.0, exact=False, tol=TOL):
    """`got` against factor * (sum of `terms`): the class by sum_class; a finite sum to tol * |factor| * sum |term| of math.fsum
    (exact=True: equality, the bar of the NormL0 value).  factor is finite and > 0.  Returns the class."""
    t = np.asarray(terms, dtype=np.float64)
    mag = magnitude(t)
    assert mag < MAG_LIMIT, (what, mag)            # a condition on the test's own inputs
    cls = sum_class(t)
    got = float(got)
    print("%s: got %r class %s sum |term| %.3g" % (what, got, cls, mag))
    if cls != "finite":
        assert scalar_class(got) == cls, (what, got, cls)
        return cls
    ref = factor * math.fsum(t.tolist())
    assert math.isfinite(got), (what, got, ref)
    if exact:
        assert got == ref, (what, got, ref)
    else:
        assert abs(got - ref) <= tol * abs(factor) * mag, (what, got, ref, mag)
    return cls


def check_qy_yy(q, y, qy, yy, what):
    """[1] and [2] of a step call from the y the device returned and the q that was passed"""
    with np.errstate(all="ignore"):
        tq, ty = q * y, y * y
    return check_sum(qy, tq, what + " [1]"), check_sum(yy, ty, what + " [2]")


def h_terms(kind, v):
    """the terms of h (without lambda) at v = (xk + sj) + y: oracle/spx_oracle.c h_term"""
    with np.errstate(all="ignore"):
        if kind == "l1":
            return np.abs(v)
        if kind == "l0":
            return (v != 0.0).astype(np.float64)   # (NaN != 0: a NaN counts, the count is always finite)
        return np.sqrt(np.abs(v))


def group_terms(v, lam, starts, sizes):
    """lambda_g * sqrt(sum_{i in g} v_i^2) per group -- 0 * Inf is NaN here as on any IEEE machine"""
    out = np.zeros(len(sizes))
    with np.errstate(all="ignore"):
        for g, (a, m) in enumerate(zip(starts, sizes)):
            sq = v[a:a + m] * v[a:a + m]
            c = sum_class(sq)
            ss = math.fsum(sq.tolist()) if c == "finite" else {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[c]
            out[g] = lam[g] * np.sqrt(ss)
    return out


# ---------------------------------------------------------------- the nan-aware bars against the oracle
def check_classes(y, ref, what):
    bad = np.flatnonzero(classes(y) != classes(ref))
    assert bad.size == 0, "%s: %d elements of another class than the oracle's, first %d: %r vs %r" % (
        what, bad.size, int(bad[0]), float(y[bad[0]]), float(ref[bad[0]]))


def check_exact(y, ref, what):
    """the L1 / L0 families: the oracle's class everywhere and its bits on every non-NaN entry"""
    check_classes(y, ref, what)
    bad = np.flatnonzero(~same_bits_or_both_nan(y, ref))
    assert bad.size == 0, "%s: %d elements differ from the oracle, first %d: %r vs %r" % (
        what, bad.size, int(bad[0]), float(y[bad[0]]), float(ref[bad[0]]))


def check_lhalf(y, ref, q, x, sj, what, box, tol=TOL):
    """RootNormLhalf(Box): tests/test_gpu_parity.py::test_special_values_lhalf -- the oracle's NaN pattern, its +-Inf, finite
    entries to tol * max(|ref|, |x + s|, |q|) (a non-finite scale counts as 1); the Box form leaves out the elements whose data
    are +-Inf or beyond 1e300, as that test does"""
    y, ref = np.asarray(y), np.asarray(ref)
    if box:
        big = lambda a: np.abs(np.nan_to_num(a, nan=0.0)) >= 1e300
        ok = ~(big(q) | big(x) | big(sj))
        y, ref = np.where(ok, y, 0.0), np.where(ok, ref, 0.0)
    assert np.array_equal(np.isnan(y), np.isnan(ref)), (what, int(np.sum(np.isnan(y) != np.isnan(ref))))
    inf = np.isinf(ref)
    assert np.array_equal(y[inf], ref[inf]), what
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        scale = np.maximum(np.maximum(np.abs(ref), np.abs(x + sj)), np.abs(q))
        bad = fin & ~(np.abs(y - ref) <= tol * np.where(np.isfinite(scale), scale, 1.0))
    assert not bad.any(), (what, int(bad.sum()), int(np.flatnonzero(bad)[0]))


def nan_norm(a):
    """2-norm over the finite entries"""
    a = np.asarray(a, dtype=np.float64)
    return float(np.linalg.norm(a[np.isfinite(a)]))


def check_b2(y, ref, x, what, tol=TOL):
    """ShiftedNormL1B2: the oracle's classes; finite entries to tol * max(||ref||, ||xk||), the norms over the finite entries"""
    check_classes(y, ref, what)
    fin = np.isfinite(ref)
    scale = max(nan_norm(ref), nan_norm(x))
    err = float(np.max(np.abs(y[fin] - ref[fin]))) if fin.any() else 0.0
    print("%s: max |y - oracle| over %d finite entries %.3e (bar %.3e)" % (what, int(fin.sum()), err, tol * scale))
    assert err <= tol * scale, (what, err, scale)


def check_group(orc, arbiter, y, ref, q, x, sj, lam, sigma, offsets, delta, what, tol=TOL):
    """ShiftedGroupNormL2(Binf): the oracle's classes; then arbiter.check_group on np.where(finite, ., 0), as
    tests/test_gpu_stress.py::_binf_run_and_check.  The arbiter's scale needs finite data, so the groups that hold a
    non-finite input or result are checked here -- finite entries to tol * max(|ref|, |xk + sj|, ||S_g|| over the finite
    entries), the arbiter's plain bar -- and handed to the arbiter as zeros."""
    check_classes(y, ref, what)
    offsets = np.asarray(offsets, dtype=np.int64)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        S = (q + x) + sj
    dirty = ~(np.isfinite(q) & np.isfinite(x) & np.isfinite(sj) & fin)
    qa, xa, sa = (np.array(v) for v in (q, x, sj))
    ya, ra = np.where(fin, y, 0.0), np.where(fin, ref, 0.0)
    lo, hi = int(offsets[0]), int(offsets[-1])
    for g in np.unique(np.searchsorted(offsets, np.flatnonzero(dirty[lo:hi]) + lo, side="right") - 1):
        sl = slice(int(offsets[g]), int(offsets[g + 1]))
        f = fin[sl] & np.isfinite(x[sl]) & np.isfinite(sj[sl])
        with np.errstate(all="ignore"):
            scale = np.maximum(np.maximum(np.abs(ref[sl]), np.abs(x[sl] + sj[sl])), nan_norm(S[sl]))
            bad = f & ~(np.abs(y[sl] - ref[sl]) <= tol * scale)
        assert not bad.any(), "%s: group %d (non-finite data): %d finite entries off the oracle, first %r vs %r" % (
            what, int(g), int(bad.sum()), float(y[sl][bad][0]), float(ref[sl][bad][0]))
        for a in (qa, xa, sa, ya, ra):
            a[sl] = 0.0
    for a, b in ((qa, q), (xa, x), (sa, sj)):      # (indices no group contains: outside the arbiter's scale)
        keep = np.ones(a.shape, dtype=bool)
        keep[lo:hi] = False
        a[keep & ~np.isfinite(b)] = 0.0
    out = ~np.isfinite(xa + sa) | ~np.isfinite(ya) | ~np.isfinite(ra)
    assert not out.any()
    return arbiter.check_group(orc, ya, ra, qa, xa, sa, lam, sigma, offsets, delta=delta, what=what)


# ---------------------------------------------------------------- the clean data of the neighbouring tests (host side)
def separable_data(n, seed):
    """tests/test_gpu_proxstep.py::_data"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    q = rng.normal(size=n)
    lo, up = -1.0 - 0.1 * rng.random(n), 1.0 + 0.1 * rng.random(n)
    selected = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    return x, sj, q, lo, up, selected


def b2_data(n):
    """tests/test_gpu_proxstep_b2.py::_data (seed = n)"""
    rng = np.random.default_rng(n)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    return x, sj, q


class GroupData:
    """The host side of tests/test_gpu_proxstep_group.py::Problem: one layout, its data and its weights."""

    def __init__(self, layout, binf, seed=0):
        kind, arg = layout
        rng = np.random.default_rng(zlib.crc32(("%s%s%d%d" % (kind, arg, binf, seed)).encode()))
        self.offsets = None
        if kind == "uniform":
            gs = arg
            ng = 301 if gs <= 128 else 61 if gs <= 1024 else 13
            n, self.gsize, sizes = gs * ng, gs, np.full(ng, gs)
        elif kind == "one":
            n, ng, self.gsize, sizes = arg, 1, arg, np.array([arg])
        else:
            ng = 700
            sizes = rng.integers(0, 61, size=ng)
            sizes[::97] = 0
            if kind == "csr_over":
                sizes[ng // 2] = 777
            head = 5
            off = head + np.concatenate([[0], np.cumsum(sizes)])
            n = int(off[-1]) + 9
            self.offsets = off.astype(np.int64)
            self.gsize = {"csr_bound": int(sizes.max()), "csr_nobound": 0, "csr_over": 60}[kind]
        self.n, self.ng, self.binf, self.sizes = n, ng, binf, np.asarray(sizes, dtype=np.int64)
        x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
        lat = n // 3
        x[:lat] = rng.integers(-8, 9, size=lat) / 4.0
        sj[:lat] = rng.integers(-2, 3, size=lat) / 4.0
        q[:lat] = rng.integers(-12, 13, size=lat) / 4.0
        x[: lat // 2] = 0.0
        if kind == "uniform":
            x[: self.gsize] = 0.0
        self.sigma, self.delta = 0.5, 1.0
        self.starts = np.asarray(self.offsets[:-1] if self.offsets is not None else np.arange(ng) * self.gsize, dtype=np.int64)
        S = (q + x) + sj
        nS = np.array([np.linalg.norm(S[a:a + m]) for a, m in zip(self.starts, sizes)])
        fac = rng.choice([0.0, 0.3, 0.7, 1.0, 1.5, 4.0, 40.0], size=ng)
        lam = np.where(nS > 0, nS, 1.0) * fac / self.sigma
        if kind != "one":
            lam[: ng // 3] = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0, 8.0], size=ng // 3)
        else:
            lam[:] = 0.6 * nS / self.sigma
        if kind == "uniform":
            lam[0], lam[1] = 40.0 * nS[0] / self.sigma, 0.3 * nS[1] / self.sigma
        self.x, self.sj, self.q, self.lam = x, sj, q, lam
        # CSR offsets over [0, n) for the host-side checks (the uniform layouts have none on the device)
        self.csr = self.offsets if self.offsets is not None else np.arange(ng + 1, dtype=np.int64) * self.gsize

    def oracle(self, orc, q, x, sj, y0=None):
        """the reference's prox on (q, x, sj); indices no group contains keep y0 (the plain operator subtracts the shift there,
        as tests/test_gpu_proxstep_group.py::test_every_layout states)"""
        kw = dict(offsets=self.offsets) if self.offsets is not None else dict(gsize=self.gsize)
        with np.errstate(all="ignore"):
            if self.binf:
                y = orc.prox_group_l2_binf(q, x, sj, self.lam, self.sigma, self.delta, **kw)
            else:
                y = orc.prox_group_l2(q, x, sj, self.lam, self.sigma, **kw)
            if y0 is not None and self.offsets is not None:
                lo, hi = int(self.offsets[0]), int(self.offsets[-1])
                out = np.r_[0:lo, hi:self.n]
                y[out] = y0 if self.binf else y0 - (x + sj)[out]
        return y

    def plant_positions(self, arbiter, y_clean):
        """element 0, the last element, the middle of a group the prox zeroes and of one it shrinks (neither the first group
        when there is another); returns (positions, zeroed group or None, shrunk group or None)"""
        if self.ng == 1:
            return positions(self.n, [self.n // 2]), None, None
        zp = arbiter.zero_pattern(y_clean, self.x, self.sj, self.csr)
        big = self.sizes >= 2
        gz = [g for g in range(1, self.ng) if big[g] and zp[g]] or [g for g in (0,) if big[g] and zp[g]]   # (Binf zeroes few: |xk| <= Delta)
        gsh = [g for g in range(1, self.ng) if big[g] and not zp[g]]
        assert gz and gsh, (len(gz), len(gsh))
        mid = lambda g: int(self.starts[g] + self.sizes[g] // 2)
        return positions(self.n, [mid(gz[0]), mid(gsh[0])]), gz[0], gsh[0]


# ---------------------------------------------------------------- the separable operators (the constructions of _nine)
SEP_LAM, SEP_SIGMA = 0.7, 1.1
SEP_OPS = [(kind, form) for kind in ("l1", "l0", "lhalf") for form in ("plain", "box", "vecbox+mask")]


def sep_box(form, lo, up, selected, n):
    """(l, u, mask) of one construction: None / the scalar box of shifted(h, xk, 0.9, NormLinf(1.0)) / vector bounds and a mask"""
    if form == "plain":
        return None
    if form == "box":
        return -0.9, 0.9, None
    mask = np.zeros(n, dtype=np.uint8)
    mask[np.asarray(selected, dtype=np.int64)] = 1
    return lo, up, mask


def sep_oracle(orc, kind, box, q, x, sj):
    with np.errstate(all="ignore"):
        if box is None:
            return getattr(orc, "prox_" + kind)(q, x, sj, SEP_LAM, SEP_SIGMA)
        l, u, mask = box
        return getattr(orc, "prox_%s_box" % kind)(q, x, sj, SEP_LAM, SEP_SIGMA, l, u, mask)


def sep_selected(box, n):
    """the indices h runs over"""
    if box is None or box[2] is None:
        return np.arange(n)
    return np.flatnonzero(box[2])


def sep_check(orc, kind, box, y, ref, q, x, sj, what):
    """item 5 for one separable operator"""
    if kind == "lhalf":
        check_classes(np.where(_lhalf_ok(box, q, x, sj), y, 0.0), np.where(_lhalf_ok(box, q, x, sj), ref, 0.0), what)
        check_lhalf(y, ref, q, x, sj, what, box is not None)
    else:
        check_exact(y, ref, what)


def _lhalf_ok(box, q, x, sj):
    if box is None:
        return np.ones(q.shape, dtype=bool)
    big = lambda a: np.abs(np.nan_to_num(a, nan=0.0)) >= 1e300
    return ~(big(q) | big(x) | big(sj))
