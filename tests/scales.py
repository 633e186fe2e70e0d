"""Scaled problems: every operator on a WHOLE problem whose magnitude is 2^k (CPU only: numpy and the oracle).

The other sweeps of the suite keep the data near 1 (tests/test_gpu_fuzz.py: 1e-6 .. 1e6) or plant single extreme elements among
ordinary ones (tests/nonfinite.py).  Here every quantity of a problem is multiplied by a power of two, so that every term of
every sum is large or tiny at once and nothing hides behind the ordinary elements, while every square, product, norm, quotient
and root-find stays a NORMAL double:

    quantity                                             scale
    q, xk, sj, g, the bounds l and u, Delta              c = 2^k
    lambda of NormL1, GroupNormL2, NormL1B2              c
    lambda of NormL0                                     c^2
    lambda of RootNormLhalf                              c^(3/2)   (k even)
    r, sigma, chi's lambda, the diagonal d of iprox!, q_scale      unchanged

With these the exact minimiser of the scaled problem is c times the minimiser of the unscaled one.  Whether the Float64 (Float32)
evaluation is equivariant BIT FOR BIT is a property of each formula: tests/test_scales_helpers.py pins it for the oracle, per
operator (BIT_EQUIVARIANT below), and names the formulas of the reference that are not scale-free (the absolute epsilon = 1 of
the ShiftedGroupNormL2Binf bracket, the absolute eps of IndBallL2, the sqrt(eps) slack of the box objectives): there the oracle
on the SCALED problem is the expectation, not the scaled answer.

Data are N(0, 1) from seeded default_rng streams, drawn in the order x, 0.3 * sj, q.  Every nonzero magnitude below 2^-10 is
raised to +-2^-10 -- of q, xk, sj and of the two sums the operators square, xk + sj and (q + xk) + sj -- and a few exact zeros
are planted (zeros in q, an all-zero group), so that at k = -500 every nonzero square is a normal double.  assert_in_range states
that condition and checks it on the host: inputs outside it are a mistake in the test, not a kernel failure.

The oracle's norm is sqrt(sum v^2) (oracle/spx_oracle.c), not overflow-safe like LinearAlgebra.norm: the sets stop at 2^+-500.
"""
import math

import numpy as np

K64 = (-500, -200, -40, 40, 200, 500)      # n <= 1e4
K64_LARGE = (-480, 480)                    # the few larger shapes
K32 = (-60, -40, 40, 60)                   # Float32
FLOOR = 2.0 ** -10                         # the smallest nonzero magnitude of the unscaled data
MAX_SUM = 1e307                            # n * max v^2 * c^2, the products and lambda * ||.|| stay below this
MIN_SQUARE = 2.3e-308                      # the smallest nonzero v^2 * c^2 stays at or above this (DBL_MIN = 2.2250738585072014e-308)
MAX_SUM32, MIN_SQUARE32 = 1e38, 1.2e-38    # Float32: bounds on the values themselves (FLT_MAX = 3.4e38, FLT_MIN = 1.1754944e-38)

# exponent of c in lambda, by the h of the operator
LAM_POW = {"l1": 1.0, "l0": 2.0, "lhalf": 1.5, "group": 1.0, "b2": 1.0, "topr": 0.0}
# operators whose ORACLE is bit-equivariant on these problems (tests/test_scales_helpers.py asserts it at every k of their set):
# the GPU comparisons may demand bits of y(2^k P) against 2^k y(P) for the ones the library holds bit for bit against the oracle
BIT_EQUIVARIANT = ("prox_l1", "prox_l0", "prox_l1_box", "prox_l0_box", "prox_lhalf", "prox_lhalf_box", "prox_group_l2",
                   "prox_indball_l0", "prox_indball_l0_binf", "prox_l1_b2", "iprox_l1", "iprox_l0", "iprox_l1_box", "iprox_l0_box")
NOT_EQUIVARIANT = ("prox_group_l2_binf", "obj_l1_b2")
F32_OPS = ("prox_l1", "prox_l0", "prox_l1_box", "prox_l0_box", "iprox_l1", "iprox_l0", "iprox_l1_box", "iprox_l0_box",
           "prox_indball_l0", "prox_indball_l0_binf", "prox_group_l2")

_H = {"prox_l1": "l1", "prox_l0": "l0", "prox_lhalf": "lhalf", "prox_l1_box": "l1", "prox_l0_box": "l0", "prox_lhalf_box": "lhalf",
      "iprox_l1": "l1", "iprox_l0": "l0", "iprox_l1_box": "l1", "iprox_l0_box": "l0", "prox_group_l2": "group",
      "prox_group_l2_binf": "group", "prox_indball_l0": "topr", "prox_indball_l0_binf": "topr", "prox_l1_b2": "b2"}


class Problem:
    """One call: op (a key of _H), the vectors q (g for iprox!), xk, sj [, d], the weights lam (a scalar, or one per group),
    sigma, and what the operator needs of l, u (scalars or vectors), mask (uint8 or None), delta, r, chi, offsets / gsize /
    index sets.  k is the scale it stands at (0 as made); read-only arrays."""

    def __init__(self, **kw):
        self.k = 0
        self.d = self.l = self.u = self.mask = self.delta = self.r = self.offsets = self.groups = None
        self.gsize = 0
        self.chi = 1.0
        self.sigma = 1.0
        self.__dict__.update(kw)
        for a in self.vectors().values():
            a.setflags(write=False)

    @property
    def h(self):
        return _H[self.op]

    @property
    def n(self):
        return self.q.shape[0]

    @property
    def f32(self):
        return self.q.dtype == np.float32

    def vectors(self):
        """the arrays that carry the scale c (d, the mask and the layouts do not)"""
        out = {"q": self.q, "xk": self.xk, "sj": self.sj}
        for name in ("l", "u"):
            v = getattr(self, name)
            if v is not None and np.ndim(v) == 1:
                out[name] = v
        return out

    def csr(self):
        """CSR offsets of the contiguous groups"""
        if self.offsets is not None:
            return np.asarray(self.offsets, dtype=np.int64)
        return np.arange(0, self.n + 1, self.gsize, dtype=np.int64)


def pow2(k):
    return math.ldexp(1.0, int(k))


def lam_shift(h, k):
    """the exponent by which lambda moves at scale 2^k"""
    e = LAM_POW[h] * k
    assert e == int(e), "RootNormLhalf: lambda scales by c^(3/2), k must be even"
    return int(e)


def scaled(problem, k):
    """the problem at scale 2^k (of the unscaled one: scaled(scaled(P, a), b) is refused)"""
    assert problem.k == 0, "scale the unscaled problem"
    kw = dict(problem.__dict__)
    sh = lambda v: None if v is None else (np.ldexp(v, int(k)) if np.ndim(v) else (type(v)(np.ldexp(v, int(k)))))
    for name in ("q", "xk", "sj", "l", "u", "delta"):
        kw[name] = sh(kw[name])
    e = lam_shift(problem.h, k)
    lam = problem.lam
    kw["lam"] = np.ldexp(lam, e) if np.ndim(lam) else type(lam)(np.ldexp(lam, e))
    kw["k"] = int(k)
    for name in ("l", "u", "delta", "lam"):
        if kw[name] is not None and not np.ndim(kw[name]):
            kw[name] = float(kw[name]) if not problem.f32 else np.float32(kw[name])
    return Problem(**kw)


def unscale(y, k):
    """2^-k y, exactly"""
    return np.ldexp(y, -int(k))


# ---------------------------------------------------------------------------------------------- the range condition
def assert_in_range(problem, k):
    """The condition under which the scaled problem is in scope, checked on the UNSCALED problem and k in log2 (nothing
    overflows here): with c = 2^k, V = the largest magnitude among q, xk, sj, the bounds, Delta / sqrt(n) (a radius is squared
    once, not summed) and the two sums the operators form first, xk + sj and (q + xk) + sj,
        n * V^2 * c^2 < 1e307          every sum of squares and of products q * y (|y| <= 2 V, a prox result being a difference
                                       of two such values: the factor 4 lies inside the headroom up to DBL_MAX = 1.8e308);
        lambda_max * n * V^(2 - p) * c^2 < 1e307          psi = lambda * (n terms |v|^(2 - p)), p = LAM_POW; the group operators:
                                       lambda_max * ngroups * sqrt(largest group) * V * c^2, the sum of lambda_g ||v_g||;
        m^2 * c^2 >= 2.3e-308          m = the smallest NONZERO magnitude among q, xk, sj, xk + sj, (q + xk) + sj and, for
                                       ShiftedGroupNormL2Binf, | |xk| - Delta | (its active terms are (xk +- Delta)^2).
    Float32 problems: the Float32 operators form no square and no sum in Float32 (the group norm and psi(y) square and add in
    Float64), so the Float32 condition is on the values themselves -- V c < 1e38, lambda c_lambda < 1e38, m c >= 1.2e-38 -- and the
    three lines above hold for the Float64 sums.  ValueError otherwise: the inputs are a mistake in the test."""
    assert problem.k == 0
    big, small = MAX_SUM, MIN_SQUARE
    t = problem.q.dtype.type
    xs = (problem.xk + problem.sj).astype(t)
    S = ((problem.q + problem.xk).astype(t) + problem.sj).astype(t)
    data = [problem.q, problem.xk, problem.sj, xs, S]
    V = max(float(np.max(np.abs(a))) if a.size else 0.0 for a in data)
    for name in ("l", "u"):
        v = getattr(problem, name)
        if v is not None:
            V = max(V, float(np.max(np.abs(v))))
    if problem.delta is not None:      # a radius is squared once, not summed
        V = max(V, float(problem.delta) / math.sqrt(max(problem.n, 1)))
    if problem.op == "prox_group_l2_binf":     # an active term of the Binf root find is (X +- Delta)^2: | |X| - Delta | is squared too
        data = data + [(np.abs(problem.xk) - t(problem.delta)).astype(t)]
    nz = [np.abs(a[a != 0]) for a in data]
    m = min((float(np.min(a)) for a in nz if a.size), default=1.0)
    n = max(problem.n, 1)
    lam = float(np.max(np.abs(problem.lam))) if np.size(problem.lam) else 0.0
    lg = math.log2
    if problem.f32:
        if V > 0 and lg(V) + k >= lg(MAX_SUM32):
            raise ValueError("scale 2^%d: max |v| * c overflows the Float32 range condition" % k)
        if lam > 0 and lg(lam) + lam_shift(problem.h, k) >= lg(MAX_SUM32):
            raise ValueError("scale 2^%d: lambda overflows the Float32 range condition" % k)
        if lg(m) + k < lg(MIN_SQUARE32):
            raise ValueError("scale 2^%d: the smallest nonzero magnitude %.3g * c is not a normal Float32" % (k, m))
    if V > 0 and lg(n) + 2 * (lg(V) + k) >= lg(big):
        raise ValueError("scale 2^%d: n * max v^2 * c^2 = 2^%.1f overflows the range condition" % (k, lg(n) + 2 * (lg(V) + k)))
    p = LAM_POW[problem.h]       # psi <= lambda * n terms of size V^(2 - p), at scale c_lambda * c^(2 - p) = c^2
    terms = float(n)
    if problem.h == "group":     # (one term per group, a norm of at most sqrt(size) V)
        sizes = np.diff(problem.csr())
        terms = len(sizes) * math.sqrt(max(int(sizes.max()), 1))
    if V > 0 and lam > 0 and lg(lam) + lg(terms) + (2 - p) * lg(V) + 2 * k >= lg(big):
        raise ValueError("scale 2^%d: lambda * ||.|| overflows the range condition" % k)
    if 2 * (lg(m) + k) < lg(small):
        raise ValueError("scale 2^%d: the smallest nonzero square (%.3g)^2 * c^2 = 2^%.1f is not a normal number" % (k, m, 2 * (lg(m) + k)))
    return True


# ---------------------------------------------------------------------------------------------- data
def _floor(a):
    """every nonzero magnitude below 2^-10 raised to +-2^-10"""
    tiny = (a != 0) & (np.abs(a) < FLOOR)
    a[tiny] = np.copysign(a.dtype.type(FLOOR), a[tiny])
    return a


def draw(n, seed, dtype=np.float64, zeros_in_q=True, zero_block=0, lattice=False, delta=None):
    """x, sj, q: N(0, 1), 0.3 N(0, 1), N(0, 1) in that order from default_rng(seed) (lattice: rounded to eighths), floored at 2^-10
    together with xk + sj and (q + xk) + sj (and | |x| - delta |, where a radius is given: the Binf groups square it);
    q[3::97] = 0 (zeros_in_q); the first zero_block elements of all three exactly 0."""
    rng = np.random.default_rng(seed)
    x, sj, q = rng.normal(size=n), 0.3 * rng.normal(size=n), rng.normal(size=n)
    if lattice:
        x, sj, q = (np.round(v * 8) / 8 for v in (x, sj, q))
    x, sj, q = (_floor(v.astype(dtype)) for v in (x, sj, q))
    if zeros_in_q:
        q[3::97] = 0
    step = dtype(4 * FLOOR)
    for _ in range(8):      # move sj (then q) where a sum the operators square is nonzero and below the floor
        if delta is not None:
            gap = np.abs(x) - dtype(delta)
            near = (gap != 0) & (np.abs(gap) < FLOOR)
            x[near] += np.copysign(step, x[near])
        xs = (x + sj).astype(dtype)
        bad = (xs != 0) & (np.abs(xs) < FLOOR)
        sj[bad] += step
        S = ((q + x).astype(dtype) + sj).astype(dtype)
        bad2 = (S != 0) & (np.abs(S) < FLOOR) & (q != 0)
        q[bad2] += step
        bad3 = (S != 0) & (np.abs(S) < FLOOR) & (q == 0)
        x[bad3] += step
        if not (bad.any() or bad2.any() or bad3.any()):
            break
    if zero_block:
        x[:zero_block] = 0; sj[:zero_block] = 0; q[:zero_block] = 0
    return x, sj, q


LAM, SIGMA = 0.7, 1.1
LS, US = -0.9, 0.9


def separable(op, n, seed=None, vec_bounds=False, masked=False, dtype=np.float64):
    """prox_* / iprox_* of NormL1, NormL0, RootNormLhalf and their boxes.  Bounds: the scalars -0.9, 0.9, or vectors in
    [-1.1, -1] and [1, 1.1]; mask: a selected third.  d of iprox!: U(0.5, 2), for the Box forms 15 % exactly 0 and 15 % negative."""
    seed = 52000 + n if seed is None else seed
    x, sj, q = draw(n, seed, dtype)
    rng = np.random.default_rng(seed + 1)
    kw = dict(op=op, q=q, xk=x, sj=sj, lam=dtype(LAM) if dtype is np.float32 else LAM, sigma=SIGMA)
    if op.startswith("iprox"):
        d = rng.uniform(0.5, 2.0, size=n)
        if op.endswith("_box"):
            r = rng.random(n)
            d = np.where(r < 0.15, 0.0, np.where(r < 0.30, -d, d))
        kw["d"] = d.astype(dtype)
    if op.endswith("_box"):
        lo, up = (-1.0 - 0.1 * rng.random(n)).astype(dtype), (1.0 + 0.1 * rng.random(n)).astype(dtype)
        kw["l"], kw["u"] = (lo, up) if vec_bounds else (dtype(LS) if dtype is np.float32 else LS, dtype(US) if dtype is np.float32 else US)
        if masked:
            m = np.zeros(n, dtype=np.uint8)
            m[rng.choice(n, size=max(1, n // 3), replace=False)] = 1
            kw["mask"] = m
    return Problem(**kw)


def groups(gs, ng, binf, seed=None, dtype=np.float64, offsets=None):
    """ng uniform groups of gs (or the CSR offsets given): lambda_g = ||S_g|| * {0.3, 0.8, 1.5} / sigma (zeroed and kept groups
    both occur; 1 for the all-zero group 0), sigma = 0.9, Delta = 0.8 (binf)."""
    n = gs * ng if offsets is None else int(offsets[-1])
    seed = 53000 + 7 * gs + ng + (1 if binf else 0) if seed is None else seed
    off = np.arange(0, n + 1, gs, dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    first = int(off[1] - off[0]) if len(off) > 2 else 0
    x, sj, q = draw(n, seed, dtype, zero_block=first, delta=0.8 if binf else None)
    rng = np.random.default_rng(seed + 1)
    S = ((q + x) + sj).astype(np.float64)
    nS = np.array([math.sqrt(float(np.sum(S[a:b] ** 2))) for a, b in zip(off[:-1], off[1:])])
    lam = (np.where(nS > 0, nS, 1.0) * rng.choice([0.3, 0.8, 1.5], size=len(nS)) / 0.9).astype(dtype)
    return Problem(op="prox_group_l2_binf" if binf else "prox_group_l2", q=q, xk=x, sj=sj, lam=lam, sigma=0.9,
                   delta=0.8 if binf else None, gsize=gs if offsets is None else 0, offsets=None if offsets is None else off)


def binf_regime():
    """The problem on which the reference's absolute epsilon = 1 (src/shiftedGroupNormL2Binf.jl:81,97) shows: 40 groups of 8 over
    N(0, 1) data from default_rng(1), drawn in the order x, 0.3 * sj, q, then lambda ~ U(0.2, 2); sigma = 0.9, Delta = 0.8.  At
    k <= -10 the bracket [lmin, lmax(ansatz = lmin + 1)] no longer encloses the root of one group, `fl * fm > 0` (:102) fires and
    the reference writes zeros there; at k = 0 it solves that group."""
    rng = np.random.default_rng(1)
    n = 320
    x, sj, q = rng.normal(size=n), 0.3 * rng.normal(size=n), rng.normal(size=n)
    lam = rng.uniform(0.2, 2.0, size=40)
    x, sj, q = (_floor(v) for v in (x, sj, q))
    return Problem(op="prox_group_l2_binf", q=q, xk=x, sj=sj, lam=lam, sigma=0.9, delta=0.8, gsize=8)


def topr(n, binf, lattice=False, seed=None, dtype=np.float64):
    seed = 54000 + n + (1 if lattice else 0) if seed is None else seed
    x, sj, q = draw(n, seed, dtype, lattice=lattice)
    return Problem(op="prox_indball_l0_binf" if binf else "prox_indball_l0", q=q, xk=x, sj=sj, lam=0.0, r=n // 3,
                   delta=(dtype(0.8) if dtype is np.float32 else 0.8) if binf else None)


def b2(n, active, seed=None):
    """ShiftedNormL1B2: Delta = 1 (the trust region is active: ||xk|| ~ sqrt(n)) or 512 (inactive up to n = 1e5; Delta^2 is
    formed, so 512 * 2^500 is about as far as a radius goes)"""
    seed = 55000 + n if seed is None else seed
    x, sj, q = draw(n, seed)
    return Problem(op="prox_l1_b2", q=q, xk=x, sj=sj, lam=1.0, sigma=1.0, delta=1.0 if active else 512.0, chi=1.0)


# ---------------------------------------------------------------------------------------------- the oracle on a problem
def oracle_y(orc, P):
    """the oracle's prox! / iprox! of the problem as it stands (Float64 or Float32 by the dtype of q)"""
    op = P.op
    with np.errstate(all="ignore"):
        if P.f32:
            if op in ("prox_l1", "prox_l0", "prox_l1_box", "prox_l0_box"):
                return orc.prox_f32(op[5:], P.q, P.xk, P.sj, P.lam, np.float32(P.sigma), P.l, P.u, mask=P.mask)
            if op in ("iprox_l1", "iprox_l0"):
                y, bad = orc.iprox_f32(op[6:], P.q, P.d, P.xk, P.sj, P.lam)
                assert bad < 0
                return y
            if op in ("iprox_l1_box", "iprox_l0_box"):
                return orc.iprox_f32(op[6:], P.q, P.d, P.xk, P.sj, P.lam, P.l, P.u, mask=P.mask)
            if op in ("prox_indball_l0", "prox_indball_l0_binf"):
                return orc.prox_indball_l0_f32(P.q, P.xk, P.sj, P.r, delta=P.delta)
            if op == "prox_group_l2":
                return orc.prox_group_l2_f32(P.q, P.xk, P.sj, P.lam, P.sigma, offsets=P.offsets, gsize=P.gsize)
            raise KeyError(op)
        if op in ("prox_l1", "prox_l0", "prox_lhalf"):
            return getattr(orc, op)(P.q, P.xk, P.sj, P.lam, P.sigma)
        if op in ("prox_l1_box", "prox_l0_box", "prox_lhalf_box"):
            return getattr(orc, op)(P.q, P.xk, P.sj, P.lam, P.sigma, P.l, P.u, mask=P.mask)
        if op in ("iprox_l1", "iprox_l0"):
            return getattr(orc, op)(P.q, P.d, P.xk, P.sj, P.lam)
        if op in ("iprox_l1_box", "iprox_l0_box"):
            return getattr(orc, op)(P.q, P.d, P.xk, P.sj, P.lam, P.l, P.u, mask=P.mask)
        if op == "prox_group_l2":
            return orc.prox_group_l2(P.q, P.xk, P.sj, P.lam, P.sigma, offsets=P.offsets, gsize=P.gsize)
        if op == "prox_group_l2_binf":
            return orc.prox_group_l2_binf(P.q, P.xk, P.sj, P.lam, P.sigma, P.delta, offsets=P.offsets, gsize=P.gsize)
        if op == "prox_indball_l0":
            return orc.prox_indball_l0(P.q, P.xk, P.sj, P.r)
        if op == "prox_indball_l0_binf":
            return orc.prox_indball_l0_binf(P.q, P.xk, P.sj, P.r, P.delta)
        if op == "prox_l1_b2":
            return orc.prox_l1_b2(P.q, P.xk, P.sj, P.lam, P.sigma, P.delta, P.chi)
    raise KeyError(op)


def oracle_h(orc, P, y):
    """h((xk + sj) + y) of the problem as it stands, over the selected indices: the h part of the oracle's objective, which is what
    the fused calls return.  (The Box forms: obj_plain over the selected indices, not obj_box -- at scale 2^500 one rounding of
    sj + y at a bound is far outside the absolute sqrt(eps) slack of the reference's feasibility scan, which the fused calls do
    not make.)"""
    if P.h in ("l1", "l0", "lhalf"):
        if P.mask is not None:
            sel = P.mask != 0
            return orc.obj_plain(P.h, y[sel], P.xk[sel], P.sj[sel], P.lam)
        return orc.obj_plain(P.h, y, P.xk, P.sj, P.lam)
    if P.h == "group":
        return orc.obj_group_l2(y, P.xk, P.sj, P.lam, offsets=P.offsets, gsize=P.gsize)
    if P.h == "b2":
        return orc.obj_plain("l1", y, P.xk, P.sj, P.lam)
    raise KeyError(P.h)


def ulps(a, b):
    """the largest distance between a and b in units of the spacing of b (0 where both are 0 or both NaN)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.abs(a)))
    d = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, d)
    return float(np.max(d)) if d.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------- planted points of psi(y)
def b2_flip_point():
    """(y, xk, sj, lambda, Delta) with ||sj + y|| = 1.5 Delta: outside the ball at k = 0 (1.5 > 1 + sqrt(eps)), and inside it at
    k = -500, where | ||sj + y|| - Delta | = 2^-501 <= the ABSOLUTE atol = eps of IndBallL2 (oracle/spx_oracle.c, orc_obj_l1_b2)"""
    n = 64
    x, sj, q = draw(n, 56001)
    y = -sj.copy()
    y[5] += 1.5           # sj + y = 1.5 e_5 up to one rounding
    return y, x, sj, 1.0, 1.0


def box_slack_point(n=33):
    """(y, xk, sj, l, u) with sj + y inside [l, u] except one index, 1e-9 above u = 0.9: at scale c it is outside by 1e-9 c,
    inside the reference's ABSOLUTE slack sqrt(eps) = 1.49e-8 at k = -40 and outside it at k = +40"""
    x, sj, q = draw(n, 56002)
    t = np.clip(q, -0.5, 0.5)
    t[7] = 0.9 + 1e-9
    y = t - sj
    return y, x, sj, LS, US


# ---------------------------------------------------------------------------------------------- the CPU table
CPU_CASES = {
    "prox_l1": lambda: separable("prox_l1", 1001), "prox_l0": lambda: separable("prox_l0", 1001),
    "prox_lhalf": lambda: separable("prox_lhalf", 1001),
    "prox_l1_box": lambda: separable("prox_l1_box", 1001, vec_bounds=True, masked=True),
    "prox_l0_box": lambda: separable("prox_l0_box", 1001, vec_bounds=True, masked=True),
    "prox_lhalf_box": lambda: separable("prox_lhalf_box", 1001, vec_bounds=True, masked=True),
    "iprox_l1": lambda: separable("iprox_l1", 1001), "iprox_l0": lambda: separable("iprox_l0", 1001),
    "iprox_l1_box": lambda: separable("iprox_l1_box", 1001, vec_bounds=True, masked=True),
    "iprox_l0_box": lambda: separable("iprox_l0_box", 1001, vec_bounds=True, masked=True),
    "prox_group_l2": lambda: groups(8, 40, False), "prox_group_l2_128": lambda: groups(128, 40, False),
    "prox_group_l2_binf_128": lambda: groups(128, 40, True),
    "prox_indball_l0": lambda: topr(1001, False), "prox_indball_l0_binf": lambda: topr(1001, True),
    "prox_l1_b2": lambda: b2(1001, True), "prox_l1_b2_inactive": lambda: b2(1001, False),
}
CPU_CASES_F32 = {
    "prox_l1": lambda: separable("prox_l1", 1001, dtype=np.float32), "prox_l0": lambda: separable("prox_l0", 1001, dtype=np.float32),
    "prox_l1_box": lambda: separable("prox_l1_box", 1001, vec_bounds=True, masked=True, dtype=np.float32),
    "prox_l0_box": lambda: separable("prox_l0_box", 1001, vec_bounds=True, masked=True, dtype=np.float32),
    "iprox_l1": lambda: separable("iprox_l1", 1001, dtype=np.float32), "iprox_l0": lambda: separable("iprox_l0", 1001, dtype=np.float32),
    "iprox_l1_box": lambda: separable("iprox_l1_box", 1001, vec_bounds=True, masked=True, dtype=np.float32),
    "iprox_l0_box": lambda: separable("iprox_l0_box", 1001, vec_bounds=True, masked=True, dtype=np.float32),
    "prox_indball_l0": lambda: topr(1001, False, dtype=np.float32), "prox_indball_l0_binf": lambda: topr(1001, True, dtype=np.float32),
    "prox_group_l2": lambda: groups(5, 40, False, dtype=np.float32),
}
ALL_K64 = tuple(sorted(set(K64 + K64_LARGE)))


def equivariance(orc, P, k):
    """max ulps between the oracle on the problem at 2^k and 2^k times the oracle on the unscaled problem (0.0: the same bits)"""
    assert_in_range(P, k)
    y0 = oracle_y(orc, P)
    yk = oracle_y(orc, scaled(P, k))
    return 0.0 if same_bits(unscale(yk, k), y0) else max(ulps(unscale(yk, k).astype(np.float64), y0.astype(np.float64)), 2.0 ** -60)


def obj_equivariance(orc, P, k):
    """the same for obj_plain("l1") at the oracle's own prox: psi scales by c * c_lambda = c^2"""
    y0 = oracle_y(orc, P)
    Pk = scaled(P, k)
    a = orc.obj_plain("l1", y0, P.xk, P.sj, P.lam)
    b = orc.obj_plain("l1", np.ldexp(y0, k), Pk.xk, Pk.sj, Pk.lam)
    return 0.0 if math.ldexp(b, -2 * k) == a else max(ulps(math.ldexp(b, -2 * k), a), 2.0 ** -60)


def binf_zeroed(orc, P, k):
    """the groups the oracle zeroes at scale 2^k (y == -(xk + sj) exactly on them), and y / 2^k"""
    import arbiter
    Pk = scaled(P, k) if k else P
    y = oracle_y(orc, Pk)
    return arbiter.zero_pattern(y, Pk.xk, Pk.sj, P.csr()), unscale(y, k)


def cpu_table(orc):
    """the lines of the CPU part of profiles/scale_equivariance.txt"""
    out = ["# oracle(2^k P) against 2^k oracle(P): `bits` = the same bit pattern, else the largest distance in ulps",
           "# Float64, k = " + " ".join("%d" % k for k in ALL_K64)]
    fmt = lambda v: "bits" if v == 0.0 else ("%.3g" % v)
    for name, mk in CPU_CASES.items():
        P = mk()
        ks = [k for k in ALL_K64 if P.h != "lhalf" or k % 2 == 0]
        out.append("%-26s %s" % (name, " ".join("%5s" % fmt(equivariance(orc, P, k)) for k in ks)))
    out.append("%-26s %s" % ('obj_plain("l1")', " ".join("%5s" % fmt(obj_equivariance(orc, CPU_CASES["prox_l1"](), k)) for k in ALL_K64)))
    out.append("# Float32, k = " + " ".join("%d" % k for k in K32))
    for name, mk in CPU_CASES_F32.items():
        P = mk()
        out.append("%-26s %s" % (name + "_f32", " ".join("%5s" % fmt(equivariance(orc, P, k)) for k in K32)))
    P = binf_regime()
    z0, y0 = binf_zeroed(orc, P, 0)
    out.append("# prox_group_l2_binf, 40 groups of 8 (scales.binf_regime): groups zeroed by the oracle per k; the others against 2^k y(P)")
    for k in (-500, -200, -40, -10, -4, 0, 4, 10, 40, 200, 500):
        z, y = binf_zeroed(orc, P, k)
        keep = np.repeat(~(z & ~z0), 8)
        out.append("k = %5d: %2d zeroed (%d more than at k = 0: %s); other groups max |y / 2^k - y(P)| = %.3g" % (
            k, int(z.sum()), int((z & ~z0).sum()), np.flatnonzero(z & ~z0).tolist(), float(np.max(np.abs(y - y0)[keep]))))
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle
    oracle.build()
    print("\n".join(cpu_table(oracle)))
