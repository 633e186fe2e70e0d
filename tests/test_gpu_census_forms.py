"""GPU: the fused Box entry points on the (vector bounds, mask) combinations and skeletons no other test launches
(profiles/kernel_census.txt).

run_separable picks launch_vec<Op, VECB, MASK> from (l_vec || u_vec) and sel_mask != NULL.  The other fused test files call
the Box entry points with scalar bounds and no mask, and with two bound vectors plus a mask: (VECB, MASK) = (false, false) and
(true, true).  Here every fused Box entry point -- spx_proxval_{l1,l0,lhalf}_box, spx_proxstep_{l1,l0,lhalf}_box,
spx_iproxstep_{l1,l0}_box -- runs, through the C ABI on a private context, with

  vv        two bound vectors, every index selected          (true, false): what shifted(h, xk, l, u) builds by default
  ss+mask   scalar bounds and a selected third                (false, true)
  vs, sv    one bound a vector, the other a scalar (a NULL pointer into the VECB kernels), each with and without the mask
  ss, vv+mask  the two combinations of the other files, so that all four run on every skeleton for every operator

on the default skeleton (LDS-staged where the operator has one), on the register-staged one with non-temporal and with plain
accesses (key 3 = 0 with key 1 = 1 / 0) and with a capped grid (key 3 = 0, key 0 = 2), each with key 17 = 1 and 0.

Sizes.  T = elements per workgroup: 2 * 256 * U with U of launch_vec -- 3072 for the L1 / L0 prox forms with scalar bounds, 2048
for the NormL0Box iprox form, 1536 for both with a bound vector -- and 2 * 256 * 4 = 2048 for k_sep_vec (RootNormLhalfBox, the
NormL1Box iprox form and every key 3 = 0 call).  n runs over 1, 2, 3, T - 1, T, T + 1, 2 T + 1 for the T of the LDS-staged and of
the register-staged form, and 6144 (a whole number of tiles of every form: one launch covers the vector, so key 17 = 1 takes
the one-launch finish; so do the even T).  Every size runs with all vectors 16-byte aligned and with all of them 8 bytes off
(the mask one byte off), which peels element 0 into k_sep_scalar; the odd sizes end in k_sep_scalar too.

Bars (the project's own, tests/test_gpu_proxstep.py and tests/test_gpu_iproxstep.py): y bit for bit against the Float64 oracle
for L1 / L0, through arbiter.check_lhalf for RootNormLhalf, and bit for bit against the library's plain spx_prox_* / spx_iprox_*;
xkn the bits of (xk + sj) + y; [0] against the oracle's obj_box of that y, exactly for NormL0 and within 1e-12 otherwise; the
other sums within 1e-12 of the sum of |term| of math.fsum over ALL indices.

Further down: one case per remaining instantiation the census showed as never launched and reachable (the operators without a
box on the register-staged skeletons, the Float32 separable kernels, the register tiles of the group operators at the sizes of
every row, small ragged and index-set groups, the top-r front kernel with sixteen samples per lane), each against the oracle its
neighbours use; and default-run cases for the forms only `soak` cases reached, brought down to n = 3e5 / 2^17 by tuning key 8."""
import ctypes
import math

import numpy as np
import pytest

import arbiter
import redzone

pytestmark = pytest.mark.gpu

TOL = 1e-12
LAM, SIGMA = 0.7, 1.1
LS, US = -0.9, 0.9          # the scalar bounds (the vectors are drawn in [-1.1, -1] and [1, 1.1])
POISON = -777.25

# entry point -> (kind, family, elements per workgroup of the default skeleton with scalar bounds / with a bound vector)
ENTRIES = {
    "proxval_l1_box": ("l1", "val", 3072, 1536),
    "proxval_l0_box": ("l0", "val", 3072, 1536),
    "proxval_lhalf_box": ("lhalf", "val", 2048, 2048),
    "proxstep_l1_box": ("l1", "step", 3072, 1536),
    "proxstep_l0_box": ("l0", "step", 3072, 1536),
    "proxstep_lhalf_box": ("lhalf", "step", 2048, 2048),
    "iproxstep_l1_box": ("l1", "istep", 2048, 2048),
    "iproxstep_l0_box": ("l0", "istep", 2048, 1536),
}
# variant -> (l is a vector, u is a vector, mask)
VARIANTS = {
    "vv": (True, True, False),
    "ss+mask": (False, False, True),
    "vs": (True, False, False),
    "vs+mask": (True, False, True),
    "sv": (False, True, False),
    "sv+mask": (False, True, True),
    # the two the other files run on the default skeleton only (and on the others for three operators): all four (VECB, MASK)
    "ss": (False, False, False),
    "vv+mask": (True, True, True),
}
SKELETONS = [  # on top of the defaults key 0 = 0, key 1 = 1, key 3 = 1
    ("default", {}),
    ("vec-nt", {3: 0, 1: 1}),
    ("vec-plain", {3: 0, 1: 0}),
    ("vec-capped", {3: 0, 0: 2}),
]
DEFAULT_KEYS = {17: 1, 3: 1, 1: 1, 0: 0}


def _tile(entry, variant):
    lv, uv, _ = VARIANTS[variant]
    return ENTRIES[entry][3 if (lv or uv) else 2]


def _sizes(entry, variant):
    out = {1, 2, 3, 6144}
    for t in (_tile(entry, variant), 2048):
        out |= {t - 1, t, t + 1, 2 * t + 1}
    return sorted(out)


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def ctx(s):
    """a private context: the tuning keys set here never reach the context the other test files share"""
    L = s._lib.load()
    c = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create(0, ctypes.byref(c)))
    yield c
    for k, v in DEFAULT_KEYS.items():
        L.spx_ctx_set_tuning(c, k, v)
    L.spx_sync(c)
    L.spx_ctx_destroy(c)


_DRAWS = {}


def _draw(n, istep):
    """x, sj, q (g), d, l, u, mask of a selected third (drawn as _data of tests/test_gpu_proxstep.py draws it); d as in
    tests/test_gpu_iproxstep.py: 70 % U(0.5, 2), 15 % exactly 0, 15 % U(-2, -0.5).  Computed once per (n, family), never changed."""
    key = (n, istep)
    if key not in _DRAWS:
        rng = np.random.default_rng(31000 + n + (7 if istep else 0))
        x = rng.normal(size=n)
        sj = rng.uniform(-0.5, 0.5, size=n)
        q = rng.normal(size=n)
        d = rng.uniform(0.5, 2.0, size=n)
        r = rng.random(n)
        d = np.where(r < 0.15, 0.0, np.where(r < 0.30, -d, d))
        lo, up = -1.0 - 0.1 * rng.random(n), 1.0 + 0.1 * rng.random(n)
        selected = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
        mask = np.zeros(n, dtype=np.uint8)
        mask[selected] = 1
        for a in (x, sj, q, d, lo, up, mask):
            a.setflags(write=False)
        _DRAWS[key] = (x, sj, q, d, lo, up, mask)
    return _DRAWS[key]


def _fsum(a):
    return math.fsum(a.tolist())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class _Vectors:
    """the device vectors of one (n, alignment): inputs uploaded once, y and xkn poisoned before every call"""

    def __init__(self, host, misaligned):
        import torch
        x, sj, q, d, lo, up, mask = host
        self.n = len(x)

        def up64(a):
            t = torch.empty(self.n + 2, dtype=torch.float64, device="cuda:0")
            v = t[1:self.n + 1] if misaligned else t[:self.n]
            v.copy_(torch.tensor(a))
            assert v.data_ptr() % 16 == (8 if misaligned else 0)
            return v

        self.x, self.sj, self.q, self.d, self.lo, self.up = (up64(a) for a in (x, sj, q, d, lo, up))
        m = torch.empty(self.n + 2, dtype=torch.uint8, device="cuda:0")
        self.mask = m[1:self.n + 1] if misaligned else m[:self.n]
        self.mask.copy_(torch.tensor(mask))
        assert self.mask.data_ptr() % 2 == (1 if misaligned else 0)
        self.y, self.xkn = up64(np.full(self.n, POISON)), up64(np.full(self.n, POISON))

    def ptrs(self):
        return {k: getattr(self, k).data_ptr() for k in ("x", "sj", "q", "d", "lo", "up", "mask", "y", "xkn")}


def _bound_args(variant, p):
    """(l_vec, u_vec, l_scalar, u_scalar, sel_mask) of the C call; the scalar next to a vector is the one the kernel must use"""
    lv, uv, mk = VARIANTS[variant]
    return (p["lo"] if lv else None, p["up"] if uv else None, LS, US, p["mask"] if mk else None)


def _host_bounds(variant, host):
    x, sj, q, d, lo, up, mask = host
    lv, uv, mk = VARIANTS[variant]
    return (lo if lv else LS), (up if uv else US), (mask if mk else None)


def _call_fused(L, ctx, entry, variant, p, n, with_xkn=True):
    """-> the host statistics of the call (1, 3 or 4 doubles)"""
    kind, fam, _, _ = ENTRIES[entry]
    fn = getattr(L, "spx_" + entry)
    b = _bound_args(variant, p)
    if fam == "val":
        st = (ctypes.c_double * 1)()
        rc = fn(ctx, p["y"], p["q"], p["x"], p["sj"], n, LAM, SIGMA, *b, 1.0, st)
    elif fam == "step":
        st = (ctypes.c_double * 3)()
        rc = fn(ctx, p["y"], p["q"], p["x"], p["sj"], n, LAM, SIGMA, *b, 1.0, p["xkn"] if with_xkn else None, st, None)
    else:
        st = (ctypes.c_double * 4)()
        rc = fn(ctx, p["y"], p["q"], p["d"], p["x"], p["sj"], n, LAM, *b, p["xkn"] if with_xkn else None, st, None)
    assert rc == 0, (entry, variant, n, rc, L.spx_last_error())
    return list(st)


def _call_plain(L, ctx, entry, variant, p, n):
    kind, fam, _, _ = ENTRIES[entry]
    b = _bound_args(variant, p)
    if fam == "istep":
        rc = getattr(L, "spx_iprox_%s_box" % kind)(ctx, p["y"], p["q"], p["d"], p["x"], p["sj"], n, LAM, *b)
    else:
        rc = getattr(L, "spx_prox_%s_box" % kind)(ctx, p["y"], p["q"], p["x"], p["sj"], n, LAM, SIGMA, *b)
    assert rc == 0 and L.spx_sync(ctx) == 0, (entry, variant, n, rc, L.spx_last_error())


def _oracle_y(orc, entry, variant, host):
    x, sj, q, d, lo, up, mask = host
    kind, fam, _, _ = ENTRIES[entry]
    l, u, m = _host_bounds(variant, host)
    if fam == "istep":
        return getattr(orc, "iprox_%s_box" % kind)(q, d, x, sj, LAM, l, u, mask=m)
    return getattr(orc, "prox_%s_box" % kind)(q, x, sj, LAM, SIGMA, l, u, mask=m)


def _check_h(kind, h, exp, what):
    print("%s: h %.17g ref %.17g" % (what, h, exp))
    assert np.isfinite(exp), (what, exp)
    if kind == "l0":
        assert h == exp, (what, h, exp)
    else:
        assert abs(h - exp) <= TOL * max(abs(exp), 1e-300), (what, h, exp)


def _sum_terms(fam, host, y):
    """the terms of the sums behind [0], over ALL indices"""
    x, sj, q, d, lo, up, mask = host
    if fam == "val":
        return []
    if fam == "step":
        return [("qy", q * y), ("yy", y * y)]
    return [("gy", q * y), ("ydy", (d * y) * y), ("yy", y * y)]


def _check_sums(fam, host, y, st, what):
    for (name, t), got in zip(_sum_terms(fam, host, y), st[1:]):
        ref, mag = _fsum(t), _fsum(np.abs(t))
        print("%s: %s %.17g ref %.17g (bar %.3g)" % (what, name, got, ref, TOL * mag))
        assert abs(got - ref) <= TOL * mag, (what, name, got, ref, mag)


def _set_keys(L, ctx, keys):
    for k, v in keys.items():
        assert L.spx_ctx_set_tuning(ctx, k, v) == 0, (k, v)


def _reference(s, orc, L, ctx, entry, variant, host, V):
    """the plain library call against the oracle, once per (n, alignment): -> (y of the plain call, obj_box of it)"""
    import torch
    x, sj, q, d, lo, up, mask = host
    kind, fam, _, _ = ENTRIES[entry]
    n = V.n
    V.y.fill_(POISON)
    torch.cuda.synchronize()
    _call_plain(L, ctx, entry, variant, V.ptrs(), n)
    y_plain = V.y.cpu().numpy().copy()
    ref = _oracle_y(orc, entry, variant, host)
    l, u, m = _host_bounds(variant, host)
    if kind == "lhalf":
        arbiter.check_lhalf(orc, y_plain, ref, q, x, sj, LAM, SIGMA, box=(l, u), mask=m, what="%s %s n=%d" % (entry, variant, n))
    else:
        assert np.array_equal(_bits(y_plain), _bits(ref)), (entry, variant, n, "plain call against the oracle")
    return y_plain, orc.obj_box(kind, y_plain, x, sj, LAM, l, u, mask=m)


def _one_call(L, ctx, entry, variant, host, V, y_plain, h_exp, what):
    """one fused call: y, xkn, [0] and the other sums against the references; -> the statistics"""
    import torch
    x, sj, q, d, lo, up, mask = host
    kind, fam, _, _ = ENTRIES[entry]
    V.y.fill_(POISON)
    V.xkn.fill_(POISON)
    torch.cuda.synchronize()
    st = _call_fused(L, ctx, entry, variant, V.ptrs(), V.n)
    y = V.y.cpu().numpy()
    assert np.array_equal(_bits(y), _bits(y_plain)), (what, "y")
    if fam != "val":
        assert np.array_equal(_bits(V.xkn.cpu().numpy()), _bits((x + sj) + y_plain)), (what, "xkn")
    _check_h(kind, st[0], h_exp, what)
    _check_sums(fam, host, y_plain, st, what)
    return st


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_fused_box_forms(s, orc, ctx, entry, variant):
    import torch
    L = s._lib.load()
    kind, fam, _, _ = ENTRIES[entry]
    try:
        for n in _sizes(entry, variant):
            host = _draw(n, fam == "istep")
            for misaligned in (False, True):
                V = _Vectors(host, misaligned)
                _set_keys(L, ctx, DEFAULT_KEYS)
                y_plain, h_exp = _reference(s, orc, L, ctx, entry, variant, host, V)
                for name, keys in SKELETONS:
                    _set_keys(L, ctx, DEFAULT_KEYS)
                    _set_keys(L, ctx, keys)
                    V.y.fill_(POISON)                       # the plain call on this skeleton: the bits of the default one
                    torch.cuda.synchronize()
                    _call_plain(L, ctx, entry, variant, V.ptrs(), n)
                    assert np.array_equal(_bits(V.y.cpu().numpy()), _bits(y_plain)), (entry, variant, n, misaligned, name, "plain")
                    got = {}
                    for k17 in (1, 0):
                        _set_keys(L, ctx, {17: k17})
                        what = "%s %s n=%d mis=%s %s key17=%d" % (entry, variant, n, misaligned, name, k17)
                        got[k17] = [float(t).hex() for t in _one_call(L, ctx, entry, variant, host, V, y_plain, h_exp, what)]
                    # the one-launch finish adds the slots in the order of the separate reduction
                    assert got[0] == got[1], (entry, variant, n, misaligned, name, got)
    finally:
        _set_keys(L, ctx, DEFAULT_KEYS)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_scalar_box_with_a_mask_sums_over_the_right_index_sets(s, orc, ctx, entry):
    """scalar bounds + mask, (VECB, MASK) = (false, true): h runs over the SELECTED indices, the other sums over ALL of them.  The
    unselected elements carry y != 0 and a nonzero h term, so a sum over the wrong set is far outside the bars."""
    L = s._lib.load()
    kind, fam, t_scalar, _ = ENTRIES[entry]
    n = t_scalar + 1
    host = _draw(n, fam == "istep")
    x, sj, q, d, lo, up, mask = host
    sel = mask != 0
    try:
        for name, keys in SKELETONS:
            _set_keys(L, ctx, DEFAULT_KEYS)
            V = _Vectors(host, False)
            y_plain, h_sel = _reference(s, orc, L, ctx, entry, "ss+mask", host, V)
            _set_keys(L, ctx, keys)
            st = _one_call(L, ctx, entry, "ss+mask", host, V, y_plain, h_sel, "%s index sets %s" % (entry, name))
            assert np.count_nonzero(y_plain[~sel]) > n // 2          # the unselected elements do carry a step
            h_all = orc.obj_box(kind, y_plain, x, sj, LAM, LS, US)
            assert abs(st[0] - h_all) > 1e-3 * h_all, (entry, name, st[0], h_sel, h_all)
            for (nm, t), got in zip(_sum_terms(fam, host, y_plain), st[1:]):
                assert abs(got - _fsum(t[sel])) > 1e-3 * _fsum(np.abs(t)), (entry, name, nm, got)
    finally:
        _set_keys(L, ctx, DEFAULT_KEYS)


# ------------------------------------------------------------------ the operators without a box on every skeleton
# name -> (kind, family, y aliases q, elements per workgroup of the LDS-staged form)
UNBOXED = {
    "prox_l1": ("l1", "plain", False, 3072), "prox_l0": ("l0", "plain", False, 3072), "prox_lhalf": ("lhalf", "plain", False, 3072),
    "prox_l1-aliased": ("l1", "plain", True, 3072),
    "proxval_l1": ("l1", "val", False, 3072), "proxval_l0": ("l0", "val", False, 3072), "proxval_lhalf": ("lhalf", "val", False, 3072),
    "proxval_l1-aliased": ("l1", "val", True, 3072),
    "proxstep_l1": ("l1", "step", False, 3072), "proxstep_l0": ("l0", "step", False, 3072), "proxstep_lhalf": ("lhalf", "step", False, 3072),
    "iprox_l1": ("l1", "iplain", False, 2048), "iprox_l0": ("l0", "iplain", False, 2048),
    "iproxstep_l1": ("l1", "istep", False, 2048), "iproxstep_l0": ("l0", "istep", False, 2048),
}


def _call_unboxed(L, ctx, name, p, n):
    """-> the host statistics (none for the plain calls)"""
    kind, fam, aliased, _ = UNBOXED[name]
    fn = getattr(L, "spx_" + name.split("-")[0])
    y = p["q"] if aliased else p["y"]
    st = []
    if fam == "plain":
        rc = fn(ctx, y, p["q"], p["x"], p["sj"], n, LAM, SIGMA)
    elif fam == "val":
        st = (ctypes.c_double * 1)()
        rc = fn(ctx, y, p["q"], p["x"], p["sj"], n, LAM, SIGMA, 1.0, st)
    elif fam == "step":
        st = (ctypes.c_double * 3)()
        rc = fn(ctx, y, p["q"], p["x"], p["sj"], n, LAM, SIGMA, 1.0, p["xkn"], st, None)
    elif fam == "iplain":
        rc = fn(ctx, y, p["q"], p["d"], p["x"], p["sj"], n, LAM, 1)
    else:
        st = (ctypes.c_double * 4)()
        rc = fn(ctx, y, p["q"], p["d"], p["x"], p["sj"], n, LAM, 1, p["xkn"], st, None)
    assert rc == 0 and L.spx_sync(ctx) == 0, (name, n, rc, L.spx_last_error())
    return list(st)


@pytest.mark.parametrize("name", list(UNBOXED))
def test_unboxed_forms_on_every_skeleton(s, orc, ctx, name):
    """ShiftedNormL1 / NormL0 / RootNormLhalf without a box -- plain, fused with the value, with the step statistics, the iprox!
    forms, and NormL1 with y === q (the reference's two-pass body: y = -xk - sj) -- on the LDS-staged skeleton and on the
    register-staged one with non-temporal and with plain accesses, key 17 = 1 and 0, at the tile edges of both, both alignments.
    The other files run the register-staged forms of these operators for NormL1 with non-temporal accesses only."""
    import torch
    L = s._lib.load()
    kind, fam, aliased, t_lds = UNBOXED[name]
    ifam = fam in ("iplain", "istep")
    sums_fam = {"plain": "val", "iplain": "val"}.get(fam, fam)
    sizes = {1, 2, 3, 6144}
    for t in (t_lds, 2048):
        sizes |= {t - 1, t, t + 1, 2 * t + 1}
    try:
        for n in sorted(sizes):
            x, sj, q, d, lo, up, mask = _draw(n, ifam)
            d = np.abs(d) + (d == 0.0)             # d > 0: the unboxed iprox! asserts it
            host = (x, sj, q, d, lo, up, mask)
            if aliased:
                ref = (-x) - sj
            elif ifam:
                ref = getattr(orc, "iprox_" + kind)(q, d, x, sj, LAM)
            else:
                ref = getattr(orc, "prox_" + kind)(q, x, sj, LAM, SIGMA)
            h_exp = orc.obj_plain(kind, ref, x, sj, LAM)
            for misaligned in (False, True):
                V = _Vectors(host, misaligned)
                y_first = None
                for skel, keys in SKELETONS[:3]:
                    _set_keys(L, ctx, DEFAULT_KEYS)
                    _set_keys(L, ctx, keys)
                    got = {}
                    for k17 in (1, 0):
                        _set_keys(L, ctx, {17: k17})
                        what = "%s n=%d mis=%s %s key17=%d" % (name, n, misaligned, skel, k17)
                        V.y.fill_(POISON)
                        V.xkn.fill_(POISON)
                        V.q.copy_(torch.tensor(q))
                        torch.cuda.synchronize()
                        st = _call_unboxed(L, ctx, name, V.ptrs(), n)
                        y = (V.q if aliased else V.y).cpu().numpy()
                        if y_first is None:
                            if kind == "lhalf":
                                arbiter.check_lhalf(orc, y, ref, q, x, sj, LAM, SIGMA, what=what)
                                h_exp = orc.obj_plain(kind, y, x, sj, LAM)
                            else:
                                assert np.array_equal(_bits(y), _bits(ref)), (what, "y against the oracle")
                            y_first = y.copy()
                        assert np.array_equal(_bits(y), _bits(y_first)), (what, "y")
                        if fam in ("step", "istep"):
                            assert np.array_equal(_bits(V.xkn.cpu().numpy()), _bits((x + sj) + y_first)), (what, "xkn")
                        if st:
                            _check_h(kind, st[0], h_exp, what)
                            _check_sums(sums_fam, host, y_first, st, what)
                        got[k17] = [float(t).hex() for t in st]
                    assert got[0] == got[1], (name, n, misaligned, skel, got)
    finally:
        _set_keys(L, ctx, DEFAULT_KEYS)


@pytest.mark.parametrize("entry", ["proxstep_l1_box", "iproxstep_l0_box", "proxval_lhalf_box"])
def test_capped_grid_strides(s, orc, ctx, entry):
    """key 3 = 0, key 0 = 1: the grid of k_sep_vec is capped at one workgroup per CU, so at n = 2048 * (CUs + 3) + 2 workgroups
    0 .. 3 take a second tile in the grid-stride loop (at the sizes above a capped grid never strides).  Two bound vectors, no
    mask."""
    import torch
    L = s._lib.load()
    kind, fam, _, _ = ENTRIES[entry]
    n = 2048 * (torch.cuda.get_device_properties(0).multi_processor_count + 3) + 2
    host = _draw(n, fam == "istep")
    try:
        V = _Vectors(host, False)
        y_plain, h_exp = _reference(s, orc, L, ctx, entry, "vv", host, V)
        _set_keys(L, ctx, {3: 0, 0: 1})
        for k17 in (1, 0):
            _set_keys(L, ctx, {17: k17})
            _one_call(L, ctx, entry, "vv", host, V, y_plain, h_exp, "%s strided key17=%d" % (entry, k17))
    finally:
        _set_keys(L, ctx, DEFAULT_KEYS)


# ------------------------------------------------------------------ Float32 separable kernels
F32_BOX = ["prox_l1_box", "prox_l0_box", "iprox_l1_box", "iprox_l0_box"]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", F32_BOX)
def test_f32_box_forms(s, orc, ctx, name, variant):
    """The Float32 Box operators on all four (VECB, MASK) kernels of k_sep_f32 and, with y alone 4 bytes off, on k_sep_f32_scalar
    (run_f32: vectors of mixed alignment); a bound vector next to a scalar bound passes a NULL pointer.  One workgroup of
    k_sep_f32 covers 256 * kF32U groups of four floats: n = 1, 5, 4099 and 3 * 4096 + 2 give a head / tail only, one partial
    tile and several.  Bit for bit against the Float32 restatement of the reference (oracle.prox_f32 / iprox_f32)."""
    import torch
    L = s._lib.load()
    op = name.split("_", 1)[1]
    lv, uv, mk = VARIANTS[variant]
    f = np.float32
    for n in (1, 5, 4099, 3 * 4096 + 2):
        x, sj, q, d, lo, up, mask = _draw(n, True)
        x, sj, q, d, lo, up = (a.astype(f) for a in (x, sj, q, d, lo, up))
        l, u, m = (lo if lv else f(LS)), (up if uv else f(US)), (mask if mk else None)
        if name.startswith("iprox"):
            ref = orc.iprox_f32(op, q, d, x, sj, f(LAM), l, u, mask=m)
        else:
            ref = orc.prox_f32(op, q, x, sj, f(LAM), f(SIGMA), l, u, mask=m)
        dev = {k: torch.tensor(a).to("cuda:0") for k, a in (("x", x), ("sj", sj), ("q", q), ("d", d), ("lo", lo), ("up", up), ("mask", mask))}
        for y_off in (0, 1):                      # 1: y alone 4 bytes off -> the element-wise kernel
            ybuf = torch.full((n + 4,), POISON, dtype=torch.float32, device="cuda:0")
            y = ybuf[y_off:y_off + n]
            torch.cuda.synchronize()
            b = (dev["lo"].data_ptr() if lv else None, dev["up"].data_ptr() if uv else None, LS, US,
                 dev["mask"].data_ptr() if mk else None)
            fn = getattr(L, "spx_%s_f32" % name)
            if name.startswith("iprox"):
                rc = fn(ctx, y.data_ptr(), dev["q"].data_ptr(), dev["d"].data_ptr(), dev["x"].data_ptr(), dev["sj"].data_ptr(), n, LAM, *b)
            else:
                rc = fn(ctx, y.data_ptr(), dev["q"].data_ptr(), dev["x"].data_ptr(), dev["sj"].data_ptr(), n, LAM, SIGMA, *b)
            assert rc == 0 and L.spx_sync(ctx) == 0, (name, variant, n, rc, L.spx_last_error())
            got = ybuf.cpu().numpy()
            assert np.array_equal(got[y_off:y_off + n].view(np.int32), ref.view(np.int32)), (name, variant, n, y_off)
            assert (got[:y_off] == f(POISON)).all() and (got[y_off + n:] == f(POISON)).all(), (name, variant, n, y_off)


@pytest.mark.parametrize("name", ["prox_l1-aliased", "iprox_l1", "iprox_l0"])
def test_f32_unboxed_elementwise_kernel(s, orc, ctx, name):
    """k_sep_f32_scalar (vectors of mixed alignment: xk alone 4 bytes off) for Float32 NormL1 with y === q and the unboxed
    iprox! forms; bit for bit against the Float32 restatement."""
    import torch
    L = s._lib.load()
    f = np.float32
    for n in (1, 5, 4099):
        x, sj, q, d, lo, up, mask = _draw(n, True)
        x, sj, q, d = (a.astype(f) for a in (x, sj, q, d))
        d = np.abs(d) + (d == 0)
        xbuf = torch.zeros(n + 4, dtype=torch.float32, device="cuda:0")
        xd = xbuf[1:n + 1]
        xd.copy_(torch.tensor(x))
        sd, qd, dd = (torch.tensor(a).to("cuda:0") for a in (sj, q, d))
        ybuf = torch.full((n + 4,), POISON, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        if name == "prox_l1-aliased":
            ref = orc.prox_f32("l1", q, x, sj, f(LAM), f(SIGMA), aliased=True)
            rc = L.spx_prox_l1_f32(ctx, qd.data_ptr(), qd.data_ptr(), xd.data_ptr(), sd.data_ptr(), n, LAM, SIGMA)
            out = qd
        else:
            ref, bad = orc.iprox_f32(name.split("_")[1], q, d, x, sj, f(LAM))
            assert bad < 0
            rc = getattr(L, "spx_%s_f32" % name)(ctx, ybuf.data_ptr(), qd.data_ptr(), dd.data_ptr(), xd.data_ptr(), sd.data_ptr(), n, LAM, 1)
            out = ybuf[:n]
        assert rc == 0 and L.spx_sync(ctx) == 0, (name, n, rc, L.spx_last_error())
        assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32)), (name, n)
        assert bool((ybuf[n:] == POISON).all())


# ------------------------------------------------------------------ register tiles of the group operators
# k_group_reg<LPG, EPL, BINF, PAIRS, LIT, FULL, VALUE, STEP>: the row of the tile table by the group size (GroupTilesPlain /
# GroupTilesBinf / GroupTilesLit in spx_group.hip), PAIRS for even sizes in 16-byte aligned vectors, FULL when the size is
# LPG * EPL.  The sizes below are, per row the other files leave out, the full tile, an even size under it and an odd one.
GROUP_SIZES = {False: [4, 32, 33, 34, 64, 129, 130, 256, 384, 386], True: [4, 6, 10, 18, 32, 33, 34, 64, 129, 130, 256]}


@pytest.mark.parametrize("binf,gs", [(b, g) for b in (False, True) for g in GROUP_SIZES[b]],
                         ids=["%s-%d" % ("binf" if b else "plain", g) for b in (False, True) for g in GROUP_SIZES[b]])
def test_group_register_tiles(s, orc, ctx, binf, gs):
    """spx_prox_group_l2[_binf], spx_proxval_group_l2[_binf] and spx_proxstep_group_l2[_binf] on uniform groups of these sizes.
    The plain call against the oracle (arbiter.check_group, the bar of tests/test_gpu_redzone.py); the fused calls: y the bits
    of the plain call, xkn the bits of (xk + sj) + y, the value within 1e-12 of the oracle's on that y, <q, y> and <y, y> within
    1e-12 of the sum of |term| of math.fsum."""
    import torch
    import zlib
    L = s._lib.load()
    ng = 301
    n = gs * ng
    rng = np.random.default_rng(zlib.crc32(("tiles%d%d" % (binf, gs)).encode()))
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    nS = np.linalg.norm(((q + x) + sj).reshape(ng, gs), axis=1)
    sigma, delta = 0.9, 0.8
    lam = nS * rng.choice([0.3, 0.8, 1.5], size=ng) / sigma
    xd, sd, qd, ld = (torch.tensor(a).to("cuda:0") for a in (x, sj, q, lam))
    tail = (delta,) if binf else ()
    sfx = "_binf" if binf else ""

    def fresh():
        return torch.full((n,), POISON, dtype=torch.float64, device="cuda:0")

    def head(y):
        return (ctx, y.data_ptr(), qd.data_ptr(), xd.data_ptr(), sd.data_ptr(), n, None, gs, ng, ld.data_ptr(), sigma, *tail)

    y0 = fresh()
    torch.cuda.synchronize()
    assert getattr(L, "spx_prox_group_l2" + sfx)(*head(y0)) == 0 and L.spx_sync(ctx) == 0, L.spx_last_error()
    y_plain = y0.cpu().numpy()
    with np.errstate(all="ignore"):
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs) if binf else orc.prox_group_l2(q, x, sj, lam, sigma, gsize=gs)
    what = "group tiles %s gs=%d" % ("binf" if binf else "plain", gs)
    arbiter.check_group(orc, y_plain, ref, q, x, sj, lam, sigma, np.arange(0, n + 1, gs), delta=delta if binf else None, what=what)
    h_exp = orc.obj_group_l2(y_plain, x, sj, lam, gsize=gs)
    y1, val = fresh(), ctypes.c_double(-1.0)
    torch.cuda.synchronize()
    assert getattr(L, "spx_proxval_group_l2" + sfx)(*head(y1), 1.0, ctypes.byref(val)) == 0, L.spx_last_error()
    assert np.array_equal(_bits(y1.cpu().numpy()), _bits(y_plain)), what
    _check_h("l1", val.value, h_exp, what + " value")
    y2, xkn, st = fresh(), fresh(), (ctypes.c_double * 3)()
    torch.cuda.synchronize()
    assert getattr(L, "spx_proxstep_group_l2" + sfx)(*head(y2), 1.0, xkn.data_ptr(), st, None) == 0, L.spx_last_error()
    assert np.array_equal(_bits(y2.cpu().numpy()), _bits(y_plain)), what
    assert np.array_equal(_bits(xkn.cpu().numpy()), _bits((x + sj) + y_plain)), what
    _check_h("l1", st[0], h_exp, what + " step")
    _check_sums("step", (x, sj, q, None, None, None, None), y_plain, list(st), what)
    # psi(y) on the same layout (k_obj_group: lanes per group by the size, 16-byte pairs for even sizes): the oracle's value
    obj = ctypes.c_double(-1.0)
    assert getattr(L, "spx_obj_group_l2" + sfx)(ctx, y0.data_ptr(), xd.data_ptr(), sd.data_ptr(), n, None, gs, ng, ld.data_ptr(), *tail,
                                                ctypes.byref(obj)) == 0, L.spx_last_error()
    exp = orc.obj_group_l2(y_plain, x, sj, lam, gsize=gs, delta=delta if binf else None)
    assert obj.value == exp or abs(obj.value - exp) <= TOL * abs(exp), (what, "psi(y)", obj.value, exp)


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("top", [8, 30], ids=["avg4", "avg15"])
def test_ragged_groups_without_a_bound_small_averages(s, orc, ctx, binf, top):
    """CSR offsets with group_size = 0 (no bound: the general route) and an average of 4 / 15 elements per group:
    k_group_mem with 4 / 8 lanes per group (spx_group_lanes_by_avg; the other files' ragged layouts average 30: 16 lanes).
    Against the oracle through arbiter.check_group."""
    import torch
    L = s._lib.load()
    rng = np.random.default_rng(4100 + top + binf)
    ng = 700
    sizes = rng.integers(0, top + 1, size=ng)
    sizes[::97] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    S = (q + x) + sj
    nS = np.array([np.linalg.norm(S[a:b]) for a, b in zip(off[:-1], off[1:])])
    sigma, delta = 0.9, 0.8
    lam = np.where(nS > 0, nS, 1.0) * rng.choice([0.3, 0.8, 1.5], size=ng) / sigma
    xd, sd, qd, ld, od = (torch.tensor(a).to("cuda:0") for a in (x, sj, q, lam, off))
    y = torch.full((n,), POISON, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    tail = (delta,) if binf else ()
    fn = getattr(L, "spx_prox_group_l2" + ("_binf" if binf else ""))
    rc = fn(ctx, y.data_ptr(), qd.data_ptr(), xd.data_ptr(), sd.data_ptr(), n, od.data_ptr(), 0, ng, ld.data_ptr(), sigma, *tail)
    assert rc == 0 and L.spx_sync(ctx) == 0, L.spx_last_error()
    with np.errstate(all="ignore"):
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, offsets=off) if binf else orc.prox_group_l2(q, x, sj, lam, sigma, offsets=off)
    arbiter.check_group(orc, y.cpu().numpy(), ref, q, x, sj, lam, sigma, off, delta=delta if binf else None, what="ragged avg %d" % (top // 2))


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("gs", [4, 16], ids=["of4", "of16"])
def test_index_set_groups_small(s, orc, binf, gs):
    """groups given as index vectors of 4 / 16 strided indices: k_group_gather with 4 / 8 lanes per group (the other files'
    index sets average 67 entries and more).  The bar of test_group_gather_index_sets: 1e-12 of max(|y|, the group's norm)."""
    import torch
    rng = np.random.default_rng(4200 + gs + binf)
    ng = 500
    n = ng * gs + 7                                   # the last 7 indices are in no group
    groups = [list(range(k, ng * gs, ng)) for k in range(ng)]
    x, sj, q, y0 = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n), rng.normal(size=n)
    lam = rng.uniform(0.3, 1.5, size=ng)
    sigma, delta = 0.9, 0.8
    xd, sd, qd, yd = (torch.tensor(a).to("cuda:0") for a in (x, sj, q, y0))
    h = s.GroupNormL2(lam.tolist(), groups)
    psi = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd) if binf else s.shifted(s.shifted(h, xd), sd)
    assert psi._layout.index is not None
    ref = orc.prox_group_l2_idx(q, x, sj, lam, sigma, groups, delta=delta if binf else None, y0=y0)
    y = s.prox_bang(yd, psi, qd, sigma).cpu().numpy()
    S = (q + x) + sj
    scale = np.abs(ref).copy()
    for g in groups:
        scale[g] = np.maximum(scale[g], np.linalg.norm(S[g]))
    bad = np.abs(y - ref) > TOL * np.maximum(scale, 1e-300)
    assert not bad.any(), (int(bad.sum()), float(np.max(np.abs(y - ref))))
    assert np.array_equal(_bits(y[ng * gs:]), _bits(ref[ng * gs:]))          # untouched / shift-only entries are exact


def test_topr_front_kernel_sixteen_samples_per_lane(s, orc):
    """k_s2_front<16>: by default only for n >= 2^26 with the cut in the bulk of the vector (r (n - r) > 0.04 n^2); tuning key
    10 = 16 selects it wherever the sample-predicted pipeline runs, and key 11 = 0 lets the pipeline start at 2^21.  Lattice
    data (ties); y bit for bit against the reference's sortperm order (orc.TopR), cuts in the tail and in the bulk."""
    L, c = s._lib.load(), s.context("cuda:0")
    import torch
    n = (1 << 21) + 3001
    rng = np.random.default_rng(n)
    x, sj = np.round(rng.normal(size=n) * 16) / 16, np.round(rng.uniform(-0.5, 0.5, size=n) * 16) / 16
    q = np.round(rng.normal(size=n) * 16) / 16
    xd, sd, qd = (torch.tensor(a).to("cuda:0") for a in (x, sj, q))
    top = orc.TopR(q, x, sj)
    try:
        s._lib.check(L.spx_ctx_set_tuning(c, 11, 0))
        s._lib.check(L.spx_ctx_set_tuning(c, 10, 16))
        for r in (777, n // 3, n // 2):
            y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd, 0.8, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
            assert np.array_equal(_bits(y), _bits(top.prox(r, 0.8))), (n, r)
    finally:
        s._lib.check(L.spx_ctx_set_tuning(c, 10, 0))
        s._lib.check(L.spx_ctx_set_tuning(c, 11, 1))


# ------------------------------------------------------------------ forms the default run reached through soak cases only
def _key8(s, c, v):
    s._lib.check(s._lib.load().spx_ctx_set_tuning(c, 8, v))


def test_b2_on_demand_tiles_in_a_graph(s, orc):
    """The ShiftedNormL1B2 passes that take their tiles from an atomic counter, zeroed by a node of the graph (spx_b2.hip: the
    storing pass hands tiles out on demand when the grid has G > 1 workgroups and there are at least 8 G tiles of 6144
    elements).  On the native grid of 256 that needs n >= 1.26e7 -- test_iteration_in_a_graph_replays_on_new_data[15000000], a
    soak case; tuning key 8 = 4 caps the grid at four workgroups, and n = 300 001 is 49 tiles.  The iteration and the
    comparison are that case's: an active trust region within 1e-12 of the norms, then two calls with an inactive one (the
    speculative pass is wrong once and right once per replay), bit for bit."""
    import torch
    n = 300_001
    rng = np.random.default_rng(n)
    x = rng.normal(size=n); sj = rng.uniform(-0.5, 0.5, size=n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = s.context("cuda:0")
    try:
        with torch.cuda.stream(side):
            _key8(s, c, 4)
            xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(sj).cuda()
            qd = torch.zeros(n, dtype=torch.float64, device="cuda")
            ys = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]
            psi_b2 = s.shifted(s.shifted(s.NormL1(1.0), xd, 1.0, s.NormL2(1.0)), sd)
            psi_b2_in = s.shifted(s.shifted(s.NormL1(1.0), xd, 1e12, s.NormL2(1.0)), sd)

            def iteration():
                s.prox_bang(ys[0], psi_b2, qd, 1.0)
                s.prox_bang(ys[1], psi_b2_in, qd, 1.0)   # follows an active call: no speculation
                s.prox_bang(ys[2], psi_b2_in, qd, 1.0)   # follows an inactive call: the speculative pass is right
                # (and the next replay's first call follows an inactive one with an active trust region: speculation wrong)

            qd.copy_(torch.from_numpy(rng.normal(size=n)))
            iteration(); iteration()           # warm-up on the capture stream: the workspaces reach their sizes
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            iteration()

        def check(q, what):
            torch.cuda.synchronize()
            ref = orc.prox_l1_b2(q, x, sj, 1.0, 1.0, 1.0, 1.0)
            assert np.max(np.abs(ys[0].cpu().numpy() - ref)) <= 1e-12 * max(np.linalg.norm(ref), np.linalg.norm(x)), what
            ref = orc.prox_l1_b2(q, x, sj, 1.0, 1.0, 1e12, 1.0)
            assert np.array_equal(_bits(ys[1].cpu().numpy()), _bits(ref)) and np.array_equal(_bits(ys[2].cpu().numpy()), _bits(ref)), what

        for rep in range(3):
            q = rng.normal(size=n) * (1.0 + rep)
            qd.copy_(torch.from_numpy(q))
            for t in ys:
                t.fill_(-777.0)
            torch.cuda.synchronize()
            g.replay()
            check(q, "replay %d" % rep)
        q = rng.normal(size=n)
        qd.copy_(torch.from_numpy(q))
        with torch.cuda.stream(side):
            iteration(); iteration()
        check(q, "eager after replays")
        q = rng.normal(size=n) * 0.5
        qd.copy_(torch.from_numpy(q))
        torch.cuda.synchronize()
        g.replay()
        check(q, "replay after eager")
    finally:
        torch.cuda.synchronize()
        _key8(s, c, 0)


def test_team_on_demand_tiles_in_a_graph(s, orc):
    """One group over the vector, the team form with the tiles of its storing pass handed out on demand (spx_group_team.hip: a
    team of W > 1 workgroups and at least 8 W tiles of 6144 elements), captured and replayed on new data.  On the native grid
    that needs n of 1.3e7 or more; tuning key 8 = 4 caps the team at four workgroups, and n = 300 002 is 49 tiles, streamed
    (four workgroups hold 36 864 elements on chip).  The comparison of test_one_group_over_the_vector_in_a_graph."""
    import torch
    n = 300_002
    rng = np.random.default_rng(n + 1)
    x = rng.normal(size=n); sj = rng.uniform(-0.5, 0.5, size=n)
    lam = 0.4 * n ** 0.5
    off = np.array([0, n], dtype=np.int64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = s.context("cuda:0")
    try:
        with torch.cuda.stream(side):
            _key8(s, c, 4)
            xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(sj).cuda()
            qd = torch.zeros(n, dtype=torch.float64, device="cuda")
            ys = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2)]
            vals = [torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(2)]
            psi_g = s.shifted(s.shifted(s.NormL2(lam), xd), sd)
            psi_b = s.shifted(s.shifted(s.NormL2(lam), xd, 0.8, s.NormLinf(1.0)), sd)

            def iteration():
                s.prox_bang(ys[0], psi_g, qd, 0.9)
                with s.device_values(vals[0]):
                    psi_g(ys[0])
                s.prox_bang(ys[1], psi_b, qd, 0.9)
                with s.device_values(vals[1]):
                    psi_b(ys[1])

            qd.copy_(torch.from_numpy(rng.normal(size=n)))
            iteration(); iteration()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            iteration()
        for rep in range(3):
            q = rng.normal(size=n) * (1.0 + rep)
            qd.copy_(torch.from_numpy(q))
            for t in ys:
                t.fill_(-777.0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            nS = np.linalg.norm((q + x) + sj)
            for k, delta in ((0, None), (1, 0.8)):
                ref = orc.prox_group_l2(q, x, sj, [lam], 0.9, offsets=off) if delta is None else orc.prox_group_l2_binf(q, x, sj, [lam], 0.9, delta, offsets=off)
                y = ys[k].cpu().numpy()
                scale = np.maximum(np.maximum(np.abs(ref), np.abs(x + sj)), nS)
                assert float(np.max(np.abs(y - ref) / scale)) <= 1e-12, (rep, k)
                vr = orc.obj_group_l2(y, x, sj, [lam], offsets=off, delta=delta)
                got = float(vals[k].item())
                assert got == vr or abs(got - vr) <= 1e-12 * abs(vr), (rep, k, got, vr)
    finally:
        torch.cuda.synchronize()
        _key8(s, c, 0)


@pytest.mark.parametrize("n", [(1 << 17) - 1, 1 << 17, (1 << 17) + 3])
def test_f32_topr_at_the_lds_form_boundary(s, orc, n):
    """Float32 top-r where the form that parks v in LDS (32 Ki elements per resident workgroup) hands over to the one that parks
    it in y: 2^23 on 256 CUs -- test_f32_topr_bit_exact[8388607 / 8388608 / 8388611], soak cases; with tuning key 8 = 4 four
    workgroups are resident and the boundary is 2^17 (the register form ends at 2^15).  The cases and the comparison of
    test_f32_topr_bit_exact."""
    from test_gpu_f32 import _f32_topr_cases
    c = s.context("cuda:0")
    try:
        _key8(s, c, 4)
        _f32_topr_cases(s, orc, n)
    finally:
        _key8(s, c, 0)


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_fused_box_forms_guard_bands(s, orc, ctx, entry, variant, mode):
    """n = T + 1 on guarded buffers: y and xkn are outputs (every element written, nothing outside them), the inputs are
    guarded against writes, and a read past their end meets the poison, which moves y or a sum.  Mode B: every vector 8 bytes
    off and the mask at offset 1."""
    import torch
    L = s._lib.load()
    kind, fam, _, _ = ENTRIES[entry]
    n = _tile(entry, variant) + 1
    host = _draw(n, fam == "istep")
    x, sj, q, d, lo, up, mask = host
    lv, uv, mk = VARIANTS[variant]
    ay, ai = redzone.F64_MODES[mode]
    z = redzone.Zone()
    p = {"y": z.add(n, torch.float64, ay, role="out", name="y").ptr()}
    yb = z.bufs[0]
    kb = None
    if fam != "val":
        kb = z.add(n, torch.float64, ay, role="out", name="xkn")
        p["xkn"] = kb.ptr()
    for nm, a in (("q", q), ("x", x), ("sj", sj)):
        p[nm] = z.add(n, torch.float64, ai, data=np.array(a), name=nm).ptr()
    if fam == "istep":
        p["d"] = z.add(n, torch.float64, ai, data=np.array(d), name="d").ptr()
    if lv:
        p["lo"] = z.add(n, torch.float64, ai, data=np.array(lo), name="l").ptr()
    if uv:
        p["up"] = z.add(n, torch.float64, ai, data=np.array(up), name="u").ptr()
    if mk:
        p["mask"] = z.add(n, torch.uint8, 1 if mode == "B" else 0, data=np.array(mask), name="mask").ptr()
    _set_keys(L, ctx, DEFAULT_KEYS)
    torch.cuda.synchronize()
    st = _call_fused(L, ctx, entry, variant, p, n)
    z.check()
    ref = _oracle_y(orc, entry, variant, host)
    l, u, m = _host_bounds(variant, host)
    y = yb.t.cpu().numpy()
    what = "%s %s guard bands mode %s" % (entry, variant, mode)
    if kind == "lhalf":
        arbiter.check_lhalf(orc, y, ref, q, x, sj, LAM, SIGMA, box=(l, u), mask=m, what=what)
    else:
        assert np.array_equal(_bits(y), _bits(ref)), what
    if kb is not None:
        assert np.array_equal(_bits(kb.t.cpu().numpy()), _bits((x + sj) + y)), what
    _check_h(kind, st[0], orc.obj_box(kind, y, x, sj, LAM, l, u, mask=m), what)
    _check_sums(fam, host, y, st, what)
