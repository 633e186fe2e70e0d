"""spx_proxval_group_l2[_binf]: prox! of ShiftedGroupNormL2(Binf) fused with the value of h at the result (csrc/spx_group.hip,
include/spx.h "group forms").  y must carry the bits of the plain prox! on q_scale * q on every route; the value is the one
spx_obj_group_l2 forms on that y, up to summation order (both sides build identical v_i = (xk + sj) + y and add non-negative
terms: the project's psi bar, 1e-12 relative)."""
import ctypes
import zlib

import numpy as np
import pytest

import arbiter
import redzone

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
VALUE_TOL = 1e-12
SPX_ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _dev(a, align8=False):
    """device copy; align8: the vector starts 8 bytes past a 16-byte boundary (the 8-byte load forms)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not align8:
        d = t.to("cuda:0")
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(t)
    return buf[1:]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class Problem:
    """One layout with its data on the device, driven through the C ABI (so that CSR layouts with and without a size bound,
    and with a bound that one group exceeds, can all be stated)."""

    def __init__(self, s, layout, binf, align8=False, seed=0, all_zeroed=False):
        import torch
        self.s, self.L, self.ctx, self.binf = s, s._lib.load(), s.context("cuda:0"), binf
        kind, arg = layout
        rng = np.random.default_rng(zlib.crc32(("%s%s%d%d" % (kind, arg, binf, seed)).encode()))
        self.offsets = None
        if kind == "uniform":
            gs = arg
            ng = 301 if gs <= 128 else 61 if gs <= 1024 else 13
            n, self.gsize, sizes = gs * ng, gs, np.full(ng, gs)
        elif kind == "one":
            n, ng, self.gsize, sizes = arg, 1, arg, np.array([arg])
        else:  # CSR: "csr_bound" (bound = largest size), "csr_nobound" (hint 0), "csr_over" (one group above the bound)
            ng = 700
            sizes = rng.integers(0, 61, size=ng)
            sizes[::97] = 0                      # empty groups
            if kind == "csr_over":
                sizes[ng // 2] = 777
            head = 5                             # offsets need not span 0:n
            off = head + np.concatenate([[0], np.cumsum(sizes)])
            n = int(off[-1]) + 9
            self.offsets = off.astype(np.int64)
            self.gsize = {"csr_bound": int(sizes.max()), "csr_nobound": 0, "csr_over": 60}[kind]
        self.n, self.ng = n, ng
        # a third of the vector on a lattice (multiples of 1/4: activity boundaries, exact roots, exact zeros of the Binf
        # bracket -- the regime of test_group_binf_lattice_and_zero_x, the deferred list), xk = 0 on part of it; the rest continuous
        x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
        lat = n // 3
        x[:lat] = rng.integers(-8, 9, size=lat) / 4.0
        sj[:lat] = rng.integers(-2, 3, size=lat) / 4.0
        q[:lat] = rng.integers(-12, 13, size=lat) / 4.0
        x[: lat // 2] = 0.0
        if kind == "uniform":
            x[: self.gsize] = 0.0                # group 0: xk = 0 under a strong lambda (below) -- zeroed by both operators
        self.sigma, self.delta = 0.5, 1.0
        # lambda by group: sigma * lambda against ||S_g|| decides zeroed / active; both occur, plus a strong-lambda tail and zeros
        starts = self.offsets[:-1] if self.offsets is not None else np.arange(ng) * self.gsize
        S = (q + x) + sj
        nS = np.array([np.linalg.norm(S[a:a + m]) for a, m in zip(starts, sizes)])
        fac = rng.choice([0.0, 0.3, 0.7, 1.0, 1.5, 4.0, 40.0], size=ng)
        lam = np.where(nS > 0, nS, 1.0) * fac / self.sigma
        if kind != "one":
            lam[: ng // 3] = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0, 8.0], size=ng // 3)   # (the lattice part: lattice weights)
        else:
            lam[:] = 0.6 * nS / self.sigma
        if kind == "uniform":                    # ... and group 1 active
            lam[0], lam[1] = 40.0 * nS[0] / self.sigma, 0.3 * nS[1] / self.sigma
        if all_zeroed:
            lam[:] = 1e6 * (1.0 + nS)
            if binf:
                x[:] = 0.0
        self.x, self.sj, self.q, self.lam = x, sj, q, lam
        self.xd, self.sd, self.qd = _dev(x, align8), _dev(sj, align8), _dev(q, align8)
        self.ld = _dev(lam)
        self.od = _dev(self.offsets) if self.offsets is not None else None
        self.align8 = align8
        self.torch = torch

    def new_y(self, fill=-777.0):
        y = _dev(np.full(self.n, fill), self.align8)
        return y

    def _tail(self):
        return (_D(self.delta),) if self.binf else ()

    def prox(self, y, q=None):
        fn = getattr(self.L, "spx_prox_group_l2" + ("_binf" if self.binf else ""))
        self.s._lib.check(fn(self.ctx, _p(y), _p(self.qd if q is None else q), _p(self.xd), _p(self.sd), self.n, _p(self.od),
                             self.gsize, self.ng, _p(self.ld), _D(self.sigma), *self._tail()))
        return y

    def proxval(self, y, q=None, q_scale=1.0, rc_only=False, value=True):
        fn = getattr(self.L, "spx_proxval_group_l2" + ("_binf" if self.binf else ""))
        out = _D(-1.0)
        rc = fn(self.ctx, _p(y), _p(self.qd if q is None else q), _p(self.xd), _p(self.sd), self.n, _p(self.od), self.gsize, self.ng,
                _p(self.ld), _D(self.sigma), *self._tail(), _D(q_scale), ctypes.byref(out) if value else None)
        if rc_only:
            return rc
        self.s._lib.check(rc)
        return y, out.value

    def psi_plain(self, y):
        """shifted(shifted(h, xk), sj)(y) on the same layout: spx_obj_group_l2"""
        out = _D(-1.0)
        self.s._lib.check(self.L.spx_obj_group_l2(self.ctx, _p(y), _p(self.xd), _p(self.sd), self.n, _p(self.od), self.gsize, self.ng,
                                                  _p(self.ld), ctypes.byref(out)))
        return out.value


LAYOUTS = [("uniform", g) for g in (1, 2, 3, 8, 16, 17, 100, 128, 300, 512, 513, 1024, 5000)] + [
    ("csr_bound", 0), ("csr_nobound", 0), ("csr_over", 0), ("one", 1000), ("one", 1_000_003)]
_ids = ["%s%s" % (k, a or "") for k, a in LAYOUTS]


def _key9(s, v):
    s._lib.check(s._lib.load().spx_ctx_set_tuning(s.context("cuda:0"), 9, v))


def _close(a, b):
    return abs(a - b) <= VALUE_TOL * max(abs(b), 1e-300)


@pytest.mark.parametrize("align8", [False, True], ids=["a16", "a8"])
@pytest.mark.parametrize("binf,key9", [(False, 0), (True, 0), (True, 1)], ids=["plain", "binf", "binf-key9"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_y_bits_and_value(s, orc, layout, binf, key9, align8):
    """Items 1 and 2: y has the bits of the plain prox! on every route; the value is psi_plain(y) = spx_obj_group_l2 on that y,
    and the oracle's on the host copy of that y, to 1e-12 relative."""
    import torch
    P = Problem(s, layout, binf, align8)
    try:
        _key9(s, key9)
        y1 = P.prox(P.new_y())
        y2, val = P.proxval(P.new_y())
        assert torch.equal(y1, y2), (layout, binf, key9, align8)
        want = P.psi_plain(y2)
    finally:
        _key9(s, 0)
    yh = y2.cpu().numpy()
    ref = orc.obj_group_l2(yh, P.x, P.sj, P.lam, offsets=P.offsets, gsize=P.gsize if P.offsets is None else 0)
    print("layout %s binf %d key9 %d align8 %d: value %.17g psi_plain %.17g oracle %.17g" % (layout, binf, key9, align8, val, want, ref))
    assert np.isfinite(val) and want > 0.0
    # both kinds of groups occur: zeroed ones (v = 0 on the whole group) and active ones
    if layout[0] == "uniform":
        v = ((P.x + P.sj) + yh).reshape(P.ng, -1)
        dead = np.all(v == 0.0, axis=1)
        assert dead.any() and (~dead).any(), layout
    assert _close(val, want), (val, want)
    assert _close(val, ref), (val, ref)


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 16), ("uniform", 1024), ("csr_bound", 0)], ids=["u128", "u16", "u1024", "csr"])
def test_value_exactly_zero_when_every_group_is_zeroed(s, layout, binf):
    import torch
    P = Problem(s, layout, binf, all_zeroed=True)
    y, val = P.proxval(P.new_y(0.0))
    lo, hi = (0, P.n) if P.offsets is None else (int(P.offsets[0]), int(P.offsets[-1]))
    assert torch.equal(y[lo:hi], -(P.xd + P.sd)[lo:hi])      # every group zeroed: xk + sj + y = 0
    assert val == 0.0 and P.psi_plain(y) == 0.0, val


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 100), ("csr_bound", 0), ("csr_over", 0), ("uniform", 1024), ("one", 1000),
                                    ("csr_nobound", 0), ("uniform", 5000)],
                         ids=["fused-u128", "fused-u100", "fused-csr", "fused-csr-over", "composed-u1024", "composed-one", "composed-csr",
                              "composed-u5000"])
def test_q_scale(s, layout, binf):
    """Item 3: q_scale = c is bit-identical to scaling q beforehand (y) and gives exactly the same value; also with y aliasing q."""
    import torch
    P = Problem(s, layout, binf, seed=3)
    c = -0.37
    qc = P.qd * c                                   # one rounded multiply per element
    yB, vB = P.proxval(P.new_y(), q=qc)
    yA, vA = P.proxval(P.new_y(), q_scale=c)
    assert torch.equal(yA, yB) and vA == vB, (layout, binf, vA, vB)
    yP = P.prox(P.new_y(), q=qc)                    # ... and both are the plain operator at c * q
    assert torch.equal(yA, yP)
    q2 = _dev(P.q, False)
    q2, vC = P.proxval(q2, q=q2, q_scale=c)         # y is q itself
    lo, hi = (0, P.n) if P.offsets is None else (int(P.offsets[0]), int(P.offsets[-1]))   # (outside the groups y keeps what it held)
    assert torch.equal(q2[lo:hi], yB[lo:hi]) and vC == vB, (layout, binf, vC, vB)


@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 8), ("csr_over", 0), ("uniform", 1024)], ids=["u128", "u8", "csr-over", "u1024"])
def test_device_value_target_and_clean_state(s, layout):
    """Item 4: with a device value target the host value is NaN and the device double equals the synchronous value exactly;
    back-to-back calls, a call after another operator has written all over the library's scratch, and alternating Binf calls
    (both count words of the deferred list) give the same double."""
    import torch
    Ps = [Problem(s, layout, False, seed=4), Problem(s, layout, True, seed=4)]
    want = []
    for P in Ps:
        y0, v0 = P.proxval(P.new_y())
        want.append((y0, v0))
    n = Ps[0].n
    topr = s.shifted(s.shifted(s.IndBallL0(max(1, n // 7)), Ps[0].xd, 0.9, s.NormLinf(1.0)), Ps[0].sd)
    scratch_user = torch.empty_like(Ps[0].qd)
    out = torch.full((1,), -3.0, dtype=torch.float64, device="cuda:0")
    for rep in range(5):                             # Binf calls alternate between the two count words
        for P, (y0, v0) in zip(Ps, want):
            with s.device_values(out):
                y, hv = P.proxval(P.new_y())
            assert hv != hv, hv                       # NaN on the host: nothing was read back
            assert float(out.item()) == v0 and torch.equal(y, y0), (rep, P.binf, float(out.item()), v0)
            out.fill_(-3.0)
            if rep == 2:
                s.prox_bang(scratch_user, topr, Ps[0].qd, 1.0)   # writes all over spx_ctx::ws
            y, v = P.proxval(P.new_y())               # synchronous again, same double
            assert v == v0 and torch.equal(y, y0)
    P = Ps[1]
    for _ in range(3):                               # Binf back to back, nothing in between
        assert P.proxval(P.new_y())[1] == want[1][1]


@pytest.mark.parametrize("gs", [16])
def test_groups_on_the_deferred_list_are_counted(s, orc, gs):
    """The terms of the groups a Binf main launch hands to the launch behind it (tile masks, dterm).  With tuning key 9 = 1 the
    groups whose root sits next to the pole of step(n) (sigma * lambda ~ 30 ||S||, the data of
    test_group_binf_reference_faithful_mode) are evaluated literally -- by the launch over the deferred list and by nothing
    else -- so every group whose y differs between key 9 = 1 and key 9 = 0 was on the list.  Such groups must occur, must carry
    a share of the value far above the 1e-12 bar, and the value must still be psi_plain(y) and the oracle's.  (Groups of 16:
    on groups of 128 this data leaves no group whose y differs between the two modes, so nothing could be asserted there; the
    masks of the wider tiles are walked deterministically by test_group_above_the_size_bound_is_counted.)"""
    import torch
    rng = np.random.default_rng(909 + gs)
    ng = 20_000
    n = ng * gs
    P = Problem.__new__(Problem)
    P.s, P.L, P.ctx, P.binf = s, s._lib.load(), s.context("cuda:0"), True
    P.n, P.ng, P.gsize, P.offsets, P.od, P.align8 = n, ng, gs, None, None, False
    P.sigma, P.delta = 1.0, 1.0
    P.x, P.sj, P.q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    nS = np.linalg.norm(((P.q + P.x) + P.sj).reshape(ng, gs), axis=1)
    P.lam = rng.uniform(1.0, 40.0, size=ng) * nS                      # sigma * lambda up to 40 ||S_g||: roots next to the pole
    P.lam[::2] = rng.uniform(0.1, 0.5, size=(ng + 1) // 2)            # every other group plainly active
    P.xd, P.sd, P.qd, P.ld = _dev(P.x), _dev(P.sj), _dev(P.q), _dev(P.lam)
    y0 = P.prox(P.new_y())
    try:
        _key9(s, 1)
        y1 = P.prox(P.new_y())
        y2, val = P.proxval(P.new_y())
        y3, val3 = P.proxval(P.new_y())
        want = P.psi_plain(y2)
    finally:
        _key9(s, 0)
    assert torch.equal(y1, y2) and torch.equal(y2, y3) and val == val3
    listed = (y1 != y0).view(ng, gs).any(dim=1).cpu().numpy()
    yh = y2.cpu().numpy()
    terms = P.lam * np.linalg.norm(((P.x + P.sj) + yh).reshape(ng, gs), axis=1)
    share = float(terms[listed].sum() / terms.sum())
    ref = orc.obj_group_l2(yh, P.x, P.sj, P.lam, gsize=gs)
    print("gs %d: %d groups on the list, share of the value %.3e; value %.17g psi_plain %.17g oracle %.17g" % (
        gs, int(listed.sum()), share, val, want, ref))
    assert listed.sum() >= 10 and share > 1e-9, (int(listed.sum()), share)
    assert _close(val, want) and _close(val, ref), (val, want, ref)


def test_group_above_the_size_bound_is_counted(s, orc):
    """CSR offsets whose size bound one group exceeds: that group is handed to the list kernel by construction (777 elements
    against tiles of 64); it is active and carries a visible share of the value."""
    for binf in (False, True):
        P = Problem(s, ("csr_over", 0), binf, seed=7)
        g = P.ng // 2
        a, b = int(P.offsets[g]), int(P.offsets[g + 1])
        assert b - a == 777 and P.gsize == 60
        nS = np.linalg.norm(((P.q + P.x) + P.sj)[a:b])
        P.lam[g] = 0.3 * nS / P.sigma
        P.ld = _dev(P.lam)
        y, val = P.proxval(P.new_y())
        yh = y.cpu().numpy()
        term = P.lam[g] * np.linalg.norm(((P.x + P.sj) + yh)[a:b])
        ref = orc.obj_group_l2(yh, P.x, P.sj, P.lam, offsets=P.offsets, gsize=0)
        print("csr_over binf %d: term of the oversize group %.6g of %.17g (oracle %.17g)" % (binf, term, val, ref))
        assert term > 1e-6 * ref, (term, ref)
        assert _close(val, ref) and _close(val, P.psi_plain(y)), (val, ref)


def test_graph_replay(s):
    """Item 5: plain and Binf at 4096 x 128 captured with a device value target after one warm call; three replays give the
    eager y and value bit for bit.  (Default queue count; no graph environment variable is touched.)"""
    import torch
    rng = np.random.default_rng(11)
    ng, gs = 4096, 128
    n = ng * gs
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    x[: n // 4] = np.round(x[: n // 4] * 4) / 4
    sj[: n // 4] = np.round(sj[: n // 4] * 4) / 4
    q[: n // 4] = np.round(q[: n // 4] * 4) / 4
    x[: n // 8] = 0.0
    nS = np.linalg.norm(((q + x) + sj).reshape(ng, gs), axis=1)
    lam = nS * rng.choice([0.3, 0.7, 1.0, 1.5, 4.0], size=ng)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd, sd, qd = (torch.from_numpy(v).cuda() for v in (x, sj, q))
        h = s.GroupNormL2.uniform(torch.from_numpy(lam).cuda(), gs)
        psis = [s.shifted(s.shifted(h, xd), sd), s.shifted(s.shifted(h, xd, 1.0, s.NormLinf(1.0)), sd)]
        ys = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in psis]
        vals = [torch.zeros(1, dtype=torch.float64, device="cuda") for _ in psis]

        def iteration():
            for psi, y, v in zip(psis, ys, vals):
                with s.device_values(v):
                    s.prox_value_bang(y, psi, qd, 1.0, q_scale=-0.5)

        iteration()                                  # the warm call
        side.synchronize()
        eager = [(y.clone(), float(v.item())) for y, v in zip(ys, vals)]
        for y0, v0 in eager:
            assert np.isfinite(v0) and v0 > 0.0
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        iteration()
    for rep in range(3):
        for y, v in zip(ys, vals):
            y.fill_(-777.0)
            v.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for (y0, v0), y, v in zip(eager, ys, vals):
            assert torch.equal(y, y0) and float(v.item()) == v0, (rep, float(v.item()), v0)
    with torch.cuda.stream(side):                    # eager again on the context that has seen a capture
        iteration()
    side.synchronize()
    for (y0, v0), y, v in zip(eager, ys, vals):
        assert torch.equal(y, y0) and float(v.item()) == v0


def test_refusals(s):
    """Item 6: the mirror keeps its TypeError for Float32, host and gather psi; the C entry points refuse a NULL value and a
    bad ngroups * group_size before anything is launched."""
    import torch
    n, gs = 1024, 16
    rng = np.random.default_rng(1)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    lam = [1.0] * (n // gs)
    chi = s.NormLinf(1.0)
    h = s.GroupNormL2.uniform(lam, gs)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    for binf in (False, True):
        tr = (1.0, chi) if binf else ()
        with pytest.raises(TypeError):               # Float32
            psi = s.shifted(s.shifted(h, xd.float(), *tr), sd.float())
            s.prox_value(psi, qd.float(), 1.0)
        with pytest.raises(TypeError):               # host
            psi = s.shifted(s.shifted(h, x.copy(), *tr), sj.copy())
            s.prox_value(psi, q.copy(), 1.0)
        with pytest.raises(TypeError):               # index sets (gather layout)
            perm = rng.permutation(n)
            hg = s.GroupNormL2(lam, [perm[i:i + gs].tolist() for i in range(0, n, gs)])
            psi = s.shifted(s.shifted(hg, xd, *tr), sd)
            assert psi._layout.index is not None
            s.prox_value(psi, qd, 1.0)
        P = Problem(s, ("uniform", 16), binf)
        y = P.new_y(-9.0)
        torch.cuda.synchronize()
        assert P.proxval(y, rc_only=True, value=False) == SPX_ERR_INVALID_ARG
        P.ng += 1                                    # ngroups * group_size != n
        assert P.proxval(y, rc_only=True) == SPX_ERR_INVALID_ARG
        P.ng -= 1
        torch.cuda.synchronize()
        assert bool((y == -9.0).all())               # nothing was launched
        y, v = P.proxval(y)                          # and the context is fine
        assert np.isfinite(v)
    with pytest.raises(TypeError):                   # the remaining operators keep theirs
        s.prox_value(s.shifted(s.shifted(s.IndBallL0(3), xd), sd), qd, 1.0)


# ---- guard bands: one guarded-buffer case per fused tile family (tests/redzone.py) ----------------------------------------
REDZONE = [("1x8-binf", True, 8, 0), ("16x8-full", False, 128, 0), ("8x16-full-binf", True, 128, 0), ("64x6-padded", False, 300, 0),
           ("odd-8byte-loads", True, 17, 8), ("odd-8byte-loads-plain", False, 17, 8)]


@pytest.mark.parametrize("name,binf,gs,align", REDZONE, ids=[r[0] for r in REDZONE])
def test_guard_bands(s, orc, name, binf, gs, align):
    """Item 7: no write outside y, no element of y unwritten, no read past the end of an input (the poison would move the
    value and y away from the oracle's)."""
    import torch
    ng = 1001
    n = gs * ng
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    nS = np.linalg.norm(((q + x) + sj).reshape(ng, gs), axis=1)
    sigma, delta = 0.9, 0.8
    lam = nS * rng.choice([0.3, 0.8, 1.5], size=ng) / sigma
    zone = redzone.Zone()
    f64 = torch.float64
    yb = zone.add(n, f64, align, role="out", name="y")
    qb, xb, sb = (zone.add(n, f64, align, data=v, name=nm) for v, nm in ((q, "q"), (x, "xk"), (sj, "sj")))
    lb = zone.add(ng, f64, 0, data=lam, name="lambda")
    L, ctx = s._lib.load(), s.context("cuda:0")
    out = _D(-1.0)
    tail = (_D(delta),) if binf else ()
    fn = getattr(L, "spx_proxval_group_l2" + ("_binf" if binf else ""))
    torch.cuda.synchronize()
    s._lib.check(fn(ctx, ctypes.c_void_p(yb.ptr()), ctypes.c_void_p(qb.ptr()), ctypes.c_void_p(xb.ptr()), ctypes.c_void_p(sb.ptr()), n,
                    None, gs, ng, ctypes.c_void_p(lb.ptr()), _D(sigma), *tail, _D(1.0), ctypes.byref(out)))
    torch.cuda.synchronize()
    got = yb.t.cpu().numpy()
    with np.errstate(all="ignore"):
        ref = (orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs) if binf else orc.prox_group_l2(q, x, sj, lam, sigma, gsize=gs))
    # (the bar of tests/test_gpu_redzone.py: 1e-12 on the group's scale, differences above it adjudicated in binary128)
    arbiter.check_group(orc, got, ref, q, x, sj, lam, sigma, np.arange(0, n + 1, gs), delta=delta if binf else None, what=name)
    want = orc.obj_group_l2(got, x, sj, lam, gsize=gs)
    assert _close(out.value, want), (out.value, want)
    zone.check()
