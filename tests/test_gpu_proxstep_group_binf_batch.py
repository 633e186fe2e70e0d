"""GPU: batched ShiftedGroupNormL2Binf prox! + step statistics with the per-problem parameters on the device
(spx_proxstep_group_l2_binf_batch, prox_step_group_binf_batch / prox_step_group_binf_batch_bang).

Built on the pattern of test_gpu_proxstep_group_batch.py.  Problem b is row b of the batch x n tensors (row stride ld >= n),
n = ngroups * group_size in uniform contiguous groups; sigma_b, Delta_b, q_scale_b and the group weights (shared or per problem,
with or without a per-problem lambda_scale) are read from device arrays by the kernel that stores y.  Every row is held to the
SINGLE call (spx_proxstep_group_l2_binf through the C ABI) on that row alone with host copies of the scalars and host-multiplied
weights, on vectors of the launch's ALIGNMENT CLASS: y and xkn bit for bit (torch.equal on the int64 views).  The class: 16-byte
pairs when group_size and ld are even and every base is 16-byte aligned -- the reference is the single call on aligned vectors;
otherwise the element-wise form -- the reference is the single call on vectors 8 bytes off a 16-byte boundary.
The sums are held to the project's bars for blocked Float64 sums: [0], whose terms are non-negative, within 1e-12 * value of the
single call's [0] AND of sum_g lambda_g sqrt(fsum(v_g^2)) from the host copies; [1] and [2] within 1e-12 * sum |terms| of
math.fsum of the host's rounded products.

Group sizes sit on both sides of every bound of the two tile tables (GroupTilesBinf: 2, 4, 8, 16, 32, 64, 128, 256, 512;
GroupTilesLit: 16, 32, 64, 128, 256, 512); ngroups at 1, around 4 GPW (GPW = 64 / lanes per group of the GroupTilesBinf row) and
on either side of the row / tiled boundary n = 12288.  Data is on the scale of the existing Binf tests: entries O(1) / sqrt(gs),
Delta about 0.3 of that, lambda from {0.7, 2, 10} and from fac * ||S_g|| / sigma, so that zeroed, root and trust-region-active
groups all occur; sigma, Delta, q_scale and lambda_scale differ from row to row, row 1 has a Delta so large that the trust region
is inactive, row 2 one so small that every entry is clipped.  Three kinds of data:
  "mixed"   : the above;
  "literal" : groups that take the reference's literal evaluation BY CONSTRUCTION (the data of
              test_gpu_launch_counts.py::test_binf_deferred_list_without_the_zero_launch: n // 20 entries of xk exactly Delta_b;
              a lattice third as in test_gpu_proxval_group.Problem); row 0 has such an entry in EVERY group (a full bitmap), row 1
              is continuous without any (an empty one);
  "pole"    : groups of 16 whose root sits next to the pole (test_gpu_proxstep_group.py::
              test_groups_on_the_deferred_list_are_counted), literal under tuning key 9 = 1 only."""
import ctypes
import math

import numpy as np
import pytest

import arbiter
import nonfinite
import redzone

pytestmark = pytest.mark.gpu

R = 12288
TOL = 1e-12
INVALID = 1
POISON = -777.25
_D = ctypes.c_double
GROUP_SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512]
BATCHES = [1, 2, 3, 7]
TILES = [(2, 1), (4, 1), (8, 1), (16, 2), (32, 4), (64, 8), (128, 8), (256, 16), (512, 32)]   # GroupTilesBinf: (bound, lanes per group)
# the weights' layouts: (shared, extra row stride, with lambda_scale)
LAMBDAS = [(True, 0, False), (True, 0, True), (False, 0, False), (False, 0, True), (False, 3, False), (False, 3, True)]
LAMBDA_IDS = ["shared", "shared-scale", "rows", "rows-scale", "rows+3", "rows+3-scale"]
OWN = LAMBDAS[2]


def _lpg(gs):
    return next(l for b, l in TILES if gs <= b)


def _quad(gs):
    """4 GPW: the groups a workgroup's four wavefronts serve side by side"""
    return 4 * (64 // _lpg(gs))


def _run(gs):
    """groups per tile of the tiled form (gbatch_run)"""
    return max(1, 3072 // (gs * _quad(gs))) * _quad(gs)


def _counts(gs):
    q, edge = _quad(gs), R // gs
    return sorted({q - 1, q, q + 1, q + 2, edge, edge + 1})


def _two_counts(gs):
    """one row-form and one tiled-form count off the multiples of 4 GPW"""
    return [_quad(gs) + 1, R // gs + 1]


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _off8(t):
    """a copy of the 1-D tensor that starts 8 bytes past a 16-byte boundary"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(t)
    return buf[1:]


def _key9(s, v):
    s._lib.check(s._lib.load().spx_ctx_set_tuning(s.context("cuda:0"), 9, v))


class Problems:
    """`rows` problems of ng groups of gs elements, their scalars and weights (per problem and shared), and -- computed once
    per (weights, alignment class, key 9), shared by every test that places these rows somewhere -- what the single call gives
    on each row: y, xkn (device, rows x n), its triple and the host references of the sums."""
    _cache = {}

    @classmethod
    def get(cls, s, gs, ng, rows=7, kind="mixed"):
        key = (gs, ng, rows, kind)
        if key not in cls._cache:
            cls._cache[key] = cls(s, gs, ng, rows, kind)
        return cls._cache[key]

    def __init__(self, s, gs, ng, rows, kind):
        import torch
        rng = np.random.default_rng(9700 + 1000 * gs + ng + {"mixed": 0, "literal": 1, "pole": 2}[kind])
        self.s, self.gs, self.ng, self.rows, self.kind = s, gs, ng, rows, kind
        self.n = n = gs * ng
        if kind == "pole":
            X, SJ, Q = rng.normal(size=(rows, n)), rng.uniform(-0.5, 0.5, size=(rows, n)), rng.normal(size=(rows, n))
            self.sig, self.dlt, self.qs, self.ls = np.ones(rows), np.ones(rows), np.ones(rows), rng.uniform(0.3, 1.5, size=rows)
            nS = np.linalg.norm(((Q + X) + SJ).reshape(rows, ng, gs), axis=2)
            lam = rng.uniform(1.0, 40.0, size=(rows, ng)) * nS       # sigma * lambda up to 40 ||S_g||: roots next to the pole
            lam[:, ::2] = rng.uniform(0.1, 0.5, size=(rows, (ng + 1) // 2))   # every other group plainly active
            shared = lam[0].copy()
        else:
            scale = 0.6 / math.sqrt(gs)
            X, SJ, Q = rng.normal(size=(rows, n)) * scale, rng.uniform(-0.5, 0.5, size=(rows, n)) * scale, rng.normal(size=(rows, n)) * scale
            self.sig, self.qs, self.ls = (rng.uniform(0.3, 1.5, size=rows) for _ in range(3))
            self.dlt = 0.3 * scale * rng.uniform(0.5, 1.5, size=rows)
            if kind == "mixed":
                if rows > 1:
                    self.dlt[1] = 1e6            # the trust region is inactive
                if rows > 2:
                    self.dlt[2] = 1e-9 * scale   # every entry is clipped
            else:
                for r in range(rows):
                    if r == 1 and rows > 1:
                        continue                                     # row 1: continuous, nothing planted (an empty bitmap)
                    lat = n // 3                                     # a lattice third, xk = 0 on part of it
                    X[r, :lat] = rng.integers(-8, 9, size=lat) / 4.0
                    SJ[r, :lat] = rng.integers(-2, 3, size=lat) / 4.0
                    Q[r, :lat] = rng.integers(-12, 13, size=lat) / 4.0
                    X[r, : lat // 2] = 0.0
                    if r == 0:                                       # row 0: an entry ON the boundary in every group (a full bitmap)
                        X[0, np.arange(ng) * gs + rng.integers(0, gs, size=ng)] = self.dlt[0]
                    else:
                        X[r, rng.integers(0, n, size=max(1, n // 20))] = self.dlt[r]
            S = (self.qs[:, None] * Q + X) + SJ
            nS = np.sqrt((S.reshape(rows, ng, gs) ** 2).sum(axis=2))
            nS1 = np.where(nS > 0, nS, 1.0)
            lam = nS1 * rng.choice([0.0, 0.3, 0.7, 1.0, 1.5, 4.0, 40.0], size=(rows, ng)) / self.sig[:, None]
            half = rng.random(size=(rows, ng)) < 0.5
            lam[half] = rng.choice([2.0, 10.0, 0.7], size=int(half.sum()))
            shared = rng.choice([2.0, 10.0, 0.7], size=ng) * rng.choice([1.0, 0.1], size=ng)
        self.X, self.SJ, self.Q, self.lam, self.shared = X, SJ, Q, lam, shared
        self.Xd, self.SJd, self.Qd = (torch.from_numpy(a).cuda() for a in (X, SJ, Q))
        self.refs = {}

    def weights(self, lam_kind, r):
        """the host-multiplied weights of row r under a layout of LAMBDAS: one rounded multiply"""
        shared, _, scaled = lam_kind
        w = self.shared if shared else self.lam[r]
        return self.ls[r] * w if scaled else w

    def single(self, r, lam_kind=OWN, off8=False, q=None, xk=None, sj=None, scal=None, w=None, xkn=True):
        """spx_proxstep_group_l2_binf on row r alone (or on the given vectors / (sigma, Delta, q_scale) / weights), every vector on
        a 16-byte boundary or (off8) 8 bytes past one: (y, xkn, [h, qy, yy])"""
        import torch
        s = self.s
        L, ctx = s._lib.load(), s.context("cuda:0")
        q = self.Qd[r] if q is None else q
        xk = self.Xd[r] if xk is None else xk
        sj = self.SJd[r] if sj is None else sj
        sig, dlt, qs = scal if scal is not None else (self.sig[r], self.dlt[r], self.qs[r])
        w = self.weights(lam_kind, r) if w is None else w
        lam = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        mk = _off8 if off8 else (lambda t: t.clone())
        q, xk, sj = mk(q), mk(xk), mk(sj)
        y, k = mk(torch.full_like(q, POISON)), mk(torch.full_like(q, POISON))
        assert all(t.data_ptr() % 16 == (8 if off8 else 0) for t in (q, xk, sj, y, k))
        st = (_D * 3)()
        rc = L.spx_proxstep_group_l2_binf(ctx, _P(y), _P(q), _P(xk), _P(sj), self.n, None, self.gs, self.ng, _P(lam), float(sig),
                                          float(dlt), float(qs), _P(k) if xkn else None, st, None)
        assert rc == 0, L.spx_last_error()
        return y, k, [st[0], st[1], st[2]]

    def ref(self, lam_kind, pairs, key9=0):
        """per (weights, class, key 9): (Y rows x n, XKN rows x n on the device, single-call triples, host sum references per row);
        the caller has set key 9 accordingly"""
        import torch
        key = (lam_kind[0], lam_kind[2], bool(pairs) or self.gs % 2 == 1, key9)   # (odd sizes: one call shape whatever the bases)
        if key not in self.refs:
            ys, ks, sts, sums = [], [], [], []
            for r in range(self.rows):
                y, k, st = self.single(r, lam_kind, off8=not key[2])
                ys.append(y.clone()); ks.append(k.clone()); sts.append(st)
                sums.append(self.sum_refs(r, y.cpu().numpy(), k.cpu().numpy(), self.weights(lam_kind, r)))
            self.refs[key] = (torch.stack(ys), torch.stack(ks), sts, sums)
        return self.refs[key]

    def sum_refs(self, r, y, v, w, q=None):
        """exactly rounded references from the host copies: v = (xk + sj) + y as stored"""
        q = self.Q[r] if q is None else q
        v2 = (v * v).reshape(self.ng, self.gs)
        h = math.fsum(float(w[g]) * math.sqrt(math.fsum(v2[g])) for g in range(self.ng))
        qy = q * y
        return h, math.fsum(qy), math.fsum(np.abs(qy)), math.fsum(y * y)


def _check_stats(got, single, ref, what):
    h, qy, mqy, yy = ref
    g0, g1, g2 = (float(v) for v in got)
    print("%s: h %.17g single %.17g host %.17g | qy %.17g ref %.17g (bar %.3g) | yy %.17g ref %.17g" % (what, g0, single[0], h, g1, qy, TOL * mqy, g2, yy))
    if any(math.isnan(v) for v in single):
        # finite data on which the single call's own y holds a NaN (met on the lattice data at group size 1, where the literal
        # evaluation follows the reference into 0 / 0): y has that call's bits, and a sum that is NaN there is NaN here
        assert all(math.isnan(g) == math.isnan(v) for g, v in zip((g0, g1, g2), single)), (what, got, single)
        return
    assert abs(g0 - single[0]) <= TOL * abs(single[0]), (what, g0, single[0])
    assert abs(g0 - h) <= TOL * h, (what, g0, h)
    assert abs(g1 - qy) <= TOL * mqy, (what, g1, qy, mqy)
    assert abs(g2 - yy) <= TOL * yy, (what, g2, yy)


def _bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


class Layout:
    """the five batch x n tensors of a call as views of flat poisoned buffers: row stride ld = n + pad, bases `off` (0 / 1)
    elements past a 256-byte boundary (xkn: xkn_off), rows = the problem rows placed at batch rows 0, 1, ...; the weights in
    the layout lam_kind of LAMBDAS"""

    def __init__(self, prob, rows, pad, off, xkn_off=None, guarded=False, lam_kind=OWN):
        import torch
        self.prob, self.rows, self.n, self.batch, self.lam_kind = prob, list(rows), prob.n, len(rows), lam_kind
        self.ld = ld = prob.n + pad
        xkn_off = off if xkn_off is None else xkn_off
        total = self.batch * ld
        self.zone = redzone.Zone() if guarded else None

        def flat(o, name):
            if guarded:   # [front guard | batch * ld elements | back guard], poison everywhere
                return self.zone.add(total, torch.float64, align_bytes=8 * o, role="inout", poison=POISON, name=name,
                                     data=torch.full((total,), POISON, dtype=torch.float64)).t
            return torch.full((total + 2,), POISON, dtype=torch.float64, device="cuda:0")[o:o + total]

        self.fy, self.fk = flat(off, "y"), flat(xkn_off, "xkn")
        self.fq, self.fx, self.fs = flat(off, "q"), flat(off, "xk"), flat(off, "sj")
        view = lambda f: f.as_strided((self.batch, self.n), (ld, 1))
        self.Y, self.K, self.Q, self.X, self.S = (view(f) for f in (self.fy, self.fk, self.fq, self.fx, self.fs))
        idx = torch.as_tensor(self.rows, device="cuda:0")
        self.Q.copy_(prob.Qd[idx]); self.X.copy_(prob.Xd[idx]); self.S.copy_(prob.SJd[idx])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[self.rows])).cuda()
        self.sig, self.dlt, self.qs = dev(prob.sig), dev(prob.dlt), dev(prob.qs)
        shared, lpad, scaled = lam_kind
        self.ls = dev(prob.ls) if scaled else None
        if shared:
            self.lam = torch.from_numpy(prob.shared).cuda()
        else:
            ldl = prob.ng + lpad
            self.flam = torch.full((self.batch * ldl,), POISON, dtype=torch.float64, device="cuda:0")
            self.lam = self.flam.as_strided((self.batch, prob.ng), (ldl, 1))
            self.lam.copy_(dev(prob.lam))
        self.out = torch.full((self.batch, 3), POISON, dtype=torch.float64, device="cuda:0")
        # the launch's alignment class (the mirror hands ld = n to the library for a single row)
        ld_eff = ld if self.batch > 1 else self.n
        self.pairs = prob.gs % 2 == 0 and ld_eff % 2 == 0 and off == 0 and xkn_off == 0
        self.pairs_without_xkn = prob.gs % 2 == 0 and ld_eff % 2 == 0 and off == 0
        if guarded:
            for g in self.zone.bufs:
                g.snap = g.buf.clone()   # (the inputs were copied in after the snapshot was taken)

    def call(self, s, xkn=True):
        return s.prox_step_group_binf_batch_bang(self.Y, self.Q, self.X, self.S, self.prob.gs, self.lam, self.sig, self.dlt, self.qs,
                                                 lam_scale=self.ls, xkn=self.K if xkn else None, out=self.out)

    def padding_untouched(self, xkn=True):
        """every element [b ld + n, (b + 1) ld) of y and xkn still holds the poison, and no row element does"""
        for f, V in ((self.fy, self.Y), (self.fk, self.K))[:2 if xkn else 1]:
            whole = f.as_strided((self.batch, self.ld), (self.ld, 1))
            assert bool((whole[:, self.n:] == POISON).all()), "padding written"
            assert not bool((V == POISON).any()), "row element not written"

    def check(self, what, xkn=True, stats=True, key9=0):
        import torch
        Yr, Kr, sts, sums = self.prob.ref(self.lam_kind, self.pairs if xkn else self.pairs_without_xkn, key9)
        idx = torch.as_tensor(self.rows, device="cuda:0")
        assert _bits(self.Y, Yr[idx]), what
        if xkn:
            assert _bits(self.K, Kr[idx]), what
        else:
            assert bool((self.fk == POISON).all()), what
        self.padding_untouched(xkn)
        if stats:
            got = self.out.cpu().numpy()
            for b, r in enumerate(self.rows):
                _check_stats(got[b], sts[r], sums[r], "%s row %d" % (what, b))


# ------------------------------------------------------------------ parity with the single call
@pytest.mark.parametrize("gs", GROUP_SIZES)
def test_gbinf_rows_equal_the_single_call(s, gs):
    for ng in _counts(gs):
        prob = Problems.get(s, gs, ng)
        for batch in BATCHES:
            for pad in (0, 1, 2, 3):
                for off in (0, 1):
                    lay = Layout(prob, range(batch), pad, off)
                    lay.call(s)
                    lay.check("gs=%d ng=%d batch=%d pad=%d off=%d" % (gs, ng, batch, pad, off))


@pytest.mark.parametrize("gs", GROUP_SIZES)
def test_gbinf_xkn_absent_and_misaligned_alone(s, gs):
    """xkn = None: y and the sums as with it, in the class of the four other vectors; xkn alone 8 bytes off (and alone on the
    boundary): the element-wise form for every row"""
    for ng in _two_counts(gs):
        prob = Problems.get(s, gs, ng)
        for pad, off in ((0, 0), (1, 0), (2, 1)):
            lay = Layout(prob, range(3), pad, off)
            lay.call(s, xkn=False)
            lay.check("no xkn gs=%d ng=%d pad=%d off=%d" % (gs, ng, pad, off), xkn=False)
        for pad, off, xkn_off in ((0, 0, 1), (2, 0, 1), (0, 1, 0)):
            lay = Layout(prob, range(3), pad, off, xkn_off=xkn_off)
            assert not lay.pairs
            lay.call(s)
            lay.check("xkn alone gs=%d ng=%d pad=%d off=%d/%d" % (gs, ng, pad, off, xkn_off))


@pytest.mark.parametrize("lam_kind", LAMBDAS, ids=LAMBDA_IDS)
def test_gbinf_weight_layouts(s, lam_kind):
    """shared weights (ldl = 0), one row per problem (ldl = ngroups, ngroups + 3), each with and without lambda_scale: the
    single call on the host-multiplied products"""
    for gs in (2, 8, 9, 128, 257):
        for ng in _two_counts(gs):
            prob = Problems.get(s, gs, ng)
            for batch, pad, off in ((1, 0, 0), (3, 0, 0), (3, 1, 0), (7, 2, 1)):
                lay = Layout(prob, range(batch), pad, off, lam_kind=lam_kind)
                lay.call(s)
                lay.check("%s gs=%d ng=%d batch=%d pad=%d off=%d" % (lam_kind, gs, ng, batch, pad, off))
                if not lam_kind[0] and lam_kind[1]:
                    whole = lay.flam.as_strided((batch, ng + 3), (ng + 3, 1))
                    assert bool((whole[:, ng:] == POISON).all())   # (the weights' padding is an input: never written)


# ------------------------------------------------------------------ literal groups
@pytest.mark.parametrize("gs", [2, 8, 16, 50, 128, 300])
def test_gbinf_literal_groups_by_construction(s, gs):
    """entries of xk exactly on the trust-region boundary and lattice data: the single call hands those groups to its LIT launch
    (its own register tile), the batched call evaluates them in the second phase of the workgroup that met them.  Row 0: such
    an entry in every group (a full bitmap); row 1: none (an empty one), next to each other.  Both forms, both classes."""
    for ng in _two_counts(gs):
        prob = Problems.get(s, gs, ng, kind="literal")
        for batch, pad, off in ((2, 0, 0), (7, 2, 0), (3, 1, 0), (7, 0, 1)):
            lay = Layout(prob, range(batch), pad, off)
            lay.call(s)
            lay.check("literal gs=%d ng=%d batch=%d pad=%d off=%d" % (gs, ng, batch, pad, off))
        lay = Layout(prob, range(3), 0, 0, lam_kind=LAMBDAS[1])
        lay.call(s, xkn=False)
        lay.check("literal, shared weights, no xkn gs=%d ng=%d" % (gs, ng), xkn=False)


def test_gbinf_literal_groups_observed(s):
    """groups of 16 whose root sits next to the pole of step(n) (sigma lambda up to 40 ||S_g||): under tuning key 9 = 1 they are
    evaluated literally, under key 9 = 0 by the closed form, and the two differ in the last bits.  First, on the SINGLE call's
    output alone: at least 10 groups per row differ between the modes (ngroups per row is raised until the single call says
    so).  Then the batched call equals the single call bit for bit in BOTH modes: an implementation that evaluates literal groups
    on the main tile, or drops them, fails here."""
    import torch
    gs, rows = 16, 3
    ng = 20_000 // rows
    try:
        for attempt in range(6):
            prob = Problems.get(s, gs, ng, rows=rows, kind="pole")
            _key9(s, 0)
            y0 = prob.ref(OWN, True, key9=0)[0]
            _key9(s, 1)
            y1 = prob.ref(OWN, True, key9=1)[0]
            differ = (y0 != y1).view(rows, ng, gs).any(dim=2).sum(dim=1).cpu().numpy()
            print("ngroups %d: groups that differ between key 9 = 0 and 1 per row: %s" % (ng, differ.tolist()))
            if differ.min() >= 10:
                break
            Problems._cache.pop((gs, ng, rows, "pole"))
            ng *= 2
        assert differ.min() >= 10, differ
        for key9 in (1, 0):
            _key9(s, key9)
            for pad, off in ((0, 0), (2, 0), (1, 1)):
                lay = Layout(prob, range(rows), pad, off)
                lay.call(s)
                lay.check("pole key9=%d pad=%d off=%d" % (key9, pad, off), key9=key9)
    finally:
        _key9(s, 0)
        Problems._cache.pop((gs, ng, rows, "pole"), None)


# ------------------------------------------------------------------ an independent check: the CPU oracle
@pytest.mark.parametrize("gs", [8, 128])
def test_gbinf_rows_against_the_oracle(s, orc, gs):
    """every row of y against oracle.prox_group_l2_binf(q_scale_b * q, ...) at 1e-12 with the binary128 arbiter adjudicating
    (arbiter.check_group), [0] against oracle.obj_group_l2 of the stored y: a bug shared with the single call cannot hide
    behind the bit parity"""
    ng = _quad(gs) + 1
    offsets = np.arange(0, gs * ng + 1, gs, dtype=np.int64)
    for kind in ("mixed", "literal"):
        prob = Problems.get(s, gs, ng, kind=kind)
        for lam_kind in (OWN, LAMBDAS[1]):
            for pad, off in ((0, 0), (1, 1)):
                lay = Layout(prob, range(7), pad, off, lam_kind=lam_kind)
                lay.call(s)
                Y, K, out = lay.Y.cpu().numpy(), lay.K.cpu().numpy(), lay.out.cpu().numpy()
                for r in range(7):
                    q = prob.qs[r] * prob.Q[r]    # one rounded multiply per element, as the kernel forms it
                    w = prob.weights(lam_kind, r)
                    ref = orc.prox_group_l2_binf(q, prob.X[r], prob.SJ[r], w, prob.sig[r], prob.dlt[r], gsize=gs)
                    arbiter.check_group(orc, Y[r], ref, q, prob.X[r], prob.SJ[r], w, prob.sig[r], offsets, delta=prob.dlt[r],
                                        what="gs=%d %s row %d" % (gs, kind, r))
                    assert np.array_equal(K[r], (prob.X[r] + prob.SJ[r]) + Y[r]), (gs, r)
                    h = orc.obj_group_l2(Y[r], prob.X[r], prob.SJ[r], w, gsize=gs)
                    assert abs(out[r, 0] - h) <= TOL * abs(h), (gs, kind, r, out[r, 0], h)


# ------------------------------------------------------------------ padding and ends
@pytest.mark.parametrize("gs", [1, 3, 8, 128, 257, 512])
def test_gbinf_guard_bands_and_padding(s, gs):
    """y and xkn between guard bands, poison everywhere: after the call the guard bands (and the inputs) are unchanged, every
    padding element still holds the poison and no row element does"""
    for kind, counts in (("mixed", [1] + _two_counts(gs)), ("literal", _two_counts(gs))):
        for ng in counts:
            prob = Problems.get(s, gs, ng, kind=kind)
            for batch, pad, off in ((1, 0, 0), (1, 3, 1), (3, 0, 1), (3, 1, 0), (3, 2, 0), (3, 2, 1), (7, 3, 0)):
                lay = Layout(prob, range(batch), pad, off, guarded=True)
                lay.call(s)
                lay.zone.check()     # guard bands of y, xkn, q, xk, sj
                for g in lay.zone.bufs[2:]:   # q, xk, sj: read only
                    assert bool((g.buf == g.snap).all()), g.name
                lay.check("guarded %s gs=%d ng=%d batch=%d pad=%d off=%d" % (kind, gs, ng, batch, pad, off))


# ------------------------------------------------------------------ the sums' bits
@pytest.mark.parametrize("gs", [1, 4, 8, 16, 33, 64, 128, 256, 300, 512])
def test_gbinf_bits_do_not_depend_on_repeat_row_or_batch(s, gs):
    """with literal groups present: a repeat; the same problem at row 0 of batch 1, row 2 of batch 3, row 6 of batch 7; batch 7
    cut to 2: the same bits in y, xkn and the three sums (the order of the sums depends on group_size, ngroups, the alignment
    class and the row's own literal groups only)"""
    same = lambda a, b: all(_bits(x, z) for x, z in zip(a, b))
    for ng in _two_counts(gs):
        prob = Problems.get(s, gs, ng, kind="literal")
        for pad, off in ((0, 0), (2, 0), (1, 0), (2, 1)):
            a, b = Layout(prob, range(7), pad, off), Layout(prob, range(7), pad, off)
            a.call(s); b.call(s); a.call(s)
            assert _bits(a.out, b.out), (gs, ng, pad, off)
            two = Layout(prob, range(2), pad, off)
            two.call(s)
            assert same((two.Y, two.K, two.out), (a.Y[:2], a.K[:2], a.out[:2])), (gs, ng, pad, off)
            # (with an odd ld the single row of batch 1 is handed ld = n and may fall into another class than the larger
            #  batches: it is left out there, the placements in batch 3 and batch 7 share their class and are compared)
            places = (([4], 0), ([0, 1, 4], 2), ([0, 1, 2, 3, 5, 6, 4], 6))
            seen = None
            for rows, at in places[1 if pad % 2 else 0:]:
                lay = Layout(prob, rows, pad, off)
                lay.call(s)
                cur = (lay.Y[at].clone(), lay.K[at].clone(), lay.out[at].clone())
                assert seen is None or same(seen, cur), (gs, ng, pad, off, at)
                seen = cur
            assert same(seen, (a.Y[4], a.K[4], a.out[4])), (gs, ng, pad, off)


# ------------------------------------------------------------------ more problems than CUs, more than 65535 rows
@pytest.mark.parametrize("batch,gs,ng", [(300, 5, 3), (70001, 2, 2)])
def test_gbinf_many_rows(s, batch, gs, ng):
    prob = Problems.get(s, gs, ng, rows=batch)
    rng = np.random.default_rng(batch)
    rows = sorted({0, 1, 2, batch - 1} | set(rng.choice(batch, size=30, replace=False).tolist()))
    for pad, off in ((0, 0), (1, 1)):
        lay = Layout(prob, range(batch), pad, off)
        lay.call(s)
        lay.padding_untouched()
        got = lay.out.cpu().numpy()
        for r in rows:
            y, k, st = prob.single(r, off8=not lay.pairs)
            assert _bits(lay.Y[r], y) and _bits(lay.K[r], k), (batch, r)
            _check_stats(got[r], st, prob.sum_refs(r, y.cpu().numpy(), k.cpu().numpy(), prob.lam[r]), "batch=%d row %d" % (batch, r))
    Problems._cache.pop((gs, ng, batch, "mixed"))


def test_gbinf_more_partials_than_one_pass_adds(s):
    """groups of 512 in tiles of 8: 16392 groups are 2049 tiles -- the per-problem reduction takes its long loop (more than 2048
    partials a plane)"""
    gs, ng = 512, 8 * 2048 + 8
    assert _run(gs) == 8
    prob = Problems.get(s, gs, ng, rows=2)
    lay = Layout(prob, range(2), 2, 0)
    lay.call(s)
    lay.padding_untouched()
    got = lay.out.cpu().numpy()
    for r in range(2):
        y, k, st = prob.single(r)
        assert _bits(lay.Y[r], y) and _bits(lay.K[r], k), r
        _check_stats(got[r], st, prob.sum_refs(r, y.cpu().numpy(), k.cpu().numpy(), prob.lam[r]), "long reduce row %d" % r)
    Problems._cache.pop((gs, ng, 2, "mixed"))


# ------------------------------------------------------------------ isolation under non-finite data
def _same_sum(a, b, mag):
    """two sums of the same terms added in different orders (include/spx.h, non-finite data)"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= 2 * TOL * mag     # (each within TOL * mag of the exact sum)


@pytest.mark.parametrize("gs", [8, 33])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 1e150])
def test_gbinf_nonfinite_row_is_isolated(s, gs, value):
    """NaN, +-Inf, 1e150 in one element of ONE row of a batch of 3 -- element 0, the last group, a group of the second tile (the
    second wave tile in the row form) -- in the sequence clean / planted / clean on one context: the planted row behaves as
    spx_proxstep_group_l2_binf does on it (a NaN group takes the literal path and is NaN throughout), the other rows and the
    clean call behind keep the bits of the clean call in front"""
    for ng in _two_counts(gs):
        prob = Problems.get(s, gs, ng)
        n = prob.n
        tiled = n > R
        second = (_run(gs) + 1 if tiled else 64 // _lpg(gs) + 1) * gs + gs // 2
        assert second < n
        for pad, off in ((0, 0), (1, 1)):
            clean = Layout(prob, range(3), pad, off)
            clean.call(s)
            for where in ("q", "xk", "sj"):
                for at in (0, n - gs // 2 - 1, second):
                    lay = Layout(prob, range(3), pad, off)
                    t = {"q": lay.Q, "xk": lay.X, "sj": lay.S}[where]
                    t[1, at] = value
                    lay.call(s)
                    lay.padding_untouched()
                    y, k, st = prob.single(1, off8=not lay.pairs, q=lay.Q[1].clone(), xk=lay.X[1].clone(), sj=lay.S[1].clone())
                    what = (gs, ng, value, where, at, pad, off)
                    # include/spx.h, non-finite data: the same bits, NaN where that is NaN (which payload a NaN carries out of a
                    # product of two NaNs is the compiler's choice of operand order, kernel by kernel)
                    yh, kh, qh = y.cpu().numpy(), k.cpu().numpy(), lay.Q[1].cpu().numpy()
                    assert nonfinite.same_bits_or_both_nan(lay.Y[1].cpu().numpy(), yh).all(), what
                    assert nonfinite.same_bits_or_both_nan(lay.K[1].cpu().numpy(), kh).all(), what
                    if math.isnan(value):
                        g = at // gs
                        mask = np.zeros(n, dtype=bool)
                        mask[g * gs:(g + 1) * gs] = True
                        assert np.isnan(yh[mask]).all() and not np.isnan(yh[~mask]).any(), what   # the group, and nothing else
                    got = lay.out[1].cpu().numpy()
                    with np.errstate(all="ignore"):
                        mags = (abs(st[0]), np.sum(np.abs(qh * yh)), np.sum(yh * yh))
                    for j in range(3):
                        assert _same_sum(float(got[j]), st[j], mags[j]), (what, j, got[j], st[j])
                    if math.isfinite(st[0]):    # [0] against the single call's: the bar of the clean rows
                        assert abs(float(got[0]) - st[0]) <= TOL * abs(st[0]), (what, got[0], st[0])
                    for b in (0, 2):
                        assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.K[b], clean.K[b]) and _bits(lay.out[b], clean.out[b]), what
            after = Layout(prob, range(3), pad, off)
            after.call(s)
            assert _bits(after.Y, clean.Y) and _bits(after.K, clean.K) and _bits(after.out, clean.out), (gs, ng, value, pad, off)


# ------------------------------------------------------------------ refusals and empties
def test_gbinf_refusals_and_empties(s):
    import torch
    gs, ng, batch = 8, 65, 3
    prob = Problems.get(s, gs, ng)
    n = prob.n
    L, G, ctx = s._lib.load(), s._lib.load_gbinf_batch(), s.context("cuda:0")
    lay = Layout(prob, range(batch), 2, 0, lam_kind=LAMBDAS[5])
    ld, ldl = lay.ld, ng + 3
    y, q, xk, sj, k = (_P(f) for f in (lay.fy, lay.fq, lay.fx, lay.fs, lay.fk))
    lam, ls, sig, dlt, qs, out = _P(lay.flam), _P(lay.ls), _P(lay.sig), _P(lay.dlt), _P(lay.qs), _P(lay.out)
    Z = None

    def call(y=y, q=q, xk=xk, sj=sj, gs=gs, ng=ng, batch=batch, ld=ld, lam=lam, ldl=ldl, ls=ls, sig=sig, dlt=dlt, qs=qs, k=k, out=out):
        return G.spx_proxstep_group_l2_binf_batch(ctx, y, q, xk, sj, gs, ng, batch, ld, lam, ldl, ls, sig, dlt, qs, k, out)

    def untouched():
        torch.cuda.synchronize()
        return bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()) and bool((lay.out == POISON).all())

    def next_call_is_right():
        assert call() == 0
        lay.check("after a refusal")
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)

    refusals = [
        ("group_size 0", lambda: call(gs=0)), ("group_size < 0", lambda: call(gs=-8)), ("group_size 513", lambda: call(gs=513, ng=1)),
        ("ngroups < 0", lambda: call(ng=-1)), ("batch < 0", lambda: call(batch=-1)),
        ("ngroups * group_size overflows", lambda: call(gs=512, ng=1 << 55, ld=(1 << 63) - 1)),
        ("ld < n", lambda: call(ld=n - 1)), ("ldl < ngroups", lambda: call(ldl=ng - 1)), ("ldl < 0", lambda: call(ldl=-1)),
        ("y == q", lambda: call(y=q)), ("xkn == y", lambda: call(k=y)), ("xkn == q", lambda: call(k=q)),
        ("xkn == xk", lambda: call(k=xk)), ("xkn == sj", lambda: call(k=sj)),
        ("lambda_vec NULL", lambda: call(lam=Z)), ("sigma NULL", lambda: call(sig=Z)), ("delta NULL", lambda: call(dlt=Z)),
        ("q_scale NULL", lambda: call(qs=Z)), ("stats_dev NULL", lambda: call(out=Z)),
        # more than 2^31 - 1 workgroups: one per problem in the row form, five per problem just above the boundary (never
        # launched: the refusal comes before anything is touched)
        ("2^31 workgroups", lambda: call(ng=1, ld=8, batch=1 << 31)),
        ("2^31 workgroups, tiled", lambda: call(ng=R // 8 + 1, ld=R + 8, ldl=0, batch=((1 << 31) - 1) // 5 + 1)),
    ]
    for what, f in refusals:
        assert f() == INVALID, what
        assert L.spx_last_error(), what
        assert untouched(), what
        next_call_is_right()
    assert call(gs=513, ng=1) == INVALID and b"spx_proxstep_group_l2_binf" in L.spx_last_error()   # (names the call for larger groups)
    # empties: batch == 0 does nothing; n == 0 (ngroups == 0) stores 3 * batch zeros (by a kernel)
    assert call(batch=0) == 0 and call(batch=0, lam=Z, sig=Z, dlt=Z, qs=Z, out=Z) == 0 and untouched()
    next_call_is_right()
    for kw in (dict(ng=0, ld=0), dict(ng=0, ld=5), dict(ng=0, ld=0, lam=Z, sig=Z, dlt=Z, qs=Z, y=Z, q=Z, xk=Z, sj=Z, k=Z)):
        assert call(**kw) == 0, kw
        torch.cuda.synchronize()
        assert bool((lay.out == 0.0).all()) and bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()), kw
        lay.out.fill_(POISON)
    next_call_is_right()
    # the mirror refuses what it can see
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Y, lay.X, lay.S, gs, lay.lam, lay.sig, lay.dlt, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, 7, lay.lam, lay.sig, lay.dlt, lay.qs)         # n is no multiple of 7
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, gs, lay.lam[:, :-1], lay.sig, lay.dlt, lay.qs)   # ngroups - 1 weights
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, gs, lay.lam, lay.sig, lay.dlt[:2], lay.qs)    # two radii
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, gs, lay.lam, lay.sig, 0.3, lay.qs)            # a host radius
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, gs, lay.lam, lay.sig, lay.dlt.cpu(), lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_group_binf_batch_bang(lay.Y, lay.Q.contiguous(), lay.X, lay.S, gs, lay.lam, lay.sig, lay.dlt, lay.qs)   # another row stride
    Yn, outn = s.prox_step_group_binf_batch(lay.Q, lay.X, lay.S, gs, lay.lam, lay.sig, lay.dlt, lay.qs, lam_scale=lay.ls)
    assert _bits(Yn, prob.ref(LAMBDAS[5], True)[0][:batch]) and Yn.stride() == lay.Q.stride() and tuple(outn.shape) == (batch, 3)


def test_gbinf_q_scale_zero_in_one_row(s):
    """q_scale[b] = 0 in one row: that row is the prox at q = 0 (the single call with q_scale = 0: same bits, [1] sums q AS
    PASSED times y), the other rows keep their bits"""
    prob = Problems.get(s, 8, 65)
    clean = Layout(prob, range(4), 0, 0)
    clean.call(s)
    lay = Layout(prob, range(4), 0, 0)
    lay.qs[3] = 0.0
    lay.call(s)
    y, k, st = prob.single(3, scal=(prob.sig[3], prob.dlt[3], 0.0))
    assert _bits(lay.Y[3], y) and _bits(lay.K[3], k)
    got = lay.out.cpu().numpy()
    _check_stats(got[3], st, prob.sum_refs(3, y.cpu().numpy(), k.cpu().numpy(), prob.lam[3]), "q_scale = 0")
    assert all(math.isfinite(v) for v in got.ravel())
    for b in (0, 1, 2):
        assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.out[b], clean.out[b])


# ------------------------------------------------------------------ the parameters follow the device
@pytest.mark.parametrize("gs", [8, 128])
def test_captured_gbinf_call_follows_the_device_parameters(s, gs):
    """one batched call captured into a graph (side stream, warm-up first: the tiled form reserves its workspace there);
    between replays sigma, Delta, q_scale and lambda_scale are overwritten ON THE DEVICE: every replay's rows equal the single
    call with the NEW scalars, bit for bit"""
    import torch
    rng = np.random.default_rng(9800 + gs)
    for ng in _two_counts(gs):
        prob = Problems.get(s, gs, ng, kind="literal")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lay = Layout(prob, range(3), 2, 0, lam_kind=LAMBDAS[1])
            lay.call(s); lay.call(s)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            lay.call(s)
        for rep in range(3):
            sig, qs, ls = (rng.uniform(0.3, 1.5, size=3) for _ in range(3))
            dlt = prob.dlt[:3] * (1.0 if rep == 0 else rng.uniform(0.25, 4.0, size=3))   # (first replay: the planted radii, literal groups)
            for t, a in ((lay.sig, sig), (lay.dlt, dlt), (lay.qs, qs), (lay.ls, ls)):
                t.copy_(torch.from_numpy(a))
            lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            lay.padding_untouched()
            got = lay.out.cpu().numpy()
            for b in range(3):
                w = ls[b] * prob.shared
                y, k, st = prob.single(b, scal=(sig[b], dlt[b], qs[b]), w=w)
                what = (gs, ng, rep, b)
                assert _bits(lay.Y[b], y) and _bits(lay.K[b], k), what
                _check_stats(got[b], st, prob.sum_refs(b, y.cpu().numpy(), k.cpu().numpy(), w), str(what))
