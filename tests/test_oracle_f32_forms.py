"""The Float32 psi(y) / ShiftedGroupNormL2.prox! restatements (second half of oracle/spx_oracle_f32.c) pinned on the CPU alone:
against the Float64 restatement on data where both are exact, against hand-derivable answers, and -- with the inputs, bars and
census of tests/f32_exact.py that tests/test_gpu_f32_exact.py applies to the device -- against seven planted mistakes."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import f32_exact as fx
import nonfinite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_f32_forms_agree_with_f64_on_dyadic_data(orc):
    """Multiples of 1/16 below 2^7 (lambda dyadic): every sum is exact in both formats, |v| and the 0 / 1 terms are the same
    numbers, every square and sum of squares fits 53 bits -- the two restatements must agree value for value.  RootNormLhalf
    on fourth powers of such numbers' square roots: v in {0, 1/16, 1/4, 9/16, 1, ...} has an exact root in both."""
    rng = np.random.default_rng(12)
    n = 20_000
    x = rng.integers(-64, 65, size=n) / 16.0
    sj = rng.integers(-16, 17, size=n) / 16.0
    y = rng.integers(-32, 33, size=n) / 16.0
    l = -(rng.integers(48, 65, size=n) / 16.0)
    u = rng.integers(48, 65, size=n) / 16.0
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    lam = 0.75
    for kind in ("l1", "l0"):
        t, bad = orc.obj_f32(kind, y, x, sj)
        assert not bad and lam * math.fsum(t.tolist()) == orc.obj_plain(kind, y, x, sj, lam)
        for lo, uo, m in ((-4.0, 4.0, None), (l, u, None), (l, u, mask), (l, 4.0, mask), (-4.0, u, None)):
            t, bad = orc.obj_f32(kind, y, x, sj, l=lo, u=uo, mask=m)
            assert not bad and lam * math.fsum(t.tolist()) == orc.obj_box(kind, y, x, sj, lam, lo, uo, m)
        t, bad = orc.obj_f32(kind, y, x, sj, l=-1.0, u=u)      # |sj + y| reaches 3: infeasible in both
        assert bad and orc.obj_box(kind, y, x, sj, lam, -1.0, u) == np.inf
    r2 = rng.integers(0, 12, size=n) / 4.0                      # exact square roots
    v = r2 * r2 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    t, bad = orc.obj_f32("lhalf", v - x - sj, x, sj)
    assert np.array_equal(t, r2) and lam * math.fsum(t.tolist()) == orc.obj_plain("lhalf", v - x - sj, x, sj, lam)
    # IndBallL0(BInf): the count and the ball
    t, bad = orc.obj_f32("l0", y, x, sj, delta=2.0)
    nnz = int(t.sum())
    assert bad == bool(np.any(np.abs(sj + y) > 2.2)) and bad
    t, bad = orc.obj_f32("l0", y, x, sj, delta=3.0)
    assert not bad
    for r in (nnz - 1, nnz):
        assert orc.obj_indball_l0(y, x, sj, r, delta=3.0) == (np.inf if nnz > r else 0.0)
    # groups: squares of multiples of 1/16 below 8 sum exactly; lambda dyadic; CSR with empty groups and uncovered ends
    offs = np.concatenate([[5], np.sort(rng.integers(5, n - 7, size=499)), [n - 7]]).astype(np.int64)
    lam_g = rng.integers(1, 9, size=500) / 8.0
    for delta in (None, 3.0):
        t, outside, badoff = orc.obj_group_f32(y, x, sj, lam_g, offsets=offs, delta=delta)
        assert not outside and not badoff
        want = orc.obj_group_l2(y, x, sj, lam_g, offsets=offs, delta=delta)
        assert abs(math.fsum(t.tolist()) - want) <= 1e-13 * want      # (the Float64 restatement adds left to right)
        t, _, _ = orc.obj_group_f32(y, x, sj, np.ones(n // 8), gsize=8, delta=delta)
        nrm = np.sqrt(np.add.reduceat(((x + sj) + y) ** 2, np.arange(0, n, 8)))
        assert np.array_equal(t, nrm)
    assert orc.obj_group_f32(y, x, sj, lam_g, offsets=offs, delta=2.0)[1]
    # prox!: perfect-square norms (3-4-5 groups scaled by powers of two), dyadic sigma lambda / snorm: exact in both
    k = 2000
    s3 = 2.0 ** rng.integers(-3, 4, size=k)
    S = np.stack([3 * s3, -4 * s3], axis=1).ravel()
    xg = rng.integers(-64, 65, size=2 * k) / 16.0
    sg = rng.integers(-16, 17, size=2 * k) / 16.0
    q = S - xg - sg
    lam2 = 5 * s3 * 2.0 ** rng.integers(-3, 2, size=k)             # sigma lambda / snorm in {1/16, ..., 1}
    a = orc.prox_group_l2_f32(q, xg, sg, lam2, 0.5, gsize=2)
    b = orc.prox_group_l2(q, xg, sg, lam2, 0.5, gsize=2)
    assert np.array_equal(a.astype(np.float64), b)
    assert fx.same_bits(orc.prox_group_l2_f32(q, xg, sg, lam2, 0.5, gsize=2, y0=q), a)


def test_f32_forms_known_answers(orc, kats):
    K = kats["derived"]["f32_forms"]
    k = K["overflow"]
    t, bad = orc.obj_f32("l1", k["y"], k["x"], k["s"])
    assert not bad and t[0] == np.inf and t[1] == k["l1_terms"][1]
    assert np.isfinite(orc.obj_plain("l1", k["y"], k["x"], k["s"], 1.0))          # the Float64 evaluation differs
    assert nonfinite.sum_class(t) == "+inf"
    k = K["group_1e30_1e-30"]
    t, _, _ = orc.obj_group_f32(k["v"], k["x"], k["s"], k["lambda"], gsize=k["gsize"])
    assert t.tolist() == k["terms"] and all(0 < v < np.inf for v in t)
    with np.errstate(over="ignore", under="ignore"):
        sq32 = np.asarray(k["v"], dtype=F32) ** 2                                   # squares formed in Float32: +Inf and 0
    assert np.all(np.isinf(sq32[:4])) and np.all(sq32[4:] == 0)
    y = orc.prox_group_l2_f32(k["v"], k["x"], k["s"], k["lambda"], k["sigma"], gsize=k["gsize"])
    assert y.astype(np.float64).tolist() == k["prox"]
    k = K["box_slack"]
    t, bad = orc.obj_f32("l1", k["y"], k["x"], k["s"], l=k["l"], u=k["u"])
    assert not bad and k["lambda"] * t[0] == k["psi"]
    assert orc.obj_box("l1", k["y"], k["x"], k["s"], k["lambda"], k["l"], k["u"]) == np.inf   # Float64 slack: infeasible
    assert orc.obj_f32("l1", k["y_below"], k["x"], k["s"], l=k["l"], u=k["u"])[1]
    assert F32(F32(k["s"][0]) + F32(k["y"][0])) == fx.T_LOW and F32(F32(k["s"][0]) + F32(k["y_below"][0])) == fx.down(fx.T_LOW)
    k = K["binf_radius"]
    t, bad = orc.obj_f32("l0", k["y"], k["x"], k["s"], delta=k["delta"])
    assert bad == k["infeasible"] and int(t.sum()) == 1
    tt = F32(F32(k["s"][0]) + F32(k["y"][0]))
    assert float(tt) > 1.1 * k["delta"] and tt <= F32(F32(1.1) * F32(k["delta"])) and tt == fx.T_OUT and F32(k["delta"]) == fx.DELTA


# ---------------------------------------------------------------------------------------------------- the inequality
def _accepts(check, *a, **k):
    try:
        check(*a, **k)
        return True
    except AssertionError:
        return False


def _old_rel(got, ref, tol):
    """the bars this suite had for a Float32 psi(y): 1e-6 relative (test_gpu_redzone), 4 eps32 (test_gpu_f32)"""
    return got == ref or abs(got - ref) <= tol * abs(ref)


def _one_off(d):
    """lambda indexed one group off, where neighbouring lambda are close (the planted 1e-31 and its neighbour stay)"""
    lam = np.roll(d["lam"], 1)
    ge = d["planted"][2]
    lam[ge:ge + 2] = d["lam"][ge:ge + 2]
    return lam


# what the relative bars this replaces (1e-6; 4 eps32) say to each variant: measured on these inputs, asserted below
OLD_BARS_ACCEPT = {"1 dropped": (True, False), "1 twice": (True, False), "2 l1": (True, True), "2 lhalf": (False, False),
                   "3": (True, True), "4 psi": (True, True), "6 psi": (True, True)}


def test_new_bars_reject_planted_mistakes(orc):
    """Seven mistakes, each evaluated as a variant of the restatement on inputs of tests/test_gpu_f32_exact.py; the right answer
    passes the new bar and every variant fails it.  What the bars this replaces said to each (asserted below):

      mistake                                              new bar   1e-6 rel   4 eps32 rel   1e-5 of scale (group prox)
      1  one element dropped / read twice, n = 4 196 353   rejects   accepts    rejects (a)   -
      2  xk + (sj + y) for (xk + sj) + y, NormL1           rejects   accepts    accepts       -
         the same, RootNormLhalf                           rejects   rejects    rejects (b)   -
      3  the L-half square root taken in Float64           rejects   accepts    accepts       -
      4  squares formed in Float32 (psi; the prox norm)    rejects   accepts    accepts       accepts
      5a the Float64 slack 1.49e-8 at the box edge         rejects   rejects    rejects (c)   -
      5b 1.1f * Delta formed in Float32                    rejects   rejects    rejects (c)   -
      6  lambda_g indexed one group off (psi; prox)        rejects   accepts    accepts       accepts
      7  every norm rounded up (the wrong neighbour)       rejects   -          -             accepts
    (a) 5.8e-7 and 5.2e-7 relative: just above 4 eps32 = 4.8e-7, which held at n <= 300 001 only.  (b) the planted exact zeros of
    (xk + sj) + y become ~1e-8 in the other order and their roots ~1e-4: 1e-5 relative.  (c) a finite value against +Inf fails any
    bar -- on THESE inputs; the inputs of the old tests had no element on the edge.
    """
    lam = float(fx.LAM)
    facts = {}

    def old(name, wrong, right):
        """what the two relative bars this replaces say to `wrong` (all the cases of one name together)"""
        a, b = _old_rel(wrong, right, 1e-6), _old_rel(wrong, right, 4 * float(fx.EPS32))
        print("%-10s relative deviation %.3g: 1e-6 %s, 4 eps32 %s" % (name, abs(wrong - right) / abs(right), a, b))
        pa, pb = facts.get(name, (True, True))
        facts[name] = (pa and a, pb and b)

    def psi(terms):
        return lam * math.fsum(terms.tolist())

    # 1: the tail of the last trip past the workgroup cap
    n = fx.SEP_SIZES[-1]
    d = fx.sep_data(n, "plain")
    t, bad = fx.sep_terms(orc, "l1", d)
    assert not bad and _accepts(fx.check_value, psi(t), "l1", t, False, "right")
    p = fx.last_trip_index(n)
    for name, wrong in (("1 dropped", psi(np.delete(t, n - 1))), ("1 twice", psi(np.append(t, t[p])))):
        assert not _accepts(fx.check_value, wrong, "l1", t, False, "1")
        old(name, wrong, psi(t))
    # 2, 3: the order of the additions, the precision of the root (n = 300 001)
    d = fx.sep_data(300_001, "plain")
    for kind in ("l1", "lhalf"):
        t, _ = fx.sep_terms(orc, kind, d)
        t2, _ = orc.obj_f32(kind, d["x"], d["sj"], d["y"])          # (sj + y) + xk == xk + (sj + y)
        assert not np.array_equal(t, t2)
        assert not _accepts(fx.check_value, psi(t2), kind, t, False, "2")
        old("2 " + kind, psi(t2), psi(t))
    t, _ = fx.sep_terms(orc, "lhalf", d)
    t3 = np.sqrt(fx.sep_terms(orc, "l1", d)[0])
    assert not _accepts(fx.check_value, psi(t3), "lhalf", t, False, "3")
    old("3", psi(t3), psi(t))
    # 5a: the Float64 slack finds the element at l - sqrt(eps32) infeasible
    for n in (1, 2049):
        d = fx.sep_data(n, "box")
        l, u, m = fx.box_args(d, "vec-vec-mask")
        t, bad = fx.sep_terms(orc, "l1_box", d, "vec-vec-mask")
        tt = (d["sj"] + d["y"]).astype(np.float64)
        assert not bad and not np.all((l.astype(np.float64) - 1.4901161193847656e-08 <= tt) & (tt <= u.astype(np.float64) + 1.4901161193847656e-08))
        assert not _accepts(fx.check_value, np.inf, "l1_box", t, False, "5a")
        assert _accepts(fx.check_value, psi(t), "l1_box", t, False, "right")
    # 5b: the radius formed in Float32 admits the element one ulp outside
        d = fx.sep_data(n, "binf")
        for poke in d["pokes"]:
            dp = fx.poked(d, poke)
            t, bad = fx.sep_terms(orc, "indball_l0_binf", dp)
            tt = dp["sj"] + dp["y"]
            assert bad and np.all(np.abs(tt) <= F32(F32(1.1) * fx.DELTA))
            assert not _accepts(fx.check_value, 0.0, "indball_l0_binf", t, bad, "5b", r=n)
            assert _accepts(fx.check_value, np.inf, "indball_l0_binf", t, bad, "right", r=n)
    # 4, 6: psi(y) of the group forms
    for lay in fx.group_layouts("obj"):
        if lay[0] not in ("uniform5", "uniform129", "ragged-empty", "trip2-gs3"):
            continue
        d = fx.group_data(lay)
        t, outside, _ = fx.obj_group_terms(orc, lay, d, False)
        right = math.fsum(t.tolist())
        assert _accepts(fx.check_group_value, right, t, outside, "right")
        offs = fx.offsets_of(lay)
        v = orc.obj_f32("l1", d["y"], d["x"], d["sj"])[0].astype(F32)
        with np.errstate(under="ignore"):
            sq = (v * v).astype(np.float64)                          # squares formed in Float32
        ss = np.array([sq[a:b].sum() for a, b in zip(offs[:-1], offs[1:])]) if lay[4] < 5000 else np.add.reduceat(sq, offs[:-1])
        t4 = d["lam"].astype(np.float64) * np.sqrt(ss)
        t6 = fx.obj_group_terms(orc, lay, dict(d, lam=_one_off(d)), False)[0]
        for name, wrong in (("4 psi", math.fsum(t4.tolist())), ("6 psi", math.fsum(t6.tolist()))):
            assert not _accepts(fx.check_group_value, wrong, t, outside, "4/6"), lay[0]
            old(name, wrong, right)
    # 4, 6, 7: the group prox
    for lay in fx.group_layouts("prox"):
        if lay[0] not in ("uniform5", "uniform129", "ragged-empty"):
            continue
        d = fx.group_data(lay)
        offs = fx.offsets_of(lay)
        ref, amb, alts = fx.prox_reference(orc, lay, d)
        assert fx.check_prox(ref, lay, ref, amb, alts, "right") == 0
        kw = dict(offsets=lay[2], gsize=lay[3] if lay[2] is None else 0, y0=d["y0"])
        S = fx.sol_of(d)
        with np.errstate(under="ignore"):
            sq = (S * S).astype(np.float64)
        sn4 = np.sqrt(np.array([sq[a:b].sum() for a, b in zip(offs[:-1], offs[1:])])).astype(F32)
        snorm, _ = fx.census(S, offs)
        sn7 = np.nextafter(snorm, fx.INF32)                         # every norm rounded up: the wrong neighbour in about half
        wrongs = {"4": orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], fx.SIGMA, snorm=sn4, **kw),
                  "6": orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], _one_off(d), fx.SIGMA, snorm=snorm, **kw),
                  "7": orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], fx.SIGMA, snorm=sn7, **kw)}
        scale = np.maximum(np.maximum(np.abs(ref.astype(np.float64)), np.abs(S.astype(np.float64))), 1.0)
        for name, w in wrongs.items():
            assert not fx.same_bits(w, ref), (lay[0], name)
            assert not _accepts(fx.check_prox, w, lay, ref, amb, alts, name), (lay[0], name)
            assert np.all(np.abs(w.astype(np.float64) - ref) <= 1e-5 * scale), (lay[0], name)      # test_gpu_redzone's old bar
    print(facts)
    assert facts == OLD_BARS_ACCEPT


@pytest.mark.parametrize("lay", fx.group_layouts("prox"), ids=[l[0] for l in fx.group_layouts("prox")])
def test_ambiguity_census_within_cap(orc, lay):
    """The groups whose exact norm sits within 1e-12 of a Float32 rounding boundary, from the reference alone: at most
    max(1, ngroups / 1000) per seeded case (the window implies a rate of ~3e-5).  A seed that breaks this is changed, not the cap.
    Outside those groups the restatement's own Float64 norm rounds as the exact norm does."""
    d = fx.group_data(lay)
    offs = fx.offsets_of(lay)
    snorm, amb = fx.census(fx.sol_of(d), offs)
    print("%s: %d groups, %d ambiguous (cap %d)" % (lay[0], lay[4], len(amb), fx.ambiguity_cap(lay[4])))
    assert len(amb) <= fx.ambiguity_cap(lay[4])
    kw = dict(offsets=lay[2], gsize=lay[3] if lay[2] is None else 0, y0=d["y0"])
    own = orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], fx.SIGMA, **kw)
    ref, amb2, alts = fx.prox_reference(orc, lay, d)
    assert set(amb2) == set(amb)
    fx.check_prox(own, lay, ref, amb, alts, lay[0])
    if "planted" in d:                      # the all-zero group, the thresholded one, the 1e-30 one that must not vanish
        gz, gt, ge = d["planted"]
        xs = (d["x"] + d["sj"]).astype(F32)
        assert snorm[gz] == 0 and fx.same_bits(ref[offs[gz]:offs[gz + 1]], (F32(0) - xs)[offs[gz]:offs[gz + 1]])
        assert 0 < snorm[gt] < fx.SIGMA * d["lam"][gt] and np.array_equal(ref[offs[gt]:offs[gt + 1]], -xs[offs[gt]:offs[gt + 1]])
        assert 0 < snorm[ge] < 1e-28 and np.all(ref[offs[ge]:offs[ge + 1]] != 0)


OTHER_GROUP_CASES = [("api-%d" % gs, lambda gs=gs: fx.api_group_case(gs)) for gs in fx.API_GROUP_SIZES] + \
                    [("redzone-" + nm, lambda nm=nm: fx.redzone_group_case(nm)) for nm in fx.REDZONE_GROUP_LAYOUTS]


@pytest.mark.parametrize("make", [m for _, m in OTHER_GROUP_CASES], ids=[i for i, _ in OTHER_GROUP_CASES])
def test_ambiguity_census_of_the_older_group_cases(orc, make):
    """the seeded Float32 group cases of tests/test_gpu_f32.py::test_f32_group_l2 and of tests/test_gpu_redzone.py (grp-f32-*):
    the same cap, from the reference alone; and the restatement's own Float64 norm agrees with the exact one outside the census"""
    lay, d, sigma = make()
    snorm, amb = fx.census(fx.sol_of(d), fx.offsets_of(lay))
    print("%s: %d groups, %d ambiguous (cap %d)" % (lay[0], lay[4], len(amb), fx.ambiguity_cap(lay[4])))
    assert len(amb) <= fx.ambiguity_cap(lay[4])
    ref, amb2, alts = fx.prox_reference(orc, lay, d, sigma=sigma)
    own = orc.prox_group_l2_f32(d["q"], d["x"], d["sj"], d["lam"], sigma, offsets=lay[2], gsize=lay[3] if lay[2] is None else 0)
    fx.check_prox(own, lay, ref, amb, alts, lay[0])


def test_census_flags_a_norm_on_a_rounding_boundary():
    """(3k, 4k) with k = 3 355 445: the norm is 5k = 16 777 225 exactly, an odd integer above 2^24 -- the midpoint of the Float32
    values 16 777 224 and 16 777 226: ambiguous, with those neighbours.  One element moved by an ulp: settled, not ambiguous."""
    k = 3_355_445
    S = np.array([3 * k, 4 * k], dtype=F32)
    assert float(S[0]) == 3 * k and float(S[1]) == 4 * k
    snorm, amb = fx.census(S, np.array([0, 2]))
    assert amb == {0: (F32(5 * k - 1), F32(5 * k + 1))} and snorm[0] in amb[0]
    for step in (-1, 1):
        S2 = np.array([3 * k, 4 * k + step], dtype=F32)
        snorm, amb = fx.census(S2, np.array([0, 2]))
        assert amb == {} and snorm[0] == F32(5 * k + step)          # the norm moves by 0.8: past the midpoint, to that neighbour
    # the same group among others, with an empty group before it and an uncovered tail
    S3 = np.concatenate([[1.0, 2.0, 2.0], S, [7.0]]).astype(F32)
    snorm, amb = fx.census(S3, np.array([0, 3, 3, 5]))
    assert list(amb) == [2] and snorm[0] == 3 and snorm[1] == 0


def test_sanitized_stand_alone_driver():
    """tests/c/oracle_f32_driver.c with oracle/spx_oracle_f32.c under AddressSanitizer + UBSan: a program of its own with
    the sanitizer runtimes linked in (it puts nothing into LD_PRELOAD), run as a child: n = 0, 1, odd n, CSR with empty groups, uncovered head and tail, offsets that break the contract."""
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    libasan = subprocess.run([gcc, "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "f32_driver_asan"])
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "oracle", "_asan", "oracle_f32_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
