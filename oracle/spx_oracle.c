/*
 * spx_oracle.c -- CPU restatement of the ShiftedProximalOperators.jl prox!() hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load it.  The product (libspx, HIP) never links,
 * loads or calls anything in oracle/.
 *
 * What it is: a single-threaded, literal restatement in plain C of the reference's Julia
 * prox! bodies (reference v0.2.2 under /root/reference, cited per function as file:line),
 * keeping the reference's floating-point association, branch order and tie-breaking.
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math (see oracle/Makefile) so no FMA contraction
 * or reassociation happens -- Julia does neither.
 *
 * Pinning status.  The reference is Julia; no Julia toolchain exists in
 * this image, so the reference itself cannot be run.  The oracle is pinned against every
 * known-answer vector the reference's own tests hold for this path (tests/golden/,
 * transcribed from test/runtests.jl:113-126,449-494,587-606,658-705 and
 * test/testsbox.jl:13-97, test/partial_prox.jl:14-39):
 *   pinned   : ShiftedNormL0Box, ShiftedNormL1Box, ShiftedRootNormLhalfBox,
 *              ShiftedGroupNormL2 (property vs NormL2 prox), ShiftedGroupNormL2Binf,
 *              RootNormLhalf (unshifted).
 *   PARITY UNPINNED by the reference's tests (source text is the only authority):
 *              ShiftedNormL0, ShiftedNormL1, ShiftedRootNormLhalf (unboxed; the boxed
 *              goldens with an inactive box do pin the same closed forms indirectly),
 *              ShiftedIndBallL0, ShiftedIndBallL0BInf (sortperm tie-break = stable,
 *              descending |v|, ties by ascending index).
 *
 * Third-party arithmetic restated here (not in /root/reference):
 *   - Roots.jl `fzero(f, a, b)` (compat "^1.0.0", unpinned; Project.toml:17): bracketing
 *     bisection on Float64 run to floating-point exhaustion.  Restated as orc_bisect().
 *   - LinearAlgebra.norm: 2-norm; summation order unspecified (BLAS dnrm2 for long
 *     contiguous views).  Restated as a plain left-to-right sum of squares + sqrt.  The
 *     restatement is NOT overflow-safe (LinearAlgebra.norm rescales, this sum does not): it is
 *     the reference's value only while every square and the sum are finite normal doubles, and
 *     the scale tests (tests/scales.py) therefore stop at 2^+-500.
 *   - Base.sortperm!(p, y, rev=true, by=abs): stable.  Restated as a stable merge sort.
 *   - Base min/max on Float64: IEEE-754-2019 minimum/maximum (-0.0 < +0.0, NaN propagates).
 *   - Base complex acos/cos, real ^, cos, acos, sqrt: libm (glibc) here; ulp-level differences
 *     vs Julia's pure-Julia libm are inside the 1e-12 relative tolerance of those operators.
 */
#define _GNU_SOURCE
#include <complex.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORC_API __attribute__((visibility("default")))

/* ---- sensitivity probes (tests/arbiter.py only; both default to 0 = the literal restatement) ----------------------------
 * The reference's result depends on third-party arithmetic it does not pin: LinearAlgebra.norm (BLAS dnrm2 for long
 * contiguous views, a generic loop otherwise: summation order and scaling unspecified, a few ulp apart) and the last ulp of
 * libm's `^` (Julia's own pow vs glibc's).  So "the reference's Float64 value" is an ensemble, not one number.  With
 * orc_set_perturbation(kn, kp) every norm2() result is moved by kn ulps and every pow() result of the RootNormLhalf closed
 * forms by kp ulps: running the oracle at (0,0), (+k,+k'), (-k,-k') samples that ensemble, and the arbiter accepts a HIP
 * result that is no further from the binary128 value than its worst member. */
static int g_norm_ulps = 0, g_pow_ulps = 0;
ORC_API void orc_set_perturbation(int norm_ulps, int pow_ulps) { g_norm_ulps = norm_ulps; g_pow_ulps = pow_ulps; }
static inline double nudge(double v, int ulps) {
  if (ulps == 0 || !(v == v) || isinf(v)) return v;
  for (int k = 0; k < (ulps < 0 ? -ulps : ulps); ++k) v = nextafter(v, ulps > 0 ? INFINITY : -INFINITY);
  return v;
}
static inline double orc_pow(double x, double y) { return nudge(pow(x, y), g_pow_ulps); }

/* ---- Julia Base.min / Base.max for Float64 (base/math.jl): sign of x - y picks the argument,
 *      so -0.0 < +0.0; NaN in either argument propagates. ---- */
static inline double jl_min(double x, double y) {
  double d = x - y;
  double a = signbit(d) ? x : y;
  return (isnan(x) || isnan(y)) ? d : a;
}
static inline double jl_max(double x, double y) {
  double d = x - y;
  double a = signbit(d) ? y : x;
  return (isnan(x) || isnan(y)) ? d : a;
}
/* Julia sign(x): x for +-0.0 and NaN, else +-1.0 */
static inline double jl_sign(double x) { return (x > 0.0) ? 1.0 : (x < 0.0) ? -1.0 : x; }

/* prox_zero, src/ShiftedProximalOperators.jl:203 */
static inline double prox_zero(double q, double l, double u) { return jl_min(jl_max(q, l), u); }

static inline int is_selected(const uint8_t* mask, int64_t i) { return mask == NULL || mask[i] != 0; }

/* ------------------------------------------------------------------------------------------
 * ShiftedNormL1.prox!  src/shiftedNormL1.jl:40-54
 *   pass 1 (:47)   y = (-xk) - sj
 *   pass 2 (:49-51) y[i] = min(max(y[i], q[i] - lambda*sigma), q[i] + lambda*sigma)
 * Two passes on purpose: if y aliases q the broadcast overwrites q before the loop reads it,
 * exactly as in the reference.
 * ------------------------------------------------------------------------------------------ */
ORC_API void orc_prox_l1(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                         double lambda, double sigma) {
  for (int64_t i = 0; i < n; ++i) y[i] = (-xk[i]) - sj[i];
  for (int64_t i = 0; i < n; ++i) {
    double qi = q[i];
    y[i] = jl_min(jl_max(y[i], qi - lambda * sigma), qi + lambda * sigma);
  }
}

/* ------------------------------------------------------------------------------------------
 * ShiftedNormL1Box.prox!  src/shiftedNormL1Box.jl:89-125
 * l/u: vector if non-NULL else the scalar; mask: byte per index, NULL = every index selected.
 * ------------------------------------------------------------------------------------------ */
ORC_API void orc_prox_l1_box(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                             double lambda, double sigma, const double* lvec, const double* uvec,
                             double lscal, double uscal, const uint8_t* mask) {
  const double sl = sigma * lambda; /* :96 */
  for (int64_t i = 0; i < n; ++i) {
    double li = lvec ? lvec[i] : lscal;
    double ui = uvec ? uvec[i] : uscal;
    double qi = q[i];
    double si = sj[i];
    if (is_selected(mask, i)) {
      double xi = xk[i];
      double xs = xi + si;
      double xsq = xs + qi;
      double t;
      if (xsq <= -sl) t = qi + sl;
      else if (xsq >= sl) t = qi - sl;
      else t = -xs;
      y[i] = jl_min(jl_max(t, li - si), ui - si); /* :118 */
    } else {
      y[i] = prox_zero(qi, li - si, ui - si); /* :121 */
    }
  }
}

/* The same loop spread over `threads` host threads (OpenMP, static contiguous chunks): NOT the reference -- which is
 * single-threaded Julia -- but a generous upper bound for what the host CPU could do on this memory-bound loop; reported
 * by bench.py next to the single-thread figure and labelled as such ("optionally an OpenMP all-core variant").
 * Results are bit-identical to orc_prox_l1_box (elements are independent). */
ORC_API void orc_prox_l1_box_mt(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                double lambda, double sigma, const double* lvec, const double* uvec,
                                double lscal, double uscal, const uint8_t* mask, int threads) {
  if (threads < 1) threads = 1;
#pragma omp parallel for num_threads(threads) schedule(static)
  for (int64_t c = 0; c < threads; ++c) {
    const int64_t lo = n / threads * c + (c < n % threads ? c : n % threads);
    const int64_t len = n / threads + (c < n % threads ? 1 : 0);
    orc_prox_l1_box(y + lo, q + lo, xk + lo, sj + lo, len, lambda, sigma, lvec ? lvec + lo : NULL, uvec ? uvec + lo : NULL,
                    lscal, uscal, mask ? mask + lo : NULL);
  }
}

/* ------------------------------------------------------------------------------------------
 * ShiftedNormL0.prox!  src/shiftedNormL0.jl:38-55
 * ------------------------------------------------------------------------------------------ */
ORC_API void orc_prox_l0(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                         double lambda, double sigma) {
  const double c = sqrt(2 * lambda * sigma); /* :45 */
  for (int64_t i = 0; i < n; ++i) {
    double xps = xk[i] + sj[i];
    double qi = q[i];
    y[i] = (fabs(xps + qi) <= c) ? -xps : qi;
  }
}

/* ------------------------------------------------------------------------------------------
 * ShiftedNormL0Box.prox!  src/shiftedNormL0Box.jl:89-131
 * ------------------------------------------------------------------------------------------ */
ORC_API void orc_prox_l0_box(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                             double lambda, double sigma, const double* lvec, const double* uvec,
                             double lscal, double uscal, const uint8_t* mask) {
  const double c = 2 * lambda * sigma; /* :96 */
  for (int64_t i = 0; i < n; ++i) {
    double li = lvec ? lvec[i] : lscal;
    double ui = uvec ? uvec[i] : uscal;
    double qi = q[i];
    double si = sj[i];
    double sq = si + qi;
    if (is_selected(mask, i)) {
      double xi = xk[i];
      double xs = xi + si;
      double xsq = xs + qi;
      double dl = li - sq, du = ui - sq;
      double val_left = dl * dl + ((xi == -li) ? 0.0 : c);  /* :110 */
      double val_right = du * du + ((xi == -ui) ? 0.0 : c); /* :111 */
      double yi = (val_left < val_right) ? (li - si) : (ui - si); /* :114 */
      double val_min = jl_min(val_left, val_right);
      double mxi = -xi;
      if (li <= mxi && mxi <= ui) { /* :116 */
        double val_0 = xsq * xsq;
        if (val_0 < val_min) yi = -xs;
        val_min = jl_min(val_0, val_min);
      }
      if (li <= sq && sq <= ui) { /* :121 */
        double val_xsq = (xsq == 0.0) ? 0.0 : c;
        if (val_xsq < val_min) yi = qi;
      }
      y[i] = yi;
    } else {
      y[i] = prox_zero(qi, li - si, ui - si); /* :127 */
    }
  }
}

/* ------------------------------------------------------------------------------------------
 * RootNormLhalf.prox! (unshifted)  src/rootNormLhalf.jl:31-51.  Returns lambda * sum sqrt|y|.
 * ------------------------------------------------------------------------------------------ */
ORC_API double orc_rootnormlhalf_prox(double* y, const double* x, int64_t n, double lambda, double gamma) {
  const double gl = gamma * lambda;
  const double threshold = pow(54.0, 1.0 / 3.0) * pow(2 * gl, 2.0 / 3.0) / 4; /* :40 */
  double ysum = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    double xi = x[i];
    if (fabs(xi) <= threshold) {
      y[i] = 0.0;
    } else {
      double phi = acos(gl / 4 * pow(fabs(xi) / 3, -3.0 / 2.0)); /* :38 */
      y[i] = 2 * jl_sign(xi) / 3 * fabs(xi) * (1 + cos(2 * M_PI / 3 - 2 * phi / 3)); /* :45 */
      ysum += sqrt(fabs(y[i]));
    }
  }
  return lambda * ysum;
}

/* ------------------------------------------------------------------------------------------
 * ShiftedRootNormLhalf.prox!  src/shiftedRootNormLhalf.jl:41-63
 *   sol = q + (xk + sj) (:50); threshold p (:49); closed form (:57); y -= (xk + sj) (:59)
 * ------------------------------------------------------------------------------------------ */
ORC_API void orc_prox_lhalf(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                            double lambda, double sigma) {
  const double nl = sigma * lambda;                                             /* :47 */
  const double p = pow(54.0, 1.0 / 3.0) * pow(2 * nl, 2.0 / 3.0) / 4;           /* :49 */
  for (int64_t i = 0; i < n; ++i) {
    double xs = xk[i] + sj[i];
    double sol = q[i] + xs;
    double aqi = fabs(sol);
    double yi;
    if (aqi <= p) {
      yi = 0.0;
    } else {
      double phi = acos(nl / 4 * orc_pow(fabs(sol) / 3, -3.0 / 2.0));            /* :48 */
      yi = 2 * jl_sign(sol) / 3 * aqi * (1 + cos(2 * M_PI / 3 - 2 * phi / 3));   /* :57 */
    }
    y[i] = yi - xs;
  }
}

/* ------------------------------------------------------------------------------------------
 * ShiftedRootNormLhalfBox.prox!  src/shiftedRootNormLhalfBox.jl:86-120
 * Complex acos (:92) -> real part (:106); four candidates, findmin = first minimum (:108-114),
 * NaN counts as minimal in Julia's findmin (isless(NaN, x) is false but findmin treats NaN as
 * the minimum); with finite inputs only candidate 4 can be NaN-derived and it is replaced by
 * Inf because `li <= NaN <= ui` is false.
 * ------------------------------------------------------------------------------------------ */
static inline double rnorm_obj(double tt, double qi, double sigma, double lambda, double xs) {
  double d = tt - qi;
  return d * d / 2 / sigma + lambda * sqrt(fabs(tt + xs)); /* :95 */
}

ORC_API void orc_prox_lhalf_box(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                double lambda, double sigma, const double* lvec, const double* uvec,
                                double lscal, double uscal, const uint8_t* mask) {
  const double twopi3 = 2 * M_PI / 3;
  for (int64_t i = 0; i < n; ++i) {
    double li = lvec ? lvec[i] : lscal;
    double ui = uvec ? uvec[i] : uscal;
    double xi = xk[i];
    double si = sj[i];
    double qi = q[i];
    if (is_selected(mask, i)) {
      double xs = xi + si; /* :94 */
      double xsq = xs + qi;
      double a = sigma * lambda / 4 * orc_pow(fabs(xsq) / 3, -3.0 / 2.0);
      double complex phi = cacos(a + 0.0 * I); /* :92 */
      double complex ang = (twopi3 - creal(2 * phi / 3)) + (-cimag(2 * phi / 3)) * I;
      double complex cs = ccos(ang);
      double val = (2 * jl_sign(xsq) / 3 * fabs(xsq)) * (1 + creal(cs)); /* :106 */

      double cand[4];
      cand[0] = rnorm_obj(li - si, qi, sigma, lambda, xs);
      cand[1] = rnorm_obj(ui - si, qi, sigma, lambda, xs);
      double mxi = -xi;
      cand[2] = (li <= mxi && mxi <= ui) ? rnorm_obj(-xs, qi, sigma, lambda, xs) : INFINITY;
      double vx = val - xi;
      cand[3] = (li <= vx && vx <= ui) ? rnorm_obj(val - xs, qi, sigma, lambda, xs) : INFINITY;
      int a_idx = 0;
      double best = cand[0];
      for (int k = 1; k < 4; ++k) {
        /* Julia findmin: first minimum; a NaN entry wins over numbers */
        if ((cand[k] < best) || (isnan(cand[k]) && !isnan(best))) { best = cand[k]; a_idx = k; }
      }
      y[i] = (a_idx == 0) ? (li - si) : (a_idx == 1) ? (ui - si) : (a_idx == 2) ? -xs : (val - xs); /* :114 */
    } else {
      y[i] = prox_zero(qi, li - si, ui - si); /* :116 */
    }
  }
}

/* ------------------------------------------------------------------------------------------
 * sortperm!(p, y, rev=true, by=abs): stable permutation, descending |y|, ties ascending index.
 * Stable bottom-up merge sort of indices.
 * ------------------------------------------------------------------------------------------ */
static inline int jl_isless(double x, double y) { /* Base.isless on Float64 (non-negative arguments here) */
  if (x != x) return 0;
  if (y != y) return 1;
  return x < y;
}
static void stable_sortperm_desc_abs(int64_t* p, const double* y, int64_t n) {
  int64_t* tmp = (int64_t*)malloc((size_t)n * sizeof(int64_t));
  for (int64_t i = 0; i < n; ++i) p[i] = i;
  int64_t* src = p;
  int64_t* dst = tmp;
  for (int64_t w = 1; w < n; w *= 2) {
    for (int64_t lo = 0; lo < n; lo += 2 * w) {
      int64_t mid = lo + w < n ? lo + w : n;
      int64_t hi = lo + 2 * w < n ? lo + 2 * w : n;
      int64_t a = lo, b = mid, k = lo;
      while (a < mid && b < hi) {
        /* take from the right run only if strictly larger in |.| (keeps stability); "larger" in Julia's total order
         * isless (the `lt` of sort): a NaN is greater than everything, NaNs are equal among themselves */
        if (jl_isless(fabs(y[src[a]]), fabs(y[src[b]]))) dst[k++] = src[b++];
        else dst[k++] = src[a++];
      }
      while (a < mid) dst[k++] = src[a++];
      while (b < hi) dst[k++] = src[b++];
    }
    int64_t* t = src; src = dst; dst = t;
  }
  if (src != p) memcpy(p, src, (size_t)n * sizeof(int64_t));
  free(tmp);
}

/* ShiftedIndBallL0.prox!  src/shiftedIndBallL0.jl:54-72 */
ORC_API void orc_prox_indball_l0(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                 int64_t r) {
  for (int64_t i = 0; i < n; ++i) y[i] = (xk[i] + sj[i]) + q[i]; /* :66 */
  int64_t* p = (int64_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int64_t));
  stable_sortperm_desc_abs(p, y, n);                             /* :68 */
  for (int64_t k = (r < 0 ? 0 : r); k < n; ++k) y[p[k]] = 0.0;   /* :69 */
  for (int64_t i = 0; i < n; ++i) y[i] = y[i] - (xk[i] + sj[i]); /* :70 */
  free(p);
}

/* ShiftedIndBallL0BInf.prox!  src/shiftedIndBallL0BInf.jl:73-95 (clamps t, not s+t) */
ORC_API void orc_prox_indball_l0_binf(double* y, const double* q, const double* xk, const double* sj,
                                      int64_t n, int64_t r, double delta) {
  for (int64_t i = 0; i < n; ++i) y[i] = (xk[i] + sj[i]) + q[i]; /* :85 */
  int64_t* p = (int64_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int64_t));
  stable_sortperm_desc_abs(p, y, n);                             /* :87 */
  for (int64_t k = (r < 0 ? 0 : r); k < n; ++k) y[p[k]] = 0.0;   /* :88 */
  for (int64_t i = 0; i < n; ++i)                                /* :90-92 */
    y[i] = jl_min(jl_max(y[i] - (xk[i] + sj[i]), -delta), delta);
  free(p);
}

/* The same two operators with the permutation of :68 / :87 handed in: tests that evaluate many r on one (q, xk, sj) sort once
 * (the sort is most of the oracle's time; the permutation does not depend on r).  p = orc_sortperm_indball(...). */
ORC_API void orc_sortperm_indball(int64_t* p, const double* q, const double* xk, const double* sj, int64_t n) {
  double* v = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  for (int64_t i = 0; i < n; ++i) v[i] = (xk[i] + sj[i]) + q[i]; /* :66 / :85 */
  stable_sortperm_desc_abs(p, v, n);                             /* :68 / :87 */
  free(v);
}
ORC_API void orc_prox_indball_l0_perm(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                      const int64_t* p, int64_t r, double delta, int binf) {
  for (int64_t i = 0; i < n; ++i) y[i] = (xk[i] + sj[i]) + q[i];
  for (int64_t k = (r < 0 ? 0 : r); k < n; ++k) y[p[k]] = 0.0;   /* :69 / :88 */
  if (binf) {
    for (int64_t i = 0; i < n; ++i) y[i] = jl_min(jl_max(y[i] - (xk[i] + sj[i]), -delta), delta); /* :90-92 */
  } else {
    for (int64_t i = 0; i < n; ++i) y[i] = y[i] - (xk[i] + sj[i]); /* :70 */
  }
}

/* ------------------------------------------------------------------------------------------
 * Groups: contiguous index ranges.  offsets != NULL: group g = [offsets[g], offsets[g+1]) (0-based);
 * offsets == NULL: uniform groups of `gsize`, group g = [g*gsize, (g+1)*gsize).
 * ------------------------------------------------------------------------------------------ */
static inline void group_range(const int64_t* offsets, int64_t gsize, int64_t g, int64_t* lo, int64_t* hi) {
  if (offsets) { *lo = offsets[g]; *hi = offsets[g + 1]; }
  else { *lo = g * gsize; *hi = (g + 1) * gsize; }
}
static double norm2(const double* v, int64_t m) {
  double s = 0.0;
  for (int64_t i = 0; i < m; ++i) s += v[i] * v[i];
  return nudge(sqrt(s), g_norm_ulps);
}

/* ShiftedGroupNormL2.prox!  src/shiftedGroupNormL2.jl:52-79.
 * As in the reference, an index covered by no group ends as (y on entry) - (xk + sj) (:77 runs over
 * every index); callers are expected to pass groups that partition 1:n. */
ORC_API void orc_prox_group_l2(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                               const int64_t* offsets, int64_t gsize, int64_t ngroups, const double* lambda,
                               double sigma) {
  double* sol = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  for (int64_t i = 0; i < n; ++i) sol[i] = (q[i] + xk[i]) + sj[i]; /* :65 */
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t lo, hi;
    group_range(offsets, gsize, g, &lo, &hi);
    double snorm = norm2(sol + lo, hi - lo); /* :69 */
    if (snorm == 0) {
      for (int64_t i = lo; i < hi; ++i) y[i] = 0.0;
    } else {
      double alpha = jl_max(1 - sigma * lambda[g] / snorm, 0.0); /* :73 */
      for (int64_t i = lo; i < hi; ++i) y[i] = alpha * sol[i];
    }
  }
  for (int64_t i = 0; i < n; ++i) y[i] = y[i] - (xk[i] + sj[i]); /* :77 */
  free(sol);
}

/* ---- ShiftedGroupNormL2Binf helpers (src/shiftedGroupNormL2Binf.jl:82-93) ---- */
typedef struct {
  const double* S; /* sol[idx] */
  const double* X; /* xk[idx] */
  int64_t m;
  double sigma, sl, delta;
  double* w; /* scratch, length m */
} froot_ctx;

static inline double softthres(double x, double a) { return jl_sign(x) * jl_max(0.0, fabs(x) - a); } /* :82 */

static double froot(const froot_ctx* c, double nn) { /* :87-93 */
  double step = nn / (c->sigma * (nn - c->sl));
  for (int64_t i = 0; i < c->m; ++i)
    c->w[i] = c->sigma * softthres(c->S[i] / c->sigma - step * c->X[i], c->delta * step) - c->S[i];
  return nn - norm2(c->w, c->m);
}

/* Roots.fzero(f, a, b) = find_zero(f, (a, b), Bisection()) [ext, Roots.jl ^1.0, unpinned]:
 *   - the bracket is SORTED first (the reference can hand over lmin > lmax when
 *     ||S|| + sigma (zlmax + lambda ||X||) < sigma lambda);
 *   - midpoint = Roots' __middle: the double whose bit pattern is the mean of the two bit patterns;
 *   - `sign(fa) * sign(fc) < 0 ? b = c : a = c` (a NaN value therefore moves the lower end);
 *   - stops when no double lies strictly between a and b and returns the end with the smaller |f|
 *     (`abs(fa) < abs(fb) ? a : b`, so a NaN fa yields b).
 * A sorted bracket with lmax < sigma*lambda straddles the pole of step(n) at n = sigma*lambda; the
 * iteration then converges onto the pole from the right-hand side exactly as a sign-bisection does. */
static double bit_middle(double x, double y) {
  uint64_t xi, yi;
  double ax = fabs(x), ay = fabs(y);
  memcpy(&xi, &ax, 8);
  memcpy(&yi, &ay, 8);
  uint64_t mid = (xi + yi) >> 1;
  double m;
  memcpy(&m, &mid, 8);
  return jl_sign(x + y) * m;
}
static double orc_bisect(const froot_ctx* c, double a, double fa, double b, double fb) {
  if (a > b) { double t = a; a = b; b = t; t = fa; fa = fb; fb = t; }
  if (fa == 0.0) return a;
  if (fb == 0.0) return b;
  for (int it = 0; it < 4096; ++it) {
    double m = bit_middle(a, b);
    if (!(a < m && m < b)) break;
    double fm = froot(c, m);
    if (jl_sign(fa) * jl_sign(fm) < 0) { b = m; fb = fm; }
    else { a = m; fa = fm; }
  }
  return (fabs(fa) < fabs(fb)) ? a : b;
}

/* ShiftedGroupNormL2Binf.prox!  src/shiftedGroupNormL2Binf.jl:67-119 */
ORC_API void orc_prox_group_l2_binf(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                    const int64_t* offsets, int64_t gsize, int64_t ngroups,
                                    const double* lambda, double sigma, double delta) {
  double* sol = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  double* w = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  for (int64_t i = 0; i < n; ++i) sol[i] = (q[i] + xk[i]) + sj[i]; /* :80 */
  const double eps = 2.220446049250313e-16;
  const double epsilon = 1.0; /* :81 */
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t lo, hi;
    group_range(offsets, gsize, g, &lo, &hi);
    int64_t m = hi - lo;
    double lam = lambda[g];
    double sl = lam * sigma; /* :85 */
    froot_ctx c = {sol + lo, xk + lo, m, sigma, sl, delta, w};
    double lmin = sl * (1 + eps); /* :94 */
    double fl = froot(&c, lmin);
    double ansatz = lmin + epsilon; /* :97 */
    double step = ansatz / (sigma * (ansatz - sl));
    for (int64_t i = 0; i < m; ++i) w[i] = softthres(c.S[i] / sigma - step * c.X[i], delta * step);
    double zlmax = norm2(w, m); /* :99 */
    double lmax = norm2(c.S, m) + sigma * (zlmax + fabs((epsilon - 1) / epsilon + 1) * lam * norm2(c.X, m)); /* :100 */
    double fm = froot(&c, lmax);
    if (fl * fm > 0) { /* :102 */
      for (int64_t i = lo; i < hi; ++i) y[i] = 0.0;
    } else {
      double nn = orc_bisect(&c, lmin, fl, lmax, fm); /* :105 */
      step = nn / (sigma * (nn - sl));
      if (fabs(nn - sl) == 0.0) { /* :107, isapprox(x, 0) with atol = 0 <=> x == 0 */
        for (int64_t i = lo; i < hi; ++i) y[i] = 0.0;
      } else {
        for (int64_t i = 0; i < m; ++i)
          w[i] = c.S[i] - sigma * softthres(c.S[i] / sigma - step * c.X[i], delta * step); /* :111 */
        double nw = norm2(w, m);
        double alpha = jl_max(0.0, 1 - sl / nw); /* :83 */
        for (int64_t i = 0; i < m; ++i) y[lo + i] = alpha * w[i];
      }
    }
    for (int64_t i = lo; i < hi; ++i) y[i] = y[i] - (xk[i] + sj[i]); /* :116 */
  }
  free(sol);
  free(w);
}

/* ---- the same two operators on arbitrary index sets (idx::Vector{Vector{Int}}, src/groupNormL2.jl:30-31,
 * test/runtests.jl:290): group g = index[ptr[g] .. ptr[g+1]) (0-based).  Literal: groups are processed in order, so an
 * index listed by several groups keeps the LAST group's value; an index in no group keeps y on entry, minus the
 * shift for ShiftedGroupNormL2 (:77 runs over every index) and untouched for the Binf form (:116 is per group). */
ORC_API void orc_prox_group_l2_idx(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                   const int64_t* ptr, const int64_t* index, int64_t ngroups, const double* lambda,
                                   double sigma) {
  double* sol = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  for (int64_t i = 0; i < n; ++i) sol[i] = (q[i] + xk[i]) + sj[i]; /* :65 */
  for (int64_t g = 0; g < ngroups; ++g) {
    double ss = 0.0;
    for (int64_t p = ptr[g]; p < ptr[g + 1]; ++p) ss += sol[index[p]] * sol[index[p]];
    double snorm = sqrt(ss); /* :69 */
    if (snorm == 0) {
      for (int64_t p = ptr[g]; p < ptr[g + 1]; ++p) y[index[p]] = 0.0;
    } else {
      double alpha = jl_max(1 - sigma * lambda[g] / snorm, 0.0); /* :73 */
      for (int64_t p = ptr[g]; p < ptr[g + 1]; ++p) y[index[p]] = alpha * sol[index[p]];
    }
  }
  for (int64_t i = 0; i < n; ++i) y[i] = y[i] - (xk[i] + sj[i]); /* :77 */
  free(sol);
}

ORC_API void orc_prox_group_l2_binf_idx(double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                        const int64_t* ptr, const int64_t* index, int64_t ngroups,
                                        const double* lambda, double sigma, double delta) {
  int64_t mmax = 1;
  for (int64_t g = 0; g < ngroups; ++g)
    if (ptr[g + 1] - ptr[g] > mmax) mmax = ptr[g + 1] - ptr[g];
  double* sol = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
  double* S = (double*)malloc((size_t)mmax * sizeof(double));
  double* X = (double*)malloc((size_t)mmax * sizeof(double));
  double* w = (double*)malloc((size_t)mmax * sizeof(double));
  for (int64_t i = 0; i < n; ++i) sol[i] = (q[i] + xk[i]) + sj[i]; /* :80 */
  const double eps = 2.220446049250313e-16;
  const double epsilon = 1.0; /* :81 */
  for (int64_t g = 0; g < ngroups; ++g) {
    const int64_t* idx = index + ptr[g];
    int64_t m = ptr[g + 1] - ptr[g];
    for (int64_t i = 0; i < m; ++i) { S[i] = sol[idx[i]]; X[i] = xk[idx[i]]; }
    double lam = lambda[g];
    double sl = lam * sigma; /* :85 */
    froot_ctx c = {S, X, m, sigma, sl, delta, w};
    double lmin = sl * (1 + eps); /* :94 */
    double fl = froot(&c, lmin);
    double ansatz = lmin + epsilon; /* :97 */
    double step = ansatz / (sigma * (ansatz - sl));
    for (int64_t i = 0; i < m; ++i) w[i] = softthres(S[i] / sigma - step * X[i], delta * step);
    double zlmax = norm2(w, m); /* :99 */
    double lmax = norm2(S, m) + sigma * (zlmax + fabs((epsilon - 1) / epsilon + 1) * lam * norm2(X, m)); /* :100 */
    double fm = froot(&c, lmax);
    if (fl * fm > 0) { /* :102 */
      for (int64_t i = 0; i < m; ++i) y[idx[i]] = 0.0;
    } else {
      double nn = orc_bisect(&c, lmin, fl, lmax, fm); /* :105 */
      step = nn / (sigma * (nn - sl));
      if (fabs(nn - sl) == 0.0) { /* :107 */
        for (int64_t i = 0; i < m; ++i) y[idx[i]] = 0.0;
      } else {
        for (int64_t i = 0; i < m; ++i) w[i] = S[i] - sigma * softthres(S[i] / sigma - step * X[i], delta * step); /* :111 */
        double nw = norm2(w, m);
        double alpha = jl_max(0.0, 1 - sl / nw); /* :83 */
        for (int64_t i = 0; i < m; ++i) y[idx[i]] = alpha * w[i];
      }
    }
    /* :116  y[idx] .-= (xk[idx] + sj[idx]): gather, subtract, scatter (a repeated index is subtracted once) */
    for (int64_t i = 0; i < m; ++i) w[i] = y[idx[i]] - (xk[idx[i]] + sj[idx[i]]);
    for (int64_t i = 0; i < m; ++i) y[idx[i]] = w[i];
  }
  free(sol); free(S); free(X); free(w);
}

/* ==========================================================================================
 * iprox!  (SURVEY.md 8f rank 1): indefinite prox  argmin 1/2 y'Dy + g'y + psi(y), D = diag(d)
 * ========================================================================================== */

/* iprox_zero(d, g, l, u)  src/ShiftedProximalOperators.jl:217-236 */
static inline double iprox_zero(double d, double g, double l, double u) {
  const double eps = 2.220446049250313e-16;
  if (d > eps) {
    double argmin_quad = -g / d;
    return jl_min(jl_max(argmin_quad, l), u);
  } else if (d < -eps) {
    double d_2 = d / 2;
    double val_l = d_2 * (l * l) + g * l;
    double val_u = d_2 * (u * u) + g * u;
    return (val_l < val_u) ? l : u;
  } else {
    if (g > 0.0) return l;
    if (g < 0.0) return u;
    return 0.0;
  }
}

/* ShiftedNormL1.iprox!  src/shiftedNormL1.jl:60-75.  Returns -1, or the (0-based) index of the first element
 * with d[i] <= 0, where the reference's `@assert d[i] > 0` throws (entries before it are already written). */
ORC_API int64_t orc_iprox_l1(double* y, const double* g, const double* d, const double* xk, const double* sj,
                             int64_t n, double lambda) {
  for (int64_t i = 0; i < n; ++i) y[i] = (-xk[i]) - sj[i]; /* :67 */
  for (int64_t i = 0; i < n; ++i) {
    if (!(d[i] > 0)) return i; /* :70 */
    y[i] = jl_min(jl_max(y[i], -g[i] / d[i] - lambda / d[i]), -g[i] / d[i] + lambda / d[i]); /* :71 */
  }
  return -1;
}

/* ShiftedNormL0.iprox!  src/shiftedNormL0.jl:61-80 */
ORC_API int64_t orc_iprox_l0(double* y, const double* g, const double* d, const double* xk, const double* sj,
                             int64_t n, double lambda) {
  for (int64_t i = 0; i < n; ++i) {
    double di = d[i];
    if (!(di > 0)) return i; /* :70 */
    double ci = sqrt(2 * lambda * di);
    double xps = xk[i] + sj[i];
    y[i] = (fabs(di * xps - g[i]) <= ci) ? -xps : (-g[i] / di);
  }
  return -1;
}

/* ShiftedNormL1Box.iprox!  src/shiftedNormL1Box.jl:131-225 */
ORC_API void orc_iprox_l1_box(double* y, const double* g, const double* d, const double* xk, const double* sj,
                              int64_t n, double lambda, const double* lvec, const double* uvec, double lscal,
                              double uscal, const uint8_t* mask) {
  const double eps = 2.220446049250313e-16;
  for (int64_t i = 0; i < n; ++i) {
    double li = lvec ? lvec[i] : lscal;
    double ui = uvec ? uvec[i] : uscal;
    double di = d[i], gi = g[i], si = sj[i], xi = xk[i];
    double xs = xi + si;
    if (!is_selected(mask, i)) { y[i] = iprox_zero(di, gi, li - si, ui - si); continue; } /* :221 */
    double left = li - si, right = ui - si;
    double yi;
    if (fabs(di) <= eps) { /* :152 */
      if (fabs(gi) <= lambda) yi = jl_min(jl_max(left, -xs), right);
      else yi = (gi > 0) ? left : right;
    } else if (di > eps) { /* :161 */
      double di_2 = di / 2;
      double lx = li + xi, ux = ui + xi;
      double gi2_di = gi / di_2;
      double fi2_di = gi2_di - 2 * xs;
      double l2_di = lambda / di_2;
      double val_left = lx * lx + fi2_di * lx + l2_di * fabs(lx);
      double val_right = ux * ux + fi2_di * ux + l2_di * fabs(ux);
      double val_min = jl_min(val_left, val_right);
      yi = (val_left < val_right) ? left : right;
      if (lx >= 0.0) {
        double a = -(gi + lambda) / di;
        if (left <= a && a <= right) yi = a;
      } else if (0.0 >= ux) {
        double a = (lambda - gi) / di;
        if (left <= a && a <= right) yi = a;
      } else {
        double y1 = -(gi + lambda) / di;
        double y2 = (lambda - gi) / di;
        if (left <= y1 && y1 <= right) {
          double v1 = xs + y1;
          double q1 = v1 * v1 + fi2_di * v1 + l2_di * fabs(v1);
          if (q1 < val_min) yi = y1;
          val_min = jl_min(q1, val_min);
        }
        if (left <= y2 && y2 <= right) {
          double v2 = xs + y2;
          double q2 = v2 * v2 + fi2_di * v2 + l2_di * fabs(v2);
          if (q2 < val_min) yi = y2;
          val_min = jl_min(q2, val_min);
        }
        if (0.0 < val_min) yi = -xs; /* val_0 = 0 */
      }
    } else { /* di <= -eps, :199 */
      double di_2 = di / 2;
      double gi2_di = gi / di_2;
      double fi2_di = gi2_di - 2 * xs;
      double l2_di = lambda / di_2;
      double lx = li + xi, ux = ui + xi;
      double val_left = lx * lx + fi2_di * lx + l2_di * fabs(lx);
      double val_right = ux * ux + fi2_di * ux + l2_di * fabs(ux);
      double val_max = jl_max(val_left, val_right);
      yi = (val_left > val_right) ? left : right;
      double mxi = -xi;
      if (li <= mxi && mxi <= ui) {
        if (0.0 > val_max) yi = -xs;
      }
    }
    y[i] = yi;
  }
}

/* ShiftedNormL0Box.iprox!  src/shiftedNormL0Box.jl:137-231 */
ORC_API void orc_iprox_l0_box(double* y, const double* g, const double* d, const double* xk, const double* sj,
                              int64_t n, double lambda, const double* lvec, const double* uvec, double lscal,
                              double uscal, const uint8_t* mask) {
  const double eps = 2.220446049250313e-16;
  for (int64_t i = 0; i < n; ++i) {
    double li = lvec ? lvec[i] : lscal;
    double ui = uvec ? uvec[i] : uscal;
    double di = d[i], gi = g[i], si = sj[i], xi = xk[i];
    double xs = xi + si;
    double mxi = -xi;
    int zero_ok = (li <= mxi && mxi <= ui);
    if (!is_selected(mask, i)) { y[i] = iprox_zero(di, gi, li - si, ui - si); continue; } /* :227 */
    double yi;
    if (fabs(di) < eps) { /* :154 */
      if (gi == 0.0) {
        yi = zero_ok ? -xs : 0.0;
      } else {
        double val_min;
        if (gi > 0.0) {
          double left = li - si;
          val_min = gi * left + ((xi == -li) ? 0.0 : lambda);
          yi = left;
        } else {
          double right = ui - si;
          val_min = gi * right + ((xi == -ui) ? 0.0 : lambda);
          yi = right;
        }
        if (zero_ok) {
          double val_0 = -gi * xs;
          if (val_0 < val_min) yi = -xs;
        }
      }
    } else {
      double di_2 = di / 2;
      double left = li - si, right = ui - si;
      double lx = li + xi, ux = ui + xi;
      double gi2_di = gi / di_2;
      double fi2_di = gi2_di - 2 * xs;
      double l2_di = lambda / di_2;
      if (di >= eps) { /* :190 */
        double aqy = -gi / di;
        double aqv = aqy + xs;
        double val_min;
        if (lx <= aqv && aqv <= ux) {
          val_min = (aqv == 0.0) ? (-(aqv * aqv)) : (-(aqv * aqv) + l2_di);
          yi = aqy;
        } else {
          double val_left = (lx == 0.0) ? 0.0 : (lx * lx + fi2_di * lx + l2_di);
          double val_right = (ux == 0.0) ? 0.0 : (ux * ux + fi2_di * ux + l2_di);
          yi = (val_left < val_right) ? left : right;
          val_min = jl_min(val_left, val_right);
        }
        if (zero_ok) {
          if (0.0 < val_min) yi = -xs;
        }
      } else { /* :213 */
        double val_left = (lx == 0.0) ? 0.0 : (lx * lx + fi2_di * lx + l2_di);
        double val_right = (ux == 0.0) ? 0.0 : (ux * ux + fi2_di * ux + l2_di);
        yi = (val_left > val_right) ? left : right;
        double val_max = jl_max(val_left, val_right);
        if (zero_ok) {
          if (0.0 > val_max) yi = -xs;
        }
      }
    }
    y[i] = yi;
  }
}

ORC_API double orc_iprox_zero(double d, double g, double l, double u) { return iprox_zero(d, g, l, u); }

/* ==========================================================================================
 * psi(y)  (SURVEY.md 8f rank 2): objective value.  Sums run left to right as the reference's loops do.
 *   kind: 0 = NormL1 (lambda * sum |v|) [ext], 1 = NormL0 (lambda * count(v != 0)) [ext],
 *         2 = RootNormLhalf (lambda * sum sqrt|v|, src/rootNormLhalf.jl:27-29)
 * ========================================================================================== */
static inline double h_term(int kind, double v) {
  return kind == 0 ? fabs(v) : (kind == 1 ? ((v != 0.0) ? 1.0 : 0.0) : sqrt(fabs(v)));
}
/* generic  src/ShiftedProximalOperators.jl:51-54 */
ORC_API double orc_obj_plain(int kind, const double* y, const double* xk, const double* sj, int64_t n, double lambda) {
  double acc = 0.0;
  for (int64_t i = 0; i < n; ++i) acc += h_term(kind, (xk[i] + sj[i]) + y[i]);
  return lambda * acc;
}
/* Box  src/shiftedNormL1Box.jl:70-82 (idem L0Box, RootNormLhalfBox) */
ORC_API double orc_obj_box(int kind, const double* y, const double* xk, const double* sj, int64_t n, double lambda,
                           const double* lvec, const double* uvec, double lscal, double uscal, const uint8_t* mask) {
  double acc = 0.0;
  for (int64_t i = 0; i < n; ++i)
    if (is_selected(mask, i)) acc += h_term(kind, (xk[i] + sj[i]) + y[i]); /* :71-72 */
  const double slack = sqrt(2.220446049250313e-16); /* :73 */
  for (int64_t i = 0; i < n; ++i) {
    double lower = lvec ? lvec[i] : lscal, upper = uvec ? uvec[i] : uscal;
    double t = sj[i] + y[i];
    if (!(lower - slack <= t && t <= upper + slack)) return INFINITY; /* :77-79 */
  }
  return lambda * acc;
}
/* IndBallLinf(r)(x) [ext: ProximalOperators IndBox, strict comparisons] */
static int outside_linf_ball(const double* sj, const double* y, int64_t n, double rad) {
  for (int64_t i = 0; i < n; ++i) { double t = sj[i] + y[i]; if (t < -rad || t > rad) return 1; }
  return 0;
}
/* ShiftedIndBallL0 (generic form) and ShiftedIndBallL0BInf  src/shiftedIndBallL0BInf.jl:44-49; delta < 0: no ball */
ORC_API double orc_obj_indball_l0(const double* y, const double* xk, const double* sj, int64_t n, int64_t r, double delta) {
  int64_t cnt = 0;
  if (delta >= 0) {
    for (int64_t i = 0; i < n; ++i) cnt += (((sj[i] + y[i]) + xk[i]) != 0.0); /* :45,:47 */
    if (outside_linf_ball(sj, y, n, 1.1 * delta)) return INFINITY;          /* :46 */
  } else {
    for (int64_t i = 0; i < n; ++i) cnt += (((xk[i] + sj[i]) + y[i]) != 0.0);
  }
  return cnt > r ? INFINITY : 0.0;
}
/* GroupNormL2  src/groupNormL2.jl:33-39; Binf form src/shiftedGroupNormL2Binf.jl:34-39 (delta < 0: plain form) */
ORC_API double orc_obj_group_l2(const double* y, const double* xk, const double* sj, int64_t n, const int64_t* offsets,
                                int64_t gsize, int64_t ngroups, const double* lambda, double delta) {
  double sum_c = 0.0;
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t lo, hi;
    group_range(offsets, gsize, g, &lo, &hi);
    double ss = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
      double v = (delta >= 0) ? ((sj[i] + y[i]) + xk[i]) : ((xk[i] + sj[i]) + y[i]);
      ss += v * v;
    }
    sum_c += lambda[g] * sqrt(ss);
  }
  if (delta >= 0 && outside_linf_ball(sj, y, n, 1.1 * delta)) return INFINITY;
  return sum_c;
}

/* psi(y) for groups given as arbitrary index sets (same value rules as orc_obj_group_l2) */
ORC_API double orc_obj_group_l2_idx(const double* y, const double* xk, const double* sj, int64_t n, const int64_t* ptr,
                                    const int64_t* index, int64_t ngroups, const double* lambda, double delta) {
  double sum_c = 0.0;
  for (int64_t g = 0; g < ngroups; ++g) {
    double ss = 0.0;
    for (int64_t p = ptr[g]; p < ptr[g + 1]; ++p) {
      int64_t i = index[p];
      double v = (delta >= 0) ? ((sj[i] + y[i]) + xk[i]) : ((xk[i] + sj[i]) + y[i]);
      ss += v * v;
    }
    sum_c += lambda[g] * sqrt(ss);
  }
  if (delta >= 0 && outside_linf_ball(sj, y, n, 1.1 * delta)) return INFINITY;
  return sum_c;
}

/* ==========================================================================================
 * ShiftedNormL1B2.prox!  src/shiftedNormL1B2.jl:50-67  
 * find_zero(froot, Delta) [ext: Roots.jl, single starting point => Order0, a bracketing hybrid]: restated as
 * "expand from Delta until froot changes sign, then bit-midpoint bisection to exhaustion" -- the sign change is
 * unique (froot(eta)/eta is non-decreasing), so any convergent method ends within an ulp of the same point; the
 * reference's own stopping tolerance is unknown (its test pins the result to sqrt(eps) only).
 * ========================================================================================== */
typedef struct { const double *q, *xk, *sj; int64_t n; double ls, delta, chil; } b2_ctx;
static double b2_norm_projb(const b2_ctx* c, double scale) { /* chi(ProjB((-xk) .* scale)) */
  double ss = 0.0;
  for (int64_t i = 0; i < c->n; ++i) {
    double sq = c->sj[i] + c->q[i];
    double p = jl_min(jl_max((-c->xk[i]) * scale, sq - c->ls), sq + c->ls); /* :56 */
    ss += p * p;
  }
  return c->chil * nudge(sqrt(ss), g_norm_ulps);
}
static double b2_froot(const b2_ctx* c, double eta) { return eta - b2_norm_projb(c, eta / c->delta); } /* :57 */

ORC_API void orc_prox_l1_b2(double* y, const double* q, const double* xk, const double* sj, int64_t n, double lambda,
                            double sigma, double delta, double chi_lambda) {
  b2_ctx c = {q, xk, sj, n, lambda * sigma, delta, chi_lambda};
  double chiy = b2_norm_projb(&c, 1.0); /* y = ProjB(-xk), :59; chi(y), :61 */
  double scale = 1.0, back = 1.0;
  if (delta <= chiy) {
    double a = delta, fa = b2_froot(&c, a);
    double eta = a;
    if (fa != 0.0) {
      double b = 2 * a, fb = b2_froot(&c, b);
      /* (an exact zero at a bracket end IS the root -- find_zero returns it; the loop used to step over froot(b) == 0, doubled
       *  once more and bisected its way to 2 b: found by tools/fuzz_r2_onelaunch.py on integer lattice data, where the GPU was
       *  right and this restatement wrong) */
      for (int it = 0; it < 2000 && !(fb >= 0) && isfinite(b); ++it) { a = b; fa = fb; b = 2 * b; fb = b2_froot(&c, b); }
      if (fb == 0.0) eta = b;
      else {
        for (int it = 0; it < 200; ++it) {
          double m = bit_middle(a, b);
          if (!(a < m && m < b)) break;
          double fm = b2_froot(&c, m);
          if (fm == 0.0) { a = b = m; fa = fb = 0.0; break; } /* an exact zero is convergence for any find_zero method */
          if (jl_sign(fa) * jl_sign(fm) < 0) { b = m; fb = fm; } else { a = m; fa = fm; }
        }
        eta = (fabs(fa) < fabs(fb)) ? a : b;
      }
    }
    scale = eta / delta; /* :63 */
    back = delta / eta;
    for (int64_t i = 0; i < n; ++i) {
      double sq = sj[i] + q[i];
      y[i] = jl_min(jl_max((-xk[i]) * scale, sq - c.ls), sq + c.ls) * back - sj[i]; /* :63,:65 */
    }
    return;
  }
  for (int64_t i = 0; i < n; ++i) {
    double sq = sj[i] + q[i];
    y[i] = jl_min(jl_max(-xk[i], sq - c.ls), sq + c.ls) - sj[i]; /* :59,:65 */
  }
}

/* Objective value 1/(2 sigma) (t-q)^2 + lambda*h(x+s+t) helpers for the brute-force second oracle
 * live in tests/ (numpy); nothing else is exported from here. */
/* (psi::ShiftedNormL1B2)(y) = h(xk + sj + y) + IndBallL2(Delta)(sj + y)   src/shiftedNormL1B2.jl:32
 * IndBallL2 [ext, ProximalOperators.jl]: 0 iff isapprox_le(norm(v), r, atol = eps, rtol = sqrt(eps)), i.e.
 * norm(v) <= r or |norm(v) - r| <= max(eps, sqrt(eps) max(norm(v), r)); +Inf otherwise. */
ORC_API double orc_obj_l1_b2(const double* y, const double* xk, const double* sj, int64_t n, double lambda, double delta) {
  double l1 = 0.0, ss = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    l1 += fabs((xk[i] + sj[i]) + y[i]);
    double t = sj[i] + y[i];
    ss += t * t;
  }
  const double eps = 2.220446049250313e-16;
  double nrm = sqrt(ss);
  double tol = fmax(eps, sqrt(eps) * fmax(nrm, fabs(delta)));
  int inside = (nrm <= delta) || (fabs(nrm - delta) <= tol);
  return inside ? lambda * l1 : INFINITY;
}

ORC_API int orc_abi_version(void) { return 4; }

/* ------------------------------------------------------------------------------------------
 * Synthetic inputs: host twin of the library's spx_synth_fill -- splitmix64 of a counter keyed by
 * (seed, stream), integer arithmetic and exact binary64 additions only, so host and device agree bit for bit.
 * kind 0: U(-1/2, 1/2); kind 1: ~N(0, 1) as the sum of 12 uniforms on [0, 1) minus 6.  Not in the reference: benchmark and
 * test plumbing (the reference's tests draw from Julia's RNG).
 * ------------------------------------------------------------------------------------------ */
static uint64_t orc_splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
ORC_API void orc_synth_fill(double* out, int64_t n, uint64_t seed, uint64_t stream, int kind, double scale, int threads) {
  const uint64_t key = orc_splitmix64(seed ^ (stream * 0xd1342543de82ef95ull));
  if (threads < 1) threads = 1;
#pragma omp parallel for num_threads(threads) schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    double v;
    if (kind == 0) {
      v = (double)(orc_splitmix64(key + (uint64_t)i) >> 11) * 0x1.0p-53 - 0.5;
    } else {
      double acc = 0.0;
      for (int k = 0; k < 12; ++k) acc += (double)(orc_splitmix64(key + (uint64_t)i * 12ull + (uint64_t)k) >> 11) * 0x1.0p-53;
      v = acc - 6.0;
    }
    out[i] = scale * v;
  }
}
