/*
 * spx_oracle_f32.c -- Float32 build of the CPU restatement, for the operators whose reference bodies are pure Float32
 * arithmetic when R = Float32 (the NormL1 / NormL0 families).
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE (same rule as spx_oracle.c).
 *
 * The reference is generic in R <: Real (src/shiftedNormL1Box.jl:89-94 etc.); with R = Float32, Int literals promote to
 * Float32 (`2 * psi.lambda * sigma`, `0`) and every +, -, *, comparison, min / max and the one sqrt is a Float32 operation.
 * x86-64 SSE evaluates `float` expressions in IEEE binary32 (no excess precision), gcc -ffp-contract=off: the loops
 * below are the same statements as in spx_oracle.c with `float` for `double`.
 * Pinning: the reference's tests hold no Float32 prox values (test/runtests.jl:196-209 checks types and psi(0) only):
 * PARITY UNPINNED by reference vectors; checked against the Float64 restatement on data where both are exact
 * (tests/test_oracle_golden.py::test_f32_oracle_agrees_with_f64_on_dyadic_data).
 *
 * psi(y) and ShiftedGroupNormL2.prox! with R = Float32 (second half of this file) are stated as include/spx.h states them:
 * every element operation in Float32, `1.1 * Delta` and its comparison in Float64, squares of group elements as Float64
 * products of Float32 values, the group norm rounded to Float32 once.  They return the TERMS of psi(y), not a sum: the
 * caller adds them exactly (tests/test_oracle_f32_forms.py pins them against the Float64 restatement and known answers).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#define ORC_API __attribute__((visibility("default")))

static inline float jl_minf(float x, float y) {
  float d = x - y;
  float a = signbit(d) ? x : y;
  return (isnan(x) || isnan(y)) ? d : a;
}
static inline float jl_maxf(float x, float y) {
  float d = x - y;
  float a = signbit(d) ? y : x;
  return (isnan(x) || isnan(y)) ? d : a;
}
static inline int is_selected(const uint8_t* mask, int64_t i) { return mask == NULL || mask[i] != 0; }

/* ShiftedNormL1.prox!  src/shiftedNormL1.jl:40-54 (two passes: y === q clobbers q first, as in the reference) */
ORC_API void orc32_prox_l1(float* y, const float* q, const float* xk, const float* sj, int64_t n, float lambda, float sigma) {
  for (int64_t i = 0; i < n; ++i) y[i] = (-xk[i]) - sj[i];
  for (int64_t i = 0; i < n; ++i) {
    float qi = q[i];
    y[i] = jl_minf(jl_maxf(y[i], qi - lambda * sigma), qi + lambda * sigma);
  }
}

/* ShiftedNormL0.prox!  src/shiftedNormL0.jl:38-55 */
ORC_API void orc32_prox_l0(float* y, const float* q, const float* xk, const float* sj, int64_t n, float lambda, float sigma) {
  const float c = sqrtf(2 * lambda * sigma); /* :45 */
  for (int64_t i = 0; i < n; ++i) {
    float xps = xk[i] + sj[i];
    float qi = q[i];
    y[i] = (fabsf(xps + qi) <= c) ? -xps : qi;
  }
}

/* ShiftedNormL1Box.prox!  src/shiftedNormL1Box.jl:89-125 */
ORC_API void orc32_prox_l1_box(float* y, const float* q, const float* xk, const float* sj, int64_t n, float lambda,
                               float sigma, const float* lvec, const float* uvec, float lscal, float uscal,
                               const uint8_t* mask) {
  const float sl = sigma * lambda; /* :96 */
  for (int64_t i = 0; i < n; ++i) {
    float li = lvec ? lvec[i] : lscal, ui = uvec ? uvec[i] : uscal;
    float qi = q[i], si = sj[i];
    if (is_selected(mask, i)) {
      float xs = xk[i] + si;
      float xsq = xs + qi;
      float t;
      if (xsq <= -sl) t = qi + sl;
      else if (xsq >= sl) t = qi - sl;
      else t = -xs;
      y[i] = jl_minf(jl_maxf(t, li - si), ui - si); /* :118 */
    } else {
      y[i] = jl_minf(jl_maxf(qi, li - si), ui - si); /* :121 */
    }
  }
}

/* ShiftedNormL0Box.prox!  src/shiftedNormL0Box.jl:89-131 */
ORC_API void orc32_prox_l0_box(float* y, const float* q, const float* xk, const float* sj, int64_t n, float lambda,
                               float sigma, const float* lvec, const float* uvec, float lscal, float uscal,
                               const uint8_t* mask) {
  const float c = 2 * lambda * sigma; /* :96 */
  for (int64_t i = 0; i < n; ++i) {
    float li = lvec ? lvec[i] : lscal, ui = uvec ? uvec[i] : uscal;
    float qi = q[i], si = sj[i];
    float sq = si + qi;
    if (is_selected(mask, i)) {
      float xi = xk[i];
      float xs = xi + si;
      float xsq = xs + qi;
      float dl = li - sq, du = ui - sq;
      float val_left = dl * dl + ((xi == -li) ? 0.0f : c);
      float val_right = du * du + ((xi == -ui) ? 0.0f : c);
      float yi = (val_left < val_right) ? (li - si) : (ui - si);
      float val_min = jl_minf(val_left, val_right);
      float mxi = -xi;
      if (li <= mxi && mxi <= ui) {
        float val_0 = xsq * xsq;
        if (val_0 < val_min) yi = -xs;
        val_min = jl_minf(val_0, val_min);
      }
      if (li <= sq && sq <= ui) {
        float val_xsq = (xsq == 0.0f) ? 0.0f : c;
        if (val_xsq < val_min) yi = qi;
      }
      y[i] = yi;
    } else {
      y[i] = jl_minf(jl_maxf(qi, li - si), ui - si); /* :127 */
    }
  }
}

/* ==========================================================================================
 * iprox! with R = Float32 (round 3): the Float64 block of spx_oracle.c, type-substituted by the Makefile
 * (src/shiftedNormL1.jl:60-75, shiftedNormL0.jl:61-80, shiftedNormL1Box.jl:131-225, shiftedNormL0Box.jl:137-231,
 * ShiftedProximalOperators.jl:217-236; thresholds eps(R) = eps(Float32)).
 * ========================================================================================== */
#include "_gen/iprox_f32.inc"

/* ==========================================================================================
 * psi(y) with R = Float32: the terms of the sum, and the feasibility verdict.
 *   kind: 0 = NormL1 (|v|) [ext], 1 = NormL0 (v != 0) [ext], 2 = RootNormLhalf (sqrt|v|, src/rootNormLhalf.jl:27-29)
 *   mode: 0 = generic, v = (xk + sj) + y                                   src/ShiftedProximalOperators.jl:51-54
 *         1 = Box: the same over the selected indices (term 0 elsewhere); verdict over EVERY index:
 *             l - sqrt(eps(Float32)) <= sj + y <= u + sqrt(eps(Float32)), all Float32  src/shiftedNormL1Box.jl:70-82
 *         2 = BInf: v = (sj + y) + xk; verdict |sj + y| <= 1.1 * Delta with the product and the comparison in Float64
 *             (the Float64 literal promotes; strict IndBox test)              src/shiftedIndBallL0BInf.jl:44-49
 * terms[i] = the Float32 term as a double (every Float32 is one).  Returns 1 if y is infeasible (psi = +Inf), else 0.
 * ========================================================================================== */
static inline float h_term32(int kind, float v) {
  return kind == 0 ? fabsf(v) : (kind == 1 ? ((v != 0.0f) ? 1.0f : 0.0f) : sqrtf(fabsf(v)));
}
ORC_API int orc32_obj_terms(double* terms, int kind, int mode, const float* y, const float* xk, const float* sj, int64_t n,
                            const float* lvec, const float* uvec, float lscal, float uscal, const uint8_t* mask, float delta) {
  const float slack = sqrtf(1.1920928955078125e-07f); /* :73, sqrt(eps(R)) */
  const double rad = 1.1 * (double)delta;              /* :46 */
  int infeasible = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (mode == 2) {
      float t = sj[i] + y[i]; /* :45 */
      if ((double)t < -rad || (double)t > rad) infeasible = 1;
      terms[i] = (double)h_term32(kind, t + xk[i]); /* :47 */
    } else {
      float v = (xk[i] + sj[i]) + y[i];
      terms[i] = (mode == 1 && !is_selected(mask, i)) ? 0.0 : (double)h_term32(kind, v); /* :71-72 */
      if (mode == 1) {
        float lower = lvec ? lvec[i] : lscal, upper = uvec ? uvec[i] : uscal;
        float t = sj[i] + y[i];
        if (!(lower - slack <= t && t <= upper + slack)) infeasible = 1; /* :77-79 */
      }
    }
  }
  return infeasible;
}

static inline void group_range32(const int64_t* offsets, int64_t gsize, int64_t g, int64_t* lo, int64_t* hi) {
  if (offsets) { *lo = offsets[g]; *hi = offsets[g + 1]; }
  else { *lo = g * gsize; *hi = (g + 1) * gsize; }
}

/* GroupNormL2  src/groupNormL2.jl:33-39; Binf form src/shiftedGroupNormL2Binf.jl:34-39 (binf != 0).
 * terms[g] = (double)lambda_g * sqrt(sum of (double)v * (double)v): v a Float32, its square exact in Float64, the sum left to right.
 * Returns bit 0: |sj + y| > 1.1 * Delta at ANY index of [0, n) (binf only); bit 1: offsets decreasing or outside [0, n] (the
 * contract of include/spx.h; the terms are then not formed). */
ORC_API int orc32_obj_group_terms(double* terms, const float* y, const float* xk, const float* sj, int64_t n,
                                  const int64_t* offsets, int64_t gsize, int64_t ngroups, const float* lambda, int binf,
                                  float delta) {
  int verdict = 0;
  if (offsets)
    for (int64_t g = 0; g < ngroups; ++g)
      if (offsets[g] > offsets[g + 1] || offsets[g] < 0 || offsets[g + 1] > n) verdict |= 2;
  if (binf) {
    const double rad = 1.1 * (double)delta;
    for (int64_t i = 0; i < n; ++i) {
      float t = sj[i] + y[i];
      if ((double)t < -rad || (double)t > rad) verdict |= 1;
    }
  }
  if (verdict & 2) return verdict;
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t lo, hi;
    group_range32(offsets, gsize, g, &lo, &hi);
    double ss = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
      float v = binf ? ((sj[i] + y[i]) + xk[i]) : ((xk[i] + sj[i]) + y[i]);
      ss += (double)v * (double)v;
    }
    terms[g] = (double)lambda[g] * sqrt(ss);
  }
  return verdict;
}

/* ShiftedGroupNormL2.prox!  src/shiftedGroupNormL2.jl:52-79 with R = Float32.  `y` holds y on entry: an index in no group
 * ends as (y on entry) - (xk + sj) (:77 runs over every index).  y may be q itself (sol is formed first, :65).
 * snorm_override != NULL: group g takes snorm_override[g] for its norm where that is not NaN -- a test evaluates a group with
 * either Float32 neighbour of a norm that sits on a rounding boundary. */
ORC_API void orc32_prox_group_l2(float* y, const float* q, const float* xk, const float* sj, int64_t n, const int64_t* offsets,
                                 int64_t gsize, int64_t ngroups, const float* lambda, float sigma,
                                 const float* snorm_override) {
  float* sol = (float*)malloc((size_t)(n > 0 ? n : 1) * sizeof(float));
  if (!sol) { fprintf(stderr, "orc32_prox_group_l2: out of memory (n = %lld)\n", (long long)n); abort(); }
  for (int64_t i = 0; i < n; ++i) sol[i] = (q[i] + xk[i]) + sj[i]; /* :65 */
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t lo, hi;
    group_range32(offsets, gsize, g, &lo, &hi);
    double ss = 0.0;
    for (int64_t i = lo; i < hi; ++i) ss += (double)sol[i] * (double)sol[i];
    float snorm = (float)sqrt(ss); /* :69 */
    if (snorm_override && !isnan(snorm_override[g])) snorm = snorm_override[g];
    if (snorm == 0) {
      for (int64_t i = lo; i < hi; ++i) y[i] = 0.0f;
    } else {
      float alpha = jl_maxf(1 - sigma * lambda[g] / snorm, 0.0f); /* :73 */
      for (int64_t i = lo; i < hi; ++i) y[i] = alpha * sol[i];
    }
  }
  for (int64_t i = 0; i < n; ++i) y[i] = y[i] - (xk[i] + sj[i]); /* :77 */
  free(sol);
}
