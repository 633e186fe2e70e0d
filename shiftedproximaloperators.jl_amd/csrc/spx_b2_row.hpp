// spx_b2_row.hpp -- the root iteration of ShiftedNormL1B2 on ONE row whose every reduction is formed by ONE owner (a workgroup:
// k_b2_batch of spx_b2_batch.hip; a plain loop on the host: tests/c/b2_batch_plan_driver.hip), stated once as __host__ __device__
// functions of plain values: given the sums (P, C[, F]) at the current eta, the next eta or "done".  No HIP include, no kernel.
//
//   ProjB(z)_i = min(max(z_i, lo_i), hi_i),  lo_i, hi_i = (sj_i + q_i) -+ lambda sigma
//   at scale r = eta / Delta:  P = sum over the unclamped i of xk_i^2,  C = sum over the clamped i of bound_i^2,
//                              ||ProjB((-xk) r)||^2 = r^2 P + C;        F = sum of the bound every element reaches as r -> inf
//   froot(eta) = eta - chi_lambda sqrt(r^2 P + C); on a fixed set of clamped elements its root is
//   eta = chi_lambda sqrt(C / (1 - chi_lambda^2 P / Delta^2))  (the piece root).
// The rule is the loop at the end of k_b2_coop (spx_b2.hip) without its early stop: a reduction here stays inside one workgroup
// and costs about a microsecond, so the iteration runs to the EXACT fixed point -- it ends when an exact step gives back the same
// (P, C) (the piece is confirmed), on froot == 0, on a step of at most 4e-16, or when the bracket [froot < 0, froot > 0] has
// collapsed.  The caller caps the number of reductions (kB2RowMaxReductions) so that degenerate parameters (Delta <= 0, NaN)
// terminate; ordinary rows need at most five.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SPX_B2_ROW_HD __host__ __device__ inline
#else
#define SPX_B2_ROW_HD inline
#endif

constexpr int kB2RowMaxReductions = 48;  // reductions of one row at most, the first (r = 1) included

enum B2RowNext { kB2RowDone = 0, kB2RowReduce = 1 };  // kB2RowReduce: form (P, C) at B2RowIter::eta and call b2_row_step

struct B2RowIter {
  double eta;     // the scale the next sums are wanted at / the root when done
  double lo, hi;  // the bracket: froot(lo) < 0 <= froot(hi)
  double pP, pC;  // the sums the last step was taken from
  bool exact;     // the last step was a piece root inside the bracket
  bool scaled;    // the trust region is active: y = ProjB((-xk) eta / Delta) Delta / eta
};

SPX_B2_ROW_HD double b2_row_inf() { return __builtin_inf(); }

// One step: (P, C) are the sums at s.eta.
SPX_B2_ROW_HD B2RowNext b2_row_step(B2RowIter& s, double P, double C, double delta, double chil) {
  const double inf = b2_row_inf();
  const double eta = s.eta;
  const double r = eta / delta;
  const double f = eta - chil * sqrt(r * r * P + C);
  if (f == 0.0 || (s.exact && P == s.pP && C == s.pC)) return kB2RowDone;
  if (f < 0.0) s.lo = eta; else s.hi = eta;
  const double den = 1.0 - chil * chil * P / (delta * delta);
  double next = (den > 0.0) ? chil * sqrt(C / den) : inf;
  s.exact = next > s.lo && next < s.hi;
  if (!s.exact) next = (s.hi == inf) ? 2.0 * s.lo : 0.5 * (s.lo + s.hi);
  if (!(next > s.lo && next < s.hi)) return kB2RowDone;  // the bracket has collapsed
  if (fabs(next - eta) / next <= 4e-16) return kB2RowDone;
  s.pP = P; s.pC = C; s.eta = next;
  return kB2RowReduce;
}

// The start: (P, C, F) are the sums at r = 1.  :61 `Delta <= chi(y)` with equality reproduces the unscaled result, so the trust
// region counts as active only for Delta < chi(y).  chi(y) = +Inf (an infinite box end): the root lies at infinity, eta = Inf.
// Otherwise the iteration starts from the bound eta = chi_lambda sqrt(F) when that is usable, else from eta = Delta.
SPX_B2_ROW_HD B2RowNext b2_row_begin(B2RowIter& s, double P, double C, double F, double delta, double chil) {
  const double inf = b2_row_inf();
  const double chiy = chil * sqrt(P + C);
  s.eta = delta; s.lo = delta; s.hi = inf; s.pP = -1.0; s.pC = -1.0; s.exact = false;
  s.scaled = delta < chiy;
  if (!s.scaled) return kB2RowDone;
  if (!(chiy < inf)) { s.eta = inf; return kB2RowDone; }
  const double ub = chil * sqrt(F);
  if (ub > delta && ub < inf) { s.eta = ub; return kB2RowReduce; }
  return b2_row_step(s, P, C, delta, chil);
}

// the scales of the storing sweep: y = min(max((-xk) r, lo), hi) rinv - sj
SPX_B2_ROW_HD void b2_row_scales(const B2RowIter& s, double delta, double* r, double* rinv) {
  *r = s.scaled ? s.eta / delta : 1.0;
  *rinv = s.scaled ? delta / s.eta : 1.0;
}
