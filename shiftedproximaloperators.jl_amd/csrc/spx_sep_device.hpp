// spx_sep_device.hpp -- the device code the separable calls share: the per-element operators (one functor per operator), the
// wrappers that add the sums of a fused call (WithValue, WithStep, WithIstep), the element site (apply_op, sep_accumulate), the
// workgroup sums and the ordered finish, and the operator table (one Row per operator: its functors, its h term, make).
// Included by spx_separable.hip (the single-problem kernels and entry points) and by spx_batch.hip (the batched call), so that
// both store the same bits: there is one body per operator and one element site.
#pragma once
#include <cmath>

#include <limits>
#include <type_traits>

#include "spx_common.hpp"

// ---------------------------------------------------------------------------------------------
// per-element operators, one body per operator for both precisions (T = double: the kernels below; T = float: k_sep_f32).
// Signature: (q, x, s, l, u, selected) -> y.  Unboxed ones ignore l, u, selected.
// Every expression keeps the reference's association (cited); the library is built with
// -ffp-contract=off so a*b+c never becomes an FMA.  Every literal is a T: with R = Float32 the reference's Int literals
// promote to Float32 (`2 * psi.lambda * sigma`, `0`), so the Float32 results are reproduced BIT FOR BIT in fp32 as well.
// ---------------------------------------------------------------------------------------------
template <class T>
struct ProxL1 {  // src/shiftedNormL1.jl:46-51
  T ls;          // lambda * sigma
  static constexpr bool kBox = false;
  static constexpr int kNIn = 3;  // input vectors besides bounds: q, xk, sj
  __device__ __forceinline__ T operator()(T q, T x, T s, T, T, bool) const {
    T t = (-x) - s;                               // :47  @. y = -xk - sj
    return jl_min(jl_max(t, q - ls), q + ls);     // :50
  }
};
template <class T>
struct ProxL1Aliased {  // y === q in the reference: the broadcast at :47 overwrites q before :50 reads it
  static constexpr bool kBox = false;
  static constexpr int kNIn = 3;
  __device__ __forceinline__ T operator()(T, T x, T s, T, T, bool) const {
    return (-x) - s;  // min(max(t, t - ls), t + ls) == t bit for bit whenever ls >= 0
  }
};
template <class T>
struct ProxL0 {  // src/shiftedNormL0.jl:45-52
  T c;           // sqrt(2 * lambda * sigma)
  static constexpr bool kBox = false;
  static constexpr int kNIn = 3;
  __device__ __forceinline__ T operator()(T q, T x, T s, T, T, bool) const {
    T xps = x + s;
    return (fabs(xps + q) <= c) ? -xps : q;
  }
};
template <class T>
struct ProxL1Box {  // src/shiftedNormL1Box.jl:96-122
  T sl;             // sigma * lambda
  static constexpr bool kBox = true;
  static constexpr int kNIn = 3;
  __device__ __forceinline__ T operator()(T q, T x, T s, T l, T u, bool sel) const {
    T xs = x + s;
    T xsq = xs + q;
    T t = (xsq <= -sl) ? (q + sl) : ((xsq >= sl) ? (q - sl) : -xs);  // :111-117
    t = sel ? t : q;                                                  // :121 prox_zero(qi, ...)
    return jl_min(jl_max(t, l - s), u - s);                           // :118
  }
};
template <class T>
struct ProxL0Box {  // src/shiftedNormL0Box.jl:96-128
  T c;              // 2 * lambda * sigma
  static constexpr bool kBox = true;
  static constexpr int kNIn = 3;
  __device__ __forceinline__ T operator()(T q, T x, T s, T l, T u, bool sel) const {
    T sq = s + q;
    T xs = x + s;
    T xsq = xs + q;
    T dl = l - sq, du = u - sq;
    T val_left = dl * dl + ((x == -l) ? T(0) : c);   // :110
    T val_right = du * du + ((x == -u) ? T(0) : c);  // :111
    T yi = (val_left < val_right) ? (l - s) : (u - s);  // :114
    T val_min = jl_min(val_left, val_right);
    T mx = -x;
    if (l <= mx && mx <= u) {  // :116
      T val_0 = xsq * xsq;
      yi = (val_0 < val_min) ? -xs : yi;
      val_min = jl_min(val_0, val_min);
    }
    if (l <= sq && sq <= u) {  // :121
      T val_xsq = (xsq == T(0)) ? T(0) : c;
      yi = (val_xsq < val_min) ? q : yi;
    }
    return sel ? yi : prox_zero(q, l - s, u - s);  // :127
  }
};
// The Float64 operators of the kernels below; kLdsKiB: KiB per wave and input vector in the LDS-staged skeleton (0: the
// register-staged one).  WithValue / WithStep below wrap them with the sums a call adds (kSumsOf)
struct OpL1 : ProxL1<double> { static constexpr int kLdsKiB = 6; };
struct OpL1Aliased : ProxL1Aliased<double> { static constexpr int kLdsKiB = 6; };
struct OpL0 : ProxL0<double> { static constexpr int kLdsKiB = 6; };
struct OpL1Box : ProxL1Box<double> { static constexpr int kLdsKiB = 6; };
struct OpL0Box : ProxL0Box<double> { static constexpr int kLdsKiB = 6; };

// ---------------------------------------------------------------------------------------------
// RootNormLhalf closed form.  Reference (src/shiftedRootNormLhalf.jl:48,57; shiftedRootNormLhalfBox.jl:92,106):
//   val = (2/3) sign(z) |z| (1 + cos(2 pi/3 - (2/3) acos(a))),   a = (sigma lambda / 4) (|z|/3)^(-3/2),  a <= 1.
// With phi = acos(-a) = pi - acos(a) and w = cos(phi/3) in [1/2, sqrt(3)/2]:  cos(2 pi/3 - (2/3) acos a) = 2 w^2 - 1,
// so  val = sign(z) * 4 t w^2  with t = |z|/3, and w is the largest root of 4 w^3 - 3 w + a = 0.
// Writing w = 1/2 + d:  4 d^3 + 6 d^2 = m := 1 - a  (d ~ sqrt(m/6) near the threshold a = 1).
// d is obtained by 2 Newton steps on g(d) = 4 d^3 + 6 d^2 - m from a cubic fit d0 = e P(e), e = sqrt(m)
// (relative error of the fit 5.4e-5 on [0, 1]; Newton squares it: 1e-9, 1e-18).  The divisions by
// g'(d) = 12 d (d + 1) use the f32 reciprocal: Newton is self-correcting, a 1e-7 error in the slope costs
// 1e-7 * |last correction| <= 1e-16.  a itself comes from an fp64 rsqrt (hardware seed + 2 Newton steps).
// Accuracy vs an 80-bit evaluation of the reference formula: <= 6e-16 |z| everywhere, the same as the
// reference's own double evaluation (tools/lhalf_proto.py); agreement with the CPU restatement is checked to
// 1e-12 in tests/.  No pow / acos / cos calls: ~55 fp64 VALU ops instead of ~250.
// ---------------------------------------------------------------------------------------------
#ifndef SPX_LHALF_NEWTON
#define SPX_LHALF_NEWTON 2  // fit 5.4e-5 -> 1.5e-9 -> 1e-18 (tools/lhalf_proto.py: 2 and 3 steps give identical errors)
#endif
__device__ __forceinline__ double rsqrt_f64(double t) {
  double y = __builtin_amdgcn_rsq(t);            // v_rsq_f64 seed
  const double h = 0.5 * t;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double e = __builtin_fma(-h * y, y, 0.5);    // 1/2 - t y^2 / 2
    y = __builtin_fma(y, e, y);
  }
  return y;
}
// sqrt(v) for v >= 0: coupled Goldschmidt step on (s, h) = (v y, y / 2) from the hardware rsq seed, then one
// residual correction (faithfully rounded; 8 VALU ops)
__device__ __forceinline__ double sqrt_f64(double v) {
  const double y = __builtin_amdgcn_rsq(v);
  double s = v * y;
  double h = 0.5 * y;
  const double r = __builtin_fma(-s, h, 0.5);
  s = __builtin_fma(s, r, s);
  h = __builtin_fma(h, r, h);
  s = __builtin_fma(__builtin_fma(-s, s, v), h, s);
  return (v > 0.0) ? s : 0.0;
}
// a = sl4 * (az/3)^(-3/2) and t = az/3
__device__ __forceinline__ double lhalf_a(double az, double sl4, double& t, double* r_out = nullptr) {
  t = az * 0.33333333333333331;
  const double r = rsqrt_f64(t);
  if (r_out) *r_out = r;
  return sl4 * (r * r * r);
}
// sign(z) * 4 t w^2 for a in [0, 1]
__device__ __forceinline__ double lhalf_val_from_a(double z, double t, double a, double* w_out = nullptr) {
  const double m = fmax(1.0 - a, 0.0);
  const double e = (double)__builtin_amdgcn_sqrtf((float)m);
  double d = e * __builtin_fma(e, __builtin_fma(e, __builtin_fma(e, -0.003676457097091405, 0.016543212998449176),
                                                 -0.05508522799226874), 0.4082262283672896);
#pragma unroll
  for (int k = 0; k < SPX_LHALF_NEWTON; ++k) {
    const double g = __builtin_fma(__builtin_fma(4.0, d, 6.0) * d, d, -m);
    const double gp = 12.0 * d * (d + 1.0);
    const double inv = (gp > 0.0) ? (double)__builtin_amdgcn_rcpf((float)gp) : 0.0;
    d = __builtin_fma(-g, inv, d);
  }
  const double w = 0.5 + d;
  if (w_out) *w_out = w;
  const double v = 4.0 * t * (w * w);
  return (z < 0.0) ? -v : v;
}
struct OpLhalf {  // src/shiftedRootNormLhalf.jl:47-60
  double sl4;     // (sigma * lambda) / 4
  double p;       // 54^(1/3) * (2 sigma lambda)^(2/3) / 4
  static constexpr bool kBox = false;
  static constexpr int kLdsKiB = 6;  // KiB per wave and input vector in the LDS-staged skeleton
  static constexpr int kNIn = 3;
      // input vectors besides bounds: q, xk, sj
  __device__ __forceinline__ double operator()(double q, double x, double s, double, double, bool) const {
    double xs = x + s;
    double sol = q + xs;  // :50
    double aq = fabs(sol);
    double t;
    double a = lhalf_a(aq, sl4, t);
    double val = lhalf_val_from_a(sol, t, fmin(a, 1.0));
    double yi = (aq <= p) ? 0.0 : val;  // :53-57
    return yi - xs;                     // :59
  }
};
struct OpLhalfBox {  // src/shiftedRootNormLhalfBox.jl:92-117
  double sl4;        // sigma * lambda / 4
  double lambda;
  double h2;         // 1 / (2 sigma)
  static constexpr bool kBox = true;
  static constexpr int kLdsKiB = 0;  // 0: register-staged skeleton (VALU-heavy: needs the occupancy; 5.97 vs 5.68 TB/s)
  static constexpr int kNIn = 3;
 
  // RNorm(tt) = (tt - q)^2 / 2 / sigma + lambda sqrt|tt + xs|   (:95); used only to pick the argmin
  __device__ __forceinline__ double rnorm(double tt, double q, double xs) const {
    double d = tt - q;
    return __builtin_fma(lambda, sqrt_f64(fabs(tt + xs)), d * d * h2);
  }
  // the same for a bound candidate, where tt may be +-Inf (one-sided / absent bounds): sqrt_f64 is an rsq iteration and
  // turns Inf into NaN, so its argument is capped -- the (tt - q)^2 term is Inf there anyway and so is the sum
  __device__ __forceinline__ double rnorm_bound(double tt, double q, double xs) const {
    double d = tt - q;
    return __builtin_fma(lambda, sqrt_f64(fmin(fabs(tt + xs), 1.0e300)), d * d * h2);
  }
  __device__ __forceinline__ double operator()(double q, double x, double s, double l, double u, bool sel) const {
    double xs = x + s;  // :94
    double xsq = xs + q;
    double axsq = fabs(xsq);
    double tl = l - s, tu = u - s;
    // candidates 1..3 (:109-111); findmin keeps the FIRST minimum -> a later one replaces only on strict <
    double best = rnorm_bound(tl, q, xs);
    double yi = tl;
    double c2 = rnorm_bound(tu, q, xs);
    if (c2 < best) { best = c2; yi = tu; }
    double mx = -x;
    double c3 = xsq * xsq * h2;  // RNorm(-xs): (-xs - q)^2 = xsq^2 and sqrt|(-xs) + xs| = 0 exactly
    if (l <= mx && mx <= u && c3 < best) { best = c3; yi = -xs; }
    // candidate 4 (:106,:112): the stationary point.  When the acos argument a exceeds 1 the reference
    // takes the real part of a complex expression, which is not a stationary point; the objective is
    // then V-shaped around v = 0 so that candidate can never be strictly smaller than the first three
    //  and is skipped here.  a is Inf/NaN for xsq == 0 -> skipped too, as in the
    // reference (`li <= NaN <= ui` is false).
    double t, r, w;
    double a = lhalf_a(axsq, sl4, t, &r);
    if (a <= 1.0) {
      double val = lhalf_val_from_a(xsq, t, a, &w);
      double vx = val - x;
      double t4 = val - xs;
#ifdef SPX_LHALFBOX_SQRT_T4
      double c4 = rnorm(t4, q, xs);
#else
      // RNorm(t4) = (t4 - q)^2 / 2 sigma + lambda sqrt|t4 + xs| with |t4 + xs| = |val| = 4 t w^2 up to rounding:
      // sqrt|val| = 2 sqrt(t) w = 2 (t r) w from the reciprocal square root already at hand -- one square root less.
      // (The value only ranks the candidates; the other three keep the faithfully rounded square root.)
      const double d4 = t4 - q;
      double c4 = __builtin_fma(lambda, 2.0 * (t * r) * w, d4 * d4 * h2);
#endif
      if (l <= vx && vx <= u && c4 < best) { best = c4; yi = t4; }
    }
    // NaN in q, xk or sj: every candidate value is NaN and findmin returns the first one (:114, `findmin` treats NaN as
    // the smallest value) -> candidate 1
    yi = (xsq != xsq) ? tl : yi;
    return sel ? yi : prox_zero(q, tl, tu);  // :116
  }
};

// ---------------------------------------------------------------------------------------------
// iprox!  (SURVEY.md 8f rank 1): argmin 1/2 y'Dy + g'y + psi(y), D = diag(d).  Four input vectors (g, d, xk, sj):
// 40 B/element (20 in Float32).  Only +, -, *, /, sqrt and comparisons: bit-exact against the reference formulas, in
// either precision (the reference's iprox! methods are generic in R; the thresholds are eps(R)).
// ---------------------------------------------------------------------------------------------
// iprox_zero(d, g, l, u)   src/ShiftedProximalOperators.jl:217-236
template <class T>
__device__ __forceinline__ T iprox_zero(T d, T g, T l, T u) {
  const T eps = std::numeric_limits<T>::epsilon();
  const T a = jl_min(jl_max(-g / d, l), u);                          // d > eps
  const T d_2 = d / 2;
  const T b = ((d_2 * (l * l) + g * l) < (d_2 * (u * u) + g * u)) ? l : u;  // d < -eps
  const T c = (g > T(0)) ? l : ((g < T(0)) ? u : T(0));              // |d| <= eps
  return (d > eps) ? a : ((d < -eps) ? b : c);
}
template <class T>
struct IproxL1 {  // src/shiftedNormL1.jl:60-75
  T lambda;
  int* flag;  // set when some d[i] <= 0 (the reference's `@assert d[i] > 0`)
  static constexpr bool kBox = false;
  static constexpr int kNIn = 4;
  __device__ __forceinline__ T call4(T g, T d, T x, T s, T, T, bool) const {
    // (raised once: a d that is wrong everywhere must not queue 1e8 atomics on one address -- 12 ns apiece)
    if (!(d > T(0)) && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(flag, 1);
    const T t = (-x) - s;                                                            // :67
    return jl_min(jl_max(t, -g / d - lambda / d), -g / d + lambda / d);              // :71
  }
};
template <class T>
struct IproxL0 {  // src/shiftedNormL0.jl:61-80
  T lambda;
  int* flag;
  static constexpr bool kBox = false;
  static constexpr int kNIn = 4;
  __device__ __forceinline__ T call4(T g, T d, T x, T s, T, T, bool) const {
    // (raised once: a d that is wrong everywhere must not queue 1e8 atomics on one address -- 12 ns apiece)
    if (!(d > T(0)) && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(flag, 1);
    const T ci = sqrt(2 * lambda * d);                                               // :71
    const T xps = x + s;
    return (fabs(d * xps - g) <= ci) ? -xps : (-g / d);                              // :73-77
  }
};
template <class T>
struct IproxL1Box {  // src/shiftedNormL1Box.jl:131-225
  T lambda;
  static constexpr bool kBox = true;
  static constexpr int kNIn = 4;
  __device__ __forceinline__ T call4(T g, T d, T x, T s, T l, T u, bool sel) const {
    const T eps = std::numeric_limits<T>::epsilon();
    const T xs = x + s;
    const T left = l - s, right = u - s;
    T yi;
    if (fabs(d) <= eps) {  // :152
      yi = (fabs(g) <= lambda) ? jl_min(jl_max(left, -xs), right) : ((g > T(0)) ? left : right);
    } else {
      const T d_2 = d / 2;
      const T lx = l + x, ux = u + x;
      const T g2_d = g / d_2;
      const T f2_d = g2_d - 2 * xs;
      const T l2_d = lambda / d_2;
      const T val_left = lx * lx + f2_d * lx + l2_d * fabs(lx);
      const T val_right = ux * ux + f2_d * ux + l2_d * fabs(ux);
      if (d > eps) {  // :161
        T val_min = jl_min(val_left, val_right);
        yi = (val_left < val_right) ? left : right;
        const T y1 = -(g + lambda) / d;
        const T y2 = (lambda - g) / d;
        if (lx >= T(0)) {
          if (left <= y1 && y1 <= right) yi = y1;
        } else if (T(0) >= ux) {
          if (left <= y2 && y2 <= right) yi = y2;
        } else {
          if (left <= y1 && y1 <= right) {
            const T v1 = xs + y1;
            const T q1 = v1 * v1 + f2_d * v1 + l2_d * fabs(v1);
            if (q1 < val_min) yi = y1;
            val_min = jl_min(q1, val_min);
          }
          if (left <= y2 && y2 <= right) {
            const T v2 = xs + y2;
            const T q2 = v2 * v2 + f2_d * v2 + l2_d * fabs(v2);
            if (q2 < val_min) yi = y2;
            val_min = jl_min(q2, val_min);
          }
          if (T(0) < val_min) yi = -xs;  // val_0 = 0
        }
      } else {  // d <= -eps, :199
        const T val_max = jl_max(val_left, val_right);
        yi = (val_left > val_right) ? left : right;
        const T mx = -x;
        if (l <= mx && mx <= u && T(0) > val_max) yi = -xs;
      }
    }
    return sel ? yi : iprox_zero(d, g, left, right);  // :221
  }
};
template <class T>
struct IproxL0Box {  // src/shiftedNormL0Box.jl:137-231
  T lambda;
  static constexpr bool kBox = true;
  static constexpr int kNIn = 4;
  __device__ __forceinline__ T call4(T g, T d, T x, T s, T l, T u, bool sel) const {
    const T eps = std::numeric_limits<T>::epsilon();
    const T xs = x + s;
    const T mx = -x;
    const bool zero_ok = (l <= mx && mx <= u);
    const T left = l - s, right = u - s;
    T yi;
    if (fabs(d) < eps) {  // :154
      if (g == T(0)) {
        yi = zero_ok ? -xs : T(0);
      } else {
        const bool pos = g > T(0);
        const T t = pos ? left : right;
        const T val_min = g * t + ((x == (pos ? -l : -u)) ? T(0) : lambda);
        yi = t;
        if (zero_ok && (-g * xs) < val_min) yi = -xs;
      }
    } else {
      const T d_2 = d / 2;
      const T lx = l + x, ux = u + x;
      const T g2_d = g / d_2;
      const T f2_d = g2_d - 2 * xs;
      const T l2_d = lambda / d_2;
      const T val_left = (lx == T(0)) ? T(0) : (lx * lx + f2_d * lx + l2_d);
      const T val_right = (ux == T(0)) ? T(0) : (ux * ux + f2_d * ux + l2_d);
      if (d >= eps) {  // :190
        const T aqy = -g / d;
        const T aqv = aqy + xs;
        T val_min;
        if (lx <= aqv && aqv <= ux) {
          val_min = (aqv == T(0)) ? (-(aqv * aqv)) : (-(aqv * aqv) + l2_d);
          yi = aqy;
        } else {
          yi = (val_left < val_right) ? left : right;
          val_min = jl_min(val_left, val_right);
        }
        if (zero_ok && T(0) < val_min) yi = -xs;
      } else {  // :213
        yi = (val_left > val_right) ? left : right;
        const T val_max = jl_max(val_left, val_right);
        if (zero_ok && T(0) > val_max) yi = -xs;
      }
    }
    return sel ? yi : iprox_zero(d, g, left, right);  // :227
  }
};
struct OpIproxL1 : IproxL1<double> { static constexpr int kLdsKiB = 4; };
struct OpIproxL0 : IproxL0<double> { static constexpr int kLdsKiB = 4; };
// register-staged: five fp64 divisions per element want the occupancy (6.10 vs 5.70 TB/s)
struct OpIproxL1Box : IproxL1Box<double> { static constexpr int kLdsKiB = 0; };
struct OpIproxL0Box : IproxL0Box<double> { static constexpr int kLdsKiB = 4; };

// ---------------------------------------------------------------------------------------------
// prox! fused with the value of h at the result ("fused with prox where possible"): the kernels
// below add Term((xk + sj) + y) over the selected indices into one partial per wavefront / workgroup
// (src/ShiftedProximalOperators.jl:51-54 for the association), a second small kernel adds the partials in index order.
// ---------------------------------------------------------------------------------------------
// (the element terms of spx_common.hpp under names of this file's own, which the kernel names carry)
struct HTermL1 : TermL1 {};
struct HTermL0 : TermL0 {};
struct HTermLhalf : TermLhalf {};
template <class Base, class Term>
struct WithValue : Base {
  static constexpr int kSums = 1;
  double* partials;  // one slot per workgroup
  double qscale;     // the prox is taken at qscale * q (R2: q = -nu * grad f, formed on the fly; 1.0 = q itself)
  // (value_publish below) when the call is ONE launch of at most kValueFuseMax workgroups, the workgroup that finishes last
  // adds the partials itself and the k_value_reduce launch is not queued (fin_hdr != NULL)
  SpxSyncHeader* fin_hdr = nullptr;
  double* fin_result = nullptr;  // the library's result slots (read back by the host forms)
  double* fin_target = nullptr;  // the caller's device slots (SpxDest::dev, may be NULL)
  double fin_scale = 1.0;        // both receive fin_scale * (sum of the h terms)
  __device__ __forceinline__ double operator()(double q, double x, double s, double l, double u, bool sel) const {
    return Base::operator()(qscale * q, x, s, l, u, sel);
  }
  __device__ __forceinline__ double hterm(double x, double s, double y, bool sel, bool = false) const {
    return sel ? Term{}((x + s) + y) : 0.0;
  }
  __device__ __forceinline__ double hterm(f64x2 x, f64x2 s, f64x2 y, bool s0, bool s1) const {  // a 16-byte pair
    return hterm(x.x, s.x, y.x, s0) + hterm(x.y, s.y, y.y, s1);
  }
};
// prox! fused with the step statistics of a solver iteration (spx_proxstep_*): besides the h terms the lane that computes
// y[i] adds q[i] * y[i] (q as passed, not qscale * q) and y[i]^2 over ALL i, and stores (xk[i] + sj[i]) + y[i] -- the point
// at which h is evaluated -- to xkn when that is not NULL.  Three partial sums per slot, in three planes `plane` doubles
// apart (partials[slot], partials[plane + slot], partials[2 plane + slot]).
template <class Base, class Term>
struct WithStep : WithValue<Base, Term> {
  static constexpr int kSums = 3;
  double* xkn = nullptr;  // NULL: no store
  int64_t plane = 0;      // doubles between the planes of `partials`
};
// iprox! fused with the step statistics of a diagonal quasi-Newton iteration (spx_iproxstep_*): Base is one of the four Iprox*
// functors (kNIn = 4: call4(g, d, xk, sj, ...) is Base's own, so y keeps the bits of spx_iprox_X).  hterm, xkn, plane, partials
// and the fin_* fields are WithStep's (qscale is not read: g and d enter as they are).  Four partial sums per slot, in four
// planes: the h terms over the selected indices, then g[i] * y[i], (d[i] * y[i]) * y[i] -- twice the quadratic term of the
// model, the lane has d in a register -- and y[i]^2 over ALL i.
template <class Base, class Term>
struct WithIstep : WithStep<Base, Term> {
  static constexpr int kNIn = 4;
  static constexpr int kSums = 4;
};
// kSumsOf<Op>: the sums a call adds besides y -- 0 (plain prox! / iprox!), 1 (WithValue: h), 3 (WithStep: h, <q, y>, <y, y>),
// 4 (WithIstep: h, <g, y>, <d .* y, y>, <y, y>).
// Everything below is written once over that count: plane p of a list of partials is added with the same statements, hence
// in the same order and to the same bits, whether it is the only plane or one of three or four.
template <class Op, class = void>
struct SumsOf { static constexpr int value = 0; };
template <class Op>
struct SumsOf<Op, decltype((void)Op::kSums)> { static constexpr int value = Op::kSums; };
template <class Op>
constexpr int kSumsOf = SumsOf<Op>::value;
// A lane's (then a workgroup's) sums.  Handed to the functions below and returned BY VALUE: an accumulator that a kernel
// passes by reference, or indexes by a loop variable, stays in memory until inlining and unrolling are done, and the element
// loops then compile to other code than with the statements written out at their sites (k_sep_vec<WithStep<OpL1, ...>>: 90
// VGPRs and five waves per SIMD instead of 80 and six; by value every kernel keeps its registers: profiles/sep_finish_kres.txt).
template <int NS>
struct SepSums { double v[NS]; };
template <class Op>
using SumsFor = SepSums<(kSumsOf<Op> > 0 ? kSumsOf<Op> : 1)>;  // (no array of length 0)
template <class Op>
__device__ __forceinline__ int64_t plane_of(const Op& op) {
  if constexpr (kSumsOf<Op> > 1) return op.plane;
  else return 0;
}

// a.v[p] summed over the first 256 lanes of a workgroup, for NS planes across one pair of barriers: wavefront butterflies,
// then the four wavefronts in order.  Every lane of the workgroup must call it; the result is valid in all of them.
template <int NS>
__device__ __forceinline__ SepSums<NS> block_sum4(SepSums<NS> a) {
  __shared__ double bs_lds[NS][4];
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < NS; ++p) a.v[p] = wave_sum(a.v[p]);
  __syncthreads();
  if ((t & 63) == 0 && t < 256) {
#pragma unroll
    for (int p = 0; p < NS; ++p) bs_lds[p][t >> 6] = a.v[p];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < NS; ++p) a.v[p] = (bs_lds[p][0] + bs_lds[p][1]) + (bs_lds[p][2] + bs_lds[p][3]);
  return a;
}
// The same sum for k_sep_lds, valid in thread 0 only, across ONE barrier and without LDS of its own: the wave's staging area
// `wl` (of `wave_bytes`, the first of them at `lds`) has been consumed, its first 8 NS bytes carry the wave's sums to thread 0.
template <int NS>
__device__ __forceinline__ SepSums<NS> block_sum4_staged(SepSums<NS> a, char* wl, const char* lds, int wave_bytes) {
#pragma unroll
  for (int p = 0; p < NS; ++p) a.v[p] = wave_sum(a.v[p]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int p = 0; p < NS; ++p) reinterpret_cast<double*>(wl)[p] = a.v[p];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* w0 = reinterpret_cast<const double*>(lds);
    const int stride = wave_bytes / 8;
#pragma unroll
    for (int p = 0; p < NS; ++p) a.v[p] = (w0[p] + w0[stride + p]) + (w0[2 * stride + p] + w0[3 * stride + p]);
  }
  return a;
}
// .v[p] = the sum of partials[p * plane + (0..count)), count <= kValueFuseMax, added by the first 256 lanes of a workgroup in
// a fixed order (all 8 NS loads of a lane in flight before the first add -- one memory round trip, whatever NS is -- a fixed
// tree, then block_sum4): the order of BOTH the one-launch form (ATOMIC: the slots were written by other workgroups of the
// same launch) and k_value_reduce on short lists, so that the two forms of a call give the same bits.  Every lane of the
// workgroup must call it.
constexpr int kValueFuseMax = 2048;
template <bool ATOMIC, int NS>
__device__ __forceinline__ SepSums<NS> value_reduce_small(const double* partials, int64_t plane, int count) {
  const int t = threadIdx.x;
  double v8[NS][8];
#pragma unroll
  for (int p = 0; p < NS; ++p) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = t + k * 256;
      const bool in = t < 256 && i < count;
      if constexpr (ATOMIC) v8[p][k] = in ? spx_atomic_load_f64(partials + p * plane + i) : 0.0;
      else v8[p][k] = in ? partials[p * plane + i] : 0.0;
    }
  }
  SepSums<NS> a;
#pragma unroll
  for (int p = 0; p < NS; ++p)
    a.v[p] = ((v8[p][0] + v8[p][1]) + (v8[p][2] + v8[p][3])) + ((v8[p][4] + v8[p][5]) + (v8[p][6] + v8[p][7]));
  return block_sum4(a);
}
// The partial sums t.v[0..NS) of this workgroup (valid in thread 0) go to its slot of the NS planes.  value_store: a later
// launch adds them -- all there is to do in a launch that can never be the only one of its call.  value_publish: in the
// one-launch form ONE ticket per workgroup (spx_fin_ticket) publishes all NS of them, and the workgroup that takes the last
// one adds the planes and stores {fin_scale * h, <q, y>, <y, y>} (NS = 1: the first of them; NS = 4: {fin_scale * h, <g, y>, <d .* y, y>, <y, y>}) to the library's result slots and
// to fin_target if set.  Every lane of the workgroup must call it.
template <class Op, int NS>
__device__ __forceinline__ void value_store(const Op& op, int64_t slot, SepSums<NS> t) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < NS; ++p) op.partials[p * plane_of(op) + slot] = t.v[p];
  }
}
template <class Op, int NS>
__device__ __forceinline__ void value_publish(const Op& op, int64_t slot, SepSums<NS> t) {
  if (op.fin_hdr == nullptr) return value_store(op, slot, t);
  const int64_t plane = plane_of(op);
  __shared__ int vp_last;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < NS; ++p) spx_atomic_store_f64(op.partials + p * plane + slot, t.v[p]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    vp_last = spx_fin_ticket(op.fin_hdr) ? 1 : 0;
  }
  __syncthreads();
  if (!vp_last) return;
  SepSums<NS> sum = value_reduce_small<true, NS>(op.partials, plane, (int)gridDim.x);
  if (threadIdx.x == 0) {
    sum.v[0] = op.fin_scale * sum.v[0];
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      op.fin_result[p] = sum.v[p];
      if (op.fin_target) op.fin_target[p] = sum.v[p];
    }
  }
}

// Workgroup b adds plane b of the partials, partials[b * plane + (0..count)), in a fixed order (reproducible run to run) and
// stores out[b], and target[b] when target != NULL (the caller's device slots): {scale * h, <q, y>, <y, y>} (NS = 4:
// {scale * h, <g, y>, <d .* y, y>, <y, y>}).
// Grid: NS workgroups.
template <int NS>
__global__ __launch_bounds__(1024) void k_value_reduce(const double* partials, int64_t plane, int64_t count, double* out,
                                                        double scale, double* target) {
  __shared__ double lds[16];
  const int b = (NS == 1) ? 0 : (int)blockIdx.x;
  partials += (int64_t)b * plane;
  double t = 0.0;
  if (count <= kValueFuseMax) {  // (the order of the one-launch form)
    t = value_reduce_small<false, 1>(partials, 0, (int)count).v[0];
  } else {
    // eight independent loads in flight per lane
    double a8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i0 = threadIdx.x; i0 < count; i0 += 8 * 1024) {
      double v8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t i = i0 + (int64_t)k * 1024;
        v8[k] = (i < count) ? partials[i < count ? i : 0] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) a8[k] += v8[k];
    }
    double acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < 16; ++w) t += lds[w];
    }
  }
  if (threadIdx.x == 0) {
    const double v = (b == 0) ? scale * t : t;
    out[b] = v;
    if (target) target[b] = v;
  }
}

// uniform call: 3-input operators ignore d
template <class Op, class T>
__device__ __forceinline__ T apply_op(const Op& op, T q, T d, T x, T s, T l, T u, bool sel) {
  if constexpr (Op::kNIn == 4) return op.call4(q, d, x, s, l, u, sel);
  else return op(q, x, s, l, u, sel);
}

// ---------------------------------------------------------------------------------------------
// streaming skeleton
// ---------------------------------------------------------------------------------------------
template <bool NT>
__device__ __forceinline__ f64x2 ld2(const f64x2* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, class V>
__device__ __forceinline__ void st2(V* p, V v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
// (xk + sj) + y, the point at which h is evaluated: element by element, the expression of hterm, whose value the compiler reuses
__device__ __forceinline__ double at_point(double x, double s, double y) { return (x + s) + y; }
__device__ __forceinline__ f64x2 at_point(f64x2 x, f64x2 s, f64x2 y) { return f64x2{(x.x + s.x) + y.x, (x.y + s.y) + y.y}; }
__device__ __forceinline__ double sum_prod(double a, double b) { return a * b; }
__device__ __forceinline__ double sum_prod(f64x2 a, f64x2 b) { return a.x * b.x + a.y * b.y; }
// (d * y) * y in that association (the library is built without contraction), the term of <d .* y, y>
__device__ __forceinline__ double sum_prod3(double d, double y) { return (d * y) * y; }
__device__ __forceinline__ double sum_prod3(f64x2 d, f64x2 y) { return (d.x * y.x) * y.x + (d.y * y.y) * y.y; }
// The sums and the xkn store of one element site, written once for the three kernels: V = f64x2 is the 16-byte pair `i` of
// the vector skeletons (s0, s1: its selection bits), V = double element `i` of the scalar kernel (s0).  q, x, s: the loaded
// q (as passed, unscaled), d (read by the four-sum form only), xk, sj; r: the result(s).  NT: the store to xn (NULL: none) is
// non-temporal.  Returns acc with the site's terms added (by value: see SepSums).  The last plane is always <y, y>.
template <bool NT, class Op, class V>
__device__ __forceinline__ SumsFor<Op> sep_accumulate(const Op& op, SumsFor<Op> acc, V q, V d, V x, V s, V r, bool s0, bool s1,
                                                      V* xn, int64_t i) {
  constexpr int NS = kSumsOf<Op>;
  if constexpr (NS >= 1) acc.v[0] += op.hterm(x, s, r, s0, s1);
  if constexpr (NS >= 3) {
    acc.v[1] += sum_prod(q, r);
    if constexpr (NS == 4) acc.v[2] += sum_prod3(d, r);
    acc.v[NS - 1] += sum_prod(r, r);
    if (xn) st2<NT>(xn + i, at_point(x, s, r));
  }
  return acc;
}
// (WithStep, WithIstep) where xkn goes, as pairs or elements; NULL: no store
template <class V, class Op>
__device__ __forceinline__ V* xkn_of(const Op& op) {
  if constexpr (kSumsOf<Op> >= 3) return reinterpret_cast<V*>(op.xkn);
  else return nullptr;
}

// ---------------------------------------------------------------------------------------------
// The operator table and the C entry points
// ---------------------------------------------------------------------------------------------
// One row per operator names its Float64 functor (Op), its Float32 functor (F32, where there is one), its
// h term and make<O>: the functor O's constants from (lambda, sigma).  Every entry point of an operator is run_...<Row>, so
// y of spx_prox_X, spx_proxval_X and spx_proxstep_X has the same bits: the three take the functor from the same row.
namespace {
struct F32L1 : ProxL1<float> {};
struct F32L1Aliased : ProxL1Aliased<float> {};
struct F32L0 : ProxL0<float> {};
struct F32L1Box : ProxL1Box<float> {};
struct F32L0Box : ProxL0Box<float> {};
struct F32IproxL1 : IproxL1<float> {};
struct F32IproxL0 : IproxL0<float> {};
struct F32IproxL1Box : IproxL1Box<float> {};
struct F32IproxL0Box : IproxL0Box<float> {};

struct RowL1 {
  using Op = OpL1; using F32 = F32L1; using Term = HTermL1;
  template <class O, class T> __host__ __device__ static O make(T lambda, T sigma) { return O{lambda * sigma}; }
};
struct RowL1Aliased {  // NormL1 with y === q: the reference's two-pass body overwrites q before it reads it
  using Op = OpL1Aliased; using F32 = F32L1Aliased; using Term = HTermL1;
  template <class O, class T> static O make(T, T) { return O{}; }
};
struct RowL0 {
  using Op = OpL0; using F32 = F32L0; using Term = HTermL0;
  template <class O, class T> __host__ __device__ static O make(T lambda, T sigma) { return O{std::sqrt(2 * lambda * sigma)}; }
};
struct RowLhalf {
  using Op = OpLhalf; using Term = HTermLhalf;
  template <class O> static O make(double lambda, double sigma) {
    const double nl = sigma * lambda;
    const double p = std::pow(54.0, 1.0 / 3.0) * std::pow(2 * nl, 2.0 / 3.0) / 4;  // shiftedRootNormLhalf.jl:49
    return O{nl / 4, p};
  }
};
struct RowL1Box {
  using Op = OpL1Box; using F32 = F32L1Box; using Term = HTermL1;
  template <class O, class T> __host__ __device__ static O make(T lambda, T sigma) { return O{sigma * lambda}; }
};
struct RowL0Box {
  using Op = OpL0Box; using F32 = F32L0Box; using Term = HTermL0;
  template <class O, class T> __host__ __device__ static O make(T lambda, T sigma) { return O{2 * lambda * sigma}; }
};
struct RowLhalfBox {
  using Op = OpLhalfBox; using Term = HTermLhalf;
  template <class O> static O make(double lambda, double sigma) { return O{sigma * lambda / 4, lambda, 0.5 / sigma}; }
};
// iprox!: the functors are {lambda} -- kFlagged: {lambda, flag}, the word they raise where d[i] <= 0
struct RowIproxL1 { using Op = OpIproxL1; using F32 = F32IproxL1; using Term = HTermL1; static constexpr bool kFlagged = true; };
struct RowIproxL0 { using Op = OpIproxL0; using F32 = F32IproxL0; using Term = HTermL0; static constexpr bool kFlagged = true; };
struct RowIproxL1Box { using Op = OpIproxL1Box; using F32 = F32IproxL1Box; using Term = HTermL1; static constexpr bool kFlagged = false; };
struct RowIproxL0Box { using Op = OpIproxL0Box; using F32 = F32IproxL0Box; using Term = HTermL0; static constexpr bool kFlagged = false; };
template <class Row, class T>
using RowOp = std::conditional_t<std::is_same<T, double>::value, typename Row::Op, typename Row::F32>;  // (rows with both)
}  // namespace
