// spx_separable.hip -- the six separable prox! kernels (ShiftedNormL1/L0/RootNormLhalf and their Box
// forms) and iprox!, on Float64 and (L1 / L0 forms) Float32 vectors.  One streaming skeleton per precision, one functor
// per operator.
//
// HBM layout: q, xk, sj, y (and l, u when they are vectors) are plain contiguous fp64 vectors.
// Algorithmic traffic: 3 reads + 1 write = 32 B/element (48 B with vector bounds, +1 B with a mask).
// Roofline: HBM bandwidth (no reuse, no contraction -> MFMA not applicable).
//
// Skeleton: a workgroup of 256 lanes walks tiles of 256*UNROLL 16-byte pairs with a block stride.
// Within a tile every wave instruction touches 1 KiB contiguous (lane i -> base + 16*i), all
// 3*UNROLL loads of a tile are issued before the first use so each lane keeps 3*UNROLL*16 B in
// flight, results are written with 16-byte stores.  q[i] is read before y[i] is written by the same
// lane and no other lane touches index i, so y may alias q.
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

// n2 = number of 16-byte pairs.  VECB: l/u are vectors.  MASK: sel mask present.
template <class Op, int UNROLL, bool VECB, bool MASK, bool NT>
__global__ __launch_bounds__(256) void k_sep_vec(double* y_, const double* q_, const double* d_, const double* xk_,
                                                  const double* sj_, const double* l_, const double* u_,
                                                  const uint8_t* mask_, double ls, double us, int64_t n2, Op op) {
  const f64x2* dv = reinterpret_cast<const f64x2*>(d_);
  constexpr int64_t TILE = 256 * UNROLL;
  f64x2* y = reinterpret_cast<f64x2*>(y_);
  const f64x2* q = reinterpret_cast<const f64x2*>(q_);
  const f64x2* xk = reinterpret_cast<const f64x2*>(xk_);
  const f64x2* sj = reinterpret_cast<const f64x2*>(sj_);
  const f64x2* lv = reinterpret_cast<const f64x2*>(l_);
  const f64x2* uv = reinterpret_cast<const f64x2*>(u_);
  const uint16_t* mk = reinterpret_cast<const uint16_t*>(mask_);
  const int64_t ntiles = (n2 + TILE - 1) / TILE;
  SumsFor<Op> acc = {};
  f64x2* const xn = xkn_of<f64x2>(op);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * TILE + threadIdx.x;
    f64x2 vq[UNROLL], vx[UNROLL], vs[UNROLL], vl[UNROLL], vu[UNROLL], vd[UNROLL];
    uint16_t vm[UNROLL];
    if (base - threadIdx.x + TILE <= n2) {
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t i = base + k * 256;
        vq[k] = ld2<NT>(q + i);
        if constexpr (Op::kNIn == 4) vd[k] = ld2<NT>(dv + i); else vd[k] = f64x2{0.0, 0.0};
        vx[k] = ld2<NT>(xk + i);
        vs[k] = ld2<NT>(sj + i);
        if constexpr (VECB && Op::kBox) {
          vl[k] = l_ ? ld2<NT>(lv + i) : f64x2{ls, ls};
          vu[k] = u_ ? ld2<NT>(uv + i) : f64x2{us, us};
        }
        if constexpr (MASK && Op::kBox) vm[k] = mk[i];
      }
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t i = base + k * 256;
        double l0 = ls, l1 = ls, u0 = us, u1 = us;
        bool s0 = true, s1 = true;
        if constexpr (VECB && Op::kBox) { l0 = vl[k].x; l1 = vl[k].y; u0 = vu[k].x; u1 = vu[k].y; }
        if constexpr (MASK && Op::kBox) { s0 = (vm[k] & 0xff) != 0; s1 = (vm[k] >> 8) != 0; }
        f64x2 r;
        r.x = apply_op(op, vq[k].x, vd[k].x, vx[k].x, vs[k].x, l0, u0, s0);
        r.y = apply_op(op, vq[k].y, vd[k].y, vx[k].y, vs[k].y, l1, u1, s1);
        acc = sep_accumulate<NT>(op, acc, vq[k], vd[k], vx[k], vs[k], r, s0, s1, xn, i);
        st2<NT>(y + i, r);
      }
    } else {  // last, partial tile
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t i = base + k * 256;
        if (i < n2) {
          f64x2 a = q[i], b = xk[i], c = sj[i];
          f64x2 dd = f64x2{0.0, 0.0};
          if constexpr (Op::kNIn == 4) dd = dv[i];
          double l0 = ls, l1 = ls, u0 = us, u1 = us;
          bool s0 = true, s1 = true;
          if constexpr (VECB && Op::kBox) {
            if (l_) { f64x2 t = lv[i]; l0 = t.x; l1 = t.y; }
            if (u_) { f64x2 t = uv[i]; u0 = t.x; u1 = t.y; }
          }
          if constexpr (MASK && Op::kBox) { uint16_t m = mk[i]; s0 = (m & 0xff) != 0; s1 = (m >> 8) != 0; }
          f64x2 r;
          r.x = apply_op(op, a.x, dd.x, b.x, c.x, l0, u0, s0);
          r.y = apply_op(op, a.y, dd.y, b.y, c.y, l1, u1, s1);
          acc = sep_accumulate<false>(op, acc, a, dd, b, c, r, s0, s1, xn, i);
          y[i] = r;
        }
      }
    }
  }
  if constexpr (kSumsOf<Op> > 0) value_publish(op, blockIdx.x, block_sum4(acc));
}

// ---------------------------------------------------------------------------------------------
// LDS-staged skeleton (the default): each wavefront owns a contiguous chunk of UNROLL KiB per input vector and
// stages it through LDS with `global_load_lds_dwordx4 ... nt` -- LDS-DMA: no VGPR destination, one contiguous
// 1 KiB piece per wave instruction -- then waits once (vmcnt(0)), reads its own 16 bytes per piece back with
// ds_read_b128 (lane-private slots: conflict-free, no barrier: nothing is shared between waves), evaluates
// the operator and writes y with non-temporal 16-byte stores.  3*UNROLL KiB are in flight per wave without
// holding registers; UNROLL = 6 -> 72 KiB of LDS per 4-wave workgroup -> two workgroups (144 KiB in flight)
// per CU.  Measured on MI355X (tools/exp/exp_stream.hip, n = 1e8, same process, interleaved rounds):
// 6.45-6.57 TB/s against 6.11-6.30 TB/s for the register-staged form above; 7 KiB per wave and more (one
// workgroup per CU) or a piece-by-piece pipelined wait lose 10-20 %.
// All loads of a wave have landed before its first store, and waves touch disjoint ranges: y may alias q.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ void dma16_nt(const f64x2* g, char* wave_lds_piece) {
  __builtin_amdgcn_global_load_lds((const void*)g, (lds_void*)wave_lds_piece, 16, 0, 2);  // aux = 2: nt
}

template <class Op, int UNROLL, bool VECB, bool MASK>
__global__ __launch_bounds__(256) void k_sep_lds(double* y_, const double* q_, const double* d_, const double* xk_,
                                                  const double* sj_, const double* l_, const double* u_,
                                                  const uint8_t* mask_, double ls, double us, int64_t n2, Op op,
                                                  int64_t xcd_chunk) {
  constexpr int NARR = Op::kNIn + ((VECB && Op::kBox) ? 2 : 0);
  const f64x2* dv = reinterpret_cast<const f64x2*>(d_);
  __shared__ __attribute__((aligned(16))) char lds[4 * NARR * UNROLL * 1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  char* wl = lds + wave * (NARR * UNROLL * 1024);
  f64x2* y = reinterpret_cast<f64x2*>(y_);
  const f64x2* q = reinterpret_cast<const f64x2*>(q_);
  const f64x2* xk = reinterpret_cast<const f64x2*>(xk_);
  const f64x2* sj = reinterpret_cast<const f64x2*>(sj_);
  const f64x2* lv = reinterpret_cast<const f64x2*>(l_);
  const f64x2* uv = reinterpret_cast<const f64x2*>(u_);
  const uint16_t* mk = reinterpret_cast<const uint16_t*>(mask_);
  // Workgroups are dealt to the 8 XCDs round-robin.  xcd_chunk == 0 (default): tile = workgroup id, so neighbouring tiles
  // land on different XCDs; xcd_chunk > 0 (spx_ctx_set_tuning key 5, experiment): XCD x works through the contiguous range
  // [x * xcd_chunk, (x + 1) * xcd_chunk) of tiles.  No tile is ever re-read, so neither L2 has anything to win -- measured.
  int64_t bid = blockIdx.x;
  if (xcd_chunk > 0) {
    bid = (int64_t)(blockIdx.x & 7) * xcd_chunk + (blockIdx.x >> 3);
    if (bid * (256 * UNROLL) >= n2) {
      if constexpr (kSumsOf<Op> > 0) {
        value_store(op, bid, SumsFor<Op>{});  // (a slot of its own: every slot the host counts is written; never the one-launch form)
      }
      return;
    }
  }
  const int64_t base = (bid * 4 + wave) * (64 * UNROLL) + lane;  // this lane's first pair
  SumsFor<Op> acc = {};
  f64x2* const xn = xkn_of<f64x2>(op);
  uint16_t vm[UNROLL];
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    int64_t i = base + k * 64;
    if (i >= n2) i = n2 - 1;  // tail: load something valid, the store is guarded
    dma16_nt(q + i, wl + (0 * UNROLL + k) * 1024);
    dma16_nt(xk + i, wl + (1 * UNROLL + k) * 1024);
    dma16_nt(sj + i, wl + (2 * UNROLL + k) * 1024);
    if constexpr (Op::kNIn == 4) dma16_nt(dv + i, wl + (3 * UNROLL + k) * 1024);
    if constexpr (VECB && Op::kBox) {
      if (l_) dma16_nt(lv + i, wl + ((Op::kNIn + 0) * UNROLL + k) * 1024);
      if (u_) dma16_nt(uv + i, wl + ((Op::kNIn + 1) * UNROLL + k) * 1024);
    }
    if constexpr (MASK && Op::kBox) vm[k] = mk[i];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every piece of this wave has landed in LDS
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int64_t i = base + k * 64;
    const f64x2 a = *reinterpret_cast<const f64x2*>(wl + (0 * UNROLL + k) * 1024 + lane * 16);
    const f64x2 b = *reinterpret_cast<const f64x2*>(wl + (1 * UNROLL + k) * 1024 + lane * 16);
    const f64x2 c = *reinterpret_cast<const f64x2*>(wl + (2 * UNROLL + k) * 1024 + lane * 16);
    double l0 = ls, l1 = ls, u0 = us, u1 = us;
    bool s0 = true, s1 = true;
    f64x2 dd = f64x2{0.0, 0.0};
    if constexpr (Op::kNIn == 4) dd = *reinterpret_cast<const f64x2*>(wl + (3 * UNROLL + k) * 1024 + lane * 16);
    if constexpr (VECB && Op::kBox) {
      if (l_) { const f64x2 t = *reinterpret_cast<const f64x2*>(wl + ((Op::kNIn + 0) * UNROLL + k) * 1024 + lane * 16); l0 = t.x; l1 = t.y; }
      if (u_) { const f64x2 t = *reinterpret_cast<const f64x2*>(wl + ((Op::kNIn + 1) * UNROLL + k) * 1024 + lane * 16); u0 = t.x; u1 = t.y; }
    }
    if constexpr (MASK && Op::kBox) { s0 = (vm[k] & 0xff) != 0; s1 = (vm[k] >> 8) != 0; }
    f64x2 r;
    r.x = apply_op(op, a.x, dd.x, b.x, c.x, l0, u0, s0);
    r.y = apply_op(op, a.y, dd.y, b.y, c.y, l1, u1, s1);
    if constexpr (kSumsOf<Op> > 0) {  // (the tail's lanes hold a copy of the last pair)
      if (i < n2) acc = sep_accumulate<true>(op, acc, a, dd, b, c, r, s0, s1, xn, i);  // (xkn out of registers: the extra store needs no LDS)
    }
    if (i < n2) __builtin_nontemporal_store(r, y + i);
  }
  // one slot per WORKGROUP (one per wavefront meant 130 208 of them at n = 1e8, and ~25 us of ordered reduction behind the pass)
  if constexpr (kSumsOf<Op> > 0) value_publish(op, bid, block_sum4_staged(acc, wl, lds, NARR * UNROLL * 1024));
}

// scalar path: unaligned vectors, and the odd last element of the vector path ([begin, n))
template <class Op>
__global__ __launch_bounds__(256) void k_sep_scalar(double* y, const double* q, const double* d_, const double* xk,
                                                     const double* sj, const double* l_, const double* u_,
                                                     const uint8_t* mask, double ls, double us, int64_t begin,
                                                     int64_t n, Op op) {
  int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  SumsFor<Op> acc = {};
  double* const xn = xkn_of<double>(op);  // (indexed from element 0)
  for (; i < n; i += stride) {
    double li = l_ ? l_[i] : ls;
    double ui = u_ ? u_[i] : us;
    bool sel = mask ? (mask[i] != 0) : true;
    double di = 0.0;
    if constexpr (Op::kNIn == 4) di = d_[i];
    const double xi = xk[i], si = sj[i];
    const double qi = q[i];
    const double yi = apply_op(op, qi, di, xi, si, li, ui, sel);
    acc = sep_accumulate<false>(op, acc, qi, di, xi, si, yi, sel, false, xn, i);
    y[i] = yi;
  }
  if constexpr (kSumsOf<Op> > 0) value_store(op, blockIdx.x, block_sum4(acc));  // (never the only launch of a call)
}

// Tuning knobs (spx_ctx_set_tuning).  Defaults from tools/sweep_sep.py on MI355X, n = 1e8 (profiles/r01_sweep_sep.txt):
// one tile per workgroup (no cap) + non-temporal loads/stores: 6.15 TB/s vs 5.66 TB/s for 16 WG/CU, plain.
// (the knobs live in the context: spx_ctx::tune_sep_*, set by spx_ctx_set_tuning)

#ifndef SPX_VECB_KIB
#define SPX_VECB_KIB 3  // KiB per wave and vector with vector bounds (5 vectors); measured at n = 1e8 (tools/bench_vecb.py): 2 -> 0.81 ms, 3 -> 0.76 ms, 4 -> 0.775 ms
#endif
template <class Op, bool VECB, bool MASK>
static int launch_vec(const SepCall<double>& c /* at its 16-byte aligned body */, int64_t n2, Op op,
                      int64_t* value_slots /* out: partial slots written (kSumsOf<Op> > 0) */,
                      const SpxSyncHeader* fuse_hdr = nullptr /* kSumsOf<Op> > 0: this launch is the whole call -- it may finish the sums itself */,
                      bool* fused = nullptr) {
  spx_ctx* const ctx = c.ctx;
  const SpxBox<double>& b = c.box;
  // (kSumsOf<Op> > 0) the one-launch form: the grid is the list of slots, short enough for one workgroup to add
  auto try_fuse = [&](int64_t blocks) {
    if constexpr (kSumsOf<Op> > 0) {
      if (fuse_hdr != nullptr && blocks <= kValueFuseMax && !ctx->tune_sep_xcd) {
        op.fin_hdr = const_cast<SpxSyncHeader*>(fuse_hdr);
        *fused = true;
      }
    }
  };
  if constexpr (Op::kLdsKiB > 0) if (ctx->tune_sep_lds) {
    // 3 input vectors: 6 KiB per wave and vector -> 72 KiB per workgroup; 5 vectors (vector bounds): 3 KiB -> 60 KiB
    constexpr int U = (VECB && Op::kBox) ? (Op::kLdsKiB > SPX_VECB_KIB ? SPX_VECB_KIB : Op::kLdsKiB) : Op::kLdsKiB;  // <= 72 KiB per workgroup
    int64_t blocks = (n2 + 256 * U - 1) / (256 * U);
    int64_t xcd_chunk = 0;
    if (ctx->tune_sep_xcd) {
      xcd_chunk = (blocks + 7) / 8;
      blocks = xcd_chunk * 8;
    }
    *value_slots = blocks;  // one per workgroup (idle workgroups of the XCD-contiguous experiment write a zero)
    try_fuse(blocks);
    hipLaunchKernelGGL((k_sep_lds<Op, U, VECB, MASK>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.d, c.xk,
                       c.sj, b.l, b.u, b.mask, b.ls, b.us, n2, op, xcd_chunk);
    SPX_LAUNCH_CHECK();
    return SPX_OK;
  }
  constexpr int UNROLL = 4;
  const int64_t ntiles = (n2 + 256 * UNROLL - 1) / (256 * UNROLL);
  int64_t blocks = ntiles;
  const int64_t cap = ctx->tune_sep_blocks_per_cu > 0 ? (int64_t)ctx->num_cu * ctx->tune_sep_blocks_per_cu : (int64_t)0x7fffffff;
  if (blocks > cap) blocks = cap;
  *value_slots = blocks;  // one per workgroup
  try_fuse(blocks);
  if (ctx->tune_sep_nt)
    hipLaunchKernelGGL((k_sep_vec<Op, UNROLL, VECB, MASK, true>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y,
                       c.q, c.d, c.xk, c.sj, b.l, b.u, b.mask, b.ls, b.us, n2, op);
  else
    hipLaunchKernelGGL((k_sep_vec<Op, UNROLL, VECB, MASK, false>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       c.y, c.q, c.d, c.xk, c.sj, b.l, b.u, b.mask, b.ls, b.us, n2, op);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}

// The workspace of a call with sums: [NS result doubles | kSepFlagOffset: the d > 0 flag word of spx_iproxstep_* | pad to 256 B
// | NS planes of partial slots].  sep_plane: doubles per plane, at least the slots of any route.
constexpr size_t kSepFlagOffset = 128;
static int64_t sep_plane(const spx_ctx* ctx, int64_t n) { return ((n / 2) / (256 * 3) + 2) * 4 + 2 * (int64_t)ctx->num_cu * 8 + 16; }
static size_t sep_ws_bytes(const spx_ctx* ctx, int64_t n, int ns) { return 256 + (size_t)ns * (size_t)sep_plane(ctx, n) * sizeof(double); }
// kSumsOf<Op> > 0: the sums {value_scale * h, <q, y>, <y, y>} (WithValue: the first of them; WithIstep: the four) go to the library's result slots,
// to dest.dev (device doubles, or NULL) and, when dest.host != NULL, back to the host -- that form synchronises and is
// refused under a capture; those callers answer n == 0 themselves.
template <class Op>
static int run_separable(const SepCall<double>& c, Op op, const SpxDest& dest = {nullptr, nullptr, 0}, double value_scale = 1.0) {
  constexpr int NS = kSumsOf<Op>;
  spx_ctx* const ctx = c.ctx;
  const int64_t n = c.n;
  if (n == 0) return SPX_OK;
  SPX_ON_DEVICE(ctx);
  double* partials = nullptr;  // ws: [results | pad to 256 B | NS planes of partial slots]
  int64_t used = 0, plane = 0;
  if constexpr (NS > 0) {
    plane = sep_plane(ctx, n);
    int rcw = spx_ws_reserve(ctx, sep_ws_bytes(ctx, n, NS));
    if (rcw) return rcw;
    partials = reinterpret_cast<double*>(static_cast<char*>(ctx->ws) + 256);
    if constexpr (NS > 1) op.plane = plane;
    if (ctx->tune_fewer_launches) {  // (the one-launch form keeps its tickets in the synchronisation state)
      rcw = spx_sync_ready(ctx);
      if (rcw) return rcw;
    }
  }
  bool fused = false;
  auto launch_scalar = [&](int64_t begin, int64_t end) -> int {
    int64_t blocks = (end - begin + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    if constexpr (NS > 0) op.partials = partials + used;
    if constexpr (NS >= 3) op.xkn = c.xkn;  // (indexed from element 0)
    hipLaunchKernelGGL((k_sep_scalar<Op>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.d, c.xk, c.sj, c.box.l,
                       c.box.u, c.box.mask, c.box.ls, c.box.us, begin, end, op);
    SPX_LAUNCH_CHECK();
    used += blocks;
    return SPX_OK;
  };
  // The vector skeletons need 16-byte aligned vectors (and a 2-byte aligned mask).  Views that all start 8 bytes off
  // (e.g. view(x, 2:n) of aligned arrays) are peeled: element 0 through the scalar kernel, the rest aligned again.
  int64_t head = 0;
  if (!c.aligned16_at(0) && n >= 3 && c.aligned16_at(1)) head = 1;
  int64_t done = 0;
  if (head) {
    int rch = launch_scalar(0, head);
    if (rch) return rch;
    done = head;
  }
  if (c.aligned16_at(head) && n - head >= 2) {
    const int64_t n2 = (n - head) / 2;
    const SepCall<double> v = c.shifted(head);
    int rc;
    int64_t slots = 0;
    const SpxSyncHeader* fh = nullptr;
    if constexpr (NS > 0) {
      op.partials = partials + used;
      // one launch covers the whole vector (no peeled element in front, no odd element behind): it may finish the sums
      if (ctx->tune_fewer_launches && head == 0 && 2 * n2 == n) {
        fh = spx_sync_header(ctx);
        op.fin_result = reinterpret_cast<double*>(ctx->ws);
        op.fin_target = dest.dev;
        op.fin_scale = value_scale;
      }
    }
    if constexpr (NS >= 3) op.xkn = v.xkn;
    if constexpr (Op::kBox) {
      const bool vecb = (v.box.l || v.box.u);
      const bool msk = (v.box.mask != nullptr);
      if (vecb && msk) rc = launch_vec<Op, true, true>(v, n2, op, &slots, fh, &fused);
      else if (vecb) rc = launch_vec<Op, true, false>(v, n2, op, &slots, fh, &fused);
      else if (msk) rc = launch_vec<Op, false, true>(v, n2, op, &slots, fh, &fused);
      else rc = launch_vec<Op, false, false>(v, n2, op, &slots, fh, &fused);
    } else {
      rc = launch_vec<Op, false, false>(v, n2, op, &slots, fh, &fused);
    }
    if (rc) return rc;
    used += slots;
    done = head + 2 * n2;
  }
  if (done < n) {
    int rct = launch_scalar(done, n);
    if (rct) return rct;
  }
  if constexpr (NS > 0) {
    double* result = reinterpret_cast<double*>(ctx->ws);
    if (!fused) {
      hipLaunchKernelGGL(k_value_reduce<NS>, dim3(NS), dim3(1024), 0, ctx->stream, (const double*)partials, plane, used, result,
                         value_scale, dest.dev);
      SPX_LAUNCH_CHECK();
    }
    const int rcc = spx_dest_check_capture(ctx, dest, NS == 1 ? "returning the value of prox_value to the host"
                                                              : "returning the step statistics to the host (pass stats = NULL)");
    if (rcc) return rcc;
    return spx_dest_return(ctx, dest, result, NS * sizeof(double));
  }
  return SPX_OK;
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
  template <class O, class T> static O make(T lambda, T sigma) { return O{lambda * sigma}; }
};
struct RowL1Aliased {  // NormL1 with y === q: the reference's two-pass body overwrites q before it reads it
  using Op = OpL1Aliased; using F32 = F32L1Aliased; using Term = HTermL1;
  template <class O, class T> static O make(T, T) { return O{}; }
};
// ... which holds for lambda * sigma >= 0 (see ProxL1Aliased).  The Float32 form takes it for any lambda, and not at n == 0.
bool l1_aliased(const SepCall<double>& c, double lambda, double sigma) { return c.y == c.q && lambda * sigma >= 0.0; }
bool l1_aliased(const SepCall<float>& c, float, float) { return c.y == c.q && c.n > 0; }
struct RowL0 {
  using Op = OpL0; using F32 = F32L0; using Term = HTermL0;
  template <class O, class T> static O make(T lambda, T sigma) { return O{std::sqrt(2 * lambda * sigma)}; }
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
  template <class O, class T> static O make(T lambda, T sigma) { return O{sigma * lambda}; }
};
struct RowL0Box {
  using Op = OpL0Box; using F32 = F32L0Box; using Term = HTermL0;
  template <class O, class T> static O make(T lambda, T sigma) { return O{2 * lambda * sigma}; }
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

template <class Row>
static int run_prox(const SepCall<double>& c, double lambda, double sigma) {
  const int rc = spx_check_common(c);
  if (rc) return rc;
  return run_separable(c, Row::template make<typename Row::Op>(lambda, sigma));
}

// ---------------------------------------------------------------------------------------------
// prox! + value of h at the result, in one pass (synchronous: *value is written on the host)
// ---------------------------------------------------------------------------------------------
template <class Row>
static int run_proxval(const SepCall<double>& c, double lambda, double sigma, double q_scale, double* value) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  SPX_REQUIRE(value != nullptr, "value is NULL");
  WithValue<typename Row::Op, typename Row::Term> op{Row::template make<typename Row::Op>(lambda, sigma), nullptr, q_scale};
  *value = lambda * 0.0;  // (n == 0, or an error: -0.0 for a negative lambda, NaN for a non-finite one)
  const SpxDest dest = spx_value_dest(c.ctx, value);
  if (c.n == 0) return spx_dest_empty(c.ctx, {nullptr, dest.dev, 1});  // (the device side only: the host keeps lambda * 0)
  rc = run_separable(c, op, dest, lambda);
  spx_value_nan_on_device(rc, dest, false, value);
  return rc;
}

// ---------------------------------------------------------------------------------------------
// prox! + step statistics in one pass (spx_proxstep_*): y, xkn = (xk + sj) + y, and {h, <q, y>, <y, y>} to a host double[3]
// (synchronous) and / or a device double[3] (enqueue only).  Float64, device pointers, the six separable operators.
// ---------------------------------------------------------------------------------------------
template <class Row>
static int run_proxstep(const SepCall<double>& c, double lambda, double sigma, double q_scale, const SpxDest& dest) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  rc = spx_step_begin(c.ctx, dest, false, c.y, {c.q}, kSpxYAliasesQ, c.xkn, c.others());
  if (rc) return rc;
  if (c.n == 0) return spx_dest_empty(c.ctx, dest);
  WithStep<typename Row::Op, typename Row::Term> op{};
  static_cast<typename Row::Op&>(op) = Row::template make<typename Row::Op>(lambda, sigma);
  op.qscale = q_scale;
  return run_separable(c, op, dest, lambda);
}

// ---------------------------------------------------------------------------------------------
// C entry points (Float64 prox!): each builds the call {ctx, y, q, d, xk, sj, n, box, xkn} from its arguments
// ---------------------------------------------------------------------------------------------
#define SPX_BOX_OF(T) SpxBox<T>{l_vec, u_vec, l_scalar, u_scalar, sel_mask}
SPX_EXPORT int spx_prox_l1(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                           double lambda, double sigma) {
  const SepCall<double> c{ctx, y, q, nullptr, xk, sj, n, {}, nullptr};
  return l1_aliased(c, lambda, sigma) ? run_prox<RowL1Aliased>(c, lambda, sigma) : run_prox<RowL1>(c, lambda, sigma);
}
SPX_EXPORT int spx_proxval_l1(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                              double lambda, double sigma, double q_scale, double* value) {
  const SepCall<double> c{ctx, y, q, nullptr, xk, sj, n, {}, nullptr};
  if (!l1_aliased(c, lambda, sigma)) return run_proxval<RowL1>(c, lambda, sigma, q_scale, value);
  SPX_REQUIRE(q_scale == 1.0, "q_scale != 1 with y aliasing q");  // (ahead of every other check)
  return run_proxval<RowL1Aliased>(c, lambda, sigma, 1.0, value);
}
SPX_EXPORT int spx_proxstep_l1(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                               double lambda, double sigma, double q_scale, double* xkn, double* stats, double* stats_dev) {
  return run_proxstep<RowL1>({ctx, y, q, nullptr, xk, sj, n, {}, xkn}, lambda, sigma, q_scale, {stats, stats_dev, 3});
}
#define SPX_PROX3(PROX, PROXVAL, PROXSTEP, ROW)                                                                                \
  SPX_EXPORT int PROX(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, double lambda, \
                      double sigma) {                                                                                         \
    return run_prox<ROW>({ctx, y, q, nullptr, xk, sj, n, {}, nullptr}, lambda, sigma);                                         \
  }                                                                                                                            \
  SPX_EXPORT int PROXVAL(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,             \
                         double lambda, double sigma, double q_scale, double* value) {                                        \
    return run_proxval<ROW>({ctx, y, q, nullptr, xk, sj, n, {}, nullptr}, lambda, sigma, q_scale, value);                      \
  }                                                                                                                            \
  SPX_EXPORT int PROXSTEP(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,            \
                          double lambda, double sigma, double q_scale, double* xkn, double* stats, double* stats_dev) {       \
    return run_proxstep<ROW>({ctx, y, q, nullptr, xk, sj, n, {}, xkn}, lambda, sigma, q_scale, {stats, stats_dev, 3});         \
  }
SPX_PROX3(spx_prox_l0, spx_proxval_l0, spx_proxstep_l0, RowL0)
SPX_PROX3(spx_prox_lhalf, spx_proxval_lhalf, spx_proxstep_lhalf, RowLhalf)
#define SPX_PROX3_BOX(PROX, PROXVAL, PROXSTEP, ROW)                                                                            \
  SPX_EXPORT int PROX(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, double lambda, \
                      double sigma, const double* l_vec, const double* u_vec, double l_scalar, double u_scalar,              \
                      const uint8_t* sel_mask) {                                                                              \
    return run_prox<ROW>({ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(double), nullptr}, lambda, sigma);                         \
  }                                                                                                                            \
  SPX_EXPORT int PROXVAL(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,             \
                         double lambda, double sigma, const double* l_vec, const double* u_vec, double l_scalar,             \
                         double u_scalar, const uint8_t* sel_mask, double q_scale, double* value) {                           \
    return run_proxval<ROW>({ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(double), nullptr}, lambda, sigma, q_scale, value);      \
  }                                                                                                                            \
  SPX_EXPORT int PROXSTEP(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,            \
                          double lambda, double sigma, const double* l_vec, const double* u_vec, double l_scalar,            \
                          double u_scalar, const uint8_t* sel_mask, double q_scale, double* xkn, double* stats,               \
                          double* stats_dev) {                                                                                \
    return run_proxstep<ROW>({ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(double), xkn}, lambda, sigma, q_scale,                 \
                             {stats, stats_dev, 3});                                                                          \
  }
SPX_PROX3_BOX(spx_prox_l1_box, spx_proxval_l1_box, spx_proxstep_l1_box, RowL1Box)
SPX_PROX3_BOX(spx_prox_l0_box, spx_proxval_l0_box, spx_proxstep_l0_box, RowL0Box)
SPX_PROX3_BOX(spx_prox_lhalf_box, spx_proxval_lhalf_box, spx_proxstep_lhalf_box, RowLhalfBox)

// ---------------------------------------------------------------------------------------------
// Float32 vectors.  The reference's structs and prox! / iprox! methods are generic in R <: Real (src/shiftedNormL1Box.jl:89-94:
// `y::AbstractVector{R}, psi::ShiftedNormL1Box{R, ...}, q::AbstractVector{R}, sigma::R`) and its tests build Float32
// operators on views (test/runtests.jl:196-209): the L1 / L0 bodies above with T = float.  (RootNormLhalf is NOT here: its
// body mixes Float64 literals -- `^(-3 / 2)`, `54^(1 / 3)` -- into the Float32 data, i.e. the reference itself computes it in
// Float64 and rounds; the fp64 entry points cover that after a conversion by the caller.)
//
// HBM: 16 B/element (read q, xk, sj, write y; +8 with vector bounds, +1 with a mask) -- half the bytes of the fp64 path.
// Skeleton: one tile of 256 lanes x 4 x (4 floats = 16 bytes) per workgroup, all 12 non-temporal 16-byte loads of a lane
// issued before first use, 16-byte non-temporal stores.  Views that start at any element (4-byte granularity) are
// peeled to a 16-byte boundary when all vectors share the misalignment; mixed alignments take 4-byte accesses.
// y === q is safe (a lane reads q[i] before it writes y[i]; lanes own disjoint indices).
// ---------------------------------------------------------------------------------------------
namespace {  // (the Float32 functors F32*: next to the operator table above)

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kF32U = 4;                       // 16-byte groups per lane and vector
constexpr int kF32Tile = 256 * kF32U;          // 16-byte groups per workgroup

// body: `n4` groups of 4 floats starting at the (16-byte aligned) pointers; head: `head` (< 4) elements in front of them
// (at [-head .. -1]) and tail: `tail` (< 4) elements behind them, taken by single lanes of workgroup 0.
template <class Op, bool VECB, bool MASK>
__global__ __launch_bounds__(256) void k_sep_f32(float* y_, const float* q_, const float* d_, const float* xk_, const float* sj_,
                                                  const float* l_, const float* u_, const uint8_t* mask, float ls,
                                                  float us, int64_t n4, int head, int tail, Op op) {
  f32x4* y = reinterpret_cast<f32x4*>(y_);
  const f32x4* q = reinterpret_cast<const f32x4*>(q_);
  const f32x4* xk = reinterpret_cast<const f32x4*>(xk_);
  const f32x4* sj = reinterpret_cast<const f32x4*>(sj_);
  const f32x4* lv = reinterpret_cast<const f32x4*>(l_);
  const f32x4* uv = reinterpret_cast<const f32x4*>(u_);
  const f32x4* dv = reinterpret_cast<const f32x4*>(d_);
  const int64_t base = (int64_t)blockIdx.x * kF32Tile + threadIdx.x;
  f32x4 a[kF32U], b[kF32U], c[kF32U], lo[kF32U], up[kF32U], dd[kF32U];
#pragma unroll
  for (int k = 0; k < kF32U; ++k) {
    int64_t i = base + k * 256;
    if (i >= n4) i = n4 > 0 ? n4 - 1 : 0;
    if (n4 > 0) {
      a[k] = __builtin_nontemporal_load(q + i);
      b[k] = __builtin_nontemporal_load(xk + i);
      c[k] = __builtin_nontemporal_load(sj + i);
      if constexpr (Op::kNIn == 4) dd[k] = __builtin_nontemporal_load(dv + i);
      if constexpr (VECB && Op::kBox) {
        lo[k] = l_ ? __builtin_nontemporal_load(lv + i) : f32x4{ls, ls, ls, ls};
        up[k] = u_ ? __builtin_nontemporal_load(uv + i) : f32x4{us, us, us, us};
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kF32U; ++k) {
    const int64_t i = base + k * 256;
    if (i < n4) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float l1 = ls, u1 = us;
        if constexpr (VECB && Op::kBox) { l1 = lo[k][e]; u1 = up[k][e]; }
        bool sel = true;
        if constexpr (MASK && Op::kBox) sel = mask[4 * i + e] != 0;
        float d1 = 0.0f;
        if constexpr (Op::kNIn == 4) d1 = dd[k][e];
        o[e] = apply_op(op, a[k][e], d1, b[k][e], c[k][e], l1, u1, sel);
      }
      __builtin_nontemporal_store(o, y + i);
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {  // the few elements outside the aligned body
    const int64_t i = ((int)threadIdx.x < head) ? (int64_t)threadIdx.x - head : 4 * n4 + ((int)threadIdx.x - head);
    float l1 = ls, u1 = us;
    if constexpr (Op::kBox) {
      if (l_) l1 = l_[i];
      if (u_) u1 = u_[i];
    }
    bool sel = true;
    if constexpr (MASK && Op::kBox) sel = mask[i] != 0;
    float d1 = 0.0f;
    if constexpr (Op::kNIn == 4) d1 = d_[i];
    y_[i] = apply_op(op, q_[i], d1, xk_[i], sj_[i], l1, u1, sel);
  }
}

// mixed alignments: 4-byte accesses
template <class Op>
__global__ __launch_bounds__(256) void k_sep_f32_scalar(float* y, const float* q, const float* d, const float* xk, const float* sj,
                                                         const float* l, const float* u, const uint8_t* mask, float ls,
                                                         float us, int64_t n, Op op) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float l1 = ls, u1 = us;
    bool sel = true;
    if constexpr (Op::kBox) {
      if (l) l1 = l[i];
      if (u) u1 = u[i];
      if (mask) sel = mask[i] != 0;
    }
    float d1 = 0.0f;
    if constexpr (Op::kNIn == 4) d1 = d[i];
    y[i] = apply_op(op, q[i], d1, xk[i], sj[i], l1, u1, sel);
  }
}

// v: the call at its aligned body
template <class Op, bool VECB, bool MK>
void launch_f32(const SepCall<float>& v, dim3 grid, int64_t n4, int head, int tail, Op op) {
  hipLaunchKernelGGL((k_sep_f32<Op, VECB, MK>), grid, dim3(256), 0, v.ctx->stream, v.y, v.q, v.d, v.xk, v.sj, v.box.l, v.box.u,
                     v.box.mask, v.box.ls, v.box.us, n4, head, tail, op);
}
template <class Op>
int run_f32(const SepCall<float>& c, Op op) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  spx_ctx* const ctx = c.ctx;
  const int64_t n = c.n;
  if (n == 0) return SPX_OK;
  SPX_ON_DEVICE(ctx);
  if (!c.same_misalignment(Op::kBox)) {
    int64_t blocks = (n + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((k_sep_f32_scalar<Op>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.d, c.xk, c.sj,
                       c.box.l, c.box.u, c.box.mask, c.box.ls, c.box.us, n, op);
    SPX_LAUNCH_CHECK();
    return SPX_OK;
  }
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(c.y) & 15u);
  int head = (int)(((16u - m) / 4u) & 3u);
  if (head > n) head = (int)n;
  const int64_t n4 = (n - head) / 4;
  const int tail = (int)(n - head - 4 * n4);
  int64_t blocks = (n4 + kF32Tile - 1) / kF32Tile;
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks);
  const bool vecb = Op::kBox && (c.box.l || c.box.u);
  const bool msk = Op::kBox && c.box.mask != nullptr;
  const SepCall<float> v = c.shifted(head);
  if (vecb && msk) launch_f32<Op, true, true>(v, grid, n4, head, tail, op);
  else if (vecb) launch_f32<Op, true, false>(v, grid, n4, head, tail, op);
  else if (msk) launch_f32<Op, false, true>(v, grid, n4, head, tail, op);
  else launch_f32<Op, false, false>(v, grid, n4, head, tail, op);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}
template <class Row>
int run_prox(const SepCall<float>& c, float lambda, float sigma) {
  return run_f32(c, Row::template make<typename Row::F32>(lambda, sigma));
}

}  // namespace

SPX_EXPORT int spx_prox_l1_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                               float lambda, float sigma) {
  const SepCall<float> c{ctx, y, q, nullptr, xk, sj, n, {}, nullptr};
  return l1_aliased(c, lambda, sigma) ? run_prox<RowL1Aliased>(c, lambda, sigma) : run_prox<RowL1>(c, lambda, sigma);
}
SPX_EXPORT int spx_prox_l0_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                               float lambda, float sigma) {
  return run_prox<RowL0>(SepCall<float>{ctx, y, q, nullptr, xk, sj, n, {}, nullptr}, lambda, sigma);
}
SPX_EXPORT int spx_prox_l1_box_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                                   float lambda, float sigma, const float* l_vec, const float* u_vec, float l_scalar,
                                   float u_scalar, const uint8_t* sel_mask) {
  return run_prox<RowL1Box>(SepCall<float>{ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(float), nullptr}, lambda, sigma);
}
SPX_EXPORT int spx_prox_l0_box_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                                   float lambda, float sigma, const float* l_vec, const float* u_vec, float l_scalar,
                                   float u_scalar, const uint8_t* sel_mask) {
  return run_prox<RowL0Box>(SepCall<float>{ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(float), nullptr}, lambda, sigma);
}


// ---------------------------------------------------------------------------------------------
// iprox! entry points
// ---------------------------------------------------------------------------------------------
// the skeleton of each precision
template <class Op>
static int run_skeleton(const SepCall<double>& c, Op op) { return run_separable(c, op); }
template <class Op>
static int run_skeleton(const SepCall<float>& c, Op op) { return run_f32(c, op); }
// The d > 0 flag word of the unboxed forms, read back (the stream is synchronised): the reference's assertion.
static int iprox_check_flag(spx_ctx* ctx, const int* flag) {
  int bad = 0;
  SPX_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SPX_HIP(hipStreamSynchronize(ctx->stream));
  if (bad) {
    spx_set_error("AssertionError: d[i] > 0");
    return SPX_ERR_ASSERT;
  }
  return SPX_OK;
}
// check_d (the flagged rows): the d > 0 flag is read back, which synchronises the stream -- refused under a capture before
// anything is enqueued
template <class Row, class T>
static int run_iprox(const SepCall<T>& c, T lambda, int check_d) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  SPX_REQUIRE(c.n == 0 || c.d != nullptr, "d is NULL");
  if constexpr (!Row::kFlagged) {
    return run_skeleton(c, RowOp<Row, T>{lambda});
  } else {
    spx_ctx* const ctx = c.ctx;
    if (c.n == 0) return SPX_OK;
    if (check_d) { rc = spx_require_not_capturing(ctx, "the d > 0 check of iprox! (pass check = 0)"); if (rc) return rc; }
    rc = spx_ws_reserve(ctx, 256);
    if (rc) return rc;
    SPX_ON_DEVICE(ctx);
    int* flag = reinterpret_cast<int*>(ctx->ws);
    { const int rz = spx_zero_async(ctx, flag, sizeof(int)); if (rz) return rz; }
    rc = run_skeleton(c, RowOp<Row, T>{lambda, flag});
    if (rc || !check_d) return rc;
    return iprox_check_flag(ctx, flag);
  }
}

// ---------------------------------------------------------------------------------------------
// iprox! + step statistics in one pass (spx_iproxstep_*): y, xkn = (xk + sj) + y and {h, <g, y>, <d .* y, y>, <y, y>} to a host
// double[4] (synchronous) and / or a device double[4] (enqueue only).  Float64, device pointers.  All four operators take the
// fused route, each on the skeleton of its plain iprox! (profiles/iproxstep_kres.txt).
// ---------------------------------------------------------------------------------------------
template <class Row>
static int run_iproxstep(const SepCall<double>& c, double lambda, int check_d, const SpxDest& dest) {
  spx_ctx* const ctx = c.ctx;
  int rc = spx_check_common(c);
  if (rc) return rc;
  SPX_REQUIRE(c.n == 0 || c.d != nullptr, "d is NULL");
  rc = spx_step_begin(ctx, dest, check_d != 0, c.y, {c.q, c.d}, "y aliases g or d (the sums would read an overwritten input)", c.xkn,
                      c.others());
  if (rc) return rc;
  if (c.n == 0) return spx_dest_empty(ctx, dest);
  WithIstep<typename Row::Op, typename Row::Term> op{};
  op.lambda = lambda;
  int* flag = nullptr;
  if constexpr (Row::kFlagged) {
    // the whole workspace of the call is reserved here, so that the flag word keeps its address through run_separable
    rc = spx_ws_reserve(ctx, sep_ws_bytes(ctx, c.n, 4));
    if (rc) return rc;
    SPX_ON_DEVICE(ctx);
    flag = reinterpret_cast<int*>(static_cast<char*>(ctx->ws) + kSepFlagOffset);  // (clear of the four result doubles)
    { const int rz = spx_zero_async(ctx, flag, sizeof(int)); if (rz) return rz; }
    op.flag = flag;
  }
  rc = run_separable(c, op, dest, lambda);
  if (rc || !check_d) return rc;
  if constexpr (Row::kFlagged) return iprox_check_flag(ctx, flag);  // (the stream has been synchronised by the copy of the statistics)
  return SPX_OK;
}

// the entry points: q of the call holds g; the Box forms have no check_d
#define SPX_IPROX3(IPROX, IPROXSTEP, IPROX_F32, ROW)                                                                           \
  SPX_EXPORT int IPROX(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,         \
                       int64_t n, double lambda, int check_d) {                                                               \
    return run_iprox<ROW>(SepCall<double>{ctx, y, g, d, xk, sj, n, {}, nullptr}, lambda, check_d);                             \
  }                                                                                                                            \
  SPX_EXPORT int IPROXSTEP(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,     \
                           int64_t n, double lambda, int check_d, double* xkn, double* stats, double* stats_dev) {            \
    return run_iproxstep<ROW>({ctx, y, g, d, xk, sj, n, {}, xkn}, lambda, check_d, {stats, stats_dev, 4});                     \
  }                                                                                                                            \
  SPX_EXPORT int IPROX_F32(spx_ctx* ctx, float* y, const float* g, const float* d, const float* xk, const float* sj,          \
                           int64_t n, float lambda, int check_d) {                                                            \
    return run_iprox<ROW>(SepCall<float>{ctx, y, g, d, xk, sj, n, {}, nullptr}, lambda, check_d);                              \
  }
SPX_IPROX3(spx_iprox_l1, spx_iproxstep_l1, spx_iprox_l1_f32, RowIproxL1)
SPX_IPROX3(spx_iprox_l0, spx_iproxstep_l0, spx_iprox_l0_f32, RowIproxL0)
#define SPX_IPROX3_BOX(IPROX, IPROXSTEP, IPROX_F32, ROW)                                                                       \
  SPX_EXPORT int IPROX(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,         \
                       int64_t n, double lambda, const double* l_vec, const double* u_vec, double l_scalar,                   \
                       double u_scalar, const uint8_t* sel_mask) {                                                            \
    return run_iprox<ROW>(SepCall<double>{ctx, y, g, d, xk, sj, n, SPX_BOX_OF(double), nullptr}, lambda, 0);                   \
  }                                                                                                                            \
  SPX_EXPORT int IPROXSTEP(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,     \
                           int64_t n, double lambda, const double* l_vec, const double* u_vec, double l_scalar,               \
                           double u_scalar, const uint8_t* sel_mask, double* xkn, double* stats, double* stats_dev) {         \
    return run_iproxstep<ROW>({ctx, y, g, d, xk, sj, n, SPX_BOX_OF(double), xkn}, lambda, 0, {stats, stats_dev, 4});           \
  }                                                                                                                            \
  SPX_EXPORT int IPROX_F32(spx_ctx* ctx, float* y, const float* g, const float* d, const float* xk, const float* sj,          \
                           int64_t n, float lambda, const float* l_vec, const float* u_vec, float l_scalar, float u_scalar,   \
                           const uint8_t* sel_mask) {                                                                         \
    return run_iprox<ROW>(SepCall<float>{ctx, y, g, d, xk, sj, n, SPX_BOX_OF(float), nullptr}, lambda, 0);                     \
  }
SPX_IPROX3_BOX(spx_iprox_l1_box, spx_iproxstep_l1_box, spx_iprox_l1_box_f32, RowIproxL1Box)
SPX_IPROX3_BOX(spx_iprox_l0_box, spx_iproxstep_l0_box, spx_iprox_l0_box_f32, RowIproxL0Box)
