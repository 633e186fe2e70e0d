// spx_lhalf_threshold.hpp -- the threshold of the RootNormLhalf closed form, p = 54^(1/3) (2 sigma lambda)^(2/3) / 4
// (src/shiftedRootNormLhalf.jl:49), formed on the device for the batched call (spx_lhalf_batch.hip).  The host forms it as
//   fl(fl(C * pow(2 nl, e)) / 4),   C = the double glibc's pow(54.0, 1.0 / 3.0) yields,   e = fl(2/3) = 2/3 - 3.70e-17
// (RowLhalf::make, spx_sep_device.hpp), and this function reproduces THAT expression: the mathematical (2 nl)^(2/3) is
// |e - 2/3| ln(2 nl) ~ 1.3e-14 (a hundred ulps) away from pow(2 nl, e) at 2 nl = 2^+-500.
// pow(x, e) without a libm pow:  x = m 8^j, m in [1, 8);  c = m^(1/3) as a double-double (a float seed, two Newton steps in
// double, one correction whose residual m - c^3 is formed exactly by fma);  x^e = c^2 (1 + (e - 2/3) ln x) 4^j up to the
// second-order term ((e - 2/3) ln x)^2 / 2 <= 3.5e-28.  Error analysis: the sum that is rounded to the
// result is within 4e-28 of x^e relatively, so the result is within 0.5 ulp + 4e-12 ulp of it -- inside the 1 ulp the contract
// of include/spx_lhalf_batch.h assumes of both sides.  The float cbrt and log only have to be right to 1e-4 and 0.03.
// __host__ __device__: tests/c/lhalf_threshold_driver.cpp runs the same statements on the host against glibc's pow.
#pragma once
#include <cmath>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

// pow(x, fl(2/3)) for x > 0 finite; pow's own answers at 0, below 0, Inf and NaN
__host__ __device__ inline double lhalf_pow_two_thirds(double x) {
  if (x == 0.0) return 0.0;
  if (!(x > 0.0)) return x - x + NAN;  // negative or NaN (an exponent that is no integer)
  if (x > 1.7976931348623157e308) return x;
  int k;
  const double f = frexp(x, &k);            // x = f 2^k, f in [1/2, 1)
  const int j = (k - 1 >= 0) ? (k - 1) / 3 : -((3 - k) / 3);  // floor((k - 1) / 3)
  const double m = ldexp(f, k - 3 * j);     // in [1, 8): exact
  double c = (double)cbrtf((float)m);
  c -= (c * c * c - m) / (3.0 * (c * c));
  c -= (c * c * c - m) / (3.0 * (c * c));
  // the correction: m - c^3 with c^2 = p + pe and c p = q + qe exactly
  const double p = c * c, pe = fma(c, c, -p);
  const double q = c * p, qe = fma(c, p, -q);
  const double cl = (((m - q) - qe) - c * pe) / (3.0 * p);
  // (c + cl)^2 = sh + sl
  const double sh = p, sl = pe + 2.0 * c * cl;
  // ln x to 0.03 is enough: it enters times e - 2/3
  const double lnx = (double)logf((float)m) + (double)(3 * j) * 0.6931471805599453;
  const double t = -3.700743415417188e-17 * lnx;  // (fl(2/3) - 2/3) ln x
  return ldexp(sh + (sl + sh * t), 2 * j);
}
// p for nl = sigma * lambda, as the host rounds it
__host__ __device__ inline double lhalf_threshold(double nl) {
  return 3.7797631496846193 /* pow(54.0, 1.0 / 3.0) */ * lhalf_pow_two_thirds(2 * nl) / 4;
}
