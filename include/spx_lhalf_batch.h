/* spx_lhalf_batch.h -- C ABI of libspx_lhalf_batch.so: the batched RootNormLhalf / RootNormLhalfBox prox! + step statistics
 * (MI355X / gfx950 only).  A library of its own next to libspx.so, against which it links: contexts, streams, status codes and
 * spx_last_error are those of spx.h; a context created by spx_ctx_create[_on_stream] serves every library.  Additive:
 * spx_abi_version() stays 1. */
#ifndef SPX_LHALF_BATCH_H
#define SPX_LHALF_BATCH_H

#include "spx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched prox! + step statistics, parameters on the device ------------------------------- */
/* `batch` problems of n elements in ONE call, each with its own lambda, sigma, q_scale (and box): what spx_batch.h has for
 * NormL1 / NormL0, for ShiftedRootNormLhalf (spx_proxstep_lhalf_batch) and ShiftedRootNormLhalfBox
 * (spx_proxstep_lhalf_box_batch).  Float64, device pointers only.
 *   layout   : problem b occupies elements [b * ld, b * ld + n) of y, q, xk, sj and xkn, ld >= n.  The elements
 *              [b * ld + n, (b + 1) * ld) are never read or written.  Any 8-byte alignment of the bases; when the bases do not
 *              all share their alignment modulo 16 the call takes an element-wise kernel (same results).
 *   lambda, sigma, q_scale, l, u : DEVICE arrays of `batch` doubles, one scalar per problem (a trust region of radius
 *              Delta_b: l[b] = -Delta_b, u[b] = Delta_b; there are no vector bounds in this form).  The kernel that stores y
 *              reads them: nothing is read back, nothing synchronises, and a captured call follows the values that are in
 *              those arrays when the graph is replayed.  They are not checked on the device.
 *   sel_mask : ONE byte mask of length n shared by all problems (indexed by the element index within the row), or NULL.
 *   y, xkn   : BOX FORM: row b has the bits of spx_proxstep_lhalf_box on that row with host copies of lambda[b], sigma[b],
 *              q_scale[b], with l[b], u[b] as l_scalar, u_scalar and with the shared mask.  The functor's constants
 *              (sigma lambda / 4, lambda, 0.5 / sigma) are products and one IEEE division, which the device rounds as the host.
 *              UNBOXED FORM: the single call compares a = |q_scale * q + (xk + sj)| (each operation rounded once, in this
 *              order) with the threshold p_host = fl(fl(C * pow(2 sigma lambda, e)) / 4), C = pow(54.0, 1.0 / 3.0),
 *              e = the double nearest 2/3, formed by the HOST's libm.  The batched kernel forms p_dev on the device from the
 *              same expression without a libm pow; |p_dev - p_host| <= 4 ulp(p_host) (each side's pow within 1 ulp of the exact
 *              value: 2 ulps; the product with C adds one rounding on each side; the division by 4 is exact), and
 *              spx_lhalf_threshold_batch stores p_dev itself.  Every element for which (a <= p_host) == (a <= p_dev) has the
 *              bits of spx_proxstep_lhalf on that row.  An element whose a lies strictly between the two thresholds, or equals
 *              the larger one, has the OTHER branch's result: exactly 0.0 - (xk + sj) where a <= p_dev, otherwise the stationary
 *              point minus (xk + sj), within 1e-12 * max(|y|, |xk + sj|, |q|) of the reference formula.  (The prox of the
 *              root-norm jumps at p: both values are minimisers to within the rounding of p.)
 *              xkn, when not NULL, is always bit for bit (xk + sj) + y of the stored y.
 *   stats_dev: DEVICE double[3 * batch], not NULL.  stats_dev[3 b + {0, 1, 2}] = {lambda[b] * sum over the SELECTED indices of
 *              sqrt|(xk + sj) + y|, sum over ALL i of q[i] * y[i] with q AS PASSED, sum over ALL i of y[i]^2} of row b, always
 *              of the stored y.  The sums are added in a fixed order that depends on n, on the parity of b * ld and on the
 *              alignment of the bases, not on batch and not on the other rows: reproducible, and the same bits wherever the
 *              problem is placed among rows of the same parity.
 *   There is no host destination: the call always only enqueues.  Capturable under the rules stated in spx.h (the same call made
 *   once before on the context; only n > 12288 needs workspace).
 *   Refused with SPX_ERR_INVALID_ARG, nothing launched: y == q; xkn equal to y, q, xk, sj or sel_mask; ld < n; batch < 0 or
 *   n < 0; a NULL parameter array (with batch > 0); stats_dev == NULL (with batch > 0); a call that needs more than 2^31 - 1
 *   workgroups (batch, or batch * ceil(n / 3072) for n > 12288).
 *   batch == 0: SPX_OK, nothing done.  n == 0: 3 * batch zeros stored to stats_dev by a kernel (no memset node).
 *   Non-finite data: the contract stated in spx.h for spx_proxstep_*, per problem -- a NaN in one row (or in its lambda[b])
 *   touches that row's y and sums only.  sigma lambda == 0, negative or NaN gives the threshold pow gives: 0, NaN, NaN. */
int spx_proxstep_lhalf_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                             int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* q_scale,
                             double* xkn, double* stats_dev);
int spx_proxstep_lhalf_box_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                 int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* l,
                                 const double* u, const uint8_t* sel_mask, const double* q_scale, double* xkn,
                                 double* stats_dev);

/* p_dev[b] = the threshold spx_proxstep_lhalf_batch compares |q_scale * q + (xk + sj)| with for (lambda[b], sigma[b]): the same
 * device function, so the value is the kernel's own (elements with a <= p_dev[b] give y = 0.0 - (xk + sj)).  lambda, sigma,
 * p_dev: DEVICE double[batch].  One small kernel, no workspace, only enqueues; capturable.  batch == 0: SPX_OK, nothing done.
 * Refused with SPX_ERR_INVALID_ARG: batch < 0; a NULL lambda, sigma or p_dev (with batch > 0). */
int spx_lhalf_threshold_batch(spx_ctx* ctx, const double* lambda, const double* sigma, int64_t batch, double* p_dev);

#ifdef __cplusplus
}
#endif

#endif /* SPX_LHALF_BATCH_H */
