/* spx_gbinf_batch.h -- C ABI of libspx_gbinf_batch.so: the batched ShiftedGroupNormL2Binf prox! + step statistics (MI355X /
 * gfx950 only).  A library of its own next to libspx.so, against which it links: contexts, streams, status codes and
 * spx_last_error are those of spx.h; a context created by spx_ctx_create[_on_stream] serves all the libraries.  Additive:
 * spx_abi_version() stays 1. */
#ifndef SPX_GBINF_BATCH_H
#define SPX_GBINF_BATCH_H

#include "spx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched trust-region group prox! + step statistics, parameters on the device ------------- */
/* `batch` group-lasso problems inside a box trust region in ONE call, each with its own sigma, radius delta, q_scale and group
 * weights: the step of a TR solver on a regularisation path, cross-validation folds, multi-start.  ShiftedGroupNormL2Binf (what
 * spx_proxstep_group_l2_binf computes), Float64, device pointers only, uniform contiguous groups of 1 .. 512 elements (larger
 * groups, CSR and gather layouts: spx_proxstep_group_l2_binf, one problem per call).  The contract is that of
 * spx_proxstep_group_l2_batch (spx_gbatch.h), restated:
 *   layout   : problem b occupies elements [b * ld, b * ld + n) of y, q, xk, sj and xkn, n = ngroups * group_size, ld >= n;
 *              group g of problem b is the group_size elements from b * ld + g * group_size on.  The elements
 *              [b * ld + n, (b + 1) * ld) are never read or written.
 *   lambda_vec, ldl, lambda_scale : the weight of group g of problem b is lambda_vec[b * ldl + g]; ldl == 0: ONE weight vector
 *              shared by all problems, otherwise ldl >= ngroups.  lambda_scale: a DEVICE double[batch] or NULL; when given the
 *              weight is lambda_scale[b] * lambda_vec[...], ONE rounded multiply -- the bits of passing the products to the
 *              single call.
 *   sigma, delta, q_scale : DEVICE double[batch], read by the workgroups of problem b; not checked on the device.  Nothing is
 *              read back, nothing synchronises, and a captured call follows the values that are in the arrays when the graph is
 *              replayed -- a solver that shrinks or grows each problem's radius on the device needs no host round trip.
 *   y, xkn   : row b has the bits of spx_proxstep_group_l2_binf on that row's data with host copies of sigma[b], delta[b],
 *              q_scale[b] and the row's weights, under the context's tuning key 9 (0 or 1) as that call honours it, ON VECTORS
 *              OF THE LAUNCH'S ALIGNMENT CLASS: the launch takes the 16-byte pairs form when group_size is even, ld is even and
 *              y, q, xk, sj and xkn (when given) are all 16-byte aligned; otherwise the element-wise form for EVERY row, whose
 *              bits are those the single call gives when one of its vectors sits 8 bytes off a 16-byte boundary (or group_size
 *              is odd).  A group the single call hands to its second (literal) launch is evaluated here on that launch's
 *              register tile, by the same workgroup in a second phase.  xkn = (xk + sj) + y; it may be NULL.
 *   stats_dev: DEVICE double[3 * batch], not NULL.  For row b: [3 b] = sum over the groups of lambda_{b,g} * sqrt(sum over the
 *              group of v_i^2) with v = (xk + sj) + y of the STORED y; [3 b + 1] = sum of q[i] * y[i] with q AS PASSED;
 *              [3 b + 2] = sum of y[i]^2.  The sums are added in a fixed order that depends on group_size, ngroups, the
 *              alignment class and the row's own data (which of its groups take the literal evaluation) only -- not on batch,
 *              on b, on the other rows or on timing: a repeat gives the same bits, and so does the problem moved to another
 *              row of a call of the same shape.
 *   There is no host destination: the call always only enqueues.  Capturable after one identical warm call (only
 *   n > 12288 needs workspace).
 *   Refused with SPX_ERR_INVALID_ARG, nothing launched: group_size < 1 or > 512 (spx_proxstep_group_l2_binf serves larger
 *   groups); ngroups < 0 or batch < 0; ngroups * group_size overflows; ld < n; ldl != 0 and ldl < ngroups; y == q; xkn equal to
 *   y, q, xk or sj; a NULL lambda_vec, sigma, delta, q_scale or stats_dev (with batch > 0 and n > 0); a call that needs more
 *   than 2^31 - 1 workgroups.
 *   batch == 0: SPX_OK, nothing done.  n == 0: 3 * batch zeros stored to stats_dev by a kernel (no memset node).
 *   Non-finite data: the contract stated in spx.h for spx_proxstep_group_l2_binf, per problem -- a group that holds a NaN takes
 *   the literal evaluation and is NaN throughout; a NaN in one row touches that row's y and sums only. */
int spx_proxstep_group_l2_binf_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                     int64_t group_size, int64_t ngroups, int64_t batch, int64_t ld,
                                     const double* lambda_vec, int64_t ldl, const double* lambda_scale,
                                     const double* sigma, const double* delta, const double* q_scale,
                                     double* xkn, double* stats_dev);

#ifdef __cplusplus
}
#endif

#endif /* SPX_GBINF_BATCH_H */
