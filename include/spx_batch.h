/* spx_batch.h -- C ABI of libspx_batch.so: the batched separable prox! + step statistics (MI355X / gfx950 only).
 * A library of its own next to libspx.so, against which it links: contexts, streams, status codes and spx_last_error are those
 * of spx.h; a context created by spx_ctx_create[_on_stream] serves both libraries.  Additive: spx_abi_version() stays 1. */
#ifndef SPX_BATCH_H
#define SPX_BATCH_H

#include "spx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched prox! + step statistics, parameters on the device ------------------------------- */
/* `batch` problems of n elements in ONE call, each with its own lambda, sigma, q_scale (and box): a regularisation path,
 * cross-validation folds, multi-start, one trust region per problem.  At solver sizes a call costs what its launch costs;
 * this call pays it once for all problems.  Float64, device pointers only; NormL1 / NormL0 and their Box forms.
 *   layout   : problem b occupies elements [b * ld, b * ld + n) of y, q, xk, sj and xkn, ld >= n.  The elements
 *              [b * ld + n, (b + 1) * ld) are never read or written.  Any 8-byte alignment of the bases; when the bases do not
 *              all share their alignment modulo 16 the call takes an element-wise kernel (same results).
 *   lambda, sigma, q_scale, l, u : DEVICE arrays of `batch` doubles, one scalar per problem (a trust region of radius
 *              Delta_b: l[b] = -Delta_b, u[b] = Delta_b; there are no vector bounds in this form).  The kernel that stores y
 *              reads them: nothing is read back, nothing synchronises, and a captured call follows the values that are in
 *              those arrays when the graph is replayed -- R2 can update nu on the device between replays.  They are not
 *              checked on the device: a problem gives what spx_proxstep_X gives with the same scalars.
 *   sel_mask : ONE byte mask of length n shared by all problems (indexed by the element index within the row), or NULL.
 *   y, xkn   : row b has exactly the contract of spx_proxstep_X on that row with lambda[b], sigma[b], q_scale[b] (l[b], u[b]
 *              as l_scalar, u_scalar): the same bits.  xkn may be NULL.
 *   stats_dev: DEVICE double[3 * batch], not NULL.  stats_dev[3 b + {0, 1, 2}] = {lambda[b] * sum over the SELECTED indices of
 *              Term((xk + sj) + y), sum over ALL i of q[i] * y[i] with q AS PASSED, sum over ALL i of y[i]^2} of row b.  The
 *              sums are added in a fixed order that depends on n, on the parity of b * ld and on the alignment of the bases,
 *              not on batch and not on the other rows: reproducible, and the same bits wherever the problem is placed among
 *              rows of the same parity.
 *   There is no host destination: the call always only enqueues.  Capturable under the rules stated in spx.h (the same call made
 *   once before on the context; only n > 12288 needs workspace).
 *   Refused with SPX_ERR_INVALID_ARG, nothing launched: y == q; xkn equal to y, q, xk, sj or sel_mask; ld < n; batch < 0 or
 *   n < 0; a NULL parameter array (with batch > 0); stats_dev == NULL (with batch > 0); a call that needs more than 2^31 - 1
 *   workgroups (batch, or batch * ceil(n / 3072) for n > 12288).
 *   batch == 0: SPX_OK, nothing done.  n == 0: 3 * batch zeros stored to stats_dev by a kernel (no memset node).
 *   Non-finite data: the contract stated in spx.h for spx_proxstep_*, per problem -- a NaN in one row touches that row's y and
 *   sums only. */
int spx_proxstep_l1_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                          int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* q_scale,
                          double* xkn, double* stats_dev);
int spx_proxstep_l0_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                          int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* q_scale,
                          double* xkn, double* stats_dev);
int spx_proxstep_l1_box_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                              int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* l,
                              const double* u, const uint8_t* sel_mask, const double* q_scale, double* xkn,
                              double* stats_dev);
int spx_proxstep_l0_box_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                              int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* l,
                              const double* u, const uint8_t* sel_mask, const double* q_scale, double* xkn,
                              double* stats_dev);

#ifdef __cplusplus
}
#endif

#endif /* SPX_BATCH_H */
