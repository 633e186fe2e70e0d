/* spx_ibatch.h -- C ABI of libspx_ibatch.so: the batched iprox! + step statistics (MI355X / gfx950 only).
 * A library of its own next to libspx.so, against which it links: contexts, streams, status codes and spx_last_error are those
 * of spx.h; a context created by spx_ctx_create[_on_stream] serves all the libraries.  Additive: spx_abi_version() stays 1. */
#ifndef SPX_IBATCH_H
#define SPX_IBATCH_H

#include "spx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched iprox! + step statistics, parameters on the device ------------------------------ */
/* `batch` problems of n elements in ONE call, the batched twins of spx_iproxstep_X: a path of diagonal quasi-Newton (R2DH)
 * problems, folds, a multi-start.  Float64, device pointers only; NormL1 / NormL0 and their Box forms.
 *   layout   : as in spx_batch.h -- problem b occupies elements [b * ld, b * ld + n) of y, g, d, xk, sj and xkn, ld >= n.  The
 *              elements [b * ld + n, (b + 1) * ld) are never read or written.  Any 8-byte alignment of the six bases; when the
 *              bases do not all share their alignment modulo 16 the call takes an element-wise kernel (same y and xkn bits).
 *   lambda, l, u : DEVICE arrays of `batch` doubles, one scalar per problem; there are no vector bounds in this form.  The
 *              kernel that stores y reads them: a captured call follows the values in those arrays when the graph is replayed.
 *   d_shift  : a DEVICE array of `batch` doubles, or NULL.  Given: the element site sees deff = d[i] + d_shift[b], ONE rounded
 *              add formed on the fly (never contracted), in place of d[i]: R2DH's D + sigma_b needs no pass of its own and
 *              follows the sigma_b a solver leaves on the device.  NULL: d enters as it is (no `+ 0.0`, which would turn a
 *              -0.0 into +0.0 and flip the sign of -g / d).
 *   sel_mask : ONE byte mask of length n shared by all problems (indexed by the element index within the row), or NULL.
 *   y, xkn   : row b has the bits of spx_iproxstep_X on that row with lambda[b] (l[b], u[b] as l_scalar, u_scalar),
 *              check_d = 0 and the vector d + d_shift[b] formed beforehand by one IEEE add.  xkn (= (xk + sj) + y) may be NULL.
 *   stats_dev: DEVICE double[4 * batch], not NULL.  stats_dev[4 b + {0, 1, 2, 3}] = {lambda[b] * sum over the SELECTED
 *              indices of Term((xk + sj) + y), sum over ALL i of g[i] * y[i], sum over ALL i of (deff[i] * y[i]) * y[i] in that
 *              association, sum over ALL i of y[i]^2} of row b.  The sums are added in a fixed order that depends on n, on the
 *              parity of b * ld and on the alignment of the bases, not on batch and not on the other rows.
 *   d_flag   : (unboxed forms) DEVICE int32[batch], not NULL when batch > 0.  After the call d_flag[b] is 1 when some deff <= 0
 *              or NaN occurred in row b, else 0: the reference's `@assert d[i] > 0`, per problem, without a read-back.  The
 *              call clears the words itself (n <= 12288: the workgroup that owns the row, inside the one launch; larger n: a
 *              zeroing kernel in front, no memset node).
 *   There is no host destination and no check_d: the call always only enqueues.  Capturable under the rules stated in spx.h
 *   (the same call made once before on the context; only n > 12288 needs workspace).
 *   Refused with SPX_ERR_INVALID_ARG, nothing launched: y == g or y == d; xkn equal to y, g, d, xk, sj or sel_mask; ld < n;
 *   batch < 0 or n < 0; NULL lambda, stats_dev, l, u or d_flag (with batch > 0); a call that needs more than 2^31 - 1
 *   workgroups (batch, or batch * ceil(n / 3072) for n > 12288).
 *   batch == 0: SPX_OK, nothing done.  n == 0: 4 * batch zeros stored to stats_dev (unboxed forms: and batch zero words to
 *   d_flag) by a kernel (no memset node).
 *   Non-finite data: the contract stated in spx.h for spx_iproxstep_*, per problem -- a NaN in one row touches that row's y,
 *   sums and flag only. */
int spx_iproxstep_l1_batch(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,
                           int64_t n, int64_t batch, int64_t ld, const double* lambda, const double* d_shift, int32_t* d_flag,
                           double* xkn, double* stats_dev);
int spx_iproxstep_l0_batch(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,
                           int64_t n, int64_t batch, int64_t ld, const double* lambda, const double* d_shift, int32_t* d_flag,
                           double* xkn, double* stats_dev);
int spx_iproxstep_l1_box_batch(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,
                               int64_t n, int64_t batch, int64_t ld, const double* lambda, const double* d_shift,
                               const double* l, const double* u, const uint8_t* sel_mask, double* xkn, double* stats_dev);
int spx_iproxstep_l0_box_batch(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,
                               int64_t n, int64_t batch, int64_t ld, const double* lambda, const double* d_shift,
                               const double* l, const double* u, const uint8_t* sel_mask, double* xkn, double* stats_dev);

#ifdef __cplusplus
}
#endif

#endif /* SPX_IBATCH_H */
