/* spx_b2_batch.h -- C ABI of libspx_b2_batch.so: the batched ShiftedNormL1B2 prox! + step statistics (MI355X / gfx950 only).
 * A library of its own next to libspx.so, against which it links: contexts, streams, status codes and spx_last_error are those
 * of spx.h; a context created by spx_ctx_create[_on_stream] serves all the libraries.  Additive: spx_abi_version() stays 1. */
#ifndef SPX_B2_BATCH_H
#define SPX_B2_BATCH_H

#include "spx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched l1 prox! inside an l2-ball trust region + step statistics, parameters on the device ------------- */
/* `batch` lasso problems inside an l2-ball trust region in ONE call, each with its own lambda, sigma, radius delta and
 * q_scale: the step of a TR solver on a regularisation path, cross-validation folds, multi-start.  ShiftedNormL1B2,
 * shifted(NormL1(lambda), xk, Delta, NormL2(1)) (what spx_proxstep_l1_b2 computes), Float64, device pointers only.  ONE workgroup
 * owns one problem through its whole root iteration: no workgroup waits for another.
 *   layout   : problem b occupies elements [b * ld, b * ld + n) of y, q, xk, sj and xkn, ld >= n.  The elements
 *              [b * ld + n, (b + 1) * ld) are never read or written.  Any 8-byte alignment is allowed: the launch takes the
 *              16-byte pairs form when ld is even, n >= 2 and y, q, xk and sj are all 16-byte aligned; otherwise the element-wise
 *              form for EVERY row (the launch's ALIGNMENT CLASS).
 *   lambda, sigma, delta, q_scale : DEVICE double[batch], read by the workgroup that owns row b.  Nothing is read back, nothing
 *              synchronises, and a captured call follows the values that are in the arrays when the graph is replayed -- a solver
 *              that shrinks or grows each problem's radius on the device needs no host round trip.  lambda[b] * sigma[b] is ONE
 *              rounded multiply, the bits of the host product the single call forms; q_scale[b] * q[i] is one rounded multiply
 *              in front of `sj[i] + ...`.
 *   chi_lambda : one host double for all rows (1.0 in every use of the reference).
 *   The parameters are not checked on the device: Delta_b > 0 and lambda_b sigma_b >= 0 are the caller's responsibility.  With
 *              anything else in row b (Delta_b <= 0, NaN) that row's y and sums are unspecified, but the call still terminates
 *              -- the root iteration has a fixed cap of reductions -- and no other row is touched.
 *   y        : y[b] is prox! of ShiftedNormL1B2 at q_scale[b] q[b], what spx_proxstep_l1_b2 computes on the row, to that call's
 *              accuracy: max |y - ref| <= 1e-12 max(||ref||_2, ||xk||_2) per row against the exact prox.  Bit identity with
 *              the single call is NOT promised in general: that call's bits depend on its grid and its partition of every sum
 *              (spx.h).  It IS promised on a row whose trust region is inactive (Delta_b >= chi(ProjB(-xk))): there y is the
 *              elementwise jl_min(jl_max(-xk, lo), hi) - sj, which needs no sum, and the row has the bits of
 *              spx_proxstep_l1_b2 on that row with host copies of its scalars.
 *   xkn      : xkn[i] = (xk[i] + sj[i]) + y[i] of the stored y, for every i.  It may be NULL, and it may sit at another alignment
 *              than the rest: then only its stores drop to 8 bytes, y and the sums keep their bits.
 *   stats_dev: DEVICE double[3 * batch], not NULL.  For row b: [3 b] = lambda[b] * sum of |(xk + sj) + y| over the STORED y;
 *              [3 b + 1] = sum of q[i] * y[i] with q AS PASSED; [3 b + 2] = sum of y[i]^2.
 *   reproducibility: every sum -- the sums P, C, F that decide the root included -- is added in a fixed order that depends on
 *              n, on the launch's alignment class and on the row's own data and scalars only; not on batch, on b, on the other
 *              rows or on timing.  A repeat gives the same bits; the same problem in another row of a call of the same shape and
 *              alignment class gives the same bits; row b of a batch gives the bits of a batch-of-1 call on that row.
 *   workspace: NONE.  The call reserves no workspace and touches nothing of the context's synchronisation state: each row's
 *              workgroup stores its own three sums, and nothing needs clearing before a launch.  There is no host destination:
 *              the call always only enqueues, and it is capturable (it has nothing a warm call would have to reserve).
 *   forms    : n <= 8192: the row's xk and box ends stay in registers across the reductions (64 .. 512 lanes by n);
 *              8192 < n <= 2^20: the workgroup re-reads its row once per reduction.
 *   Refused with SPX_ERR_INVALID_ARG, nothing launched: y == q; xkn equal to y, q, xk or sj; ld < n; n < 0 or batch < 0;
 *   n > 2^20 (spx_proxstep_l1_b2 holds such a problem on chip across many CUs: one problem per call); batch > 2^31 - 1; a NULL
 *   lambda, sigma, delta, q_scale or stats_dev with batch > 0.
 *   batch == 0: SPX_OK, nothing done.  n == 0: 3 * batch zeros stored to stats_dev by a kernel (no memset node).
 *   Non-finite data: the contract stated in spx.h for spx_proxstep_l1_b2 ("NON-FINITE DATA"), per problem -- a NaN or +-Inf in
 *   one row touches that row's y and sums only. */
int spx_proxstep_l1_b2_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                             int64_t n, int64_t batch, int64_t ld,
                             const double* lambda, const double* sigma, const double* delta, const double* q_scale,
                             double chi_lambda, double* xkn, double* stats_dev);

#ifdef __cplusplus
}
#endif

#endif /* SPX_B2_BATCH_H */
