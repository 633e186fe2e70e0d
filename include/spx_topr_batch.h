/* spx_topr_batch.h -- C ABI of libspx_topr_batch.so: the batched ShiftedIndBallL0 / ShiftedIndBallL0BInf prox! + step statistics
 * (MI355X / gfx950 only).  A library of its own next to libspx.so, against which it links: contexts, streams, status codes and
 * spx_last_error are those of spx.h; a context created by spx_ctx_create[_on_stream] serves all the libraries.  Additive:
 * spx_abi_version() stays 1. */
#ifndef SPX_TOPR_BATCH_H
#define SPX_TOPR_BATCH_H

#include "spx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched top-r prox! (with and without an l-infinity trust region) + step statistics, parameters on the device ---- */
/* `batch` top-r problems in ONE call, each with its own r (and radius delta) and q_scale: best-subset or IHT over a path of r,
 * cross-validation folds, multi-start.  ShiftedIndBallL0, shifted(IndBallL0(r), xk) shifted by sj, and ShiftedIndBallL0BInf,
 * shifted(IndBallL0(r), xk, Delta, NormLinf(1)) (what spx_prox_indball_l0 / spx_prox_indball_l0_binf compute), Float64, device
 * pointers only.  ONE workgroup owns one problem through its whole selection: no workgroup waits for another.
 *   layout   : problem b occupies elements [b * ld, b * ld + n) of y, q, xk, sj and xkn, ld >= n.  The elements
 *              [b * ld + n, (b + 1) * ld) are never read or written.  Any 8-byte alignment is allowed: the launch takes the
 *              16-byte pairs form when ld is even, n >= 2 and y, q, xk and sj are all 16-byte aligned; otherwise the element-wise
 *              form for EVERY row (the launch's ALIGNMENT CLASS).
 *   r, delta, q_scale : DEVICE int64_t[batch], double[batch], double[batch], read by the workgroup that owns row b.  Nothing is
 *              read back, nothing synchronises, and a captured call follows the values that are in the arrays when the graph is
 *              replayed -- a solver that walks each problem's sparsity or radius on the device needs no host round trip.
 *              r[b] <= 0 keeps nothing, r[b] >= n keeps everything.  The parameters are not checked on the device: with
 *              Delta_b <= 0 or NaN row b holds whatever jl_min(jl_max(., -Delta_b), Delta_b) gives -- the values
 *              spx_prox_indball_l0_binf gives with that Delta -- the call still terminates (the selection has a fixed cap of
 *              passes) and no other row is touched.
 *   y        : with v = (xk + sj) + q_scale[b] q, where q_scale[b] * q[i] is ONE rounded multiply: the r[b] entries of v largest
 *              in magnitude are kept -- ties to the lowest index first, all NaNs one key above Inf, the order of the reference's
 *              stable sort -- the others zeroed, then xk + sj is subtracted; the BInf form then clamps with
 *              jl_min(jl_max(., -Delta_b), Delta_b).  Row b of y has the BITS of spx_prox_indball_l0[_binf] on that row with
 *              r[b] (and delta[b]) and a q that was multiplied by q_scale[b] on the host -- in every form and at every alignment:
 *              the selection is exact and every element is computed by the single call's expression.
 *   xkn      : xkn[i] = (xk[i] + sj[i]) + y[i] of the stored y, for every i.  It may be NULL, and it may sit at another alignment
 *              than the rest: then only its stores drop to 8 bytes, y and the sums keep their bits.
 *   stats_dev: DEVICE double[3 * batch], not NULL.  For row b: [3 b] = the NUMBER of i with (xk[i] + sj[i]) + y[i] != 0 over the
 *              STORED y, as a double, exact (a NaN counts as nonzero); [3 b + 1] = sum of q[i] * y[i] with q AS PASSED;
 *              [3 b + 2] = sum of y[i]^2.
 *              h of the new point -- the indicator of the l0 ball -- is 0 iff stats_dev[3 b] <= r[b], and +Inf otherwise.  The
 *              plain form always lands in the ball.  The BInf form need not: a dropped entry is clamp(0 - (xk + sj), +-Delta), so
 *              xk + sj + y stays nonzero wherever |xk + sj| > Delta.  [3 b] is the count and not h because the count is what the
 *              caller cannot recover from h: h follows from the count by one comparison, and a solver that shrinks Delta or r
 *              wants to know by how much the point misses the ball.
 *   reproducibility: the selection is exact, and every sum is added in a fixed order that depends on n and on the launch's
 *              alignment class only; not on batch, on b, on the other rows or on timing.  A repeat gives the same bits; the same
 *              problem in another row of a call of the same shape and alignment class gives the same bits; row b of a batch gives
 *              the bits of a batch-of-1 call on that row.
 *   workspace: NONE.  The call reserves no workspace and touches nothing of the context's synchronisation state: each row's
 *              workgroup stores its own three doubles, and nothing needs clearing before a launch.  There is no host destination:
 *              the call always only enqueues, and it is capturable cold (it has nothing a warm call would have to reserve).
 *   forms    : n <= 8192: v, xk + sj and q of the row stay in registers across the digit passes (64 .. 512 lanes by n), 40 bytes
 *              of traffic per element; 8192 < n <= 2^20: the workgroup parks v in the row of y and re-reads it once per digit,
 *              which is why y may be none of the inputs.
 *   **THE WRONG TOOL FOR ONE LARGE PROBLEM**: one workgroup runs on one CU.  With batch = 1 the call is no faster than
 *              spx_prox_indball_l0[_binf] at any n, and beyond n = 8192 it is SLOWER: 0.74 - 0.91 of that call's speed at n = 1e4,
 *              0.16 - 0.17 at n = 1e5 (profiles/topr_proxstep_batch_timing.txt); at n = 1e5 sixteen rows gain only 2.2 - 2.4x over
 *              the loop.  A single problem of more than a few thousand elements belongs to spx_prox_indball_l0[_binf], which
 *              spreads it over many CUs.  From batch = 16 on and n <= 1e4 the call is 11 - 780x the loop of single calls.
 *   Refused with SPX_ERR_INVALID_ARG, nothing launched: y equal to q, xk or sj; xkn equal to y, q, xk or sj; ld < n; n < 0 or
 *   batch < 0; n > 2^20 (spx_prox_indball_l0[_binf] spreads such a problem over many CUs: one problem per call);
 *   batch > 2^31 - 1; a NULL r, delta, q_scale or stats_dev with batch > 0.
 *   batch == 0: SPX_OK, nothing done.  n == 0: 3 * batch zeros stored to stats_dev by a kernel (no memset node).
 *   Non-finite data: per problem -- a NaN or +-Inf in one row touches that row's y and sums only; inside the row they are ordered
 *   as above (NaN above Inf above every finite value). */
int spx_proxstep_indball_l0_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                  int64_t n, int64_t batch, int64_t ld,
                                  const int64_t* r, const double* q_scale, double* xkn, double* stats_dev);
int spx_proxstep_indball_l0_binf_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                       int64_t n, int64_t batch, int64_t ld,
                                       const int64_t* r, const double* delta, const double* q_scale,
                                       double* xkn, double* stats_dev);

#ifdef __cplusplus
}
#endif

#endif /* SPX_TOPR_BATCH_H */
