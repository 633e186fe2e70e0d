// spx_row_batch.hpp -- the one-workgroup-per-row batched site, stated once (spx_b2_batch.hip: ShiftedNormL1B2; spx_topr_batch.hip:
// ShiftedIndBallL0[BInf]).  ONE workgroup owns ONE problem from its first load to its last store: no exchange words, no
// spx_ctx::sync, no workspace.  Which form, tile and unit: row_batch_plan (spx_plan.hpp).  Here is what every such kernel does the
// same way -- the workgroup sum, the load of a unit of a vector, the stores of a unit of y and of xkn -- and the host run: the
// refusals, the alignment bits, the plan, zeros by a kernel when n == 0, the launch.  What a kernel does with a unit stays in its
// own file.  What differs between the calls on the host is a Kind (one struct in each .hip file):
//   kLibName       the library, for the text of the ABI mismatch
//   kShape         the RowBatchShape of the call (spx_plan.hpp)
//   Params         the call's own arguments behind the vectors (parameter arrays, scalars)
//   null_params(par), kNullParams      is one of the parameter arrays NULL, and the refusal text that lists them
//   refuse_alias(c)      the text of the call's own alias refusal beyond y != q and xkn, or NULL
//   kNTooLarge     the refusal text of n > n_max, which names the single call that serves such a problem
//   launch<LANES, EPL, REG, PAIRS>(c, par, p)      the kernel
#pragma once
#include "spx_common.hpp"
#include "spx_plan.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// The device side
// ---------------------------------------------------------------------------------------------
// sums of NV values over a workgroup of <= 16 wavefronts, the same bits in every lane; lds = [3][16], the slots of absent
// wavefronts zero (b2_block_sum_n of spx_b2.hip).  Starts with a barrier.
template <int NV>
__device__ __forceinline__ void row_block_sum(double (&v)[3], double (*lds)[16]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum_dpp(v[k]);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[k][w] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = fold16_sum(lds[k][threadIdx.x & 15]);
}

// A row of n elements at p in units of E = PAIRS ? 2 : 1 elements: ufull = n / E full units (>= 1; pairs: n >= 2) and, in the
// pairs form with odd n, the one-element unit n / 2 behind them.
// Unit u of the rows p[0 .. NVEC) that a pass reads together: loads at a clamped index, never past the row's last full unit, so
// that they need no guard and are all in flight at once; the lane that owns the odd row's last element fetches it alone, behind
// ONE branch for all the vectors (a branch per vector costs 1 to 4 % of a call: profiles/row_batch_shared_timing.txt).  What a
// slot beyond the row holds is the caller's to mask.
template <bool PAIRS, int NVEC>
__device__ __forceinline__ void row_load_unit(const double* const (&p)[NVEC], int u, int ufull, int n, double (&v)[NVEC][PAIRS ? 2 : 1]) {
  const int uc = u < ufull ? u : ufull - 1;
  if constexpr (PAIRS) {
#pragma unroll
    for (int k = 0; k < NVEC; ++k) {
      const f64x2 a = reinterpret_cast<const f64x2*>(p[k])[uc];
      v[k][0] = a.x; v[k][1] = a.y;
    }
    if (2 * u == n - 1) {
#pragma unroll
      for (int k = 0; k < NVEC; ++k) v[k][0] = p[k][n - 1];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NVEC; ++k) v[k][0] = p[k][uc];
  }
}
// Unit u of y (u within the row): (o0, o1) by one 16-byte store where the unit is a full pair, else o0 alone -- the element-wise
// form, or the last element of an odd row
template <bool PAIRS>
__device__ __forceinline__ void row_store_y(double* y, int u, bool full, double o0, double o1) {
  if (PAIRS && full) reinterpret_cast<f64x2*>(y)[u] = f64x2{o0, o1};
  else y[u * (PAIRS ? 2 : 1)] = o0;
}
// ... and of xkn (or NULL): a full pair by one 16-byte store, or by two 8-byte stores where xkn sits 8 bytes off (!xkn_pairs)
template <bool PAIRS>
__device__ __forceinline__ void row_store_xkn(double* xkn, bool xkn_pairs, int u, bool full, double w0, double w1) {
  if (xkn == nullptr) return;
  if (PAIRS && full) {
    if (xkn_pairs) reinterpret_cast<f64x2*>(xkn)[u] = f64x2{w0, w1};
    else { xkn[2 * u] = w0; xkn[2 * u + 1] = w1; }
  } else {
    xkn[u * (PAIRS ? 2 : 1)] = w0;
  }
}

// ---------------------------------------------------------------------------------------------
// The host run
// ---------------------------------------------------------------------------------------------
// the operands every row-owner call has, stated once at the entry point
struct RowBatchCall {
  spx_ctx* ctx;
  double* y;
  const double *q, *xk, *sj;
  int64_t n, batch, ld;
  double *xkn, *stats_dev;  // stats_dev: three doubles per problem
};
template <class Kind, int LANES, int EPL, bool REG>
void row_batch_launch(const RowBatchCall& c, const typename Kind::Params& par, const RowBatchPlan& p) {
  if (p.pairs) Kind::template launch<LANES, EPL, REG, true>(c, par, p);
  else Kind::template launch<LANES, EPL, REG, false>(c, par, p);
}
// the resident launch: one walk of the shape's tile table
template <class Kind, int TILE>
void row_batch_launch_tile(const RowBatchCall& c, const typename Kind::Params& par, const RowBatchPlan& p) {
  if constexpr (TILE < Kind::kShape.tile_count) {
    if (p.tile == TILE) row_batch_launch<Kind, Kind::kShape.tiles[TILE].lanes, Kind::kShape.tiles[TILE].epl, true>(c, par, p);
    else row_batch_launch_tile<Kind, TILE + 1>(c, par, p);
  }
}
// Every refusal is made before anything is enqueued.  There is no host destination: the call only enqueues.
template <class Kind>
int run_row_batch(const RowBatchCall& c, const typename Kind::Params& par) {
  spx_ctx* const ctx = c.ctx;
  SPX_REQUIRE_SHARED_ABI(Kind::kLibName);
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(c.n >= 0, "n < 0");
  SPX_REQUIRE(c.batch >= 0, "batch < 0");
  if (c.batch == 0) return SPX_OK;
  SPX_REQUIRE(c.stats_dev != nullptr, "stats_dev is NULL");
  SPX_REQUIRE(!Kind::null_params(par), Kind::kNullParams);
  SPX_REQUIRE(c.ld >= c.n, "ld < n");
  const void* const in[4] = {c.y, c.q, c.xk, c.sj};
  if (c.n > 0) {
    for (const void* v : in) SPX_REQUIRE(v != nullptr, "NULL vector with n > 0");
    SPX_REQUIRE(c.y != c.q, kSpxYAliasesQ);
    const char* const alias = Kind::refuse_alias(c);
    SPX_REQUIRE(alias == nullptr, alias);
    if (c.xkn != nullptr) {
      for (const void* o : in) SPX_REQUIRE(c.xkn != o, "xkn is one of the other vectors");
    }
  }
  int bits = spx_aligned16(c.xkn) ? 0 : 1 << 4;
  for (int v = 0; v < 4; ++v) bits |= spx_aligned16(in[v]) ? 0 : 1 << v;
  const RowBatchPlan p = row_batch_plan(Kind::kShape, c.n, c.batch, c.ld, bits);
  SPX_REQUIRE(p.ok || p.why != RowBatchRefusal::kNTooLarge, Kind::kNTooLarge);
  SPX_REQUIRE(p.ok, "batch > 2^31 - 1");
  SPX_ON_DEVICE(ctx);
  if (c.n == 0) return spx_zero_async(ctx, c.stats_dev, (size_t)c.batch * 3 * sizeof(double));  // zeros for every problem, by a kernel
  if (p.form == RowBatchForm::kResident) row_batch_launch_tile<Kind, 0>(c, par, p);
  else row_batch_launch<Kind, Kind::kShape.walk_lanes, 0, false>(c, par, p);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}

}  // namespace
