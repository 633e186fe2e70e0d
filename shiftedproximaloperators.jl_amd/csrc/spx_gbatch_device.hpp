// spx_gbatch_device.hpp -- the host run of the batched group calls (spx_gbatch.hip: ShiftedGroupNormL2, spx_gbinf_batch.hip:
// ShiftedGroupNormL2Binf), stated once, as run_batch (spx_batch_device.hpp) states the separable calls': the refusals, the
// alignment bits, the plan (gbatch_plan, spx_plan.hpp), the workspace of the tiled form, zeros by a kernel when n == 0, the
// launch and the reduce of the tiled form's partials.  What differs between the calls is a Kind (one struct in each .hip file):
//   kLibName       the library, for the text of the ABI mismatch
//   Tiles          the tile table of the main launch (GroupTilesPlain, GroupTilesBinf)
//   kHasDelta      the call has a delta array
//   kBadGroupSize, kNullParams      the refusal texts that name the call's own single-call entry point and parameter arrays
//   launch<Row, TILED, PAIRS>(c, p, out)      the kernel that stores y, on the size's row of Tiles
//   kReduce        the reduce kernel of the tiled form
#pragma once
#include "spx_group_common.hpp"
#include "spx_batch_device.hpp"

namespace {
// the operands of a batched group call, stated once at the entry point (delta: kHasDelta only)
struct GBatchCall {
  spx_ctx* ctx;
  double* y;
  const double *q, *xk, *sj;
  int64_t group_size, ngroups, batch, ld;
  const double* lambda_vec;
  int64_t ldl;
  const double *lambda_scale, *sigma, *delta, *q_scale;
  double *xkn, *stats_dev;
};
// Every refusal is made before anything is enqueued.  There is no host destination: the call only enqueues.
template <class Kind>
int run_gbatch(const GBatchCall& c) {
  spx_ctx* const ctx = c.ctx;
  SPX_REQUIRE_SHARED_ABI(Kind::kLibName);
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(c.group_size >= 1 && c.group_size <= kGroupRegMax, Kind::kBadGroupSize);
  SPX_REQUIRE(c.ngroups >= 0, "ngroups < 0");
  SPX_REQUIRE(c.batch >= 0, "batch < 0");
  SPX_REQUIRE(c.ngroups <= INT64_MAX / c.group_size, "ngroups * group_size overflows");
  const int64_t n = c.ngroups * c.group_size;
  if (c.batch == 0) return SPX_OK;
  SPX_REQUIRE(c.stats_dev != nullptr, "stats_dev is NULL");
  SPX_REQUIRE(c.ld >= n, "ld < n");
  SPX_REQUIRE(c.ldl == 0 || c.ldl >= c.ngroups, "ldl is neither 0 (shared weights) nor >= ngroups");
  const void* const in[4] = {c.y, c.q, c.xk, c.sj};
  if (n > 0) {
    SPX_REQUIRE(c.lambda_vec != nullptr && c.sigma != nullptr && (!Kind::kHasDelta || c.delta != nullptr) && c.q_scale != nullptr,
                Kind::kNullParams);
    for (const void* v : in) SPX_REQUIRE(v != nullptr, "NULL vector with n > 0");
    SPX_REQUIRE(c.y != c.q, kSpxYAliasesQ);
    if (c.xkn != nullptr) {
      for (const void* o : in) SPX_REQUIRE(c.xkn != o, "xkn is one of the other vectors");
    }
  }
  int bits = spx_aligned16(c.xkn) ? 0 : 1 << 4;
  for (int v = 0; v < 4; ++v) bits |= spx_aligned16(in[v]) ? 0 : 1 << v;
  const GBatchPlan p = gbatch_plan(c.group_size, Kind::Tiles::lpg(c.group_size), c.ngroups, c.batch, c.ld, bits);
  SPX_REQUIRE(p.ok, "the call needs more than 2^31 - 1 workgroups");
  if (n == 0) {  // zeros for every problem, by a kernel
    SPX_ON_DEVICE(ctx);
    return spx_zero_async(ctx, c.stats_dev, (size_t)c.batch * kGBatchPlanes * sizeof(double));
  }
  const bool tiled = p.form == BatchForm::kTiled;
  if (tiled) {
    const int rcw = spx_ws_reserve(ctx, p.ws_bytes);
    if (rcw) return rcw;
  }
  SPX_ON_DEVICE(ctx);
  double* const out = tiled ? reinterpret_cast<double*>(ctx->ws) : c.stats_dev;
  Kind::Tiles::select(c.group_size, [&](auto row) {
    with_bool(tiled, [&](auto T) {
      with_bool(p.pairs, [&](auto P) { Kind::template launch<decltype(row), decltype(T)::value, decltype(P)::value>(c, p, out); });
    });
  });
  SPX_LAUNCH_CHECK();
  if (tiled) {
    hipLaunchKernelGGL(Kind::kReduce, dim3((unsigned)c.batch), dim3(256), 0, ctx->stream, (const double*)out, p.tiles_per_problem,
                       c.stats_dev);
    SPX_LAUNCH_CHECK();
  }
  return SPX_OK;
}
}  // namespace
