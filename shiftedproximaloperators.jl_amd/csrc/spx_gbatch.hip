// spx_gbatch.hip -- batched ShiftedGroupNormL2 prox! + step statistics, parameters on the device (spx_proxstep_group_l2_batch,
// include/spx_gbatch.h).  Built into a library of its own, libspx_gbatch.so, which links against libspx.so (the context, its
// workspace, the error text).  `batch` problems of ngroups uniform groups in ONE launch, problem b at elements [b * ld, b * ld + n)
// of every vector; sigma[b], q_scale[b] and the group weights are read from device memory by the workgroup that stores y.
// The group site is group_l2_step_site (spx_group_common.hpp) on the size's row of GroupTilesPlain: the tile and the
// lane-to-element mapping of the single call's k_group_reg, hence its bits in y and xkn.  Which form, run, grid and workspace:
// gbatch_plan (spx_plan.hpp); the host run: run_gbatch (spx_gbatch_device.hpp).  No workgroup waits for another: no tickets, no
// atomics; the only synchronisation is the pair of barriers inside block_sum4.
//   row form   : workgroup b owns problem b; wave w takes the wave tiles (64 / LPG groups each) w, w + 4, ...; the lanes keep
//                their three sums in registers, block_sum4 adds them and lane 0 stores the triple.  One launch, no workspace.
//   tiled form : workgroup (b, t) takes the groups gbatch_tile_groups(t) the same way and stores three partials to
//                batch_slot(b, plane, t); k_gbatch_reduce, one workgroup per problem, adds them in a fixed order
//                (batch_reduce_body, plane 0 as it is: the terms carry their weights).
#include "spx_gbatch.h"
#include "spx_gbatch_device.hpp"

namespace {
// what a kernel is launched with
struct GBatchArgs {
  double* y;
  const double *q, *xk, *sj;
  double* xkn;  // or NULL
  const double *lambda, *lscale /* or NULL */, *sigma, *qscale;
  int64_t ngroups, ld, ldl, run, tiles;
  int gsize;
  double* out;  // stats_dev (row form) or the partials (TILED)
};

template <int LPG, int EPL, bool TILED, bool PAIRS>
__global__ __launch_bounds__(256) void k_group_batch(GBatchArgs k) {
  constexpr int GPW = 64 / LPG;  // groups per wave tile
  const int lane = threadIdx.x & 63;
  const int j = lane % LPG;
  const int slot = lane / LPG;
  const int w = threadIdx.x >> 6;
  int64_t b = blockIdx.x, t = 0, g_lo = 0, g_hi = k.ngroups;
  if constexpr (TILED) {
    batch_workgroup(blockIdx.x, k.tiles, &b, &t);
    gbatch_tile_groups(k.ngroups, t, k.run, &g_lo, &g_hi);
  }
  // the problem's scalars: b is uniform, so these are scalar loads
  const double sigma = k.sigma[b], qs = k.qscale[b];
  const bool scaled = k.lscale != nullptr;
  const double ls = scaled ? k.lscale[b] : 0.0;
  const double* const lam_row = k.lambda + b * k.ldl;
  const int64_t off = b * k.ld;
  const int64_t GS = k.gsize;
  // as k_group_reg decides: cached accesses where a lane's pairs share cache lines with each other (one or two lanes per group) or
  // a partly filled tile of up to 16 lanes per group leaves runs that straddle lines; full tiles and wide groups stream
  const bool cached = LPG <= 2 || (LPG <= 16 && k.gsize != LPG * EPL);
  GroupStepSums acc = {0.0, 0.0, 0.0};
  for (int64_t g0 = g_lo + (int64_t)w * GPW; g0 < g_hi; g0 += 4 * GPW) {  // wave-uniform trip count
    const bool valid = (g0 + slot) < g_hi;
    const int64_t g = valid ? (g0 + slot) : (g_hi - 1);  // idle slots shadow the last group, no store
    double lam = lam_row[g];
    if (scaled) lam = ls * lam;  // one rounded multiply (the library is built without contraction)
    const int64_t base = off + g * GS;
    acc = group_l2_step_site<LPG, EPL, PAIRS>(acc, k.y + base, k.q + base, k.xk + base, k.sj + base, k.xkn ? k.xkn + base : nullptr,
                                              k.gsize, j, valid, lam, sigma, qs, cached);
  }
  SepSums<3> s = {{acc.h, acc.qy, acc.yy}};
  s = block_sum4(s);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      if constexpr (TILED) k.out[batch_slot(b, p, t, k.tiles, kGBatchPlanes)] = s.v[p];
      else k.out[3 * b + p] = s.v[p];
    }
  }
}
__global__ __launch_bounds__(256) void k_gbatch_reduce(const double* partials, int64_t tiles, double* stats) {
  batch_reduce_body<kGBatchPlanes, false>(partials, tiles, nullptr, stats);
}
// what the host run (run_gbatch, spx_gbatch_device.hpp) takes from this call
struct GroupL2Kind {
  static constexpr const char* kLibName = "libspx_gbatch.so";
  using Tiles = GroupTilesPlain;
  static constexpr bool kHasDelta = false;
  static constexpr const char* kBadGroupSize = "group_size outside 1 .. 512 (larger groups: spx_proxstep_group_l2, one problem per call)";
  static constexpr const char* kNullParams = "a parameter array (lambda_vec, sigma, q_scale) is NULL";
  template <class Row, bool TILED, bool PAIRS>
  static void launch(const GBatchCall& c, const GBatchPlan& p, double* out) {
    const GBatchArgs a{c.y, c.q, c.xk, c.sj, c.xkn, c.lambda_vec, c.lambda_scale, c.sigma, c.q_scale, c.ngroups, c.ld, c.ldl, p.run,
                       p.tiles_per_problem, (int)c.group_size, out};
    hipLaunchKernelGGL((k_group_batch<Row::lpg, Row::epl, TILED, PAIRS>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, a);
  }
  static constexpr auto kReduce = k_gbatch_reduce;
};
}  // namespace

SPX_EXPORT int spx_proxstep_group_l2_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                           int64_t group_size, int64_t ngroups, int64_t batch, int64_t ld,
                                           const double* lambda_vec, int64_t ldl, const double* lambda_scale, const double* sigma,
                                           const double* q_scale, double* xkn, double* stats_dev) {
  return run_gbatch<GroupL2Kind>({ctx, y, q, xk, sj, group_size, ngroups, batch, ld, lambda_vec, ldl, lambda_scale, sigma, nullptr, q_scale,
                                  xkn, stats_dev});
}
