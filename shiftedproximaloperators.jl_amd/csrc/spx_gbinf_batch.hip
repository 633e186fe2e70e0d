// spx_gbinf_batch.hip -- batched ShiftedGroupNormL2Binf prox! + step statistics, parameters on the device
// (spx_proxstep_group_l2_binf_batch, include/spx_gbinf_batch.h).  Built into a library of its own, libspx_gbinf_batch.so, which
// links against libspx.so (the context, its workspace, the error text).  `batch` trust-region problems of ngroups uniform groups
// in ONE launch, problem b at elements [b * ld, b * ld + n) of every vector; sigma[b], delta[b], q_scale[b] and the group weights
// are read from device memory by the workgroup that stores y.  Which form, run, grid and workspace: gbatch_plan (spx_plan.hpp)
// with the lanes per group of the size's row of GroupTilesBinf; the host run: run_gbatch (spx_gbatch_device.hpp).
//   row form   : workgroup b owns problem b; one launch, no workspace.
//   tiled form : workgroup (b, t) takes the groups gbatch_tile_groups(t) and stores three partials to batch_slot(b, plane, t);
//                k_binf_batch_reduce, one workgroup per problem, adds them in a fixed order (batch_reduce_body).
// A workgroup runs two phases over its own groups:
//   main    : wave w takes the wave tiles (64 / LPG groups each) w, w + 4, ... through group_l2_binf_step_site -- the tile, the
//             lane-to-element mapping and the statements of the single call's main launch.  A group whose root find asks for
//             the reference's literal evaluation (BINF_LITERAL) stores nothing and adds nothing: its bit is set in a bitmap in
//             LDS (1.5 KiB; LDS atomics, several wave tiles share a word).
//   literal : behind one barrier -- skipped when no bit is set -- the waves walk the bitmap in the fixed order of
//             binf_walk_bit (spx_plan.hpp) and evaluate the flagged groups through group_l2_binf_literal_site on the size's row
//             of GroupTilesLit: the tile of the single call's LIT launch, hence its bits.
// Both phases add into the same per-lane sums; block_sum4 adds those and lane 0 stores the triple.  No workgroup waits for
// another: no global atomics, no tickets, no count words, no list in memory, no second launch for the literal groups.
#include "spx_gbinf_batch.h"
#include "spx_gbatch_device.hpp"

namespace {
// min waves/SIMD of the tiles of 8 elements per lane and fewer; 16 elements per lane: 2 (as k_group_reg, spx_group.hip)
constexpr int kBinfBatchWaves = 3;

// what a kernel is launched with
struct GBinfArgs {
  double* y;
  const double *q, *xk, *sj;
  double* xkn;  // or NULL
  const double *lambda, *lscale /* or NULL */, *sigma, *delta, *qscale;
  int64_t ngroups, ld, ldl, run, tiles;
  int gsize;
  int pole_lit;  // tuning key 9
  double* out;   // stats_dev (row form) or the partials (TILED)
};

template <int LPG, int EPL, bool TILED, bool PAIRS>
__global__ __launch_bounds__(256, EPL >= 16 ? 2 : kBinfBatchWaves) void k_binf_batch(GBinfArgs k) {
  using LitRow = typename GroupTileOf<LPG * EPL, GroupTilesLit>::type;  // (a main tile holds exactly its row's bound)
  constexpr int LLPG = LitRow::lpg, LEPL = LitRow::epl;
  constexpr int GPW = 64 / LPG;    // groups per wave tile, main phase
  constexpr int LGPW = 64 / LLPG;  // literal phase
  __shared__ unsigned long long bitmap[kBinfBitmapWords];
  __shared__ unsigned int any_literal;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  int64_t b = blockIdx.x, t = 0, g_lo = 0, g_hi = k.ngroups;
  if constexpr (TILED) {
    batch_workgroup(blockIdx.x, k.tiles, &b, &t);
    // (a 64-bit division runs on the vector unit: hand the uniform quotients back to the scalar registers, or everything derived
    //  from them -- the row's offset, its scalars, the tile's bounds -- occupies vector registers across the root find)
    b = __builtin_amdgcn_readfirstlane((int)b);  // (both below 2^31: the grid is)
    t = __builtin_amdgcn_readfirstlane((int)t);
    gbatch_tile_groups(k.ngroups, t, k.run, &g_lo, &g_hi);
  }
  const int ng = (int)(g_hi - g_lo);  // <= kBatchRowMax: gbatch_plan gives a workgroup that many elements, or one run of groups
  const int nwords = binf_bitmap_words(ng);
  for (int i = threadIdx.x; i < nwords; i += 256) bitmap[i] = 0ull;
  if (threadIdx.x == 0) any_literal = 0u;
  __syncthreads();
  // the problem's scalars: b is uniform, so these are scalar loads
  const double sigma = k.sigma[b], delta = k.delta[b], qs = k.qscale[b];
  const bool scaled = k.lscale != nullptr;
  const double ls = scaled ? k.lscale[b] : 0.0;
  const double* const lam_wg = k.lambda + b * k.ldl + g_lo;  // the weights of the workgroup's groups
  // the workgroup's first element is folded into the vectors (scalar); a lane's group then sits at a 32-bit offset behind them
  const int64_t first = b * k.ld + g_lo * (int64_t)k.gsize;
  double* const y = k.y + first;
  const double *const q = k.q + first, *const xk = k.xk + first, *const sj = k.sj + first;
  double* const xkn = k.xkn ? k.xkn + first : nullptr;
  GroupStepSums acc = {0.0, 0.0, 0.0};
  {
    const int j = lane % LPG;
    const int slot = lane / LPG;
    // as k_group_reg decides: cached accesses on the one- and two-lane tiles and on partly filled tiles of up to 16 lanes per
    // group in the pairs form; full tiles and wide groups stream
    const bool cached = LPG <= 2 || (PAIRS && LPG <= 16 && k.gsize != LPG * EPL);
    for (int l0 = w * GPW; l0 < ng; l0 += 4 * GPW) {  // wave-uniform trip count
      const bool valid = (l0 + slot) < ng;
      const int lg = valid ? (l0 + slot) : (ng - 1);  // idle slots shadow the last group, no store
      double lam = lam_wg[lg];
      if (scaled) lam = ls * lam;  // one rounded multiply (the library is built without contraction)
      const bool literal = group_l2_binf_step_site<LPG, EPL, PAIRS>(acc, y, q, xk, sj, xkn, (unsigned int)(lg * k.gsize), k.gsize, j, valid,
                                                                    lam, sigma, delta, qs, k.pole_lit != 0, cached);
      if (__ballot(literal) != 0ull) {  // wave-uniform, rare
        if (literal && j == 0) atomicOr(&bitmap[lg >> 6], 1ull << (lg & 63));
        if (lane == 0) any_literal = 1u;
      }
    }
  }
  __syncthreads();
  if (__builtin_amdgcn_readfirstlane(any_literal) != 0u) {
    const int j = lane % LLPG;
    const int slot = lane / LLPG;
    for (int wi = w; wi < nwords; wi += kBinfWalkWaves) {
      const unsigned long long mine = bitmap[wi];  // every lane reads the same word: made scalar, the loops below are wave-uniform
      // (readfirstlane returns a signed int: through unsigned, or the low half's bit 31 would fill the high half)
      const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(mine >> 32));
      const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)mine);
      const unsigned long long word = ((unsigned long long)hi << 32) | (unsigned long long)lo;
      const int passes = binf_walk_passes(word, LGPW);
      for (int p = 0; p < passes; ++p) {
        int bit = binf_walk_bit(word, LGPW, p, slot);
        bool valid = bit >= 0;
        if (!valid) bit = binf_walk_bit(word, LGPW, p, 0);  // idle slots shadow the pass's first group, no store
        int lg = wi * 64 + bit;                             // < ng: only a valid group's bit is ever set ...
        if (lg >= ng) { lg = ng - 1; valid = false; }       // ... and a bit that is not a group's is never followed into memory
        double lam = lam_wg[lg];
        if (scaled) lam = ls * lam;
        acc = group_l2_binf_literal_site<LLPG, LEPL, PAIRS>(acc, y, q, xk, sj, xkn, (unsigned int)(lg * k.gsize), k.gsize, j, valid, lam,
                                                            sigma, delta, qs);
      }
    }
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
__global__ __launch_bounds__(256) void k_binf_batch_reduce(const double* partials, int64_t tiles, double* stats) {
  batch_reduce_body<kGBatchPlanes, false>(partials, tiles, nullptr, stats);
}
// what the host run (run_gbatch, spx_gbatch_device.hpp) takes from this call
struct GroupBinfKind {
  static constexpr const char* kLibName = "libspx_gbinf_batch.so";
  using Tiles = GroupTilesBinf;
  static constexpr bool kHasDelta = true;
  static constexpr const char* kBadGroupSize = "group_size outside 1 .. 512 (larger groups: spx_proxstep_group_l2_binf, one problem per call)";
  static constexpr const char* kNullParams = "a parameter array (lambda_vec, sigma, delta, q_scale) is NULL";
  template <class Row, bool TILED, bool PAIRS>
  static void launch(const GBatchCall& c, const GBatchPlan& p, double* out) {
    static_assert(Row::lpg * Row::epl == Row::maxg, "k_binf_batch names its GroupTilesLit row by the main tile's capacity");
    const GBinfArgs a{c.y, c.q, c.xk, c.sj, c.xkn, c.lambda_vec, c.lambda_scale, c.sigma, c.delta, c.q_scale, c.ngroups, c.ld, c.ldl, p.run,
                      p.tiles_per_problem, (int)c.group_size, c.ctx->tune_binf_literal, out};
    hipLaunchKernelGGL((k_binf_batch<Row::lpg, Row::epl, TILED, PAIRS>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, a);
  }
  static constexpr auto kReduce = k_binf_batch_reduce;
};
}  // namespace

SPX_EXPORT int spx_proxstep_group_l2_binf_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                                int64_t group_size, int64_t ngroups, int64_t batch, int64_t ld,
                                                const double* lambda_vec, int64_t ldl, const double* lambda_scale,
                                                const double* sigma, const double* delta, const double* q_scale, double* xkn,
                                                double* stats_dev) {
  return run_gbatch<GroupBinfKind>({ctx, y, q, xk, sj, group_size, ngroups, batch, ld, lambda_vec, ldl, lambda_scale, sigma, delta, q_scale,
                                    xkn, stats_dev});
}
