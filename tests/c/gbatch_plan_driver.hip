/* Stand-alone driver for the device-free plan of the batched group call (csrc/spx_plan.hpp: gbatch_plan, gbatch_run,
 * gbatch_tile_groups, with batch_workgroup and batch_slot of the separable calls) -- the functions k_group_batch of
 * csrc/spx_gbatch.hip finds its groups with -- on the tile table the kernel is instantiated from (GroupTilesPlain,
 * csrc/spx_group_common.hpp).  The walk of a workgroup is restated here wave by wave, slot by slot and lane by lane with the
 * lane-to-element mapping of group_l2_step_site (pairs: lane j owns the pairs j, j + LPG, ...; element-wise: the elements
 * j, j + LPG, ...).  Over group_size = 1 .. 512, with ngroups around the multiples of 4 (64 / LPG) -- the groups a workgroup
 * serves side by side --, around the row / tiled boundary and around the multiples of a tile's run:
 *   - every group belongs to exactly one (problem, tile) and, inside it, to one slot of one wave tile of one wave;
 *   - tiles hold whole groups; a run is a multiple of 4 (64 / LPG) groups and at most kBatchTile elements unless one such
 *     multiple is already larger;
 *   - every element of every row is touched exactly once and no padding element is (sampled ngroups, batch of 2);
 *   - the form, the run and the tiles depend on (group_size, ngroups) only -- not on batch, ld or the alignment bits; pairs
 *     exactly when group_size and ld are even and no base is off a 16-byte boundary;
 *   - grid and workspace are as stated, every slot of the workspace written by one workgroup;
 *   - a grid beyond 2^31 - 1 workgroups is refused, at the edge accepted.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_gbatch_plan_host.py; it has its own main, the library is not loaded, no HIP call is made. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "spx_group_common.hpp"

static long g_checked = 0;
static int g_fail = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++g_checked;                                                                               \
    if (!(cond)) { if (g_fail < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

static int tile_epl(int64_t gs) {
  int e = 0;
  GroupTilesPlain::select(gs, [&](auto row) { e = decltype(row)::epl; });
  return e;
}

// k_group_batch: the groups the workgroup that owns [g_lo, g_hi) serves -- touch(group) once per (wave, wave tile, live slot)
template <class Touch>
static void walk_groups(int64_t g_lo, int64_t g_hi, int gpw, Touch&& touch) {
  for (int w = 0; w < 4; ++w)
    for (int64_t g0 = g_lo + (int64_t)w * gpw; g0 < g_hi; g0 += 4 * gpw)
      for (int slot = 0; slot < gpw; ++slot)
        if (g0 + slot < g_hi) touch(g0 + slot);
}
// group_l2_step_site: the elements [0, gs) of a group its LPG lanes store, EPL slots each
template <class Mark>
static void walk_site(int64_t gs, int lpg, int epl, bool pairs, Mark&& mark) {
  for (int j = 0; j < lpg; ++j) {
    if (pairs) {
      const int64_t npairs = gs >> 1;
      for (int k = 0; k < epl / 2; ++k)
        if (k * lpg + j < npairs) { mark(2 * (int64_t)(k * lpg + j)); mark(2 * (int64_t)(k * lpg + j) + 1); }
    } else {
      for (int k = 0; k < epl; ++k)
        if (k * lpg + j < gs) mark((int64_t)(k * lpg + j));
    }
  }
}

static void check_site(int64_t gs, int lpg, int epl) {
  CHECK(lpg * epl >= gs && 64 % lpg == 0 && epl % 2 == 0);
  for (int pairs = 0; pairs < 2; ++pairs) {
    if (pairs && (gs & 1)) continue;
    std::vector<unsigned char> hits((size_t)gs, 0);
    int64_t outside = 0;
    walk_site(gs, lpg, epl, pairs != 0, [&](int64_t e) { if (e < 0 || e >= gs) ++outside; else ++hits[(size_t)e]; });
    int64_t bad = 0;
    for (int64_t e = 0; e < gs; ++e) bad += hits[(size_t)e] != 1;
    CHECK(bad == 0 && outside == 0);
  }
}

// every group of every problem in exactly one (problem, tile), once
static void check_groups(int64_t gs, int lpg, int64_t ngroups, int64_t batch, const GBatchPlan& p) {
  const int gpw = 64 / lpg;
  std::vector<unsigned char> hits((size_t)(batch * ngroups), 0);
  int64_t outside = 0;
  for (int64_t wg = 0; wg < p.grid; ++wg) {
    int64_t b = wg, t = 0, lo = 0, hi = ngroups;
    if (p.form == BatchForm::kTiled) {
      batch_workgroup(wg, p.tiles_per_problem, &b, &t);
      gbatch_tile_groups(ngroups, t, p.run, &lo, &hi);
      CHECK(b >= 0 && b < batch && t >= 0 && t < p.tiles_per_problem && b * p.tiles_per_problem + t == wg);
      CHECK(lo == t * p.run && hi > lo && hi <= ngroups && (hi - lo == p.run || t == p.tiles_per_problem - 1));  // whole groups, no empty tile
      CHECK((hi - lo) * gs <= kBatchTile || hi - lo == 4 * gpw);
    }
    walk_groups(lo, hi, gpw, [&](int64_t g) { if (g < 0 || g >= ngroups) ++outside; else ++hits[(size_t)(b * ngroups + g)]; });
  }
  int64_t bad = 0;
  for (size_t i = 0; i < hits.size(); ++i) bad += hits[i] != 1;
  CHECK(bad == 0 && outside == 0);
}

// a batch of two rows with `pad` elements of padding: the launch, workgroup by workgroup, touches every row element once
static void check_elements(int64_t gs, int lpg, int epl, int64_t ngroups, int64_t pad, int bits) {
  const int64_t batch = 2, n = ngroups * gs, ld = n + pad, total = batch * ld;
  const GBatchPlan p = gbatch_plan(gs, lpg, ngroups, batch, ld, bits);
  CHECK(p.ok);
  std::vector<unsigned char> hits((size_t)total, 0);
  int64_t outside = 0;
  for (int64_t wg = 0; wg < p.grid; ++wg) {
    int64_t b = wg, t = 0, lo = 0, hi = ngroups;
    if (p.form == BatchForm::kTiled) {
      batch_workgroup(wg, p.tiles_per_problem, &b, &t);
      gbatch_tile_groups(ngroups, t, p.run, &lo, &hi);
    }
    walk_groups(lo, hi, 64 / lpg, [&](int64_t g) {
      const int64_t base = b * ld + g * gs;
      if (p.pairs) CHECK((base & 1) == 0);  // (8-byte units from a 16-byte boundary: every group starts on one)
      walk_site(gs, lpg, epl, p.pairs, [&](int64_t e) {
        if (base + e < 0 || base + e >= total) ++outside; else ++hits[(size_t)(base + e)];
      });
    });
  }
  int64_t bad = 0;
  for (int64_t e = 0; e < total; ++e) bad += hits[(size_t)e] != ((e % ld) < n ? 1 : 0);  // rows once, padding never
  CHECK(bad == 0 && outside == 0);
}

static void check_call(int64_t gs, int lpg, int64_t ngroups, int64_t batch, int64_t ld, int bits, const GBatchPlan& of_shape) {
  const int64_t n = ngroups * gs;
  const GBatchPlan p = gbatch_plan(gs, lpg, ngroups, batch, ld, bits);
  CHECK(p.ok);
  CHECK(p.form == of_shape.form && p.run == of_shape.run && p.tiles_per_problem == of_shape.tiles_per_problem);
  CHECK((p.form == BatchForm::kRow) == (n <= kBatchRowMax));
  CHECK(p.pairs == ((gs & 1) == 0 && (ld & 1) == 0 && bits == 0));
  if (p.form == BatchForm::kRow) {
    CHECK(p.grid == batch && p.ws_bytes == 0 && p.tiles_per_problem == 1 && p.run == ngroups);
  } else {
    const int64_t quad = 4 * (64 / lpg);
    CHECK(p.run == gbatch_run(gs, lpg) && p.run % quad == 0 && p.run >= quad);
    CHECK(p.run * gs <= kBatchTile || p.run == quad);
    CHECK((p.run + quad) * gs > kBatchTile);  // the largest such run
    CHECK(p.tiles_per_problem == (ngroups + p.run - 1) / p.run && p.tiles_per_problem >= 5);
    CHECK(p.grid == batch * p.tiles_per_problem);
    CHECK(p.ws_bytes == (size_t)batch * kGBatchPlanes * (size_t)p.tiles_per_problem * sizeof(double));
    if (batch > 0) {
      const int64_t slots = (int64_t)(p.ws_bytes / sizeof(double)), tiles = p.tiles_per_problem;
      CHECK(batch_slot(0, 0, 0, tiles, kGBatchPlanes) == 0 && batch_slot(batch - 1, kGBatchPlanes - 1, tiles - 1, tiles, kGBatchPlanes) == slots - 1);
      if (p.grid <= 64) {  // every slot the reduce reads is written by one workgroup
        std::vector<unsigned char> seen((size_t)slots, 0);
        for (int64_t wg = 0; wg < p.grid; ++wg) {
          int64_t b, t;
          batch_workgroup(wg, tiles, &b, &t);
          for (int pl = 0; pl < kGBatchPlanes; ++pl) ++seen[(size_t)batch_slot(b, pl, t, tiles, kGBatchPlanes)];
        }
        int64_t bad = 0;
        for (int64_t s = 0; s < slots; ++s) bad += seen[(size_t)s] != 1;
        CHECK(bad == 0);
      }
    }
  }
  CHECK(p.grid <= kBatchGridMax);
}

int main() {
  const int64_t batches[] = {0, 1, 2, 3, 7, 256, 65536, 70001};
  const int aligns[] = {0, 1 << 4, 1, 31};  // all on a boundary; xkn alone off; y alone off; all off
  for (int64_t gs = 1; gs <= kGroupRegMax; ++gs) {
    const int lpg = GroupTilesPlain::lpg(gs), epl = tile_epl(gs);
    CHECK(lpg > 0 && epl > 0);
    check_site(gs, lpg, epl);
    const int64_t quad = 4 * (64 / lpg), edge = kBatchRowMax / gs, run = gbatch_run(gs, lpg);
    std::vector<int64_t> counts = {0, 1, 2, quad - 1, quad, quad + 1, 2 * quad - 1, 2 * quad, 2 * quad + 1, 3 * quad + 1, edge - 1, edge,
                                   edge + 1, edge + quad, run - 1, run, run + 1, 5 * run - 1, 5 * run, 5 * run + 1, 2 * edge + 3};
    for (int64_t ngroups : counts) {
      if (ngroups < 0) continue;
      const GBatchPlan of_shape = gbatch_plan(gs, lpg, ngroups, 1, ngroups * gs, 0);
      for (int64_t batch : batches)
        for (int64_t pad = 0; pad < 4; ++pad)
          for (int bits : aligns) check_call(gs, lpg, ngroups, batch, ngroups * gs + pad, bits, of_shape);
      if (ngroups > 0) {
        const GBatchPlan p3 = gbatch_plan(gs, lpg, ngroups, 3, ngroups * gs, 0);
        check_groups(gs, lpg, ngroups, 3, p3);
      }
    }
    for (int64_t ngroups : {(int64_t)1, quad + 1, edge, edge + 1})
      for (int64_t pad : {0, 1, 2})
        for (int bits : {0, 1 << 4}) check_elements(gs, lpg, epl, ngroups, pad, bits);
  }
  // more than 2^31 - 1 workgroups: refused, at the edge accepted
  CHECK(gbatch_plan(8, 4, 4, kBatchGridMax, 32, 0).ok && !gbatch_plan(8, 4, 4, kBatchGridMax + 1, 32, 0).ok);
  CHECK(!gbatch_plan(8, 4, 0, kBatchGridMax + 1, 0, 0).ok);
  {
    const int64_t gs = 8, ngroups = kBatchRowMax / gs + 1;  // just tiled
    const GBatchPlan one = gbatch_plan(gs, 4, ngroups, 1, ngroups * gs, 0);
    CHECK(one.form == BatchForm::kTiled && one.tiles_per_problem == 5);
    const int64_t most = kBatchGridMax / one.tiles_per_problem;
    const GBatchPlan a = gbatch_plan(gs, 4, ngroups, most, ngroups * gs, 0), b = gbatch_plan(gs, 4, ngroups, most + 1, ngroups * gs, 0);
    CHECK(a.ok && a.grid == most * one.tiles_per_problem && !b.ok);
    CHECK(!gbatch_plan(gs, 4, ngroups, (int64_t)1 << 62, ngroups * gs, 0).ok);  // (no overflow on the way to the refusal)
  }
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
