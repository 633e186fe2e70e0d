/* Stand-alone driver for the device-free plan of the batched separable call (csrc/spx_plan.hpp: batch_plan, batch_row_map,
 * batch_tiles, batch_tile_units, batch_workgroup, batch_slot) -- the functions k_sep_batch and k_batch_reduce of
 * spx_batch.hip walk a row with.  The walk of a workgroup is restated here lane by lane and marks the elements it touches.
 * Over n = 0 ... 2 kBatchRowMax + 7, batch in {0, 1, 2, 3, 255, 256, 257, 65535, 65536, 70001}, ld - n in {0, 1, 2, 3}, the bases
 * all on a 16-byte boundary, all 8 bytes off it, and mixed (the element-wise form):
 *   - every element of a row is touched exactly once, whichever parity the row starts at, and nothing outside [0, n) is.
 *     For EVERY n this is shown in two steps: the tiles' unit intervals partition [0, count) in order (checked for every n),
 *     and the lanes of a workgroup touch every unit of an interval [lo, hi) exactly once.  The second step depends on hi - lo
 *     alone and is checked for EVERY length 0 ... a full tile, in both forms, on tile 0 and on tile 1 (check_tile_lanes).  The
 *     lane-by-lane walk of whole rows (head, pairs, tail together) on top of that is SAMPLED, not run for every n: n <= 700,
 *     n within 9 of every multiple of half a tile, and every 37th n.  The walk restates
 *     batch_tile's loop here (the kernel's own loop carries device loads and stores); what it shares with the kernel is the
 *     mapping functions of spx_plan.hpp;
 *   - a row's pairs start on a 16-byte boundary, rows stay inside [b ld, b ld + n), i.e. clear of the padding;
 *   - workgroup -> (problem, tile) is a bijection onto batch x tiles;
 *   - ws_bytes holds exactly the slots the reduce reads, each written by one workgroup;
 *   - the form depends on n only; a grid beyond 2^31 - 1 workgroups is refused.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_batch_plan_host.py; it has its own main, the library is not loaded, no HIP call is made. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "spx_plan.hpp"

static long g_checked = 0;
static int g_fail = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++g_checked;                                                                               \
    if (!(cond)) { if (g_fail < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

constexpr int kLanes = 256;
constexpr int kPairsPerLane = 6, kElemsPerLane = 12;  // U of batch_tile<.., f64x2, ..> and <.., double, ..>

// batch_tile of spx_batch.hip: the units lane `lane` of the workgroup touches in tile `tile` of `count` units
template <class Touch>
static void walk_tile(int64_t count, int64_t tile, int U, Touch&& touch) {
  int64_t lo, hi;
  batch_tile_units(count, tile, kLanes * U, &lo, &hi);
  for (int lane = 0; lane < kLanes; ++lane) {
    const int64_t base = lo + lane;
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + (int64_t)k * kLanes;
      if (hi - lo == (int64_t)kLanes * U || i < hi) touch(i);
    }
  }
}
// k_sep_batch: the elements of row b (relative to the row's start) that the workgroup owning tiles [t0, t1) touches
static void walk_workgroup(std::vector<unsigned char>& hits, int64_t* outside, int64_t n, int64_t b, int64_t ld, int base_odd,
                           bool pairs, int64_t tiles, int64_t t0, int64_t t1) {
  auto mark = [&](int64_t e) { if (e < 0 || e >= n) ++*outside; else ++hits[(size_t)e]; };
  if (pairs) {
    const BatchRowMap r = batch_row_map(n, b, ld, base_odd);
    for (int64_t t = t0; t < t1; ++t) walk_tile(r.npairs, t, kPairsPerLane, [&](int64_t i) { mark(r.head + 2 * i); mark(r.head + 2 * i + 1); });
    if (t0 == 0 && r.head) mark(0);
    if (t1 == tiles && r.tail) mark(n - 1);
  } else {
    for (int64_t t = t0; t < t1; ++t) walk_tile(n, t, kElemsPerLane, [&](int64_t i) { mark(i); });
  }
}

// the lanes of one workgroup touch every unit of a tile's interval exactly once and nothing else: every length, tiles 0 and 1
static void check_tile_lanes() {
  for (int U : {kPairsPerLane, kElemsPerLane}) {
    const int upt = kLanes * U;
    for (int64_t tile = 0; tile < 2; ++tile) {
      for (int64_t len = 0; len <= upt; ++len) {
        const int64_t count = tile * upt + len;
        std::vector<unsigned char> hits((size_t)count, 0);
        int64_t outside = 0;
        walk_tile(count, tile, U, [&](int64_t i) { if (i < 0 || i >= count) ++outside; else ++hits[(size_t)i]; });
        int64_t bad = 0;
        for (int64_t i = 0; i < count; ++i) bad += hits[(size_t)i] != (i >= tile * upt ? 1 : 0);
        CHECK(bad == 0 && outside == 0);
      }
    }
  }
}

static bool lane_level(int64_t n) {
  if (n <= 700 || n % 37 == 0) return true;
  const int64_t half = kBatchTile / 2;
  const int64_t r = n % half;
  return r <= 9 || r >= half - 9;
}

// one row of n elements that starts at parity `par` (b = par, ld = 1 puts it there), walked by the row form (one workgroup)
// and by the tiled form (one workgroup per tile)
static void check_row_coverage(int64_t n) {
  const int64_t tiles = batch_tiles(n);
  CHECK(tiles == (n + kBatchTile - 1) / kBatchTile);
  for (int pairs = 0; pairs < 2; ++pairs) {
    for (int par = 0; par < 2; ++par) {
      const BatchRowMap r = batch_row_map(n, par, 1, 0);
      CHECK(r.head == (n > 0 ? par : 0) && r.head + 2 * r.npairs + r.tail == n && (r.tail == 0 || r.tail == 1) && r.npairs >= 0);
      // tile intervals: contiguous, in order, together [0, count), none longer than a tile
      const int64_t count = pairs ? r.npairs : n;
      const int upt = kLanes * (pairs ? kPairsPerLane : kElemsPerLane);
      int64_t at = 0;
      for (int64_t t = 0; t < tiles; ++t) {
        int64_t lo, hi;
        batch_tile_units(count, t, upt, &lo, &hi);
        CHECK(lo == at && hi >= lo && hi - lo <= upt && hi <= count);
        at = hi;
      }
      CHECK(at == count);
      if (!lane_level(n)) continue;
      for (int tiled = 0; tiled < 2; ++tiled) {
        std::vector<unsigned char> hits((size_t)n, 0);
        int64_t outside = 0;
        if (!tiled) walk_workgroup(hits, &outside, n, par, 1, 0, pairs != 0, tiles, 0, tiles);
        else for (int64_t t = 0; t < tiles; ++t) walk_workgroup(hits, &outside, n, par, 1, 0, pairs != 0, tiles, t, t + 1);
        int64_t bad = 0;
        for (int64_t e = 0; e < n; ++e) bad += hits[(size_t)e] != 1;
        CHECK(bad == 0 && outside == 0);
      }
    }
  }
}

static void check_call(int64_t n, int64_t batch, int64_t ld, int bits, BatchForm form_of_n) {
  const BatchPlan p = batch_plan(n, batch, ld, bits);
  CHECK(p.ok);
  CHECK(p.form == form_of_n && (p.form == BatchForm::kRow) == (n <= kBatchRowMax));
  CHECK(p.pairs == (bits == 0 || bits == kBatchAllOff) && p.base_odd == (bits == kBatchAllOff ? 1 : 0));
  const int64_t tiles = p.tiles_per_problem;
  CHECK(tiles == batch_tiles(n));
  if (p.form == BatchForm::kRow) CHECK(p.grid == batch && p.ws_bytes == 0);
  else CHECK(p.grid == batch * tiles && p.ws_bytes == (size_t)batch * 3 * (size_t)tiles * sizeof(double));
  CHECK(p.grid <= kBatchGridMax);
  if (batch == 0 || n == 0) return;
  // rows: inside [b ld, b ld + n), clear of the padding [b ld + n, (b + 1) ld); the pairs start on a 16-byte boundary
  const int64_t rows[] = {0, 1, 2, 3, batch / 2, batch - 2, batch - 1};
  for (int64_t b : rows) {
    if (b < 0 || b >= batch) continue;
    const int64_t e0 = b * ld;
    CHECK(e0 + n <= (b + 1) * ld && e0 + n <= batch * ld);
    if (p.pairs) {
      const BatchRowMap r = batch_row_map(n, b, ld, p.base_odd);
      CHECK(r.head + 2 * r.npairs + r.tail == n);
      if (r.npairs > 0) CHECK(((e0 + r.head + p.base_odd) & 1) == 0);  // (8-byte units from a 16-byte boundary)
      CHECK((r.npairs + kLanes * kPairsPerLane - 1) / (kLanes * kPairsPerLane) <= tiles);
    }
  }
  if (p.form != BatchForm::kTiled) return;
  // workgroup -> (problem, tile): onto batch x tiles, one workgroup each; its three slots inside the workspace, no two alike
  const int64_t slots = (int64_t)(p.ws_bytes / sizeof(double));
  auto check_wg = [&](int64_t wg) {
    int64_t b, t;
    batch_workgroup(wg, tiles, &b, &t);
    CHECK(b >= 0 && b < batch && t >= 0 && t < tiles && b * tiles + t == wg);
    for (int pl = 0; pl < 3; ++pl) {
      const int64_t s = batch_slot(b, pl, t, tiles);
      CHECK(s >= 0 && s < slots && s == (b * 3 + pl) * tiles + t);
    }
  };
  if (p.grid <= 64) {
    std::vector<unsigned char> seen((size_t)slots, 0);
    for (int64_t wg = 0; wg < p.grid; ++wg) {
      check_wg(wg);
      int64_t b, t;
      batch_workgroup(wg, tiles, &b, &t);
      for (int pl = 0; pl < 3; ++pl) ++seen[(size_t)batch_slot(b, pl, t, tiles)];
    }
    int64_t bad = 0;
    for (int64_t s = 0; s < slots; ++s) bad += seen[(size_t)s] != 1;  // every slot the reduce reads is written once
    CHECK(bad == 0);
  } else {
    const int64_t wgs[] = {0, 1, tiles - 1, tiles, p.grid / 2, p.grid - tiles, p.grid - 1};
    for (int64_t wg : wgs) check_wg(wg);
  }
  CHECK(batch_slot(batch - 1, 2, tiles - 1, tiles) == slots - 1 && batch_slot(0, 0, 0, tiles) == 0);
}

int main() {
  const int64_t batches[] = {0, 1, 2, 3, 255, 256, 257, 65535, 65536, 70001};
  const int aligns[] = {0, kBatchAllOff, 1 << 4 /* xkn alone 8 bytes off: element-wise */};
  check_tile_lanes();
  for (int64_t n = 0; n <= 2 * kBatchRowMax + 7; ++n) {
    check_row_coverage(n);
    const BatchForm form_of_n = batch_plan(n, 1, n, 0).form;
    for (int64_t batch : batches)
      for (int64_t pad = 0; pad < 4; ++pad)
        for (int bits : aligns) check_call(n, batch, n + pad, bits, form_of_n);
  }
  // more than 2^31 - 1 workgroups: refused, at the edge accepted
  CHECK(batch_plan(5, kBatchGridMax, 5, 0).ok && !batch_plan(5, kBatchGridMax + 1, 5, 0).ok);
  CHECK(!batch_plan(0, kBatchGridMax + 1, 0, 0).ok);
  {
    const int64_t n = kBatchRowMax + 1, tiles = batch_tiles(n);  // 5 tiles a problem
    CHECK(tiles == 5);
    const int64_t most = kBatchGridMax / tiles;
    const BatchPlan a = batch_plan(n, most, n, 0), b = batch_plan(n, most + 1, n, 0);
    CHECK(a.ok && a.grid == most * tiles && !b.ok);
    CHECK(!batch_plan(n, (int64_t)1 << 62, n, 0).ok);  // (no overflow on the way to the refusal)
  }
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
