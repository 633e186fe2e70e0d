/* Stand-alone driver for the device-free plan of the batched iprox! call (csrc/spx_plan.hpp: ibatch_plan, ibatch_slot and the
 * mapping functions it shares with the batched prox!: batch_row_map, batch_tiles, batch_tile_units, batch_workgroup) -- the
 * functions k_isep_batch and k_ibatch_reduce of spx_ibatch.hip walk a row with.  The walk of a workgroup is restated here
 * lane by lane, with the two halves in which ibatch_tile stages a full tile, and marks the elements it touches in each of the
 * SIX vectors of the call (y, g, d, xk, sj, xkn) laid out with their padding.
 * Over n = 0 ... 2 kBatchRowMax + 7, batch in {0, 1, 2, 3, 255, 256, 257, 65535, 65536, 70001}, ld - n in {0, 1, 2, 3}, the bases
 * all on a 16-byte boundary, all 8 bytes off it, and mixed (the element-wise form):
 *   - every element of every row of all six vectors is touched exactly once, whichever parity the row starts at, and no
 *     padding element [b ld + n, (b + 1) ld) is: a batch of three rows with its padding is walked lane by lane for the SAMPLED
 *     sizes (n <= 700, n within 9 of every multiple of half a tile, every 74th n); for EVERY n the tiles' unit intervals are
 *     shown to partition [0, count) in order, and the lanes of a workgroup to touch every unit of an interval of EVERY length
 *     0 ... a full tile exactly once, in both forms, in the staged order (check_tile_lanes);
 *   - a lane visits its units in the order k = 0 .. U - 1 whether a tile is staged whole or in two halves;
 *   - a row's pairs start on a 16-byte boundary;
 *   - workgroup -> (problem, tile) is a bijection onto batch x tiles;
 *   - the four-plane workspace holds exactly the slots the reduce reads, each written by one workgroup;
 *   - the form depends on n only; a grid beyond 2^31 - 1 workgroups is refused.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_ibatch_plan_host.py; it has its own main, the library is not loaded, no HIP call is made. */
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
constexpr int kPairsPerLane = 6, kElemsPerLane = 12;  // U of ibatch_tile<.., f64x2, ..> and <.., double, ..>

// ibatch_tile of spx_ibatch.hip: the units lane `lane` of the workgroup touches in tile `tile` of `count` units, in the lane's
// own order -- a full tile in two halves of U / 2 units, the last tile of a row unit by unit
template <class Touch>
static void walk_tile(int64_t count, int64_t tile, int U, Touch&& touch) {
  int64_t lo, hi;
  batch_tile_units(count, tile, kLanes * U, &lo, &hi);
  const int H = U / 2;
  for (int lane = 0; lane < kLanes; ++lane) {
    const int64_t base = lo + lane;
    int64_t last = -1;
    if (hi - lo == (int64_t)kLanes * U) {
      for (int h = 0; h < 2; ++h)
        for (int k = 0; k < H; ++k) {
          const int64_t i = base + (int64_t)(h * H + k) * kLanes;
          CHECK(i > last);  // (the order of accumulation over k: ascending, as without the staging)
          last = i;
          touch(i);
        }
    } else {
      for (int k = 0; k < U; ++k) {
        const int64_t i = base + (int64_t)k * kLanes;
        if (i < hi) touch(i);
      }
    }
  }
}
// k_isep_batch: the elements (absolute, within a vector of batch * ld elements) that the workgroup owning tiles [t0, t1) of
// problem b touches
template <class Mark>
static void walk_workgroup(Mark&& mark, int64_t n, int64_t b, int64_t ld, int base_odd, bool pairs, int64_t tiles, int64_t t0,
                           int64_t t1) {
  const int64_t off = b * ld;
  if (pairs) {
    const BatchRowMap r = batch_row_map(n, b, ld, base_odd);
    for (int64_t t = t0; t < t1; ++t)
      walk_tile(r.npairs, t, kPairsPerLane, [&](int64_t i) { mark(off + r.head + 2 * i); mark(off + r.head + 2 * i + 1); });
    if (t0 == 0 && r.head) mark(off);
    if (t1 == tiles && r.tail) mark(off + n - 1);
  } else {
    for (int64_t t = t0; t < t1; ++t) walk_tile(n, t, kElemsPerLane, [&](int64_t i) { mark(off + i); });
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
  if (n <= 700 || n % 74 == 0) return true;
  const int64_t half = kBatchTile / 2;
  const int64_t r = n % half;
  return r <= 9 || r >= half - 9;
}

// the tile intervals of a row: contiguous, in order, together [0, count), none longer than a tile -- every n, both parities
static void check_row_intervals(int64_t n) {
  const int64_t tiles = batch_tiles(n);
  CHECK(tiles == (n + kBatchTile - 1) / kBatchTile);
  for (int pairs = 0; pairs < 2; ++pairs) {
    for (int par = 0; par < 2; ++par) {
      const BatchRowMap r = batch_row_map(n, par, 1, 0);
      CHECK(r.head == (n > 0 ? par : 0) && r.head + 2 * r.npairs + r.tail == n && (r.tail == 0 || r.tail == 1) && r.npairs >= 0);
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
    }
  }
}

// Three rows of n elements with `pad` elements of padding each, all six vectors: the launch of the plan, workgroup by
// workgroup, touches every row element of every vector exactly once and no padding element.  The six vectors are walked with
// the one mapping the kernel applies to all of them (they share ld and, in the pairs form, their alignment).
static void check_batch_coverage(int64_t n, int64_t pad, int bits) {
  const int64_t batch = 3, ld = n + pad;
  const BatchPlan p = ibatch_plan(n, batch, ld, bits);
  CHECK(p.ok);
  if (n == 0) return;
  const int64_t tiles = p.tiles_per_problem, total = batch * ld;
  // one 8-bit counter per vector, packed: the kernel applies the one mapping to all six (IRow), so a touch counts in each
  constexpr uint64_t kOnce = 0x010101010101ull;
  std::vector<uint64_t> hits((size_t)total, 0);
  int64_t outside = 0;
  for (int64_t wg = 0; wg < p.grid; ++wg) {
    int64_t b = wg, t0 = 0, t1 = tiles;
    if (p.form == BatchForm::kTiled) { batch_workgroup(wg, tiles, &b, &t0); t1 = t0 + 1; }
    walk_workgroup([&](int64_t e) {
      if (e < 0 || e >= total) { ++outside; return; }
      hits[(size_t)e] += kOnce;
    }, n, b, ld, p.base_odd, p.pairs, tiles, t0, t1);
  }
  int64_t bad = 0;
  for (int64_t e = 0; e < total; ++e) bad += hits[(size_t)e] != ((e % ld) < n ? kOnce : 0);  // rows once, padding never
  CHECK(bad == 0 && outside == 0);
}

static void check_call(int64_t n, int64_t batch, int64_t ld, int bits, BatchForm form_of_n) {
  const BatchPlan p = ibatch_plan(n, batch, ld, bits);
  CHECK(p.ok);
  CHECK(p.form == form_of_n && (p.form == BatchForm::kRow) == (n <= kBatchRowMax));
  CHECK(p.pairs == (bits == 0 || bits == kIbatchAllOff) && p.base_odd == (bits == kIbatchAllOff ? 1 : 0));
  const int64_t tiles = p.tiles_per_problem;
  CHECK(tiles == batch_tiles(n));
  if (p.form == BatchForm::kRow) CHECK(p.grid == batch && p.ws_bytes == 0);
  else CHECK(p.grid == batch * tiles && p.ws_bytes == (size_t)batch * 4 * (size_t)tiles * sizeof(double));
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
  // workgroup -> (problem, tile): onto batch x tiles, one workgroup each; its four slots inside the workspace, no two alike
  const int64_t slots = (int64_t)(p.ws_bytes / sizeof(double));
  auto check_wg = [&](int64_t wg) {
    int64_t b, t;
    batch_workgroup(wg, tiles, &b, &t);
    CHECK(b >= 0 && b < batch && t >= 0 && t < tiles && b * tiles + t == wg);
    for (int pl = 0; pl < kIbatchPlanes; ++pl) {
      const int64_t s = ibatch_slot(b, pl, t, tiles);
      CHECK(s >= 0 && s < slots && s == (b * 4 + pl) * tiles + t);
    }
  };
  if (p.grid <= 64) {
    std::vector<unsigned char> seen((size_t)slots, 0);
    for (int64_t wg = 0; wg < p.grid; ++wg) {
      check_wg(wg);
      int64_t b, t;
      batch_workgroup(wg, tiles, &b, &t);
      for (int pl = 0; pl < kIbatchPlanes; ++pl) ++seen[(size_t)ibatch_slot(b, pl, t, tiles)];
    }
    // the reduce of problem b reads [ibatch_slot(b, 0, 0), + 4 tiles): every slot of the workspace, each written once
    int64_t bad = 0;
    for (int64_t b = 0; b < batch; ++b)
      for (int64_t k = 0; k < kIbatchPlanes * tiles; ++k) bad += seen[(size_t)(ibatch_slot(b, 0, 0, tiles) + k)] != 1;
    CHECK(bad == 0 && slots == batch * kIbatchPlanes * tiles);
  } else {
    const int64_t wgs[] = {0, 1, tiles - 1, tiles, p.grid / 2, p.grid - tiles, p.grid - 1};
    for (int64_t wg : wgs) check_wg(wg);
  }
  CHECK(ibatch_slot(batch - 1, kIbatchPlanes - 1, tiles - 1, tiles) == slots - 1 && ibatch_slot(0, 0, 0, tiles) == 0);
}

int main() {
  const int64_t batches[] = {0, 1, 2, 3, 255, 256, 257, 65535, 65536, 70001};
  const int aligns[] = {0, kIbatchAllOff, 1 << 5 /* xkn alone 8 bytes off: element-wise */, 1 << 2 /* d alone */};
  static_assert(kIbatchVectors == 6 && kIbatchPlanes == 4, "six vectors, four sums");
  check_tile_lanes();
  for (int64_t n = 0; n <= 2 * kBatchRowMax + 7; ++n) {
    check_row_intervals(n);
    if (lane_level(n))
      for (int64_t pad = 0; pad < 4; ++pad)
        for (int bits : {0, kIbatchAllOff, 1 << 5}) check_batch_coverage(n, pad, bits);
    const BatchForm form_of_n = ibatch_plan(n, 1, n, 0).form;
    for (int64_t batch : batches)
      for (int64_t pad = 0; pad < 4; ++pad)
        for (int bits : aligns) check_call(n, batch, n + pad, bits, form_of_n);
  }
  // more than 2^31 - 1 workgroups: refused, at the edge accepted
  CHECK(ibatch_plan(5, kBatchGridMax, 5, 0).ok && !ibatch_plan(5, kBatchGridMax + 1, 5, 0).ok);
  CHECK(!ibatch_plan(0, kBatchGridMax + 1, 0, 0).ok);
  {
    const int64_t n = kBatchRowMax + 1, tiles = batch_tiles(n);  // 5 tiles a problem
    CHECK(tiles == 5);
    const int64_t most = kBatchGridMax / tiles;
    const BatchPlan a = ibatch_plan(n, most, n, 0), b = ibatch_plan(n, most + 1, n, 0);
    CHECK(a.ok && a.grid == most * tiles && !b.ok);
    CHECK(!ibatch_plan(n, (int64_t)1 << 62, n, 0).ok);  // (no overflow on the way to the refusal)
  }
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
