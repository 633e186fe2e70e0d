/* Stand-alone driver for the device-free plan of the batched separable calls (csrc/spx_plan.hpp: batch_plan, batch_row_map,
 * batch_tiles, batch_tile_units, batch_workgroup, batch_slot) -- the functions the kernel body and the reduce of
 * spx_batch_device.hpp walk a row with.  `batch_plan_driver prox` checks the batched prox! (five vectors y, q, xk, sj, xkn, three
 * planes, a full tile's loads in one stage), `batch_plan_driver iprox` the batched iprox! (six vectors y, g, d, xk, sj, xkn,
 * four planes, two stages).  The walk of a workgroup is restated here lane by lane, in the stages of batch_tile, and marks
 * the elements it touches in each of the kind's vectors (the kernel applies the one mapping to all of them: BatchRow).
 * Over n = 0 ... 2 kBatchRowMax + 7, batch in {0, 1, 2, 3, 255, 256, 257, 65535, 65536, 70001}, ld - n in {0, 1, 2, 3}, the bases
 * all on a 16-byte boundary, all 8 bytes off it, and mixed (the element-wise form: xkn alone off, iprox also d alone):
 *   - every element of every row of every vector is touched exactly once, whichever parity the row starts at, and nothing
 *     outside [0, n) of a row is, no padding element [b ld + n, (b + 1) ld) either.  For EVERY n this is shown in two steps:
 *     the tiles' unit intervals partition [0, count) in order (check_row_intervals), and the lanes of a workgroup touch every
 *     unit of an interval [lo, hi) exactly once.  The second step depends on hi - lo alone and is checked for EVERY length
 *     0 ... a full tile, in both forms, on tile 0 and on tile 1 (check_tile_lanes).  The lane-by-lane walks on top of that are
 *     SAMPLED, not run for every n (n <= 700, n within 9 of every multiple of half a tile, every 37th n): one row at either
 *     parity walked by the row form and by the tiled form (check_row_coverage), and a batch of three rows with its padding
 *     walked workgroup by workgroup as the plan launches it (check_batch_coverage).  The walk restates batch_tile's loop here
 *     (the kernel's own loop carries device loads and stores); what it shares with the kernel is the mapping functions of
 *     spx_plan.hpp;
 *   - a lane visits its units in the order k = 0 .. U - 1 whether a tile is staged whole or in groups;
 *   - a row's pairs start on a 16-byte boundary, rows stay inside [b ld, b ld + n), i.e. clear of the padding;
 *   - workgroup -> (problem, tile) is a bijection onto batch x tiles;
 *   - ws_bytes holds exactly the slots the reduce reads, each written by one workgroup;
 *   - the form depends on n only; a grid beyond 2^31 - 1 workgroups is refused.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_batch_plan_host.py and tests/test_ibatch_plan_host.py; it has its own main, the library is not loaded, no HIP call
 * is made. */
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
static BatchKind g_kind;  // the vectors and planes of the call under test
static int g_stages;      // Kind::kStages of its batch_tile

// batch_tile: the units lane `lane` of the workgroup touches in tile `tile` of `count` units, in the lane's own order -- a full
// tile in g_stages groups of U / g_stages units, the last tile of a row unit by unit
template <class Touch>
static void walk_tile(int64_t count, int64_t tile, int U, Touch&& touch) {
  int64_t lo, hi;
  batch_tile_units(count, tile, kLanes * U, &lo, &hi);
  const int H = U / g_stages;
  for (int lane = 0; lane < kLanes; ++lane) {
    const int64_t base = lo + lane;
    int64_t last = -1;
    if (hi - lo == (int64_t)kLanes * U) {
      for (int h = 0; h < g_stages; ++h)
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
// batch_body: the elements (absolute, within a vector of batch * ld elements) that the workgroup owning tiles [t0, t1) of
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
    CHECK(U % g_stages == 0);
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

// one row of n elements that starts at parity `par` (b = par, ld = 1 puts it there), walked by the row form (one workgroup)
// and by the tiled form (one workgroup per tile), whichever the plan would choose at this n
static void check_row_coverage(int64_t n) {
  const int64_t tiles = batch_tiles(n);
  for (int pairs = 0; pairs < 2; ++pairs)
    for (int par = 0; par < 2; ++par)
      for (int tiled = 0; tiled < 2; ++tiled) {
        std::vector<unsigned char> hits((size_t)n, 0);
        int64_t outside = 0;
        auto mark = [&](int64_t e) { if (e < par || e >= par + n) ++outside; else ++hits[(size_t)(e - par)]; };
        if (!tiled) walk_workgroup(mark, n, par, 1, 0, pairs != 0, tiles, 0, tiles);
        else for (int64_t t = 0; t < tiles; ++t) walk_workgroup(mark, n, par, 1, 0, pairs != 0, tiles, t, t + 1);
        int64_t bad = 0;
        for (int64_t e = 0; e < n; ++e) bad += hits[(size_t)e] != 1;
        CHECK(bad == 0 && outside == 0);
      }
}

// Three rows of n elements with `pad` elements of padding each, all the kind's vectors: the launch of the plan, workgroup by
// workgroup, touches every row element of every vector exactly once and no padding element.  The vectors are walked with
// the one mapping the kernel applies to all of them (they share ld and, in the pairs form, their alignment).
static void check_batch_coverage(int64_t n, int64_t pad, int bits) {
  const int64_t batch = 3, ld = n + pad;
  const BatchPlan p = batch_plan(n, batch, ld, bits, g_kind);
  CHECK(p.ok);
  if (n == 0) return;
  const int64_t tiles = p.tiles_per_problem, total = batch * ld;
  // one 8-bit counter per vector, packed: a touch counts in each
  uint64_t once = 0;
  for (int v = 0; v < g_kind.vectors; ++v) once |= (uint64_t)1 << (8 * v);
  std::vector<uint64_t> hits((size_t)total, 0);
  int64_t outside = 0;
  for (int64_t wg = 0; wg < p.grid; ++wg) {
    int64_t b = wg, t0 = 0, t1 = tiles;
    if (p.form == BatchForm::kTiled) { batch_workgroup(wg, tiles, &b, &t0); t1 = t0 + 1; }
    walk_workgroup([&](int64_t e) {
      if (e < 0 || e >= total) { ++outside; return; }
      hits[(size_t)e] += once;
    }, n, b, ld, p.base_odd, p.pairs, tiles, t0, t1);
  }
  int64_t bad = 0;
  for (int64_t e = 0; e < total; ++e) bad += hits[(size_t)e] != ((e % ld) < n ? once : 0);  // rows once, padding never
  CHECK(bad == 0 && outside == 0);
}

static void check_call(int64_t n, int64_t batch, int64_t ld, int bits, BatchForm form_of_n) {
  const int planes = g_kind.planes, all_off = g_kind.all_off();
  const BatchPlan p = batch_plan(n, batch, ld, bits, g_kind);
  CHECK(p.ok);
  CHECK(p.form == form_of_n && (p.form == BatchForm::kRow) == (n <= kBatchRowMax));
  CHECK(p.pairs == (bits == 0 || bits == all_off) && p.base_odd == (bits == all_off ? 1 : 0));
  const int64_t tiles = p.tiles_per_problem;
  CHECK(tiles == batch_tiles(n));
  if (p.form == BatchForm::kRow) CHECK(p.grid == batch && p.ws_bytes == 0);
  else CHECK(p.grid == batch * tiles && p.ws_bytes == (size_t)batch * planes * (size_t)tiles * sizeof(double));
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
  // workgroup -> (problem, tile): onto batch x tiles, one workgroup each; its slots inside the workspace, no two alike
  const int64_t slots = (int64_t)(p.ws_bytes / sizeof(double));
  auto check_wg = [&](int64_t wg) {
    int64_t b, t;
    batch_workgroup(wg, tiles, &b, &t);
    CHECK(b >= 0 && b < batch && t >= 0 && t < tiles && b * tiles + t == wg);
    for (int pl = 0; pl < planes; ++pl) {
      const int64_t s = batch_slot(b, pl, t, tiles, planes);
      CHECK(s >= 0 && s < slots && s == (b * planes + pl) * tiles + t);
    }
  };
  if (p.grid <= 64) {
    std::vector<unsigned char> seen((size_t)slots, 0);
    for (int64_t wg = 0; wg < p.grid; ++wg) {
      check_wg(wg);
      int64_t b, t;
      batch_workgroup(wg, tiles, &b, &t);
      for (int pl = 0; pl < planes; ++pl) ++seen[(size_t)batch_slot(b, pl, t, tiles, planes)];
    }
    // the reduce of problem b reads [batch_slot(b, 0, 0), + planes tiles): every slot of the workspace, each written once
    int64_t bad = 0;
    for (int64_t b = 0; b < batch; ++b)
      for (int64_t k = 0; k < planes * tiles; ++k) bad += seen[(size_t)(batch_slot(b, 0, 0, tiles, planes) + k)] != 1;
    CHECK(bad == 0 && slots == batch * planes * tiles);
  } else {
    const int64_t wgs[] = {0, 1, tiles - 1, tiles, p.grid / 2, p.grid - tiles, p.grid - 1};
    for (int64_t wg : wgs) check_wg(wg);
  }
  CHECK(batch_slot(batch - 1, planes - 1, tiles - 1, tiles, planes) == slots - 1 && batch_slot(0, 0, 0, tiles, planes) == 0);
}

int main(int argc, char** argv) {
  const bool iprox = argc == 2 && !strcmp(argv[1], "iprox");
  if (!iprox && !(argc == 2 && !strcmp(argv[1], "prox"))) { printf("usage: %s prox|iprox\n", argv[0]); return 2; }
  g_kind = iprox ? kBatchIprox : kBatchProx;
  g_stages = iprox ? 2 : 1;
  CHECK(g_kind.vectors == (iprox ? 6 : 5) && g_kind.planes == (iprox ? 4 : 3));
  const int64_t batches[] = {0, 1, 2, 3, 255, 256, 257, 65535, 65536, 70001};
  const int xkn_off = 1 << (g_kind.vectors - 1);  // xkn alone 8 bytes off: element-wise
  std::vector<int> aligns = {0, g_kind.all_off(), xkn_off};
  if (iprox) aligns.push_back(1 << 2);  // d alone
  check_tile_lanes();
  for (int64_t n = 0; n <= 2 * kBatchRowMax + 7; ++n) {
    check_row_intervals(n);
    if (lane_level(n)) {
      check_row_coverage(n);
      for (int64_t pad = 0; pad < 4; ++pad)
        for (int bits : {0, g_kind.all_off(), xkn_off}) check_batch_coverage(n, pad, bits);
    }
    const BatchForm form_of_n = batch_plan(n, 1, n, 0, g_kind).form;
    for (int64_t batch : batches)
      for (int64_t pad = 0; pad < 4; ++pad)
        for (int bits : aligns) check_call(n, batch, n + pad, bits, form_of_n);
  }
  // more than 2^31 - 1 workgroups: refused, at the edge accepted
  CHECK(batch_plan(5, kBatchGridMax, 5, 0, g_kind).ok && !batch_plan(5, kBatchGridMax + 1, 5, 0, g_kind).ok);
  CHECK(!batch_plan(0, kBatchGridMax + 1, 0, 0, g_kind).ok);
  {
    const int64_t n = kBatchRowMax + 1, tiles = batch_tiles(n);  // 5 tiles a problem
    CHECK(tiles == 5);
    const int64_t most = kBatchGridMax / tiles;
    const BatchPlan a = batch_plan(n, most, n, 0, g_kind), b = batch_plan(n, most + 1, n, 0, g_kind);
    CHECK(a.ok && a.grid == most * tiles && !b.ok);
    CHECK(!batch_plan(n, (int64_t)1 << 62, n, 0, g_kind).ok);  // (no overflow on the way to the refusal)
  }
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
