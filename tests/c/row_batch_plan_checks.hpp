/* The checks on row_batch_plan (csrc/spx_plan.hpp) that hold for every row-owner batched call, over a grid of n, batch, ld and
 * alignment bits, for the shape the driver passes (kB2BatchShape: b2_batch_plan_driver.hip; kToprBatchShape:
 * topr_batch_plan_driver.hip) --
 *   - the lane slots of the plan's workgroup, walked as the kernels walk them (row_batch_unit, row_batch_units), visit every
 *     element of a row exactly once and nothing beyond it;
 *   - a resident tile holds the row, and the tile before it would not; the form, the tile and the lanes depend on n alone,
 *     pairs on (n >= 2, the parity of ld, the alignment bits of y, q, xk, sj) alone, xkn_pairs on xkn's bit besides;
 *   - n = n_max and batch = 2^31 - 1 are accepted, one more of either is refused, each with its own reason.
 * Included behind the driver's CHECK macro. */
#pragma once
#include <stdint.h>

#include <vector>

#include "spx_plan.hpp"

// every (lane, slot) of the plan's workgroup -> its unit -> the elements of the row it covers
static void check_cover(const RowBatchShape& s, int64_t n, const RowBatchPlan& p, std::vector<unsigned char>& seen) {
  const int E = p.pairs ? 2 : 1;
  const int64_t utot = row_batch_units(n, p.pairs);
  int64_t slots;
  if (p.form == RowBatchForm::kResident) {
    slots = p.epl / E;
  } else {  // the row walk: whole rounds of walk_unroll units per lane until the row is covered
    const int64_t round = (int64_t)p.lanes * s.walk_unroll;
    slots = (utot + round - 1) / round * s.walk_unroll;
  }
  seen.assign((size_t)n, 0);
  long beyond = 0, twice = 0;
  for (int t = 0; t < p.lanes; ++t)
    for (int64_t k = 0; k < slots; ++k) {
      const int64_t u = row_batch_unit(k, p.lanes, t);
      if (u >= utot) continue;  // an idle slot
      for (int e = 0; e < E; ++e) {
        const int64_t i = u * E + e;
        if (i >= n) { if (!(p.pairs && e == 1 && i == n)) ++beyond; continue; }  // (the missing half of an odd row's last unit)
        if (seen[(size_t)i]++) ++twice;
      }
    }
  long missed = 0;
  for (int64_t i = 0; i < n; ++i) missed += seen[(size_t)i] == 0;
  CHECK(beyond == 0);
  CHECK(twice == 0);
  CHECK(missed == 0);
}

static void run_row_batch_plan_checks(const RowBatchShape& s) {
  std::vector<int64_t> ns = {0, 1, 2, 3, 7, 63, 64, 65, 1000, 5000, 10000, 12289, 100000, 1000003};
  for (int i = 0; i < s.tile_count; ++i) {
    const int64_t cap = (int64_t)s.tiles[i].lanes * s.tiles[i].epl;
    for (int64_t d = -2; d <= 2; ++d) ns.push_back(cap + d);
  }
  for (int64_t d = -1; d <= 2; ++d) ns.push_back(s.row_max + d);
  ns.push_back(2 * s.row_max + 3);
  for (int64_t d = -2; d <= 0; ++d) ns.push_back(s.n_max + d);
  for (int64_t m = 1; m <= 3; ++m)  // around whole rounds of the row walk
    for (int64_t d = -1; d <= 1; ++d) ns.push_back(4 * m * s.walk_lanes * s.walk_unroll + d);
  const int64_t batches[] = {1, 2, 3, 7, 256, 70001, kBatchGridMax};
  const int64_t pads[] = {0, 1, 2, 5};
  std::vector<unsigned char> seen;
  for (int64_t n : ns) {
    const RowBatchPlan ref = row_batch_plan(s, n, 1, n, 0);
    CHECK(ref.ok);
    for (int64_t batch : batches)
      for (int64_t pad : pads)
        for (int bits = 0; bits < 32; ++bits) {  // all 32 alignment classes; pads 1 and 5 give odd ld for even n and the reverse
          const int64_t ld = n + pad;
          const RowBatchPlan p = row_batch_plan(s, n, batch, ld, bits);
          CHECK(p.ok && p.why == RowBatchRefusal::kNone);
          CHECK(p.grid == batch);
          // the form is a function of n alone (not of batch, ld or the alignment), pairs of the alignment class
          CHECK(p.form == ref.form && p.tile == ref.tile && p.lanes == ref.lanes && p.epl == ref.epl);
          CHECK(p.pairs == ((bits & 15) == 0 && (ld & 1) == 0 && n >= 2));
          CHECK(p.xkn_pairs == (p.pairs && (bits & 16) == 0));
          CHECK((p.form == RowBatchForm::kResident) == (n <= s.row_max));
          if (p.form == RowBatchForm::kResident) {
            CHECK(p.tile >= 0 && p.tile < s.tile_count);
            CHECK(p.lanes == s.tiles[p.tile].lanes && p.epl == s.tiles[p.tile].epl);
            CHECK((int64_t)p.lanes * p.epl >= n);
            if (p.tile > 0) CHECK((int64_t)s.tiles[p.tile - 1].lanes * s.tiles[p.tile - 1].epl < n);
            CHECK(p.epl % 2 == 0 && p.lanes % 64 == 0 && p.lanes <= 1024);
          } else {
            CHECK(p.lanes == s.walk_lanes && p.tile == -1 && p.epl == 0);
          }
        }
    // the cover, once per alignment class (it does not depend on batch)
    for (int cls = 0; cls < 2; ++cls) {
      const RowBatchPlan p = row_batch_plan(s, n, 3, n + (n & 1), cls ? 1 : 0);
      CHECK(p.pairs == (cls == 0 && n >= 2));
      check_cover(s, n, p, seen);
    }
  }
  // the tiles: a row of 1e3 does not take a CU-wide workgroup, the largest tile is the resident bound
  CHECK(row_batch_plan(s, 1000, 1, 1000, 0).lanes == 256 && row_batch_plan(s, 256, 1, 256, 0).lanes == 64);
  CHECK((int64_t)s.tiles[s.tile_count - 1].lanes * s.tiles[s.tile_count - 1].epl == s.row_max);
  CHECK(row_batch_plan(s, 8192, 9, 8192, 0).form == RowBatchForm::kResident && row_batch_plan(s, 8193, 9, 8194, 0).form == RowBatchForm::kWalk);
  // the bounds
  CHECK(s.n_max == ((int64_t)1 << 20) && s.row_max == 8192);
  CHECK(row_batch_plan(s, s.n_max, kBatchGridMax, s.n_max, 0).ok);
  {
    const RowBatchPlan p = row_batch_plan(s, s.n_max + 1, 1, s.n_max + 1, 0);
    CHECK(!p.ok && p.why == RowBatchRefusal::kNTooLarge);
    const RowBatchPlan g = row_batch_plan(s, 5, kBatchGridMax + 1, 5, 0);
    CHECK(!g.ok && g.why == RowBatchRefusal::kBatchTooLarge);
    const RowBatchPlan h = row_batch_plan(s, INT64_MAX, INT64_MAX, INT64_MAX, 31);
    CHECK(!h.ok);
  }
}
