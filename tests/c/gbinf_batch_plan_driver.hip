/* Stand-alone driver for the device-free plan of the batched Binf group call (csrc/spx_plan.hpp: gbatch_plan with the lanes
 * per group of the size's row of GroupTilesBinf, and the bit walk of the second phase: binf_bitmap_words, binf_walk_passes,
 * binf_walk_bit, kBinfWalkWaves, kBinfBitmapWords) -- the functions k_binf_batch of csrc/spx_gbinf_batch.hip finds its groups
 * and its literal groups with.  Over group_size = 1 .. 512, with ngroups around the multiples of 4 (64 / LPG), around the
 * row / tiled boundary and around the multiples of a tile's run:
 *   - every group belongs to exactly one (problem, tile); tiles hold whole groups;
 *   - the bitmap index of a group inside its workgroup stays below the bitmap's capacity (kBinfBitmapWords words);
 *   - the second phase's assignment of set bits to (wave, pass, slot), restated here as the kernel walks it, visits every set
 *     bit exactly once, no clear bit, and in ascending group order per wave -- for empty, full, single-bit, alternating and
 *     pseudo-random bitmaps, at the slots per pass of the size's row of GroupTilesLit;
 *   - the form, the run and the tiles depend on (group_size, ngroups) only;
 *   - a grid beyond 2^31 - 1 workgroups is refused, at the edge accepted.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_gbinf_batch_plan_host.py; it has its own main, the library is not loaded, no HIP call is made. */
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

// the main phase of k_binf_batch: the local groups [0, ng) wave by wave, wave tile by wave tile, slot by slot
template <class Touch>
static void walk_main(int ng, int gpw, Touch&& touch) {
  for (int w = 0; w < 4; ++w)
    for (int l0 = w * gpw; l0 < ng; l0 += 4 * gpw)
      for (int slot = 0; slot < gpw; ++slot)
        if (l0 + slot < ng) touch(l0 + slot);
}

// the literal phase of k_binf_batch over a bitmap of `ng` groups: visit(wave, local group) in the order a wave meets them
template <class Visit>
static void walk_literal(const std::vector<unsigned long long>& bitmap, int ng, int slots, Visit&& visit) {
  const int nwords = binf_bitmap_words(ng);
  for (int w = 0; w < kBinfWalkWaves; ++w)
    for (int wi = w; wi < nwords; wi += kBinfWalkWaves) {
      const unsigned long long word = bitmap[(size_t)wi];
      const int passes = binf_walk_passes(word, slots);
      for (int p = 0; p < passes; ++p)
        for (int slot = 0; slot < slots; ++slot) {
          const int bit = binf_walk_bit(word, slots, p, slot);
          if (bit >= 0) visit(w, wi * 64 + bit);
        }
      // nothing is left behind the last pass
      CHECK(binf_walk_bit(word, slots, passes, 0) == -1);
      if (word != 0ull) CHECK(passes >= 1 && binf_walk_bit(word, slots, passes - 1, 0) >= 0);
    }
}

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned long long next_random() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return g_rng;
}

// one bitmap: every set bit once, no clear bit, ascending per wave
static void check_walk(const std::vector<unsigned long long>& bitmap, int ng, int slots) {
  std::vector<unsigned char> hits((size_t)ng, 0);
  int last[kBinfWalkWaves];
  for (int w = 0; w < kBinfWalkWaves; ++w) last[w] = -1;
  long outside = 0, unordered = 0;
  walk_literal(bitmap, ng, slots, [&](int w, int lg) {
    if (lg < 0 || lg >= ng) { ++outside; return; }
    ++hits[(size_t)lg];
    if (lg <= last[w]) ++unordered;
    last[w] = lg;
  });
  long bad = 0;
  for (int g = 0; g < ng; ++g) bad += hits[(size_t)g] != (unsigned char)((bitmap[(size_t)(g >> 6)] >> (g & 63)) & 1ull);
  CHECK(bad == 0 && outside == 0 && unordered == 0);
}

static void check_bitmaps(int ng, int slots) {
  const int nwords = binf_bitmap_words(ng);
  CHECK(nwords >= 1 && nwords <= kBinfBitmapWords && (int64_t)nwords * 64 >= ng && (int64_t)(nwords - 1) * 64 < ng);
  auto fill = [&](auto&& bit_of) {
    std::vector<unsigned long long> bm((size_t)nwords, 0ull);
    for (int g = 0; g < ng; ++g)
      if (bit_of(g)) bm[(size_t)(g >> 6)] |= 1ull << (g & 63);
    return bm;
  };
  check_walk(fill([](int) { return false; }), ng, slots);                // empty
  check_walk(fill([](int) { return true; }), ng, slots);                 // full
  check_walk(fill([](int g) { return (g & 1) == 0; }), ng, slots);       // alternating
  check_walk(fill([](int g) { return (g & 1) == 1; }), ng, slots);
  for (int g : {0, 31, 32, 63, 64, ng / 2, ng - 1})                      // a single bit (31 / 32: the halves of a word)
    if (g >= 0 && g < ng) check_walk(fill([g](int h) { return h == g; }), ng, slots);
  for (int rep = 0; rep < 2; ++rep) {
    const unsigned long long thin = rep ? 15ull : 1ull;                  // about 1/2 and 1/16 of the bits
    check_walk(fill([&](int) { return (next_random() & thin) == 0ull; }), ng, slots);
  }
}

// every group of every problem in exactly one (problem, tile), once; its bitmap index below the capacity
static void check_groups(int64_t gs, int lpg, int64_t ngroups, int64_t batch, const GBatchPlan& p, int lit_slots) {
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
    }
    const int64_t ng = hi - lo;
    CHECK(ng >= 1 && ng <= kBatchRowMax && binf_bitmap_words(ng) <= kBinfBitmapWords);   // the bitmap holds the workgroup's groups
    CHECK((ng - 1) >> 6 < kBinfBitmapWords);
    CHECK(ng * gs <= INT32_MAX);                                                         // a lane's 32-bit element offset
    walk_main((int)ng, gpw, [&](int lg) {
      const int64_t g = lo + lg;
      if (g < lo || g >= hi) ++outside; else ++hits[(size_t)(b * ngroups + g)];
    });
    if (wg == 0 || wg == p.grid - 1) check_bitmaps((int)ng, lit_slots);
  }
  int64_t bad = 0;
  for (size_t i = 0; i < hits.size(); ++i) bad += hits[i] != 1;
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
    CHECK(p.run == gbatch_run(gs, lpg) && p.run % quad == 0 && p.run >= quad && p.run <= kBatchRowMax);
    CHECK(p.tiles_per_problem == (ngroups + p.run - 1) / p.run && p.tiles_per_problem >= 2);
    CHECK(p.grid == batch * p.tiles_per_problem);
    CHECK(p.ws_bytes == (size_t)batch * kGBatchPlanes * (size_t)p.tiles_per_problem * sizeof(double));
  }
  CHECK(p.grid <= kBatchGridMax);
}

int main() {
  const int64_t batches[] = {0, 1, 2, 3, 7, 256, 65536, 70001};
  const int aligns[] = {0, 1 << 4, 1, 31};  // all on a boundary; xkn alone off; y alone off; all off
  CHECK(kBinfBitmapWords * 64 == kBatchRowMax && kBinfWalkWaves == 4);
  for (int64_t gs = 1; gs <= kGroupRegMax; ++gs) {
    const int lpg = GroupTilesBinf::lpg(gs), lit_lpg = GroupTilesLit::lpg(gs);
    CHECK(lpg > 0 && lit_lpg > 0 && 64 % lpg == 0 && 64 % lit_lpg == 0);
    const int lit_slots = 64 / lit_lpg;
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
        check_groups(gs, lpg, ngroups, 3, p3, lit_slots);
      }
    }
  }
  // single words, every slot count of GroupTilesLit: the k-th set bit, pass by pass
  for (int slots : {2, 4, 8, 16}) {
    const unsigned long long words[] = {0ull, 1ull, 1ull << 31, 1ull << 32, 1ull << 63, 0x80000000ull, 0xFFFFFFFFull, 0xFFFFFFFF00000000ull,
                                        0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull, ~0ull, next_random(), next_random() & next_random()};
    for (unsigned long long word : words) {
      const int bits = __builtin_popcountll(word);
      CHECK(binf_walk_passes(word, slots) == (bits + slots - 1) / slots);
      int seen = 0, prev = -1;
      for (int p = 0; p < binf_walk_passes(word, slots); ++p)
        for (int s = 0; s < slots; ++s) {
          const int bit = binf_walk_bit(word, slots, p, s);
          if (p * slots + s < bits) { CHECK(bit > prev && bit < 64 && ((word >> bit) & 1ull)); prev = bit; ++seen; }
          else CHECK(bit == -1);
        }
      CHECK(seen == bits);
    }
  }
  // more than 2^31 - 1 workgroups: refused, at the edge accepted
  CHECK(gbatch_plan(8, 1, 4, kBatchGridMax, 32, 0).ok && !gbatch_plan(8, 1, 4, kBatchGridMax + 1, 32, 0).ok);
  CHECK(!gbatch_plan(8, 1, 0, kBatchGridMax + 1, 0, 0).ok);
  {
    const int64_t gs = 8, ngroups = kBatchRowMax / gs + 1;  // just tiled: runs of 256 groups on the one-lane tile
    const GBatchPlan one = gbatch_plan(gs, 1, ngroups, 1, ngroups * gs, 0);
    CHECK(one.form == BatchForm::kTiled && one.run == 256 && one.tiles_per_problem == 7);
    const int64_t most = kBatchGridMax / one.tiles_per_problem;
    const GBatchPlan a = gbatch_plan(gs, 1, ngroups, most, ngroups * gs, 0), b = gbatch_plan(gs, 1, ngroups, most + 1, ngroups * gs, 0);
    CHECK(a.ok && a.grid == most * one.tiles_per_problem && !b.ok);
    CHECK(!gbatch_plan(gs, 1, ngroups, (int64_t)1 << 62, ngroups * gs, 0).ok);  // (no overflow on the way to the refusal)
  }
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
