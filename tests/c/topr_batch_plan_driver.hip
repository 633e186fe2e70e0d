/* Stand-alone driver for the device-free parts of the batched top-r calls (spx_proxstep_indball_l0[_binf]_batch):
 *   (a) topr_batch_plan (csrc/spx_plan.hpp) over a grid of n, batch, ld and alignment bits --
 *     - the lane slots of the plan's workgroup, walked as k_topr_batch of csrc/spx_topr_batch.hip walks them (topr_batch_unit,
 *       topr_batch_units), visit every element of a row exactly once and nothing beyond it;
 *     - a resident tile holds the row, and the tile before it would not; the form, the tile and the lanes depend on n alone,
 *       pairs on (n >= 2, the parity of ld, the alignment bits of y, q, xk, sj) alone, xkn_pairs on xkn's bit besides;
 *     - n = kToprBatchNMax and batch = 2^31 - 1 are accepted, one more of either is refused, each with its own reason.
 *   (b) the selection of csrc/spx_topr_row.hpp (topr_key, topr_row_begin, topr_row_digit, topr_row_step, topr_row_keep) on host
 *     arrays, every histogram a plain loop: the kept set against a STABLE descending sort by |v| (NaN above Inf, all NaNs equal),
 *     for every r in {-1, 0, 1, ..., n, n + 1}, on random values, a constant with alternating sign, a 2^-8 lattice, values over
 *     2^+-500, two keys that differ in the last bit with the cut between them, NaNs and +-Inf mixed in, and all zeros.
 *     Prints "n N key_passes K index_passes I" with the maxima per size.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_topr_batch_plan_host.py; it has its own main, the library is not loaded, no HIP call is made. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "spx_plan.hpp"
#include "spx_topr_row.hpp"

static long g_checked = 0;
static int g_fail = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++g_checked;                                                                               \
    if (!(cond)) { if (g_fail < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

// ---- (a) the plan -------------------------------------------------------------------------------
// every (lane, slot) of the plan's workgroup -> its unit -> the elements of the row it covers
static void check_cover(int64_t n, const ToprBatchPlan& p, std::vector<unsigned char>& seen) {
  const int E = p.pairs ? 2 : 1;
  const int64_t utot = topr_batch_units(n, p.pairs);
  int64_t slots;
  if (p.form == ToprBatchForm::kResident) {
    slots = p.epl / E;
  } else {  // the row walk: whole rounds of kToprBatchWalkUnroll units per lane until the row is covered
    const int64_t round = (int64_t)p.lanes * kToprBatchWalkUnroll;
    slots = (utot + round - 1) / round * kToprBatchWalkUnroll;
  }
  seen.assign((size_t)n, 0);
  long beyond = 0, twice = 0;
  for (int t = 0; t < p.lanes; ++t)
    for (int64_t k = 0; k < slots; ++k) {
      const int64_t u = topr_batch_unit(k, p.lanes, t);
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

static void run_plan_checks() {
  std::vector<int64_t> ns = {0, 1, 2, 3, 7, 63, 64, 65, 1000, 5000, 10000, 100000, 1000003};
  for (int i = 0; i < kToprBatchTileCount; ++i) {
    const int64_t cap = (int64_t)kToprBatchTiles[i].lanes * kToprBatchTiles[i].epl;
    for (int64_t d = -1; d <= 1; ++d) ns.push_back(cap + d);
  }
  for (int64_t d = -1; d <= 2; ++d) ns.push_back(kToprBatchRowMax + d);
  ns.push_back(2 * kToprBatchRowMax + 3);
  for (int64_t d = -2; d <= 0; ++d) ns.push_back(kToprBatchNMax + d);
  for (int64_t m = 1; m <= 3; ++m)  // around whole rounds of the row walk
    for (int64_t d = -1; d <= 1; ++d) ns.push_back(4 * m * kToprBatchWalkLanes * kToprBatchWalkUnroll + d);
  const int64_t batches[] = {1, 2, 3, 7, 256, 70001, kBatchGridMax};
  const int64_t pads[] = {0, 1, 2, 5};
  std::vector<unsigned char> seen;
  for (int64_t n : ns) {
    const ToprBatchPlan ref = topr_batch_plan(n, 1, n, 0);
    CHECK(ref.ok);
    for (int64_t batch : batches)
      for (int64_t pad : pads)
        for (int bits = 0; bits < 32; ++bits) {  // all 32 alignment classes; pads 1 and 5 give odd ld for even n and the reverse
          const int64_t ld = n + pad;
          const ToprBatchPlan p = topr_batch_plan(n, batch, ld, bits);
          CHECK(p.ok && p.why == ToprBatchRefusal::kNone);
          CHECK(p.grid == batch);
          // the form is a function of n alone (not of batch, ld or the alignment), pairs of the alignment class
          CHECK(p.form == ref.form && p.tile == ref.tile && p.lanes == ref.lanes && p.epl == ref.epl);
          CHECK(p.pairs == ((bits & 15) == 0 && (ld & 1) == 0 && n >= 2));
          CHECK(p.xkn_pairs == (p.pairs && (bits & 16) == 0));
          CHECK((p.form == ToprBatchForm::kResident) == (n <= kToprBatchRowMax));
          if (p.form == ToprBatchForm::kResident) {
            CHECK(p.tile >= 0 && p.tile < kToprBatchTileCount);
            CHECK(p.lanes == kToprBatchTiles[p.tile].lanes && p.epl == kToprBatchTiles[p.tile].epl);
            CHECK((int64_t)p.lanes * p.epl >= n);
            if (p.tile > 0) CHECK((int64_t)kToprBatchTiles[p.tile - 1].lanes * kToprBatchTiles[p.tile - 1].epl < n);
            CHECK(p.epl % 2 == 0 && p.lanes % 64 == 0 && p.lanes <= 1024);
          } else {
            CHECK(p.lanes == kToprBatchWalkLanes && p.tile == -1 && p.epl == 0);
          }
        }
    // the cover, once per alignment class (it does not depend on batch)
    for (int cls = 0; cls < 2; ++cls) {
      const ToprBatchPlan p = topr_batch_plan(n, 3, n + (n & 1), cls ? 1 : 0);
      CHECK(p.pairs == (cls == 0 && n >= 2));
      check_cover(n, p, seen);
    }
  }
  // the tiles: a row of 1e3 does not take a CU-wide workgroup, the largest tile is the resident bound
  CHECK(topr_batch_plan(1000, 1, 1000, 0).lanes == 256 && topr_batch_plan(256, 1, 256, 0).lanes == 64);
  CHECK((int64_t)kToprBatchTiles[kToprBatchTileCount - 1].lanes * kToprBatchTiles[kToprBatchTileCount - 1].epl == kToprBatchRowMax);
  CHECK(topr_batch_plan(8192, 9, 8192, 0).form == ToprBatchForm::kResident && topr_batch_plan(8193, 9, 8194, 0).form == ToprBatchForm::kWalk);
  // the bounds
  CHECK(kToprBatchNMax == ((int64_t)1 << 20) && kToprBatchRowMax == 8192);
  CHECK(topr_batch_plan(kToprBatchNMax, kBatchGridMax, kToprBatchNMax, 0).ok);
  {
    const ToprBatchPlan p = topr_batch_plan(kToprBatchNMax + 1, 1, kToprBatchNMax + 1, 0);
    CHECK(!p.ok && p.why == ToprBatchRefusal::kNTooLarge);
    const ToprBatchPlan g = topr_batch_plan(5, kBatchGridMax + 1, 5, 0);
    CHECK(!g.ok && g.why == ToprBatchRefusal::kBatchTooLarge);
    const ToprBatchPlan h = topr_batch_plan(INT64_MAX, INT64_MAX, INT64_MAX, 31);
    CHECK(!h.ok);
  }
}

// ---- (b) the selection -------------------------------------------------------------------------------
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() {  // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return g_rng * 0x2545f4914f6cdd1dull;
}
static double rnd_unit() { return (double)(rnd64() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }
static double from_bits(uint64_t b) { double v; memcpy(&v, &b, sizeof v); return v; }

enum Kind { kRandom, kConstant, kLattice, kWide, kLastBit, kNonFinite, kZeros, kKinds };
static const char* const kKindNames[kKinds] = {"random", "constant", "lattice", "wide", "lastbit", "nonfinite", "zeros"};

static std::vector<double> make_row(Kind kind, int64_t n) {
  std::vector<double> v((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    double x = 0.0;
    switch (kind) {
      case kRandom: x = rnd_unit(); break;
      case kConstant: x = (i & 1) ? -0.75 : 0.75; break;                                    // one key: the index decides
      case kLattice: x = (double)((int64_t)(rnd64() % 33) - 16) * (1.0 / 256.0); break;       // 17 keys, zeros among them
      case kWide: x = ldexp(rnd_unit(), (int)(rnd64() % 1001) - 500); break;                 // the whole exponent range
      case kLastBit: x = from_bits(0x3ff0000000000000ull + (rnd64() & 1)) * ((rnd64() & 2) ? -1.0 : 1.0); break;  // two adjacent keys
      case kNonFinite: {
        const unsigned m = (unsigned)(rnd64() % 16);
        x = m == 0 ? from_bits(0x7ff8000000000000ull) : m == 1 ? from_bits(0xfff0000000000001ull)  // two spellings of NaN
          : m == 2 ? (double)INFINITY : m == 3 ? -(double)INFINITY : m == 4 ? 1e150 : rnd_unit();
        break;
      }
      default: x = (i & 1) ? -0.0 : 0.0; break;
    }
    v[(size_t)i] = x;
  }
  return v;
}

struct PassCount { int key, index; };

// the selection as the kernel runs it, every histogram a plain loop over the row
static ToprRowState select_row(const std::vector<uint64_t>& key, int64_t r, PassCount* pc) {
  const int64_t n = (int64_t)key.size();
  uint64_t kmin = ~0ull, kmax = 0ull;
  for (uint64_t k : key) { kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax; }
  ToprRowState st = topr_row_begin(n, r, kmin, kmax);
  std::vector<uint32_t> hist((size_t)kToprBins);
  pc->key = pc->index = 0;
  for (int pass = 0; pass < kToprMaxPasses && st.phase != kToprResolved; ++pass) {
    std::fill(hist.begin(), hist.end(), 0u);
    CHECK(st.width >= 1 && st.width <= kToprDigitBits && st.shift >= 0 && st.shift + st.width <= 64);
    CHECK(st.quota >= 1 && st.quota < n);
    int64_t counted = 0;
    for (int64_t i = 0; i < n; ++i) {
      unsigned int d;
      if (topr_row_digit(st, key[(size_t)i], i, &d)) {
        if (d >= (1u << st.width)) { CHECK(false); continue; }
        ++hist[d];
        ++counted;
      }
    }
    CHECK(counted >= st.quota);  // the undecided part holds the quota
    if (st.phase == kToprKeyDigits) ++pc->key; else ++pc->index;
    st = topr_row_step(st, hist.data());
  }
  return st;
}

static void run_select_checks() {
  // the key: |v| order for finite values and Inf, -0 == +0, every NaN one key above Inf
  CHECK(topr_key(0.0) == 0 && topr_key(-0.0) == 0);
  CHECK(topr_key(-1.5) == topr_key(1.5) && topr_key(1.5) < topr_key(-1.5000000000000002));
  CHECK(topr_key(5e-324) == 1 && topr_key(1e308) < topr_key((double)INFINITY) && topr_key(-(double)INFINITY) == kToprInfKey);
  CHECK(topr_key(from_bits(0x7ff0000000000001ull)) == kToprNanKey && topr_key(from_bits(0xffffffffffffffffull)) == kToprNanKey);
  CHECK(kToprNanKey > kToprInfKey);
  const int64_t ns[] = {1, 2, 3, 64, 65, 1000, 4097, 8193};
  for (int64_t n : ns) {
    PassCount worst{0, 0};
    for (int kind = 0; kind < kKinds; ++kind) {
      const std::vector<double> v = make_row((Kind)kind, n);
      std::vector<uint64_t> key((size_t)n);
      for (int64_t i = 0; i < n; ++i) key[(size_t)i] = topr_key(v[(size_t)i]);
      // the reference: a stable sort, descending |v| by isless (NaN the largest, NaNs equal) -- rank[i] = place of i
      std::vector<int64_t> perm((size_t)n), rank((size_t)n);
      for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = i;
      std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
        const double x = fabs(v[(size_t)a]), y = fabs(v[(size_t)b]);
        const bool xn = x != x, yn = y != y;
        return xn != yn ? xn : (!xn && x > y);
      });
      for (int64_t k = 0; k < n; ++k) rank[(size_t)perm[(size_t)k]] = k;
      long wrong = 0;
      PassCount most{0, 0};
      for (int64_t r = -1; r <= n + 1; ++r) {
        PassCount pc;
        const ToprRowState st = select_row(key, r, &pc);
        CHECK(st.phase == kToprResolved);
        most.key = pc.key > most.key ? pc.key : most.key;
        most.index = pc.index > most.index ? pc.index : most.index;
        for (int64_t i = 0; i < n; ++i) wrong += topr_row_keep(st, key[(size_t)i], i) != (rank[(size_t)i] < r);
      }
      if (wrong) printf("n %ld %s: %ld wrong keep decisions\n", (long)n, kKindNames[kind], wrong);
      CHECK(wrong == 0);
      CHECK(most.key <= 6 && most.index <= 2);
      // one key value: no key digit at all, and the index digits the size needs (n - 1 < 2^12: one; 8193: two)
      if (kind == kConstant || kind == kZeros) {
        CHECK(most.key == 0);
        if (n > 2) CHECK(most.index == (n - 1 < 4096 ? 1 : 2));
      }
      if (kind == kLastBit) CHECK(most.key <= 1 && (n < 64 || most.key == 1));  // a span of one bit: one digit of one bit
      worst.key = most.key > worst.key ? most.key : worst.key;
      worst.index = most.index > worst.index ? most.index : worst.index;
    }
    printf("n %ld key_passes %d index_passes %d\n", (long)n, worst.key, worst.index);
  }
}

int main() {
  run_plan_checks();
  run_select_checks();
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
