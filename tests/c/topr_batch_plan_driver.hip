/* Stand-alone driver for the device-free parts of the batched top-r calls (spx_proxstep_indball_l0[_binf]_batch):
 *   (a) row_batch_plan (csrc/spx_plan.hpp) on kToprBatchShape over a grid of n, batch, ld and alignment bits: the checks of
 *     tests/c/row_batch_plan_checks.hpp (the cover of a row by the lane slots as k_topr_batch of csrc/spx_topr_batch.hip walks
 *     them, the tile choice, what form and pairs depend on, the refusals at kToprBatchNMax + 1 and batch = 2^31).
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

// ---- (a) the plan: the checks every row-owner call shares, on this call's shape ---------------------
#include "row_batch_plan_checks.hpp"

static void run_plan_checks() {
  run_row_batch_plan_checks(kToprBatchShape);
  // the shape is the named constants
  CHECK(kToprBatchShape.tiles == kToprBatchTiles && kToprBatchShape.tile_count == kToprBatchTileCount);
  CHECK(kToprBatchShape.row_max == kToprBatchRowMax && kToprBatchShape.n_max == kToprBatchNMax);
  CHECK(kToprBatchShape.walk_lanes == kToprBatchWalkLanes && kToprBatchShape.walk_unroll == kToprBatchWalkUnroll);
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
