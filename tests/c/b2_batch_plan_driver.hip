/* Stand-alone driver for the device-free parts of the batched ShiftedNormL1B2 call (spx_proxstep_l1_b2_batch):
 *   no argument : b2_batch_plan (csrc/spx_plan.hpp) over a grid of n, batch, ld and alignment bits --
 *     - the lane slots of the plan's workgroup, walked as k_b2_batch of csrc/spx_b2_batch.hip walks them (b2_batch_unit,
 *       b2_batch_units), visit every element of a row exactly once and nothing beyond it;
 *     - a resident tile holds the row, and the tile before it would not; the form, the tile and the lanes depend on n alone,
 *       pairs on (n >= 2, the parity of ld, the alignment bits of y, q, xk, sj) alone, xkn_pairs on xkn's bit besides;
 *     - n = kB2BatchNMax and batch = 2^31 - 1 are accepted, one more of either is refused, each with its own reason.
 *   rows IN OUT : the step rule of csrc/spx_b2_row.hpp (b2_row_begin, b2_row_step, b2_row_scales) on the rows of the binary file
 *     IN, every sum a plain sequential loop on the host with the element expressions of the kernel.  IN: int64 rows, then per
 *     row int64 n, double lambda, sigma, delta, q_scale, chi_lambda, then q[n], xk[n], sj[n].  OUT: per row int64 reductions,
 *     then y[n].  Prints "row R n N reductions K" per row.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_b2_batch_plan_host.py; it has its own main, the library is not loaded, no HIP call is made. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "spx_plan.hpp"
#include "spx_b2_row.hpp"

static long g_checked = 0;
static int g_fail = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++g_checked;                                                                               \
    if (!(cond)) { if (g_fail < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

// ---- (a) the plan -------------------------------------------------------------------------------
// every (lane, slot) of the plan's workgroup -> its unit -> the elements of the row it covers
static void check_cover(int64_t n, const B2BatchPlan& p, std::vector<unsigned char>& seen) {
  const int E = b2_batch_unit_elems(p.pairs);
  const int64_t utot = b2_batch_units(n, p.pairs);
  int64_t slots;
  if (p.form == B2BatchForm::kResident) {
    slots = p.epl / E;
  } else {  // the row walk: whole rounds of kB2BatchWalkUnroll units per lane until the row is covered
    const int64_t round = (int64_t)p.lanes * kB2BatchWalkUnroll;
    slots = (utot + round - 1) / round * kB2BatchWalkUnroll;
  }
  seen.assign((size_t)n, 0);
  long beyond = 0, twice = 0;
  for (int t = 0; t < p.lanes; ++t)
    for (int64_t k = 0; k < slots; ++k) {
      const int64_t u = b2_batch_unit(k, p.lanes, t);
      if (u >= utot) continue;  // an idle slot: zeros
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

static int run_plan_checks() {
  std::vector<int64_t> ns = {1, 2, 3, 7, 63, 64, 65, 1000, 5000, 10000, 12289, 100000, 1000003};
  for (int i = 0; i < kB2BatchTileCount; ++i) {
    const int64_t cap = (int64_t)kB2BatchTiles[i].lanes * kB2BatchTiles[i].epl;
    for (int64_t d = -2; d <= 2; ++d) ns.push_back(cap + d);
  }
  for (int64_t d = -1; d <= 2; ++d) ns.push_back(kB2BatchRowMax + d);
  ns.push_back(2 * kB2BatchRowMax + 3);
  for (int64_t d = -2; d <= 0; ++d) ns.push_back(kB2BatchNMax + d);
  for (int64_t m = 1; m <= 3; ++m)  // around whole rounds of the row walk
    for (int64_t d = -1; d <= 1; ++d) ns.push_back(4 * m * kB2BatchWalkLanes * kB2BatchWalkUnroll + d);
  const int64_t batches[] = {1, 2, 3, 7, 256, 70001, kBatchGridMax};
  const int64_t pads[] = {0, 1, 2, 5};
  std::vector<unsigned char> seen;
  for (int64_t n : ns) {
    const B2BatchPlan ref = b2_batch_plan(n, 1, n, 0);
    CHECK(ref.ok);
    for (int64_t batch : batches)
      for (int64_t pad : pads)
        for (int bits = 0; bits < 32; ++bits) {
          const int64_t ld = n + pad;
          const B2BatchPlan p = b2_batch_plan(n, batch, ld, bits);
          CHECK(p.ok && p.why == B2BatchRefusal::kNone);
          CHECK(p.grid == batch);
          // the form is a function of n alone, pairs of the alignment class
          CHECK(p.form == ref.form && p.tile == ref.tile && p.lanes == ref.lanes && p.epl == ref.epl);
          CHECK(p.pairs == ((bits & 15) == 0 && (ld & 1) == 0 && n >= 2));
          CHECK(p.xkn_pairs == (p.pairs && (bits & 16) == 0));
          CHECK((p.form == B2BatchForm::kResident) == (n <= kB2BatchRowMax));
          if (p.form == B2BatchForm::kResident) {
            CHECK(p.tile >= 0 && p.tile < kB2BatchTileCount);
            CHECK(p.lanes == kB2BatchTiles[p.tile].lanes && p.epl == kB2BatchTiles[p.tile].epl);
            CHECK((int64_t)p.lanes * p.epl >= n);
            if (p.tile > 0) CHECK((int64_t)kB2BatchTiles[p.tile - 1].lanes * kB2BatchTiles[p.tile - 1].epl < n);
            CHECK(p.epl % 2 == 0 && p.lanes % 64 == 0 && p.lanes <= 1024);
          } else {
            CHECK(p.lanes == kB2BatchWalkLanes && p.tile == -1);
          }
        }
    // the cover, once per alignment class (it does not depend on batch)
    for (int cls = 0; cls < 2; ++cls) {
      const B2BatchPlan p = b2_batch_plan(n, 3, n + (n & 1), cls ? 1 : 0);
      CHECK(p.pairs == (cls == 0 && n >= 2));
      check_cover(n, p, seen);
    }
  }
  // the bounds
  CHECK(kB2BatchNMax == ((int64_t)1 << 20) && kB2BatchRowMax == 8192);
  CHECK(b2_batch_plan(kB2BatchNMax, kBatchGridMax, kB2BatchNMax, 0).ok);
  {
    const B2BatchPlan p = b2_batch_plan(kB2BatchNMax + 1, 1, kB2BatchNMax + 1, 0);
    CHECK(!p.ok && p.why == B2BatchRefusal::kNTooLarge);
    const B2BatchPlan g = b2_batch_plan(5, kBatchGridMax + 1, 5, 0);
    CHECK(!g.ok && g.why == B2BatchRefusal::kBatchTooLarge);
    const B2BatchPlan h = b2_batch_plan(INT64_MAX, INT64_MAX, INT64_MAX, 31);
    CHECK(!h.ok);
  }
  printf("%ld checks\n", g_checked);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}

// ---- (b) the step rule on the host ----------------------------------------------------------------
// Base.min / Base.max on Float64 (jl_min, jl_max of csrc/spx_common.hpp)
static bool signbit_of(double d) { uint64_t b; memcpy(&b, &d, 8); return (b >> 63) != 0; }
static double jl_min_h(double x, double y) { const double d = x - y; return (x != x || y != y) ? d : (signbit_of(d) ? x : y); }
static double jl_max_h(double x, double y) { const double d = x - y; return (x != x || y != y) ? d : (signbit_of(d) ? y : x); }

struct Row {
  int64_t n;
  double lam, sigma, delta, qs, chil;
  std::vector<double> q, xk, sj, y;
};

// (P, C[, F]) of the row at scale r: sequential sums of the kernel's element terms
static void row_sums(const Row& w, double r, bool first, double* P, double* C, double* F) {
  const double ls = w.lam * w.sigma;
  double p = 0.0, c = 0.0, f = 0.0;
  bool bad = false;
  for (int64_t i = 0; i < w.n; ++i) {
    const double sq = w.sj[(size_t)i] + w.qs * w.q[(size_t)i];
    const double lo = sq - ls, hi = sq + ls, x = w.xk[(size_t)i];
    const double z = (-x) * r;
    bad |= (z != z) | (lo != lo) | (hi != hi);
    const double pzf = fmin(fmax(z, lo), hi);
    const bool un = pzf == z;
    const double xm = un ? x : 0.0, cm = un ? 0.0 : pzf;
    p = fma(xm, xm, p);
    c = fma(cm, cm, c);
    if (first) {
      const double far = (x < 0.0) ? hi : (x > 0.0) ? lo : pzf;
      f = fma(far, far, f);
    }
  }
  *P = bad ? NAN : p;
  *C = c;
  if (first) *F = f;
}

static int run_row(Row& w) {
  double P = 0.0, C = 0.0, F = 0.0;
  B2RowIter it;
  row_sums(w, 1.0, true, &P, &C, &F);
  int reds = 1;
  B2RowNext next = b2_row_begin(it, P, C, F, w.delta, w.chil);
  for (; next == kB2RowReduce && reds < kB2RowMaxReductions; ++reds) {
    row_sums(w, it.eta / w.delta, false, &P, &C, &F);
    next = b2_row_step(it, P, C, w.delta, w.chil);
  }
  double r, rinv;
  b2_row_scales(it, w.delta, &r, &rinv);
  const double ls = w.lam * w.sigma;
  w.y.resize((size_t)w.n);
  for (int64_t i = 0; i < w.n; ++i) {
    const double s = w.sj[(size_t)i], sq = s + w.qs * w.q[(size_t)i];
    w.y[(size_t)i] = jl_min_h(jl_max_h((-w.xk[(size_t)i]) * r, sq - ls), sq + ls) * rinv - s;
  }
  return reds;
}

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int run_rows(const char* in, const char* out) {
  FILE* fi = fopen(in, "rb");
  if (!fi) { printf("cannot open %s\n", in); return 2; }
  FILE* fo = fopen(out, "wb");
  if (!fo) { fclose(fi); printf("cannot open %s\n", out); return 2; }
  int64_t rows = 0;
  int rc = 0;
  if (!read_exact(fi, &rows, 8) || rows < 0 || rows > 100000) rc = 2;
  for (int64_t k = 0; k < rows && rc == 0; ++k) {
    Row w;
    double par[5];
    if (!read_exact(fi, &w.n, 8) || w.n < 0 || w.n > kB2BatchNMax || !read_exact(fi, par, sizeof(par))) { rc = 2; break; }
    w.lam = par[0]; w.sigma = par[1]; w.delta = par[2]; w.qs = par[3]; w.chil = par[4];
    w.q.resize((size_t)w.n); w.xk.resize((size_t)w.n); w.sj.resize((size_t)w.n);
    if (!read_exact(fi, w.q.data(), (size_t)w.n * 8) || !read_exact(fi, w.xk.data(), (size_t)w.n * 8) ||
        !read_exact(fi, w.sj.data(), (size_t)w.n * 8)) { rc = 2; break; }
    const int64_t reds = run_row(w);
    printf("row %lld n %lld reductions %lld\n", (long long)k, (long long)w.n, (long long)reds);
    fwrite(&reds, 8, 1, fo);
    if (w.n > 0) fwrite(w.y.data(), 8, (size_t)w.n, fo);
  }
  fclose(fi);
  fclose(fo);
  if (rc) { printf("bad input\n"); return rc; }
  printf("cap %d\nok\n", kB2RowMaxReductions);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "rows") == 0) return run_rows(argv[2], argv[3]);
  if (argc == 1) return run_plan_checks();
  printf("usage: %s | %s rows IN OUT\n", argv[0], argv[0]);
  return 2;
}
