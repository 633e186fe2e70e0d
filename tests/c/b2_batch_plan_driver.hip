/* Stand-alone driver for the device-free parts of the batched ShiftedNormL1B2 call (spx_proxstep_l1_b2_batch):
 *   no argument : row_batch_plan (csrc/spx_plan.hpp) on kB2BatchShape over a grid of n, batch, ld and alignment bits: the checks
 *     of tests/c/row_batch_plan_checks.hpp (the cover of a row by the lane slots as k_b2_batch of csrc/spx_b2_batch.hip walks
 *     them, the tile choice, what form and pairs depend on, the refusals at kB2BatchNMax + 1 and batch = 2^31).
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

// ---- (a) the plan: the checks every row-owner call shares, on this call's shape ---------------------
#include "row_batch_plan_checks.hpp"

static int run_plan_checks() {
  run_row_batch_plan_checks(kB2BatchShape);
  // the shape is the named constants
  CHECK(kB2BatchShape.tiles == kB2BatchTiles && kB2BatchShape.tile_count == kB2BatchTileCount);
  CHECK(kB2BatchShape.row_max == kB2BatchRowMax && kB2BatchShape.n_max == kB2BatchNMax);
  CHECK(kB2BatchShape.walk_lanes == kB2BatchWalkLanes && kB2BatchShape.walk_unroll == kB2BatchWalkUnroll);
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
