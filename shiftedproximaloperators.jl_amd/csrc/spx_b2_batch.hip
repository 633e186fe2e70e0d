// spx_b2_batch.hip -- batched ShiftedNormL1B2 prox! + step statistics, parameters on the device (spx_proxstep_l1_b2_batch,
// include/spx_b2_batch.h).  Built into a library of its own, libspx_b2_batch.so, which links against libspx.so (the context, the
// error text, the zero-fill kernel of the empty call).  `batch` trust-region lasso problems in ONE launch, problem b at elements
// [b * ld, b * ld + n) of every vector; lambda[b], sigma[b], delta[b], q_scale[b] are read from device memory by the workgroup
// that owns the row.
//
// ONE workgroup owns ONE problem from its first sum to its last store.  The single call (k_b2_coop, spx_b2.hip) spreads one problem
// over a resident grid and pays a memory round trip for every reduction of the root find; here every reduction is a wave sum and
// one pass through LDS, nobody waits for another workgroup, and nothing depends on what is resident: no exchange words, no
// spx_ctx::sync, no workspace, no residency query.  The iteration is that of spx_b2.hip's head comment, its rule stated once in
// spx_b2_row.hpp (b2_row_begin, b2_row_step) and run to the exact fixed point:
//   1. the sums P, C at r = 1 and the bound sum F;   2. Delta < chi_lambda sqrt(P + C)?   3. active: start from chi_lambda sqrt(F);
//   4. piece roots, safeguarded by the bracket, one reduction each;   5. the storing sweep
//      y = jl_min(jl_max((-xk) r, lo), hi) rinv - sj -- Julia-semantics min / max at the store only, fma-masked sums elsewhere.
// Every lane forms the same totals (a fixed shape: wave_sum_dpp, then fold16_sum over the wavefronts' slots) and redoes the
// scalar update for itself, so the workgroup needs no broadcast.
// Which form: row_batch_plan on kB2BatchShape (spx_plan.hpp); the site shared with the other row-owner calls: spx_row_batch.hpp.
//   row-resident (REG): the lane's units -- xk and both box ends -- are loaded once, by unconditional loads at clamped indices so
//              that all of them are in flight, and stay in registers across the reductions.
//   row walk   (!REG): 1024 lanes re-read the row once per reduction, kB2BatchWalkUnroll units in flight per lane.
// A slot beyond the row holds xk = lo = hi = 0 and adds exact zeros to every sum, so no sum is guarded.
#include <cmath>
#include <type_traits>

#include "spx_b2_batch.h"
#include "spx_row_batch.hpp"
#include "spx_b2_row.hpp"

namespace {

// what a kernel is launched with
struct B2BatchArgs {
  double* y;
  const double *q, *xk, *sj;
  double* xkn;  // or NULL
  const double *lambda, *sigma, *delta, *qscale;
  double chil;
  int64_t ld;
  int n;         // <= kB2BatchNMax
  int xkn_pairs;
  double* stats;
};

template <int LANES, int EPL, bool REG, bool PAIRS>
__global__ __launch_bounds__(LANES) void k_b2_batch(B2BatchArgs k) {
  constexpr int E = PAIRS ? 2 : 1;            // elements of a unit
  constexpr int UPL = REG ? EPL / E : 1;      // units a lane keeps in registers
  static_assert(!REG || EPL % 2 == 0, "whole pairs per lane");
  __shared__ double lds[3][16];
  const int t = threadIdx.x;
  if (t < 48) (&lds[0][0])[t] = 0.0;  // (the first block sum starts with a barrier)
  // the problem's scalars: the row is uniform, so these are scalar loads
  const int64_t b = blockIdx.x;
  const double lam = k.lambda[b];
  const double ls = lam * k.sigma[b];  // `psi.lambda * sigma`: one rounded multiply (the library is built without contraction)
  const double delta = k.delta[b], qs = k.qscale[b], chil = k.chil;
  const int64_t off = b * k.ld;
  double* const y = k.y + off;
  const double *const q = k.q + off, *const xk = k.xk + off, *const sj = k.sj + off;
  double* const xkn = k.xkn ? k.xkn + off : nullptr;
  const int n = k.n;
  const int ufull = n / E;                              // units of E elements; >= 1 (pairs: n >= 2)
  const int utot = (int)row_batch_units(n, PAIRS);      // ... and the one-element unit of an odd row in the pairs form

  // unit u as the sums want it: xk and the box (sj + q_scale q) -+ lambda sigma of its elements, zeros beyond the row
  auto load_unit = [&](int u, double (&x)[E], double (&lo)[E], double (&hi)[E]) {
    const double* const in[3] = {xk, sj, q};
    double w[3][E];
    row_load_unit<PAIRS>(in, u, ufull, n, w);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool valid = u * E + e < n;
      const double sq = w[1][e] + qs * w[2][e];  // `sj .+ q` (:56) at q_scale q: one rounded multiply in front of the sum
      x[e] = valid ? w[0][e] : 0.0;
      lo[e] = valid ? sq - ls : 0.0;
      hi[e] = valid ? sq + ls : 0.0;
    }
  };
  double X[REG ? EPL : 1], LO[REG ? EPL : 1], HI[REG ? EPL : 1];
  if constexpr (REG) {
#pragma unroll
    for (int kk = 0; kk < UPL; ++kk) {
      double x[E], lo[E], hi[E];
      load_unit((int)row_batch_unit(kk, LANES, t), x, lo, hi);
#pragma unroll
      for (int e = 0; e < E; ++e) { X[kk * E + e] = x[e]; LO[kk * E + e] = lo[e]; HI[kk * E + e] = hi[e]; }
    }
  }
  // the sums at scale r over one element (acc of k_b2_coop): v_max_f64 / v_min_f64 and masked fma operands; a NaN operand -- which
  // they would drop -- is tracked and poisons P, as the reference's norm would be NaN
  bool bad = false;
  auto one = [&](double lo, double hi, double x, double r, bool first, double (&v)[3]) {
    const double z = (-x) * r;
    bad |= (z != z) | (lo != lo) | (hi != hi);
    const double pzf = fmin(fmax(z, lo), hi);
    const bool un = (pzf == z);
    const double xm = un ? x : 0.0, cm = un ? 0.0 : pzf;
    v[0] = __builtin_fma(xm, xm, v[0]);
    v[1] = __builtin_fma(cm, cm, v[1]);
    if (first) {
      const double far = (x < 0.0) ? hi : (x > 0.0) ? lo : pzf;  // -x > 0: z -> +inf -> hi
      v[2] = __builtin_fma(far, far, v[2]);
    }
  };
  double P = 0.0, C = 0.0, F = 0.0;
  // one reduction: (P, C[, F]) of the row at scale r, in every lane
  auto reduce = [&](double r, bool first) {
    double v[3] = {0.0, 0.0, 0.0};
    bad = false;
    if constexpr (REG) {
#pragma unroll
      for (int kk = 0; kk < UPL; ++kk) {
#pragma unroll
        for (int e = 0; e < E; ++e) one(LO[kk * E + e], HI[kk * E + e], X[kk * E + e], r, first, v);
      }
    } else {
      for (int base = 0; base < utot; base += LANES * kB2BatchWalkUnroll) {
        double x[kB2BatchWalkUnroll][E], lo[kB2BatchWalkUnroll][E], hi[kB2BatchWalkUnroll][E];
#pragma unroll
        for (int j = 0; j < kB2BatchWalkUnroll; ++j) load_unit(base + j * LANES + t, x[j], lo[j], hi[j]);
#pragma unroll
        for (int j = 0; j < kB2BatchWalkUnroll; ++j) {
#pragma unroll
          for (int e = 0; e < E; ++e) one(lo[j][e], hi[j][e], x[j][e], r, first, v);
        }
      }
    }
    if (bad) v[0] = __longlong_as_double(0x7ff8000000000000ll);
    if (first) row_block_sum<3>(v, lds);
    else row_block_sum<2>(v, lds);
    P = v[0]; C = v[1];
    if (first) F = v[2];
  };
  // ---- the root iteration (spx_b2_row.hpp), every lane for itself on identical sums
  B2RowIter it;
  reduce(1.0, true);
  B2RowNext next = b2_row_begin(it, P, C, F, delta, chil);
  for (int reds = 1; next == kB2RowReduce && reds < kB2RowMaxReductions; ++reds) {
    reduce(it.eta / delta, false);
    next = b2_row_step(it, P, C, delta, chil);
  }
  double r, rinv;
  b2_row_scales(it, delta, &r, &rinv);
  // ---- the storing sweep: y (:59 / :63, :65, bit-faithful), xkn = (xk + sj) + y, and the three sums over the STORED y
  double h[3] = {0.0, 0.0, 0.0};  // sum |(xk + sj) + y|, sum q y (q AS PASSED), sum y^2
  auto outv = [&](double lo, double hi, double x, double s) -> double { return jl_min(jl_max((-x) * r, lo), hi) * rinv - s; };
  auto sums = [&](double qr, double v, double o) {
    h[0] += fabs(v);
    h[1] += qr * o;
    h[2] += o * o;
  };
  auto store_unit = [&](int u, const double (&x)[E], const double (&lo)[E], const double (&hi)[E]) {
    if (u >= utot) return;
    if (PAIRS && u < ufull) {
      const f64x2 s2 = reinterpret_cast<const f64x2*>(sj)[u], q2 = reinterpret_cast<const f64x2*>(q)[u];
      const f64x2 o{outv(lo[0], hi[0], x[0], s2.x), outv(lo[E - 1], hi[E - 1], x[E - 1], s2.y)};
      const f64x2 v{(x[0] + s2.x) + o.x, (x[E - 1] + s2.y) + o.y};
      row_store_y<PAIRS>(y, u, true, o.x, o.y);
      row_store_xkn<PAIRS>(xkn, k.xkn_pairs, u, true, v.x, v.y);
      sums(q2.x, v.x, o.x);
      sums(q2.y, v.y, o.y);
    } else {  // one element: the element-wise form, or the last element of an odd row
      const int i = u * E;
      const double s = sj[i], qr = q[i];
      const double o = outv(lo[0], hi[0], x[0], s);
      const double v = (x[0] + s) + o;
      row_store_y<PAIRS>(y, u, false, o, o);
      row_store_xkn<PAIRS>(xkn, k.xkn_pairs, u, false, v, v);
      sums(qr, v, o);
    }
  };
  if constexpr (REG) {
#pragma unroll
    for (int kk = 0; kk < UPL; ++kk) {
      double x[E], lo[E], hi[E];
#pragma unroll
      for (int e = 0; e < E; ++e) { x[e] = X[kk * E + e]; lo[e] = LO[kk * E + e]; hi[e] = HI[kk * E + e]; }
      store_unit((int)row_batch_unit(kk, LANES, t), x, lo, hi);
    }
  } else {
    for (int base = 0; base < utot; base += LANES * kB2BatchWalkUnroll) {
      double x[kB2BatchWalkUnroll][E], lo[kB2BatchWalkUnroll][E], hi[kB2BatchWalkUnroll][E];
#pragma unroll
      for (int j = 0; j < kB2BatchWalkUnroll; ++j) load_unit(base + j * LANES + t, x[j], lo[j], hi[j]);
#pragma unroll
      for (int j = 0; j < kB2BatchWalkUnroll; ++j) store_unit(base + j * LANES + t, x[j], lo[j], hi[j]);
    }
  }
  row_block_sum<3>(h, lds);
  if (t == 0) {
    k.stats[3 * b] = lam * h[0];
    k.stats[3 * b + 1] = h[1];
    k.stats[3 * b + 2] = h[2];
  }
}

// what differs from the other row-owner calls on the host (run_row_batch, spx_row_batch.hpp)
struct B2BatchKind {
  static constexpr const char* kLibName = "libspx_b2_batch.so";
  static constexpr RowBatchShape kShape = kB2BatchShape;
  struct Params {
    const double *lambda, *sigma, *delta, *q_scale;
    double chi_lambda;
  };
  static bool null_params(const Params& a) { return a.lambda == nullptr || a.sigma == nullptr || a.delta == nullptr || a.q_scale == nullptr; }
  static constexpr const char* kNullParams = "a parameter array (lambda, sigma, delta, q_scale) is NULL";
  static const char* refuse_alias(const RowBatchCall&) { return nullptr; }
  static constexpr const char* kNTooLarge =
      "n > 2^20: one workgroup per problem is the wrong tool (spx_proxstep_l1_b2 holds such a problem on chip across many CUs, one "
      "problem per call)";
  template <int LANES, int EPL, bool REG, bool PAIRS>
  static void launch(const RowBatchCall& c, const Params& a, const RowBatchPlan& p) {
    hipLaunchKernelGGL((k_b2_batch<LANES, EPL, REG, PAIRS>), dim3((unsigned)p.grid), dim3(LANES), 0, c.ctx->stream,
                       B2BatchArgs{c.y, c.q, c.xk, c.sj, c.xkn, a.lambda, a.sigma, a.delta, a.q_scale, a.chi_lambda, c.ld, (int)c.n,
                                   p.xkn_pairs ? 1 : 0, c.stats_dev});
  }
};

}  // namespace

SPX_EXPORT int spx_proxstep_l1_b2_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                        int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* delta,
                                        const double* q_scale, double chi_lambda, double* xkn, double* stats_dev) {
  return run_row_batch<B2BatchKind>({ctx, y, q, xk, sj, n, batch, ld, xkn, stats_dev}, {lambda, sigma, delta, q_scale, chi_lambda});
}
