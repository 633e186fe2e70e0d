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
// Which form: b2_batch_plan (spx_plan.hpp).
//   row-resident (REG): the lane's units -- xk and both box ends -- are loaded once, by unconditional loads at clamped indices so
//              that all of them are in flight, and stay in registers across the reductions.
//   row walk   (!REG): 1024 lanes re-read the row once per reduction, kB2BatchWalkUnroll units in flight per lane.
// A slot beyond the row holds xk = lo = hi = 0 and adds exact zeros to every sum, so no sum is guarded.
#include <cmath>
#include <type_traits>

#include "spx_b2_batch.h"
#include "spx_common.hpp"
#include "spx_plan.hpp"
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

// sums of NV values over a workgroup of <= 16 wavefronts, the same bits in every lane; lds = [3][16], the slots of absent
// wavefronts zero (b2_block_sum_n of spx_b2.hip)
template <int NV>
__device__ __forceinline__ void b2b_block_sum(double (&v)[3], double (*lds)[16]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum_dpp(v[k]);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[k][w] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = fold16_sum(lds[k][threadIdx.x & 15]);
}

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
  const int utot = (int)b2_batch_units(n, PAIRS);       // ... and the one-element unit of an odd row in the pairs form

  // unit u as the sums want it: xk and the box (sj + q_scale q) -+ lambda sigma of its elements, zeros beyond the row.  Loads at
  // a clamped index, never past the row's last full unit; the lane that owns the odd row's last element fetches it alone.
  auto load_unit = [&](int u, double (&x)[E], double (&lo)[E], double (&hi)[E]) {
    const int uc = u < ufull ? u : ufull - 1;
    double xv[E], sv[E], qv[E];
    if constexpr (PAIRS) {
      const f64x2 a = reinterpret_cast<const f64x2*>(xk)[uc], c = reinterpret_cast<const f64x2*>(sj)[uc],
                  d = reinterpret_cast<const f64x2*>(q)[uc];
      xv[0] = a.x; xv[1] = a.y; sv[0] = c.x; sv[1] = c.y; qv[0] = d.x; qv[1] = d.y;
      if (2 * u == n - 1) { xv[0] = xk[n - 1]; sv[0] = sj[n - 1]; qv[0] = q[n - 1]; }
    } else {
      xv[0] = xk[uc]; sv[0] = sj[uc]; qv[0] = q[uc];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool valid = u * E + e < n;
      const double sq = sv[e] + qs * qv[e];  // `sj .+ q` (:56) at q_scale q: one rounded multiply in front of the sum
      x[e] = valid ? xv[e] : 0.0;
      lo[e] = valid ? sq - ls : 0.0;
      hi[e] = valid ? sq + ls : 0.0;
    }
  };
  double X[REG ? EPL : 1], LO[REG ? EPL : 1], HI[REG ? EPL : 1];
  if constexpr (REG) {
#pragma unroll
    for (int kk = 0; kk < UPL; ++kk) {
      double x[E], lo[E], hi[E];
      load_unit((int)b2_batch_unit(kk, LANES, t), x, lo, hi);
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
    if (first) b2b_block_sum<3>(v, lds);
    else b2b_block_sum<2>(v, lds);
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
      reinterpret_cast<f64x2*>(y)[u] = o;
      if (xkn != nullptr) {
        if (k.xkn_pairs) reinterpret_cast<f64x2*>(xkn)[u] = v;
        else { xkn[2 * u] = v.x; xkn[2 * u + 1] = v.y; }
      }
      sums(q2.x, v.x, o.x);
      sums(q2.y, v.y, o.y);
    } else {  // one element: the element-wise form, or the last element of an odd row
      const int i = u * E;
      const double s = sj[i], qr = q[i];
      const double o = outv(lo[0], hi[0], x[0], s);
      const double v = (x[0] + s) + o;
      y[i] = o;
      if (xkn != nullptr) xkn[i] = v;
      sums(qr, v, o);
    }
  };
  if constexpr (REG) {
#pragma unroll
    for (int kk = 0; kk < UPL; ++kk) {
      double x[E], lo[E], hi[E];
#pragma unroll
      for (int e = 0; e < E; ++e) { x[e] = X[kk * E + e]; lo[e] = LO[kk * E + e]; hi[e] = HI[kk * E + e]; }
      store_unit((int)b2_batch_unit(kk, LANES, t), x, lo, hi);
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
  b2b_block_sum<3>(h, lds);
  if (t == 0) {
    k.stats[3 * b] = lam * h[0];
    k.stats[3 * b + 1] = h[1];
    k.stats[3 * b + 2] = h[2];
  }
}

template <int LANES, int EPL, bool REG>
void b2_batch_launch(spx_ctx* ctx, const B2BatchPlan& p, const B2BatchArgs& a) {
  if (p.pairs) hipLaunchKernelGGL((k_b2_batch<LANES, EPL, REG, true>), dim3((unsigned)p.grid), dim3(LANES), 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_b2_batch<LANES, EPL, REG, false>), dim3((unsigned)p.grid), dim3(LANES), 0, ctx->stream, a);
}
template <int TILE>
void b2_batch_launch_tile(spx_ctx* ctx, const B2BatchPlan& p, const B2BatchArgs& a) {
  if constexpr (TILE < kB2BatchTileCount) {
    if (p.tile == TILE) b2_batch_launch<kB2BatchTiles[TILE].lanes, kB2BatchTiles[TILE].epl, true>(ctx, p, a);
    else b2_batch_launch_tile<TILE + 1>(ctx, p, a);
  }
}

}  // namespace

// Every refusal is made before anything is enqueued.  There is no host destination: the call only enqueues.
SPX_EXPORT int spx_proxstep_l1_b2_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                        int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* delta,
                                        const double* q_scale, double chi_lambda, double* xkn, double* stats_dev) {
  // the libraries share spx_ctx and four functions: refuse to touch a context of a libspx.so built from other sources
  if (spx_shared_abi() != kSpxSharedAbi) {
    spx_set_error("libspx_b2_batch.so and libspx.so do not match (shared layout %d, expected %d): rebuild both", spx_shared_abi(),
                  kSpxSharedAbi);
    return SPX_ERR_INTERNAL;
  }
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(n >= 0, "n < 0");
  SPX_REQUIRE(batch >= 0, "batch < 0");
  if (batch == 0) return SPX_OK;
  SPX_REQUIRE(stats_dev != nullptr, "stats_dev is NULL");
  SPX_REQUIRE(lambda != nullptr && sigma != nullptr && delta != nullptr && q_scale != nullptr,
              "a parameter array (lambda, sigma, delta, q_scale) is NULL");
  SPX_REQUIRE(ld >= n, "ld < n");
  const void* const in[4] = {y, q, xk, sj};
  if (n > 0) {
    for (const void* v : in) SPX_REQUIRE(v != nullptr, "NULL vector with n > 0");
    SPX_REQUIRE(y != q, kSpxYAliasesQ);
    if (xkn != nullptr) {
      for (const void* o : in) SPX_REQUIRE(xkn != o, "xkn is one of the other vectors");
    }
  }
  int bits = spx_aligned16(xkn) ? 0 : 1 << 4;
  for (int v = 0; v < 4; ++v) bits |= spx_aligned16(in[v]) ? 0 : 1 << v;
  const B2BatchPlan p = b2_batch_plan(n, batch, ld, bits);
  SPX_REQUIRE(p.ok || p.why != B2BatchRefusal::kNTooLarge,
              "n > 2^20: one workgroup per problem is the wrong tool (spx_proxstep_l1_b2 holds such a problem on chip across many CUs, one "
              "problem per call)");
  SPX_REQUIRE(p.ok, "batch > 2^31 - 1");
  SPX_ON_DEVICE(ctx);
  if (n == 0) return spx_zero_async(ctx, stats_dev, (size_t)batch * 3 * sizeof(double));  // zeros for every problem, by a kernel
  const B2BatchArgs a{y, q, xk, sj, xkn, lambda, sigma, delta, q_scale, chi_lambda, ld, (int)n, p.xkn_pairs ? 1 : 0, stats_dev};
  if (p.form == B2BatchForm::kResident) b2_batch_launch_tile<0>(ctx, p, a);
  else b2_batch_launch<kB2BatchWalkLanes, 0, false>(ctx, p, a);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}
