// spx_batch.hip -- batched separable prox! + step statistics, parameters on the device (spx_proxstep_*_batch, include/spx_batch.h).
// Built into a library of its own, libspx_batch.so, which links against libspx.so (the context, its workspace, the error text).
// The element sites are the single call's: the functors, WithStep, sep_accumulate, the block sums and the operator table come
// from spx_sep_device.hpp, which spx_separable.hip includes as well.
#include "spx_sep_device.hpp"

#include "spx_batch.h"
#include "spx_plan.hpp"  // batch_plan and the row / tile mapping of the kernels below

// ---------------------------------------------------------------------------------------------
// Batched prox! + step statistics, parameters on the device (spx_proxstep_*_batch): `batch` problems of n elements in ONE
// launch, problem b at elements [b * ld, b * ld + n) of y, q, xk, sj and xkn; lambda[b], sigma[b], q_scale[b] (Box forms: l[b],
// u[b]) are read from device memory by the workgroup that stores y, so a captured call follows the values a solver leaves
// there.  Each element site is the one of spx_proxstep_X (the functor of the same Row::make, WithStep, sep_accumulate): y and
// xkn have that call's bits.  No workgroup waits for another: no tickets, no atomics.
//   row form   (n <= kBatchRowMax): one workgroup owns a problem, walks it tile by tile with its three sums in registers and
//              stores the three statistics itself -- one launch, no workspace.
//   tiled form (larger n): workgroup (b, t) takes tile t of problem b and stores three partials to the workspace
//              ([problem][plane][tile]); k_batch_reduce, one workgroup per problem, adds them in a fixed order.
// Which form, grid and workspace: batch_plan (spx_plan.hpp), a function of n alone as far as a problem's bits go.
// Alignment: all vectors share ld, so when their bases share bit 3 of the address every row is peeled by the kernel -- a head of
// 0 or 1 elements (batch_row_map: the parity of b * ld), 16-byte pairs, a tail of 0 or 1 elements; bases of mixed alignment take
// the element-wise instantiation (PAIRS = false).  The mask is shared by the problems and read by bytes.
// ---------------------------------------------------------------------------------------------
namespace {
template <class V>
__device__ __forceinline__ V ldv_nt(const V* p) { return __builtin_nontemporal_load(p); }
template <class Op>
__device__ __forceinline__ double apply_v(const Op& op, double q, double x, double s, double l, double u, bool s0, bool) {
  return apply_op(op, q, 0.0, x, s, l, u, s0);
}
template <class Op>
__device__ __forceinline__ f64x2 apply_v(const Op& op, f64x2 q, f64x2 x, f64x2 s, double l, double u, bool s0, bool s1) {
  f64x2 r;
  r.x = apply_op(op, q.x, 0.0, x.x, s.x, l, u, s0);
  r.y = apply_op(op, q.y, 0.0, x.y, s.y, l, u, s1);
  return r;
}
// One tile of a row: its units [lo, hi) of `count` (batch_tile_units).  V = f64x2: the pairs behind the row's head, U = 6 per lane;
// V = double: the elements of the element-wise form, U = 12.  All 3 U loads of a full tile are issued before the first use.
// m: the mask at the first unit of the row (MASK), l, u: the problem's box.  Returns acc with the tile's terms added.
template <class Op, class V, bool MASK, int U>
__device__ __forceinline__ SepSums<3> batch_tile(const Op& op, SepSums<3> acc, V* y, const V* q, const V* xk, const V* sj, V* xn,
                                                 const uint8_t* m, double l, double u, int64_t count, int64_t tile) {
  constexpr int E = (int)(sizeof(V) / sizeof(double));
  static_assert(256 * U * E == kBatchTile, "a tile is kBatchTile elements");
  int64_t lo, hi;
  batch_tile_units(count, tile, 256 * U, &lo, &hi);
  const int64_t base = lo + threadIdx.x;
  const V zero = V{};
  if (hi - lo == 256 * U) {
    V vq[U], vx[U], vs[U];
    uint8_t m0[U], m1[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + k * 256;
      vq[k] = ldv_nt(q + i);
      vx[k] = ldv_nt(xk + i);
      vs[k] = ldv_nt(sj + i);
      if constexpr (MASK) { m0[k] = m[E * i]; m1[k] = m[E * i + (E - 1)]; }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + k * 256;
      bool s0 = true, s1 = true;
      if constexpr (MASK) { s0 = m0[k] != 0; s1 = m1[k] != 0; }
      const V r = apply_v(op, vq[k], vx[k], vs[k], l, u, s0, s1);
      acc = sep_accumulate<true>(op, acc, vq[k], zero, vx[k], vs[k], r, s0, s1, xn, i);
      st2<true>(y + i, r);
    }
  } else {  // the last tile of the row
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + k * 256;
      if (i < hi) {
        const V a = q[i], b = xk[i], c = sj[i];
        bool s0 = true, s1 = true;
        if constexpr (MASK) { s0 = m[E * i] != 0; s1 = m[E * i + (E - 1)] != 0; }
        const V r = apply_v(op, a, b, c, l, u, s0, s1);
        acc = sep_accumulate<false>(op, acc, a, zero, b, c, r, s0, s1, xn, i);
        y[i] = r;
      }
    }
  }
  return acc;
}
// element i of a row by one lane: the head and the tail of the pairs form
template <class Op, bool MASK>
__device__ __forceinline__ SepSums<3> batch_element(const Op& op, SepSums<3> acc, double* y, const double* q, const double* xk,
                                                    const double* sj, double* xn, const uint8_t* mask, double l, double u,
                                                    int64_t i) {
  bool sel = true;
  if constexpr (MASK) sel = mask[i] != 0;
  const double qi = q[i], xi = xk[i], si = sj[i];
  const double r = apply_v(op, qi, xi, si, l, u, sel, false);
  acc = sep_accumulate<false>(op, acc, qi, 0.0, xi, si, r, sel, false, xn, i);
  y[i] = r;
  return acc;
}

// Grid: `batch` workgroups (row form: TILED = false, a workgroup walks the `tiles` tiles of its problem) or tiles * batch
// (TILED: batch_workgroup).  out: stats_dev (row form) or the partials (TILED).
template <class Row, bool TILED, bool PAIRS, bool MASK>
__global__ __launch_bounds__(256) void k_sep_batch(double* y_, const double* q_, const double* xk_, const double* sj_, double* xkn_,
                                                    const double* __restrict__ lambda, const double* __restrict__ sigma,
                                                    const double* __restrict__ qscale, const double* __restrict__ lo,
                                                    const double* __restrict__ up, const uint8_t* mask, int64_t n, int64_t ld,
                                                    int64_t tiles, int base_odd, double* out) {
  using Base = typename Row::Op;
  using Op = WithStep<Base, typename Row::Term>;
  int64_t b = blockIdx.x, t0 = 0, t1 = tiles;
  if constexpr (TILED) {
    batch_workgroup(blockIdx.x, tiles, &b, &t0);
    t1 = t0 + 1;
  }
  // the problem's scalars: b is uniform, so these are scalar loads; the functor's constants are formed as the host forms them
  const double lam = lambda[b];
  Op op{};
  static_cast<Base&>(op) = Row::template make<Base>(lam, sigma[b]);
  op.qscale = qscale[b];
  double l = 0.0, u = 0.0;
  if constexpr (Base::kBox) { l = lo[b]; u = up[b]; }
  const int64_t off = b * ld;
  double* const y = y_ + off;
  const double* const q = q_ + off;
  const double* const xk = xk_ + off;
  const double* const sj = sj_ + off;
  double* const xn = xkn_ ? xkn_ + off : nullptr;
  SepSums<3> acc = {};
  if constexpr (PAIRS) {
    const BatchRowMap r = batch_row_map(n, b, ld, base_odd);
    const uint8_t* const m = MASK ? mask + r.head : nullptr;
    for (int64_t t = t0; t < t1; ++t)
      acc = batch_tile<Op, f64x2, MASK, 6>(op, acc, reinterpret_cast<f64x2*>(y + r.head), reinterpret_cast<const f64x2*>(q + r.head),
                                           reinterpret_cast<const f64x2*>(xk + r.head), reinterpret_cast<const f64x2*>(sj + r.head),
                                           xn ? reinterpret_cast<f64x2*>(xn + r.head) : nullptr, m, l, u, r.npairs, t);
    if (t0 == 0 && r.head && threadIdx.x == 0) acc = batch_element<Op, MASK>(op, acc, y, q, xk, sj, xn, mask, l, u, 0);
    if (t1 == tiles && r.tail && threadIdx.x == 255) acc = batch_element<Op, MASK>(op, acc, y, q, xk, sj, xn, mask, l, u, n - 1);
  } else {
    for (int64_t t = t0; t < t1; ++t) acc = batch_tile<Op, double, MASK, 12>(op, acc, y, q, xk, sj, xn, mask, l, u, n, t);
  }
  acc = block_sum4(acc);
  if (threadIdx.x == 0) {
    if constexpr (TILED) {
#pragma unroll
      for (int p = 0; p < 3; ++p) out[batch_slot(b, p, t0, tiles)] = acc.v[p];
    } else {
      out[3 * b + 0] = lam * acc.v[0];
      out[3 * b + 1] = acc.v[1];
      out[3 * b + 2] = acc.v[2];
    }
  }
}
// Workgroup b adds the three planes of problem b's partials, `tiles` slots each, in a fixed order -- the order of the single
// call's sums on short lists (value_reduce_small), eight loads in flight per lane on long ones -- and stores
// stats[3 b + {0, 1, 2}] = {lambda[b] * h terms, <q, y>, <y, y>}.  Grid: batch.
__global__ __launch_bounds__(256) void k_batch_reduce(const double* partials, int64_t tiles, const double* __restrict__ lambda,
                                                       double* stats) {
  const int64_t b = blockIdx.x;
  const double* const part = partials + batch_slot(b, 0, 0, tiles);
  SepSums<3> s;
  if (tiles <= kValueFuseMax) {
    s = value_reduce_small<false, 3>(part, tiles, (int)tiles);
  } else {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      double a8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int64_t i0 = threadIdx.x; i0 < tiles; i0 += 8 * 256) {
        double v8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int64_t i = i0 + (int64_t)k * 256;
          v8[k] = (i < tiles) ? part[p * tiles + (i < tiles ? i : 0)] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) a8[k] += v8[k];
      }
      s.v[p] = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
    }
    s = block_sum4(s);
  }
  if (threadIdx.x == 0) {
    stats[3 * b + 0] = lambda[b] * s.v[0];
    stats[3 * b + 1] = s.v[1];
    stats[3 * b + 2] = s.v[2];
  }
}

// the operands of a batched call, stated once at the entry point
struct BatchCall {
  spx_ctx* ctx;
  double* y;
  const double *q, *xk, *sj;
  int64_t n, batch, ld;
  const double *lambda, *sigma, *l, *u;
  const uint8_t* mask;
  const double* q_scale;
  double *xkn, *stats_dev;
};
template <class F>
void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
template <class Row, bool TILED, bool PAIRS, bool MASK>
void launch_batch(const BatchCall& c, const BatchPlan& p, double* out) {
  hipLaunchKernelGGL((k_sep_batch<Row, TILED, PAIRS, MASK>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, c.y, c.q, c.xk,
                     c.sj, c.xkn, c.lambda, c.sigma, c.q_scale, c.l, c.u, c.mask, c.n, c.ld, p.tiles_per_problem, p.base_odd, out);
}
// Every refusal is made before anything is enqueued.  There is no host destination: the call only enqueues.
template <class Row>
int run_proxstep_batch(const BatchCall& c) {
  constexpr bool kBox = Row::Op::kBox;
  spx_ctx* const ctx = c.ctx;
  // the two libraries share spx_ctx and four functions: refuse to touch a context of a libspx.so built from other sources
  if (spx_shared_abi() != kSpxSharedAbi) {
    spx_set_error("libspx_batch.so and libspx.so do not match (shared layout %d, expected %d): rebuild both", spx_shared_abi(), kSpxSharedAbi);
    return SPX_ERR_INTERNAL;
  }
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(c.n >= 0, "n < 0");
  SPX_REQUIRE(c.batch >= 0, "batch < 0");
  if (c.batch == 0) return SPX_OK;
  SPX_REQUIRE(c.stats_dev != nullptr, "stats_dev is NULL");
  SPX_REQUIRE(c.lambda != nullptr && c.sigma != nullptr && c.q_scale != nullptr, "a parameter array (lambda, sigma, q_scale) is NULL");
  if constexpr (kBox) SPX_REQUIRE(c.l != nullptr && c.u != nullptr, "a bound array (l, u) is NULL");
  SPX_REQUIRE(c.ld >= c.n, "ld < n");
  if (c.n > 0) {
    SPX_REQUIRE(c.y && c.q && c.xk && c.sj, "NULL vector with n > 0");
    SPX_REQUIRE(c.y != c.q, kSpxYAliasesQ);
    if (c.xkn != nullptr)
      for (const void* o : {(const void*)c.y, (const void*)c.q, (const void*)c.xk, (const void*)c.sj, (const void*)c.mask})
        SPX_REQUIRE(c.xkn != o, "xkn is one of the other vectors");
  }
  const auto bit3 = [](const void* ptr) { return (int)((reinterpret_cast<uintptr_t>(ptr) >> 3) & 1u); };
  const int bits = bit3(c.y) | (bit3(c.q) << 1) | (bit3(c.xk) << 2) | (bit3(c.sj) << 3) | (bit3(c.xkn ? c.xkn : c.y) << 4);
  const BatchPlan p = batch_plan(c.n, c.batch, c.ld, bits);
  SPX_REQUIRE(p.ok, "the call needs more than 2^31 - 1 workgroups");
  if (c.n == 0) {  // three zeros per problem, by a kernel
    SPX_ON_DEVICE(ctx);
    return spx_zero_async(ctx, c.stats_dev, (size_t)c.batch * 3 * sizeof(double));
  }
  const bool tiled = p.form == BatchForm::kTiled;
  if (tiled) {
    const int rcw = spx_ws_reserve(ctx, p.ws_bytes);
    if (rcw) return rcw;
  }
  SPX_ON_DEVICE(ctx);
  double* const out = tiled ? reinterpret_cast<double*>(ctx->ws) : c.stats_dev;
  const bool msk = kBox && c.mask != nullptr;
  with_bool(tiled, [&](auto T) {
    with_bool(p.pairs, [&](auto P) {
      if constexpr (kBox) {
        with_bool(msk, [&](auto M) { launch_batch<Row, decltype(T)::value, decltype(P)::value, decltype(M)::value>(c, p, out); });
      } else {
        launch_batch<Row, decltype(T)::value, decltype(P)::value, false>(c, p, out);
      }
    });
  });
  SPX_LAUNCH_CHECK();
  if (tiled) {
    hipLaunchKernelGGL(k_batch_reduce, dim3((unsigned)c.batch), dim3(256), 0, ctx->stream, (const double*)out, p.tiles_per_problem,
                       c.lambda, c.stats_dev);
    SPX_LAUNCH_CHECK();
  }
  return SPX_OK;
}
}  // namespace

#define SPX_PROXSTEP_BATCH(NAME, ROW)                                                                                          \
  SPX_EXPORT int NAME(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, int64_t batch, \
                      int64_t ld, const double* lambda, const double* sigma, const double* q_scale, double* xkn,              \
                      double* stats_dev) {                                                                                    \
    return run_proxstep_batch<ROW>({ctx, y, q, xk, sj, n, batch, ld, lambda, sigma, nullptr, nullptr, nullptr, q_scale, xkn,   \
                                    stats_dev});                                                                              \
  }
SPX_PROXSTEP_BATCH(spx_proxstep_l1_batch, RowL1)
SPX_PROXSTEP_BATCH(spx_proxstep_l0_batch, RowL0)
#define SPX_PROXSTEP_BATCH_BOX(NAME, ROW)                                                                                      \
  SPX_EXPORT int NAME(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, int64_t batch, \
                      int64_t ld, const double* lambda, const double* sigma, const double* l, const double* u,                \
                      const uint8_t* sel_mask, const double* q_scale, double* xkn, double* stats_dev) {                        \
    return run_proxstep_batch<ROW>({ctx, y, q, xk, sj, n, batch, ld, lambda, sigma, l, u, sel_mask, q_scale, xkn, stats_dev}); \
  }
SPX_PROXSTEP_BATCH_BOX(spx_proxstep_l1_box_batch, RowL1Box)
SPX_PROXSTEP_BATCH_BOX(spx_proxstep_l0_box_batch, RowL0Box)
