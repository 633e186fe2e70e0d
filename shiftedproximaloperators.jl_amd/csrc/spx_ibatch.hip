// spx_ibatch.hip -- batched iprox! + step statistics, parameters on the device (spx_iproxstep_*_batch, include/spx_ibatch.h).
// Built into a library of its own, libspx_ibatch.so, which links against libspx.so (the context, its workspace, the error text).
// The element sites are the single call's: the four Iprox* functors, WithIstep, sep_accumulate, the block sums and the operator
// table come from spx_sep_device.hpp, which spx_separable.hip and spx_batch.hip include as well.
#include "spx_sep_device.hpp"

#include "spx_ibatch.h"
#include "spx_plan.hpp"  // ibatch_plan and the row / tile mapping of the kernels below

// ---------------------------------------------------------------------------------------------
// Batched iprox! + step statistics (spx_iproxstep_*_batch): `batch` problems of n elements in ONE launch, problem b at elements
// [b * ld, b * ld + n) of y, g, d, xk, sj and xkn; lambda[b] (Box forms: l[b], u[b]) and d_shift[b] are read from device memory
// by the workgroup that stores y, so a captured call follows the values a solver leaves there.  Each element site is the one of
// spx_iproxstep_X (the functor of the same row of the operator table, WithIstep, sep_accumulate) at deff = d[i] + d_shift[b] --
// one rounded add (the library is built without contraction) -- or at d[i] itself when d_shift is NULL: y and xkn have that
// call's bits.  No workgroup waits for another: no tickets, no sums through atomics.
//   row form   (n <= kBatchRowMax): one workgroup owns a problem, walks it tile by tile with its four sums in registers and
//              stores the four statistics itself -- one launch, no workspace.  Unboxed forms: it clears the problem's d_flag
//              word first (one lane, an agent-scope store, then a barrier) -- the functors raise it with agent-scope atomics.
//   tiled form (larger n): workgroup (b, t) takes tile t of problem b and stores four partials to the workspace
//              ([problem][plane][tile]); k_ibatch_reduce, one workgroup per problem, adds them in a fixed order.  The d_flag
//              words are cleared by the zeroing kernel in front of the launch.
// Which form, grid and workspace: ibatch_plan (spx_plan.hpp), a function of n alone as far as a problem's bits go.
// Alignment: all vectors share ld, so when their bases share bit 3 of the address every row is peeled by the kernel -- a head of
// 0 or 1 elements (batch_row_map: the parity of b * ld), 16-byte pairs, a tail of 0 or 1 elements; bases of mixed alignment take
// the element-wise instantiation (PAIRS = false).  The mask is shared by the problems and read by bytes.
// ---------------------------------------------------------------------------------------------
namespace {
template <class V>
__device__ __forceinline__ V ldv_nt(const V* p) { return __builtin_nontemporal_load(p); }
template <class Op>
__device__ __forceinline__ double iapply_v(const Op& op, double g, double d, double x, double s, double l, double u, bool s0, bool) {
  return apply_op(op, g, d, x, s, l, u, s0);
}
template <class Op>
__device__ __forceinline__ f64x2 iapply_v(const Op& op, f64x2 g, f64x2 d, f64x2 x, f64x2 s, double l, double u, bool s0, bool s1) {
  f64x2 r;
  r.x = apply_op(op, g.x, d.x, x.x, s.x, l, u, s0);
  r.y = apply_op(op, g.y, d.y, x.y, s.y, l, u, s1);
  return r;
}
// deff = d + d_shift[b], one rounded add; d itself when the call has no d_shift (uniform per launch: no `+ 0.0`, which would
// lose the sign of a -0.0)
__device__ __forceinline__ double shift_d(double d, double sh, bool shifted) { return shifted ? d + sh : d; }
__device__ __forceinline__ f64x2 shift_d(f64x2 d, double sh, bool shifted) {
  return f64x2{shifted ? d.x + sh : d.x, shifted ? d.y + sh : d.y};
}
// the six vectors of a row (xn may be NULL), as pairs behind the row's head or as elements
template <class V>
struct IRow {
  V* y;
  const V *g, *d, *xk, *sj;
  V* xn;
};
// One tile of a row: its units [lo, hi) of `count` (batch_tile_units).  V = f64x2: the pairs behind the row's head, U = 6 per lane;
// V = double: the elements of the element-wise form, U = 12.  The loads of a full tile are staged in two halves of U / 2 units
// (four input vectors at six pairs per lane would hold 96 VGPRs of data before the first use); a lane adds its units in the
// order k = 0 .. U - 1 either way.  m: the mask at the first unit of the row (MASK), l, u: the problem's box.  Returns acc with
// the tile's terms added.
template <class Op, class V, bool MASK, int U>
__device__ __forceinline__ SepSums<4> ibatch_tile(const Op& op, SepSums<4> acc, const IRow<V>& r, const uint8_t* m, double l,
                                                  double u, double sh, bool shifted, int64_t count, int64_t tile) {
  constexpr int E = (int)(sizeof(V) / sizeof(double));
  constexpr int H = U / 2;
  static_assert(256 * U * E == kBatchTile && U % 2 == 0, "a tile is kBatchTile elements, staged in two halves");
  int64_t lo, hi;
  batch_tile_units(count, tile, 256 * U, &lo, &hi);
  const int64_t base = lo + threadIdx.x;
  if (hi - lo == 256 * U) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      V vg[H], vd[H], vx[H], vs[H];
      uint8_t m0[H], m1[H];
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const int64_t i = base + (h * H + k) * 256;
        vg[k] = ldv_nt(r.g + i);
        vd[k] = ldv_nt(r.d + i);
        vx[k] = ldv_nt(r.xk + i);
        vs[k] = ldv_nt(r.sj + i);
        if constexpr (MASK) { m0[k] = m[E * i]; m1[k] = m[E * i + (E - 1)]; }
      }
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const int64_t i = base + (h * H + k) * 256;
        bool s0 = true, s1 = true;
        if constexpr (MASK) { s0 = m0[k] != 0; s1 = m1[k] != 0; }
        const V de = shift_d(vd[k], sh, shifted);
        const V y = iapply_v(op, vg[k], de, vx[k], vs[k], l, u, s0, s1);
        acc = sep_accumulate<true>(op, acc, vg[k], de, vx[k], vs[k], y, s0, s1, r.xn, i);
        st2<true>(r.y + i, y);
      }
    }
  } else {  // the last tile of the row
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + k * 256;
      if (i < hi) {
        const V a = r.g[i], b = r.xk[i], c = r.sj[i];
        const V de = shift_d(r.d[i], sh, shifted);
        bool s0 = true, s1 = true;
        if constexpr (MASK) { s0 = m[E * i] != 0; s1 = m[E * i + (E - 1)] != 0; }
        const V y = iapply_v(op, a, de, b, c, l, u, s0, s1);
        acc = sep_accumulate<false>(op, acc, a, de, b, c, y, s0, s1, r.xn, i);
        r.y[i] = y;
      }
    }
  }
  return acc;
}
// element i of a row by one lane: the head and the tail of the pairs form
template <class Op, bool MASK>
__device__ __forceinline__ SepSums<4> ibatch_element(const Op& op, SepSums<4> acc, const IRow<double>& r, const uint8_t* mask,
                                                     double l, double u, double sh, bool shifted, int64_t i) {
  bool sel = true;
  if constexpr (MASK) sel = mask[i] != 0;
  const double gi = r.g[i], xi = r.xk[i], si = r.sj[i];
  const double de = shift_d(r.d[i], sh, shifted);
  const double y = iapply_v(op, gi, de, xi, si, l, u, sel, false);
  acc = sep_accumulate<false>(op, acc, gi, de, xi, si, y, sel, false, r.xn, i);
  r.y[i] = y;
  return acc;
}

// Grid: `batch` workgroups (row form: TILED = false, a workgroup walks the `tiles` tiles of its problem) or tiles * batch
// (TILED: batch_workgroup).  out: stats_dev (row form) or the partials (TILED).  dshift: NULL = d as it is.  dflag: the unboxed
// forms' words, one per problem (NULL for the Box forms).
template <class Row, bool TILED, bool PAIRS, bool MASK>
__global__ __launch_bounds__(256) void k_isep_batch(double* y_, const double* g_, const double* d_, const double* xk_,
                                                     const double* sj_, double* xkn_, const double* __restrict__ lambda,
                                                     const double* __restrict__ dshift, const double* __restrict__ lo,
                                                     const double* __restrict__ up, const uint8_t* mask, int* dflag, int64_t n,
                                                     int64_t ld, int64_t tiles, int base_odd, double* out) {
  using Base = typename Row::Op;
  using Op = WithIstep<Base, typename Row::Term>;
  int64_t b = blockIdx.x, t0 = 0, t1 = tiles;
  if constexpr (TILED) {
    batch_workgroup(blockIdx.x, tiles, &b, &t0);
    t1 = t0 + 1;
  }
  // the problem's scalars: b is uniform, so these are scalar loads
  const double lam = lambda[b];
  const bool shifted = dshift != nullptr;
  const double sh = shifted ? dshift[b] : 0.0;
  Op op{};
  op.lambda = lam;
  double l = 0.0, u = 0.0;
  if constexpr (Base::kBox) { l = lo[b]; u = up[b]; }
  if constexpr (Row::kFlagged) {
    op.flag = dflag + b;
    if constexpr (!TILED) {  // the row's owner clears the word before the row's first element site
      if (threadIdx.x == 0) __hip_atomic_store(op.flag, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __syncthreads();
    }
  }
  const int64_t off = b * ld;
  const IRow<double> row{y_ + off, g_ + off, d_ + off, xk_ + off, sj_ + off, xkn_ ? xkn_ + off : nullptr};
  SepSums<4> acc = {};
  if constexpr (PAIRS) {
    const BatchRowMap r = batch_row_map(n, b, ld, base_odd);
    const uint8_t* const m = MASK ? mask + r.head : nullptr;
    const IRow<f64x2> prs{reinterpret_cast<f64x2*>(row.y + r.head), reinterpret_cast<const f64x2*>(row.g + r.head),
                          reinterpret_cast<const f64x2*>(row.d + r.head), reinterpret_cast<const f64x2*>(row.xk + r.head),
                          reinterpret_cast<const f64x2*>(row.sj + r.head),
                          row.xn ? reinterpret_cast<f64x2*>(row.xn + r.head) : nullptr};
    for (int64_t t = t0; t < t1; ++t) acc = ibatch_tile<Op, f64x2, MASK, 6>(op, acc, prs, m, l, u, sh, shifted, r.npairs, t);
    if (t0 == 0 && r.head && threadIdx.x == 0) acc = ibatch_element<Op, MASK>(op, acc, row, mask, l, u, sh, shifted, 0);
    if (t1 == tiles && r.tail && threadIdx.x == 255) acc = ibatch_element<Op, MASK>(op, acc, row, mask, l, u, sh, shifted, n - 1);
  } else {
    for (int64_t t = t0; t < t1; ++t) acc = ibatch_tile<Op, double, MASK, 12>(op, acc, row, mask, l, u, sh, shifted, n, t);
  }
  acc = block_sum4(acc);
  if (threadIdx.x == 0) {
    if constexpr (TILED) {
#pragma unroll
      for (int p = 0; p < 4; ++p) out[ibatch_slot(b, p, t0, tiles)] = acc.v[p];
    } else {
      out[4 * b + 0] = lam * acc.v[0];
      out[4 * b + 1] = acc.v[1];
      out[4 * b + 2] = acc.v[2];
      out[4 * b + 3] = acc.v[3];
    }
  }
}
// Workgroup b adds the four planes of problem b's partials, `tiles` slots each, in a fixed order -- the order of the single
// call's sums on short lists (value_reduce_small), eight loads in flight per lane on long ones -- and stores
// stats[4 b + {0, 1, 2, 3}] = {lambda[b] * h terms, <g, y>, <deff .* y, y>, <y, y>}.  Grid: batch.
__global__ __launch_bounds__(256) void k_ibatch_reduce(const double* partials, int64_t tiles, const double* __restrict__ lambda,
                                                        double* stats) {
  const int64_t b = blockIdx.x;
  const double* const part = partials + ibatch_slot(b, 0, 0, tiles);
  SepSums<4> s;
  if (tiles <= kValueFuseMax) {
    s = value_reduce_small<false, 4>(part, tiles, (int)tiles);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
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
    stats[4 * b + 0] = lambda[b] * s.v[0];
    stats[4 * b + 1] = s.v[1];
    stats[4 * b + 2] = s.v[2];
    stats[4 * b + 3] = s.v[3];
  }
}

// the operands of a batched call, stated once at the entry point
struct IbatchCall {
  spx_ctx* ctx;
  double* y;
  const double *g, *d, *xk, *sj;
  int64_t n, batch, ld;
  const double *lambda, *d_shift;
  int32_t* d_flag;
  const double *l, *u;
  const uint8_t* mask;
  double *xkn, *stats_dev;
};
template <class F>
void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
template <class Row, bool TILED, bool PAIRS, bool MASK>
void launch_ibatch(const IbatchCall& c, const BatchPlan& p, double* out) {
  hipLaunchKernelGGL((k_isep_batch<Row, TILED, PAIRS, MASK>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, c.y, c.g, c.d,
                     c.xk, c.sj, c.xkn, c.lambda, c.d_shift, c.l, c.u, c.mask, c.d_flag, c.n, c.ld, p.tiles_per_problem, p.base_odd,
                     out);
}
// Every refusal is made before anything is enqueued.  There is no host destination: the call only enqueues.
template <class Row>
int run_iproxstep_batch(const IbatchCall& c) {
  constexpr bool kBox = Row::Op::kBox;
  static_assert(Row::kFlagged == !kBox, "the unboxed forms carry the d > 0 flag");
  spx_ctx* const ctx = c.ctx;
  // the libraries share spx_ctx and four functions: refuse to touch a context of a libspx.so built from other sources
  if (spx_shared_abi() != kSpxSharedAbi) {
    spx_set_error("libspx_ibatch.so and libspx.so do not match (shared layout %d, expected %d): rebuild both", spx_shared_abi(), kSpxSharedAbi);
    return SPX_ERR_INTERNAL;
  }
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(c.n >= 0, "n < 0");
  SPX_REQUIRE(c.batch >= 0, "batch < 0");
  if (c.batch == 0) return SPX_OK;
  SPX_REQUIRE(c.stats_dev != nullptr, "stats_dev is NULL");
  SPX_REQUIRE(c.lambda != nullptr, "lambda is NULL");
  if constexpr (kBox) SPX_REQUIRE(c.l != nullptr && c.u != nullptr, "a bound array (l, u) is NULL");
  if constexpr (!kBox) SPX_REQUIRE(c.d_flag != nullptr, "d_flag is NULL");
  SPX_REQUIRE(c.ld >= c.n, "ld < n");
  if (c.n > 0) {
    SPX_REQUIRE(c.y && c.g && c.d && c.xk && c.sj, "NULL vector with n > 0");
    SPX_REQUIRE(c.y != c.g && c.y != c.d, "y aliases g or d (the sums would read an overwritten input)");
    if (c.xkn != nullptr)
      for (const void* o : {(const void*)c.y, (const void*)c.g, (const void*)c.d, (const void*)c.xk, (const void*)c.sj, (const void*)c.mask})
        SPX_REQUIRE(c.xkn != o, "xkn is one of the other vectors");
  }
  const auto bit3 = [](const void* ptr) { return (int)((reinterpret_cast<uintptr_t>(ptr) >> 3) & 1u); };
  const int bits = bit3(c.y) | (bit3(c.g) << 1) | (bit3(c.d) << 2) | (bit3(c.xk) << 3) | (bit3(c.sj) << 4) |
                   (bit3(c.xkn ? c.xkn : c.y) << 5);
  const BatchPlan p = ibatch_plan(c.n, c.batch, c.ld, bits);
  SPX_REQUIRE(p.ok, "the call needs more than 2^31 - 1 workgroups");
  if (c.n == 0) {  // four zeros (and a clear flag word) per problem, by a kernel
    SPX_ON_DEVICE(ctx);
    if constexpr (!kBox) {
      const int rz = spx_zero_async(ctx, c.d_flag, (size_t)c.batch * sizeof(int32_t));
      if (rz) return rz;
    }
    return spx_zero_async(ctx, c.stats_dev, (size_t)c.batch * 4 * sizeof(double));
  }
  const bool tiled = p.form == BatchForm::kTiled;
  if (tiled) {
    const int rcw = spx_ws_reserve(ctx, p.ws_bytes);
    if (rcw) return rcw;
  }
  SPX_ON_DEVICE(ctx);
  if constexpr (!kBox) {
    if (tiled) {  // (a kernel node, never a memset node; the row form clears its word inside the launch)
      const int rz = spx_zero_async(ctx, c.d_flag, (size_t)c.batch * sizeof(int32_t));
      if (rz) return rz;
    }
  }
  double* const out = tiled ? reinterpret_cast<double*>(ctx->ws) : c.stats_dev;
  const bool msk = kBox && c.mask != nullptr;
  with_bool(tiled, [&](auto T) {
    with_bool(p.pairs, [&](auto P) {
      if constexpr (kBox) {
        with_bool(msk, [&](auto M) { launch_ibatch<Row, decltype(T)::value, decltype(P)::value, decltype(M)::value>(c, p, out); });
      } else {
        launch_ibatch<Row, decltype(T)::value, decltype(P)::value, false>(c, p, out);
      }
    });
  });
  SPX_LAUNCH_CHECK();
  if (tiled) {
    hipLaunchKernelGGL(k_ibatch_reduce, dim3((unsigned)c.batch), dim3(256), 0, ctx->stream, (const double*)out, p.tiles_per_problem,
                       c.lambda, c.stats_dev);
    SPX_LAUNCH_CHECK();
  }
  return SPX_OK;
}
}  // namespace

#define SPX_IPROXSTEP_BATCH(NAME, ROW)                                                                                          \
  SPX_EXPORT int NAME(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj, int64_t n, \
                      int64_t batch, int64_t ld, const double* lambda, const double* d_shift, int32_t* d_flag, double* xkn,     \
                      double* stats_dev) {                                                                                      \
    return run_iproxstep_batch<ROW>({ctx, y, g, d, xk, sj, n, batch, ld, lambda, d_shift, d_flag, nullptr, nullptr, nullptr,    \
                                     xkn, stats_dev});                                                                          \
  }
SPX_IPROXSTEP_BATCH(spx_iproxstep_l1_batch, RowIproxL1)
SPX_IPROXSTEP_BATCH(spx_iproxstep_l0_batch, RowIproxL0)
#define SPX_IPROXSTEP_BATCH_BOX(NAME, ROW)                                                                                      \
  SPX_EXPORT int NAME(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj, int64_t n, \
                      int64_t batch, int64_t ld, const double* lambda, const double* d_shift, const double* l, const double* u, \
                      const uint8_t* sel_mask, double* xkn, double* stats_dev) {                                                \
    return run_iproxstep_batch<ROW>({ctx, y, g, d, xk, sj, n, batch, ld, lambda, d_shift, nullptr, l, u, sel_mask, xkn,         \
                                     stats_dev});                                                                               \
  }
SPX_IPROXSTEP_BATCH_BOX(spx_iproxstep_l1_box_batch, RowIproxL1Box)
SPX_IPROXSTEP_BATCH_BOX(spx_iproxstep_l0_box_batch, RowIproxL0Box)
