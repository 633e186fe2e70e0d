// spx_batch_device.hpp -- the batched separable calls (spx_batch.hip: prox!, spx_ibatch.hip: iprox!), stated once: the walk of
// a row tile by tile, the kernel body, the reduce of the tiled form's partials and the host run.  A call is `batch` problems
// of n elements in ONE launch, problem b at elements [b * ld, b * ld + n) of every vector; its parameters are read from device
// memory by the workgroup that stores y, so a captured call follows the values a solver leaves there.  The element sites are
// the single call's (apply_op, sep_accumulate of spx_sep_device.hpp): y and xkn have that call's bits.  No workgroup waits for
// another: no tickets, no sums through atomics.
//   row form   (n <= kBatchRowMax): one workgroup owns a problem, walks it tile by tile with its sums in registers and stores
//              the statistics itself -- one launch, no workspace.
//   tiled form (larger n): workgroup (b, t) takes tile t of problem b and stores its partials to the workspace
//              ([problem][plane][tile]); the reduce kernel, one workgroup per problem, adds them in a fixed order.
// Which form, grid and workspace: batch_plan (spx_plan.hpp), a function of n alone as far as a problem's bits go.
// (The batched group calls, spx_gbatch.hip and spx_gbinf_batch.hip, have kernel bodies of their own and a host run of their
//  own, run_gbatch of spx_gbatch_device.hpp; they share the workspace layout, the reduce -- batch_reduce_body -- and with_bool.)
// Alignment: all vectors share ld, so when their bases share bit 3 of the address every row is peeled by the kernel -- a head of
// 0 or 1 elements (batch_row_map: the parity of b * ld), 16-byte pairs, a tail of 0 or 1 elements; bases of mixed alignment take
// the element-wise instantiation (PAIRS = false).  The mask is shared by the problems and read by bytes.
//
// What differs between the calls is a Kind (ProxKind, IproxKind: one struct in each .hip file):
//   kPlan            the vectors and planes of the call (BatchKind, spx_plan.hpp); a plane per sum of Op
//   kStages          the loads of a full tile are issued in kStages groups of U / kStages units before their first use
//   kHasD            the call has a d vector (and a d_shift); otherwise d is the constant zero
//   Op<Row>, make_op the functor of a Row and its constants for problem b, formed on the device as the host forms them
//   kLibName, refuse_params, refuse_alias, inputs, zero_flags, launch, kReduce     the host run's share (run_batch below)
#pragma once
#include "spx_sep_device.hpp"

#include "spx_plan.hpp"

namespace {
template <class V>
__device__ __forceinline__ V ldv_nt(const V* p) { return __builtin_nontemporal_load(p); }
template <class Op>
__device__ __forceinline__ double apply_v(const Op& op, double a, double d, double x, double s, double l, double u, bool s0, bool) {
  return apply_op(op, a, d, x, s, l, u, s0);
}
template <class Op>
__device__ __forceinline__ f64x2 apply_v(const Op& op, f64x2 a, f64x2 d, f64x2 x, f64x2 s, double l, double u, bool s0, bool s1) {
  f64x2 r;
  r.x = apply_op(op, a.x, d.x, x.x, s.x, l, u, s0);
  r.y = apply_op(op, a.y, d.y, x.y, s.y, l, u, s1);
  return r;
}
// deff = d + d_shift[b], one rounded add; d itself when the call has no d_shift (uniform per launch: no `+ 0.0`, which would
// lose the sign of a -0.0)
__device__ __forceinline__ double shift_d(double d, double sh, bool shifted) { return shifted ? d + sh : d; }
__device__ __forceinline__ f64x2 shift_d(f64x2 d, double sh, bool shifted) {
  return f64x2{shifted ? d.x + sh : d.x, shifted ? d.y + sh : d.y};
}
// the vectors of a row (a: q or g; d: kHasD only; xn may be NULL), as pairs behind the row's head or as elements
template <class V>
struct BatchRow {
  V* y;
  const V *a, *d, *xk, *sj;
  V* xn;
};
// what a kernel is launched with (the union of the two calls' parameters; the __global__ wrappers fill it)
struct BatchArgs {
  BatchRow<double> v;  // the bases of the vectors
  const double *lambda, *sigma, *qscale, *dshift, *lo, *up;
  const uint8_t* mask;
  int* dflag;
  int64_t n, ld, tiles;
  int base_odd;
  double* out;  // stats_dev (row form) or the partials (TILED)
};

// d at unit i as loaded (shift_d is applied at the site); the constant zero for a call without d
template <class Kind, bool NT, class V>
__device__ __forceinline__ V load_d(const V* d, int64_t i) {
  if constexpr (!Kind::kHasD) return V{};
  else if constexpr (NT) return ldv_nt(d + i);
  else return d[i];
}
// One element site: unit i of row r from its loaded a, d, xk, sj and selection bits.  l, u: the problem's box; sh, shifted:
// shift_d (kHasD).  NT: the stores are non-temporal.  Returns acc with the site's terms added.
template <class Kind, bool NT, class Op, class V>
__device__ __forceinline__ SumsFor<Op> batch_site(const Op& op, SumsFor<Op> acc, const BatchRow<V>& r, int64_t i, V a, V d, V x, V s,
                                                  bool s0, bool s1, double l, double u, double sh, bool shifted) {
  if constexpr (Kind::kHasD) d = shift_d(d, sh, shifted);
  const V y = apply_v(op, a, d, x, s, l, u, s0, s1);
  acc = sep_accumulate<NT>(op, acc, a, d, x, s, y, s0, s1, r.xn, i);
  st2<NT>(r.y + i, y);
  return acc;
}
// One tile of a row: its units [lo, hi) of `count` (batch_tile_units).  V = f64x2: the pairs behind the row's head, U = 6 per lane;
// V = double: the elements of the element-wise form, U = 12.  The loads of a full tile are issued before their first use, in
// kStages groups of U / kStages units (iprox!: four input vectors at six pairs per lane would hold 96 VGPRs of data at once); a
// lane adds its units in the order k = 0 .. U - 1 either way.  m: the mask at the first unit of the row (MASK).
template <class Kind, class Op, class V, bool MASK, int U>
__device__ __forceinline__ SumsFor<Op> batch_tile(const Op& op, SumsFor<Op> acc, const BatchRow<V>& r, const uint8_t* m, double l,
                                                  double u, double sh, bool shifted, int64_t count, int64_t tile) {
  constexpr int E = (int)(sizeof(V) / sizeof(double));
  constexpr int H = U / Kind::kStages;
  static_assert(256 * U * E == kBatchTile && U % Kind::kStages == 0, "a tile is kBatchTile elements, staged in equal groups");
  int64_t lo, hi;
  batch_tile_units(count, tile, 256 * U, &lo, &hi);
  const int64_t base = lo + threadIdx.x;
  if (hi - lo == 256 * U) {
#pragma unroll
    for (int h = 0; h < Kind::kStages; ++h) {
      V va[H], vd[H], vx[H], vs[H];
      uint8_t m0[H], m1[H];
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const int64_t i = base + (h * H + k) * 256;
        va[k] = ldv_nt(r.a + i);
        vd[k] = load_d<Kind, true>(r.d, i);
        vx[k] = ldv_nt(r.xk + i);
        vs[k] = ldv_nt(r.sj + i);
        if constexpr (MASK) { m0[k] = m[E * i]; m1[k] = m[E * i + (E - 1)]; }
      }
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const int64_t i = base + (h * H + k) * 256;
        bool s0 = true, s1 = true;
        if constexpr (MASK) { s0 = m0[k] != 0; s1 = m1[k] != 0; }
        acc = batch_site<Kind, true>(op, acc, r, i, va[k], vd[k], vx[k], vs[k], s0, s1, l, u, sh, shifted);
      }
    }
  } else {  // the last tile of the row
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + k * 256;
      if (i < hi) {
        const V a = r.a[i], b = r.xk[i], c = r.sj[i];
        const V d = load_d<Kind, false>(r.d, i);
        bool s0 = true, s1 = true;
        if constexpr (MASK) { s0 = m[E * i] != 0; s1 = m[E * i + (E - 1)] != 0; }
        acc = batch_site<Kind, false>(op, acc, r, i, a, d, b, c, s0, s1, l, u, sh, shifted);
      }
    }
  }
  return acc;
}
// element i of a row by one lane: the head and the tail of the pairs form
template <class Kind, class Op, bool MASK>
__device__ __forceinline__ SumsFor<Op> batch_element(const Op& op, SumsFor<Op> acc, const BatchRow<double>& r, const uint8_t* mask,
                                                     double l, double u, double sh, bool shifted, int64_t i) {
  bool sel = true;
  if constexpr (MASK) sel = mask[i] != 0;
  const double a = r.a[i], b = r.xk[i], c = r.sj[i];
  const double d = load_d<Kind, false>(r.d, i);
  return batch_site<Kind, false>(op, acc, r, i, a, d, b, c, sel, false, l, u, sh, shifted);
}

// The kernel that stores y.  Grid: `batch` workgroups (row form: TILED = false, a workgroup walks the `tiles` tiles of its
// problem) or tiles * batch (TILED: batch_workgroup).
template <class Kind, class Row, bool TILED, bool PAIRS, bool MASK>
__device__ __forceinline__ void batch_body(const BatchArgs& k) {
  using Op = typename Kind::template Op<Row>;
  constexpr int NS = Kind::kPlan.planes;
  static_assert(kSumsOf<Op> == NS, "one plane per sum of the functor");
  const int64_t tiles = k.tiles;
  int64_t b = blockIdx.x, t0 = 0, t1 = tiles;
  if constexpr (TILED) {
    batch_workgroup(blockIdx.x, tiles, &b, &t0);
    t1 = t0 + 1;
  }
  // the problem's scalars: b is uniform, so these are scalar loads
  const double lam = k.lambda[b];
  bool shifted = false;
  double sh = 0.0;
  if constexpr (Kind::kHasD) {
    shifted = k.dshift != nullptr;
    sh = shifted ? k.dshift[b] : 0.0;
  }
  const Op op = Kind::template make_op<Row, TILED>(k, b, lam);
  double l = 0.0, u = 0.0;
  if constexpr (Row::Op::kBox) { l = k.lo[b]; u = k.up[b]; }
  const int64_t off = b * k.ld, n = k.n;
  const BatchRow<double> row{k.v.y + off, k.v.a + off, Kind::kHasD ? k.v.d + off : nullptr, k.v.xk + off, k.v.sj + off,
                             k.v.xn ? k.v.xn + off : nullptr};
  SumsFor<Op> acc = {};
  if constexpr (PAIRS) {
    const BatchRowMap r = batch_row_map(n, b, k.ld, k.base_odd);
    const uint8_t* const m = MASK ? k.mask + r.head : nullptr;
    const BatchRow<f64x2> prs{reinterpret_cast<f64x2*>(row.y + r.head), reinterpret_cast<const f64x2*>(row.a + r.head),
                              Kind::kHasD ? reinterpret_cast<const f64x2*>(row.d + r.head) : nullptr,
                              reinterpret_cast<const f64x2*>(row.xk + r.head), reinterpret_cast<const f64x2*>(row.sj + r.head),
                              row.xn ? reinterpret_cast<f64x2*>(row.xn + r.head) : nullptr};
    for (int64_t t = t0; t < t1; ++t) acc = batch_tile<Kind, Op, f64x2, MASK, 6>(op, acc, prs, m, l, u, sh, shifted, r.npairs, t);
    if (t0 == 0 && r.head && threadIdx.x == 0) acc = batch_element<Kind, Op, MASK>(op, acc, row, k.mask, l, u, sh, shifted, 0);
    if (t1 == tiles && r.tail && threadIdx.x == 255) acc = batch_element<Kind, Op, MASK>(op, acc, row, k.mask, l, u, sh, shifted, n - 1);
  } else {
    for (int64_t t = t0; t < t1; ++t) acc = batch_tile<Kind, Op, double, MASK, 12>(op, acc, row, k.mask, l, u, sh, shifted, n, t);
  }
  acc = block_sum4(acc);
  if (threadIdx.x == 0) {
    if constexpr (TILED) {
#pragma unroll
      for (int p = 0; p < NS; ++p) k.out[batch_slot(b, p, t0, tiles, NS)] = acc.v[p];
    } else {
      k.out[NS * b] = lam * acc.v[0];
#pragma unroll
      for (int p = 1; p < NS; ++p) k.out[NS * b + p] = acc.v[p];
    }
  }
}
// The reduce of the tiled form: workgroup b adds the NS planes of problem b's partials, `tiles` slots each, in a fixed order --
// the order of the single call's sums on short lists (value_reduce_small), eight loads in flight per lane on long ones -- and
// stores stats[NS b + p]: plane 0 times lambda[b] (SCALE0; the group call's terms carry their own weights: plane 0 as it is,
// lambda unused), the other planes as they are.  Grid: batch.
template <int NS, bool SCALE0 = true>
__device__ __forceinline__ void batch_reduce_body(const double* partials, int64_t tiles, const double* lambda, double* stats) {
  const int64_t b = blockIdx.x;
  const double* const part = partials + batch_slot(b, 0, 0, tiles, NS);
  SepSums<NS> s;
  if (tiles <= kValueFuseMax) {
    s = value_reduce_small<false, NS>(part, tiles, (int)tiles);
  } else {
#pragma unroll
    for (int p = 0; p < NS; ++p) {
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
    if constexpr (SCALE0) stats[NS * b] = lambda[b] * s.v[0];
    else stats[NS * b] = s.v[0];
#pragma unroll
    for (int p = 1; p < NS; ++p) stats[NS * b + p] = s.v[p];
  }
}

// ---------------------------------------------------------------------------------------------
// The host run
// ---------------------------------------------------------------------------------------------
// the operands of a batched call, stated once at the entry point (a: q or g; what a call does not have stays NULL)
struct BatchCall {
  spx_ctx* ctx;
  double* y;
  const double *a, *d, *xk, *sj;
  int64_t n, batch, ld;
  const double* lambda;
  double *xkn, *stats_dev;
  const double *sigma = nullptr, *q_scale = nullptr, *d_shift = nullptr;
  int32_t* d_flag = nullptr;
  const double *l = nullptr, *u = nullptr;
  const uint8_t* mask = nullptr;
};
using BatchReduceKernel = void (*)(const double*, int64_t, const double*, double*);
template <class F>
void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
// Every refusal is made before anything is enqueued.  There is no host destination: the call only enqueues.  The Kind names
// its library (kLibName), refuses its parameter arrays (refuse_params) and aliases (refuse_alias), lists y and its input vectors
// in the order of the alignment bits (inputs), clears the words its functors raise (zero_flags: a kernel node, never a memset
// node), launches its kernel (launch) and names its reduce kernel (kReduce).
template <class Kind, class Row>
int run_batch(const BatchCall& c) {
  constexpr bool kBox = Row::Op::kBox;
  constexpr int NS = Kind::kPlan.planes;
  spx_ctx* const ctx = c.ctx;
  SPX_REQUIRE_SHARED_ABI(Kind::kLibName);
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(c.n >= 0, "n < 0");
  SPX_REQUIRE(c.batch >= 0, "batch < 0");
  if (c.batch == 0) return SPX_OK;
  SPX_REQUIRE(c.stats_dev != nullptr, "stats_dev is NULL");
  if (const int rc = Kind::template refuse_params<Row>(c)) return rc;
  if constexpr (kBox) SPX_REQUIRE(c.l != nullptr && c.u != nullptr, "a bound array (l, u) is NULL");
  SPX_REQUIRE(c.ld >= c.n, "ld < n");
  const auto in = Kind::inputs(c);
  static_assert(std::tuple_size<decltype(in)>::value + 1 == Kind::kPlan.vectors, "y, the inputs and xkn are the kind's vectors");
  if (c.n > 0) {
    for (const void* v : in) SPX_REQUIRE(v != nullptr, "NULL vector with n > 0");
    if (const int rc = Kind::refuse_alias(c)) return rc;
    if (c.xkn != nullptr) {
      for (const void* o : in) SPX_REQUIRE(c.xkn != o, "xkn is one of the other vectors");
      SPX_REQUIRE(c.xkn != (const void*)c.mask, "xkn is one of the other vectors");
    }
  }
  const auto bit3 = [](const void* ptr) { return (int)((reinterpret_cast<uintptr_t>(ptr) >> 3) & 1u); };
  int bits = bit3(c.xkn ? c.xkn : c.y) << in.size();
  for (size_t k = 0; k < in.size(); ++k) bits |= bit3(in[k]) << k;
  const BatchPlan p = batch_plan(c.n, c.batch, c.ld, bits, Kind::kPlan);
  SPX_REQUIRE(p.ok, "the call needs more than 2^31 - 1 workgroups");
  if (c.n == 0) {  // zeros (and clear flag words) for every problem, by a kernel
    SPX_ON_DEVICE(ctx);
    if (const int rz = Kind::template zero_flags<Row>(c)) return rz;
    return spx_zero_async(ctx, c.stats_dev, (size_t)c.batch * NS * sizeof(double));
  }
  const bool tiled = p.form == BatchForm::kTiled;
  if (tiled) {
    const int rcw = spx_ws_reserve(ctx, p.ws_bytes);
    if (rcw) return rcw;
  }
  SPX_ON_DEVICE(ctx);
  if (tiled) {  // (the row form clears its word inside the launch)
    if (const int rz = Kind::template zero_flags<Row>(c)) return rz;
  }
  double* const out = tiled ? reinterpret_cast<double*>(ctx->ws) : c.stats_dev;
  const bool msk = kBox && c.mask != nullptr;
  with_bool(tiled, [&](auto T) {
    with_bool(p.pairs, [&](auto P) {
      with_bool(msk, [&](auto M) {
        if constexpr (kBox || !decltype(M)::value) Kind::template launch<Row, decltype(T)::value, decltype(P)::value, decltype(M)::value>(c, p, out);
      });
    });
  });
  SPX_LAUNCH_CHECK();
  if (tiled) {
    hipLaunchKernelGGL(Kind::kReduce, dim3((unsigned)c.batch), dim3(256), 0, ctx->stream, (const double*)out, p.tiles_per_problem,
                       c.lambda, c.stats_dev);
    SPX_LAUNCH_CHECK();
  }
  return SPX_OK;
}
}  // namespace

// the parameters a Box entry point has between the call's own and q_scale / xkn
#define SPX_BATCH_BOX_PARAMS const double *l, const double *u, const uint8_t *sel_mask,
