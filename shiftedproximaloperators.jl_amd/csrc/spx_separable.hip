// spx_separable.hip -- the six separable prox! kernels (ShiftedNormL1/L0/RootNormLhalf and their Box
// forms) and iprox!, on Float64 and (L1 / L0 forms) Float32 vectors.  One streaming skeleton per precision, one functor
// per operator.
//
// HBM layout: q, xk, sj, y (and l, u when they are vectors) are plain contiguous fp64 vectors.
// Algorithmic traffic: 3 reads + 1 write = 32 B/element (48 B with vector bounds, +1 B with a mask).
// Roofline: HBM bandwidth (no reuse, no contraction -> MFMA not applicable).
//
// Skeleton: a workgroup of 256 lanes walks tiles of 256*UNROLL 16-byte pairs with a block stride.
// Within a tile every wave instruction touches 1 KiB contiguous (lane i -> base + 16*i), all
// 3*UNROLL loads of a tile are issued before the first use so each lane keeps 3*UNROLL*16 B in
// flight, results are written with 16-byte stores.  q[i] is read before y[i] is written by the same
// lane and no other lane touches index i, so y may alias q.
#include "spx_sep_device.hpp"  // the operators, the element site, the block sums, the operator table

// n2 = number of 16-byte pairs.  VECB: l/u are vectors.  MASK: sel mask present.
template <class Op, int UNROLL, bool VECB, bool MASK, bool NT>
__global__ __launch_bounds__(256) void k_sep_vec(double* y_, const double* q_, const double* d_, const double* xk_,
                                                  const double* sj_, const double* l_, const double* u_,
                                                  const uint8_t* mask_, double ls, double us, int64_t n2, Op op) {
  const f64x2* dv = reinterpret_cast<const f64x2*>(d_);
  constexpr int64_t TILE = 256 * UNROLL;
  f64x2* y = reinterpret_cast<f64x2*>(y_);
  const f64x2* q = reinterpret_cast<const f64x2*>(q_);
  const f64x2* xk = reinterpret_cast<const f64x2*>(xk_);
  const f64x2* sj = reinterpret_cast<const f64x2*>(sj_);
  const f64x2* lv = reinterpret_cast<const f64x2*>(l_);
  const f64x2* uv = reinterpret_cast<const f64x2*>(u_);
  const uint16_t* mk = reinterpret_cast<const uint16_t*>(mask_);
  const int64_t ntiles = (n2 + TILE - 1) / TILE;
  SumsFor<Op> acc = {};
  f64x2* const xn = xkn_of<f64x2>(op);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * TILE + threadIdx.x;
    f64x2 vq[UNROLL], vx[UNROLL], vs[UNROLL], vl[UNROLL], vu[UNROLL], vd[UNROLL];
    uint16_t vm[UNROLL];
    if (base - threadIdx.x + TILE <= n2) {
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t i = base + k * 256;
        vq[k] = ld2<NT>(q + i);
        if constexpr (Op::kNIn == 4) vd[k] = ld2<NT>(dv + i); else vd[k] = f64x2{0.0, 0.0};
        vx[k] = ld2<NT>(xk + i);
        vs[k] = ld2<NT>(sj + i);
        if constexpr (VECB && Op::kBox) {
          vl[k] = l_ ? ld2<NT>(lv + i) : f64x2{ls, ls};
          vu[k] = u_ ? ld2<NT>(uv + i) : f64x2{us, us};
        }
        if constexpr (MASK && Op::kBox) vm[k] = mk[i];
      }
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t i = base + k * 256;
        double l0 = ls, l1 = ls, u0 = us, u1 = us;
        bool s0 = true, s1 = true;
        if constexpr (VECB && Op::kBox) { l0 = vl[k].x; l1 = vl[k].y; u0 = vu[k].x; u1 = vu[k].y; }
        if constexpr (MASK && Op::kBox) { s0 = (vm[k] & 0xff) != 0; s1 = (vm[k] >> 8) != 0; }
        f64x2 r;
        r.x = apply_op(op, vq[k].x, vd[k].x, vx[k].x, vs[k].x, l0, u0, s0);
        r.y = apply_op(op, vq[k].y, vd[k].y, vx[k].y, vs[k].y, l1, u1, s1);
        acc = sep_accumulate<NT>(op, acc, vq[k], vd[k], vx[k], vs[k], r, s0, s1, xn, i);
        st2<NT>(y + i, r);
      }
    } else {  // last, partial tile
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) {
        const int64_t i = base + k * 256;
        if (i < n2) {
          f64x2 a = q[i], b = xk[i], c = sj[i];
          f64x2 dd = f64x2{0.0, 0.0};
          if constexpr (Op::kNIn == 4) dd = dv[i];
          double l0 = ls, l1 = ls, u0 = us, u1 = us;
          bool s0 = true, s1 = true;
          if constexpr (VECB && Op::kBox) {
            if (l_) { f64x2 t = lv[i]; l0 = t.x; l1 = t.y; }
            if (u_) { f64x2 t = uv[i]; u0 = t.x; u1 = t.y; }
          }
          if constexpr (MASK && Op::kBox) { uint16_t m = mk[i]; s0 = (m & 0xff) != 0; s1 = (m >> 8) != 0; }
          f64x2 r;
          r.x = apply_op(op, a.x, dd.x, b.x, c.x, l0, u0, s0);
          r.y = apply_op(op, a.y, dd.y, b.y, c.y, l1, u1, s1);
          acc = sep_accumulate<false>(op, acc, a, dd, b, c, r, s0, s1, xn, i);
          y[i] = r;
        }
      }
    }
  }
  if constexpr (kSumsOf<Op> > 0) value_publish(op, blockIdx.x, block_sum4(acc));
}

// ---------------------------------------------------------------------------------------------
// LDS-staged skeleton (the default): each wavefront owns a contiguous chunk of UNROLL KiB per input vector and
// stages it through LDS with `global_load_lds_dwordx4 ... nt` -- LDS-DMA: no VGPR destination, one contiguous
// 1 KiB piece per wave instruction -- then waits once (vmcnt(0)), reads its own 16 bytes per piece back with
// ds_read_b128 (lane-private slots: conflict-free, no barrier: nothing is shared between waves), evaluates
// the operator and writes y with non-temporal 16-byte stores.  3*UNROLL KiB are in flight per wave without
// holding registers; UNROLL = 6 -> 72 KiB of LDS per 4-wave workgroup -> two workgroups (144 KiB in flight)
// per CU.  Measured on MI355X (tools/exp/exp_stream.hip, n = 1e8, same process, interleaved rounds):
// 6.45-6.57 TB/s against 6.11-6.30 TB/s for the register-staged form above; 7 KiB per wave and more (one
// workgroup per CU) or a piece-by-piece pipelined wait lose 10-20 %.
// All loads of a wave have landed before its first store, and waves touch disjoint ranges: y may alias q.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ void dma16_nt(const f64x2* g, char* wave_lds_piece) {
  __builtin_amdgcn_global_load_lds((const void*)g, (lds_void*)wave_lds_piece, 16, 0, 2);  // aux = 2: nt
}

template <class Op, int UNROLL, bool VECB, bool MASK>
__global__ __launch_bounds__(256) void k_sep_lds(double* y_, const double* q_, const double* d_, const double* xk_,
                                                  const double* sj_, const double* l_, const double* u_,
                                                  const uint8_t* mask_, double ls, double us, int64_t n2, Op op,
                                                  int64_t xcd_chunk) {
  constexpr int NARR = Op::kNIn + ((VECB && Op::kBox) ? 2 : 0);
  const f64x2* dv = reinterpret_cast<const f64x2*>(d_);
  __shared__ __attribute__((aligned(16))) char lds[4 * NARR * UNROLL * 1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  char* wl = lds + wave * (NARR * UNROLL * 1024);
  f64x2* y = reinterpret_cast<f64x2*>(y_);
  const f64x2* q = reinterpret_cast<const f64x2*>(q_);
  const f64x2* xk = reinterpret_cast<const f64x2*>(xk_);
  const f64x2* sj = reinterpret_cast<const f64x2*>(sj_);
  const f64x2* lv = reinterpret_cast<const f64x2*>(l_);
  const f64x2* uv = reinterpret_cast<const f64x2*>(u_);
  const uint16_t* mk = reinterpret_cast<const uint16_t*>(mask_);
  // Workgroups are dealt to the 8 XCDs round-robin.  xcd_chunk == 0 (default): tile = workgroup id, so neighbouring tiles
  // land on different XCDs; xcd_chunk > 0 (spx_ctx_set_tuning key 5, experiment): XCD x works through the contiguous range
  // [x * xcd_chunk, (x + 1) * xcd_chunk) of tiles.  No tile is ever re-read, so neither L2 has anything to win -- measured.
  int64_t bid = blockIdx.x;
  if (xcd_chunk > 0) {
    bid = (int64_t)(blockIdx.x & 7) * xcd_chunk + (blockIdx.x >> 3);
    if (bid * (256 * UNROLL) >= n2) {
      if constexpr (kSumsOf<Op> > 0) {
        value_store(op, bid, SumsFor<Op>{});  // (a slot of its own: every slot the host counts is written; never the one-launch form)
      }
      return;
    }
  }
  const int64_t base = (bid * 4 + wave) * (64 * UNROLL) + lane;  // this lane's first pair
  SumsFor<Op> acc = {};
  f64x2* const xn = xkn_of<f64x2>(op);
  uint16_t vm[UNROLL];
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    int64_t i = base + k * 64;
    if (i >= n2) i = n2 - 1;  // tail: load something valid, the store is guarded
    dma16_nt(q + i, wl + (0 * UNROLL + k) * 1024);
    dma16_nt(xk + i, wl + (1 * UNROLL + k) * 1024);
    dma16_nt(sj + i, wl + (2 * UNROLL + k) * 1024);
    if constexpr (Op::kNIn == 4) dma16_nt(dv + i, wl + (3 * UNROLL + k) * 1024);
    if constexpr (VECB && Op::kBox) {
      if (l_) dma16_nt(lv + i, wl + ((Op::kNIn + 0) * UNROLL + k) * 1024);
      if (u_) dma16_nt(uv + i, wl + ((Op::kNIn + 1) * UNROLL + k) * 1024);
    }
    if constexpr (MASK && Op::kBox) vm[k] = mk[i];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every piece of this wave has landed in LDS
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int64_t i = base + k * 64;
    const f64x2 a = *reinterpret_cast<const f64x2*>(wl + (0 * UNROLL + k) * 1024 + lane * 16);
    const f64x2 b = *reinterpret_cast<const f64x2*>(wl + (1 * UNROLL + k) * 1024 + lane * 16);
    const f64x2 c = *reinterpret_cast<const f64x2*>(wl + (2 * UNROLL + k) * 1024 + lane * 16);
    double l0 = ls, l1 = ls, u0 = us, u1 = us;
    bool s0 = true, s1 = true;
    f64x2 dd = f64x2{0.0, 0.0};
    if constexpr (Op::kNIn == 4) dd = *reinterpret_cast<const f64x2*>(wl + (3 * UNROLL + k) * 1024 + lane * 16);
    if constexpr (VECB && Op::kBox) {
      if (l_) { const f64x2 t = *reinterpret_cast<const f64x2*>(wl + ((Op::kNIn + 0) * UNROLL + k) * 1024 + lane * 16); l0 = t.x; l1 = t.y; }
      if (u_) { const f64x2 t = *reinterpret_cast<const f64x2*>(wl + ((Op::kNIn + 1) * UNROLL + k) * 1024 + lane * 16); u0 = t.x; u1 = t.y; }
    }
    if constexpr (MASK && Op::kBox) { s0 = (vm[k] & 0xff) != 0; s1 = (vm[k] >> 8) != 0; }
    f64x2 r;
    r.x = apply_op(op, a.x, dd.x, b.x, c.x, l0, u0, s0);
    r.y = apply_op(op, a.y, dd.y, b.y, c.y, l1, u1, s1);
    if constexpr (kSumsOf<Op> > 0) {  // (the tail's lanes hold a copy of the last pair)
      if (i < n2) acc = sep_accumulate<true>(op, acc, a, dd, b, c, r, s0, s1, xn, i);  // (xkn out of registers: the extra store needs no LDS)
    }
    if (i < n2) __builtin_nontemporal_store(r, y + i);
  }
  // one slot per WORKGROUP (one per wavefront meant 130 208 of them at n = 1e8, and ~25 us of ordered reduction behind the pass)
  if constexpr (kSumsOf<Op> > 0) value_publish(op, bid, block_sum4_staged(acc, wl, lds, NARR * UNROLL * 1024));
}

// scalar path: unaligned vectors, and the odd last element of the vector path ([begin, n))
template <class Op>
__global__ __launch_bounds__(256) void k_sep_scalar(double* y, const double* q, const double* d_, const double* xk,
                                                     const double* sj, const double* l_, const double* u_,
                                                     const uint8_t* mask, double ls, double us, int64_t begin,
                                                     int64_t n, Op op) {
  int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  SumsFor<Op> acc = {};
  double* const xn = xkn_of<double>(op);  // (indexed from element 0)
  for (; i < n; i += stride) {
    double li = l_ ? l_[i] : ls;
    double ui = u_ ? u_[i] : us;
    bool sel = mask ? (mask[i] != 0) : true;
    double di = 0.0;
    if constexpr (Op::kNIn == 4) di = d_[i];
    const double xi = xk[i], si = sj[i];
    const double qi = q[i];
    const double yi = apply_op(op, qi, di, xi, si, li, ui, sel);
    acc = sep_accumulate<false>(op, acc, qi, di, xi, si, yi, sel, false, xn, i);
    y[i] = yi;
  }
  if constexpr (kSumsOf<Op> > 0) value_store(op, blockIdx.x, block_sum4(acc));  // (never the only launch of a call)
}

// Tuning knobs (spx_ctx_set_tuning).  Defaults from tools/sweep_sep.py on MI355X, n = 1e8 (profiles/r01_sweep_sep.txt):
// one tile per workgroup (no cap) + non-temporal loads/stores: 6.15 TB/s vs 5.66 TB/s for 16 WG/CU, plain.
// (the knobs live in the context: spx_ctx::tune_sep_*, set by spx_ctx_set_tuning)

#ifndef SPX_VECB_KIB
#define SPX_VECB_KIB 3  // KiB per wave and vector with vector bounds (5 vectors); measured at n = 1e8 (tools/bench_vecb.py): 2 -> 0.81 ms, 3 -> 0.76 ms, 4 -> 0.775 ms
#endif
template <class Op, bool VECB, bool MASK>
static int launch_vec(const SepCall<double>& c /* at its 16-byte aligned body */, int64_t n2, Op op,
                      int64_t* value_slots /* out: partial slots written (kSumsOf<Op> > 0) */,
                      const SpxSyncHeader* fuse_hdr = nullptr /* kSumsOf<Op> > 0: this launch is the whole call -- it may finish the sums itself */,
                      bool* fused = nullptr) {
  spx_ctx* const ctx = c.ctx;
  const SpxBox<double>& b = c.box;
  // (kSumsOf<Op> > 0) the one-launch form: the grid is the list of slots, short enough for one workgroup to add
  auto try_fuse = [&](int64_t blocks) {
    if constexpr (kSumsOf<Op> > 0) {
      if (fuse_hdr != nullptr && blocks <= kValueFuseMax && !ctx->tune_sep_xcd) {
        op.fin_hdr = const_cast<SpxSyncHeader*>(fuse_hdr);
        *fused = true;
      }
    }
  };
  if constexpr (Op::kLdsKiB > 0) if (ctx->tune_sep_lds) {
    // 3 input vectors: 6 KiB per wave and vector -> 72 KiB per workgroup; 5 vectors (vector bounds): 3 KiB -> 60 KiB
    constexpr int U = (VECB && Op::kBox) ? (Op::kLdsKiB > SPX_VECB_KIB ? SPX_VECB_KIB : Op::kLdsKiB) : Op::kLdsKiB;  // <= 72 KiB per workgroup
    int64_t blocks = (n2 + 256 * U - 1) / (256 * U);
    int64_t xcd_chunk = 0;
    if (ctx->tune_sep_xcd) {
      xcd_chunk = (blocks + 7) / 8;
      blocks = xcd_chunk * 8;
    }
    *value_slots = blocks;  // one per workgroup (idle workgroups of the XCD-contiguous experiment write a zero)
    try_fuse(blocks);
    hipLaunchKernelGGL((k_sep_lds<Op, U, VECB, MASK>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.d, c.xk,
                       c.sj, b.l, b.u, b.mask, b.ls, b.us, n2, op, xcd_chunk);
    SPX_LAUNCH_CHECK();
    return SPX_OK;
  }
  constexpr int UNROLL = 4;
  const int64_t ntiles = (n2 + 256 * UNROLL - 1) / (256 * UNROLL);
  int64_t blocks = ntiles;
  const int64_t cap = ctx->tune_sep_blocks_per_cu > 0 ? (int64_t)ctx->num_cu * ctx->tune_sep_blocks_per_cu : (int64_t)0x7fffffff;
  if (blocks > cap) blocks = cap;
  *value_slots = blocks;  // one per workgroup
  try_fuse(blocks);
  if (ctx->tune_sep_nt)
    hipLaunchKernelGGL((k_sep_vec<Op, UNROLL, VECB, MASK, true>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y,
                       c.q, c.d, c.xk, c.sj, b.l, b.u, b.mask, b.ls, b.us, n2, op);
  else
    hipLaunchKernelGGL((k_sep_vec<Op, UNROLL, VECB, MASK, false>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       c.y, c.q, c.d, c.xk, c.sj, b.l, b.u, b.mask, b.ls, b.us, n2, op);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}

// The workspace of a call with sums: [NS result doubles | kSepFlagOffset: the d > 0 flag word of spx_iproxstep_* | pad to 256 B
// | NS planes of partial slots].  sep_plane: doubles per plane, at least the slots of any route.
constexpr size_t kSepFlagOffset = 128;
static int64_t sep_plane(const spx_ctx* ctx, int64_t n) { return ((n / 2) / (256 * 3) + 2) * 4 + 2 * (int64_t)ctx->num_cu * 8 + 16; }
static size_t sep_ws_bytes(const spx_ctx* ctx, int64_t n, int ns) { return 256 + (size_t)ns * (size_t)sep_plane(ctx, n) * sizeof(double); }
// kSumsOf<Op> > 0: the sums {value_scale * h, <q, y>, <y, y>} (WithValue: the first of them; WithIstep: the four) go to the library's result slots,
// to dest.dev (device doubles, or NULL) and, when dest.host != NULL, back to the host -- that form synchronises and is
// refused under a capture; those callers answer n == 0 themselves.
template <class Op>
static int run_separable(const SepCall<double>& c, Op op, const SpxDest& dest = {nullptr, nullptr, 0}, double value_scale = 1.0) {
  constexpr int NS = kSumsOf<Op>;
  spx_ctx* const ctx = c.ctx;
  const int64_t n = c.n;
  if (n == 0) return SPX_OK;
  SPX_ON_DEVICE(ctx);
  double* partials = nullptr;  // ws: [results | pad to 256 B | NS planes of partial slots]
  int64_t used = 0, plane = 0;
  if constexpr (NS > 0) {
    plane = sep_plane(ctx, n);
    int rcw = spx_ws_reserve(ctx, sep_ws_bytes(ctx, n, NS));
    if (rcw) return rcw;
    partials = reinterpret_cast<double*>(static_cast<char*>(ctx->ws) + 256);
    if constexpr (NS > 1) op.plane = plane;
    if (ctx->tune_fewer_launches) {  // (the one-launch form keeps its tickets in the synchronisation state)
      rcw = spx_sync_ready(ctx);
      if (rcw) return rcw;
    }
  }
  bool fused = false;
  auto launch_scalar = [&](int64_t begin, int64_t end) -> int {
    int64_t blocks = (end - begin + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    if constexpr (NS > 0) op.partials = partials + used;
    if constexpr (NS >= 3) op.xkn = c.xkn;  // (indexed from element 0)
    hipLaunchKernelGGL((k_sep_scalar<Op>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.d, c.xk, c.sj, c.box.l,
                       c.box.u, c.box.mask, c.box.ls, c.box.us, begin, end, op);
    SPX_LAUNCH_CHECK();
    used += blocks;
    return SPX_OK;
  };
  // The vector skeletons need 16-byte aligned vectors (and a 2-byte aligned mask).  Views that all start 8 bytes off
  // (e.g. view(x, 2:n) of aligned arrays) are peeled: element 0 through the scalar kernel, the rest aligned again.
  int64_t head = 0;
  if (!c.aligned16_at(0) && n >= 3 && c.aligned16_at(1)) head = 1;
  int64_t done = 0;
  if (head) {
    int rch = launch_scalar(0, head);
    if (rch) return rch;
    done = head;
  }
  if (c.aligned16_at(head) && n - head >= 2) {
    const int64_t n2 = (n - head) / 2;
    const SepCall<double> v = c.shifted(head);
    int rc;
    int64_t slots = 0;
    const SpxSyncHeader* fh = nullptr;
    if constexpr (NS > 0) {
      op.partials = partials + used;
      // one launch covers the whole vector (no peeled element in front, no odd element behind): it may finish the sums
      if (ctx->tune_fewer_launches && head == 0 && 2 * n2 == n) {
        fh = spx_sync_header(ctx);
        op.fin_result = reinterpret_cast<double*>(ctx->ws);
        op.fin_target = dest.dev;
        op.fin_scale = value_scale;
      }
    }
    if constexpr (NS >= 3) op.xkn = v.xkn;
    if constexpr (Op::kBox) {
      const bool vecb = (v.box.l || v.box.u);
      const bool msk = (v.box.mask != nullptr);
      if (vecb && msk) rc = launch_vec<Op, true, true>(v, n2, op, &slots, fh, &fused);
      else if (vecb) rc = launch_vec<Op, true, false>(v, n2, op, &slots, fh, &fused);
      else if (msk) rc = launch_vec<Op, false, true>(v, n2, op, &slots, fh, &fused);
      else rc = launch_vec<Op, false, false>(v, n2, op, &slots, fh, &fused);
    } else {
      rc = launch_vec<Op, false, false>(v, n2, op, &slots, fh, &fused);
    }
    if (rc) return rc;
    used += slots;
    done = head + 2 * n2;
  }
  if (done < n) {
    int rct = launch_scalar(done, n);
    if (rct) return rct;
  }
  if constexpr (NS > 0) {
    double* result = reinterpret_cast<double*>(ctx->ws);
    if (!fused) {
      hipLaunchKernelGGL(k_value_reduce<NS>, dim3(NS), dim3(1024), 0, ctx->stream, (const double*)partials, plane, used, result,
                         value_scale, dest.dev);
      SPX_LAUNCH_CHECK();
    }
    const int rcc = spx_dest_check_capture(ctx, dest, NS == 1 ? "returning the value of prox_value to the host"
                                                              : "returning the step statistics to the host (pass stats = NULL)");
    if (rcc) return rcc;
    return spx_dest_return(ctx, dest, result, NS * sizeof(double));
  }
  return SPX_OK;
}

namespace {
// ... which holds for lambda * sigma >= 0 (see ProxL1Aliased).  The Float32 form takes it for any lambda, and not at n == 0.
bool l1_aliased(const SepCall<double>& c, double lambda, double sigma) { return c.y == c.q && lambda * sigma >= 0.0; }
bool l1_aliased(const SepCall<float>& c, float, float) { return c.y == c.q && c.n > 0; }
}  // namespace

template <class Row>
static int run_prox(const SepCall<double>& c, double lambda, double sigma) {
  const int rc = spx_check_common(c);
  if (rc) return rc;
  return run_separable(c, Row::template make<typename Row::Op>(lambda, sigma));
}

// ---------------------------------------------------------------------------------------------
// prox! + value of h at the result, in one pass (synchronous: *value is written on the host)
// ---------------------------------------------------------------------------------------------
template <class Row>
static int run_proxval(const SepCall<double>& c, double lambda, double sigma, double q_scale, double* value) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  SPX_REQUIRE(value != nullptr, "value is NULL");
  WithValue<typename Row::Op, typename Row::Term> op{Row::template make<typename Row::Op>(lambda, sigma), nullptr, q_scale};
  *value = lambda * 0.0;  // (n == 0, or an error: -0.0 for a negative lambda, NaN for a non-finite one)
  const SpxDest dest = spx_value_dest(c.ctx, value);
  if (c.n == 0) return spx_dest_empty(c.ctx, {nullptr, dest.dev, 1});  // (the device side only: the host keeps lambda * 0)
  rc = run_separable(c, op, dest, lambda);
  spx_value_nan_on_device(rc, dest, false, value);
  return rc;
}

// ---------------------------------------------------------------------------------------------
// prox! + step statistics in one pass (spx_proxstep_*): y, xkn = (xk + sj) + y, and {h, <q, y>, <y, y>} to a host double[3]
// (synchronous) and / or a device double[3] (enqueue only).  Float64, device pointers, the six separable operators.
// ---------------------------------------------------------------------------------------------
template <class Row>
static int run_proxstep(const SepCall<double>& c, double lambda, double sigma, double q_scale, const SpxDest& dest) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  rc = spx_step_begin(c.ctx, dest, false, c.y, {c.q}, kSpxYAliasesQ, c.xkn, c.others());
  if (rc) return rc;
  if (c.n == 0) return spx_dest_empty(c.ctx, dest);
  WithStep<typename Row::Op, typename Row::Term> op{};
  static_cast<typename Row::Op&>(op) = Row::template make<typename Row::Op>(lambda, sigma);
  op.qscale = q_scale;
  return run_separable(c, op, dest, lambda);
}

// ---------------------------------------------------------------------------------------------
// C entry points (Float64 prox!): each builds the call {ctx, y, q, d, xk, sj, n, box, xkn} from its arguments
// ---------------------------------------------------------------------------------------------
#define SPX_BOX_OF(T) SpxBox<T>{l_vec, u_vec, l_scalar, u_scalar, sel_mask}
SPX_EXPORT int spx_prox_l1(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                           double lambda, double sigma) {
  const SepCall<double> c{ctx, y, q, nullptr, xk, sj, n, {}, nullptr};
  return l1_aliased(c, lambda, sigma) ? run_prox<RowL1Aliased>(c, lambda, sigma) : run_prox<RowL1>(c, lambda, sigma);
}
SPX_EXPORT int spx_proxval_l1(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                              double lambda, double sigma, double q_scale, double* value) {
  const SepCall<double> c{ctx, y, q, nullptr, xk, sj, n, {}, nullptr};
  if (!l1_aliased(c, lambda, sigma)) return run_proxval<RowL1>(c, lambda, sigma, q_scale, value);
  SPX_REQUIRE(q_scale == 1.0, "q_scale != 1 with y aliasing q");  // (ahead of every other check)
  return run_proxval<RowL1Aliased>(c, lambda, sigma, 1.0, value);
}
SPX_EXPORT int spx_proxstep_l1(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                               double lambda, double sigma, double q_scale, double* xkn, double* stats, double* stats_dev) {
  return run_proxstep<RowL1>({ctx, y, q, nullptr, xk, sj, n, {}, xkn}, lambda, sigma, q_scale, {stats, stats_dev, 3});
}
#define SPX_PROX3(PROX, PROXVAL, PROXSTEP, ROW)                                                                                \
  SPX_EXPORT int PROX(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, double lambda, \
                      double sigma) {                                                                                         \
    return run_prox<ROW>({ctx, y, q, nullptr, xk, sj, n, {}, nullptr}, lambda, sigma);                                         \
  }                                                                                                                            \
  SPX_EXPORT int PROXVAL(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,             \
                         double lambda, double sigma, double q_scale, double* value) {                                        \
    return run_proxval<ROW>({ctx, y, q, nullptr, xk, sj, n, {}, nullptr}, lambda, sigma, q_scale, value);                      \
  }                                                                                                                            \
  SPX_EXPORT int PROXSTEP(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,            \
                          double lambda, double sigma, double q_scale, double* xkn, double* stats, double* stats_dev) {       \
    return run_proxstep<ROW>({ctx, y, q, nullptr, xk, sj, n, {}, xkn}, lambda, sigma, q_scale, {stats, stats_dev, 3});         \
  }
SPX_PROX3(spx_prox_l0, spx_proxval_l0, spx_proxstep_l0, RowL0)
SPX_PROX3(spx_prox_lhalf, spx_proxval_lhalf, spx_proxstep_lhalf, RowLhalf)
#define SPX_PROX3_BOX(PROX, PROXVAL, PROXSTEP, ROW)                                                                            \
  SPX_EXPORT int PROX(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, double lambda, \
                      double sigma, const double* l_vec, const double* u_vec, double l_scalar, double u_scalar,              \
                      const uint8_t* sel_mask) {                                                                              \
    return run_prox<ROW>({ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(double), nullptr}, lambda, sigma);                         \
  }                                                                                                                            \
  SPX_EXPORT int PROXVAL(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,             \
                         double lambda, double sigma, const double* l_vec, const double* u_vec, double l_scalar,             \
                         double u_scalar, const uint8_t* sel_mask, double q_scale, double* value) {                           \
    return run_proxval<ROW>({ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(double), nullptr}, lambda, sigma, q_scale, value);      \
  }                                                                                                                            \
  SPX_EXPORT int PROXSTEP(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,            \
                          double lambda, double sigma, const double* l_vec, const double* u_vec, double l_scalar,            \
                          double u_scalar, const uint8_t* sel_mask, double q_scale, double* xkn, double* stats,               \
                          double* stats_dev) {                                                                                \
    return run_proxstep<ROW>({ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(double), xkn}, lambda, sigma, q_scale,                 \
                             {stats, stats_dev, 3});                                                                          \
  }
SPX_PROX3_BOX(spx_prox_l1_box, spx_proxval_l1_box, spx_proxstep_l1_box, RowL1Box)
SPX_PROX3_BOX(spx_prox_l0_box, spx_proxval_l0_box, spx_proxstep_l0_box, RowL0Box)
SPX_PROX3_BOX(spx_prox_lhalf_box, spx_proxval_lhalf_box, spx_proxstep_lhalf_box, RowLhalfBox)

// ---------------------------------------------------------------------------------------------
// Float32 vectors.  The reference's structs and prox! / iprox! methods are generic in R <: Real (src/shiftedNormL1Box.jl:89-94:
// `y::AbstractVector{R}, psi::ShiftedNormL1Box{R, ...}, q::AbstractVector{R}, sigma::R`) and its tests build Float32
// operators on views (test/runtests.jl:196-209): the L1 / L0 bodies above with T = float.  (RootNormLhalf is NOT here: its
// body mixes Float64 literals -- `^(-3 / 2)`, `54^(1 / 3)` -- into the Float32 data, i.e. the reference itself computes it in
// Float64 and rounds; the fp64 entry points cover that after a conversion by the caller.)
//
// HBM: 16 B/element (read q, xk, sj, write y; +8 with vector bounds, +1 with a mask) -- half the bytes of the fp64 path.
// Skeleton: one tile of 256 lanes x 4 x (4 floats = 16 bytes) per workgroup, all 12 non-temporal 16-byte loads of a lane
// issued before first use, 16-byte non-temporal stores.  Views that start at any element (4-byte granularity) are
// peeled to a 16-byte boundary when all vectors share the misalignment; mixed alignments take 4-byte accesses.
// y === q is safe (a lane reads q[i] before it writes y[i]; lanes own disjoint indices).
// ---------------------------------------------------------------------------------------------
namespace {  // (the Float32 functors F32*: next to the operator table above)

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kF32U = 4;                       // 16-byte groups per lane and vector
constexpr int kF32Tile = 256 * kF32U;          // 16-byte groups per workgroup

// body: `n4` groups of 4 floats starting at the (16-byte aligned) pointers; head: `head` (< 4) elements in front of them
// (at [-head .. -1]) and tail: `tail` (< 4) elements behind them, taken by single lanes of workgroup 0.
template <class Op, bool VECB, bool MASK>
__global__ __launch_bounds__(256) void k_sep_f32(float* y_, const float* q_, const float* d_, const float* xk_, const float* sj_,
                                                  const float* l_, const float* u_, const uint8_t* mask, float ls,
                                                  float us, int64_t n4, int head, int tail, Op op) {
  f32x4* y = reinterpret_cast<f32x4*>(y_);
  const f32x4* q = reinterpret_cast<const f32x4*>(q_);
  const f32x4* xk = reinterpret_cast<const f32x4*>(xk_);
  const f32x4* sj = reinterpret_cast<const f32x4*>(sj_);
  const f32x4* lv = reinterpret_cast<const f32x4*>(l_);
  const f32x4* uv = reinterpret_cast<const f32x4*>(u_);
  const f32x4* dv = reinterpret_cast<const f32x4*>(d_);
  const int64_t base = (int64_t)blockIdx.x * kF32Tile + threadIdx.x;
  f32x4 a[kF32U], b[kF32U], c[kF32U], lo[kF32U], up[kF32U], dd[kF32U];
#pragma unroll
  for (int k = 0; k < kF32U; ++k) {
    int64_t i = base + k * 256;
    if (i >= n4) i = n4 > 0 ? n4 - 1 : 0;
    if (n4 > 0) {
      a[k] = __builtin_nontemporal_load(q + i);
      b[k] = __builtin_nontemporal_load(xk + i);
      c[k] = __builtin_nontemporal_load(sj + i);
      if constexpr (Op::kNIn == 4) dd[k] = __builtin_nontemporal_load(dv + i);
      if constexpr (VECB && Op::kBox) {
        lo[k] = l_ ? __builtin_nontemporal_load(lv + i) : f32x4{ls, ls, ls, ls};
        up[k] = u_ ? __builtin_nontemporal_load(uv + i) : f32x4{us, us, us, us};
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kF32U; ++k) {
    const int64_t i = base + k * 256;
    if (i < n4) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float l1 = ls, u1 = us;
        if constexpr (VECB && Op::kBox) { l1 = lo[k][e]; u1 = up[k][e]; }
        bool sel = true;
        if constexpr (MASK && Op::kBox) sel = mask[4 * i + e] != 0;
        float d1 = 0.0f;
        if constexpr (Op::kNIn == 4) d1 = dd[k][e];
        o[e] = apply_op(op, a[k][e], d1, b[k][e], c[k][e], l1, u1, sel);
      }
      __builtin_nontemporal_store(o, y + i);
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {  // the few elements outside the aligned body
    const int64_t i = ((int)threadIdx.x < head) ? (int64_t)threadIdx.x - head : 4 * n4 + ((int)threadIdx.x - head);
    float l1 = ls, u1 = us;
    if constexpr (Op::kBox) {
      if (l_) l1 = l_[i];
      if (u_) u1 = u_[i];
    }
    bool sel = true;
    if constexpr (MASK && Op::kBox) sel = mask[i] != 0;
    float d1 = 0.0f;
    if constexpr (Op::kNIn == 4) d1 = d_[i];
    y_[i] = apply_op(op, q_[i], d1, xk_[i], sj_[i], l1, u1, sel);
  }
}

// mixed alignments: 4-byte accesses
template <class Op>
__global__ __launch_bounds__(256) void k_sep_f32_scalar(float* y, const float* q, const float* d, const float* xk, const float* sj,
                                                         const float* l, const float* u, const uint8_t* mask, float ls,
                                                         float us, int64_t n, Op op) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float l1 = ls, u1 = us;
    bool sel = true;
    if constexpr (Op::kBox) {
      if (l) l1 = l[i];
      if (u) u1 = u[i];
      if (mask) sel = mask[i] != 0;
    }
    float d1 = 0.0f;
    if constexpr (Op::kNIn == 4) d1 = d[i];
    y[i] = apply_op(op, q[i], d1, xk[i], sj[i], l1, u1, sel);
  }
}

// v: the call at its aligned body
template <class Op, bool VECB, bool MK>
void launch_f32(const SepCall<float>& v, dim3 grid, int64_t n4, int head, int tail, Op op) {
  hipLaunchKernelGGL((k_sep_f32<Op, VECB, MK>), grid, dim3(256), 0, v.ctx->stream, v.y, v.q, v.d, v.xk, v.sj, v.box.l, v.box.u,
                     v.box.mask, v.box.ls, v.box.us, n4, head, tail, op);
}
template <class Op>
int run_f32(const SepCall<float>& c, Op op) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  spx_ctx* const ctx = c.ctx;
  const int64_t n = c.n;
  if (n == 0) return SPX_OK;
  SPX_ON_DEVICE(ctx);
  if (!c.same_misalignment(Op::kBox)) {
    int64_t blocks = (n + 255) / 256;
    const int64_t cap = (int64_t)ctx->num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((k_sep_f32_scalar<Op>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.d, c.xk, c.sj,
                       c.box.l, c.box.u, c.box.mask, c.box.ls, c.box.us, n, op);
    SPX_LAUNCH_CHECK();
    return SPX_OK;
  }
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(c.y) & 15u);
  int head = (int)(((16u - m) / 4u) & 3u);
  if (head > n) head = (int)n;
  const int64_t n4 = (n - head) / 4;
  const int tail = (int)(n - head - 4 * n4);
  int64_t blocks = (n4 + kF32Tile - 1) / kF32Tile;
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks);
  const bool vecb = Op::kBox && (c.box.l || c.box.u);
  const bool msk = Op::kBox && c.box.mask != nullptr;
  const SepCall<float> v = c.shifted(head);
  if (vecb && msk) launch_f32<Op, true, true>(v, grid, n4, head, tail, op);
  else if (vecb) launch_f32<Op, true, false>(v, grid, n4, head, tail, op);
  else if (msk) launch_f32<Op, false, true>(v, grid, n4, head, tail, op);
  else launch_f32<Op, false, false>(v, grid, n4, head, tail, op);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}
template <class Row>
int run_prox(const SepCall<float>& c, float lambda, float sigma) {
  return run_f32(c, Row::template make<typename Row::F32>(lambda, sigma));
}

}  // namespace

SPX_EXPORT int spx_prox_l1_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                               float lambda, float sigma) {
  const SepCall<float> c{ctx, y, q, nullptr, xk, sj, n, {}, nullptr};
  return l1_aliased(c, lambda, sigma) ? run_prox<RowL1Aliased>(c, lambda, sigma) : run_prox<RowL1>(c, lambda, sigma);
}
SPX_EXPORT int spx_prox_l0_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                               float lambda, float sigma) {
  return run_prox<RowL0>(SepCall<float>{ctx, y, q, nullptr, xk, sj, n, {}, nullptr}, lambda, sigma);
}
SPX_EXPORT int spx_prox_l1_box_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                                   float lambda, float sigma, const float* l_vec, const float* u_vec, float l_scalar,
                                   float u_scalar, const uint8_t* sel_mask) {
  return run_prox<RowL1Box>(SepCall<float>{ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(float), nullptr}, lambda, sigma);
}
SPX_EXPORT int spx_prox_l0_box_f32(spx_ctx* ctx, float* y, const float* q, const float* xk, const float* sj, int64_t n,
                                   float lambda, float sigma, const float* l_vec, const float* u_vec, float l_scalar,
                                   float u_scalar, const uint8_t* sel_mask) {
  return run_prox<RowL0Box>(SepCall<float>{ctx, y, q, nullptr, xk, sj, n, SPX_BOX_OF(float), nullptr}, lambda, sigma);
}


// ---------------------------------------------------------------------------------------------
// iprox! entry points
// ---------------------------------------------------------------------------------------------
// the skeleton of each precision
template <class Op>
static int run_skeleton(const SepCall<double>& c, Op op) { return run_separable(c, op); }
template <class Op>
static int run_skeleton(const SepCall<float>& c, Op op) { return run_f32(c, op); }
// The d > 0 flag word of the unboxed forms, read back (the stream is synchronised): the reference's assertion.
static int iprox_check_flag(spx_ctx* ctx, const int* flag) {
  int bad = 0;
  SPX_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SPX_HIP(hipStreamSynchronize(ctx->stream));
  if (bad) {
    spx_set_error("AssertionError: d[i] > 0");
    return SPX_ERR_ASSERT;
  }
  return SPX_OK;
}
// check_d (the flagged rows): the d > 0 flag is read back, which synchronises the stream -- refused under a capture before
// anything is enqueued
template <class Row, class T>
static int run_iprox(const SepCall<T>& c, T lambda, int check_d) {
  int rc = spx_check_common(c);
  if (rc) return rc;
  SPX_REQUIRE(c.n == 0 || c.d != nullptr, "d is NULL");
  if constexpr (!Row::kFlagged) {
    return run_skeleton(c, RowOp<Row, T>{lambda});
  } else {
    spx_ctx* const ctx = c.ctx;
    if (c.n == 0) return SPX_OK;
    if (check_d) { rc = spx_require_not_capturing(ctx, "the d > 0 check of iprox! (pass check = 0)"); if (rc) return rc; }
    rc = spx_ws_reserve(ctx, 256);
    if (rc) return rc;
    SPX_ON_DEVICE(ctx);
    int* flag = reinterpret_cast<int*>(ctx->ws);
    { const int rz = spx_zero_async(ctx, flag, sizeof(int)); if (rz) return rz; }
    rc = run_skeleton(c, RowOp<Row, T>{lambda, flag});
    if (rc || !check_d) return rc;
    return iprox_check_flag(ctx, flag);
  }
}

// ---------------------------------------------------------------------------------------------
// iprox! + step statistics in one pass (spx_iproxstep_*): y, xkn = (xk + sj) + y and {h, <g, y>, <d .* y, y>, <y, y>} to a host
// double[4] (synchronous) and / or a device double[4] (enqueue only).  Float64, device pointers.  All four operators take the
// fused route, each on the skeleton of its plain iprox! (profiles/iproxstep_kres.txt).
// ---------------------------------------------------------------------------------------------
template <class Row>
static int run_iproxstep(const SepCall<double>& c, double lambda, int check_d, const SpxDest& dest) {
  spx_ctx* const ctx = c.ctx;
  int rc = spx_check_common(c);
  if (rc) return rc;
  SPX_REQUIRE(c.n == 0 || c.d != nullptr, "d is NULL");
  rc = spx_step_begin(ctx, dest, check_d != 0, c.y, {c.q, c.d}, "y aliases g or d (the sums would read an overwritten input)", c.xkn,
                      c.others());
  if (rc) return rc;
  if (c.n == 0) return spx_dest_empty(ctx, dest);
  WithIstep<typename Row::Op, typename Row::Term> op{};
  op.lambda = lambda;
  int* flag = nullptr;
  if constexpr (Row::kFlagged) {
    // the whole workspace of the call is reserved here, so that the flag word keeps its address through run_separable
    rc = spx_ws_reserve(ctx, sep_ws_bytes(ctx, c.n, 4));
    if (rc) return rc;
    SPX_ON_DEVICE(ctx);
    flag = reinterpret_cast<int*>(static_cast<char*>(ctx->ws) + kSepFlagOffset);  // (clear of the four result doubles)
    { const int rz = spx_zero_async(ctx, flag, sizeof(int)); if (rz) return rz; }
    op.flag = flag;
  }
  rc = run_separable(c, op, dest, lambda);
  if (rc || !check_d) return rc;
  if constexpr (Row::kFlagged) return iprox_check_flag(ctx, flag);  // (the stream has been synchronised by the copy of the statistics)
  return SPX_OK;
}

// the entry points: q of the call holds g; the Box forms have no check_d
#define SPX_IPROX3(IPROX, IPROXSTEP, IPROX_F32, ROW)                                                                           \
  SPX_EXPORT int IPROX(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,         \
                       int64_t n, double lambda, int check_d) {                                                               \
    return run_iprox<ROW>(SepCall<double>{ctx, y, g, d, xk, sj, n, {}, nullptr}, lambda, check_d);                             \
  }                                                                                                                            \
  SPX_EXPORT int IPROXSTEP(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,     \
                           int64_t n, double lambda, int check_d, double* xkn, double* stats, double* stats_dev) {            \
    return run_iproxstep<ROW>({ctx, y, g, d, xk, sj, n, {}, xkn}, lambda, check_d, {stats, stats_dev, 4});                     \
  }                                                                                                                            \
  SPX_EXPORT int IPROX_F32(spx_ctx* ctx, float* y, const float* g, const float* d, const float* xk, const float* sj,          \
                           int64_t n, float lambda, int check_d) {                                                            \
    return run_iprox<ROW>(SepCall<float>{ctx, y, g, d, xk, sj, n, {}, nullptr}, lambda, check_d);                              \
  }
SPX_IPROX3(spx_iprox_l1, spx_iproxstep_l1, spx_iprox_l1_f32, RowIproxL1)
SPX_IPROX3(spx_iprox_l0, spx_iproxstep_l0, spx_iprox_l0_f32, RowIproxL0)
#define SPX_IPROX3_BOX(IPROX, IPROXSTEP, IPROX_F32, ROW)                                                                       \
  SPX_EXPORT int IPROX(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,         \
                       int64_t n, double lambda, const double* l_vec, const double* u_vec, double l_scalar,                   \
                       double u_scalar, const uint8_t* sel_mask) {                                                            \
    return run_iprox<ROW>(SepCall<double>{ctx, y, g, d, xk, sj, n, SPX_BOX_OF(double), nullptr}, lambda, 0);                   \
  }                                                                                                                            \
  SPX_EXPORT int IPROXSTEP(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj,     \
                           int64_t n, double lambda, const double* l_vec, const double* u_vec, double l_scalar,               \
                           double u_scalar, const uint8_t* sel_mask, double* xkn, double* stats, double* stats_dev) {         \
    return run_iproxstep<ROW>({ctx, y, g, d, xk, sj, n, SPX_BOX_OF(double), xkn}, lambda, 0, {stats, stats_dev, 4});           \
  }                                                                                                                            \
  SPX_EXPORT int IPROX_F32(spx_ctx* ctx, float* y, const float* g, const float* d, const float* xk, const float* sj,          \
                           int64_t n, float lambda, const float* l_vec, const float* u_vec, float l_scalar, float u_scalar,   \
                           const uint8_t* sel_mask) {                                                                         \
    return run_iprox<ROW>(SepCall<float>{ctx, y, g, d, xk, sj, n, SPX_BOX_OF(float), nullptr}, lambda, 0);                     \
  }
SPX_IPROX3_BOX(spx_iprox_l1_box, spx_iproxstep_l1_box, spx_iprox_l1_box_f32, RowIproxL1Box)
SPX_IPROX3_BOX(spx_iprox_l0_box, spx_iproxstep_l0_box, spx_iprox_l0_box_f32, RowIproxL0Box)
