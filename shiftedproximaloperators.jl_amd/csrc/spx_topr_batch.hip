// spx_topr_batch.hip -- batched ShiftedIndBallL0 / ShiftedIndBallL0BInf prox! + step statistics, parameters on the device
// (spx_proxstep_indball_l0_batch, spx_proxstep_indball_l0_binf_batch; include/spx_topr_batch.h).  Built into a library of its own,
// libspx_topr_batch.so, which links against libspx.so (the context, the error text, the zero-fill kernel of the empty call).
// `batch` top-r problems in ONE launch, problem b at elements [b * ld, b * ld + n) of every vector; r[b], delta[b], q_scale[b] are
// read from device memory by the workgroup that owns the row.
//
// ONE workgroup owns ONE problem from its first load to its last store: nobody waits for another workgroup, nothing depends on
// what is resident -- no exchange words, no spx_ctx::sync, no workspace.  The selection is the exact MSD radix select of
// spx_topr_row.hpp (topr_row_begin, topr_row_digit, topr_row_advance, topr_row_keep), the idea of k_sel_small (spx_select.hip):
//   1. v = (xk + sj) + q_scale q and the span [kmin, kmax] of the row's keys;
//   2. per digit: a histogram of 4096 bins in LDS (a wavefront adds the bin of its first pending lane once, with its population
//      count: tied data and index digits send whole wavefronts to one bin), located by wavefront 0 in two 64-wide scans;
//   3. the storing pass: y = (keep ? v : 0) - (xk + sj) [clamped], xkn = (xk + sj) + y, the count of nonzeros of xkn and the two
//      sums, by a fixed-order workgroup reduce (wave_sum_dpp, then fold16_sum over the wavefronts' slots).
// Which form: row_batch_plan on kToprBatchShape (spx_plan.hpp); the site shared with the other row-owner calls: spx_row_batch.hpp.
//   row-resident (REG): the lane's units -- v, xk + sj and q -- are loaded once, by unconditional loads at clamped indices so that
//              all of them are in flight, and stay in registers across the digit passes: 40 B/element of traffic.
//   row walk   (!REG): 1024 lanes park v in the row of y and re-read it once per digit, kToprBatchWalkUnroll units in flight per
//              lane.  A lane owns the same units in every pass and re-reads only what it stored itself, so y needs no fence between
//              passes -- which is why y may be none of the inputs.
#include <type_traits>

#include "spx_topr_batch.h"
#include "spx_row_batch.hpp"
#include "spx_topr_row.hpp"

namespace {

// what a kernel is launched with
struct ToprBatchArgs {
  double* y;
  const double *q, *xk, *sj;
  double* xkn;  // or NULL
  const int64_t* r;
  const double *delta, *qscale;  // delta: NULL in the plain form
  int64_t ld;
  int n;  // 1 .. kToprBatchNMax
  int xkn_pairs;
  double* stats;
};

// Histogram add of a wavefront's digits with the heavy hitter peeled off first: the bin of the first pending lane is added ONCE
// with its population count, the rest go lane by lane (atomics on one LDS address are serialised).  Called by whole wavefronts;
// `in` = this lane contributes.
__device__ __forceinline__ void topr_hist_add(unsigned int* h, unsigned int digit, bool in) {
  const unsigned long long todo = __ballot(in);
  if (todo == 0ull) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)todo) - 1;
  const unsigned int d0 = __shfl(digit, leader, 64);
  const bool same = in && digit == d0;
  const unsigned long long peel = __ballot(same);
  if (lane == leader) atomicAdd(&h[d0], (unsigned int)__popcll(peel));
  else if (in && !same) atomicAdd(&h[digit], 1u);
}

// A state every lane read from shared memory, moved to scalar registers
__device__ __forceinline__ int topr_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t topr_uni(uint64_t v) {
  return ((uint64_t)(unsigned int)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
         (uint64_t)(unsigned int)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffu));
}
__device__ __forceinline__ int64_t topr_uni(int64_t v) { return (int64_t)topr_uni((uint64_t)v); }
__device__ __forceinline__ ToprRowState topr_uniform(const ToprRowState& a) {
  ToprRowState o;
  o.phase = topr_uni(a.phase); o.shift = topr_uni(a.shift); o.width = topr_uni(a.width); o.idx_bits = topr_uni(a.idx_bits);
  o.base = topr_uni(a.base); o.prefix = topr_uni(a.prefix); o.quota = topr_uni(a.quota); o.t_ge = topr_uni(a.t_ge);
  o.t_eq = topr_uni(a.t_eq); o.icut = topr_uni(a.icut);
  return o;
}

// inclusive prefix sum over the 64 lanes of a wavefront
__device__ __forceinline__ unsigned int topr_wave_scan(unsigned int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned int up = __shfl_up(v, off, 64);
    if (lane >= off) v += up;
  }
  return v;
}

// The step of spx_topr_row.hpp on a complete histogram, by wavefront 0 (called by its 64 lanes only): lane l sums the 64 bins
// [64 l, 64 l + 64) of the scan order, a wavefront scan finds the run that holds the quota-th element, a second one the bin.  The
// lane that owns the bin stores the next state.  Bins at and above 2^width are zero.
__device__ __forceinline__ void topr_scan_step(const unsigned int* hist, const ToprRowState& st, ToprRowState* out) {
  const int l = threadIdx.x & 63;
  const bool desc = st.phase == kToprKeyDigits;  // keys from the top, indices from the bottom
  const uint4* const h4 = reinterpret_cast<const uint4*>(hist) + 16 * (desc ? 63 - l : l);
  unsigned int sum = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint4 a = h4[(j + l) & 15];  // (rotated: the lanes of a quarter wavefront read different banks)
    sum += (a.x + a.y) + (a.z + a.w);
  }
  const unsigned int quota = (unsigned int)st.quota;  // 1 .. n - 1
  const unsigned int inc = topr_wave_scan(sum);
  const unsigned long long holds = __ballot(inc - sum < quota && inc >= quota);
  if (holds == 0ull) return;  // (a complete histogram always holds the quota)
  const int owner = __ffsll((long long)holds) - 1;
  const unsigned int before = __shfl(inc - sum, owner, 64);
  const int pos = 64 * owner + l;
  const int bin = desc ? kToprBins - 1 - pos : pos;
  const unsigned int c = hist[bin];
  const unsigned int run = before + topr_wave_scan(c) - c;
  if (run < quota && run + c >= quota) *out = topr_row_advance(st, (uint64_t)bin, (uint64_t)run, (uint64_t)c);
}

template <int LANES, int EPL, bool REG, bool PAIRS, bool BINF>
__global__ __launch_bounds__(LANES) void k_topr_batch(ToprBatchArgs k) {
  constexpr int E = PAIRS ? 2 : 1;            // elements of a unit
  constexpr int UPL = REG ? EPL / E : 1;      // units a lane keeps in registers
  constexpr int WU = kToprBatchWalkUnroll;
  static_assert(!REG || EPL % 2 == 0, "whole pairs per lane");
  __shared__ __attribute__((aligned(16))) unsigned int hist[kToprBins];
  __shared__ double lds[3][16];
  __shared__ unsigned long long kmm[2];
  __shared__ ToprRowState sst;
  const int t = threadIdx.x;
  if (t < 48) (&lds[0][0])[t] = 0.0;
  if (t == 0) { kmm[0] = ~0ull; kmm[1] = 0ull; }
  // the problem's scalars: the row is uniform, so these are scalar loads
  const int64_t b = blockIdx.x;
  const int64_t r = k.r[b];
  const double qs = k.qscale[b];
  double delta = 0.0;
  if constexpr (BINF) delta = k.delta[b];
  const int64_t off = b * k.ld;
  double* const y = k.y + off;
  const double *const q = k.q + off, *const xk = k.xk + off, *const sj = k.sj + off;
  double* const xkn = k.xkn ? k.xkn + off : nullptr;
  const int n = k.n;
  const int ufull = n / E;                              // units of E elements; >= 1 (pairs: n >= 2)
  const int utot = (int)row_batch_units(n, PAIRS);      // ... and the one-element unit of an odd row in the pairs form
  __syncthreads();

  // unit u of the inputs: v = (xk + sj) + q_scale q (shiftedIndBallL0.jl:66 at q_scale q: one rounded multiply in front of the sum;
  // from_y: the parked v instead), xs = xk + sj, q as passed.  What a slot beyond the row holds is never used.
  auto load_in = [&](int u, double (&v)[E], double (&xs)[E], double (&qv)[E], bool from_y) {
    if (from_y) {
      const double* const in[4] = {xk, sj, q, y};
      double w[4][E];
      row_load_unit<PAIRS>(in, u, ufull, n, w);
#pragma unroll
      for (int e = 0; e < E; ++e) { xs[e] = w[0][e] + w[1][e]; qv[e] = w[2][e]; v[e] = w[3][e]; }
    } else {
      const double* const in[3] = {xk, sj, q};
      double w[3][E];
      row_load_unit<PAIRS>(in, u, ufull, n, w);
#pragma unroll
      for (int e = 0; e < E; ++e) { xs[e] = w[0][e] + w[1][e]; qv[e] = w[2][e]; v[e] = xs[e] + qs * qv[e]; }
    }
  };
  // row walk: v of unit u goes to the row of y
  auto park = [&](int u, const double (&v)[E]) {
    if (u < utot) row_store_y<PAIRS>(y, u, u < ufull, v[0], v[E - 1]);
  };
  uint64_t kmin = ~0ull, kmax = 0ull;
  auto track = [&](int u, const double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint64_t key = topr_key(v[e]);
      if (u * E + e < n) {
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
      }
    }
  };
  // ---- pass 0: v (kept in registers, or parked in y) and the span of its keys
  double V[REG ? EPL : 1], XS[REG ? EPL : 1], Q[REG ? EPL : 1];
  if constexpr (REG) {
#pragma unroll
    for (int kk = 0; kk < UPL; ++kk) {
      double v[E], xs[E], qv[E];
      const int u = (int)row_batch_unit(kk, LANES, t);
      load_in(u, v, xs, qv, false);
      track(u, v);
#pragma unroll
      for (int e = 0; e < E; ++e) { V[kk * E + e] = v[e]; XS[kk * E + e] = xs[e]; Q[kk * E + e] = qv[e]; }
    }
  } else {
    for (int base = 0; base < utot; base += LANES * WU) {
      double v[WU][E], xs[WU][E], qv[WU][E];
#pragma unroll
      for (int j = 0; j < WU; ++j) load_in(base + j * LANES + t, v[j], xs[j], qv[j], false);
#pragma unroll
      for (int j = 0; j < WU; ++j) {
        track(base + j * LANES + t, v[j]);
        park(base + j * LANES + t, v[j]);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t a = __shfl_xor((unsigned long long)kmin, o, 64), c = __shfl_xor((unsigned long long)kmax, o, 64);
    kmin = a < kmin ? a : kmin;
    kmax = c > kmax ? c : kmax;
  }
  if ((t & 63) == 0) { atomicMin(&kmm[0], (unsigned long long)kmin); atomicMax(&kmm[1], (unsigned long long)kmax); }
  __syncthreads();
  if (t == 0) sst = topr_row_begin(n, r, kmm[0], kmm[1]);
  // ---- the digit passes (spx_topr_row.hpp): a histogram of the row, then the step, until resolved
  auto count_unit = [&](const ToprRowState& st, int u, const double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = u * E + e;
      unsigned int digit;
      const bool in = topr_row_digit(st, topr_key(v[e]), i, &digit) && i < n;
      topr_hist_add(hist, digit, in);
    }
  };
  ToprRowState st;
  for (int pass = 0;; ++pass) {
    __syncthreads();
    st = topr_uniform(sst);
    if (st.phase == kToprResolved || pass == kToprMaxPasses) break;
    for (int j = t; j < kToprBins / 4; j += LANES) reinterpret_cast<uint4*>(hist)[j] = uint4{0u, 0u, 0u, 0u};
    __syncthreads();
    if constexpr (REG) {
#pragma unroll
      for (int kk = 0; kk < UPL; ++kk) {
        double v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = V[kk * E + e];
        count_unit(st, (int)row_batch_unit(kk, LANES, t), v);
      }
    } else {
      for (int base = 0; base < utot; base += LANES * WU) {
        const double* const parked[1] = {y};  // the row walk reads v where pass 0 left it
        double v[WU][1][E];
#pragma unroll
        for (int j = 0; j < WU; ++j) row_load_unit<PAIRS>(parked, base + j * LANES + t, ufull, n, v[j]);
#pragma unroll
        for (int j = 0; j < WU; ++j) count_unit(st, base + j * LANES + t, v[j][0]);
      }
    }
    __syncthreads();
    if (t < 64) topr_scan_step(hist, st, &sst);
  }
  // ---- the storing pass: y (shiftedIndBallL0.jl:69-70, shiftedIndBallL0BInf.jl:91), xkn = (xk + sj) + y, and over the STORED y the
  // count of nonzeros of xkn (a sum of exact ones), sum q y (q AS PASSED), sum y^2
  double h[3] = {0.0, 0.0, 0.0};
  auto outv = [&](double v, double xs, int i) -> double {
    const double kept = topr_row_keep(st, topr_key(v), i) ? v : 0.0;
    const double o = kept - xs;
    if constexpr (BINF) return jl_min(jl_max(o, -delta), delta);
    else return o;
  };
  auto sums = [&](double qr, double w, double o) {
    h[0] += (w != 0.0) ? 1.0 : 0.0;  // (NaN counts)
    h[1] += qr * o;
    h[2] += o * o;
  };
  auto store_unit = [&](int u, const double (&v)[E], const double (&xs)[E], const double (&qv)[E]) {
    if (u >= utot) return;
    if (PAIRS && u < ufull) {
      const f64x2 o{outv(v[0], xs[0], 2 * u), outv(v[E - 1], xs[E - 1], 2 * u + 1)};
      const f64x2 w{xs[0] + o.x, xs[E - 1] + o.y};
      row_store_y<PAIRS>(y, u, true, o.x, o.y);
      row_store_xkn<PAIRS>(xkn, k.xkn_pairs, u, true, w.x, w.y);
      sums(qv[0], w.x, o.x);
      sums(qv[E - 1], w.y, o.y);
    } else {  // one element: the element-wise form, or the last element of an odd row
      const int i = u * E;
      const double o = outv(v[0], xs[0], i);
      const double w = xs[0] + o;
      row_store_y<PAIRS>(y, u, false, o, o);
      row_store_xkn<PAIRS>(xkn, k.xkn_pairs, u, false, w, w);
      sums(qv[0], w, o);
    }
  };
  if constexpr (REG) {
#pragma unroll
    for (int kk = 0; kk < UPL; ++kk) {
      double v[E], xs[E], qv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) { v[e] = V[kk * E + e]; xs[e] = XS[kk * E + e]; qv[e] = Q[kk * E + e]; }
      store_unit((int)row_batch_unit(kk, LANES, t), v, xs, qv);
    }
  } else {
    for (int base = 0; base < utot; base += LANES * WU) {
      double v[WU][E], xs[WU][E], qv[WU][E];
#pragma unroll
      for (int j = 0; j < WU; ++j) load_in(base + j * LANES + t, v[j], xs[j], qv[j], true);
#pragma unroll
      for (int j = 0; j < WU; ++j) store_unit(base + j * LANES + t, v[j], xs[j], qv[j]);
    }
  }
  row_block_sum<3>(h, lds);
  if (t == 0) {
    k.stats[3 * b] = h[0];
    k.stats[3 * b + 1] = h[1];
    k.stats[3 * b + 2] = h[2];
  }
}

// what differs from the other row-owner calls on the host (run_row_batch, spx_row_batch.hpp)
template <bool BINF>
struct ToprBatchKind {
  static constexpr const char* kLibName = "libspx_topr_batch.so";
  static constexpr RowBatchShape kShape = kToprBatchShape;
  struct Params {
    const int64_t* r;
    const double *delta, *q_scale;  // delta: NULL in the plain form
  };
  static bool null_params(const Params& a) { return a.r == nullptr || a.q_scale == nullptr || (BINF && a.delta == nullptr); }
  static constexpr const char* kNullParams = BINF ? "a parameter array (r, delta, q_scale) is NULL" : "a parameter array (r, q_scale) is NULL";
  static const char* refuse_alias(const RowBatchCall& c) {
    return c.y != c.xk && c.y != c.sj ? nullptr : "y is xk or sj (v is parked in the row of y between the digit passes)";
  }
  static constexpr const char* kNTooLarge =
      BINF ? "n > 2^20: one workgroup per problem is the wrong tool (spx_prox_indball_l0_binf spreads such a problem over many "
             "CUs, one problem per call)"
           : "n > 2^20: one workgroup per problem is the wrong tool (spx_prox_indball_l0 spreads such a problem over many CUs, "
             "one problem per call)";
  template <int LANES, int EPL, bool REG, bool PAIRS>
  static void launch(const RowBatchCall& c, const Params& a, const RowBatchPlan& p) {
    hipLaunchKernelGGL((k_topr_batch<LANES, EPL, REG, PAIRS, BINF>), dim3((unsigned)p.grid), dim3(LANES), 0, c.ctx->stream,
                       ToprBatchArgs{c.y, c.q, c.xk, c.sj, c.xkn, a.r, a.delta, a.q_scale, c.ld, (int)c.n, p.xkn_pairs ? 1 : 0,
                                     c.stats_dev});
  }
};

}  // namespace

SPX_EXPORT int spx_proxstep_indball_l0_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                             int64_t batch, int64_t ld, const int64_t* r, const double* q_scale, double* xkn,
                                             double* stats_dev) {
  return run_row_batch<ToprBatchKind<false>>({ctx, y, q, xk, sj, n, batch, ld, xkn, stats_dev}, {r, nullptr, q_scale});
}

SPX_EXPORT int spx_proxstep_indball_l0_binf_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                                  int64_t n, int64_t batch, int64_t ld, const int64_t* r, const double* delta,
                                                  const double* q_scale, double* xkn, double* stats_dev) {
  return run_row_batch<ToprBatchKind<true>>({ctx, y, q, xk, sj, n, batch, ld, xkn, stats_dev}, {r, delta, q_scale});
}
