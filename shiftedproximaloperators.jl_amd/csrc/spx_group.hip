// spx_group.hip -- ShiftedGroupNormL2.prox! and ShiftedGroupNormL2Binf.prox! (group-l2 block soft-threshold,
// with an l-infinity trust region in the Binf form).
//
// HBM layout: q, xk, sj, y contiguous fp64; groups are contiguous index ranges (CSR offsets or a uniform
// size); lambda is one fp64 per group.  Algorithmic traffic: 32 B/element + 8 B/group.
// Roofline: HBM bandwidth; the Binf form adds a per-group scalar root find that runs out of registers.
//
// Mapping.  Fast path (uniform group size LPG*EPL, 16-byte aligned): a group is owned by LPG lanes of a
// wavefront (LPG = 16 for the 128-element groups of the BASELINE config, so one wave works on 4 groups at
// once), each lane keeps EPL elements of S = (q + xk) + sj, X = xk, xk + sj and S/sigma in registers; q/xk/sj
// are read once with non-temporal 16-byte loads and y is written once.  Sums over a group are DPP
// butterflies inside a 16-lane row (no LDS).  Packing several groups into a wave amortises the
// per-group scalar arithmetic of the Binf root find (divisions, square roots), which every lane of a
// group executes redundantly.  Other shapes: a wavefront or a 256-lane workgroup per group, elements
// re-read from L1/L2 for every reduction.
#include <limits>
#include <type_traits>

#include "spx_group_common.hpp"

#ifdef SPX_DEBUG_PEEK  // diagnostic builds only: [0] last raw count the LIT launch read, [1] LIT launches that read a count
                       // outside [0, ngroups], [2] LIT launches, [3] count at the entry of the last main launch, [4] main
                       // launches, [5] main launches that found the count outside [0, ngroups] on entry
__device__ long long g_group_dbg[8];
extern "C" __attribute__((visibility("default"))) int spx_debug_group_words(long long* out8, int reset) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_group_dbg), sizeof(g_group_dbg));
  if (e == hipSuccess && reset) {
    long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_group_dbg), z, sizeof(z));
  }
  return (int)e;
}
#endif


// ---------------------------------------------------------------------------------------------
// prox! fused with the value of h at the result (spx_proxval_group_l2[_binf]).  A launch that stores groups adds their terms
// lambda_g * ||((xk + sj) + y)[g]|| into one partial sum per workgroup (one tile per wavefront: tens of thousands of them at
// n = 1e8).  The call's LAST launch (hdr != NULL) finishes in two levels on the ticket words of the objective kernels
// (SpxSyncHeader::fin_class / fin_top, the two halves of spx_fin_ticket): the workgroup that takes the last ticket of class j
// (workgroups j, j + 8, ...) adds the partials j, j + 8, ... -- eight workgroups work side by side, every lane keeps eight loads in
// flight -- and the one that takes the last of the eight top tickets adds the eight class sums.  Every sum has a fixed shape:
// the value is reproducible run to run.  The ticket words reset themselves, so the same nodes replay in a graph.
//   one launch (plain operator, uniform groups): the partials are the launch's own (agent-scope stores / loads);
//   a launch behind the main one (Binf: the LIT launch; CSR: k_group_list_val): the partials are the finished main launch's.
// Groups a main launch hands on (deferred list: Binf literal evaluation, ragged groups above the size bound) reach the launch
// behind it in the order their atomics retired -- not a fixed one.  So that launch adds nothing up: it stores each group's term
// in dterm[g]; the main launch leaves one 64-bit mask per wavefront tile (bit = the lane that handed a group on) and one flag per
// workgroup (any); the class sums carry the number of flagged workgroups, and only when there is one does the last workgroup
// walk the flags and add the terms of the flagged workgroups' tiles in group order -- after the partials, a fixed order whatever
// the list looked like, and no work at all in the common case of an empty list.
// ---------------------------------------------------------------------------------------------
struct GroupNoVal {};
struct GroupValWs {
  double result;     // read back by the host
  double cpart[8];   // class sums of the partials
  double cany[8];    // ... and of the flags
  double pad[15];    // (the partials start on a 256-byte boundary)
};
struct GroupVal {
  double qs;           // q_scale: the prox is taken at qs * q
  double* part;        // partial sums, one per workgroup of the (main) launch ...
  double* any;         // ... and 1.0 where that workgroup handed a group on (NULL: this call has no list)
  int nmain;           // workgroups of the main launch (a launch behind it: how many partials there are)
  bool behind;         // this launch runs behind the main one: it adds the main launch's partials, has none of its own
  SpxSyncHeader* hdr;  // non-NULL: this is the last launch of the call
  GroupValWs* ws;
  double* target;      // the device destination of the value (SpxDest::dev, may be NULL)
  unsigned long long* dmask;  // [tile] (main launch: written; last launch: read for flagged workgroups)
  double* dterm;              // [group]
  int lpg_main;               // lanes per group of the main launch's tile (bit -> group)
};
// The step form (spx_proxstep_group_l2[_binf]): three sums where GroupVal has one -- [0] the h terms as above, [1] q[i] * y[i]
// (q as passed, not qs * q), [2] y[i]^2 -- and xkn = (xk + sj) + y stored next to y.  Three planes of everything that carries a sum:
// the partials `nmain` doubles apart in `part` (the flags behind the third), the class sums in GroupStepWs, the terms of the
// handed-on groups `dplane` doubles apart in `dterm`.  ONE ticket per workgroup publishes its three partials, and every plane is
// added with the statements, hence in the order and to the bits, of the single sum.
struct GroupStepWs {
  double result[3];    // read back by the host
  double cpart[3][8];  // class sums of the three planes of partials
  double cany[8];      // ... and of the flags
  double pad[29];      // (the partials start on a 256-byte boundary)
};
struct GroupStep : GroupVal {
  double* xkn;        // (xk + sj) + y, or NULL
  double* stats_dev;  // the caller's device double[3], or NULL
  GroupStepWs* sws;   // (takes the place of `ws`)
  int64_t dplane;     // doubles between the planes of `dterm`
};
static_assert(sizeof(GroupValWs) == 256 && sizeof(GroupStepWs) == 512, "the partials start on a 256-byte boundary");
static_assert(offsetof(GroupValWs, result) == 0 && offsetof(GroupStepWs, result) == 0, "the host reads the result words from the start of the block");
template <class GV>
constexpr int kGroupSums = std::is_same<GV, GroupStep>::value ? 3 : 1;
// x[i0], x[i0 + step], ... (cnt of them) added by the workgroup: lane t takes the elements t, t + 256, ..., eight loads in flight
// -- of each of the NS planes `plane` doubles apart, all of them issued before the first is added
template <bool ATOMIC, int NS>
__device__ __forceinline__ void gval_strided_sum(const double* x, int64_t plane, int64_t i0, int64_t step, int64_t cnt, double (&a)[NS]) {
#pragma unroll
  for (int p = 0; p < NS; ++p) a[p] = 0.0;
  for (int64_t k0 = threadIdx.x; k0 < cnt; k0 += 256 * 8) {
    double v[NS][8];
#pragma unroll
    for (int p = 0; p < NS; ++p) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = k0 + 256 * u;
        const double* q = x + p * plane + i0 + step * (k < cnt ? k : 0);
        const double w = ATOMIC ? spx_atomic_load_f64(q) : *q;
        v[p][u] = k < cnt ? w : 0.0;
      }
    }
#pragma unroll
    for (int p = 0; p < NS; ++p) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[p] += v[p][u];
    }
  }
}
// `acc`: the lane's sums (GroupVal: one, non-zero in one lane per group; GroupStep: three); `handed`: this lane handed a group on.
// Every lane of the (256-lane) workgroup must call it.
template <class GV>
__device__ __forceinline__ void gval_finish(double (&acc)[kGroupSums<GV>], bool handed, const GV& gv) {
  constexpr int NS = kGroupSums<GV>;
  __shared__ double gv_lds[NS][4];
  __shared__ int gv_flag;
  auto block_sum = [&](auto& v) {  // (every plane crosses the one pair of barriers)
    constexpr int M = sizeof(v) / sizeof(double);
#pragma unroll
    for (int p = 0; p < M; ++p) v[p] = wave_sum(v[p]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int p = 0; p < M; ++p) gv_lds[p][threadIdx.x >> 6] = v[p];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < M; ++p) v[p] = (gv_lds[p][0] + gv_lds[p][1]) + (gv_lds[p][2] + gv_lds[p][3]);
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (this wavefront's dterm stores have left before its workgroup takes a ticket)
  if (!gv.behind) {
    block_sum(acc);
    if (gv.any != nullptr) {
      const int any = __syncthreads_or(handed ? 1 : 0);
      if (threadIdx.x == 0) gv.any[blockIdx.x] = any ? 1.0 : 0.0;
    }
    if (gv.hdr == nullptr) {
      if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < NS; ++p) gv.part[(int64_t)p * gv.nmain + blockIdx.x] = acc[p];
      }
      return;
    }
  }
  const unsigned int grid = gridDim.x, j = blockIdx.x % (unsigned)kSpxBarSplit;
  const unsigned int classes = grid < (unsigned)kSpxBarSplit ? grid : (unsigned)kSpxBarSplit;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!gv.behind) {
#pragma unroll
      for (int p = 0; p < NS; ++p) spx_atomic_store_f64(&gv.part[(int64_t)p * gv.nmain + blockIdx.x], acc[p]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int want = (grid - j + (unsigned)kSpxBarSplit - 1u) / (unsigned)kSpxBarSplit;  // workgroups j, j + 8, ...
    const unsigned int c = __hip_atomic_fetch_add(&gv.hdr->fin_class[32u * j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gv_flag = (c + 1u == want) ? 1 : 0;
    if (gv_flag) __hip_atomic_store(&gv.hdr->fin_class[32u * j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!gv_flag) return;
  // the last workgroup of class j: the partials j, j + classes, ... (and how many of their workgroups handed a group on)
  double* const cpart = [&] { if constexpr (NS == 1) return &gv.ws->cpart[0]; else return &gv.sws->cpart[0][0]; }();
  double* const cany = [&] { if constexpr (NS == 1) return &gv.ws->cany[0]; else return &gv.sws->cany[0]; }();
  const int64_t cnt = (int64_t)j < gv.nmain ? ((int64_t)gv.nmain - j + classes - 1) / classes : 0;
  double a[NS];
  if (gv.behind) gval_strided_sum<false>(gv.part, gv.nmain, j, classes, cnt, a);
  else gval_strided_sum<true>(gv.part, gv.nmain, j, classes, cnt, a);
  block_sum(a);
  double f[1] = {0.0};
  if (gv.any != nullptr && gv.behind) {
    gval_strided_sum<false>(gv.any, 0, j, classes, cnt, f);
    block_sum(f);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < NS; ++p) spx_atomic_store_f64(&cpart[8 * p + j], a[p]);
    spx_atomic_store_f64(&cany[j], f[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(&gv.hdr->fin_top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gv_flag = (t + 1u == classes) ? 1 : 0;
    if (gv_flag) __hip_atomic_store(&gv.hdr->fin_top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!gv_flag) return;
  // the last workgroup of the launch: the class sums in class order, then the handed-on groups (usually none)
  __shared__ double gv_total[NS + 1];
  if (threadIdx.x == 0) {
    double v[NS], n = 0.0;
#pragma unroll
    for (int p = 0; p < NS; ++p) v[p] = 0.0;
    for (unsigned int c = 0; c < classes; ++c) {
#pragma unroll
      for (int p = 0; p < NS; ++p) v[p] += spx_atomic_load_f64(&cpart[8 * p + c]);
      n += spx_atomic_load_f64(&cany[c]);
    }
#pragma unroll
    for (int p = 0; p < NS; ++p) gv_total[p] = v[p];
    gv_total[NS] = n;
  }
  __syncthreads();
  double total[NS];
#pragma unroll
  for (int p = 0; p < NS; ++p) total[p] = gv_total[p];
  if (gv_total[NS] != 0.0) {  // (the same in every lane)
    double d[NS];
#pragma unroll
    for (int p = 0; p < NS; ++p) d[p] = 0.0;
    int64_t dplane = 0;
    if constexpr (NS == 3) dplane = gv.dplane;
    const int gpw = 64 / gv.lpg_main;
    for (int64_t b = threadIdx.x; b < gv.nmain; b += 256) {
      if (gv.any[b] == 0.0) continue;
      for (int w = 0; w < 4; ++w) {
        unsigned long long m = gv.dmask[4 * b + w];
        while (m) {
          const int bit = __ffsll((long long)m) - 1;
          m &= m - 1;
#pragma unroll
          for (int p = 0; p < NS; ++p) d[p] += spx_atomic_load_f64(&gv.dterm[p * dplane + (4 * b + w) * gpw + bit / gv.lpg_main]);
        }
      }
    }
    block_sum(d);
#pragma unroll
    for (int p = 0; p < NS; ++p) total[p] += d[p];
  }
  if (threadIdx.x == 0) {
    if constexpr (NS == 1) {
      gv.ws->result = total[0];
      if (gv.target) *gv.target = total[0];
    } else {
#pragma unroll
      for (int p = 0; p < NS; ++p) {
        gv.sws->result[p] = total[p];
        if (gv.stats_dev) gv.stats_dev[p] = total[p];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// fast path kernel: uniform groups of LPG*EPL elements; LPG lanes own a group, 64/LPG groups per wave;
// the group is resident in registers.  Lane j of a group owns the 16-byte pairs j, j + LPG, j + 2 LPG, ...
// ---------------------------------------------------------------------------------------------
#ifndef SPX_PADDED_CACHED
#define SPX_PADDED_CACHED 1  // A/B switch (round 4): cached accesses on partly filled tiles of <= 16 lanes per group (kPaddedCached)
#endif
#ifndef SPX_GROUP_PREFETCH
#define SPX_GROUP_PREFETCH 1  // A/B switch (round 4): Binf tiles of one / two lanes x 8 elements come in through LDS as whole kilobytes (kPre)
#endif
#ifndef SPX_GROUP_WAVES
#define SPX_GROUP_WAVES 3  // min waves/SIMD (VGPR cap) of the 8-element tiles.  Binf 1e6x128 on 16 lanes x 8: 3 (162 VGPRs, no spill) 0.84 ms; 4 (128, cold paths spill) 0.93 ms; 5: 1.49 ms
// Binf tiles with 16 elements per lane (8 x 16 for 128-element groups: 8 groups per wave) run at 2 waves/SIMD (220 VGPRs today; the figures in this comment are the compiler's at the time of each measurement):
// the kernel is VALU-bound and the wave-uniform scalar work of the root find is shared by twice as many elements --
// 0.79 -> 0.70 ms at 1e6 x 128 in spite of the lower occupancy.
#endif
// PAIRS: the group size is even (every group starts 16-byte aligned): lane j owns the pairs j, j + LPG, ...; pairs past
// the end of the group are read as zeros (zeros are neutral in every sum of both operators).  !PAIRS: odd group size,
// lane j owns the elements j, j + LPG, ... through 8-byte loads.
// LIT (Binf only): second launch over the deferred list -- `deferred` is then read: [0] = number of groups, [1..] = their
// ids -- evaluating the reference's expressions literally on the register-resident group (binf_literal_reg).
// FULL (PAIRS only): the group size is exactly LPG * EPL -- no pair of the tile is masked, which takes the zero-fill selects
// and the clamped addresses (~7 % of the kernel's VALU instructions) out of the BASELINE shapes (128 = 8 x 16 = 16 x 8).
// VALUE (spx_proxval_group_l2[_binf]): the prox is taken at gv.qs * q (one rounded multiply in front of `+ xk`), and the lane
// that holds a group's y adds the group's term of h((xk + sj) + y) -- lambda_g * sqrt(sum of squares) over the STORED y, in the
// association of k_obj_group MODE 0 -- into a per-lane sum that gval_finish turns into one partial per workgroup (GroupVal
// above).  A group this launch does not store (deferred to the LIT launch / the list kernel) is counted by the launch that does.
// VALUE = false: `gv` is an empty struct and none of this is compiled.
// STEP (spx_proxstep_group_l2[_binf], with VALUE; `gv` is a GroupStep): that lane also stores v = (xk + sj) + y to gv.xkn the way it
// stores y, and adds q * y and y * y of its elements into two more sums.  q is wanted AS PASSED and the kernel keeps neither q
// nor qs * q (only S = (qs * q + xk) + sj): it is read again once y is stored -- from the wavefront's staging buffer where the tile
// came in through LDS (kDma, kPre: the buffer is not reused before the next tile), else from memory, where the lines this
// wavefront fetched a few microseconds ago are still on chip -- which costs no register across the root find.
template <int LPG, int EPL, bool BINF, bool PAIRS, bool LIT = false, bool FULL = false, bool VALUE = false, bool STEP = false>
__global__ __launch_bounds__(256, (BINF && EPL >= 16) ? 2 : SPX_GROUP_WAVES) void k_group_reg(double* y_, const double* q_, const double* xk_, const double* sj_,
                                                    int64_t ngroups, int gsize, const double* __restrict__ lambda,
                                                    double sigma, double delta,
                                                    long long* deferred /* [1..] = groups ([0]: the count, unless dcount points elsewhere) */,
                                                    const int64_t* __restrict__ offsets /* !PAIRS only: ragged groups */,
                                                    int* status /* spx_ctx::status_dev */, int pole_lit /* tuning key 9 */,
                                                    unsigned long long* dcount /* the list's count word: deferred[0], or one of SpxSyncHeader::grp_deferred */,
                                                    unsigned long long* dclear /* LIT: the count word the NEXT call uses, zeroed here (or NULL) */,
                                                    typename std::conditional<STEP, GroupStep, typename std::conditional<VALUE, GroupVal, GroupNoVal>::type>::type gv) {
  static_assert((EPL % 2) == 0, "EPL must be even (16-byte pairs)");
  static_assert(VALUE || !STEP, "the step form extends the value form");
  const int64_t GS = gsize;  // <= LPG * EPL
  constexpr int GPW = 64 / LPG;  // groups per wave
  const int lane = threadIdx.x & 63;
  const int j = lane % LPG;
  const int slot = lane / LPG;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // plain GroupNormL2 stages its loads through LDS (LDS-DMA, +2 %: 0.650-0.664 vs 0.666-0.677 ms at 1e6 x 128);
  // the Binf form is VALU-bound and loses 6 % to the lower occupancy the LDS footprint allows, so it keeps register loads
  constexpr bool kDma = !BINF && PAIRS;
  // Round 4 -- partly filled tiles (a group size that is not lanes x elements, e.g. 100 on 8 x 16): the 16-byte pairs a group's
  // lanes fetch per instruction are a run of 16 LPG bytes that starts wherever the group does -- 800-byte groups: three runs
  // of four straddle two 128-byte lines -- and the next run of the group continues in the line the last one ended in.
  // Non-temporal accesses gave that line up in between; cached ones keep it: Binf groups of 20 / 50 / 66 / 100 / 120 at
  // n = 1e8: 1001 / 809 / 936 / 708 / 607 -> 807 / 719 / 840 / 652 / 583 us (4.52 -> 4.91 TB/s on groups of 100), the plain
  // operator on groups of 10 / 66 / 100: 671 / 664 / 600 -> 611 / 585 / 567 us.  Runs of 512 bytes and more (32 and 64 lanes
  // per group) are better off streaming (groups of 300 / 500: 2-4 % slower cached).
  constexpr bool kPaddedCached = SPX_PADDED_CACHED && PAIRS && !FULL && !LIT && LPG <= 16;
  // Round 4 -- Binf on the one- and two-lane tiles of 8 elements per lane (groups of 5 .. 16): the tile comes in and goes out
  // through a buffer of the wavefront in LDS, as whole kilobytes (tile_dma / tile_regs below).
  constexpr bool kPre = BINF && PAIRS && !LIT && EPL == 8 && LPG <= 2 && !(LPG == 2 && FULL) && SPX_GROUP_PREFETCH;
  __shared__ __attribute__((aligned(16))) char dma_lds[(kDma || kPre) ? 4 * 3 * (EPL / 2) * 1024 : 16];
  const int npairs = gsize >> 1;
  // (the list can hold at most every group once: a count outside [0, ngroups] is never followed into memory -- and never
  //  skipped silently either: the context's status word is raised and every later call fails, spx_common.hpp)
  const int64_t nlist = LIT ? (int64_t)*dcount : 0;
  if (LIT && dclear != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *dclear = 0ull;  // (nobody else touches that word in this call)
  const bool bad_count = LIT && (nlist < 0 || nlist > ngroups);
  if (bad_count && blockIdx.x == 0 && threadIdx.x == 0) spx_raise_status(status, kSpxStatusCorrupt);
  const int64_t ntodo = LIT ? (bad_count ? 0 : nlist) : ngroups;
#ifdef SPX_DEBUG_PEEK  // diagnostic builds (tools/r3/graph_fault_probe.py): what the count word held when a launch read it
  if (deferred != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    if constexpr (LIT) {
      g_group_dbg[0] = nlist;
      if (nlist < 0 || nlist > ngroups) g_group_dbg[1] += 1;
      g_group_dbg[2] += 1;
    } else {
      g_group_dbg[3] = (long long)__hip_atomic_load(dcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (g_group_dbg[3] < 0 || g_group_dbg[3] > ngroups) g_group_dbg[5] += 1;
      g_group_dbg[4] += 1;
    }
  }
#endif
  typedef __attribute__((address_space(3))) void lds_void;
  char* const wl = dma_lds + (threadIdx.x >> 6) * (3 * (EPL / 2) * 1024);  // (kDma / kPre) this wavefront's staging buffer
  // kPre (round 4, Binf on the one- and two-lane tiles of 8 elements per lane): the tile goes through the wavefront's buffer.
  //   tile_dma(t)  : the tile of wave iteration t -- GPW consecutive groups, GPW * npairs consecutive 16-byte pairs -- comes in
  //                  as whole kilobytes (lane l fetches pair 64 k + l) and lies linearly in the buffer (direct loads had every
  //                  lane fetch 16 bytes of its own 64-byte run per instruction: 32 lines touched four times each);
  //   tile_regs(t) : every lane picks up its own pairs (a 64-byte run per lane on the one-lane tiles: 4-way bank conflicts on
  //                  12 LDS reads, nothing next to the root find);
  // Groups of 8 at n = 1e8: 660 -> 636 us; of 6 / 12 / 14: -4 .. -7 %; y sent back the same way (parked in the buffer, stored as
  // whole kilobytes) changes nothing (634 us) and costs registers: the lanes store their own pairs.
  // (Tried on top and dropped: a resident grid whose wavefronts fetch tile i + 1 during the root find of tile i -- one buffer
  //  per wavefront is enough, the tile is copied to registers before the next DMA is issued; stores never waited for.  Bit
  //  identical and SLOWER: 665 us on groups of 8, and the second tile's registers spill on the partly filled tiles.  The
  //  hardware's own hand-out of one-tile workgroups hides the loads at least as well.)
  auto tile_dma = [&](int64_t t0) {
    const int64_t left = ntodo - t0;
    const int tile_pairs = (int)(left < GPW ? left : GPW) * npairs;  // (wave-uniform)
    const f64x2* tq = reinterpret_cast<const f64x2*>(q_ + t0 * GS);
    const f64x2* tx = reinterpret_cast<const f64x2*>(xk_ + t0 * GS);
    const f64x2* ts = reinterpret_cast<const f64x2*>(sj_ + t0 * GS);
#pragma unroll
    for (int k = 0; k < EPL / 2; ++k) {
      if (k * 64 < tile_pairs) {  // (wave-uniform)
        const int pp = (k * 64 + lane < tile_pairs) ? (k * 64 + lane) : 0;
        __builtin_amdgcn_global_load_lds((const void*)(tq + pp), (lds_void*)(wl + (0 * (EPL / 2) + k) * 1024), 16, 0, 2);
        __builtin_amdgcn_global_load_lds((const void*)(tx + pp), (lds_void*)(wl + (1 * (EPL / 2) + k) * 1024), 16, 0, 2);
        __builtin_amdgcn_global_load_lds((const void*)(ts + pp), (lds_void*)(wl + (2 * (EPL / 2) + k) * 1024), 16, 0, 2);
      }
    }
  };
  auto tile_regs = [&](int64_t t0, f64x2 (&nq)[EPL / 2], f64x2 (&nx)[EPL / 2], f64x2 (&ns)[EPL / 2]) {
    const int64_t left = ntodo - t0;
    const int slot_e = ((t0 + slot) < ntodo) ? slot : (int)(left - 1);  // idle slots shadow the last group of the tile
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < EPL / 2; ++k) {
      const int p = (FULL || k * LPG + j < npairs) ? (slot_e * npairs + k * LPG + j) : 0;  // masked pairs: zeroed below
      nq[k] = *reinterpret_cast<const f64x2*>(wl + (0 * (EPL / 2)) * 1024 + p * 16);
      nx[k] = *reinterpret_cast<const f64x2*>(wl + (1 * (EPL / 2)) * 1024 + p * 16);
      ns[k] = *reinterpret_cast<const f64x2*>(wl + (2 * (EPL / 2)) * 1024 + p * 16);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  bool handed_on = false;  // (VALUE) this lane put its group on the deferred list
  double hsum = 0.0;  // (VALUE) lane 0 of each group's lanes: sum of lambda_g * ||((xk + sj) + y)[g]|| over the groups stored here
  double qsum = 0.0, ysum = 0.0;  // (STEP) every lane: q[i] * y[i] and y[i]^2 over the elements it stored
  for (int64_t g0 = wave * GPW; g0 < ntodo; g0 += nwaves * GPW) {  // wave-uniform trip count
    bool valid = (g0 + slot) < ntodo;
    const int64_t gi = valid ? (g0 + slot) : (ntodo - 1);  // idle slots shadow the last group, no store
    int64_t g = gi;
    if constexpr (LIT) {
      g = (int64_t)deferred[1 + gi];
      if (g < 0 || g >= ngroups) {  // (never an id from outside the layout; reported, not skipped silently)
        if (valid && j == 0) spx_raise_status(status, kSpxStatusCorrupt);
        g = 0;
        valid = false;
      }
    }
    int64_t base = g * GS;
    int gs = gsize;  // this group's size (row-uniform)
    if constexpr (!PAIRS) {
      if (offsets) {  // ragged groups whose sizes the caller bounded by the tile (group_size hint)
        base = offsets[g];
        const int64_t sz = offsets[g + 1] - base;
        if (sz > LPG * EPL || sz < 0) {  // the hint was wrong for this group: the general kernel takes it
          if (valid && j == 0) { deferred[1 + atomicAdd(dcount, 1ull)] = g; handed_on = true; }
          valid = false;
          gs = 0;
        } else {
          gs = (int)sz;
        }
      }
    }
    RegGroup<EPL, BINF && !FULL && !LIT> grp;
    if constexpr (BINF && !FULL && !LIT) {  // live slots of the tile (wave-uniform: the launch's group size / size bound)
      const int slices = PAIRS ? (npairs + LPG - 1) / LPG : ((gsize + LPG - 1) / LPG + 1) / 2;
      grp.live = (2 * slices < EPL && offsets == nullptr) ? 2 * slices : EPL;  // (ragged groups: `gsize` is only the caller's hint -- a
                                                                                 //  group above it that still fits the tile is served here)
    }
    {
      if constexpr (PAIRS) {
        const f64x2* q2 = reinterpret_cast<const f64x2*>(q_ + base);
        const f64x2* x2 = reinterpret_cast<const f64x2*>(xk_ + base);
        const f64x2* s2 = reinterpret_cast<const f64x2*>(sj_ + base);
        f64x2 vq[EPL / 2], vx[EPL / 2], vs[EPL / 2];
        if constexpr (kPre) {
          tile_dma(g0);
          tile_regs(g0, vq, vx, vs);
        } else if constexpr (kDma) {
          // LDS-DMA staging (as k_sep_lds): piece k of a wave = the k-th 16-byte pair of each lane; lane `lane` of the
          // wave lands at byte 16*lane of the piece, whichever group slot it serves
#pragma unroll
          for (int k = 0; k < EPL / 2; ++k) {
            const int p = (FULL || k * LPG + j < npairs) ? (k * LPG + j) : 0;  // masked pairs re-read pair 0, zeroed below
            __builtin_amdgcn_global_load_lds((const void*)(q2 + p), (lds_void*)(wl + (0 * (EPL / 2) + k) * 1024), 16, 0, kPaddedCached ? 0 : 2);
            __builtin_amdgcn_global_load_lds((const void*)(x2 + p), (lds_void*)(wl + (1 * (EPL / 2) + k) * 1024), 16, 0, kPaddedCached ? 0 : 2);
            __builtin_amdgcn_global_load_lds((const void*)(s2 + p), (lds_void*)(wl + (2 * (EPL / 2) + k) * 1024), 16, 0, kPaddedCached ? 0 : 2);
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
          for (int k = 0; k < EPL / 2; ++k) {
            vq[k] = *reinterpret_cast<const f64x2*>(wl + (0 * (EPL / 2) + k) * 1024 + lane * 16);
            vx[k] = *reinterpret_cast<const f64x2*>(wl + (1 * (EPL / 2) + k) * 1024 + lane * 16);
            vs[k] = *reinterpret_cast<const f64x2*>(wl + (2 * (EPL / 2) + k) * 1024 + lane * 16);
          }
        } else {
#pragma unroll
          for (int k = 0; k < EPL / 2; ++k) {
            const int p = (FULL || k * LPG + j < npairs) ? (k * LPG + j) : 0;
            if constexpr (LPG <= 2 || kPaddedCached) {  // a lane's pairs share cache lines with each other, not with its neighbours': cached accesses
              vq[k] = q2[p]; vx[k] = x2[p]; vs[k] = s2[p];
            } else {
              vq[k] = __builtin_nontemporal_load(q2 + p);
              vx[k] = __builtin_nontemporal_load(x2 + p);
              vs[k] = __builtin_nontemporal_load(s2 + p);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < EPL / 2; ++k) {
          const bool in = FULL || (k * LPG + j) < npairs;
          const f64x2 zero2 = f64x2{0.0, 0.0};
          f64x2 a = in ? vq[k] : zero2;
          const f64x2 b = in ? vx[k] : zero2, c = in ? vs[k] : zero2;
          if constexpr (VALUE) { a.x = gv.qs * a.x; a.y = gv.qs * a.y; }  // (rounded here: never contracted into the sum below)
          grp.S[2 * k] = (a.x + b.x) + c.x;  // shiftedGroupNormL2.jl:65 / shiftedGroupNormL2Binf.jl:80
          grp.S[2 * k + 1] = (a.y + b.y) + c.y;
          grp.X[2 * k] = b.x;
          grp.X[2 * k + 1] = b.y;
          grp.XS[2 * k] = b.x + c.x;
          grp.XS[2 * k + 1] = b.y + c.y;
        }
      } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
          const int e = k * LPG + j;
          const bool in = e < gs;
          const int64_t i = base + (in ? e : 0);
          double a = in ? q_[i] : 0.0;
          const double b = in ? xk_[i] : 0.0, c = in ? sj_[i] : 0.0;
          if constexpr (VALUE) a = gv.qs * a;
          grp.S[k] = (a + b) + c;
          grp.X[k] = b;
          grp.XS[k] = b + c;
        }
      }
    }
    const double lam = lambda[g];
    double out[EPL];
    if constexpr (!BINF) {
      double ss = 0.0;
#pragma unroll
      for (int k = 0; k < EPL; ++k) ss += grp.S[k] * grp.S[k];
      const double snorm = sqrt(lanes_sum<LPG>(ss));                                       // shiftedGroupNormL2.jl:69
      const double alpha = (snorm == 0.0) ? 0.0 : jl_max(1 - sigma * lam / snorm, 0.0);  // :70-73
#pragma unroll
      for (int k = 0; k < EPL; ++k) out[k] = ((snorm == 0.0) ? 0.0 : alpha * grp.S[k]) - grp.XS[k];  // :74,:77
    } else if constexpr (LIT) {
      binf_literal_reg<LPG, EPL, false>(grp, lam, sigma, delta, out);
#pragma unroll
      for (int k = 0; k < EPL; ++k) out[k] = out[k] - grp.XS[k];  // :116
    } else {
      double ru;
      const int status = binf_root<LPG>(grp, lam, sigma, delta, nullptr, ru, pole_lit != 0);
      const double sl = lam * sigma;
      if (status == BINF_LITERAL) {
        // rare (degenerate bracket / exact zero / NaN): handed to k_group_list, which evaluates the reference's
        // expressions literally; keeping that code out of this kernel saves ~40 VGPRs
        // (one atomic per group.  A data set whose groups ALL defer is bound by this counter: the hardware already merges
        //  the atomics of a wavefront into one request, ~11 ns each on the one address -- 8e6 groups of 16 = 5e5 requests
        //  = 6 ms; merging them in software changes nothing.  Sharded lists would; not needed for the cases at hand.)
        if (valid && j == 0) { deferred[1 + atomicAdd(dcount, 1ull)] = g; handed_on = true; }
        valid = false;
      }
      if (status != BINF_ROOT || ru == 0.0) {  // shiftedGroupNormL2Binf.jl:102-103, :107-108
#pragma unroll
        for (int k = 0; k < EPL; ++k) out[k] = 0.0 - grp.XS[k];
      } else {
        const double tau = ru * fast_rcp(sl + ru);  // = alpha at the root (:83 with ||w|| = n)
#pragma unroll
        for (int k = 0; k < EPL; ++k) out[k] = binf_y(grp.S[k], grp.X[k], tau, delta) - grp.XS[k];  // :110-116
      }
    }
    if constexpr (VALUE) {
      // v = (xk + sj) + y of the elements this lane is about to store; slots past the end of the group add nothing
      double vv = 0.0;
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        const bool in = FULL || (PAIRS ? ((k >> 1) * LPG + j) < npairs : (k * LPG + j) < gs);
        const double v = grp.XS[k] + out[k];
        vv += in ? v * v : 0.0;
      }
      vv = lanes_sum<LPG>(vv);
      if constexpr (LIT) {  // (a handed-on group: its term has a slot of its own, see GroupVal)
        if (valid && j == 0) spx_atomic_store_f64(&gv.dterm[g], lam * sqrt(vv));
      } else {
        if (valid && j == 0) hsum += lam * sqrt(vv);
      }
    }
    if (valid) {
      if constexpr (PAIRS) {
        f64x2* y2 = reinterpret_cast<f64x2*>(y_ + base);
#pragma unroll
        for (int k = 0; k < EPL / 2; ++k)
          if (FULL || k * LPG + j < npairs) {
            if constexpr (LPG <= 2 || kPaddedCached) y2[k * LPG + j] = f64x2{out[2 * k], out[2 * k + 1]};  // (merged into whole lines by the L2)
            else __builtin_nontemporal_store(f64x2{out[2 * k], out[2 * k + 1]}, y2 + k * LPG + j);
          }
      } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k)
          if (k * LPG + j < gs) y_[base + k * LPG + j] = out[k];
      }
    }
    if constexpr (STEP) {
      if (valid && gv.xkn != nullptr) {  // v as the h term formed it, stored the way y is
        if constexpr (PAIRS) {
          f64x2* v2 = reinterpret_cast<f64x2*>(gv.xkn + base);
#pragma unroll
          for (int k = 0; k < EPL / 2; ++k)
            if (FULL || k * LPG + j < npairs) {
              const f64x2 v = f64x2{grp.XS[2 * k] + out[2 * k], grp.XS[2 * k + 1] + out[2 * k + 1]};
              if constexpr (LPG <= 2 || kPaddedCached) v2[k * LPG + j] = v;
              else __builtin_nontemporal_store(v, v2 + k * LPG + j);
            }
        } else {
#pragma unroll
          for (int k = 0; k < EPL; ++k)
            if (k * LPG + j < gs) gv.xkn[base + k * LPG + j] = grp.XS[k] + out[k];
        }
      }
      asm volatile("" ::: "memory");  // (q is read AGAIN below: the values loaded above are not kept alive across the root find)
      double qy = 0.0, yy = 0.0;
      if constexpr (PAIRS) {
        const f64x2* q2 = reinterpret_cast<const f64x2*>(q_ + base);
        [[maybe_unused]] const int slot_e = ((g0 + slot) < ntodo) ? slot : (int)(ntodo - g0 - 1);  // (kPre: as tile_regs)
#pragma unroll
        for (int k = 0; k < EPL / 2; ++k) {
          const bool in = FULL || (k * LPG + j) < npairs;
          const int p = in ? (k * LPG + j) : 0;
          f64x2 a;
          if constexpr (kPre) a = *reinterpret_cast<const f64x2*>(wl + (slot_e * npairs + p) * 16);
          else if constexpr (kDma) a = *reinterpret_cast<const f64x2*>(wl + k * 1024 + lane * 16);
          else if constexpr (LPG <= 2 || kPaddedCached) a = q2[p];
          else a = __builtin_nontemporal_load(q2 + p);
          qy += in ? a.x * out[2 * k] : 0.0;
          qy += in ? a.y * out[2 * k + 1] : 0.0;
          yy += in ? out[2 * k] * out[2 * k] : 0.0;
          yy += in ? out[2 * k + 1] * out[2 * k + 1] : 0.0;
        }
      } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
          const bool in = (k * LPG + j) < gs;
          const double a = q_[base + (in ? k * LPG + j : 0)];
          qy += in ? a * out[k] : 0.0;
          yy += in ? out[k] * out[k] : 0.0;
        }
      }
      if constexpr (LIT) {  // (a handed-on group: two more slots of its own)
        qy = lanes_sum<LPG>(qy);
        yy = lanes_sum<LPG>(yy);
        if (valid && j == 0) {
          spx_atomic_store_f64(&gv.dterm[gv.dplane + g], qy);
          spx_atomic_store_f64(&gv.dterm[2 * gv.dplane + g], yy);
        }
      } else if (valid) {
        qsum += qy;
        ysum += yy;
      }
    }
  }
  if constexpr (VALUE) {
    if constexpr (!LIT) {  // (the host gives every wavefront one tile in these launches: tile = wavefront)
      if (gv.dmask != nullptr) {
        const unsigned long long m = __ballot(handed_on);
        if (lane == 0) gv.dmask[wave] = m;
      }
    }
    if constexpr (STEP) {
      double acc[3] = {hsum, qsum, ysum};
      gval_finish(acc, handed_on, gv);
    } else {
      double acc[1] = {hsum};
      gval_finish(acc, handed_on, gv);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// general kernels: TEAM lanes per group, elements re-read from memory for every reduction.
//   k_group_mem    : contiguous groups (CSR offsets or uniform size)
//   k_group_gather : arbitrary index sets (the reference's idx::Vector{Vector{Int}}, src/groupNormL2.jl:30-31)
// Both run group_body on an element provider (MemGroup / GatherGroup).
// ---------------------------------------------------------------------------------------------
// Gather provider.  `sol` = (q + xk) + sj was materialised by k_gather_prepare (as the reference's psi.sol, :65 -- so
// y may alias q and groups may overlap); owner[j] = the LAST group containing j: only that group stores y[j], which is
// what the reference's sequential loop over the groups leaves behind.
template <int TEAM>
struct GatherGroup {
  static constexpr bool kReg = false;
  static constexpr int kEpl = 1;
  const double* sol;
  const double* xk;
  const double* sj;
  const int64_t* index;
  const int* owner;
  int64_t lo, hi;  // positions in `index`
  int lane;
  int g;
  template <class F>
  __device__ __forceinline__ void for_each(F&& f) const {
    for (int64_t p = lo + lane; p < hi; p += TEAM) {
      const int64_t j = index[p];
      f(sol[j], xk[j]);
    }
  }
  // y[j] = f(S, X) - (xk + sj) for every owned element
  template <class F>
  __device__ __forceinline__ void store(double* y, F&& f) const {
    for (int64_t p = lo + lane; p < hi; p += TEAM) {
      const int64_t j = index[p];
      const double x = xk[j], s = sj[j];
      const double v = f(sol[j], x) - (x + s);
      if (owner[j] == g) y[j] = v;
    }
  }
};


template <int TEAM, bool BINF>
__global__ __launch_bounds__(256) void k_group_mem(double* y, const double* q, const double* xk, const double* sj,
                                                    int64_t n, const int64_t* __restrict__ offsets, int64_t gsize,
                                                    int64_t ngroups, const double* __restrict__ lambda, double sigma,
                                                    double delta, const long long* list /* NULL, or [0] = count, [1..] */,
                                                    int* status /* spx_ctx::status_dev */, int pole_lit,
                                                    const int* big_active /* NULL, or a device word: skip groups of >= big_min elements (spx_group_team.hip has them) */,
                                                    int64_t big_min) {
  __shared__ double lds[8];
  const bool skip_big = big_active != nullptr && *big_active != 0;
  constexpr int TPB = 256 / TEAM;  // teams per block
  const int lane = threadIdx.x % TEAM;
  const int64_t team = (int64_t)blockIdx.x * TPB + threadIdx.x / TEAM;
  const int64_t nteams = (int64_t)gridDim.x * TPB;
  const int64_t nlist = list ? (int64_t)list[0] : 0;
  const bool bad_count = list && (nlist < 0 || nlist > ngroups);  // (as k_group_reg: reported through the status word)
  if (bad_count && blockIdx.x == 0 && threadIdx.x == 0) spx_raise_status(status, kSpxStatusCorrupt);
  const int64_t ntodo = list ? (bad_count ? 0 : nlist) : ngroups;
  for (int64_t t = team; t < ntodo; t += nteams) {  // for TEAM == 256 the trip count is block-uniform
    const int64_t g = list ? (int64_t)list[1 + t] : t;
    if (g < 0 || g >= ngroups) {  // (never an id from outside the layout; block-uniform for TEAM == 256)
      if (lane == 0) spx_raise_status(status, kSpxStatusCorrupt);
      continue;
    }
    int64_t lo, hi;
    if (offsets) { lo = offsets[g]; hi = offsets[g + 1]; }
    else { lo = g * gsize; hi = lo + gsize; }
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    if (skip_big && hi - lo >= big_min) continue;  // (team- and block-uniform)
    MemGroup<TEAM> grp{q, xk, sj, lo, hi, lane};
    group_body<TEAM, BINF>(grp, y, lambda[g], sigma, delta, lds, list != nullptr, pole_lit != 0);
    if constexpr (TEAM == 256) __syncthreads();
  }
}

// spx_proxval_group_l2[_binf], ragged layouts with a size bound: the groups the register tiles handed on (above the bound /
// literal evaluation), as k_group_mem<64> does with a list -- a wavefront per group, the prox taken at qs * q -- plus each
// group's term of the value from the y just stored (every lane re-reads its own elements); the call's last launch.
template <int TEAM>
struct ScaledMemGroup {  // MemGroup at qs * q
  static constexpr bool kReg = false;
  static constexpr int kEpl = 1;
  const double* q;
  const double* xk;
  const double* sj;
  int64_t lo, hi;
  int lane;
  double qs;
  template <class F>
  __device__ __forceinline__ void for_each(F&& f) const {
    for (int64_t i = lo + lane; i < hi; i += TEAM) {
      const double x = xk[i], a = qs * q[i];
      f((a + x) + sj[i], x);
    }
  }
  template <class F>
  __device__ __forceinline__ void store(double* y, F&& f) const {
    for (int64_t i = lo + lane; i < hi; i += TEAM) {
      const double x = xk[i], s = sj[i], a = qs * q[i];
      const double S = (a + x) + s;
      y[i] = f(S, x) - (x + s);
    }
  }
};
template <bool BINF>
__global__ __launch_bounds__(256) void k_group_list_val(double* y, const double* q, const double* xk, const double* sj,
                                                         int64_t n, const int64_t* __restrict__ offsets, int64_t gsize,
                                                         int64_t ngroups, const double* __restrict__ lambda, double sigma,
                                                         double delta, const long long* list /* [0] = count, [1..] */,
                                                         int* status, int pole_lit, GroupVal gv) {
  __shared__ double lds[8];
  constexpr int TEAM = 64, TPB = 256 / TEAM;
  const int lane = threadIdx.x % TEAM;
  const int64_t team = (int64_t)blockIdx.x * TPB + threadIdx.x / TEAM;
  const int64_t nteams = (int64_t)gridDim.x * TPB;
  const int64_t nlist = (int64_t)list[0];
  const bool bad_count = nlist < 0 || nlist > ngroups;  // (as k_group_reg: reported through the status word)
  if (bad_count && blockIdx.x == 0 && threadIdx.x == 0) spx_raise_status(status, kSpxStatusCorrupt);
  const int64_t ntodo = bad_count ? 0 : nlist;
  for (int64_t t = team; t < ntodo; t += nteams) {
    const int64_t g = (int64_t)list[1 + t];
    if (g < 0 || g >= ngroups) {
      if (lane == 0) spx_raise_status(status, kSpxStatusCorrupt);
      continue;
    }
    int64_t lo, hi;
    if (offsets) { lo = offsets[g]; hi = offsets[g + 1]; }
    else { lo = g * gsize; hi = lo + gsize; }
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    ScaledMemGroup<TEAM> grp{q, xk, sj, lo, hi, lane, gv.qs};
    group_body<TEAM, BINF>(grp, y, lambda[g], sigma, delta, lds, true, pole_lit != 0);
    double vv = 0.0;
    for (int64_t i = lo + lane; i < hi; i += TEAM) {  // (this lane's own stores)
      const double v = (xk[i] + sj[i]) + y[i];
      vv += v * v;
    }
    vv = lanes_sum<TEAM>(vv);
    if (lane == 0) spx_atomic_store_f64(&gv.dterm[g], lambda[g] * sqrt(vv));  // (its own slot: GroupVal)
  }
  double none[1] = {0.0};
  gval_finish(none, false, gv);
}
// y = c * q, elementwise (the composed routes of spx_proxval_group_* with q_scale != 1: the prox then runs at q := y)
// CSR layouts: only over [offsets[0], offsets[ngroups]) -- the indices no group contains keep the caller's y for the operator.
__global__ __launch_bounds__(256) void k_group_scale(double* y, const double* q, double c, int64_t n,
                                                      const int64_t* __restrict__ offsets, int64_t ngroups) {
  int64_t lo = 0, hi = n;
  if (offsets) {
    lo = offsets[0]; hi = offsets[ngroups];
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride) y[i] = c * q[i];
}

// Large uniform groups (512 < size <= kLdsGroupMax): one workgroup per group, S = (q + xk) + sj and X = xk staged in
// LDS once (q, xk, sj are read from HBM exactly once; the final store re-reads sj only), every reduction of the root
// find then runs out of LDS instead of re-reading the group from L2.
// Measured (1.28e8 elements, TB/s, LDS kernel vs general kernel): size 1000: 4.8 vs 3.9 (L2), 2.5 vs 1.5 (Binf);
// 2048: 5.0 / 3.3; 4096: 3.3 vs 3.9 / 2.6 vs 1.5; 8192: 2.4 vs 3.9 / 1.6 vs 1.5 -- the LDS footprint leaves one or two
// workgroups per CU, so the plain form switches back to the general kernel above 2048 and the Binf form above 4096.
constexpr int kLdsGroupMax = 4096;  // elements (Binf); 2 x 32 KiB of LDS
constexpr int kLdsGroupMaxPlain = 2048;
struct LdsGroup {
  static constexpr bool kReg = false;
  static constexpr int kEpl = 1;
  const double* S;   // LDS
  const double* X;   // LDS
  const double* sj;  // global, group base
  int64_t lo;        // first element of the group
  int m, tid;
  template <class F>
  __device__ __forceinline__ void for_each(F&& f) const {
    for (int i = tid; i < m; i += 256) f(S[i], X[i]);
  }
  template <class F>
  __device__ __forceinline__ void store(double* y, F&& f) const {
    for (int i = tid; i < m; i += 256) {
      const double x = X[i], s = sj[i];
      y[lo + i] = f(S[i], x) - (x + s);
    }
  }
};

template <bool BINF>
__global__ __launch_bounds__(256) void k_group_lds(double* y, const double* q, const double* xk, const double* sj,
                                                    int64_t n, const int64_t* __restrict__ offsets /* NULL: uniform */,
                                                    int64_t gsize /* group size, or the bound on it with offsets */,
                                                    int64_t ngroups, const double* __restrict__ lambda, double sigma,
                                                    double delta, int pole_lit) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];  // S[gsize] | X[gsize]
  __shared__ double lds[8];
  double* S = dyn;
  double* X = dyn + gsize;
  const int tid = threadIdx.x;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    int64_t lo = g * gsize, sz = gsize;
    if (offsets) {
      lo = offsets[g];
      int64_t hi = offsets[g + 1];
      if (lo < 0) lo = 0;
      if (hi > n) hi = n;
      sz = hi > lo ? hi - lo : 0;
      if (sz > gsize) {  // the caller's bound was wrong for this group: straight from memory, as the general kernel
        MemGroup<256> big{q, xk, sj, lo, hi, tid};
        group_body<256, BINF>(big, y, lambda[g], sigma, delta, lds, false, pole_lit != 0);
        __syncthreads();
        continue;
      }
    }
    const int m = (int)sz;
    for (int i = tid; i < m; i += 256) {
      const double x = xk[lo + i];
      S[i] = (q[lo + i] + x) + sj[lo + i];  // shiftedGroupNormL2.jl:65 / shiftedGroupNormL2Binf.jl:80
      X[i] = x;
    }
    __syncthreads();  // the group is staged (and q fully read: y may alias q)
    LdsGroup grp{S, X, sj + lo, lo, m, tid};
    group_body<256, BINF>(grp, y, lambda[g], sigma, delta, lds, false, pole_lit != 0);
    __syncthreads();  // all reads of S / X done before the next group overwrites them
  }
}

// sol = (q + xk) + sj (:65 / :80), owner = -1
__global__ __launch_bounds__(256) void k_gather_prepare(double* __restrict__ sol, int* __restrict__ owner,
                                                         const double* q, const double* xk, const double* sj, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    sol[i] = (q[i] + xk[i]) + sj[i];
    owner[i] = -1;
  }
}

// owner[j] = max{g : j in idx_g}; flags an index outside [0, n) (the reference: BoundsError)
__global__ __launch_bounds__(256) void k_gather_owner(int* owner, const int64_t* __restrict__ ptr,
                                                       const int64_t* __restrict__ index, int64_t ngroups, int64_t n,
                                                       int64_t nnz, int* flag) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    int64_t lo = ptr[g], hi = ptr[g + 1];
    if (lo < 0 || hi > nnz || lo > hi) { if (lane == 0) atomicOr(flag, 2); continue; }
    for (int64_t p = lo + lane; p < hi; p += 64) {
      const int64_t j = index[p];
      if ((j < 0 || j >= n) && (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1) == 0) atomicOr(flag, 1);
      else atomicMax(owner + j, (int)g);
    }
  }
}

template <int TEAM, bool BINF>
__global__ __launch_bounds__(256) void k_group_gather(double* y, const double* sol, const double* xk, const double* sj,
                                                       const int* owner, const int64_t* __restrict__ ptr,
                                                       const int64_t* __restrict__ index, int64_t ngroups,
                                                       const double* __restrict__ lambda, double sigma, double delta,
                                                       int pole_lit) {
  __shared__ double lds[8];
  constexpr int TPB = 256 / TEAM;
  const int lane = threadIdx.x % TEAM;
  const int64_t team = (int64_t)blockIdx.x * TPB + threadIdx.x / TEAM;
  const int64_t nteams = (int64_t)gridDim.x * TPB;
  for (int64_t g = team; g < ngroups; g += nteams) {
    GatherGroup<TEAM> grp{sol, xk, sj, index, owner, ptr[g], ptr[g + 1], lane, (int)g};
    group_body<TEAM, BINF>(grp, y, lambda[g], sigma, delta, lds, false, pole_lit != 0);
    if constexpr (TEAM == 256) __syncthreads();
  }
}

// indices no group contains keep the caller's y (the reference never assigns them) minus the shift (:77 / :116)
__global__ __launch_bounds__(256) void k_gather_rest(double* y, const double* xk, const double* sj, const int* owner,
                                                      int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (owner[i] < 0) y[i] = y[i] - (xk[i] + sj[i]);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The arguments of a contiguous-group call (spx_prox_group_l2[_binf], spx_proxval_group_l2[_binf]).
struct GroupCall {
  spx_ctx* ctx;
  double* y;
  const double *q, *xk, *sj;
  int64_t n;
  const int64_t* offsets;
  int64_t gsize, ngroups;
  const double* lambda;
  double sigma, delta;
};

// Register tiles: GroupTile, GroupTiles and the tables GroupTilesPlain, GroupTilesBinf and GroupTilesLit are
// spx_group_common.hpp's (the batched calls, spx_gbatch.hip and spx_gbinf_batch.hip, walk the same tables).

// What the k_group_reg launches of a call share.
struct GroupRegArgs {
  const GroupCall& c;
  long long* deferred;
  unsigned long long* dcount;
  bool pairs;  // 16-byte loads: uniform groups of even size in 16-byte aligned vectors; otherwise 8-byte loads
};
// One k_group_reg launch.  PAIRS by the loads; FULL (main launches only) when the groups fill the tile; `gv` is passed on by VALUE.
// (a GroupStep: the step form).  dclear: the LIT launch's, NULL for a main launch.
template <int LPG, int EPL, bool BINF, bool LIT, bool VALUE, class GV>
static void launch_group_reg(const GroupRegArgs& a, dim3 grid, unsigned long long* dclear, const GV& gv) {
  const GroupCall& c = a.c;
  constexpr bool STEP = VALUE && std::is_same<GV, GroupStep>::value;
  typename std::conditional<VALUE, GV, GroupNoVal>::type v{};
  if constexpr (VALUE) v = gv;
  auto launch = [&](auto pairs, auto full) {
    hipLaunchKernelGGL((k_group_reg<LPG, EPL, BINF, decltype(pairs)::value, LIT, decltype(full)::value, VALUE, STEP>), grid, dim3(256), 0,
                       c.ctx->stream, c.y, c.q, c.xk, c.sj, c.ngroups, (int)c.gsize, c.lambda, c.sigma, c.delta, a.deferred,
                       c.offsets, c.ctx->status_dev, c.ctx->tune_binf_literal, a.dcount, dclear, v);
  };
  if (!a.pairs) return launch(std::false_type{}, std::false_type{});
  if constexpr (!LIT) {
    if (c.gsize == LPG * EPL) return launch(std::true_type{}, std::true_type{});
  }
  launch(std::true_type{}, std::false_type{});
}

// ShiftedGroupNormL2 with CSR offsets, which need not span 0:n (src/shiftedGroupNormL2.jl:77 runs over every index): the
// indices no group covers.  Enqueued only; the caller's SPX_LAUNCH_CHECK follows.
template <bool BINF>
static void group_uncovered(const GroupCall& c) {
  if (!BINF && c.offsets)
    hipLaunchKernelGGL(k_csr_uncovered<double>, dim3(256), dim3(256), 0, c.ctx->stream, c.y, c.xk, c.sj, c.offsets, c.ngroups, c.n);
}

// The routes of a contiguous-group call, by the group size (uniform) or the caller's bound on the sizes (CSR offsets).
enum class GroupRoute {
  None,     // n == 0 or no group at all
  Reg,      // at most kGroupRegMax elements: register tiles
  Lds,      // up to kLdsGroupMax[Plain]: LDS-resident group per workgroup
  General,  // larger, or ragged without a bound: wavefront / workgroup per group, teams of workgroups for the large ones
};
// Validates the arguments and names the route.  Enqueues nothing.
template <bool BINF>
static int group_classify(const GroupCall& c, GroupRoute* route) {
  int rc = spx_check_common(c.ctx, c.y, c.q, c.xk, c.sj, c.n);
  if (rc) return rc;
  SPX_REQUIRE(c.ngroups >= 0, "ngroups < 0");
  *route = GroupRoute::None;
  if (c.n == 0 || c.ngroups == 0) return SPX_OK;
  SPX_REQUIRE(c.lambda != nullptr, "lambda_vec is NULL");
  if (!c.offsets) {
    SPX_REQUIRE(c.gsize > 0, "group_size <= 0 with NULL group_offsets");
    SPX_REQUIRE(c.ngroups <= c.n / c.gsize && c.ngroups * c.gsize == c.n, "ngroups * group_size != n");
  }
  if (c.gsize > 0 && c.gsize <= kGroupRegMax) *route = GroupRoute::Reg;
  else if (c.gsize > kGroupRegMax && c.gsize <= (BINF ? kLdsGroupMax : kLdsGroupMaxPlain)) *route = GroupRoute::Lds;
  else *route = GroupRoute::General;
  return SPX_OK;
}

// y may alias q on every route: every kernel finishes all reductions of a group (team barrier / wave lockstep) before
// the group's first store, and the storing lane re-reads q[i] itself just before writing y[i].

// Register tiles.  Ragged groups (CSR offsets + an upper bound on the sizes in group_size) use the same tiles through the 8-byte
// loads; a group that exceeds the bound after all is handed to the general kernel.
// VALUE (run_group_val below): the launches also form h at the result, see GroupVal; dest: where it goes.
// STEP (run_group_step below, uniform groups only): ... and xkn and the two other sums, see GroupStep; dest: the three statistics.
template <bool BINF, bool VALUE, bool STEP = false>
static int group_route_reg(const GroupCall& c, double q_scale = 1.0, const SpxDest& dest = {nullptr, nullptr, 0}, double* xkn = nullptr) {
  static_assert(VALUE || !STEP, "the step form extends the value form");
  using GV = typename std::conditional<STEP, GroupStep, GroupVal>::type;
  constexpr int NS = STEP ? 3 : 1;  // sums per workgroup / handed-on group
  using Tiles = typename std::conditional<BINF, GroupTilesBinf, GroupTilesPlain>::type;
  spx_ctx* ctx = c.ctx;
  const int64_t ngroups = c.ngroups;
  SPX_ON_DEVICE(ctx);
  const bool ragged = c.offsets != nullptr;  // ragged groups with a size bound from the caller
  const int lpg = Tiles::lpg(c.gsize);
  const int gpw = 64 / lpg;
  int64_t blocks = (ngroups + 4 * gpw - 1) / (4 * gpw);  // 4 waves per 256-thread block
  if (blocks > 0x7fffffff) blocks = 0x7fffffff;
  const dim3 grid((unsigned)blocks);
  int rc;
  long long* deferred = nullptr;
  unsigned long long *dcount = nullptr, *dclear = nullptr;
  // VALUE: one reservation -- [deferred list | GroupValWs | partials and flags of the main launch | tile masks | dterm]
  GV gv_main{}, gv_last{};
  [[maybe_unused]] GroupValWs* vws = nullptr;  // (STEP: a GroupStepWs)
  if constexpr (VALUE) {
    const size_t list_bytes = (BINF || ragged) ? (((size_t)(ngroups + 1) * sizeof(long long) + 256 + 255) & ~(size_t)255) : 0;
    // (a wavefront per tile: the masks of the handed-on groups are indexed by wavefront)
    SPX_REQUIRE(blocks * 4 * gpw >= ngroups, "too many groups for the fused value form");
    const size_t head_bytes = STEP ? sizeof(GroupStepWs) : sizeof(GroupValWs);
    const size_t part_bytes = ((size_t)blocks * (NS + 1) * sizeof(double) + 255) & ~(size_t)255;  // partials (NS planes) | flags
    const size_t mask_bytes = list_bytes ? (size_t)blocks * 4 * sizeof(unsigned long long) : 0;
    rc = spx_ws_reserve(ctx, list_bytes + head_bytes + part_bytes + mask_bytes + (list_bytes ? (size_t)ngroups * NS * sizeof(double) : 0) + 256);
    if (rc) return rc;
    rc = spx_sync_ready(ctx);
    if (rc) return rc;
    vws = reinterpret_cast<GroupValWs*>(static_cast<char*>(ctx->ws) + list_bytes);
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(vws) + head_bytes);
    const bool one = !(BINF || ragged);  // the main launch is the call's last one
    unsigned long long* dmask = one ? nullptr : reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(part) + part_bytes);
    double* dterm = one ? nullptr : reinterpret_cast<double*>(reinterpret_cast<char*>(part) + part_bytes + mask_bytes);
    static_cast<GroupVal&>(gv_main) = GroupVal{q_scale, part, one ? nullptr : part + NS * blocks, (int)blocks, false, one ? spx_sync_header(ctx) : nullptr, vws,
                                               STEP ? nullptr : dest.dev, dmask, dterm, lpg};
    if constexpr (STEP) {
      gv_main.xkn = xkn;
      gv_main.stats_dev = dest.dev;
      gv_main.sws = reinterpret_cast<GroupStepWs*>(vws);
      gv_main.dplane = ngroups;
    }
    gv_last = gv_main;
    gv_last.behind = true;
    gv_last.hdr = spx_sync_header(ctx);
  }
  if (BINF || ragged) {  // list of the groups whose bracket needs the reference's literal evaluation / oversize groups
    if constexpr (!VALUE) {
      rc = spx_ws_reserve(ctx, (size_t)(ngroups + 1) * sizeof(long long) + 256);
      if (rc) return rc;
    }
    deferred = reinterpret_cast<long long*>(ctx->ws);
    dcount = reinterpret_cast<unsigned long long*>(deferred);
    // Round 4: the zero-fill of the count word was a launch of its own in front of every call (a Binf call at solver sizes:
    // 17 us against 10.5 for the plain operator, tools/r4/small_latency_all.py).  Uniform Binf layouts now count in one of
    // two words of the synchronisation state (zero-initialised, never written by another operator): a call uses [set], its
    // LIT launch -- queued unconditionally behind the main one -- zeroes [set ^ 1] for the next call.  Under a stream capture
    // (one set would replay for ever) and for ragged layouts the word in front of the list and its zero-fill node stay.
    const bool graph_safe = spx_graph_safe(ctx);
    if (BINF && !ragged && ctx->tune_fewer_launches && !graph_safe) {
      rc = spx_sync_ready(ctx);
      if (rc) return rc;
      SpxSyncHeader* hdr = spx_sync_header(ctx);
      dcount = reinterpret_cast<unsigned long long*>(&hdr->grp_deferred[ctx->track.grp_def_set]);
      dclear = reinterpret_cast<unsigned long long*>(&hdr->grp_deferred[ctx->track.grp_def_set ^ 1]);
      ctx->track.grp_def_set ^= 1;
    } else {
      rc = spx_zero_async(ctx, deferred, sizeof(long long)); if (rc) return rc;
    }
  }
  const bool aligned = spx_aligned16(c.y) && spx_aligned16(c.q) && spx_aligned16(c.xk) && spx_aligned16(c.sj) && spx_aligned16(xkn);
  const GroupRegArgs args{c, deferred, dcount, !ragged && (c.gsize & 1) == 0 && aligned};
  group_uncovered<BINF>(c);
  Tiles::select(c.gsize, [&](auto row) {
    launch_group_reg<decltype(row)::lpg, decltype(row)::epl, BINF, false, VALUE>(args, grid, nullptr, gv_main);
  });
  if (BINF && !ragged) {
    // The deferred list (usually empty: the kernel returns at once) on register tiles as well.  The literal
    // evaluation is ~60 dependent passes over a group; from memory (k_group_mem) a long list is bound by L2 misses.
    if constexpr (BINF) {
      const dim3 lgrid((unsigned)(blocks < (int64_t)ctx->num_cu * 8 ? blocks : (int64_t)ctx->num_cu * 8));
      GroupTilesLit::select(c.gsize, [&](auto row) {
        launch_group_reg<decltype(row)::lpg, decltype(row)::epl, true, true, VALUE>(args, lgrid, dclear, gv_last);
      });
    }
  } else if (ragged) {  // usually an empty list: the kernel returns at once
    if constexpr (VALUE)
      hipLaunchKernelGGL((k_group_list_val<BINF>), dim3((unsigned)(ctx->num_cu * 2)), dim3(256), 0, ctx->stream, c.y, c.q, c.xk,
                         c.sj, c.n, c.offsets, c.gsize, ngroups, c.lambda, c.sigma, c.delta, (const long long*)deferred,
                         ctx->status_dev, ctx->tune_binf_literal, gv_last);
    else
      hipLaunchKernelGGL((k_group_mem<64, BINF>), dim3((unsigned)(ctx->num_cu * 2)), dim3(256), 0, ctx->stream, c.y, c.q, c.xk,
                         c.sj, c.n, c.offsets, c.gsize, ngroups, c.lambda, c.sigma, c.delta, (const long long*)deferred,
                         ctx->status_dev, ctx->tune_binf_literal, (const int*)nullptr, (int64_t)0);
  }
  SPX_LAUNCH_CHECK();
  // (STEP: GroupStepWs::result takes the place of GroupValWs::result, both at offset 0 -- static_assert at the structs)
  if constexpr (VALUE) return spx_dest_return(ctx, dest, &vws->result, (size_t)dest.count * sizeof(double));
  return SPX_OK;
}

// kGroupRegMax < group size (uniform) or size bound (ragged, CSR offsets) <= kLdsGroupMax[Plain]: LDS-resident group per workgroup
template <bool BINF>
static int group_route_lds(const GroupCall& c) {
  spx_ctx* ctx = c.ctx;
  SPX_ON_DEVICE(ctx);
  group_uncovered<BINF>(c);
  const size_t dyn = (size_t)c.gsize * 2 * sizeof(double);
  // per device (the attribute belongs to the function ON the current device) and cheap: set on every call that needs it,
  // no process-wide cache that a second GPU or a second thread would find in the wrong state
  if (dyn > 48 * 1024)
    SPX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_group_lds<BINF>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsGroupMax * 2 * (int)sizeof(double)));
  const int64_t cap_blocks = (int64_t)ctx->num_cu * 8;
  const int64_t blocks = c.ngroups < cap_blocks ? c.ngroups : cap_blocks;
  hipLaunchKernelGGL((k_group_lds<BINF>), dim3((unsigned)blocks), dim3(256), dyn, ctx->stream, c.y, c.q, c.xk, c.sj, c.n, c.offsets,
                     c.gsize, c.ngroups, c.lambda, c.sigma, c.delta, ctx->tune_binf_literal);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}

// Everything else: ragged groups without a size bound from the caller (or with one above the LDS-resident form's), and
// large groups -- first of all ONE group over the whole vector, the reference's default GroupNormL2
// (src/groupNormL2.jl:30-31, shifted(NormL2(lambda), xk): src/shiftedGroupNormL2.jl:34-35): a team of workgroups per
// group (spx_group_team.hip) instead of one workgroup (n = 1e8: 384 ms plain / 1349 ms Binf that way).
template <bool BINF>
static int group_route_general(const GroupCall& c) {
  spx_ctx* ctx = c.ctx;
  const int64_t ngroups = c.ngroups;
  SPX_ON_DEVICE(ctx);
  const int* big_active = nullptr;   // ragged layouts: device word of the team plan, "the large groups are taken care of"
  const int64_t big_min = (BINF ? kLdsGroupMax : kLdsGroupMaxPlain) + 1;  // ragged layouts: a group of at least this many elements is
                                                                          // a large one (what the LDS-resident kernel does not hold, as for uniform groups)
  if (ctx->tune_team) {
    if (!c.offsets) {
      const int tg = spx_group_team_max_grid(ctx, BINF);
      // (teams of ONE workgroup that take several groups in turn beat the one-workgroup-per-group kernels below at every count
      //  of large groups -- 1e8 elements in groups of 5000 ... 200 000: plain 0.88-1.07 -> 0.62-0.99 ms, Binf 2.0-3.4 -> 1.0-1.8 ms,
      //  tools/r4/team_crossover.py -- on chip up to 9216 elements, two passes instead of one per reduction beyond; tuning key 16
      //  = groups per workgroup up to which the team form is used, for that A/B)
      if (tg >= 1 && (ctx->tune_team_factor == 0 || ngroups < (int64_t)ctx->tune_team_factor * tg))
        return spx_group_team_launch(ctx, BINF, c.y, c.q, c.xk, c.sj, c.n, nullptr, c.gsize, ngroups, c.lambda, c.sigma, c.delta);
    } else if (ngroups <= 65536) {
      const int rc = spx_group_team_plan(ctx, BINF, c.y, c.q, c.xk, c.sj, c.n, c.offsets, ngroups, big_min, &big_active);
      if (rc) return rc;
    }
  }
  group_uncovered<BINF>(c);
  const int team = spx_group_lanes_by_avg((double)c.n / (double)ngroups);
  const int tpb = 256 / team;
  const int64_t cap_blocks = (int64_t)ctx->num_cu * 8;
  int64_t blocks = (ngroups + tpb - 1) / tpb;
  if (blocks > cap_blocks) blocks = cap_blocks;
  spx_with_lanes<4, 8, 16, 32, 64, 256>(team, [&](auto lanes) {
    hipLaunchKernelGGL((k_group_mem<decltype(lanes)::value, BINF>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, c.y, c.q, c.xk,
                       c.sj, c.n, c.offsets, c.gsize, ngroups, c.lambda, c.sigma, c.delta, (const long long*)nullptr, ctx->status_dev,
                       ctx->tune_binf_literal, big_active, big_min);
  });
  SPX_LAUNCH_CHECK();
  if (big_active)  // the large groups of a ragged layout (the kernel returns at once when the plan found none)
    return spx_group_team_launch(ctx, BINF, c.y, c.q, c.xk, c.sj, c.n, c.offsets, c.gsize, ngroups, c.lambda, c.sigma, c.delta);
  return SPX_OK;
}

// The prox on the route group_classify named.
template <bool BINF>
static int group_run(const GroupCall& c, GroupRoute route) {
  switch (route) {
    case GroupRoute::Reg: return group_route_reg<BINF, false>(c);
    case GroupRoute::Lds: return group_route_lds<BINF>(c);
    case GroupRoute::General: return group_route_general<BINF>(c);
    case GroupRoute::None: break;
  }
  // no group at all: ShiftedGroupNormL2 still subtracts the shift everywhere (:77)
  if (c.n == 0 || BINF || !c.offsets) return SPX_OK;
  SPX_ON_DEVICE(c.ctx);
  group_uncovered<BINF>(c);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}

template <bool BINF>
static int run_group(const GroupCall& c) {
  GroupRoute route;
  const int rc = group_classify<BINF>(c, &route);
  if (rc) return rc;
  return group_run<BINF>(c, route);
}

SPX_EXPORT int spx_prox_group_l2(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                 int64_t n, const int64_t* group_offsets, int64_t group_size, int64_t ngroups,
                                 const double* lambda_vec, double sigma) {
  return run_group<false>({ctx, y, q, xk, sj, n, group_offsets, group_size, ngroups, lambda_vec, sigma, 0.0});
}

SPX_EXPORT int spx_prox_group_l2_binf(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                      int64_t n, const int64_t* group_offsets, int64_t group_size, int64_t ngroups,
                                      const double* lambda_vec, double sigma, double delta) {
  return run_group<true>({ctx, y, q, xk, sj, n, group_offsets, group_size, ngroups, lambda_vec, sigma, delta});
}

// ---------------------------------------------------------------------------------------------
// prox! fused with h at the result (include/spx.h, "group forms").  The register-tile route: the value comes out of the
// launches that store y.  Every other route (LDS-resident groups, the general kernels, teams of workgroups): composed in
// this call -- y = q_scale * q where the scale is not 1, the unchanged prox at q := y, then the one-launch psi(y)
// (spx_obj_group_l2_to) on the same stream.
// ---------------------------------------------------------------------------------------------
template <bool BINF>
static int run_group_val_to(const GroupCall& c, double q_scale, const SpxDest& dest) {
  GroupRoute route;
  int rc = group_classify<BINF>(c, &route);
  if (rc) return rc;
  spx_ctx* ctx = c.ctx;
  rc = spx_dest_check_capture(ctx, dest, "returning the value to the host");  // (refused before anything is enqueued)
  if (rc) return rc;
  spx_dest_zero_host(dest);
  if (route == GroupRoute::Reg) return group_route_reg<BINF, true>(c, q_scale, dest);
  if (route == GroupRoute::None) {  // h of no group at all; y as the plain operator leaves it (it does not read q)
    rc = group_run<BINF>(c, route);
    if (rc) return rc;
    return spx_dest_empty(ctx, dest);
  }
  GroupCall scaled = c;
  if (q_scale != 1.0) {
    SPX_ON_DEVICE(ctx);
    int64_t eb = (c.n + 255) / 256;
    if (eb > (int64_t)ctx->num_cu * 8) eb = (int64_t)ctx->num_cu * 8;
    hipLaunchKernelGGL(k_group_scale, dim3((unsigned)eb), dim3(256), 0, ctx->stream, c.y, c.q, q_scale, c.n, c.offsets, c.ngroups);
    SPX_LAUNCH_CHECK();
    scaled.q = c.y;
  }
  rc = group_run<BINF>(scaled, route);
  if (rc) return rc;
  // (the h part for the Binf operator too: not spx_obj_group_l2_binf)
  return spx_obj_group_l2_to(ctx, c.y, c.xk, c.sj, c.n, c.offsets, c.gsize, c.ngroups, c.lambda, dest);
}
// the entry points' form: the destination from (ctx, value)
template <bool BINF>
static int run_group_val(const GroupCall& c, double q_scale, double* value) {
  SPX_REQUIRE(value != nullptr, "value is NULL");
  const SpxDest dest = spx_value_dest(c.ctx, value);
  *value = 0.0;
  const int rc = run_group_val_to<BINF>(c, q_scale, dest);
  spx_value_nan_on_device(rc, dest, c.n == 0 || c.ngroups == 0, value);  // (no group at all: the empty call)
  return rc;
}

SPX_EXPORT int spx_proxval_group_l2(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                    const int64_t* group_offsets, int64_t group_size, int64_t ngroups,
                                    const double* lambda_vec, double sigma, double q_scale, double* value) {
  return run_group_val<false>({ctx, y, q, xk, sj, n, group_offsets, group_size, ngroups, lambda_vec, sigma, 0.0}, q_scale, value);
}

SPX_EXPORT int spx_proxval_group_l2_binf(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                         int64_t n, const int64_t* group_offsets, int64_t group_size, int64_t ngroups,
                                         const double* lambda_vec, double sigma, double delta, double q_scale,
                                         double* value) {
  return run_group_val<true>({ctx, y, q, xk, sj, n, group_offsets, group_size, ngroups, lambda_vec, sigma, delta}, q_scale, value);
}

// ---------------------------------------------------------------------------------------------
// prox! fused with the step statistics (include/spx.h, "group forms" of spx_proxstep_*).  Uniform groups on the register tiles:
// everything comes out of the launches that store y (k_group_reg, STEP).  Every other layout is composed in this call: the
// unchanged run_group_val with SpxSyncHeader::grp_step_h as its device destination -- y and h -- then ONE streaming launch for xkn and
// the two sums, which also hands h on to the result slots.
// ---------------------------------------------------------------------------------------------
// xkn = (xk + sj) + y, <q, y>, <y, y> over [0, n): a grid-stride loop, VEC: 16-byte accesses (every vector 16-byte aligned; the
// odd last element is taken by one lane).  The finish is gval_finish's on three planes; plane 0 carries nothing but *h, added
// by workgroup 0 to zeros, so that the last workgroup stores the triple {h, <q, y>, <y, y>}.
template <bool VEC>
__global__ __launch_bounds__(256) void k_group_step_tail(const double* q, const double* y, const double* xk, const double* sj,
                                                          double* xkn, int64_t n, const double* h, GroupStep gv) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  double qy = 0.0, yy = 0.0;
  if constexpr (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = t; i < n2; i += stride) {
      const f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(q) + i);
      const f64x2 b = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(y) + i);
      if (xkn != nullptr) {
        const f64x2 x = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(xk) + i);
        const f64x2 s = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sj) + i);
        __builtin_nontemporal_store(f64x2{(x.x + s.x) + b.x, (x.y + s.y) + b.y}, reinterpret_cast<f64x2*>(xkn) + i);
      }
      qy += a.x * b.x;
      qy += a.y * b.y;
      yy += b.x * b.x;
      yy += b.y * b.y;
    }
    if ((n & 1) && t == 0) {
      const int64_t i = n - 1;
      if (xkn != nullptr) xkn[i] = (xk[i] + sj[i]) + y[i];
      qy += q[i] * y[i];
      yy += y[i] * y[i];
    }
  } else {
    for (int64_t i = t; i < n; i += stride) {
      const double b = y[i];
      if (xkn != nullptr) xkn[i] = (xk[i] + sj[i]) + b;
      qy += q[i] * b;
      yy += b * b;
    }
  }
  double acc[3] = {t == 0 ? *h : 0.0, qy, yy};
  gval_finish(acc, false, gv);
}

// [GroupStepWs | three planes of partials] of the tail launch (spx_common.hpp: shared with spx_proxstep_l1_b2)
SpxStepTail spx_step_tail_plan(spx_ctx* ctx, const double* y, const double* q, const double* xk, const double* sj, const double* xkn,
                               int64_t n) {
  SpxStepTail tail;
  tail.vec = spx_aligned16(y) && spx_aligned16(q) && spx_aligned16(xk) && spx_aligned16(sj) && spx_aligned16(xkn);
  const int64_t work = tail.vec ? (n + 1) / 2 : n;
  tail.blocks = (work + 255) / 256;
  if (tail.blocks > (int64_t)ctx->num_cu * 8) tail.blocks = (int64_t)ctx->num_cu * 8;
  tail.bytes = sizeof(GroupStepWs) + (size_t)tail.blocks * 3 * sizeof(double) + 256;
  return tail;
}

int spx_step_tail_run(spx_ctx* ctx, const SpxStepTail& tail, const double* q, const double* y, const double* xk, const double* sj,
                      double* xkn, int64_t n, const double* h, const SpxDest& dest) {
  SPX_ON_DEVICE(ctx);
  GroupStep gv{};
  GroupStepWs* sws = reinterpret_cast<GroupStepWs*>(ctx->ws);
  static_cast<GroupVal&>(gv) = GroupVal{1.0, reinterpret_cast<double*>(sws + 1), nullptr, (int)tail.blocks, false, spx_sync_header(ctx), nullptr, nullptr, nullptr, nullptr, 64};
  gv.xkn = xkn;
  gv.stats_dev = dest.dev;
  gv.sws = sws;
  if (tail.vec) hipLaunchKernelGGL(k_group_step_tail<true>, dim3((unsigned)tail.blocks), dim3(256), 0, ctx->stream, q, y, xk, sj, xkn, n, h, gv);
  else hipLaunchKernelGGL(k_group_step_tail<false>, dim3((unsigned)tail.blocks), dim3(256), 0, ctx->stream, q, y, xk, sj, xkn, n, h, gv);
  SPX_LAUNCH_CHECK();
  return spx_dest_return(ctx, dest, sws->result, 3 * sizeof(double));
}

template <bool BINF>
static int run_group_step(const GroupCall& c, double q_scale, double* xkn, double* stats, double* stats_dev) {
  GroupRoute route;
  int rc = group_classify<BINF>(c, &route);
  if (rc) return rc;
  spx_ctx* ctx = c.ctx;
  const SpxDest dest{stats, stats_dev, 3};
  rc = spx_step_begin(ctx, dest, false, c.y, {c.q}, kSpxYAliasesQ, xkn, {c.y, c.q, c.xk, c.sj});
  if (rc) return rc;
  if (route == GroupRoute::None) {  // no group at all: three zeros; y as the plain operator leaves it (it does not read q)
    rc = group_run<BINF>(c, route);
    if (rc) return rc;
    return spx_dest_empty(ctx, dest);
  }
  if (route == GroupRoute::Reg && c.offsets == nullptr) return group_route_reg<BINF, true, true>(c, q_scale, dest, xkn);
  // composed: the workspace of the tail launch is reserved before anything is enqueued
  const SpxStepTail tail = spx_step_tail_plan(ctx, c.y, c.q, c.xk, c.sj, xkn, c.n);
  rc = spx_ws_reserve(ctx, tail.bytes);
  if (rc) return rc;
  rc = spx_sync_ready(ctx);
  if (rc) return rc;
  SpxSyncHeader* hdr = spx_sync_header(ctx);
  rc = run_group_val_to<BINF>(c, q_scale, SpxDest{nullptr, &hdr->grp_step_h, 1});
  if (rc) return rc;
  return spx_step_tail_run(ctx, tail, c.q, c.y, c.xk, c.sj, xkn, c.n, &hdr->grp_step_h, dest);
}

SPX_EXPORT int spx_proxstep_group_l2(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                     const int64_t* group_offsets, int64_t group_size, int64_t ngroups,
                                     const double* lambda_vec, double sigma, double q_scale, double* xkn, double* stats,
                                     double* stats_dev) {
  return run_group_step<false>({ctx, y, q, xk, sj, n, group_offsets, group_size, ngroups, lambda_vec, sigma, 0.0}, q_scale, xkn, stats,
                               stats_dev);
}

SPX_EXPORT int spx_proxstep_group_l2_binf(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                          int64_t n, const int64_t* group_offsets, int64_t group_size, int64_t ngroups,
                                          const double* lambda_vec, double sigma, double delta, double q_scale, double* xkn,
                                          double* stats, double* stats_dev) {
  return run_group_step<true>({ctx, y, q, xk, sj, n, group_offsets, group_size, ngroups, lambda_vec, sigma, delta}, q_scale, xkn, stats,
                              stats_dev);
}

// ---------------------------------------------------------------------------------------------
// gather-index groups: idx_g = group_index[group_ptr[g] .. group_ptr[g+1])
// ---------------------------------------------------------------------------------------------
template <bool BINF>
static int run_group_gather(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                            const int64_t* ptr, const int64_t* index, int64_t ngroups, int64_t nnz,
                            const double* lambda, double sigma, double delta) {
  int rc = spx_check_common(ctx, y, q, xk, sj, n);
  if (rc) return rc;
  SPX_REQUIRE(ngroups >= 0 && ngroups < 0x7fffffff, "ngroups out of range");
  SPX_REQUIRE(nnz >= 0, "nnz < 0");
  if (n == 0) return SPX_OK;
  if (ngroups > 0) SPX_REQUIRE(ptr != nullptr && lambda != nullptr, "group_ptr or lambda_vec is NULL");
  if (nnz > 0) SPX_REQUIRE(index != nullptr, "group_index is NULL");
  if (ngroups > 0) {  // (the index-set validation below reads a flag back: refused before anything is enqueued)
    const int rcc = spx_require_not_capturing(ctx, "validating a group layout");
    if (rcc) return rcc;
  }
  SPX_ON_DEVICE(ctx);
  // workspace: flag (256 B) | sol (n doubles) | owner (n ints)
  const size_t sol_off = 256, own_off = sol_off + (size_t)n * sizeof(double);
  rc = spx_ws_reserve(ctx, own_off + (size_t)n * sizeof(int) + 256);
  if (rc) return rc;
  char* ws = static_cast<char*>(ctx->ws);
  int* flag = reinterpret_cast<int*>(ws);
  double* sol = reinterpret_cast<double*>(ws + sol_off);
  int* owner = reinterpret_cast<int*>(ws + own_off);
  const int64_t cap_blocks = (int64_t)ctx->num_cu * 8;
  int64_t eb = (n + 255) / 256;
  if (eb > cap_blocks) eb = cap_blocks;
  SPX_HIP(hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_gather_prepare, dim3((unsigned)eb), dim3(256), 0, ctx->stream, sol, owner, q, xk, sj, n);
  if (ngroups > 0) {
    int64_t gb = (ngroups + 3) / 4;
    if (gb > cap_blocks) gb = cap_blocks;
    hipLaunchKernelGGL(k_gather_owner, dim3((unsigned)gb), dim3(256), 0, ctx->stream, owner, ptr, index, ngroups, n, nnz,
                       flag);
    SPX_LAUNCH_CHECK();
    int hflag = 0;  // the reference throws BoundsError before touching y: check before the stores
    SPX_HIP(hipMemcpyAsync(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SPX_HIP(hipStreamSynchronize(ctx->stream));
    if (hflag & 2) { spx_set_error("invalid argument: group_ptr is not a non-decreasing sequence inside [0, nnz]"); return SPX_ERR_INVALID_ARG; }
    if (hflag & 1) { spx_set_error("invalid argument: group index outside [0, n) (BoundsError)"); return SPX_ERR_INVALID_ARG; }
    const int team = spx_group_lanes_by_avg((double)nnz / (double)ngroups);
    const int tpb = 256 / team;
    int64_t tb = (ngroups + tpb - 1) / tpb;
    if (tb > cap_blocks) tb = cap_blocks;
    spx_with_lanes<4, 8, 16, 32, 64, 256>(team, [&](auto lanes) {
      hipLaunchKernelGGL((k_group_gather<decltype(lanes)::value, BINF>), dim3((unsigned)tb), dim3(256), 0, ctx->stream, y, sol, xk, sj,
                         owner, ptr, index, ngroups, lambda, sigma, delta, ctx->tune_binf_literal);
    });
  }
  // :77 subtracts the shift at EVERY index; the Binf form does so per group (:116) and leaves the rest of y alone
  if (!BINF) hipLaunchKernelGGL(k_gather_rest, dim3((unsigned)eb), dim3(256), 0, ctx->stream, y, xk, sj, owner, n);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}

SPX_EXPORT int spx_prox_group_l2_gather(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj,
                                        int64_t n, const int64_t* group_ptr, const int64_t* group_index,
                                        int64_t ngroups, int64_t nnz, const double* lambda_vec, double sigma) {
  return run_group_gather<false>(ctx, y, q, xk, sj, n, group_ptr, group_index, ngroups, nnz, lambda_vec, sigma, 0.0);
}

SPX_EXPORT int spx_prox_group_l2_binf_gather(spx_ctx* ctx, double* y, const double* q, const double* xk,
                                             const double* sj, int64_t n, const int64_t* group_ptr,
                                             const int64_t* group_index, int64_t ngroups, int64_t nnz,
                                             const double* lambda_vec, double sigma, double delta) {
  return run_group_gather<true>(ctx, y, q, xk, sj, n, group_ptr, group_index, ngroups, nnz, lambda_vec, sigma, delta);
}
