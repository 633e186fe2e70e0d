// spx_plan.hpp -- WHICH kernel runs, on WHICH grid, with WHICH workspace: the decisions of the calls whose kernels synchronise
// inside one launch (top-r: spx_select.hip; ShiftedNormL1B2: spx_b2.hip; large groups on teams: spx_group_team.hip) and of the
// batched separable calls (spx_batch.hip, spx_ibatch.hip), the batched group calls (spx_gbatch.hip, spx_gbinf_batch.hip) and the
// batched ShiftedNormL1B2 call (spx_b2_batch.hip) and the batched top-r calls (spx_topr_batch.hip), as plain functions of plain values.  No HIP include, no runtime call, no kernel, no spx_ctx: what a call would do at a given n,
// alignment, residency and tuning is computable -- and testable, tests/c/plan_driver.hip -- on a CPU.
//
// Residency comes in through `cap`: cap(kernel) returns what spx_resident_cap returns for that kernel (0 = it cannot run; the
// library's `cap` has then set the error text).  The plan functions ask LAZILY, in a fixed order: every question takes one of
// the context's 32 occupancy slots the first time it is asked.
// The constants the decisions share with the kernels are stated here once.  Nothing of a kernel's signature lives here; where
// a layout needs the size of a device-side struct, the caller passes sizeof.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---------------------------------------------------------------------------------------------
// top-r (spx_select.hip)
// ---------------------------------------------------------------------------------------------
constexpr int64_t kSmallNCoop = 1 << 13;  // k_sel_small serves up to here, k_sel_coop the sizes above
constexpr int kCoopEpl = 8;       // k_sel_coop<REG>: elements per lane at most (16 spill: 1024-lane workgroups leave 128 VGPRs per lane)
constexpr int kLdsEpl = 16;       // k_sel_lds, Float64: elements per lane (128 KiB of LDS per 1024-lane workgroup)
constexpr int kLdsEpl32 = 32;     // k_sel_lds, Float32
constexpr int kLdsRegX = 8;       // k_sel_lds<.., kLdsRegX>: that many more elements per lane in registers
constexpr int64_t kLdsMinN = (int64_t)1 << 20;  // k_sel_lds serves the sizes above this (and below what the resident grid holds)
constexpr int kFrontBlocks = 64;  // grid of k_s2_front (its sample layout is tied to it)
#ifndef SPX_SEL_REG_MAX_LOG2
#define SPX_SEL_REG_MAX_LOG2 21  // largest n (log2) on the register-resident one-launch select = what 256 CUs hold at 8 elements per lane (n = 2e6: 37 us vs 57 us for the sample-predicted pipeline; beyond it the one-launch form parks v in y and is no faster: tools/r2/topr_midn.py)
#endif
constexpr int kWaveSlots = 64;        // candidate entries per wavefront of the main pass
constexpr int kMainUnroll = 6;        // KiB per wave and vector in the main pass (as k_sep_lds)
constexpr int kMainTilePairs = 256 * kMainUnroll;  // 16-byte pairs per workgroup of the main pass
constexpr int kShortList = 4096;      // candidates left after the first digit that k_s2_finish resolves in LDS

// the kernels whose residency the decision asks for
enum class SelKernel { kCoopReg, kCoopMem, kLdsVec, kLdsScalar, kLdsRegX, kFront1, kFront2, kFront4, kFront16, kTail };
// The exact select in ONE launch: k_sel_coop (v in registers: kCoopReg; v parked in y: kCoopMem) or k_sel_lds (v parked in
// LDS; kLdsRegX: and 8 more elements per lane in registers, Float64 and 16-byte aligned vectors only)
enum class SelForm { kCoopReg, kCoopMem, kLds, kLdsRegX };
// one workgroup (k_sel_small) / one launch of a resident grid (SelForm) / the sample-predicted pipeline / nothing can run
enum class SelRoute { kSmall, kExact, kFast, kError };

struct SelIn {
  bool f64;        // Float64 (the sample-predicted pipeline and the hybrid LDS + register form are Float64 only)
  int64_t n, r;
  bool vec;        // y, q, xk, sj all 16-byte aligned
  bool all_off8;   // all four 8 bytes off a 16-byte boundary (a view that starts at an odd element)
  int num_cu;
  int sel_fast, sel_small, front_spl, sel_reg16;  // tuning keys 2, 6, 10, 11
  int force_grid;  // key 100 (test builds; 0 elsewhere): the grid of the form that parks v in y, residency or not
};
struct SelPlan {
  SelRoute route;
  SelForm form;    // kExact
  bool vec;
  int64_t g;       // kExact: the grid
  int ioff;        // Float64: 1 = the pipeline runs on the aligned rest and its wave 0 takes element 0 along
  int spl;         // Float64: samples per lane of the front kernel (1, 2, 4, 16)
  int64_t g_tail;  // kFast: the grid of k_s2_tail
};

inline SelKernel sel_front_kernel(int spl) {
  return spl == 16 ? SelKernel::kFront16 : spl == 4 ? SelKernel::kFront4 : spl == 2 ? SelKernel::kFront2 : SelKernel::kFront1;
}

template <class Cap>
SelPlan sel_plan(const SelIn& in, Cap&& cap) {
  const int64_t n = in.n, r = in.r, num_cu = in.num_cu;
  const bool vec = in.vec;
  SelPlan p{SelRoute::kExact, SelForm::kCoopMem, vec, 0, 0, 1, 0};
  const auto on_cus = [num_cu](int64_t c) { return c < num_cu ? c : num_cu; };
  // one workgroup, one launch, no scratch -- up to 8192 elements (n = 16 384: 32 us in one workgroup, 21 us on two;
  // n = 65 536: 84 vs 19 us -- tools/r2/topr_small.py)
  if (n <= kSmallNCoop && in.sel_small) { p.route = SelRoute::kSmall; return p; }
  // Residency of the kernels that synchronise inside one launch: a grid never exceeds what the occupancy query says can be
  // resident at once; a form whose grid does not fit hands over to the one that works with any grid.
  const int64_t cap_reg = cap(SelKernel::kCoopReg);
  const int64_t cap_mem = cap(SelKernel::kCoopMem);
  if (cap_mem < 1) { p.route = SelRoute::kError; return p; }
  const int64_t reg_cap = (int64_t)kCoopEpl * 1024 * on_cus(cap_reg);  // (2 Mi elements on 256 CUs)
  // ... and with v parked in LDS (k_sel_lds: 16 Ki Float64 / 32 Ki Float32 elements per resident workgroup, 4 Mi / 8 Mi on 256
  // CUs).  y must not overlap the inputs elsewhere than element for element (a lane reads all its inputs before it writes:
  // aliasing q, xk or sj exactly is fine, as in the other one-launch forms).
  const int lds_slots = in.f64 ? kLdsEpl : kLdsEpl32;
  int64_t lds_cap = 0;
  if (in.sel_reg16) lds_cap = (int64_t)lds_slots * 1024 * on_cus(cap(vec ? SelKernel::kLdsVec : SelKernel::kLdsScalar));
  const int64_t g_mem = on_cus(cap_mem);  // grid of the form that parks v in y: any size >= 1 works
  // (k_sel_lds: every CU the grid may have -- the load phase is most of the kernel and wants all of them pulling; a rendezvous
  //  costs 1.4 us with 256 workgroups since the arrivals are spread over eight counters)
  const int64_t g_lds = lds_cap / ((int64_t)lds_slots * 1024);
  if (!in.f64) {
    // Float32: k_sel_lds above what the register form holds (2 Mi; below, registers win: n = 2e6 39 / 41 us against 43 / 45 --
    // the Float32 first digit is not folded and the LDS form's third pass costs more), 8 elements per lane in registers;
    // beyond what the grid holds: the form that parks v in y (n = 8e6: 97 -> 64 us, tools/r3/topr_f32_midn.py).  The
    // sample-predicted single pass is Float64 only (~44 B/element here instead of 16, 0.7 ms at n = 1e8).
    const bool lds = n <= lds_cap && n > reg_cap;
    const bool reg = !lds && n <= reg_cap;
    p.form = lds ? SelForm::kLds : reg ? SelForm::kCoopReg : SelForm::kCoopMem;
    p.g = lds ? g_lds : reg ? (n + (int64_t)kCoopEpl * 1024 - 1) / ((int64_t)kCoopEpl * 1024) : g_mem;
    return p;
  }
  // Float64: the sample-predicted pipeline above what the one-launch forms hold, k_sel_lds from 1 Mi elements on, the
  // hybrid LDS + register form up to 6 Mi, elements per lane graded by n on the register form.
  p.ioff = (!vec && in.all_off8) ? 1 : 0;
  // samples per lane of the front kernel: 1 / 2 / 4 by n (see k_s2_front); 16 for a cut in the bulk of a large vector -- the band
  // is +-6 sigma of the SAMPLE rank, sigma^2 = M p (1 - p): its share of the vector shrinks with sqrt(M), and at r = n/2 the band
  // of the 4-sample form holds 1.2 % of the vector as candidates (main pass +40 us, compaction +20 us; tuning key 10 overrides)
  const double pcut = (double)r / (double)n;
  p.spl = n >= ((int64_t)1 << 25) ? 4 : (n >= ((int64_t)1 << 23) ? 2 : 1);
  if (n >= ((int64_t)1 << 26) && pcut * (1.0 - pcut) > 0.04) p.spl = 16;
  if (in.front_spl == 1 || in.front_spl == 2 || in.front_spl == 4 || in.front_spl == 16) p.spl = in.front_spl;
  const int64_t cap_front = cap(sel_front_kernel(p.spl));
  // ... and 6 Mi with 8 more elements per lane in registers (k_sel_lds<.., REGX>: 16-byte aligned vectors only; tuning key 11 = 2
  // keeps the pipeline from 4 Mi on).  The sample-predicted pipeline (six launches, ~50 us of them fixed cost) takes over above
  // what the resident grid holds on chip.
  int64_t hyb_cap = 0;
  if (in.sel_reg16 == 1 && vec && lds_cap > 0) {
    hyb_cap = (int64_t)(kLdsEpl + kLdsRegX) * 1024 * on_cus(cap(SelKernel::kLdsRegX));
    if (hyb_cap > 0x7fffffff) hyb_cap = 0;  // (the form indexes with 32-bit integers)
  }
  int64_t fast_min = ((int64_t)1 << SPX_SEL_REG_MAX_LOG2) + 1;
  if (lds_cap >= fast_min) fast_min = lds_cap + 1;
  if (hyb_cap >= fast_min) fast_min = hyb_cap + 1;
  const bool try_fast = in.sel_fast && (vec || p.ioff) && (n - p.ioff) >= fast_min && r > 0 && r < n &&
                        cap_front >= kFrontBlocks;  // (the front kernel's sample layout is tied to its grid)
  if (try_fast) {
    const int64_t cap_tail = cap(SelKernel::kTail);
    if (cap_tail < 1) { p.route = SelRoute::kError; return p; }
    p.route = SelRoute::kFast;
    p.g_tail = cap_tail < 256 ? on_cus(cap_tail) : (num_cu < 256 ? num_cu : 256);  // (<= 256: SelSync::tie_part)
    return p;
  }
  // exact select in ONE launch: register-resident up to 8 Ki elements per resident workgroup, v parked in y beyond that
  // k_sel_lds from 1 Mi elements on (n = 2e6: 34 / 42 us at r = n/100 / n/2 against 39 / 45 with v in registers; n = 1e6:
  // 36 / 30 against 35 / 29 -- tools/r3/topr_small_grid.py), and wherever the register form's grid does not fit
  const bool lds = n <= lds_cap && (n > kLdsMinN || n > reg_cap);
  const bool hyb = !lds && n > lds_cap && n <= hyb_cap;  // (vec: hyb_cap is 0 otherwise)
  const bool reg = !lds && !hyb && n <= reg_cap;
  // Register form: 1 / 2 / 4 / 8 elements per lane by n -- the fewer elements a lane walks per pass the better, until the
  // workgroups are so many that their histogram flushes and arrivals cost more (us per call at r = n/100, 1 / 2 / 4 / 8 per
  // lane: n = 3e4 17.4 / 18.4 / 20.7 / 24.1; n = 1e5 19.8 / 19.3 / 20.8 / 24.4; n = 3e5 26.8 / 22.8 / 22.1 / 24.9; n = 1e6
  // 35.6 / 35.7 / 36.6 / 34.7 -- tools/r3/topr_small_grid.py)
  const int64_t epl = n <= 65536 ? 1 : n <= 196608 ? 2 : n <= 655360 ? 4 : kCoopEpl;
  p.form = lds ? SelForm::kLds : hyb ? SelForm::kLdsRegX : reg ? SelForm::kCoopReg : SelForm::kCoopMem;
  p.g = g_mem;
  if (reg) {
    const int64_t gmax = on_cus(cap_reg);
    p.g = (n + epl * 1024 - 1) / (epl * 1024);
    if (p.g > gmax) p.g = gmax;  // (n <= reg_cap: 8 elements per lane always fit)
  }
  if (lds) p.g = g_lds;
  if (hyb) p.g = hyb_cap / ((int64_t)(kLdsEpl + kLdsRegX) * 1024);
  // the planted fault of tests/test_gpu_robustness.py: a grid that cannot be resident
  if (!reg && !lds && !hyb && in.force_grid > 0) p.g = in.force_grid;
  return p;
}

// Workspace of the sample-predicted pipeline: one candidate region + count word per wavefront of the main pass, the class
// counts of tie mode, the shared overflow list behind the regions, and the short list k_s2_finish resolves.
struct SelFastWs {
  int64_t n2;         // 16-byte pairs of the aligned rest
  int64_t mblocks;    // grid of the main pass
  int64_t nregions, ccap;
  unsigned int ovf_cap;
  size_t off_cnt, off_cls, off_ckey, off_lkey, off_lidx, off_lval, bytes;
};
inline SelFastWs sel_fast_ws(int64_t n, int ioff, size_t wave_count_bytes, size_t class_count_bytes, size_t cand_bytes) {
  SelFastWs w;
  w.n2 = (n - ioff) >> 1;
  w.mblocks = (w.n2 + kMainTilePairs - 1) / kMainTilePairs;
  w.nregions = w.mblocks * 4;
  w.ccap = w.nregions * kWaveSlots;
  // the shared overflow list behind the per-wave regions: room for a band that is contiguous in the vector (sorted input)
  const int64_t ovf_cap64 = (n / 64 > 65536) ? n / 64 : 65536;
  w.ovf_cap = (unsigned int)(ovf_cap64 > 0x7fffffff ? 0x7fffffff : ovf_cap64);
  w.off_cnt = 256;
  w.off_cls = (w.off_cnt + (size_t)w.nregions * wave_count_bytes + 255) & ~(size_t)255;   // tie mode: class members per slot
  w.off_ckey = (w.off_cls + (size_t)(w.nregions + 2) * class_count_bytes + 255) & ~(size_t)255;
  w.off_lkey = w.off_ckey + ((size_t)w.ccap + (size_t)w.ovf_cap) * cand_bytes;
  w.off_lidx = w.off_lkey + (size_t)kShortList * sizeof(uint64_t);
  w.off_lval = w.off_lidx + (size_t)kShortList * sizeof(int64_t);
  w.bytes = w.off_lval + (size_t)kShortList * sizeof(double) + 256;
  return w;
}

// ---------------------------------------------------------------------------------------------
// ShiftedNormL1B2 (spx_b2.hip)
// ---------------------------------------------------------------------------------------------
// register-resident form: 512 lanes x 16 elements per workgroup (256 VGPRs per lane).  1024 lanes x 8 spill under their 128
// VGPRs (loop invariants the compiler keeps per element: the box ends, the store addresses), and the first touch of a wave's
// scratch memory costs microseconds at the start of every launch; 1024 x 16 spill 120 registers and run 2x slower.
constexpr int kB2Epl = 16;
constexpr int kB2RegThreads = 512;
constexpr int kB2RegBlock = kB2Epl * kB2RegThreads;  // elements per workgroup of the register-resident form
constexpr int kB2Cols = 256;   // workgroups at most

// The four forms of k_b2_coop, which are also the kernels whose residency the decision asks for (of the PLAIN kernels, for
// prox, proxval and proxstep alike: y's bits depend on the grid).
enum B2Form { kB2FormReg = 0, kB2FormLds = 1, kB2FormVec = 2, kB2Form8 = 3 };

struct B2In {
  int64_t n;
  bool vec;    // n >= 2 and y, q, xk, sj all 16-byte aligned
  int b2_lds;  // tuning key 12
};
struct B2Plan {
  bool ok;          // false: the streaming form cannot be resident (nothing can run)
  B2Form form;
  int64_t g;        // the grid
  int64_t epl;      // kB2FormReg: elements per lane the grid was sized for (4 / 8 / 16); 0 on the other forms
  int64_t gmax_reg, gmax_mem, gmax_lds;  // resident workgroups (<= kB2Cols) of the forms that were asked; gmax_lds 0 if it was not
  unsigned int cand_cap;  // streaming form: entries per candidate region (one region per wavefront of the grid)
  size_t ws_bytes;        // streaming form: the workspace; 0 on the others
};

template <class Cap>
B2Plan b2_plan(const B2In& in, size_t cand_elem_bytes, Cap&& cap) {
  const int64_t n = in.n;
  B2Plan p{};
  // Residency: the grid of a launch that synchronises inside itself never exceeds what can be resident at once; the
  // streaming form works with any grid >= 1, the register-resident one needs ceil(n / 8192) workgroups.
  const int64_t cap_reg = cap(kB2FormReg);
  const int64_t cap_mem = cap(in.vec ? kB2FormVec : kB2Form8);
  if (cap_mem < 1) return p;
  p.ok = true;
  p.gmax_reg = cap_reg < kB2Cols ? cap_reg : kB2Cols;
  p.gmax_mem = cap_mem < kB2Cols ? cap_mem : kB2Cols;
  const bool reg = n <= (int64_t)kB2RegBlock * p.gmax_reg;
  // xk parked in LDS, 16 Ki elements per workgroup: between what the register form holds and 4 Mi (256 CUs); tuning key 12 = 0
  // sends those sizes to the streaming form as in round 2 (n = 4e6: 111 us per call against 61)
  bool ldsx = false;
  if (!reg && in.b2_lds) {
    const int64_t cap_lds = cap(kB2FormLds);
    p.gmax_lds = cap_lds < kB2Cols ? cap_lds : kB2Cols;
    ldsx = n <= (int64_t)kB2Epl * 1024 * p.gmax_lds;
  }
  p.g = reg ? (n + kB2RegBlock - 1) / kB2RegBlock : p.gmax_mem;
  if (ldsx) p.g = p.gmax_lds;  // (n > 2 Mi here unless the grid is capped: every resident workgroup, <= 16 elements per lane)
  if (reg) {
    // the register form: 4 / 8 / 16 elements per lane by n -- more workgroups sweep fewer elements each, until their exchange
    // costs more than the sweep saves (us per call, Delta = 1, 16 / 8 / 4 / 2 per lane: n = 1e4 22.2 / 21.3 / 20.5 / 20.5;
    // n = 1e5 25.4 / 23.3 / 22.5 / 23.4; n = 3e5 26.6 / 24.8 / 25.4 / 28.3; n = 1e6 30.4 / 31.9 / 31.1 / 31.4 -- tools/r3/b2_midn.py)
    p.epl = n <= 131072 ? 4 : n <= 524288 ? 8 : kB2Epl;
    int64_t gg = (n + p.epl * kB2RegThreads - 1) / (p.epl * kB2RegThreads);
    if (gg > p.gmax_reg) gg = p.gmax_reg;
    if (gg > p.g) p.g = gg;
  }
  if (p.g < 1) p.g = 1;
  p.form = ldsx ? kB2FormLds : reg ? kB2FormReg : in.vec ? kB2FormVec : kB2Form8;
  // streaming form: candidate regions, one per wavefront of the grid -- room for 8 % of its share of the vector (the bracket
  // of +-1.5 % around the sample's root holds the breakpoints of 1-2 % on ordinary data; a full region = plain iteration)
  if (!reg && !ldsx) {
    const int64_t waves = p.g * 16;
    const int64_t share = (n + waves - 1) / waves;
    int64_t c = share / 12 + 64;
    if (c > 0x7fffffff) c = 0x7fffffff;
    p.cand_cap = (unsigned int)c;
    p.ws_bytes = (size_t)waves * (size_t)c * cand_elem_bytes + 256;
  }
  return p;
}

// ---------------------------------------------------------------------------------------------
// large contiguous groups on teams of workgroups (spx_group_team.hip)
// ---------------------------------------------------------------------------------------------
constexpr int kGtCols = 256;       // workgroups of a team launch at most (the exchange words: spx_group_common.hpp)
constexpr int kTmThreads = 1024;
constexpr int kTmMaxJobs = 65536;  // large groups a device-side plan holds at most

struct TeamLayout {
  bool vec;
  int par, G, Wu;
  int64_t grid;
  size_t plan_bytes, status_bytes, cand_bytes;
  unsigned int cand_cap;
};
// bit 3 of q's address, and whether xk, sj and y share it: which of the two kernels of a form runs (and is asked for residency)
inline void team_alignment(uintptr_t y, uintptr_t q, uintptr_t xk, uintptr_t sj, TeamLayout* L) {
  const auto bit3 = [](uintptr_t p) { return (int)((p >> 3) & 1u); };
  L->par = bit3(q);
  L->vec = bit3(xk) == L->par && bit3(sj) == L->par && bit3(y) == L->par;
}
// L->par and L->vec are set (team_alignment); cap: resident workgroups of the form's kernel; team_fast: tuning key 14;
// has_offsets: CSR groups (a device-side plan) -- gsize is not looked at; plan_hdr_bytes, job_bytes, cand_elem_bytes: sizeof
// TeamPlanHdr, TeamJob and a candidate.  Non-zero when nothing can be resident.
inline int team_layout(int64_t cap, int team_fast, bool binf, int64_t n, bool has_offsets, int64_t gsize, int64_t ngroups,
                       size_t plan_hdr_bytes, size_t job_bytes, size_t cand_elem_bytes, TeamLayout* L) {
  if (cap > kGtCols) cap = kGtCols;
  if (cap < 1) return 1;
  L->G = (int)cap;
  L->Wu = 1;
  L->grid = L->G;
  int64_t per_wg = 2 * ((n + L->G - 1) / L->G);  // elements of one job per workgroup (a device-side plan: at most about that)
  if (!has_offsets) {
    if (ngroups < L->G) {
      int64_t w = L->G / ngroups;
      const int64_t wmax = (gsize + 2047) / 2048;  // no fewer than ~2048 elements per workgroup
      if (w > wmax) w = wmax;
      if (w < 1) w = 1;
      L->Wu = (int)w;
      L->grid = ngroups * w;
    }
    per_wg = (gsize + L->Wu - 1) / L->Wu;
  }
  L->plan_bytes = has_offsets ? ((plan_hdr_bytes + (size_t)kTmMaxJobs * job_bytes + 255) & ~(size_t)255) : 0;
  {  // one word per job: at most kTmMaxJobs jobs in a device-side plan, ngroups jobs for uniform groups
    size_t jobs_max = (size_t)kTmMaxJobs;
    if (!has_offsets && (size_t)ngroups > jobs_max) jobs_max = (size_t)ngroups;
    L->status_bytes = (jobs_max * sizeof(int) + 255) & ~(size_t)255;
  }
  L->cand_cap = 0;
  L->cand_bytes = 0;
  if (binf && team_fast) {
    // one candidate region per wavefront of the grid: a quarter of the wavefront's share of a job (the breakpoints inside a
    // bracket of +-hw around the sample's root are a few times hw of the elements on ordinary data; a full region = the
    // generic body decides)
    int64_t c = per_wg / (kTmThreads / 64) / 4 + 64;
    if (c > 0x7fffffff) c = 0x7fffffff;
    L->cand_cap = (unsigned int)c;
    L->cand_bytes = (size_t)L->grid * (kTmThreads / 64) * (size_t)c * cand_elem_bytes;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// batched separable calls (spx_batch_device.hpp; prox!: spx_proxstep_*_batch, spx_batch.hip; iprox!: spx_iproxstep_*_batch,
// spx_ibatch.hip): `batch` problems of n elements, problem b at elements [b * ld, b * ld + n) of every vector.  The functions
// the kernels walk a row with are the ones below, so the mapping (workgroup -> problem, tile, head, pairs, tail) is what
// tests/c/batch_plan_driver.hip enumerates on a CPU.  The two kinds of call differ here in two numbers only (BatchKind).
// ---------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#define SPX_PLAN_HD __host__ __device__
#else
#define SPX_PLAN_HD
#endif
constexpr int kBatchTile = 3072;            // elements of a row per tile: 256 lanes x 6 pairs (element-wise: x 12 elements)
constexpr int64_t kBatchRowMax = 4 * (int64_t)kBatchTile;  // one workgroup owns a whole problem up to here (12288); beyond: one tile per workgroup
constexpr int64_t kBatchGridMax = 0x7fffffff;
struct BatchKind {
  int vectors;  // one bit each in base_alignment_bits, in this order; an absent xkn counts as y
  int planes;   // sums per problem = planes of partials in the tiled form's workspace
  constexpr int all_off() const { return (1 << vectors) - 1; }
};
constexpr BatchKind kBatchProx{5, 3};   // y, q, xk, sj, xkn;    h terms, <q, y>, <y, y>
constexpr BatchKind kBatchIprox{6, 4};  // y, g, d, xk, sj, xkn; h terms, <g, y>, <d .* y, y>, <y, y>

enum class BatchForm { kRow, kTiled };
struct BatchPlan {
  bool ok;          // false: the call needs more than kBatchGridMax workgroups (refused)
  BatchForm form;   // a function of n alone: a problem's bits do not depend on its neighbours
  bool pairs;       // 16-byte accesses with per-row peeling; false: element-wise
  int base_odd;     // pairs: the bases sit 8 bytes off a 16-byte boundary
  int64_t grid;     // workgroups of the launch that stores y
  int64_t tiles_per_problem;
  size_t ws_bytes;  // tiled form: the kind's planes of partials per problem, laid out [problem][plane][tile]
};
// A row in the pairs form: `head` (0 or 1) scalar elements up to the row's first 16-byte boundary, npairs pairs, `tail` (0 or 1)
// scalar elements.  Element-wise form: n units of one element, no head, no tail.
struct BatchRowMap { int head; int64_t npairs; int tail; };
SPX_PLAN_HD inline BatchRowMap batch_row_map(int64_t n, int64_t b, int64_t ld, int base_odd) {
  BatchRowMap m;
  m.head = (int)((b * ld + base_odd) & 1);
  if (m.head > n) m.head = (int)n;
  m.npairs = (n - m.head) >> 1;
  m.tail = (int)(n - m.head - 2 * m.npairs);
  return m;
}
SPX_PLAN_HD inline int64_t batch_tiles(int64_t n) { return (n + kBatchTile - 1) / kBatchTile; }
// the units (pairs, or elements in the element-wise form) [*lo, *hi) of `count` that tile `tile` owns, units_per_tile a time
SPX_PLAN_HD inline void batch_tile_units(int64_t count, int64_t tile, int units_per_tile, int64_t* lo, int64_t* hi) {
  const int64_t a = tile * units_per_tile;
  const int64_t e = a + units_per_tile;
  *lo = a < count ? a : count;
  *hi = e < count ? e : count;
}
// workgroup -> (problem, tile) of the tiled form, and the slot of its partial sum `plane` (of `planes`) in the workspace
SPX_PLAN_HD inline void batch_workgroup(int64_t wg, int64_t tiles, int64_t* problem, int64_t* tile) {
  *problem = wg / tiles;
  *tile = wg - *problem * tiles;
}
SPX_PLAN_HD inline int64_t batch_slot(int64_t problem, int plane, int64_t tile, int64_t tiles, int planes) {
  return (problem * planes + plane) * tiles + tile;
}

// base_alignment_bits: bit k set = vector k of the kind starts 8 bytes off a 16-byte boundary
inline BatchPlan batch_plan(int64_t n, int64_t batch, int64_t ld, int base_alignment_bits, BatchKind kind) {
  (void)ld;  // (the rows' parities come from ld in batch_row_map; the launch shape does not depend on it)
  BatchPlan p{};
  p.form = n <= kBatchRowMax ? BatchForm::kRow : BatchForm::kTiled;
  p.pairs = base_alignment_bits == 0 || base_alignment_bits == kind.all_off();
  p.base_odd = (p.pairs && base_alignment_bits != 0) ? 1 : 0;
  p.tiles_per_problem = batch_tiles(n);
  if (p.form == BatchForm::kRow) {
    p.grid = batch;
  } else {
    if (batch > kBatchGridMax / p.tiles_per_problem) return p;  // (no overflow: tiles_per_problem >= 5 here)
    p.grid = batch * p.tiles_per_problem;
    p.ws_bytes = (size_t)batch * kind.planes * (size_t)p.tiles_per_problem * sizeof(double);
  }
  p.ok = p.grid <= kBatchGridMax;
  return p;
}

// ---------------------------------------------------------------------------------------------
// batched group call (spx_proxstep_group_l2_batch, spx_gbatch.hip): `batch` problems of ngroups uniform contiguous groups of
// group_size elements, problem b at elements [b * ld, b * ld + ngroups * group_size) of every vector.  A wavefront serves
// 64 / lpg groups at a time (a wave tile; lpg = the lanes per group of the size's row of GroupTilesPlain, spx_group_common.hpp,
// handed in by the caller: the table is stated there, once).
//   row form   (n = ngroups * group_size <= kBatchRowMax): one workgroup owns a problem; wave w takes its wave tiles w, w + 4, ...
//   tiled form (larger n): workgroup (b, t) takes the groups [t * run, (t + 1) * run) of problem b -- whole groups, `run` a
//              multiple of the 4 wave tiles a workgroup serves side by side, about kBatchTile elements -- and stores three
//              partials to batch_slot(b, plane, t); the reduce kernel, one workgroup per problem, adds them.
// Form, run and tiles are functions of (group_size, ngroups) alone: a problem's bits do not depend on batch or on its row.
// Pairs (16-byte accesses): group_size even, ld even and every base on a 16-byte boundary -- every group of every row then
// starts on one; otherwise the element-wise form for the whole launch.
// ---------------------------------------------------------------------------------------------
constexpr int kGBatchPlanes = 3;  // h terms, <q, y>, <y, y>
struct GBatchPlan {
  bool ok;          // false: the call needs more than kBatchGridMax workgroups (refused)
  BatchForm form;
  bool pairs;
  int64_t run;      // groups per workgroup of the tiled form (row form: all of them)
  int64_t tiles_per_problem;
  int64_t grid;     // workgroups of the launch that stores y
  size_t ws_bytes;  // tiled form: kGBatchPlanes planes of partials per problem, [problem][plane][tile]
};
// groups per tile of the tiled form: the largest multiple of 4 * (64 / lpg) groups within kBatchTile elements, at least one
SPX_PLAN_HD inline int64_t gbatch_run(int64_t group_size, int lpg) {
  const int64_t quad = 4 * (64 / lpg);
  const int64_t k = kBatchTile / (group_size * quad);
  return (k < 1 ? 1 : k) * quad;
}
// the groups [*lo, *hi) of a problem that tile `tile` owns
SPX_PLAN_HD inline void gbatch_tile_groups(int64_t ngroups, int64_t tile, int64_t run, int64_t* lo, int64_t* hi) {
  const int64_t a = tile * run;
  const int64_t e = a + run;
  *lo = a < ngroups ? a : ngroups;
  *hi = e < ngroups ? e : ngroups;
}
// base_alignment_bits: bit k set = vector k of y, q, xk, sj, xkn starts off a 16-byte boundary (an absent xkn: clear).
// ngroups * group_size must not overflow (the caller refuses that first).
inline GBatchPlan gbatch_plan(int64_t group_size, int lpg, int64_t ngroups, int64_t batch, int64_t ld, int base_alignment_bits) {
  GBatchPlan p{};
  const int64_t n = ngroups * group_size;
  p.form = n <= kBatchRowMax ? BatchForm::kRow : BatchForm::kTiled;
  p.pairs = (group_size & 1) == 0 && (ld & 1) == 0 && base_alignment_bits == 0;
  if (p.form == BatchForm::kRow) {
    p.run = ngroups;
    p.tiles_per_problem = 1;
    p.grid = batch;
  } else {
    p.run = gbatch_run(group_size, lpg);
    p.tiles_per_problem = (ngroups + p.run - 1) / p.run;
    if (batch > kBatchGridMax / p.tiles_per_problem) return p;  // (no overflow: tiles_per_problem >= 5 here)
    p.grid = batch * p.tiles_per_problem;
    p.ws_bytes = (size_t)batch * kGBatchPlanes * (size_t)p.tiles_per_problem * sizeof(double);
  }
  p.ok = p.grid <= kBatchGridMax;
  return p;
}

// ---------------------------------------------------------------------------------------------
// batched Binf group call (spx_proxstep_group_l2_binf_batch, spx_gbinf_batch.hip): gbatch_plan with the lanes per group of the
// size's row of GroupTilesBinf.  A workgroup keeps one bit per group it owns -- group g of the workgroup's [g_lo, g_hi) is bit
// (g - g_lo) & 63 of word (g - g_lo) >> 6 -- and sets it where the group wants the literal evaluation; a workgroup owns at most
// kBatchRowMax groups (row form, groups of one element; a tile of the tiled form holds at most kBatchTile).  Behind one barrier
// the workgroup walks the bitmap in a fixed order, which is all of this section: wave w takes the words w, w + kBinfWalkWaves,
// ...; a word's set bits are served `slots` at a time (slots = 64 / lanes per group of the GroupTilesLit row), in ascending order:
// pass p gives slot s the (p * slots + s)-th set bit.  Every set bit is visited once, and a wave meets its groups in ascending
// order -- so the order in which a lane adds its terms depends on the row's own bits alone.
// ---------------------------------------------------------------------------------------------
constexpr int kBinfBitmapWords = (int)(kBatchRowMax / 64);  // 192 words, 1.5 KiB
constexpr int kBinfWalkWaves = 4;                           // wavefronts of a workgroup
SPX_PLAN_HD inline int binf_bitmap_words(int64_t groups) { return (int)((groups + 63) / 64); }
// passes a word needs at `slots` groups a pass
SPX_PLAN_HD inline int binf_walk_passes(unsigned long long word, int slots) {
  return (__builtin_popcountll(word) + slots - 1) / slots;
}
// the bit (0 .. 63) that slot `slot` of pass `pass` serves, or -1 when the word has no such set bit
SPX_PLAN_HD inline int binf_walk_bit(unsigned long long word, int slots, int pass, int slot) {
  const int k = pass * slots + slot;
  for (int i = 0; i < k && word != 0ull; ++i) word &= word - 1ull;  // drop the k lowest set bits
  return word != 0ull ? __builtin_ctzll(word) : -1;
}

// ---------------------------------------------------------------------------------------------
// row-owner batched calls (spx_row_batch.hpp): `batch` problems of n elements, problem b at elements [b * ld, b * ld + n) of
// every vector.  ONE workgroup owns a problem from its first load to its last store: no workgroup waits for another, so there is
// no residency question and no workspace.  What a call alone decides is its shape (RowBatchShape); the plan is the same function
// of it for every call.
//   row-resident (n <= row_max): the row stays in registers; lanes x elements per lane by n (the shape's tiles) -- a row of 1e3
//              takes 256 lanes, not a CU-wide workgroup.
//   row walk   (row_max < n <= n_max): walk_lanes lanes re-read the row once per pass (from L2 or the Infinity Cache at these
//              sizes), walk_unroll units in flight per lane.  Beyond n_max the call is refused: a single call serves such a problem.
// A lane owns the units u = k * lanes + t (k = 0, 1, ...) in EVERY pass; a unit is a 16-byte pair of elements (pairs) or one
// element (element-wise).  Pairs: y, q, xk, sj all on a 16-byte boundary, ld even and n >= 2 -- every row then starts on one; a
// row of odd n ends in a unit of one element.  Otherwise the element-wise form for the whole launch.  xkn takes no part in the
// choice: where it sits 8 bytes off, only its stores drop to 8 bytes (xkn_pairs).
// Form, tile and pairs are functions of n and the alignment class alone: a problem's bits do not depend on batch or on its row.
// ---------------------------------------------------------------------------------------------
struct RowBatchTile { int lanes, epl; };
struct RowBatchShape {
  const RowBatchTile* tiles;  // ascending by lanes x epl; the last one holds row_max elements
  int tile_count;
  int64_t row_max;            // the resident bound
  int64_t n_max;
  int walk_lanes;
  int walk_unroll;            // units a lane of the row walk has in flight
};
enum class RowBatchForm { kResident, kWalk };
enum class RowBatchRefusal { kNone, kNTooLarge, kBatchTooLarge };
struct RowBatchPlan {
  bool ok;
  RowBatchRefusal why;  // !ok
  RowBatchForm form;
  int tile;             // kResident: the row of the shape's tiles; -1 on the walk
  int lanes;            // of the workgroup
  int epl;              // kResident: elements per lane held in registers; 0 on the walk
  bool pairs;
  bool xkn_pairs;       // xkn is stored by 16-byte pairs too
  int64_t grid;         // = batch
};
// units of a row: full ones and, in the pairs form with odd n, one of a single element behind them
SPX_PLAN_HD inline int64_t row_batch_units(int64_t n, bool pairs) { return pairs ? (n + 1) >> 1 : n; }
// the unit that slot k of lane t owns
SPX_PLAN_HD inline int64_t row_batch_unit(int64_t k, int lanes, int t) { return k * lanes + t; }
// base_alignment_bits: bit k set = vector k of y, q, xk, sj, xkn starts off a 16-byte boundary (an absent xkn: clear)
inline RowBatchPlan row_batch_plan(const RowBatchShape& s, int64_t n, int64_t batch, int64_t ld, int base_alignment_bits) {
  RowBatchPlan p{};
  if (n > s.n_max) { p.why = RowBatchRefusal::kNTooLarge; return p; }
  if (batch > kBatchGridMax) { p.why = RowBatchRefusal::kBatchTooLarge; return p; }
  p.pairs = (base_alignment_bits & 15) == 0 && (ld & 1) == 0 && n >= 2;
  p.xkn_pairs = p.pairs && (base_alignment_bits & 16) == 0;
  if (n <= s.row_max) {
    p.form = RowBatchForm::kResident;
    p.tile = 0;
    while ((int64_t)s.tiles[p.tile].lanes * s.tiles[p.tile].epl < n) ++p.tile;
    p.lanes = s.tiles[p.tile].lanes;
    p.epl = s.tiles[p.tile].epl;
  } else {
    p.form = RowBatchForm::kWalk;
    p.tile = -1;
    p.lanes = s.walk_lanes;
    p.epl = 0;
  }
  p.grid = batch;
  p.ok = true;
  return p;
}

// batched ShiftedNormL1B2 call (spx_proxstep_l1_b2_batch, spx_b2_batch.hip): the workgroup runs the whole root iteration
// (spx_b2_row.hpp).  Resident: xk and the box ends of the row stay in registers across the reductions; the largest tile is that
// of k_b2_coop<REG>.  Walk: the row is re-read once per reduction.  n > kB2BatchNMax: spx_proxstep_l1_b2 holds such a problem on
// chip across many CUs.
constexpr int64_t kB2BatchRowMax = kB2RegBlock;          // 8192: 512 lanes x 16 elements, the tile of k_b2_coop<REG>
constexpr int64_t kB2BatchNMax = (int64_t)1 << 20;
constexpr int kB2BatchWalkLanes = 1024;
constexpr int kB2BatchWalkUnroll = 4;
constexpr int kB2BatchTileCount = 4;
constexpr RowBatchTile kB2BatchTiles[kB2BatchTileCount] = {{64, 4}, {256, 4}, {256, 16}, {kB2RegThreads, kB2Epl}};  // 256, 1024, 4096, 8192 elements
constexpr RowBatchShape kB2BatchShape = {kB2BatchTiles, kB2BatchTileCount, kB2BatchRowMax, kB2BatchNMax, kB2BatchWalkLanes,
                                         kB2BatchWalkUnroll};

// batched top-r calls (spx_proxstep_indball_l0[_binf]_batch, spx_topr_batch.hip): the workgroup runs the whole selection
// (spx_topr_row.hpp).  Resident: v, xk + sj and q of the row stay in registers across the digit passes; the largest tile is what
// the histogram in LDS and three doubles per element leave room for.  Walk: v is parked in the row of y and re-read once per
// digit.  n > kToprBatchNMax: spx_prox_indball_l0[_binf] spreads such a problem over many CUs.
constexpr int64_t kToprBatchRowMax = 8192;               // 512 lanes x 16 elements
constexpr int64_t kToprBatchNMax = (int64_t)1 << 20;
constexpr int kToprBatchWalkLanes = 1024;
constexpr int kToprBatchWalkUnroll = 4;
constexpr int kToprBatchTileCount = 4;
constexpr RowBatchTile kToprBatchTiles[kToprBatchTileCount] = {{64, 4}, {256, 4}, {256, 16}, {512, 16}};  // 256, 1024, 4096, 8192 elements
constexpr RowBatchShape kToprBatchShape = {kToprBatchTiles, kToprBatchTileCount, kToprBatchRowMax, kToprBatchNMax,
                                           kToprBatchWalkLanes, kToprBatchWalkUnroll};
