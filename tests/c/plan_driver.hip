/* Stand-alone driver for the device-free plan functions (csrc/spx_plan.hpp): sel_plan, sel_fast_ws, b2_plan, team_alignment and
 * team_layout.  Each is compared with the decision code it replaced -- run_select and run_select_fast of spx_select.hip (form,
 * grid, tail grid, workspace layout), run_b2 of spx_b2.hip, team_layout of spx_group_team.hip -- restated here word for word,
 * with the context's fields in a plain struct (Ctx) and spx_resident_cap answering from a table that also records which kernels
 * were asked, in which order.  Compared: every field of the plan, the route or error, and the sequence of kernels asked.
 * Over: both precisions; residency 0, 1, 2, 4, 64, 255, 256, 304 and 100000 for all kernels and for each kernel on its own
 * (front also 63 against 64); tuning keys 2, 6, 12, 14 on and off, key 11 in {0, 1, 2}, key 10 in {0, 1, 2, 3, 4, 16}, forced
 * grid 0 and 5; vectors all aligned, all 8 bytes off, mixed; n = 1, 2, every constant the code names and every bound it derives
 * from the residency in force at -1, 0, +1, 2^31 +- 1, 10^10; r = 0, 1, n/100, n/2, n - 1, n and the r next to
 * pcut (1 - pcut) = 0.04.  The pointers are integers and are never dereferenced.
 * Compiled with hipcc --offload-host-only and -Xarch_host -fsanitize=address,undefined and run as a child by
 * tests/test_plan_host.py; it has its own main, the library is not loaded, no HIP call is made.
 * `plan_driver print PREC N R ALIGN CAP [K2 K6 K10 K11 K12]` prints the plans of one call instead (tools/README.md). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "spx_plan.hpp"

static long g_checked = 0;
static int g_fail = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++g_checked;                                                                               \
    if (!(cond)) { if (g_fail < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

// ---------------------------------------------------------------------------------------------
// stand-ins for what the restated code reads
// ---------------------------------------------------------------------------------------------
enum { SPX_OK = 0, SPX_ERR_INTERNAL = 5 };
struct Asked {  // the kernels asked, in order
  int k[8];
  int n = 0;
  void add(int id) { if (n < 8) k[n] = id; ++n; }
  bool operator==(const Asked& o) const { return n == o.n && n <= 8 && std::equal(k, k + n, o.k); }
};
struct Ctx {
  int num_cu = 256;
  int tune_sel_fast = 1, tune_sel_small = 1, tune_front_spl = 0, tune_sel_reg16 = 1, tune_b2_lds = 1, tune_team_fast = 1;
  int tune_force_grid = 0;
  int64_t cap_sel[10] = {};  // by SelKernel
  int64_t cap_b2[4] = {};    // by B2Form
  int64_t cap_team = 0;
  Asked asked;
};
static int64_t spx_resident_cap(Ctx* ctx, SelKernel k, int, size_t) { ctx->asked.add((int)k); return ctx->cap_sel[(int)k]; }
static int64_t spx_resident_cap(Ctx* ctx, B2Form k, int, size_t) { ctx->asked.add((int)k); return ctx->cap_b2[(int)k]; }
static inline bool spx_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// vector i of a call at byte offset `off` of its own page
template <class T>
static T* at(int i, int off) { return reinterpret_cast<T*>((uintptr_t)0x100000 + (uintptr_t)0x1000 * i + (uintptr_t)off); }

// device-side structs of spx_select.hip and spx_group_team.hip, for their sizes
struct WaveCount { unsigned int cand, above; };
struct ClassCount { unsigned int hi, lo; };
struct Cand { uint64_t key; int64_t idx; double val; };
struct f64x2 { double x, y; };
struct TeamJob { int64_t lo, hi; int gid, first, W, pad; };
struct TeamPlanHdr { int active, njobs, loop, pad; int wg_job[kGtCols]; };

// ---------------------------------------------------------------------------------------------
// top-r as it was: run_select, with run_select_fast's tail grid behind it.  A launch is recorded, not made.
// ---------------------------------------------------------------------------------------------
struct OldSel {
  int rc = SPX_OK;
  SelRoute route = SelRoute::kExact;
  SelForm form = SelForm::kCoopMem;
  bool vec = false;
  int64_t g = 0, g_tail = 0;
  int ioff = 0, spl = 1;
};
static int old_select_fast(Ctx* ctx, int ioff, int spl, OldSel* o) {
  const int64_t cap_tail = spx_resident_cap(ctx, SelKernel::kTail, 1024, 0);
  if (cap_tail < 1) return SPX_ERR_INTERNAL;
  const int64_t g_tail = cap_tail < 256 ? (cap_tail < ctx->num_cu ? cap_tail : ctx->num_cu) : (ctx->num_cu < 256 ? ctx->num_cu : 256);  // (<= 256: SelSync::tie_part)
  o->route = SelRoute::kFast;
  o->g_tail = g_tail;
  o->ioff = ioff;
  o->spl = spl;
  return SPX_OK;
}
template <class T>
static int old_select(Ctx* ctx, T* y, const T* q, const T* xk, const T* sj, int64_t n, int64_t r, OldSel* o) {
  if (n <= kSmallNCoop && ctx->tune_sel_small) {
    o->route = SelRoute::kSmall;
    return SPX_OK;
  }
  const bool vec = spx_aligned16(y) && spx_aligned16(q) && spx_aligned16(xk) && spx_aligned16(sj);
  const int64_t cap_reg = spx_resident_cap(ctx, SelKernel::kCoopReg, 1024, 0);
  const int64_t cap_mem = spx_resident_cap(ctx, SelKernel::kCoopMem, 1024, 0);
  if (cap_mem < 1) return SPX_ERR_INTERNAL;  // (message set by spx_resident_cap)
  const int64_t reg_cap = (int64_t)kCoopEpl * 1024 * (cap_reg < ctx->num_cu ? cap_reg : ctx->num_cu);  // (2 Mi elements on 256 CUs)
  constexpr int kLdsSlots = std::is_same<T, double>::value ? kLdsEpl : kLdsEpl32;
  int64_t lds_cap = 0;
  if (ctx->tune_sel_reg16) {
    const int64_t capl = vec ? spx_resident_cap(ctx, SelKernel::kLdsVec, 1024, 0)
                             : spx_resident_cap(ctx, SelKernel::kLdsScalar, 1024, 0);
    lds_cap = (int64_t)kLdsSlots * 1024 * (capl < ctx->num_cu ? capl : ctx->num_cu);
  }
  const int64_t g_mem = cap_mem < ctx->num_cu ? cap_mem : ctx->num_cu;  // grid of the form that parks v in y: any size >= 1 works
  const int64_t g_lds = lds_cap / ((int64_t)kLdsSlots * 1024);
  SelForm form;
  int64_t g;
  if constexpr (std::is_same<T, float>::value) {
    const bool lds = n <= lds_cap && n > reg_cap;
    const bool reg = !lds && n <= reg_cap;
    form = lds ? SelForm::kLds : reg ? SelForm::kCoopReg : SelForm::kCoopMem;
    g = lds ? g_lds : reg ? (n + (int64_t)kCoopEpl * 1024 - 1) / ((int64_t)kCoopEpl * 1024) : g_mem;
  } else {
    auto off8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 8u; };
    const int ioff = (!vec && off8(y) && off8(q) && off8(xk) && off8(sj)) ? 1 : 0;
    const double pcut = (double)r / (double)n;
    int spl = n >= ((int64_t)1 << 25) ? 4 : (n >= ((int64_t)1 << 23) ? 2 : 1);
    if (n >= ((int64_t)1 << 26) && pcut * (1.0 - pcut) > 0.04) spl = 16;
    if (ctx->tune_front_spl == 1 || ctx->tune_front_spl == 2 || ctx->tune_front_spl == 4 || ctx->tune_front_spl == 16) spl = ctx->tune_front_spl;
    const SelKernel front_fn = spl == 16 ? SelKernel::kFront16
                             : spl == 4 ? SelKernel::kFront4
                             : spl == 2 ? SelKernel::kFront2
                                        : SelKernel::kFront1;
    const int64_t cap_front = spx_resident_cap(ctx, front_fn, 1024, 0);
    int64_t hyb_cap = 0;
    if (ctx->tune_sel_reg16 == 1 && vec && lds_cap > 0) {
      const int64_t caph = spx_resident_cap(ctx, SelKernel::kLdsRegX, 1024, 0);
      hyb_cap = (int64_t)(kLdsEpl + kLdsRegX) * 1024 * (caph < ctx->num_cu ? caph : ctx->num_cu);
      if (hyb_cap > 0x7fffffff) hyb_cap = 0;  // (the form indexes with 32-bit integers)
    }
    int64_t fast_min = ((int64_t)1 << SPX_SEL_REG_MAX_LOG2) + 1;
    if (lds_cap >= fast_min) fast_min = lds_cap + 1;
    if (hyb_cap >= fast_min) fast_min = hyb_cap + 1;
    const bool try_fast = ctx->tune_sel_fast && (vec || ioff) && (n - ioff) >= fast_min && r > 0 && r < n &&
                          cap_front >= kFrontBlocks;  // (the front kernel's sample layout is tied to its grid)
    if (try_fast) return old_select_fast(ctx, ioff, spl, o);
    const bool lds = n <= lds_cap && (n > kLdsMinN || n > reg_cap);
    const bool hyb = !lds && n > lds_cap && n <= hyb_cap;  // (vec: hyb_cap is 0 otherwise)
    const bool reg = !lds && !hyb && n <= reg_cap;
    const int64_t epl = n <= 65536 ? 1 : n <= 196608 ? 2 : n <= 655360 ? 4 : kCoopEpl;
    form = lds ? SelForm::kLds : hyb ? SelForm::kLdsRegX : reg ? SelForm::kCoopReg : SelForm::kCoopMem;
    g = g_mem;
    if (reg) {
      const int64_t gmax = cap_reg < ctx->num_cu ? cap_reg : ctx->num_cu;
      g = (n + epl * 1024 - 1) / (epl * 1024);
      if (g > gmax) g = gmax;  // (n <= reg_cap: 8 elements per lane always fit)
    }
    if (lds) g = g_lds;
    if (hyb) g = hyb_cap / ((int64_t)(kLdsEpl + kLdsRegX) * 1024);
    // (the test build's hook; a forced grid of 0 is the product build)
    if (!reg && !lds && !hyb && ctx->tune_force_grid > 0) g = ctx->tune_force_grid;
    o->ioff = ioff;
    o->spl = spl;
  }
  o->form = form;
  o->vec = vec;
  o->g = g;
  return SPX_OK;
}

// what run_select fills in from a call
template <class T>
static SelIn sel_in_of(const Ctx& c, T* y, const T* q, const T* xk, const T* sj, int64_t n, int64_t r) {
  auto off8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 8u; };
  SelIn in{};
  in.f64 = std::is_same<T, double>::value;
  in.n = n;
  in.r = r;
  in.vec = spx_aligned16(y) && spx_aligned16(q) && spx_aligned16(xk) && spx_aligned16(sj);
  in.all_off8 = off8(y) && off8(q) && off8(xk) && off8(sj);
  in.num_cu = c.num_cu;
  in.sel_fast = c.tune_sel_fast;
  in.sel_small = c.tune_sel_small;
  in.front_spl = c.tune_front_spl;
  in.sel_reg16 = c.tune_sel_reg16;
  in.force_grid = c.tune_force_grid;
  return in;
}

template <class T>
static void check_select(Ctx& c, int align, int64_t n, int64_t r) {
  // align 0: all 16-byte aligned; 1: all 8 bytes off; 2: mixed
  T* y = at<T>(0, align == 1 ? 8 : 0);
  const T* q = at<const T>(1, align ? 8 : 0);
  const T* xk = at<const T>(2, align == 1 ? 8 : 0);
  const T* sj = at<const T>(3, align ? 8 : 0);
  OldSel o;
  c.asked = Asked{};
  o.rc = old_select<T>(&c, y, q, xk, sj, n, r, &o);
  const Asked old_asked = c.asked;
  Asked new_asked;
  const SelPlan p = sel_plan(sel_in_of<T>(c, y, q, xk, sj, n, r), [&](SelKernel k) {
    new_asked.add((int)k);
    return c.cap_sel[(int)k];
  });
  CHECK(new_asked == old_asked);
  CHECK((p.route == SelRoute::kError) == (o.rc != SPX_OK));
  if (o.rc != SPX_OK) return;
  CHECK(p.route == o.route);
  if (o.route == SelRoute::kSmall) return;
  CHECK(p.ioff == o.ioff && p.spl == o.spl);
  if (o.route == SelRoute::kFast) CHECK(p.g_tail == o.g_tail && p.g_tail >= 1 && p.g_tail <= 256);
  else CHECK(p.form == o.form && p.vec == o.vec && p.g == o.g);
}

// the workspace of run_select_fast as it was, against sel_fast_ws
static void check_fast_ws(int64_t n, int ioff) {
  const int64_t n2 = (n - ioff) >> 1;
  const int64_t mblocks = (n2 + kMainTilePairs - 1) / kMainTilePairs;
  const int64_t nregions = mblocks * 4;
  const int64_t ccap = nregions * kWaveSlots;
  const int64_t ovf_cap64 = (n / 64 > 65536) ? n / 64 : 65536;
  const unsigned int ovf_cap = (unsigned int)(ovf_cap64 > 0x7fffffff ? 0x7fffffff : ovf_cap64);
  const size_t off_cnt = 256;
  const size_t off_cls = (off_cnt + (size_t)nregions * sizeof(WaveCount) + 255) & ~(size_t)255;   // tie mode: class members per slot
  const size_t off_ckey = (off_cls + (size_t)(nregions + 2) * sizeof(ClassCount) + 255) & ~(size_t)255;
  const size_t off_lkey = off_ckey + ((size_t)ccap + (size_t)ovf_cap) * sizeof(Cand);
  const size_t off_lidx = off_lkey + (size_t)kShortList * sizeof(uint64_t);
  const size_t off_lval = off_lidx + (size_t)kShortList * sizeof(int64_t);
  const size_t total = off_lval + (size_t)kShortList * sizeof(double) + 256;
  const SelFastWs w = sel_fast_ws(n, ioff, sizeof(WaveCount), sizeof(ClassCount), sizeof(Cand));
  CHECK(w.n2 == n2 && w.mblocks == mblocks && w.nregions == nregions && w.ccap == ccap && w.ovf_cap == ovf_cap);
  CHECK(w.off_cnt == off_cnt && w.off_cls == off_cls && w.off_ckey == off_ckey && w.off_lkey == off_lkey && w.off_lidx == off_lidx &&
        w.off_lval == off_lval && w.bytes == total);
  // (ascending; the count words are an empty region below two elements, which the pipeline never sees)
  CHECK((w.off_cnt < w.off_cls || (w.nregions == 0 && w.off_cnt == w.off_cls)) && w.off_cls < w.off_ckey && w.off_ckey < w.off_lkey && w.off_lkey < w.off_lidx &&
        w.off_lidx < w.off_lval && w.off_lval < w.bytes);
  CHECK(w.off_cnt + (size_t)w.nregions * sizeof(WaveCount) <= w.off_cls);
  CHECK(w.off_cls + (size_t)(w.nregions + 2) * sizeof(ClassCount) <= w.off_ckey);
  CHECK(w.off_ckey + ((size_t)w.ccap + w.ovf_cap) * sizeof(Cand) <= w.off_lkey);
  CHECK(w.off_lkey + (size_t)kShortList * 8 <= w.off_lidx && w.off_lidx + (size_t)kShortList * 8 <= w.off_lval &&
        w.off_lval + (size_t)kShortList * 8 <= w.bytes);
  CHECK(w.off_cnt % 256 == 0 && w.off_cls % 256 == 0 && w.off_ckey % 256 == 0);
}

// ---------------------------------------------------------------------------------------------
// ShiftedNormL1B2 as it was: run_b2 from the residency questions to the reservation of the workspace
// ---------------------------------------------------------------------------------------------
struct OldB2 {
  int rc = SPX_OK;
  B2Form form = kB2FormReg;
  int64_t g = 0, epl = 0, gmax_reg = 0, gmax_mem = 0, gmax_lds = 0;
  unsigned int cand_cap = 0;
  size_t ws_bytes = 0;
};
static int old_b2(Ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, OldB2* o) {
  const bool vec = n >= 2 && spx_aligned16(y) && spx_aligned16(q) && spx_aligned16(xk) && spx_aligned16(sj);
  const int64_t cap_reg = spx_resident_cap(ctx, kB2FormReg, kB2RegThreads, 0);
  const int64_t cap_mem = vec ? spx_resident_cap(ctx, kB2FormVec, 1024, 0)
                              : spx_resident_cap(ctx, kB2Form8, 1024, 0);
  if (cap_mem < 1) return SPX_ERR_INTERNAL;  // (message set by spx_resident_cap)
  const int64_t gmax_reg = cap_reg < kB2Cols ? cap_reg : kB2Cols;
  const int64_t gmax_mem = cap_mem < kB2Cols ? cap_mem : kB2Cols;
  const bool reg = n <= (int64_t)kB2RegBlock * gmax_reg;
  bool ldsx = false;
  int64_t gmax_lds = 0;
  if (!reg && ctx->tune_b2_lds) {
    const int64_t cap_lds = spx_resident_cap(ctx, kB2FormLds, 1024, 0);
    gmax_lds = cap_lds < kB2Cols ? cap_lds : kB2Cols;
    ldsx = n <= (int64_t)kB2Epl * 1024 * gmax_lds;
  }
  int64_t g = reg ? (n + kB2RegBlock - 1) / kB2RegBlock : gmax_mem;
  if (ldsx) g = gmax_lds;  // (n > 2 Mi here unless the grid is capped: every resident workgroup, <= 16 elements per lane)
  if (reg) {
    const int64_t epl = n <= 131072 ? 4 : n <= 524288 ? 8 : kB2Epl;
    int64_t gg = (n + epl * kB2RegThreads - 1) / (epl * kB2RegThreads);
    if (gg > gmax_reg) gg = gmax_reg;
    if (gg > g) g = gg;
    o->epl = epl;
  }
  if (g < 1) g = 1;
  const B2Form form = ldsx ? kB2FormLds : reg ? kB2FormReg : vec ? kB2FormVec : kB2Form8;
  unsigned int cand_cap = 0;
  if (!reg && !ldsx) {
    const int64_t waves = g * 16;
    const int64_t share = (n + waves - 1) / waves;
    int64_t cap = share / 12 + 64;
    if (cap > 0x7fffffff) cap = 0x7fffffff;
    cand_cap = (unsigned int)cap;
    o->ws_bytes = (size_t)waves * (size_t)cap * sizeof(f64x2) + 256;
  }
  o->form = form;
  o->g = g;
  o->gmax_reg = gmax_reg;
  o->gmax_mem = gmax_mem;
  o->gmax_lds = gmax_lds;
  o->cand_cap = cand_cap;
  return SPX_OK;
}
static void check_b2(Ctx& c, int align, int64_t n) {
  double* y = at<double>(0, align == 1 ? 8 : 0);
  const double* q = at<const double>(1, align ? 8 : 0);
  const double* xk = at<const double>(2, align == 1 ? 8 : 0);
  const double* sj = at<const double>(3, align ? 8 : 0);
  OldB2 o;
  c.asked = Asked{};
  o.rc = old_b2(&c, y, q, xk, sj, n, &o);
  const Asked old_asked = c.asked;
  Asked new_asked;
  const bool vec = n >= 2 && spx_aligned16(y) && spx_aligned16(q) && spx_aligned16(xk) && spx_aligned16(sj);
  const B2Plan p = b2_plan(B2In{n, vec, c.tune_b2_lds}, sizeof(f64x2), [&](B2Form f) {
    new_asked.add((int)f);
    return c.cap_b2[(int)f];
  });
  CHECK(new_asked == old_asked);
  CHECK(p.ok == (o.rc == SPX_OK));
  if (o.rc != SPX_OK) return;
  CHECK(p.form == o.form && p.g == o.g && p.epl == o.epl && p.g >= 1 && p.g <= kB2Cols);
  CHECK(p.gmax_reg == o.gmax_reg && p.gmax_mem == o.gmax_mem && p.gmax_lds == o.gmax_lds);
  CHECK(p.cand_cap == o.cand_cap && p.ws_bytes == o.ws_bytes);
}

// ---------------------------------------------------------------------------------------------
// team_layout of spx_group_team.hip as it was (one kernel is asked, whatever the layout: its answer is Ctx::cap_team)
// ---------------------------------------------------------------------------------------------
struct OldTeamLayout {
  bool vec;
  int par, G, Wu;
  int64_t grid;
  size_t plan_bytes, status_bytes, cand_bytes;
  unsigned int cand_cap;
};
static int old_team_layout(Ctx* ctx, bool binf, const double* y, const double* q, const double* xk, const double* sj, int64_t n,
                           const int64_t* offsets, int64_t gsize, int64_t ngroups, OldTeamLayout* L) {
  const auto bit3 = [](const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1u); };
  L->par = bit3(q);
  L->vec = bit3(xk) == L->par && bit3(sj) == L->par && bit3(y) == L->par;
  int64_t cap = ctx->cap_team;
  if (cap > kGtCols) cap = kGtCols;
  if (cap < 1) return SPX_ERR_INTERNAL;  // (message set by spx_resident_cap)
  L->G = (int)cap;
  L->Wu = 1;
  L->grid = L->G;
  int64_t per_wg = 2 * ((n + L->G - 1) / L->G);  // elements of one job per workgroup (a device-side plan: at most about that)
  if (!offsets) {
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
  L->plan_bytes = offsets ? ((sizeof(TeamPlanHdr) + (size_t)kTmMaxJobs * sizeof(TeamJob) + 255) & ~(size_t)255) : 0;
  {  // one word per job: at most kTmMaxJobs jobs in a device-side plan, ngroups jobs for uniform groups
    size_t jobs_max = (size_t)kTmMaxJobs;
    if (!offsets && (size_t)ngroups > jobs_max) jobs_max = (size_t)ngroups;
    L->status_bytes = (jobs_max * sizeof(int) + 255) & ~(size_t)255;
  }
  L->cand_cap = 0;
  L->cand_bytes = 0;
  if (binf && ctx->tune_team_fast) {
    int64_t c = per_wg / (kTmThreads / 64) / 4 + 64;
    if (c > 0x7fffffff) c = 0x7fffffff;
    L->cand_cap = (unsigned int)c;
    L->cand_bytes = (size_t)L->grid * (kTmThreads / 64) * (size_t)c * sizeof(f64x2);
  }
  return SPX_OK;
}
static void check_team(Ctx& c, bool binf, int bits, bool csr, int64_t n, int64_t gsize, int64_t ngroups) {
  const double* y = at<const double>(0, (bits & 1) ? 8 : 0);
  const double* q = at<const double>(1, (bits & 2) ? 8 : 0);
  const double* xk = at<const double>(2, (bits & 4) ? 8 : 0);
  const double* sj = at<const double>(3, (bits & 8) ? 8 : 0);
  const int64_t* offsets = csr ? at<const int64_t>(4, 0) : nullptr;
  OldTeamLayout o{};
  c.asked = Asked{};
  const int rc = old_team_layout(&c, binf, y, q, xk, sj, n, offsets, gsize, ngroups, &o);
  TeamLayout L{};
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  team_alignment(addr(y), addr(q), addr(xk), addr(sj), &L);
  CHECK(L.par == o.par && L.vec == o.vec);
  const int rn = team_layout(c.cap_team, c.tune_team_fast, binf, n, offsets != nullptr, gsize, ngroups, sizeof(TeamPlanHdr),
                             sizeof(TeamJob), sizeof(f64x2), &L);
  CHECK((rn != 0) == (rc != SPX_OK));
  if (rc != SPX_OK) return;
  CHECK(L.par == o.par && L.vec == o.vec && L.G == o.G && L.Wu == o.Wu && L.grid == o.grid);
  CHECK(L.plan_bytes == o.plan_bytes && L.status_bytes == o.status_bytes && L.cand_bytes == o.cand_bytes && L.cand_cap == o.cand_cap);
  CHECK(L.plan_bytes % 256 == 0 && L.status_bytes % 256 == 0 && L.G >= 1 && L.G <= kGtCols && L.grid >= 1 && L.grid <= kGtCols);
}

// ---------------------------------------------------------------------------------------------
// the grid of cases
// ---------------------------------------------------------------------------------------------
static const int64_t kCaps[] = {0, 1, 2, 4, 64, 255, 256, 304, 100000};

static void around(std::vector<int64_t>& v, int64_t x) { for (int64_t d = -1; d <= 1; ++d) if (x + d >= 1) v.push_back(x + d); }
static void dedupe(std::vector<int64_t>& v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}
static std::vector<int64_t> named_sizes() {
  std::vector<int64_t> v = {1, 2, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) + 1, 10000000000LL};
  for (int64_t x : {(int64_t)8192, (int64_t)65536, (int64_t)196608, (int64_t)655360, (int64_t)1 << 20, (int64_t)1 << 21,
                    (int64_t)131072, (int64_t)524288, (int64_t)1 << 23, (int64_t)1 << 25, (int64_t)1 << 26})
    around(v, x);
  return v;
}
// the bounds run_select derives from the residency in force: reg_cap, lds_cap, hyb_cap, fast_min
template <class T>
static std::vector<int64_t> sel_sizes(const Ctx& c) {
  std::vector<int64_t> v = named_sizes();
  const auto cus = [&](int64_t cap) { return cap < c.num_cu ? cap : (int64_t)c.num_cu; };
  const int64_t slots = std::is_same<T, double>::value ? kLdsEpl : kLdsEpl32;
  const int64_t reg_cap = (int64_t)kCoopEpl * 1024 * cus(c.cap_sel[(int)SelKernel::kCoopReg]);
  int64_t fast_min = ((int64_t)1 << SPX_SEL_REG_MAX_LOG2) + 1;
  around(v, reg_cap);
  for (SelKernel k : {SelKernel::kLdsVec, SelKernel::kLdsScalar}) {
    const int64_t lds_cap = c.tune_sel_reg16 ? slots * 1024 * cus(c.cap_sel[(int)k]) : 0;
    around(v, lds_cap);
    if (lds_cap >= fast_min) fast_min = lds_cap + 1;
  }
  const int64_t hyb_cap = (int64_t)(kLdsEpl + kLdsRegX) * 1024 * cus(c.cap_sel[(int)SelKernel::kLdsRegX]);
  around(v, hyb_cap);
  if (c.tune_sel_reg16 == 1 && hyb_cap <= 0x7fffffff && hyb_cap >= fast_min) fast_min = hyb_cap + 1;
  around(v, fast_min);
  around(v, fast_min + 1);  // (n - ioff >= fast_min with ioff = 1)
  dedupe(v);
  return v;
}
static std::vector<int64_t> ranks(int64_t n) {
  std::vector<int64_t> v = {0, 1, n / 100, n / 2, n - 1, n};
  const double p = 0.5 * (1.0 - sqrt(1.0 - 4.0 * 0.04));  // p (1 - p) = 0.04, and 1 - p
  for (double root : {p, 1.0 - p}) {
    const int64_t f = (int64_t)floor(root * (double)n);
    for (int64_t d = -1; d <= 2; ++d) v.push_back(f + d);
  }
  for (auto& r : v) r = r < 0 ? 0 : r > n ? n : r;
  dedupe(v);
  return v;
}

template <class T>
static void sweep_select_keys(Ctx& c) {
  static const int k10[] = {0, 1, 2, 3, 4, 16};
  for (int fast = 0; fast < 2; ++fast) for (int small = 0; small < 2; ++small) for (int reg16 = 0; reg16 < 3; ++reg16)
    for (int force : {0, 5}) {
      c.tune_sel_fast = fast; c.tune_sel_small = small; c.tune_sel_reg16 = reg16; c.tune_force_grid = force;
      const std::vector<int64_t> sizes = sel_sizes<T>(c);
      for (int64_t n : sizes) {
        const std::vector<int64_t> rs = ranks(n);
        for (int spl : k10) {
          c.tune_front_spl = spl;
          for (int align = 0; align < 3; ++align)
            for (int64_t r : rs) check_select<T>(c, align, n, r);
        }
      }
    }
}
template <class T>
static void sweep_select() {
  Ctx c;
  for (int num_cu : {256, 100000}) {
    c.num_cu = num_cu;
    for (int64_t all : kCaps) {  // every kernel alike
      for (auto& x : c.cap_sel) x = all;
      sweep_select_keys<T>(c);
    }
  }
  c.num_cu = 256;
  for (int k = 0; k < 10; ++k)  // each kernel on its own, the others at 256
    for (int64_t one : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)4, (int64_t)63, (int64_t)64, (int64_t)255, (int64_t)304, (int64_t)100000}) {
      for (auto& x : c.cap_sel) x = 256;
      c.cap_sel[k] = one;
      sweep_select_keys<T>(c);
    }
  // reg = 0 with mem > 0 on a device of many CUs; the hybrid form's 32-bit limit with everything else small
  c.num_cu = 100000;
  for (auto& x : c.cap_sel) x = 100000;
  c.cap_sel[(int)SelKernel::kCoopReg] = 0;
  sweep_select_keys<T>(c);
  for (auto& x : c.cap_sel) x = 256;
  c.cap_sel[(int)SelKernel::kLdsRegX] = 100000;
  sweep_select_keys<T>(c);
}

static void sweep_fast_ws() {
  std::vector<int64_t> v = named_sizes();
  for (int64_t x : {(int64_t)2 * kMainTilePairs, (int64_t)64 * 65536, (int64_t)64 * 0x7fffffff, (int64_t)6 << 20}) around(v, x);
  around(v, 2 * kMainTilePairs + 1);
  dedupe(v);
  for (int64_t n : v) for (int ioff = 0; ioff < 2; ++ioff) check_fast_ws(n, ioff);
}

static void sweep_b2() {
  Ctx c;
  auto sizes = [&]() {
    std::vector<int64_t> v = named_sizes();
    for (int f : {0, 1, 2, 3}) {
      const int64_t gmax = c.cap_b2[f] < kB2Cols ? c.cap_b2[f] : kB2Cols;
      around(v, (int64_t)kB2RegBlock * gmax);
      around(v, (int64_t)16384 * gmax);
    }
    dedupe(v);
    return v;
  };
  auto run = [&]() {
    for (int lds = 0; lds < 2; ++lds) {
      c.tune_b2_lds = lds;
      for (int64_t n : sizes()) for (int align = 0; align < 3; ++align) check_b2(c, align, n);
    }
  };
  for (int64_t all : kCaps) { for (auto& x : c.cap_b2) x = all; run(); }
  for (int k = 0; k < 4; ++k)
    for (int64_t one : kCaps)
      for (int64_t rest : {(int64_t)256, (int64_t)4}) {
        for (auto& x : c.cap_b2) x = rest;
        c.cap_b2[k] = one;
        run();
      }
}

static void sweep_team() {
  Ctx c;
  const std::vector<int64_t> sizes = named_sizes();
  for (int64_t cap : kCaps) for (int fast = 0; fast < 2; ++fast) for (int binf = 0; binf < 2; ++binf) {
    c.cap_team = cap; c.tune_team_fast = fast;
    for (int bits = 0; bits < 16; ++bits)
      for (int64_t n : sizes) {
        check_team(c, binf, bits, true, n, 0, 1);  // a device-side plan: gsize 0, as spx_group_team_plan passes it
        for (int64_t ng : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)65535, (int64_t)65536, (int64_t)65537, (int64_t)1000000}) {
          check_team(c, binf, bits, true, n, n / ng, ng);
          for (int64_t gs : {(int64_t)0, (int64_t)1, (int64_t)2047, (int64_t)2048, (int64_t)2049, (int64_t)9216, (int64_t)9217, n / ng + 1, n})
            check_team(c, binf, bits, false, n, gs, ng);
        }
      }
  }
}

// `print`: the plans of one call, as a table row per plan
static int print_plans(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: plan_driver print f32|f64 N R aligned|off8|mixed CAP [K2 K6 K10 K11 K12]\n"); return 2; }
  Ctx c;
  const bool f64 = strcmp(argv[2], "f32") != 0;
  const int64_t n = atoll(argv[3]), r = atoll(argv[4]);
  const int align = !strcmp(argv[5], "off8") ? 1 : !strcmp(argv[5], "mixed") ? 2 : 0;
  const int64_t cap = atoll(argv[6]);
  if (argc > 7) c.tune_sel_fast = atoi(argv[7]);
  if (argc > 8) c.tune_sel_small = atoi(argv[8]);
  if (argc > 9) c.tune_front_spl = atoi(argv[9]);
  if (argc > 10) c.tune_sel_reg16 = atoi(argv[10]);
  if (argc > 11) c.tune_b2_lds = atoi(argv[11]);
  static const char* kRoute[] = {"small", "exact", "fast", "error"};
  static const char* kForm[] = {"coop-reg", "coop-mem", "lds", "lds-regx"};
  static const char* kB2[] = {"reg", "lds", "vec", "8"};
  SelIn in{};
  in.f64 = f64; in.n = n; in.r = r; in.vec = align == 0; in.all_off8 = align == 1; in.num_cu = c.num_cu;
  in.sel_fast = c.tune_sel_fast; in.sel_small = c.tune_sel_small; in.front_spl = c.tune_front_spl; in.sel_reg16 = c.tune_sel_reg16;
  printf("top-r   asked:");
  const SelPlan p = sel_plan(in, [&](SelKernel k) { printf(" %d", (int)k); return cap; });
  printf("  route %s form %s vec %d g %lld ioff %d spl %d g_tail %lld\n", kRoute[(int)p.route], kForm[(int)p.form], (int)p.vec,
         (long long)p.g, p.ioff, p.spl, (long long)p.g_tail);
  if (p.route == SelRoute::kFast) {
    const SelFastWs w = sel_fast_ws(n, p.ioff, sizeof(WaveCount), sizeof(ClassCount), sizeof(Cand));
    printf("        main grid %lld regions %lld ccap %lld ovf_cap %u offsets %zu %zu %zu %zu %zu %zu bytes %zu\n", (long long)w.mblocks,
           (long long)w.nregions, (long long)w.ccap, w.ovf_cap, w.off_cnt, w.off_cls, w.off_ckey, w.off_lkey, w.off_lidx, w.off_lval, w.bytes);
  }
  printf("B2      asked:");
  const B2Plan b = b2_plan(B2In{n, n >= 2 && align == 0, c.tune_b2_lds}, sizeof(f64x2), [&](B2Form f) { printf(" %s", kB2[f]); return cap; });
  printf("  ok %d form %s g %lld epl %lld cand_cap %u ws %zu\n", (int)b.ok, kB2[b.form], (long long)b.g, (long long)b.epl, b.cand_cap, b.ws_bytes);
  TeamLayout L{};
  L.vec = align != 2;
  if (!team_layout(cap, c.tune_team_fast, true, n, false, n, 1, sizeof(TeamPlanHdr), sizeof(TeamJob), sizeof(f64x2), &L))
    printf("team    one Binf group: G %d Wu %d grid %lld status %zu cand_cap %u cand %zu\n", L.G, L.Wu, (long long)L.grid, L.status_bytes,
           L.cand_cap, L.cand_bytes);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "print")) return print_plans(argc, argv);
  sweep_select<double>();
  sweep_select<float>();
  sweep_fast_ws();
  sweep_b2();
  sweep_team();
  if (g_fail) { printf("%d of %ld checks failed\n", g_fail, g_checked); return 1; }
  printf("%ld comparisons\nok\n", g_checked);
  return 0;
}
