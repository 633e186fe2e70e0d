// spx_common.hpp -- shared host/device helpers of libspx (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "spx.h"

#define SPX_EXPORT extern "C" __attribute__((visibility("default")))

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
struct spx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  int num_cu = 256;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  // library-owned scratch (top-r selection state, flags); grown on demand, never shrunk
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // device staging area of the host-pointer entry points (spx_host.hip); grown on demand, never shrunk
  void* stage = nullptr;
  size_t stage_bytes = 0;
  // Persistent device state of the kernels that synchronise inside one launch (grid-barrier counters, histograms that must
  // be zero on entry, exchange words, tickets): one block of kSpxSyncBytes in a fixed layout (below), allocated and zeroed
  // when the context is created, never moved and never shared with `ws` (which every operator overwrites from offset 0).
  // Null only while a context created during a stream capture has not yet run a call that needs it (spx_sync_ready).
  void* sync = nullptr;
  // The host's view of the alternating sets in `sync`: which set the next launch uses and which sets earlier launches left
  // dirty.  Describes a zero block: reset (value-initialised) whenever the block is zeroed.
  struct SyncTrack {
    int coop_parity = 0;             // spx_select.hip: a launch uses counter/histogram set `parity` and clears set `parity ^ 1`,
                                     // which the previous launch on this stream used and has finished with
    int sel_hist_next = 0;           // spx_select.hip: histogram set (0/1) the next k_sel_coop launch uses ...
    int sel_hist_dirty[2] = {0, 0};  // ... and which sets a previous launch left non-zero
    int b2_set = 0;                  // ShiftedNormL1B2: the set of partial-sum words the next launch uses (spx_b2.hip, b2_put)
    int b2_dirty_g[2] = {0, 0};      // ... and how many workgroups wrote into each set (0 = clean)
    int team_set = 0;                // spx_group_team.hip: the set of exchange words the next team launch uses (it clears the other one)
    int grp_def_set = 0;             // spx_group.hip: which of SpxSyncHeader::grp_deferred the next call uses (it clears the other one)
  } track;
  // Graph-safe mode (sticky, set the first time a call finds its stream capturing: spx_capture_check).  The kernels that
  // synchronise inside one launch keep device state between launches (barrier counters, histogram sets, exchange words) that
  // the host tracks by alternating sets -- a captured launch would replay ONE set for ever.  In graph-safe mode every such
  // launch is preceded by a memset of exactly the state it uses (a node of the same graph) and the sets are fixed.
  int graph_safe = 0;
  // spx_ctx_set_value_target: when non-NULL, the value-returning entry points (spx_obj_*, spx_proxval_*) store their
  // result in this DEVICE double and return after enqueueing, without the read-back / stream synchronisation.  Read once per
  // call, by spx_value_dest at the entry point; never written outside spx_ctx.hip
  double* value_target = nullptr;
  // tuning knobs (spx_ctx_set_tuning): per context, so that two contexts / threads never see each other's experiments
  int tune_sep_blocks_per_cu = 0;  // key 0: 0 = no cap (one tile per workgroup)
  int tune_sep_nt = 1;             // key 1: non-temporal loads / stores
  int tune_sel_fast = 1;           // key 2: sample-predicted top-r path
  int tune_sep_lds = 1;            // key 3: LDS-staged separable skeleton
  int tune_sel_spec = 1;           // key 4: single-pass (speculative store) form of the top-r fast path
  int tune_sep_xcd = 0;            // key 5: XCD-contiguous tile ranges (experiment)
  int tune_sel_small = 1;          // key 6: one-workgroup top-r for n <= 8192
  int tune_coop_cap = 0;           // key 8: pretend that only this many workgroups of an in-launch synchronised kernel are
                                   //        resident at once (0 = what the occupancy query says): exercises the smaller-grid paths
  int tune_binf_literal = 0;       // key 9: GroupNormL2Binf groups whose root sits next to the pole of step(n) (u < n/1000) take
                                   //        the reference's literal Float64 evaluation (reproduces a reference run bit pattern
                                   //        by bit pattern where the default is the more accurate side: include/spx.h)
  int tune_front_spl = 0;          // key 10: samples per lane of the top-r front kernel (1, 2, 4, 16; 0 = by n and r / n)
  int tune_sel_reg16 = 1;          // key 11: register-resident one-launch top-r at 16 elements per lane (2 Mi < n <= 4 Mi on 256 CUs)
  int tune_b2_lds = 1;             // key 12: ShiftedNormL1B2 with xk parked in LDS between the register form and the streaming form (2 Mi < n <= 4 Mi)
  int tune_team = 1;               // key 13: large contiguous groups (first of all ONE group over the whole vector) are owned by a team of
                                   //         workgroups (spx_group_team.hip); 0 = one workgroup per group as in rounds 1-3
  int tune_team_fast = 1;          // key 14: ... and the Binf form of that takes its sample-predicted two-pass path (0 = generic body: one
                                   //         streaming pass per reduction)
  int tune_team_factor = 0;        // key 16: the team form serves uniform large groups while there are fewer than this many per workgroup of its
                                   //         grid (0 = default, see group_route_general in spx_group.hip); an A/B knob
  int tune_fewer_launches = 1;     // key 17: psi(y) in one launch (the last workgroup finishes: spx_fin_ticket) and the Binf group operators without the
                                   //         zero-fill launch of their deferred list (count words that alternate); 0 = the launches of rounds 1-3
  int tune_b2_step_compose = 0;    // key 18: spx_proxstep_l1_b2 takes its composed route (the VALUE launch + one streaming launch) on every form;
                                   //         0 = fused wherever the form has a STEP kernel.  An A/B knob: y, xkn and [0] keep their bits
  int tune_force_grid = 0;         // key 100, test builds only (-DSPX_TEST_HOOKS): launch the one-launch top-r with THIS many workgroups,
                                   //          residency or not -- the planted fault behind tests/test_gpu_robustness.py
  int tune_force_team = 0;         // key 102, test builds only: the last workgroup of every team of k_group_team arrives late (spx_group_team.hip)
  int tune_force_tail = 0;         // key 101, test builds only: the same for the tail kernel of the sampled top-r pipeline (k_s2_tail)
  // Device-side status word in host-mapped pinned memory (spx_ctx.hip): a kernel that gives up waiting for the other
  // workgroups of its launch, or finds library-owned state outside its layout, stores a non-zero code here (system-scope
  // store); every entry point looks at it before it enqueues anything (SPX_ON_DEVICE) and fails with SPX_ERR_INTERNAL from
  // then on, until spx_sync has reported it.  No stream synchronisation and no read-back is involved.
  volatile int* status_host = nullptr;
  int* status_dev = nullptr;
  // Workspace blocks that a captured graph may still reference (graph_safe): never freed before the context is destroyed.
  void* retired[64] = {};
  int nretired = 0;
  // resident workgroups per CU of the in-launch synchronised kernels (hipOccupancyMaxActiveBlocksPerMultiprocessor),
  // queried once per kernel and context: spx_resident_cap
  const void* occ_fn[32] = {};
  int occ_blocks[32] = {};
  int nocc = 0;
#ifdef SPX_TEST_HOOKS  // (last, and in test builds only: the product's layout and its kSpxSharedAbi are what they were)
  int tune_ws_fill = 0;            // key 103: fill pattern of library-owned scratch (`ws` and `stage`): 0 off, 1 zero bytes, 2 the word
                                   //          0x00000001, 3 0xFF bytes.  Setting it fills both blocks as they are; from then on every block
                                   //          spx_ws_reserve or the staging allocator newly allocates is filled before the call's first launch
  int tune_ws_trace = 0;           // key 104: every spx_ws_reserve call site and the staging allocator print one line to stdout per call:
                                   //          "SPX_WS_SITE <file> <function> <line> <bytes>" (tests/test_gpu_ws_poison.py, tests/ws_sites.json)
#endif
};

// codes of spx_ctx::status_host (bits)
constexpr int kSpxStatusTimeout = 1;    // an in-launch synchronised kernel gave up waiting for its own workgroups
constexpr int kSpxStatusCorrupt = 2;    // library-owned device state outside its layout (deferred-group list)

// (SPX_SHARED: also called from libspx_batch.so, which links against this library: csrc/spx_batch.hip.  What the two share --
//  the layout of spx_ctx and these signatures -- is stamped: kSpxSharedAbi is compiled into both, libspx.so answers with its own
//  through spx_shared_abi(), and the batched entry points refuse a library that answers otherwise.  Raise the version whenever
//  spx_ctx or one of the SPX_SHARED functions changes.)
#define SPX_SHARED __attribute__((visibility("default")))
constexpr int kSpxSharedVersion = 1;
constexpr int kSpxSharedAbi = kSpxSharedVersion * 65536 + (int)sizeof(spx_ctx);
SPX_SHARED int spx_shared_abi();
SPX_SHARED void spx_set_error(const char* fmt, ...);
// the first statement of every entry point of a batch library `lib` ("libspx_batch.so", ...): the libraries share spx_ctx and four
// functions, so refuse to touch a context of a libspx.so built from other sources
#define SPX_REQUIRE_SHARED_ABI(lib)                                                                                       \
  do {                                                                                                                    \
    if (spx_shared_abi() != kSpxSharedAbi) {                                                                              \
      spx_set_error("%s and libspx.so do not match (shared layout %d, expected %d): rebuild both", lib, spx_shared_abi(), \
                    kSpxSharedAbi);                                                                                       \
      return SPX_ERR_INTERNAL;                                                                                            \
    }                                                                                                                     \
  } while (0)
SPX_SHARED int spx_ws_reserve(spx_ctx* ctx, size_t bytes);
#ifdef SPX_TEST_HOOKS
// Test builds: every call site of spx_ws_reserve names itself (key 104) before it reserves; the staging allocator (spx_host.hip)
// reports through spx_hook_trace and fills what it allocates through spx_hook_fill (key 103).  Nothing of this exists in the
// product build.
SPX_SHARED int spx_ws_reserve_at(spx_ctx* ctx, size_t bytes, const char* file, const char* func, int line);
void spx_hook_trace(const spx_ctx* ctx, const char* file, const char* func, int line, size_t bytes);
int spx_hook_fill(spx_ctx* ctx, void* ptr, size_t bytes);  // the pattern of key 103 over [ptr, ptr + bytes), by a kernel on the stream
#define spx_ws_reserve(ctx, bytes) spx_ws_reserve_at((ctx), (bytes), __FILE__, __func__, __LINE__)
#endif
// spx_ctx::sync is there unless the context was created while its stream was being captured: then the first call that needs
// it allocates it outside a capture and refuses inside one (SPX_ERR_INVALID_ARG, before anything is enqueued)
int spx_sync_alloc(spx_ctx* ctx);
static inline int spx_sync_ready(spx_ctx* ctx) { return ctx->sync ? SPX_OK : spx_sync_alloc(ctx); }
int spx_ctx_count(int device);                     // live contexts on a device
// How many workgroups of `fn` (block_threads lanes, dyn_lds bytes of dynamic LDS) can be resident at once on the context's
// device: occupancy query x number of CUs, cached per kernel; spx_ctx_set_tuning key 8 lowers it (tests).  Every launch that
// synchronises inside itself sizes its grid with this and takes a smaller-grid form when the grid it wants does not fit --
// a workgroup must never wait for one that cannot be placed.  0 with an error set if the kernel cannot run at all.
int64_t spx_resident_cap(spx_ctx* ctx, const void* fn, int block_threads, size_t dyn_lds);
int spx_blocks_per_cu(spx_ctx* ctx, const void* fn, int block_threads, size_t dyn_lds);  // workgroups a CU holds at once; -1: error
SPX_SHARED int spx_status_report(spx_ctx* ctx);    // SPX_ERR_INTERNAL + message for a non-zero device status word
// Is ctx's stream being captured into a graph?  Sets spx_ctx::graph_safe (sticky) when it is.  Calls that would have to
// synchronise the stream or (re)allocate refuse to run while capturing (SPX_ERR_INVALID_ARG, spx_require_not_capturing).
// Zero-fill on the context's stream by a KERNEL (4-byte words): used instead of hipMemsetAsync / hipMemset2DAsync wherever
// a call may be captured into a graph -- a captured iteration replayed through torch.cuda.CUDAGraph faulted in a way that
// implicated the runtime's memset nodes (round 2; plain kernel nodes replay fine).  bytes, pitch, width: multiples of 4.
SPX_SHARED int spx_zero_async(spx_ctx* ctx, void* ptr, size_t bytes);
int spx_zero2d_async(spx_ctx* ctx, void* ptr, size_t pitch_bytes, size_t width_bytes, size_t rows);
bool spx_capture_check(spx_ctx* ctx);
int spx_require_not_capturing(spx_ctx* ctx, const char* what);
// Does an in-launch synchronised launch take its graph-safe form (see spx_ctx::graph_safe)?  Switches the mode on if capturing.
static inline bool spx_graph_safe(spx_ctx* ctx) { return spx_capture_check(ctx) || ctx->graph_safe; }

// spx_group_team.hip (large contiguous groups on teams of workgroups), called from group_route_general in spx_group.hip
int spx_group_team_max_grid(spx_ctx* ctx, bool binf);
int spx_group_team_plan(spx_ctx* ctx, bool binf, const double* y, const double* q, const double* xk, const double* sj,
                        int64_t n, const int64_t* offsets, int64_t ngroups, int64_t big_min, const int** active_dev);
int spx_group_team_launch(spx_ctx* ctx, bool binf, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                          const int64_t* offsets, int64_t gsize, int64_t ngroups, const double* lambda, double sigma,
                          double delta);

// The streaming launch that the composed routes of spx_proxstep_group_* and spx_proxstep_l1_b2 end in (spx_group.hip): after a
// value call has stored y and left h in the device double *h, ONE launch stores xkn = (xk + sj) + y (xkn may be NULL) and forms
// <q, y> and <y, y>; its last workgroup stores {*h, <q, y>, <y, y>} to the device destination; a host destination reads them back.
// plan: the launch shape and the workspace it needs from offset 0 of spx_ctx::ws (reserve it before the call's first launch; the
// value call may use the same bytes, it has finished with them on the stream before the tail runs).
struct SpxStepTail {
  bool vec;       // 16-byte accesses: every vector, xkn included, is 16-byte aligned
  int64_t blocks;
  size_t bytes;
};
SpxStepTail spx_step_tail_plan(spx_ctx* ctx, const double* y, const double* q, const double* xk, const double* sj, const double* xkn,
                               int64_t n);
struct SpxDest;
int spx_step_tail_run(spx_ctx* ctx, const SpxStepTail& tail, const double* q, const double* y, const double* xk, const double* sj,
                      double* xkn, int64_t n, const double* h, const SpxDest& dest);

// Two launches that synchronise inside themselves must not run side by side on one device: each would hold CUs while it
// waits for workgroups of its own that cannot be placed.  Contexts on different streams are therefore chained through one
// event per device whenever more than one context exists on it (a stream-side dependency, the host never blocks).
// Constructed before such a launch (or a sequence that contains one), destroyed after it.  spx_ctx.hip.
struct SpxCoopLaunchGuard {
  spx_ctx* ctx;
  bool chained;
  bool capturing;
  explicit SpxCoopLaunchGuard(spx_ctx* c);
  ~SpxCoopLaunchGuard();
};

#define SPX_HIP(call)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      spx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return SPX_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)

// Entry points run on the context's device and leave the caller's current device as they found it (an array library
// working on another GPU must not have its current device changed under it).
struct SpxDeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit SpxDeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) err = hipSetDevice(device);
  }
  ~SpxDeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
#define SPX_ON_DEVICE_RAW(ctx)                  \
  SpxDeviceGuard spx_device_guard((ctx)->device); \
  SPX_HIP(spx_device_guard.err)
// ... and refuse to enqueue anything on a context whose device side has reported a failure (spx_ctx::status_host)
#define SPX_ON_DEVICE(ctx)                                                       \
  if ((ctx)->status_host != nullptr && *(ctx)->status_host != 0) return spx_status_report(ctx); \
  SPX_ON_DEVICE_RAW(ctx)

#define SPX_REQUIRE(cond, msg)                 \
  do {                                         \
    if (!(cond)) {                             \
      spx_set_error("invalid argument: %s", msg); \
      return SPX_ERR_INVALID_ARG;              \
    }                                          \
  } while (0)

#define SPX_LAUNCH_CHECK()                                                   \
  do {                                                                       \
    hipError_t e_ = hipGetLastError();                                       \
    if (e_ != hipSuccess) {                                                  \
      spx_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return SPX_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)

static inline int spx_check_common(spx_ctx* ctx, const void* y, const void* q, const void* xk,
                                   const void* sj, int64_t n) {
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(n >= 0, "n < 0");
  if (n > 0) SPX_REQUIRE(y && q && xk && sj, "NULL vector with n > 0");
  return SPX_OK;
}

static inline bool spx_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// f(std::integral_constant<int, W>{}) for the W among WS... that equals v: a runtime value (lanes per group, samples per lane,
// a flag) as a template argument.  False when v is none of them (f is not called).
template <int... WS, class F>
static inline bool spx_with_lanes(int v, F&& f) {
  return ((v == WS ? (f(std::integral_constant<int, WS>{}), true) : false) || ...);
}

// ---------------------------------------------------------------------------------------------
// Where the `count` doubles that a call returns next to y go.  Built once, at the entry point, and passed down as an argument:
// nothing below an entry point looks at spx_ctx::value_target.
// ---------------------------------------------------------------------------------------------
struct SpxDest {
  double* host;  // non-NULL: the result is read back and the stream synchronised (refused under a capture)
  double* dev;   // the caller's device doubles, or NULL
  int count;
};
// A value call (spx_obj_*, spx_proxval_*): the context's device target if it has one, else the caller's host double.
static inline SpxDest spx_value_dest(const spx_ctx* ctx, double* value) {
  double* const target = ctx ? ctx->value_target : nullptr;
  return target ? SpxDest{nullptr, target, 1} : SpxDest{value, nullptr, 1};
}
// ... whose host double is NaN when the value stays on the device.  (An empty or a failed call keeps the zero the entry point wrote.)
static inline void spx_value_nan_on_device(int rc, const SpxDest& d, bool empty, double* value) {
  if (rc == SPX_OK && d.dev != nullptr && !empty) *value = __builtin_nan("");
}
// A host destination synchronises: not under a capture.  what: the entry point's own words.
static inline int spx_dest_check_capture(spx_ctx* ctx, const SpxDest& d, const char* what) {
  return d.host ? spx_require_not_capturing(ctx, what) : SPX_OK;
}
static inline void spx_dest_zero_host(const SpxDest& d) {
  if (d.host) for (int i = 0; i < d.count; ++i) d.host[i] = 0.0;
}
// The empty call (n == 0, no group at all): zeros, on the device by a kernel rather than a memset node (spx_zero_async).
static inline int spx_dest_empty(spx_ctx* ctx, const SpxDest& d) {
  spx_dest_zero_host(d);
  if (!d.dev) return SPX_OK;
  SPX_ON_DEVICE(ctx);
  return spx_zero_async(ctx, d.dev, (size_t)d.count * sizeof(double));
}
// The return: with a host destination, `bytes` of the library's result words `words` (device memory) are copied to `into`
// (d.host unless given) and the stream is synchronised; without one nothing is read back and the call returns after enqueueing.
static inline int spx_dest_return(spx_ctx* ctx, const SpxDest& d, const void* words, size_t bytes, void* into = nullptr) {
  if (!d.host) return SPX_OK;
  SPX_HIP(hipMemcpyAsync(into ? into : d.host, words, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SPX_HIP(hipStreamSynchronize(ctx->stream));
  return SPX_OK;
}
// What every spx_proxstep_* / spx_iproxstep_* entry point checks before it enqueues anything, in this order: a destination at
// all; check_d only with a host destination; y none of `inputs` (the sums read them after y is stored; y_msg names them); xkn
// none of `others`; no host destination under a capture.  Then the host destination is zeroed.
// (Others: a braced list, or SepCall::others() below)
template <class Others = std::initializer_list<const void*>>
static inline int spx_step_begin(spx_ctx* ctx, const SpxDest& d, bool check_d, const void* y,
                                 std::initializer_list<const void*> inputs, const char* y_msg, const void* xkn,
                                 const Others& others) {
  SPX_REQUIRE(d.host != nullptr || d.dev != nullptr, "stats and stats_dev are both NULL");
  SPX_REQUIRE(!check_d || d.host != nullptr, "check_d needs the host form of the statistics (stats != NULL): it synchronises");
  for (const void* p : inputs) SPX_REQUIRE(y == nullptr || y != p, y_msg);
  if (xkn != nullptr)
    for (const void* p : others) SPX_REQUIRE(xkn != p, "xkn is one of the other vectors");
  const int rc = spx_dest_check_capture(ctx, d, "returning the step statistics to the host (pass stats = NULL)");
  if (rc) return rc;
  spx_dest_zero_host(d);
  return SPX_OK;
}
constexpr const char* kSpxYAliasesQ = "y aliases q (<q, y> of an overwritten q)";
// The contiguous-group objective h(xk + sj + y) with its destination as an argument (spx_objective.hip): what spx_obj_group_l2
// runs, and what the composed routes of spx_proxval_group_* / spx_proxstep_group_* end in.
int spx_obj_group_l2_to(spx_ctx* ctx, const double* y, const double* xk, const double* sj, int64_t n, const int64_t* group_offsets,
                        int64_t group_size, int64_t ngroups, const double* lambda_vec, const SpxDest& dest);

// ---------------------------------------------------------------------------------------------
// The operands of a separable call (spx_separable.hip; the Box tail also in spx_objective.hip), built once, at the entry point,
// and passed down by reference: only a kernel launch spells the fields out, in the kernel's parameter order.
// ---------------------------------------------------------------------------------------------
// The Box tail: the bounds as vectors (NULL: the scalar) and the selection mask (NULL: every index).  Value-initialised: no box.
template <class T>
struct SpxBox {
  const T *l, *u;
  T ls, us;
  const uint8_t* mask;
};
// q holds g in the iprox forms; d and xkn are NULL where the call has none.  Each member below states the vectors of a call once.
template <class T>
struct SepCall {
  spx_ctx* ctx;
  T* y;
  const T *q, *d, *xk, *sj;
  int64_t n;
  SpxBox<T> box;
  T* xkn;

  // the same call `head` elements further on (the mask: bytes); a NULL stays NULL
  SepCall shifted(int64_t head) const {
    auto sh = [head](auto* p) { return p ? p + head : p; };
    return {ctx, sh(y), sh(q), sh(d), sh(xk), sh(sj), n, {sh(box.l), sh(box.u), box.ls, box.us, sh(box.mask)}, sh(xkn)};
  }
  // Float64 vector skeletons: is every vector 16-byte aligned at element h, and the mask 2-byte aligned there?
  bool aligned16_at(int64_t h) const {
    auto a16 = [h](const T* p) { return !p || spx_aligned16(p + h); };
    return a16(y) && a16(q) && a16(d) && a16(xk) && a16(sj) && a16(box.l) && a16(box.u) && a16(xkn) &&
           (!box.mask || ((reinterpret_cast<uintptr_t>(box.mask) + (uintptr_t)h) & 1u) == 0);
  }
  // Float32 vector skeleton: do y, q, xk, sj, d and -- for a Box operator -- l and u start equally far, a whole number of
  // elements, from a 16-byte boundary?  (The mask is read by bytes; there is no Float32 form with xkn.)
  bool same_misalignment(bool bounds_count) const {
    auto mis = [](const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u); };
    const unsigned m = mis(y);
    auto eq = [&](const T* p) { return !p || mis(p) == m; };
    return m % 4 == 0 && mis(q) == m && mis(xk) == m && mis(sj) == m && eq(d) && (!bounds_count || (eq(box.l) && eq(box.u)));
  }
  // what xkn must be none of (spx_step_begin)
  std::array<const void*, 8> others() const { return {{y, q, d, xk, sj, box.l, box.u, box.mask}}; }
};
template <class T>
static inline int spx_check_common(const SepCall<T>& c) { return spx_check_common(c.ctx, c.y, c.q, c.xk, c.sj, c.n); }

// ---------------------------------------------------------------------------------------------
// device math with the reference's (Julia Base) semantics
// ---------------------------------------------------------------------------------------------
typedef double f64x2 __attribute__((ext_vector_type(2)));

// Base.min / Base.max on Float64: the sign of x - y picks the argument, so -0.0 < +0.0;
// a NaN in either argument propagates (IEEE-754-2019 minimum / maximum).
__device__ __forceinline__ double jl_min(double x, double y) {
  double d = x - y;
  double a = (__double_as_longlong(d) < 0) ? x : y;
  return (x != x || y != y) ? d : a;
}
__device__ __forceinline__ double jl_max(double x, double y) {
  double d = x - y;
  double a = (__double_as_longlong(d) < 0) ? y : x;
  return (x != x || y != y) ? d : a;
}
// the same on Float32 (overloads in the SAME scope as the Float64 forms: a float overload declared in an inner namespace would
// hide these and silently round every double argument to float)
__device__ __forceinline__ float jl_min(float x, float y) {
  const float d = x - y;
  const float a = (__float_as_int(d) < 0) ? x : y;
  return (x != x || y != y) ? d : a;
}
__device__ __forceinline__ float jl_max(float x, float y) {
  const float d = x - y;
  const float a = (__float_as_int(d) < 0) ? y : x;
  return (x != x || y != y) ? d : a;
}
// Base.sign: +-1.0, or x itself for +-0.0 / NaN
__device__ __forceinline__ double jl_sign(double x) { return (x > 0.0) ? 1.0 : (x < 0.0) ? -1.0 : x; }
// prox_zero(q, l, u) = min(max(q, l), u)   src/ShiftedProximalOperators.jl:203
template <class T>
__device__ __forceinline__ T prox_zero(T q, T l, T u) { return jl_min(jl_max(q, l), u); }

namespace {
// element terms of h (the objectives, spx_objective.hip, and the prox! fused with its value, spx_separable.hip)
// (float overloads: the Float32 forms.  The reference forms xsy and every term in Float32 -- which entries are exactly zero,
//  the rounding of each square root -- and adds them up in Float32; here the terms are Float32 values, the SUM is Float64.)
struct TermL1 {  // NormL1 [ext]
  __device__ __forceinline__ double operator()(double v) const { return fabs(v); }
  __device__ __forceinline__ double operator()(float v) const { return (double)fabsf(v); }
};
struct TermL0 {  // NormL0, IndBallL0 [ext]
  __device__ __forceinline__ double operator()(double v) const { return (v != 0.0) ? 1.0 : 0.0; }
  __device__ __forceinline__ double operator()(float v) const { return (v != 0.0f) ? 1.0 : 0.0; }
};
struct TermLhalf {  // src/rootNormLhalf.jl:27-29
  __device__ __forceinline__ double operator()(double v) const { return sqrt(fabs(v)); }
  __device__ __forceinline__ double operator()(float v) const { return (double)__builtin_sqrtf(fabsf(v)); }
};
}  // namespace

// sum over the 64 lanes of a wavefront, result in every lane (xor butterfly; DPP/permute lowered by hipcc)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// A double moved between lanes by DPP (row operations: quad_perm, row_half_mirror, row_mirror -- inside a 16-lane row)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// sum / max over the 64 lanes of a wavefront, result in every lane: DPP inside the 16-lane rows, two permutes across them
// (the xor butterfly of wave_sum is six permutes per double: the reductions of a root find are latency, not bandwidth)
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ double wave_max_dpp(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  v = fmax(v, dpp_f64<0x140>(v));
  v = fmax(v, __shfl_xor(v, 16, 64));
  v = fmax(v, __shfl_xor(v, 32, 64));
  return v;
}
// sum over the 16 lanes of a row, result in every lane of the row (a fixed shape: the same bits in every row that holds the same 16 values)
__device__ __forceinline__ double fold16_sum(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  return v;
}

// The layout of spx_ctx::sync, one block of kSpxSyncBytes per context (zero-filled when the context is created, and by
// spx_sync after a timeout; spx_ctx::track is reset with it):
//   [0, 2 MiB)          spx_select.hip: SelSync, whose head is the SpxSyncHeader below (spx_sync_header)
//   [2 MiB, 4 MiB)      spx_b2.hip: two sets of partial-sum words (spx_sync_b2)
//   [4 MiB, 4.5 MiB + 4 KiB)  spx_group_team.hip: two sets of exchange words, two sets of tile counters (spx_sync_team)
constexpr size_t kSpxSyncSelBytes = (size_t)2 << 20;  // >= sizeof(SelSync) (static_assert in spx_select.hip)
constexpr size_t kSpxSyncB2Offset = kSpxSyncSelBytes;
constexpr size_t kSpxSyncB2Bytes = (size_t)2 << 20;   // (static_assert in spx_b2.hip)
constexpr size_t kSpxSyncTeamOffset = kSpxSyncB2Offset + kSpxSyncB2Bytes;
constexpr size_t kSpxSyncTeamBytes = ((size_t)512 << 10) + 4096;  // (static_assert in spx_group_common.hpp)
constexpr size_t kSpxSyncBytes = kSpxSyncTeamOffset + kSpxSyncTeamBytes;

// Head of spx_ctx::sync, shared by every kernel that synchronises inside one launch.
constexpr int kSpxBarSplit = 8;  // arrival counters per grid barrier (see spx_grid_rendezvous)
struct SpxSyncHeader {
  unsigned int bar[2][kSpxBarSplit * 32];  // grid-barrier counters, kSpxBarSplit 128-byte lines per set: a launch uses [parity] and clears [parity ^ 1]
  int b2_last_scaled;       // ShiftedNormL1B2: did the previous call on this context find the trust region active?
  int timed_out;            // sticky: a workgroup gave up waiting for the others (kSpxPollLimit); no workgroup waits any more
  int* status;              // device view of spx_ctx::status_host (host-mapped): the failure is reported by the NEXT libspx call
  // Round 4 (launch counts at solver sizes: a call below ~1e6 elements costs what its launches cost):
  long long grp_deferred[2];  // count words of the Binf group operators' deferred list: a call uses [set] and clears [set ^ 1] (spx_group.hip)
  unsigned int fin_top;       // the objective kernels' "last workgroup" tickets (spx_fin_ticket below); zero between launches
  int fin_flag;               // ... and their infeasibility bits; zero between launches
  double b2_value;            // spx_proxval_l1_b2 without a device value target: the launch stores h here, the host reads it back
  double grp_step_h;          // spx_proxstep_group_*, composed routes: the device destination of the value part, picked up by the tail launch (spx_group.hip)
  double b2_step[3];          // spx_proxstep_l1_b2 with a host result: the launch stores {h, <q, y>, <y, y>} here, the host reads them back
                              // (composed route: [0] is the device destination of the value part, picked up by the tail launch)
  int pad[12];
  unsigned int fin_class[kSpxBarSplit * 32];  // first-level tickets, one 128-byte line each
};
static_assert(sizeof(SpxSyncHeader) == 2 * kSpxBarSplit * 32 * 4 + 128 + kSpxBarSplit * 32 * 4, "SpxSyncHeader layout");
static inline SpxSyncHeader* spx_sync_header(spx_ctx* ctx) { return static_cast<SpxSyncHeader*>(ctx->sync); }
static inline unsigned long long* spx_sync_b2(spx_ctx* ctx) {
  return reinterpret_cast<unsigned long long*>(static_cast<char*>(ctx->sync) + kSpxSyncB2Offset);
}
static inline unsigned long long* spx_sync_team(spx_ctx* ctx) {
  return reinterpret_cast<unsigned long long*>(static_cast<char*>(ctx->sync) + kSpxSyncTeamOffset);
}

// Every wait of one workgroup for others is bounded: kSpxPollLimit polls (each a memory round trip plus a short sleep: a few
// seconds in all, against microseconds of legitimate waiting).  A workgroup that gives up sets SpxSyncHeader::timed_out,
// after which no workgroup of that context waits any more -- the grid drains instead of hanging the device, the kernels
// that store a result store NaN (spx_poisoned) -- and raises the context's host-mapped status word, which makes the next
// libspx call on the context (any entry point, not only spx_sync) fail with SPX_ERR_INTERNAL.  It happens when the
// workgroups of the launch are not all resident (a grid of another process or of a graph replay holding the CUs: the
// in-process cases are excluded by spx_resident_cap and SpxCoopLaunchGuard), when the synchronisation state is corrupt (a
// context shared by two threads, device memory overwritten) -- or in tools/planted_faults.sh.
#ifndef SPX_POLL_LIMIT_LOG2
#define SPX_POLL_LIMIT_LOG2 22
#endif
constexpr unsigned int kSpxPollLimit = 1u << SPX_POLL_LIMIT_LOG2;
__device__ __forceinline__ void spx_raise_status(int* status, int code) {
  if (status != nullptr) __hip_atomic_store(status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ bool spx_wait_expired(unsigned int& spins, SpxSyncHeader* hdr) {
  if (++spins < 64u) return false;                       // (cheap path: the flag is not even read for short waits)
  if ((spins & 63u) != 0u && spins < kSpxPollLimit) return false;
  if (spins >= kSpxPollLimit) {
    __hip_atomic_store(&hdr->timed_out, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    spx_raise_status(hdr->status, kSpxStatusTimeout);
    return true;
  }
  return __hip_atomic_load(&hdr->timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}
// Has any workgroup of this context given up?  Asked once, before the result of an in-launch synchronised kernel is stored.
__device__ __forceinline__ bool spx_poisoned(SpxSyncHeader* hdr) {
  return __hip_atomic_load(&hdr->timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// ---------------------------------------------------------------------------------------------
// Grid barrier for kernels whose workgroups are all resident (grid <= number of CUs, one workgroup per CU): monotonic
// counters in spx_ctx::sync.  Recipe of MI355X_MICROARCH.md ("inter-workgroup visibility"): every storing wave drains its
// stores, workgroup barrier, wave 0: agent-scope release (L2 write-back) -> arrive (agent-scope atomic add) -> relaxed polls
// -> agent-scope acquire (L1 / non-coherent L2 lines invalidated), workgroup barrier, then plain loads.
// `target` = (number of barriers passed so far in this launch + 1) * gridDim.x.  Every workgroup of the grid must call
// it the same number of times (the exit condition every wave reaches: no early return between barriers).
// Arrivals are spread over kSpxBarSplit counters (workgroup b adds to counter b % 8, each on its own 128-byte line) and
// lanes 0..7 of wave 0 poll one counter each: atomics on ONE address retire ~12 ns apart and the polls of 256 workgroups
// queue in front of the last arrivals -- measured without fences (tools/exp/grid_barrier.hip): 3.75 -> 1.44 us per
// rendezvous with 256 workgroups, 2.0 -> 1.2 with 128, 1.3 -> 1.1 with 64 (16 counters: 2.2 / 1.2 / 1.1; a two-level tree 2.4).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void spx_bar_arrive_and_wait(unsigned int* counters, unsigned int target, SpxSyncHeader* hdr) {
  // (wave 0, all 64 lanes)
  const unsigned int lane = threadIdx.x;
  const unsigned int phase = target / gridDim.x;
  if (lane == 0) __hip_atomic_fetch_add(&counters[32u * (blockIdx.x % (unsigned)kSpxBarSplit)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // counter j hears from the workgroups j, j + 8, ...
  const unsigned int want = (lane < (unsigned)kSpxBarSplit && lane < gridDim.x)
                                ? ((gridDim.x - lane + (unsigned)kSpxBarSplit - 1u) / (unsigned)kSpxBarSplit) * phase : 0u;
  unsigned int spins = 0;
  while (true) {
    const unsigned int have = lane < (unsigned)kSpxBarSplit ? __hip_atomic_load(&counters[32u * lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    if (__ballot(have < want) == 0ull) break;
    if (spx_wait_expired(spins, hdr)) break;  // (the same in every lane)
    __builtin_amdgcn_s_sleep(1);
  }
}
// The counters of the set a LATER launch will use are cleared by workgroup 0 of this one.
__device__ __forceinline__ void spx_bar_reset(unsigned int* counters) {
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)kSpxBarSplit) counters[32u * threadIdx.x] = 0u;
}
__device__ __forceinline__ void spx_grid_barrier(unsigned int* counters, unsigned int target, SpxSyncHeader* hdr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x < 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    spx_bar_arrive_and_wait(counters, target, hdr);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

// The same rendezvous WITHOUT cache maintenance, for kernels whose workgroups exchange nothing but words written and read
// with agent-scope atomics (spx_atomic_store_f64 / spx_atomic_load_f64 below: `sc1` accesses that bypass the non-coherent
// caches).  The release / acquire fences are most of a barrier's cost when few workgroups meet (3.5 of ~4 us).
// Every wave must have waited for its own atomic stores (s_waitcnt vmcnt(0)) before it calls this.
__device__ __forceinline__ void spx_grid_rendezvous(unsigned int* counters, unsigned int target, SpxSyncHeader* hdr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's atomic stores have left
  __syncthreads();
  if (threadIdx.x < 64) spx_bar_arrive_and_wait(counters, target, hdr);
  __syncthreads();
}
__device__ __forceinline__ void spx_atomic_store_f64(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double spx_atomic_load_f64(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
}

// "Am I the last workgroup of this launch?" -- for kernels that end in a small serial step (the ordered sum of the workgroups'
// partial results) which used to be a launch of its own.  Called by ONE lane per workgroup, after that lane has waited for the
// agent-scope atomic stores of everything the last workgroup will read (s_waitcnt vmcnt(0)); the workgroup that gets `true`
// reads those words with agent-scope atomic loads.  Two levels: workgroup b takes a ticket on counter b % 8 (a 128-byte line
// each: returning atomics on ONE address retire ~12 ns apart, 2048 workgroups ending together would queue for 25 us), the last
// of a class takes one on the top counter.  Every counter is reset by the lane that takes its last ticket, so the words are
// zero between launches -- nothing to clear in front of a launch, nothing that alternates: the same node replays in a graph.
__device__ __forceinline__ bool spx_fin_ticket(SpxSyncHeader* hdr) {
  const unsigned int grid = gridDim.x, j = blockIdx.x % (unsigned)kSpxBarSplit;
  const unsigned int want = (grid - j + (unsigned)kSpxBarSplit - 1u) / (unsigned)kSpxBarSplit;  // workgroups j, j + 8, ...
  const unsigned int c = __hip_atomic_fetch_add(&hdr->fin_class[32u * j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c + 1u != want) return false;
  __hip_atomic_store(&hdr->fin_class[32u * j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned int classes = grid < (unsigned)kSpxBarSplit ? grid : (unsigned)kSpxBarSplit;
  const unsigned int t = __hip_atomic_fetch_add(&hdr->fin_top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t + 1u != classes) return false;
  __hip_atomic_store(&hdr->fin_top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}
