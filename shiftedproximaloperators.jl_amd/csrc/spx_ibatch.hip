// spx_ibatch.hip -- batched iprox! + step statistics, parameters on the device (spx_iproxstep_*_batch, include/spx_ibatch.h).
// Built into a library of its own, libspx_ibatch.so, which links against libspx.so (the context, its workspace, the error text).
// The walk, the kernel body, the reduce and the host run are spx_batch_device.hpp's; here is what this call alone has: the
// vectors y, g, d, xk, sj, xkn, lambda[b] (Box forms: l[b], u[b]) and d_shift[b] read by the workgroup that stores y, and four
// statistics per problem: {lambda[b] * h terms, <g, y>, <deff .* y, y>, <y, y>}.  Each element site is the one of spx_iproxstep_X
// (the functor of the same row of the operator table, WithIstep, sep_accumulate) at deff = d[i] + d_shift[b] -- one rounded
// add (the library is built without contraction) -- or at d[i] itself when d_shift is NULL.
// The unboxed forms' functors raise the problem's d_flag word with agent-scope atomics.  Row form: the workgroup that owns the
// problem clears the word first (one lane, an agent-scope store, then a barrier).  Tiled form: the words are cleared by the
// zeroing kernel in front of the launch.
#include "spx_ibatch.h"
#include "spx_batch_device.hpp"

namespace {
struct IproxKind {
  static constexpr BatchKind kPlan = kBatchIprox;
  static constexpr int kStages = 2;  // four input vectors: a full tile's loads are staged in two halves
  static constexpr bool kHasD = true;
  template <class Row>
  using Op = WithIstep<typename Row::Op, typename Row::Term>;
  template <class Row, bool TILED>
  static __device__ __forceinline__ Op<Row> make_op(const BatchArgs& k, int64_t b, double lam) {
    Op<Row> op{};
    op.lambda = lam;
    if constexpr (Row::kFlagged) {
      op.flag = k.dflag + b;
      if constexpr (!TILED) {  // the row's owner clears the word before the row's first element site
        if (threadIdx.x == 0) __hip_atomic_store(op.flag, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
      }
    }
    return op;
  }

  static constexpr const char* kLibName = "libspx_ibatch.so";
  static const BatchReduceKernel kReduce;
  template <class Row>
  static int refuse_params(const BatchCall& c) {
    static_assert(Row::kFlagged == !Row::Op::kBox, "the unboxed forms carry the d > 0 flag");
    SPX_REQUIRE(c.lambda != nullptr, "lambda is NULL");
    if constexpr (Row::kFlagged) SPX_REQUIRE(c.d_flag != nullptr, "d_flag is NULL");
    return SPX_OK;
  }
  static int refuse_alias(const BatchCall& c) {
    SPX_REQUIRE(c.y != c.a && c.y != c.d, "y aliases g or d (the sums would read an overwritten input)");
    return SPX_OK;
  }
  static std::array<const void*, 5> inputs(const BatchCall& c) { return {c.y, c.a, c.d, c.xk, c.sj}; }
  template <class Row>
  static int zero_flags(const BatchCall& c) {
    if constexpr (Row::kFlagged) return spx_zero_async(c.ctx, c.d_flag, (size_t)c.batch * sizeof(int32_t));
    else return SPX_OK;
  }
  template <class Row, bool TILED, bool PAIRS, bool MASK>
  static void launch(const BatchCall& c, const BatchPlan& p, double* out);
};

// dshift: NULL = d as it is.  dflag: the unboxed forms' words, one per problem (NULL for the Box forms).
template <class Row, bool TILED, bool PAIRS, bool MASK>
__global__ __launch_bounds__(256) void k_isep_batch(double* y_, const double* g_, const double* d_, const double* xk_,
                                                     const double* sj_, double* xkn_, const double* __restrict__ lambda,
                                                     const double* __restrict__ dshift, const double* __restrict__ lo,
                                                     const double* __restrict__ up, const uint8_t* mask, int* dflag, int64_t n,
                                                     int64_t ld, int64_t tiles, int base_odd, double* out) {
  batch_body<IproxKind, Row, TILED, PAIRS, MASK>({{y_, g_, d_, xk_, sj_, xkn_}, lambda, nullptr, nullptr, dshift, lo, up, mask, dflag, n, ld, tiles, base_odd, out});
}
__global__ __launch_bounds__(256) void k_ibatch_reduce(const double* partials, int64_t tiles, const double* __restrict__ lambda,
                                                        double* stats) {
  batch_reduce_body<4>(partials, tiles, lambda, stats);
}
const BatchReduceKernel IproxKind::kReduce = k_ibatch_reduce;
template <class Row, bool TILED, bool PAIRS, bool MASK>
void IproxKind::launch(const BatchCall& c, const BatchPlan& p, double* out) {
  hipLaunchKernelGGL((k_isep_batch<Row, TILED, PAIRS, MASK>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, c.y, c.a, c.d,
                     c.xk, c.sj, c.xkn, c.lambda, c.d_shift, c.l, c.u, c.mask, c.d_flag, c.n, c.ld, p.tiles_per_problem, p.base_odd,
                     out);
}
}  // namespace

// MID: what stands between d_shift and xkn -- d_flag (unboxed) or l, u, sel_mask (Box)
#define SPX_IBATCH_FLAG_PARAM int32_t *d_flag,
#define SPX_IPROXSTEP_BATCH(NAME, ROW, MID, ...)                                                                                \
  SPX_EXPORT int NAME(spx_ctx* ctx, double* y, const double* g, const double* d, const double* xk, const double* sj, int64_t n, \
                      int64_t batch, int64_t ld, const double* lambda, const double* d_shift, MID double* xkn,                 \
                      double* stats_dev) {                                                                                      \
    return run_batch<IproxKind, ROW>({ctx, y, g, d, xk, sj, n, batch, ld, lambda, xkn, stats_dev, nullptr, nullptr, d_shift,    \
                                      __VA_ARGS__});                                                                            \
  }
SPX_IPROXSTEP_BATCH(spx_iproxstep_l1_batch, RowIproxL1, SPX_IBATCH_FLAG_PARAM, d_flag)
SPX_IPROXSTEP_BATCH(spx_iproxstep_l0_batch, RowIproxL0, SPX_IBATCH_FLAG_PARAM, d_flag)
SPX_IPROXSTEP_BATCH(spx_iproxstep_l1_box_batch, RowIproxL1Box, SPX_BATCH_BOX_PARAMS, nullptr, l, u, sel_mask)
SPX_IPROXSTEP_BATCH(spx_iproxstep_l0_box_batch, RowIproxL0Box, SPX_BATCH_BOX_PARAMS, nullptr, l, u, sel_mask)
