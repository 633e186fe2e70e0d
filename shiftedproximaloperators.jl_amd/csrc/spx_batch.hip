// spx_batch.hip -- batched separable prox! + step statistics, parameters on the device (spx_proxstep_*_batch, include/spx_batch.h).
// Built into a library of its own, libspx_batch.so, which links against libspx.so (the context, its workspace, the error text).
// The walk, the kernel body, the reduce and the host run are spx_batch_device.hpp's; here is what this call alone has: the
// vectors y, q, xk, sj, xkn (d is the constant zero), lambda[b], sigma[b], q_scale[b] (Box forms: l[b], u[b]) read by the workgroup
// that stores y, and three statistics per problem: {lambda[b] * h terms, <q, y>, <y, y>}.  Each element site is the one of
// spx_proxstep_X: the functor of the same Row::make, WithStep, sep_accumulate.
#include "spx_batch.h"
#include "spx_batch_device.hpp"

namespace {
struct ProxKind {
  static constexpr BatchKind kPlan = kBatchProx;
  static constexpr int kStages = 1;  // all 3 U loads of a full tile are issued before the first use
  static constexpr bool kHasD = false;
  template <class Row>
  using Op = WithStep<typename Row::Op, typename Row::Term>;
  // the functor's constants are formed as the host forms them
  template <class Row, bool TILED>
  static __device__ __forceinline__ Op<Row> make_op(const BatchArgs& k, int64_t b, double lam) {
    using Base = typename Row::Op;
    Op<Row> op{};
    static_cast<Base&>(op) = Row::template make<Base>(lam, k.sigma[b]);
    op.qscale = k.qscale[b];
    return op;
  }

  static constexpr const char* kLibName = "libspx_batch.so";
  static const BatchReduceKernel kReduce;
  template <class Row>
  static int refuse_params(const BatchCall& c) {
    SPX_REQUIRE(c.lambda != nullptr && c.sigma != nullptr && c.q_scale != nullptr, "a parameter array (lambda, sigma, q_scale) is NULL");
    return SPX_OK;
  }
  static int refuse_alias(const BatchCall& c) {
    SPX_REQUIRE(c.y != c.a, kSpxYAliasesQ);
    return SPX_OK;
  }
  static std::array<const void*, 4> inputs(const BatchCall& c) { return {c.y, c.a, c.xk, c.sj}; }
  template <class Row>
  static int zero_flags(const BatchCall&) { return SPX_OK; }
  template <class Row, bool TILED, bool PAIRS, bool MASK>
  static void launch(const BatchCall& c, const BatchPlan& p, double* out);
};

template <class Row, bool TILED, bool PAIRS, bool MASK>
__global__ __launch_bounds__(256) void k_sep_batch(double* y_, const double* q_, const double* xk_, const double* sj_, double* xkn_,
                                                    const double* __restrict__ lambda, const double* __restrict__ sigma,
                                                    const double* __restrict__ qscale, const double* __restrict__ lo,
                                                    const double* __restrict__ up, const uint8_t* mask, int64_t n, int64_t ld,
                                                    int64_t tiles, int base_odd, double* out) {
  batch_body<ProxKind, Row, TILED, PAIRS, MASK>({{y_, q_, nullptr, xk_, sj_, xkn_}, lambda, sigma, qscale, nullptr, lo, up, mask, nullptr, n, ld, tiles, base_odd, out});
}
__global__ __launch_bounds__(256) void k_batch_reduce(const double* partials, int64_t tiles, const double* __restrict__ lambda,
                                                       double* stats) {
  batch_reduce_body<3>(partials, tiles, lambda, stats);
}
const BatchReduceKernel ProxKind::kReduce = k_batch_reduce;
template <class Row, bool TILED, bool PAIRS, bool MASK>
void ProxKind::launch(const BatchCall& c, const BatchPlan& p, double* out) {
  hipLaunchKernelGGL((k_sep_batch<Row, TILED, PAIRS, MASK>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, c.y, c.a, c.xk,
                     c.sj, c.xkn, c.lambda, c.sigma, c.q_scale, c.l, c.u, c.mask, c.n, c.ld, p.tiles_per_problem, p.base_odd, out);
}
}  // namespace

#define SPX_PROXSTEP_BATCH(NAME, ROW, BOX_PARAMS, ...)                                                                          \
  SPX_EXPORT int NAME(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n, int64_t batch,  \
                      int64_t ld, const double* lambda, const double* sigma, BOX_PARAMS const double* q_scale, double* xkn,   \
                      double* stats_dev) {                                                                                     \
    return run_batch<ProxKind, ROW>({ctx, y, q, nullptr, xk, sj, n, batch, ld, lambda, xkn, stats_dev, sigma, q_scale, nullptr, \
                                     nullptr, __VA_ARGS__});                                                                   \
  }
SPX_PROXSTEP_BATCH(spx_proxstep_l1_batch, RowL1, , nullptr, nullptr, nullptr)
SPX_PROXSTEP_BATCH(spx_proxstep_l0_batch, RowL0, , nullptr, nullptr, nullptr)
SPX_PROXSTEP_BATCH(spx_proxstep_l1_box_batch, RowL1Box, SPX_BATCH_BOX_PARAMS, l, u, sel_mask)
SPX_PROXSTEP_BATCH(spx_proxstep_l0_box_batch, RowL0Box, SPX_BATCH_BOX_PARAMS, l, u, sel_mask)
