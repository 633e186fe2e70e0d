// spx_lhalf_batch.hip -- batched RootNormLhalf(Box) prox! + step statistics, parameters on the device
// (spx_proxstep_lhalf[_box]_batch, spx_lhalf_threshold_batch: include/spx_lhalf_batch.h).  Built into a library of its own,
// libspx_lhalf_batch.so, which links against libspx.so (the context, its workspace, the error text).  The walk, the kernel body,
// the reduce and the host run are spx_batch_device.hpp's, the plan is kBatchProx: what spx_batch.hip has for NormL1 / NormL0.
// Here is what this call alone has: the two rows whose functor constants are formed ON THE DEVICE (RowLhalf::make and
// RowLhalfBox::make of spx_sep_device.hpp are host functions; that header is left as it is).
//   LhalfBox: sigma lambda / 4, lambda, 0.5 / sigma -- products and one IEEE division, the host's bits (-ffp-contract=off).
//   Lhalf:    sigma lambda / 4 and the threshold p, which the host forms with glibc's pow: lhalf_threshold
//             (spx_lhalf_threshold.hpp) reproduces the host's expression to within 4 ulps, and spx_lhalf_threshold_batch stores
//             the very value the kernel compares with.
#include "spx_lhalf_batch.h"
#include "spx_batch_device.hpp"
#include "spx_lhalf_threshold.hpp"

#ifndef SPX_LHALF_BATCH_STAGES
#define SPX_LHALF_BATCH_STAGES 1  // 1, 2, 3 or 6 (A/B builds: profiles/lhalf_proxstep_batch_kres.txt)
#endif

namespace {
struct BatchRowLhalf {
  using Op = OpLhalf; using Term = HTermLhalf;
  template <class O> __device__ static O make(double lambda, double sigma) {
    const double nl = sigma * lambda;
    return O{nl / 4, lhalf_threshold(nl)};  // the one call of lhalf_threshold: the kernels and the threshold call come here
  }
};
struct BatchRowLhalfBox {
  using Op = OpLhalfBox; using Term = HTermLhalf;
  template <class O> __device__ static O make(double lambda, double sigma) { return O{sigma * lambda / 4, lambda, 0.5 / sigma}; }
};

struct LhalfKind {
  static constexpr BatchKind kPlan = kBatchProx;
  static constexpr int kStages = SPX_LHALF_BATCH_STAGES;
  static constexpr bool kHasD = false;
  template <class Row>
  using Op = WithStep<typename Row::Op, typename Row::Term>;
  // once per workgroup, before the walk: what the threshold needs is not live in the loop
  template <class Row, bool TILED>
  static __device__ __forceinline__ Op<Row> make_op(const BatchArgs& k, int64_t b, double lam) {
    using Base = typename Row::Op;
    Op<Row> op{};
    static_cast<Base&>(op) = Row::template make<Base>(lam, k.sigma[b]);
    op.qscale = k.qscale[b];
    return op;
  }

  static constexpr const char* kLibName = "libspx_lhalf_batch.so";
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
__global__ __launch_bounds__(256) void k_lhalf_batch(double* y_, const double* q_, const double* xk_, const double* sj_, double* xkn_,
                                                      const double* __restrict__ lambda, const double* __restrict__ sigma,
                                                      const double* __restrict__ qscale, const double* __restrict__ lo,
                                                      const double* __restrict__ up, const uint8_t* mask, int64_t n, int64_t ld,
                                                      int64_t tiles, int base_odd, double* out) {
  batch_body<LhalfKind, Row, TILED, PAIRS, MASK>({{y_, q_, nullptr, xk_, sj_, xkn_}, lambda, sigma, qscale, nullptr, lo, up, mask, nullptr, n, ld, tiles, base_odd, out});
}
__global__ __launch_bounds__(256) void k_lhalf_batch_reduce(const double* partials, int64_t tiles, const double* __restrict__ lambda,
                                                             double* stats) {
  batch_reduce_body<3>(partials, tiles, lambda, stats);
}
// p_dev[b]: the threshold of problem b as k_lhalf_batch<BatchRowLhalf, ...> forms it.  Grid: ceil(batch / 256).
__global__ __launch_bounds__(256) void k_lhalf_threshold_batch(const double* __restrict__ lambda, const double* __restrict__ sigma,
                                                                int64_t batch, double* p_dev) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < batch) p_dev[b] = BatchRowLhalf::make<OpLhalf>(lambda[b], sigma[b]).p;
}
const BatchReduceKernel LhalfKind::kReduce = k_lhalf_batch_reduce;
template <class Row, bool TILED, bool PAIRS, bool MASK>
void LhalfKind::launch(const BatchCall& c, const BatchPlan& p, double* out) {
  hipLaunchKernelGGL((k_lhalf_batch<Row, TILED, PAIRS, MASK>), dim3((unsigned)p.grid), dim3(256), 0, c.ctx->stream, c.y, c.a, c.xk,
                     c.sj, c.xkn, c.lambda, c.sigma, c.q_scale, c.l, c.u, c.mask, c.n, c.ld, p.tiles_per_problem, p.base_odd, out);
}
}  // namespace

SPX_EXPORT int spx_proxstep_lhalf_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                        int64_t batch, int64_t ld, const double* lambda, const double* sigma, const double* q_scale,
                                        double* xkn, double* stats_dev) {
  return run_batch<LhalfKind, BatchRowLhalf>({ctx, y, q, nullptr, xk, sj, n, batch, ld, lambda, xkn, stats_dev, sigma, q_scale, nullptr,
                                              nullptr, nullptr, nullptr, nullptr});
}
SPX_EXPORT int spx_proxstep_lhalf_box_batch(spx_ctx* ctx, double* y, const double* q, const double* xk, const double* sj, int64_t n,
                                            int64_t batch, int64_t ld, const double* lambda, const double* sigma,
                                            SPX_BATCH_BOX_PARAMS const double* q_scale, double* xkn, double* stats_dev) {
  return run_batch<LhalfKind, BatchRowLhalfBox>({ctx, y, q, nullptr, xk, sj, n, batch, ld, lambda, xkn, stats_dev, sigma, q_scale,
                                                 nullptr, nullptr, l, u, sel_mask});
}
SPX_EXPORT int spx_lhalf_threshold_batch(spx_ctx* ctx, const double* lambda, const double* sigma, int64_t batch, double* p_dev) {
  SPX_REQUIRE_SHARED_ABI(LhalfKind::kLibName);
  SPX_REQUIRE(ctx != nullptr, "ctx is NULL");
  SPX_REQUIRE(batch >= 0, "batch < 0");
  if (batch == 0) return SPX_OK;
  SPX_REQUIRE(lambda != nullptr && sigma != nullptr, "a parameter array (lambda, sigma) is NULL");
  SPX_REQUIRE(p_dev != nullptr, "p_dev is NULL");
  const int64_t grid = (batch + 255) / 256;
  SPX_REQUIRE(grid <= 2147483647, "the call needs more than 2^31 - 1 workgroups");
  SPX_ON_DEVICE(ctx);
  hipLaunchKernelGGL(k_lhalf_threshold_batch, dim3((unsigned)grid), dim3(256), 0, ctx->stream, lambda, sigma, batch, p_dev);
  SPX_LAUNCH_CHECK();
  return SPX_OK;
}
