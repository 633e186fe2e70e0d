/* Stand-alone driver for the host helpers of csrc/spx_common.hpp that need no device: the destination of a value call
 * (spx_value_dest, spx_value_nan_on_device), the argument checks of the step entry points and their message selection (spx_step_begin),
 * and the host half of the empty call (spx_dest_empty without a device destination).  Compiled with hipcc and
 * -Xarch_host -fsanitize=address,undefined and run as a child by tests/test_result_dest_host.py; it has its own main, the
 * library is not loaded, no HIP call is made.  The four library functions the helpers reach are stubbed here. */
#include <cmath>
#include <cstring>
#include <string>

#include "spx_common.hpp"

static std::string g_msg;
static bool g_capturing = false;
static int g_zeroed = 0;
void spx_set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_msg = buf;
}
int spx_require_not_capturing(spx_ctx*, const char* what) {
  if (!g_capturing) return SPX_OK;
  spx_set_error("invalid argument: %s is not possible while the stream is being captured into a graph", what);
  return SPX_ERR_INVALID_ARG;
}
int spx_zero_async(spx_ctx*, void*, size_t) { ++g_zeroed; return SPX_OK; }
int spx_status_report(spx_ctx*) { return SPX_ERR_INTERNAL; }

static int g_fail = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_fail = 1; } \
  } while (0)
static bool refused(int rc, const char* words) { return rc == SPX_ERR_INVALID_ARG && g_msg.find(words) != std::string::npos; }

int main() {
  spx_ctx* ctx = new spx_ctx;
  double value = -1.0, target = -2.0;
  // the destination of a value call
  SpxDest d = spx_value_dest(ctx, &value);
  CHECK(d.host == &value && d.dev == nullptr && d.count == 1);
  CHECK(spx_value_dest(nullptr, &value).host == &value);
  spx_value_nan_on_device(SPX_OK, d, false, &value);
  CHECK(value == -1.0);  // a host destination: *value is the call's
  ctx->value_target = &target;
  d = spx_value_dest(ctx, &value);
  CHECK(d.host == nullptr && d.dev == &target && d.count == 1);
  value = -0.0;  // (what the entry point wrote: kept by an empty and by a failed call, sign and all)
  spx_value_nan_on_device(SPX_OK, d, true, &value);
  CHECK(value == 0.0 && std::signbit(value));
  spx_value_nan_on_device(SPX_ERR_HIP, d, false, &value);
  CHECK(value == 0.0 && std::signbit(value));
  spx_value_nan_on_device(SPX_OK, d, false, &value);
  CHECK(std::isnan(value));
  CHECK(target == -2.0);
  // the capture refusal: host destinations only, the entry point's words
  g_capturing = true;
  CHECK(spx_dest_check_capture(ctx, d, "x") == SPX_OK);
  CHECK(refused(spx_dest_check_capture(ctx, SpxDest{&value, nullptr, 1}, "returning psi(y) to the host"), "returning psi(y) to the host is not possible"));
  g_capturing = false;
  // the empty call without a device destination: zeros on the host, nothing enqueued
  double st[4] = {1.0, 2.0, 3.0, 4.0}, vec[8][4];
  CHECK(spx_dest_empty(ctx, SpxDest{st, nullptr, 3}) == SPX_OK && st[0] == 0.0 && st[1] == 0.0 && st[2] == 0.0 && st[3] == 4.0 && g_zeroed == 0);
  CHECK(spx_dest_return(ctx, SpxDest{nullptr, &target, 1}, &target, sizeof(double)) == SPX_OK);  // no host destination: no copy
  // the checks of the step entry points, in their order
  const double *y = vec[0], *q = vec[1], *dd = vec[2], *xk = vec[3], *sj = vec[4], *l = vec[5], *u = nullptr;
  const void* mask = vec[6];
  double* xkn = vec[7];
  const char* ymsg = "y aliases g or d (the sums would read an overwritten input)";
  auto begin = [&](const SpxDest& dest, bool check_d, const void* yy, const void* xx) {
    st[0] = st[1] = st[2] = st[3] = 7.0;
    g_msg.clear();
    return spx_step_begin(ctx, dest, check_d, yy, {q, dd}, ymsg, xx, {yy, q, dd, xk, sj, l, u, mask});
  };
  const SpxDest both{st, &target, 4}, dev_only{nullptr, &target, 4}, none{nullptr, nullptr, 4};
  CHECK(begin(both, true, y, xkn) == SPX_OK && st[0] == 0.0 && st[3] == 0.0 && g_msg.empty());
  CHECK(begin(dev_only, false, y, nullptr) == SPX_OK && st[0] == 7.0);
  CHECK(begin(both, false, nullptr, nullptr) == SPX_OK);  // (n == 0 with NULL vectors)
  CHECK(refused(begin(none, true, q, q), "stats and stats_dev are both NULL") && st[0] == 7.0);  // the first of several faults
  CHECK(refused(begin(dev_only, true, q, q), "check_d needs the host form"));
  CHECK(refused(begin(both, false, q, q), ymsg) && st[0] == 7.0);
  CHECK(refused(begin(both, false, dd, xkn), ymsg));
  const void* others[] = {y, q, dd, xk, sj, l, mask};
  for (const void* p : others) CHECK(refused(begin(both, false, y, p), "xkn is one of the other vectors") && st[0] == 7.0);
  g_capturing = true;
  CHECK(refused(begin(both, false, y, xkn), "returning the step statistics to the host (pass stats = NULL) is not possible") && st[0] == 7.0);
  CHECK(begin(dev_only, false, y, xkn) == SPX_OK);
  CHECK(refused(begin(both, false, y, y), "xkn is one of the other vectors"));  // an alias is reported before the capture
  delete ctx;
  if (!g_fail) printf("ok\n");
  return g_fail;
}
