/* Stand-alone driver for the device-free members of SepCall (csrc/spx_common.hpp): shifted, aligned16_at, same_misalignment and
 * others.  Each is compared with the hand-written enumeration of "every vector of the call" that it replaced in
 * spx_separable.hip, restated here word for word: the Float64 alignment predicate and head shifts of run_separable, the Float32
 * misalignment test and head shifts of run_f32, the `others` lists of run_proxstep and run_iproxstep.  Over every NULL /
 * non-NULL pattern of {d, l, u, mask, xkn}, every vector at byte offsets 0 and 8 (Float64; the mask also at 1) or 0, 4, 8, 12
 * (Float32), head 0 and 1 (Float64) or 0..3 (Float32).  The pointers are integers and are never dereferenced.
 * Compiled with hipcc and -Xarch_host -fsanitize=address,undefined and run as a child by tests/test_sep_call_host.py; it has
 * its own main, the library is not loaded, no HIP call is made. */
#include <vector>

#include "spx_common.hpp"

static long g_checked = 0;
static int g_fail = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++g_checked;                                                                               \
    if (!(cond)) { if (g_fail < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

// vector i of a call at byte offset `off` of its own 4 KiB page; state 0 of an optional vector: NULL
template <class P>
static P at(int i, int off) { return reinterpret_cast<P>((uintptr_t)0x100000 + (uintptr_t)0x1000 * i + (uintptr_t)off); }
template <class P>
static P opt(int i, const int* offs, int state) { return state == 0 ? nullptr : at<P>(i, offs[state - 1]); }

static std::vector<const void*> non_null(std::initializer_list<const void*> l) {
  std::vector<const void*> v;
  for (const void* p : l) if (p) v.push_back(p);
  return v;
}

static void check_f64(double* y, const double* q, const double* d, const double* xk, const double* sj, const double* l,
                      const double* u, const uint8_t* mask, double* xkn) {
  const double ls = -1.5, us = 2.5;
  const SepCall<double> c{nullptr, y, q, d, xk, sj, 1000, {l, u, ls, us, mask}, xkn};
  // run_separable, as it was
  auto vec_ok_at = [&](int64_t h) {
    auto a16 = [&](const double* p) { return !p || spx_aligned16(p + h); };
    return a16(y) && a16(q) && a16(xk) && a16(sj) && a16(d) && a16(l) && a16(u) && a16(xkn) &&
           (!mask || ((reinterpret_cast<uintptr_t>(mask) + (uintptr_t)h) & 1u) == 0);
  };
  for (int64_t head = 0; head < 2; ++head) {
    CHECK(c.aligned16_at(head) == vec_ok_at(head));
    auto sh = [&](const double* p) { return p ? p + head : p; };
    double* yv = y + head;
    const double *qv = sh(q), *dv = sh(d), *xv = sh(xk), *sv = sh(sj), *lv = sh(l), *uv = sh(u);
    const uint8_t* mv = mask ? mask + head : mask;
    double* xn = xkn ? xkn + head : nullptr;
    const SepCall<double> v = c.shifted(head);
    CHECK(v.y == yv && v.q == qv && v.d == dv && v.xk == xv && v.sj == sv && v.box.l == lv && v.box.u == uv && v.box.mask == mv &&
          v.xkn == xn);
    CHECK(v.ctx == c.ctx && v.n == c.n && v.box.ls == ls && v.box.us == us);
  }
  // spx_step_begin's `others`: run_iproxstep's list, which is run_proxstep's when the call has no d
  const auto o = c.others();
  std::vector<const void*> mine;
  for (const void* p : o) if (p) mine.push_back(p);
  CHECK(mine == non_null({y, q, d, xk, sj, l, u, mask}));
  if (!d) CHECK(mine == non_null({y, q, xk, sj, l, u, mask}));
}

static void check_f32(float* y, const float* q, const float* d, const float* xk, const float* sj, const float* l, const float* u,
                      const uint8_t* mask, float* xkn) {
  const SepCall<float> c{nullptr, y, q, d, xk, sj, 1000, {l, u, -1.5f, 2.5f, mask}, xkn};
  // run_f32, as it was
  for (int kbox = 0; kbox < 2; ++kbox) {
    auto mis = [](const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u); };
    const unsigned m = mis(y);
    bool same = (m % 4 == 0) && mis(q) == m && mis(xk) == m && mis(sj) == m && (!d || mis(d) == m);
    if (kbox) same = same && (!l || mis(l) == m) && (!u || mis(u) == m);
    CHECK(c.same_misalignment(kbox != 0) == same);
  }
  for (int head = 0; head < 4; ++head) {
    const uint8_t* mk = mask ? mask + head : nullptr;
    const float* lp = l ? l + head : nullptr;
    const float* up = u ? u + head : nullptr;
    const float* dp = d ? d + head : nullptr;
    const SepCall<float> v = c.shifted(head);
    CHECK(v.y == y + head && v.q == q + head && v.d == dp && v.xk == xk + head && v.sj == sj + head && v.box.l == lp &&
          v.box.u == up && v.box.mask == mk);
    CHECK(v.box.ls == -1.5f && v.box.us == 2.5f && v.n == c.n);
  }
}

int main() {
  {  // a value-initialised box is "no box"
    const SpxBox<double> none{};
    CHECK(!none.l && !none.u && !none.mask && none.ls == 0.0 && none.us == 0.0);
  }
  const int off64[2] = {0, 8}, mask64[3] = {0, 8, 1}, off32[4] = {0, 4, 8, 12};
  // Float64: y, q, xk, sj at 2 offsets each; d, l, u, xkn NULL or at 2 offsets; the mask NULL or at 3
  for (int r = 0; r < 16; ++r)
    for (int sd = 0; sd < 3; ++sd) for (int sl = 0; sl < 3; ++sl) for (int su = 0; su < 3; ++su)
      for (int sm = 0; sm < 4; ++sm) for (int sx = 0; sx < 3; ++sx)
        check_f64(at<double*>(0, off64[r & 1]), at<const double*>(1, off64[(r >> 1) & 1]), opt<const double*>(2, off64, sd),
                  at<const double*>(3, off64[(r >> 2) & 1]), at<const double*>(4, off64[(r >> 3) & 1]),
                  opt<const double*>(5, off64, sl), opt<const double*>(6, off64, su), opt<const uint8_t*>(7, mask64, sm),
                  opt<double*>(8, off64, sx));
  // Float32: 4 offsets each
  for (int r = 0; r < 256; ++r)
    for (int sd = 0; sd < 5; ++sd) for (int sl = 0; sl < 5; ++sl) for (int su = 0; su < 5; ++su)
      for (int sm = 0; sm < 5; ++sm) for (int sx = 0; sx < 5; ++sx)
        check_f32(at<float*>(0, off32[r & 3]), at<const float*>(1, off32[(r >> 2) & 3]), opt<const float*>(2, off32, sd),
                  at<const float*>(3, off32[(r >> 4) & 3]), at<const float*>(4, off32[(r >> 6) & 3]),
                  opt<const float*>(5, off32, sl), opt<const float*>(6, off32, su), opt<const uint8_t*>(7, off32, sm),
                  opt<float*>(8, off32, sx));
  if (g_fail) { printf("%d of %ld checks failed\n", g_fail, g_checked); return 1; }
  printf("ok\n");
  return 0;
}
