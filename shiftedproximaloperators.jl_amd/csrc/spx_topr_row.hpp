// spx_topr_row.hpp -- the exact top-r selection of ShiftedIndBallL0[BInf] on ONE row whose every histogram is formed by ONE owner
// (a workgroup: k_topr_batch of spx_topr_batch.hip; a plain loop on the host: tests/c/topr_batch_plan_driver.hip), stated once as
// __host__ __device__ functions of plain values.  No HIP include, no kernel.
//
// The reference sorts: sortperm!(p, y, rev = true, by = abs), a STABLE permutation -- descending |v|, ties in ascending index, NaN
// the largest value and all NaNs equal (isless).  Only the set of the first r entries matters, so the prox is an exact selection in
// the composite order (key descending, index ascending) with key = bits(|v|), every NaN mapped to one key above Inf: the order
// spx_select.hip states.  The selection is an MSD radix select with 12-bit digits:
//   key digits   of key - base over the part of key space still undecided, [base, base + 2^(shift + width)).  The first interval
//                is the data's own span [kmin, kmax], so no exponent bin runs hot; every further one is the bucket that holds the
//                cut.  The histogram is scanned from the top.
//   index digits only when the threshold key is shared by more elements than the quota left: the digits of i over {i : key_i ==
//                t_eq}, most significant first, scanned from the bottom.
//   resolved     keep_i = key_i >= t_ge || (key_i == t_eq && i <= icut).
// A pass costs the owner one histogram of the row; a Float64 row of n <= 2^20 needs at most 6 key digits and 2 index digits.
// spx_select.hip keeps its own statement of the same rule (it is not edited to use this one); the result is an exact selection,
// so two correct statements give the same kept set -- tests/test_gpu_proxstep_topr_batch.py holds the batched call to the single
// call bit for bit.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SPX_TOPR_ROW_HD __host__ __device__ inline
#else
#define SPX_TOPR_ROW_HD inline
#endif

constexpr int kToprDigitBits = 12;
constexpr int kToprBins = 1 << kToprDigitBits;
constexpr int kToprMaxPasses = 16;  // histogram passes of one row at most (the caller's cap: <= 6 key + <= 2 index digits are needed)
constexpr uint64_t kToprInfKey = 0x7ff0000000000000ull;
constexpr uint64_t kToprNanKey = 0x7ff8000000000000ull;

enum ToprPhase { kToprKeyDigits = 0, kToprIndexDigits = 1, kToprResolved = 2 };

struct ToprRowState {
  int phase;        // ToprPhase
  int shift;        // low bit of the digit the next histogram looks at
  int width;        // its width in bits
  int idx_bits;     // significant bits of n - 1
  uint64_t base;    // key digits: low end of the undecided interval
  uint64_t prefix;  // index digits: the decided high index bits
  int64_t quota;    // elements still to be taken from the undecided part
  uint64_t t_ge;    // keep if key >= t_ge
  uint64_t t_eq;    // keep if key == t_eq && i <= icut
  int64_t icut;
};

// the 64-bit key of a double: bits(|v|), every NaN one key above Inf
SPX_TOPR_ROW_HD uint64_t topr_key_of_bits(uint64_t bits) {
  const uint64_t k = bits & 0x7fffffffffffffffull;
  return k > kToprInfKey ? kToprNanKey : k;
}
SPX_TOPR_ROW_HD uint64_t topr_key(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return topr_key_of_bits(b);
}

SPX_TOPR_ROW_HD int topr_bit_length(uint64_t x) {
  int b = 0;
  while (b < 64 && (x >> b) != 0) ++b;
  return b;
}
// index digits, most significant first: the top digit takes the bits that do not fill a whole digit
SPX_TOPR_ROW_HD void topr_first_index_digit(ToprRowState& s) {
  const int bits = s.idx_bits;
  if (bits == 0) { s.phase = kToprResolved; s.icut = 0; return; }  // (n == 1 never gets here: r <= 0 or r >= n)
  const int w = bits % kToprDigitBits ? bits % kToprDigitBits : kToprDigitBits;
  s.phase = kToprIndexDigits;
  s.prefix = 0;
  s.shift = bits - w;
  s.width = w;
}

// the state before the first histogram: n elements, keep r, the row's keys span [kmin, kmax]
SPX_TOPR_ROW_HD ToprRowState topr_row_begin(int64_t n, int64_t r, uint64_t kmin, uint64_t kmax) {
  ToprRowState s;
  s.idx_bits = n > 1 ? topr_bit_length((uint64_t)(n - 1)) : 0;
  s.phase = kToprResolved;
  s.shift = 0;
  s.width = 0;
  s.base = kmin;
  s.prefix = 0;
  s.quota = 0;
  s.t_ge = ~0ull;  // no key reaches it: nothing kept
  s.t_eq = ~0ull;
  s.icut = -1;
  if (r <= 0 || n <= 0) return s;
  if (r >= n) { s.t_ge = 0ull; return s; }  // everything kept
  s.quota = r;
  if (kmax == kmin) {  // one key value: straight to the index digits
    s.t_eq = kmin;
    s.t_ge = kmin + 1;  // keys are < 2^63
    topr_first_index_digit(s);
    return s;
  }
  const int sb = topr_bit_length(kmax - kmin);  // every key is inside [base, base + 2^sb)
  s.phase = kToprKeyDigits;
  s.width = sb < kToprDigitBits ? sb : kToprDigitBits;
  s.shift = sb - s.width;
  return s;
}

// does element i with key `key` count in the histogram of state s, and in which bin
SPX_TOPR_ROW_HD bool topr_row_digit(const ToprRowState& s, uint64_t key, int64_t i, unsigned int* digit) {
  const int hs = s.shift + s.width;
  const unsigned int mask = (1u << s.width) - 1u;
  if (s.phase == kToprKeyDigits) {
    const uint64_t rel = key - s.base;
    *digit = (unsigned int)(rel >> s.shift) & mask;
    return key >= s.base && (hs >= 64 || (rel >> hs) == 0);
  }
  *digit = (unsigned int)((uint64_t)i >> s.shift) & mask;
  return key == s.t_eq && ((uint64_t)i >> hs) == s.prefix;
}

// the state after a scan located the bucket of the quota-th element: `before` elements precede the bucket in scan order (key
// digits: from the top; index digits: from the bottom), `count` are in it
SPX_TOPR_ROW_HD ToprRowState topr_row_advance(const ToprRowState& st, uint64_t bucket, uint64_t before, uint64_t count) {
  ToprRowState o = st;
  const uint64_t left = (uint64_t)st.quota - before;  // to be taken from this bucket: 1 <= left <= count
  if (st.phase == kToprKeyDigits) {
    const uint64_t lowkey = st.base + (bucket << st.shift);
    if (left == count) {  // the whole bucket is kept: no tie
      o.phase = kToprResolved;
      o.t_ge = lowkey;
    } else if (st.shift == 0) {  // the full key is known and more elements share it than are wanted
      o.t_ge = lowkey + 1;
      o.t_eq = lowkey;
      o.quota = (int64_t)left;
      topr_first_index_digit(o);
    } else {  // the next digit inside this bucket
      o.base = lowkey;
      o.quota = (int64_t)left;
      o.width = st.shift < kToprDigitBits ? st.shift : kToprDigitBits;
      o.shift = st.shift - o.width;
    }
    return o;
  }
  const uint64_t prefix = (st.prefix << st.width) | bucket;
  if (left == count || st.shift == 0) {  // every index of this bucket is kept
    o.phase = kToprResolved;
    o.icut = (int64_t)(((prefix + 1) << st.shift) - 1);
  } else {
    o.prefix = prefix;
    o.quota = (int64_t)left;
    o.width = st.shift < kToprDigitBits ? st.shift : kToprDigitBits;
    o.shift = st.shift - o.width;
  }
  return o;
}

// One step: hist[d] = the number of elements topr_row_digit puts into bin d (bins >= 2^width are not looked at).  The kernel
// locates the bucket with a workgroup scan and calls topr_row_advance; this is the same step as a plain loop.
template <class Count>
SPX_TOPR_ROW_HD ToprRowState topr_row_step(const ToprRowState& st, const Count* hist) {
  const int nb = 1 << st.width;
  const uint64_t quota = (uint64_t)st.quota;
  uint64_t run = 0;
  for (int pos = 0; pos < nb; ++pos) {
    const int bin = st.phase == kToprKeyDigits ? nb - 1 - pos : pos;
    const uint64_t c = (uint64_t)hist[bin];
    if (run + c >= quota) return topr_row_advance(st, (uint64_t)bin, run, c);
    run += c;
  }
  ToprRowState o = st;  // a histogram that does not hold the quota: not one of this row's
  o.phase = kToprResolved;
  return o;
}

SPX_TOPR_ROW_HD bool topr_row_keep(const ToprRowState& s, uint64_t key, int64_t i) {
  return key >= s.t_ge || (key == s.t_eq && i <= s.icut);
}
