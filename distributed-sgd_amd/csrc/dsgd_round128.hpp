// ONE rounding of a two-word fixed-point sum to double (csrc/dsgd_rp64.hpp, Rp64Acc<double>::round: the finish of the Double-value gradient).
//
// The sum is T = HI * 2^32 + LO, HI a signed and LO an unsigned 64-bit word: an exact integer of up to 97 bits.  The
// result is the double nearest to T * 2^exp2, ties to even -- written out as shift, round bit and sticky bit over the two
// words, with no 128-bit type and no library conversion, so that the device and a host test compile the same lines
// (tests/test_fp64_values_abi.py compares it with Python's correctly rounded float(int)).
//
// T * 2^exp2 must be a normal double or zero: the callers' unit 2^exp2 is at least 2^-160 whenever a value passes the
// 1e-20 filter (vexp >= -66, exp2 = vexp - shift - 32 >= vexp - 94).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSGD_R128_HD __host__ __device__
#else
#define DSGD_R128_HD
#endif

DSGD_R128_HD inline double dsgd_round128(long long hi, unsigned long long lo, int exp2) {
  // T in two's complement over two words: th (signed, high) : tl (low)
  unsigned long long tl = (unsigned long long)hi << 32;
  long long th = hi >> 32;   // (arithmetic: the sign travels)
  const unsigned long long sum = tl + lo;
  if (sum < tl) th += 1;     // the carry out of the low word
  tl = sum;
  const bool neg = th < 0;
  unsigned long long mh = (unsigned long long)th, ml = tl;
  if (neg) {                 // |T|
    ml = ~ml + 1ull;
    mh = ~mh + (ml == 0ull ? 1ull : 0ull);
  }
  if (mh == 0ull && ml == 0ull) return 0.0;
  const int top = mh ? 127 - __builtin_clzll(mh) : 63 - __builtin_clzll(ml);   // the highest set bit
  unsigned long long q;      // the leading (up to) 53 bits
  int sh = 0;                // bits dropped below them
  if (top <= 52) {
    q = ml;                  // exact
  } else {
    sh = top - 52;           // 1 .. 75
    q = sh >= 64 ? mh >> (sh - 64) : (ml >> sh) | (mh << (64 - sh));
    const int rb = sh - 1;   // the round bit's position
    const bool round = rb >= 64 ? ((mh >> (rb - 64)) & 1ull) != 0ull : ((ml >> rb) & 1ull) != 0ull;
    const bool sticky = rb >= 64 ? (ml != 0ull || (mh & ((1ull << (rb - 64)) - 1ull)) != 0ull) : (ml & ((1ull << rb) - 1ull)) != 0ull;
    if (round && (sticky || (q & 1ull))) q += 1ull;   // nearest, ties to even (q == 2^53 after a carry is still exact)
  }
  // q <= 2^53 converts exactly; the power of two is exact as well
  double r = (double)(long long)q;
  int e = sh + exp2;
  // (ldexp by hand in exact steps: every factor and every product is a normal double)
  while (e > 0) {
    const int s = e > 1000 ? 1000 : e;
    unsigned long long bits = (unsigned long long)(1023 + s) << 52;
    double p;
    __builtin_memcpy(&p, &bits, sizeof(p));
    r = r * p;
    e -= s;
  }
  while (e < 0) {
    const int s = e < -1000 ? 1000 : -e;
    unsigned long long bits = (unsigned long long)(1023 - s) << 52;
    double p;
    __builtin_memcpy(&p, &bits, sizeof(p));
    r = r * p;
    e += s;
  }
  return neg ? -r : r;
}
