// ygm_dtoa.hpp -- Number::toString(x) of a finite double (ECMA-262 6.1.6.1.20), host and device: what JSON.stringify
// writes for a number.  The walkers reach it for the float32 / float64 tags of a ContentAny when the context was opened
// with YGM_F_FLOATS (v2::any_json's FLOATS form); tools/snapdev/dtoadev.cpp runs the same code on the host.
//
//   digits  the fewest decimal digits that read back as x, and among those the closest to x: Schubfach (R. Giulietti,
//           "The Schubfach way to render doubles", 2020), whose one table is g(k) -- the 128 most significant bits of
//           10^k, rounded up -- for k = -292 .. 324 (ygm_dtoa_pow5.inc, written by tools/gen_pow5.py; 617 entries,
//           9872 bytes of __device__ const data in global memory: one 16-byte load per number)
//   layout  x = digits * 10^(n - k), k the digit count:   k <= n <= 21  digits, then n - k zeros
//                                                           0 < n <= 21  a point after n digits
//                                                          -6 < n <= 0   "0.", -n zeros, the digits
//                                                           otherwise    d[.ddd]e(+|-)(n - 1)
//           zero and negative zero are "0".  At most 25 bytes: -1.7976931348623157e+308 has 24, and seventeen digits
//           behind "-0.00000" (-0.0000027410441684333906) one more.
//
// Integer arithmetic only (no double, no long double, no printf), so host and device compute the same bits; the one
// 64 x 64 -> 128 bit product is mul_hi (__umul64hi / unsigned __int128) -- two of them and one low product for each of
// the three candidates of a number: slow-class multiplies, paid once per number and not per digit.  The digits are not kept in an array (a local
// array indexed at run time lives in scratch): they are packed four bits each into one register (sixteen of them, the
// seventeenth beside it) and written most significant first.
#pragma once
#include <stdint.h>

#include "ygm_v1.hpp"

namespace ygm {
namespace dtoa {

constexpr int32_t K_MIN = -292, K_MAX = 324;
#ifdef YGM_HOST_BUILD
static const uint64_t POW5[K_MAX - K_MIN + 1][2] = {
#else
static __device__ const uint64_t POW5[K_MAX - K_MIN + 1][2] = {
#endif
#include "ygm_dtoa_pow5.inc"
};

YDEV uint64_t mul_hi(uint64_t a, uint64_t b) {
#ifdef YGM_HOST_BUILD
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#else
  return __umul64hi(a, b);
#endif
}
// the high 64 bits of g * cp (g = hi:lo, 128 bits; cp < 2^60), with every lower bit of the product folded into bit 0
YDEV uint64_t round_to_odd(uint64_t hi, uint64_t lo, uint64_t cp) {
  const uint64_t x1 = mul_hi(lo, cp);
  uint64_t y0 = hi * cp, y1 = mul_hi(hi, cp);
  y0 += x1;
  if (y0 < x1) y1++;
  return y1 | (uint64_t)(y0 > 1);
}

// a float32's bits widened exactly to a double's, as JavaScript reads a Float32Array element
YDEV uint64_t widen_f32(uint32_t b) {
  const uint64_t sign = (uint64_t)(b >> 31) << 63;
  uint32_t e = (b >> 23) & 255u, f = b & 0x7FFFFFu;
  if (e == 255u) return sign | (0x7FFull << 52) | ((uint64_t)f << 29);
  if (e == 0u) {
    if (f == 0u) return sign;
    e = 1u;
    while (!(f & 0x800000u)) { f <<= 1; e--; }   // (a subnormal float is a normal double: e wraps below zero, 896 brings it back)
    f &= 0x7FFFFFu;
  }
  return sign | ((uint64_t)(e + 896u) << 52) | ((uint64_t)f << 29);
}
YDEV bool finite(uint64_t bits) { return ((bits >> 52) & 0x7FFu) != 0x7FFu; }

// the shortest digits m and exponent e with x = m * 10^e, for the fraction and biased exponent of a finite double that
// is not zero; m < 10^17 and may end in zeros
YDEV void shortest(uint64_t frac, uint32_t bexp, uint64_t& m, int32_t& e) {
  const uint64_t c = bexp ? (frac | (1ull << 52)) : frac;
  const int32_t q = bexp ? (int32_t)bexp - 1075 : -1074;
  const bool even = !(c & 1u);
  const bool narrow = frac == 0 && bexp > 1u;   // a power of two: its lower neighbour is half as far as the upper one
  const uint64_t cbl = 4 * c - 2 + (narrow ? 1u : 0u), cb = 4 * c, cbr = 4 * c + 2;
  const int32_t k = narrow ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22;   // floor(log10(3/4 * 2^q)), floor(log10(2^q))
  const int32_t h = q + ((-k * 1741647) >> 19) + 1;                                // q + floor(log2(10^-k)) + 1: 1 .. 4
  const uint64_t hi = POW5[-k - K_MIN][0], lo = POW5[-k - K_MIN][1];
  const uint64_t vbl = round_to_odd(hi, lo, cbl << h), vb = round_to_odd(hi, lo, cb << h), vbr = round_to_odd(hi, lo, cbr << h);
  const uint64_t lower = vbl + (even ? 0u : 1u), upper = vbr - (even ? 0u : 1u);
  const uint64_t s = vb >> 2;
  if (s >= 10) {   // one digit fewer, when exactly one of its two candidates lies inside
    const uint64_t sp = s / 10;
    const bool up = lower <= 40 * sp, wp = 40 * sp + 40 <= upper;
    if (up != wp) { m = sp + (wp ? 1u : 0u); e = k + 1; return; }
  }
  const bool u = lower <= 4 * s, w = 4 * s + 4 <= upper;
  if (u != w) { m = s + (w ? 1u : 0u); e = k; return; }
  const uint64_t mid = 4 * s + 2;   // both inside: the closer one, a tie to the even one
  m = s + ((vb > mid || (vb == mid && (s & 1u))) ? 1u : 0u); e = k;
}

// Number::toString of the finite double `bits` through writer O (O::b): at most 25 bytes
template <class O>
YDEV void write(O& o, uint64_t bits) {
  const uint64_t frac = bits & ((1ull << 52) - 1u);
  const uint32_t bexp = (uint32_t)(bits >> 52) & 0x7FFu;
  if (!frac && !bexp) { o.b('0'); return; }
  if (bits >> 63) o.b('-');
  uint64_t m; int32_t e;
  shortest(frac, bexp, m, e);
  while (m % 10 == 0) { m /= 10; e++; }
  uint64_t bcd = 0; uint32_t k = 0;   // digit j (least significant first) in bits [4j, 4j + 4); the 17th in `m` after the loop
  while (m && k < 16u) { bcd |= (m % 10) << (4u * k); m /= 10; k++; }
  const uint32_t top = (uint32_t)m;
  if (top) k++;
  const int32_t n = (int32_t)k + e;
  uint32_t i = 0;   // digits written
#define YGM_DTOA_DIGIT() do { const uint32_t j_ = k - 1u - i; o.b((uint8_t)('0' + (j_ == 16u ? top : (uint32_t)(bcd >> (4u * j_)) & 15u))); i++; } while (0)
  if (n > 21 || n <= -6) {
    YGM_DTOA_DIGIT();
    if (k > 1u) { o.b('.'); while (i < k) YGM_DTOA_DIGIT(); }
    o.b('e'); o.b(n > 0 ? '+' : '-');
    const uint32_t x = (uint32_t)(n > 0 ? n - 1 : 1 - n);
    if (x >= 100u) o.b((uint8_t)('0' + x / 100u));
    if (x >= 10u) o.b((uint8_t)('0' + x / 10u % 10u));
    o.b((uint8_t)('0' + x % 10u));
  } else if (n <= 0) {
    o.b('0'); o.b('.');
    for (int32_t z = n; z < 0; z++) o.b('0');
    while (i < k) YGM_DTOA_DIGIT();
  } else {
    while (i < k) { if ((int32_t)i == n) o.b('.'); YGM_DTOA_DIGIT(); }
    for (int32_t z = (int32_t)k; z < n; z++) o.b('0');
  }
#undef YGM_DTOA_DIGIT
}

}  // namespace dtoa
}  // namespace ygm
