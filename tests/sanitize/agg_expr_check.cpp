// agg_expr_check.cpp -- the factor and product arithmetic of MI_AGG_SUM_EXPR (ExprStepInt / ExprStepDouble of
// duckdb-arrow_amd/csrc/agg_merge.hpp, the header the aggregate kernels compile) against plain restatements: unsigned
// __int128 for the integers, the stated rounding order for the doubles.  A program of its own for
// g++ -fsanitize=address,undefined -ffp-contract=off.  No arguments; prints "<checks> checks, <failed> failed" and exits 1
// on a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "agg_merge.hpp"

using namespace miarrow::aggmerge;

namespace {
long failed = 0, checks = 0;

void Expect(bool ok, const char* what, long a = 0, long b = 0) {
  checks++;
  if (!ok && failed++ < 20) std::fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
}

typedef unsigned __int128 u128;
typedef __int128 i128;
u128 U(uint64_t lo, uint64_t hi) { return (static_cast<u128>(hi) << 64) | lo; }
// int64 -> 128 bits, sign-extended, by the language's own conversion
u128 S(int64_t v) { return static_cast<u128>(static_cast<i128>(v)); }

const int64_t kConstants[] = {0, 1, -1, INT64_MIN, INT64_MAX, 100, -100, 3};

// a stored value of `width` bytes, read as the kernels read it: sign- or zero-extended to 128 bits
u128 Extend(uint64_t raw, int width, bool is_signed) {
  switch (width) {
    case 1: return is_signed ? S(static_cast<int8_t>(raw)) : static_cast<u128>(static_cast<uint8_t>(raw));
    case 2: return is_signed ? S(static_cast<int16_t>(raw)) : static_cast<u128>(static_cast<uint16_t>(raw));
    case 4: return is_signed ? S(static_cast<int32_t>(raw)) : static_cast<u128>(static_cast<uint32_t>(raw));
    default: return is_signed ? S(static_cast<int64_t>(raw)) : static_cast<u128>(raw);
  }
}

std::vector<uint64_t> RawValues(int width) {
  const uint64_t mask = width == 8 ? ~0ull : (1ull << (8 * width)) - 1;
  const uint64_t top = 1ull << (8 * width - 1);
  return {0, 1, 2, 7, top - 1, top, top + 1, mask - 1, mask, 0x5A5A5A5A5A5A5A5Aull & mask, 0xA5A5A5A5A5A5A5A5ull & mask};
}

// ---- one factor: add + mul * v modulo 2^128, every width and signedness, every constant
void CheckIntFactor() {
  for (int width : {1, 2, 4, 8})
    for (bool is_signed : {true, false})
      for (uint64_t raw : RawValues(width)) {
        const u128 v = Extend(raw, width, is_signed);
        for (int64_t mul : kConstants)
          for (int64_t add : kConstants) {
            uint64_t lo = 0xDEADBEEFull, hi = 0xFEEDull;   // `first`: what was there is not read
            ExprStepInt(true, true, mul, add, static_cast<uint64_t>(v), static_cast<uint64_t>(v >> 64), &lo, &hi);
            Expect(U(lo, hi) == S(add) + S(mul) * v, "factor add + mul * v against unsigned __int128", width, is_signed);
            lo = 5;
            hi = 9;
            ExprStepInt(true, false, mul, add, static_cast<uint64_t>(v), static_cast<uint64_t>(v >> 64), &lo, &hi);
            Expect(U(lo, hi) == S(add), "a constant factor is add, sign-extended; mul and the value are ignored");
          }
      }
  // a plain column is its value
  for (uint64_t raw : RawValues(8))
    for (bool is_signed : {true, false}) {
      const u128 v = Extend(raw, 8, is_signed);
      uint64_t lo = 0, hi = 0;
      ExprStepInt(true, true, 1, 0, static_cast<uint64_t>(v), static_cast<uint64_t>(v >> 64), &lo, &hi);
      Expect(U(lo, hi) == v, "mul 1, add 0: the value itself");
    }
}

// ---- products of 2 .. 4 factors, those that wrap past 2^128 included
void CheckIntProduct() {
  const std::vector<uint64_t> raws = {0, 1, 3, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, 0x123456789ABCDEFull};
  long wrapped = 0;
  for (bool is_signed : {true, false})
    for (uint64_t r0 : raws)
      for (uint64_t r1 : raws)
        for (int64_t mul : {int64_t{1}, int64_t{-1}, INT64_MIN, INT64_MAX})
          for (int64_t add : {int64_t{0}, int64_t{100}, INT64_MIN, INT64_MAX}) {
            const u128 v0 = Extend(r0, 8, is_signed), v1 = Extend(r1, 8, is_signed);
            const u128 f0 = S(add) + S(mul) * v0, f1 = S(0) + S(1) * v1, f2 = S(add), f3 = S(7) + S(mul) * v0;
            uint64_t lo = 0, hi = 0;
            ExprStepInt(true, true, mul, add, static_cast<uint64_t>(v0), static_cast<uint64_t>(v0 >> 64), &lo, &hi);
            ExprStepInt(false, true, 1, 0, static_cast<uint64_t>(v1), static_cast<uint64_t>(v1 >> 64), &lo, &hi);
            Expect(U(lo, hi) == f0 * f1, "two factors");
            ExprStepInt(false, false, 0, add, 0, 0, &lo, &hi);
            Expect(U(lo, hi) == f0 * f1 * f2, "three factors, the third a constant");
            ExprStepInt(false, true, mul, 7, static_cast<uint64_t>(v0), static_cast<uint64_t>(v0 >> 64), &lo, &hi);   // the same column again
            Expect(U(lo, hi) == f0 * f1 * f2 * f3, "four factors, the first column twice");
            // did the true product leave 128 bits?  (magnitudes: the product of four 127-bit magnitudes does not fit)
            if (f0 != 0 && (f0 * f1) / f0 != f1) wrapped++;
          }
  Expect(wrapped > 100, "the cases hold products that wrap past 2^128", wrapped);
  // (2^64 - 1)^2 * (2^64 - 1): past 2^128, by hand
  uint64_t lo = 0, hi = 0;
  ExprStepInt(true, true, 1, 0, UINT64_MAX, 0, &lo, &hi);
  ExprStepInt(false, true, 1, 0, UINT64_MAX, 0, &lo, &hi);
  Expect(lo == 1 && hi == UINT64_MAX - 1, "(2^64 - 1)^2 = 2^128 - 2^65 + 1");
  ExprStepInt(false, true, 1, 0, UINT64_MAX, 0, &lo, &hi);
  Expect(U(lo, hi) == U(1, UINT64_MAX - 1) * static_cast<u128>(UINT64_MAX), "(2^64 - 1)^3 modulo 2^128");
  // INT64_MIN * INT64_MIN * INT64_MIN * INT64_MIN = 2^252 = 0 modulo 2^128; nothing signed overflows on the way (UBSan)
  const u128 m = S(INT64_MIN);
  lo = hi = 0;
  for (int f = 0; f < 4; f++) ExprStepInt(f == 0, true, INT64_MIN, INT64_MIN, static_cast<uint64_t>(m), static_cast<uint64_t>(m >> 64), &lo, &hi);
  const u128 fac = S(INT64_MIN) + S(INT64_MIN) * m;
  Expect(U(lo, hi) == fac * fac * fac * fac, "INT64_MIN everywhere");
}

// ---- doubles: (mul * v) + add, each rounded once; the shortcuts; the product left to right
double Mul(double a, double b) {
  volatile double r = a * b;
  return r;
}
double Add(double a, double b) {
  volatile double r = a + b;
  return r;
}
bool SameBits(double a, double b) { return BitsOf(a) == BitsOf(b); }

void CheckDouble() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> values = {0.0, -0.0, 1.0, -1.0, 0.1, -0.3, 1e308, -1e308, 4.9e-324, 1.0 / 3.0, 123456.789, inf, -inf, nan,
                                      DoubleOf(0x7FF8000000000123ull)};
  const std::vector<double> consts = {0.0, -0.0, 1.0, -1.0, 0.5, 100.0, 1.0 / 3.0, -7.25, 1e300};
  for (double v : values)
    for (double mul : consts)
      for (double add : consts) {
        double want = mul == 1.0 ? v : Mul(mul, v);
        if (BitsOf(add) != 0) want = Add(want, add);
        const double got = ExprStepDouble(true, true, mul, add, v, 12345.0);
        Expect(SameBits(got, want) || (std::isnan(got) && std::isnan(want)), "factor (mul * v) + add, rounded twice, with the shortcuts");
        Expect(SameBits(ExprStepDouble(true, false, mul, add, v, 12345.0), add), "a constant factor is add");
        const double p = ExprStepDouble(false, true, mul, add, v, 3.7);
        Expect(SameBits(p, Mul(3.7, want)) || (std::isnan(p) && std::isnan(want)), "the product takes the factor on the right, rounded once");
      }
  // a plain column is its value bit for bit: -0.0 stays -0.0 (adding +0.0 would make it +0.0), a NaN keeps its payload
  Expect(BitsOf(ExprStepDouble(true, true, 1.0, 0.0, -0.0, 0.0)) == 0x8000000000000000ull, "-0.0 through mul 1.0, add +0.0");
  Expect(BitsOf(ExprStepDouble(true, true, 1.0, 0.0, DoubleOf(0x7FF8000000000123ull), 0.0)) == 0x7FF8000000000123ull, "NaN payload through a plain factor");
  // an add of -0.0 is not the shortcut: -0.0 + -0.0 = -0.0, and +0.0 + -0.0 = +0.0
  Expect(BitsOf(ExprStepDouble(true, true, 1.0, -0.0, -0.0, 0.0)) == 0x8000000000000000ull, "-0.0 + -0.0");
  Expect(BitsOf(ExprStepDouble(true, true, 1.0, -0.0, 0.0, 0.0)) == 0ull, "+0.0 + -0.0");
  // a mul of -1.0 is a multiplication: -1.0 * 0.0 = -0.0
  Expect(BitsOf(ExprStepDouble(true, true, -1.0, 0.0, 0.0, 0.0)) == 0x8000000000000000ull, "-1.0 * +0.0");
  // no fma: with mul = v = 1 + 2^-30 and add = -(1 + 2^-29) the rounded product is 1 + 2^-29 exactly and the sum 0; a
  // fused multiply-add would return 2^-60
  const double x = 1.0 + std::ldexp(1.0, -30);
  Expect(ExprStepDouble(true, true, x, -(1.0 + std::ldexp(1.0, -29)), x, 0.0) == 0.0, "the multiplication is rounded before the addition");
  // left to right: ((a * b) * c) * d
  const double a = 1.0 / 3.0, b = 3.0000000000000004, c = 1e-3, d = 7.0 / 9.0;
  double p = ExprStepDouble(true, true, 1.0, 0.0, a, 0.0);
  p = ExprStepDouble(false, true, 1.0, 0.0, b, p);
  p = ExprStepDouble(false, true, 1.0, 0.0, c, p);
  p = ExprStepDouble(false, true, 1.0, 0.0, d, p);
  Expect(SameBits(p, Mul(Mul(Mul(a, b), c), d)), "the product is taken left to right");
}

// ---- Merge treats the expression sum as the two sums it has
void CheckMerge() {
  Partial s = {5, 0, 2, 0};
  Merge(kOpSumExpr, kClassSigned, &s, Partial{UINT64_MAX, UINT64_MAX, 3, 4});   // + (-1)
  Expect(s.lo == 4 && s.hi == 0 && s.count == 5 && s.flags == 4, "Merge(SUM_EXPR) adds 128-bit values, counts and flags");
  Partial d = {BitsOf(1.5), 0, 1, 0};
  Merge(kOpSumExpr, kClassFloat, &d, Partial{BitsOf(2.25), 0, 2, 0});
  Expect(DoubleOf(d.lo) == 3.75 && d.count == 3, "Merge(SUM_EXPR) adds doubles");
  Partial n = {0, 0, 0, 0};
  Expect(IsNull(kOpSumExpr, n), "no contributor: NULL");
  Merge(kOpSumExpr, kClassFloat, &n, Partial{BitsOf(-0.0), 0, 1, 0});
  Expect(n.lo == 0x8000000000000000ull && n.count == 1, "the first contributor is copied, -0.0 included");
  Expect(kOpSumExpr == 7 && kMaxExprFactors == 4, "the constants of the header");
}
}  // namespace

int main() {
  CheckIntFactor();
  CheckIntProduct();
  CheckDouble();
  CheckMerge();
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
