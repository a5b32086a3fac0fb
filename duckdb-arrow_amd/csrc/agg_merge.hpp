// agg_merge.hpp -- how two partial results of one aggregate of mi_scan_aggregate become one.  One header for hipcc and a
// plain C++ compiler: the lanes of agg_windows, its wave and workgroup reductions, agg_combine, the host's merge of the
// per-device results (MultiDeviceScan::Aggregate) and the stand-alone check under tests/sanitize/ all compile these
// functions, so a value is folded by the same rule wherever it is folded.  Nothing here allocates.
//
// A partial is {lo, hi, count, flags}:
//   count   rows that contributed (COUNT(*): the selected rows; COUNT(col): the selected rows that are not NULL; the
//           others: the selected rows whose input -- both factors of a product, every column an expression names -- is
//           not NULL).  count == 0 is the NULL rule: "no contributor", the partial is the identity of every merge, and
//           SUM / MIN / MAX of it is NULL.
//   lo, hi  integer classes: a 128-bit two's-complement integer -- the sum (wrapping modulo 2^128), or the minimum /
//           maximum sign- or zero-extended; kClassWide orders by `hi` signed, then `lo` unsigned, which is the order of
//           the extended narrow integers too.  kClassFloat: lo = the bits of a double (hi = 0) -- the sum, or the
//           canonical minimum / maximum in the total order of filter_key.hpp (NaN greatest, -0.0 = +0.0).
//   flags   MI_ST_* bits the kernel raised for this partial; a merge ORs them.
// The double sum is merged as `into + from` in the order the caller merges: every reduction here has one fixed shape, so
// the same file, options and device count give the same bits.
#pragma once

#include <cstdint>
#include <cstring>

#include "filter_key.hpp"

namespace miarrow {
namespace aggmerge {

// the operations (== MI_AGG_* of mi_arrow_ipc.h)
constexpr int kOpCountStar = 1, kOpCount = 2, kOpSum = 3, kOpSumProduct = 4, kOpMin = 5, kOpMax = 6;
constexpr int kOpSumExpr = 7;       // SUM of a product of 1 .. kMaxExprFactors affine factors, each add + mul * column or a constant
constexpr int kMaxExprFactors = 4;  // (== MI_MAX_EXPR_FACTORS)
// what a column's values are (== MI_AGG_CLASS_* of mi_arrow_ipc.h)
constexpr int kClassAny = 0;        // COUNT alone: only the validity is read
constexpr int kClassSigned = 1;     // width 1 / 2 / 4 / 8, sign-extended
constexpr int kClassUnsigned = 2;   // width 1 / 2 / 4 / 8, zero-extended: a uint64 of 2^63 or more is positive
constexpr int kClassFloat = 3;      // width 4 / 8, widened to double
constexpr int kClassWide = 4;       // width 16: hugeint_t{uint64 lower; int64 upper}
constexpr int kMaxAggregates = 8;

struct Partial {
  uint64_t lo, hi, count, flags;
};

constexpr uint64_t kCanonicalNaN = 0x7FF8000000000000ull;

MI_KEY_FN uint64_t BitsOf(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
MI_KEY_FN double DoubleOf(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}

//! {lo, hi} += {blo, bhi} modulo 2^128
MI_KEY_FN void Add128(uint64_t* lo, uint64_t* hi, uint64_t blo, uint64_t bhi) {
  const uint64_t nlo = *lo + blo;
  *hi += bhi + (nlo < *lo ? 1ull : 0ull);
  *lo = nlo;
}

//! a double as MIN / MAX return it: every NaN is the one quiet NaN, -0.0 is +0.0
MI_KEY_FN uint64_t CanonicalBits(double v) {
  const uint64_t b = BitsOf(v);
  const uint64_t mag = b & 0x7FFFFFFFFFFFFFFFull;
  if (mag > 0x7FF0000000000000ull) return kCanonicalNaN;
  return mag == 0 ? 0ull : b;
}

//! a < b in the order of the class (`is_float`: canonical double bits in `lo`; else 128-bit integers)
MI_KEY_FN bool Less(bool is_float, uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi) {
  if (is_float) return filterkey::FloatKey(static_cast<int64_t>(alo)) < filterkey::FloatKey(static_cast<int64_t>(blo));
  return filterkey::WideLess(static_cast<int64_t>(ahi), alo, static_cast<int64_t>(bhi), blo);
}

//! into = into (+) from for the aggregate `op` over values of class `cls` (for a product: kClassFloat or an integer class).
//! kOpSumExpr merges as the two other sums do.  WITH_EXPR = false is for a caller that never holds a kOpSumExpr -- the
//! kernel instantiations for programs without an expression, and the combine kernels, whose launchers hand an expression
//! sum over as kOpSum -- and compiles the test for it away, so those kernels are the code they were before expressions.
template <bool WITH_EXPR = true>
MI_KEY_FN void Merge(int op, int cls, Partial* into, const Partial& from) {
  into->flags |= from.flags;
  if (from.count == 0) return;   // the NULL rule: nothing contributed, nothing changes
  if (into->count == 0) {
    into->lo = from.lo;
    into->hi = from.hi;
    into->count = from.count;
    return;
  }
  const bool is_float = cls == kClassFloat;
  if (op == kOpSum || op == kOpSumProduct || (WITH_EXPR && op == kOpSumExpr)) {
    if (is_float) into->lo = BitsOf(DoubleOf(into->lo) + DoubleOf(from.lo));
    else Add128(&into->lo, &into->hi, from.lo, from.hi);
  } else if (op == kOpMin) {
    if (Less(is_float, from.lo, from.hi, into->lo, into->hi)) { into->lo = from.lo; into->hi = from.hi; }
  } else if (op == kOpMax) {
    if (Less(is_float, into->lo, into->hi, from.lo, from.hi)) { into->lo = from.lo; into->hi = from.hi; }
  }
  into->count += from.count;
}

//! one contributing value folded into a partial: the same as Merge with a partial of count 1
template <bool WITH_EXPR = true>
MI_KEY_FN void Fold(int op, int cls, Partial* into, uint64_t lo, uint64_t hi) {
  const Partial one = {lo, hi, 1ull, 0ull};
  Merge<WITH_EXPR>(op, cls, into, one);
}

// ---- the expression of kOpSumExpr: f_0 * f_1 * ... * f_{F-1}, a factor add + mul * v or the constant add.  One step takes the
// product of the factors before it (`first`: there is none) and returns it times this factor.

//! integer expressions: v sign- or zero-extended to {vlo, vhi} by the caller, mul and add sign-extended here; the factor
//! and the product modulo 2^128, in unsigned arithmetic throughout (nothing signed can overflow)
MI_KEY_FN void ExprStepInt(bool first, bool has_column, int64_t mul, int64_t add, uint64_t vlo, uint64_t vhi, uint64_t* lo, uint64_t* hi) {
  typedef unsigned __int128 u128;
  const u128 a = (static_cast<u128>(add < 0 ? ~0ull : 0ull) << 64) | static_cast<uint64_t>(add);
  u128 f = a;
  if (has_column) {
    const u128 m = (static_cast<u128>(mul < 0 ? ~0ull : 0ull) << 64) | static_cast<uint64_t>(mul);
    const u128 v = (static_cast<u128>(vhi) << 64) | vlo;
    f = a + m * v;
  }
  if (!first) f = ((static_cast<u128>(*hi) << 64) | *lo) * f;
  *lo = static_cast<uint64_t>(f);
  *hi = static_cast<uint64_t>(f >> 64);
}

//! a * b and a + b rounded once each, never contracted into an fma (the host compiler may contract `a * b + c` otherwise)
MI_KEY_FN double MulRn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  volatile double r = a * b;
  return r;
#endif
}
MI_KEY_FN double AddRn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  volatile double r = a + b;
  return r;
#endif
}

//! floating-point expressions: the factor is (mul * v) + add, each rounded once; a mul of exactly 1.0 skips the
//! multiplication and an add of exactly +0.0 the addition, so a plain column is its value bit for bit (-0.0, NaN payloads);
//! the product is taken left to right, each step rounded once
MI_KEY_FN double ExprStepDouble(bool first, bool has_column, double mul, double add, double v, double product) {
  double f = add;
  if (has_column) {
    f = mul == 1.0 ? v : MulRn(mul, v);
    if (BitsOf(add) != 0ull) f = AddRn(f, add);
  }
  return first ? f : MulRn(product, f);
}

//! SUM / MIN / MAX over no contributor is NULL; a COUNT never is
MI_KEY_FN bool IsNull(int op, const Partial& p) { return op != kOpCountStar && op != kOpCount && p.count == 0; }

}  // namespace aggmerge
}  // namespace miarrow
