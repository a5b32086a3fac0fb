// filter_key.hpp -- the order DuckDB gives FLOAT / DOUBLE and 128-bit integers, as the filter kernel (K6) and the host
// compare them.  One header for hipcc and a plain C++ compiler: the kernel, the host side of the filter (constants,
// dictionary match maps), mi_filter_float_key and the stand-alone check under tests/sanitize/ all compile these functions.
//
// Floating point: a total order in which every NaN equals every other NaN (whatever its sign or payload) and is greater
// than everything else, +inf included, and -0.0 = +0.0.  The value's bits `b`, read as a signed integer of the value's
// width, map to a key that compares as a signed integer exactly as the values compare:
//   NaN -> MAX,  -0.0 -> 0,  otherwise b >= 0 ? b : b ^ MAX        (MAX = 0x7FFFFFFF / INT64_MAX)
// Negative values keep their sign bit and have their magnitude bits flipped, so a larger magnitude is a smaller key; the
// key -1 (the image -0.0 would have) is never produced.  Strict bounds are inclusive bounds on key +- 1.
//
// 128-bit integers (HUGEINT, DECIMAL(19..38)) are hugeint_t{uint64 lower; int64 upper}: `upper` signed, then `lower` unsigned.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // __forceinline__
#define MI_KEY_FN __host__ __device__ __forceinline__
#else
#define MI_KEY_FN inline
#endif

namespace miarrow {
namespace filterkey {

MI_KEY_FN int32_t FloatKey(int32_t b) {
  const int32_t max = 0x7FFFFFFF;
  const int32_t mag = b & max;
  if (mag > 0x7F800000) return max;   // NaN: exponent all ones, mantissa not zero
  if (mag == 0) return 0;             // +0.0 and -0.0
  return b >= 0 ? b : b ^ max;
}

MI_KEY_FN int64_t FloatKey(int64_t b) {
  const int64_t max = 0x7FFFFFFFFFFFFFFFll;
  const int64_t mag = b & max;
  if (mag > 0x7FF0000000000000ll) return max;
  if (mag == 0) return 0;
  return b >= 0 ? b : b ^ max;
}

//! Host: the key of `v` as a column of `width` bytes holds it -- 4: rounded to float32 first, as DuckDB casts a constant to
//! the column's type (the key is an int32 key, sign-extended); 8: the double itself
inline int64_t FloatKeyOfDouble(double v, int32_t width) {
  if (width == 4) {
    const float f = static_cast<float>(v);
    int32_t b;
    std::memcpy(&b, &f, 4);
    return FloatKey(b);
  }
  int64_t b;
  std::memcpy(&b, &v, 8);
  return FloatKey(b);
}

//! a < b on (upper signed, lower unsigned)
MI_KEY_FN bool WideLess(int64_t a_upper, uint64_t a_lower, int64_t b_upper, uint64_t b_lower) {
  return a_upper < b_upper || (a_upper == b_upper && a_lower < b_lower);
}
//! lo <= v <= hi
MI_KEY_FN bool WideInRange(int64_t v_upper, uint64_t v_lower, int64_t lo_upper, uint64_t lo_lower, int64_t hi_upper, uint64_t hi_lower) {
  return !WideLess(v_upper, v_lower, lo_upper, lo_lower) && !WideLess(hi_upper, hi_lower, v_upper, v_lower);
}

}  // namespace filterkey
}  // namespace miarrow
