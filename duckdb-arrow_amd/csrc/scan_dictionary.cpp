// scan_dictionary.cpp -- see scan_dictionary.hpp.
#include "scan_dictionary.hpp"

#include <cstring>

#include "extension_format.hpp"

namespace miarrow {

bool DictionaryKindIsFlat(int32_t kind) {
  switch (kind) {
    case MI_K_COPY: case MI_K_BOOL: case MI_K_DEC128: case MI_K_DATE64: case MI_K_MUL_I32: case MI_K_MUL_I64: case MI_K_DIV_I64:
    case MI_K_STR32: case MI_K_STR64: case MI_K_FIXED_BINARY: case MI_K_DURATION: case MI_K_INTERVAL_MONTHS: case MI_K_INTERVAL_MDN:
    case MI_K_NARROW: case MI_K_HALF_FLOAT: case MI_K_UUID: case MI_K_BOOL8:
      return true;
    default:
      return false;
  }
}

uint32_t HalfToFloatBits(uint16_t h) {
  const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu;
  uint32_t man = h & 0x3FFu;
  if (exp == 0x1F) return sign | 0x7F800000u | (man << 13);
  if (exp != 0) return sign | ((exp + 112u) << 23) | (man << 13);
  if (man == 0) return sign;
  uint32_t e = 113;   // subnormal half: normalise
  while (!(man & 0x400u)) { man <<= 1; e--; }
  return sign | (e << 23) | ((man & 0x3FFu) << 13);
}

namespace {

// the new string values: FIXED_BINARY straight from buffer 1; STR32 / STR64 through the offsets in buffer 1 into buffer 2 (the
// offsets are validated here; the device validates them again)
void AppendHostStrings(const DecodedBatch& b, int32_t kind, int64_t param, int64_t n_old, int64_t n_new, DictHostValues* out) {
  const mi_buffer_span* sp = &b.buffers[0];
  const int64_t ow = kind == MI_K_STR64 ? 8 : 4;
  // SliceBatch has checked both lengths for every batch a reader hands out (batch_slice.cpp, `s1.length < need1`); they are
  // checked again because everything below reads by them
  if (kind == MI_K_FIXED_BINARY) {
    if (param < 0 || sp[1].length < n_new * param) throw InternalException("Arrow IPC validation failed: dictionary values buffer is too short");
  } else if (n_new > 0 && sp[1].length < (n_new + 1) * ow) {
    throw InternalException("Arrow IPC validation failed: dictionary offsets buffer is too short");
  }
  for (int64_t i = 0; i < n_new; i++) {
    std::string v;
    if (out->host_valid[static_cast<size_t>(n_old + i)] != 0) {
      if (kind == MI_K_FIXED_BINARY) {
        v.assign(reinterpret_cast<const char*>(b.body + sp[1].offset + i * param), static_cast<size_t>(param));
      } else {
        int64_t o0, o1;
        if (kind == MI_K_STR32) {
          int32_t a, c;
          std::memcpy(&a, b.body + sp[1].offset + 4 * i, 4);
          std::memcpy(&c, b.body + sp[1].offset + 4 * (i + 1), 4);
          o0 = a; o1 = c;
        } else {
          std::memcpy(&o0, b.body + sp[1].offset + 8 * i, 8);
          std::memcpy(&o1, b.body + sp[1].offset + 8 * (i + 1), 8);
        }
        if (o0 < 0 || o1 < o0 || o1 > sp[2].length) throw InternalException("Arrow IPC validation failed: dictionary offsets");
        v.assign(reinterpret_cast<const char*>(b.body + sp[2].offset + o0), static_cast<size_t>(o1 - o0));
      }
    }
    out->host_strings.push_back(std::move(v));
  }
}

// the new fixed-width values as the decode leaves them (float16 widened, exactly; arrow.uuid as hugeint_t, arrow.bool8 as 0 / 1;
// every other admitted type as it is stored)
void AppendHostValues(const DecodedBatch& b, int32_t kind, int32_t width, int64_t n_old, int64_t n_new, DictHostValues* out) {
  const mi_buffer_span* sp = &b.buffers[0];
  const size_t vw = static_cast<size_t>(width), sw = kind == MI_K_HALF_FLOAT ? 2 : vw;
  if (sp[1].length < n_new * static_cast<int64_t>(sw)) throw InternalException("Arrow IPC validation failed: dictionary values buffer is too short");
  out->host_values.resize(static_cast<size_t>(n_old + n_new) * vw, 0);
  uint8_t* dst = out->host_values.data() + static_cast<size_t>(n_old) * vw;
  const uint8_t* src = b.body + sp[1].offset;
  if (kind == MI_K_UUID) {
    for (int64_t i = 0; i < n_new; i++) {
      const extfmt::UuidValue u = extfmt::UuidFromArrow(src + 16 * i);
      std::memcpy(dst + 16 * i, &u.lower, 8);
      std::memcpy(dst + 16 * i + 8, &u.upper, 8);
    }
    return;
  }
  if (kind == MI_K_BOOL8) {
    for (int64_t i = 0; i < n_new; i++) dst[i] = extfmt::Bool8(static_cast<int8_t>(src[i]));
    return;
  }
  if (kind != MI_K_HALF_FLOAT) {
    if (n_new > 0) std::memcpy(dst, src, static_cast<size_t>(n_new) * vw);
    return;
  }
  for (int64_t i = 0; i < n_new; i++) {
    uint16_t h;
    std::memcpy(&h, src + 2 * i, 2);
    const uint32_t bits = HalfToFloatBits(h);
    std::memcpy(dst + 4 * i, &bits, 4);
  }
}

}  // namespace

void BuildDictionaryHost(const DecodedBatch& b, int32_t kind, int32_t width, int64_t param, bool keep_values, const DictHostValues* old,
                         uint64_t* words, size_t n_words, DictHostValues* out) {
  const int64_t n_new = b.column_length[0];
  const int64_t n_old = old ? static_cast<int64_t>(old->host_valid.size()) : 0;
  const int64_t n = n_old + n_new;
  if (n_new < 0 || static_cast<size_t>((n + 1 + 63) / 64) > n_words) throw InternalException("dictionary validity words are too few");
  // the validity words come from the Arrow bitmap (the admitted value types are flat: a value is NULL exactly when its bit says so)
  for (size_t i = 0; i < n_words; i++) words[i] = ~0ull;
  auto set_bit = [&](int64_t i, bool v) {
    if (v) words[static_cast<size_t>(i >> 6)] |= 1ull << (i & 63);
    else words[static_cast<size_t>(i >> 6)] &= ~(1ull << (i & 63));
  };
  for (int64_t i = 0; i < n_old; i++) set_bit(i, old->host_valid[static_cast<size_t>(i)] != 0);
  const mi_buffer_span* sp = &b.buffers[0];
  const bool has_bitmap = sp[0].length > 0 && b.null_count[0] != 0;
  if (has_bitmap && sp[0].length < (n_new + 7) / 8) throw InternalException("Arrow IPC validation failed: dictionary validity bitmap is too short");
  for (int64_t i = 0; i < n_new; i++) set_bit(n_old + i, !has_bitmap || ((b.body[sp[0].offset + (i >> 3)] >> (i & 7)) & 1));
  out->host_valid.resize(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; i++) out->host_valid[static_cast<size_t>(i)] = (words[static_cast<size_t>(i >> 6)] >> (i & 63)) & 1;
  if (IsStringKind(kind)) {
    if (old) out->host_strings = old->host_strings;
    AppendHostStrings(b, kind, param, n_old, n_new, out);
  } else if (keep_values) {
    if (old) out->host_values = old->host_values;
    AppendHostValues(b, kind, width, n_old, n_new, out);
  }
}

}  // namespace miarrow
