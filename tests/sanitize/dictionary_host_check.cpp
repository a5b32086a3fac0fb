// dictionary_host_check.cpp -- the host side of a dictionary version (duckdb-arrow_amd/csrc/scan_dictionary.cpp:
// BuildDictionaryHost, HalfToFloatBits, DictionaryKindIsFlat) over hand-built DictionaryBatch bodies, as a program of its own
// for g++ -fsanitize=address,undefined.  Every body is one allocation of exactly its size and the buffer a case is about lies
// at its end, so a read past that buffer is a read past the allocation: ASan judges it.  Expected words and strings are
// written out here; the expected floats are the bit patterns of numpy.float16(...).astype(numpy.float32).
// No arguments; prints "<checks> checks, <failed> failed" and exits 1 on a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scan_dictionary.hpp"

using namespace miarrow;

namespace {
long failed = 0, checks = 0;
std::string current;

void Expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  checks++;
  if (!ok && failed++ < 40) std::fprintf(stderr, "FAILED [%s]: %s (%lld, %lld)\n", current.c_str(), what, a, b);
}

typedef std::vector<uint8_t> Bytes;

template <typename T>
Bytes Raw(const std::vector<T>& v) {
  Bytes b(v.size() * sizeof(T));
  if (!v.empty()) std::memcpy(b.data(), v.data(), b.size());
  return b;
}
Bytes Bitmap(const std::vector<int>& valid) {
  Bytes b((valid.size() + 7) / 8, 0);
  for (size_t i = 0; i < valid.size(); i++)
    if (valid[i]) b[i / 8] |= static_cast<uint8_t>(1u << (i % 8));
  return b;
}

// One DictionaryBatch: {validity, buffer 1, buffer 2} in one malloc of exactly the bytes they take, 8-byte aligned, the
// buffer `last` at the very end without padding behind it.
struct Message {
  uint8_t* body = nullptr;
  DecodedBatch b;
  Message(const Bytes& validity, const Bytes& buf1, const Bytes& buf2, int64_t n, int64_t null_count, int last) {
    const Bytes* bufs[3] = {&validity, &buf1, &buf2};
    int order[3] = {0, 1, 2};
    std::swap(order[last], order[2]);
    mi_buffer_span spans[3];
    size_t at = 0;
    for (int k = 0; k < 3; k++) {
      const int w = order[k];
      spans[w].offset = static_cast<int64_t>(at);
      spans[w].length = static_cast<int64_t>(bufs[w]->size());
      at += k < 2 ? (bufs[w]->size() + 7) / 8 * 8 : bufs[w]->size();
    }
    body = static_cast<uint8_t*>(std::malloc(at ? at : 1));
    std::memset(body, 0xEE, at);
    for (int w = 0; w < 3; w++)
      if (!bufs[w]->empty()) std::memcpy(body + spans[w].offset, bufs[w]->data(), bufs[w]->size());
    b.is_dictionary = true;
    b.length = n;
    b.body = body;
    b.body_size = static_cast<int64_t>(at);
    b.column_length.push_back(n);
    b.null_count.push_back(null_count);
    for (int w = 0; w < 3; w++) b.buffers.push_back(spans[w]);
  }
  ~Message() { std::free(body); }
  Message(const Message&) = delete;
};

constexpr size_t kWords = 4;   // more words than any case needs: the rest must come back all ones

// runs the function; true = it raised InternalException
bool Build(const Message& m, int32_t kind, int32_t width, int64_t param, bool keep_values, const DictHostValues* old, uint64_t* words, DictHostValues* out) {
  try {
    BuildDictionaryHost(m.b, kind, width, param, keep_values, old, words, kWords, out);
  } catch (const InternalException&) {
    return true;
  }
  return false;
}

// ---- validity words: word edges, bitmap or none, null_count 0 beside a bitmap
void CheckValidity() {
  for (int64_t n : {0, 1, 63, 64, 65}) {
    std::vector<int> valid(static_cast<size_t>(n));
    std::vector<int32_t> values(static_cast<size_t>(n));
    int64_t nulls = 0;
    for (int64_t i = 0; i < n; i++) {
      valid[static_cast<size_t>(i)] = i % 3 != 0;
      nulls += i % 3 == 0;
      values[static_cast<size_t>(i)] = static_cast<int32_t>(i);
    }
    for (int mode = 0; mode < 3; mode++) {   // 0: bitmap with NULLs, 1: no bitmap, 2: a bitmap with zero bits but null_count 0
      current = "validity n=" + std::to_string(n) + " mode " + std::to_string(mode);
      const Message m(mode == 1 ? Bytes() : Bitmap(valid), Raw(values), Bytes(), n, mode == 0 ? nulls : 0, /*last*/ 0);
      uint64_t words[kWords] = {1, 2, 3, 4};
      DictHostValues out;
      Expect(!Build(m, MI_K_COPY, 4, 0, false, nullptr, words, &out), "a clean dictionary builds");
      const bool nulls_count = mode == 0;
      for (int64_t i = 0; i < static_cast<int64_t>(kWords) * 64; i++) {
        const bool expect = i < n ? (!nulls_count || i % 3 != 0) : true;   // past the values every bit is set, the one at n too
        Expect(((words[i >> 6] >> (i & 63)) & 1) == (expect ? 1u : 0u), "validity bit", i);
      }
      Expect(static_cast<int64_t>(out.host_valid.size()) == n, "host_valid has one entry per value", static_cast<long long>(out.host_valid.size()));
      for (int64_t i = 0; i < n; i++) Expect((out.host_valid[static_cast<size_t>(i)] != 0) == (!nulls_count || i % 3 != 0), "host_valid", i);
      Expect(out.host_strings.empty() && out.host_values.empty(), "an integer dictionary keeps no values on the host");
      // the same words, written out: valid when i mod 3 != 0 is the 12-bit pattern 0xDB6 from bit 0 upward
      if (mode == 0 && n == 64) Expect(words[0] == 0x6DB6DB6DB6DB6DB6ull && words[1] == ~0ull, "64 values fill word 0; the extra NULL entry lands in a new word");
      if (mode == 0 && n == 65) Expect(words[0] == 0x6DB6DB6DB6DB6DB6ull && words[1] == ~0ull, "value 64 (valid) is bit 0 of word 1");
      if (mode == 0 && n == 63) Expect(words[0] == 0xEDB6DB6DB6DB6DB6ull, "63 values: bit 63 stays set for the caller to clear");
      if (mode == 0 && n == 1) Expect(words[0] == ~1ull, "one NULL value");
      if (mode != 0 && n > 0) Expect(words[0] == ~0ull, "without NULLs every bit is set");
    }
  }
}

// ---- replace and delta
void CheckDelta() {
  current = "delta 63 + 2";
  DictHostValues old;
  for (int i = 0; i < 63; i++) old.host_valid.push_back(i % 5 != 1);
  const Message m(Bitmap({0, 1}), Raw(std::vector<int32_t>{7, 8}), Bytes(), 2, 1, 0);
  uint64_t words[kWords];
  DictHostValues out;
  Expect(!Build(m, MI_K_COPY, 4, 0, false, &old, words, &out), "a delta builds");
  Expect(out.host_valid.size() == 65, "old entries then new ones");
  for (int i = 0; i < 63; i++) Expect(((words[0] >> i) & 1) == (i % 5 != 1 ? 1u : 0u), "old bits first", i);
  Expect(((words[0] >> 63) & 1) == 0 && (words[1] & 1) == 1 && words[1] == ~0ull, "the new bits follow: entry 63 NULL, entry 64 valid, the bit at 65 left set");
  current = "replace";
  DictHostValues again;
  Expect(!Build(m, MI_K_COPY, 4, 0, false, nullptr, words, &again), "a replacement builds");
  Expect(again.host_valid.size() == 2 && (words[0] & 3) == 2 && (words[0] | 3) == ~0ull, "a replacement starts from nothing");
}

// ---- strings
void CheckStrings() {
  const std::string payload = "a" "hello, dictionary of strings";   // "a", "", NULL (empty range), the long one
  const std::vector<std::string> want = {"a", "", "", "hello, dictionary of strings"};
  const Bytes validity = Bitmap({1, 1, 0, 1}), data(payload.begin(), payload.end());
  uint64_t words[kWords];
  for (int wide = 0; wide < 2; wide++) {
    current = wide ? "STR64" : "STR32";
    const Bytes offsets = wide ? Raw(std::vector<int64_t>{0, 1, 1, 1, 29}) : Raw(std::vector<int32_t>{0, 1, 1, 1, 29});
    const int32_t kind = wide ? MI_K_STR64 : MI_K_STR32;
    for (int last = 1; last <= 2; last++) {   // the offsets at the end of the body, then the payload
      const Message m(validity, offsets, data, 4, 1, last);
      DictHostValues out;
      Expect(!Build(m, kind, 16, 0, false, nullptr, words, &out), "clean strings build");
      Expect(out.host_strings == want, "the values, an empty string and a NULL string among them");
      Expect(out.host_valid == std::vector<char>({1, 1, 0, 1}) && (words[0] & 0x1F) == 0x1B, "validity of the strings");
      // a delta keeps the old strings in front
      DictHostValues more;
      const Message m2(Bytes(), wide ? Raw(std::vector<int64_t>{0, 2}) : Raw(std::vector<int32_t>{0, 2}), Bytes({'z', 'z'}), 1, 0, last);
      Expect(!Build(m2, kind, 16, 0, false, &out, words, &more), "a string delta builds");
      std::vector<std::string> all = want;
      all.push_back("zz");
      Expect(more.host_strings == all && more.host_valid == std::vector<char>({1, 1, 0, 1, 1}), "old strings then new ones");
    }
    // damaged twins of the same message
    const Bytes decreasing = wide ? Raw(std::vector<int64_t>{0, 1, 0, 1, 29}) : Raw(std::vector<int32_t>{0, 1, 0, 1, 29});
    const Bytes negative = wide ? Raw(std::vector<int64_t>{-1, 1, 1, 1, 29}) : Raw(std::vector<int32_t>{-1, 1, 1, 1, 29});
    const Bytes past = wide ? Raw(std::vector<int64_t>{0, 1, 1, 1, 30}) : Raw(std::vector<int32_t>{0, 1, 1, 1, 30});
    const Bytes shorter = wide ? Raw(std::vector<int64_t>{0, 1, 1, 1}) : Raw(std::vector<int32_t>{0, 1, 1, 1});
    const Bytes all_valid = Bitmap({1, 1, 1, 1});
    DictHostValues out;
    { const Message m(all_valid, decreasing, data, 4, 0, 2); Expect(Build(m, kind, 16, 0, false, nullptr, words, &out), "decreasing offsets raise"); }
    { const Message m(all_valid, negative, data, 4, 0, 2); Expect(Build(m, kind, 16, 0, false, nullptr, words, &out), "a negative offset raises"); }
    { const Message m(all_valid, past, data, 4, 0, 2); Expect(Build(m, kind, 16, 0, false, nullptr, words, &out), "a last offset past the payload raises"); }
    { const Message m(all_valid, shorter, data, 4, 0, 1); Expect(Build(m, kind, 16, 0, false, nullptr, words, &out), "an offsets buffer one entry short raises"); }
    { const Message m(all_valid, Bytes(), data, 4, 0, 1); Expect(Build(m, kind, 16, 0, false, nullptr, words, &out), "no offsets buffer at all raises"); }
    { const Message m(Bytes(), Bytes(), Bytes(), 0, 0, 1); out = DictHostValues(); Expect(!Build(m, kind, 16, 0, false, nullptr, words, &out) && out.host_strings.empty(), "an empty string dictionary needs no offsets"); }
  }
  current = "FIXED_BINARY";
  const Bytes fixed = {'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i'};
  {
    const Message m(Bitmap({1, 0, 1}), fixed, Bytes(), 3, 1, 1);
    DictHostValues out;
    Expect(!Build(m, MI_K_FIXED_BINARY, 16, 3, false, nullptr, words, &out), "clean fixed-size binary builds");
    Expect(out.host_strings == std::vector<std::string>({"abc", "", "ghi"}), "fixed-size values, NULL as empty");
  }
  {
    const Message m(Bytes(), Bytes(fixed.begin(), fixed.end() - 1), Bytes(), 3, 0, 1);
    DictHostValues out;
    Expect(Build(m, MI_K_FIXED_BINARY, 16, 3, false, nullptr, words, &out), "a fixed-size values buffer one byte short raises");
  }
}

// ---- fixed-width values kept for filters
void CheckValues() {
  uint64_t words[kWords];
  // numpy.array(h, numpy.uint16).view(numpy.float16).astype(numpy.float32).view(numpy.uint32): +-0, the smallest and the largest
  // subnormal, the smallest normal, +-65504, +-inf, NaNs with their payload, and three ordinary values
  const struct { uint16_t h; uint32_t f; } table[] = {
      {0x0000, 0x00000000u}, {0x8000, 0x80000000u}, {0x0001, 0x33800000u}, {0x03FF, 0x387FC000u}, {0x8001, 0xB3800000u}, {0x0400, 0x38800000u},
      {0x7BFF, 0x477FE000u}, {0xFBFF, 0xC77FE000u}, {0x7C00, 0x7F800000u}, {0xFC00, 0xFF800000u}, {0x7E00, 0x7FC00000u}, {0xFE01, 0xFFC02000u},
      {0x7C01, 0x7F802000u}, {0x3C00, 0x3F800000u}, {0xC000, 0xC0000000u}, {0x3555, 0x3EAAA000u}};
  const size_t nt = sizeof(table) / sizeof(table[0]);
  current = "float16";
  for (size_t i = 0; i < nt; i++) Expect(HalfToFloatBits(table[i].h) == table[i].f, "HalfToFloatBits against numpy", table[i].h, HalfToFloatBits(table[i].h));
  // and every half that is a number against the value its fields spell (ldexp: no shared arithmetic)
  for (uint32_t h = 0; h < 65536; h++) {
    const uint32_t e = (h >> 10) & 31, man = h & 1023;
    if (e == 31) continue;
    const float v = (h & 0x8000 ? -1.0f : 1.0f) * (e ? std::ldexp(1.0f + man / 1024.0f, static_cast<int>(e) - 15) : std::ldexp(static_cast<float>(man), -24));
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    Expect(HalfToFloatBits(static_cast<uint16_t>(h)) == bits, "HalfToFloatBits against ldexp", h);
  }
  {
    std::vector<uint16_t> halves;
    for (size_t i = 0; i < nt; i++) halves.push_back(table[i].h);
    const Message m(Bytes(), Raw(halves), Bytes(), static_cast<int64_t>(nt), 0, 1);
    DictHostValues out;
    Expect(!Build(m, MI_K_HALF_FLOAT, 4, 0, true, nullptr, words, &out), "clean float16 values build");
    Expect(out.host_values.size() == nt * 4, "4 bytes per widened value");
    for (size_t i = 0; i < nt && out.host_values.size() == nt * 4; i++) Expect(std::memcmp(out.host_values.data() + 4 * i, &table[i].f, 4) == 0, "widened value", static_cast<long long>(i));
    // a delta of two more behind them
    const Message m2(Bitmap({1, 0}), Raw(std::vector<uint16_t>{0x3C00, 0x7BFF}), Bytes(), 2, 1, 1);
    DictHostValues more;
    Expect(!Build(m2, MI_K_HALF_FLOAT, 4, 0, true, &out, words, &more), "a float16 delta builds");
    Expect(more.host_values.size() == (nt + 2) * 4 && std::memcmp(more.host_values.data(), out.host_values.data(), nt * 4) == 0, "old values in front");
    const uint32_t tail[2] = {0x3F800000u, 0x477FE000u};   // (the value of a NULL entry is stored as it is; host_valid says it does not count)
    Expect(more.host_values.size() == (nt + 2) * 4 && std::memcmp(more.host_values.data() + nt * 4, tail, 8) == 0, "new values behind");
    Expect(more.host_valid.size() == nt + 2 && more.host_valid[nt] == 1 && more.host_valid[nt + 1] == 0, "validity of the delta");
    // one element short, next to the clean twin above
    halves.pop_back();
    const Message m3(Bytes(), Raw(halves), Bytes(), static_cast<int64_t>(nt), 0, 1);
    DictHostValues bad;
    Expect(Build(m3, MI_K_HALF_FLOAT, 4, 0, true, nullptr, words, &bad), "a float16 values buffer one element short raises");
    // not kept unless a filter can compare the column
    DictHostValues none;
    Expect(!Build(m, MI_K_HALF_FLOAT, 4, 0, false, nullptr, words, &none) && none.host_values.empty(), "keep_values false keeps none");
  }
  current = "float64";
  {
    const std::vector<double> v = {0.0, -0.0, 1.5, -2.25e300, 4.9e-324};
    const Message m(Bytes(), Raw(v), Bytes(), 5, 0, 1);
    DictHostValues out;
    Expect(!Build(m, MI_K_COPY, 8, 0, true, nullptr, words, &out), "clean float64 values build");
    Expect(out.host_values == Raw(v), "float64 values are kept as stored");
    const Bytes raw = Raw(v);
    const Message m2(Bytes(), Bytes(raw.begin(), raw.begin() + 32), Bytes(), 5, 0, 1);
    DictHostValues bad;
    Expect(Build(m2, MI_K_COPY, 8, 0, true, nullptr, words, &bad), "a float64 values buffer one element short raises");
  }
  current = "128-bit";
  {
    Bytes v(48);
    for (size_t i = 0; i < v.size(); i++) v[i] = static_cast<uint8_t>(i * 7 + 1);
    const Message m(Bytes(), v, Bytes(), 3, 0, 1);
    DictHostValues out;
    Expect(!Build(m, MI_K_COPY, 16, 0, true, nullptr, words, &out), "clean 128-bit values build");
    Expect(out.host_values == v, "128-bit values are kept as stored");
    const Message m2(Bytes(), Bytes(v.begin(), v.end() - 16), Bytes(), 3, 0, 1);
    DictHostValues bad;
    Expect(Build(m2, MI_K_COPY, 16, 0, true, nullptr, words, &bad), "a 128-bit values buffer one element short raises");
  }
}

// ---- a bitmap one byte short, next to its clean twin
void CheckShortBitmap() {
  current = "short bitmap";
  std::vector<int> valid(9, 1);
  valid[8] = 0;
  const std::vector<int32_t> values(9, 5);
  uint64_t words[kWords];
  DictHostValues out;
  { const Message m(Bitmap(valid), Raw(values), Bytes(), 9, 1, 0); Expect(!Build(m, MI_K_COPY, 4, 0, false, nullptr, words, &out) && (words[0] & 0x1FF) == 0xFF, "two bitmap bytes for nine values"); }
  { const Message m(Bytes(1, 0xFF), Raw(values), Bytes(), 9, 1, 0); Expect(Build(m, MI_K_COPY, 4, 0, false, nullptr, words, &out), "a bitmap one byte short raises"); }
  current = "words";
  {   // the destination words are checked too: 200 values need four words, three are given
    const Message m(Bytes(), Raw(std::vector<int32_t>(200, 1)), Bytes(), 200, 0, 1);
    bool raised = false;
    try {
      BuildDictionaryHost(m.b, MI_K_COPY, 4, 0, false, nullptr, words, 3, &out);
    } catch (const InternalException&) {
      raised = true;
    }
    Expect(raised, "too few destination words raise");
  }
}

void CheckKinds() {
  current = "kinds";
  for (int32_t k : {MI_K_COPY, MI_K_BOOL, MI_K_DEC128, MI_K_STR32, MI_K_STR64, MI_K_FIXED_BINARY, MI_K_NARROW, MI_K_HALF_FLOAT}) Expect(DictionaryKindIsFlat(k), "a flat kind is admitted", k);
  for (int32_t k : {MI_K_DICT, MI_K_RUN_END}) Expect(!DictionaryKindIsFlat(k), "a kind with children or a dictionary of its own is refused", k);
  Expect(IsStringKind(MI_K_STR32) && IsStringKind(MI_K_STR64) && IsStringKind(MI_K_FIXED_BINARY) && !IsStringKind(MI_K_COPY), "string kinds");
}

}  // namespace

int main() {
  CheckValidity();
  CheckDelta();
  CheckStrings();
  CheckValues();
  CheckShortBitmap();
  CheckKinds();
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
