// like_match_check.cpp -- csrc/like_match.hpp alone under ASan + UBSan (g++ -fsanitize=address,undefined), run by
// tests/test_like_match_host.py as a child process.  Every pattern and every row sits in a heap allocation of exactly its
// length, so a read one byte past either ends the program.  One line per (op, pattern, row):
//   <op> <pattern in hex, or -> <row in hex, or -> <1 | 0 | E<what Compile answered>>
// which the test compares with Python's own evaluation.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "like_match.hpp"

using namespace miarrow::likematch;

namespace {
struct Exact {   // a heap copy of exactly size() bytes
  uint8_t* p;
  uint32_t n;
  explicit Exact(const std::string& s) : p(new uint8_t[s.size()]), n(static_cast<uint32_t>(s.size())) { std::memcpy(p, s.data(), s.size()); }
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

std::string Hex(const std::string& s) {
  if (s.empty()) return "-";
  static const char* d = "0123456789abcdef";
  std::string out;
  for (unsigned char c : s) {
    out.push_back(d[c >> 4]);
    out.push_back(d[c & 15]);
  }
  return out;
}
}  // namespace

int main() {
  const std::string long_row = std::string(150, 'x') + "needle" + std::string(150, 'y') + "nee";
  const std::vector<std::string> rows = {
      "", "a", "b", "ab", "ba", "aa", "aab", "aaab", "abab", "aba", "ababa", "abababa", "abc", "abbc", "abcabc", "abcab",
      "special", "xspecial", "specialx", "xspe", "cialx", "spe", "twelve bytes", "thirteen byte", "a%b", "a_b", "100%", "%", "_",
      std::string("\x00", 1), std::string("a\x00" "b", 3), std::string("\xff\xfe\x00\xff", 4), "\xff", std::string(300, 'a'),
      std::string(299, 'a') + "b", long_row, "the special requests of the customer", "requests are special"};
  const std::vector<std::string> likes = {
      "", "%", "%%", "a", "a%", "%a", "%a%", "a%a", "ab%bc", "%ab%ab%", "%abc", "abc%", "%aba%ba%", "%%a%%b%%", "%a%b%", "%aab%",
      "%abab%", "%special%requests%", "%spe%cial%", "%special", "special%", "a%b%a%b%a%b%a%b", "%a%b%a%b%a%b%a%b%", "a%b%a%b%a%b%a%b%a",
      "a_b", "_", "%_%", "\\%", "100\\%", "%needle%", "%needle%nee", "x%nee", "%xneedle%", std::string("%\x00%", 3), "%\xff", "%xy%"};
  const std::vector<std::string> needles = {
      "", "a", "b", "ab", "aab", "abab", "%", "_", "a%b", "a_b", "special", "spe", "cial", "needle", "nee", "yne", "xn",
      std::string("\x00", 1), "\xff", std::string("\x00\xff", 2), std::string("\xfe\x00", 2), "twelve bytes", "thirteen byte", "thirteen bytes",
      std::string(300, 'a'), std::string(301, 'a'), std::string(298, 'a') + "b", std::string(16, 'a'), std::string(17, 'a')};
  struct Case { int32_t op; const std::vector<std::string>* patterns; };
  const Case cases[] = {{kOpLike, &likes}, {kOpNotLike, &likes}, {kOpContains, &needles}, {kOpEndsWith, &needles}, {7, &needles}};
  for (const Case& c : cases)
    for (const std::string& pattern : *c.patterns) {
      const Exact pat(pattern);
      Pattern compiled;
      const int rc = Compile(c.op, pat.p, pat.n, &compiled);
      for (const std::string& r : rows) {
        const Exact row(r);
        if (rc != kCompiled) std::printf("%d %s %s E%d\n", c.op, Hex(pattern).c_str(), Hex(r).c_str(), rc);
        else std::printf("%d %s %s %d\n", c.op, Hex(pattern).c_str(), Hex(r).c_str(), Passes(compiled, pat.p, row.p, row.n) ? 1 : 0);
      }
    }
  return 0;
}
