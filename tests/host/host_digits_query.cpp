// The host digit arithmetic of both engines (prmers_amd/csrc/host_digits.hpp) for the tests (no GPU): one query per line of stdin, Python
// integers judge the answers (tests/test_host_digits.py).
//   carry <p> <n> <d_0> ... <d_{n-1}>   digits in natural order, weakly carried (anything below 2^63)
//       -> carry  <n digits>    strong_carry
//          ones   <0|1>         is_all_ones of those
//          res64  <u64>         res64_of_head of the first min(n, 8) of them
//          words  <wc words>    pack_words into wc = ceil(p / 32) words
//          unpack <n digits>    unpack_words of those words
//   fold <p> <w_0> ... <w_{wc-1}>       -> fold <wc words>   fold_words_mod_mp
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host_digits.hpp"

namespace hd = mi355::host_digits;

template <class T>
static void print(const char* tag, const std::vector<T>& v) {
  std::printf("%s", tag);
  for (const T x : v) std::printf(" %" PRIu64, uint64_t(x));
  std::printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    uint32_t p = 0;
    if (!(in >> op >> p)) continue;
    const size_t wc = (size_t(p) + 31) / 32;
    if (op == "fold") {
      std::vector<uint32_t> w(wc);
      for (auto& x : w) in >> x;
      if (!in) { std::fprintf(stderr, "fold: expected %zu words\n", wc); return 2; }
      hd::fold_words_mod_mp(w.data(), wc, p);
      print("fold", w);
    } else if (op == "carry") {
      size_t n = 0;
      in >> n;
      std::vector<uint64_t> d(n);
      for (auto& x : d) in >> x;
      if (!in || n == 0) { std::fprintf(stderr, "carry: expected n digits\n"); return 2; }
      const std::vector<uint8_t> width = hd::digit_widths(p, n);
      hd::strong_carry(d.data(), width);
      print("carry", d);
      std::printf("ones %d\n", hd::is_all_ones(d.data(), width) ? 1 : 0);
      std::printf("res64 %" PRIu64 "\n", hd::res64_of_head(d.data(), width, n < 8 ? n : 8));
      std::vector<uint32_t> w(wc);
      hd::pack_words(d.data(), width, w.data(), wc);
      print("words", w);
      std::vector<uint64_t> back(n);
      hd::unpack_words(w.data(), wc, width, back.data());
      print("unpack", back);
    } else {
      std::fprintf(stderr, "unknown query '%s'\n", op.c_str());
      return 2;
    }
  }
  return 0;
}
