// gf::add_lazy_any through its host form: the case family of the device self-test (selftest_cases.hpp GfLazySum), both operands over
// [0, 2^64), against 128-bit integers.
#include <cstdio>

#include "selftest_cases.hpp"

int main() {
  const std::string e = mi355::cases::run_on_host<mi355::cases::GfLazySum>();
  if (!e.empty()) { std::printf("FAIL %s\n", e.c_str()); return 1; }
  std::printf("OK\n");
  return 0;
}
