// Host-side plan facts for the tests (no GPU): one line per argument.
//   <p>[:<spec>]  ->  p=<p> n=<n> q=<q> c=<C> a_fast=<fused factor bound>   (make_plan without tables)
//   ts:<p>        ->  ts p=<p> n=<transform_size(p)>                        (0: no admissible size)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "plan.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a.rfind("ts:", 0) == 0) {
      const uint32_t p = uint32_t(std::strtoul(a.c_str() + 3, nullptr, 10));
      const size_t n = mi355::transform_size(p);
      std::printf("ts p=%u n=%zu\n", p, n == size_t(-1) ? size_t(0) : n);
      continue;
    }
    const size_t colon = a.find(':');
    const uint32_t p = uint32_t(std::strtoul(a.substr(0, colon).c_str(), nullptr, 10));
    const std::string spec = colon == std::string::npos ? std::string() : a.substr(colon + 1);
    const mi355::Plan pl = mi355::make_plan(p, spec.c_str(), false);
    std::printf("p=%u n=%zu q=%u c=%u a_fast=%u\n", p, pl.n, pl.q, pl.C, pl.a_fast);
  }
  return 0;
}
