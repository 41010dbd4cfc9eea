// Host-side capacity of the fused multiply-by-sum (no GPU): one line per argument <p>[:<spec>]
//   ->  p=<p> n=<n> q=<q> c=<C> sum_fast=<0|1>        (make_plan without tables; plan.hpp sum_product_ok)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "plan.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t colon = a.find(':');
    const uint32_t p = uint32_t(std::strtoul(a.substr(0, colon).c_str(), nullptr, 10));
    const std::string spec = colon == std::string::npos ? std::string() : a.substr(colon + 1);
    const mi355::Plan pl = mi355::make_plan(p, spec.c_str(), false);
    std::printf("p=%u n=%zu q=%u c=%u sum_fast=%d\n", p, pl.n, pl.q, pl.C, int(pl.sum_fast));
  }
  return 0;
}
