// Host-side plan facts for the tests (no GPU): one line per argument.
//   <p>[:<spec>]           ->  p=<p> n=<n> q=<q> c=<C> a_fast=<fused factor bound>   (make_plan without tables)
//   ts:<p>                 ->  ts p=<p> n=<transform_size(p)>                        (0: no admissible size)
//   k:<p>[:<spec>][@<sel>] ->  k <p>:<spec>@<sel> r5= m1= m2= c= split5= cols=<variant> rows=<variant>
//                              (choose_kernels with MI355_KERNELS = sel; no @: unset)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "plan.hpp"

// (in the order of plan.hpp ColKernels / RowKernels)
static const char* kCols[] = {"generic", "split", "radix8-512", "radix8-1024", "radix8-2048", "radix4-pairs", "radix4-planes", "radix5-1280", "radix5-2560"};
static const char* kRows[] = {"generic", "radix4-pairs", "radix4-planes", "rows4096", "rows8192", "rows2048-one", "rows2048-two"};

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a.rfind("ts:", 0) == 0) {
      const uint32_t p = uint32_t(std::strtoul(a.c_str() + 3, nullptr, 10));
      const size_t n = mi355::transform_size(p);
      std::printf("ts p=%u n=%zu\n", p, n == size_t(-1) ? size_t(0) : n);
      continue;
    }
    if (a.rfind("k:", 0) == 0) {
      const size_t at = a.find('@');
      const std::string ps = a.substr(2, at == std::string::npos ? std::string::npos : at - 2);
      const size_t colon = ps.find(':');
      const std::string spec = colon == std::string::npos ? std::string() : ps.substr(colon + 1);
      const mi355::Plan pl = mi355::make_plan(uint32_t(std::strtoul(ps.c_str(), nullptr, 10)), spec.c_str(), false);
      const std::string sel = at == std::string::npos ? std::string() : a.substr(at + 1);
      const mi355::KernelChoice k = mi355::choose_kernels(pl, at == std::string::npos ? nullptr : sel.c_str());
      std::printf("k %s r5=%u m1=%u m2=%u c=%u split5=%d cols=%s rows=%s\n", a.c_str() + 2, pl.r5, pl.M1, pl.M2, pl.C, int(pl.split5),
                  kCols[int(k.cols)], kRows[int(k.rows)]);
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
