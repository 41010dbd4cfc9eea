// Tag words of raw register images for the tests (no GPU): one line per argument.
//   <p>[:<spec>][@<sel>] ->  tag <p>:<spec>@<sel> r5= m1= m2= c= split5= cols=<n> rows=<n> digits=<hex> image=<hex>
//                            (register_tag of make_plan + choose_kernels with MI355_KERNELS = sel; no @: unset)
//   crt:<p>:<n>:<odd>:<logH1>:<logH2>:<radix8> -> tag crt:... digits=<hex> image=<hex>   (layout_tag as CrtEngine::data_tag fills it)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "plan.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a.rfind("crt:", 0) == 0) {
      unsigned long v[6] = {0, 0, 0, 0, 0, 0};
      size_t pos = 4;
      for (int k = 0; k < 6 && pos <= a.size(); ++k) {
        const size_t e = a.find(':', pos);
        v[k] = std::strtoul(a.substr(pos, e == std::string::npos ? std::string::npos : e - pos).c_str(), nullptr, 10);
        pos = e == std::string::npos ? a.size() + 1 : e + 1;
      }
      const uint64_t d = mi355::layout_tag(false, mi355::kFamilyCrt, uint32_t(v[0]), v[1], uint32_t(v[2]), 0, 0, 0, 0);
      const uint64_t m = mi355::layout_tag(true, mi355::kFamilyCrt, uint32_t(v[0]), v[1], uint32_t(v[2]), uint32_t(v[3]), uint32_t(v[4]), 0, v[5] ? 2u : 1u);
      std::printf("tag %s digits=%016llx image=%016llx\n", a.c_str(), (unsigned long long)d, (unsigned long long)m);
      continue;
    }
    const size_t at = a.find('@');
    const std::string ps = a.substr(0, at);
    const size_t colon = ps.find(':');
    const std::string spec = colon == std::string::npos ? std::string() : ps.substr(colon + 1);
    const std::string sel = at == std::string::npos ? std::string() : a.substr(at + 1);
    const mi355::Plan pl = mi355::make_plan(uint32_t(std::strtoul(ps.c_str(), nullptr, 10)), spec.c_str(), false);
    const mi355::KernelChoice k = mi355::choose_kernels(pl, at == std::string::npos ? nullptr : sel.c_str());
    std::printf("tag %s r5=%u m1=%u m2=%u c=%u split5=%d cols=%d rows=%d digits=%016llx image=%016llx\n", a.c_str(), pl.r5, pl.M1, pl.M2, pl.C, int(pl.split5),
                int(k.cols), int(k.rows), (unsigned long long)mi355::register_tag(pl, k, false), (unsigned long long)mi355::register_tag(pl, k, true));
  }
  return 0;
}
