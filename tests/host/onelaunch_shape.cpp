// The work-group shape of the one-launch kernel for the tests (no GPU): one line per argument.
//   <p>:<lanes>[:<spec>]  ->  p=<p> lanes=<B> n= m1= m2= c= r5= sum_fast= tl=<threads per lane> k=<lanes per group> groups= lds=<bytes per group>
// (make_plan without tables on "<spec>,lanes=<B>,onelaunch", then plan.hpp onelaunch_shape)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "plan.hpp"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t c1 = a.find(':'), c2 = c1 == std::string::npos ? c1 : a.find(':', c1 + 1);
    if (c1 == std::string::npos) { std::fprintf(stderr, "usage: onelaunch_shape <p>:<lanes>[:<spec>] ...\n"); return 2; }
    const uint32_t p = uint32_t(std::strtoul(a.substr(0, c1).c_str(), nullptr, 10));
    const std::string lanes = a.substr(c1 + 1, c2 == std::string::npos ? std::string::npos : c2 - c1 - 1);
    const std::string spec = (c2 == std::string::npos ? std::string() : a.substr(c2 + 1) + ",") + "lanes=" + lanes + ",onelaunch";
    const mi355::Plan pl = mi355::make_plan(p, spec.c_str(), false);
    const mi355::OneLaunchShape s = mi355::onelaunch_shape(pl.m, pl.r5, pl.lanes);
    std::printf("p=%u lanes=%u n=%zu m1=%u m2=%u c=%u r5=%u sum_fast=%d tl=%u k=%u groups=%u lds=%zu\n", p, pl.lanes, pl.n, pl.M1, pl.M2, pl.C, pl.r5,
                int(pl.sum_fast), s.TL, s.K, s.groups, s.lds);
  }
  return 0;
}
