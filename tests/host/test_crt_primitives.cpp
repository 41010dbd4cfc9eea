// The arithmetic of the second field family (crt_field.hpp, crt_arith.hpp) on the host, against unsigned __int128 arithmetic mod M61 / M31:
// scalars over any 64-bit value, the limb-wise complex products at their operand bounds (M61, M61 + 7, limb edges), the lazy and the generic
// radix-2/4/8 butterflies with every input at the maximum, the odd-axis DFTs with the engine's own root tables, and DigitWalk for every digit
// of a few sizes.  The cases and the checks are those of the device self-test (selftest_cases.hpp), here through the host forms.
#include <cstdio>
#include "selftest_cases.hpp"
using namespace mi355::cases;
template <class Fam> static int run(const char* name) {
  const std::string e = run_on_host<Fam>();
  if (!e.empty()) { printf("%s: %s\n", name, e.c_str()); return 1; }
  return 0;
}
int main() {
  int bad = 0;
  bad += run<CrtScalar>("scalars"); bad += run<CrtCmul>("cmul"); bad += run<CrtBfly>("bfly"); bad += run<CrtOdd>("dft_odd"); bad += run<CrtWalk>("DigitWalk");
  printf(bad ? "FAIL %d\n" : "OK %d\n", bad);
  return bad != 0;
}
