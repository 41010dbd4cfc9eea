// Device self-test of the arithmetic the kernels are built from: the GF(P) primitives (gf.hpp, gfdft.hpp), their consumers in the radix-8 kernels
// (kernels_v2_common.hpp: dft8p, seam, p2_mul, dft4) and the second field family (crt_field.hpp, crt_arith.hpp).  The device code paths differ
// from the host ones (inline-assembly reductions, borrow-reusing sub, P left for a negated zero; intrinsics and 64-bit shifts in the second family),
// so the case families of selftest_cases.hpp are evaluated on the GPU itself, one lane per case, and checked against 128-bit host arithmetic --
// the second family also word for word against the host evaluation of the same templates.  Reached through mi355_engine_selftest().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "kernels_v2_common.hpp"
#include "selftest_cases.hpp"

namespace mi355 {

namespace {
using namespace cases;

template <class Fam>
__global__ void k_selftest_family(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, const uint64_t* __restrict__ aux, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fam::eval(in + size_t(i) * Fam::IN, out + size_t(i) * Fam::OUT, aux);
}

__global__ void k_selftest_dft4(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t f[4], g[4];
  for (int j = 0; j < 4; ++j) f[j] = g[j] = in[size_t(i) * 4 + j];
  v2::dft4<false>(f[0], f[1], f[2], f[3]); v2::dft4<true>(g[0], g[1], g[2], g[3]);
  for (int j = 0; j < 4; ++j) { out[size_t(i) * 8 + j] = f[j]; out[size_t(i) * 8 + 4 + j] = g[j]; }
}

// eight waves to a work-group, the wave index made scalar as the kernels do, so that the switch of seam is taken wave-uniformly
__global__ void __launch_bounds__(512) k_selftest_chain(const uint64_t* __restrict__ tuples, size_t ntuples, const uint64_t* __restrict__ fac, uint64_t* __restrict__ out) {
  const int g = blockIdx.x * 512 + threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 7);
  const uint64_t* ta = tuples + 8 * GfChain::tuple_of(g, 0, ntuples);
  const uint64_t* tb = tuples + 8 * GfChain::tuple_of(g, 1, ntuples);
  uint64_t* o = out + size_t(g) * GfChain::OUT;
  v2::P2 x[8], y[8];
  uint64_t sw[8];
  for (int k = 0; k < 8; ++k) { x[k] = y[k] = {ta[k], tb[k]}; sw[k] = fac[size_t(g) * 8 + k]; }
  v2::dft8p<false, 1>(x);
  v2::seam<6, false, true>(x, wave);
  for (int k = 0; k < 8; ++k) { o[k] = x[k].a; o[8 + k] = x[k].b; }
  v2::dft8p<false, 2>(x);
  for (int k = 0; k < 8; ++k) { x[k] = v2::p2_mul(x[k], sw[k]); o[16 + k] = x[k].a; o[24 + k] = x[k].b; }
  v2::dft8p<true>(y);
  v2::seam<6, true>(y, wave);
  v2::dft8p<true, 2>(y);
  for (int k = 0; k < 8; ++k) { y[k] = v2::p2_mul(y[k], sw[k]); o[32 + k] = y[k].a; o[40 + k] = y[k].b; }
}

void chk(hipError_t e, const char* what) { if (e != hipSuccess) throw std::runtime_error(std::string("selftest: ") + what + ": " + hipGetErrorString(e)); }

struct DevWords {   // device copy of a word vector (freed on every way out)
  uint64_t* p = nullptr;
  explicit DevWords(size_t n) { chk(hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * 8), "hipMalloc"); }
  explicit DevWords(const std::vector<uint64_t>& v) : DevWords(v.size()) { if (!v.empty()) chk(hipMemcpy(p, v.data(), v.size() * 8, hipMemcpyHostToDevice), "copy"); }
  ~DevWords() { (void)hipFree(p); }
  DevWords(const DevWords&) = delete;
  DevWords& operator=(const DevWords&) = delete;
  void fetch(std::vector<uint64_t>& v, const char* what) const { chk(hipMemcpy(v.data(), p, v.size() * 8, hipMemcpyDeviceToHost), what); }
};

// one family: cases up, one lane per case, results down, check; in / out are left for the caller
template <class Fam>
void run_family(const char* name, std::vector<uint64_t>& in, std::vector<uint64_t>& out) {
  std::vector<uint64_t> aux;
  in.clear(); Fam::fill(in); Fam::aux(aux);
  const size_t n = in.size() / Fam::IN;
  out.assign(n * Fam::OUT, 0);
  {
    DevWords din(in), daux(aux), dout(out.size());
    hipLaunchKernelGGL(k_selftest_family<Fam>, dim3(uint32_t((n + 63) / 64)), dim3(64), 0, 0, din.p, dout.p, daux.p, int(n));
    chk(hipGetLastError(), name);
    dout.fetch(out, name);
  }
  if (Fam::kHostEqualsDevice) {   // plain C++ on both sides: the same words
    std::vector<uint64_t> h(Fam::OUT);
    for (size_t i = 0; i < n; ++i) {
      Fam::eval(in.data() + i * Fam::IN, h.data(), aux.data());
      for (int k = 0; k < Fam::OUT; ++k)
        if (h[k] != out[i * Fam::OUT + k])
          throw std::runtime_error(std::string("selftest: ") + name + msg(": device and host evaluation differ, case %zu word %d: %016llx / %016llx", i, k, MI355_X(out[i * Fam::OUT + k]), MI355_X(h[k])));
    }
  }
  const std::string err = Fam::check(in.data(), out.data(), n);
  if (!err.empty()) throw std::runtime_error("selftest: " + err);
}
}  // namespace

// throws std::runtime_error with the first mismatch
void selftest_primitives(int device) {
  chk(hipSetDevice(device), "hipSetDevice");
  std::vector<uint64_t> in, out, tuples, dft8_out;
  run_family<GfScalar>("gf scalars", in, out);
  run_family<GfLazySum>("gf lazy sum", in, out);
  run_family<GfDft8>("gf dft8", tuples, dft8_out);
  {   // v2::dft4
    in.clear(); GfDft4::fill(in);
    const size_t n = in.size() / GfDft4::IN;
    out.assign(n * GfDft4::OUT, 0);
    DevWords din(in), dout(out.size());
    hipLaunchKernelGGL(k_selftest_dft4, dim3(uint32_t((n + 63) / 64)), dim3(64), 0, 0, din.p, dout.p, int(n));
    chk(hipGetLastError(), "gf dft4");
    dout.fetch(out, "gf dft4");
    const std::string err = GfDft4::check(in.data(), out.data(), n);
    if (!err.empty()) throw std::runtime_error("selftest: " + err);
  }
  {   // the lazy outputs through their consumers
    std::vector<uint64_t> fac; GfChain::factors(fac);
    const size_t ntuples = tuples.size() / 8;
    out.assign(size_t(GfChain::kThreads) * GfChain::OUT, 0);
    DevWords dt(tuples), df(fac), dout(out.size());
    hipLaunchKernelGGL(k_selftest_chain, dim3(GfChain::kThreads / 512), dim3(512), 0, 0, dt.p, ntuples, df.p, dout.p);
    chk(hipGetLastError(), "gf chain");
    dout.fetch(out, "gf chain");
    const std::string err = GfChain::check(tuples.data(), ntuples, fac.data(), out.data(), dft8_out.data());
    if (!err.empty()) throw std::runtime_error("selftest: " + err);
  }
  run_family<CrtScalar>("crt scalars", in, out);
  run_family<CrtCmul>("crt cmul", in, out);
  run_family<CrtBfly>("crt bfly", in, out);
  run_family<CrtOdd>("crt dft_odd", in, out);
  run_family<CrtWalk>("crt DigitWalk", in, out);
}

}  // namespace mi355
