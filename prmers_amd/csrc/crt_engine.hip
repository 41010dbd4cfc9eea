// Resident engine of the squaring x <- x^2 a mod 2^p - 1 over GF(M61^2) x GF(M31^2) with a prime-factor axis of radix 1, 3 or 9 (SURVEY.md
// 8f row N1): size policy, root tables, the register file and the host side of every operation.  Host code only: the kernels and their
// launchers are crt_kernels.hip (crt_kernels.hpp), the device-side canonical form is canon.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "canon.hpp"
#include "crt_arith.hpp"
#include "crt_engine.hpp"
#include "crt_kernels.hpp"
#include "host_digits.hpp"
#include "plan.hpp"

namespace mi355 {
namespace {

using crt::F31; using crt::F61; using crt::M31; using crt::M61;

void chk(hipError_t e, const char* what) { if (e != hipSuccess) throw std::runtime_error(std::string("crt engine: ") + what + ": " + hipGetErrorString(e)); }

using crt::pow31; using crt::pow61;

// an element of exact order 2^k in the norm-1 subgroup of Z/p[i] (order p + 1 = 2^61 resp. 2^31): (t + i)^((p - 1) 2^(bits - k)) for the first t
// that gives exact order 2^k; the exponent is applied as (p - 1) first (z^(p-1) = conj(z) / z has norm 1), then by squaring
template <class F>
typename F::C root_2k(unsigned k, unsigned bits) {
  using C = typename F::C;
  for (typename F::S t = 2;; ++t) {
    const C g{t, 1};
    // g^(p-1): p - 1 = 2^bits - 2
    C r{1, 0}, b = g;
    for (unsigned i = 0; i < bits; ++i) { if (i >= 1) r = crt::cmul<F>(r, b); b = crt::cmul<F>(b, b); }   // sum of 2^i, i = 1 .. bits-1 = 2^bits - 2
    for (unsigned i = k; i < bits; ++i) r = crt::cmul<F>(r, r);                                          // ^ 2^(bits - k)
    C z = r;
    for (unsigned i = 1; i < k; ++i) z = crt::cmul<F>(z, z);
    if (z.re == F::M - 1 && z.im == 0) return r;   // r^(2^(k-1)) = -1: exact order 2^k
  }
}

// r^t for the odd t < 8 that makes r^(2^(ln-3)) the wanted 8th root (the four primitive 8th roots are the odd powers of any one)
template <class F>
typename F::C normalise_root(typename F::C r, unsigned ln, typename F::C want) {
  using C = typename F::C;
  C w8 = r;
  for (unsigned i = 3; i < ln; ++i) w8 = crt::cmul<F>(w8, w8);
  C p = w8;
  const C w8sq = crt::cmul<F>(w8, w8);
  for (unsigned t = 1; t < 8; t += 2) {
    if (p.re == want.re && p.im == want.im) {
      C out{1, 0};
      for (unsigned i = 0; i < t; ++i) out = crt::cmul<F>(out, r);
      return out;
    }
    p = crt::cmul<F>(p, w8sq);
  }
  throw std::runtime_error("crt engine: no 8th root of the expected form");
}

}  // namespace

size_t crt_transform_size(uint32_t p, uint32_t odd) {   // m2:479-503: smallest odd 2^ln with log2(n) + 2 (p / n + 1) < 92
  for (unsigned ln = 3; ln <= 28; ++ln) {
    const size_t n = size_t(odd) << ln;
    if (n > p) break;
    if (std::log2(double(n)) + 2.0 * (double(p) / double(n) + 1.0) < 92.0) return n;
  }
  return 0;
}

// Automatic choice between the stock power-of-two size and the prime-factor sizes, the reference's policy (README.md:888-926,
// third_party/aevum/src/FFTConfig.cpp:425-520): radix 9 when the stock / PFA size ratio reaches 1.60, else radix 3 when it reaches 1.30,
// else the stock plan.  With the size rule above the candidates below the stock 2^k are 9 2^(k-4) (ratio 1.778) and 3 2^(k-2) (1.333).
// (The reference's exponent boundaries come from its measured bits-per-word tables, fftbpw.h, which admit ~39 bits per word where the
// worst-case rule used here admits ~34: same policy, boundaries of this engine's own capacity rule; tests/test_host_logic.py.)
uint32_t crt_auto_radix(uint32_t p, size_t* words) {
  const size_t stock = crt_transform_size(p, 1), n3 = crt_transform_size(p, 3), n9 = crt_transform_size(p, 9);
  uint32_t odd = 1;
  size_t n = stock;
  if (n9 && stock && double(stock) / double(n9) >= 1.60) { odd = 9; n = n9; }
  else if (n3 && stock && double(stock) / double(n3) >= 1.30) { odd = 3; n = n3; }
  else if (!stock) { if (n9) { odd = 9; n = n9; } else if (n3) { odd = 3; n = n3; } }
  if (words) *words = n;
  return n ? odd : 0;
}

struct CrtEngine::Impl {
  crt::Geom g;
  crt::Grid gr;
  CanonGeom cg{};                 // the digit layout as canon.hip sees it (natural order)
  crt::CrtKernels kernels{};      // chosen once from the grid, MI355_CRT_KERNELS and MI355_CRT_TUNE
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[kKernels + 1] = {};
  std::vector<void*> owned;       // every device allocation of the engine; freed by ~Impl
  struct Register {
    uint64_t* x = nullptr;        // [n] digits, logical order, weakly carried
    F61::C* i61 = nullptr;        // packed spectrum of a multiplicand (set_multiplicand), allocated on first use
    F31::C* i31 = nullptr;
    bool image = false;           // holds a multiplicand image instead of digits
  };
  std::vector<Register> regs;
  uint64_t* scratch = nullptr;    // [n] digits: temporary of addsub
  crt::Work Z{};                  // the transform's work arrays
  crt::FastTables T{};            // omega_m^k (u61 / u31) for every kernel set, the other tables for the radix-8 one
  uint64_t* w61 = nullptr;        // [n] + [n] unweighted residues between k_back and k_crt_runs_linked (two-kernel form only)
  uint32_t* w31 = nullptr;
  uint64_t* edge = nullptr;       // edge words of the carry sweep (crt::edge_words)
  std::vector<uint8_t> width;
  // device-side canonical form (canon.hip, SURVEY.md 8f N4 extended to this family): scratch + two outputs of n digits, allocated on first use
  void* canon = nullptr;
  uint64_t* canon_out[2] = {nullptr, nullptr};
  bool host_carry = false;       // MI355_HOST_CARRY=1: the round-2 host paths (A/B tests)
  // bits by which a register's digits may exceed their widths: 0 after a carry sweep, +1 per digit-wise addition; a transform needs
  // log2(n) + 2 (w + excess) < 92 and relaxes the register first (one local carry pass) when that fails
  std::vector<int> excess;

  template <class V> V* alloc(size_t count) {
    void* q = nullptr;
    chk(hipMalloc(&q, count * sizeof(V)), "hipMalloc");
    owned.push_back(q);
    return static_cast<V*>(q);
  }
  size_t slots() const { return size_t(gr.odd) * gr.h; }
  void ensure_image(Register& r) {   // the planes of a multiplicand image
    if (r.i61) return;
    r.i61 = alloc<F61::C>(slots()); r.i31 = alloc<F31::C>(slots());
  }
  ~Impl() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* q : owned) (void)hipFree(q);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

const char* CrtEngine::stage_name(size_t k) {
  static const char* names[kKernels] = {"k_front", "k_rows_fwd", "k_pointwise", "k_rows_inv", "k_back", "k_crt_carry"};
  return k < kKernels ? names[k] : "";
}

CrtEngine::CrtEngine(uint32_t p, size_t reg_count, uint32_t odd, size_t n_forced, int device, const char* spec) : im_(new Impl) {
  Impl& im = *im_;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available: the MI355X engine has no CPU fallback");
  if (odd != 1 && odd != 3 && odd != 9) throw std::runtime_error("crt engine: odd radix must be 1, 3 or 9");
  if (reg_count == 0 || reg_count > 64) throw std::runtime_error("crt engine: register count must be 1 .. 64");
  const size_t n = n_forced ? n_forced : crt_transform_size(p, odd);
  if (!n) throw std::runtime_error("crt engine: no admissible transform size for this exponent");
  if (std::log2(double(n)) + 2.0 * (double(p) / double(n) + 1.0) >= 92.0) throw std::runtime_error("crt engine: transform too small for this exponent");
  im.g = crt::make_geom(p, n, odd, 1);
  // the carry sweep hands a run's carry to the next run and lets it die inside that run's kRun digits: (kRun - 1) words must hold a
  // coefficient of up to 92 bits (every size the reference's rule picks has more than 20 bits per word)
  if (uint64_t(im.g.q) * (crt::kRun - 1) < 100) throw std::runtime_error("crt engine: fewer than 15 bits per word at this transform size");
  crt::Grid& gr = im.gr;
  gr.odd = odd; gr.ln = im.g.ln; gr.m = 1u << gr.ln; gr.h = gr.m >> 1; gr.logh = gr.ln - 1;
  if (gr.ln < 3) throw std::runtime_error("crt engine: power-of-two axis too short");
  uint32_t logH2 = std::min<uint32_t>(10, gr.logh);
  if (spec && std::strncmp(spec, "h2=", 3) == 0) logH2 = uint32_t(std::atoi(spec + 3));
  if (logH2 < 1 || logH2 > std::min<uint32_t>(10, gr.logh) || gr.logh - logH2 > 11) throw std::runtime_error("crt engine: bad row split");
  gr.logH2 = logH2; gr.logH1 = gr.logh - logH2;
  gr.minv = 0;
  if (odd > 1) for (uint32_t y = 1; y < odd; ++y) if ((uint64_t(gr.m % odd) * y) % odd == 1) gr.minv = y;
  {
    const crt::OddTables ot = crt::make_odd_tables(odd);   // crt_arith.hpp: the tables the CPU and device tests of dft_odd use too
    for (unsigned k = 0; k < 9; ++k) { gr.r61[k] = ot.r61[k]; gr.r61i[k] = ot.r61i[k]; gr.r31[k] = ot.r31[k]; gr.r31i[k] = ot.r31i[k]; }
    gr.c3_61 = ot.c3_61; gr.c3_31 = ot.c3_31;
    gr.mm = gr.m % odd;
    gr.pm = uint32_t((uint64_t(p) * gr.m) % n);
    gr.lpm61 = uint32_t(uint64_t(im.g.l61) * (gr.pm % 61) % 61); gr.lpm31 = uint32_t(uint64_t(im.g.l31) * (gr.pm % 31) % 31);
  }
  { const char* tn = std::getenv("MI355_CRT_TUNE"); gr.tune = tn ? uint32_t(std::atoi(tn)) : 0u; }
  gr.s61 = pow61((uint64_t(odd) * gr.h) % M61, M61 - 2); gr.s31 = pow31(uint32_t((uint64_t(odd) * gr.h) % M31), M31 - 2);
  im.kernels = crt::choose_kernels(gr, std::getenv("MI355_CRT_KERNELS"));

  im.device = device;
  chk(hipSetDevice(device), "hipSetDevice");
  chk(hipStreamCreateWithFlags(&im.stream, hipStreamNonBlocking), "stream");
  for (auto& e : im.ev) chk(hipEventCreate(&e), "event");
  chk(crt::configure(im.kernels), "lds attribute");
  const size_t h = gr.h;
  im.regs.resize(reg_count);
  im.scratch = im.alloc<uint64_t>(n);
  for (auto& r : im.regs) { r.x = im.alloc<uint64_t>(n); chk(hipMemset(r.x, 0, n * 8), "memset"); }
  im.Z.Z61 = im.alloc<F61::C>(im.slots()); im.Z.Z31 = im.alloc<F31::C>(im.slots());
  if (!im.kernels.back_fused) { im.w61 = im.alloc<uint64_t>(n); im.w31 = im.alloc<uint32_t>(n); }
  im.edge = im.alloc<uint64_t>(crt::edge_words(im.g, gr));
  {
    // omega_m^k, k <= h.  The generator is rotated (an odd power keeps its order) so that omega_m^(m/8) is (1 + i) / sqrt 2 = (1 + i) 2^30
    // resp. (1 + i) 2^15: the radix-8 steps of crt_rows.hpp multiply by that root with an add, a sub and two bit rotations
    std::vector<F61::C> u61(h + 1); std::vector<F31::C> u31(h + 1);
    const F61::C w61 = normalise_root<F61>(root_2k<F61>(gr.ln, 61), gr.ln, F61::C{uint64_t(1) << 30, uint64_t(1) << 30});
    const F31::C w31 = normalise_root<F31>(root_2k<F31>(gr.ln, 31), gr.ln, F31::C{1u << 15, 1u << 15});
    F61::C a{1, 0}; F31::C b{1, 0};
    for (size_t k = 0; k <= h; ++k) { u61[k] = a; u31[k] = b; a = crt::cmul<F61>(a, w61); b = crt::cmul<F31>(b, w31); }
    // count entries omega_m^(x stride) per field (beyond h through omega_m^h = -1)
    std::vector<F61::C> t61; std::vector<F31::C> t31;
    auto upload = [&](size_t count, size_t stride, const F61::C*& d61, const F31::C*& d31) {
      t61.resize(count); t31.resize(count);
      for (size_t x = 0; x < count; ++x) {
        const size_t e = x * stride;
        t61[x] = e <= h ? u61[e] : crt::cneg<F61>(u61[e - h]); t31[x] = e <= h ? u31[e] : crt::cneg<F31>(u31[e - h]);
      }
      F61::C* q61 = im.alloc<F61::C>(count); F31::C* q31 = im.alloc<F31::C>(count);
      chk(hipMemcpy(q61, t61.data(), count * 16, hipMemcpyHostToDevice), "copy"); chk(hipMemcpy(q31, t31.data(), count * 8, hipMemcpyHostToDevice), "copy");
      d61 = q61; d31 = q31;
    };
    upload(h + 1, 1, im.T.u61, im.T.u31);
    if (im.kernels.radix8) {   // omega_L^x = omega_m^(x m / L) for the two pass lengths (x < L), omega_m^(H1 k2), the two-level table
      const size_t H1 = size_t(1) << gr.logH1, H2 = size_t(1) << gr.logH2, m = size_t(gr.m);
      upload(H1, m / H1, im.T.w1_61, im.T.w1_31);
      upload(H2, m / H2, im.T.w2_61, im.T.w2_31);
      upload(H2, H1, im.T.v61, im.T.v31);
      upload(1024, 1, im.T.lo61, im.T.lo31);              // m >= 2^12 on this path
      upload(m >> 10, 1024, im.T.hi61, im.T.hi31);
    }
  }
  im.width = host_digits::digit_widths(p, n);
  im.cg = CanonGeom::natural(p, uint32_t(n), odd);
  im.excess.assign(reg_count, 0);
  { const char* hc = std::getenv("MI355_HOST_CARRY"); im.host_carry = hc && hc[0] == '1'; }
}
CrtEngine::~CrtEngine() = default;

size_t CrtEngine::size() const { return im_->g.n; }
uint32_t CrtEngine::exponent() const { return im_->g.p; }
std::string CrtEngine::describe() const {
  const crt::Grid& gr = im_->gr;
  return "crt-hip:n=" + std::to_string(im_->g.n) + ":odd=" + std::to_string(gr.odd) + ":m=" + std::to_string(gr.m) + ":h1=" + std::to_string(1u << gr.logH1) + ":h2=" +
         std::to_string(1u << gr.logH2) + (im_->kernels.radix8 ? ":radix8" : ":generic");
}
size_t CrtEngine::algorithmic_bytes() const {   // digits r + w, 4 row passes r + w, and (two-kernel form only) the carry sweep's input w + r
  return size_t(im_->g.n) * (8 + 8 + 8 * 12 + (im_->kernels.back_fused ? 0 : 2 * 12));
}

void CrtEngine::sync() {
  chk(hipSetDevice(im_->device), "hipSetDevice");
  chk(hipStreamSynchronize(im_->stream), "sync");
  chk(hipGetLastError(), "kernel");
}

// forward transform of register `reg` into the work arrays Z (front + forward columns; the rows are part of the next stage), then
//   mode 0: square, inverse, carry sweep back into `reg` (x a)
//   mode 1: rows forward only -> the packed spectrum becomes the image of register `other` (set_multiplicand)
//   mode 2: multiply by the image of register `other`, inverse, carry sweep back into `reg` (x a)
// Timed runs record an event around each of the kKernels stages of kernel_name.
void CrtEngine::launch_transform(size_t reg, int mode, size_t other, uint32_t a, bool timed) {
  Impl& im = *im_;
  const crt::Grid& gr = im.gr;
  const crt::CrtKernels& k = im.kernels;
  crt::Geom g = im.g; g.a = a;
  hipStream_t s = im.stream;
  uint64_t* x = im.regs[reg].x;
  F61::C* i61 = mode ? im.regs[other].i61 : nullptr; F31::C* i31 = mode ? im.regs[other].i31 : nullptr;
  int e = 0;
  auto mark = [&] { if (timed) chk(hipEventRecord(im.ev[e++], s), "event"); };
  mark();
  crt::launch_front(g, gr, x, im.Z, s);
  mark();
  if (k.radix8) {   // stages: k_rows_fwd = forward columns, k_pointwise = the fused row kernel, k_rows_inv = inverse columns
    crt::launch_cols(gr, im.T, k.cols_split, false, im.Z, s);
    mark();
    crt::launch_mid(gr, im.T, mode, im.Z, i61, i31, s);
    if (mode == 1) return;
    mark();
    crt::launch_cols(gr, im.T, k.cols_split, true, im.Z, s);
    mark();
  } else {
    crt::launch_rows_generic(gr, im.T, false, im.Z, s);
    mark();
    if (mode == 1) {
      chk(hipMemcpyAsync(i61, im.Z.Z61, im.slots() * 16, hipMemcpyDeviceToDevice, s), "copy");
      chk(hipMemcpyAsync(i31, im.Z.Z31, im.slots() * 8, hipMemcpyDeviceToDevice, s), "copy");
      return;
    }
    crt::launch_pointwise(gr, im.T, im.Z, i61, i31, s);
    mark();
    crt::launch_rows_generic(gr, im.T, true, im.Z, s);
    mark();
  }
  if (k.back_fused) {   // stage k_back: the fused kernel; stage k_crt_carry: the range edges
    crt::launch_back_carry(g, gr, im.Z, x, im.edge, s);
    mark();
    crt::launch_range_edges(g, gr, x, im.edge, s);
    mark();
    return;
  }
  crt::launch_back(gr, im.Z, im.w61, im.w31, s);
  mark();
  crt::launch_carry_linked(g, im.w61, im.w31, x, im.edge, s);
  mark();
}

size_t CrtEngine::reg_count() const { return im_->regs.size(); }

bool CrtEngine::holds_image(size_t reg) const { return im_->regs[reg].image; }

// Headroom of the transform: the convolution sums stay below M61 M31 ~ 2^92 while log2(n) + 2 (w + excess) < 92 (the size rule is that
// bound at excess 0).  A register that has been through digit-wise additions is relaxed first when it would not fit: one local carry
// pass (canon.hip k_local) brings digits of w + e bits below 2^w + 2^e.
void CrtEngine::ensure_headroom(size_t reg) {
  Impl& im = *im_;
  const int e = im.excess[reg];
  if (e == 0) return;
  const double bits = std::log2(double(im.g.n)) + 2.0 * (double(im.g.q) + 1.0 + double(e));
  if (bits < 92.0 && e < 8) return;
  chk(canon_local_pass(im.cg, im.regs[reg].x, im.scratch, im.stream), "relax");
  std::swap(im.regs[reg].x, im.scratch);
  im.excess[reg] = 0;
}

// canonical digits of `reg` on the device (strong carry with wrap-around, 2^p - 1 -> 0 and flag [0]); slot 0 / 1
uint64_t* CrtEngine::canon_digits(size_t reg, int slot) {
  Impl& im = *im_;
  chk(hipSetDevice(im.device), "hipSetDevice");
  if (!im.canon) {
    const size_t sb = (canon_scratch_bytes<uint64_t>(im.cg) + 255) & ~size_t(255);
    im.canon = im.alloc<unsigned char>(sb + 2 * size_t(im.g.n) * 8);
    im.canon_out[0] = reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(im.canon) + sb);
    im.canon_out[1] = im.canon_out[0] + im.g.n;
    chk(hipMemsetAsync(canon_flags<uint64_t>(im.cg, im.canon), 0, 16 * 4, im.stream), "memset");
  }
  chk(canon_launch(im.cg, im.regs[reg].x, im.canon_out[slot], im.canon, im.stream), "canon");
  return im.canon_out[slot];
}
// flags: [0] all ones, [1] a digit too wide for the 0/1 chain (fall back to the host carry), [2] compare differs; cleared for the next use
bool CrtEngine::canon_flags_ok(uint32_t (&flags)[4]) {
  Impl& im = *im_;
  uint32_t* df = canon_flags<uint64_t>(im.cg, im.canon);
  chk(hipMemcpyAsync(flags, df, 16, hipMemcpyDeviceToHost, im.stream), "copy");
  chk(hipMemsetAsync(df, 0, 16 * 4, im.stream), "memset");
  chk(hipStreamSynchronize(im.stream), "sync");
  return flags[1] == 0;
}

void CrtEngine::square_mul(size_t reg, uint32_t a) {
  need_residue(reg, "square_mul"); need_factor(a, "square_mul");
  chk(hipSetDevice(im_->device), "hipSetDevice");
  ensure_headroom(reg);
  launch_transform(reg, 0, 0, a, false);
  im_->excess[reg] = 0;
}

// dst <- the transformed image of src (engine::set_multiplicand, engine.h:53); dst may be src
void CrtEngine::set_multiplicand(size_t dst, size_t src) {
  Impl& im = *im_;
  need_residue(src, "set_multiplicand"); need_register(dst, "set_multiplicand");
  chk(hipSetDevice(im.device), "hipSetDevice");
  Impl::Register& d = im.regs[dst];
  im.ensure_image(d);
  ensure_headroom(src);
  launch_transform(src, 1, dst, 1, false);
  d.image = true;
}

// dst <- dst * src * a with src a multiplicand image (engine::mul, engine.h:60)
void CrtEngine::mul(size_t dst, size_t src, uint32_t a) {
  Impl& im = *im_;
  need_residue(dst, "mul"); need_image(src, "mul"); need_factor(a, "mul");
  chk(hipSetDevice(im.device), "hipSetDevice");
  ensure_headroom(dst);
  launch_transform(dst, 2, src, a, false);
  im.excess[dst] = 0;
}

void CrtEngine::copy(size_t dst, size_t src) {
  Impl& im = *im_;
  need_register(dst, "copy"); need_register(src, "copy");
  if (dst == src) return;
  chk(hipSetDevice(im.device), "hipSetDevice");
  Impl::Register& d = im.regs[dst]; const Impl::Register& r = im.regs[src];
  if (r.image) {
    im.ensure_image(d);
    chk(hipMemcpyAsync(d.i61, r.i61, im.slots() * 16, hipMemcpyDeviceToDevice, im.stream), "copy");
    chk(hipMemcpyAsync(d.i31, r.i31, im.slots() * 8, hipMemcpyDeviceToDevice, im.stream), "copy");
  } else {
    chk(hipMemcpyAsync(d.x, r.x, size_t(im.g.n) * 8, hipMemcpyDeviceToDevice, im.stream), "copy");
    im.excess[dst] = im.excess[src];
  }
  d.image = r.image;
}

// dst <- dst + src, digit-wise on weakly carried digits (engine::add, engine.h:64)
void CrtEngine::add(size_t dst, size_t src) {
  Impl& im = *im_;
  need_residue(dst, "add"); need_residue(src, "add");
  chk(hipSetDevice(im.device), "hipSetDevice");
  crt::launch_add_digits(im.regs[dst].x, im.regs[src].x, im.g.n, im.stream);
  im.excess[dst] = std::max(im.excess[dst], im.excess[src]) + 1;
  if (im.excess[dst] >= 8) ensure_headroom(dst);   // repeated additions without a transform in between
}

// the canonical digits of `src` on the device (slot 1), through the host when the device chain reports a digit too wide for it
const uint64_t* CrtEngine::canonical_on_device(size_t src) {
  Impl& im = *im_;
  const uint64_t* c = canon_digits(src, 1);
  uint32_t flags[4];
  if (canon_flags_ok(flags) && !im.host_carry) return c;
  std::vector<uint64_t> d(im.g.n);
  get_digits_host(src, d.data());
  chk(hipMemcpy(im.canon_out[1], d.data(), size_t(im.g.n) * 8, hipMemcpyHostToDevice), "copy");
  return im.canon_out[1];
}

// dst <- dst - src = dst + (2^p - 1 - src): the digit-wise complement of the canonical form of src, taken on the device
void CrtEngine::sub_reg(size_t dst, size_t src) {
  Impl& im = *im_;
  need_residue(dst, "sub_reg"); need_residue(src, "sub_reg");
  const uint64_t* c = canonical_on_device(src);
  chk(canon_add_complement(im.cg, im.regs[dst].x, c, im.stream), "sub_reg");
  im.excess[dst] = im.excess[dst] + 1;
  if (im.excess[dst] >= 8) ensure_headroom(dst);
}

// sum -> sum_out (and sum_copy), difference -> diff_out (and diff_copy); -1: not wanted.  a and b may be among the outputs.
void CrtEngine::addsub(long sum_out, long sum_copy, long diff_out, long diff_copy, size_t a, size_t b) {
  Impl& im = *im_;
  need_residue(a, "addsub"); need_residue(b, "addsub");
  const long outs[4] = {sum_out, sum_copy, diff_out, diff_copy};
  for (int i = 0; i < 4; ++i) {
    if (outs[i] >= long(im.regs.size())) throw std::runtime_error("addsub: register index out of range");
    for (int j = 0; j < i; ++j) if (outs[i] >= 0 && outs[i] == outs[j]) throw std::runtime_error("addsub: output registers must differ");
  }
  if ((sum_copy >= 0 && sum_out < 0) || (diff_copy >= 0 && diff_out < 0)) throw std::runtime_error("addsub: copy output without a primary output");
  chk(hipSetDevice(im.device), "hipSetDevice");
  const size_t n = im.g.n, bytes = n * 8;
  // scratch = a + (2^p - 1 - b): the complement of the canonical digits of b (taken on the device, as in sub_reg), before anything is overwritten
  const int ea = im.excess[a], eb = im.excess[b];
  if (diff_out >= 0) {
    const uint64_t* c = canonical_on_device(b);
    chk(hipMemcpyAsync(im.scratch, im.regs[a].x, bytes, hipMemcpyDeviceToDevice, im.stream), "copy");
    chk(canon_add_complement(im.cg, im.scratch, c, im.stream), "addsub");
  }
  if (sum_out >= 0) {
    if (size_t(sum_out) == b) {   // b + a
      crt::launch_add_digits(im.regs[b].x, im.regs[a].x, im.g.n, im.stream);
    } else {
      if (size_t(sum_out) != a) chk(hipMemcpyAsync(im.regs[sum_out].x, im.regs[a].x, bytes, hipMemcpyDeviceToDevice, im.stream), "copy");
      crt::launch_add_digits(im.regs[sum_out].x, im.regs[b].x, im.g.n, im.stream);
    }
    im.regs[sum_out].image = false; im.excess[sum_out] = std::max(ea, eb) + 1;
    if (sum_copy >= 0) { chk(hipMemcpyAsync(im.regs[sum_copy].x, im.regs[sum_out].x, bytes, hipMemcpyDeviceToDevice, im.stream), "copy"); im.regs[sum_copy].image = false; im.excess[sum_copy] = im.excess[sum_out]; }
  }
  if (diff_out >= 0) {
    chk(hipMemcpyAsync(im.regs[diff_out].x, im.scratch, bytes, hipMemcpyDeviceToDevice, im.stream), "copy");
    im.regs[diff_out].image = false; im.excess[diff_out] = ea + 1;
    if (diff_copy >= 0) { chk(hipMemcpyAsync(im.regs[diff_copy].x, im.scratch, bytes, hipMemcpyDeviceToDevice, im.stream), "copy"); im.regs[diff_copy].image = false; im.excess[diff_copy] = ea + 1; }
  }
}

void CrtEngine::set_u32(size_t reg, uint32_t a) {
  Impl& im = *im_;
  need_register(reg, "set");
  chk(hipSetDevice(im.device), "hipSetDevice");
  chk(hipMemsetAsync(im.regs[reg].x, 0, size_t(im.g.n) * 8, im.stream), "memset");
  if (a) crt::launch_set_small(im.g, im.regs[reg].x, a, im.stream);
  im.regs[reg].image = false; im.excess[reg] = 0;
}
void CrtEngine::sub_u32(size_t reg, uint32_t a) {
  Impl& im = *im_;
  need_residue(reg, "sub");
  chk(hipSetDevice(im.device), "hipSetDevice");
  if (a) crt::launch_sub_small(im.g, im.regs[reg].x, a, im.stream);
}

void CrtEngine::set_raw_digits(size_t reg, const uint64_t* d, size_t count) {
  Impl& im = *im_;
  need_register(reg, "set_digits");
  if (count != im.g.n) throw std::runtime_error("set_digits: wrong digit count");
  for (size_t j = 0; j < count; ++j) if (d[j] >> 62) throw std::runtime_error("set_digits: digit out of range");
  chk(hipSetDevice(im.device), "hipSetDevice");
  chk(hipStreamSynchronize(im.stream), "sync");
  chk(hipMemcpy(im.regs[reg].x, d, count * 8, hipMemcpyHostToDevice), "copy");
  im.regs[reg].image = false;
  int e = 0;   // callers may hand over digits wider than their slots (weakly carried vectors)
  for (size_t j = 0; j < count; ++j) { const int bits = d[j] ? 64 - __builtin_clzll(d[j]) : 0; e = std::max(e, bits - int(im.width[j])); }
  im.excess[reg] = e;
}

// digits as they are on the device (weakly carried) or canonical: strong carry with wrap-around, 2^p - 1 stays all ones.
// The canonical form is made on the device (canon.hip); MI355_HOST_CARRY=1 or a device chain that reports an over-wide digit use the
// host loop below (the reference's way: engine_gpu.h:1534-1561).
void CrtEngine::get_raw_digits(size_t reg, uint64_t* d, size_t count, bool canonical) {
  Impl& im = *im_;
  need_residue(reg, "get_digits");
  if (count != im.g.n) throw std::runtime_error("get_digits: wrong digit count");
  if (!canonical) {
    sync();
    chk(hipMemcpy(d, im.regs[reg].x, count * 8, hipMemcpyDeviceToHost), "copy");
    return;
  }
  if (!im.host_carry) {
    const uint64_t* c = canon_digits(reg, 0);
    chk(hipMemcpyAsync(d, c, count * 8, hipMemcpyDeviceToHost, im.stream), "copy");
    uint32_t flags[4];
    if (canon_flags_ok(flags)) {
      if (flags[0]) for (size_t j = 0; j < count; ++j) d[j] = host_digits::ones(im.width[j]);
      return;
    }
  }
  get_digits_host(reg, d);
}
void CrtEngine::get_digits_host(size_t reg, uint64_t* d) {
  Impl& im = *im_;
  sync();
  chk(hipMemcpy(d, im.regs[reg].x, size_t(im.g.n) * 8, hipMemcpyDeviceToHost), "copy");
  host_digits::strong_carry(d, im.width);
}

void CrtEngine::get_digits(size_t reg, uint64_t* d, size_t count) {
  Impl& im = *im_;
  get_raw_digits(reg, d, count, true);
  for (size_t j = 0; j < count; ++j) {
    if (im.width[j] > 32) throw std::runtime_error("get_digits: this transform size has words of more than 32 bits, which the value | width << 32 encoding cannot hold (use get_words)");
    d[j] |= uint64_t(im.width[j]) << 32;
  }
}
void CrtEngine::set_digits(size_t reg, const uint64_t* d, size_t count) {
  Impl& im = *im_;
  if (count != im.g.n) throw std::runtime_error("set_digits: wrong digit count");
  std::vector<uint64_t> v(count);
  for (size_t j = 0; j < count; ++j) {
    if ((d[j] >> 32) != im.width[j]) throw std::runtime_error("set_digits: digit width mismatch");
    v[j] = d[j] & 0xffffffffull;
  }
  set_raw_digits(reg, v.data(), count);
}

// canonical little-endian 32-bit words of the residue, 2^p - 1 -> 0 (what the plugin ABI exchanges: EngineApi.cpp:210-218).  Packed on the
// device from the canonical digits (canon.hip k_pack_words, which sees 2^p - 1 as zeros): ceil(p / 32) words cross PCIe, not n u64 digits.
void CrtEngine::get_words(size_t reg, uint32_t* w, size_t count) {
  Impl& im = *im_;
  const size_t need = word_count();
  if (count < need) throw std::runtime_error("get_words: buffer too small");
  need_residue(reg, "get_words");
  if (!im.host_carry) {
    const uint64_t* c = canon_digits(reg, 0);
    uint32_t* dw = static_cast<uint32_t*>(im.canon);   // the pipeline's first work array (8 n bytes >= the words) is free once the digits are out
    chk(canon_pack_words(im.cg, c, dw, im.stream), "pack");
    chk(hipMemcpyAsync(w, dw, need * 4, hipMemcpyDeviceToHost, im.stream), "copy");
    uint32_t flags[4];
    if (canon_flags_ok(flags)) { std::memset(w + need, 0, (count - need) * 4); return; }
  }
  std::vector<uint64_t> d(im.g.n);
  get_digits_host(reg, d.data());
  host_digits::pack_words(d.data(), im.width, w, count);
}
// reg <- the value of `count` little-endian 32-bit words (< 2^p; bits beyond p must be zero): the words go up and are cut into digits on the
// device (canon.hip k_unpack_words); MI355_HOST_CARRY=1 cuts them on the host
void CrtEngine::set_words(size_t reg, const uint32_t* w, size_t count) {
  Impl& im = *im_;
  const size_t n = im.g.n, need = word_count();
  if (count > need) for (size_t k = need; k < count; ++k) if (w[k]) throw std::runtime_error("set_words: value does not fit 2^p");
  if (count >= need && (im.g.p & 31) && (w[need - 1] >> (im.g.p & 31))) throw std::runtime_error("set_words: value does not fit 2^p");
  if (!im.host_carry) {
    need_register(reg, "set_words");
    chk(hipSetDevice(im.device), "hipSetDevice");
    uint32_t* dw = reinterpret_cast<uint32_t*>(im.scratch);   // 8 n bytes: room for the words of every admissible size
    if (count < need) chk(hipMemsetAsync(dw, 0, need * 4, im.stream), "memset");
    chk(hipMemcpyAsync(dw, w, std::min(count, need) * 4, hipMemcpyHostToDevice, im.stream), "copy");
    chk(canon_unpack_words(im.cg, dw, im.regs[reg].x, im.stream), "unpack");
    chk(hipStreamSynchronize(im.stream), "sync");
    im.regs[reg].image = false;
    im.excess[reg] = 0;
    return;
  }
  std::vector<uint64_t> d(n);
  host_digits::unpack_words(w, count, im.width, d.data());
  set_raw_digits(reg, d.data(), n);
}
// the low 64 bits of the canonical residue: canonical form on the device, the first digits cross PCIe
uint64_t CrtEngine::res64(size_t reg) {
  Impl& im = *im_;
  need_residue(reg, "res64");
  if (!im.host_carry) {
    const uint64_t* c = canon_digits(reg, 0);
    const size_t have = std::min<size_t>(im.g.n, 8);     // widths are at least 15 bits here (constructor): 8 digits hold more than 64 bits
    uint64_t head[8];
    chk(hipMemcpyAsync(head, c, have * 8, hipMemcpyDeviceToHost, im.stream), "copy");
    uint32_t flags[4];
    if (canon_flags_ok(flags)) {
      if (flags[0]) return 0;                             // 2^p - 1 = 0
      return host_digits::res64_of_head(head, im.width, have);
    }
  }
  std::vector<uint32_t> w(word_count() + 2, 0);
  get_words(reg, w.data(), w.size());
  return uint64_t(w[0]) | (uint64_t(w[1]) << 32);
}
// same value mod 2^p - 1 (engine::is_equal, engine.h:148): both canonical forms and the comparison on the device, 16 bytes cross PCIe
// (the reference reads both registers back: engine.h:148-157)
bool CrtEngine::equal(size_t a, size_t b) {
  Impl& im = *im_;
  need_residue(a, "is_equal"); need_residue(b, "is_equal");
  if (!im.host_carry) {
    const uint64_t* ca = canon_digits(a, 0);
    const uint64_t* cb = canon_digits(b, 1);
    chk(canon_compare(ca, cb, im.g.n, canon_flags<uint64_t>(im.cg, im.canon) + 2, im.stream), "compare");
    uint32_t flags[4];
    if (canon_flags_ok(flags)) return flags[2] == 0;      // (2^p - 1 is written as 0 by both, so 0 == 2^p - 1 holds)
  }
  return equal_words(a, b);
}

size_t CrtEngine::register_data_size() const { return size_t(im_->g.n) * 12 + 8; }
void CrtEngine::get_data(size_t src, void* data, size_t size) {
  Impl& im = *im_;
  need_register(src, "get_data");
  if (size != register_data_size()) throw std::runtime_error("get_data: size mismatch");
  sync();
  unsigned char* out = static_cast<unsigned char*>(data);
  const size_t n = im.g.n, slots = size_t(im.gr.odd) * im.gr.h;   // 2 slots' worth of words per slot: 16 + 8 bytes = 12 bytes a word
  std::memset(out, 0, size);
  const Impl::Register& r = im.regs[src];
  if (r.image) { chk(hipMemcpy(out, r.i61, slots * 16, hipMemcpyDeviceToHost), "copy"); chk(hipMemcpy(out + slots * 16, r.i31, slots * 8, hipMemcpyDeviceToHost), "copy"); }
  else chk(hipMemcpy(out, r.x, n * 8, hipMemcpyDeviceToHost), "copy");
  const uint64_t tag = data_tag(r.image);
  std::memcpy(out + n * 12, &tag, 8);
}
// Digits lie in logical order: (p, n, odd) say everything.  A multiplicand image is the packed spectrum as the row stage leaves it -- the
// radix-8 row kernel (crt_rows.hpp) or the generic passes, on the H1 x H2 split of this engine -- so those belong to an image's tag.
uint64_t CrtEngine::data_tag(bool image) const {
  const crt::Grid& gr = im_->gr;
  return layout_tag(image, kFamilyCrt, im_->g.p, im_->g.n, gr.odd, image ? gr.logH1 : 0u, image ? gr.logH2 : 0u, 0u,
                    image ? (im_->kernels.radix8 ? 2u : 1u) : 0u);
}
void CrtEngine::check_data(const void* data, size_t size) const {
  if (size != register_data_size()) throw std::runtime_error("set_data: size mismatch");
  uint64_t tag = 0;
  std::memcpy(&tag, static_cast<const unsigned char*>(data) + size_t(im_->g.n) * 12, 8);
  if (tag <= 1) throw std::runtime_error("set_data: the image carries no layout fingerprint (written by an earlier version of the library)");
  if (tag != data_tag((tag & 1) != 0))
    throw std::runtime_error(std::string("set_data: ") + ((tag & 1) ? "multiplicand image of another exponent, size or kernel set (" : "register image of another exponent or size (") + describe() + " here)");
}
void CrtEngine::set_data(size_t dst, const void* data, size_t size) {
  Impl& im = *im_;
  need_register(dst, "set_data");
  check_data(data, size);
  const unsigned char* in = static_cast<const unsigned char*>(data);
  const size_t n = im.g.n, slots = size_t(im.gr.odd) * im.gr.h;
  uint64_t tag = 0;
  std::memcpy(&tag, in + n * 12, 8);
  tag &= 1;   // what the register holds; the rest is the fingerprint check_data has just compared
  sync();
  Impl::Register& r = im.regs[dst];
  if (tag == 1) {
    im.ensure_image(r);
    chk(hipMemcpy(r.i61, in, slots * 16, hipMemcpyHostToDevice), "copy"); chk(hipMemcpy(r.i31, in + slots * 16, slots * 8, hipMemcpyHostToDevice), "copy");
  } else {
    chk(hipMemcpy(r.x, in, n * 8, hipMemcpyHostToDevice), "copy");
    int e = 0;   // the image holds weakly carried digits, possibly after additions: measure what it needs
    for (size_t j = 0; j < n; ++j) { uint64_t v; std::memcpy(&v, in + j * 8, 8); const int bits = v ? 64 - __builtin_clzll(v) : 0; e = std::max(e, bits - int(im.width[j])); }
    im.excess[dst] = e;
  }
  r.image = tag == 1;
}

void CrtEngine::time_square_mul(size_t reg, uint32_t a, uint32_t sub, size_t iters, double* total_ms, double* kernel_ms, size_t kernel_count) {
  Impl& im = *im_;
  if (sub) throw std::runtime_error("time_square_mul: no deferred subtraction on the crt family");
  need_residue(reg, "time_square_mul");
  chk(hipSetDevice(im.device), "hipSetDevice");
  std::vector<double> acc(kKernels, 0.0);
  double total = 0;
  for (size_t it = 0; it < iters; ++it) {
    launch_transform(reg, 0, 0, a, true);
    chk(hipEventSynchronize(im.ev[kKernels]), "sync");
    for (int k = 0; k < kKernels; ++k) { float ms = 0; chk(hipEventElapsedTime(&ms, im.ev[k], im.ev[k + 1]), "elapsed"); acc[k] += ms; }
    float ms = 0; chk(hipEventElapsedTime(&ms, im.ev[0], im.ev[kKernels]), "elapsed"); total += ms;
  }
  chk(hipGetLastError(), "kernel");
  if (total_ms) *total_ms = total;   // sum over the iterations, like Engine::time_square_mul
  for (size_t k = 0; k < kernel_count && k < size_t(kKernels); ++k) if (kernel_ms) kernel_ms[k] = iters ? acc[k] / double(iters) : 0;
}

}  // namespace mi355
