// Case families of the primitive tests, shared by the device self-test (selftest.hip: one lane per case) and the CPU tests
// (tests/host/test_primitives.cpp, test_crt_primitives.cpp: the host forms of the same functions).  A family is
//   IN / OUT   words per case;   fill(in)   the cases (edge lists first, then a seeded sample);   aux(a)   constant words every case reads;
//   eval(in, out, aux)   the functions under test, host + device;   check(in, out, n)   128-bit integer arithmetic, first mismatch as text.
// Rule: a function documented to take a lazy (un-folded) operand is called over [0, 2^64) in that operand; every other operand over its
// documented range including the largest value.  Plain C++ (no HIP needed).
#pragma once
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "crt_arith.hpp"
#include "gfdft.hpp"

namespace mi355 {

void selftest_primitives(int device);   // selftest.hip: every family below on the GPU, one lane per case; throws on the first mismatch

namespace cases {

typedef unsigned __int128 u128;
constexpr uint64_t P = gf::P;

struct Rng {   // the self-test's generator (64-bit LCG)
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s ^ (s >> 29); }
};

inline std::string msg(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline std::string msg(const char* fmt, ...) {
  char buf[400];
  va_list ap; va_start(ap, fmt); std::vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  return buf;
}
#define MI355_X(v) ((unsigned long long)(v))

inline uint64_t gf_mulmod(uint64_t a, uint64_t b) { return uint64_t((u128(a % P) * (b % P)) % P); }
inline const uint64_t* gf_pow2_table() {   // 2^s mod P, s < 192
  static uint64_t t[192];
  if (!t[0]) { t[0] = 1; for (int s = 1; s < 192; ++s) t[s] = uint64_t((u128(t[s - 1]) * 2) % P); }
  return t;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// GF(P) scalars
// ------------------------------------------------------------------------------------------------------------------------------------
// The device multiplication ends in sub32_c / reduce_tail (gf.hpp), which branch on a borrow bw and a carry; this is their integer model,
// used to make sure that the operand list reaches every case: returns bw | carry << 1 | (r >= P) << 2 | c << 3.
inline unsigned mul_tail_case(uint64_t a, uint64_t b) {
  const uint64_t a0 = uint32_t(a), a1 = a >> 32, b0 = uint32_t(b), b1 = b >> 32;
  const uint64_t t0 = a0 * b0, t1 = a0 * b1 + (t0 >> 32);
  const u128 t2w = u128(a1 * b0) + t1;
  const uint64_t t2 = uint64_t(t2w), c = uint64_t(t2w >> 64);
  const uint64_t t3 = a1 * b1 + (t2 >> 32);
  const uint64_t lo = (t2 << 32) | uint32_t(t0), hh = t3 >> 32, hl = uint32_t(t3);
  const unsigned bw = u128(lo) < u128(hh) + c;
  const uint64_t x = lo - hh - c;
  const u128 rw = u128(x) + u128(hl) * 0xffffffffull;
  return bw | unsigned(rw >> 64) << 1 | unsigned(uint64_t(rw) >= P) << 2 | unsigned(c) << 3;
}

template <unsigned... S>
GF_HD void mul_pow2_const(uint64_t x, uint64_t* o, std::integer_sequence<unsigned, S...>) { ((o[S] = gf::mul_pow2(x, S)), ...); }   // s a compile-time constant

struct GfScalar {
  static constexpr int IN = 2, OUT = 7 + 192 + 192;
  static constexpr bool kHostEqualsDevice = false;   // the device forms may leave another representative (P for a negated zero)
  static void aux(std::vector<uint64_t>&) {}
  static void edges(std::vector<uint64_t>& e) {
    e = {0, 1, 2, P - 1, P - 2, P, 0xffffffffull, 0x100000000ull, 0xffffffff00000000ull, 0x8000000000000000ull, 0xfffffffeffffffffull, 0x00000000fffffffeull,
         0x123456789abcdef0ull % P,
         // operands whose products take the rare paths of gf::mul's tail: 2^64 - 1 = (2^32 + 1)(2^32 - 1) (low half >= P, no carry), (P - 1)^2 (borrow
         // out of lo - hh - c), products with an empty low word or an all-ones high word
         0x100000001ull, 0x00000001ffffffffull, 0xfffffffe00000001ull, 0x0000000100000000ull + 0xfffffffeull, 0xffffffff00000000ull - 1, 0x00000000ffff0001ull,
         0xffff0000ffff0001ull,
         // borrow without carry (2^33 2^63: empty low word under a high word), borrow with the carry c of the middle column
         0x200000000ull, 0xc000000000000000ull, 0x7fffffffcull, 0xfffffffdffffffffull,
         // above P: the lazy representatives (P - 1 = 2^64 - 2^32 and P - 2 are in the first row)
         P + 1, P + 0xfffffffeull, 0xffffffffffffffffull, 0xffffffff80000000ull, 0xffffffff00000002ull, 0xfffffffffffffffeull};
  }
  static void fill(std::vector<uint64_t>& in) {
    std::vector<uint64_t> e; edges(e);
    for (uint64_t x : e) for (uint64_t y : e) { in.push_back(x); in.push_back(y); }
    Rng r(0x9e3779b97f4a7c15ull);
    for (int i = 0; i < 4096; ++i) { in.push_back(r.next() % P); in.push_back(r.next() % P); }
    for (int i = 0; i < 1024; ++i) { in.push_back(r.next() | (i & 1 ? 0xffffffff00000000ull : 0)); in.push_back(r.next() % P); }   // lazy first operand
    for (int i = 0; i < 1024; ++i) { in.push_back(r.next() % P); in.push_back(r.next() | (i & 1 ? 0xffffffff00000000ull : 0)); }   // lazy second operand
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    const uint64_t x = in[0], y = in[1];
    o[0] = gf::add(x, y);
    o[1] = gf::sub(x, y);
    o[2] = gf::mul(x, y);
    o[3] = gf::add_lazy(x, y);
    o[4] = gf::fold(x + y);
    o[5] = gf::mul_u32(x, uint32_t(y));
    o[6] = gf::fold(x);
    for (unsigned s = 0; s < 192; ++s) o[7 + s] = gf::mul_pow2(x, s);   // runtime s: every branch of mul_pow2
    mul_pow2_const(x, o + 7 + 192, std::make_integer_sequence<unsigned, 192>());
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    const uint64_t* p2 = gf_pow2_table();
    unsigned seen = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t x = in[2 * i], y = in[2 * i + 1], xm = x % P, ym = y % P;
      const uint64_t* o = out + i * OUT;
      const uint64_t sum = uint64_t((u128(xm) + ym) % P), dif = uint64_t((u128(xm) + P - ym) % P);
      const bool one_small = x <= P || y <= P;
#define MI355_FAIL(op, s, got) return msg("gf %s: a=%016llx b=%016llx s=%u got %016llx", op, MI355_X(x), MI355_X(y), unsigned(s), MI355_X(got))
      if (x <= P && y <= P && (o[0] % P != sum || o[0] > P)) MI355_FAIL("add", 0, o[0]);                 // P as either operand included
      if (y <= P && (o[1] % P != dif || (x <= P && o[1] > P))) MI355_FAIL("sub", 0, o[1]);               // lazy minuend: congruent; operands <= P: <= P
      if (one_small && o[2] != gf_mulmod(x, y)) MI355_FAIL("mul", 0, o[2]);                             // canonical (< P)
      if (one_small && o[3] % P != sum) MI355_FAIL("add_lazy", 0, o[3]);
      if (o[4] != (x + y) % P) MI355_FAIL("fold", 0, o[4]);
      if (o[5] != gf_mulmod(x, uint32_t(y))) MI355_FAIL("mul_u32", 0, o[5]);
      if (o[6] != xm) MI355_FAIL("fold", 1, o[6]);
      for (unsigned k = 0; k < 384; ++k) {
        const unsigned s = k % 192;
        const uint64_t r = o[7 + k];
        if (r % P != gf_mulmod(x, p2[s]) || (s != 0 && r > P)) MI355_FAIL(k < 192 ? "mul_pow2" : "mul_pow2 (constant s)", s, r);
      }
#undef MI355_FAIL
      if (one_small) { const unsigned c = mul_tail_case(x, y); seen |= 1u << (c & 3); if ((c & 7) == 4) seen |= 1u << 4; if ((c & 9) == 9) seen |= 1u << 5; }
    }
    // every (borrow, carry) case of the product's tail, "r >= P without either", and a borrow together with the middle column's carry
    if (seen != 0x3f) return msg("gf mul: the operand list misses a tail case (seen mask %02x)", seen);
    return "";
  }
};

// gf::add_lazy_any: the sum of two multiplicand-image words in the row sweeps' mode 3 (multiply by the sum of two images).  BOTH operands
// are lazy, so both run over [0, 2^64); the sum's only consumer is a product with another lazy word (the transformed residue), which is
// evaluated too.  out = sum, sum * x.
struct GfLazySum {
  static constexpr int IN = 2, OUT = 2;
  static constexpr bool kHostEqualsDevice = false;
  static void aux(std::vector<uint64_t>&) {}
  static void fill(std::vector<uint64_t>& in) {
    std::vector<uint64_t> e; GfScalar::edges(e);
    for (uint64_t x : e) for (uint64_t y : e) { in.push_back(x); in.push_back(y); }
    Rng r(0xa4093822299f31d0ull);
    for (int i = 0; i < 4096; ++i) { in.push_back(r.next()); in.push_back(r.next()); }
    // both operands in [P, 2^64) or just below P: the carry fold of the sum lands next to 2^64
    for (int i = 0; i < 4096; ++i) {
      const uint64_t hi = 0xffffffff00000000ull, lo = 0xfffffffe00000000ull;
      in.push_back((r.next() & 0xffffffffull) | (i & 1 ? hi : lo)); in.push_back((r.next() & 0xffffffffull) | (i & 2 ? hi : lo));
    }
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    o[0] = gf::add_lazy_any(in[0], in[1]);
    o[1] = gf::mul(o[0], in[0]);
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    size_t both_lazy = 0, sum_lazy = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t x = in[2 * i], y = in[2 * i + 1];
      const uint64_t sum = uint64_t((u128(x % P) + y % P) % P);
      if (out[2 * i] % P != sum) return msg("gf add_lazy_any: a=%016llx b=%016llx got %016llx", MI355_X(x), MI355_X(y), MI355_X(out[2 * i]));
      if (out[2 * i + 1] != gf_mulmod(sum, x)) return msg("gf mul of a lazy sum: a=%016llx b=%016llx got %016llx", MI355_X(x), MI355_X(y), MI355_X(out[2 * i + 1]));
      both_lazy += (x > P && y > P); sum_lazy += out[2 * i] > P;
    }
    if (!both_lazy || !sum_lazy) return msg("gf add_lazy_any: the operand list misses a lazy case (both operands above P: %zu, sum above P: %zu)", both_lazy, sum_lazy);
    return "";
  }
};

// ------------------------------------------------------------------------------------------------------------------------------------
// GF(P) butterflies
// ------------------------------------------------------------------------------------------------------------------------------------
// values whose sums and differences land on and around P and 2^64: 8-tuples over this alphabet put un-folded values into every slot that
// gfdft.hpp allows to be lazy
inline const std::vector<uint64_t>& gf_alphabet() {
  static const std::vector<uint64_t> a = {0, 1, P - 1, P - 2, 0xffffffffull, P - 0xffffffffull, P - 0x100000000ull, 0x8000000000000000ull, 0x7fffffff80000001ull, P};
  return a;   // nine canonical values, then P (the device's negated zero)
}
// sum_j x[j] w^(jk), w = 2^lw (of order N), on canonical integers
inline void gf_direct_dft(const uint64_t* x, uint64_t* y, int N, unsigned lw) {
  const uint64_t* p2 = gf_pow2_table();
  for (int k = 0; k < N; ++k) {
    u128 s = 0;
    for (int j = 0; j < N; ++j) s += gf_mulmod(x[j], p2[(lw * unsigned(j * k)) % 192]);
    y[k] = uint64_t(s % P);
  }
}
inline void gf_tuples(std::vector<uint64_t>& in, int N, int sampled9, int sampled10, int random) {
  const std::vector<uint64_t>& a = gf_alphabet();
  for (uint64_t v : a) for (int j = 0; j < N; ++j) in.push_back(v);                        // all-equal tuples
  Rng r(0x243f6a8885a308d3ull);
  for (int i = 0; i < sampled9; ++i) for (int j = 0; j < N; ++j) in.push_back(a[r.next() % 9]);
  for (int i = 0; i < sampled10; ++i) for (int j = 0; j < N; ++j) in.push_back(a[r.next() % 10]);
  for (int i = 0; i < random; ++i) for (int j = 0; j < N; ++j) in.push_back(r.next() % P);
}

struct GfDft8 {
  static constexpr int IN = 8, OUT = 48;   // variant v = 3 INV + LAZY, slot k at 8 v + k
  static constexpr bool kHostEqualsDevice = false;
  static void aux(std::vector<uint64_t>&) {}
  static void fill(std::vector<uint64_t>& in) {
    gf_tuples(in, 8, 2048, 1024, 512);
    // Every 4-tuple of canonical alphabet values on four of the inputs (the even ones, the odd ones, and the two mixed halves) with the other four
    // at zero: a random tuple rarely keeps an un-folded sum alive through all three levels (slot 6 of LAZY = 2 needs x0 + x4 in [P, 2^64) and
    // nothing large taken off it afterwards)
    const std::vector<uint64_t>& a = gf_alphabet();
    const int where[4][4] = {{0, 2, 4, 6}, {1, 3, 5, 7}, {0, 1, 4, 5}, {0, 3, 4, 7}};
    for (const auto& w : where)
      for (int p = 0; p < 9; ++p) for (int q = 0; q < 9; ++q) for (int r = 0; r < 9; ++r) for (int s = 0; s < 9; ++s) {
        uint64_t v[8] = {};
        v[w[0]] = a[p]; v[w[1]] = a[q]; v[w[2]] = a[r]; v[w[3]] = a[s];
        for (int j = 0; j < 8; ++j) in.push_back(v[j]);
      }
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    uint64_t x[6][8];
    for (int v = 0; v < 6; ++v) for (int j = 0; j < 8; ++j) x[v][j] = in[j];
    gf::dft8<false, 0>(x[0]); gf::dft8<false, 1>(x[1]); gf::dft8<false, 2>(x[2]);
    gf::dft8<true, 0>(x[3]); gf::dft8<true, 1>(x[4]); gf::dft8<true, 2>(x[5]);
    for (int v = 0; v < 6; ++v) for (int j = 0; j < 8; ++j) o[8 * v + j] = x[v][j];
  }
  static bool may_be_lazy(int lazy, int slot) { return lazy == 2 ? slot != 7 : lazy == 1 ? (slot == 1 || slot == 2 || slot == 3 || slot == 5) : false; }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n, size_t* counts = nullptr) {   // counts[48]: outputs above P per variant and slot
    size_t above[6][8] = {};
    for (size_t i = 0; i < n; ++i) {
      uint64_t want[2][8];
      gf_direct_dft(in + 8 * i, want[0], 8, 120); gf_direct_dft(in + 8 * i, want[1], 8, 72);   // omega_8 = 2^120, its inverse 2^72
      for (int v = 0; v < 6; ++v) for (int k = 0; k < 8; ++k) {
        const uint64_t r = out[i * OUT + 8 * v + k];
        if (r % P != want[v / 3][k] || (!may_be_lazy(v % 3, k) && r > P))
          return msg("gf dft8<%s, %d> slot %d: got %016llx want %016llx, input %016llx %016llx %016llx %016llx %016llx %016llx %016llx %016llx", v / 3 ? "inverse" : "forward",
                     v % 3, k, MI355_X(r), MI355_X(want[v / 3][k]), MI355_X(in[8 * i]), MI355_X(in[8 * i + 1]), MI355_X(in[8 * i + 2]), MI355_X(in[8 * i + 3]),
                     MI355_X(in[8 * i + 4]), MI355_X(in[8 * i + 5]), MI355_X(in[8 * i + 6]), MI355_X(in[8 * i + 7]));
        above[v][k] += r > P;
      }
    }
    // coverage: the cases must really have put an un-folded value into every slot that may hold one
    if (counts) for (int v = 0; v < 6; ++v) for (int k = 0; k < 8; ++k) counts[8 * v + k] = above[v][k];
    for (int v = 0; v < 6; ++v) for (int k = 0; k < 8; ++k)
      if (may_be_lazy(v % 3, k) && !above[v][k]) return msg("gf dft8<%s, %d>: no case left a value above P in slot %d", v / 3 ? "inverse" : "forward", v % 3, k);
    return "";
  }
};

// v2::dft4 (kernels_v2_common.hpp, device only: evaluated by selftest.hip): every 4-tuple over the alphabet, both directions; out = forward[4], inverse[4]
struct GfDft4 {
  static constexpr int IN = 4, OUT = 8;
  static void fill(std::vector<uint64_t>& in) {
    const std::vector<uint64_t>& a = gf_alphabet();
    for (uint64_t p : a) for (uint64_t q : a) for (uint64_t r : a) for (uint64_t s : a) { in.push_back(p); in.push_back(q); in.push_back(r); in.push_back(s); }
    gf_tuples(in, 4, 0, 0, 512);
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      uint64_t want[2][4];
      gf_direct_dft(in + 4 * i, want[0], 4, 48); gf_direct_dft(in + 4 * i, want[1], 4, 144);   // omega_4 = 2^48
      for (int k = 0; k < 8; ++k) {
        const uint64_t r = out[i * OUT + k];
        if (r % P != want[k / 4][k % 4] || r > P)
          return msg("gf dft4<%s> slot %d: got %016llx want %016llx, input %016llx %016llx %016llx %016llx", k / 4 ? "inverse" : "forward", k % 4, MI355_X(r),
                     MI355_X(want[k / 4][k % 4]), MI355_X(in[4 * i]), MI355_X(in[4 * i + 1]), MI355_X(in[4 * i + 2]), MI355_X(in[4 * i + 3]));
      }
    }
    return "";
  }
};

// The consumers of the lazy butterfly outputs, as the radix-8 kernels chain them (kernels_v2.hip, k2_rows; device only, evaluated by selftest.hip
// with eight waves to a work-group).  Thread g (wave w = g / 64 mod 8) takes the tuples tuple_of(g, 0) (plane a) and tuple_of(g, 1) (plane b) of GfDft8's list and
// eight factors (table-like: canonical) and returns, plane a then plane b, eight slots each:
//   forward:  dft8p<false, 1>, seam<6, false, true>(w)  -> out[0..15];   then dft8p<false, 2>, p2_mul by the factors -> out[16..31]
//   inverse:  dft8p<true>, seam<6, true>(w), dft8p<true, 2>, p2_mul by the factors -> out[32..47]
struct GfChain {
  static constexpr int OUT = 48, kThreads = 512 * 8;
  static void factors(std::vector<uint64_t>& f) {
    Rng r(0x13198a2e03707344ull);
    const uint64_t e[4] = {0, 1, P - 1, 0xffffffffull};
    for (int i = 0; i < kThreads * 8; ++i) { const uint64_t v = r.next(); f.push_back((v & 0x1f) < 4 ? e[v & 3] : v % P); }
  }
  static GF_HDM size_t tuple_of(int g, int plane, size_t ntuples) { return (size_t(2 * g + plane) * 7) % ntuples; }   // spread over the whole list
  // seam exponent of slot k at wave w: omega_64^(k w) = 2^(39 k w)
  static unsigned seam_shift(int k, int w, bool inv) { const unsigned f = (gf::LOG2_W64 * unsigned(k) * unsigned(w)) % 192u; return inv ? (192u - f) % 192u : f; }
  // dft8_out: GfDft8's device outputs for the same tuples (the coverage condition reads the forward LAZY = 1 slots from it)
  static std::string check(const uint64_t* tuples, size_t ntuples, const uint64_t* fac, const uint64_t* out, const uint64_t* dft8_out) {
    const uint64_t* p2 = gf_pow2_table();
    size_t folded[8] = {};
    for (int g = 0; g < kThreads; ++g) {
      const int w = (g >> 6) & 7;
      for (int plane = 0; plane < 2; ++plane) {
        const size_t tu = tuple_of(g, plane, ntuples);
        const uint64_t* in = tuples + 8 * tu;
        const uint64_t* o = out + size_t(g) * OUT;
        for (int inv = 0; inv < 2; ++inv) {
          uint64_t a[8], b[8], c[8];
          gf_direct_dft(in, a, 8, inv ? 72 : 120);
          for (int k = 0; k < 8; ++k) b[k] = gf_mulmod(a[k], p2[seam_shift(k, w, inv)]);
          gf_direct_dft(b, c, 8, inv ? 72 : 120);
          for (int k = 0; k < 8; ++k) {
            const uint64_t want = gf_mulmod(c[k], fac[size_t(g) * 8 + k]);
            if (!inv) {
              const uint64_t s1 = o[8 * plane + k];   // after the seam every slot is folded: shifted (<= P), or folded by FOLD0 at wave 0
              if (s1 % P != b[k] || s1 > P)
                return msg("gf chain forward, after seam<6> at wave %d, slot %d: got %016llx want %016llx (tuple %zu)", w, k, MI355_X(s1), MI355_X(b[k]), tu);
            }
            const uint64_t r = o[(inv ? 32 : 16) + 8 * plane + k];
            if (r != want) return msg("gf chain %s, after the multiplication, wave %d slot %d: got %016llx want %016llx (tuple %zu)", inv ? "inverse" : "forward", w, k, MI355_X(r), MI355_X(want), tu);
          }
        }
        if (w == 0) for (int k = 0; k < 8; ++k) folded[k] += dft8_out[tu * GfDft8::OUT + 8 * 1 + k] > P;
      }
    }
    for (int k : {1, 2, 3, 5})
      if (!folded[k]) return msg("gf chain: wave 0 (the FOLD0 case of seam<6>) met no value above P in slot %d", k);
    return "";
  }
};

// ------------------------------------------------------------------------------------------------------------------------------------
// second family: Z/M61, Z/M31 and their complex extensions
// ------------------------------------------------------------------------------------------------------------------------------------
using crt::F31; using crt::F61; using crt::M31; using crt::M61;

struct Cx { uint64_t re, im; };   // reference complex arithmetic mod m on integers
inline Cx cx_mul(Cx a, Cx b, uint64_t m) {
  const u128 re = (u128(a.re % m) * (b.re % m) + u128(m - a.im % m) * (b.im % m)) % m, im = (u128(a.re % m) * (b.im % m) + u128(a.im % m) * (b.re % m)) % m;
  return {uint64_t(re), uint64_t(im)};
}
inline Cx cx_add(Cx a, Cx b, uint64_t m) { return {uint64_t((u128(a.re % m) + b.re % m) % m), uint64_t((u128(a.im % m) + b.im % m) % m)}; }
inline Cx cx_conj(Cx a, uint64_t m) { return {a.re % m, (m - a.im % m) % m}; }
// sum_q x[q] w^(q k), w a primitive N-th root given as a complex (scalars: im = 0)
inline void cx_direct_dft(const Cx* x, Cx* y, int N, Cx w, uint64_t m) {
  Cx pw[16]; pw[0] = {1, 0};
  for (int e = 1; e < N; ++e) pw[e] = cx_mul(pw[e - 1], w, m);
  for (int k = 0; k < N; ++k) { Cx s{0, 0}; for (int q = 0; q < N; ++q) s = cx_add(s, cx_mul(x[q], pw[(q * k) % N], m), m); y[k] = s; }
}
inline Cx root_of_radix(int R, uint64_t m, bool inv) {   // omega_8 = (1 + i) / sqrt 2 = (1 + i) 2^30 resp. (1 + i) 2^15; omega_4 = i; omega_2 = -1
  const uint64_t h = m == M61 ? (1ull << 30) : (1ull << 15);
  const Cx w = R == 8 ? Cx{h, h} : R == 4 ? Cx{0, 1} : Cx{m - 1, 0};
  return inv ? cx_conj(w, m) : w;
}

struct CrtScalar {
  static constexpr int IN = 2, OUT = 16 + 61 + 31;
  static constexpr bool kHostEqualsDevice = true;
  static void aux(std::vector<uint64_t>&) {}
  static void fill(std::vector<uint64_t>& in) {
    const uint64_t e[] = {0, 1, 2, M61 - 1, M61, M61 + 1, M61 + 7, 2 * M61, 2 * M61 + 1, 4 * M61, 8 * M61, 8 * M61 + 1, 0xffffffffffffffffull, M31 - 1, M31, M31 + 1, 0x80000000ull,
                          0xffffffffull, 0x100000000ull, (uint64_t(M31) << 31) | M31, 0x3fffffffffffffffull, 0x4000000000000000ull, 0x7fffffffffffffffull, 0x8000000000000000ull,
                          0xfffffffffffffffeull, 0x2000000000000000ull, 0x1fffffff80000000ull, 0x7fffffff00000000ull, 0xffffffff00000000ull};
    for (uint64_t x : e) for (uint64_t y : e) { in.push_back(x); in.push_back(y); }
    Rng r(0xa4093822299f31d0ull);
    for (int i = 0; i < 4096; ++i) { in.push_back(r.next()); in.push_back(r.next()); }
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    const uint64_t v = in[0], w = in[1];
    const uint64_t cv = crt::red61(v), cw = crt::red61(w);
    const uint32_t dv = crt::red31(v), dw = crt::red31(w);
    o[0] = cv; o[1] = dv; o[2] = crt::fold61(v); o[3] = crt::canon61(v); o[4] = crt::shl30_61(v);
    o[5] = crt::mul61(v & M61, w & M61); o[6] = crt::mul31(uint32_t(v) & M31, uint32_t(w) & M31);   // operands up to M itself
    o[7] = F61::half(cv); o[8] = F31::half(dv); o[9] = crt::red31_63(v >> 1);
    o[10] = F61::add(cv, cw); o[11] = F61::sub(cv, cw); o[12] = F61::neg(cv); o[13] = F31::add(dv, dw); o[14] = F31::sub(dv, dw); o[15] = F31::neg(dv);
    for (uint32_t s = 0; s < 61; ++s) o[16 + s] = crt::rot61(cv, s);
    for (uint32_t s = 0; s < 31; ++s) o[77 + s] = crt::rot31(dv, s);
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      const uint64_t v = in[2 * i], w = in[2 * i + 1], cv = v % M61, cw = w % M61, dv = v % M31, dw = w % M31;
      const uint64_t* o = out + i * OUT;
      uint64_t want[16] = {cv, dv, cv, cv, uint64_t((u128(cv) << 30) % M61), uint64_t(u128(v & M61) * (w & M61) % M61), (v & M31) * (w & M31) % M31,
                           uint64_t(u128(cv) * ((M61 + 1) / 2) % M61), dv * ((uint64_t(M31) + 1) / 2) % M31, (v >> 1) % M31,
                           (cv + cw) % M61, (cv + M61 - cw) % M61, (M61 - cv) % M61, (dv + dw) % M31, (dv + M31 - dw) % M31, (M31 - dv) % M31};
      for (int k = 0; k < 16; ++k) {
        const bool lazy = k == 2 || k == 4;   // fold61: <= M61 + 7; shl30_61: < 2^61 + 2^33
        const bool ok = lazy ? (o[k] % M61 == want[k] && o[k] <= (k == 2 ? M61 + 7 : (1ull << 61) + (1ull << 33))) : o[k] == want[k];
        if (!ok) return msg("crt scalar op %d: v=%016llx w=%016llx got %016llx want %016llx", k, MI355_X(v), MI355_X(w), MI355_X(o[k]), MI355_X(want[k]));
      }
      for (uint32_t s = 0; s < 61; ++s)
        if (o[16 + s] != uint64_t((u128(cv) << s) % M61)) return msg("crt rot61: a=%016llx s=%u got %016llx", MI355_X(cv), s, MI355_X(o[16 + s]));
      for (uint32_t s = 0; s < 31; ++s)
        if (o[77 + s] != uint64_t((u128(dv) << s) % M31)) return msg("crt rot31: a=%08llx s=%u got %016llx", MI355_X(dv), s, MI355_X(o[77 + s]));
    }
    return "";
  }
};

// complex products: in = x61.re, x61.im (<= M61 + 7: folded), w61.re, w61.im (canonical), x31.re, x31.im, w31.re, w31.im (canonical)
struct CrtCmul {
  static constexpr int IN = 8, OUT = 8;
  static constexpr bool kHostEqualsDevice = true;
  static void aux(std::vector<uint64_t>&) {}
  static void fill(std::vector<uint64_t>& in) {
    const uint64_t x61[] = {0, 1, M61 - 1, M61, M61 + 1, M61 + 7, 0x7fffffffull, 0x80000000ull, M61 - 0x7fffffffull, 0x1fffffff80000000ull, 0x3fffffffull << 31, 0x1555555555555555ull};
    const uint64_t w61[] = {0, 1, M61 - 1, M61 - 2, 0x7fffffffull, 0x80000000ull, 0x1fffffff80000000ull, 0x3fffffffull << 31, 1ull << 30, 0x0aaaaaaaaaaaaaaaull};
    const uint64_t x31[] = {0, 1, M31 - 1, M31 - 2, 0xffffull, 0x10000ull, 0x40000000ull, 0x3fffffffull, 0x55555555ull, 0x7fff0000ull, 0x00008000ull, 2};
    const uint64_t w31[] = {0, 1, M31 - 1, M31 - 2, 0xffffull, 0x10000ull, 0x40000000ull, 0x3fffffffull, 0x8000ull, 0x2aaaaaaaull};
    for (int a = 0; a < 12; ++a) for (int b = 0; b < 12; ++b) for (int c = 0; c < 10; ++c) for (int d = 0; d < 10; ++d)
      for (uint64_t v : {x61[a], x61[b], w61[c], w61[d], x31[a], x31[b], w31[c], w31[d]}) in.push_back(v);
    Rng r(0x082efa98ec4e6c89ull);
    for (int i = 0; i < 4096; ++i) {
      for (int k = 0; k < 2; ++k) { const uint64_t v = r.next() % (M61 + 8); in.push_back((i & 7) == 7 ? M61 + (v & 7) : v); }
      for (int k = 0; k < 2; ++k) in.push_back(r.next() % M61);
      for (int k = 0; k < 4; ++k) in.push_back(r.next() % M31);
    }
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    const crt::Lz61 x{in[0], in[1]}; const F61::C w{in[2], in[3]};
    const F31::C y{uint32_t(in[4]), uint32_t(in[5])}, u{uint32_t(in[6]), uint32_t(in[7])};
    const F61::C a = crt::cmul61<false>(x, w), b = crt::cmul61<true>(x, w);
    const F31::C c = crt::cmul31<false>(y, u), d = crt::cmul31<true>(y, u);
    o[0] = a.re; o[1] = a.im; o[2] = b.re; o[3] = b.im; o[4] = c.re; o[5] = c.im; o[6] = d.re; o[7] = d.im;
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      const uint64_t* v = in + 8 * i; const uint64_t* o = out + 8 * i;
      const Cx a = cx_mul({v[0], v[1]}, {v[2], v[3]}, M61), b = cx_mul({v[0], v[1]}, cx_conj({v[2], v[3]}, M61), M61);
      const Cx c = cx_mul({v[4], v[5]}, {v[6], v[7]}, M31), d = cx_mul({v[4], v[5]}, cx_conj({v[6], v[7]}, M31), M31);
      const uint64_t want[8] = {a.re, a.im, b.re, b.im, c.re, c.im, d.re, d.im};
      for (int k = 0; k < 8; ++k)
        if (o[k] != want[k])
          return msg("crt %s<%s> %s: x=(%016llx, %016llx) w=(%016llx, %016llx) got %016llx want %016llx", k < 4 ? "cmul61" : "cmul31", (k & 2) ? "conj" : "plain", (k & 1) ? "im" : "re",
                     MI355_X(v[k < 4 ? 0 : 4]), MI355_X(v[k < 4 ? 1 : 5]), MI355_X(v[k < 4 ? 2 : 6]), MI355_X(v[k < 4 ? 3 : 7]), MI355_X(o[k]), MI355_X(want[k]));
    }
    return "";
  }
};

// butterflies: in = eight complex values of Z/M61 (<= M61: the lazy forms take M61 itself; the generic forms get it canonicalised), then eight of Z/M31.
// out: for the kinds (bfly61, bfly<F61>, bfly<F31>), the directions (forward, inverse) and R = 2, 4, 8: R complex values (28 per kind)
struct CrtBfly {
  static constexpr int IN = 32, OUT = 3 * 28 * 2;
  static constexpr bool kHostEqualsDevice = true;
  static void aux(std::vector<uint64_t>&) {}
  static void push(std::vector<uint64_t>& in, const uint64_t (&re)[8], const uint64_t (&im)[8], uint64_t top61, uint64_t top31) {   // values as fractions of the top: 0 .. 3 -> 0, 1, top - 1, top
    const auto pick = [](uint64_t c, uint64_t top) { return c == 0 ? 0 : c == 1 ? 1 : c == 2 ? top - 1 : top; };
    for (int j = 0; j < 8; ++j) { in.push_back(pick(re[j], top61)); in.push_back(pick(im[j], top61)); }
    for (int j = 0; j < 8; ++j) { in.push_back(pick(re[j], top31)); in.push_back(pick(im[j], top31)); }
  }
  static void fill(std::vector<uint64_t>& in) {
    for (uint64_t top = 2; top < 4; ++top) {   // the maximum: M - 1 (canonical), then M itself ("<= M61")
      for (unsigned mask = 0; mask < 256; ++mask) for (int var = 0; var < 4; ++var) {   // 0 / maximum in every pattern over the eight inputs; mask 255: all at the maximum
        uint64_t re[8], im[8];
        for (int j = 0; j < 8; ++j) { re[j] = (mask >> j & 1) ? top : 0; im[j] = var == 0 ? re[j] : var == 1 ? top - re[j] : var == 2 ? 0 : top; }
        push(in, re, im, M61, M31);
      }
    }
    const uint64_t a61[] = {0, 1, M61 - 1, M61 - 2, M61, 0x7fffffffull, 0x80000000ull, 1ull << 60, 0x1fffffff80000000ull, 1ull << 30, M61 >> 1, (M61 >> 1) + 1};
    const uint64_t a31[] = {0, 1, M31 - 1, M31 - 2, M31 - 1, 0xffffull, 0x10000ull, 1ull << 30, 0x7fff8000ull, 1ull << 15, M31 >> 1, (M31 >> 1) + 1};
    Rng r(0x452821e638d01377ull);
    for (int i = 0; i < 2048; ++i) {
      uint64_t pick[16];
      for (int j = 0; j < 16; ++j) pick[j] = r.next() % 12;
      for (int j = 0; j < 16; ++j) in.push_back(a61[pick[j]]);
      for (int j = 0; j < 16; ++j) in.push_back(a31[pick[j]]);
    }
    for (int i = 0; i < 2048; ++i) {
      for (int j = 0; j < 16; ++j) in.push_back(r.next() % M61);
      for (int j = 0; j < 16; ++j) in.push_back(r.next() % M31);
    }
  }
  template <int R, bool INV>
  static GF_HDM void one(const uint64_t* in, uint64_t* o61l, uint64_t* o61g, uint64_t* o31g) {
    crt::Lz61 x[R]; F61::C y[R]; F31::C z[R];
    for (int q = 0; q < R; ++q) {
      x[q] = {in[2 * q], in[2 * q + 1]};
      y[q] = {in[2 * q] >= M61 ? in[2 * q] - M61 : in[2 * q], in[2 * q + 1] >= M61 ? in[2 * q + 1] - M61 : in[2 * q + 1]};
      z[q] = {uint32_t(in[16 + 2 * q] >= M31 ? in[16 + 2 * q] - M31 : in[16 + 2 * q]), uint32_t(in[16 + 2 * q + 1] >= M31 ? in[16 + 2 * q + 1] - M31 : in[16 + 2 * q + 1])};
    }
    crt::bfly61<R, INV>(x); crt::bfly<F61, R, INV>(y); crt::bfly<F31, R, INV>(z);
    for (int q = 0; q < R; ++q) { o61l[2 * q] = x[q].re; o61l[2 * q + 1] = x[q].im; o61g[2 * q] = y[q].re; o61g[2 * q + 1] = y[q].im; o31g[2 * q] = z[q].re; o31g[2 * q + 1] = z[q].im; }
  }
  static constexpr int off(int inv, int R) { return 2 * (14 * inv + (R == 2 ? 0 : R == 4 ? 2 : 6)); }   // word offset inside a kind
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    one<2, false>(in, o + off(0, 2), o + 56 + off(0, 2), o + 112 + off(0, 2)); one<4, false>(in, o + off(0, 4), o + 56 + off(0, 4), o + 112 + off(0, 4));
    one<8, false>(in, o + off(0, 8), o + 56 + off(0, 8), o + 112 + off(0, 8));
    one<2, true>(in, o + off(1, 2), o + 56 + off(1, 2), o + 112 + off(1, 2)); one<4, true>(in, o + off(1, 4), o + 56 + off(1, 4), o + 112 + off(1, 4));
    one<8, true>(in, o + off(1, 8), o + 56 + off(1, 8), o + 112 + off(1, 8));
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      const uint64_t* v = in + IN * i; const uint64_t* o = out + OUT * i;
      Cx x61[8], x31[8];
      for (int q = 0; q < 8; ++q) { x61[q] = {v[2 * q], v[2 * q + 1]}; x31[q] = {v[16 + 2 * q], v[16 + 2 * q + 1]}; }
      for (int inv = 0; inv < 2; ++inv) for (int R = 2; R <= 8; R *= 2) {
        Cx w61[8], w31[8];
        cx_direct_dft(x61, w61, R, root_of_radix(R, M61, inv), M61); cx_direct_dft(x31, w31, R, root_of_radix(R, M31, inv), M31);
        for (int q = 0; q < R; ++q) for (int c = 0; c < 2; ++c) {
          const uint64_t want61 = c ? w61[q].im : w61[q].re, want31 = c ? w31[q].im : w31[q].re;
          const uint64_t lz = o[off(inv, R) + 2 * q + c], g61 = o[56 + off(inv, R) + 2 * q + c], g31 = o[112 + off(inv, R) + 2 * q + c];
          const char* bad = lz % M61 != want61 ? "bfly61" : g61 != want61 ? "bfly<F61>" : g31 != want31 ? "bfly<F31>" : nullptr;   // lazy: congruent; generic: canonical
          if (bad) return msg("crt %s<%d, %s> output %d %s: got %016llx / %016llx / %016llx want %016llx / %016llx (case %zu)", bad, R, inv ? "inverse" : "forward", q, c ? "im" : "re",
                              MI355_X(lz), MI355_X(g61), MI355_X(g31), MI355_X(want61), MI355_X(want31), i);
        }
      }
    }
    return "";
  }
};

// odd axis: in = nine complex values of Z/M61, nine of Z/M31 (canonical); aux = the engine's tables for radix 3 and radix 9 (make_odd_tables):
// per radix r61[9], r61i[9], c3_61, r31[9], r31i[9], c3_31 (38 words).  out: per field (M61, M31): dft_odd<3> forward, inverse, dft_odd<9> forward, inverse
struct CrtOdd {
  static constexpr int IN = 36, OUT = 2 * 48, kAux = 38;
  static constexpr bool kHostEqualsDevice = true;
  static void aux(std::vector<uint64_t>& a) {
    for (unsigned odd : {3u, 9u}) {
      const crt::OddTables t = crt::make_odd_tables(odd);
      for (int k = 0; k < 9; ++k) a.push_back(t.r61[k]);
      for (int k = 0; k < 9; ++k) a.push_back(t.r61i[k]);
      a.push_back(t.c3_61);
      for (int k = 0; k < 9; ++k) a.push_back(t.r31[k]);
      for (int k = 0; k < 9; ++k) a.push_back(t.r31i[k]);
      a.push_back(t.c3_31);
    }
  }
  static void fill(std::vector<uint64_t>& in) {
    const uint64_t a61[] = {0, 1, M61 - 1, M61 - 2, 1ull << 60, M61 >> 1, (M61 >> 1) + 1, 0x1fffffff80000000ull};
    const uint64_t a31[] = {0, 1, M31 - 1, M31 - 2, 1ull << 30, M31 >> 1, (M31 >> 1) + 1, 0x7fff8000ull};
    for (unsigned mask = 0; mask < 512; ++mask) for (int var = 0; var < 3; ++var) {   // 0 / M - 1 in every pattern
      for (int f = 0; f < 2; ++f) for (int j = 0; j < 9; ++j) {
        const uint64_t top = f ? M31 - 1 : M61 - 1, re = (mask >> j & 1) ? top : 0;
        in.push_back(re); in.push_back(var == 0 ? re : var == 1 ? top - re : top);
      }
    }
    Rng r(0xbe5466cf34e90c6cull);
    for (int i = 0; i < 2048; ++i) {
      uint64_t pick[18];
      for (int j = 0; j < 18; ++j) pick[j] = r.next() % 8;
      for (int j = 0; j < 18; ++j) in.push_back(a61[pick[j]]);
      for (int j = 0; j < 18; ++j) in.push_back(a31[pick[j]]);
    }
    for (int i = 0; i < 1024; ++i) {
      for (int j = 0; j < 18; ++j) in.push_back(r.next() % M61);
      for (int j = 0; j < 18; ++j) in.push_back(r.next() % M31);
    }
  }
  template <class F, int ODD>
  static GF_HDM void one(const uint64_t* in, uint64_t* o, const uint64_t* tab) {   // tab: r[9], ri[9], c3
    typename F::S r[9], ri[9];
    for (int k = 0; k < 9; ++k) { r[k] = typename F::S(tab[k]); ri[k] = typename F::S(tab[9 + k]); }
    const typename F::S c3 = typename F::S(tab[18]);
    typename F::C x[ODD], y[ODD];
    for (int k = 0; k < ODD; ++k) { x[k] = {typename F::S(in[2 * k]), typename F::S(in[2 * k + 1])}; y[k] = x[k]; }
    crt::dft_odd<F, ODD>(x, r, c3); crt::dft_odd<F, ODD>(y, ri, F::neg(c3));   // as k_front and k_back call it
    for (int k = 0; k < ODD; ++k) { o[2 * k] = x[k].re; o[2 * k + 1] = x[k].im; o[2 * ODD + 2 * k] = y[k].re; o[2 * ODD + 2 * k + 1] = y[k].im; }
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t* aux) {
    one<F61, 3>(in, o, aux); one<F61, 9>(in, o + 12, aux + kAux);
    one<F31, 3>(in + 18, o + 48, aux + 19); one<F31, 9>(in + 18, o + 60, aux + kAux + 19);
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    std::vector<uint64_t> a; aux(a);
    for (size_t i = 0; i < n; ++i) for (int f = 0; f < 2; ++f) for (int odd = 3; odd <= 9; odd *= 3) {
      const uint64_t m = f ? M31 : M61;
      const uint64_t* tab = a.data() + (odd == 9 ? kAux : 0) + 19 * f;
      const uint64_t* o = out + OUT * i + 48 * f + (odd == 9 ? 12 : 0);
      Cx x[9], y[9];
      for (int k = 0; k < odd; ++k) x[k] = {in[IN * i + 18 * f + 2 * k], in[IN * i + 18 * f + 2 * k + 1]};
      for (int inv = 0; inv < 2; ++inv) {
        cx_direct_dft(x, y, odd, Cx{tab[inv ? 9 + 1 : 1], 0}, m);
        for (int k = 0; k < odd; ++k) {
          const uint64_t gr = o[2 * odd * inv + 2 * k], gi = o[2 * odd * inv + 2 * k + 1];
          if (gr != y[k].re || gi != y[k].im)
            return msg("crt dft_odd<%s, %d> %s output %d: got (%016llx, %016llx) want (%016llx, %016llx) (case %zu)", f ? "F31" : "F61", odd, inv ? "inverse" : "forward", k, MI355_X(gr),
                       MI355_X(gi), MI355_X(y[k].re), MI355_X(y[k].im), i);
        }
      }
    }
    return "";
  }
};

// DigitWalk: in = p, n, odd, j.  out: width, weight61, weight31, unweight61, unweight31 from start(j), then the same five from start(j - j mod 8) and
// j mod 8 steps of next() (the carry sweep's way through a run)
struct CrtWalk {
  static constexpr int IN = 4, OUT = 10;
  static constexpr bool kHostEqualsDevice = true;
  static void aux(std::vector<uint64_t>&) {}
  static void fill(std::vector<uint64_t>& in) {
    const uint32_t sizes[][3] = {{521, 32, 1}, {127, 8, 1}, {1279, 96, 3}, {9941, 576, 9}, {86243, 4608, 9}, {216091, 12288, 3}, {11213, 1024, 1}, {3021377, 147456, 9}};
    for (const auto& s : sizes)
      for (uint32_t j = 0; j < s[1]; ++j) if (s[1] <= 16384 || j < 4096 || j >= s[1] - 4096) { in.push_back(s[0]); in.push_back(s[1]); in.push_back(s[2]); in.push_back(j); }
  }
  static GF_HDM void five(const crt::DigitWalk& d, const crt::Geom& g, uint64_t* o) {
    o[0] = d.width(g); o[1] = d.weight61(); o[2] = d.weight31(); o[3] = d.unweight61(); o[4] = d.unweight31();
  }
  static GF_HDM void eval(const uint64_t* in, uint64_t* o, const uint64_t*) {
    crt::Geom g;   // the fields the walk reads, as make_geom sets them (checked against make_geom on the host)
    const uint32_t p = uint32_t(in[0]), n = uint32_t(in[1]), j = uint32_t(in[3]);
    g.p = p; g.n = n; g.odd = uint32_t(in[2]); g.ln = 0; g.a = 1; g.inv31 = 0;
    g.l61 = 0; g.l31 = 0;
    for (uint32_t y = 1; y < 61; ++y) if ((uint64_t(n % 61) * y) % 61 == 1) g.l61 = y;
    for (uint32_t y = 1; y < 31; ++y) if ((uint64_t(n % 31) * y) % 31 == 1) g.l31 = y;
    g.q = p / n; g.t = p % n;
    g.lt61 = uint32_t(uint64_t(g.l61) * (g.t % 61) % 61); g.lt31 = uint32_t(uint64_t(g.l31) * (g.t % 31) % 31);
    crt::DigitWalk d; d.start(g, j); five(d, g, o);
    d.start(g, j & ~7u);
    for (uint32_t k = 0; k < (j & 7u); ++k) d.next(g);
    five(d, g, o + 5);
  }
  static std::string check(const uint64_t* in, const uint64_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      const uint64_t p = in[4 * i], nn = in[4 * i + 1], j = in[4 * i + 3];
      const crt::Geom g = crt::make_geom(uint32_t(p), size_t(nn), uint32_t(in[4 * i + 2]), 1);
      if ((uint64_t(g.l61) * nn) % 61 != 1 || (uint64_t(g.l31) * nn) % 31 != 1 || g.q != p / nn || g.t != p % nn) return msg("crt make_geom(p=%llu, n=%llu): inverse or quotient wrong", MI355_X(p), MI355_X(nn));
      const auto ceil_div = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
      const uint64_t width = ceil_div(p * (j + 1), nn) - ceil_div(p * j, nn);
      // weight of digit j: 2^(ceil(p j / n) - p j / n) = 2^(e / n), e = (n - p j mod n) mod n; 2^(1 / n) = 2^l with l n = 1 (mod 61 resp. 31)
      const uint64_t e = (nn - (p * j) % nn) % nn;
      uint64_t l61 = 0, l31 = 0;
      for (uint64_t y = 1; y < 61; ++y) if ((nn * y) % 61 == 1) l61 = y;
      for (uint64_t y = 1; y < 31; ++y) if ((nn * y) % 31 == 1) l31 = y;
      const uint64_t w61 = (l61 * (e % 61)) % 61, w31 = (l31 * (e % 31)) % 31;
      const uint64_t want[5] = {width, w61, w31, (61 - w61) % 61, (31 - w31) % 31};
      for (int k = 0; k < 10; ++k)
        if (out[OUT * i + k] != want[k % 5]) return msg("crt DigitWalk p=%llu n=%llu j=%llu field %d (%s): got %llu want %llu", MI355_X(p), MI355_X(nn), MI355_X(j), k % 5, k < 5 ? "start" : "next", MI355_X(out[OUT * i + k]), MI355_X(want[k % 5]));
    }
    return "";
  }
};

// run a family on the host forms: fill, evaluate, check
template <class Fam>
inline std::string run_on_host() {
  std::vector<uint64_t> in, a; Fam::fill(in); Fam::aux(a);
  const size_t n = in.size() / Fam::IN;
  std::vector<uint64_t> out(n * Fam::OUT);
  for (size_t i = 0; i < n; ++i) Fam::eval(in.data() + i * Fam::IN, out.data() + i * Fam::OUT, a.data());
  return Fam::check(in.data(), out.data(), n);
}

}  // namespace cases
}  // namespace mi355
