// Transform plan for one exponent: sizes, tile geometry and the small host-built tables.
//
// Host-only (no HIP), so the size policy and the index maps are testable without a GPU.
//
// Reference behaviour kept:  n = ibdwt::transform_size(p) (include/marin/ibdwt.h:17-43), digit
// widths ceil(p(j+1)/n) - ceil(pj/n) (ibdwt.h:127-132), weights 2^frac(-pj/n) built from
// nr2 = 554^((P-1)/192/n) (ibdwt.h:116-143), roots from generator 7 (arith.h:72).
// What is different by design (MI355X-first):
//   * the length-m (m = n/2 pairs) transform is a two-level decomposition m = M1 x M2 ("columns" of
//     length M1 at stride M2, then contiguous rows of length M2) so one squaring is three sweeps
//     (front, middle, back) instead of the reference's five transform kernels + two carry kernels;
//   * the weights are never stored per digit: w_j = TA[i1] * TB[2*i2+b] / (wrap ? 2 : 1) with
//     M1 + 2*M2 table entries (the reference streams a 2n-word table, 128 MiB at n = 2^23);
//   * registers hold UNWEIGHTED digits as u32 in a tile-major order chosen so that both the front
//     and the back sweep touch them fully coalesced.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "gf.hpp"

namespace mi355 {

inline size_t transform_size(uint32_t exponent) {
  // ibdwt.h:17-43: smallest n in {2^k, 5*2^k}, k <= 26, with 2*(floor(p/n)+1) + log2(n) < 64
  uint32_t w = 0, log2_n = 1, log2_n5 = 2;
  do { ++log2_n; w = exponent >> log2_n; } while ((w + 1) * 2 + log2_n >= 64);
  do { ++log2_n5; w = exponent / (5u << log2_n5); } while ((w + 1) * 2 + (log2_n5 + 2.4) >= 64);
  const size_t invalid = size_t(-1);
  const size_t n2 = (log2_n <= 26) ? (size_t(1) << log2_n) : invalid;
  const size_t n5 = (log2_n5 <= 26) ? (size_t(5) << log2_n5) : invalid;
  return n2 < n5 ? n2 : n5;
}

inline int ilog2(size_t v) { int r = -1; while (v) { v >>= 1; ++r; } return r; }

inline uint32_t bitrev(uint32_t i, int bits) {
  uint32_t r = 0;
  for (int k = 0; k < bits; ++k) { r = (r << 1) | (i & 1); i >>= 1; }
  return r;
}

struct Plan {
  uint32_t p = 0;
  size_t n = 0, m = 0;      // digits, pairs
  uint32_t r5 = 1;          // 1 or 5
  uint32_t M1 = 1, M2 = 1;  // m = M1 * M2, M2 = 2^logM2, M1 = r5 * L1, L1 = 2^logL1
  uint32_t L1 = 1, logL1 = 0, logM2 = 0;
  uint32_t C = 1;           // adjacent columns per front/back tile (runs of 2C digits)
  bool split5 = false;      // columns of 5 L1 pairs beyond LDS: the radix-5 stage runs through memory (kernels.hip k_front_split_*), C = 1
  uint32_t lanes = 1;       // independent residues per register (plan token lanes=B): every operation acts on all of them in one launch
  bool onelaunch = false;   // plan token onelaunch (n <= 8192): a product is one launch, front, row and back sweep of a lane in one work-group (kernels.hip k_onelaunch)
  uint32_t q = 0, t = 0;    // p = q*n + t
  uint32_t twh = 0;         // omega_m^e = TWlo[e & (2^twh-1)] * TWhi[e >> twh]
  uint32_t a_fast = 1;      // largest factor the back sweeps multiply in themselves (fused_factor_ok); above it: factor 1 + k_scale
  bool sum_fast = false;    // dst x (a + b) fits one product (sum_product_ok): mul_sum runs the row sweep's mode 3; else two products
  size_t lds_front = 0, lds_mid = 0;

  // host tables (uploaded as-is)
  std::vector<uint32_t> SA, SB;          // p*j mod n split: SA[i1] + SB[2*i2+b]
  std::vector<uint64_t> TA, TAi, TB, TBi;  // 2^(1/n) powers; TAi carries the 1/m factor
  std::vector<uint64_t> TWlo, TWhi;      // two-level omega_m table
  std::vector<uint64_t> UT1, UT2;        // omega_M1^e (e < M1), omega_M2^e (e < M2)
  // seam twiddles of the radix-8 kernels, laid out [b][k1][k2] so that a thread's 8 words are contiguous (64 B):
  // S2r[b*64+ka] = omega_4096^(ka*b) (rows of 4096 = 64 x 64), S1r[b*(M1/64)+ka] = omega_M1^(ka*b) (columns M1 = 512/1024/2048 = (M1/64) x 64); *i = inverses
  std::vector<uint64_t> S2r, S2ri, S1r, S1ri;
  // register-resident column kernels: one word per (tile, thread) with 2 bits per digit of the thread's 16
  // digits (run d1 = 0..R-1 of i1 = 512 d1 + t, digit k of the run at bits 2 (d1 2C + k)): width - q, wrap
  std::vector<uint32_t> DI;
  uint64_t I4 = 0, I4inv = 0;            // omega_4, omega_4^-1 (forward root convention)
  uint64_t W5[5] = {1, 0, 0, 0, 0}, W5i[5] = {1, 0, 0, 0, 0};
  uint64_t W5c[4] = {0, 0, 0, 0};        // 5-point DFT constants {beta, k1, k2-k1, k1+k2} (kernels.hip dft5)

  size_t tiles() const { return M2 / C; }
  size_t runs() const { return tiles() * M1; }

  // width of digit with s = p*j mod n   (derivation: DESIGN.md "digit widths on the fly")
  uint32_t width_of_s(uint64_t s) const {
    return q + ((s + t > 0) ? 1u : 0u) + ((s + t > n) ? 1u : 0u) - ((s > 0) ? 1u : 0u);
  }
  uint32_t width(size_t j) const { return width_of_s((uint64_t(p) * j) % n); }

  // memory position (u32 index) of natural digit j inside a register (tile-major)
  size_t pos(size_t j) const {
    const size_t i = j >> 1, b = j & 1;
    const size_t i1 = i / M2, i2 = i % M2;
    const size_t T = i2 / C, c = i2 % C;
    return ((T * M1 + i1) * C + c) * 2 + b;
  }

  std::string describe() const {
    char buf[160];
    std::snprintf(buf, sizeof buf, "marin-hip:n=%zu:m1=%u:m2=%u:c=%u%s", n, M1, M2, C, split5 ? ":split5" : "");
    return std::string(buf) + (lanes > 1 ? ":lanes=" + std::to_string(lanes) : std::string()) + (onelaunch ? ":onelaunch" : "");
  }
};

// Whether the back sweeps' fused x a (adc_mul, marin.cl:194-201: carry = (r >> w) + (u >> w) a in 64 bits) is exact for factor a on a
// plan with digit widths q / q + 1, n digits and runs of 2C digits.  The inputs it covers: every digit j below 2^w_j, its OWN width (q or
// q + 1), except the one per run that keeps the remainder of a carry-in (apply_carry_in / run_carry_in: three digits absorb it, the fourth
// keeps the rest: digit E).  It does NOT cover "2^(q+1) - 1 on every digit", although the terms below are written with D = 2^(q+1) - 1: the
// unweighted coefficient is z_k = sum x_i x_j 2^c(i,j) with c in {0, 1} the carry of the two weight exponents (sum_product_ok below), and
// the terms leave that factor 2 out.  With digits inside their own widths two things make up for it: a narrow digit is below D / 2, and
// chi = U >> q shifts by the narrow width where most digits of a full range are wide.  At the top of a range, all digits at their maximum,
// the exact carry word at a_fast reaches 0.9999 of 2^64 and stays below it; with 2^(q+1) - 1 on every digit it passes 2^64 (p = 44497: 1.27).
// tests/chain_model.py is the exact chain, tests/test_factor_bound_cases.py holds both findings and the first factor that overflows.
//   convolution sum  u ~ sum x_i^2 (Cauchy-Schwarz) = (n - n/2C) D^2 + (n/2C) E^2, which must stay below the field prime;
//   back sweep       r = dlo a + carry + addend (< 2^32) and carry' = (r >> q) + (u >> q) a below 2^64 at the carry's fixed point;
//   next sweep       E = D + (carry >> 3q) + 3, the digit the carry word leaves behind (below 2^31, so that x a fits k_scale too).
// Runs of two digits (C = 1) take their carries at once and the local carry passes restore the digits (Engine::carry_fix_now, sized for
// a <= 15): only the 64-bit terms are checked there, and a_fast is capped at 15.
// mult: the convolution bound times mult (sum_product_ok below: dst x (y1 + y2) with factor 1).
inline bool carry_chain_ok(uint32_t q, size_t n, uint32_t C, uint64_t a, unsigned mult) {
  typedef unsigned __int128 u128;
  const u128 field = (u128(1) << 64) - (u128(1) << 32) + 1, lim = u128(1) << 64;
  const u128 D = (u128(1) << (q + 1)) - 1;
  const size_t runs = n / (2 * size_t(C));
  u128 E = D;
  for (int it = 0; it < 64; ++it) {
    const u128 U = u128(mult) * ((C >= 2) ? u128(n - runs) * D * D + u128(runs) * E * E : u128(n) * D * D);
    if (U >= field) return false;
    const u128 chi = U >> q;
    u128 c = 0;
    for (int k = 0; k < 4096; ++k) {   // carry_{k+1} = f(carry_k) rises to its fixed point, which bounds every run
      const u128 r = D * a + c + (u128(1) << 32);
      if (r >= lim) return false;
      const u128 c2 = (r >> q) + chi * a;
      if (c2 >= lim) return false;
      if (c2 == c) break;
      c = c2;
    }
    if (C < 2) return true;
    const u128 E2 = D + (c >> (3 * q)) + 3;
    if (E2 >= (u128(1) << 31)) return false;
    if (E2 <= E) return true;
    E = E2;
  }
  return false;
}
inline bool fused_factor_ok(uint32_t q, size_t n, uint32_t C, uint64_t a) { return carry_chain_ok(q, n, C, a, 1); }

// Whether dst x (y1 + y2), the row sweeps' multiply-by-the-sum-of-two-images (kernels.hpp, mode 3), is exact as ONE product.  The summed
// multiplicand has digits up to 2 D (and 2 E, the run-remainder digit, once per run), the residue side D and E as before: by Cauchy-Schwarz
// on two vectors of equal bound sum x_i (2 y_i) <= 2 ((n - n/2C) D^2 + (n/2C) E^2).  The unweighted coefficient is z_k = sum x_i y_j 2^c(i,j)
// with c = e_i + e_j - e_k in {0, 1} (e_j = ceil(p j / n) - p j / n, the exponent of digit j's weight), so the bound on z_k is twice that
// again.  (fused_factor_ok leaves this factor out: for one operand pair it is the bit the size rule 2 (q + 1) + log2 n < 64 keeps free.  Here
// it decides: near the top of a range, where almost every digit is wide, about half the pairs have c = 1, and all-ones operands at
// p = 204799 overflow the field with the doubled multiplicand.)  So: the model above at factor 1 with the convolution bound times 4,
// iterated to the fixed point of E (the result is the next operation's input on either side).  Crude form: 2 (q + 1) + 1 + log2 n < 64 --
// one bit more than the size rule, so the largest exponents of a transform size with odd log2 n, and of some 5 2^k sizes, do not have it.
// Runs of two digits: the carry passes are sized for a factor of 15, the doubling is 2.
inline bool sum_product_ok(uint32_t q, size_t n, uint32_t C) { return carry_chain_ok(q, n, C, 1, 4); }

// Kernel variants of the column sweeps (front and back) and of the row sweep.
enum class ColKernels : uint8_t {
  kGeneric,                      // kernels.hip k_front, k_back<EXT>: every shape whose columns fit LDS
  kSplit,                        // kernels.hip k_front_split_a/b, k_back_split_a/b: columns of 5 L1 pairs beyond LDS (split5)
  kRadix8R1, kRadix8R2, kRadix8R4,   // kernels_v2.hip k1_cols<R>, k3_cols<R, EXT>: M1 = 512 R, M1 C = 4096
  kRadix4Pairs, kRadix4Planes,   // kernels_v3.hip k1_cols256<Form>, k3_cols256<Form, EXT>: 256 x 4
  kRadix5, kRadix5J1,            // kernels_v5.hip k1_cols5<J>, k3_cols5<J, EXT>: 1280 x 4 (J = 0), 2560 x 2 (J = 1)
};
enum class RowKernels : uint8_t {
  kGeneric,                      // kernels.hip k_middle
  kRadix4Pairs, kRadix4Planes,   // kernels_v3.hip k2_rows1024<Form, mode>: rows of 1024
  kRadix8,                       // kernels_v2.hip k2_rows<Pairs, mode, 1, 0>: rows of 4096
  kRadix8Wide,                   // k2_rows<Pairs, mode, 2, 0>: rows of 8192 as two 4096-point halves, 1024 threads
  kRows2048One, kRows2048Two,    // k2_rows<Planes, mode, 1, 1> (one row per tile), k2_rows<Pairs, mode, 1, 1> (two rows per tile)
};

struct KernelChoice {
  ColKernels cols = ColKernels::kGeneric;
  RowKernels rows = RowKernels::kGeneric;
  bool resident_cols() const { return cols != ColKernels::kGeneric && cols != ColKernels::kSplit; }   // register-resident column kernels
  bool fused_back() const { return cols != ColKernels::kSplit; }   // a back sweep with extras (kernels.hpp BackExt)
};

// The kernels that serve a shape (r5, M1, M2, C, split5); the first matching rule wins.  make_plan builds the seam and digit-info tables
// of exactly these, choose_kernels narrows them.
//   radix-4 columns: one plane per thread where the tiles make a single round (at most two per CU), else a pair per thread;
//   radix-4 rows: one plane per thread with one row per CU or fewer (the pair form takes 12.8 us at C2 against 10.6 us for the generic
//     rows), a pair per thread above (n = 5 2^19: 26.0 against 30.1 us); profiles/r04_ab_radix4_set.txt has the same-box A/B of both;
//   rows of 2048: two to a tile (n = 2^21: 0.0645 -> 0.0577 ms, n = 5 2^20: 0.130 -> 0.120 ms against the generic rows,
//     profiles/r03_summary.md), but one row per tile below 512 rows and at 1280 rows, where 640 two-row tiles are 1.25 rounds of the chip
//     (0.0428 -> 0.0378 ms at n = 2^20, 0.1182 -> 0.1137 at 5 2^20, 0.0571 -> 0.0586 at n = 2^21: profiles/r04_ab_rows2048_planes.txt).
inline KernelChoice served_kernels(uint32_t r5, uint32_t M1, uint32_t M2, uint32_t C, bool split5) {
  KernelChoice k;
  if (split5) k.cols = ColKernels::kSplit;
  else if (r5 == 5 && ((M1 == 1280 && C == 4) || (M1 == 2560 && C == 2)) && M2 >= 8)
    k.cols = M1 == 2560 ? ColKernels::kRadix5J1 : ColKernels::kRadix5;
  else if (r5 == 1 && M1 == 256 && C == 4 && M2 >= 8)
    k.cols = M2 / 4 <= 512 ? ColKernels::kRadix4Planes : ColKernels::kRadix4Pairs;
  else if (r5 == 1 && (M1 == 512 || M1 == 1024 || M1 == 2048) && M1 * C == 4096 && M2 >= 2 * C)
    k.cols = M1 == 512 ? ColKernels::kRadix8R1 : M1 == 1024 ? ColKernels::kRadix8R2 : ColKernels::kRadix8R4;
  if (M2 == 1024) k.rows = M1 < 512 ? RowKernels::kRadix4Planes : RowKernels::kRadix4Pairs;
  else if (M2 == 4096) k.rows = RowKernels::kRadix8;
  else if (M2 == 8192) k.rows = RowKernels::kRadix8Wide;
  else if (M2 == 2048 && (M1 < 512 || M1 == 1280)) k.rows = RowKernels::kRows2048One;
  else if (M2 == 2048 && M1 % 2 == 0 && M1 >= 512) k.rows = RowKernels::kRows2048Two;
  return k;
}

// threads per tile of the register-resident column kernels (the digit-info words and four-step tables are [tile][thread]); 0: none
inline uint32_t threads_per_tile(ColKernels c) {
  switch (c) {
    case ColKernels::kRadix8R1: case ColKernels::kRadix8R2: case ColKernels::kRadix8R4: return 512;
    case ColKernels::kRadix4Pairs: case ColKernels::kRadix4Planes: return 256;
    case ColKernels::kRadix5: case ColKernels::kRadix5J1: return 640;
    default: return 0;
  }
}

inline uint32_t fused_factor_limit(uint32_t q, size_t n, uint32_t C) {
  uint64_t lo = 1, hi = 0xffffffffu;
  if (!fused_factor_ok(q, n, C, 1)) return 1;   // (never for a plan of the size rule; factor 1 is the plain squaring either way)
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (fused_factor_ok(q, n, C, mid)) lo = mid; else hi = mid - 1;
  }
  return uint32_t(C >= 2 ? lo : std::min<uint64_t>(lo, 15));
}

constexpr uint32_t kMaxLanes = 65535;   // the lane is blockIdx.y

// One-launch products (plan token onelaunch; kernels.hip k_onelaunch): a work-group holds K whole lanes with TL threads each, and per lane
// the work buffer and as much transform scratch, m pairs of 16 bytes each, in LDS.
//   TL: one thread per pair, up to 1024 threads -- 640 where the transform has a radix-5 stage: TL keeps the factor 5 of m = 5 2^k, so that
//       the lane's threads split evenly into teams over its M1 = 5 L1 rows as well as over its M2 / C tiles;
//   K:  the lanes that make a group of about 256 threads where a lane has fewer, but no more than the lane count rounded up to a power of two.
// 32 m K bytes of LDS: 128 KiB at n = 8192 (K = 1), at most 8 KiB wherever K > 1.
constexpr size_t kOneLaunchMaxN = 8192;
struct OneLaunchShape { uint32_t TL, K, groups; size_t lds; };
inline OneLaunchShape onelaunch_shape(size_t m, uint32_t r5, uint32_t lanes) {
  OneLaunchShape s;
  s.TL = uint32_t(std::min<size_t>(m, r5 == 5 ? 640 : 1024));
  uint32_t cap = 1;
  while (cap < lanes) cap <<= 1;
  s.K = std::min(std::max(1u, 256u / s.TL), cap);
  s.groups = (lanes + s.K - 1) / s.K;
  s.lds = size_t(s.K) * m * 32;
  return s;
}

// spec: "" (auto) or comma/colon separated "m2=<pow2>", "c=<pow2>", "lanes=<1..65535>", "onelaunch"
inline Plan make_plan(uint32_t p, const char* spec = nullptr, bool build_tables = true) {
  if (p < 3) throw std::runtime_error("exponent must be >= 3");
  Plan pl;
  pl.p = p;
  pl.n = transform_size(p);
  if (pl.n == size_t(-1)) throw std::runtime_error("exponent too large for the Goldilocks IBDWT");
  pl.m = pl.n / 2;
  pl.r5 = (pl.m % 5 == 0) ? 5 : 1;
  const int k = ilog2(pl.m / pl.r5);

  long want_m2 = -1, want_c = -1;
  bool want_split = false;
  if (spec && *spec) {
    std::string s(spec);
    for (size_t i = 0; i < s.size();) {
      size_t e = s.find_first_of(",:; ", i);
      if (e == std::string::npos) e = s.size();
      const std::string tok = s.substr(i, e - i);
      if (tok.rfind("m2=", 0) == 0) want_m2 = std::atol(tok.c_str() + 3);
      else if (tok.rfind("c=", 0) == 0) want_c = std::atol(tok.c_str() + 2);
      else if (tok == "split5") want_split = true;   // tests: the split column sweeps at a small 5 2^k size
      else if (tok.rfind("lanes=", 0) == 0) {
        const std::string v = tok.substr(6);
        if (v.empty() || v.size() > 5 || v.find_first_not_of("0123456789") != std::string::npos || std::atol(v.c_str()) < 1 || std::atol(v.c_str()) > long(kMaxLanes))
          throw std::runtime_error("bad lanes in plan spec: '" + tok + "' (lanes=1 .. lanes=" + std::to_string(kMaxLanes) + ")");
        pl.lanes = uint32_t(std::atol(v.c_str()));
      }
      else if (tok == "onelaunch") pl.onelaunch = true;
      else if (!tok.empty() && tok != "marin-hip" && tok.rfind("n=", 0) != 0 && tok.rfind("m1=", 0) != 0)
        throw std::runtime_error("unknown plan token '" + tok + "'");
      i = e + 1;
    }
  }

  if (pl.onelaunch && pl.n > kOneLaunchMaxN)
    throw std::runtime_error("onelaunch: a residue and its work buffer must fit the LDS of one CU, n <= " + std::to_string(kOneLaunchMaxN) + " (p <= 204799); n = " + std::to_string(pl.n) + " here");

  // rows vs columns: balance the work-group counts of the row sweep (M1 groups) and the column
  // sweeps (M2/C groups), keep a row <= 4096 pairs (64 KiB of LDS) and a column <= 1024 (x r5)
  int b = (k + 3) / 2;
  const int bmin = k - (pl.r5 == 5 ? 8 : 10);
  if (b < bmin) b = bmin;
  if (b > 12) b = 12;
  if (b > k) b = k;
  if (b < 1) b = 1;
  if (want_m2 > 0) {
    b = ilog2(size_t(want_m2));
    if ((long(1) << b) != want_m2 || b > k || b < 1 || b > 13) throw std::runtime_error("bad m2 in plan spec");
  } else {
    // very large transforms: 8192-pair rows (128 KiB) so that M1 stays <= 2048 -- or 2560 = 5 x 512, which the register-resident radix-5
    // columns serve with runs of two pairs (kernels_v5.hip, J = 1): n = 5 2^22 runs as 2560 x 4096 instead of 1280 x 8192
    while ((pl.m >> b) > (pl.r5 == 5 ? 2560u : 2048u) && b < 13 && b < k) ++b;
    if (pl.r5 == 5 && (pl.m >> b) > 10240 && b < k) b = std::min(13, k);   // n = 5 2^26: rows of 8192, columns of 5 x 4096 (split sweeps)
  }
  pl.logM2 = uint32_t(b);
  pl.M2 = 1u << b;
  pl.M1 = uint32_t(pl.m / pl.M2);
  pl.L1 = pl.M1 / pl.r5;
  pl.logL1 = uint32_t(ilog2(pl.L1));
  // columns live in LDS on the generic kernel set: M1 x C pairs of 16 bytes within the 160 KiB of a CU; beyond that (n = 5 2^26:
  // 5 x 4096 pairs) the radix-5 stage goes through memory and only the L1 = M1 / 5 part needs LDS
  if (want_split && pl.r5 != 5) throw std::runtime_error("split5 needs a 5 * 2^k transform");
  pl.split5 = want_split || size_t(pl.M1) * 16 > 160 * 1024;
  if (pl.split5 && (pl.r5 != 5 || size_t(pl.L1) * 16 > 128 * 1024)) throw std::runtime_error("transform size not supported (columns beyond the split sweeps)");
  if (pl.split5 && pl.lanes > 1) throw std::runtime_error("lanes: not with the split column sweeps (split5)");

  // tile: up to 4096 pairs (64 KiB), runs of at most 16 pairs (256 B of the work buffer);
  // grow to 8192 pairs (128 KiB) when that is what C >= 4 needs
  uint32_t C = 1;
  while (C * 2 <= pl.M2 && size_t(pl.M1) * (C * 2) <= 4096 && C < 16) C *= 2;
  // (not for columns of 2048: the register-resident column kernels take them as 4096-pair tiles with C = 2)
  while (C < 4 && C * 2 <= pl.M2 && size_t(pl.M1) * (C * 2) <= 8192 && !(pl.r5 == 1 && pl.M1 == 2048)) C *= 2;
  while (C > 4 && pl.M2 / C < 256) C /= 2;   // mid-size transforms: enough tiles to fill 256 CUs
  // runs of two digits cannot absorb the run carries of a large transform (they leave log2(n) - 2 excess bits on a digit):
  // take C = 2 wherever the tile still fits the 160 KiB of LDS; beyond that the engine adds a local carry pass
  if (C == 1 && pl.M2 >= 2 && size_t(pl.M1) * 2 * 16 <= 160 * 1024 && pl.n >= (size_t(1) << 19)) C = 2;
  if (pl.split5) C = 1;
  // columns of 256 run on the register-resident radix-4 kernels with runs of four pairs (kernels_v3.hip): n = 2^20 as 256 x 2048 with
  // C = 4 takes 0.043 ms per squaring against 0.051 with C = 8 on the generic columns (round 4, profiles/r04_ab_radix4_set.txt)
  if (pl.r5 == 1 && pl.M1 == 256 && pl.M2 >= 8 && C > 4 && !pl.split5) C = 4;
  if (want_c > 0 && !pl.split5) {
    C = uint32_t(want_c);
    if ((C & (C - 1)) != 0 || C > pl.M2 || size_t(pl.M1) * C > 10240) throw std::runtime_error("bad c in plan spec");
  }
  pl.C = C;
  if (pl.onelaunch && pl.split5) throw std::runtime_error("onelaunch: not with the split column sweeps (split5)");
  if (pl.onelaunch && pl.C < 2) throw std::runtime_error("onelaunch: not with runs of two digits (c=1), whose carries go in at once through passes of their own");
  pl.lds_front = pl.split5 ? 0 : size_t(pl.M1) * pl.C * 16;
  pl.lds_mid = size_t(pl.M2) * 16;
  pl.q = uint32_t(p / pl.n);
  pl.t = uint32_t(p % pl.n);
  pl.a_fast = fused_factor_limit(pl.q, pl.n, pl.C);
  pl.sum_fast = sum_product_ok(pl.q, pl.n, pl.C);
  if (!build_tables) return pl;

  const size_t n = pl.n, m = pl.m;
  const uint64_t r = gf::root_of_two(n);   // 2^(1/n)
  const uint64_t om = gf::root_of_unity(m);
  const uint64_t inv_m = gf::inv(uint64_t(m) % gf::P);

  // entries [0, M1): digit 2*(M2*i1 + i2) + b split as SA[i1] + SB[2*i2 + b];  entries [M1, 2*M1): the odd
  // digit's "+p" moved to the i1 side, SA[M1 + i1] + SB[2*i2], so that both digits of a pair share the
  // column factor TB[2*i2] (the register-resident column kernels fold it into one four-step twiddle chain)
  pl.SA.resize(2 * size_t(pl.M1)); pl.TA.resize(2 * size_t(pl.M1)); pl.TAi.resize(2 * size_t(pl.M1));
  for (uint32_t i1 = 0; i1 < 2 * pl.M1; ++i1) {
    const uint64_t s0 = (uint64_t(2) * pl.M2 % n * (uint64_t(p) % n) % n * (i1 % pl.M1)) % n;
    const uint64_t s = (i1 < pl.M1) ? s0 : (s0 + pl.t) % n;
    pl.SA[i1] = uint32_t(s);
    pl.TA[i1] = gf::pow(r, (n - s) % n);
    pl.TAi[i1] = gf::mul(gf::inv(pl.TA[i1]), inv_m);
  }
  pl.SB.resize(2 * size_t(pl.M2)); pl.TB.resize(2 * size_t(pl.M2)); pl.TBi.resize(2 * size_t(pl.M2));
  for (uint32_t x = 0; x < 2 * pl.M2; ++x) {
    const uint64_t s = (uint64_t(p) * x) % n;
    pl.SB[x] = uint32_t(s);
    pl.TB[x] = gf::pow(r, (n - s) % n);
    pl.TBi[x] = gf::inv(pl.TB[x]);
  }
  pl.twh = uint32_t((ilog2(m) + 2) / 2);
  // (TWhi covers exponents below m + 2^20: the row kernels index it with label + M1 k, k < M2, and a frequency label of the prime-factor
  // columns -- kernels.hpp col_label -- is an unreduced 1536 k0 + 1025 kr < 2^20)
  const size_t lo_n = size_t(1) << pl.twh, hi_n = ((m + (size_t(1) << 20)) >> pl.twh) + 2;
  pl.TWlo.resize(lo_n); pl.TWhi.resize(hi_n);
  pl.TWlo[0] = 1; for (size_t i = 1; i < lo_n; ++i) pl.TWlo[i] = gf::mul(pl.TWlo[i - 1], om);
  const uint64_t step = gf::mul(pl.TWlo[lo_n - 1], om);
  pl.TWhi[0] = 1; for (size_t i = 1; i < hi_n; ++i) pl.TWhi[i] = gf::mul(pl.TWhi[i - 1], step);
  const uint64_t om1 = gf::pow(om, pl.M2), om2 = gf::pow(om, pl.M1);
  pl.UT1.resize(pl.M1); pl.UT1[0] = 1; for (uint32_t i = 1; i < pl.M1; ++i) pl.UT1[i] = gf::mul(pl.UT1[i - 1], om1);
  pl.UT2.resize(pl.M2); pl.UT2[0] = 1; for (uint32_t i = 1; i < pl.M2; ++i) pl.UT2[i] = gf::mul(pl.UT2[i - 1], om2);
  const KernelChoice kc = (pl.lanes > 1 || pl.onelaunch) ? KernelChoice{} : served_kernels(pl.r5, pl.M1, pl.M2, pl.C, pl.split5);   // (choose_kernels)
  if (kc.rows == RowKernels::kRadix8 || kc.rows == RowKernels::kRadix8Wide) {   // rows of 8192 = one radix-2 level over two 4096-point transforms
    const uint32_t st = pl.M2 / 4096;       // omega_4096 = omega_M2^st
    pl.S2r.resize(4096); pl.S2ri.resize(4096);
    for (uint32_t b = 0; b < 64; ++b) for (uint32_t ka = 0; ka < 64; ++ka) {
      const uint32_t e = ka * b;
      const uint32_t idx = b * 64 + (ka & 7) * 8 + (ka >> 3);   // [b][k1][k2], ka = k1 + 8 k2: a thread's 8 words are contiguous
      pl.S2r[idx] = pl.UT2[st * e]; pl.S2ri[idx] = pl.UT2[st * ((4096 - e) & 4095)];
    }
  }
  if (kc.rows == RowKernels::kRows2048One || kc.rows == RowKernels::kRows2048Two) {
    // rows of 2048 (kernels_v2.hip, RL = 1 and the one-row form): [b][k1][k2] with k1 = 4 row + k1', omega_2048^((k1' + 4 k2) b)
    pl.S2r.resize(4096); pl.S2ri.resize(4096);
    for (uint32_t b = 0; b < 64; ++b) for (uint32_t k1 = 0; k1 < 8; ++k1) for (uint32_t k2 = 0; k2 < 8; ++k2) {
      const uint32_t e = (((k1 & 3) + 4 * k2) * b) & 2047;
      pl.S2r[b * 64 + k1 * 8 + k2] = pl.UT2[e]; pl.S2ri[b * 64 + k1 * 8 + k2] = pl.UT2[(2048 - e) & 2047];
    }
  }
  const uint32_t tpt = threads_per_tile(kc.cols);
  if (tpt == 512) {   // radix-8 columns, M1 = 512 R = (8R) x 64
    const uint32_t ka_n = pl.M1 / 64;
    pl.S1r.resize(pl.M1); pl.S1ri.resize(pl.M1);
    for (uint32_t b = 0; b < 64; ++b) for (uint32_t ka = 0; ka < ka_n; ++ka) {
      const uint32_t e = ka * b;
      const uint32_t Rr = pl.M1 / 512, idx = b * ka_n + (ka % Rr) * 8 + (ka / Rr);   // [b][k1][k2], ka = k1 + R k2
      pl.S1r[idx] = pl.UT1[e]; pl.S1ri[idx] = pl.UT1[(pl.M1 - e) & (pl.M1 - 1)];
    }
  }
  if (m % 4 == 0) { pl.I4 = gf::pow(om, m / 4); pl.I4inv = gf::inv(pl.I4); }
  else { pl.I4 = gf::root_of_unity(4); pl.I4inv = gf::inv(pl.I4); }
  if (tpt) {
    // digit-info words of the register-resident column kernels: thread t of tile T owns the runs i1 = t + tpt d1 (M1 / tpt runs of 2C digits;
    // radix-8: R runs of 16 / R digits, radix-4: one of eight, radix-5: two of eight or four of four), 2 bits per digit at 2 (d1 2C + k)
    const uint32_t NR = pl.M1 / tpt, ND = 2 * pl.C;
    pl.DI.assign(pl.tiles() * tpt, 0u);
    for (size_t T = 0; T < pl.tiles(); ++T)
      for (uint32_t t = 0; t < tpt; ++t) {
        uint32_t w = 0;
        for (uint32_t d1 = 0; d1 < NR; ++d1)
          for (uint32_t k = 0; k < ND; ++k) {
            const uint32_t i1 = tpt * d1 + t, i2 = uint32_t(T) * pl.C + (k >> 1);
            const uint64_t sb = pl.SB[2 * i2 + (k & 1)], s = (uint64_t(pl.SA[i1]) + sb) % n;
            const uint64_t wa = (k & 1) ? pl.SA[pl.M1 + i1] : pl.SA[i1], wb = pl.SB[2 * i2];   // the split the kernels weight with
            const uint32_t wbit = pl.width_of_s(s) - pl.q, wrap = (wa > 0 && wb > 0 && wa + wb <= n) ? 1u : 0u;
            w |= (wbit | (wrap << 1)) << (2 * (d1 * ND + k));
          }
        pl.DI[T * tpt + t] = w;
      }
  }
  if (pl.I4 != (uint64_t(1) << 48)) throw std::runtime_error("internal: omega_4 is expected to be 2^48");   // the kernels shift instead of multiplying
  if (pl.r5 == 5) {
    const uint64_t w5 = gf::pow(om, m / 5);
    for (int i = 0; i < 5; ++i) { pl.W5[i] = gf::pow(w5, uint64_t(i)); pl.W5i[i] = gf::inv(pl.W5[i]); }
    const uint64_t a = gf::add(pl.W5[1], pl.W5[4]), b = gf::add(pl.W5[2], pl.W5[3]);
    const uint64_t k1 = gf::half(gf::sub(pl.W5[1], pl.W5[4])), k2 = gf::half(gf::sub(pl.W5[2], pl.W5[3]));
    pl.W5c[0] = gf::half(gf::half(gf::sub(a, b))); pl.W5c[1] = k1; pl.W5c[2] = gf::sub(k2, k1); pl.W5c[3] = gf::add(k1, k2);
  }
  return pl;
}

// The kernels a plan runs: those that serve its shape, narrowed by MI355_KERNELS (A/B tests, debugging): unset or "v2" keeps them,
// "v2rows" / "v2cols" keep only the register-resident rows / columns, anything else takes the generic ones (the split sweeps stay).
inline KernelChoice choose_kernels(const Plan& pl, const char* mi355_kernels) {
  if (pl.lanes > 1) return KernelChoice{};   // lane engines run the generic set, whatever serves the shape (the only one that reads DevPlan.lanes)
  if (pl.onelaunch) return KernelChoice{};   // one-launch products are built from the generic bodies and write their registers and images
  KernelChoice k = served_kernels(pl.r5, pl.M1, pl.M2, pl.C, pl.split5);
  const std::string sel = mi355_kernels ? mi355_kernels : "v2";
  if (sel != "v2" && sel != "v2rows") k.rows = RowKernels::kGeneric;
  if (sel != "v2" && sel != "v2cols" && k.resident_cols()) k.cols = ColKernels::kGeneric;
  return k;
}

// The tag word that closes a raw register image (get_data / set_data / checkpoints; register_machine.hpp).  Bit 0 says what the register
// holds (0: digits, 1: a multiplicand image); bits 1 .. 63 are a fingerprint of everything the bytes in front of it depend on, so that an
// engine loads only what an engine of the same layout wrote: set_data refuses any other tag, a bare 0 / 1 of earlier versions included
// (bit 63 is always set: a fingerprint is never zero).  Switches that change neither the order nor the form of the stored words
// (MI355_TUNE, MI355_HOST_CARRY, and MI355_KERNELS for digits) are not part of it.
constexpr uint32_t kFamilyGoldilocks = 1, kFamilyCrt = 2;
inline uint64_t layout_tag(bool image, uint32_t family, uint32_t p, uint64_t n, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t flags, uint32_t form) {
  const uint64_t words[8] = {family, p, n, d1, d2, d3, flags, form};
  uint64_t h = 0x6d69333535746167ull;
  for (uint64_t w : words) {   // splitmix64's finaliser, chained over the fields: every field reaches every bit
    uint64_t z = (h ^ w) + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    h = z ^ (z >> 31);
  }
  return ((h | (uint64_t(1) << 63)) & ~uint64_t(1)) | (image ? 1u : 0u);
}
// Goldilocks registers.  Digits lie in tile-major order (Plan::pos): a function of (n, M1, M2, C); split5 decides C.  A multiplicand image
// is the work buffer as the row kernel's mode 2 leaves it: its words are in the form of that row kernel, and its rows in the order of the
// column sweeps' frequency labels (kernels.hpp col_label).  Every column kernel of a power-of-two transform leaves the rows bit-reversed;
// with a radix-5 stage each column variant has a label map of its own (Engine::Engine), so there the column variant belongs to the form.
inline uint64_t register_tag(const Plan& pl, const KernelChoice& kc, bool image) {
  const uint32_t form = image ? 1u + uint32_t(kc.rows) + (pl.r5 == 5 ? 8u * (1u + uint32_t(kc.cols)) : 0u) : 0u;
  return layout_tag(image, kFamilyGoldilocks, pl.p, pl.n, pl.M1, pl.M2, pl.C, pl.split5 ? 1u : 0u, form);
}

}  // namespace mi355
