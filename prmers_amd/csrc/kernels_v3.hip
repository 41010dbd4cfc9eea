// gfx950 kernels, register-resident radix-4 set ("v3") for the small transforms: tiles of 1024 pairs, 256 thread indices with 4 pairs each
// (256 or 512 lanes, depending on the lane form below).
//
// BASELINE configs[1] (p = 9815459, n = 2^19: columns of 256 with runs of four pairs, rows of 1024) is the shape the reference serves with
// forward1024_0 / sqr512 / backward1024_0 (kernels/marin.cl:1190,1517, schedule include/marin/engine_gpu.h:1591).  A 4096-pair tile of the
// radix-8 set (kernels_v2.hip) would give it 64 work-groups for 256 CUs, and that set's wave-specialised shift seams need eight waves per
// tile; the generic set (kernels.hip) keeps the tile in LDS and walks it with run-time loops: 10 passes per row transform, each with its
// table words on the critical path, about twice the instructions per word.  Here a tile is held in registers by ONE wave per SIMD:
//   * rows of 1024 = 4.4.4.4.4 and columns of 256 = 4.4.4.4 as decimation-in-frequency radix-4 steps in registers (omega_4 = 2^48: add, sub
//     and one shift), LDS only for the digit-permuting exchanges between the steps (four per direction in a row, 3 + 1 in a column);
//   * the twiddle after a step is one table word per register from the universal omega_M1 / omega_M2 tables (2 KiB / 8 KiB, cache resident),
//     ALL requested at kernel entry, so that no exchange waits for memory: with one wave per SIMD nothing else would hide that latency;
//   * every exchange has its own LDS slot map, chosen conflict-free for the lane groups gfx950 serves 128-bit accesses in (stores: eight
//     groups of 8 lanes on 32 banks, loads: four non-contiguous groups of 16 lanes on 64 banks; census in tools/lds_census.py);
//   * digits, run carries, weights (TA / TB split, halved-weight bits in the DI table), the four-step twiddle chain and the work-buffer
//     row order are those of the other two sets, so the sets interoperate kernel by kernel.
// Shapes served: rows M2 = 1024 (any M1, also the 5 2^k sizes whose columns run on kernels_v5.hip); columns M1 = 256 with C = 4.
// Value ranges as in kernels_v2.hip: canonical values everywhere (P for a negated zero).
//
// Every kernel exists in two lane forms (plan.hpp served_kernels picks one), written once as a template on the form:
//   Pairs   a pair per thread (256 threads): the fewest instructions per word;
//   Planes  one plane per thread (512 threads: lane 2 t + plane, the two words of a pair go through identical, independent arithmetic):
//           where a CU gets one tile or fewer the launch lasts as long as one wave's dependent stream, and two waves per SIMD with half
//           the stream each are shorter than one.  Same stages, maps and table words; LDS slots are 8 bytes (2 map(i) + plane); a lane
//           meets its partner plane through a DPP lane swap (quad_perm 1,0,3,2).
#include "kernels_v2_common.hpp"

namespace mi355 {
namespace v3 {
using v2::P2;
using v2::lds_barrier;
using v2::mulw;

constexpr uint32_t kThreads = 256;   // thread indices t of a tile (lanes: see the forms)
constexpr uint32_t kLdsBytes = 1024 * 16;

// slot maps of the exchanges (16-byte slots of the 1024-pair tile)
__device__ __forceinline__ uint32_t m0(uint32_t i) { return i; }
__device__ __forceinline__ uint32_t m2(uint32_t i) { return i ^ ((i >> 2) & 15u); }
__device__ __forceinline__ uint32_t m3(uint32_t i) { return i ^ ((i >> 3) & 15u); }

// ---- lane forms: element type E, lanes per tile, thread index t and plane, at(i): address of pair index i in global memory and LDS alike,
// halves(tab): the element of a table split into 256 even-digit and 256 odd-digit words, edge: the slot map of the column kernels' exchange
// between run order and transform order (the one exchange whose map differs: each is conflict-free for its own slot width) ----
struct Pairs {
  using E = P2;
  static constexpr uint32_t kBlock = kThreads, pln = 0;
  const uint32_t t = threadIdx.x;
  template <class I> __device__ __forceinline__ I at(I i) const { return i; }
  __device__ __forceinline__ P2 halves(const uint64_t* __restrict__ tab) const { return {tab[t], tab[256 + t]}; }
  static __device__ __forceinline__ uint32_t edge(uint32_t i) { return m3(i); }
};
struct Planes {
  using E = uint64_t;
  static constexpr uint32_t kBlock = 2 * kThreads;
  const uint32_t t = threadIdx.x >> 1, pln = threadIdx.x & 1u;
  template <class I> __device__ __forceinline__ I at(I i) const { return 2 * i + pln; }
  __device__ __forceinline__ uint64_t halves(const uint64_t* __restrict__ tab) const { return tab[256 * pln + t]; }
  static __device__ __forceinline__ uint32_t edge(uint32_t i) { return m2(i); }
};
__device__ __forceinline__ uint64_t swap_planes(uint64_t v) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_update_dpp(0, int(uint32_t(v)), 0xB1, 0xF, 0xF, false));
  const uint32_t hi = uint32_t(__builtin_amdgcn_update_dpp(0, int(uint32_t(v >> 32)), 0xB1, 0xF, 0xF, false));
  return (uint64_t(hi) << 32) | lo;
}

// element arithmetic of the stages
template <bool INV>
__device__ __forceinline__ void dft4(P2 (&x)[4]) {
  v2::dft4<INV>(x[0].a, x[1].a, x[2].a, x[3].a);
  v2::dft4<INV>(x[0].b, x[1].b, x[2].b, x[3].b);
}
template <bool INV>
__device__ __forceinline__ void dft4(uint64_t (&x)[4]) { v2::dft4<INV>(x[0], x[1], x[2], x[3]); }
template <class E>
__device__ __forceinline__ void twiddle3(E (&x)[4], const uint64_t (&w)[3]) {
#pragma unroll
  for (int k = 1; k < 4; ++k) x[k] = mulw(x[k], w[k - 1]);
}

// the digit fields of a thread index as the stages see it
__device__ __forceinline__ uint32_t hi2(uint32_t t) { return t >> 6; }          // top digit
__device__ __forceinline__ uint32_t d2nd(uint32_t t) { return (t >> 4) & 3u; }
__device__ __forceinline__ uint32_t d3rd(uint32_t t) { return (t >> 2) & 3u; }
// tile index of (top | second | third | fourth = j | low two bits of t) and friends: the five base-4 digits of a tile element
__device__ __forceinline__ uint32_t idx_a(uint32_t t, uint32_t j) { return 256u * j + t; }                                         // (j | t)
__device__ __forceinline__ uint32_t idx_b(uint32_t t, uint32_t j) { return 256u * hi2(t) + 64u * j + (t & 63u); }                  // (t7..6 | j | t5..0)
__device__ __forceinline__ uint32_t idx_c(uint32_t t, uint32_t j) { return 256u * hi2(t) + 64u * d2nd(t) + 16u * j + (t & 15u); }  // (t7..4 | j | t3..0)
__device__ __forceinline__ uint32_t idx_d(uint32_t t, uint32_t j) { return (t & ~3u) * 4u + 4u * j + (t & 3u); }                   // (t7..2 | j | t1..0)
__device__ __forceinline__ uint32_t idx_e(uint32_t t, uint32_t j) { return 4u * t + j; }                                           // (t | j)

// one exchange through LDS: register k goes to tile element WI(t, k), register j comes from element RI(t, j), slots by MAP
using Idx = uint32_t (*)(uint32_t, uint32_t);
using Map = uint32_t (*)(uint32_t);
template <Idx WI, Idx RI, Map MAP, class Form>
__device__ __forceinline__ void exchange(const Form& f, typename Form::E (&x)[4]) {
  typename Form::E* X = reinterpret_cast<typename Form::E*>(v2::smem_v2);
  lds_barrier();
#pragma unroll
  for (int k = 0; k < 4; ++k) X[f.at(MAP(WI(f.t, k)))] = x[k];
  lds_barrier();
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = X[f.at(MAP(RI(f.t, j)))];
}

// The three twiddled stages that rows and columns share.  Tile element e = 256 d1 + 64 d2 + 16 d3 + (low four bits); thread t keeps its
// index, the registers hold:
//   d1 (elements 256 j + t)        -> k1 ; x w[0]
//   d2 (k1 = t7..6, rest t5..0)     -> k2 ; x w[1]
//   d3 (k1, k2 = t5..4, rest t3..0) -> k3 ; x w[2]     and the exchange to (k1, k2, k3 = t3..2 | j | t1..0)
// inverse3 is the mirror image with the inverse table words.
template <class Form, int NS>
__device__ __forceinline__ void forward3(const Form& f, typename Form::E (&x)[4], const uint64_t (&w)[NS][3]) {
  dft4<false>(x); twiddle3(x, w[0]); exchange<idx_a, idx_b, m0>(f, x);
  dft4<false>(x); twiddle3(x, w[1]); exchange<idx_b, idx_c, m0>(f, x);
  dft4<false>(x); twiddle3(x, w[2]); exchange<idx_c, idx_d, m2>(f, x);
}
template <class Form, int NS>
__device__ __forceinline__ void inverse3(const Form& f, typename Form::E (&x)[4], const uint64_t (&v)[NS][3]) {
  exchange<idx_d, idx_c, m2>(f, x); twiddle3(x, v[2]); dft4<true>(x);
  exchange<idx_c, idx_b, m0>(f, x); twiddle3(x, v[1]); dft4<true>(x);
  exchange<idx_b, idx_a, m0>(f, x); twiddle3(x, v[0]); dft4<true>(x);
}

// ---------------------------------------------------------------------------------------------
// middle, M2 = 1024 = 4.4.4.4.4.  Element e = 256 d1 + 64 d2 + 16 d3 + 4 d4 + d5:
//   S1 d1 -> k1 ; x omega_1024^(k1 t)         S2 d2 -> k2 ; x omega_256^(k2 (t & 63))        S3 d3 -> k3 ; x omega_64^(k3 (t & 15))
//   S4 d4 (k1, k2, k3 = t3..2, d5 = t1..0) -> k4 ; x omega_16^(k4 (t & 3))
//   S5 d5 (k1, k2, k3, k4 = t1..0)         -> k5 ; X[k], k = k1 + 4 k2 + 16 k3 + 64 k4 + 256 k5
// pointwise in registers (rho = rho0 omega_4^k5), then the mirror image back to natural order.
// mode 0: square, 1: multiply by image Y, 2: forward only (writes the image: register j of thread t at pair 256 j + t),
// 3: multiply by the word-wise sum of the images Y and Y2 (mode 1 with y = Y[i] + Y2[i], gf::add_lazy_any),
// 4: mode 0 that first stores what mode 2 would store to Wimg (the image of the operand, from the registers the pointwise stage reads next).
// ---------------------------------------------------------------------------------------------
struct RowWords { uint64_t w[4][3], v[4][3]; };   // omega_1024^e after S1 .. S4, and their inverses
// every table word of the kernel is requested at its entry: nothing after the first exchange waits for memory again
template <bool INVERSE_TOO>
__device__ __forceinline__ void rows_prefetch(const uint64_t* __restrict__ UT, uint32_t t, RowWords& tw) {
#pragma unroll
  for (uint32_t k = 1; k < 4; ++k) {
    const uint32_t e[4] = {k * t, 4 * k * (t & 63u), 16 * k * (t & 15u), 64 * k * (t & 3u)};
#pragma unroll
    for (int s = 0; s < 4; ++s) tw.w[s][k - 1] = UT[e[s]];
    if (INVERSE_TOO) {
#pragma unroll
      for (int s = 0; s < 4; ++s) tw.v[s][k - 1] = UT[(1024 - e[s]) & 1023];
    }
  }
}
template <class Form>
__device__ __forceinline__ void rows_forward(const Form& f, typename Form::E (&x)[4], const RowWords& tw) {
  forward3(f, x, tw.w);
  dft4<false>(x); twiddle3(x, tw.w[3]); exchange<idx_d, idx_e, m2>(f, x);
  dft4<false>(x);
}
template <class Form>
__device__ __forceinline__ void rows_inverse(const Form& f, typename Form::E (&x)[4], const RowWords& tw) {
  dft4<true>(x);
  exchange<idx_e, idx_d, m2>(f, x); twiddle3(x, tw.v[3]); dft4<true>(x);
  inverse3(f, x, tw.v);
}

// pointwise: register k5 holds X[kb + 256 k5]; rho = rho0 omega_4^k5 = rho0 {1, 2^48, -1, -2^48}.  Y, Y2: the images, base: the row's first word
template <int mode>
__device__ __forceinline__ void pointwise(const Pairs& f, P2 (&x)[4], uint64_t rho0, const uint64_t* __restrict__ Y, const uint64_t* __restrict__ Y2, size_t base) {
#pragma unroll
  for (int k5 = 0; k5 < 4; ++k5) {
    const P2 u = x[k5];
    P2 r;
    uint64_t q, s0;
    if (mode == 0) {   // (u0 + u1 t)^2 mod (t^2 - rho), marin.cl:379-384
      q = gf::mul(gf::sqr(u.b), rho0);
      s0 = gf::sqr(u.a);
      r.b = gf::dbl(gf::mul(u.b, u.a));
    } else {           // marin.cl:387-392
      P2 y = reinterpret_cast<const P2*>(Y + base)[256 * k5 + f.t];
      if (mode == 3) {
        const P2 z = reinterpret_cast<const P2*>(Y2 + base)[256 * k5 + f.t];
        y = {gf::add_lazy_any(y.a, z.a), gf::add_lazy_any(y.b, z.b)};
      }
      q = gf::mul(gf::mul(u.b, y.b), rho0);
      s0 = gf::mul(u.a, y.a);
      r.b = gf::add(gf::mul(u.a, y.b), gf::mul(u.b, y.a));
    }
    if (k5 & 1) q = gf::mul_pow2(q, 48);
    r.a = (k5 & 2) ? gf::sub(s0, q) : gf::add(s0, q);
    x[k5] = r;
  }
}
// lane a holds u.a, lane b holds u.b: every lane computes its own square / product, the product by rho travels from the b lane to the a lane
template <int mode>
__device__ __forceinline__ void pointwise(const Planes& f, uint64_t (&x)[4], uint64_t rho0, const uint64_t* __restrict__ Y, const uint64_t* __restrict__ Y2, size_t base) {
#pragma unroll
  for (int k5 = 0; k5 < 4; ++k5) {
    const uint64_t u = x[k5], uo = swap_planes(u);
    uint64_t m1, cross;
    if (mode == 0) {   // (u0 + u1 t)^2 mod (t^2 - rho), marin.cl:379-384
      m1 = gf::sqr(u);                      // a: u.a^2, b: u.b^2
      cross = gf::dbl(gf::mul(u, uo));      // 2 u.a u.b (both lanes)
    } else {           // marin.cl:387-392
      uint64_t y = (Y + base)[f.at(256 * k5 + f.t)];
      if (mode == 3) y = gf::add_lazy_any(y, (Y2 + base)[f.at(256 * k5 + f.t)]);
      const uint64_t yo = swap_planes(y);
      m1 = gf::mul(u, y);                   // a: u.a y.a, b: u.b y.b
      const uint64_t mx = gf::mul(u, yo);   // a: u.a y.b, b: u.b y.a
      cross = gf::add(mx, swap_planes(mx));
    }
    uint64_t q = swap_planes(gf::mul(m1, rho0));   // lane a receives u.b^2 rho0 (u.b y.b rho0)
    if (k5 & 1) q = gf::mul_pow2(q, 48);
    const uint64_t ra = (k5 & 2) ? gf::sub(m1, q) : gf::add(m1, q);
    x[k5] = f.pln ? cross : ra;
  }
}

template <class Form, int mode>
__global__ void __launch_bounds__(Form::kBlock) k2_rows1024(DevPlan pl, const uint64_t* __restrict__ Win, const uint64_t* __restrict__ Yimg,
                                                            const uint64_t* __restrict__ Yimg2, uint64_t* __restrict__ Wimg, uint64_t* __restrict__ Wout) {
  using E = typename Form::E;
  const Form f;
  const uint32_t t = f.t, row = blockIdx.x;
  const size_t base = size_t(row) * 2048;   // words of a row, either form
  const E* in = reinterpret_cast<const E*>(Win + base);
  E* out = reinterpret_cast<E*>(Wout + base);
  E x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = in[f.at(256 * j + t)];
  RowWords tw;
  rows_prefetch<mode != 2>(pl.UT2, t, tw);
  // rho0 = omega_m^(k1row + M1 kb): row frequency of the thread's register 0 after S5 (kernels.hip freq1 for the row's own frequency)
  const uint32_t kb = hi2(t) + 4 * d2nd(t) + 16 * d3rd(t) + 64 * (t & 3u);
  const uint32_t blk = row / pl.L1, qq = row - blk * pl.L1;
  const uint32_t k1row = col_label(pl, blk, pl.logL1 ? (__brev(qq) >> (32 - pl.logL1)) : 0u);
  const uint64_t erho = rho_exponent(pl, k1row, kb);
  uint64_t rho_lo = 0, rho_hi = 0;
  if (mode != 2) { rho_lo = pl.TWlo[erho & ((1u << pl.twh) - 1)]; rho_hi = pl.TWhi[erho >> pl.twh]; }

  rows_forward(f, x, tw);
  if (mode == 4) {
    E* img = reinterpret_cast<E*>(Wimg + base);
#pragma unroll
    for (int j = 0; j < 4; ++j) img[f.at(256 * j + t)] = x[j];
  }
  if (mode != 2) {
    pointwise<(mode == 4 ? 0 : mode)>(f, x, gf::mul(rho_lo, rho_hi), Yimg, Yimg2, base);
    rows_inverse(f, x, tw);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[f.at(256 * j + t)] = x[j];
}

// ---------------------------------------------------------------------------------------------
// Column tiles, M1 = 256 = 4.4.4.4 with C = 4 pairs per run (tile = 1024 pairs).  Tile element (i1, c), i1 = 64 d1 + 16 d2 + 4 d3 + d4,
// tile index 4 i1 + c (five base-4 digits d1 | d2 | d3 | d4 | c).
// front (digits -> work buffer):
//   S0 thread i1 = t, registers c: one run of 8 digits -> weight                    ; exchange (t | c) -> (d1 | t)
//   S1 thread (d2 d3 d4 | c) regs d1 -> k1 ; x omega_256^(k1 (t >> 2))
//   S2 thread (k1 | d3 d4 | c) regs d2 -> k2 ; x omega_64^(k2 ((t >> 2) & 15))
//   S3 thread (k1 k2 | d4 | c) regs d3 -> k3 ; x omega_16^(k3 ((t >> 2) & 3))
//   S4 thread (k1 k2 k3 | c)   regs d4 -> k4 ; k1col = k1 + 4 k2 + 16 k3 + 64 k4
//   then the four-step twiddle omega_m^(i2 k1col) * TB (geometric in k4: one chain multiply per pair) and the store to work-buffer row
//   bitrev(k1col), column i2 = 4 T + c.
// back is the mirror image, followed by unweight and the sequential carry of the thread's run.
// Planes: plane a = the even digits of the run, plane b the odd ones; both lanes of a pair load the run and compute its carry-in / carry
// chain (a few integer instructions), each weights, transforms and twiddles its own plane.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rev2(uint32_t k) { return ((k & 1u) << 1) | (k >> 1); }

// table words first: omega_256^e after S1 .. S3 (INV: their inverses)
template <bool INV>
__device__ __forceinline__ void cols_prefetch(const uint64_t* __restrict__ UT, uint32_t t, uint64_t (&w)[3][3]) {
#pragma unroll
  for (uint32_t k = 1; k < 4; ++k) {
    const uint32_t e[3] = {k * (t >> 2), 4 * k * ((t >> 2) & 15u), 16 * k * ((t >> 2) & 3u)};
#pragma unroll
    for (int s = 0; s < 3; ++s) w[s][k - 1] = UT[INV ? (256 - e[s]) & 255 : e[s]];
  }
}
template <class Form>
__device__ __forceinline__ void cols_forward(const Form& f, typename Form::E (&x)[4], const uint64_t (&w)[3][3]) {
  exchange<idx_e, idx_a, Form::edge>(f, x);
  forward3(f, x, w);
  dft4<false>(x);
}
template <class Form>
__device__ __forceinline__ void cols_inverse(const Form& f, typename Form::E (&x)[4], const uint64_t (&v)[3][3]) {
  dft4<true>(x);
  inverse3(f, x, v);
  exchange<idx_a, idx_e, Form::edge>(f, x);
}
// the four-step chain over the thread's four rows: x[j] *= ca ratio^j
template <class E>
__device__ __forceinline__ void chain4(E (&x)[4], uint64_t ca, uint64_t ratio) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[j] = mulw(x[j], ca);
    if (j < 3) ca = gf::mul(ca, ratio);
  }
}

// digits -> weighted elements (v2::weigh_run; Planes: the same weights, this lane's plane of each pair)
__device__ __forceinline__ void weigh(const Pairs&, P2 tah, uint32_t nowrap, const uint32_t (&dg)[8], P2 (&x)[4]) { v2::weigh_run<8>(tah.a, tah.b, nowrap, 0, dg, x); }
__device__ __forceinline__ void weigh(const Planes& f, uint64_t tah, uint32_t nowrap, const uint32_t (&dg)[8], uint64_t (&x)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    // (a select between two elements of dg would be turned into a run-time index and put the array into scratch: mask arithmetic instead)
    const uint32_t d = dg[2 * c] ^ ((dg[2 * c] ^ dg[2 * c + 1]) & (0u - f.pln));
    const uint32_t sh = nowrap >> (4 * c + 1 + 2 * f.pln);
    x[c] = gf::mul_u32(tah, d << (sh & 1u));
  }
}

template <class Form>
__global__ void __launch_bounds__(Form::kBlock) k1_cols256(DevPlan pl, const uint32_t* __restrict__ digits, const uint64_t* __restrict__ cbuf_in,
                                                           uint64_t* __restrict__ Wout) {
  using E = typename Form::E;
  const Form f;
  const uint32_t t = f.t, T = blockIdx.x;
  uint64_t w[3][3];
  cols_prefetch<false>(pl.UT1, t, w);
  const uint32_t c4 = t & 3u, kb = hi2(t) + 4 * d2nd(t) + 16 * d3rd(t), i2 = 4 * T + c4;
  const uint64_t fca0 = pl.F0f[size_t(T) * kThreads + t], fB = pl.FBf[i2];   // chain start omega_m^(i2 kb) TB[2 i2], ratio omega_m^(64 i2)
  const uint32_t di = pl.DI[size_t(T) * kThreads + t];
  const E tah = f.halves(pl.TAh);
  uint32_t dg[8];
  v2::load_run(digits, size_t(T) * kThreads + t, dg);
  // compiler fence: the requests above stay at the kernel's entry (otherwise the table words move below the carry-in branch, behind the
  // wait for the digits, and the weights cost a second memory round trip)
  asm volatile("" ::: "memory");
  if (cbuf_in) v2::apply_carry_in<8>(pl, di, 0, v2::carry_in_of(pl, cbuf_in, T, t), dg);
  E x[4];
  weigh(f, tah, ~di, dg, x);
  cols_forward(f, x, w);
  chain4(x, fca0, fB);
  const uint32_t row0 = __brev(kb) >> 24;   // bitrev8(kb): its low 2 bits are zero
  E* W = reinterpret_cast<E*>(Wout);
#pragma unroll
  for (int j = 0; j < 4; ++j) W[f.at(size_t(row0 + rev2(j)) * pl.M2 + i2)] = x[j];
}

// transformed elements -> the run's eight values in digit order, unweighted (tai, or tai2 where the exponents wrapped: the weight was halved)
__device__ __forceinline__ void unweigh(const Pairs&, uint32_t di, P2 tai, P2 tai2, const P2 (&x)[4], uint64_t (&u)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool wrap = ((di >> (2 * k)) & 2u) != 0;   // digit-info table: width - q, wrap
    u[k] = (k & 1) ? gf::mul(x[k >> 1].b, wrap ? tai2.b : tai.b) : gf::mul(x[k >> 1].a, wrap ? tai2.a : tai.a);
  }
}
// this lane's plane (digit 2 c + plane of the run i1 = t), then both lanes take the partner's four values (the swaps stay outside the select
// between own and oth: a DPP read from a lane that a divergent branch has switched off returns nothing)
__device__ __forceinline__ void unweigh(const Planes& f, uint32_t di, uint64_t tai, uint64_t tai2, const uint64_t (&x)[4], uint64_t (&u)[8]) {
  uint64_t own[4], oth[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bool wrap = ((di >> (2 * (2 * c + int(f.pln)))) & 2u) != 0;
    own[c] = gf::mul(x[c], wrap ? tai2 : tai);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) oth[c] = swap_planes(own[c]);
#pragma unroll
  for (int k = 0; k < 8; ++k) u[k] = ((k & 1) == int(f.pln)) ? own[k >> 1] : oth[k >> 1];
}
// digits and carry word of run `run`; Planes: lane a stores the first four digits (and the carry word), lane b the last four
__device__ __forceinline__ void store_run(const Pairs&, uint32_t* __restrict__ digits, uint64_t* __restrict__ cbuf, size_t run, const uint32_t (&dg)[8], uint64_t carry) {
  v2::store_run(digits, run, dg);
  cbuf[run] = carry;
}
__device__ __forceinline__ void store_run(const Planes& f, uint32_t* __restrict__ digits, uint64_t* __restrict__ cbuf, size_t run, const uint32_t (&dg)[8], uint64_t carry) {
  uint4* dst = reinterpret_cast<uint4*>(digits) + run * 2;
  dst[f.pln] = f.pln ? make_uint4(dg[4], dg[5], dg[6], dg[7]) : make_uint4(dg[0], dg[1], dg[2], dg[3]);
  if (!f.pln) cbuf[run] = carry;
}

template <class Form, bool EXT>
__global__ void __launch_bounds__(Form::kBlock) k3_cols256(DevPlan pl, const uint64_t* __restrict__ Win, uint32_t* __restrict__ digits, uint64_t* __restrict__ cbuf,
                                                           uint32_t a, BackExt ext) {
  using E = typename Form::E;
  const Form f;
  const uint32_t t = f.t, T = v2::tile_of_block(pl, blockIdx.x, gridDim.x);
  uint64_t v[3][3];
  cols_prefetch<true>(pl.UT1, t, v);
  const uint32_t c4 = t & 3u, kb = hi2(t) + 4 * d2nd(t) + 16 * d3rd(t), i2 = 4 * T + c4;
  const uint32_t di = pl.DI[size_t(T) * kThreads + t];
  const E tai = f.halves(pl.TAi);
  const uint64_t ca = pl.F0i[size_t(T) * kThreads + t], B = pl.FBi[i2];   // chain start omega_m^-(i2 kb) TBi[2 i2], ratio omega_m^-(64 i2)
  const uint32_t row0 = __brev(kb) >> 24;
  const E* W = reinterpret_cast<const E*>(Win);
  E x[4];   // (requested before the addend run: one scheduling region for both would cost the pair form an occupancy step)
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = W[f.at(size_t(row0 + rev2(j)) * pl.M2 + i2)];
  uint32_t ad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (EXT && ext.add_digits) {
    v2::load_run(ext.add_digits, size_t(T) * kThreads + t, ad);
    if (ext.add_cbuf) v2::apply_carry_in<8>(pl, di, 0, v2::carry_in_of(pl, ext.add_cbuf, T, t), ad);
  }
  chain4(x, ca, B);
  cols_inverse(f, x, v);
  // unweight, x a, carry along the thread's run (i1 = t)
  uint64_t u[8];
  unweigh(f, di, tai, f.halves(pl.TAi2), x, u);
  uint64_t carry = 0;
  uint32_t dg[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) dg[k] = v2::adc_mul(u[k], a, EXT ? ad[k] : 0u, pl.q + ((di >> (2 * k)) & 1u), carry);
  store_run(f, digits, cbuf, size_t(T) * 256 + t, dg, carry);
  if (EXT && ext.digits2) store_run(f, ext.digits2, ext.cbuf2, size_t(T) * 256 + t, dg, carry);
}

// chain starts and ratios of the four-step twiddle chains (same thread map as the last stage of k1_cols256 / first stage of k3_cols256):
// F0f[T][t] = omega_m^(i2 kb) TB[2 i2], F0i the inverse with TBi, FBf[i2] = omega_m^(64 i2), FBi its inverse
__global__ void __launch_bounds__(kThreads) k_build_f0(DevPlan pl, uint64_t* __restrict__ f0f, uint64_t* __restrict__ f0i, uint64_t* __restrict__ fbf,
                                                       uint64_t* __restrict__ fbi) {
  const uint32_t t = threadIdx.x, T = blockIdx.x;
  const uint32_t c4 = t & 3u, kb = hi2(t) + 4 * d2nd(t) + 16 * d3rd(t), i2 = 4 * T + c4;
  const uint32_t ea = i2 * kb;
  f0f[size_t(T) * kThreads + t] = gf::mul(v2::tw_lookup(pl, ea), pl.TB[2 * i2]);
  f0i[size_t(T) * kThreads + t] = gf::mul(v2::tw_lookup(pl, ea ? pl.m - ea : 0), pl.TBi[2 * i2]);
  if (t < 4) {
    const uint32_t eb = i2 * 64;
    fbf[i2] = v2::tw_lookup(pl, eb);
    fbi[i2] = v2::tw_lookup(pl, eb ? pl.m - eb : 0);
  }
}

}  // namespace v3

// ------------------------------- launchers ---------------------------------------------------
template <class Form>
static hipError_t rows1024(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) {
  const dim3 grid(pl.M1), block(Form::kBlock);
  switch (mode) {
    case 0: hipLaunchKernelGGL((v3::k2_rows1024<Form, 0>), grid, block, v3::kLdsBytes, s, pl, Win, Y, Y2, Wimg, Wout); break;
    case 1: hipLaunchKernelGGL((v3::k2_rows1024<Form, 1>), grid, block, v3::kLdsBytes, s, pl, Win, Y, Y2, Wimg, Wout); break;
    case 2: hipLaunchKernelGGL((v3::k2_rows1024<Form, 2>), grid, block, v3::kLdsBytes, s, pl, Win, Y, Y2, Wimg, Wout); break;
    case 3: hipLaunchKernelGGL((v3::k2_rows1024<Form, 3>), grid, block, v3::kLdsBytes, s, pl, Win, Y, Y2, Wimg, Wout); break;
    case 4: hipLaunchKernelGGL((v3::k2_rows1024<Form, 4>), grid, block, v3::kLdsBytes, s, pl, Win, Y, Y2, Wimg, Wout); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t v3_rows1024_pairs(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) { return rows1024<v3::Pairs>(pl, Win, Y, Y2, Wimg, Wout, mode, s); }
hipError_t v3_rows1024_planes(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) { return rows1024<v3::Planes>(pl, Win, Y, Y2, Wimg, Wout, mode, s); }

template <class Form>
static hipError_t cols_front(const DevPlan& pl, const uint32_t* digits, const uint64_t* cbuf_in, uint64_t* W, hipStream_t s) {
  hipLaunchKernelGGL(v3::k1_cols256<Form>, dim3(pl.M2 / 4), dim3(Form::kBlock), v3::kLdsBytes, s, pl, digits, cbuf_in, W);
  return hipGetLastError();
}
template <class Form>
static hipError_t cols_back(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s) {
  hipLaunchKernelGGL((v3::k3_cols256<Form, false>), dim3(pl.M2 / 4), dim3(Form::kBlock), v3::kLdsBytes, s, pl, W, digits, cbuf, a, BackExt());
  return hipGetLastError();
}
template <class Form>
static hipError_t cols_back_ext(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& x, hipStream_t s) {
  hipLaunchKernelGGL((v3::k3_cols256<Form, true>), dim3(pl.M2 / 4), dim3(Form::kBlock), v3::kLdsBytes, s, pl, W, digits, cbuf, a, x);
  return hipGetLastError();
}
static hipError_t cols_fourstep(const DevPlan& pl, uint64_t* f0f, uint64_t* f0i, uint64_t* fbf, uint64_t* fbi, hipStream_t s) {
  hipLaunchKernelGGL(v3::k_build_f0, dim3(pl.M2 / 4), dim3(v3::kThreads), 0, s, pl, f0f, f0i, fbf, fbi);
  return hipGetLastError();
}
template <class Form>
static ColSweeps cols() { return ColSweeps{cols_front<Form>, cols_back<Form>, cols_back_ext<Form>, cols_fourstep}; }
ColSweeps v3_cols(bool planes) { return planes ? cols<v3::Planes>() : cols<v3::Pairs>(); }

}  // namespace mi355
