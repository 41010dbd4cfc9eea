// gfx950 kernels, register-resident radix-8 set ("v2") for the large power-of-two shapes.
//
// Same three sweeps as kernels.hip, but each work-group of 512 threads keeps its 4096-pair tile in
// registers (8 pairs per thread) and uses LDS only to exchange between radix-8 stages, and the stages
// are grouped into multiplication-free 64-point blocks:
//   * inside a block every root of unity is a power of two (omega_64 = 2^39): butterflies are add/sub
//     plus constant shifts (gfdft.hpp), the twiddle between the two radix-8 halves of a block is a
//     shift whose amount is uniform per wavefront (the thread->element maps below put the digit that
//     selects it in the wave index): the seam is compiled once per wave index with constant shifts and
//     selected by one scalar switch;
//   * only the seam between two blocks is a general GF(P) multiplication (one per element and
//     direction, from a universal omega_M table), against three per radix-4 level pair in the
//     reference's schedule (marin.cl:304-318: fwd4/bck4 with r1, r23.s0, r23.s1).
// Shapes served: rows M2 = 4096 (8.8.8.8), 8192 (2 x 4096 under one radix-2 level) and 2048 (4.8.8.8: two rows to a tile, or one row with
// one plane per thread -- the Planes form below); columns M1 = 512 R (R.8.8.8, R = 1, 2, 4) with C = 8/R pairs per run.  The small
// transforms run on the radix-4 set (kernels_v3.hip), columns of 1280 on kernels_v5.hip, everything else on the generic set.
// Row order of the work buffer and digit layout are those of kernels.hip, so the two sets interoperate
// kernel by kernel (the multiplicand image layout differs: an engine uses one middle kernel for both
// set_multiplicand and mul).
// Value ranges: field values are canonical ([0, P)) except that (a) a negated zero may be P (gf.hpp,
// mul_pow2) and (b) sums marked LAZY (gfdft.hpp) may be any 64-bit representative; (b) only ever feeds a
// multiplication, a shift or the minuend / lazy-sum slot that gfdft.hpp names, and every kernel's last arithmetic step before a store is a
// multiplication or a canonical add/sub -- except the row kernel's last inverse stage, whose un-folded outputs the back sweep multiplies first --
// so nothing non-canonical other than P reaches a canonical-only operand or a digit.
//
// LDS exchanges (P2 = 16 B slots, slot map phys() of kernels_v2_common.hpp against bank conflicts):
//   writer "thread-major": slot t*8 + r          reader: slot j*512 + t'
//   writer "wave-major":   slot w*512 + r*64 + f(lane)   reader: slot j*512 + t'
// which is the digit permutation that hands each thread the 8 elements of its next radix-8.
#include "kernels_v2_common.hpp"

namespace mi355 {
namespace v2 {
// ---------------------------------------------------------------------------------------------
// middle, M2 = 4096 = 8.8.8.8.  Element index e = 512 d1 + 64 d2 + 8 d3 + d4.
//   S1 thread (d2|d3|d4) regs d1 -> k1 ; shift omega_64^(k1 d2)         [d2 = wave]
//   S2 thread (d3|d4|k1) regs d2 -> k2 ; general omega_4096^((k1+8k2)(8d3+d4))
//   S3 thread (d4|k1|k2) regs d3 -> k3 ; shift omega_64^(k3 d4)         [d4 = wave]
//   S4 thread (k3|k1|k2) regs d4 -> k4 ; X[k], k = k1 + 8 k2 + 64 k3 + 512 k4
// pointwise in registers, then the mirror image back to natural order.
// mode 0: square, 1: multiply by image Y, 2: forward only (writes the image), 3: multiply by the word-wise sum of the images Y and Y2
// (mode 1 with y = Y[i] + Y2[i]: both are un-folded mode-2 outputs, gf::add_lazy_any), 4: mode 0 that first stores what mode 2 would
// store to Wimg (the image of the operand, straight from the registers the pointwise stage reads next).
// ---------------------------------------------------------------------------------------------
// H = 2 serves rows of 8192 with 1024 threads: one radix-2 level on top (element i and i + 4096; thread group
// h = 0 forms the sums, h = 1 the differences times omega_8192^i, each group loads both halves), then each
// group runs the 4096-point machinery on its own LDS half (2 x 72 KiB); output index k of group h is row
// frequency 2k + h.  The inverse ends with the mirror butterfly through LDS.
// RL = 1 serves rows of 2048 (round 3; the reference's sqr512 / forward1024 shapes, kernels/marin.cl:1190,1517): a tile is two adjacent rows,
// the first-stage registers 4 r .. 4 r + 3 belong to row r of the tile, the first stage is a radix-4 per row (32-point blocks: seam
// omega_32^(k1' d2), still uniform per wave), the table seam reads omega_2048^((k1' + 4 k2)(8 d3 + d4)) (plan.hpp builds S2r for this shape)
// and everything after it is the 4096-point code with the row carried in the top bit of the k1 field: X[k], k = k1' + 4 k2 + 32 k3 + 256 k4
// of row 2 tile + (k1 >> 2).  n = 2^21: 0.0645 -> 0.0577 ms, n = 5 2^20 (p ~ 100 M): 0.130 -> 0.120 ms (same-box A/B against the generic rows,
// profiles/r03_summary.md).  (Four rows of 1024 to a tile -- RL = 2, a radix-2 first stage -- were built and measured too: n = 5 2^19 has only
// 320 such tiles for 256 CUs and lost 2.4 % against the generic rows; not kept.)
//
// Lane forms.  Pairs: a pair per thread, all of the above.  Planes (round 4): rows of 2048, one row to a tile, ONE PLANE PER THREAD.  The two
// planes of a pair go through the same GF(P)-linear transform and meet only in the pointwise step, so the "two rows to a tile" code runs
// unchanged on 64-bit words with the row bit read as the plane bit: a tile is one row of 2048 pairs = 4096 words, 512 threads x 8 words, the
// first-stage registers 4 pl .. 4 pl + 3 are plane pl of the four pairs a thread loads (16-byte loads and stores as before), after the last
// forward exchange plane = lane >> 5, and the pointwise step trades words with lane ^ 32 (ds_bpermute: crossbar only, no LDS memory).  Half
// the registers and half the serial work per thread of the pair form, twice the tiles: where two rows to a tile leave CUs without a tile
// (n = 2^20: 128 tiles) or with one group of eight waves (n = 2^21) this fills the chip.  LDS: 32 KiB of 8-byte slots, map i ^ ((i >> 3) & 31)
// (conflict-free for the 16-lane / 32-lane groups 64-bit accesses are served in: thread-major, strided and wave-major orders alike).
// Its multiplicand image (mode 2 -> mode 1) is word 512 k4 + t of the row, i.e. plane-major inside 64-word runs -- private to this form.
// The kernel below is written once on the form; only the tile load, the pointwise step and the tile store are overloads on its element.
__device__ __forceinline__ uint32_t phys8(uint32_t i) { return i ^ ((i >> 3) & 31u); }
struct Pairs {
  using E = P2;
  static constexpr uint32_t kLds = kLdsBytes, kTilePairs = 4096;   // LDS bytes and pairs of a 512-thread tile
  static __device__ __forceinline__ uint32_t map(uint32_t i) { return phys(i); }
};
struct Planes {
  using E = uint64_t;
  static constexpr uint32_t kLds = 4096 * 8, kTilePairs = 2048;
  static __device__ __forceinline__ uint32_t map(uint32_t i) { return phys8(i); }
};

// the radix-4 first stage of rows of 2048 on registers 0 .. 3 and 4 .. 7: the two rows of a tile (both planes), or the two planes of a row
template <bool INV>
__device__ __forceinline__ void dft4x2(P2 (&x)[8]) {
  dft4<INV>(x[0].a, x[1].a, x[2].a, x[3].a); dft4<INV>(x[0].b, x[1].b, x[2].b, x[3].b);
  dft4<INV>(x[4].a, x[5].a, x[6].a, x[7].a); dft4<INV>(x[4].b, x[5].b, x[6].b, x[7].b);
}
template <bool INV>
__device__ __forceinline__ void dft4x2(uint64_t (&x)[8]) { dft4<INV>(x[0], x[1], x[2], x[3]); dft4<INV>(x[4], x[5], x[6], x[7]); }

// ---- tile load: in = the work-group's first pair; H = 2: with the radix-2 level on top ----
template <int H>
__device__ __forceinline__ void load_tile(P2 (&x)[8], const DevPlan& pl, const P2* in, uint32_t t, uint32_t h) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (H == 1) x[j] = w_load(&in[512 * j + t]);
    else {
      const P2 lo = in[512 * j + t], hi = in[4096 + 512 * j + t];
      if (h == 0) x[j] = {gf::add(lo.a, hi.a), gf::add(lo.b, hi.b)};
      else x[j] = p2_mul(P2{gf::sub(lo.a, hi.a), gf::sub(lo.b, hi.b)}, pl.UT2[512 * j + t]);
    }
  }
}
template <int H>
__device__ __forceinline__ void load_tile(uint64_t (&x)[8], const DevPlan&, const P2* in, uint32_t t, uint32_t) {
#pragma unroll
  for (int d = 0; d < 4; ++d) { const P2 v = in[512 * d + t]; x[d] = v.a; x[4 + d] = v.b; }
}

// ---- pointwise: reg k4 holds X[kb + 512 k4] (rows of 2048: kb + 256 k4); rho = omega_m^(k1row + M1 k) = rho0 * omega_8^k4,
// omega_8^k4 = 2^(120 k4): +1, -2^24, +2^48, -2^72, -1, +2^24, -2^48, +2^72.  Y, Y2: the images of the work-group half's tile ----
__device__ __forceinline__ unsigned rho_shift(int k4) { return 24u * (k4 & 3); }
__device__ __forceinline__ bool rho_neg(int k4) { return (k4 == 1) || (k4 == 3) || (k4 == 4) || (k4 == 6); }
template <int mode>
__device__ __forceinline__ void pointwise(P2 (&x)[8], uint64_t rho0, const uint64_t* __restrict__ Yimg, const uint64_t* __restrict__ Yimg2, uint32_t t) {
  const P2* Y = reinterpret_cast<const P2*>(Yimg);
#pragma unroll
  for (int k4 = 0; k4 < 8; ++k4) {
    const unsigned sh = rho_shift(k4);
    const bool neg = rho_neg(k4);
    const P2 u = x[k4];
    P2 r;
    if (mode == 0) {   // (u0 + u1 t)^2 mod (t^2 - rho), marin.cl:379-384
      const uint64_t q = gf::mul_pow2(gf::mul(gf::sqr(u.b), rho0), sh);
      const uint64_t s0 = gf::sqr(u.a);
      r.a = neg ? gf::sub(s0, q) : gf::add(s0, q);
      r.b = gf::dbl(gf::mul(u.b, u.a));   // (u.a may be an un-folded sum: double the product, not the operand)
    } else {           // marin.cl:387-392
      P2 y = Y[512 * k4 + t];
      if (mode == 3) {
        const P2 z = reinterpret_cast<const P2*>(Yimg2)[512 * k4 + t];
        y = {gf::add_lazy_any(y.a, z.a), gf::add_lazy_any(y.b, z.b)};
      }
      const uint64_t q = gf::mul_pow2(gf::mul(gf::mul(u.b, y.b), rho0), sh);
      const uint64_t s0 = gf::mul(u.a, y.a);
      r.a = neg ? gf::sub(s0, q) : gf::add(s0, q);
      r.b = gf::add(gf::mul(u.a, y.b), gf::mul(u.b, y.a));
    }
    x[k4] = r;
  }
}
__device__ __forceinline__ uint64_t swap32(uint64_t v, uint32_t partner_byte) {   // the word lane ^ 32 holds
  const uint32_t lo = uint32_t(__builtin_amdgcn_ds_bpermute(int(partner_byte), int(uint32_t(v))));
  const uint32_t hi = uint32_t(__builtin_amdgcn_ds_bpermute(int(partner_byte), int(uint32_t(v >> 32))));
  return (uint64_t(hi) << 32) | lo;
}
// thread (k3|pl|k1'|k2) holds plane pl = lane >> 5 of the pair; plane a computes and keeps the t^0 word
template <int mode>
__device__ __forceinline__ void pointwise(uint64_t (&x)[8], uint64_t rho0, const uint64_t* __restrict__ Y, const uint64_t* __restrict__ Z, uint32_t t) {
  const uint32_t lane = t & 63, pln = lane >> 5, partner = ((lane ^ 32u) << 2);
#pragma unroll
  for (int k4 = 0; k4 < 8; ++k4) {
    const unsigned sh = rho_shift(k4);
    const bool neg = rho_neg(k4);
    const uint64_t w = x[k4];
    uint64_t keep, send;
    if (mode == 0) {
      const uint64_t o = swap32(w, partner);
      keep = gf::sqr(w);                                            // a^2 | b^2
      send = gf::mul(pln ? keep : w, pln ? rho0 : o);               // a b | b^2 rho0
      if (pln) send = gf::mul_pow2(send, sh);
    } else {
      uint64_t y = Y[512 * k4 + t], yo = Y[512 * k4 + (t ^ 32u)];
      if (mode == 3) { y = gf::add_lazy_any(y, Z[512 * k4 + t]); yo = gf::add_lazy_any(yo, Z[512 * k4 + (t ^ 32u)]); }
      keep = gf::mul(w, y);                                         // a ya | b yb
      send = gf::mul(w, yo);                                        // a yb | b ya
      if (pln) { const uint64_t q = gf::mul_pow2(gf::mul(keep, rho0), sh); keep = send; send = q; }   // plane b keeps b ya, sends b yb rho
    }
    const uint64_t recv = swap32(send, partner);
    if (mode == 0) x[k4] = pln ? gf::dbl(recv) : (neg ? gf::sub(keep, recv) : gf::add(keep, recv));
    else x[k4] = pln ? gf::add(keep, recv) : (neg ? gf::sub(keep, recv) : gf::add(keep, recv));
  }
}

// ---- tile store: out = first pair of the work-group half's tile; H = 2: after the mirror of the top radix-2 level through LDS,
// lo = A + B w^-i, hi = A - B w^-i (A from group 0, B from group 1) ----
template <int H>
__device__ __forceinline__ void store_tile(P2 (&x)[8], const DevPlan& pl, P2* out, P2* X, uint32_t t, uint32_t h) {
  if (H == 2) {
    if (h == 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const uint32_t i = 512 * j + t; x[j] = p2_mul(x[j], pl.UT2[i ? 8192 - i : 0]); }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) X[phys(j * 512 + t)] = x[j];
    __syncthreads();
    const P2* Xo = reinterpret_cast<const P2*>(smem_v2) + (1 - h) * kLdsSlots;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const P2 o = Xo[phys(j * 512 + t)];
      x[j] = (h == 0) ? P2{gf::add(x[j].a, o.a), gf::add(x[j].b, o.b)} : P2{gf::sub(o.a, x[j].a), gf::sub(o.b, x[j].b)};
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) w_store(&out[512 * j + t], x[j]);
}
template <int H>
__device__ __forceinline__ void store_tile(uint64_t (&x)[8], const DevPlan&, P2* out, uint64_t*, uint32_t t, uint32_t) {
#pragma unroll
  for (int d = 0; d < 4; ++d) out[512 * d + t] = P2{x[d], x[4 + d]};
}

// seam twiddles of a thread: [b][k1][k2], 64 contiguous bytes
__device__ __forceinline__ void load_seam_words(const uint64_t* __restrict__ S, uint32_t t, uint64_t (&sw)[8]) {
  const uint32_t k1 = t & 7, b = t >> 3;
  const uint64_t* __restrict__ tw = S + b * 64 + k1 * 8;
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) sw[k2] = tw[k2];
}

template <class Form, int mode, int H, int RL>
__global__ void __launch_bounds__(512 * H, 4) k2_rows(DevPlan pl, const uint64_t* __restrict__ Win, const uint64_t* __restrict__ Yimg,
                                                      const uint64_t* __restrict__ Yimg2, uint64_t* __restrict__ Wimg, uint64_t* __restrict__ Wout) {
  using E = typename Form::E;
  constexpr bool PLANES = (sizeof(E) == 8);
  static_assert(RL == 0 || (RL == 1 && H == 1), "two rows to a tile only with one tile per work-group");
  static_assert(!PLANES || (H == 1 && RL == 1), "the plane form exists for one row of 2048 only (the row bit of RL = 1 is its plane bit)");
  constexpr int R1 = 8 >> RL;           // first-stage radix
  const uint32_t h = (H == 2) ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 9) : 0u;
  if (H == 1 && !PLANES) boost_if_late(pl.boost_rows);
  E* X = reinterpret_cast<E*>(smem_v2) + h * kLdsSlots;
  const uint32_t t = threadIdx.x & 511, lane = t & 63, wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 7);
  const uint32_t tile = PROBE_BLOCK(pl);
  const uint32_t row = (RL && !PLANES) ? (tile << RL) + (lane >> (6 - RL)) : tile;    // several rows: the row this thread's S4 outputs (and pointwise words) belong to
  PROBE_BEGIN(pl)
  const size_t tile0 = size_t(tile) * (Form::kTilePairs * H), half0 = tile0 + h * 4096;   // first pair of the work-group's tile(s), of this half's
  E x[8];
  // table words of the pointwise stage, requested first: their latency hides behind the forward transform
  // S4 thread (k3|k1|k2): frequency base k1 + 8 k2 + 64 k3 (rows of 2048: k1' + R1 k2 + 8 R1 k3 with k1' = k1 & (R1 - 1))
  const uint32_t kb = ((lane >> 3) & uint32_t(R1 - 1)) + R1 * (lane & 7) + 8 * R1 * wave;
  const uint32_t blk = row / pl.L1, qq = row - blk * pl.L1;       // column-DFT slot -> frequency (kernels.hip freq1)
  const uint32_t k1row = col_label(pl, blk, pl.logL1 ? (__brev(qq) >> (32 - pl.logL1)) : 0u);
  const uint64_t erho = rho_exponent(pl, k1row, H * kb + h);   // row frequency of X[kb]: H kb + h
  const uint64_t rho_lo = pl.TWlo[erho & ((1u << pl.twh) - 1)], rho_hi = pl.TWhi[erho >> pl.twh];

  // ---- forward ----
  load_tile<H>(x, pl, reinterpret_cast<const P2*>(Win) + tile0, t, h);
  if constexpr (RL) { dft4x2<false>(x); seam<5, false>(x, wave); }
  else {
    dft8p<false, 1>(x);   // outputs 1..7 are shifted next, output 0 is not
    seam<6, false, true>(x, wave);
  }
  uint64_t sw[8];   // seam twiddles: loaded before the exchange so that their latency hides behind it
  load_seam_words(pl.S2r, t, sw);
  exch_thread_major<Form::map, true>(X, x, t);
  dft8p<false, 2>(x);   // all outputs are multiplied next
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) x[k2] = mulw(x[k2], sw[k2]);
  exch_thread_major<Form::map, true>(X, x, t);
  dft8p<false, 1>(x);
  seam<6, false, true>(x, wave);
  exch_wave_major<Form::map, true>(X, x, t, wave, lane);
  dft8p<false, 2>(x);   // mode 2 stores them for a later multiplication (un-folded sums), the pointwise stage multiplies

  if (mode == 2 || mode == 4) {   // the image: register j of thread t at element 512 j + t of the tile, in the form's element
    E* img = reinterpret_cast<E*>((mode == 2 ? Wout : Wimg) + 2 * half0);
#pragma unroll
    for (int j = 0; j < 8; ++j) img[512 * j + t] = x[j];
    if (mode == 2) return;
  }

  PROBE_MID(pl)
  pointwise<(mode == 4 ? 0 : mode)>(x, gf::mul(rho_lo, rho_hi), Yimg + 2 * half0, Yimg2 + 2 * half0, t);

  // ---- inverse (mirror) ----
  dft8p<true>(x);
  exch_wave_major<Form::map, false>(X, x, t, wave, lane);
  seam<6, true>(x, wave);
  dft8p<true, 2>(x);   // exchanged, then multiplied by the seam twiddles
  load_seam_words(pl.S2ri, t, sw);
  exch_thread_major<Form::map, false>(X, x, t);
  if (H == 1 && !PLANES) __builtin_amdgcn_s_setprio(0);   // boosted groups: back to normal for the last stages (measured best drop point)
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) x[k2] = mulw(x[k2], sw[k2]);
  dft8p<true>(x);
  exch_thread_major<Form::map, false>(X, x, t);
  if constexpr (RL) { seam<5, true>(x, wave); dft4x2<true>(x); }
  else {
    seam<6, true>(x, wave);
    if (H == 1) dft8p<true, 2>(x);   // stored for a back sweep, which multiplies by its twiddle first
    else dft8p<true>(x);
  }
  store_tile<H>(x, pl, reinterpret_cast<P2*>(Wout) + half0, X, t, h);
  PROBE_END(pl)
}

// ---------------------------------------------------------------------------------------------
// Column tiles, M1 = 512 R = R.8.8.8 with R in {1, 2, 4} and C = 8 / R pairs per run (tile = 4096 pairs).
// Tile element (i1, c), i1 = 512 d1 + 64 d2 + 8 d3 + d4 (d1 < R).  kc = k1 C + c is a 3-bit register /
// thread field throughout.
// front_tile (digits -> work buffer):
//   S1 thread (d2|d3|d4) regs (d1,c): R whole runs of 2C digits -> weight -> DFT_R -> k1 ; shift omega_8R^(k1 d2)
//   S2 thread (d3|d4|k1|c) regs d2 -> k2 ; general omega_M1^((k1 + R k2)(8d3+d4))
//   S3 thread (d4|k1|c|k2) regs d3 -> k3 ; shift omega_64^(k3 d4)
//   S4 thread (k3|k1|k2|c) regs d4 -> k4 ; k1col = k1 + R k2 + 8R k3 + 64R k4
//   then the four-step twiddle omega_m^(i2 k1col) * TB (geometric in k4: one chain multiply per pair)
//   and the store to work-buffer row bitrev(k1col), column i2 = C T + c.
// back_tile is the mirror image, followed by unweight and the sequential carry of the thread's R runs.
// ---------------------------------------------------------------------------------------------

template <int R> struct ColShape {
  static constexpr int C = 8 / R;                      // pairs per run
  static constexpr int LC = (C == 8) ? 3 : (C == 4) ? 2 : 1;
  static constexpr int LR = 3 - LC;
  static constexpr int M1 = 512 * R, LM = 9 + LR, ND = 2 * C;   // digits per run
  // wave-major exchanges of the column sweeps: lane = (k1 C + c) 8 + k2  ->  slot offset (k1 | k2 | c)
  static __device__ __forceinline__ uint32_t lane_offset(uint32_t lane) { return ((lane >> (3 + LC)) << (3 + LC)) | ((lane & 7) << LC) | ((lane >> 3) & (C - 1)); }
};

// S1 of the front: DFT_R over d1 (register slots d1 C + c -> k1 C + c), then x[k1 C + c] *= omega_8R^(k1 W)
template <int R, int W>
__device__ __forceinline__ void stage_r_fwd_const(P2 (&x)[8]) {
  constexpr int C = 8 / R;
  if (R == 2) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const P2 u = x[c], v = x[C + c];
      x[c] = {gf::add(u.a, v.a), gf::add(u.b, v.b)};
      x[C + c] = {gf::sub(u.a, v.a), gf::sub(u.b, v.b)};
    }
  } else if (R == 4) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      dft4<false>(x[c].a, x[C + c].a, x[2 * C + c].a, x[3 * C + c].a);
      dft4<false>(x[c].b, x[C + c].b, x[2 * C + c].b, x[3 * C + c].b);
    }
  }
#pragma unroll
  for (int k1 = 1; k1 < R; ++k1) {
    const unsigned s = ((8u / unsigned(R)) * gf::LOG2_W64 * unsigned(k1) * unsigned(W)) % 192u;   // omega_8R = omega_64^(8/R)
#pragma unroll
    for (int c = 0; c < C; ++c) x[k1 * C + c] = {gf::mul_pow2(x[k1 * C + c].a, s), gf::mul_pow2(x[k1 * C + c].b, s)};
  }
}
// last stage of the back: the inverse seam, then the inverse DFT_R.  For R = 2 a negative sign (shift >= 96)
// is absorbed by swapping the sum and the difference.
template <int R, int W>
__device__ __forceinline__ void stage_r_inv_const(P2 (&x)[8]) {
  constexpr int C = 8 / R;
  if (R == 2) {
    const unsigned f = (192u - (4u * gf::LOG2_W64 * unsigned(W)) % 192u) % 192u;
    const bool neg = f >= 96u;
    const unsigned s = neg ? f - 96u : f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const P2 u = x[c];
      const P2 v = {gf::mul_pow2(x[C + c].a, s), gf::mul_pow2(x[C + c].b, s)};
      const P2 sum = {gf::add(u.a, v.a), gf::add(u.b, v.b)}, dif = {gf::sub(u.a, v.a), gf::sub(u.b, v.b)};
      x[c] = neg ? dif : sum;
      x[C + c] = neg ? sum : dif;
    }
  } else if (R == 4) {
#pragma unroll
    for (int k1 = 1; k1 < R; ++k1) {
      const unsigned s = (192u - ((8u / unsigned(R)) * gf::LOG2_W64 * unsigned(k1) * unsigned(W)) % 192u) % 192u;
#pragma unroll
      for (int c = 0; c < C; ++c) x[k1 * C + c] = {gf::mul_pow2(x[k1 * C + c].a, s), gf::mul_pow2(x[k1 * C + c].b, s)};
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      dft4<true>(x[c].a, x[C + c].a, x[2 * C + c].a, x[3 * C + c].a);
      dft4<true>(x[c].b, x[C + c].b, x[2 * C + c].b, x[3 * C + c].b);
    }
  }
}

// digits of the thread's R runs (i1 = 512 d1 + t) of tile T  ->  work buffer (forward columns).
template <int R>
__device__ __forceinline__ void front_tile(const DevPlan& pl, P2* X, uint32_t T, uint32_t t, uint32_t lane, uint32_t wave,
                                           const uint32_t (&dg)[R][16 / R], uint32_t di, uint64_t* __restrict__ Wout) {
  using S = ColShape<R>;
  constexpr int C = S::C, LC = S::LC;
  P2 x[8];
#pragma unroll
  for (int d1 = 0; d1 < R; ++d1) weigh_run<S::ND>(pl.TAh[512 * d1 + t], pl.TAh[S::M1 + 512 * d1 + t], ~di, d1, dg[d1], &x[C * d1]);
#define MI355_CALL(W) stage_r_fwd_const<R, W>(x)
  MI355_SWITCH8(wave, MI355_CALL)
#undef MI355_CALL
  uint64_t sw[8];   // seam twiddles, requested before the exchange that hides their latency
  {
    const uint32_t k1 = (t & 7) >> LC, b = t >> 3;
    const uint64_t* __restrict__ tw = pl.S1r + b * (8 * R) + k1 * 8;   // [b][k1][k2]
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) sw[k2] = tw[k2];
  }
  exch_thread_major<phys, true>(X, x, t);
  dft8p<false, 2>(x);
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) x[k2] = p2_mul(x[k2], sw[k2]);
  // four-step twiddle ingredients for the last stage (thread (k3|k1|k2|c)), requested two exchanges early
  const uint32_t fc = t & (C - 1), fkb = ((t >> (3 + LC)) & (R - 1)) + R * ((t >> LC) & 7) + 8 * R * (t >> 6), fi2 = C * T + fc;
  // chain start omega_m^(i2 kb) TB[2 i2] and ratio omega_m^(64R i2), ready-made per (tile, thread) / per column
  const uint64_t fca0 = pl.F0f[size_t(T) * 512 + t], fB = pl.FBf[fi2];
  exch_thread_major<phys, true>(X, x, t);
  dft8p<false, 1>(x);
  seam<6, false, true>(x, wave);
  exch_wave_major<phys, true>(X, x, t, wave, S::lane_offset(lane));
  dft8p<false, 2>(x);   // four-step twiddle next
  {
    const uint32_t kb = fkb, i2 = fi2;
    const uint64_t B = fB;
    uint64_t ca = fca0;   // one chain for both digits of a pair (plan.hpp: SA/TA second half)
    const uint32_t row0 = __brev(kb) >> (32 - S::LM);   // bitrev(kb): its low 3 bits are zero
    P2* W = reinterpret_cast<P2*>(Wout);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t rj = ((j & 1) << 2) | (j & 2) | (j >> 2);   // bitrev3(j)
      w_store(&W[size_t(row0 + rj) * pl.M2 + i2], P2{gf::mul(x[j].a, ca), gf::mul(x[j].b, ca)});
      if (j < 7) ca = gf::mul(ca, B);
    }
  }
}

// work buffer -> digits of the thread's R runs of tile T (inverse columns, unweight, x a, carry).
// cout[d1]: carry leaving run d1 (every run starts from zero; the next sweep folds the carry words in).
// ADD: ad[d1][k] (the digits of another residue's runs, pending carries already folded in) join the carry chain (mul_add)
template <int R, bool ADD>
__device__ __forceinline__ void back_tile(const DevPlan& pl, P2* X, uint32_t T, uint32_t t, uint32_t lane, uint32_t wave,
                                          const uint64_t* __restrict__ Win, uint32_t a, uint32_t di, uint32_t (&dg)[R][16 / R], uint64_t (&cout)[R],
                                          const uint32_t (*ad)[16 / R]) {
  using S = ColShape<R>;
  constexpr int C = S::C, LC = S::LC;
  P2 x[8];
  {
    const uint32_t c = t & (C - 1), k2 = (t >> LC) & 7, k1 = (t >> (3 + LC)) & (R - 1), k3 = t >> 6;
    const uint32_t kb = k1 + R * k2 + 8 * R * k3;
    const uint32_t i2 = C * T + c;
    // chain start omega_m^-(i2 kb) TBi[2 i2] and ratio omega_m^-(64R i2), ready-made (k_build_f0)
    uint64_t ca = pl.F0i[size_t(T) * 512 + t];   // one chain for both digits of a pair (plan.hpp: SA/TA second half)
    const uint64_t B = pl.FBi[i2];
    const uint32_t row0 = __brev(kb) >> (32 - S::LM);
    const P2* W = reinterpret_cast<const P2*>(Win);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t rj = ((j & 1) << 2) | (j & 2) | (j >> 2);
      x[j] = w_load(&W[size_t(row0 + rj) * pl.M2 + i2]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = {gf::mul(x[j].a, ca), gf::mul(x[j].b, ca)};
      if (j < 7) ca = gf::mul(ca, B);
    }
  }
  dft8p<true>(x);
  exch_wave_major<phys, false>(X, x, t, wave, S::lane_offset(lane));
  seam<6, true>(x, wave);
  dft8p<true, 2>(x);
  uint64_t sw[8];
  {
    const uint32_t k1 = (t & 7) >> LC, b = t >> 3;
    const uint64_t* __restrict__ tw = pl.S1ri + b * (8 * R) + k1 * 8;   // [b][k1][k2]
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) sw[k2] = tw[k2];
  }
  exch_thread_major<phys, false>(X, x, t);
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) x[k2] = p2_mul(x[k2], sw[k2]);
  dft8p<true>(x);
  // unweighting tables of the carry phase (thread (d2|d3|d4): runs i1 = 512 d1 + t), requested one exchange early;
  // odd digits take theirs from the second half of SA / TAi
  // (the doubled entries too, from their own table -- except with four runs a thread, where 16 more registers across the exchange would spill)
  constexpr bool PRE2 = (R <= 2);
  uint64_t btai_e[R], btai_o[R], btai2_e[R], btai2_o[R];
#pragma unroll
  for (int d1 = 0; d1 < R; ++d1) {
    btai_e[d1] = pl.TAi[512 * d1 + t]; btai_o[d1] = pl.TAi[S::M1 + 512 * d1 + t];
    if (PRE2) { btai2_e[d1] = pl.TAi2[512 * d1 + t]; btai2_o[d1] = pl.TAi2[S::M1 + 512 * d1 + t]; }
  }
  exch_thread_major<phys, false>(X, x, t);
#define MI355_CALL(W) stage_r_inv_const<R, W>(x)
  MI355_SWITCH8(wave, MI355_CALL)
#undef MI355_CALL
#pragma unroll
  for (int d1 = 0; d1 < R; ++d1)   // wrapped exponents: weight was halved
    cout[d1] = unweigh_carry<S::ND, ADD>(pl, di, d1, &x[C * d1], btai_e[d1], btai_o[d1], PRE2 ? btai2_e[d1] : gf::dbl(btai_e[d1]),
                                         PRE2 ? btai2_o[d1] : gf::dbl(btai_o[d1]), a, ADD ? ad[d1] : nullptr, dg[d1]);
}

// front sweep: digits (+ deferred run carries cbuf_in, nullable) -> work buffer
template <int R>
__global__ void __launch_bounds__(512, 4) k1_cols(DevPlan pl, const uint32_t* __restrict__ digits, const uint64_t* __restrict__ cbuf_in,
                                                  uint64_t* __restrict__ Wout) {
  P2* X = reinterpret_cast<P2*>(smem_v2);
  const uint32_t t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // tile order: with two pairs per run (R = 4) four tiles share each 128-byte line of the work buffer, and keeping
  // them on one XCD lets its L2 merge the 32-byte pieces (n = 2^24: front sweep 97 -> 89 us); with runs of eight pairs (R = 1) the
  // XCD-contiguous order wins too (n = 2^22: 20.3 -> 19.0 us), with four (R = 2) the plain order does (C3: 34.5 vs 35.4 us; round 3,
  // same-box A/B with MI355_TUNE bit 5, which forces the XCD-contiguous order; profiles/r03_microbench_pitch.txt has the bare patterns)
  const uint32_t T = (R != 2 || (pl.tune & 32)) ? tile_of_block(pl, PROBE_BLOCK(pl), PROBE_GRID(pl)) : PROBE_BLOCK(pl);
  boost_if_late(pl.boost_tiles);
  PROBE_BEGIN(pl)
  uint32_t dg[R][16 / R];
  const uint32_t di = pl.DI[size_t(T) * 512 + t];
#pragma unroll
  for (int d1 = 0; d1 < R; ++d1) {
    const uint32_t i1 = 512 * d1 + t;
    load_run(digits, size_t(T) * (512 * R) + i1, dg[d1]);
    if (cbuf_in) apply_carry_in<16 / R>(pl, di, d1, carry_in_of(pl, cbuf_in, T, i1), dg[d1]);
  }
  front_tile<R>(pl, X, T, t, lane, wave, dg, di, Wout);
  PROBE_END(pl)
}

// back sweep: work buffer -> digits + one carry word per run.  EXT: with extras (kernels.hpp BackExt), a second destination register
// and / or an addend in the carry chain
template <int R, bool EXT>
__global__ void __launch_bounds__(512, 4) k3_cols(DevPlan pl, const uint64_t* __restrict__ Win, uint32_t* __restrict__ digits,
                                                  uint64_t* __restrict__ cbuf, uint32_t a, BackExt ext) {
  P2* X = reinterpret_cast<P2*>(smem_v2);
  const uint32_t t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), T = tile_of_block(pl, PROBE_BLOCK(pl), PROBE_GRID(pl));
  boost_if_late(pl.boost_tiles);
  PROBE_BEGIN(pl)
  uint32_t dg[R][16 / R], ad[R][16 / R];
  uint64_t cout[R];
  const uint32_t di = pl.DI[size_t(T) * 512 + t];
  if (EXT) {
#pragma unroll
    for (int d1 = 0; d1 < R; ++d1) {
#pragma unroll
      for (int k = 0; k < 16 / R; ++k) ad[d1][k] = 0;
      if (ext.add_digits) {
        const uint32_t i1 = 512 * d1 + t;
        load_run(ext.add_digits, size_t(T) * (512 * R) + i1, ad[d1]);
        if (ext.add_cbuf) apply_carry_in<16 / R>(pl, di, d1, carry_in_of(pl, ext.add_cbuf, T, i1), ad[d1]);
      }
    }
  }
  back_tile<R, EXT>(pl, X, T, t, lane, wave, Win, a, di, dg, cout, ad);
#pragma unroll
  for (int d1 = 0; d1 < R; ++d1) {
    const size_t run = size_t(T) * (512 * R) + 512 * d1 + t;
    store_run(digits, run, dg[d1]);
    cbuf[run] = cout[d1];
    if (EXT && ext.digits2) { store_run(ext.digits2, run, dg[d1]); ext.cbuf2[run] = cout[d1]; }
  }
  PROBE_END(pl)
}

}  // namespace v2

namespace v2 {
// chain starts and ratios of the four-step twiddle chains of the column kernels (same thread map as the last
// stage of front_tile / first stage of back_tile): F0f[T][t] = omega_m^(i2 kb) TB[2 i2], F0i the inverse with
// TBi, FBf[i2] = omega_m^(64R i2), FBi its inverse.
template <int R>
__global__ void __launch_bounds__(512) k_build_f0(DevPlan pl, uint64_t* __restrict__ f0f, uint64_t* __restrict__ f0i,
                                                  uint64_t* __restrict__ fbf, uint64_t* __restrict__ fbi) {
  using S = ColShape<R>;
  constexpr int C = S::C, LC = S::LC;
  const uint32_t t = threadIdx.x, T = blockIdx.x;
  const uint32_t c = t & (C - 1), kb = ((t >> (3 + LC)) & (R - 1)) + R * ((t >> LC) & 7) + 8 * R * (t >> 6), i2 = C * T + c;
  const uint32_t ea = i2 * kb;
  f0f[size_t(T) * 512 + t] = gf::mul(tw_lookup(pl, ea), pl.TB[2 * i2]);
  f0i[size_t(T) * 512 + t] = gf::mul(tw_lookup(pl, ea ? pl.m - ea : 0), pl.TBi[2 * i2]);
  if (t < C) {
    const uint32_t eb = i2 * (64 * R);
    fbf[i2] = tw_lookup(pl, eb);
    fbi[i2] = tw_lookup(pl, eb ? pl.m - eb : 0);
  }
}
}  // namespace v2

// ------------------------------- launchers ---------------------------------------------------

// columns of 512 R: one 4096-pair tile per work-group of 512 threads
template <int R>
static hipError_t cols_front(const DevPlan& pl, const uint32_t* digits, const uint64_t* cbuf_in, uint64_t* W, hipStream_t s) {
  hipLaunchKernelGGL(v2::k1_cols<R>, dim3(pl.M2 / pl.C), dim3(512), v2::kLdsBytes, s, pl, digits, cbuf_in, W);
  return hipGetLastError();
}
template <int R>
static hipError_t cols_back(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s) {
  hipLaunchKernelGGL((v2::k3_cols<R, false>), dim3(pl.M2 / pl.C), dim3(512), v2::kLdsBytes, s, pl, W, digits, cbuf, a, BackExt());
  return hipGetLastError();
}
template <int R>
static hipError_t cols_back_ext(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& x, hipStream_t s) {
  hipLaunchKernelGGL((v2::k3_cols<R, true>), dim3(pl.M2 / pl.C), dim3(512), v2::kLdsBytes, s, pl, W, digits, cbuf, a, x);
  return hipGetLastError();
}
template <int R>
static hipError_t cols_fourstep(const DevPlan& pl, uint64_t* f0f, uint64_t* f0i, uint64_t* fbf, uint64_t* fbi, hipStream_t s) {
  hipLaunchKernelGGL(v2::k_build_f0<R>, dim3(pl.M2 / pl.C), dim3(512), 0, s, pl, f0f, f0i, fbf, fbi);
  return hipGetLastError();
}
template <int R>
static ColSweeps cols() { return {cols_front<R>, cols_back<R>, cols_back_ext<R>, cols_fourstep<R>}; }
ColSweeps v2_cols(uint32_t R) { return R == 1 ? cols<1>() : R == 2 ? cols<2>() : cols<4>(); }

// rows: one instantiation per mode (the squaring kernel carries no multiply / image code); H = 2: rows of 8192 (1024 threads),
// RL = 1: rows of 2048, two to a tile (Pairs) or one with a plane per thread (Planes).  The modes of a family are listed once, in
// row_kernel: the launcher and v2_configure both read that table.
using RowKernel = void (*)(DevPlan, const uint64_t*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*);
constexpr int kRowModes = 5;
template <class Form, int H, int RL>
static RowKernel row_kernel(int mode) {
  static const RowKernel k[kRowModes] = {v2::k2_rows<Form, 0, H, RL>, v2::k2_rows<Form, 1, H, RL>, v2::k2_rows<Form, 2, H, RL>, v2::k2_rows<Form, 3, H, RL>,
                                         v2::k2_rows<Form, 4, H, RL>};
  return (mode >= 0 && mode < kRowModes) ? k[mode] : nullptr;
}
template <class Form, int H, int RL>
static hipError_t rows(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) {
  const RowKernel k = row_kernel<Form, H, RL>(mode);
  if (!k) return hipErrorInvalidValue;
  constexpr uint32_t kRowsPerTile = RL ? Form::kTilePairs / 2048 : 1;   // rows of 2048: two to a tile of pairs, one to a tile of planes
  hipLaunchKernelGGL(k, dim3(pl.M1 / kRowsPerTile), dim3(512 * H), H * Form::kLds, s, pl, Win, Y, Y2, Wimg, Wout);
  return hipGetLastError();
}
hipError_t v2_rows4096(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) { return rows<v2::Pairs, 1, 0>(pl, Win, Y, Y2, Wimg, Wout, mode, s); }
hipError_t v2_rows8192(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) { return rows<v2::Pairs, 2, 0>(pl, Win, Y, Y2, Wimg, Wout, mode, s); }
hipError_t v2_rows2048_two(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) { return rows<v2::Pairs, 1, 1>(pl, Win, Y, Y2, Wimg, Wout, mode, s); }
hipError_t v2_rows2048_one(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) { return rows<v2::Planes, 1, 1>(pl, Win, Y, Y2, Wimg, Wout, mode, s); }

// more than 64 KiB of LDS per work-group must be asked for, kernel by kernel (the plane rows use 32 KiB: nothing to set)
static hipError_t set_lds(const void* kernel, size_t bytes) { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)); }
template <int H, int RL>
static hipError_t configure_rows() {
  for (int mode = 0; mode < kRowModes; ++mode) {
    const hipError_t e = set_lds(reinterpret_cast<const void*>(row_kernel<v2::Pairs, H, RL>(mode)), H * v2::Pairs::kLds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t v2_configure() {
  hipError_t e = configure_rows<1, 0>();
  if (e == hipSuccess) e = configure_rows<2, 0>();
  if (e == hipSuccess) e = configure_rows<1, 1>();
  for (const void* f : {reinterpret_cast<const void*>(v2::k1_cols<1>), reinterpret_cast<const void*>(v2::k1_cols<2>), reinterpret_cast<const void*>(v2::k1_cols<4>),
                        reinterpret_cast<const void*>(v2::k3_cols<1, false>), reinterpret_cast<const void*>(v2::k3_cols<2, false>), reinterpret_cast<const void*>(v2::k3_cols<4, false>),
                        reinterpret_cast<const void*>(v2::k3_cols<1, true>), reinterpret_cast<const void*>(v2::k3_cols<2, true>), reinterpret_cast<const void*>(v2::k3_cols<4, true>)})
    if (e == hipSuccess) e = set_lds(f, v2::kLdsBytes);
  return e == hipSuccess ? v5_configure() : e;
}

#if defined(MI355_PROBE)
hipError_t v2_probe_launch(const DevPlan& pl, int kind, int grid_mult, int extra_lds, const uint32_t* digits, uint64_t* cbuf, uint64_t* W, uint32_t* dout, hipStream_t s) {
  const size_t lds = v2::kLdsBytes + size_t(extra_lds);
  if (kind == 1) {
    hipError_t e = set_lds(reinterpret_cast<const void*>(v2::k2_rows<v2::Pairs, 0, 1, 0>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((v2::k2_rows<v2::Pairs, 0, 1, 0>), dim3(pl.M1 * grid_mult), dim3(512), lds, s, pl, W, nullptr, nullptr, nullptr, W);
    return hipGetLastError();
  }
  const dim3 grid((pl.M2 / pl.C) * grid_mult), block(512);
  if (kind == 0) {
    hipError_t e = set_lds(reinterpret_cast<const void*>(v2::k1_cols<2>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(v2::k1_cols<2>, grid, block, lds, s, pl, digits, cbuf, W);
  } else {
    hipError_t e = set_lds(reinterpret_cast<const void*>(v2::k3_cols<2, false>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((v2::k3_cols<2, false>), grid, block, lds, s, pl, W, dout, cbuf, 1u, BackExt());
  }
  return hipGetLastError();
}
#endif

}  // namespace mi355
