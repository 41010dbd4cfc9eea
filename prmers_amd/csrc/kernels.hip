// gfx950 kernels for the Goldilocks IBDWT squaring (generic, size-agnostic set).
//
// One squaring x <- x^2 * a mod 2^p-1 is three sweeps over m = n/2 pairs (u64,u64), m = M1 x M2:
//   k_front : digits(u32, tile-major) -> weight -> length-M1 column DFT (LDS) -> twiddle -> work buffer
//   k_middle: length-M2 row DFT (LDS) -> pointwise square / multiply mod (t^2 - rho) -> inverse row DFT
//   k_back  : twiddle^-1 -> inverse column DFT (LDS) -> unweight -> base-2^width carry over runs of 2C
//             digits -> digits(u32) + one carry word per run
//   k_carry_fix: adds each run's carry word into the first digits of the next run (weak carry)
//   k_onelaunch: the three sweeps of a small transform (n <= 8192) in one launch, a whole residue per work-group, work buffer in LDS
//   k_batch: a queue of such products, run-wise sums and differences and copies in one launch, every work-group for its own residues
// This replaces the reference's kernel chain forward64_0 / forward256 / sqr512 / backward256 /
// backward64_0 / carry_weight_mul_p1 / carry_weight_p2 (include/marin/engine_gpu.h:1568-1630,
// kernels/marin.cl:989-1075,1517-1528,1696-1728,2198-2216).  Butterfly algebra follows
// marin.cl:304-392 (radix-4 with sqrt(-1), pair squaring mod t^2 - rho), restated for a plain
// DIF/DIT ordering with universal root tables.
//
// All kernels take the geometry in a DevPlan by value; nothing is compiled per exponent.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "gf.hpp"
#include "kernels.hpp"

namespace mi355 {

struct alignas(16) P2 { uint64_t a, b; };

__device__ __forceinline__ P2 p2_add(P2 x, P2 y) { return {gf::add(x.a, y.a), gf::add(x.b, y.b)}; }
__device__ __forceinline__ P2 p2_sub(P2 x, P2 y) { return {gf::sub(x.a, y.a), gf::sub(x.b, y.b)}; }
__device__ __forceinline__ P2 p2_mul(P2 x, uint64_t w) { return {gf::mul(x.a, w), gf::mul(x.b, w)}; }
__device__ __forceinline__ P2 p2_shift48(P2 x) { return {gf::mul_pow2(x.a, 48), gf::mul_pow2(x.b, 48)}; }
// the same on one word of a pair (lds_pow2_passes, one plane per thread)
__device__ __forceinline__ uint64_t p2_add(uint64_t x, uint64_t y) { return gf::add(x, y); }
__device__ __forceinline__ uint64_t p2_sub(uint64_t x, uint64_t y) { return gf::sub(x, y); }
__device__ __forceinline__ uint64_t p2_mul(uint64_t x, uint64_t w) { return gf::mul(x, w); }
__device__ __forceinline__ uint64_t p2_shift48(uint64_t x) { return gf::mul_pow2(x, 48); }

// omega_m^e from the two-level table (e < m)
__device__ __forceinline__ uint64_t tw_lookup(const DevPlan& pl, uint64_t e) {
  const uint64_t lo = pl.TWlo[e & ((1u << pl.twh) - 1)], hi = pl.TWhi[e >> pl.twh];
  return gf::mul(lo, hi);
}

// column-DFT output slot -> frequency k1 (radix-5 block major, bit reversed inside the block)
__device__ __forceinline__ uint32_t freq1(const DevPlan& pl, uint32_t pos) {
  const uint32_t blk = pos >> pl.logL1, q = pos & (pl.L1 - 1);   // L1 is a power of two
  const uint32_t rq = pl.logL1 ? (__brev(q) >> (32 - pl.logL1)) : 0u;
  return col_label(pl, blk, rq);
}

// p*j mod n for digit (i1, x = 2*i2+b), its width, and whether the factored weight wrapped
__device__ __forceinline__ void digit_info(const DevPlan& pl, uint32_t sa, uint32_t sb, uint32_t& width, bool& wrap) {
  uint64_t s = uint64_t(sa) + sb;
  wrap = (sa > 0) && (sb > 0) && (s <= pl.n);
  if (s >= pl.n) s -= pl.n;
  width = pl.q + ((s + pl.t > 0) ? 1u : 0u) + ((s + pl.t > pl.n) ? 1u : 0u) - ((s > 0) ? 1u : 0u);
}

// ---------------------------------------------------------------------------------------------
// radix-4 / radix-2 passes over an LDS array of pairs.
// Elements of one transform sit at X[(base + i) * stride + col]; `groups` independent transforms of
// length L (blocks x columns) are processed by the whole work-group.  root[e * rstep] = omega_L^e.
// ---------------------------------------------------------------------------------------------
// E = P2: a butterfly of pairs per thread.  E = uint64_t: one PLANE of it (the two words of a pair go through identical, independent
// arithmetic; element e, plane b at word 2 e + b): twice the threads, half the instruction stream per wave.  Small tiles are
// latency-bound -- one or two waves per SIMD, so a launch lasts as long as the dependent instruction stream of one wave (C2: 0.041 ms for
// three launches whose VALU work is 3 us) -- and the way to shorten that stream is more threads with less work each, not wider
// butterflies (a radix-8 form made C2 35 % slower).
template <bool INVERSE, class E>
__device__ __forceinline__ void lds_pow2_passes(P2* Xp, uint32_t L, uint32_t logL, uint32_t nblocks, uint32_t ncols, uint32_t logcols,
                                                const uint64_t* __restrict__ root, uint32_t rootN, uint32_t rstep, uint32_t tid, uint32_t nthr) {
  constexpr uint32_t W = sizeof(P2) / sizeof(E);   // E's per pair
  E* X = reinterpret_cast<E*>(Xp);
  // forward: len = L, L/4, ... (radix-4) then a final radix-2 when log2 L is odd; inverse mirrors
  const uint32_t n4 = logL / 2, has2 = logL & 1;
  const uint32_t npass = n4 + has2;
  for (uint32_t ps = 0; ps < npass; ++ps) {
    const uint32_t pf = INVERSE ? (npass - 1 - ps) : ps;  // pass index in forward order
    if (pf < n4) {
      const uint32_t loglen = logL - 2 * pf, len = 1u << loglen, q = len >> 2;
      const uint32_t per = L >> 2;  // butterflies per transform
      const uint32_t total = per * nblocks * ncols * W;
      const uint32_t tstep = (L >> loglen) * rstep;  // omega_len^t = root[t * tstep]
      for (uint32_t idxw = tid; idxw < total; idxw += nthr) {
        // W, ncols, per and q are powers of two: shifts and masks, no integer division in the loop
        const uint32_t plane = idxw & (W - 1), idx = idxw / W;
        const uint32_t col = idx & (ncols - 1), bi = idx >> logcols;
        const uint32_t blk = bi >> (logL - 2), bj = bi & (per - 1);
        const uint32_t sub = bj >> (loglen - 2), t = bj & (q - 1);
        const uint32_t e0 = W * ((blk * L + sub * len + t) * ncols + col) + plane, es = W * q * ncols;
        const uint32_t r1 = t * tstep;
        const E x0 = X[e0], x1 = X[e0 + es], x2 = X[e0 + 2 * es], x3 = X[e0 + 3 * es];
        if (!INVERSE) {
          const uint64_t w1 = root[r1], w2 = root[2 * r1], w3 = root[3 * r1];
          const E a = p2_add(x0, x2), b = p2_add(x1, x3), c = p2_sub(x0, x2), d = p2_shift48(p2_sub(x1, x3));   // omega_4 = 2^48 (checked in make_plan)
          X[e0] = p2_add(a, b);
          X[e0 + es] = p2_mul(p2_sub(a, b), w2);
          X[e0 + 2 * es] = p2_mul(p2_add(c, d), w1);
          X[e0 + 3 * es] = p2_mul(p2_sub(c, d), w3);
        } else {
          // inverse roots: omega^-e = root[(N - e) % N]
          const uint64_t w1 = root[r1 ? rootN - r1 : 0], w2 = root[r1 ? rootN - 2 * r1 : 0], w3 = root[r1 ? rootN - 3 * r1 : 0];
          const E y1 = p2_mul(x1, w2);
          const E A = p2_add(x0, y1), B = p2_sub(x0, y1);
          const E y2 = p2_mul(x2, w1), y3 = p2_mul(x3, w3);
          const E Cc = p2_add(y2, y3), D = p2_shift48(p2_sub(y3, y2));   // omega_4^-1 = -2^48
          X[e0] = p2_add(A, Cc);
          X[e0 + 2 * es] = p2_sub(A, Cc);
          X[e0 + es] = p2_add(B, D);
          X[e0 + 3 * es] = p2_sub(B, D);
        }
      }
    } else {
      // radix-2, len = 2: no twiddle
      const uint32_t per = L >> 1, total = per * nblocks * ncols * W;
      for (uint32_t idxw = tid; idxw < total; idxw += nthr) {
        const uint32_t plane = idxw & (W - 1), idx = idxw / W;
        const uint32_t col = idx & (ncols - 1), bi = idx >> logcols;
        const uint32_t blk = bi >> (logL - 1), bj = bi & (per - 1);
        const uint32_t e0 = W * ((blk * L + 2 * bj) * ncols + col) + plane;
        const E u = X[e0], v = X[e0 + W * ncols];
        X[e0] = p2_add(u, v);
        X[e0 + W * ncols] = p2_sub(u, v);
      }
    }
    __syncthreads();
  }
}

template <bool INVERSE>
__device__ __forceinline__ void lds_pow2_dft(P2* X, uint32_t L, uint32_t logL, uint32_t nblocks, uint32_t ncols, uint32_t logcols,
                                             const uint64_t* __restrict__ root, uint32_t rootN, uint32_t rstep, uint32_t tid, uint32_t nthr) {
  // small tiles: one plane per thread (see above); the work-group was sized for that by the launcher
  if (nthr * 2 >= (L >> 2) * nblocks * ncols * 2 && nthr > (L >> 2) * nblocks * ncols) {
    lds_pow2_passes<INVERSE, uint64_t>(X, L, logL, nblocks, ncols, logcols, root, rootN, rstep, tid, nthr);
  } else {
    lds_pow2_passes<INVERSE, P2>(X, L, logL, nblocks, ncols, logcols, root, rootN, rstep, tid, nthr);
  }
}

// 5-point DFT, X[k] = sum_r x[r] w^(rk) with w = omega_5 (INVERSE: w^-1), 4 general multiplications:
//   t1 = x1+x4, t2 = x2+x3, t3 = x1-x4, t4 = x2-x3, t5 = t1+t2;  X0 = x0 + t5
//   A = x0 - t5/4 (1 + (w+w^4) + (w^2+w^3) = 0; -1/4 = 2^94);  B1,2 = A +- beta (t1 - t2), beta = ((w+w^4) - (w^2+w^3))/4
//   P = k1 t3 + k2 t4, Q = k2 t3 - k1 t4 with k1 = (w-w^4)/2, k2 = (w^2-w^3)/2, from three products
//   k1 (t3+t4), (k2-k1) t4, (k1+k2) t3;  X1,4 = B1 +- P, X2,3 = B2 +- Q (signs swapped for the inverse).
// c5 = {beta, k1, k2-k1, k1+k2} (plan.hpp).
template <bool INVERSE>
__device__ __forceinline__ void dft5(P2 (&x)[5], const uint64_t (&c5)[4]) {
  const P2 t1 = p2_add(x[1], x[4]), t2 = p2_add(x[2], x[3]), t3 = p2_sub(x[1], x[4]), t4 = p2_sub(x[2], x[3]);
  const P2 t5 = p2_add(t1, t2);
  const P2 A = p2_add(x[0], P2{gf::mul_pow2(t5.a, 94), gf::mul_pow2(t5.b, 94)});
  const P2 m2 = p2_mul(p2_sub(t1, t2), c5[0]);
  const P2 B1 = p2_add(A, m2), B2 = p2_sub(A, m2);
  const P2 m3 = p2_mul(p2_add(t3, t4), c5[1]), m4 = p2_mul(t4, c5[2]), m5 = p2_mul(t3, c5[3]);
  const P2 Pp = p2_add(m3, m4), Q = p2_sub(m5, m3);
  x[0] = p2_add(x[0], t5);
  if (!INVERSE) { x[1] = p2_add(B1, Pp); x[4] = p2_sub(B1, Pp); x[2] = p2_add(B2, Q); x[3] = p2_sub(B2, Q); }
  else          { x[1] = p2_sub(B1, Pp); x[4] = p2_add(B1, Pp); x[2] = p2_sub(B2, Q); x[3] = p2_add(B2, Q); }
}

// radix-5 stage of the column DFT (first forward / last inverse): 5 blocks of L1.
// Mixed-radix form (lab_u == 1: the split sweeps, and every plan with L1 = 1): inputs (L1 r + t), twiddle omega_M1^(t k) on output k.
// Prime-factor form (round 4; 5 and L1 are coprime): inputs i1 = (L1 r + 5 t) mod M1, no twiddle, output k0 in place at L1 k0 + (5 t mod L1) --
// the same five slots -- so block k0 holds its sequence permuted by t -> 5 t mod L1, the power-of-two transform of that block puts the
// frequency kr = 5 k mod L1 at output k, and slot (k0, k) holds the column frequency (lab_u k0 + 5 k) mod M1 with lab_u = L1 (L1^-1 mod 5):
// the frequency label the engine hands to every kernel (kernels.hpp col_label).  Four table products per butterfly and direction fewer.
template <bool INVERSE>
__device__ __forceinline__ void lds_radix5(const DevPlan& pl, P2* X, uint32_t ncols, uint32_t tid, uint32_t nthr) {
  const uint32_t L1 = pl.L1, total = L1 * ncols;
  const bool pfa = pl.lab_u != 1;
  for (uint32_t idx = tid; idx < total; idx += nthr) {
    const uint32_t col = idx & (ncols - 1), t = idx >> pl.logC;   // ncols = C
    const uint32_t t5 = 5 * t, rho = pfa ? (t5 & (L1 - 1)) : t, w0 = pfa ? (t5 >> pl.logL1) : 0u;   // 5 t = rho + L1 w0: input r sits in block (r + w0) mod 5
    P2 x[5];
    if (!INVERSE) {
#pragma unroll
      for (uint32_t r = 0; r < 5; ++r) { const uint32_t b = r + w0; x[r] = X[(L1 * (b >= 5 ? b - 5 : b) + rho) * ncols + col]; }
      dft5<false>(x, pl.W5c);
      if (!pfa) {
#pragma unroll
        for (int k = 1; k < 5; ++k) x[k] = p2_mul(x[k], pl.UT1[t * k]);  // t*k < M1
      }
#pragma unroll
      for (int r = 0; r < 5; ++r) X[(L1 * r + rho) * ncols + col] = x[r];
    } else {
#pragma unroll
      for (int r = 0; r < 5; ++r) x[r] = X[(L1 * r + rho) * ncols + col];
      if (!pfa) {
#pragma unroll
        for (int k = 1; k < 5; ++k) x[k] = p2_mul(x[k], pl.UT1[(t * k) ? pl.M1 - t * k : 0]);
      }
      dft5<true>(x, pl.W5c);
#pragma unroll
      for (uint32_t r = 0; r < 5; ++r) { const uint32_t b = r + w0; X[(L1 * (b >= 5 ? b - 5 : b) + rho) * ncols + col] = x[r]; }
    }
  }
  __syncthreads();
}

extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

// Lanes (kernels.hpp DevPlan.lanes): blockIdx.y is the lane, blockIdx.x what it is without lanes.  Every kernel moves its pointers, which
// are those of lane 0, to its lane first; null stays null.  64-bit offsets: a lane may lie beyond 4 GiB.
// Every entry point is compiled twice from its one source, k<LANES>: k<false>, which a plain engine launches (pl.lanes == 1), leaves the
// pointers alone.  As a run-time offset of lane 0 the same arithmetic cost the latency-bound launches of a plain engine 0.8-3.4 %
// (profiles/generic_one_entry_ab.txt).
template <bool LANES, class T> __device__ __forceinline__ T* lane_reg(const DevPlan& pl, T* p) {   // a register, the work buffer or an image: 8 n bytes a lane
  if (!LANES) return p;
  return p ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + uint64_t(blockIdx.y) * pl.n * 8) : nullptr;
}
template <bool LANES, class T> __device__ __forceinline__ T* lane_cbuf(const DevPlan& pl, T* p) {   // a carry buffer: one word per run
  if (!LANES) return p;
  return p ? p + uint64_t(blockIdx.y) * pl.M1 * (pl.M2 >> pl.logC) : nullptr;
}

// previous run (in digit order) of run (T, i1): same row, previous tile; first tile wraps to the
// last tile of the previous row (cyclic: 2^p = 1)
__device__ __forceinline__ uint64_t carry_in_of(const DevPlan& pl, const uint64_t* cbuf, uint32_t T, uint32_t i1) {
  const uint32_t NT = pl.M2 / pl.C;
  if (T > 0) return *(cbuf + size_t(T - 1) * pl.M1 + i1);
  return *(cbuf + size_t(NT - 1) * pl.M1 + (i1 ? i1 - 1 : pl.M1 - 1));
}

// Digit k (value v, `width` bits) of a run of ndig digits takes the run's incoming carry word c (weak carry: adc4, marin.cl:203-212): three
// masked digits, the remainder stays on the fourth; runs of two digits (C = 1) take all of it on the second.
__device__ __forceinline__ uint64_t take_carry_in(uint64_t v, uint64_t& c, uint32_t k, uint32_t ndig, uint32_t width) {
  if (k < 3 && k + 1 < ndig) { v += c; c = v >> width; v &= (uint64_t(1) << width) - 1; }
  else if (k == 3 || k + 1 == ndig) { v += c; c = 0; }
  return v;
}
// the same for a tile kernel that holds the run's first four digits dd (C >= 2)
__device__ __forceinline__ void run_carry_in(const DevPlan& pl, uint32_t sa, uint32_t T, uint64_t cin, uint32_t (&dd)[4]) {
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    uint32_t width; bool wr;
    digit_info(pl, sa, pl.SB[2 * (T * pl.C) + k], width, wr);
    dd[k] = uint32_t(take_carry_in(dd[k], cin, k, 4, width));
  }
}

// Weighted pair of the digits d of pair (i1, i2), sb = SB[2 i2]: weight = TA * TB / (wrap ? 2 : 1), TB left to the four-step twiddle.  The
// odd digit takes its exponent split from the second half of SA / TA (plan.hpp) so that both digits of the pair share the column factor
// TB[2 i2]; the halving sits on TA and the digits that do not wrap are doubled instead (a digit is below 2^width <= 2^30, and below 2^31
// where it keeps the rest of a carry-in, plan.hpp carry_chain_ok: the doubled digit still fits 32 bits and the product stays a mul_u32).
__device__ __forceinline__ P2 weigh_pair(const DevPlan& pl, uint32_t i1, uint32_t sb, uint2 d) {
  uint32_t w0, w1; bool wr0, wr1;
  digit_info(pl, pl.SA[i1], sb, w0, wr0);
  digit_info(pl, pl.SA[pl.M1 + i1], sb, w1, wr1);
  return {gf::mul_u32(pl.TAh[i1], d.x << (wr0 ? 0 : 1)), gf::mul_u32(pl.TAh[pl.M1 + i1], d.y << (wr1 ? 0 : 1))};
}

// Four-step twiddle of work-buffer element (pos, i2) times the column factor of its pair: omega_m^(i2 k1) TB[2 i2], INVERSE the inverse of both.
// have: pre holds the three table words of the forward one, requested earlier (front_body).
struct TwPre { uint64_t lo = 0, hi = 0, tb = 0; };
template <bool INVERSE>
__device__ __forceinline__ uint64_t fourstep_word(const DevPlan& pl, uint32_t pos, uint32_t i2, bool have = false, TwPre pre = TwPre()) {
  const uint32_t ex = i2 * freq1(pl, pos);   // i2 < M2, k1 < M1: below m, no reduction needed
  const uint64_t tw = have ? gf::mul(pre.lo, pre.hi) : tw_lookup(pl, INVERSE ? (ex ? pl.m - ex : 0) : ex);
  return gf::mul(tw, have ? pre.tb : INVERSE ? pl.TBi[2 * i2] : pl.TB[2 * i2]);
}

// ---------------------------------------------------------------------------------------------
// front: one work-group per tile T (C adjacent columns, all M1 rows)
// ---------------------------------------------------------------------------------------------
// body of the front sweep for tile T.  Offsets go onto the pointers one at a time (dg + i1 * C + c, not dg[i1 * C + c], here and in
// back_body): a 32-bit sum may wrap, and the compiler then no longer merges the neighbouring accesses.
// WB: the work buffer's element type as the caller has it -- words of global memory (k_front) or pairs of the LDS array (k_onelaunch, which
// hands over an offset of smem_raw itself: once inlined, the accesses are LDS accesses, not flat ones).  The same in middle_body and back_body.
template <class WB>
__device__ __forceinline__ void front_body(const DevPlan& pl, const uint32_t* digits, const uint64_t* cbuf_in, WB* Wout, uint32_t T,
                                           P2* X, uint32_t tid, uint32_t nthr) {
  const uint32_t C = pl.C, M1 = pl.M1, tile = M1 * C;
  const uint2* dg = reinterpret_cast<const uint2*>(digits) + size_t(T) * tile;

  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t i1 = e >> pl.logC, c = e & (C - 1), i2 = T * C + c;
    uint2 d = dg[e];
    const uint32_t sa = pl.SA[i1];   // before the branch: inside it the load is issued a second time for the weighting (12 instructions more)
    if (cbuf_in && c < 2) {
      // deferred run carries (C >= 2): the carry word left by the previous run goes into the first digits of this one.  The two
      // threads that own the run's first two pairs each redo the four-digit chain and keep their pair.
      const uint64_t cin = carry_in_of(pl, cbuf_in, T, i1);
      if (cin) {
        const uint2* run = dg + i1 * C;
        const uint2 p0 = run[0], p1 = run[1];
        uint32_t dd[4] = {p0.x, p0.y, p1.x, p1.y};
        run_carry_in(pl, sa, T, cin, dd);
        d = c ? make_uint2(dd[2], dd[3]) : make_uint2(dd[0], dd[1]);
      }
    }
    X[e] = weigh_pair(pl, i1, pl.SB[2 * i2], d);
  }
  __syncthreads();

  // small tiles (one output element per thread): the three table words of its four-step twiddle are requested before the transform,
  // whose passes hide their latency (latency-bound launches: see lds_pow2_passes)
  const bool one = tile <= nthr;
  TwPre pre;
  if (one && tid < tile) {
    const uint32_t pos = tid >> pl.logC, i2 = T * C + (tid & (C - 1));
    const uint64_t ex = uint64_t(i2) * freq1(pl, pos);
    pre.lo = pl.TWlo[ex & ((1u << pl.twh) - 1)]; pre.hi = pl.TWhi[ex >> pl.twh]; pre.tb = pl.TB[2 * i2];
  }
  if (pl.r5 == 5) lds_radix5<false>(pl, X, C, tid, nthr);
  if (pl.logL1) lds_pow2_dft<false>(X, pl.L1, pl.logL1, pl.r5, C, pl.logC, pl.UT1, M1, pl.r5, tid, nthr);

  P2* W = reinterpret_cast<P2*>(Wout);
  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t pos = e >> pl.logC, i2 = T * C + (e & (C - 1));
    P2* out = W + size_t(pos) * pl.M2 + i2;
    *out = p2_mul(X[e], fourstep_word<false>(pl, pos, i2, one, pre));
  }
}
template <bool LANES>
__global__ void __launch_bounds__(1024) k_front(DevPlan pl, const uint32_t* __restrict__ digits, const uint64_t* __restrict__ cbuf_in,
                                                uint64_t* __restrict__ Wout) {
  if (blockIdx.x >= pl.boost_tiles) __builtin_amdgcn_s_setprio(3);   // last half round: see kernels_v2.hip, boost_if_late (C4: -2.7 %); never with lanes
  front_body(pl, lane_reg<LANES>(pl, digits), lane_cbuf<LANES>(pl, cbuf_in), lane_reg<LANES>(pl, Wout), blockIdx.x, reinterpret_cast<P2*>(smem_raw), threadIdx.x, blockDim.x);
}

// ---------------------------------------------------------------------------------------------
// middle: one work-group per row.  mode 0: square, 1: multiply by image Y, 2: forward only, 3: multiply by the sum of the images Y and Y2.
// mode 4 (KEEP, k_middle_keep): mode 0 that also stores the forward transform of the operand to Wimg, as mode 2 would store it.
// ---------------------------------------------------------------------------------------------
// live (k_onelaunch: a lane beyond the last one, which only keeps its group's barriers company): false stores nothing to memory.
template <bool KEEP = false, class WI, class WO>
__device__ __forceinline__ void middle_body(const DevPlan& pl, const WI* Win, const uint64_t* Yimg, const uint64_t* Yimg2, WO* Wout, int mode, uint32_t row,
                                            P2* X, uint32_t tid, uint32_t nthr, uint64_t* Wimg = nullptr, bool live = true) {
  const uint32_t M2 = pl.M2;
  const P2* in = reinterpret_cast<const P2*>(Win) + size_t(row) * M2;
  P2* out = reinterpret_cast<P2*>(Wout) + size_t(row) * M2;

  for (uint32_t e = tid; e < M2; e += nthr) X[e] = in[e];
  __syncthreads();
  const uint32_t k1 = freq1(pl, row);
  const bool one = M2 <= nthr;   // one element per thread: its twiddle words are requested before the transform (see k_front)
  uint64_t pre_lo = 0, pre_hi = 0;
  if (one && tid < M2 && mode != 2) {
    const uint64_t ex = rho_exponent(pl, k1, __brev(tid) >> (32 - pl.logM2));
    pre_lo = pl.TWlo[ex & ((1u << pl.twh) - 1)]; pre_hi = pl.TWhi[ex >> pl.twh];
  }
  lds_pow2_dft<false>(X, M2, pl.logM2, 1, 1, 0, pl.UT2, M2, 1, tid, nthr);
  if (mode == 2) {   // (Wout is the image here: memory)
    if (live) for (uint32_t e = tid; e < M2; e += nthr) out[e] = X[e];
    return;
  }
  if constexpr (KEEP) {   // every thread stores the elements it squares next: no barrier between the two
    P2* img = reinterpret_cast<P2*>(Wimg) + size_t(row) * M2;
    if (live) for (uint32_t e = tid; e < M2; e += nthr) img[e] = X[e];
  }
  const P2* Y = reinterpret_cast<const P2*>(Yimg) + size_t(row) * M2;
  for (uint32_t e = tid; e < M2; e += nthr) {
    const uint32_t k2 = __brev(e) >> (32 - pl.logM2);
    const uint64_t rho = one ? gf::mul(pre_lo, pre_hi) : tw_lookup(pl, rho_exponent(pl, k1, k2));
    const P2 u = X[e];
    P2 r;
    if (mode == 0) {  // (u0 + u1 t)^2 mod (t^2 - rho), marin.cl:379-384
      r.a = gf::add(gf::sqr(u.a), gf::mul(gf::sqr(u.b), rho));
      r.b = gf::mul(u.b, gf::dbl(u.a));
    } else {          // marin.cl:387-392
      P2 y = Y[e];
      if (mode == 3) {   // the image of a sum is the word-wise sum of the images (lazy: the products below take any representative)
        const P2 z = reinterpret_cast<const P2*>(Yimg2)[size_t(row) * M2 + e];
        y = {gf::add_lazy_any(y.a, z.a), gf::add_lazy_any(y.b, z.b)};
      }
      r.a = gf::add(gf::mul(u.a, y.a), gf::mul(gf::mul(u.b, y.b), rho));
      r.b = gf::add(gf::mul(u.a, y.b), gf::mul(u.b, y.a));
    }
    X[e] = r;
  }
  __syncthreads();
  lds_pow2_dft<true>(X, M2, pl.logM2, 1, 1, 0, pl.UT2, M2, 1, tid, nthr);
  for (uint32_t e = tid; e < M2; e += nthr) out[e] = X[e];
}
template <bool LANES>
__global__ void __launch_bounds__(1024) k_middle(DevPlan pl, const uint64_t* __restrict__ Win, const uint64_t* __restrict__ Yimg,
                                                const uint64_t* __restrict__ Yimg2, uint64_t* __restrict__ Wout, int mode) {
  middle_body(pl, lane_reg<LANES>(pl, Win), lane_reg<LANES>(pl, Yimg), lane_reg<LANES>(pl, Yimg2), lane_reg<LANES>(pl, Wout), mode, blockIdx.x, reinterpret_cast<P2*>(smem_raw),
              threadIdx.x, blockDim.x);
}
template <bool LANES>
__global__ void __launch_bounds__(1024) k_middle_keep(DevPlan pl, const uint64_t* __restrict__ Win, uint64_t* __restrict__ Wimg, uint64_t* __restrict__ Wout) {
  middle_body<true>(pl, lane_reg<LANES>(pl, Win), nullptr, nullptr, lane_reg<LANES>(pl, Wout), 0, blockIdx.x, reinterpret_cast<P2*>(smem_raw), threadIdx.x, blockDim.x,
                    lane_reg<LANES>(pl, Wimg));
}
// Across lanes (include/mi355_lanecross.h): the one place where a lane reads another lane's data.  The sibling block of size 2^level of
// lane l starts at lane ((l >> level) ^ 1) << level (level <= 31, so below 2^32 for every lane an engine can have; 64 bits all the same).
__device__ __forceinline__ uint64_t sibling_lane(uint32_t lane, uint32_t level) { return ((uint64_t(lane) >> level) ^ 1u) << level; }
// mode 1 whose multiplicand image is the sibling lane's image of Ysrc where that lane exists, else the own lane's image of Yalt (lane
// engines only: the lane is blockIdx.y).  Ysrc, Yalt are those of lane 0; a lane is pl.n words of 8 bytes, offsets in 64 bits.
__global__ void __launch_bounds__(1024) k_middle_sibling(DevPlan pl, const uint64_t* __restrict__ Win, const uint64_t* __restrict__ Ysrc,
                                                        const uint64_t* __restrict__ Yalt, uint64_t* __restrict__ Wout, uint32_t level) {
  const uint64_t g = sibling_lane(blockIdx.y, level);
  const uint64_t* Y = g < pl.lanes ? Ysrc + g * pl.n : Yalt + uint64_t(blockIdx.y) * pl.n;
  middle_body(pl, lane_reg<true>(pl, Win), Y, nullptr, lane_reg<true>(pl, Wout), 1, blockIdx.x, reinterpret_cast<P2*>(smem_raw), threadIdx.x, blockDim.x);
}

// ---------------------------------------------------------------------------------------------
// back: inverse of front + unweight + carry over the tile's M1 runs of 2C digits
// ---------------------------------------------------------------------------------------------
// Row i1's unweighting factors, even / odd digit (second half of the tables: see weigh_pair); tai2 serves the wrapped exponents, whose
// weight was halved.  unweigh: word x of a pair of that row, digit b, column exponent sb = SB[2 i2] -> the unweighted value and its width.
struct RowUnweight { uint32_t sa[2]; uint64_t tai[2], tai2[2]; };
__device__ __forceinline__ RowUnweight row_unweight(const DevPlan& pl, uint32_t i1) {
  return {{pl.SA[i1], pl.SA[pl.M1 + i1]}, {pl.TAi[i1], pl.TAi[pl.M1 + i1]}, {pl.TAi2[i1], pl.TAi2[pl.M1 + i1]}};
}
__device__ __forceinline__ uint64_t unweigh(const DevPlan& pl, const RowUnweight& r, int b, uint32_t sb, uint64_t x, uint32_t& width) {
  bool wrap;
  digit_info(pl, r.sa[b], sb, width, wrap);
  return gf::mul(x, wrap ? r.tai2[b] : r.tai[b]);
}
// One step of the carry chain: u a + addend + carry -> a digit of `width` bits and the next carry
__device__ __forceinline__ uint32_t adc_mul(uint64_t u, uint32_t a, uint32_t addend, uint32_t width, uint64_t& carry) {
  const uint64_t mask = (uint64_t(1) << width) - 1;
  uint64_t r;
  if (a == 1) {               // the common case (uniform): no 64-bit multiplies
    r = u + carry + addend;   // u < P only (up to 0.62 2^64 at the top of a range), carry < 2^(64 - width), addend < 2^32: the sum stays below 2^64 (tests/chain_model.py)
    carry = r >> width;
  } else {                    // adc_mul (marin.cl:194-201): digit first, so that everything stays in 64 bits
    const uint64_t dlo = u & mask, chi = u >> width;
    r = dlo * a + carry + addend;
    carry = (r >> width) + chi * a;
  }
  return uint32_t(r & mask);
}

// blocks that share an XCD (b, b + 8, ...) take neighbouring tiles: the 64-byte pieces of a work-buffer line meet in one L2
// (same order as the register-resident back sweep; C4: 93.3 -> 90.4 us).  MI355_TUNE bit 0 switches it off.
__device__ __forceinline__ uint32_t xcd_tile(const DevPlan& pl, uint32_t b, uint32_t groups) {
  return (!(pl.tune & 1) && groups % 8 == 0) ? (b & 7) * (groups >> 3) + (b >> 3) : b;
}
template <bool EXT, class WB>
__device__ __forceinline__ void back_body(const DevPlan& pl, const WB* Win, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& ext, uint32_t T,
                                          P2* X, uint32_t tid, uint32_t nthr, bool live = true) {
  const uint32_t C = pl.C, M1 = pl.M1, tile = M1 * C;
  const P2* W = reinterpret_cast<const P2*>(Win);

  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t pos = e >> pl.logC, i2 = T * C + (e & (C - 1));
    const P2 x = *(W + size_t(pos) * pl.M2 + i2);
    X[e] = p2_mul(x, fourstep_word<true>(pl, pos, i2));   // one column factor per pair (see weigh_pair)
  }
  __syncthreads();

  if (pl.logL1) lds_pow2_dft<true>(X, pl.L1, pl.logL1, pl.r5, C, pl.logC, pl.UT1, M1, pl.r5, tid, nthr);
  if (pl.r5 == 5) lds_radix5<true>(pl, X, C, tid, nthr);

  uint2* dg = reinterpret_cast<uint2*>(digits) + size_t(T) * tile;
  for (uint32_t i1 = tid; i1 < M1; i1 += nthr) {
    const RowUnweight uw = row_unweight(pl, i1);
    uint64_t carry = 0;
    uint32_t addh[4] = {0, 0, 0, 0};   // first digits of the addend's run with its pending carry folded in (C >= 2)
    const uint2* ad = nullptr;
    if (EXT && ext.add_digits) {
      ad = reinterpret_cast<const uint2*>(ext.add_digits) + size_t(T) * tile + size_t(i1) * C;
      if (ext.add_cbuf) {
        const uint2 p0 = ad[0], p1 = ad[1];
        addh[0] = p0.x; addh[1] = p0.y; addh[2] = p1.x; addh[3] = p1.y;
        run_carry_in(pl, uw.sa[0], T, carry_in_of(pl, ext.add_cbuf, T, i1), addh);
      }
    }
    for (uint32_t c = 0; c < C; ++c) {
      const uint32_t i2 = T * C + c;
      const P2 x = X[i1 * C + c];
      const uint32_t sb = pl.SB[2 * i2];
      uint32_t out[2];
      uint32_t av[2] = {0, 0};
      if (EXT && ad) {
        if (ext.add_cbuf && c < 2) { av[0] = addh[2 * c]; av[1] = addh[2 * c + 1]; }
        else { const uint2 q = ad[c]; av[0] = q.x; av[1] = q.y; }
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        uint32_t width;
        const uint64_t u = unweigh(pl, uw, b, sb, b ? x.b : x.a, width);
        out[b] = adc_mul(u, a, EXT ? av[b] : 0u, width, carry);
      }
      if (!live) continue;   // (k_onelaunch, a lane beyond the last one: the chain ran, nothing leaves it)
      *(dg + i1 * C + c) = make_uint2(out[0], out[1]);
      if (EXT && ext.digits2) reinterpret_cast<uint2*>(ext.digits2)[size_t(T) * tile + size_t(i1) * C + c] = make_uint2(out[0], out[1]);
    }
    if (!live) continue;
    *(cbuf + size_t(T) * M1 + i1) = carry;
    if (EXT && ext.digits2) ext.cbuf2[size_t(T) * M1 + i1] = carry;
  }
}
template <bool EXT, bool LANES>
__global__ void __launch_bounds__(1024) k_back(DevPlan pl, const uint64_t* __restrict__ Win, uint32_t* __restrict__ digits,
                                              uint64_t* __restrict__ cbuf, uint32_t a, BackExt ext) {
  if (blockIdx.x >= pl.boost_tiles) __builtin_amdgcn_s_setprio(3);   // last half round: see kernels_v2.hip, boost_if_late (C4: -2.7 %); never with lanes
  BackExt x;
  if (EXT) {
    x.digits2 = lane_reg<LANES>(pl, ext.digits2); x.cbuf2 = lane_cbuf<LANES>(pl, ext.cbuf2);
    x.add_digits = lane_reg<LANES>(pl, ext.add_digits); x.add_cbuf = lane_cbuf<LANES>(pl, ext.add_cbuf);
  }
  back_body<EXT>(pl, lane_reg<LANES>(pl, Win), lane_reg<LANES>(pl, digits), lane_cbuf<LANES>(pl, cbuf), a, x, xcd_tile(pl, blockIdx.x, gridDim.x),
                 reinterpret_cast<P2*>(smem_raw), threadIdx.x, blockDim.x);
}

// ---------------------------------------------------------------------------------------------
// One launch for a whole product (plan token onelaunch, n <= 8192): front sweep, row sweep and back sweep of a lane in ONE work-group, with
// the work buffer in LDS instead of memory.  At these sizes the three launches above are dependent launches of almost no arithmetic, and
// a lane's column tile (8 pairs at p = 1277) leaves most of a wave idle.
// A work-group holds K whole lanes with TL threads each (plan.hpp onelaunch_shape): the lane is blockIdx.x K + threadIdx.x / TL.  Per lane
// LDS holds the work buffer (m pairs) and as much transform scratch.  A lane's threads split into teams that run the sweep bodies above
// side by side, one tile (front, back) or one row a team; every team makes the same number of trips and the bodies' barrier counts depend
// on the plan alone, so every thread of the group reaches every barrier.  The group's barriers separate the phases: all of a lane's digits
// are read before the first is written, so dst may be src.
// A tail group has lanes beyond the last one: they run on the last lane's inputs, reach every barrier and store nothing (live).
// Registers, carry words and images are those of the three launches: digits and carries bit for bit (exact integers), image words as
// field elements in the same order.
// ---------------------------------------------------------------------------------------------
// lane_reg / lane_cbuf for a lane that is not blockIdx.y.  The pointers come out of the argument block as plain pointers; they are device
// memory, and saying so keeps the accesses through them global ones instead of flat ones.
template <class T> __device__ __forceinline__ T* lane_at(T* p, uint32_t lane, uint64_t bytes) {
  typedef __attribute__((address_space(1))) unsigned char GlobalByte;
  return p ? (T*)((GlobalByte*)(p) + lane * bytes) : nullptr;
}
// The kernel's one argument: plan, operands and the back sweep's extras.  The kernel reads it through args_again(), the argument block
// behind a pointer the compiler does not see through, once per phase: each phase then loads the members it uses when it starts.  Read from
// the argument itself, the members of all three phases are loaded at the kernel's entry and stay in scalar registers to its end, more
// than a wave has (over a hundred of them spilled).  The argument block is constant memory, so these are scalar loads.
struct OneLaunchPack { DevPlan pl; OneLaunchArgs oa; BackExt x; };
__device__ __forceinline__ const OneLaunchPack& args_again() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();   // the only argument: offset 0
  asm volatile("" : "+s"(p));
  return *(const OneLaunchPack*)p;
}
// A thread's place in its group: its lane, whether that lane exists (live), the lane's LDS, and its team and thread of the team in the
// column phases (c...) and the row phase (r...).  Plan and block shape alone decide it: k_batch works it out once for all its operations.
struct LanePlace {
  uint32_t lane, lt, TL, cteam, cteams, ctid, ct, rteam, rteams, rtid, rt, NT, M1;
  uint64_t rb, cb;   // bytes of a lane's register, of its carry words
  bool live;
  P2 *W, *Xc, *Xr;   // the lane's work buffer; its team's transform scratch in the column and in the row phases
};
__device__ __forceinline__ LanePlace lane_place(const DevPlan& pl, uint32_t TL, uint32_t K) {
  LanePlace t;
  const uint32_t gl = threadIdx.x / TL, lt = threadIdx.x - gl * TL;   // lane of the group, thread of the lane
  t.lt = lt; t.TL = TL;
  t.live = blockIdx.x * K + gl < pl.lanes;
  t.lane = t.live ? blockIdx.x * K + gl : pl.lanes - 1;
  t.rb = uint64_t(pl.n) * 8; t.cb = uint64_t(pl.M1) * (pl.M2 >> pl.logC) * 8;
  t.W = reinterpret_cast<P2*>(smem_raw) + size_t(gl) * 2 * pl.m;   // the lane's work buffer; its transform scratch follows
  t.M1 = pl.M1; t.NT = pl.M2 >> pl.logC;
  // column teams: TL = r5 2^j threads over NT = 2^i tiles; row teams: over M1 = r5 L1 rows.  Each count divides both.
  t.cteams = min(t.NT, TL / pl.r5); t.ct = TL / t.cteams; t.cteam = lt / t.ct; t.ctid = lt - t.cteam * t.ct;
  t.rteams = min(t.M1, TL); t.rt = TL / t.rteams; t.rteam = lt / t.rt; t.rtid = lt - t.rteam * t.rt;
  t.Xc = t.W + pl.m + size_t(t.cteam) * (t.M1 << pl.logC);
  t.Xr = t.W + pl.m + size_t(t.rteam) * pl.M2;
  return t;
}
// The three phases of a product for the thread at t, for k_onelaunch and k_batch alike.  again() hands out plan, operands and extras anew
// (a view of three references behind a pointer the compiler does not see through); every trip of every phase asks for them, so nothing of
// one phase is held in scalar registers through another.  Every thread of the group reaches every barrier; mode 2 ends after the rows.
// SIB (k_onelaunch_sibling only; oa.mode is kModeSibling): the rows multiply by the image at oa.y of the lane's sibling of oa.level where
// that lane exists, else by the own lane's image at oa.y2.  The choice is the thread's: the lanes of a group, and of a wave where TL < 64,
// have different partners.  A lane beyond the last one multiplies by the last lane's choice, like everything it does.
template <bool EXT, bool SIB = false, class Again>
__device__ __forceinline__ void product_phases(const LanePlace& t, Again again) {
  for (uint32_t T = t.cteam; T < t.NT; T += t.cteams) {
    const auto& g = again();
    front_body(g.pl, lane_at(g.oa.src, t.lane, t.rb), lane_at(g.oa.src_cbuf, t.lane, t.cb), t.W, T, t.Xc, t.ctid, t.ct);
    __syncthreads();
  }

  for (uint32_t row = t.rteam; row < t.M1; row += t.rteams) {
    const auto& g = again();
    const uint32_t mode = uint32_t(g.oa.mode);
    uint64_t* img = lane_at(g.oa.img, t.lane, t.rb);
    if (mode == 2) middle_body(g.pl, t.W, nullptr, nullptr, img, 2, row, t.Xr, t.rtid, t.rt, nullptr, t.live);
    else if (mode == 4) middle_body<true>(g.pl, t.W, nullptr, nullptr, t.W, 0, row, t.Xr, t.rtid, t.rt, img, t.live);
    else if constexpr (SIB) {
      const uint64_t sib = sibling_lane(t.lane, g.oa.level);
      const uint64_t* y = sib < g.pl.lanes ? lane_at(g.oa.y, uint32_t(sib), t.rb) : lane_at(g.oa.y2, t.lane, t.rb);   // (lane x bytes in 64 bits)
      middle_body(g.pl, t.W, y, nullptr, t.W, 1, row, t.Xr, t.rtid, t.rt);
    }
    else middle_body(g.pl, t.W, lane_at(g.oa.y, t.lane, t.rb), lane_at(g.oa.y2, t.lane, t.rb), t.W, int(mode), row, t.Xr, t.rtid, t.rt);
    __syncthreads();
  }
  if (again().oa.mode == 2) return;

  for (uint32_t T = t.cteam; T < t.NT; T += t.cteams) {
    const auto& g = again();
    BackExt x;
    if (EXT) {
      x.digits2 = lane_at(g.x.digits2, t.lane, t.rb); x.cbuf2 = lane_at(g.x.cbuf2, t.lane, t.cb);
      x.add_digits = lane_at(g.x.add_digits, t.lane, t.rb); x.add_cbuf = lane_at(g.x.add_cbuf, t.lane, t.cb);
    }
    back_body<EXT>(g.pl, t.W, lane_at(g.oa.dst, t.lane, t.rb), lane_at(g.oa.dst_cbuf, t.lane, t.cb), g.oa.a, x, T, t.Xc, t.ctid, t.ct, t.live);
    __syncthreads();   // the next trip refills the scratch that the carry chains of this one read
  }
}
struct OneLaunchAgain { __device__ __forceinline__ const OneLaunchPack& operator()() const { return args_again(); } };
template <bool EXT>
__global__ void __launch_bounds__(1024) k_onelaunch(OneLaunchPack) {
  LanePlace t;
  {
    const OneLaunchPack& g = args_again();
    t = lane_place(g.pl, g.oa.TL, g.oa.K);
  }
  product_phases<EXT>(t, OneLaunchAgain());
}
// the product by a sibling lane's image (product_phases SIB): an entry point of its own, k_onelaunch and k_batch keep their code
__global__ void __launch_bounds__(1024) k_onelaunch_sibling(OneLaunchPack) {
  LanePlace t;
  {
    const OneLaunchPack& g = args_again();
    t = lane_place(g.pl, g.oa.TL, g.oa.K);
  }
  product_phases<false, true>(t, OneLaunchAgain());
}

// ---------------------------------------------------------------------------------------------
// Batches: a queue of register operations of a one-launch engine in ONE launch.  A lane lives in one work-group for every
// operation (the shape is the plan's and the block's, lane_place), so no operation of a lane waits on another group: each group walks the
// descriptors in order for its own lanes, with a group barrier after every operation.
//   Memory.  Unlike k_onelaunch, an operation here reads digits, carry words and images that OTHER waves of the group stored a few
//   operations earlier in the same launch.  The barrier between operations is __syncthreads(), a workgroup-scope release / acquire (the
//   stores of every wave have completed and are visible to the group's loads behind it), never a bare s_barrier.  None of that data is
//   read through the scalar cache, which vector stores do not update: every such address depends on the thread index, and nothing here
//   declares it const __restrict__, read-only or non-temporal.  Plan tables and the descriptors do not change during the launch; the
//   descriptors are read as constant memory (scalar loads), anew in every phase like the argument block of k_onelaunch.
//   Carry buffers.  The host resolved every carry buffer when the operation was issued (engine.hip take_spare_cbuf / adopt_cbuf): a
//   product writes its new words to a spare buffer while carry_in_of reads the neighbouring runs' words of the old one, and the buffer
//   one operation releases may be the spare the next one writes.  That is safe because a lane never leaves its group and a barrier stands
//   between the two operations.
//   Barriers.  Every thread of a group walks every descriptor; kind and mode are the same for all of them.  A lane beyond the last one
//   (live == false) runs the products on the last lane's inputs for the barriers' sake, skips the other kinds, and stores nothing.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void linear_body(const DevPlan& pl, const LinArgs& la, uint32_t run);   // (with the run-wise kernels, below)
struct BatchPack { DevPlan pl; const BatchOp* ops; uint32_t count; };
__device__ __forceinline__ const BatchPack& batch_args_again() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const BatchPack*)p;
}
// descriptor i, read anew: constant for the launch, so constant address space (scalar loads), behind a pointer the compiler does not see through
__device__ __forceinline__ const BatchOp& batch_op_again(const BatchOp* ops, uint32_t i) {
  typedef const __attribute__((address_space(4))) BatchOp* ConstOp;
  ConstOp p = (ConstOp)(ops) + i;
  asm volatile("" : "+s"(p));
  return *(const BatchOp*)p;
}
struct ProductView { const DevPlan& pl; const OneLaunchArgs& oa; const BackExt& x; };
struct BatchAgain {   // plan and product i of the queue, for product_phases
  uint32_t i;
  __device__ __forceinline__ ProductView operator()() const {
    const BatchPack& g = batch_args_again();
    const BatchOp& op = batch_op_again(g.ops, i);
    return ProductView{g.pl, op.oa, op.x};
  }
};
__global__ void __launch_bounds__(1024) k_batch(BatchPack) {
  LanePlace t0;
  uint32_t live0;
  {
    const BatchPack& g = batch_args_again();
    const uint32_t TL = min(g.pl.m, g.pl.r5 == 5 ? 640u : 1024u);   // plan.hpp onelaunch_shape; K is what the block holds
    t0 = lane_place(g.pl, TL, blockDim.x / TL);
    live0 = t0.live;
  }
  // (the count, too, is read where it is needed: only i is held through an operation)
  for (uint32_t i = 0; i < batch_args_again().count; ++i) {
    // The thread's own numbers pass through an empty asm in every round: the lane masks of the conditions on them (thread below the tile
    // size, team below the tile count, live) are then worked out where they are used.  As loop invariants they were hoisted out of the
    // loop and held in scalar registers through all of it, six more than a wave has (spilled to a vector register).
    LanePlace t = t0;
    uint32_t live = live0;
    asm volatile("" : "+v"(t.lt), "+v"(t.cteam), "+v"(t.ctid), "+v"(t.rteam), "+v"(t.rtid), "+v"(live));
    t.live = live != 0;
    const uint32_t kind = batch_op_again(batch_args_again().ops, i).kind;
    if (kind == BatchOp::kProduct) {
      product_phases<true>(t, BatchAgain{i});
    } else if (kind == BatchOp::kLinear) {
      if (t.live) {
        const BatchPack& g = batch_args_again();
        const LinArgs& la = batch_op_again(g.ops, i).la;
        LinArgs l;
        l.a = lane_at(la.a, t.lane, t.rb); l.ca = lane_at(la.ca, t.lane, t.cb); l.b = lane_at(la.b, t.lane, t.rb); l.cb = lane_at(la.cb, t.lane, t.cb);
        l.s1 = lane_at(la.s1, t.lane, t.rb); l.cs1 = lane_at(la.cs1, t.lane, t.cb); l.s2 = lane_at(la.s2, t.lane, t.rb); l.cs2 = lane_at(la.cs2, t.lane, t.cb);
        l.d1 = lane_at(la.d1, t.lane, t.rb); l.cd1 = lane_at(la.cd1, t.lane, t.cb); l.d2 = lane_at(la.d2, t.lane, t.rb); l.cd2 = lane_at(la.cd2, t.lane, t.cb);
        for (uint32_t run = t.lt; run < t.M1 * t.NT; run += t.TL) linear_body(g.pl, l, run);
      }
    } else if (t.live) {   // kCopy: the register as it stands, 16 bytes a thread and trip, then its pending carry words
      const BatchOp& op = batch_op_again(batch_args_again().ops, i);
      const uint4* src = reinterpret_cast<const uint4*>(lane_at(op.la.a, t.lane, t.rb));
      uint4* dst = reinterpret_cast<uint4*>(lane_at(op.la.s1, t.lane, t.rb));
      for (uint32_t e = t.lt, ne = op.copy_bytes / 16; e < ne; e += t.TL) dst[e] = src[e];
      const uint64_t* csrc = lane_at(op.la.ca, t.lane, t.cb);
      uint64_t* cdst = lane_at(op.la.cs1, t.lane, t.cb);
      if (csrc) for (uint32_t run = t.lt; run < t.M1 * t.NT; run += t.TL) cdst[run] = csrc[run];
    }
    __syncthreads();   // the next operation reads what this one stored
  }
}

// ---------------------------------------------------------------------------------------------
// Columns too long for LDS: M1 = 5 L1 with 16 M1 bytes above a CU's 160 KiB -- n = 5 * 2^26, the largest entry of the reference's
// schedule (include/marin/engine_gpu.h:1624; forward80_0 ... there).  The radix-5 stage of the column transform runs on its own through a
// second work buffer U ([k0][i2][t]: 5 blocks x M2 columns x L1 pairs), one thread per (column, t) and C = 1; the power-of-two part of
// every block stays LDS-resident (L1 pairs x Cb columns).  Four sweeps instead of two around the row kernel: correct first, this size
// exists for exponents above 3.0e9.  (Never with lanes: plan.hpp refuses them at this size.)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_front_split_a(DevPlan pl, const uint32_t* __restrict__ digits, uint64_t* __restrict__ Uout) {
  const size_t e = size_t(blockIdx.x) * 256 + threadIdx.x;
  const uint32_t t = uint32_t(e & (pl.L1 - 1)), i2 = uint32_t(e >> pl.logL1), M1 = pl.M1;
  if (i2 >= pl.M2) return;
  const uint2* dg = reinterpret_cast<const uint2*>(digits) + size_t(i2) * M1;   // C = 1: tile i2 holds the column's M1 pairs
  const uint32_t sb = pl.SB[2 * i2];
  P2 x[5];
#pragma unroll
  for (int r = 0; r < 5; ++r) { const uint32_t i1 = pl.L1 * r + t; x[r] = weigh_pair(pl, i1, sb, dg[i1]); }
  dft5<false>(x, pl.W5c);
#pragma unroll
  for (int k = 1; k < 5; ++k) x[k] = p2_mul(x[k], pl.UT1[t * k]);
  P2* U = reinterpret_cast<P2*>(Uout);
#pragma unroll
  for (int k0 = 0; k0 < 5; ++k0) U[(size_t(k0) * pl.M2 + i2) * pl.L1 + t] = x[k0];
}
// block k0, columns Cb T .. Cb T + Cb - 1: L1-point transforms in LDS, four-step twiddle, rows k0 L1 + p of the work buffer
__global__ void __launch_bounds__(1024) k_front_split_b(DevPlan pl, const uint64_t* __restrict__ Uin, uint64_t* __restrict__ Wout, uint32_t logCb) {
  P2* X = reinterpret_cast<P2*>(smem_raw);
  const uint32_t tid = threadIdx.x, nthr = blockDim.x, Cb = 1u << logCb, per = pl.M2 >> logCb;
  const uint32_t k0 = blockIdx.x / per, T = blockIdx.x - k0 * per, tile = pl.L1 << logCb;
  const P2* U = reinterpret_cast<const P2*>(Uin);
  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t c = e >> pl.logL1, pp = e & (pl.L1 - 1);   // reads run along t: contiguous
    X[(pp << logCb) + c] = U[(size_t(k0) * pl.M2 + (T << logCb) + c) * pl.L1 + pp];
  }
  __syncthreads();
  if (pl.logL1) lds_pow2_dft<false>(X, pl.L1, pl.logL1, 1, Cb, logCb, pl.UT1, pl.M1, pl.r5, tid, nthr);
  P2* W = reinterpret_cast<P2*>(Wout);
  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t pp = e >> logCb, c = e & (Cb - 1), i2 = (T << logCb) + c, pos = k0 * pl.L1 + pp;
    W[size_t(pos) * pl.M2 + i2] = p2_mul(X[e], fourstep_word<false>(pl, pos, i2));
  }
}
__global__ void __launch_bounds__(1024) k_back_split_b(DevPlan pl, const uint64_t* __restrict__ Win, uint64_t* __restrict__ Uout, uint32_t logCb) {
  P2* X = reinterpret_cast<P2*>(smem_raw);
  const uint32_t tid = threadIdx.x, nthr = blockDim.x, Cb = 1u << logCb, per = pl.M2 >> logCb;
  const uint32_t k0 = blockIdx.x / per, T = blockIdx.x - k0 * per, tile = pl.L1 << logCb;
  const P2* W = reinterpret_cast<const P2*>(Win);
  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t pp = e >> logCb, c = e & (Cb - 1), i2 = (T << logCb) + c, pos = k0 * pl.L1 + pp;
    X[e] = p2_mul(W[size_t(pos) * pl.M2 + i2], fourstep_word<true>(pl, pos, i2));
  }
  __syncthreads();
  if (pl.logL1) lds_pow2_dft<true>(X, pl.L1, pl.logL1, 1, Cb, logCb, pl.UT1, pl.M1, pl.r5, tid, nthr);
  P2* U = reinterpret_cast<P2*>(Uout);
  for (uint32_t e = tid; e < tile; e += nthr) {
    const uint32_t c = e >> pl.logL1, pp = e & (pl.L1 - 1);
    U[(size_t(k0) * pl.M2 + (T << logCb) + c) * pl.L1 + pp] = X[(pp << logCb) + c];
  }
}
// inverse radix-5 stage, unweighting, x a and the carry inside every pair (runs of two digits: the engine follows with k_carry_fix and
// the local carry passes, as for every C = 1 plan)
__global__ void __launch_bounds__(256) k_back_split_a(DevPlan pl, const uint64_t* __restrict__ Uin, uint32_t* __restrict__ digits, uint64_t* __restrict__ cbuf,
                                                     uint32_t a) {
  const size_t e = size_t(blockIdx.x) * 256 + threadIdx.x;
  const uint32_t t = uint32_t(e & (pl.L1 - 1)), i2 = uint32_t(e >> pl.logL1), M1 = pl.M1;
  if (i2 >= pl.M2) return;
  const P2* U = reinterpret_cast<const P2*>(Uin);
  P2 x[5];
#pragma unroll
  for (int k0 = 0; k0 < 5; ++k0) x[k0] = U[(size_t(k0) * pl.M2 + i2) * pl.L1 + t];
#pragma unroll
  for (int k = 1; k < 5; ++k) x[k] = p2_mul(x[k], pl.UT1[(t * k) ? M1 - t * k : 0]);
  dft5<true>(x, pl.W5c);
  uint2* dg = reinterpret_cast<uint2*>(digits) + size_t(i2) * M1;
  const uint32_t sb = pl.SB[2 * i2];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const uint32_t i1 = pl.L1 * r + t;
    const RowUnweight uw = row_unweight(pl, i1);
    uint64_t carry = 0;
    uint32_t out[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      uint32_t width;
      const uint64_t u = unweigh(pl, uw, b, sb, b ? x[r].b : x[r].a, width);
      out[b] = adc_mul(u, a, 0u, width, carry);
    }
    dg[i1] = make_uint2(out[0], out[1]);
    cbuf[size_t(i2) * M1 + i1] = carry;
  }
}

// ---------------------------------------------------------------------------------------------
// run-wise kernels: one thread per run (T, i1) of 2C digits
// ---------------------------------------------------------------------------------------------
struct RunHead { uint32_t T, i1; size_t ci, off; };   // ci: index of the run's carry word; off: of its first digit
// run number `run` of a lane (as the sweep bodies take (tid, nthr): the caller says which); false beyond the last one
__device__ __forceinline__ bool run_head(const DevPlan& pl, RunHead& r, uint32_t run) {
  const uint32_t M1 = pl.M1;
  if (run >= M1 * (pl.M2 / pl.C)) return false;
  r.T = run / M1; r.i1 = run - r.T * M1;
  r.ci = size_t(r.T) * M1 + r.i1; r.off = r.ci * pl.C * 2;
  return true;
}
// the run-wise kernels' own: one thread per run
__device__ __forceinline__ bool run_head(const DevPlan& pl, RunHead& r) { return run_head(pl, r, blockIdx.x * blockDim.x + threadIdx.x); }

// a, b (+ their pending carry words) -> sum and / or difference, each written to up to two
// registers, with the run's carry-out word left pending (kernels.hpp LinArgs).  The difference is a - b + 2 Mp
// digit by digit (neg2_mp4, marin.cl:246-256), so nothing goes negative: digits are below 2^width + a small excess.
__device__ __forceinline__ void linear_body(const DevPlan& pl, const LinArgs& la, uint32_t run) {
  RunHead r;
  if (!run_head(pl, r, run)) return;
  const uint32_t C = pl.C, sa = pl.SA[r.i1];
  const size_t off = r.off;
  uint64_t ca = la.ca ? carry_in_of(pl, la.ca, r.T, r.i1) : 0, cb = la.cb ? carry_in_of(pl, la.cb, r.T, r.i1) : 0;
  uint64_t cs = 0, cd = 0;
  const bool want_s = la.s1 != nullptr, want_d = la.d1 != nullptr;
  for (uint32_t k = 0; k < 2 * C; ++k) {
    uint32_t width; bool wrap;
    digit_info(pl, sa, pl.SB[2 * (r.T * C) + k], width, wrap);
    const uint64_t mask = (uint64_t(1) << width) - 1;
    const uint64_t av = take_carry_in(la.a[off + k], ca, k, 2 * C, width), bv = take_carry_in(la.b[off + k], cb, k, 2 * C, width);
    if (want_s) {
      const uint64_t v = av + bv + cs;
      const uint32_t o = uint32_t(v & mask);
      cs = v >> width;
      la.s1[off + k] = o;
      if (la.s2) la.s2[off + k] = o;
    }
    if (want_d) {
      const uint64_t v = av + (4 * mask - bv) + cd;   // b's digit may exceed its width by a carry remainder: 4 Mp keeps it positive
      const uint32_t o = uint32_t(v & mask);
      cd = v >> width;
      la.d1[off + k] = o;
      if (la.d2) la.d2[off + k] = o;
    }
  }
  if (want_s) { la.cs1[r.ci] = cs; if (la.s2) la.cs2[r.ci] = cs; }
  if (want_d) { la.cd1[r.ci] = cd; if (la.d2) la.cd2[r.ci] = cd; }
}
template <bool LANES>
__global__ void __launch_bounds__(256) k_linear(DevPlan pl, LinArgs la) {
  LinArgs l;
  l.a = lane_reg<LANES>(pl, la.a); l.ca = lane_cbuf<LANES>(pl, la.ca); l.b = lane_reg<LANES>(pl, la.b); l.cb = lane_cbuf<LANES>(pl, la.cb);
  l.s1 = lane_reg<LANES>(pl, la.s1); l.cs1 = lane_cbuf<LANES>(pl, la.cs1); l.s2 = lane_reg<LANES>(pl, la.s2); l.cs2 = lane_cbuf<LANES>(pl, la.cs2);
  l.d1 = lane_reg<LANES>(pl, la.d1); l.cd1 = lane_cbuf<LANES>(pl, la.cd1); l.d2 = lane_reg<LANES>(pl, la.d2); l.cd2 = lane_cbuf<LANES>(pl, la.cd2);
  linear_body(pl, l, blockIdx.x * blockDim.x + threadIdx.x);
}

// x a for the factors above the plan's fused bound (plan.hpp fused_factor_limit; Engine::scale): the run's digits with their pending
// carry-in taken as k_linear takes them, times a with a carry through the run, whose carry-out word is left pending.  Digit outputs may
// alias the input, cout must not alias cin.
// Bounds: a digit after the carry-in is below 2^31 (fused_factor_ok), so digit a + carry < 2^63 + 2^(64 - q).
__device__ __forceinline__ void scale_body(const DevPlan& pl, const uint32_t* in, const uint64_t* cin, uint32_t* out, uint64_t* cout, uint32_t a) {
  RunHead r;
  if (!run_head(pl, r)) return;
  const uint32_t C = pl.C, sa = pl.SA[r.i1];
  uint64_t ci = cin ? carry_in_of(pl, cin, r.T, r.i1) : 0, c = 0;
  for (uint32_t k = 0; k < 2 * C; ++k) {
    uint32_t width; bool wrap;
    digit_info(pl, sa, pl.SB[2 * (r.T * C) + k], width, wrap);
    const uint64_t v = take_carry_in(in[r.off + k], ci, k, 2 * C, width) * a + c;
    out[r.off + k] = uint32_t(v & ((uint64_t(1) << width) - 1));
    c = v >> width;
  }
  cout[r.ci] = c;
}
template <bool LANES>
__global__ void __launch_bounds__(256) k_scale(DevPlan pl, const uint32_t* __restrict__ in, const uint64_t* __restrict__ cin,
                                               uint32_t* __restrict__ out, uint64_t* __restrict__ cout, uint32_t a) {
  scale_body(pl, lane_reg<LANES>(pl, in), lane_cbuf<LANES>(pl, cin), lane_reg<LANES>(pl, out), lane_cbuf<LANES>(pl, cout), a);
}

// carry fix: weak carry (the remainder, if any, stays on the run's last digit: same contract as adc4, marin.cl:203-212); a loop of its
// own, which ends as soon as no carry is left
__device__ __forceinline__ void carry_fix_body(const DevPlan& pl, uint32_t* digits, const uint64_t* cbuf) {
  RunHead r;
  if (!run_head(pl, r)) return;
  const uint32_t C = pl.C;
  uint64_t cin = carry_in_of(pl, cbuf, r.T, r.i1);
  if (cin == 0) return;
  uint32_t* d = digits + r.off;
  const uint32_t sa = pl.SA[r.i1];   // after the early exit
  for (uint32_t k = 0; k < 2 * C; ++k) {
    if (k == 2 * C - 1) { d[k] += uint32_t(cin); break; }
    uint32_t width; bool wrap;
    digit_info(pl, sa, pl.SB[2 * (r.T * C) + k], width, wrap);
    const uint64_t v = uint64_t(d[k]) + cin;
    d[k] = uint32_t(v & ((uint64_t(1) << width) - 1));
    cin = v >> width;
    if (cin == 0) break;
  }
}
template <bool LANES>
__global__ void __launch_bounds__(256) k_carry_fix(DevPlan pl, uint32_t* __restrict__ digits, const uint64_t* __restrict__ cbuf) {
  carry_fix_body(pl, lane_reg<LANES>(pl, digits), lane_cbuf<LANES>(pl, cbuf));
}


// digit j -> memory slot (Plan::pos)
__device__ __forceinline__ size_t slot_of(const DevPlan& pl, uint32_t j) {
  const uint32_t i = j >> 1, b = j & 1;
  const uint32_t i1 = i / pl.M2, i2 = i - i1 * pl.M2;
  const uint32_t T = i2 / pl.C, c = i2 - T * pl.C;
  return ((size_t(T) * pl.M1 + i1) * pl.C + c) * 2 + b;
}

// x <- x - a with borrow, one thread (marin.cl:2376-2393)
__device__ __forceinline__ void sub_small_body(const DevPlan& pl, uint32_t* digits, uint32_t a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t borrow = a;
  for (int lap = 0; lap < 3 && borrow; ++lap) {
    for (uint32_t j = 0; j < pl.n && borrow; ++j) {
      const uint32_t i = j >> 1, i1 = i / pl.M2, i2 = i - i1 * pl.M2;
      uint32_t width; bool wrap;
      digit_info(pl, pl.SA[i1], pl.SB[2 * i2 + (j & 1)], width, wrap);
      const size_t s = slot_of(pl, j);
      const uint64_t dv = digits[s];
      if (dv >= borrow) { digits[s] = uint32_t(dv - borrow); borrow = 0; }
      else {
        // borrow k units of 2^width: smallest k with dv + k*2^width >= borrow
        const uint64_t need = borrow - dv;
        const uint64_t k = (need + (uint64_t(1) << width) - 1) >> width;
        digits[s] = uint32_t(dv + (k << width) - borrow);
        borrow = k;
      }
    }
  }
}
template <bool LANES>
__global__ void k_sub_small(DevPlan pl, uint32_t* __restrict__ digits, uint32_t a) { sub_small_body(pl, lane_reg<LANES>(pl, digits), a); }

// ------------------------------- launch wrappers ---------------------------------------------


static inline uint32_t block_for(size_t work) {
  size_t b = 64;
  while (b < 512 && b < work) b <<= 1;
  return uint32_t(b);
}

// work-group size for a tile of `pairs` pairs: a quarter of it (one radix-4 butterfly per thread and pass), or half of it when the whole
// launch has no more work-groups than the chip has CUs (latency-bound: one plane per thread, lds_pow2_passes)
static inline uint32_t block_for_small(const DevPlan& pl, size_t pairs) {
  const size_t groups = pl.lanes * (size_t(pl.M1) * pl.M2 / (pairs ? pairs : 1));   // of the whole launch: a lane engine's launch has `lanes` times the tiles
  // at most one work-group per CU (with two per CU the classic form wins: n = 2^21, 0.066 vs 0.073 ms; profiles/r02_ab_small_tiles.txt)
  if (groups > 256) return block_for(pairs / 4 ? pairs / 4 : 1);
  // one pair per thread in the element-wise loops where the tile allows (C2: 0.0331 -> 0.0318 ms), else one plane per thread
  size_t b = 64;
  while (b < 1024 && b < pairs) b <<= 1;
  return uint32_t(b);
}

// every launch: its grid without lanes in x, the lanes in y
hipError_t launch_front(const DevPlan& pl, const uint32_t* digits, const uint64_t* cbuf_in, uint64_t* W, hipStream_t s) {
  const size_t tile = size_t(pl.M1) * pl.C;
  hipLaunchKernelGGL(pl.lanes > 1 ? k_front<true> : k_front<false>, dim3(pl.M2 / pl.C, pl.lanes), dim3(block_for_small(pl, tile)), tile * 16, s, pl, digits, cbuf_in, W);
  return hipGetLastError();
}
hipError_t launch_middle(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s) {
  if (mode < 0 || mode > 4) return hipErrorInvalidValue;
  const dim3 grid(pl.M1, pl.lanes), block(block_for_small(pl, pl.M2));
  if (mode == 4) hipLaunchKernelGGL(pl.lanes > 1 ? k_middle_keep<true> : k_middle_keep<false>, grid, block, size_t(pl.M2) * 16, s, pl, Win, Wimg, Wout);
  else hipLaunchKernelGGL(pl.lanes > 1 ? k_middle<true> : k_middle<false>, grid, block, size_t(pl.M2) * 16, s, pl, Win, Y, Y2, Wout, mode);
  return hipGetLastError();
}
// the row sweep of a product by a sibling lane's image (k_middle_sibling): lane engines only, grid and block of launch_middle
hipError_t launch_middle_sibling(const DevPlan& pl, const uint64_t* Win, const uint64_t* Ysrc, const uint64_t* Yalt, uint64_t* Wout, uint32_t level, hipStream_t s) {
  if (pl.lanes < 2 || level > 31 || !Ysrc || !Yalt) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_middle_sibling, dim3(pl.M1, pl.lanes), dim3(block_for_small(pl, pl.M2)), size_t(pl.M2) * 16, s, pl, Win, Ysrc, Yalt, Wout, level);
  return hipGetLastError();
}
template <bool EXT>
static hipError_t launch_back_of(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& x, hipStream_t s) {
  const size_t tile = size_t(pl.M1) * pl.C;
  hipLaunchKernelGGL((pl.lanes > 1 ? k_back<EXT, true> : k_back<EXT, false>), dim3(pl.M2 / pl.C, pl.lanes), dim3(block_for_small(pl, tile)), tile * 16, s, pl, W, digits, cbuf, a, x);
  return hipGetLastError();
}
hipError_t launch_back(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s) {
  return launch_back_of<false>(pl, W, digits, cbuf, a, BackExt(), s);
}
hipError_t launch_back_ext(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& x, hipStream_t s) {
  return launch_back_of<true>(pl, W, digits, cbuf, a, x, s);
}
// one-launch products: `groups` work-groups of K lanes x TL threads, per lane 2 m pairs of LDS (plan.hpp onelaunch_shape)
constexpr size_t kOneLaunchMaxLds = 128 * 1024;   // n = 8192: 4096 pairs of work buffer and as much scratch
hipError_t launch_onelaunch(const DevPlan& pl, const OneLaunchArgs& oa, const BackExt& x, hipStream_t s) {
  const size_t lds = size_t(oa.K) * pl.m * 32;
  if (oa.mode < 0 || oa.mode > kModeSibling || !oa.TL || !oa.K || oa.K * oa.TL > 1024 || lds > kOneLaunchMaxLds || size_t(oa.groups) * oa.K < pl.lanes) return hipErrorInvalidValue;
  if (oa.mode == kModeSibling) {   // no extras, both images, a level that keeps the sibling's lane below 2^32
    if (x.any() || !oa.y || !oa.y2 || oa.level > 31) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_onelaunch_sibling, dim3(oa.groups), dim3(oa.K * oa.TL), lds, s, OneLaunchPack{pl, oa, x});
    return hipGetLastError();
  }
  hipLaunchKernelGGL(x.any() ? k_onelaunch<true> : k_onelaunch<false>, dim3(oa.groups), dim3(oa.K * oa.TL), lds, s, OneLaunchPack{pl, oa, x});
  return hipGetLastError();
}
// a batch: `count` descriptors in device memory, the grid, block and LDS of the one-launch products
hipError_t launch_batch(const DevPlan& pl, const BatchOp* ops, uint32_t count, uint32_t TL, uint32_t K, uint32_t groups, hipStream_t s) {
  const size_t lds = size_t(K) * pl.m * 32;
  const uint32_t cap = pl.r5 == 5 ? 640u : 1024u;   // the kernel takes TL from the plan (plan.hpp onelaunch_shape) and K from the block
  if (!ops || !count || !TL || !K || K * TL > 1024 || lds > kOneLaunchMaxLds || size_t(groups) * K < pl.lanes || TL != (pl.m < cap ? pl.m : cap))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_batch, dim3(groups), dim3(K * TL), lds, s, BatchPack{pl, ops, count});
  return hipGetLastError();
}
// the split column sweeps (M1 = 5 L1 beyond LDS): U is a second work buffer of 8 n bytes
static uint32_t split_log_cb(const DevPlan& pl) { uint32_t l = 0; while ((size_t(pl.L1) << (l + 1)) * 16 <= size_t(128) * 1024 && (2u << l) <= pl.M2 && l < 2) ++l; return l; }
hipError_t launch_front_split(const DevPlan& pl, const uint32_t* digits, uint64_t* U, uint64_t* W, hipStream_t s) {
  const size_t threads = size_t(pl.M2) * pl.L1;
  hipLaunchKernelGGL(k_front_split_a, dim3(uint32_t((threads + 255) / 256)), dim3(256), 0, s, pl, digits, U);
  const uint32_t lcb = split_log_cb(pl);
  const size_t tile = size_t(pl.L1) << lcb;
  hipLaunchKernelGGL(k_front_split_b, dim3(5 * (pl.M2 >> lcb)), dim3(block_for(tile / 4 ? tile / 4 : 1)), tile * 16, s, pl, U, W, lcb);
  return hipGetLastError();
}
hipError_t launch_back_split(const DevPlan& pl, const uint64_t* W, uint64_t* U, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s) {
  const uint32_t lcb = split_log_cb(pl);
  const size_t tile = size_t(pl.L1) << lcb;
  hipLaunchKernelGGL(k_back_split_b, dim3(5 * (pl.M2 >> lcb)), dim3(block_for(tile / 4 ? tile / 4 : 1)), tile * 16, s, pl, W, U, lcb);
  const size_t threads = size_t(pl.M2) * pl.L1;
  hipLaunchKernelGGL(k_back_split_a, dim3(uint32_t((threads + 255) / 256)), dim3(256), 0, s, pl, U, digits, cbuf, a);
  return hipGetLastError();
}
hipError_t configure_split(const DevPlan& pl) {
  const size_t bytes = (size_t(pl.L1) << split_log_cb(pl)) * 16;
  if (bytes <= 48 * 1024) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_front_split_b), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_back_split_b), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
}
// the run-wise launches: 256 runs a work-group
static dim3 run_grid(const DevPlan& pl) { return dim3(uint32_t((size_t(pl.M1) * (pl.M2 / pl.C) + 255) / 256), pl.lanes); }
hipError_t launch_linear(const DevPlan& pl, const LinArgs& la, hipStream_t s) {
  hipLaunchKernelGGL(pl.lanes > 1 ? k_linear<true> : k_linear<false>, run_grid(pl), dim3(256), 0, s, pl, la);
  return hipGetLastError();
}
hipError_t launch_scale(const DevPlan& pl, const uint32_t* in, const uint64_t* cin, uint32_t* out, uint64_t* cout, uint32_t a, hipStream_t s) {
  hipLaunchKernelGGL(pl.lanes > 1 ? k_scale<true> : k_scale<false>, run_grid(pl), dim3(256), 0, s, pl, in, cin, out, cout, a);
  return hipGetLastError();
}
hipError_t launch_carry_fix(const DevPlan& pl, uint32_t* digits, const uint64_t* cbuf, hipStream_t s) {
  hipLaunchKernelGGL(pl.lanes > 1 ? k_carry_fix<true> : k_carry_fix<false>, run_grid(pl), dim3(256), 0, s, pl, digits, cbuf);
  return hipGetLastError();
}
hipError_t launch_sub_small(const DevPlan& pl, uint32_t* digits, uint32_t a, hipStream_t s) {
  hipLaunchKernelGGL(pl.lanes > 1 ? k_sub_small<true> : k_sub_small<false>, dim3(1, pl.lanes), dim3(64), 0, s, pl, digits, a);
  return hipGetLastError();
}
// the dynamic-LDS attribute of the five tile kernels: of the instantiations without lanes for every engine (as before there were lanes),
// of those with lanes for an engine that has them
template <bool LANES>
static hipError_t configure_kernels_of(size_t lds_front, size_t lds_mid) {
  const struct { const void* fn; size_t lds; } ks[5] = {
      {reinterpret_cast<const void*>(k_front<LANES>), lds_front}, {reinterpret_cast<const void*>(k_back<false, LANES>), lds_front},
      {reinterpret_cast<const void*>(k_back<true, LANES>), lds_front}, {reinterpret_cast<const void*>(k_middle<LANES>), lds_mid},
      {reinterpret_cast<const void*>(k_middle_keep<LANES>), lds_mid}};
  for (const auto& k : ks)
    if (k.lds > 48 * 1024) {
      hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(k.lds));
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}
// The one-launch entry points get the LDS of their largest size whatever the engine's own: the value is the same for every engine, so
// engines of different sizes in one process never lower it for one another.
hipError_t configure_kernels(size_t lds_front, size_t lds_mid, uint32_t lanes, bool onelaunch) {
  hipError_t e = configure_kernels_of<false>(lds_front, lds_mid);
  if (e == hipSuccess && lanes > 1) e = configure_kernels_of<true>(lds_front, lds_mid);
  if (e == hipSuccess && onelaunch) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_onelaunch<false>), hipFuncAttributeMaxDynamicSharedMemorySize, int(kOneLaunchMaxLds));
  if (e == hipSuccess && onelaunch) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_onelaunch<true>), hipFuncAttributeMaxDynamicSharedMemorySize, int(kOneLaunchMaxLds));
  if (e == hipSuccess && onelaunch) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch), hipFuncAttributeMaxDynamicSharedMemorySize, int(kOneLaunchMaxLds));
  if (e == hipSuccess && onelaunch && lanes > 1) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_onelaunch_sibling), hipFuncAttributeMaxDynamicSharedMemorySize, int(kOneLaunchMaxLds));
  if (e == hipSuccess && lanes > 1 && lds_mid > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_middle_sibling), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_mid));
  return e;
}

}  // namespace mi355
