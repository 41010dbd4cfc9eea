// The pieces of the fused unweight + Garner + carry sweep of the paired-NTT squaring over GF(M61^2) x GF(M31^2), each
// written once for every kernel of crt_kernels.hip that needs it.  Reference: third_party/aevum/src/cl/carry.cl:506-588 (FFT3161 `carry`)
// with weightAndCarryPair, carryutil.cl:440-470 ("n3161 = n61 * M31 + n31"); CPU form docs/mersenne2_mixed_crt_2d_half_fast/
// mersenne2_mixed_crt_2d_half_fast.cpp:429-441,931-1001.  A sweep takes the two residues of every (still weighted, already scaled)
// convolution coefficient in logical digit order and leaves digits in base 2^width (widths up to 39 bits: u64).  One thread owns a run of
// kRun consecutive digits: sequential carry inside the run, then the carry of the run before it goes through the run's own digits and what
// is left (0 or a unit) in front of the following run, without further propagation (weak carry).  ~60 VALU instructions per word (two
// rotations, one M61 multiply, 128-bit carry arithmetic).  Device only; included by crt_kernels.hip.
#pragma once
#include "crt_arith.hpp"
#include "crt_kernels.hpp"

namespace mi355 {
namespace crt {

typedef unsigned __int128 u128;

// sum -> its low `width` bits, the rest to carry
__device__ __forceinline__ uint64_t cut(u128 sum, uint32_t width, u128& carry) {
  carry = sum >> width;
  return uint64_t(sum) & ((uint64_t(1) << width) - 1);
}

// One digit: unweight the residues (r61, r31) of the coefficient at dw, Garner, times a, add the carry, cut to the digit's width; dw moves on.
__device__ __forceinline__ uint64_t carry_digit(const Geom& g, DigitWalk& dw, uint64_t r61, uint32_t r31, uint32_t& width, u128& carry) {
  const uint64_t x61 = rot61(r61, dw.unweight61());
  const uint32_t x31 = rot31(r31, dw.unweight31());
  // Garner: v = x31 + M31 * ((x61 - x31) / M31 mod M61)  <  M61 * M31
  const uint64_t d = x61 >= x31 ? x61 - x31 : x61 + M61 - x31;
  const uint64_t t = mul61(d, g.inv31);
  const u128 v = ((u128)t << 31) - t + x31;
  width = dw.width(g);
  dw.next(g);
  return cut(v * g.a + carry, width, carry);
}

// `carry` through the digits of the run at j0 (in memory), until it is gone -- a 92-bit carry is after three digits -- or the run ends;
// returns what is left after the last digit
__device__ __forceinline__ uint64_t carry_through(const Geom& g, uint64_t* __restrict__ digits, uint32_t j0, u128 carry) {
  DigitWalk dw; dw.start(g, j0);
  for (int k = 0; k < kRun; ++k) {
    digits[j0 + k] = cut((u128)digits[j0 + k] + carry, dw.width(g), carry);
    if (carry == 0) break;
    dw.next(g);
  }
  return uint64_t(carry);
}

// Hand-over between the 256 runs of a work-group (all threads call it; two barriers): the carry leaving each run goes through the digits
// out[] (widths wd[]) of the run after it, what is left of it in front of the run after that one.  first: this run has no predecessor in
// the work-group.  Returns the leftover of this run's own pass, which (with `carry`) is what a last run hands to the next work-group.
struct RunLink { uint64_t lo[256], hi[256], left[256]; };
__device__ __forceinline__ uint64_t link_runs(RunLink& L, uint64_t (&out)[kRun], const uint32_t (&wd)[kRun], u128 carry, bool live, bool first) {
  const uint32_t tid = threadIdx.x;
  L.lo[tid] = uint64_t(carry); L.hi[tid] = uint64_t(carry >> 64);
  __syncthreads();
  u128 in = first ? 0 : (((u128)L.hi[tid - 1] << 64) | L.lo[tid - 1]);
  if (live) {
#pragma unroll
    for (int k = 0; k < kRun; ++k) out[k] = cut((u128)out[k] + in, wd[k], in);
  }
  L.left[tid] = uint64_t(in);
  __syncthreads();
  if (live && !first) out[0] += L.left[tid - 1];
  return uint64_t(in);
}
__device__ __forceinline__ void store_run(uint64_t* __restrict__ digits, uint32_t j0, const uint64_t (&out)[kRun]) {
  ulonglong2* po = reinterpret_cast<ulonglong2*>(digits + j0);
#pragma unroll
  for (int k = 0; k < kRun / 2; ++k) po[k] = make_ulonglong2(out[2 * k], out[2 * k + 1]);
}
// edge words of a chain of runs: the 128-bit carry and the leftover of its last run
__device__ __forceinline__ void store_edge(uint64_t* __restrict__ e, u128 carry, uint64_t left) { e[0] = uint64_t(carry); e[1] = uint64_t(carry >> 64); e[2] = left; }

// First run (at j0) of a chain: the carry of the chain before it in digit order (edge words prev[0 .. 2]) runs through its digits, the
// leftovers go in front of this run and of the next one (at jnext) without further propagation
__device__ __forceinline__ void fold_edge(const Geom& g, uint64_t* __restrict__ digits, const uint64_t* __restrict__ prev, uint32_t j0, uint32_t jnext) {
  const uint64_t left = carry_through(g, digits, j0, ((u128)prev[1] << 64) | prev[0]);
  digits[j0] += prev[2];
  if (left) digits[jnext] += left;
}

// Inverse odd axis of slot s, 1 / (odd h), spilled to the LDS planes [2 row + (re: even position, im: odd position)][thread]
template <int ODD>
__device__ __forceinline__ void back_to_planes(const Grid& gr, const F61::C* __restrict__ Z61, const F31::C* __restrict__ Z31, uint32_t s,
                                               uint64_t (&S61)[2 * ODD][256], uint32_t (&S31)[2 * ODD][256]) {
  const uint32_t tid = threadIdx.x;
  F61::C in61[ODD]; F31::C in31[ODD];
#pragma unroll
  for (int k = 0; k < ODD; ++k) { in61[k] = Z61[size_t(k) * gr.h + s]; in31[k] = Z31[size_t(k) * gr.h + s]; }
  dft_odd<F61, ODD>(in61, gr.r61i, F61::neg(gr.c3_61));
  dft_odd<F31, ODD>(in31, gr.r31i, F31::neg(gr.c3_31));
#pragma unroll
  for (int k = 0; k < ODD; ++k) {
    const F61::C o61 = cscale<F61>(in61[k], gr.s61); const F31::C o31 = cscale<F31>(in31[k], gr.s31);
    S61[2 * k][tid] = o61.re; S61[2 * k + 1][tid] = o61.im; S31[2 * k][tid] = o31.re; S31[2 * k + 1][tid] = o31.im;
  }
}

}  // namespace crt
}  // namespace mi355
