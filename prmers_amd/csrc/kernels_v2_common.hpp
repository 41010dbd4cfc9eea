// Shared pieces of the register-resident kernel sets (kernels_v2.hip: radix-8 rows and columns; kernels_v5.hip: radix-5 columns): pair type,
// LDS exchange templates, the wave-index-specialised shift seams, the run head and carry tail of the column sweeps, table lookups, barrier
// and probe helpers (the radix-4 set, kernels_v3.hip, takes its element arithmetic, run head and carry tail from here too).  Two translation units because the
// two sets want different instruction schedulers (Makefile: kernels_v2.hip is built with -amdgpu-sched-strategy=iterative-maxocc, -1 % at
// C3 and -1.7 % at n = 2^24 in a same-box A/B; the radix-5 kernels lose 0.8 % with it and 40 % with max-ilp: profiles/r03_ab_sched_strategies.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gfdft.hpp"
#include "kernels.hpp"

namespace mi355 {
namespace v2 {

struct alignas(16) P2 { uint64_t a, b; };

// LDS slot of tile element i (16-byte slots).  The exchanges write and read the tile in three lane orders -- thread-major (slot 8 t + r),
// strided / wave-major (consecutive lanes on consecutive slots) and the column kernels' (k1 | k2 | c) order -- and a 128-bit access is served
// in fixed lane groups: stores in eight groups of 8 contiguous lanes on 32 banks, loads in four NON-contiguous groups of 16 lanes
// ({0-3, 12-15, 20-27}, ...) on 64 banks (MI355X_MICROARCH.md, LDS).  Round 4: i ^ ((i >> 3) & 15) is conflict-free for every one of the
// row kernel's six orders (census: tools/lds_census.py; the round-1 skew i + i / 8 left the consecutive-lane loads 2-way conflicted -- the 18 %
// of SQ_LDS_BANK_CONFLICT over SQ_LDS_IDX_ACTIVE that VERDICT r03 lists) and needs no padding: 64 KiB instead of 72 per group.
// The old skew lost to this map in a same-box A/B at C3, C4 and five other sizes (profiles/r04_ab_lds_map.txt).
__device__ __forceinline__ uint32_t phys(uint32_t i) { return i ^ ((i >> 3) & 15u); }
constexpr uint32_t kLdsSlots = 4096;
constexpr uint32_t kLdsBytes = kLdsSlots * 16;

// Work-buffer accesses of the sweeps: plain loads and stores.  The non-temporal hint on them was 3.5-4.5 % slower at C3 and up to 60 %
// at n = 2^24, where non-temporal stores keep the L2 from merging the tiles' pieces of a line (profiles/r04_ab_nontemporal.txt).
__device__ __forceinline__ void w_store(P2* p, P2 v) { *p = v; }
__device__ __forceinline__ P2 w_load(const P2* p) { return *p; }

__device__ __forceinline__ P2 p2_mul(P2 x, uint64_t w) { return {gf::mul(x.a, w), gf::mul(x.b, w)}; }

template <bool INV, int LAZY = 0>
__device__ __forceinline__ void dft8p(P2 (&x)[8]) {
  uint64_t u[8], v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { u[j] = x[j].a; v[j] = x[j].b; }
  gf::dft8<INV, LAZY>(u);
  gf::dft8<INV, LAZY>(v);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = {u[j], v[j]};
}

// The same steps on one plane per thread (element uint64_t): kernels written once for both lane forms call these overloads.
template <bool INV, int LAZY = 0>
__device__ __forceinline__ void dft8p(uint64_t (&x)[8]) { gf::dft8<INV, LAZY>(x); }
__device__ __forceinline__ P2 mulw(P2 x, uint64_t w) { return p2_mul(x, w); }
__device__ __forceinline__ uint64_t mulw(uint64_t x, uint64_t w) { return gf::mul(x, w); }
__device__ __forceinline__ P2 shiftw(P2 x, unsigned s) { return {gf::mul_pow2(x.a, s), gf::mul_pow2(x.b, s)}; }
__device__ __forceinline__ uint64_t shiftw(uint64_t x, unsigned s) { return gf::mul_pow2(x, s); }
__device__ __forceinline__ P2 foldw(P2 x) { return {gf::fold(x.a), gf::fold(x.b)}; }
__device__ __forceinline__ uint64_t foldw(uint64_t x) { return gf::fold(x); }

// Seams inside a 64-point block: x[k] *= omega_64^(k w) = 2^(39 k w) with w uniform over the wavefront.
// The wave index is made a template parameter: every shift amount is then a compile-time constant and
// mul_pow2 collapses to its 8-11 instruction cases (a general multiply by a scalar-built power of two,
// the previous form, is 24).  The caller switches on the scalar wave index once per seam and each wave
// runs only its own copy (code grows by ~1 KB per copy; measured -5 % on the row kernel, -4 % on the
// column kernels).
// LB = 6: the eight registers are one block member each.  LB = 5 (32-point blocks, rows of 2048: omega_32 = 2^78): registers 4 g + k1', two
// groups g of four (two rows of a tile, or the two planes of a row), x[4 g + k1'] *= omega_32^(+-k1' w).
// FOLD0: the caller left x[1..3] and x[5] un-folded (dft8 LAZY = 1) because the shifts accept any operand; wave 0
// shifts by nothing, so it folds them here instead.
template <int LB, int W, bool INV, bool FOLD0, class E>
__device__ __forceinline__ void seam_const(E (&x)[8]) {
  static_assert(LB == 6 || (LB == 5 && !FOLD0), "64-point blocks, or 32-point blocks after a canonical radix-4");
  if constexpr (W == 0) {
    if (FOLD0) { x[1] = foldw(x[1]); x[2] = foldw(x[2]); x[3] = foldw(x[3]); x[5] = foldw(x[5]); }
  } else {
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      constexpr int R1 = 1 << (LB - 3);   // registers per block
      if ((k & (R1 - 1)) == 0) continue;
      const unsigned f = ((64u >> LB) * gf::LOG2_W64 * unsigned(k & (R1 - 1)) * unsigned(W)) % 192u;
      x[k] = shiftw(x[k], INV ? (192u - f) % 192u : f);
    }
  }
}

#define MI355_SWITCH8(w, CALL) \
  switch (w) {                 \
    case 0: CALL(0); break;    \
    case 1: CALL(1); break;    \
    case 2: CALL(2); break;    \
    case 3: CALL(3); break;    \
    case 4: CALL(4); break;    \
    case 5: CALL(5); break;    \
    case 6: CALL(6); break;    \
    default: CALL(7); break;   \
  }

template <int LB, bool INV, bool FOLD0 = false, class E>
__device__ __forceinline__ void seam(E (&x)[8], uint32_t wave) {
#define MI355_CALL(W) seam_const<LB, W, INV, FOLD0>(x)
  MI355_SWITCH8(wave, MI355_CALL)
#undef MI355_CALL
}

// omega_m^e from the two-level table (e < m)
__device__ __forceinline__ uint64_t tw_lookup(const DevPlan& pl, uint64_t e) {
  const uint64_t lo = pl.TWlo[e & ((1u << pl.twh) - 1)], hi = pl.TWhi[e >> pl.twh];
  return gf::mul(lo, hi);
}

extern __shared__ __attribute__((aligned(16))) unsigned char smem_v2[];

// block -> tile for the back sweep: blocks that share an XCD (b, b+8, ... under round-robin dispatch)
// get neighbouring tiles, so the two 64-byte halves of a 128-byte work-buffer line meet in one L2
// (speed only; measured 73 -> 66 us at C3).  MI355_TUNE bit 0 switches it off.
__device__ __forceinline__ uint32_t tile_of_block(const DevPlan& pl, uint32_t b, uint32_t nblocks) {
  if (!(pl.tune & 1) && (nblocks % 8 == 0)) return (b & 7) * (nblocks >> 3) + (b >> 3);
  return b;
}
// Issue-priority boost for the work-groups of the last half round.  Two work-groups share a CU and the older
// one wins the issue arbitration, so at the end of a launch every CU is left with one late-started group
// running alone at ~3/4 of the pair rate.  Raising the priority of exactly those late
// groups (block index >= boost_from, set by the engine from the grid size and the CU count) lets them overtake
// their older neighbour, and the two finish closer together: -3 % per squaring at C3 (same-box A/B).
__device__ __forceinline__ void boost_if_late(uint32_t boost_from) {
  if (blockIdx.x >= boost_from) __builtin_amdgcn_s_setprio(3);
}

// Barrier for LDS exchanges: waits for this wave's LDS operations only.  __syncthreads() also drains the vector-memory
// counter (it carries a work-group fence), which makes every wave wait at the barrier for table words that were
// requested on purpose before the exchange; global data is not exchanged between waves inside these kernels.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#if defined(MI355_PROBE)
// timeline probe: thread 0 of every work-group records {realtime0, realtime1, shader clock0, clock1, HW_ID, XCC_ID, mid realtime}
#define PROBE_BEGIN(pl)                                                                             \
  uint64_t pb_r0_ = 0, pb_c0_ = 0, pb_rm_ = 0;                                                      \
  if (pl.probe) { pb_r0_ = __builtin_amdgcn_s_memrealtime(); pb_c0_ = __builtin_amdgcn_s_memtime(); }
#define PROBE_MID(pl) if (pl.probe) pb_rm_ = __builtin_amdgcn_s_memrealtime();
#define PROBE_END(pl)                                                                               \
  if (pl.probe && threadIdx.x == 0) {                                                               \
    uint64_t* o_ = pl.probe + size_t(blockIdx.x) * 8;                                               \
    o_[0] = pb_r0_; o_[1] = __builtin_amdgcn_s_memrealtime(); o_[2] = pb_c0_; o_[3] = __builtin_amdgcn_s_memtime(); \
    o_[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4); o_[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20); o_[6] = pb_rm_; \
  }
#define PROBE_BLOCK(pl) (pl.probe_mod ? blockIdx.x % pl.probe_mod : blockIdx.x)
#define PROBE_GRID(pl) (pl.probe_mod ? pl.probe_mod : gridDim.x)
#else
#define PROBE_BEGIN(pl)
#define PROBE_MID(pl)
#define PROBE_END(pl)
#define PROBE_BLOCK(pl) blockIdx.x
#define PROBE_GRID(pl) gridDim.x
#endif

// LDS exchanges of a 4096-element tile (barrier, write 8, barrier, read 8) on the element E of either lane form, slots by MAP.
// Thread-major (slot 8 t + r) <-> strided (slot 512 j + t); TO_STRIDED: written thread-major and read strided, otherwise the mirror image.
using SlotMap = uint32_t (*)(uint32_t);
template <SlotMap MAP, bool TO_STRIDED, class E>
__device__ __forceinline__ void exch_thread_major(E* X, E (&x)[8], uint32_t t) {
  lds_barrier();
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) X[MAP(TO_STRIDED ? t * 8 + k : k * 512 + t)] = x[k];
  lds_barrier();
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) x[k] = X[MAP(TO_STRIDED ? k * 512 + t : t * 8 + k)];
}
// Wave-major (slot 512 wave + 64 r + off; off: the lane, or the column kernels' (k1 | k2 | c) order of its bits) <-> strided.
template <SlotMap MAP, bool TO_STRIDED, class E>
__device__ __forceinline__ void exch_wave_major(E* X, E (&x)[8], uint32_t t, uint32_t wave, uint32_t off) {
  lds_barrier();
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) X[MAP(TO_STRIDED ? wave * 512 + k * 64 + off : k * 512 + t)] = x[k];
  lds_barrier();
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) x[k] = X[MAP(TO_STRIDED ? k * 512 + t : wave * 512 + k * 64 + off)];
}

// previous run (in digit order) of run (T, i1); see kernels.hip
__device__ __forceinline__ uint64_t carry_in_of(const DevPlan& pl, const uint64_t* cbuf, uint32_t T, uint32_t i1) {
  const uint32_t NT = pl.M2 / pl.C;
  if (T > 0) return cbuf[size_t(T - 1) * pl.M1 + i1];
  return cbuf[size_t(NT - 1) * pl.M1 + (i1 ? i1 - 1 : pl.M1 - 1)];
}

// out[k] = sum_j in[j] omega_4^(jk), omega_4 = 2^48 (forward; the inverse uses omega_4^-1 = -2^48), in place
template <bool INV>
__device__ __forceinline__ void dft4(uint64_t& x0, uint64_t& x1, uint64_t& x2, uint64_t& x3) {
  const uint64_t a0 = gf::add(x0, x2), a1 = gf::add(x1, x3), b0 = gf::sub(x0, x2);
  const uint64_t b1 = gf::mul_pow2(INV ? gf::sub(x3, x1) : gf::sub(x1, x3), 48);
  x0 = gf::add(a0, a1); x2 = gf::sub(a0, a1); x1 = gf::add(b0, b1); x3 = gf::sub(b0, b1);
}

// weak carry of a run's incoming carry word into its first digits (adc4, marin.cl:203-212)
// di: the thread's word of the digit-info table (2 bits per digit: width - q, wrap), run = index of the run
// among the thread's R runs
template <int ND>
__device__ __forceinline__ void apply_carry_in(const DevPlan& pl, uint32_t di, int run, uint64_t cin, uint32_t (&d)[ND]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t width = pl.q + ((di >> (2 * (run * ND + k))) & 1u);
    const uint64_t v = uint64_t(d[k]) + cin;
    d[k] = __builtin_amdgcn_ubfe(uint32_t(v), 0u, width);
    cin = v >> width;
  }
  d[3] += uint32_t(cin);
}

// ---- run head and carry tail of the register-resident column sweeps (kernels_v2.hip, kernels_v3.hip) ----
// (kernels_v5.hip keeps copies of its own, and its dead `sub` / `scale` parameters: without those two alone its back sweep at C4,
// k3_cols5<0, false>, runs at 73-74 us instead of 58 in some processes, same-box A/B in profiles/radix8_forms_ab.txt, measurements 1-3b;
// the ISAs differ in nothing that explains it, the cause is open)
// digit runs <-> registers: run number `run` of a register (tile-major) is ND consecutive u32
template <int ND>
__device__ __forceinline__ void load_run(const uint32_t* __restrict__ digits, size_t run, uint32_t (&d)[ND]) {
  const uint4* src = reinterpret_cast<const uint4*>(digits) + run * (ND / 4);
#pragma unroll
  for (int q = 0; q < ND / 4; ++q) { const uint4 v = src[q]; d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w; }
}
template <int ND>
__device__ __forceinline__ void store_run(uint32_t* __restrict__ digits, size_t run, const uint32_t (&d)[ND]) {
  uint4* dst = reinterpret_cast<uint4*>(digits) + run * (ND / 4);
#pragma unroll
  for (int q = 0; q < ND / 4; ++q) dst[q] = make_uint4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
}
// digits of one run -> its ND / 2 weighted pairs (run: index among the thread's runs, for the thread's word of the digit-info table).
// Weight TA*TB, halved when the exponents wrap: the halving is moved onto TA (once per run: tah, and tah1 for the odd digits, whose exponent
// is split SA[M1 + i1] + SB[2 i2], plan.hpp) and the un-wrapped digits are doubled instead (digits are < 2^31, the product stays a mul_u32);
// nowrap = ~di: bit 2 idx + 1 of di says that the weight exponents of digit idx wrapped
template <int ND>
__device__ __forceinline__ void weigh_run(uint64_t tah, uint64_t tah1, uint32_t nowrap, int run, const uint32_t (&dg)[ND], P2* x) {
#pragma unroll
  for (int c = 0; c < ND / 2; ++c) {
    const int idx = run * ND + 2 * c;
    x[c] = {gf::mul_u32(tah, dg[2 * c] << ((nowrap >> (2 * idx + 1)) & 1u)), gf::mul_u32(tah1, dg[2 * c + 1] << ((nowrap >> (2 * idx + 3)) & 1u))};
  }
}
// one digit of the carry chain: u a + addend + carry -> digit of `width` bits, carry (adc_mul, marin.cl:194-201)
__device__ __forceinline__ uint32_t adc_mul(uint64_t u, uint32_t a, uint32_t addend, uint32_t width, uint64_t& carry) {
  if (a == 1) {               // the common case (uniform): no 64-bit multiplies
    const uint64_t r = u + carry + addend;   // u < P only, carry < 2^(64 - width), addend < 2^32: below 2^64 (see kernels.hip adc_mul)
    carry = r >> width;
    return __builtin_amdgcn_ubfe(uint32_t(r), 0u, width);   // width < 32: one bit-field extract
  }
  const uint64_t mask = (uint64_t(1) << width) - 1;
  const uint64_t dlo = u & mask, chi = u >> width;
  const uint64_t r = dlo * a + carry + addend;
  carry = (r >> width) + chi * a;
  return uint32_t(r & mask);
}
// the ND / 2 pairs of one run -> unweighted (tai_e / tai_o for the even / odd digits, tai2_* where the exponents wrapped: the weight was
// halved), x a, sequential carry from zero -> digits; returns the carry leaving the run.
// ADD: ad[k] (the digits of another residue's run, pending carries already folded in) join the carry chain (mul_add)
template <int ND, bool ADD>
__device__ __forceinline__ uint64_t unweigh_carry(const DevPlan& pl, uint32_t di, int run, const P2* x, uint64_t tai_e, uint64_t tai_o,
                                                  uint64_t tai2_e, uint64_t tai2_o, uint32_t a, const uint32_t* ad, uint32_t (&dg)[ND]) {
  uint64_t carry = 0;
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    const uint32_t bits = di >> (2 * (run * ND + k));   // digit-info table: width - q, wrap
    const P2 v = x[k >> 1];
    const bool wrap = (bits & 2u) != 0;
    const uint64_t u = (k & 1) ? gf::mul(v.b, wrap ? tai2_o : tai_o) : gf::mul(v.a, wrap ? tai2_e : tai_e);
    dg[k] = adc_mul(u, a, ADD ? ad[k] : 0u, pl.q + (bits & 1u), carry);
  }
  return carry;
}

}  // namespace v2

hipError_t v5_configure();   // (kernels_v5.hip; called by v2_configure)

}  // namespace mi355
