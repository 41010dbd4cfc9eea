// Device-side view of a Plan and the kernel launch entry points (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi355 {

struct DevPlan {
  uint32_t n, m, M1, M2, L1, logL1, logM2, r5, C, logC, q, t, twh;
  // Residues per register (plan token lanes=B; 1: a plain engine).  A register slot -- and the work buffer, and a multiplicand image -- is
  // `lanes` single-lane registers 8 n bytes apart, a carry buffer `lanes` x M1 M2 / C words.  The generic kernels (kernels.hip) take the lane
  // from blockIdx.y and move their pointers, which are those of lane 0, to it (their instantiations k<true>; lanes == 1 launches k<false>,
  // which leaves the pointers alone); no other kernel set reads this.
  uint32_t lanes;
  const uint32_t *SA, *SB;
  const uint64_t *TA, *TAi, *TB, *TBi;
  const uint64_t *TAh, *TAi2;   // TA / 2 and 2 TAi, entry by entry: what the sweeps multiply with when the exponent split wraps (no per-thread half / double)
  const uint64_t *TWlo, *TWhi, *UT1, *UT2;
  const uint64_t *S2r, *S2ri, *S1r, *S1ri;   // seam tables of the radix-8 kernels (null when the shape is not served)
  uint64_t I4, I4inv;   // no kernel reads them any more (omega_4 = 2^48 is a shift); they stay so that every later member keeps its offset
  uint64_t W5c[4];   // 5-point DFT constants {beta, k1, k2-k1, k1+k2} (kernels.hip dft5)
  const uint64_t *F0f, *F0i, *FBf, *FBi;   // four-step chain starts [tile][thread] and ratios [column] of the v2 column kernels
  const uint32_t* DI;   // digit-info words of the v2 column kernels: [tile][thread] 16 x (width - q, wrap), or null
  uint32_t boost_rows, boost_tiles;   // first block index of the last half round of the row / column launches (or ~0u)
  // Frequency label of the column-transform output slot (blk, rq): lab_u blk + lab_v rq.  (1, r5) for the mixed-radix columns of every kernel
  // set but one; the radix-5 columns in prime-factor form (kernels_v5.hip) hold the frequency (PU k0 + PV kr) mod M1 in slot (k0, kr) and the
  // engine sets (PU, PV) when they run both column sweeps.  See col_label() below.
  uint32_t lab_u, lab_v;
  uint32_t lab_red;   // the generic prime-factor radix-5 stage (kernels.hip lds_radix5): labels are taken mod M1 (lab_red = M1; they are below 5 M1); 0: as they are
#if defined(MI355_PROBE)
  uint64_t* probe;        // timeline probe (tools/probe.py, libmi355_engine_probe.so only): 8 words per work-group, or null
  uint32_t probe_mod;     // blockIdx.x is taken modulo this (launches of several rounds over the same tiles)
#endif
  uint32_t tune;   // MI355_TUNE (A/B runs), read by the kernels only: bit 0 plain (not XCD-contiguous) tile order in the back sweeps; bit 5 the other tile order in the front sweeps
  uint32_t onelaunch;   // plan token onelaunch: products run as one launch of k_onelaunch (kernels.hip).  Last, so that no other member moves.
};

#if defined(__HIPCC__)
// Frequency label of the column-transform output slot (blk, rq) -- rq the bit-reversed position inside the radix-5 block (kernels.hip freq1).
// Every use of a column frequency k1 (the four-step twiddle omega_m^(i2 k1), the point rho = omega_m^(k1 + M1 k) of the pointwise stage) only
// needs SOME integer congruent to it mod M1, the same one in the front sweep, the row sweep and the back sweep: a representative k1 + M1 s
// shifts the row transform's outputs by s places and the total frequency k1 + M1 k2 stays what the label says.  The prime-factor columns use
// PU blk + PV rq unreduced (< 2^20; their twiddle chains step through rq by constant ratios); the two-level root table reaches m + 2^20.
__device__ __forceinline__ uint32_t col_label(const DevPlan& pl, uint32_t blk, uint32_t rq) {
  uint32_t l = pl.lab_u * blk + pl.lab_v * rq;
  if (pl.lab_red) {   // the generic kernels multiply a label by a column index and need the product below m: the representative below M1
#pragma unroll
    for (int i = 0; i < 4; ++i) l = (l >= pl.lab_red) ? l - pl.lab_red : l;
  }
  return l;
}
// exponent of rho = omega_m^(label + M1 k): below m + 2^20 (plan.hpp TWhi)
__device__ __forceinline__ uint64_t rho_exponent(const DevPlan& pl, uint32_t label, uint64_t k) { return uint64_t(label) + uint64_t(pl.M1) * k; }
#endif

// Extras of a back sweep (the reference's fused carry variants, kernels/marin.cl:2160-2365):
//   digits2 / cbuf2: a second register that receives the same result (square_mul_copy, mul_copy)
//   add_digits (+ add_cbuf: its run carries when they are still pending): a residue added inside the carry chain (mul_add)
struct BackExt {
  uint32_t* digits2 = nullptr; uint64_t* cbuf2 = nullptr;
  const uint32_t* add_digits = nullptr; const uint64_t* add_cbuf = nullptr;
  bool any() const { return digits2 || add_digits; }
};
// Linear combinations of digit registers in one sweep (add / sub_reg / addsub / addsub_copy, marin.cl:1856-1947):
// a, b with their pending run carries (null when none); outputs sum (s1, s2) and difference (d1, d2), each with the carry
// words it leaves pending.  Digit outputs may alias the inputs; carry outputs must not alias ca / cb.
struct LinArgs {
  const uint32_t* a = nullptr; const uint64_t* ca = nullptr; const uint32_t* b = nullptr; const uint64_t* cb = nullptr;
  uint32_t* s1 = nullptr; uint64_t* cs1 = nullptr; uint32_t* s2 = nullptr; uint64_t* cs2 = nullptr;
  uint32_t* d1 = nullptr; uint64_t* cd1 = nullptr; uint32_t* d2 = nullptr; uint64_t* cd2 = nullptr;
};
hipError_t launch_linear(const DevPlan& pl, const LinArgs& la, hipStream_t s);
// out = (in + its pending carries cin, nullable) x a, run-wise, carry-out words to cout (kernels.hip k_scale)
hipError_t launch_scale(const DevPlan& pl, const uint32_t* in, const uint64_t* cin, uint32_t* out, uint64_t* cout, uint32_t a, hipStream_t s);
hipError_t launch_carry_fix(const DevPlan& pl, uint32_t* digits, const uint64_t* cbuf, hipStream_t s);
hipError_t launch_sub_small(const DevPlan& pl, uint32_t* digits, uint32_t a, hipStream_t s);

// Launchers of the sweeps, one per kernel variant (plan.hpp ColKernels / RowKernels).  The engine takes those of its plan's variants once
// and calls them as they are: none of them tests the shape.
//   front: digits (+ the run carries cbuf_in left by the last back sweep, nullable; needs C >= 2) -> work buffer W
//   back: W -> digits x a + one carry word per run; back_ext: with the extras of BackExt
//   build_fourstep (register-resident columns): the chain starts and ratios of their four-step twiddles (tiles x threads x 2 + M2 x 2 words)
//   rows: Win -> Wout (mode 0: squaring, 1: times the multiplicand image Y, 2: forward only, Wout a multiplicand image,
//         3: times the SUM of the images Y and Y2, added word by word in the field: the forward transform is linear, so that is the image of
//         the sum of the two residues; Y2 is read in mode 3 only,
//         4: squaring that also stores the forward transform of its operand to Wimg, in the form in which the same kernel's mode 2 stores
//         it: Wimg is then a multiplicand image of the operand; written in mode 4 only)
typedef hipError_t (*FrontFn)(const DevPlan& pl, const uint32_t* digits, const uint64_t* cbuf_in, uint64_t* W, hipStream_t s);
typedef hipError_t (*BackFn)(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s);
typedef hipError_t (*BackExtFn)(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& x, hipStream_t s);
typedef hipError_t (*FourStepFn)(const DevPlan& pl, uint64_t* f0f, uint64_t* f0i, uint64_t* fbf, uint64_t* fbi, hipStream_t s);
typedef hipError_t (*RowsFn)(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
struct ColSweeps { FrontFn front; BackFn back; BackExtFn back_ext; FourStepFn build_fourstep; };

// generic set (kernels.hip): tiles in LDS, any shape, pl.lanes lanes as grid.y (the run-wise launchers above too)
// (onelaunch: the entry points of the one-launch products and of the batches too, to the LDS of their largest size)
hipError_t configure_kernels(size_t lds_front, size_t lds_mid, uint32_t lanes, bool onelaunch);
hipError_t launch_front(const DevPlan& pl, const uint32_t* digits, const uint64_t* cbuf_in, uint64_t* W, hipStream_t s);
hipError_t launch_middle(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
// rows in mode 1 with the image of lane l read from Ysrc at l's sibling lane of `level` where that lane exists, else from Yalt at lane l
// (include/mi355_lanecross.h; k_middle_sibling).  Lane engines only, level <= 31.
hipError_t launch_middle_sibling(const DevPlan& pl, const uint64_t* Win, const uint64_t* Ysrc, const uint64_t* Yalt, uint64_t* Wout, uint32_t level, hipStream_t s);
hipError_t launch_back(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s);
hipError_t launch_back_ext(const DevPlan& pl, const uint64_t* W, uint32_t* digits, uint64_t* cbuf, uint32_t a, const BackExt& x, hipStream_t s);
// One-launch products (plan token onelaunch, n <= 8192; kernels.hip k_onelaunch): front sweep, row sweep and back sweep of a lane in one
// work-group, the work buffer in LDS.  A group holds K whole lanes with TL threads each (plan.hpp onelaunch_shape), `groups` of them.
//   src (+ src_cbuf: its pending run carries, nullable) -> front; rows in `mode` (the modes of RowsFn above: y, y2 read in modes 1 and 3, img
//   written in modes 2 and 4); unless mode 2: back into dst, dst_cbuf with factor a and the extras x.  dst may be src: a lane's digits are all
//   read before the first is written.  dst_cbuf must not be src_cbuf or x.add_cbuf.
//   mode kModeSibling (lane engines; k_onelaunch_sibling, a launch of its own, never a descriptor of a batch): mode 1 whose image is read at y
//   from the lane's sibling of `level` -- lane ((l >> level) ^ 1) << level -- where that lane exists, else at y2 from the own lane; no extras.
constexpr int kModeSibling = 5;
struct OneLaunchArgs {
  const uint32_t* src = nullptr; const uint64_t* src_cbuf = nullptr;
  const uint64_t* y = nullptr; const uint64_t* y2 = nullptr; uint64_t* img = nullptr;
  uint32_t* dst = nullptr; uint64_t* dst_cbuf = nullptr;
  uint32_t a = 1; int mode = 0;
  uint32_t TL = 0, K = 0, groups = 0;
  uint32_t level = 0;   // kModeSibling only.  In what was padding: the size and every other member's offset are what they were
};
static_assert(sizeof(OneLaunchArgs) == 80, "OneLaunchArgs: the level sits in the padding, the argument block of the existing kernels is unchanged");
hipError_t launch_onelaunch(const DevPlan& pl, const OneLaunchArgs& oa, const BackExt& x, hipStream_t s);
// Batches (kernels.hip k_batch): a run of register operations of a one-launch engine as ONE launch with the grid, block and
// LDS of k_onelaunch.  Every work-group walks the descriptors in order for its own lanes, a group barrier after each.  All pointers are
// those of lane 0, resolved by the host when the operation was issued (carry buffers included), exactly as the single launches take them.
//   kProduct: oa and x, as launch_onelaunch takes them (oa.TL, oa.K, oa.groups are not read: the launch has its own)
//   kLinear:  la, as launch_linear takes it
//   kCopy:    la.s1 <- la.a, copy_bytes bytes a lane (a multiple of 16); la.cs1 <- la.ca, a lane's carry words, where la.ca is not null
struct BatchOp {
  enum : uint32_t { kProduct = 0, kLinear = 1, kCopy = 2 };
  uint32_t kind = kProduct, copy_bytes = 0;
  OneLaunchArgs oa;
  BackExt x;
  LinArgs la;
};
hipError_t launch_batch(const DevPlan& pl, const BatchOp* ops, uint32_t count, uint32_t TL, uint32_t K, uint32_t groups, hipStream_t s);
// columns of 5 L1 pairs that do not fit LDS (n = 5 * 2^26): the radix-5 stage through a second work buffer U (8 n bytes), C = 1
hipError_t configure_split(const DevPlan& pl);
hipError_t launch_front_split(const DevPlan& pl, const uint32_t* digits, uint64_t* U, uint64_t* W, hipStream_t s);
hipError_t launch_back_split(const DevPlan& pl, const uint64_t* W, uint64_t* U, uint32_t* digits, uint64_t* cbuf, uint32_t a, hipStream_t s);

// register-resident sets; v2_configure sets the LDS size of the radix-8 and radix-5 kernels
hipError_t v2_configure();
ColSweeps v2_cols(uint32_t R);    // radix-8 columns of 512 R, R = 1, 2, 4 (kernels_v2.hip)
ColSweeps v3_cols(bool planes);   // radix-4 columns of 256 x 4, a pair or a plane per thread (kernels_v3.hip)
ColSweeps v5_cols(bool j1);       // radix-5 columns of 1280 x 4 or (j1) 2560 x 2 (kernels_v5.hip)
void v5_pfa(bool j1, uint32_t* u, uint32_t* v);   // the frequency map of their prime-factor form (DevPlan.lab_u / lab_v)
hipError_t v2_rows4096(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
hipError_t v2_rows8192(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
hipError_t v2_rows2048_one(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
hipError_t v2_rows2048_two(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
hipError_t v3_rows1024_pairs(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
hipError_t v3_rows1024_planes(const DevPlan& pl, const uint64_t* Win, const uint64_t* Y, const uint64_t* Y2, uint64_t* Wimg, uint64_t* Wout, int mode, hipStream_t s);
#if defined(MI355_PROBE)
// one launch of sweep `kind` (0 front, 1 rows, 2 back) over grid_mult x the normal grid with extra_lds bytes of padding LDS:
// the rows of 4096 and the columns of 1024 x 4 (v2), the columns of 1280 x 4 (v5)
hipError_t v2_probe_launch(const DevPlan& pl, int kind, int grid_mult, int extra_lds, const uint32_t* digits, uint64_t* cbuf, uint64_t* W, uint32_t* dout, hipStream_t s);
hipError_t v5_probe_launch(const DevPlan& pl, int kind, int grid_mult, int extra_lds, const uint32_t* digits, uint64_t* cbuf, uint64_t* W, uint32_t* dout, hipStream_t s);
#endif

}  // namespace mi355
