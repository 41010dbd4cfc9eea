// Host API of the device-side canonical form (canon.hip): strong carry with wrap-around into natural order, compare, residue words <-> digits.
// One set of launchers for both digit types, T = uint32_t (Goldilocks engine: tile-major registers, widths below 32) or uint64_t (the
// GF(M61^2) x GF(M31^2) engine: natural order, widths up to 39 bits); the geometry says which layout a register has.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace mi355 {

struct CanonGeom {   // n = r5 * 2^logn2 (r5: the odd factor 1, 3, 5 or 9); M1 = 0: natural digit order
  uint32_t p, n, logn2, r5, M1, M2, C;
  static CanonGeom tile_major(const DevPlan& pl, uint32_t p);          // the registers of a Goldilocks plan (plan.hpp Plan::pos)
  static CanonGeom natural(uint32_t p, uint32_t n, uint32_t odd);      // digits in natural order, n = odd * 2^k
};

// scratch of canon_launch: two arrays of n digits, block aggregates, block carries, 16 flag words
template <class T> size_t canon_scratch_bytes(const CanonGeom& g);
// flags (device, inside scratch; the caller clears them): [0] value was 2^p - 1 (written as 0), [1] a digit was still too wide for the 0/1
// carry chain (sticky; the caller then uses the host carry), [2] compare result (sticky)
template <class T> uint32_t* canon_flags(const CanonGeom& g, void* scratch);
// digits: a register in the geometry's layout (run carries applied; any excess the three local passes remove).  out: n canonical digits in
// natural order, 2^p - 1 -> 0
template <class T> hipError_t canon_launch(const CanonGeom& g, const T* digits, T* out, void* scratch, hipStream_t s);
template <class T> hipError_t canon_compare(const T* a, const T* b, uint32_t n, uint32_t* diff_flag, hipStream_t s);
// canon: n canonical digits in natural order (canon_launch) -> words: ceil(p / 32) little-endian words of the residue
template <class T> hipError_t canon_pack_words(const CanonGeom& g, const T* canon, uint32_t* words, hipStream_t s);
// words: ceil(p / 32) words of a value below 2^p -> the digits of a register in the geometry's layout
template <class T> hipError_t canon_unpack_words(const CanonGeom& g, const uint32_t* words, T* digits, hipStream_t s);

// ---- a chunk of lanes in one launch sequence (tile-major uint32_t registers; lane l of the register lies in_stride digits behind lane 0) ----
// The scratch of the lane-wise pipeline is bounded: an engine with more lanes than canon_chunk_lanes takes them chunk by chunk.
constexpr size_t kCanonLanesScratchBytes = size_t(64) << 20;
size_t canon_lane_bytes(size_t n);                    // scratch of one lane: four arrays of n digits, block aggregates, block carries, 16 flag words
size_t canon_chunk_lanes(size_t n, size_t lanes);     // lanes per chunk: as many as fit kCanonLanesScratchBytes, at least 1, at most `lanes`
// scratch: L * canon_lane_bytes(n); canonical digits go to output slot 0 or 1 of the scratch.  flags: 16 words a lane, [0] [1] [2] as above (the caller clears them)
uint32_t* canon_lanes_flags(const CanonGeom& g, void* scratch, size_t L);
hipError_t canon_launch_lanes(const CanonGeom& g, const uint32_t* digits, size_t in_stride, size_t L, int slot, void* scratch, hipStream_t s);
hipError_t canon_compare_lanes(const CanonGeom& g, size_t L, void* scratch, hipStream_t s);   // slot 0 against slot 1 -> flag [2] of each lane
// slot's canonical digits -> ceil(p / 32) words a lane, lane after lane, in *words (inside the scratch: the work arrays are free by then)
hipError_t canon_pack_words_lanes(const CanonGeom& g, size_t L, int slot, void* scratch, uint32_t** words, hipStream_t s);
// the way back: ceil(p / 32) words a lane, lane after lane (each a value below 2^p), -> the digits of L lanes of a register, lane l
// out_stride digits behind lane 0 (`out`)
hipError_t canon_unpack_words_lanes(const CanonGeom& g, const uint32_t* words, uint32_t* out, size_t out_stride, size_t L, hipStream_t s);

// natural order only (uint64_t): one local carry pass in -> out (digits of up to w + e bits come out below 2^w + 2^e), and
// dst += the digit-wise complement of a canonical residue, i.e. dst - canon mod 2^p - 1
hipError_t canon_local_pass(const CanonGeom& g, const uint64_t* in, uint64_t* out, hipStream_t s);
hipError_t canon_add_complement(const CanonGeom& g, uint64_t* dst, const uint64_t* canon, hipStream_t s);

// tile-major registers of a Goldilocks plan only
hipError_t canon_relax(const DevPlan& pl, uint32_t p, const uint32_t* in, uint32_t* out, hipStream_t s);   // one local carry pass, tile-major both sides
hipError_t canon_scatter(const DevPlan& pl, uint32_t p, const uint32_t* nat, uint32_t* digits, hipStream_t s);   // natural order -> tile-major
hipError_t canon_set_small(const DevPlan& pl, uint32_t p, uint32_t* digits, uint32_t value, hipStream_t s);

}  // namespace mi355
