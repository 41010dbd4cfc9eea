// Host-side digit arithmetic of both engines (engine.hip, crt_engine.hip): the fallback paths behind MI355_HOST_CARRY=1 or a device chain that
// reports an over-wide digit, and the few head digits of res64.  The reference does all of this on the host (include/marin/engine_gpu.h:1534-1561,
// include/marin/engine.h:173-295).  A residue is n digits in natural order, digit j in base 2^width[j] at bit offset ceil(p j / n); digits are
// uint64_t for both families (the Goldilocks engine widens its u32 staging).  Arithmetic only: which counts and values a call accepts is each
// engine's policy (register_machine.hpp).  Plain C++: no HIP header, so tests/host/host_digits_query.cpp builds it with g++ alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mi355 {
namespace host_digits {

typedef unsigned __int128 u128;

// width[j] = ceil(p (j + 1) / n) - ceil(p j / n) (ibdwt.h:127-132)
inline std::vector<uint8_t> digit_widths(uint32_t p, size_t n) {
  std::vector<uint8_t> width(n);
  uint64_t prev = 0;
  for (size_t j = 0; j < n; ++j) {
    const uint64_t next = (uint64_t(p) * (j + 1) + n - 1) / n;
    width[j] = uint8_t(next - prev);
    prev = next;
  }
  return width;
}
inline uint64_t ones(uint8_t w) { return (uint64_t(1) << w) - 1; }

// Strong carry in place: every digit below 2^width, the carry out of the last digit re-enters digit 0 (2^p = 1), laps until it is zero
// (engine_gpu.h:1543-1557).  Digits below 2^63 come through (digit + carry stays below 2^64).  The value 2^p - 1 stays all ones.
inline void strong_carry(uint64_t* d, const std::vector<uint8_t>& width) {
  const size_t n = width.size();
  uint64_t c = 0;
  for (size_t k = 0; k < n; ++k) {
    const uint64_t t = d[k] + c;
    d[k] = t & ones(width[k]);
    c = t >> width[k];
  }
  while (c != 0) {
    for (size_t k = 0; k < n && c != 0; ++k) {
      const uint64_t t = d[k] + c;
      d[k] = t & ones(width[k]);
      c = t >> width[k];
    }
  }
}

// the canonical digits of 2^p - 1, which is 0 (engine.h:188-196)
inline bool is_all_ones(const uint64_t* d, const std::vector<uint8_t>& width) {
  for (size_t k = 0; k < width.size(); ++k) if (d[k] != ones(width[k])) return false;
  return true;
}

// canonical digits -> `count` little-endian 32-bit words of the residue in [0, 2^p - 1): all ones come out as 0; bits at and above 32 count
// are dropped.  A digit of 39 bits that starts at bit 26 or above of a word spans three words: 128-bit pieces.
inline void pack_words(const uint64_t* d, const std::vector<uint8_t>& width, uint32_t* w, size_t count) {
  for (size_t i = 0; i < count; ++i) w[i] = 0;
  if (is_all_ones(d, width)) return;
  size_t bit = 0;
  for (size_t k = 0; k < width.size(); ++k) {
    const size_t i = bit >> 5;
    const u128 v = u128(d[k]) << (bit & 31);
    for (size_t x = 0; x < 3 && i + x < count; ++x) w[i + x] |= uint32_t(v >> (32 * x));
    bit += width[k];
  }
}

// `count` words (words at and above count read as zero) -> digits: digit k is the width[k] bits at its offset (engine.h:206-232)
inline void unpack_words(const uint32_t* w, size_t count, const std::vector<uint8_t>& width, uint64_t* d) {
  size_t bit = 0;
  for (size_t k = 0; k < width.size(); ++k) {
    const size_t i = bit >> 5;
    u128 v = 0;
    for (size_t x = 0; x < 3 && i + x < count; ++x) v |= u128(w[i + x]) << (32 * x);
    d[k] = uint64_t(v >> (bit & 31)) & ones(width[k]);
    bit += width[k];
  }
}

// The ceil(p / 32) words of any value below 2^(32 count), folded below 2^p with 2^p = 1: the bits at and above p are added in at bit 0 until
// none is left (2^p - 1 stays as it is: the digits' canonical form decides that one)
inline void fold_words_mod_mp(uint32_t* w, size_t count, uint32_t p) {
  const unsigned top = p % 32;
  if (top == 0 || count == 0) return;
  while (uint64_t c = w[count - 1] >> top) {
    w[count - 1] &= (1u << top) - 1;
    for (size_t i = 0; c != 0 && i < count; ++i) {
      c += w[i];
      w[i] = uint32_t(c);
      c >>= 32;
    }
  }
}

// the low 64 bits of the value of the first `have` canonical digits (engine.h:257-269): the digits up to the one that reaches bit 64
inline uint64_t res64_of_head(const uint64_t* d, const std::vector<uint8_t>& width, size_t have) {
  uint64_t r = 0;
  unsigned s = 0;
  for (size_t k = 0; k < have && s < 64; ++k) {
    r |= d[k] << s;
    s += width[k];
  }
  return r;
}

}  // namespace host_digits
}  // namespace mi355
