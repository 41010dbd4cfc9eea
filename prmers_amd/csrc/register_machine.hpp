// RegisterMachine: the one interface of both field families behind the C ABI (capi.cpp holds one pointer to it).  Engine (engine.hip,
// Goldilocks) and CrtEngine (crt_engine.hip, GF(M61^2) x GF(M31^2)) implement the primitives; the composed operations are written once here,
// as the reference's `engine` base class writes them (include/marin/engine.h:65-131, restated in include/mi355/engine_iface.h:44-58), and a
// family overrides the ones it can fuse into fewer sweeps.
//
// Where the two families answer differently, on purpose (each keeps its own argument policy; host_digits.hpp does the arithmetic only):
//   get_words   Engine wants count == word_count().  CrtEngine accepts a longer buffer and zero-fills it.
//   set_words   Engine folds the bits at and above p back in (2^p = 1).  CrtEngine refuses a value that has any.
//   res64       of the value 2^p - 1: Engine returns the low 64 bits of the all-ones digit vector, as the reference's digit::res64 does
//               (engine.h:257-269).  CrtEngine returns 0.
//   get_digits / set_digits (value | width << 32): CrtEngine refuses them at transform sizes with digits wider than 32 bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace mi355 {

class RegisterMachine {
 public:
  virtual ~RegisterMachine() = default;

  // ---- the primitives ----
  virtual uint32_t exponent() const = 0;
  virtual size_t size() const = 0;        // transform size n: digits per register
  virtual size_t reg_count() const = 0;
  virtual std::string describe() const = 0;
  virtual size_t algorithmic_bytes() const = 0;
  virtual void sync() = 0;

  virtual void set_u32(size_t dst, uint32_t v) = 0;
  virtual void copy(size_t dst, size_t src) = 0;
  virtual void square_mul(size_t reg, uint32_t factor) = 0;      // reg = reg^2 * factor
  virtual void set_multiplicand(size_t dst, size_t src) = 0;     // dst = the transformed image of src; dst may be src
  virtual void mul(size_t dst, size_t src, uint32_t factor) = 0; // dst = dst * src * factor, src a multiplicand image
  virtual void add(size_t dst, size_t src) = 0;
  virtual void sub_reg(size_t dst, size_t src) = 0;
  virtual void sub_u32(size_t reg, uint32_t v) = 0;
  virtual bool equal(size_t lhs, size_t rhs) = 0;                // same value mod 2^p - 1
  // sum -> sum (and sum_copy), difference -> diff (and diff_copy) of the residues a and b; -1: not wanted
  virtual void addsub(long sum, long sum_copy, long diff, long diff_copy, size_t a, size_t b) = 0;

  virtual void set_digits(size_t dst, const uint64_t* d, size_t count) = 0;   // n canonical digits, value | width << 32 (engine.h:23-25)
  virtual void get_digits(size_t src, uint64_t* d, size_t count) = 0;
  virtual void set_words(size_t dst, const uint32_t* w, size_t count) = 0;    // little-endian 32-bit words of the residue
  virtual void get_words(size_t src, uint32_t* w, size_t count) = 0;          // canonical: 2^p - 1 reads as 0
  virtual uint64_t res64(size_t src) = 0;

  // Lanes (include/mi355_lanes.h): an engine made with the plan token lanes=B holds B independent residues per register and applies every
  // operation to all of them; these read and write one.  A machine without lanes has the one lane 0, which is the register itself.
  virtual size_t lanes() const { return 1; }
  virtual void set_words_lane(size_t lane, size_t dst, const uint32_t* w, size_t count) { need_lane(lane, "set_words"); set_words(dst, w, count); }
  virtual void get_words_lane(size_t lane, size_t src, uint32_t* w, size_t count) { need_lane(lane, "get_words"); get_words(src, w, count); }
  virtual uint64_t res64_lane(size_t lane, size_t src) { need_lane(lane, "res64"); return res64(src); }
  // Every lane at once (include/mi355_lanewise.h): out[l] = lane l of lhs and of rhs are the same value mod 2^p - 1, and the canonical words
  // of every lane, lane l at l * word_count().  A machine without lanes answers for its one lane through equal / get_words.
  virtual void equal_lanes(size_t lhs, size_t rhs, uint8_t* out, size_t count) {
    if (count != lanes()) throw std::runtime_error("lanewise_equal: count must equal the lane count (" + std::to_string(lanes()) + ")");
    need_residue(lhs, "lanewise_equal"); need_residue(rhs, "lanewise_equal");
    out[0] = equal(lhs, rhs) ? 1 : 0;
  }
  virtual void get_words_lanes(size_t src, uint32_t* w, size_t count) {
    if (count != lanes() * word_count()) throw std::runtime_error("lanewise_get_words: count must equal lanes x word_count()");
    need_residue(src, "lanewise_get_words");
    get_words(src, w, count);
  }
  // and written: lane l of dst = the residue whose words are w[l * word_count() ..); a machine without lanes writes its one lane through set_words
  virtual void set_words_lanes(size_t dst, const uint32_t* w, size_t count) {
    if (count != lanes() * word_count()) throw std::runtime_error("lanewise_set_words: count must equal lanes x word_count()");
    need_register(dst, "lanewise_set_words");
    set_words(dst, w, count);
  }

  // Across lanes (include/mi355_lanecross.h): dst[l] = dst[l] * src[g] with g = ((l >> level) ^ 1) << level, the first lane of l's sibling
  // block of size 2^level, where g is a lane; dst[l] * alt[l] where it is not.  src and alt are multiplicand images, the factor is 1.
  // A machine with one lane has no sibling in range at any level, so the operation is mul(dst, alt): written here, once, for both
  // families.  An engine with lanes overrides it.  Checked before the first launch.
  virtual void mul_sibling(size_t dst, size_t src, size_t alt, uint32_t level) {
    check_mul_sibling(dst, src, alt, level);
    if (lanes() != 1) throw std::runtime_error("mul_sibling: not implemented for this engine with lanes");
    mul(dst, alt, 1);
  }

  // Batches (include/mi355_batch.h): the register operations between batch_begin and batch_end run as one launch.  Only the Goldilocks
  // engine with one-launch products has them (engine.hpp); stats: operations queued so far, batch launches so far, capacity, pending now.
  virtual void batch_begin() { throw std::runtime_error("batch_begin: batches are not implemented for the crt field family"); }
  virtual void batch_end() { throw std::runtime_error("batch_end: no batch is open (batch_begin comes first)"); }
  virtual void batch_stats(uint64_t out[4]) const { out[0] = out[1] = out[2] = out[3] = 0; }

  virtual size_t register_data_size() const = 0;                              // raw register images (engine.h:134-146)
  virtual void get_data(size_t src, void* data, size_t size) = 0;
  virtual void set_data(size_t dst, const void* data, size_t size) = 0;
  // throws unless `data` is an image this engine can load.  The base checks the size; both engines add the tag word (plan.hpp layout_tag)
  // of their own layout -- an image of another plan, exponent, family or (for a multiplicand) kernel set is refused, never loaded as
  // something else.  set_data runs it first; set_checkpoint runs it on every register before it loads one.
  virtual void check_data(const void* /*data*/, size_t size) const {
    if (size != register_data_size()) throw std::runtime_error("set_data: size mismatch");
  }

  // `iters` squarings (each followed by sub_u32(reg, sub) when sub != 0) under HIP events: total and per-stage times
  virtual void time_square_mul(size_t reg, uint32_t factor, uint32_t sub, size_t iters, double* total_ms, double* kernel_ms, size_t kernel_count) = 0;
  virtual size_t kernel_count() const = 0;
  virtual const char* kernel_name(size_t k) const = 0;

  // ---- compositions of the primitives; a family overrides what it fuses ----
  virtual void mul_add(size_t dst, size_t mul_src, size_t add_src, uint32_t factor) { mul(dst, mul_src, factor); add(dst, add_src); }
  virtual void square_mul_copy(size_t src, size_t dst_copy, uint32_t factor) { square_mul(src, factor); copy(dst_copy, src); }
  virtual void mul_copy(size_t dst, size_t src, size_t dst_copy, uint32_t factor) { mul(dst, src, factor); copy(dst_copy, dst); }

  // count x { square_mul(reg, factor); sub_u32(reg, sub) }: the inner loop of a PRP (sub = 0) or Lucas-Lehmer (sub = 2) run between two checks
  virtual void square_mul_n(size_t reg, uint32_t factor, size_t count, uint32_t sub) {
    need_residue(reg, "square_mul_n"); need_factor(factor, "square_mul_n");
    for (size_t i = 0; i < count; ++i) { square_mul(reg, factor); if (sub) sub_u32(reg, sub); }
  }

  // a = a^h * b (b squared first when square_b): the fold of a PRP proof (PRPLL's expMul / expMul2).  set_multiplicand(tmp, a), left-to-right
  // binary square_mul / mul over the bits of h below its top bit, set_multiplicand(b, b), mul(a, b): b and tmp end as multiplicand images.
  // Everything is checked before the first launch, so a refused call leaves the registers as they were.
  virtual void exp_mul(size_t a, uint64_t h, size_t b, size_t tmp, bool square_b) {
    need_residue(a, "exp_mul"); need_residue(b, "exp_mul"); need_register(tmp, "exp_mul");
    if (a == b || a == tmp || b == tmp) throw std::runtime_error("exp_mul: a, b and tmp must be three different registers");
    if (square_b) square_mul(b, 1);
    if (h == 0) copy(a, b);
    set_multiplicand(tmp, a);
    int top = 63;
    while (top > 0 && !((h >> top) & 1)) --top;
    for (int i = top - 1; i >= 0 && h != 0; --i) {
      square_mul(a, 1);
      if ((h >> i) & 1) mul(a, tmp, 1);
    }
    set_multiplicand(b, b);
    if (h != 0) mul(a, b, 1);
  }

  // dst = dst * (a + b) for two multiplicand images (left intact, may be the same register), tmp scratch: the inner step of P-1 stage 2.
  // Two products, exact for every plan; checked before the first launch.
  virtual void mul_sum(size_t dst, size_t src_a, size_t src_b, size_t tmp) {
    check_mul_sum(dst, src_a, src_b, tmp);
    copy(tmp, dst); mul(dst, src_a, 1); mul(tmp, src_b, 1); add(dst, tmp);
  }
  virtual bool mul_sum_is_fused() const { return false; }

  // img_out = the multiplicand image of src, then src = src^2 * factor: the two values of a Montgomery ladder step (X + Z and X - Z) that are
  // both squared and multiplied by.  img_out must not be src; checked before the first launch.
  virtual void square_mul_prepare(size_t src, size_t img_out, uint32_t factor) {
    check_square_mul_prepare(src, img_out, factor);
    set_multiplicand(img_out, src); square_mul(src, factor);
  }
  virtual bool square_mul_prepare_is_fused() const { return false; }

  // reg = reg^(2^nbits) * factor^B, B the nbits-bit integer in `bits` (most significant bit first, packed in bytes, bit 7 of a byte first):
  // one square_mul(reg, bit ? factor : 1) per bit (stage 1 of P-1: 3^E)
  virtual void square_mul_bits(size_t reg, uint32_t factor, const uint8_t* bits, size_t nbits) {
    if (!check_square_mul_bits(reg, factor, bits, nbits)) return;
    for (size_t i = 0; i < nbits; ++i) square_mul(reg, bit_of(bits, i) ? factor : 1u);
  }

  // ---- the same for every family ----
  size_t word_count() const { return (size_t(exponent()) + 31) / 32; }
  size_t checkpoint_size() const { return reg_count() * register_data_size(); }   // every register's image, in order (engine.h:142-146)
  void get_checkpoint(void* data, size_t size) {
    if (size != checkpoint_size()) throw std::runtime_error("get_checkpoint: size mismatch");
    const size_t rs = register_data_size();
    for (size_t r = 0; r < reg_count(); ++r) get_data(r, static_cast<unsigned char*>(data) + r * rs, rs);
  }
  void set_checkpoint(const void* data, size_t size) {
    if (size != checkpoint_size()) throw std::runtime_error("set_checkpoint: size mismatch");
    const size_t rs = register_data_size();
    for (size_t r = 0; r < reg_count(); ++r) check_data(static_cast<const unsigned char*>(data) + r * rs, rs);   // all or nothing
    for (size_t r = 0; r < reg_count(); ++r) set_data(r, static_cast<const unsigned char*>(data) + r * rs, rs);
  }

 protected:
  virtual bool holds_image(size_t reg) const = 0;   // reg < reg_count(): a multiplicand image, not a residue

  // argument checks, run before an operation's first launch
  void need_register(size_t reg, const char* op) const {
    if (reg >= reg_count()) throw std::runtime_error(std::string(op) + ": register index out of range");
  }
  void need_lane(size_t lane, const char* op) const {
    if (lane >= lanes()) throw std::runtime_error(std::string(op) + ": lane index out of range (the engine has " + std::to_string(lanes()) + ")");
  }
  void need_residue(size_t reg, const char* op) const {
    need_register(reg, op);
    if (holds_image(reg)) throw std::runtime_error(std::string(op) + ": register holds a multiplicand image, not a residue");
  }
  void need_image(size_t reg, const char* op) const {
    need_register(reg, op);
    if (!holds_image(reg)) throw std::runtime_error(std::string(op) + ": the source register is not a multiplicand (call set_multiplicand first)");
  }
  static void need_factor(uint32_t factor, const char* op) {
    if (factor == 0) throw std::runtime_error(std::string(op) + ": factor must be >= 1");
  }
  void check_mul_sum(size_t dst, size_t src_a, size_t src_b, size_t tmp) const {
    need_residue(dst, "mul_sum"); need_image(src_a, "mul_sum"); need_image(src_b, "mul_sum"); need_register(tmp, "mul_sum");
    if (dst == tmp || tmp == src_a || tmp == src_b)
      throw std::runtime_error("mul_sum: dst, tmp and the multiplicands must be different registers (src_a == src_b is allowed)");
  }
  void check_mul_sibling(size_t dst, size_t src, size_t alt, uint32_t level) const {
    need_register(dst, "mul_sibling"); need_register(src, "mul_sibling"); need_register(alt, "mul_sibling");
    if (dst == src || dst == alt) throw std::runtime_error("mul_sibling: dst must differ from src and from alt (src == alt is allowed)");
    need_residue(dst, "mul_sibling"); need_image(src, "mul_sibling"); need_image(alt, "mul_sibling");
    if (level > 31) throw std::runtime_error("mul_sibling: level must be at most 31 (a sibling block has 2^level lanes)");
  }
  void check_square_mul_prepare(size_t src, size_t img_out, uint32_t factor) const {
    need_residue(src, "square_mul_prepare"); need_register(img_out, "square_mul_prepare"); need_factor(factor, "square_mul_prepare");
    if (img_out == src) throw std::runtime_error("square_mul_prepare: img_out must differ from src");
  }
  bool check_square_mul_bits(size_t reg, uint32_t factor, const uint8_t* bits, size_t nbits) const {   // false: nothing to do
    need_residue(reg, "square_mul_bits");
    need_factor(factor, "square_mul_bits");
    if (nbits != 0 && !bits) throw std::runtime_error("square_mul_bits: null bit string");
    return nbits != 0;
  }
  static bool bit_of(const uint8_t* bits, size_t i) { return (bits[i >> 3] >> (7 - (i & 7))) & 1; }
  // the host fallback of equal(): both residues as canonical words (2^p - 1 reads as 0)
  bool equal_words(size_t lhs, size_t rhs) {
    std::vector<uint32_t> a(word_count()), b(word_count());
    get_words(lhs, a.data(), a.size()); get_words(rhs, b.data(), b.size());
    return a == b;
  }
};

}  // namespace mi355
