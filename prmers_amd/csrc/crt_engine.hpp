// Resident engine of the GF(M61^2) x GF(M31^2) squaring (crt_engine.hip): a register file of residues (digits of up to 39 bits in
// logical order) with the operations of the reference's plugin ABI (third_party/aevum/src/EngineApi.h:28-59): set, copy, square_mul,
// set_multiplicand / mul, add, sub, compare, read-back as canonical words.  Selected behind mi355_engine_create with
// fft_spec = "crt[:odd][:words=N][:h2=K]" (capi.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>

#include "register_machine.hpp"

namespace mi355 {

size_t crt_transform_size(uint32_t p, uint32_t odd);
uint32_t crt_auto_radix(uint32_t p, size_t* words);   // 1, 3 or 9 by the reference's stock / PFA size-ratio gates (0: no admissible size)

// The compositions of register_machine.hpp are this family's only form of them (one hidden scratch register serves addsub).
class CrtEngine final : public RegisterMachine {
 public:
  static constexpr int kKernels = 6;
  static const char* stage_name(size_t k);

  // odd in {1, 3, 9}; n_words = 0: the smallest admissible odd * 2^k; spec: "h2=K" forces rows of 2^K complex values (tests)
  CrtEngine(uint32_t p, size_t reg_count, uint32_t odd, size_t n_words, int device, const char* spec);
  ~CrtEngine() override;
  CrtEngine(const CrtEngine&) = delete;
  CrtEngine& operator=(const CrtEngine&) = delete;

  size_t size() const override;
  size_t reg_count() const override;
  uint32_t exponent() const override;
  std::string describe() const override;
  size_t algorithmic_bytes() const override;

  void set_u32(size_t reg, uint32_t a) override;
  void copy(size_t dst, size_t src) override;
  void square_mul(size_t reg, uint32_t a) override;
  void set_multiplicand(size_t dst, size_t src) override;
  void mul(size_t dst, size_t src, uint32_t a) override;
  void add(size_t dst, size_t src) override;
  void sub_reg(size_t dst, size_t src) override;
  void sub_u32(size_t reg, uint32_t a) override;
  void addsub(long sum_out, long sum_copy, long diff_out, long diff_copy, size_t a, size_t b) override;
  bool equal(size_t a, size_t b) override;
  // the family's own digits: plain u64 values in base 2^width_j, as they are on the device (weakly carried) or canonical
  void set_raw_digits(size_t reg, const uint64_t* d, size_t count);
  void get_raw_digits(size_t reg, uint64_t* d, size_t count, bool canonical);
  // engine::get / engine::set form (engine.h:24-25): canonical value | width << 32 -- only for sizes whose words have at most 32 bits
  void get_digits(size_t reg, uint64_t* d, size_t count) override;
  void set_digits(size_t reg, const uint64_t* d, size_t count) override;
  void set_words(size_t reg, const uint32_t* w, size_t count) override;
  void get_words(size_t reg, uint32_t* w, size_t count) override;
  uint64_t res64(size_t reg) override;
  // raw register images (engine.h:134-146): 12 bytes per word + an 8-byte tag (kind + layout fingerprint); a residue uses the first 8 n bytes (digits), a
  // multiplicand all 12 n (its packed spectrum).  Implementation-defined, as the reference's images are.
  size_t register_data_size() const override;
  void get_data(size_t src, void* data, size_t size) override;
  void set_data(size_t dst, const void* data, size_t size) override;
  void check_data(const void* data, size_t size) const override;
  void sync() override;
  // every iteration is bracketed by events; this family has no deferred subtraction (sub must be 0)
  void time_square_mul(size_t reg, uint32_t a, uint32_t sub, size_t iters, double* total_ms, double* kernel_ms, size_t kernel_count) override;
  size_t kernel_count() const override { return kKernels; }
  const char* kernel_name(size_t k) const override { return stage_name(k); }

 private:
  struct Impl;
  std::unique_ptr<Impl> im_;
  bool holds_image(size_t reg) const override;
  uint64_t data_tag(bool image) const;                    // the tag word of this engine's raw images (plan.hpp layout_tag)
  void ensure_headroom(size_t reg);                       // relax a register whose additions would overflow the next transform
  uint64_t* canon_digits(size_t reg, int slot);           // device-side canonical form (canon.hip), slot 0 / 1
  bool canon_flags_ok(uint32_t (&flags)[4]);
  const uint64_t* canonical_on_device(size_t src);        // canonical digits of src in device memory (slot 1)
  void get_digits_host(size_t reg, uint64_t* d);          // read-back + host carry (fallback, MI355_HOST_CARRY=1: host_digits.hpp)
  void launch_transform(size_t reg, int mode, size_t other, uint32_t a, bool timed);
};

}  // namespace mi355
