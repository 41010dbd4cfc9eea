// Host side of RegisterMachine::square_mul_prepare (no GPU): a stub machine of four registers holding small integers modulo 2^p - 1 that
// logs every primitive it runs.  The default composition must refuse a bad call before any primitive runs, and on a good call run
// set_multiplicand(img_out, src) then square_mul(src, factor).  Prints "OK" or the first failure.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "register_machine.hpp"

namespace {

struct Stub final : mi355::RegisterMachine {
  static constexpr uint64_t kMp = (uint64_t(1) << 31) - 1;
  std::vector<uint64_t> val = std::vector<uint64_t>(4, 0);
  std::vector<bool> img = std::vector<bool>(4, false);
  std::string log;

  uint32_t exponent() const override { return 31; }
  size_t size() const override { return 4; }
  size_t reg_count() const override { return val.size(); }
  std::string describe() const override { return "stub"; }
  size_t algorithmic_bytes() const override { return 0; }
  void sync() override {}
  void set_u32(size_t dst, uint32_t v) override { val[dst] = v % kMp; img[dst] = false; }
  void copy(size_t dst, size_t src) override { val[dst] = val[src]; img[dst] = img[src]; }
  void square_mul(size_t r, uint32_t f) override { log += "Q" + std::to_string(r) + "*" + std::to_string(f) + ";"; val[r] = val[r] * val[r] % kMp * f % kMp; }
  void set_multiplicand(size_t dst, size_t src) override { log += "P" + std::to_string(dst) + "<" + std::to_string(src) + ";"; val[dst] = val[src]; img[dst] = true; }
  void mul(size_t dst, size_t src, uint32_t f) override { log += "M;"; val[dst] = val[dst] * val[src] % kMp * f % kMp; }
  void add(size_t, size_t) override { log += "A;"; }
  void sub_reg(size_t, size_t) override { log += "S;"; }
  void sub_u32(size_t, uint32_t) override { log += "s;"; }
  bool equal(size_t a, size_t b) override { return val[a] == val[b]; }
  void addsub(long, long, long, long, size_t, size_t) override { log += "L;"; }
  void set_digits(size_t, const uint64_t*, size_t) override {}
  void get_digits(size_t, uint64_t*, size_t) override {}
  void set_words(size_t, const uint32_t*, size_t) override {}
  void get_words(size_t, uint32_t*, size_t) override {}
  uint64_t res64(size_t r) override { return val[r]; }
  size_t register_data_size() const override { return 8; }
  void get_data(size_t, void*, size_t) override {}
  void set_data(size_t, const void*, size_t) override {}
  void time_square_mul(size_t, uint32_t, uint32_t, size_t, double*, double*, size_t) override {}
  size_t kernel_count() const override { return 0; }
  const char* kernel_name(size_t) const override { return ""; }
  bool holds_image(size_t r) const override { return img[r]; }
};

int fail(const char* what) { std::printf("FAIL: %s\n", what); return 1; }

// the call must throw, and neither run a primitive nor change a register
bool refused(Stub& m, size_t src, size_t out, uint32_t f) {
  const std::vector<uint64_t> v0 = m.val;
  const std::vector<bool> i0 = m.img;
  m.log.clear();
  try { m.square_mul_prepare(src, out, f); } catch (const std::runtime_error& e) {
    return m.log.empty() && m.val == v0 && m.img == i0 && std::strstr(e.what(), "square_mul_prepare") != nullptr;
  }
  return false;
}

}  // namespace

int main() {
  Stub m;
  m.set_u32(0, 5); m.set_u32(1, 7); m.set_u32(2, 11); m.set_multiplicand(2, 2); m.set_u32(3, 13);
  if (m.square_mul_prepare_is_fused()) return fail("the default composition calls itself fused");
  if (!refused(m, 0, 0, 1)) return fail("src == img_out was not refused cleanly");
  if (!refused(m, 2, 1, 1)) return fail("an image as src was not refused cleanly");
  if (!refused(m, 0, 1, 0)) return fail("factor 0 was not refused cleanly");
  if (!refused(m, 0, 4, 1)) return fail("img_out out of range was not refused cleanly");
  if (!refused(m, 4, 1, 1)) return fail("src out of range was not refused cleanly");
  if (!refused(m, size_t(-1), 1, 1)) return fail("src = -1 was not refused cleanly");
  m.log.clear();
  m.square_mul_prepare(0, 2, 3);   // img_out held an image before
  if (m.log != "P2<0;Q0*3;") return fail("the composition is not set_multiplicand(img_out, src); square_mul(src, factor)");
  if (m.val[0] != 75 || m.val[2] != 5 || !m.img[2] || m.img[0]) return fail("wrong values or kinds after the composition");
  m.log.clear();
  m.square_mul_prepare(1, 3, 1);   // img_out held a residue before
  if (m.log != "P3<1;Q1*1;" || m.val[1] != 49 || m.val[3] != 7 || !m.img[3]) return fail("second call");
  std::printf("OK\n");
  return 0;
}
