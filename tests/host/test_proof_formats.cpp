// The proof layer of include/mi355/caller_formats.h without a GPU (tests/test_proof.py drives it):
//   sha3 N                      SHA3-256 of the N bytes (i * 7 + 1) mod 256, as hex
//   points P POWER DIR          the proof points, and the residues 3^(2^i) written there through ProofPoints::save
//   build P POWER DIR OUT       build_proof on a GMP-backed stand-in engine from the point files under DIR, saved to OUT
//   verify FILE                 exit code 0: the proof verifies on the stand-in, 1: it does not (or does not load)
#include <gmp.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mi355/caller_formats.h"

namespace fmt = mi355::formats;

// the six operations build_proof / verify_proof use, on mpz residues mod 2^p - 1
class GmpEngine {
 public:
  GmpEngine(uint32_t p, size_t regs) : p_(p), r_(regs) {
    for (auto& z : r_) mpz_init(z.v);
    mpz_init(m_); mpz_init(t_);
    mpz_setbit(m_, p); mpz_sub_ui(m_, m_, 1);
  }
  ~GmpEngine() { for (auto& z : r_) mpz_clear(z.v); mpz_clear(m_); mpz_clear(t_); }
  GmpEngine(const GmpEngine&) = delete;
  void set_words(size_t reg, const std::vector<uint32_t>& w) { mpz_import(r_.at(reg).v, w.size(), -1, 4, -1, 0, w.data()); }
  std::vector<uint32_t> get_words(size_t reg) {
    mpz_mod(t_, r_.at(reg).v, m_);
    std::vector<uint32_t> w((size_t(p_) + 31) / 32, 0u);
    size_t count = 0;
    mpz_export(w.data(), &count, -1, 4, -1, 0, t_);
    return w;
  }
  void exp_mul(size_t a, uint64_t h, size_t b, size_t tmp) { fold(a, h, b, tmp, false); }
  void exp_mul2(size_t a, uint64_t h, size_t b, size_t tmp) { fold(a, h, b, tmp, true); }
  void square_mul_n(size_t reg, size_t count) {
    for (size_t i = 0; i < count; ++i) { mpz_mul(t_, r_.at(reg).v, r_.at(reg).v); mpz_mod(r_.at(reg).v, t_, m_); }
  }
  bool is_equal(size_t a, size_t b) {
    mpz_mod(r_.at(a).v, r_.at(a).v, m_); mpz_mod(r_.at(b).v, r_.at(b).v, m_);
    return mpz_cmp(r_.at(a).v, r_.at(b).v) == 0;
  }

 private:
  struct Z { mpz_t v; };
  void fold(size_t a, uint64_t h, size_t b, size_t tmp, bool square) {
    if (a == b || a == tmp || b == tmp) throw std::runtime_error("exp_mul: registers must differ");
    if (square) { mpz_mul(t_, r_.at(b).v, r_.at(b).v); mpz_mod(r_.at(b).v, t_, m_); }
    if (h == 0) { mpz_set(r_.at(a).v, r_.at(b).v); return; }
    mpz_t e; mpz_init(e);
    mpz_import(e, 1, -1, 8, 0, 0, &h);
    mpz_powm(t_, r_.at(a).v, e, m_);
    mpz_clear(e);
    mpz_mul(t_, t_, r_.at(b).v);
    mpz_mod(r_.at(a).v, t_, m_);
    mpz_set_ui(r_.at(b).v, 0); mpz_set_ui(r_.at(tmp).v, 0);   // consumed
  }
  uint32_t p_;
  std::vector<Z> r_;
  mpz_t m_, t_;
};

int main(int argc, char** argv) {
  try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "sha3" && argc == 3) {
      const size_t n = std::strtoul(argv[2], nullptr, 10);
      std::vector<unsigned char> data(n);
      for (size_t i = 0; i < n; ++i) data[i] = static_cast<unsigned char>(i * 7 + 1);
      fmt::Sha3_256 h;
      // in two pieces, so that the streaming path is exercised too
      h.update(data.data(), n / 3).update(data.data() + n / 3, n - n / 3);
      for (unsigned char c : h.finish()) std::printf("%02x", c);
      std::printf("\n");
      return 0;
    }
    if (cmd == "points" && argc == 5) {
      const uint32_t p = uint32_t(std::strtoul(argv[2], nullptr, 10)), power = uint32_t(std::strtoul(argv[3], nullptr, 10));
      const fmt::ProofPoints pts(p, power, argv[4]);
      GmpEngine e(p, 1);
      std::vector<uint32_t> w((size_t(p) + 31) / 32, 0u);
      w[0] = 3;
      e.set_words(0, w);
      for (uint32_t it = 1; it <= p; ++it) {
        e.square_mul_n(0, 1);
        if (pts.should_checkpoint(it) && !pts.save(it, e.get_words(0))) return 3;
      }
      for (uint32_t pt : pts.points()) std::printf("%u ", pt);
      std::printf("\n");
      return 0;
    }
    if (cmd == "build" && argc == 6) {
      const uint32_t p = uint32_t(std::strtoul(argv[2], nullptr, 10)), power = uint32_t(std::strtoul(argv[3], nullptr, 10));
      GmpEngine e(p, power + 1);
      const fmt::Proof pr = fmt::build_proof(e, p, power, argv[4], stdout);
      return pr.save(argv[5]) ? 0 : 3;
    }
    if (cmd == "verify" && argc == 3) {
      fmt::Proof pr;
      try { pr = fmt::Proof::load(argv[2]); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
      GmpEngine e(pr.p, fmt::kProofVerifyRegisters);
      return fmt::verify_proof(e, pr) ? 0 : 1;
    }
    std::fprintf(stderr, "usage: sha3 N | points P POWER DIR | build P POWER DIR OUT | verify FILE\n");
    return 2;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "Error: %s\n", e.what());
    return 2;
  }
}
