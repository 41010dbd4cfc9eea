// engine_hip: the reference's `engine` interface (include/marin/engine.h) served by
// libmi355_engine.so through its C ABI (include/mi355_engine.h).  Header-only, dlopen-based, written
// after the reference's own plugin adapter (src/aevum/EngineAevum.cpp:75-82,225-243,252-493):
// same load order (environment variable, then next to the executable / cwd), same error policy
// (0 from the ABI -> std::runtime_error("MI355 <op> failed: <last_error>"), EngineAevum.cpp:477-485).
//
// Drop-in hook: in src/marin/gpu.cpp:149 replace
//     return new engine_gpu(q, reg_count, device, verbose);
// by
//     return new engine_hip(q, reg_count, device, verbose);
// so that `-engine-marin` selects this backend.
#pragma once
#ifdef MI355_USE_REFERENCE_ENGINE_H
#include "marin/engine.h"
#else
#include "engine_iface.h"
#endif

#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

class engine_hip final : public engine {
  struct Api {
    void* so = nullptr;
    const char* (*version)() = nullptr;
    const char* (*last_error)() = nullptr;
    void* (*create)(uint32_t, size_t, uint32_t, int, const char*, const char*) = nullptr;
    void (*destroy)(void*) = nullptr;
    size_t (*transform_size)(void*) = nullptr;
    size_t (*word_count)(void*) = nullptr;
    int (*sync)(void*) = nullptr;
    int (*set_u32)(void*, size_t, uint32_t) = nullptr;
    int (*copy)(void*, size_t, size_t) = nullptr;
    int (*prepare)(void*, size_t, size_t) = nullptr;
    int (*square_mul)(void*, size_t, uint32_t) = nullptr;
    int (*mul)(void*, size_t, size_t, uint32_t) = nullptr;
    int (*add)(void*, size_t, size_t) = nullptr;
    int (*sub_reg)(void*, size_t, size_t) = nullptr;
    int (*sub_u32)(void*, size_t, uint32_t) = nullptr;
    int (*equal)(void*, size_t, size_t, int*) = nullptr;
    int (*get_digits)(void*, size_t, uint64_t*, size_t) = nullptr;
    int (*set_digits)(void*, size_t, const uint64_t*, size_t) = nullptr;
    size_t (*register_data_size)(void*) = nullptr;
    int (*get_data)(void*, size_t, void*, size_t) = nullptr;
    int (*set_data)(void*, size_t, const void*, size_t) = nullptr;
    size_t (*checkpoint_size)(void*) = nullptr;
    int (*get_checkpoint)(void*, void*, size_t) = nullptr;
    int (*set_checkpoint)(void*, const void*, size_t) = nullptr;
    int (*addsub)(void*, size_t, size_t, size_t, size_t) = nullptr;
    int (*addsub_copy)(void*, size_t, size_t, size_t, size_t, size_t, size_t) = nullptr;
    int (*mul_add)(void*, size_t, size_t, size_t, uint32_t) = nullptr;
    int (*square_mul_copy)(void*, size_t, size_t, uint32_t) = nullptr;
    int (*mul_copy)(void*, size_t, size_t, size_t, uint32_t) = nullptr;
    int (*square_mul_n)(void*, size_t, uint32_t, size_t, uint32_t) = nullptr;   // optional (libraries before round 3 lack it)
    // optional as well (a library or test shim without them is served by the compositions below)
    int (*set_words)(void*, size_t, const uint32_t*, size_t) = nullptr;
    int (*get_words)(void*, size_t, uint32_t*, size_t) = nullptr;
    int (*exp_mul)(void*, size_t, uint64_t, size_t, size_t) = nullptr;
    int (*exp_mul2)(void*, size_t, uint64_t, size_t, size_t) = nullptr;
    int (*mul_sum)(void*, size_t, size_t, size_t, size_t) = nullptr;
    int (*mul_sum_is_fused)(void*) = nullptr;
    int (*square_mul_bits)(void*, size_t, uint32_t, const uint8_t*, size_t) = nullptr;
    int (*square_mul_prepare)(void*, size_t, size_t, uint32_t) = nullptr;
    int (*square_mul_prepare_is_fused)(void*) = nullptr;

    template <class F> void bind(F& f, const char* name) {
      f = reinterpret_cast<F>(dlsym(so, name));
      if (!f) throw std::runtime_error(std::string("libmi355_engine.so lacks symbol ") + name);
    }
    explicit Api(const std::string& hint) {
      std::vector<std::string> cand;
      if (const char* e = std::getenv("MI355_ENGINE_LIB")) cand.push_back(e);
      if (!hint.empty()) cand.push_back(hint);
      cand.push_back("./libmi355_engine.so");
      cand.push_back("libmi355_engine.so");
      cand.push_back("/usr/local/lib/prmers/libmi355_engine.so");
      std::string tried;
      for (const auto& c : cand) {
        so = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (so) break;
        tried += " " + c;
      }
      if (!so) throw std::runtime_error("cannot load libmi355_engine.so (tried:" + tried + ")");
      bind(version, "mi355_engine_version"); bind(last_error, "mi355_engine_last_error");
      bind(create, "mi355_engine_create"); bind(destroy, "mi355_engine_destroy");
      bind(transform_size, "mi355_engine_transform_size"); bind(word_count, "mi355_engine_word_count");
      bind(sync, "mi355_engine_sync"); bind(set_u32, "mi355_engine_set_u32"); bind(copy, "mi355_engine_copy");
      bind(prepare, "mi355_engine_prepare"); bind(square_mul, "mi355_engine_square_mul"); bind(mul, "mi355_engine_mul");
      bind(add, "mi355_engine_add"); bind(sub_reg, "mi355_engine_sub_reg"); bind(sub_u32, "mi355_engine_sub_u32");
      bind(equal, "mi355_engine_equal"); bind(get_digits, "mi355_engine_get_digits"); bind(set_digits, "mi355_engine_set_digits");
      bind(register_data_size, "mi355_engine_register_data_size"); bind(get_data, "mi355_engine_get_data");
      bind(set_data, "mi355_engine_set_data"); bind(checkpoint_size, "mi355_engine_checkpoint_size");
      bind(get_checkpoint, "mi355_engine_get_checkpoint"); bind(set_checkpoint, "mi355_engine_set_checkpoint");
      bind(addsub, "mi355_engine_addsub"); bind(addsub_copy, "mi355_engine_addsub_copy"); bind(mul_add, "mi355_engine_mul_add");
      bind(square_mul_copy, "mi355_engine_square_mul_copy"); bind(mul_copy, "mi355_engine_mul_copy");
      square_mul_n = reinterpret_cast<decltype(square_mul_n)>(dlsym(so, "mi355_engine_square_mul_n"));
      set_words = reinterpret_cast<decltype(set_words)>(dlsym(so, "mi355_engine_set_words"));
      get_words = reinterpret_cast<decltype(get_words)>(dlsym(so, "mi355_engine_get_words"));
      exp_mul = reinterpret_cast<decltype(exp_mul)>(dlsym(so, "mi355_engine_exp_mul"));
      exp_mul2 = reinterpret_cast<decltype(exp_mul2)>(dlsym(so, "mi355_engine_exp_mul2"));
      mul_sum = reinterpret_cast<decltype(mul_sum)>(dlsym(so, "mi355_engine_mul_sum"));
      mul_sum_is_fused = reinterpret_cast<decltype(mul_sum_is_fused)>(dlsym(so, "mi355_engine_mul_sum_is_fused"));
      square_mul_bits = reinterpret_cast<decltype(square_mul_bits)>(dlsym(so, "mi355_engine_square_mul_bits"));
      square_mul_prepare = reinterpret_cast<decltype(square_mul_prepare)>(dlsym(so, "mi355_engine_square_mul_prepare"));
      square_mul_prepare_is_fused = reinterpret_cast<decltype(square_mul_prepare_is_fused)>(dlsym(so, "mi355_engine_square_mul_prepare_is_fused"));
    }
    ~Api() { if (so) dlclose(so); }
  };

  Api _api;
  void* _h = nullptr;
  size_t _n = 0;

  void ok(int rc, const char* op) const {
    if (!rc) throw std::runtime_error(std::string("MI355 ") + op + " failed: " + _api.last_error());
  }
  void exp_mul_any(const Reg a, const uint64_t h, const Reg b, const Reg tmp, const bool square_b) const {
    if (auto f = square_b ? _api.exp_mul2 : _api.exp_mul) { ok(f(_h, a, h, b, tmp), square_b ? "exp_mul2" : "exp_mul"); return; }
    if (a == b || a == tmp || b == tmp) throw std::runtime_error("MI355 exp_mul failed: a, b and tmp must be three different registers");
    if (square_b) square_mul(b);
    if (h == 0) copy(a, b);
    set_multiplicand(tmp, a);
    int top = 63;
    while (top > 0 && !((h >> top) & 1)) --top;
    for (int i = top - 1; i >= 0 && h != 0; --i) { square_mul(a); if ((h >> i) & 1) mul(a, tmp); }
    set_multiplicand(b, b);
    if (h != 0) mul(a, b);
  }

 protected:
  void get(uint64_t* const d, const size_t src) const override { ok(_api.get_digits(_h, src, d, _n), "get"); }
  void set(const size_t dst, uint64_t* const d) const override { ok(_api.set_digits(_h, dst, d, _n), "set"); }

 public:
  // fft_spec: "" = the Goldilocks path with its automatic plan, "m2=..,c=.." a forced plan, "crt[:odd][:words=N]" the
  // GF(M61^2) x GF(M31^2) family with a prime-factor axis (the reference hands its -fft string to its plugin the same way,
  // src/aevum/EngineAevum.cpp:252-300)
  engine_hip(const uint32_t q, const size_t reg_count, const size_t device, const bool verbose, const std::string& lib_hint = "",
             const std::string& fft_spec = "")
      : _api(lib_hint) {
    _h = _api.create(q, reg_count, uint32_t(device), verbose ? 1 : 0, fft_spec.empty() ? nullptr : fft_spec.c_str(), nullptr);
    if (!_h) throw std::runtime_error(std::string("MI355 create failed: ") + _api.last_error());
    _n = _api.transform_size(_h);
  }
  ~engine_hip() override { if (_h) _api.destroy(_h); }
  engine_hip(const engine_hip&) = delete;
  engine_hip& operator=(const engine_hip&) = delete;

  size_t get_size() const override { return _n; }
  void sync() const override { ok(_api.sync(_h), "sync"); }
  void set(const Reg dst, const uint32_t a) const override { ok(_api.set_u32(_h, dst, a), "set"); }
  void copy(const Reg dst, const Reg src) const override { ok(_api.copy(_h, dst, src), "copy"); }
  void square_mul(const Reg src, const uint32_t a = 1) const override { ok(_api.square_mul(_h, src, a), "square_mul"); }
  void set_multiplicand(const Reg dst, const Reg src) const override { ok(_api.prepare(_h, dst, src), "set_multiplicand"); }
  void mul(const Reg dst, const Reg src, const uint32_t a = 1) const override { ok(_api.mul(_h, dst, src, a), "mul"); }
  void sub(const Reg src, const uint32_t a) const override { ok(_api.sub_u32(_h, src, a), "sub"); }
  void add(const Reg dst, const Reg src) const override { ok(_api.add(_h, dst, src), "add"); }
  void sub_reg(const Reg dst, const Reg src) const override { ok(_api.sub_reg(_h, dst, src), "sub_reg"); }
  // count x { src = src^2 * a; src -= sub }: the run of plain iterations of the callers' loops (RunPrpOrLlMarin.cpp:338-409) as one call;
  // not part of the reference's engine (a non-virtual extra of this adapter), the loop of calls when the library does not export it
  void square_mul_n(const Reg src, const size_t count, const uint32_t a = 1, const uint32_t sub_after = 0) const {
    if (_api.square_mul_n) { ok(_api.square_mul_n(_h, src, a, count, sub_after), "square_mul_n"); return; }
    for (size_t i = 0; i < count; ++i) { square_mul(src, a); if (sub_after) sub(src, sub_after); }
  }
  // a = a^h * b (exp_mul) / a^h * b^2 (exp_mul2): the fold of a PRP proof (PRPLL's expMul / expMul2) as one library call; b and tmp are
  // consumed.  Not part of the reference's engine; the composition of its operations when the library does not export them.
  void exp_mul(const Reg a, const uint64_t h, const Reg b, const Reg tmp) const { exp_mul_any(a, h, b, tmp, false); }
  void exp_mul2(const Reg a, const uint64_t h, const Reg b, const Reg tmp) const { exp_mul_any(a, h, b, tmp, true); }
  // The P-1 operations (prmers_amd/pm1.py), non-virtual extras like square_mul_n: the compositions when the library does not export them.
  // dst = dst * (a + b) for two multiplicand images (left intact; tmp is scratch): one product where the plan's capacity allows it
  void mul_sum(const Reg dst, const Reg src_a, const Reg src_b, const Reg tmp) const {
    if (_api.mul_sum) { ok(_api.mul_sum(_h, dst, src_a, src_b, tmp), "mul_sum"); return; }
    if (dst == tmp || dst == src_a || dst == src_b || tmp == src_a || tmp == src_b) throw std::runtime_error("MI355 mul_sum failed: dst, tmp and the multiplicands must differ");
    copy(tmp, dst); mul(dst, src_a); mul(tmp, src_b); add(dst, tmp);
  }
  bool mul_sum_is_fused() const { return _api.mul_sum_is_fused && _api.mul_sum_is_fused(_h) != 0; }
  // src = src^(2^nbits) * a^B, B the nbits bits of `bits` (most significant first, packed in bytes): one square_mul per bit in one call
  void square_mul_bits(const Reg src, const uint32_t a, const uint8_t* bits, const size_t nbits) const {
    if (_api.square_mul_bits) { ok(_api.square_mul_bits(_h, src, a, bits, nbits), "square_mul_bits"); return; }
    for (size_t i = 0; i < nbits; ++i) square_mul(src, ((bits[i >> 3] >> (7 - (i & 7))) & 1) ? a : 1u);
  }
  // The ECM operation (prmers_amd/ecm.py): img_out = the multiplicand image of src, then src = src^2 * a -- one squaring whose row sweep
  // keeps the transform of its operand; set_multiplicand + square_mul when the library does not export it
  void square_mul_prepare(const Reg src, const Reg img_out, const uint32_t a = 1) const {
    if (_api.square_mul_prepare) { ok(_api.square_mul_prepare(_h, src, img_out, a), "square_mul_prepare"); return; }
    if (src == img_out) throw std::runtime_error("MI355 square_mul_prepare failed: img_out must differ from src");
    set_multiplicand(img_out, src); square_mul(src, a);
  }
  bool square_mul_prepare_is_fused() const { return _api.square_mul_prepare_is_fused && _api.square_mul_prepare_is_fused(_h) != 0; }
  // the canonical residue as ceil(p / 32) little-endian words (2^p - 1 reads as 0) / a register from such words: packed and cut on the
  // device by the library, through the digit vector when it does not export the word entry points
  std::vector<uint32_t> get_words(const Reg src) const {
    if (_api.get_words && _api.word_count) {
      std::vector<uint32_t> w(_api.word_count(_h));
      ok(_api.get_words(_h, src, w.data(), w.size()), "get_words");
      return w;
    }
    std::vector<uint64_t> d(_n);
    get(d.data(), src);
    size_t bits = 0;
    bool ones = true;
    for (uint64_t v : d) { bits += size_t(v >> 32); ones = ones && uint32_t(v) == (uint64_t(1) << (v >> 32)) - 1; }
    std::vector<uint32_t> w((bits + 31) / 32, 0u);
    if (ones) return w;
    size_t bit = 0;
    for (uint64_t v : d) {
      const uint64_t x = uint64_t(uint32_t(v)) << (bit % 32);
      w[bit / 32] |= uint32_t(x);
      if (bit / 32 + 1 < w.size()) w[bit / 32 + 1] |= uint32_t(x >> 32);
      bit += size_t(v >> 32);
    }
    return w;
  }
  void set_words(const Reg dst, const std::vector<uint32_t>& w) const {
    if (_api.set_words) { ok(_api.set_words(_h, dst, w.data(), w.size()), "set_words"); return; }
    std::vector<uint64_t> d(_n);
    get(d.data(), dst);   // the widths
    size_t bit = 0;
    for (uint64_t& v : d) {
      const unsigned width = unsigned(v >> 32);
      const size_t i = bit / 32;
      uint64_t u = (i < w.size() ? w[i] : 0u) >> (bit % 32);
      if (bit % 32) u |= uint64_t(i + 1 < w.size() ? w[i + 1] : 0u) << (32 - bit % 32);
      v = (u & ((uint64_t(1) << width) - 1)) | (uint64_t(width) << 32);
      bit += width;
    }
    set(dst, d.data());
  }
  // fused variants: one sweep each in the library instead of the base-class compositions (engine.h:65-131)
  void mul_add(const Reg dst, const Reg mul_src, const Reg add_src, const uint32_t a = 1) const override { ok(_api.mul_add(_h, dst, mul_src, add_src, a), "mul_add"); }
  void addsub(const Reg sum_out, const Reg diff_out, const Reg a, const Reg b) const override { ok(_api.addsub(_h, sum_out, diff_out, a, b), "addsub"); }
  void square_mul_copy(const Reg src, const Reg dst_copy, const uint32_t a = 1) const override { ok(_api.square_mul_copy(_h, src, dst_copy, a), "square_mul_copy"); }
  void mul_copy(const Reg dst, const Reg src, const Reg dst_copy, const uint32_t a = 1) const override { ok(_api.mul_copy(_h, dst, src, dst_copy, a), "mul_copy"); }
  void addsub_copy(const Reg sum, const Reg diff, const Reg sum_copy, const Reg diff_copy, const Reg a, const Reg b) const override {
    ok(_api.addsub_copy(_h, sum, diff, sum_copy, diff_copy, a, b), "addsub_copy");
  }
  bool is_equal(const Reg lhs, const Reg rhs) const
#if defined(MI355_HAVE_GMP) || defined(MI355_USE_REFERENCE_ENGINE_H)
      override
#endif
  { int eq = 0; ok(_api.equal(_h, lhs, rhs, &eq), "is_equal"); return eq != 0; }

  size_t get_register_data_size() const override { return _api.register_data_size(_h); }
  bool get_data(std::vector<char>& data, const Reg src) const override {   // false on size mismatch (engine_gpu.h:2138)
    return data.size() == get_register_data_size() && _api.get_data(_h, src, data.data(), data.size()) != 0;
  }
  bool set_data(const Reg dst, const std::vector<char>& data) const override {
    return data.size() == get_register_data_size() && _api.set_data(_h, dst, data.data(), data.size()) != 0;
  }
  size_t get_checkpoint_size() const override { return _api.checkpoint_size(_h); }
  bool get_checkpoint(std::vector<char>& data) const override {
    return data.size() == get_checkpoint_size() && _api.get_checkpoint(_h, data.data(), data.size()) != 0;
  }
  bool set_checkpoint(const std::vector<char>& data) const override {
    return data.size() == get_checkpoint_size() && _api.set_checkpoint(_h, data.data(), data.size()) != 0;
  }
};
