// Caller-side formats around the engine boundary, in C++: what the reference's PRP / LL driver reads and
// writes next to the squaring loop, so that a run on the MI355X engine leaves the files a PrMers user expects.
//   * checkpoint file, version 2, CRC trailer      -- src/modes/RunPrpOrLlMarin.cpp:150-211, include/marin/file.h:40-111
//   * worktodo.txt entries and their rotation      -- src/io/WorktodoParser.cpp:78-400,402-427, RunPrpOrLlMarin.cpp:727-751
//   * result line (PrimeNet-style JSON)            -- src/io/JsonBuilder.cpp:322-472
//   * PRP proof checkpoints (residue files)        -- src/core/ProofSetMarin.cpp:56-122,156-158, ProofManagerMarin.cpp:84-120
//   * PRP proof file, hash chain, build / verify   -- src/core/ProofMarin.cpp:33-217, ProofSetMarin.cpp:213-311
//   * words / type-1 residue / hex                  -- include/core/AlgoUtils.hpp:165-223
// Header-only, no dependency on the engine library: everything works on an `engine` (include/mi355/engine_iface.h or the
// reference's include/marin/engine.h) or on plain vectors, so it is testable without a GPU (tests/host/test_caller_formats.cpp).
// Formats are the reference's; the code is not (nothing here is copied: same bytes on disk, different implementation).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include "../mi355_engine.h"
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace mi355 {
namespace formats {

// ---- CRC-32 (reflected 0xEDB88320), as file.h:60-84 and ProofSetMarin's computeCRC32 use it -------------------------
inline uint32_t crc32_update(uint32_t crc, const void* data, size_t len) {
  static uint32_t table[256];
  static bool ready = false;
  if (!ready) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t r = i;
      for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ 0xedb88320u : r >> 1;
      table[i] = r;
    }
    ready = true;
  }
  const unsigned char* p = static_cast<const unsigned char*>(data);
  uint32_t c = ~crc;
  for (size_t i = 0; i < len; ++i) c = (c >> 8) ^ table[(c ^ p[i]) & 0xffu];
  return ~c;
}

// ---- residue words (AlgoUtils.hpp:165-223) ---------------------------------------------------------------------------
// digits[i] = value | width << 32 (engine::get): little-endian 32-bit words of the p-bit residue
inline std::vector<uint32_t> pack_words(const std::vector<uint64_t>& digits, uint32_t p) {
  std::vector<uint32_t> out((size_t(p) + 31) / 32, 0u);
  size_t bit = 0;
  for (uint64_t d : digits) {
    const unsigned w = unsigned(d >> 32);
    uint64_t v = uint32_t(d);
    if (w < 32) v &= (uint64_t(1) << w) - 1;
    const size_t i = bit / 32, s = bit % 32;
    if (i < out.size()) {
      const uint64_t x = v << s;
      out[i] |= uint32_t(x);
      if (i + 1 < out.size()) out[i + 1] |= uint32_t(x >> 32);
    }
    bit += w;
  }
  return out;
}
// x / 3 mod 2^p - 1 on the word vector (the residue plus the right multiple of Mp is divisible by 3)
inline void div3_words(uint32_t p, std::vector<uint32_t>& W) {
  uint32_t r3 = 0;
  for (uint32_t w : W) r3 = (r3 + w % 3) % 3;
  uint32_t rem = (3 - r3) % 3;   // Mp == 1 (mod 3) for odd p: adding rem * Mp makes the value divisible by 3; rem * 2^p enters at the top
  const unsigned top = p % 32;
  for (size_t i = W.size(); i-- > 0;) {
    const uint64_t t = (uint64_t(rem) << ((i + 1 == W.size()) ? top : 32)) + W[i];   // the top word holds p mod 32 bits
    W[i] = uint32_t(t / 3);
    rem = uint32_t(t % 3);
  }
}
inline void prp3_div9(uint32_t p, std::vector<uint32_t>& W) { div3_words(p, W); div3_words(p, W); }   // type-1 residue of a base-3 PRP
inline std::string res64_hex(const std::vector<uint32_t>& W) {
  const uint64_t r = (uint64_t(W.size() > 1 ? W[1] : 0) << 32) | (W.empty() ? 0u : W[0]);
  char buf[24];
  std::snprintf(buf, sizeof buf, "%016llX", static_cast<unsigned long long>(r));
  return buf;
}
inline std::string res2048_hex(const std::vector<uint32_t>& W) {
  std::string s;
  char buf[12];
  for (int i = 63; i >= 0; --i) { std::snprintf(buf, sizeof buf, "%08x", size_t(i) < W.size() ? W[size_t(i)] : 0u); s += buf; }
  return s;
}

// ---- checkpoint file (RunPrpOrLlMarin.cpp:190-211): int version = 2, u32 p, u32 mode (1 PRP / 2 LL), u32 backend,
//      u32 iteration, double elapsed, the engine's checkpoint image, u32 (~crc ^ 0xa23777ac) over everything before it ----
constexpr uint32_t kBackendMarinOpenCL = 1, kBackendAevum = 2, kBackendMi355 = 3;   // images are backend-specific (:166-170)
inline std::string checkpoint_name(uint32_t p, bool ll, const std::string& dir = ".") {
  return (std::filesystem::path(dir) / (std::string(ll ? "llunsafe_" : "") + "m_" + std::to_string(p) + ".ckpt")).string();
}
template <class Engine>
bool save_checkpoint(const std::string& path, const Engine& eng, uint32_t p, bool ll, uint32_t iteration, double elapsed) {
  std::vector<char> image(eng.get_checkpoint_size());
  if (!eng.get_checkpoint(image)) return false;
  const std::string fresh = path + ".new", old = path + ".old";
  {
    std::ofstream f(fresh, std::ios::binary);
    if (!f) return false;
    uint32_t crc = 0;
    auto put = [&](const void* d, size_t n) { f.write(static_cast<const char*>(d), std::streamsize(n)); crc = crc32_update(crc, d, n); };
    const int version = 2;
    const uint32_t mode = ll ? 2u : 1u, backend = kBackendMi355;
    put(&version, sizeof version); put(&p, 4); put(&mode, 4); put(&backend, 4); put(&iteration, 4); put(&elapsed, sizeof elapsed);
    put(image.data(), image.size());
    const uint32_t trailer = ~crc ^ 0xa23777acu;
    f.write(reinterpret_cast<const char*>(&trailer), 4);
    if (!f.good()) return false;
  }
  std::error_code ec;
  std::filesystem::remove(old, ec);
  if (std::filesystem::exists(path)) std::filesystem::rename(path, old, ec);   // keep the previous one as .old
  std::filesystem::rename(fresh, path, ec);
  return !ec;
}
// 0: loaded (iteration / elapsed set, registers restored); -1: no file; -2: damaged or for another exponent; -3: another mode / backend
template <class Engine>
int load_checkpoint(const std::string& path, const Engine& eng, uint32_t p, bool ll, uint32_t& iteration, double& elapsed) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return -1;
  uint32_t crc = 0;
  auto get = [&](void* d, size_t n) { f.read(static_cast<char*>(d), std::streamsize(n)); if (f.gcount() != std::streamsize(n)) return false; crc = crc32_update(crc, d, n); return true; };
  int version = 0;
  uint32_t rp = 0, mode = 0, backend = 0;
  if (!get(&version, sizeof version) || !get(&rp, 4) || rp != p || version != 2) return -2;
  if (!get(&mode, 4) || !get(&backend, 4)) return -2;
  if (mode != (ll ? 2u : 1u) || backend != kBackendMi355) return -3;
  if (!get(&iteration, 4) || !get(&elapsed, sizeof elapsed)) return -2;
  std::vector<char> image(eng.get_checkpoint_size());
  if (!get(image.data(), image.size())) return -2;
  const uint32_t want = ~crc ^ 0xa23777acu;
  uint32_t trailer = 0;
  f.read(reinterpret_cast<char*>(&trailer), 4);
  if (f.gcount() != 4 || trailer != want) return -2;
  return eng.set_checkpoint(image) ? 0 : -2;
}

// ---- Gerbicz-Li rollback point next to a checkpoint (the reference keeps itersave / jsave in its backup manager and reloads them on
//      a resume, RunPrpOrLlMarin.cpp:251-255).  <ckpt>.gl: u32 magic "GL3R", u32 iteration of the checkpoint it belongs to, u64 itersave,
//      u64 jsave, u64 checkpass, u32 CRC-32 of the 32 bytes before it.  R4 / R5 (the state those counters name) travel in the checkpoint. ----
constexpr uint32_t kGerbiczMagic = 0x474C3352u;
struct GerbiczState { uint64_t itersave = 0, jsave = 0, checkpass = 0; };
inline bool save_gerbicz_state(const std::string& ckpt_path, uint32_t iteration, const GerbiczState& g) {
  unsigned char b[36];
  std::memcpy(b, &kGerbiczMagic, 4); std::memcpy(b + 4, &iteration, 4);
  std::memcpy(b + 8, &g.itersave, 8); std::memcpy(b + 16, &g.jsave, 8); std::memcpy(b + 24, &g.checkpass, 8);
  const uint32_t crc = crc32_update(0, b, 32);
  std::memcpy(b + 32, &crc, 4);
  const std::string fresh = ckpt_path + ".gl.new";
  { std::ofstream f(fresh, std::ios::binary); f.write(reinterpret_cast<const char*>(b), 36); if (!f.good()) return false; }
  // the side file rotates with the checkpoint (<ckpt>.gl.old belongs to <ckpt>.old), so a resume from the older generation -- a torn main
  // checkpoint, or a crash between the two renames -- still finds the rollback point that generation was verified from
  std::error_code ec;
  if (std::filesystem::exists(ckpt_path + ".gl", ec)) std::filesystem::rename(ckpt_path + ".gl", ckpt_path + ".gl.old", ec);
  std::filesystem::rename(fresh, ckpt_path + ".gl", ec);
  return !ec;
}
// the rollback point of the checkpoint written at `iteration`, from whichever generation of the side file names that iteration
inline bool load_gerbicz_state(const std::string& ckpt_path, uint32_t iteration, GerbiczState& g) {
  for (const char* suffix : {".gl", ".gl.old"}) {
    std::ifstream f(ckpt_path + suffix, std::ios::binary);
    unsigned char b[37];
    f.read(reinterpret_cast<char*>(b), 37);
    if (f.gcount() != 36) continue;
    uint32_t magic, it, crc;
    std::memcpy(&magic, b, 4); std::memcpy(&it, b + 4, 4); std::memcpy(&crc, b + 32, 4);
    if (magic != kGerbiczMagic || it != iteration || crc != crc32_update(0, b, 32)) continue;
    std::memcpy(&g.itersave, b + 8, 8); std::memcpy(&g.jsave, b + 16, 8); std::memcpy(&g.checkpass, b + 24, 8);
    return true;
  }
  return false;
}

// ---- worktodo.txt (WorktodoParser.cpp:98-104,331-348): PRP=[aid,]k,b,n,c[,...] / PRPDC= / Test=[aid,]p[,...] / DoubleCheck= ----
struct WorkEntry { bool valid = false; bool ll = false; uint32_t exponent = 0; std::string aid, raw; };
inline WorkEntry parse_worktodo_line(const std::string& line_in) {
  WorkEntry e;
  std::string line = line_in;
  while (!line.empty() && (line.back() == '\r' || line.back() == '\n' || line.back() == ' ')) line.pop_back();
  e.raw = line;
  const size_t eq = line.find('=');
  if (line.empty() || line[0] == '#' || eq == std::string::npos) return e;
  std::string key = line.substr(0, eq);
  std::transform(key.begin(), key.end(), key.begin(), [](unsigned char c) { return char(std::toupper(c)); });
  if (key == "PRP" || key == "PRPDC") e.ll = false;
  else if (key == "TEST" || key == "DOUBLECHECK") e.ll = true;
  else return e;
  std::vector<std::string> parts;
  std::stringstream ss(line.substr(eq + 1));
  for (std::string tok; std::getline(ss, tok, ',');) {
    const size_t a = tok.find_first_not_of(' '), b = tok.find_last_not_of(' ');
    parts.push_back(a == std::string::npos ? std::string() : tok.substr(a, b - a + 1));
  }
  auto is_hex32 = [](const std::string& s) { return s.size() == 32 && s.find_first_not_of("0123456789abcdefABCDEF") == std::string::npos; };
  size_t i = 0;
  if (i < parts.size() && (parts[i].empty() || parts[i] == "N/A")) ++i;
  if (i < parts.size() && (is_hex32(parts[i]) || parts[i] == "AID" || parts[i] == "N/A")) { if (is_hex32(parts[i])) e.aid = parts[i]; ++i; }
  auto is_num = [](const std::string& s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos; };
  if (parts.size() >= i + 4 && parts[i] == "1" && parts[i + 1] == "2" && is_num(parts[i + 2]) && parts[i + 3] == "-1") {
    e.exponent = uint32_t(std::stoul(parts[i + 2])); e.valid = true;           // k,b,n,c = 1,2,p,-1
  } else if (e.ll && i < parts.size() && is_num(parts[i])) {
    e.exponent = uint32_t(std::stoul(parts[i])); e.valid = true;               // Test=p[,how far factored[,P-1 done]]
  }
  return e;
}
inline WorkEntry first_worktodo_entry(const std::string& path) {
  std::ifstream f(path);
  for (std::string l; std::getline(f, l);) { WorkEntry e = parse_worktodo_line(l); if (e.valid) return e; }
  return WorkEntry();
}
// Rotation after a finished entry (removeFirstProcessed, WorktodoParser.cpp:402-427): the first non-empty line moves to
// save_path (appended), the rest stays.  Returns whether another work line remains (the reference then restarts itself).
inline bool rotate_worktodo(const std::string& path, const std::string& save_path, bool* removed = nullptr) {
  std::ifstream in(path);
  std::vector<std::string> keep;
  bool skipped = false;
  std::string first;
  for (std::string l; std::getline(in, l);) {
    if (!skipped && !l.empty()) { skipped = true; first = l; continue; }
    keep.push_back(l);
  }
  in.close();
  if (removed) *removed = skipped;
  if (!skipped) return false;
  { std::ofstream save(save_path, std::ios::app); save << first << "\n"; }
  const std::string tmp = path + ".tmp";
  { std::ofstream out(tmp); for (const auto& l : keep) out << l << "\n"; }
  std::error_code ec;
  std::filesystem::rename(tmp, path, ec);
  for (const auto& l : keep) if (!l.empty() && l[0] != '#') return true;
  return false;
}

// ---- result line (JsonBuilder.cpp:322-472: key order of the PRP / LL work types) ----------------------------------------
struct ResultInfo {
  uint32_t exponent = 0; bool ll = false, is_prime = false;
  std::string res64, res2048; unsigned gerbicz_errors = 0, fft_length = 0;
  std::string program_version = "mi355-marin-hip " MI355_ENGINE_VERSION, os_name = "Linux", os_arch = "x86_64", user, computer, aid, timestamp;
  unsigned port = 8;
};
inline std::string json_escape(const std::string& s) {
  std::string o = "\"";
  for (char c : s) { if (c == '"' || c == '\\') { o += '\\'; o += c; } else if (c == '\n') o += "\\n"; else o += c; }
  return o + "\"";
}
inline std::string result_json(const ResultInfo& r) {
  std::ostringstream o;
  o << "{\"status\":" << json_escape(r.is_prime ? "P" : "C") << ",\"exponent\":" << r.exponent << ",\"worktype\":" << json_escape(r.ll ? "LL" : "PRP-3")
    << ",\"res64\":" << json_escape(r.res64);
  if (!r.ll) o << ",\"res2048\":" << json_escape(r.res2048) << ",\"residue-type\":1";
  o << ",\"errors\":{\"gerbicz\":" << r.gerbicz_errors << "},\"shift-count\":0";
  if (r.fft_length) o << ",\"fft-length\":" << r.fft_length;
  o << ",\"program\":{\"name\":\"prmers\",\"version\":" << json_escape(r.program_version) << ",\"port\":" << r.port << "}";
  o << ",\"os\":{\"os\":" << json_escape(r.os_name);
  if (!r.os_arch.empty()) o << ",\"architecture\":" << json_escape(r.os_arch);
  o << "}";
  if (!r.user.empty()) o << ",\"user\":" << json_escape(r.user);
  if (!r.computer.empty()) o << ",\"computer\":" << json_escape(r.computer);
  if (!r.aid.empty()) o << ",\"aid\":" << json_escape(r.aid);
  if (!r.timestamp.empty()) o << ",\"timestamp\":" << json_escape(r.timestamp);
  o << "}";
  return o.str();
}

// ---- PRP proof checkpoints (ProofSetMarin.cpp:56-122): the 2^power iterations whose residues a proof of that power needs;
//      each residue is stored as <p>/proof/<iteration>: u32 CRC-32 of the words, then the ceil(p/32) little-endian words ----
class ProofPoints {
 public:
  ProofPoints(uint32_t exponent, uint32_t power, const std::string& base_dir = ".") : p_(exponent), power_(power) {
    dir_ = (std::filesystem::path(base_dir) / std::to_string(exponent) / "proof").string();
    points_.push_back(0);
    uint32_t span = (exponent + 1) / 2;
    for (uint32_t level = 0; level < power; ++level, span = (span + 1) / 2) {
      const size_t have = points_.size();
      for (size_t i = 0; i < have; ++i) points_.push_back(points_[i] + span);
    }
    points_.front() = exponent;   // the residue after all p squarings replaces iteration 0
    std::sort(points_.begin(), points_.end());
  }
  const std::vector<uint32_t>& points() const { return points_; }
  bool should_checkpoint(uint32_t iteration) const { return std::binary_search(points_.begin(), points_.end(), iteration); }
  std::string file_of(uint32_t iteration) const { return (std::filesystem::path(dir_) / std::to_string(iteration)).string(); }
  // words: canonical residue after `iteration` squarings (pack_words of engine::get); no-op for other iterations
  bool save(uint32_t iteration, const std::vector<uint32_t>& words) const {
    if (!should_checkpoint(iteration)) return false;
    std::filesystem::create_directories(dir_);
    std::ofstream f(file_of(iteration), std::ios::binary);
    const uint32_t crc = crc32_update(0, words.data(), words.size() * 4);
    f.write(reinterpret_cast<const char*>(&crc), 4);
    f.write(reinterpret_cast<const char*>(words.data()), std::streamsize(words.size() * 4));
    return f.good();
  }
  std::vector<uint32_t> load(uint32_t iteration) const {
    std::ifstream f(file_of(iteration), std::ios::binary);
    if (!f) throw std::runtime_error("cannot open proof checkpoint " + file_of(iteration));
    uint32_t crc = 0;
    std::vector<uint32_t> words((size_t(p_) + 31) / 32);
    f.read(reinterpret_cast<char*>(&crc), 4);
    f.read(reinterpret_cast<char*>(words.data()), std::streamsize(words.size() * 4));
    if (!f.good() || crc != crc32_update(0, words.data(), words.size() * 4)) throw std::runtime_error("damaged proof checkpoint " + file_of(iteration));
    return words;
  }
  // every residue up to and including iteration `limit` is on disk (ProofSetMarin::isValidTo)
  bool valid_to(uint32_t limit) const {
    for (uint32_t pt : points_) { if (pt > limit) break; if (pt < p_ && !std::filesystem::exists(file_of(pt))) return false; }
    return true;
  }
 private:
  uint32_t p_, power_;
  std::string dir_;
  std::vector<uint32_t> points_;
};

// ---- SHA3-256 (FIPS 202) for the hash chain of a proof.  Written for this header: the round constants come from the standard's LFSR
//      (x^8 + x^6 + x^5 + x^4 + 1) and the rotation offsets from its (x, y) -> (y, 2x + 3y) walk, both generated at first use; pinned by
//      digests that hashlib computes (tests/test_proof.py) ---------------------------------------------------------------------------
class Sha3_256 {
 public:
  Sha3_256() { std::memset(a_, 0, sizeof a_); }
  Sha3_256& update(const void* data, size_t len) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < len; ++i) {
      a_[fill_ >> 3] ^= uint64_t(p[i]) << (8 * (fill_ & 7));   // lanes are little-endian
      if (++fill_ == kRate) { permute(a_); fill_ = 0; }
    }
    return *this;
  }
  std::vector<unsigned char> finish() {   // 32 bytes; the object is spent afterwards
    a_[fill_ >> 3] ^= uint64_t(0x06) << (8 * (fill_ & 7));                 // domain bits 01 + first pad bit
    a_[(kRate - 1) >> 3] ^= uint64_t(0x80) << (8 * ((kRate - 1) & 7));      // last pad bit
    permute(a_);
    std::vector<unsigned char> out(32);
    for (size_t i = 0; i < 32; ++i) out[i] = static_cast<unsigned char>(a_[i >> 3] >> (8 * (i & 7)));
    return out;
  }

 private:
  static constexpr size_t kRate = 136;   // 1600 - 2 * 256 bits
  struct Tables {
    uint64_t rc[24];
    unsigned rot[25];
    Tables() {
      unsigned lfsr = 1;
      for (int r = 0; r < 24; ++r) {
        rc[r] = 0;
        for (int j = 0; j < 7; ++j) {
          if (lfsr & 1u) rc[r] ^= uint64_t(1) << ((1u << j) - 1);
          lfsr = ((lfsr << 1) ^ ((lfsr & 0x80u) ? 0x71u : 0u)) & 0xffu;
        }
      }
      rot[0] = 0;
      for (unsigned t = 0, x = 1, y = 0; t < 24; ++t) {
        rot[x + 5 * y] = ((t + 1) * (t + 2) / 2) % 64;
        const unsigned ny = (2 * x + 3 * y) % 5;
        x = y; y = ny;
      }
    }
  };
  static uint64_t rotl(uint64_t v, unsigned s) { return s ? (v << s) | (v >> (64 - s)) : v; }
  static void permute(uint64_t* A) {
    static const Tables T;
    uint64_t B[25], C[5];
    for (int round = 0; round < 24; ++round) {
      for (int x = 0; x < 5; ++x) C[x] = A[x] ^ A[x + 5] ^ A[x + 10] ^ A[x + 15] ^ A[x + 20];
      for (int x = 0; x < 5; ++x) {
        const uint64_t d = C[(x + 4) % 5] ^ rotl(C[(x + 1) % 5], 1);
        for (int y = 0; y < 5; ++y) A[x + 5 * y] ^= d;
      }
      for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y) B[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(A[x + 5 * y], T.rot[x + 5 * y]);
      for (int y = 0; y < 5; ++y)
        for (int x = 0; x < 5; ++x) A[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
      A[0] ^= T.rc[round];
    }
  }
  uint64_t a_[25];
  size_t fill_ = 0;
};

// ---- PRP proof: file (GIMPS version 2, ProofMarin::save / load, src/core/ProofMarin.cpp:33-199), hash chain, build and verify on an
//      engine -- the C++ twin of prmers_amd/proof.py: same bytes from both ------------------------------------------------------------
inline size_t proof_residue_size(uint32_t p) { return (size_t(p) - 1) / 8 + 1; }
inline std::string proof_file_name(uint32_t p, uint32_t power) { return std::to_string(p) + "-" + std::to_string(power) + ".proof"; }   // ProofManagerMarin.cpp:129-132
// SHA3-256 over [the previous digest,] the (p - 1) / 8 + 1 little-endian bytes of a residue
inline std::vector<unsigned char> proof_hash(uint32_t p, const std::vector<uint32_t>& words, const std::vector<unsigned char>& prefix = {}) {
  std::vector<unsigned char> bytes(words.size() * 4);
  for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = static_cast<unsigned char>(words[i / 4] >> (8 * (i % 4)));
  Sha3_256 h;
  if (!prefix.empty()) h.update(prefix.data(), prefix.size());
  return h.update(bytes.data(), proof_residue_size(p)).finish();
}
inline uint64_t proof_hash64(const std::vector<unsigned char>& digest) {   // its first 8 bytes, little-endian
  uint64_t h = 0;
  for (int i = 7; i >= 0; --i) h = (h << 8) | digest[size_t(i)];
  return h;
}

struct Proof {
  uint32_t p = 0;
  std::vector<uint32_t> B;
  std::vector<std::vector<uint32_t>> middles;
  uint32_t power() const { return uint32_t(middles.size()); }

  std::string bytes() const {
    std::string out = "PRP PROOF\nVERSION=2\nHASHSIZE=64\nPOWER=" + std::to_string(power()) + "\nNUMBER=M" + std::to_string(p) + "\n";
    auto put = [&](const std::vector<uint32_t>& r) { for (size_t i = 0; i < proof_residue_size(p); ++i) out += char((i / 4 < r.size() ? r[i / 4] : 0u) >> (8 * (i % 4))); };
    put(B);
    for (const auto& m : middles) put(m);
    return out;
  }
  bool save(const std::string& path) const {
    std::ofstream f(path, std::ios::binary);
    const std::string b = bytes();
    f.write(b.data(), std::streamsize(b.size()));
    return f.good();
  }
  // refuses any other version or hash size, a power outside 1 .. 12, cofactor proofs (a NUMBER with '/') and a file that is too short or too long
  static Proof load(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open proof file " + path);
    const std::string raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    auto line = [&]() {
      const size_t e = raw.find('\n', pos);
      if (e == std::string::npos) throw std::runtime_error(path + ": incomplete proof header");
      const std::string l = raw.substr(pos, e - pos);
      pos = e + 1;
      return l;
    };
    auto field = [&](const char* key) {
      const std::string l = line(), k = std::string(key) + "=";
      if (l.compare(0, k.size(), k) != 0) throw std::runtime_error(path + ": unexpected header line " + l);
      return l.substr(k.size());
    };
    auto number = [&](const std::string& v, const char* what) -> uint64_t {
      if (v.empty() || v.size() > 10 || v.find_first_not_of("0123456789") != std::string::npos) throw std::runtime_error(path + ": bad " + what + " " + v);
      return std::stoull(v);
    };
    if (line() != "PRP PROOF") throw std::runtime_error(path + ": not a PRP proof file");
    const std::string version = field("VERSION"), hashsize = field("HASHSIZE"), power = field("POWER"), num = field("NUMBER");
    if (version != "2") throw std::runtime_error(path + ": unsupported proof version " + version);
    if (hashsize != "64") throw std::runtime_error(path + ": unsupported hash size " + hashsize);
    const uint64_t k = number(power, "power");
    if (k < 1 || k > 12) throw std::runtime_error(path + ": proof power " + power + " is outside 1 .. 12");
    if (num.find('/') != std::string::npos) throw std::runtime_error(path + ": proofs of cofactors (" + num + ") are not supported");
    if (num.empty() || num[0] != 'M') throw std::runtime_error(path + ": NUMBER=" + num + " is not a Mersenne number");
    const uint64_t e = number(num.substr(1), "exponent");
    if (e < 2 || e > 0xffffffffull) throw std::runtime_error(path + ": bad exponent " + num);
    Proof pr;
    pr.p = uint32_t(e);
    const size_t size = proof_residue_size(pr.p);
    if (raw.size() - pos != size * (k + 1)) throw std::runtime_error(path + ": " + std::to_string(raw.size() - pos) + " residue bytes where power " + power + " needs " + std::to_string(size * (k + 1)));
    auto take = [&]() {
      std::vector<uint32_t> r((size_t(pr.p) + 31) / 32, 0u);
      for (size_t i = 0; i < size; ++i) r[i / 4] |= uint32_t(static_cast<unsigned char>(raw[pos + i])) << (8 * (i % 4));
      pos += size;
      return r;
    };
    pr.B = take();
    for (uint64_t i = 0; i < k; ++i) pr.middles.push_back(take());
    return pr;
  }
};

// the 64-bit exponents h_0 .. h_(k-1) of a proof
inline std::vector<uint64_t> proof_hash_chain(const Proof& pr) {
  std::vector<unsigned char> digest = proof_hash(pr.p, pr.B);
  std::vector<uint64_t> hs;
  for (const auto& m : pr.middles) { digest = proof_hash(pr.p, m, digest); hs.push_back(proof_hash64(digest)); }
  return hs;
}

// Engine: set_words(reg, words), get_words(reg), exp_mul(a, h, b, tmp), exp_mul2(a, h, b, tmp), square_mul_n(reg, count), is_equal(a, b)
// (engine_hip has them; tests/host/test_proof_formats.cpp runs the two functions on a GMP stand-in).
//
// The proof of M_p from the point files under <base_dir>/<p>/proof/ (ProofSetMarin::computeProof, src/core/ProofSetMarin.cpp:213-311, with
// every fold "below <- below^h * top" as one exp_mul on the engine instead of a host mpz power).  Level L loads the residues at
// points[s (2 i + 1) - 1], s = 2^(power - L - 1), onto a stack of registers and folds for every trailing one bit of i; the register left is
// the level's middle.  Needs power + 1 registers: the stack never exceeds `power`, register `power` is the temporary.  A missing or
// damaged point file throws with its name (ProofPoints::load).  log: one line per level, as the reference prints them.
template <class Engine>
Proof build_proof(Engine& eng, uint32_t p, uint32_t power, const std::string& base_dir = ".", std::FILE* log = nullptr) {
  if (power < 1 || power > 12) throw std::runtime_error("proof power " + std::to_string(power) + " is outside 1 .. 12");
  const ProofPoints pts(p, power, base_dir);
  const size_t tmp = power;
  Proof pr;
  pr.p = p;
  pr.B = pts.load(p);
  std::vector<unsigned char> digest = proof_hash(p, pr.B);
  std::vector<uint64_t> hashes;
  for (uint32_t level = 0; level < power; ++level) {
    const size_t s = size_t(1) << (power - level - 1);
    size_t top = 0;
    for (size_t i = 0; i < (size_t(1) << level); ++i) {
      eng.set_words(top++, pts.load(pts.points()[s * (2 * i + 1) - 1]));
      for (uint32_t k = 0; (i >> k) & 1; ++k) { --top; eng.exp_mul(top - 1, hashes[level - 1 - k], top, tmp); }
    }
    if (top != 1) throw std::runtime_error("internal: proof stack not folded");
    pr.middles.push_back(eng.get_words(0));
    digest = proof_hash(p, pr.middles.back(), digest);
    hashes.push_back(proof_hash64(digest));
    if (log) {
      const std::vector<uint32_t>& m = pr.middles.back();
      const uint64_t m64 = (uint64_t(m.size() > 1 ? m[1] : 0u) << 32) | m[0];
      std::fprintf(log, "proof [%u] : M %016llx, h %016llx\n", level, static_cast<unsigned long long>(m64), static_cast<unsigned long long>(hashes.back()));
    }
  }
  return pr;
}

// true when the proof shows B = 3^(2^p): A = 3, B = proof.B, span = p; per middle M with its h: B <- M^h * (B^2 if span is odd, else B),
// A <- A^h * M, span <- (span + 1) / 2; then A^(2^span) == B on the engine.  Needs 5 registers.
constexpr size_t kProofVerifyRegisters = 5;
template <class Engine>
bool verify_proof(Engine& eng, const Proof& pr) {
  size_t RA = 0, RB = 1, RM = 2, RM2 = 3, RT = 4;
  std::vector<uint32_t> three((size_t(pr.p) + 31) / 32, 0u);
  three[0] = 3;
  eng.set_words(RA, three);
  eng.set_words(RB, pr.B);
  const std::vector<uint64_t> hs = proof_hash_chain(pr);
  uint64_t span = pr.p;
  for (size_t i = 0; i < pr.middles.size(); ++i) {
    eng.set_words(RM, pr.middles[i]);
    eng.set_words(RM2, pr.middles[i]);
    if (span & 1) eng.exp_mul2(RM, hs[i], RB, RT); else eng.exp_mul(RM, hs[i], RB, RT);   // the new B, in RM
    eng.exp_mul(RA, hs[i], RM2, RT);
    std::swap(RB, RM);
    span = (span + 1) / 2;
  }
  eng.square_mul_n(RA, size_t(span));
  return eng.is_equal(RA, RB);
}

}  // namespace formats
}  // namespace mi355
