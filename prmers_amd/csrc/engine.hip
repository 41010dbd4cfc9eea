// Engine implementation: buffers, host-side digit I/O, kernel sequencing.
#include "engine.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "host_digits.hpp"

namespace mi355 {

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #expr); \
  } while (0)

// launchers of the chosen column variant (the split sweeps are launched by run_front / run_back: they need the second buffer)
static ColSweeps col_sweeps(ColKernels k) {
  switch (k) {
    case ColKernels::kRadix8R1: return v2_cols(1);
    case ColKernels::kRadix8R2: return v2_cols(2);
    case ColKernels::kRadix8R4: return v2_cols(4);
    case ColKernels::kRadix4Pairs: return v3_cols(false);
    case ColKernels::kRadix4Planes: return v3_cols(true);
    case ColKernels::kRadix5: return v5_cols(false);
    case ColKernels::kRadix5J1: return v5_cols(true);
    case ColKernels::kSplit: return ColSweeps{};
    default: return ColSweeps{launch_front, launch_back, launch_back_ext, nullptr};
  }
}
static RowsFn row_sweep(RowKernels k) {
  switch (k) {
    case RowKernels::kRadix4Pairs: return v3_rows1024_pairs;
    case RowKernels::kRadix4Planes: return v3_rows1024_planes;
    case RowKernels::kRadix8: return v2_rows4096;
    case RowKernels::kRadix8Wide: return v2_rows8192;
    case RowKernels::kRows2048One: return v2_rows2048_one;
    case RowKernels::kRows2048Two: return v2_rows2048_two;
    default: return launch_middle;
  }
}

template <class T>
static const T* upload(unsigned char*& cursor, unsigned char* base, const std::vector<T>& v, std::vector<unsigned char>& host) {
  const size_t off = size_t(cursor - base);
  std::memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
  const T* p = reinterpret_cast<const T*>(cursor);
  cursor += (v.size() * sizeof(T) + 255) & ~size_t(255);
  return p;
}

Engine::Engine(uint32_t p, size_t reg_count, int device, bool verbose, const char* spec)
    : pl_(make_plan(p, spec, true)), device_(device), verbose_(verbose), nregs_(reg_count) {
  if (reg_count == 0) throw std::runtime_error("register_count must be > 0");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    throw std::runtime_error("no HIP device available: the MI355X engine has no CPU fallback");
  if (device < 0 || device >= ndev) throw std::runtime_error("HIP device index out of range");
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));

  reg_bytes_ = pl_.n * 8;  // digits use the first 4n bytes, a multiplicand image all 8n
  lanes_ = pl_.lanes;
  const size_t slot_bytes = lanes_ * reg_bytes_, cb_words = lanes_ * pl_.runs();   // a slot is `lanes` registers, one behind the other
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&regs_), (nregs_ + 1) * slot_bytes));
  HIPCHK(hipMemsetAsync(regs_, 0, (nregs_ + 1) * slot_bytes, stream_));
  slot_.resize(nregs_ + 1);
  for (size_t r = 0; r <= nregs_; ++r) slot_[r] = regs_ + r * slot_bytes;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&cbuf_), (nregs_ + 4) * cb_words * 8));
  HIPCHK(hipMemsetAsync(cbuf_, 0, (nregs_ + 4) * cb_words * 8, stream_));
  cb_.resize(nregs_);
  for (size_t r = 0; r < nregs_; ++r) cb_[r] = cbuf_ + r * cb_words;
  for (size_t r = nregs_; r < nregs_ + 4; ++r) cb_spare_.push_back(cbuf_ + r * cb_words);
  kind_.assign(nregs_, kDigits);
  pending_carry_.assign(nregs_, 0);

  // one allocation for all tables
  auto padded = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
  std::vector<uint64_t> tah(pl_.TA.size()), tai2(pl_.TAi.size());
  for (size_t i = 0; i < tah.size(); ++i) { tah[i] = gf::half(pl_.TA[i]); tai2[i] = gf::dbl(pl_.TAi[i]); }
  const size_t total = padded(pl_.SA.size() * 4) + padded(pl_.SB.size() * 4) + padded(pl_.TA.size() * 8) * 4 +
                       padded(pl_.TB.size() * 8) * 2 + padded(pl_.TWlo.size() * 8) + padded(pl_.TWhi.size() * 8) +
                       padded(pl_.UT1.size() * 8) + padded(pl_.UT2.size() * 8) + padded(pl_.S2r.size() * 8) * 2 +
                       padded(pl_.S1r.size() * 8) * 2 + 1024;
  HIPCHK(hipMalloc(&tables_, total));
  std::vector<unsigned char> host(total, 0);
  unsigned char* base = static_cast<unsigned char*>(tables_);
  unsigned char* cur = base;
  dp_.SA = upload(cur, base, pl_.SA, host);
  dp_.SB = upload(cur, base, pl_.SB, host);
  dp_.TA = upload(cur, base, pl_.TA, host);
  dp_.TAi = upload(cur, base, pl_.TAi, host);
  dp_.TAh = upload(cur, base, tah, host);
  dp_.TAi2 = upload(cur, base, tai2, host);
  dp_.TB = upload(cur, base, pl_.TB, host);
  dp_.TBi = upload(cur, base, pl_.TBi, host);
  dp_.TWlo = upload(cur, base, pl_.TWlo, host);
  dp_.TWhi = upload(cur, base, pl_.TWhi, host);
  dp_.UT1 = upload(cur, base, pl_.UT1, host);
  dp_.UT2 = upload(cur, base, pl_.UT2, host);
  dp_.S2r = pl_.S2r.empty() ? nullptr : upload(cur, base, pl_.S2r, host);
  dp_.S2ri = pl_.S2ri.empty() ? nullptr : upload(cur, base, pl_.S2ri, host);
  dp_.S1r = pl_.S1r.empty() ? nullptr : upload(cur, base, pl_.S1r, host);
  dp_.S1ri = pl_.S1ri.empty() ? nullptr : upload(cur, base, pl_.S1ri, host);
  HIPCHK(hipMemcpy(tables_, host.data(), total, hipMemcpyHostToDevice));

  dp_.n = uint32_t(pl_.n); dp_.m = uint32_t(pl_.m);
  dp_.M1 = pl_.M1; dp_.M2 = pl_.M2; dp_.L1 = pl_.L1; dp_.logL1 = pl_.logL1; dp_.logM2 = pl_.logM2;
  dp_.r5 = pl_.r5; dp_.C = pl_.C; dp_.logC = 0; while ((1u << dp_.logC) < pl_.C) ++dp_.logC; dp_.q = pl_.q; dp_.t = pl_.t; dp_.twh = pl_.twh;
  dp_.lanes = pl_.lanes;
  dp_.onelaunch = pl_.onelaunch ? 1u : 0u;
  one_ = onelaunch_shape(pl_.m, pl_.r5, pl_.lanes);
  dp_.I4 = pl_.I4; dp_.I4inv = pl_.I4inv;
  dp_.DI = nullptr;
  dp_.F0f = dp_.F0i = dp_.FBf = dp_.FBi = nullptr;
  if (!pl_.DI.empty()) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&di_), pl_.DI.size() * 4));
    HIPCHK(hipMemcpy(di_, pl_.DI.data(), pl_.DI.size() * 4, hipMemcpyHostToDevice));
    dp_.DI = di_;
  }
  for (int i = 0; i < 4; ++i) dp_.W5c[i] = pl_.W5c[i];
  { const char* tn = std::getenv("MI355_TUNE"); dp_.tune = tn ? uint32_t(std::atoi(tn)) : 0u; }
  {
    // the register-resident kernels keep two 512-thread work-groups per CU: a launch of more than one round
    // boosts the groups of its last half round (kernels_v2.hip, boost_if_late)
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_));
    const uint32_t slots = 2u * uint32_t(prop.multiProcessorCount);
    auto from = [&](size_t grid) { return grid > slots ? uint32_t(grid - size_t(slots) * 50 / 100) : ~0u; };
    dp_.boost_rows = from(pl_.M2 == 2048 ? pl_.M1 / 2 : pl_.M1);   // (rows of 2048 go two to a tile on the register-resident row kernel)
    dp_.boost_tiles = lanes_ > 1 ? ~0u : from(pl_.tiles());   // with a lane dimension the last half round of a launch is not the top of blockIdx.x
  }
  HIPCHK(configure_kernels(pl_.lds_front, pl_.lds_mid, pl_.lanes, pl_.onelaunch));
  if (pl_.split5) {
    HIPCHK(configure_split(dp_));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&split_), reg_bytes_));
  }
  // kernel variants: those that serve the shape (plan.hpp), narrowed by MI355_KERNELS=generic|v2rows|v2cols (A/B tests, debugging);
  // with lanes always the generic set, whose launches take the lanes as grid.y (kernels.hpp DevPlan.lanes); with one-launch products too
  kc_ = choose_kernels(pl_, std::getenv("MI355_KERNELS"));
  cols_ = col_sweeps(kc_.cols);
  rows_ = row_sweep(kc_.rows);
  dp_.lab_u = 1; dp_.lab_v = pl_.r5; dp_.lab_red = 0;
  if (kc_.cols == ColKernels::kRadix5 || kc_.cols == ColKernels::kRadix5J1) {   // radix-5 columns in prime-factor form: their own frequency labels
    v5_pfa(kc_.cols == ColKernels::kRadix5J1, &dp_.lab_u, &dp_.lab_v);
  } else if (kc_.cols == ColKernels::kGeneric && pl_.r5 == 5 && pl_.L1 > 1) {   // the generic radix-5 stage in prime-factor form (kernels.hip lds_radix5)
    uint32_t u = 1; while ((pl_.L1 * u) % 5 != 1) ++u;
    dp_.lab_u = pl_.L1 * u;   // L1 (L1^-1 mod 5); lab_v stays 5
    dp_.lab_red = pl_.M1;     // lab_u blk + 5 rq <= 16 L1 + 5 (L1 - 1) < 5 M1: four conditional subtractions
  }
  {   // every exponent label + M1 k, k < M2, that a row kernel looks up lies inside the two-level root table (plan.hpp TWhi)
    const uint64_t max_label = dp_.lab_red ? uint64_t(pl_.M1) - 1 : uint64_t(dp_.lab_u) * (pl_.r5 - 1) + uint64_t(dp_.lab_v) * (pl_.L1 - 1);
    if (max_label + uint64_t(pl_.M1) * (pl_.M2 - 1) >= (uint64_t(pl_.TWhi.size()) << pl_.twh))
      throw std::runtime_error("internal: column frequency labels beyond the root table");
  }
  if (kc_.resident_cols() || kc_.rows != RowKernels::kGeneric) HIPCHK(v2_configure());
  if (kc_.resident_cols()) {   // four-step chain starts and ratios: built once on the device (2 x tiles x threads + 2 x M2 words)
    const size_t nt = pl_.tiles() * threads_per_tile(kc_.cols);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&f0_), (2 * nt + 2 * size_t(pl_.M2)) * 8));
    HIPCHK(cols_.build_fourstep(dp_, f0_, f0_ + nt, f0_ + 2 * nt, f0_ + 2 * nt + pl_.M2, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    dp_.F0f = f0_; dp_.F0i = f0_ + nt; dp_.FBf = f0_ + 2 * nt; dp_.FBi = f0_ + 2 * nt + pl_.M2;
  }

  width_ = host_digits::digit_widths(p, pl_.n);   // natural order
  cg_ = CanonGeom::tile_major(dp_, p);
  { const char* hc = std::getenv("MI355_HOST_CARRY"); host_carry_ = hc && hc[0] == '1'; }
  HIPCHK(hipStreamSynchronize(stream_));
  if (verbose_) std::fprintf(stderr, "[mi355] p=%u %s regs=%zu device=%d\n", p, pl_.describe().c_str(), nregs_, device_);
}

Engine::~Engine() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  if (regs_) (void)hipFree(regs_);
  if (cbuf_) (void)hipFree(cbuf_);
  if (tables_) (void)hipFree(tables_);
  if (di_) (void)hipFree(di_);
  if (f0_) (void)hipFree(f0_);
  if (split_) (void)hipFree(split_);
  if (canon_) (void)hipFree(canon_);
  if (canon_lanes_) (void)hipFree(canon_lanes_);
  for (int h = 0; h < 2; ++h) {   // (what a batch still had queued is dropped: nothing of it was launched)
    if (batch_read_[h]) (void)hipEventDestroy(batch_read_[h]);
    if (batch_stage_[h]) (void)hipHostFree(batch_stage_[h]);
  }
  if (batch_dev_) (void)hipFree(batch_dev_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

void Engine::sync() {
  HIPCHK(hipSetDevice(device_));
  HIPCHK(hipStreamSynchronize(stream()));
}

void Engine::normalize(size_t r) {
  if (kind_[r] != kDigits) return;
  if (pending_carry_[r]) {
    HIPCHK(launch_carry_fix(dp_, digits(r), cbuf(r), stream()));
    pending_carry_[r] = 0;
  }
}

// Runs of two digits (C = 1): the run carries go into the digits at once.  A carry word has about w + log2(n) bits (the
// convolution sums of unsigned digits are ~ n 2^(2w-2)); its first digit absorbs w of them and the rest lands on the
// run's second digit, log2(n) - 2 (+ log2 a) bits above its width -- too much for the next squaring once that exceeds w.
// Local carry passes (canon.hip k_relax) take w bits off per pass; as many as it takes to get below the width follow.
void Engine::carry_fix_now(size_t r, int excess) {
  HIPCHK(launch_carry_fix(dp_, digits(r), cbuf(r), stream()));
  pending_carry_[r] = 0;
  if (pl_.C >= 2) return;
  if (excess < 0) excess = ilog2(pl_.n) + 1 + 4 - 2;   // log2(n) rounded up, factor a up to 15 (plan.hpp a_fast)
  const int w = int(pl_.q);                 // the narrower digit width
  while (excess > w - 2) {
    for (size_t l = 0; l < lanes_; ++l)   // (lane by lane: runs of two digits are not the ladder's plans)
      HIPCHK(canon_relax(dp_, pl_.p, digits(r, l), digits(nregs_, l), stream()));
    swap_with_work(r);
    excess -= w;
  }
}

// digits(r) (+ its pending run carries) -> work(); digits(r) stay as they are.  (Runs of two digits never leave carries pending:
// every operation that writes run carries on a plan with C < 2 takes them in at once, carry_fix_now.)
void Engine::run_front(size_t r) {
  if (kc_.cols == ColKernels::kSplit) HIPCHK(launch_front_split(dp_, digits(r), split_, work(), stream()));
  else HIPCHK(cols_.front(dp_, digits(r), pending_carry_[r] ? cbuf(r) : nullptr, work(), stream()));
}

void Engine::run_middle(const uint64_t* in, const uint64_t* y, uint64_t* out, int mode, const uint64_t* y2, uint64_t* img) {
  HIPCHK(rows_(dp_, in, y, y2, img, out, mode, stream()));
}

// work() -> digits(r) + run carries in cbuf(r): runs of 2C >= 4 digits leave them to the next sweep, which folds them in, runs of two
// digits take them at once.  ev (nullable): two events recorded around that carry fix (time_square_mul)
void Engine::run_back(size_t r, uint32_t a, hipEvent_t* ev) {
  if (kc_.cols == ColKernels::kSplit) HIPCHK(launch_back_split(dp_, work(), split_, digits(r), cbuf(r), a, stream()));
  else HIPCHK(cols_.back(dp_, work(), digits(r), cbuf(r), a, stream()));
  if (ev) HIPCHK(hipEventRecord(ev[0], stream()));
  if (pl_.C >= 2) pending_carry_[r] = 1;
  else carry_fix_now(r);
  if (ev) HIPCHK(hipEventRecord(ev[1], stream()));
}

// One-launch products (plan token onelaunch; kernels.hip k_onelaunch): front sweep on digits(r) (+ its pending run carries), the row sweep
// in `mode` (y, y2: multiplicand images read in modes 1 and 3; img: the image written in modes 2 and 4) and, unless mode 2, the back sweep
// into digits(r) with factor a and the extras of back_ext, all in one launch.  The new run carries go to a spare buffer: the launch reads
// the pending ones of r and of the addend, which may be r itself.  Such plans have runs of four digits or more (plan.hpp), so the carries
// stay pending.
// mode kModeSibling (mul_sibling): y is read at the lane's sibling of `level`, y2 at the own lane.  Never queued: the sibling's image may
// be what another work-group of the running queue stores, so the queue runs first (stream()) and this is a launch of its own.
void Engine::one_launch(size_t r, int mode, const uint64_t* y, const uint64_t* y2, uint64_t* img, uint32_t a, long copy_to, long add_src, uint32_t level) {
  OneLaunchArgs oa;
  oa.src = digits(r); oa.src_cbuf = pending_carry_[r] ? cbuf(r) : nullptr;
  oa.y = y; oa.y2 = y2; oa.img = img; oa.a = a; oa.mode = mode; oa.level = level;
  oa.TL = one_.TL; oa.K = one_.K; oa.groups = one_.groups;
  const bool queued = batching_ && mode != kModeSibling;
  BackExt x;
  if (mode == 2) {
    if (queued) { BatchOp& op = batch_slot(); op.kind = BatchOp::kProduct; op.oa = oa; }
    else HIPCHK(launch_onelaunch(dp_, oa, x, stream()));
    return;
  }
  if (copy_to >= 0 && size_t(copy_to) != r) { x.digits2 = digits(size_t(copy_to)); x.cbuf2 = cbuf(size_t(copy_to)); }
  if (add_src >= 0) { x.add_digits = digits(size_t(add_src)); x.add_cbuf = pending_carry_[size_t(add_src)] ? cbuf(size_t(add_src)) : nullptr; }
  uint64_t* fresh = take_spare_cbuf();
  oa.dst = digits(r); oa.dst_cbuf = fresh;
  if (queued) { BatchOp& op = batch_slot(); op.kind = BatchOp::kProduct; op.oa = oa; op.x = x; }   // the pointers as they are resolved now
  else HIPCHK(launch_onelaunch(dp_, oa, x, stream()));
  adopt_cbuf(r, fresh);
  kind_[r] = kDigits; pending_carry_[r] = 1;
  if (x.digits2) { kind_[size_t(copy_to)] = kDigits; pending_carry_[size_t(copy_to)] = 1; }
}

// ---- host digit I/O -------------------------------------------------------------------------

void Engine::write_values(size_t dst, const std::vector<uint32_t>& natural) {
  // natural order goes up as it is; the tile-major order is made on the device (canon.hip k_scatter)
  HIPCHK(hipSetDevice(device_));
  HIPCHK(hipStreamSynchronize(stream()));
  uint32_t* nat = reinterpret_cast<uint32_t*>(work());
  HIPCHK(hipMemcpy(nat, natural.data(), pl_.n * 4, hipMemcpyHostToDevice));
  for (size_t l = 0; l < lanes_; ++l) HIPCHK(canon_scatter(dp_, pl_.p, nat, digits(dst, l), stream()));   // every lane
  HIPCHK(hipStreamSynchronize(stream()));
  kind_[dst] = kDigits;
  pending_carry_[dst] = 0;
}

// canonical digits of register r (strong carry with wrap-around, 2^p - 1 -> 0) in natural order, on the device
uint32_t* Engine::canon_digits(size_t r, int slot, size_t lane) {
  need_residue(r, "get");
  HIPCHK(hipSetDevice(device_));
  const size_t sw = canon_scratch_bytes<uint32_t>(cg_) / 4;
  if (!canon_) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&canon_), (sw + 2 * pl_.n) * 4));
    HIPCHK(hipMemsetAsync(canon_flags<uint32_t>(cg_, canon_), 0, 16 * 4, stream()));
  }
  normalize(r);
  uint32_t* out = canon_ + sw + size_t(slot) * pl_.n;
  HIPCHK(canon_launch(cg_, digits(r, lane), out, canon_, stream()));
  return out;
}

// flags: [0] all ones, [1] chain too wide (fall back), [2] compare differs; clears the sticky ones for the next use
bool Engine::canon_flags_ok(uint32_t (&flags)[4]) {
  uint32_t* df = canon_flags<uint32_t>(cg_, canon_);
  HIPCHK(hipMemcpyAsync(flags, df, 16, hipMemcpyDeviceToHost, stream()));
  HIPCHK(hipMemsetAsync(df, 0, 16 * 4, stream()));
  HIPCHK(hipStreamSynchronize(stream()));
  return flags[1] == 0;
}

void Engine::read_values(size_t src, std::vector<uint64_t>& v) {
  if (host_carry_) { read_values_host(src, v); return; }
  uint32_t* d = canon_digits(src, 0);
  uint32_t flags[4];
  stage_.resize(pl_.n);
  HIPCHK(hipMemcpyAsync(stage_.data(), d, pl_.n * 4, hipMemcpyDeviceToHost, stream()));
  if (!canon_flags_ok(flags)) { read_values_host(src, v); return; }
  v.resize(pl_.n);
  if (flags[0]) {   // 2^p - 1: the reference's get() leaves the digits all ones (engine.h:188-196 maps them to 0 later)
    for (size_t k = 0; k < pl_.n; ++k) v[k] = host_digits::ones(width_[k]);
  } else {
    for (size_t k = 0; k < pl_.n; ++k) v[k] = stage_[k];
  }
}

void Engine::read_values_host(size_t src, std::vector<uint64_t>& v, size_t lane) {
  need_residue(src, "get");
  stage_.resize(pl_.n);
  HIPCHK(hipSetDevice(device_));
  normalize(src);
  HIPCHK(hipStreamSynchronize(stream()));
  HIPCHK(hipMemcpy(stage_.data(), digits(src, lane), pl_.n * 4, hipMemcpyDeviceToHost));
  v.resize(pl_.n);
  const size_t M2 = pl_.M2, C = pl_.C, M1 = pl_.M1;
  for (size_t i = 0; i < pl_.m; ++i) {
    const size_t i1 = i / M2, i2 = i % M2, T = i2 / C, c = i2 % C;
    const size_t s = ((T * M1 + i1) * C + c) * 2;
    v[2 * i] = stage_[s];
    v[2 * i + 1] = stage_[s + 1];
  }
  host_digits::strong_carry(v.data(), width_);
}

void Engine::set_u32(size_t dst, uint32_t value) {
  need_register(dst, "set");
  HIPCHK(hipSetDevice(device_));
  // spread the constant over the first digits (the reference stores it whole in digit 0,
  // engine_gpu.h:1444-1449; same value, but never an over-wide digit); every lane gets it
  for (size_t l = 0; l < lanes_; ++l) {
    HIPCHK(hipMemsetAsync(digits(dst, l), 0, pl_.n * 4, stream()));
    if (value) HIPCHK(canon_set_small(dp_, pl_.p, digits(dst, l), value, stream()));
  }
  kind_[dst] = kDigits;
  pending_carry_[dst] = 0;
}

void Engine::set_digits(size_t dst, const uint64_t* d, size_t count) {
  need_register(dst, "set_digits");
  if (count != pl_.n) throw std::runtime_error("set_digits: count must equal the transform size");
  std::vector<uint32_t> nat(pl_.n);
  for (size_t k = 0; k < pl_.n; ++k) nat[k] = uint32_t(d[k]);
  write_values(dst, nat);
}

void Engine::get_digits(size_t src, uint64_t* d, size_t count) {
  no_lanes("get_digits");
  if (count != pl_.n) throw std::runtime_error("get_digits: count must equal the transform size");
  std::vector<uint64_t> v;
  read_values(src, v);
  for (size_t k = 0; k < pl_.n; ++k) d[k] = uint32_t(v[k]) | (uint64_t(width_[k]) << 32);  // engine_gpu.h:1560
}

uint64_t Engine::res64(size_t src) { no_lanes("res64"); return res64_of(src, 0); }
uint64_t Engine::res64_lane(size_t lane, size_t src) { need_lane(lane, "res64"); return res64_of(src, lane); }

uint64_t Engine::res64_of(size_t src, size_t lane) {
  std::vector<uint64_t> v;
  size_t have = pl_.n;
  if (host_carry_) {
    read_values_host(src, v, lane);
  } else {
    // the low 64 bits live in the first few digits: canonicalise on the device, read back only those
    uint32_t* d = canon_digits(src, 0, lane);
    have = std::min<size_t>(pl_.n, 16);
    uint32_t head[16], flags[4];
    HIPCHK(hipMemcpyAsync(head, d, have * 4, hipMemcpyDeviceToHost, stream()));
    if (!canon_flags_ok(flags)) { read_values_host(src, v, lane); have = pl_.n; }
    else { v.resize(have); for (size_t k = 0; k < have; ++k) v[k] = flags[0] ? host_digits::ones(width_[k]) : head[k]; }
  }
  return host_digits::res64_of_head(v.data(), width_, have);
}

// The words are packed on the device from the canonical digits (canon.hip k_pack_words; 2^p - 1 comes out as 0 there): word_count() words
// cross PCIe instead of the n digits.  MI355_HOST_CARRY=1, or a canonical form that falls back, take the host loop (host_digits.hpp).
void Engine::get_words(size_t src, uint32_t* w, size_t count) { no_lanes("get_words"); words_of(src, 0, w, count); }
void Engine::get_words_lane(size_t lane, size_t src, uint32_t* w, size_t count) { need_lane(lane, "get_words"); words_of(src, lane, w, count); }

void Engine::words_of(size_t src, size_t lane, uint32_t* w, size_t count) {
  if (count != word_count()) throw std::runtime_error("get_words: count must equal word_count()");
  if (!host_carry_) {
    uint32_t* d = canon_digits(src, 0, lane);
    uint32_t* dw = canon_;   // the pipeline's first work array (n words >= word_count(): widths are below 32) is free once the digits are out
    HIPCHK(canon_pack_words(cg_, d, dw, stream()));
    HIPCHK(hipMemcpyAsync(w, dw, count * 4, hipMemcpyDeviceToHost, stream()));
    uint32_t flags[4];
    if (canon_flags_ok(flags)) return;
  }
  std::vector<uint64_t> v;
  read_values_host(src, v, lane);
  host_digits::pack_words(v.data(), width_, w, count);
}

void Engine::set_words(size_t dst, const uint32_t* w, size_t count) {
  need_register(dst, "set_words");
  if (count != word_count()) throw std::runtime_error("set_words: count must equal word_count()");
  put_words(dst, w, count, 0, lanes_);   // every lane
  kind_[dst] = kDigits;
  pending_carry_[dst] = 0;
}

// One lane of a register of digits; the other lanes stay as they are, pending run carries included: the kind and the pending flag are
// the register's, so an image is refused (set the register to a value first) and this lane's pending carry words are cleared instead.
void Engine::set_words_lane(size_t lane, size_t dst, const uint32_t* w, size_t count) {
  need_lane(lane, "set_words");
  need_register(dst, "set_words");
  if (count != word_count()) throw std::runtime_error("set_words: count must equal word_count()");
  if (lanes_ == 1) { set_words(dst, w, count); return; }
  if (kind_[dst] != kDigits)
    throw std::runtime_error("set_words: the register holds a multiplicand image, and the kind is the register's, not the lane's (write a value to every lane first)");
  if (pending_carry_[dst]) {
    HIPCHK(hipSetDevice(device_));
    HIPCHK(hipMemsetAsync(cbuf(dst) + lane * pl_.runs(), 0, pl_.runs() * 8, stream()));
  }
  put_words(dst, w, count, lane, lane + 1);
}

void Engine::put_words(size_t dst, const uint32_t* w, size_t count, size_t lane0, size_t lane1) {
  // bits at and above p are folded back (2^p = 1), so any count-word value is accepted; the fold runs on the host, before the upload,
  // and only for a value that has such bits
  std::vector<uint32_t> src;
  if (host_carry_ || ((pl_.p % 32) && (w[count - 1] >> (pl_.p % 32)))) {
    src.assign(w, w + count);
    host_digits::fold_words_mod_mp(src.data(), count, pl_.p);
    w = src.data();
  }
  HIPCHK(hipSetDevice(device_));
  if (!host_carry_) {
    // the words go up as they are and are cut into digits on the device (canon.hip k_unpack_words), straight into tile-major order
    uint32_t* dw = reinterpret_cast<uint32_t*>(work());
    HIPCHK(hipMemcpyAsync(dw, w, count * 4, hipMemcpyHostToDevice, stream()));
    HIPCHK(canon_unpack_words(cg_, dw, digits(dst, lane0), stream()));
    // The same value on every lane (set_words on a lane engine; the broadcast of prmers_amd/lanecross.py): the first lane is cut into digits,
    // the others are copies of it, doubling -- log2 B copies where a launch a lane was 512 launches.  Whole lanes of 8 n bytes: what lies
    // behind a lane's 4 n bytes of digits is read by nothing while the register holds digits.
    for (size_t have = 1; have < lane1 - lane0; have *= 2) {
      const size_t more = std::min(have, lane1 - lane0 - have);
      HIPCHK(hipMemcpyAsync(slot_[dst] + (lane0 + have) * reg_bytes_, slot_[dst] + lane0 * reg_bytes_, more * reg_bytes_, hipMemcpyDeviceToDevice, stream()));
    }
    HIPCHK(hipStreamSynchronize(stream()));
    return;
  }
  std::vector<uint64_t> v(pl_.n);
  host_digits::unpack_words(w, count, width_, v.data());
  const std::vector<uint32_t> natural(v.begin(), v.end());
  HIPCHK(hipStreamSynchronize(stream()));
  uint32_t* nat = reinterpret_cast<uint32_t*>(work());
  HIPCHK(hipMemcpy(nat, natural.data(), pl_.n * 4, hipMemcpyHostToDevice));
  for (size_t l = lane0; l < lane1; ++l) HIPCHK(canon_scatter(dp_, pl_.p, nat, digits(dst, l), stream()));
  HIPCHK(hipStreamSynchronize(stream()));
}

bool Engine::equal(size_t lhs, size_t rhs) {
  no_lanes("equal");
  if (!host_carry_) {
    // both registers canonicalised and compared on the device: 16 bytes cross PCIe (the reference reads both
    // registers back and carries them on the host: engine.h:148-157 via engine_gpu.h:1534-1561)
    uint32_t* a = canon_digits(lhs, 0);
    uint32_t* b = canon_digits(rhs, 1);
    HIPCHK(canon_compare(a, b, uint32_t(pl_.n), canon_flags<uint32_t>(cg_, canon_) + 2, stream()));
    uint32_t flags[4];
    if (canon_flags_ok(flags)) return flags[2] == 0;
  }
  return equal_words(lhs, rhs);
}

// ---- every lane at once (include/mi355_lanewise.h) -------------------------------------------
// The pipeline of canon.hip with the lanes as grid.y: a chunk of lanes (canon_chunk_lanes: the scratch stays within
// kCanonLanesScratchBytes) is one launch sequence and one read of its flag words, where lane by lane it is seven launches and a
// synchronising read for each.  Pending run carries are folded in first, for all lanes in one launch (normalize).

void* Engine::lanes_scratch(size_t chunk) {
  if (!canon_lanes_) {   // the chunk size is a function of the engine's n and lane count: one size for good
    HIPCHK(hipMalloc(&canon_lanes_, chunk * canon_lane_bytes(pl_.n)));
    canon_lanes_chunk_ = chunk;
  }
  if (chunk > canon_lanes_chunk_) throw std::runtime_error("internal: lane-wise scratch made for " + std::to_string(canon_lanes_chunk_) + " lanes, asked for " + std::to_string(chunk));
  lane_flags_.resize(chunk * 16);
  return canon_lanes_;
}

void Engine::words_host(size_t src, size_t lane, uint32_t* w) {
  std::vector<uint64_t> v;
  read_values_host(src, v, lane);
  host_digits::pack_words(v.data(), width_, w, word_count());
}

void Engine::equal_lanes(size_t lhs, size_t rhs, uint8_t* out, size_t count) {
  if (lanes_ == 1) { RegisterMachine::equal_lanes(lhs, rhs, out, count); return; }
  if (count != lanes_) throw std::runtime_error("lanewise_equal: count must equal the lane count (" + std::to_string(lanes_) + ")");
  need_residue(lhs, "lanewise_equal"); need_residue(rhs, "lanewise_equal");
  HIPCHK(hipSetDevice(device_));
  std::vector<uint32_t> a(word_count()), b(word_count());
  auto on_host = [&](size_t l) { words_host(lhs, l, a.data()); words_host(rhs, l, b.data()); out[l] = a == b ? 1 : 0; };
  if (host_carry_) { for (size_t l = 0; l < lanes_; ++l) on_host(l); return; }
  normalize(lhs); normalize(rhs);
  const size_t chunk = canon_chunk_lanes(pl_.n, lanes_), stride = reg_bytes_ / 4;
  void* scratch = lanes_scratch(chunk);
  for (size_t l0 = 0; l0 < lanes_; l0 += chunk) {
    const size_t L = std::min(chunk, lanes_ - l0);
    uint32_t* df = canon_lanes_flags(cg_, scratch, L);
    HIPCHK(hipMemsetAsync(df, 0, L * 16 * 4, stream()));
    HIPCHK(canon_launch_lanes(cg_, digits(lhs, l0), stride, L, 0, scratch, stream()));
    HIPCHK(canon_launch_lanes(cg_, digits(rhs, l0), stride, L, 1, scratch, stream()));
    HIPCHK(canon_compare_lanes(cg_, L, scratch, stream()));
    HIPCHK(hipMemcpyAsync(lane_flags_.data(), df, L * 16 * 4, hipMemcpyDeviceToHost, stream()));
    HIPCHK(hipStreamSynchronize(stream()));
    for (size_t l = 0; l < L; ++l) {
      if (lane_flags_[l * 16 + 1]) on_host(l0 + l);   // a digit was too wide for the 0/1 chain: this lane through the host carry
      else out[l0 + l] = lane_flags_[l * 16 + 2] == 0 ? 1 : 0;
    }
  }
}

void Engine::get_words_lanes(size_t src, uint32_t* w, size_t count) {
  if (lanes_ == 1) { RegisterMachine::get_words_lanes(src, w, count); return; }
  const size_t wc = word_count();
  if (count != lanes_ * wc) throw std::runtime_error("lanewise_get_words: count must equal lanes x word_count()");
  need_residue(src, "lanewise_get_words");
  HIPCHK(hipSetDevice(device_));
  if (host_carry_) { for (size_t l = 0; l < lanes_; ++l) words_host(src, l, w + l * wc); return; }
  normalize(src);
  const size_t chunk = canon_chunk_lanes(pl_.n, lanes_), stride = reg_bytes_ / 4;
  void* scratch = lanes_scratch(chunk);
  for (size_t l0 = 0; l0 < lanes_; l0 += chunk) {
    const size_t L = std::min(chunk, lanes_ - l0);
    uint32_t* df = canon_lanes_flags(cg_, scratch, L);
    uint32_t* dw = nullptr;
    HIPCHK(hipMemsetAsync(df, 0, L * 16 * 4, stream()));
    HIPCHK(canon_launch_lanes(cg_, digits(src, l0), stride, L, 0, scratch, stream()));
    HIPCHK(canon_pack_words_lanes(cg_, L, 0, scratch, &dw, stream()));
    HIPCHK(hipMemcpyAsync(w + l0 * wc, dw, L * wc * 4, hipMemcpyDeviceToHost, stream()));
    HIPCHK(hipMemcpyAsync(lane_flags_.data(), df, L * 16 * 4, hipMemcpyDeviceToHost, stream()));
    HIPCHK(hipStreamSynchronize(stream()));
    for (size_t l = 0; l < L; ++l)
      if (lane_flags_[l * 16 + 1]) words_host(src, l0 + l, w + (l0 + l) * wc);
  }
}

// The way back: the words of every lane go up a chunk at a time into the same scratch (one copy) and are cut into the digits of the
// chunk's lanes in one launch (canon.hip k_unpack_words with the lanes as grid.y), where lane by lane each lane is an upload, a launch and a
// synchronise.  The register becomes digits on every lane; what it held (an image, pending run carries) is gone, as after set_words.
void Engine::set_words_lanes(size_t dst, const uint32_t* w, size_t count) {
  if (lanes_ == 1) { RegisterMachine::set_words_lanes(dst, w, count); return; }
  const size_t wc = word_count();
  need_register(dst, "lanewise_set_words");
  if (count != lanes_ * wc) throw std::runtime_error("lanewise_set_words: count must equal lanes x word_count()");
  HIPCHK(hipSetDevice(device_));
  if (host_carry_) {
    for (size_t l = 0; l < lanes_; ++l) put_words(dst, w + l * wc, wc, l, l + 1);
  } else {
    const size_t chunk = canon_chunk_lanes(pl_.n, lanes_), stride = reg_bytes_ / 4;
    uint32_t* dw = static_cast<uint32_t*>(lanes_scratch(chunk));   // wc <= n: the words of a chunk fit its first work array
    const uint32_t top = pl_.p % 32;
    std::vector<uint32_t> folded;
    for (size_t l0 = 0; l0 < lanes_; l0 += chunk) {
      const size_t L = std::min(chunk, lanes_ - l0);
      const uint32_t* src = w + l0 * wc;
      // bits at and above p are folded back on the host (2^p = 1), as put_words does, and only for the lanes that have such bits
      bool any = false;
      for (size_t l = 0; top && l < L && !any; ++l) any = (src[l * wc + wc - 1] >> top) != 0;
      if (any) {
        folded.assign(src, src + L * wc);
        for (size_t l = 0; l < L; ++l)
          if (folded[l * wc + wc - 1] >> top) host_digits::fold_words_mod_mp(folded.data() + l * wc, wc, pl_.p);
        src = folded.data();
      }
      HIPCHK(hipMemcpyAsync(dw, src, L * wc * 4, hipMemcpyHostToDevice, stream()));
      HIPCHK(canon_unpack_words_lanes(cg_, dw, digits(dst, l0), stride, L, stream()));
      HIPCHK(hipStreamSynchronize(stream()));
    }
  }
  kind_[dst] = kDigits;
  pending_carry_[dst] = 0;
}

// ---- register operations -------------------------------------------------------------------

void Engine::copy(size_t dst, size_t src) {
  need_register(dst, "copy"); need_register(src, "copy");
  if (dst == src) return;
  HIPCHK(hipSetDevice(device_));
  // the register is copied as it stands: digits with their pending run carries (no carry sweep),
  // a multiplicand image whole; with lanes the whole slot (a lane's digits are the first half of its 8n bytes)
  const size_t bytes = lanes_ > 1 ? lanes_ * reg_bytes_ : (kind_[src] == kDigits) ? pl_.n * 4 : reg_bytes_;
  const bool carries = kind_[src] == kDigits && pending_carry_[src];
  if (batching_) {   // the same bytes, lane by lane, by the lane's threads
    const size_t per_lane = bytes / lanes_;
    if (per_lane % 16 || per_lane > 0xFFFFFFFFu) throw std::runtime_error("internal: batch copy of a register that is no multiple of 16 bytes");
    BatchOp& op = batch_slot();
    op.kind = BatchOp::kCopy; op.copy_bytes = uint32_t(per_lane);
    op.la.a = digits(src); op.la.s1 = digits(dst);
    if (carries) { op.la.ca = cbuf(src); op.la.cs1 = cbuf(dst); }
  } else {
    HIPCHK(hipMemcpyAsync(slot_[dst], slot_[src], bytes, hipMemcpyDeviceToDevice, stream()));
    if (carries) HIPCHK(hipMemcpyAsync(cbuf(dst), cbuf(src), lanes_ * pl_.runs() * 8, hipMemcpyDeviceToDevice, stream()));
  }
  pending_carry_[dst] = (kind_[src] == kDigits) ? pending_carry_[src] : 0;
  kind_[dst] = kind_[src];
}

void Engine::square_chain(size_t r, uint32_t a, hipEvent_t* ev) {
  if (a > pl_.a_fast) { square_chain(r, 1, ev); scale(r, a); return; }   // beyond the fused carry's bound (plan.hpp fused_factor_limit)
  if (pl_.onelaunch) { one_launch(r, 0, nullptr, nullptr, nullptr, a, -1, -1); return; }   // (never with events: time_square_mul refuses the plan)
  if (ev) HIPCHK(hipEventRecord(ev[0], stream()));
  run_front(r);
  if (ev) HIPCHK(hipEventRecord(ev[1], stream()));
  run_middle(work(), nullptr, work(), 0);
  if (ev) HIPCHK(hipEventRecord(ev[2], stream()));
  run_back(r, a, ev ? ev + 3 : nullptr);
}

void Engine::square_mul(size_t r, uint32_t a) {
  need_residue(r, "square_mul"); need_factor(a, "square_mul");
  HIPCHK(hipSetDevice(device_));
  square_chain(r, a, nullptr);
}

void Engine::square_mul_n(size_t r, uint32_t a, size_t count, uint32_t sub) {
  need_residue(r, "square_mul_n"); need_factor(a, "square_mul_n");
  if (count == 0) return;
  HIPCHK(hipSetDevice(device_));
  for (size_t i = 0; i < count; ++i) { square_chain(r, a, nullptr); if (sub) sub_u32(r, sub); }
}

void Engine::set_multiplicand(size_t dst, size_t src) {
  need_residue(src, "set_multiplicand"); need_register(dst, "set_multiplicand");
  HIPCHK(hipSetDevice(device_));
  if (pl_.onelaunch) one_launch(src, 2, nullptr, nullptr, image(dst), 1, -1, -1);
  else {
    run_front(src);
    run_middle(work(), nullptr, image(dst), 2);
  }
  kind_[dst] = kImage;
  pending_carry_[dst] = 0;
}

void Engine::mul(size_t dst, size_t src, uint32_t a) {
  need_residue(dst, "mul"); need_image(src, "mul"); need_factor(a, "mul");
  HIPCHK(hipSetDevice(device_));
  if (pl_.onelaunch) one_launch(dst, 1, image(src), nullptr, nullptr, a > pl_.a_fast ? 1u : a, -1, -1);
  else {
    run_front(dst);
    run_middle(work(), image(src), work(), 1);
    run_back(dst, a > pl_.a_fast ? 1u : a);
  }
  if (a > pl_.a_fast) scale(dst, a);
}

// dst[l] = dst[l] x src[sibling of l at `level`] where that lane exists, else dst[l] x alt[l] (include/mi355_lanecross.h): mul with factor 1
// whose row sweep takes its image from another lane (kernels.hip k_middle_sibling / k_onelaunch_sibling).  Everything is checked before the
// first launch.  Inside a batch the queue runs first (one_launch, stream()).
void Engine::mul_sibling(size_t dst, size_t src, size_t alt, uint32_t level) {
  if (lanes_ == 1) { RegisterMachine::mul_sibling(dst, src, alt, level); return; }   // no sibling in range: mul(dst, alt)
  check_mul_sibling(dst, src, alt, level);
  HIPCHK(hipSetDevice(device_));
  if (pl_.onelaunch) { one_launch(dst, kModeSibling, image(src), image(alt), nullptr, 1, -1, -1, level); return; }
  run_front(dst);
  HIPCHK(launch_middle_sibling(dp_, work(), image(src), image(alt), work(), level, stream()));
  run_back(dst, 1);
}

// r = r x a, run-wise (kernels.hip k_scale): the factors above the plan's fused bound follow the operation with factor 1
void Engine::scale(size_t r, uint32_t a) {
  need_residue(r, "scale");
  uint64_t* fresh = take_spare_cbuf();
  const uint64_t* cin = pending_carry_[r] ? cbuf(r) : nullptr;
  HIPCHK(launch_scale(dp_, digits(r), cin, digits(r), fresh, a, stream()));
  adopt_cbuf(r, fresh);
  pending_carry_[r] = 1;
  // runs of two digits: the carry words (below 2^34: digit < 2^(q+2) after the passes, times a < 2^32) go in at once
  if (pl_.C < 2) carry_fix_now(r, 34 - int(pl_.q));
}

uint64_t* Engine::take_spare_cbuf() {
  if (cb_spare_.empty()) throw std::runtime_error("internal: no spare carry buffer");
  uint64_t* b = cb_spare_.back();
  cb_spare_.pop_back();
  return b;
}
void Engine::adopt_cbuf(size_t r, uint64_t* fresh) {
  cb_spare_.push_back(cb_[r]);
  cb_[r] = fresh;
}

// sum -> s1 (and s2), difference -> d1 (and d2); -1: not wanted.  One run-wise sweep on pending-carry digits
// (kernels.hip k_linear); the results leave their run carries pending for the next front sweep.
void Engine::addsub(long s1, long s2, long d1, long d2, size_t a, size_t b) {
  HIPCHK(hipSetDevice(device_));
  need_residue(a, "addsub"); need_residue(b, "addsub");
  const long outs[4] = {s1, s2, d1, d2};
  for (int i = 0; i < 4; ++i)
    if (outs[i] >= 0) { need_register(size_t(outs[i]), "addsub"); for (int j = 0; j < i; ++j) if (outs[j] == outs[i]) throw std::runtime_error("addsub: output registers must differ"); }
  LinArgs la;
  la.a = digits(a); la.ca = pending_carry_[a] ? cbuf(a) : nullptr;
  la.b = digits(b); la.cb = pending_carry_[b] ? cbuf(b) : nullptr;
  uint64_t* fresh[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4; ++i) if (outs[i] >= 0) fresh[i] = take_spare_cbuf();
  if (s1 >= 0) { la.s1 = digits(size_t(s1)); la.cs1 = fresh[0]; }
  if (s2 >= 0) { la.s2 = digits(size_t(s2)); la.cs2 = fresh[1]; }
  if (d1 >= 0) { la.d1 = digits(size_t(d1)); la.cd1 = fresh[2]; }
  if (d2 >= 0) { la.d2 = digits(size_t(d2)); la.cd2 = fresh[3]; }
  if ((s2 >= 0 && s1 < 0) || (d2 >= 0 && d1 < 0)) throw std::runtime_error("internal: copy output without a primary output");
  if (batching_) { BatchOp& op = batch_slot(); op.kind = BatchOp::kLinear; op.la = la; }
  else HIPCHK(launch_linear(dp_, la, stream()));
  for (int i = 0; i < 4; ++i)
    if (outs[i] >= 0) {
      const size_t r = size_t(outs[i]);
      adopt_cbuf(r, fresh[i]);
      kind_[r] = kDigits; pending_carry_[r] = 1;
      if (pl_.C < 2) carry_fix_now(r);   // runs of two digits: no deferred fold
    }
}

void Engine::add(size_t dst, size_t src) { addsub(long(dst), -1, -1, -1, dst, src); }
void Engine::sub_reg(size_t dst, size_t src) { addsub(-1, -1, long(dst), -1, dst, src); }

// back sweep of work() into dst with the extras of kernels.hpp BackExt
void Engine::back_ext(size_t dst, uint32_t a, long copy_to, long add_src) {
  BackExt x;
  if (copy_to >= 0 && size_t(copy_to) != dst) { x.digits2 = digits(size_t(copy_to)); x.cbuf2 = cbuf(size_t(copy_to)); }
  if (add_src >= 0) { x.add_digits = digits(size_t(add_src)); x.add_cbuf = pending_carry_[size_t(add_src)] ? cbuf(size_t(add_src)) : nullptr; }
  uint64_t* fresh = take_spare_cbuf();   // the addend may be dst itself: its pending carries are read while the new ones are written
  HIPCHK(cols_.back_ext(dp_, work(), digits(dst), fresh, a, x, stream()));
  adopt_cbuf(dst, fresh);
  const size_t outs[2] = {dst, x.digits2 ? size_t(copy_to) : dst};
  for (int i = 0; i < (x.digits2 ? 2 : 1); ++i) {
    const size_t r = outs[i];
    kind_[r] = kDigits; pending_carry_[r] = 1;
    if (pl_.C < 2) carry_fix_now(r);
  }
}

void Engine::square_mul_copy(size_t src, size_t dst_copy, uint32_t a) {
  need_residue(src, "square_mul_copy"); need_register(dst_copy, "square_mul_copy"); need_factor(a, "square_mul_copy");
  HIPCHK(hipSetDevice(device_));
  if (dst_copy == src || !kc_.fused_back() || a > pl_.a_fast) { RegisterMachine::square_mul_copy(src, dst_copy, a); return; }
  if (pl_.onelaunch) { one_launch(src, 0, nullptr, nullptr, nullptr, a, long(dst_copy), -1); return; }
  run_front(src);
  run_middle(work(), nullptr, work(), 0);
  back_ext(src, a, long(dst_copy), -1);
}

void Engine::mul_copy(size_t dst, size_t src, size_t dst_copy, uint32_t a) {
  need_residue(dst, "mul_copy"); need_image(src, "mul_copy"); need_register(dst_copy, "mul_copy"); need_factor(a, "mul_copy");
  if (dst_copy == src) throw std::runtime_error("mul_copy: the multiplicand must differ from the outputs");
  HIPCHK(hipSetDevice(device_));
  if (dst_copy == dst || !kc_.fused_back() || a > pl_.a_fast) { RegisterMachine::mul_copy(dst, src, dst_copy, a); return; }
  if (pl_.onelaunch) { one_launch(dst, 1, image(src), nullptr, nullptr, a, long(dst_copy), -1); return; }
  run_front(dst);
  run_middle(work(), image(src), work(), 1);
  back_ext(dst, a, long(dst_copy), -1);
}

void Engine::mul_add(size_t dst, size_t mul_src, size_t add_src, uint32_t a) {
  need_residue(dst, "mul_add"); need_image(mul_src, "mul_add"); need_residue(add_src, "mul_add"); need_factor(a, "mul_add");
  HIPCHK(hipSetDevice(device_));
  if (!kc_.fused_back() || a > pl_.a_fast) {   // no fused sweep (split sweeps; factors above the fused bound): the base-class composition (engine.h:65-70)
    if (add_src == dst)
      throw std::runtime_error(!kc_.fused_back() ? "mul_add: add_src == dst needs the fused sweep, which this transform size does not have"
                                          : "mul_add: add_src == dst needs the fused sweep, which takes factors up to the plan's fused bound only (mi355_engine.h)");
    RegisterMachine::mul_add(dst, mul_src, add_src, a); return;
  }
  if (pl_.onelaunch) { one_launch(dst, 1, image(mul_src), nullptr, nullptr, a, -1, long(add_src)); return; }
  run_front(dst);   // reads digits(dst) (+ pending carries) and leaves them in place
  run_middle(work(), image(mul_src), work(), 1);
  back_ext(dst, a, -1, long(add_src));
}

// dst = dst (a + b).  Everything is checked before the first launch, so a refused call leaves the registers as they were.
void Engine::mul_sum(size_t dst, size_t src_a, size_t src_b, size_t tmp) {
  if (!pl_.sum_fast) { RegisterMachine::mul_sum(dst, src_a, src_b, tmp); return; }   // the summed operand is beyond the plan's capacity (plan.hpp sum_product_ok)
  check_mul_sum(dst, src_a, src_b, tmp);
  HIPCHK(hipSetDevice(device_));
  if (pl_.onelaunch) { one_launch(dst, 3, image(src_a), image(src_b), nullptr, 1, -1, -1); return; }
  run_front(dst);   // pending run carries (and a borrowed-through sub) of dst go in exactly as in mul
  run_middle(work(), image(src_a), work(), 3, image(src_b));
  run_back(dst, 1);
}

// img_out = the multiplicand image of src, src = src^2 a: a squaring whose row sweep (mode 4) also stores the forward transform it squares.
// The front sweep has taken src's pending run carries in by then, so the image is the one set_multiplicand(img_out, src) would write now.
void Engine::square_mul_prepare(size_t src, size_t img_out, uint32_t a) {
  check_square_mul_prepare(src, img_out, a);
  HIPCHK(hipSetDevice(device_));
  if (pl_.onelaunch) one_launch(src, 4, nullptr, nullptr, image(img_out), a > pl_.a_fast ? 1u : a, -1, -1);
  else {
    run_front(src);
    run_middle(work(), nullptr, work(), 4, nullptr, image(img_out));
  }
  kind_[img_out] = kImage;
  pending_carry_[img_out] = 0;
  if (!pl_.onelaunch) run_back(src, a > pl_.a_fast ? 1u : a);
  if (a > pl_.a_fast) scale(src, a);   // beyond the fused carry's bound: the rule of square_mul
}

void Engine::square_mul_bits(size_t r, uint32_t factor, const uint8_t* bits, size_t nbits) {
  if (!check_square_mul_bits(r, factor, bits, nbits)) return;
  HIPCHK(hipSetDevice(device_));
  for (size_t i = 0; i < nbits; ++i) square_chain(r, bit_of(bits, i) ? factor : 1u, nullptr);
}

void Engine::sub_u32(size_t r, uint32_t v) {
  need_residue(r, "sub");
  if (v == 0) return;
  HIPCHK(hipSetDevice(device_));
  // (not deferred into the next front sweep as a field element: digit 0 plus its carry may be below v, and the sums of a sparse register
  // then go negative, which the unsigned back sweep reads as values near the field prime; the borrow below is exact for every register)
  // the small subtraction only touches the digit vector (cyclic borrow), so run carries that are still pending
  // for the next front sweep can stay pending: value = digits + carries - v either way
  HIPCHK(launch_sub_small(dp_, digits(r), v, stream()));
}

// ---- batches ----------------------------------------------------------------------------------

void Engine::batch_begin() {
  if (!pl_.onelaunch) throw std::runtime_error("batch_begin: batches need one-launch products (plan token onelaunch): only there does a lane stay inside one work-group");
  if (batching_) throw std::runtime_error("batch_begin: a batch is open already (batch_end comes first)");
  HIPCHK(hipSetDevice(device_));
  if (!batch_dev_) {
    for (int h = 0; h < 2; ++h) {
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&batch_stage_[h]), kBatchCapacity * sizeof(BatchOp), hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&batch_read_[h], hipEventDisableTiming));
    }
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&batch_dev_), kBatchCapacity * sizeof(BatchOp)));
  }
  batching_ = true;
}

void Engine::batch_end() {
  if (!batching_) throw std::runtime_error("batch_end: no batch is open (batch_begin comes first)");
  batching_ = false;   // first: the batch is closed whatever the flush says
  HIPCHK(hipSetDevice(device_));
  flush_batch();
}

void Engine::batch_stats(uint64_t out[4]) const {
  out[0] = batch_ops_; out[1] = batch_launches_; out[2] = kBatchCapacity; out[3] = batch_pending_;
}

BatchOp& Engine::batch_slot() {
  if (batch_pending_ == kBatchCapacity) flush_batch();
  ++batch_ops_;
  return *new (&batch_stage_[batch_half_][batch_pending_++]) BatchOp();
}

// The descriptors of the half just filled go to the device buffer and run, both on the stream: the copy waits for the launch before it,
// which read the buffer.  Then the other half is the one to fill, once the launch that read it last is over.
void Engine::flush_batch() {
  if (!batch_pending_) return;
  const int h = batch_half_;
  const size_t count = batch_pending_;
  batch_pending_ = 0;   // (stream_, not stream(): this is the flush)
  HIPCHK(hipMemcpyAsync(batch_dev_, batch_stage_[h], count * sizeof(BatchOp), hipMemcpyHostToDevice, stream_));
  HIPCHK(launch_batch(dp_, batch_dev_, uint32_t(count), one_.TL, one_.K, one_.groups, stream_));
  HIPCHK(hipEventRecord(batch_read_[h], stream_));
  batch_in_flight_[h] = true;
  ++batch_launches_;
  batch_half_ = h ^ 1;
  if (batch_in_flight_[batch_half_]) { HIPCHK(hipEventSynchronize(batch_read_[batch_half_])); batch_in_flight_[batch_half_] = false; }
}

// ---- raw images -----------------------------------------------------------------------------

void Engine::get_data(size_t src, void* data, size_t size) {
  no_lanes("get_data");
  need_register(src, "get_data");
  if (size != register_data_size()) throw std::runtime_error("get_data: size mismatch");
  HIPCHK(hipSetDevice(device_));
  normalize(src);
  HIPCHK(hipStreamSynchronize(stream()));
  HIPCHK(hipMemcpy(data, slot_[src], reg_bytes_, hipMemcpyDeviceToHost));
  const uint64_t tag = register_tag(pl_, kc_, kind_[src] == kImage);
  std::memcpy(static_cast<unsigned char*>(data) + reg_bytes_, &tag, 8);
}

// the tag must be this engine's own for digits or for an image (plan.hpp register_tag): the size alone is the same for every plan of an
// exponent, and the bytes of another plan would load as a permutation of the digits
void Engine::check_data(const void* data, size_t size) const {
  no_lanes("set_data");
  if (size != register_data_size()) throw std::runtime_error("set_data: size mismatch");
  uint64_t tag = 0;
  std::memcpy(&tag, static_cast<const unsigned char*>(data) + reg_bytes_, 8);
  if (tag <= 1) throw std::runtime_error("set_data: the image carries no layout fingerprint (written by an earlier version of the library)");
  if (tag != register_tag(pl_, kc_, (tag & 1) != 0))
    throw std::runtime_error((tag & 1) ? "set_data: multiplicand image of another exponent, plan or kernel set (" + pl_.describe() + " here)"
                                       : "set_data: register image of another exponent or plan (" + pl_.describe() + " here)");
}

void Engine::set_data(size_t dst, const void* data, size_t size) {
  need_register(dst, "set_data");
  check_data(data, size);
  uint64_t tag = 0;
  std::memcpy(&tag, static_cast<const unsigned char*>(data) + reg_bytes_, 8);
  HIPCHK(hipSetDevice(device_));
  HIPCHK(hipStreamSynchronize(stream()));
  HIPCHK(hipMemcpy(slot_[dst], data, reg_bytes_, hipMemcpyHostToDevice));
  kind_[dst] = (tag & 1) ? kImage : kDigits;
  pending_carry_[dst] = 0;
}

// ---- measurement ----------------------------------------------------------------------------

namespace {
struct EventPool {   // HIP events owned for the length of one measurement
  std::vector<hipEvent_t> evs;
  hipEvent_t make() {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    evs.push_back(e);
    return e;
  }
  ~EventPool() { for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
};
}  // namespace

const char* Engine::stage_name(size_t k) {
  static const char* names[kKernels] = {"k_front", "k_middle", "k_back", "k_carry_fix", "k_sub_small", "event_overhead"};
  return k < kKernels ? names[k] : "";
}

// kernel_ms[k]: average duration of kernel k of one squaring (-1: that kernel is not launched on this path),
// from one event between consecutive kernels on the engine's stream, minus the cost of an event record itself
// (kernel_ms[5], measured as the spacing of back-to-back records on the same stream: without the subtraction every
// interval carries one record, ~4-5 us, and a path that launches no kernel between two records shows it as a kernel).
void Engine::time_square_mul(size_t r, uint32_t a, uint32_t sub, size_t iters, double* total_ms, double* kernel_ms, size_t kcount) {
  no_lanes("time_square_mul");
  if (pl_.onelaunch) throw std::runtime_error("time_square_mul: not with one-launch products (plan token onelaunch): a squaring has no phases to time");
  need_residue(r, "time_square_mul");
  if (a == 0 || iters == 0) throw std::runtime_error("time_square_mul: factor and iters must be >= 1");
  HIPCHK(hipSetDevice(device_));
  EventPool pool;   // destroys its events on every way out (a HIPCHK that throws mid-batch used to leak them)
  const hipEvent_t e0 = pool.make(), e1 = pool.make();
  HIPCHK(hipStreamSynchronize(stream()));
  HIPCHK(hipEventRecord(e0, stream()));
  square_mul_n(r, a, iters, sub);
  HIPCHK(hipEventRecord(e1, stream()));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  if (total_ms) *total_ms = ms;

  if (kernel_ms && kcount) {
    for (size_t k = 0; k < kcount; ++k) kernel_ms[k] = 0;
    const size_t reps = std::min<size_t>(iters, 64);
    const size_t per = 6;
    std::vector<hipEvent_t> ev(reps * per);
    for (auto& x : ev) x = pool.make();
    // cost of one event record: spacing of back-to-back records on a batch of its own (its size does not depend on `iters`)
    double overhead = 0;
    {
      constexpr size_t kBatch = 64, kSkip = 8;   // the first records carry the queue start-up
      std::vector<hipEvent_t> oe(kBatch);
      for (auto& x : oe) x = pool.make();
      for (size_t i = 0; i < kBatch; ++i) HIPCHK(hipEventRecord(oe[i], stream()));
      HIPCHK(hipStreamSynchronize(stream()));
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, oe[kSkip], oe[kBatch - 1]));
      overhead = double(t) / double(kBatch - 1 - kSkip);
    }
    for (size_t i = 0; i < reps; ++i) {
      square_chain(r, a, &ev[i * per]);
      if (sub) sub_u32(r, sub);
      HIPCHK(hipEventRecord(ev[i * per + 5], stream()));
    }
    HIPCHK(hipStreamSynchronize(stream()));
    for (size_t i = 0; i < reps; ++i)
      for (size_t k = 0; k < 5 && k < kcount; ++k) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, ev[i * per + k], ev[i * per + k + 1]));
        kernel_ms[k] += double(t) / double(reps);
      }
    // which of the five slots hold a kernel on this path
    const bool fix_now = pl_.C < 2;                                    // k_carry_fix right after the back sweep
    const bool sub_kernel = sub != 0;                                  // k_sub_small
    const bool launched[5] = {true, true, true, fix_now, sub_kernel};
    for (size_t k = 0; k < 5 && k < kcount; ++k) kernel_ms[k] = launched[k] ? std::max(0.0, kernel_ms[k] - overhead) : -1.0;
    if (kcount > 5) kernel_ms[5] = overhead;
  }
}

#if defined(MI355_PROBE)
void Engine::probe(int kind, int grid_mult, int extra_lds, int boost_pct, size_t iters, double* avg_ms, uint64_t* tl, size_t tl_words) {
  HIPCHK(hipSetDevice(device_));
  if (!kc_.resident_cols() || kc_.rows == RowKernels::kGeneric) throw std::runtime_error("probe: needs the register-resident kernels");
  if (grid_mult < 1 || kind < 0 || kind > 2) throw std::runtime_error("probe: bad arguments");
  // probe launches: the rows of 4096, the columns of 1024 x 4 (v2) and of 1280 x 4 (v5)
  const bool v5 = kind != 1 && kc_.cols == ColKernels::kRadix5;
  if (kind == 1 ? kc_.rows != RowKernels::kRadix8 : !(v5 || kc_.cols == ColKernels::kRadix8R2)) HIPCHK(hipErrorNotSupported);
  const size_t base = (kind == 1) ? pl_.M1 : pl_.tiles(), grid = base * size_t(grid_mult);
  if (tl && tl_words < grid * 8) throw std::runtime_error("probe: timeline buffer too small");
  DevPlan d = dp_;
  d.probe = nullptr; d.probe_mod = uint32_t(base);
  {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_));
    const size_t per_cu = extra_lds >= 20 * 1024 ? 1 : 2;
    const size_t slots = per_cu * size_t(prop.multiProcessorCount);
    const int bp = boost_pct < 0 ? -boost_pct : boost_pct;
    const uint32_t from = (bp > 0 && grid > slots) ? uint32_t(grid - slots * size_t(bp) / 100) : ~0u;
    d.boost_rows = d.boost_tiles = from;
  }
  uint64_t* dtl = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dtl), grid * 64));
  HIPCHK(hipMemset(dtl, 0, grid * 64));
  uint32_t* dout = reinterpret_cast<uint32_t*>(slot_[0]);   // register 0 is scratch here
  auto launch = [&](const DevPlan& dd) {
    HIPCHK((v5 ? v5_probe_launch : v2_probe_launch)(dd, kind, grid_mult, extra_lds, digits(1 % nregs_), kind == 2 ? cbuf(0) : nullptr, work(), dout, stream()));
  };
  for (int w = 0; w < 3; ++w) launch(d);
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipStreamSynchronize(stream()));
  HIPCHK(hipEventRecord(e0, stream()));
  for (size_t i = 0; i < iters; ++i) launch(d);
  HIPCHK(hipEventRecord(e1, stream()));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  if (avg_ms) *avg_ms = double(ms) / double(iters ? iters : 1);
  HIPCHK(hipEventDestroy(e0)); HIPCHK(hipEventDestroy(e1));
  if (tl) {
    d.probe = dtl;
    // (boost_pct < 0: the instrumented launch follows a launch of ANOTHER kernel, as in a squaring, instead of a launch of itself)
    if (boost_pct < 0) { if (kind == 1) HIPCHK(cols_.back(dp_, work(), dout, cbuf(0), 1, stream())); else run_middle(work(), nullptr, work(), 0); }
    launch(d);
    HIPCHK(hipStreamSynchronize(stream()));
    HIPCHK(hipMemcpy(tl, dtl, grid * 64, hipMemcpyDeviceToHost));
  }
  HIPCHK(hipFree(dtl));
  HIPCHK(v2_configure());   // restore the LDS attributes
}
#endif

}  // namespace mi355
