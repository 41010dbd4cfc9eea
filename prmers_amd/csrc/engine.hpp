// Engine: one exponent, one HIP device, one stream, reg_count registers.
// The register machine of the reference's `engine` (include/marin/engine.h:16-303) for the Marin
// path, re-designed for MI355X (see plan.hpp / kernels.hip).  Exposed through capi.cpp only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "canon.hpp"
#include "kernels.hpp"
#include "plan.hpp"
#include "register_machine.hpp"

namespace mi355 {

class Engine final : public RegisterMachine {
 public:
  Engine(uint32_t p, size_t reg_count, int device, bool verbose, const char* spec);
  ~Engine() override;
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  uint32_t exponent() const override { return pl_.p; }
  std::string describe() const override { return pl_.describe(); }
  size_t size() const override { return pl_.n; }
  size_t reg_count() const override { return nregs_; }

  void sync() override;
  void set_u32(size_t dst, uint32_t v) override;
  void set_digits(size_t dst, const uint64_t* d, size_t count) override;
  void get_digits(size_t src, uint64_t* d, size_t count) override;
  void set_words(size_t dst, const uint32_t* w, size_t count) override;
  void get_words(size_t src, uint32_t* w, size_t count) override;
  uint64_t res64(size_t src) override;
  // Lanes (plan token lanes=B): B residues per register, every operation on all of them in one launch.  The writes above
  // then write every lane; the reads, equal, raw images and time_square_mul are refused, and these read or write one lane.
  size_t lanes() const override { return lanes_; }
  void set_words_lane(size_t lane, size_t dst, const uint32_t* w, size_t count) override;
  void get_words_lane(size_t lane, size_t src, uint32_t* w, size_t count) override;
  uint64_t res64_lane(size_t lane, size_t src) override;
  // every lane in one launch sequence per chunk of lanes (canon.hip canon_launch_lanes); a lane whose chain reports an over-wide digit,
  // and every lane under MI355_HOST_CARRY=1, goes through the host carry
  void equal_lanes(size_t lhs, size_t rhs, uint8_t* out, size_t count) override;
  void get_words_lanes(size_t src, uint32_t* w, size_t count) override;
  // the words of every lane into dst, one upload and one launch per chunk of lanes (canon.hip canon_unpack_words_lanes); dst becomes digits
  void set_words_lanes(size_t dst, const uint32_t* w, size_t count) override;
  void copy(size_t dst, size_t src) override;
  void set_multiplicand(size_t dst, size_t src) override;
  void square_mul(size_t r, uint32_t a) override;
  void mul(size_t dst, size_t src, uint32_t a) override;
  // across lanes (include/mi355_lanecross.h): mul by the image of the lane's sibling block's first lane, by alt's own-lane image where there is none
  void mul_sibling(size_t dst, size_t src, size_t alt, uint32_t level) override;
  void add(size_t dst, size_t src) override;
  void sub_reg(size_t dst, size_t src) override;
  void sub_u32(size_t r, uint32_t v) override;
  bool equal(size_t lhs, size_t rhs) override;
  // one run-wise sweep (the reference's fused variants: include/marin/engine.h:65-131; kernels/marin.cl:1856-1947)
  void addsub(long sum, long sum_copy, long diff, long diff_copy, size_t a, size_t b) override;
  // What this family fuses (kernels/marin.cl:2160-2365): the copy or the addend goes into the back sweep's carry chain where the plan has the
  // fused back sweep and the factor is within its bound, else the base composition
  void mul_add(size_t dst, size_t mul_src, size_t add_src, uint32_t a) override;
  void square_mul_copy(size_t src, size_t dst_copy, uint32_t a) override;
  void mul_copy(size_t dst, size_t src, size_t dst_copy, uint32_t a) override;
  // three launches per squaring, straight down square_chain (the benchmark's path); one with the plan token onelaunch (one_launch below)
  void square_mul_n(size_t r, uint32_t a, size_t count, uint32_t sub) override;
  void square_mul_bits(size_t r, uint32_t factor, const uint8_t* bits, size_t nbits) override;
  // one product through the row sweep's mode 3 where the plan's capacity allows it (plan.hpp sum_product_ok), else the base's two products;
  // for P-1 stage 2, A <- A (X_k - Y_j), the table is stored as images of Mp - Y_j
  void mul_sum(size_t dst, size_t src_a, size_t src_b, size_t tmp) override;
  bool mul_sum_is_fused() const override { return pl_.sum_fast; }
  // front sweep, rows in mode 4 (a squaring that stores the forward transform of its operand to img_out), back sweep: the two sweeps of
  // set_multiplicand(img_out, src) become one more store of 8n bytes.  Every plan has it.
  void square_mul_prepare(size_t src, size_t img_out, uint32_t a) override;
  bool square_mul_prepare_is_fused() const override { return true; }

  // Batches (plan token onelaunch only): between batch_begin and batch_end the register operations that are products,
  // run-wise sums and differences or copies -- copy, add, sub_reg, addsub, every form one_launch serves, the loops of square_mul_n
  // (sub == 0) and square_mul_bits -- are checked and booked as always and then queued; the queue runs as ONE launch (kernels.hip
  // k_batch).  Anything else the engine puts on its stream flushes the queue first (stream()), a full queue flushes by itself, and
  // batch_end flushes.  Destroying the engine discards what is queued.
  static constexpr size_t kBatchCapacity = 256;   // descriptors a launch takes
  void batch_begin() override;
  void batch_end() override;
  void batch_stats(uint64_t out[4]) const override;

  size_t register_data_size() const override { return reg_bytes_ + 8; }
  void get_data(size_t src, void* data, size_t size) override;
  void set_data(size_t dst, const void* data, size_t size) override;
  void check_data(const void* data, size_t size) const override;

  // measurement
  static constexpr size_t kKernels = 6;   // five kernel slots of a squaring + the measured cost of an event record
  static const char* stage_name(size_t k);
  size_t kernel_count() const override { return kKernels; }
  const char* kernel_name(size_t k) const override { return stage_name(k); }
  void time_square_mul(size_t r, uint32_t a, uint32_t sub, size_t iters, double* total_ms, double* kernel_ms, size_t kcount) override;
  size_t algorithmic_bytes() const override { return 48 * pl_.n; }
#if defined(MI355_PROBE)
  // diagnostics build only: `iters` timed launches of one sweep (kind 0 front, 1 rows, 2 back) over grid_mult x its grid with
  // extra_lds bytes of padding LDS (forces fewer groups per CU), then one launch with the timeline probe on (8 words per group -> tl)
  void probe(int kind, int grid_mult, int extra_lds, int boost_pct, size_t iters, double* avg_ms, uint64_t* tl, size_t tl_words);
#endif

 private:
  // kDigits: unweighted u32 digits (+ deferred run carries); kImage: multiplicand
  enum Kind : uint8_t { kDigits = 0, kImage = 1 };
  bool holds_image(size_t r) const override { return kind_[r] == kImage; }
  // lane l of a slot lies l * reg_bytes_ behind lane 0, lane l of a carry buffer l * runs() words (kernels.hpp DevPlan.lanes)
  uint32_t* digits(size_t r, size_t lane = 0) { return reinterpret_cast<uint32_t*>(slot_[r] + lane * reg_bytes_); }
  void no_lanes(const char* op) const {   // operations a lane engine does not have
    if (lanes_ > 1) throw std::runtime_error(std::string(op) + ": not with lanes (per-lane I/O: mi355_lanes_* in include/mi355_lanes.h)");
  }
  uint64_t* image(size_t r) { return reinterpret_cast<uint64_t*>(slot_[r]); }
  uint64_t* work() { return reinterpret_cast<uint64_t*>(slot_[nregs_]); }
  void swap_with_work(size_t r) { std::swap(slot_[r], slot_[nregs_]); }
  void read_values(size_t src, std::vector<uint64_t>& v);   // natural order, strongly carried digits
  void read_values_host(size_t src, std::vector<uint64_t>& v, size_t lane = 0);   // the same through D2H + host carry (reference's way: host_digits.hpp)
  uint32_t* canon_digits(size_t r, int slot, size_t lane = 0);   // device: canonical digits of r in natural order (canon.hip), slot 0 / 1
  void words_of(size_t src, size_t lane, uint32_t* w, size_t count);   // get_words of one lane
  uint64_t res64_of(size_t src, size_t lane);
  // fold w mod 2^p - 1 where it has bits at or above p, upload it to the work buffer and cut it into the digits of lanes [lane0, lane1) of dst
  void put_words(size_t dst, const uint32_t* w, size_t count, size_t lane0, size_t lane1);
  bool canon_flags_ok(uint32_t (&flags)[4]);    // reads the flag words; false: fall back to the host carry
  void words_host(size_t src, size_t lane, uint32_t* w);   // the canonical words of one lane through read_values_host
  void* lanes_scratch(size_t chunk);            // device scratch of the lane-wise pipeline for `chunk` lanes (made at first use)
  void write_values(size_t dst, const std::vector<uint32_t>& natural);
  void square_chain(size_t r, uint32_t a, hipEvent_t* ev);
  uint64_t* cbuf(size_t r) { return cb_[r]; }
  uint64_t* take_spare_cbuf();                      // carry-word buffers are handed around like the register slots
  void adopt_cbuf(size_t r, uint64_t* fresh);       // r's pending carries are now in `fresh`; its old buffer becomes spare
  void back_ext(size_t dst, uint32_t a, long copy_to, long add_src);
  // a whole product in one launch (plan token onelaunch): front, rows in `mode`, back with factor a and the extras of back_ext
  void one_launch(size_t r, int mode, const uint64_t* y, const uint64_t* y2, uint64_t* img, uint32_t a, long copy_to, long add_src, uint32_t level = 0);
  void normalize(size_t r);          // apply deferred run carries
  void carry_fix_now(size_t r, int excess = -1);   // run carries into the digits right away (plans with runs of two digits cannot defer
                                                   // them); excess: bits of a carry word above the first digit's width (-1: a <= 15)
  void scale(size_t r, uint32_t a);   // r x a, run-wise (k_scale): factors above pl_.a_fast
  void run_front(size_t r);          // digits(r) (+ pending run carries) -> work_
  void run_middle(const uint64_t* in, const uint64_t* y, uint64_t* out, int mode, const uint64_t* y2 = nullptr, uint64_t* img = nullptr);
  void run_back(size_t r, uint32_t a, hipEvent_t* ev = nullptr);
  // The engine's stream for everything that is not queued: the one place where a batch is flushed.  Whatever is put on the stream --
  // a launch, a copy, a memset, a synchronisation before a host copy -- asks for it here, so it runs behind the operations queued before it.
  hipStream_t stream() { if (batch_pending_) flush_batch(); return stream_; }
  void flush_batch();            // the queue as one launch of k_batch; then the other staging half is filled
  BatchOp& batch_slot();         // the next free descriptor of the queue (a full queue is flushed first)

  Plan pl_;
  DevPlan dp_{};
  CanonGeom cg_{};           // dp_ as canon.hip sees it (tile-major registers)
  int device_ = 0;
  bool verbose_ = false;
  hipStream_t stream_ = nullptr;
  size_t nregs_ = 0, reg_bytes_ = 0;
  size_t lanes_ = 1;         // residues per register (pl_.lanes)
  OneLaunchShape one_{};     // lanes per work-group and threads per lane of the one-launch products (plan.hpp onelaunch_shape)
  unsigned char* regs_ = nullptr;            // (reg_count + 1) slots of lanes x 8n bytes; the extra one is the work buffer
  std::vector<unsigned char*> slot_;          // slot_[r]: storage of register r; slot_[reg_count]: work buffer (swappable)
  uint64_t* cbuf_ = nullptr;                  // reg_count + 4 buffers of lanes x runs() carry words
  std::vector<uint64_t*> cb_, cb_spare_;      // cb_[r]: the buffer register r uses now
  void* tables_ = nullptr;
  uint64_t* split_ = nullptr;   // second work buffer of the split column sweeps (plan.split5: n = 5 2^26)
  uint64_t* f0_ = nullptr;   // four-step chain starts / ratios of the register-resident column kernels
  uint32_t* di_ = nullptr;   // digit-info words of the register-resident column kernels (plan.hpp DI)
  std::vector<uint8_t> kind_;
  std::vector<uint8_t> pending_carry_;   // cbuf(r) not yet folded into the digits (never on plans with C < 2)
  KernelChoice kc_;          // kernel variants of the sweeps (plan.hpp choose_kernels)
  ColSweeps cols_{};         // launchers of kc_.cols (none for the split sweeps)
  RowsFn rows_ = nullptr;    // launcher of kc_.rows
  std::vector<uint8_t> width_;   // natural order
  std::vector<uint32_t> stage_;  // host staging (one register of digits)
  uint32_t* canon_ = nullptr;    // device scratch of the canonicalisation: work arrays + two outputs of n digits (lazy)
  void* canon_lanes_ = nullptr;  // the same for a chunk of lanes (canon.hpp canon_chunk_lanes; lazy)
  size_t canon_lanes_chunk_ = 0; // lanes canon_lanes_ was made for
  std::vector<uint32_t> lane_flags_;   // host copy of a chunk's flag words
  bool host_carry_ = false;      // MI355_HOST_CARRY=1: compare / res64 / read-back through the host (A/B tests)
  // batches: descriptors are written into one of two pinned halves, go to the device buffer by a copy on the stream and are read there by
  // the launch behind it; a half is written again only after the event recorded behind the launch that read it
  bool batching_ = false;        // between batch_begin and batch_end
  size_t batch_pending_ = 0;     // descriptors in the half being filled
  int batch_half_ = 0;
  BatchOp* batch_stage_[2] = {nullptr, nullptr};   // pinned, kBatchCapacity descriptors each (made by the first batch_begin)
  hipEvent_t batch_read_[2] = {nullptr, nullptr};  // recorded behind the launch that read the half; null until there was one
  bool batch_in_flight_[2] = {false, false};
  BatchOp* batch_dev_ = nullptr;
  uint64_t batch_ops_ = 0, batch_launches_ = 0;    // batch_stats
};

}  // namespace mi355
