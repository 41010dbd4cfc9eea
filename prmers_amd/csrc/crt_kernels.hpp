// Device-side view of a GF(M61^2) x GF(M31^2) transform and the launch entry points of its kernels (crt_kernels.hip).  The engine
// (crt_engine.hip) fills a Grid and the tables once, takes the kernel choice of its size once and calls one launcher per stage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crt_field.hpp"

namespace mi355 {
namespace crt {

struct Grid {
  uint32_t odd, ln, m, h, logh, logH1, logH2, minv;   // h = 2^logh = H1 H2; minv = m^-1 mod odd
  uint64_t r61[9], r61i[9], s61, c3_61;               // odd-root powers r^e, their inverses, 1 / (odd h), (w3 - w3^2) / 2
  uint32_t r31[9], r31i[9], s31, c3_31;
  uint32_t mm, pm, lpm61, lpm31;                      // m mod odd; p m mod n and its images l61 (p m) mod 61, l31 (p m) mod 31
  uint32_t tune;                                      // MI355_CRT_TUNE (A/B runs): bit 0 plain tile order in the column kernels, bit 1 back and carry as two kernels
};

struct FastTables {   // per field: omega_L^x for the two pass lengths (x < L), omega_m^(H1 k2) (k2 < H2), omega_m^k (k <= h),
                      // and the two-level table of the four-step twiddles: omega_m^e = lo[e & 1023] * hi[e >> 10] (e < m)
  const F61::C *w1_61, *w2_61, *v61, *u61, *lo61, *hi61;   // (the generic kernels read u61 / u31 only)
  const F31::C *w1_31, *w2_31, *v31, *u31, *lo31, *hi31;
};

struct Work { F61::C* Z61; F31::C* Z31; };   // [odd][h] slots per field

// Which kernels serve a size, chosen once per engine.  set = MI355_CRT_KERNELS: "generic" the radix-2 row passes, "joint" / "split" both
// fields in one column launch / one field per launch (A/B runs and tests); null: the measured default.
struct CrtKernels {
  bool radix8;       // crt_rows.hpp (rows of 1024, columns of 2 .. 2048) instead of k_pass + k_pointwise
  bool cols_split;   // k_cols_one per field instead of k_cols_fast
  bool back_fused;   // k_back_carry + k_crt_range_edges instead of k_back + k_crt_runs_linked + k_crt_edges
};
CrtKernels choose_kernels(const Grid& gr, const char* set);
hipError_t configure(const CrtKernels& k);   // the dynamic-LDS attributes of the chosen kernels (current device)
size_t edge_words(const Geom& g, const Grid& gr);   // size of the edge buffer of the carry sweeps, in 64-bit words

// one launcher per stage; mode 0: square, 1: forward only, the packed spectrum goes to the image (i61, i31), 2: multiply by that image
void launch_front(const Geom& g, const Grid& gr, const uint64_t* x, Work Z, hipStream_t s);
void launch_cols(const Grid& gr, const FastTables& T, bool split, bool inverse, Work Z, hipStream_t s);
void launch_mid(const Grid& gr, const FastTables& T, int mode, Work Z, F61::C* i61, F31::C* i31, hipStream_t s);
void launch_rows_generic(const Grid& gr, const FastTables& T, bool inverse, Work Z, hipStream_t s);
void launch_pointwise(const Grid& gr, const FastTables& T, Work Z, const F61::C* i61, const F31::C* i31, hipStream_t s);
void launch_back(const Grid& gr, Work Z, uint64_t* out61, uint32_t* out31, hipStream_t s);
void launch_back_carry(const Geom& g, const Grid& gr, Work Z, uint64_t* digits, uint64_t* edge, hipStream_t s);
void launch_range_edges(const Geom& g, const Grid& gr, uint64_t* digits, const uint64_t* edge, hipStream_t s);
// the unweight + Garner + carry sweep on the residues of k_back: run-to-run hand-over inside a work-group, then the group edges
void launch_carry_linked(const Geom& g, const uint64_t* in61, const uint32_t* in31, uint64_t* digits, uint64_t* edge, hipStream_t s);
void launch_add_digits(uint64_t* dst, const uint64_t* src, uint32_t n, hipStream_t s);
void launch_set_small(const Geom& g, uint64_t* x, uint32_t a, hipStream_t s);
void launch_sub_small(const Geom& g, uint64_t* x, uint32_t a, hipStream_t s);

}  // namespace crt

// mi355_crt_carry: the carry sweep on its own, on caller-supplied residues of both fields (tests/test_gpu_crt_carry.py)
void crt_carry_host(uint32_t p, size_t n, uint32_t odd, uint32_t a, const uint64_t* in61, const uint32_t* in31, uint64_t* digits_out,
                    uint64_t* residual_out, int device, double* kernel_ms);

}  // namespace mi355
