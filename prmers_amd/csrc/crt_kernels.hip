// Kernels of the squaring x <- x^2 a mod 2^p - 1 over GF(M61^2) x GF(M31^2) with a prime-factor (Good-Thomas) axis of radix 1, 3 or 9, and
// their launchers: the second field family of the reference.  Reference: the Aevum backend, third_party/aevum/src/cl/
// fft-middle.cl:663-720 (pfaDft3, radix 9 = 3 x 3 with scalar roots), pfaunpack.cl:12-56 (index map), carry.cl:506-588, policy
// README.md:907-926; CPU illustration docs/mersenne2_mixed_crt_2d_half_fast/mersenne2_mixed_crt_2d_half_fast.cpp ("m2:").
//
// n = odd * m words of up to 39 bits, m = 2^ln.  Logical digit j sits at grid coordinate (a, b) = (j mod odd, j mod m); there are no
// twiddles between the two axes (m2:733-758).  Row a of the grid is a real sequence of length m, held as h = m / 2 values of
// Z/p[i] (slot s = (b = 2s) + i (b = 2s + 1)), once for p = M61 (16 bytes a slot) and once for p = M31 (8 bytes): 12 bytes a word.
//   front      digits -> weight (bit rotations) -> DFT of length odd along a with scalar roots -> Z[a][s]
//   rows       half-length complex DFT of every row, h = H1 x H2 four-step (columns of H1 through LDS, twiddle omega_h^(k1 i2),
//              rows of H2 through LDS); frequency k = k1 + H1 k2 ends at slot k1 H2 + k2
//   pointwise  conjugate-symmetric untangling of the packed real rows, square, re-tangle (m2:829-915 in its textbook split form)
//   rows^-1, back: inverse odd DFT, 1 / (odd h), scatter to logical order; then the fused unweight + Garner + carry sweep (crt_carry.hpp)
// Two kernel sets for the rows: the straightforward one in this file (radix-2 butterflies in LDS, one launch per stage) and the radix-8
// one of crt_rows.hpp; see DESIGN.md for the measured cost.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "crt_arith.hpp"
#include "crt_carry.hpp"
#include "crt_kernels.hpp"
#include "crt_rows.hpp"

namespace mi355 {
namespace crt {

constexpr uint32_t kPassElems = 2048;   // complex values of one work-group of a row pass (32 KiB of LDS for M61)

template <class F>
__device__ __forceinline__ typename F::C tw_m(const typename F::C* __restrict__ U, uint32_t e, uint32_t h) {   // omega_m^e, e < m = 2h
  return e < h ? U[e] : cneg<F>(U[e - h]);
}

__device__ __forceinline__ uint32_t brev(uint32_t i, uint32_t bits) { return bits ? (__brev(i) >> (32 - bits)) : 0u; }

// ---- front: weight + odd axis --------------------------------------------------------------------------------------------
// thread = slot s (b = 2s, 2s + 1) of every row.  For t = 0 .. odd-1 the digit pair (b + m t) is one 16-byte load; digit j belongs to
// row a = j mod odd, which changes with t and b: the weighted values go through a private LDS column ([a][thread], no barrier) to
// reach the registers of the odd-axis DFT in row order.
template <int ODD>
__global__ void __launch_bounds__(256) k_front(Geom g, Grid gr, const uint64_t* __restrict__ x, F61::C* __restrict__ Z61, F31::C* __restrict__ Z31) {
  __shared__ uint64_t S61[2 * ODD][256];
  __shared__ uint32_t S31[2 * ODD][256];
  const uint32_t tid = threadIdx.x, s = blockIdx.x * 256 + tid;
  if (s >= gr.h) return;
  const uint32_t b = 2 * s;
  DigitWalk w; w.start(g, b);                             // digit b + m t: s = p j mod n advances by p m mod n
  uint32_t a = b % ODD;                                   // row of digit b + m t
#pragma unroll
  for (int t = 0; t < ODD; ++t) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(x + b + size_t(gr.m) * t);
    DigitWalk d = w;
    const uint32_t a1 = (a + 1 == ODD) ? 0 : a + 1;       // digit b + 1 + m t sits one row further
    S61[2 * a][tid] = rot61(red61(v.x), d.weight61()); S31[2 * a][tid] = rot31(red31(v.x), d.weight31());
    d.next(g);
    S61[2 * a1 + 1][tid] = rot61(red61(v.y), d.weight61()); S31[2 * a1 + 1][tid] = rot31(red31(v.y), d.weight31());
    w.next(g, gr.pm, gr.lpm61, gr.lpm31);
    a += gr.mm; if (a >= ODD) a -= ODD;
  }
  F61::C in61[ODD]; F31::C in31[ODD];
#pragma unroll
  for (int k = 0; k < ODD; ++k) { in61[k] = {S61[2 * k][tid], S61[2 * k + 1][tid]}; in31[k] = {S31[2 * k][tid], S31[2 * k + 1][tid]}; }
  dft_odd<F61, ODD>(in61, gr.r61, gr.c3_61);
  dft_odd<F31, ODD>(in31, gr.r31, gr.c3_31);
#pragma unroll
  for (int ka = 0; ka < ODD; ++ka) { Z61[size_t(ka) * gr.h + s] = in61[ka]; Z31[size_t(ka) * gr.h + s] = in31[ka]; }
}

// ---- back: inverse odd axis, 1 / (odd h), to logical order (16-byte and 8-byte stores of digit pairs) ----------------------
template <int ODD>
__global__ void __launch_bounds__(256) k_back(Grid gr, const F61::C* __restrict__ Z61, const F31::C* __restrict__ Z31, uint64_t* __restrict__ out61,
                                              uint32_t* __restrict__ out31) {
  __shared__ uint64_t S61[2 * ODD][256];
  __shared__ uint32_t S31[2 * ODD][256];
  const uint32_t tid = threadIdx.x, s = blockIdx.x * 256 + tid;
  if (s >= gr.h) return;
  back_to_planes<ODD>(gr, Z61, Z31, s, S61, S31);
  const uint32_t b = 2 * s;
  uint32_t a = b % ODD;
#pragma unroll
  for (int t = 0; t < ODD; ++t) {
    const uint32_t a1 = (a + 1 == ODD) ? 0 : a + 1;
    const size_t j = b + size_t(gr.m) * t;
    *reinterpret_cast<ulonglong2*>(out61 + j) = make_ulonglong2(S61[2 * a][tid], S61[2 * a1 + 1][tid]);
    *reinterpret_cast<uint2*>(out31 + j) = make_uint2(S31[2 * a][tid], S31[2 * a1 + 1][tid]);
    a += gr.mm; if (a >= ODD) a -= ODD;
  }
}

// ---- the carry sweep on residues in HBM (the pieces: crt_carry.hpp) -----------------------------------------------------------
// a run's residues (16-byte loads, all in flight before the carry chain starts; n is a multiple of kRun, checked on the host), then its
// digits with the sequential carry inside the run
__device__ __forceinline__ void carry_run(const Geom& g, const uint64_t* __restrict__ in61, const uint32_t* __restrict__ in31, uint32_t j0,
                                          uint64_t (&out)[kRun], uint32_t (&wd)[kRun], u128& carry) {
  uint64_t v61[kRun]; uint32_t v31[kRun];
  const ulonglong2* p61 = reinterpret_cast<const ulonglong2*>(in61 + j0);
  const uint4* p31 = reinterpret_cast<const uint4*>(in31 + j0);
#pragma unroll
  for (int k = 0; k < kRun / 2; ++k) { const ulonglong2 q = p61[k]; v61[2 * k] = q.x; v61[2 * k + 1] = q.y; }
#pragma unroll
  for (int k = 0; k < kRun / 4; ++k) { const uint4 q = p31[k]; v31[4 * k] = q.x; v31[4 * k + 1] = q.y; v31[4 * k + 2] = q.z; v31[4 * k + 3] = q.w; }
  DigitWalk dw; dw.start(g, j0);
#pragma unroll
  for (int k = 0; k < kRun; ++k) out[k] = carry_digit(g, dw, v61[k], v31[k], wd[k], carry);
}

// The sweep alone (mi355_crt_carry): digits[j]: value mod 2^width_j; carry_out[2 run .. 2 run + 1]: the 128-bit carry leaving the run
__global__ void __launch_bounds__(256) k_crt_runs(Geom g, const uint64_t* __restrict__ in61, const uint32_t* __restrict__ in31,
                                                  uint64_t* __restrict__ digits, uint64_t* __restrict__ carry_out) {
  const uint32_t run = blockIdx.x * 256 + threadIdx.x;
  const uint32_t j0 = run * kRun;
  if (j0 >= g.n) return;
  uint64_t out[kRun]; uint32_t wd[kRun];
  u128 carry = 0;
  carry_run(g, in61, in31, j0, out, wd, carry);
  store_run(digits, j0, out);
  carry_out[2 * size_t(run)] = uint64_t(carry);
  carry_out[2 * size_t(run) + 1] = uint64_t(carry >> 64);
}

// the carry word of the previous run (cyclically: 2^p = 1) goes through this run; what is left after its last digit (at most
// a few units) is returned in residual[run] for the final strong carry
__global__ void __launch_bounds__(256) k_crt_runs_fix(Geom g, uint64_t* __restrict__ digits, const uint64_t* __restrict__ carry_in, uint64_t* __restrict__ residual) {
  const uint32_t run = blockIdx.x * 256 + threadIdx.x;
  const uint32_t nruns = g.n / kRun;
  if (run >= nruns) return;
  const uint32_t prev = run ? run - 1 : nruns - 1;
  residual[run] = carry_through(g, digits, run * kRun, ((u128)carry_in[2 * size_t(prev) + 1] << 64) | carry_in[2 * size_t(prev)]);
}

// The same sweep with the run-to-run hand-over inside the work-group (the engine's path at odd 1 and in the two-kernel form): only the
// first run of a work-group depends on another work-group: edge_out[3 g .. 3 g + 2] = carry (128 bits) and leftover of the last run of
// group g, folded in by k_crt_edges (n / 2048 threads) -- instead of a second sweep over all digits (k_crt_runs_fix, 42 us at 9.4 M words).
__global__ void __launch_bounds__(256) k_crt_runs_linked(Geom g, const uint64_t* __restrict__ in61, const uint32_t* __restrict__ in31,
                                                         uint64_t* __restrict__ digits, uint64_t* __restrict__ edge_out) {
  __shared__ RunLink link;
  const uint32_t tid = threadIdx.x, run = blockIdx.x * 256 + tid;
  const uint32_t j0 = run * kRun;
  const bool live = j0 < g.n;
  uint64_t out[kRun]; uint32_t wd[kRun];
  u128 carry = 0;
  if (live) carry_run(g, in61, in31, j0, out, wd, carry);
  const uint64_t left = link_runs(link, out, wd, carry, live, tid == 0);
  if (live) store_run(digits, j0, out);
  // the last live run of the group hands over to the next group
  const uint32_t nruns = g.n / kRun, last = min(blockIdx.x * 256u + 255u, nruns - 1);
  if (run == last) store_edge(edge_out + 3 * size_t(blockIdx.x), carry, left);
}
// first run of every work-group: the carry of the previous group's last run (cyclically: 2^p = 1)
__global__ void __launch_bounds__(256) k_crt_edges(Geom g, uint64_t* __restrict__ digits, const uint64_t* __restrict__ edge) {
  const uint32_t grp = blockIdx.x * 256 + threadIdx.x;
  const uint32_t nruns = g.n / kRun, ngroups = (nruns + 255) / 256;
  if (grp >= ngroups) return;
  const uint32_t prev = grp ? grp - 1 : ngroups - 1, j0 = grp * 256u * kRun;
  fold_edge(g, digits, edge + 3 * size_t(prev), j0, (j0 + kRun) % g.n);
}

// ---- back + carry in one kernel: the inverse odd axis of 256 slots, then the carry sweep on the 2 x 256 x ODD digits they hold, straight
// out of LDS -- the unweighted residues (12 bytes a word) make no round trip through HBM between k_back and k_crt_runs_linked, and one
// launch goes.  The slots s0 .. s0 + 255 of a work-group hold ODD ranges of 512 consecutive digits, [2 s0 + m t, 2 s0 + 512 + m t): one
// thread per run of kRun digits (64 runs a range, ODD x 64 virtual threads on 256 real ones), run-to-run hand-over inside a range as in
// k_crt_runs_linked; edge_out[3 (ODD g + t) ..] = edge words of the last run of range t, folded into the following range by
// k_crt_range_edges (n / 512 threads).  Reference: third_party/aevum/src/cl/carry.cl:506-588 (carry), fft-middle.cl:663-720 (pfaDft).
template <int ODD>
__global__ void __launch_bounds__(256) k_back_carry(Geom g, Grid gr, const F61::C* __restrict__ Z61, const F31::C* __restrict__ Z31, uint64_t* __restrict__ digits,
                                                    uint64_t* __restrict__ edge_out) {
  __shared__ uint64_t S61[2 * ODD][256];
  __shared__ uint32_t S31[2 * ODD][256];
  __shared__ RunLink link;
  const uint32_t tid = threadIdx.x, s0 = blockIdx.x * 256;   // h is a multiple of 256 on this path (choose_kernels)
  back_to_planes<ODD>(gr, Z61, Z31, s0 + tid, S61, S31);
  __syncthreads();
  for (uint32_t base = 0; base < uint32_t(ODD) * 64u; base += 256u) {
    const uint32_t vt = base + tid, t = vt >> 6, r = tid & 63u;   // range, run inside the range (base is a multiple of 256)
    const bool live = vt < uint32_t(ODD) * 64u;
    uint64_t out[kRun]; uint32_t wd[kRun];
    u128 carry = 0;
    uint32_t j0 = 0;
    if (live) {
      const uint32_t sl0 = 4u * r;
      j0 = 2u * (s0 + sl0) + gr.m * t;
      DigitWalk dw; dw.start(g, j0);
      const uint32_t a0 = (2u * (s0 + sl0) + gr.mm * t) % uint32_t(ODD);   // row of digit j0 (j mod ODD with m = mm mod ODD)
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const uint32_t sl = sl0 + uint32_t(k >> 1);
        const uint32_t a = (a0 + uint32_t(k)) % uint32_t(ODD);            // digit j0 + k sits in row (j0 + k) mod ODD
        const uint32_t plane = 2u * a + uint32_t(k & 1);                   // even position: re, odd position: im
        out[k] = carry_digit(g, dw, S61[plane][sl], S31[plane][sl], wd[k], carry);
      }
    }
    const uint64_t left = link_runs(link, out, wd, carry, live, r == 0);
    if (live) {
      store_run(digits, j0, out);
      if (r == 63u) store_edge(edge_out + 3 * (size_t(blockIdx.x) * ODD + t), carry, left);
    }
    __syncthreads();   // the hand-over words are reused by the next ranges
  }
}
// first run of every range: the carry of the range before it in digit order (same t of the previous work-group; the last group's range t - 1
// for the first group; cyclically, 2^p = 1) -- k_crt_edges for the ranges of k_back_carry
__global__ void __launch_bounds__(256) k_crt_range_edges(Geom g, Grid gr, uint64_t* __restrict__ digits, const uint64_t* __restrict__ edge) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x, G = gr.h >> 8, odd = gr.odd;
  if (idx >= G * odd) return;
  const uint32_t grp = idx / odd, t = idx - grp * odd;
  const uint32_t prev = grp ? (grp - 1) * odd + t : (G - 1) * odd + (t ? t - 1 : odd - 1);
  const uint32_t j0 = 512u * grp + gr.m * t;
  fold_edge(g, digits, edge + 3 * size_t(prev), j0, j0 + kRun);   // (a range has 512 digits: the next run is still inside it)
}

// ---- one pass of the row transforms --------------------------------------------------------------------------------------
// A work-group holds CA transforms of length L = 2^logL in LDS.  cols != 0: the transforms are the columns i2 .. i2 + CA - 1 of
// the H1 x H2 view of one row (stride H2), followed (forward) or preceded (inverse) by the four-step twiddle omega_h^(+-k1 i2);
// cols == 0: they are CA consecutive contiguous segments (the rows of that view, or whole grid rows when H1 = 1).
// Radix-2 decimation in frequency; the bit-reversed result is read back in natural order.
template <class F>
__global__ void __launch_bounds__(256) k_pass(Grid gr, typename F::C* __restrict__ Z, const typename F::C* __restrict__ U, uint32_t logL, uint32_t CA,
                                              int cols, int inverse) {
  using C = typename F::C;
  __shared__ C X[kPassElems];
  const uint32_t L = 1u << logL, tid = threadIdx.x, nt = blockDim.x;
  const uint32_t per_row = gr.h >> logL;               // transforms per grid row
  const uint32_t d0 = blockIdx.x * CA;                 // first transform of this group (CA divides per_row)
  const uint32_t row = d0 / per_row, r0 = d0 - row * per_row;
  C* base = Z + size_t(row) * gr.h;
  const uint32_t H2 = 1u << gr.logH2;
  // load
  for (uint32_t e = tid; e < CA * L; e += nt) {
    uint32_t c, i; size_t addr;
    if (cols) { c = e % CA; i = e / CA; addr = size_t(i) * H2 + (r0 + c); }
    else { i = e & (L - 1); c = e >> logL; addr = size_t(r0 + c) * L + i; }
    C v = base[addr];
    if (cols && inverse) {   // conj(omega_h^(k1 i2)) = conj(omega_m^(2 k1 i2)): here i is k1
      v = cmul<F>(v, cconj<F>(tw_m<F>(U, 2u * i * (r0 + c), gr.h)));
    }
    X[c * L + i] = v;
  }
  // butterflies
  const uint32_t ushift = gr.ln - logL;                // omega_L^j = omega_m^(j m / L)
  for (uint32_t half = L >> 1, sh = 0; half >= 1; half >>= 1, ++sh) {
    __syncthreads();
    for (uint32_t bfy = tid; bfy < CA * (L >> 1); bfy += nt) {
      const uint32_t c = bfy / (L >> 1), q = bfy - c * (L >> 1);
      const uint32_t j = q & (half - 1), i = ((q - j) << 1) + j;
      const C u = X[c * L + i], v = X[c * L + i + half];
      C w = U[size_t(j << sh) << ushift];
      if (inverse) w = cconj<F>(w);
      X[c * L + i] = cadd<F>(u, v);
      X[c * L + i + half] = (j == 0) ? csub<F>(u, v) : cmul<F>(csub<F>(u, v), w);
    }
  }
  __syncthreads();
  // store, natural order
  for (uint32_t e = tid; e < CA * L; e += nt) {
    uint32_t c, k; size_t addr;
    if (cols) { c = e % CA; k = e / CA; addr = size_t(k) * H2 + (r0 + c); }
    else { k = e & (L - 1); c = e >> logL; addr = size_t(r0 + c) * L + k; }
    C v = X[c * L + brev(k, logL)];
    if (cols && !inverse) v = cmul<F>(v, tw_m<F>(U, 2u * k * (r0 + c), gr.h));
    base[addr] = v;
  }
}

// ---- pointwise -----------------------------------------------------------------------------------------------------------
// Row of m reals packed as h complex values z; Z = DFT_h(z).  With W = omega_m:
//   X_k = (Z_k + conj Z_{-k}) / 2 + W^k (Z_k - conj Z_{-k}) / (2i)          k = 0 .. h      (the real sequence's spectrum)
//   Y_k = X_k^2
//   Z'_k = (Y_k + conj Y_{h-k}) / 2 + i conj(W^k) (Y_k - conj Y_{h-k}) / 2  k = 0 .. h - 1  (packed spectrum of the square)
// One thread owns the pair (k, h - k), k <= h / 2; frequency k = k1 + H1 k2 sits at slot k1 H2 + k2.
__device__ __forceinline__ uint32_t slot_of(const Grid& gr, uint32_t k) { return ((k & ((1u << gr.logH1) - 1)) << gr.logH2) + (k >> gr.logH1); }

template <class F>
__device__ __forceinline__ typename F::C repack(typename F::C yk, typename F::C yhk, typename F::C w) {
  const typename F::C yc = cconj<F>(yhk);
  const typename F::C e = cadd<F>(yk, yc), d = cmul<F>(csub<F>(yk, yc), cconj<F>(w));
  return chalf<F>(cadd<F>(e, cmul_i<F>(d)));
}

template <class F>
__device__ __forceinline__ typename F::C spectrum_lin(typename F::C zk, typename F::C zmk, typename F::C w) {
  const typename F::C zc = cconj<F>(zmk);
  const typename F::C e = cadd<F>(zk, zc), o = cdiv_i<F>(csub<F>(zk, zc));
  return chalf<F>(cadd<F>(e, cmul<F>(w, o)));
}
// I == nullptr: square; otherwise multiply by the packed spectrum I (same slot order)
template <class F>
__global__ void __launch_bounds__(256) k_pointwise(Grid gr, typename F::C* __restrict__ Z, const typename F::C* __restrict__ U, const typename F::C* __restrict__ I) {
  using C = typename F::C;
  const uint32_t per_row = (gr.h >> 1) + 1;
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= per_row * gr.odd) return;
  const uint32_t row = idx / per_row, k = idx - row * per_row;
  C* z = Z + size_t(row) * gr.h;
  const C* im = I ? I + size_t(row) * gr.h : nullptr;
  const uint32_t h = gr.h;
  auto prod = [&](C zk, C zmk, C ik, C imk, C w) {
    const C x = spectrum_lin<F>(zk, zmk, w);
    return im ? cmul<F>(x, spectrum_lin<F>(ik, imk, w)) : csqr<F>(x);
  };
  if (k == 0) {
    const C z0 = z[0], i0 = im ? im[0] : z0;
    const C y0 = prod(z0, z0, i0, i0, U[0]);              // X_0
    const C yh = prod(z0, z0, i0, i0, U[h]);              // X_h (W^h = -1)
    z[0] = repack<F>(y0, yh, U[0]);
    if (h >= 2) {   // the self-paired middle slot
      const uint32_t sm = slot_of(gr, h >> 1);
      const C zm = z[sm], imm = im ? im[sm] : zm;
      const C ym = prod(zm, zm, imm, imm, U[h >> 1]);
      z[sm] = repack<F>(ym, ym, U[h >> 1]);
    }
    return;
  }
  if (2 * k >= h) return;   // k = h / 2 was handled with k = 0
  const uint32_t sa = slot_of(gr, k), sb = slot_of(gr, h - k);
  const C za = z[sa], zb = z[sb];
  const C ia = im ? im[sa] : za, ib = im ? im[sb] : zb;
  const C wa = U[k], wb = U[h - k];
  const C ya = prod(za, zb, ia, ib, wa), yb = prod(zb, za, ib, ia, wb);
  z[sa] = repack<F>(ya, yb, wa);
  z[sb] = repack<F>(yb, ya, wb);
}

// dst[j] += src[j]: digit-wise sum of two weakly carried residues (one more bit per digit; the next squaring's carry sweep absorbs it)
__global__ void __launch_bounds__(256) k_add_digits(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, uint32_t n) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) dst[j] += src[j];
}

// ---- small helpers -------------------------------------------------------------------------------------------------------
__global__ void k_set_small(Geom g, uint64_t* __restrict__ x, uint32_t a) {   // x = a (one thread: a touches at most a few digits)
  if (blockIdx.x || threadIdx.x) return;
  uint64_t v = a;
  DigitWalk dw; dw.start(g, 0);
  for (uint32_t j = 0; j < g.n && v; ++j) { const uint32_t w = dw.width(g); x[j] = v & ((uint64_t(1) << w) - 1); v >>= w; dw.next(g); }
}
__global__ void k_sub_small(Geom g, uint64_t* __restrict__ x, uint32_t a) {   // x -= a with borrow and wrap-around (m2:1095-1111)
  if (blockIdx.x || threadIdx.x) return;
  uint64_t borrow = a;
  for (int lap = 0; lap < 3 && borrow; ++lap) {
    DigitWalk dw; dw.start(g, 0);
    for (uint32_t j = 0; j < g.n && borrow; ++j) {
      const uint32_t w = dw.width(g);
      const uint64_t v = x[j];
      if (v >= borrow) { x[j] = v - borrow; borrow = 0; }
      else { const uint64_t need = borrow - v, k = (need + (uint64_t(1) << w) - 1) >> w; x[j] = v + (k << w) - borrow; borrow = k; }
      dw.next(g);
    }
  }
}

// ==========================================================================================================================
// host: kernel choice and launchers
// ==========================================================================================================================
namespace {
constexpr uint32_t kSlots61 = 4096, kSlots31 = 8192;   // slots per work-group of the one-field column kernels (68 KiB of LDS each)
constexpr size_t kLds61 = size_t(kSlots61 + kSlots61 / 16) * 16, kLds31 = size_t(kSlots31 + kSlots31 / 16) * 8;
const dim3 b256(256);
dim3 slot_groups(const Grid& gr) { return dim3((gr.h + 255) / 256); }
}  // namespace

CrtKernels choose_kernels(const Grid& gr, const char* set) {
  auto is = [&](const char* name) { return set && std::strcmp(set, name) == 0; };
  CrtKernels k;
  k.radix8 = gr.logH2 == 10 && gr.logH1 >= 1 && gr.logH1 <= 11 && !is("generic");
  // columns: one field per launch where that gives wider row segments (H2 columns must hold at least one group of each kind).
  // Measured: at H1 = 512 the joint kernel is faster (0.121 / 0.114 ms against 0.150 / 0.132), from H1 = 1024 on the split ones are
  k.cols_split = k.radix8 && !is("joint") && (gr.logH1 >= 10 || is("split")) && (kSlots31 >> gr.logH1) >= 1 && (kSlots31 >> gr.logH1) <= (1u << gr.logH2);
  // back + carry fused wherever a work-group has whole ranges of 512 digits; MI355_CRT_TUNE bit 1: the two-kernel form
  k.back_fused = gr.odd > 1 && (gr.h & 255u) == 0 && !(gr.tune & 2u);
  return k;
}

hipError_t configure(const CrtKernels& k) {
  if (!k.radix8) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cols_one<F61, false, kSlots61>), hipFuncAttributeMaxDynamicSharedMemorySize, int(kLds61));
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cols_one<F61, true, kSlots61>), hipFuncAttributeMaxDynamicSharedMemorySize, int(kLds61));
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cols_one<F31, false, kSlots31>), hipFuncAttributeMaxDynamicSharedMemorySize, int(kLds31));
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cols_one<F31, true, kSlots31>), hipFuncAttributeMaxDynamicSharedMemorySize, int(kLds31));
  return e;
}

// three words per chain of runs: k_crt_runs_linked writes one chain per work-group of 256 runs, ceil(n / kRun / 256) of them; k_back_carry
// one per range of 512 digits, odd ranges in each of its h / 256 work-groups (it runs only where 256 divides h)
size_t edge_words(const Geom& g, const Grid& gr) {
  const size_t groups = (size_t(g.n) / kRun + 255) / 256, ranges = size_t(gr.h >> 8) * gr.odd;
  return 3 * std::max(groups, ranges);
}

void launch_front(const Geom& g, const Grid& gr, const uint64_t* x, Work Z, hipStream_t s) {
  switch (gr.odd) {
    case 1: hipLaunchKernelGGL((k_front<1>), slot_groups(gr), b256, 0, s, g, gr, x, Z.Z61, Z.Z31); break;
    case 3: hipLaunchKernelGGL((k_front<3>), slot_groups(gr), b256, 0, s, g, gr, x, Z.Z61, Z.Z31); break;
    default: hipLaunchKernelGGL((k_front<9>), slot_groups(gr), b256, 0, s, g, gr, x, Z.Z61, Z.Z31); break;
  }
}

void launch_cols(const Grid& gr, const FastTables& T, bool split, bool inverse, Work Z, hipStream_t s) {
  const uint32_t H2 = 1u << gr.logH2;
  if (!split) {
    const dim3 grid(gr.odd * (H2 / (kFastSlots >> gr.logH1)));
    if (inverse) hipLaunchKernelGGL((k_cols_fast<true>), grid, b256, kFastLdsBytes, s, gr, T, Z.Z61, Z.Z31);
    else hipLaunchKernelGGL((k_cols_fast<false>), grid, b256, kFastLdsBytes, s, gr, T, Z.Z61, Z.Z31);
    return;
  }
  const dim3 g61(gr.odd * H2 / std::max(1u, kSlots61 >> gr.logH1)), g31(gr.odd * H2 / std::max(1u, kSlots31 >> gr.logH1));
  if (inverse) {
    hipLaunchKernelGGL((k_cols_one<F61, true, kSlots61>), g61, dim3(kSlots61 / 8), kLds61, s, gr, T.w1_61, T.lo61, T.hi61, Z.Z61);
    hipLaunchKernelGGL((k_cols_one<F31, true, kSlots31>), g31, dim3(kSlots31 / 8), kLds31, s, gr, T.w1_31, T.lo31, T.hi31, Z.Z31);
  } else {
    hipLaunchKernelGGL((k_cols_one<F61, false, kSlots61>), g61, dim3(kSlots61 / 8), kLds61, s, gr, T.w1_61, T.lo61, T.hi61, Z.Z61);
    hipLaunchKernelGGL((k_cols_one<F31, false, kSlots31>), g31, dim3(kSlots31 / 8), kLds31, s, gr, T.w1_31, T.lo31, T.hi31, Z.Z31);
  }
}

void launch_mid(const Grid& gr, const FastTables& T, int mode, Work Z, F61::C* i61, F31::C* i31, hipStream_t s) {
  const dim3 grid(gr.odd * (1u << gr.logH1) / 2);
  if (mode == 0) hipLaunchKernelGGL((k_mid_fast<0>), grid, b256, kFastLdsBytes, s, gr, T, Z.Z61, Z.Z31, i61, i31);
  else if (mode == 1) hipLaunchKernelGGL((k_mid_fast<1>), grid, b256, kFastLdsBytes, s, gr, T, Z.Z61, Z.Z31, i61, i31);
  else hipLaunchKernelGGL((k_mid_fast<2>), grid, b256, kFastLdsBytes, s, gr, T, Z.Z61, Z.Z31, i61, i31);
}

template <class F>
static void launch_rows(const Grid& gr, typename F::C* Z, const typename F::C* U, bool inverse, hipStream_t s) {
  auto pass = [&](uint32_t logL, int cols) {
    const uint32_t L = 1u << logL;
    uint32_t CA = std::max<uint32_t>(1, kPassElems / L);
    const uint32_t per_row = gr.h >> logL;
    CA = std::min(CA, per_row);                       // powers of two: CA divides per_row
    const uint32_t groups = gr.odd * per_row / CA;
    hipLaunchKernelGGL((k_pass<F>), dim3(groups), b256, 0, s, gr, Z, U, logL, CA, cols, inverse ? 1 : 0);
  };
  if (!inverse) {
    if (gr.logH1) pass(gr.logH1, 1);
    pass(gr.logH2, 0);
  } else {
    pass(gr.logH2, 0);
    if (gr.logH1) pass(gr.logH1, 1);
  }
}
void launch_rows_generic(const Grid& gr, const FastTables& T, bool inverse, Work Z, hipStream_t s) {
  launch_rows<F61>(gr, Z.Z61, T.u61, inverse, s);
  launch_rows<F31>(gr, Z.Z31, T.u31, inverse, s);
}

void launch_pointwise(const Grid& gr, const FastTables& T, Work Z, const F61::C* i61, const F31::C* i31, hipStream_t s) {
  const uint32_t pw = ((gr.h >> 1) + 1) * gr.odd;
  hipLaunchKernelGGL((k_pointwise<F61>), dim3((pw + 255) / 256), b256, 0, s, gr, Z.Z61, T.u61, i61);
  hipLaunchKernelGGL((k_pointwise<F31>), dim3((pw + 255) / 256), b256, 0, s, gr, Z.Z31, T.u31, i31);
}

void launch_back(const Grid& gr, Work Z, uint64_t* out61, uint32_t* out31, hipStream_t s) {
  switch (gr.odd) {
    case 1: hipLaunchKernelGGL((k_back<1>), slot_groups(gr), b256, 0, s, gr, Z.Z61, Z.Z31, out61, out31); break;
    case 3: hipLaunchKernelGGL((k_back<3>), slot_groups(gr), b256, 0, s, gr, Z.Z61, Z.Z31, out61, out31); break;
    default: hipLaunchKernelGGL((k_back<9>), slot_groups(gr), b256, 0, s, gr, Z.Z61, Z.Z31, out61, out31); break;
  }
}

void launch_back_carry(const Geom& g, const Grid& gr, Work Z, uint64_t* digits, uint64_t* edge, hipStream_t s) {
  const dim3 grid(gr.h >> 8);
  switch (gr.odd) {   // (odd 1 has no fused form: choose_kernels)
    case 3: hipLaunchKernelGGL((k_back_carry<3>), grid, b256, 0, s, g, gr, Z.Z61, Z.Z31, digits, edge); break;
    case 9: hipLaunchKernelGGL((k_back_carry<9>), grid, b256, 0, s, g, gr, Z.Z61, Z.Z31, digits, edge); break;
    default: throw std::logic_error("crt kernels: back + carry in one kernel needs odd 3 or 9");
  }
}
void launch_range_edges(const Geom& g, const Grid& gr, uint64_t* digits, const uint64_t* edge, hipStream_t s) {
  hipLaunchKernelGGL(k_crt_range_edges, dim3((uint32_t(gr.h >> 8) * gr.odd + 255) / 256), b256, 0, s, g, gr, digits, edge);
}

void launch_carry_linked(const Geom& g, const uint64_t* in61, const uint32_t* in31, uint64_t* digits, uint64_t* edge, hipStream_t s) {
  const uint32_t nruns = g.n / kRun, groups = (nruns + 255) / 256;
  hipLaunchKernelGGL(k_crt_runs_linked, dim3(groups), b256, 0, s, g, in61, in31, digits, edge);
  hipLaunchKernelGGL(k_crt_edges, dim3((groups + 255) / 256), b256, 0, s, g, digits, edge);
}

void launch_add_digits(uint64_t* dst, const uint64_t* src, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_add_digits, dim3((n + 255) / 256), b256, 0, s, dst, src, n);
}
void launch_set_small(const Geom& g, uint64_t* x, uint32_t a, hipStream_t s) { hipLaunchKernelGGL(k_set_small, dim3(1), dim3(1), 0, s, g, x, a); }
void launch_sub_small(const Geom& g, uint64_t* x, uint32_t a, hipStream_t s) { hipLaunchKernelGGL(k_sub_small, dim3(1), dim3(1), 0, s, g, x, a); }

}  // namespace crt

// The sweep alone, host buffers in, host buffers out (mi355_crt_carry: a parity / timing entry point; the resident engine is
// crt_engine.hip): k_crt_runs + k_crt_runs_fix, digits and the per-run residual; returns the time of the two kernels in ms through
// *kernel_ms when it is non-null
void crt_carry_host(uint32_t p, size_t n, uint32_t odd, uint32_t a, const uint64_t* in61, const uint32_t* in31, uint64_t* digits_out,
                    uint64_t* residual_out, int device, double* kernel_ms) {
  using namespace crt;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available: the MI355X engine has no CPU fallback");
  auto chk = [](hipError_t e, const char* what) { if (e != hipSuccess) throw std::runtime_error(std::string("crt_carry: ") + what + ": " + hipGetErrorString(e)); };
  const Geom g = make_geom(p, n, odd, a);
  chk(hipSetDevice(device), "hipSetDevice");
  const size_t nruns = n / kRun;
  const dim3 grid(uint32_t((nruns + 255) / 256));
  uint64_t *d61 = nullptr, *dd = nullptr, *dc = nullptr, *dr = nullptr; uint32_t* d31 = nullptr;
  chk(hipMalloc(reinterpret_cast<void**>(&d61), n * 8), "hipMalloc"); chk(hipMalloc(reinterpret_cast<void**>(&d31), n * 4), "hipMalloc");
  chk(hipMalloc(reinterpret_cast<void**>(&dd), n * 8), "hipMalloc"); chk(hipMalloc(reinterpret_cast<void**>(&dc), nruns * 16), "hipMalloc");
  chk(hipMalloc(reinterpret_cast<void**>(&dr), nruns * 8), "hipMalloc");
  chk(hipMemcpy(d61, in61, n * 8, hipMemcpyHostToDevice), "copy"); chk(hipMemcpy(d31, in31, n * 4, hipMemcpyHostToDevice), "copy");
  hipEvent_t e0, e1;
  chk(hipEventCreate(&e0), "event"); chk(hipEventCreate(&e1), "event");
  for (int rep = 0; rep < (kernel_ms ? 5 : 1); ++rep) {   // timed runs repeat the sweep (same inputs, same outputs)
    chk(hipEventRecord(e0), "event");
    hipLaunchKernelGGL(k_crt_runs, grid, b256, 0, nullptr, g, d61, d31, dd, dc);
    hipLaunchKernelGGL(k_crt_runs_fix, grid, b256, 0, nullptr, g, dd, dc, dr);
    chk(hipEventRecord(e1), "event");
    chk(hipEventSynchronize(e1), "sync");
  }
  chk(hipGetLastError(), "launch");
  if (kernel_ms) { float ms = 0; chk(hipEventElapsedTime(&ms, e0, e1), "elapsed"); *kernel_ms = ms; }
  chk(hipMemcpy(digits_out, dd, n * 8, hipMemcpyDeviceToHost), "copy"); chk(hipMemcpy(residual_out, dr, nruns * 8, hipMemcpyDeviceToHost), "copy");
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(d61); (void)hipFree(d31); (void)hipFree(dd); (void)hipFree(dc); (void)hipFree(dr);
}

}  // namespace mi355
