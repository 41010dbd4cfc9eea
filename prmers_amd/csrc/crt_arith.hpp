// Arithmetic of the second field family that the kernels of crt_kernels.hip (crt_rows.hpp, crt_carry.hpp) are built from, host + gfx950 device and
// includable by a plain C++ compiler: the 8th-root rotations, the lazy Z/M61 forms with their radix-2/4/8 butterflies, the limb-wise
// complex products, the generic butterflies and the odd-axis DFTs.  No LDS, grid or table code here: a kernel and a CPU test
// (tests/host/test_crt_primitives.cpp) instantiate the same templates.
#pragma once
#include "crt_field.hpp"

namespace mi355 {
namespace crt {

// multiplication by the 8th root (1 + i) / sqrt 2 and by its conjugate: 1 / sqrt 2 = 2^30 in Z/M61, 2^15 in Z/M31
template <class F> struct Rot8;
template <> struct Rot8<F61> { static GF_HDM uint64_t r(uint64_t a) { return rot61(a, 30); } };
template <> struct Rot8<F31> { static GF_HDM uint32_t r(uint32_t a) { return rot31(a, 15); } };
template <class F, bool INV>
GF_HD typename F::C mul_w8(typename F::C a) {
  if (!INV) return {Rot8<F>::r(F::sub(a.re, a.im)), Rot8<F>::r(F::add(a.re, a.im))};
  return {Rot8<F>::r(F::add(a.re, a.im)), Rot8<F>::r(F::sub(a.im, a.re))};
}
template <class F, bool INV>
GF_HD typename F::C mul_w4(typename F::C a) { return INV ? cdiv_i<F>(a) : cmul_i<F>(a); }   // omega_4 = i

// ---- Z/M61 without a reduction per operation -------------------------------------------------------------------------------------
// M61 leaves three spare bits in a 64-bit register, exactly what the three levels of a radix-8 butterfly need: with canonical inputs
// (<= M61) the sums are plain 64-bit additions (one v_lshl_add_u64) and a difference is a + (K - b) with K = M61, 2 M61, 4 M61 at the
// three levels, so every intermediate stays <= 8 M61 = 2^64 - 8.  The products fold their operands once ((v & M61) + (v >> 61) <= M61 + 7),
// split them into 31-bit limbs and accumulate both products of a complex component limb-wise in 64-bit multiply-adds
// (re = a c + b (M61 - d): M61 - d is a bit complement of d's limbs), with ONE reduction per component: 16 multiply-adds and two
// reductions per complex product instead of four full multiplications with a reduction each.
constexpr uint64_t K1 = M61, K2 = 2 * M61, K4 = 4 * M61;
GF_HD uint64_t fold61(uint64_t v) { return (v & M61) + (v >> 61); }                    // any v -> <= M61 + 7
GF_HD uint64_t canon61(uint64_t v) { v = fold61(v); return v >= M61 ? v - M61 : v; }  // any v -> [0, M61)
GF_HD uint64_t shl30_61(uint64_t v) { return ((v & 0x7fffffffull) << 30) + (v >> 31); } // v 2^30, any v -> < 2^61 + 2^33
struct Lz61 { uint64_t re, im; };   // lazy complex value; bounds are tracked in the comments of the callers

template <bool INV, uint64_t K>   // x * omega_8 (or its conjugate); components <= K on entry, <= 2 M61 on exit (K <= 2 M61)
GF_HD Lz61 lz_w8(Lz61 a) {
  if (!INV) return {shl30_61(a.re + (K - a.im)), shl30_61(a.re + a.im)};
  return {shl30_61(a.re + a.im), shl30_61(a.im + (K - a.re))};
}
template <bool INV, uint64_t K>   // x * i (or / i); components <= K stay <= K
GF_HD Lz61 lz_w4(Lz61 a) { return INV ? Lz61{a.im, K - a.re} : Lz61{K - a.im, a.re}; }
template <uint64_t K> GF_HD Lz61 lz_add(Lz61 a, Lz61 b) { return {a.re + b.re, a.im + b.im}; }
template <uint64_t K> GF_HD Lz61 lz_sub(Lz61 a, Lz61 b) { return {a.re + (K - b.re), a.im + (K - b.im)}; }   // b <= K

// canonical in (<= M61), lazy out (<= 8 M61 for R = 8, 4 M61 for R = 4, 2 M61 for R = 2)
template <int R, bool INV>
GF_HD void bfly61(Lz61 (&x)[R]) {
  if constexpr (R == 2) {
    const Lz61 a = lz_add<K1>(x[0], x[1]), b = lz_sub<K1>(x[0], x[1]);
    x[0] = a; x[1] = b;
  } else if constexpr (R == 4) {
    const Lz61 a0 = lz_add<K1>(x[0], x[2]), a1 = lz_add<K1>(x[1], x[3]), b0 = lz_sub<K1>(x[0], x[2]), b1 = lz_w4<INV, K2>(lz_sub<K1>(x[1], x[3]));
    x[0] = lz_add<K2>(a0, a1); x[2] = lz_sub<K2>(a0, a1); x[1] = lz_add<K2>(b0, b1); x[3] = lz_sub<K2>(b0, b1);
  } else {
    const Lz61 a0 = lz_add<K1>(x[0], x[4]), a1 = lz_add<K1>(x[1], x[5]), a2 = lz_add<K1>(x[2], x[6]), a3 = lz_add<K1>(x[3], x[7]);           // <= 2 M61
    const Lz61 b0 = lz_sub<K1>(x[0], x[4]), b1 = lz_w8<INV, K2>(lz_sub<K1>(x[1], x[5])), b2 = lz_w4<INV, K2>(lz_sub<K1>(x[2], x[6])),
              b3 = lz_w4<INV, K2>(lz_w8<INV, K2>(lz_sub<K1>(x[3], x[7])));                                                                  // <= 2 M61
    const Lz61 c0 = lz_add<K2>(a0, a2), c1 = lz_add<K2>(a1, a3), d0 = lz_sub<K2>(a0, a2), d1 = lz_w4<INV, K4>(lz_sub<K2>(a1, a3));            // <= 4 M61
    const Lz61 e0 = lz_add<K2>(b0, b2), e1 = lz_add<K2>(b1, b3), f0 = lz_sub<K2>(b0, b2), f1 = lz_w4<INV, K4>(lz_sub<K2>(b1, b3));
    x[0] = lz_add<K4>(c0, c1); x[4] = lz_sub<K4>(c0, c1); x[2] = lz_add<K4>(d0, d1); x[6] = lz_sub<K4>(d0, d1);                               // <= 8 M61
    x[1] = lz_add<K4>(e0, e1); x[5] = lz_sub<K4>(e0, e1); x[3] = lz_add<K4>(f0, f1); x[7] = lz_sub<K4>(f0, f1);
  }
}

// (a + i b)(c + i d) or, CONJ, (a + i b)(c - i d): a, b <= M61 + 7 (folded), c, d canonical; canonical result
template <bool CONJ>
GF_HD F61::C cmul61(Lz61 x, F61::C w) {
  const uint32_t a0 = uint32_t(x.re) & 0x7fffffffu, a1 = uint32_t(x.re >> 31), b0 = uint32_t(x.im) & 0x7fffffffu, b1 = uint32_t(x.im >> 31);
  const uint32_t c0 = uint32_t(w.re) & 0x7fffffffu, c1 = uint32_t(w.re >> 31);
  uint32_t d0 = uint32_t(w.im) & 0x7fffffffu, d1 = uint32_t(w.im >> 31);
  uint32_t n0 = d0 ^ 0x7fffffffu, n1 = d1 ^ 0x3fffffffu;                        // limbs of M61 - d
  if (CONJ) { uint32_t t = d0; d0 = n0; n0 = t; t = d1; d1 = n1; n1 = t; }
  const uint64_t P0 = uint64_t(a0) * c0 + uint64_t(b0) * n0;                      // < 2^63
  const uint64_t P1 = uint64_t(a0) * c1 + uint64_t(a1) * c0 + uint64_t(b0) * n1 + uint64_t(b1) * n0;   // < 2^63
  const uint64_t P2 = uint64_t(a1) * c1 + uint64_t(b1) * n1;                      // <= 2^61
  const uint64_t Q0 = uint64_t(a0) * d0 + uint64_t(b0) * c0;
  const uint64_t Q1 = uint64_t(a0) * d1 + uint64_t(a1) * d0 + uint64_t(b0) * c1 + uint64_t(b1) * c0;
  const uint64_t Q2 = uint64_t(a1) * d1 + uint64_t(b1) * c1;
  // P0 + P1 2^31 + P2 2^62 with 2^61 = 1: P1 = l + h 2^30 -> l 2^31 + h; P2 2^62 -> 2 P2; the sum stays below 2^64
  const uint64_t S = P0 + (P2 << 1) + (P1 >> 30) + (uint64_t(uint32_t(P1) & 0x3fffffffu) << 31);
  const uint64_t T = Q0 + (Q2 << 1) + (Q1 >> 30) + (uint64_t(uint32_t(Q1) & 0x3fffffffu) << 31);
  return {canon61(S), canon61(T)};
}

// Z/M31[i] product with both partial products of a component accumulated in one 64-bit multiply-add chain (a c + b (M31 - d) < 2^63)
// and one reduction per component (canonical operands and result)
GF_HD uint32_t red31_63(uint64_t x) {                       // x < 2^63
  const uint32_t y = (uint32_t(x) & M31) + (uint32_t(x >> 31) & M31) + uint32_t(x >> 62);   // <= 2^32 - 1
  const uint32_t z = (y & M31) + (y >> 31);                                       // <= M31 + 1
#if defined(__HIP_DEVICE_COMPILE__)
  return min(z, z - M31);                                                         // unsigned wrap: z < M31 keeps z
#else
  return z < z - M31 ? z : z - M31;
#endif
}
template <bool CONJ>
GF_HD F31::C cmul31(F31::C x, F31::C w) {
  const uint32_t d = CONJ ? (w.im ^ M31) : w.im, n = CONJ ? w.im : (w.im ^ M31);  // M31 - d is the bit complement
  return {red31_63(uint64_t(x.re) * w.re + uint64_t(x.im) * n), red31_63(uint64_t(x.re) * d + uint64_t(x.im) * w.re)};
}

// out[k] = sum_q in[q] w^(qk), w = omega_R (forward) or its conjugate (INV, unnormalised); natural order in and out
template <class F, int R, bool INV>
GF_HD void bfly(typename F::C (&x)[R]) {
  using C = typename F::C;
  if constexpr (R == 2) {
    const C a = cadd<F>(x[0], x[1]), b = csub<F>(x[0], x[1]);
    x[0] = a; x[1] = b;
  } else if constexpr (R == 4) {
    const C a0 = cadd<F>(x[0], x[2]), a1 = cadd<F>(x[1], x[3]), b0 = csub<F>(x[0], x[2]), b1 = mul_w4<F, INV>(csub<F>(x[1], x[3]));
    x[0] = cadd<F>(a0, a1); x[2] = csub<F>(a0, a1); x[1] = cadd<F>(b0, b1); x[3] = csub<F>(b0, b1);
  } else {
    const C a0 = cadd<F>(x[0], x[4]), a1 = cadd<F>(x[1], x[5]), a2 = cadd<F>(x[2], x[6]), a3 = cadd<F>(x[3], x[7]);
    const C b0 = csub<F>(x[0], x[4]), b1 = mul_w8<F, INV>(csub<F>(x[1], x[5])), b2 = mul_w4<F, INV>(csub<F>(x[2], x[6])),
            b3 = mul_w4<F, INV>(mul_w8<F, INV>(csub<F>(x[3], x[7])));
    const C c0 = cadd<F>(a0, a2), c1 = cadd<F>(a1, a3), d0 = csub<F>(a0, a2), d1 = mul_w4<F, INV>(csub<F>(a1, a3));
    const C e0 = cadd<F>(b0, b2), e1 = cadd<F>(b1, b3), f0 = csub<F>(b0, b2), f1 = mul_w4<F, INV>(csub<F>(b1, b3));
    x[0] = cadd<F>(c0, c1); x[4] = csub<F>(c0, c1); x[2] = cadd<F>(d0, d1); x[6] = csub<F>(d0, d1);
    x[1] = cadd<F>(e0, e1); x[5] = csub<F>(e0, e1); x[3] = cadd<F>(f0, f1); x[7] = csub<F>(f0, f1);
  }
}

// ---- odd axis: DFT of length 1, 3 or 9 with scalar roots --------------------------------------------------------------------
// DFT-3 with w + w^2 = -1: y0 = x0 + (x1 + x2), y1,2 = x0 - (x1 + x2) / 2 +- c (x1 - x2), c = (w - w^2) / 2: one scalar product.
// DFT-9 = 3 x 3 (Cooley-Tukey): three DFT-3 over a1 (a = 3 a1 + a0), twiddles r^(a0 k0) (four non-trivial), three DFT-3 over a0
// -> X[k0 + 3 k1]: 10 scalar-times-complex products instead of the 64 of the direct sums.  (Reference: fft-middle.cl:663-720.)
template <class F>
GF_HD void dft3(typename F::C& x0, typename F::C& x1, typename F::C& x2, typename F::S c) {
  using C = typename F::C;
  const C t1 = cadd<F>(x1, x2), t2 = cscale<F>(csub<F>(x1, x2), c);
  const C u = csub<F>(x0, chalf<F>(t1));
  x0 = cadd<F>(x0, t1); x1 = cadd<F>(u, t2); x2 = csub<F>(u, t2);
}
template <class F, int ODD>
GF_HD void dft_odd(typename F::C (&x)[ODD], const typename F::S* __restrict__ r /* r^e, e < 9 */, typename F::S c3) {
  using C = typename F::C;
  if (ODD == 3) {
    dft3<F>(x[0], x[1], x[2], c3);
  } else if (ODD == 9) {
#pragma unroll
    for (int a0 = 0; a0 < 3; ++a0) dft3<F>(x[a0], x[a0 + 3], x[a0 + 6], c3);     // x[a0 + 3 k0] <- Y[a0][k0]
    x[1 + 3] = cscale<F>(x[1 + 3], r[1]); x[1 + 6] = cscale<F>(x[1 + 6], r[2]);
    x[2 + 3] = cscale<F>(x[2 + 3], r[2]); x[2 + 6] = cscale<F>(x[2 + 6], r[4]);
    C y[9];
#pragma unroll
    for (int k0 = 0; k0 < 3; ++k0) {
      C z0 = x[3 * k0], z1 = x[3 * k0 + 1], z2 = x[3 * k0 + 2];
      dft3<F>(z0, z1, z2, c3);
      y[k0] = z0; y[k0 + 3] = z1; y[k0 + 6] = z2;                                // X[k0 + 3 k1]
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = y[k];
  }
}

// ---- host: the scalar tables of the odd axis (CrtEngine's constructor; the tests of dft_odd use the same ones) ----
template <class S, class POW>
inline S odd_root(unsigned odd, S modulus, POW pw) {   // a primitive odd-th root of unity among the scalars (odd | p - 1)
  for (S g = 2;; ++g) {
    const S r = pw(g, (uint64_t(modulus) - 1) / odd);
    bool ok = r != 1;
    for (unsigned d = 2; ok && d < odd; ++d) if (odd % d == 0 && pw(r, odd / d) == 1) ok = false;
    if (ok && pw(r, odd) == 1) return r;
  }
}
struct OddTables { uint64_t r61[9], r61i[9], c3_61; uint32_t r31[9], r31i[9], c3_31; };   // r^e, r^-e (e < 9), (w3 - w3^2) / 2
inline OddTables make_odd_tables(unsigned odd) {   // odd = 1, 3 or 9
  OddTables t;
  const uint64_t r61 = odd > 1 ? odd_root<uint64_t>(odd, M61, pow61) : 1;
  const uint32_t r31 = odd > 1 ? odd_root<uint32_t>(odd, M31, pow31) : 1;
  for (unsigned k = 0; k < 9; ++k) {
    t.r61[k] = pow61(r61, k % odd); t.r61i[k] = pow61(r61, (odd - k % odd) % odd);
    t.r31[k] = pow31(r31, k % odd); t.r31i[k] = pow31(r31, (odd - k % odd) % odd);
  }
  const unsigned cube = odd == 9 ? 3 : 1;            // w3 = r^3 for radix 9, r itself for radix 3
  const uint64_t w61 = t.r61[cube % 9], w61sq = mul61(w61, w61);
  const uint32_t w31 = t.r31[cube % 9], w31sq = mul31(w31, w31);
  t.c3_61 = odd > 1 ? F61::half(F61::sub(w61, w61sq)) : 0; t.c3_31 = odd > 1 ? F31::half(F31::sub(w31, w31sq)) : 0;
  return t;
}

}  // namespace crt
}  // namespace mi355
