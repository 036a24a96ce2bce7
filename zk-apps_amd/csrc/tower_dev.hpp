// zkmi — the Fq2 -> Fq6 -> Fq12 tower, the two Miller steps, the merged Miller loop and the final exponentiation chain of
// pairing_dev.hip, written ONCE over the Fq2 type E2 (its base field is FQ):
//   Fq2P    a lane pair per value on the device (pairing_dev.hip's kernels),
//   Fq2     the host's canonical field, for the formula self-checks against pairing.hip,
//   Fq2_28  both components in one lane, and an interval type: the testing library's instantiations (tower_selftest.hpp).
// Everything has internal linkage: the out-of-line device routines (PD_CALL) are one copy per translation unit.
#pragma once
#include "field28.hpp"

namespace zkmi {

namespace {

#define PD_CALL __device__ __attribute__((noinline))
PD_CALL Fq28 fq_mul(Fq28 a, Fq28 b) { return Fq28::mul_inline(a, b); }
__host__ inline Fq28 fq_mul(Fq28 a, Fq28 b) { return Fq28::mul_inline(a, b); }  // host instantiation (testing library)
PD_CALL Fq2P e2_mul(Fq2P a, Fq2P b) { return a * b; }
PD_CALL Fq2P e2_sqr(Fq2P a) { return a.sqr(); }
PD_CALL Fq2P e2_mul_sub_mul(Fq2P a, Fq2P b, Fq2P c, Fq2P d) { return f_mul_sub_mul(a, b, c, d); }  // a b - c d, one reduction
#define PD_INL __device__ __forceinline__
#define PD_HD __host__ __device__ __forceinline__

PD_INL Fq2P e2_mul_fq(const Fq2P& a, const Fq28& k) { return {fq_mul(a.v, k)}; }
// xi = 1 + u: (c0 - c1) + (c0 + c1) u
PD_INL Fq2P e2_mul_xi(const Fq2P& a) {
  const Fq28 p = Fq2P::partner(a.v);
  return {a.v + Fq2P::sel(Fq2P::odd(), p, Fq2P::negl(p))};
}
// Magnitudes.  Every add, sub, neg and dbl below only carries; a value is an integer v = x + k p held in limbs, and the one
// thing a Montgomery reduction needs is  sum over its partial products of |a||b| < R p / 2 = 1260.1 p^2  (R = 2^392): then
// T / R lies in (-p/2, p/2) and the result (T + m p) / R, 0 <= m < R, in (-p/2, 3p/2).  An Fq2P product sums two partial
// products per lane, f_mul_sub_mul four, a squaring ONE of lazily doubled operands (2|a|)^2.  The 64-bit columns hold 14 limb
// products per partial product plus the reduction's 14 x 2^56 below 2^63 as long as top limbs stay below 2^28 (|v| < 2520 p).
// shrink() brings a value back to (-2 p, 2 p): every coefficient e12_sqr / e12_mul / e12_mul_line / e12_inv return and x, y
// of T pass through it, once per round of the loops.  What the tower then reaches, measured by running these very templates
// over intervals from the kernels' entry conditions (zkmi_selftest_tower_bounds; tests/test_cpu_tower.py holds the maxima
// to the limits, DESIGN.md 5.6.1 has the table): operands of products up to 22.5 p (d - x3 in step_tangent), sums up to
// 202.5 p^2, columns below 2^62.2, inputs of shrink up to 23 p, inputs of is_zero up to 3 p (exact to 4 p).
//
// a - q p with q = floor(float(top limb) / 106513), p = (0x1a011 + 0.1197..) 2^364: |q - v/p| < 1 + |v/p| (3 x 2^-24 +
// 1.13e-6) -- the float's conversion, the reciprocal's and the product's rounding, and the limbs of p below the top one --
// so the result lies in (-2 p, 2 p) (in fact (-0.03 p, 1.03 p)) for |v| < 2^14 p, where the top limb still fits int32.
PD_HD Fq28 shrink(const Fq28& a) {
  const int32_t q = (int32_t)floorf((float)a.l[13] * (1.0f / 106513.0f));
  Fq28 r;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 13; i++) {
    const int64_t v = (int64_t)a.l[i] - (int64_t)q * Fq28Params::MOD[i] + c;
    r.l[i] = (int32_t)v & Fq28::MASK;
    c = v >> 28;
  }
  r.l[13] = (int32_t)((int64_t)a.l[13] - (int64_t)q * Fq28Params::MOD[13] + c);
  return r;
}
PD_INL Fq2P shrink(const Fq2P& a) { return {shrink(a.v)}; }

// The tower and the two steps are written once over the Fq2 type E2 (its base field is FQ): Fq2P on the device, and the
// host's Fq2 for the formula self-check against pairing.hip (zkmi_selftest_miller_formulas, testing library).
inline Fq2 e2_mul(const Fq2& a, const Fq2& b) { return a * b; }
inline Fq2 e2_sqr(const Fq2& a) { return a.sqr(); }
inline Fq2 e2_mul_sub_mul(const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) { return a * b - c * d; }
inline Fq2 e2_mul_fq(const Fq2& a, const Fq& k) { return a.mul_fq(k); }
inline Fq2 e2_mul_xi(const Fq2& a) { return a.mul_xi(); }
inline Fq2 shrink(const Fq2& a) { return a; }
// conjugation and inversion in Fq2.  Device: the norm c0^2 + c1^2 takes one exchange with the partner lane, both lanes run
// the limb inversion (Fp28::inv, the one to_affine() uses: x^(p-2), 0 -> 0, no branch on data) and scale their component.
PD_INL Fq2P e2_conj(const Fq2P& a) { return {Fq2P::sel(Fq2P::odd(), a.v.neg(), a.v)}; }
PD_CALL Fq28 fq_inv(Fq28 a) { return a.inv(); }
PD_INL Fq2P e2_inv(const Fq2P& a) {
  const Fq28 s = fq_mul(a.v, a.v);
  const Fq28 t = fq_mul(a.v, fq_inv(s + Fq2P::partner(s)));
  return {Fq2P::sel(Fq2P::odd(), t.neg(), t)};
}
inline Fq2 e2_conj(const Fq2& a) { return a.conj(); }
inline Fq2 e2_inv(const Fq2& a) { return a.inv(); }
#define PD_T template <class E2> __host__ __device__ __forceinline__
#define PD_TQ template <class E2, class FQ> __host__ __device__ __forceinline__

// Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v) as in pairing.hpp
template <class E2>
struct E6 {
  E2 a0, a1, a2;
};
template <class E2>
struct E12 {
  E6<E2> c0, c1;
};
PD_T E6<E2> operator+(const E6<E2>& a, const E6<E2>& b) { return {a.a0 + b.a0, a.a1 + b.a1, a.a2 + b.a2}; }
PD_T E6<E2> operator-(const E6<E2>& a, const E6<E2>& b) { return {a.a0 - b.a0, a.a1 - b.a1, a.a2 - b.a2}; }
PD_T E6<E2> e6_mul_v(const E6<E2>& a) { return {e2_mul_xi(a.a2), a.a0, a.a1}; }
PD_T E6<E2> e6_dbl(const E6<E2>& a) { return {a.a0.dbl(), a.a1.dbl(), a.a2.dbl()}; }
PD_T E6<E2> shrink(const E6<E2>& a) { return {shrink(a.a0), shrink(a.a1), shrink(a.a2)}; }
PD_T E6<E2> e6_mul(const E6<E2>& a, const E6<E2>& b) {
  const E2 t0 = e2_mul(a.a0, b.a0), t1 = e2_mul(a.a1, b.a1), t2 = e2_mul(a.a2, b.a2);
  const E2 c0 = t0 + e2_mul_xi(e2_mul(a.a1 + a.a2, b.a1 + b.a2) - t1 - t2);
  const E2 c1 = e2_mul(a.a0 + a.a1, b.a0 + b.a1) - t0 - t1 + e2_mul_xi(t2);
  const E2 c2 = e2_mul(a.a0 + a.a2, b.a0 + b.a2) - t0 - t2 + t1;
  return {c0, c1, c2};
}
PD_T E12<E2> e12_one() { return {{E2::one(), E2::zero(), E2::zero()}, {E2::zero(), E2::zero(), E2::zero()}}; }
// complex squaring over Fq6: c0 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1, c1 = 2 a0 a1
PD_T E12<E2> e12_sqr(const E12<E2>& a) {
  const E6<E2> ab = e6_mul(a.c0, a.c1);
  const E6<E2> s = e6_mul(a.c0 + a.c1, a.c0 + e6_mul_v(a.c1));
  return {shrink(s - ab - e6_mul_v(ab)), shrink(e6_dbl(ab))};
}
PD_T E12<E2> e12_mul(const E12<E2>& a, const E12<E2>& b) {
  const E6<E2> t0 = e6_mul(a.c0, b.c0), t1 = e6_mul(a.c1, b.c1);
  const E6<E2> c1 = e6_mul(a.c0 + a.c1, b.c0 + b.c1) - t0 - t1;
  return {shrink(t0 + e6_mul_v(t1)), shrink(c1)};
}
// f * (l0 + (l1 v + l2 v^2) w): 14 products instead of the dense 18
PD_T E12<E2> e12_mul_line(const E12<E2>& f, const E2& l0, const E2& l1, const E2& l2) {
  const E6<E2> t0 = {e2_mul(f.c0.a0, l0), e2_mul(f.c0.a1, l0), e2_mul(f.c0.a2, l0)};
  E6<E2> t1;
  {
    const E6<E2>& a = f.c1;  // a * (l1 v + l2 v^2)
    const E2 m1 = e2_mul(a.a1, l1), m2 = e2_mul(a.a2, l2);
    t1.a0 = e2_mul_xi(e2_mul(a.a1 + a.a2, l1 + l2) - m1 - m2);
    t1.a1 = e2_mul(a.a0, l1) + e2_mul_xi(m2);
    t1.a2 = e2_mul(a.a0, l2) + m1;
  }
  const E6<E2> c1 = e6_mul(f.c0 + f.c1, E6<E2>{l0, l1, l2}) - t0 - t1;
  return {shrink(t0 + e6_mul_v(t1)), shrink(c1)};
}

template <class E2>
struct Jac {
  E2 x, y, z;
};
// T <- 2 T (dbl-2009-l, a = 0) and the tangent at the old T through (xP, yP), times 2 Y Z^3
PD_TQ void step_tangent(Jac<E2>& t, const FQ& xp, const FQ& nyp, E2& l0, E2& l1, E2& l2) {
  const E2 a = e2_sqr(t.x), b = e2_sqr(t.y), c = e2_sqr(b);
  const E2 d = (e2_sqr(t.x + b) - a - c).dbl();
  const E2 e = a.dbl() + a;
  const E2 zz = e2_sqr(t.z);
  const E2 x3 = e2_sqr(e) - d.dbl();
  const E2 y3 = e2_mul(e, d - x3) - c.dbl().dbl().dbl();
  const E2 z3 = e2_mul(t.y, t.z).dbl();
  l0 = e2_mul_xi(e2_mul_fq(e2_mul(z3, zz), nyp));
  l1 = b.dbl() - e2_mul(e, t.x);
  l2 = e2_mul_fq(e2_mul(e, zz), xp);
  t = {shrink(x3), shrink(y3), z3};
}
// T <- T + Q (Q affine) and the chord through (xP, yP), times Z3
PD_TQ void step_chord(Jac<E2>& t, const E2& xq, const E2& yq, const FQ& xp, const FQ& nyp, E2& l0, E2& l1, E2& l2) {
  const E2 zz = e2_sqr(t.z);
  const E2 h = e2_mul(xq, zz) - t.x;
  const E2 r = e2_mul(yq, e2_mul(t.z, zz)) - t.y;
  const E2 hh = e2_sqr(h);
  const E2 hhh = e2_mul(h, hh), v = e2_mul(t.x, hh);
  const E2 x3 = e2_sqr(r) - hhh - v.dbl();
  const E2 y3 = e2_mul_sub_mul(r, v - x3, t.y, hhh);
  const E2 z3 = e2_mul(t.z, h);
  l0 = e2_mul_xi(e2_mul_fq(z3, nyp));
  l1 = e2_mul_sub_mul(z3, yq, r, xq);
  l2 = e2_mul_fq(r, xp);
  t = {shrink(x3), shrink(y3), z3};
}

constexpr uint64_t X_ABS = 0xd201000000010000ull;
// f_{|x|,Q}(P), not conjugated: the 63 steps of |x| and its 5 additions as ONE loop of 68 rounds whose kind is uniform
PD_TQ E12<E2> miller_rounds(const E2& xq, const E2& yq, const FQ& xp, const FQ& nyp) {
  Jac<E2> t = {xq, yq, E2::one()};
  E12<E2> f = e12_one<E2>();
  int b = 62;
  bool chord = false;
#pragma unroll 1
  while (b >= 0) {
    E2 l0, l1, l2;
    if (!chord) {
      f = e12_sqr(f);
      step_tangent(t, xp, nyp, l0, l1, l2);
    } else {
      step_chord(t, xq, yq, xp, nyp, l0, l1, l2);
    }
    f = e12_mul_line(f, l0, l1, l2);
    if (!chord && ((X_ABS >> b) & 1ull)) {
      chord = true;
    } else {
      chord = false;
      b--;
    }
  }
  return f;
}

using E2 = Fq2P;
using E12P = E12<Fq2P>;

// 12 canonical little-endian words <-> Montgomery limbs (Fp28::from_canonical / to_canonical through the shared product)
PD_HD Fq28 limbs_from_words(const uint32_t* __restrict__ q, bool* all_zero) {
  uint32_t w[12];
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    w[i] = q[i];
    acc |= w[i];
  }
  *all_zero = acc == 0;
  Fq28 a, r2;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    const int bit = 28 * i, wi = bit >> 5, sh = bit & 31;
    uint64_t v = w[wi];
    if (wi + 1 < 12) v |= (uint64_t)w[wi + 1] << 32;
    a.l[i] = (int32_t)((v >> sh) & (uint32_t)Fq28::MASK);
    r2.l[i] = Fq28Params::R2[i];
  }
  return fq_mul(a, r2);
}
PD_HD void limbs_to_words(const Fq28& a, uint32_t* __restrict__ q, bool write) {
  Fq28 o = Fq28::zero();
  o.l[0] = 1;
  const Fq28 c = fq_mul(a, o);  // in [0, p]
  bool is_p = true;
#pragma unroll
  for (int i = 0; i < 14; i++) is_p &= (c.l[i] == Fq28Params::MOD[i]);
  uint32_t w[12];
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = 0;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    const uint64_t v = is_p ? 0u : (uint64_t)(uint32_t)c.l[i];
    const int bit = 28 * i, wi = bit >> 5, sh = bit & 31;
    const uint64_t s = v << sh;
    w[wi] |= (uint32_t)s;
    if (wi + 1 < 12) w[wi + 1] |= (uint32_t)(s >> 32);
  }
  if (write) {
#pragma unroll
    for (int i = 0; i < 12; i++) q[i] = w[i];
  }
}

// ---- final exponentiation --------------------------------------------------------------------------------------------
// f^((p^12 - 1)/r) EXACTLY (the bytes of pairing.hip's final_exponentiation, no fixed power of it), written once over E2
// like the Miller loop: Fq2P on the device, the host's Fq2 for the formula self-check (zkmi_selftest_final_exp_formulas).
//   easy part  m = f^((p^6 - 1)(p^2 + 1)):  conj(f) f^-1 with the tower inversion Fq12 -> Fq6 -> Fq2 -> Fq, then the p^2 map
//   hard part  (p^4 - p^2 + 1)/r = c (x + p)(x^2 + p^2 - 1) + 1,  c = (x - 1)^2 / 3 (126 bits),  x = -0xd201000000010000
//              (checked with big integers: oracle/bls12_381.py's P and R; tests/test_cpu_final_exp.py pins it):
//                a = m^c,   b = a^x a^p,   result = b^(x^2) b^(p^2) b^-1 m
//              x < 0 and m is in the cyclotomic subgroup, where the inverse is the conjugate: a^x = conj(a^|x|).
// Cost: 125 + 3 x 63 = 314 squarings and 47 + 3 x 5 + 6 = 68 products in Fq12 (e12_sqr is correct in the cyclotomic
// subgroup too), one inversion in Fq (~570 Fq products), two p maps and three p^2 maps; the host path spends 1 268 + 762
// squarings.  All exponent bits are compile-time constants: ONE loop of 376 rounds whose kind (square / multiply by the
// base) is wave-uniform, as miller_rounds drives X_ABS; the three phase changes are uniform branches inside it.
// Magnitudes: e12_sqr / e12_mul shrink every coefficient they return, the maps and the inversion return products or shrunk
// sums of a few products: the chain stays inside the bounds stated above shrink().
// An input of 0 (or garbage in a dead lane pair) meets no trap and no data-dependent branch: its inversion returns 0.
//
// Frobenius maps.  An element is sum_k c_k w^k with c_k in Fq2 and k = 2 j + i for the coefficient of v^j w^i (w^2 = v,
// w^6 = xi), so  (c w^k)^p = conj(c) xi^(k (p-1)/6) w^k  and  (c w^k)^(p^2) = c xi^(k (p^2-1)/6) w^k, the latter factor in
// Fq because xi^((p^2-1)/6) = N(xi)^((p-1)/6) = 2^((p-1)/6).  The tables hold the canonical values for k = 1..5, computed as
// pow(xi, k (p-1)/6) and pow(xi, k (p^2-1)/6) in Fq[u]/(u^2 + 1) with the big integers of oracle/bls12_381.py (P).
struct FrobK {
  static constexpr uint32_t P1[5][2][12] = {
      {{0x92235fb8u, 0x8d0775edu, 0x63e7813du, 0xf67ea53du, 0x84bab9c4u, 0x7b2443d7u, 0x3cbd5f4fu, 0x0fd603fdu, 0x202c0d1fu, 0xc231beb4u, 0x02bb0667u, 0x1904d3bfu},
       {0x6ddc4af3u, 0x2cf78a12u, 0x4d6c7ec2u, 0x282d5ac1u, 0x71f63c5fu, 0xec0c8ec9u, 0xb6c7b36fu, 0x54a14787u, 0x231f9fb8u, 0x88e9e902u, 0x36c4e032u, 0x00fc3e2bu}},
      {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
       {0x0000aaacu, 0x8bfd0000u, 0x4f49fffdu, 0x409427ebu, 0x0fb85f9bu, 0x897d2965u, 0x89759ad4u, 0xaa0d857du, 0x63d4de85u, 0xec024086u, 0x397fe699u, 0x1a0111eau}},
      {{0xede3cc09u, 0xc81084fbu, 0x72ec05f4u, 0xee67992fu, 0x009241c5u, 0x77f76e17u, 0xc2d3435eu, 0x48395dabu, 0x6bd17ffeu, 0x6831e36du, 0x37ff400bu, 0x06af0e04u},
       {0xede3cc09u, 0xc81084fbu, 0x72ec05f4u, 0xee67992fu, 0x009241c5u, 0x77f76e17u, 0xc2d3435eu, 0x48395dabu, 0x6bd17ffeu, 0x6831e36du, 0x37ff400bu, 0x06af0e04u}},
      {{0x0000aaadu, 0x8bfd0000u, 0x4f49fffdu, 0x409427ebu, 0x0fb85f9bu, 0x897d2965u, 0x89759ad4u, 0xaa0d857du, 0x63d4de85u, 0xec024086u, 0x397fe699u, 0x1a0111eau},
       {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},
      {{0x80078116u, 0x9b18fae9u, 0x257f8732u, 0xc63a3e6eu, 0x8e9c0566u, 0x8beadf4du, 0x0c0b8feeu, 0xf3981624u, 0x48b1e045u, 0xdf47fa6bu, 0x013a5fd8u, 0x05b2cfd9u},
       {0x7ff82995u, 0x1ee60516u, 0x8bd478cdu, 0x5871c190u, 0x6814f0bdu, 0xdb45f353u, 0xe77982d0u, 0x70df3560u, 0xfa99cc91u, 0x6bd3ad4au, 0x384586c1u, 0x144e4211u}},
  };
  static constexpr uint32_t P2[5][12] = {
      {0xfffeffffu, 0x2e01ffffu, 0x620a0002u, 0xde17d813u, 0xe6f89688u, 0xddb3a93bu, 0x6a0f77eau, 0xba69c607u, 0xdf76ce51u, 0x5f19672fu, 0x00000000u, 0x00000000u},
      {0xfffefffeu, 0x2e01ffffu, 0x620a0002u, 0xde17d813u, 0xe6f89688u, 0xddb3a93bu, 0x6a0f77eau, 0xba69c607u, 0xdf76ce51u, 0x5f19672fu, 0x00000000u, 0x00000000u},
      {0xffffaaaau, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau},
      {0x0000aaacu, 0x8bfd0000u, 0x4f49fffdu, 0x409427ebu, 0x0fb85f9bu, 0x897d2965u, 0x89759ad4u, 0xaa0d857du, 0x63d4de85u, 0xec024086u, 0x397fe699u, 0x1a0111eau},
      {0x0000aaadu, 0x8bfd0000u, 0x4f49fffdu, 0x409427ebu, 0x0fb85f9bu, 0x897d2965u, 0x89759ad4u, 0xaa0d857du, 0x63d4de85u, 0xec024086u, 0x397fe699u, 0x1a0111eau},
  };
};
// the constants in the field representation of E2 (the pointer argument only selects the overload)
template <int K>
PD_INL Fq2P frob_p1(const Fq2P*) {
  uint32_t w[12];
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = Fq2P::odd() ? FrobK::P1[K][1][i] : FrobK::P1[K][0][i];
  bool z;
  return {limbs_from_words(w, &z)};
}
template <int K>
PD_INL Fq28 frob_p2(const Fq2P*) {
  uint32_t w[12];
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = FrobK::P2[K][i];
  bool z;
  return limbs_from_words(w, &z);
}
template <int K>
inline Fq2 frob_p1(const Fq2*) {
  Fq2 r;
  for (int i = 0; i < 12; i++) {
    r.c0.l[i] = FrobK::P1[K][0][i];
    r.c1.l[i] = FrobK::P1[K][1][i];
  }
  return r.to_mont();
}
template <int K>
inline Fq frob_p2(const Fq2*) {
  Fq r;
  for (int i = 0; i < 12; i++) r.l[i] = FrobK::P2[K][i];
  return r.to_mont();
}
PD_T E12<E2> e12_frob_p(const E12<E2>& a) {
  const E2* t = nullptr;
  return {{e2_conj(a.c0.a0), e2_mul(e2_conj(a.c0.a1), frob_p1<1>(t)), e2_mul(e2_conj(a.c0.a2), frob_p1<3>(t))},
          {e2_mul(e2_conj(a.c1.a0), frob_p1<0>(t)), e2_mul(e2_conj(a.c1.a1), frob_p1<2>(t)),
           e2_mul(e2_conj(a.c1.a2), frob_p1<4>(t))}};
}
PD_T E12<E2> e12_frob_p2(const E12<E2>& a) {
  const E2* t = nullptr;
  return {{a.c0.a0, e2_mul_fq(a.c0.a1, frob_p2<1>(t)), e2_mul_fq(a.c0.a2, frob_p2<3>(t))},
          {e2_mul_fq(a.c1.a0, frob_p2<0>(t)), e2_mul_fq(a.c1.a1, frob_p2<2>(t)), e2_mul_fq(a.c1.a2, frob_p2<4>(t))}};
}
PD_T E12<E2> e12_conj(const E12<E2>& a) { return {a.c0, {a.c1.a0.neg(), a.c1.a1.neg(), a.c1.a2.neg()}}; }
// pairing.hip's Fq6::inv and Fq12::inv over E2
PD_T E6<E2> e6_inv(const E6<E2>& a) {
  const E2 c0 = e2_sqr(a.a0) - e2_mul_xi(e2_mul(a.a1, a.a2));
  const E2 c1 = e2_mul_xi(e2_sqr(a.a2)) - e2_mul(a.a0, a.a1);
  const E2 c2 = e2_sqr(a.a1) - e2_mul(a.a0, a.a2);
  const E2 t = e2_inv(shrink(e2_mul(a.a0, c0) + e2_mul_xi(e2_mul(a.a2, c1) + e2_mul(a.a1, c2))));
  return {e2_mul(c0, t), e2_mul(c1, t), e2_mul(c2, t)};
}
PD_T E12<E2> e12_inv(const E12<E2>& a) {
  const E6<E2> t = e6_inv(shrink(shrink(e6_mul(a.c0, a.c0)) - e6_mul_v(shrink(e6_mul(a.c1, a.c1)))));
  const E6<E2> c1 = e6_mul(a.c1, t);
  return {shrink(e6_mul(a.c0, t)), shrink(E6<E2>{c1.a0.neg(), c1.a1.neg(), c1.a2.neg()})};
}
// the dense product and the squaring as ONE out-of-line routine each on the device: the chain has a dozen call sites
PD_CALL E12P e12_mul_o(E12P a, E12P b) { return e12_mul(a, b); }
PD_CALL E12P e12_sqr_o(E12P a) { return e12_sqr(a); }
inline E12<Fq2> e12_mul_o(const E12<Fq2>& a, const E12<Fq2>& b) { return e12_mul(a, b); }
inline E12<Fq2> e12_sqr_o(const E12<Fq2>& a) { return e12_sqr(a); }

constexpr uint64_t C_HI = 0x396c8c005555e156ull, C_LO = 0x8c00aaab0000aaabull;  // c = (x - 1)^2 / 3, bits 125..0
PD_T E12<E2> final_exp_chain(const E12<E2>& f) {
  E12<E2> m = e12_mul_o(e12_conj(f), e12_inv(f));  // f^(p^6 - 1)
  m = e12_mul_o(e12_frob_p2(m), m);                // ^(p^2 + 1)
  // phase 0: acc = m^c;  1: acc = a^|x|;  2, 3: acc = b^|x|, (b^|x|)^|x|.  The top bit of each exponent is the start value.
  E12<E2> base = m, acc = m, u = m;
  int phase = 0, b = 124;
  bool mult = false;
#pragma unroll 1
  while (phase < 4) {
    if (mult) acc = e12_mul_o(acc, base);
    else acc = e12_sqr_o(acc);
    const uint64_t word = phase ? X_ABS : (b >= 64 ? C_HI : C_LO);
    if (!mult && ((word >> (b & 63)) & 1ull)) {
      mult = true;
      continue;
    }
    mult = false;
    if (--b >= 0) continue;
    b = 62;
    if (phase == 1) {
      base = e12_mul_o(e12_conj(acc), e12_frob_p(base));                  // b = a^x a^p
      u = e12_mul_o(e12_mul_o(e12_frob_p2(base), e12_conj(base)), u);     // b^(p^2 - 1) m
      acc = base;
    } else {
      base = acc;  // phase 0: a = m^c;  phase 2: b^|x|, raised to |x| again (the signs cancel)
    }
    phase++;
  }
  return e12_mul_o(acc, u);
}

// f == 1, the status test of k_final_exp: every coefficient of f - 1 is zero in both lanes of the pair.  is_zero is exact
// for |v| <= 4 p; f comes out of e12_mul shrunk below 2 p and one() is canonical, so f.c0.a0 - 1 lies in (-3 p, 2 p).
PD_INL bool e12_is_one(const E12P& f) {
  int mine = (f.c0.a0 - E2::one()).v.is_zero() ? 1 : 0;
  mine &= (f.c0.a1.v.is_zero() && f.c0.a2.v.is_zero() && f.c1.a0.v.is_zero() && f.c1.a1.v.is_zero() && f.c1.a2.v.is_zero()) ? 1 : 0;
  return (mine & __builtin_amdgcn_mov_dpp(mine, 0xB1, 0xF, 0xF, true)) != 0;
}


}  // namespace

}  // namespace zkmi
