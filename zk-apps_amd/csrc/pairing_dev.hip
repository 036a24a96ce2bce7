// zkmi — prod_i e(P_i, Q_i) with the Miller loops and their product on the device and ONE final exponentiation on the
// host (zkmi_pairing_product_dev).  pairing.hip is the specification: the same M-twist line embedding
//   -yP*xi + (yT - l*xT) v w + (l*xP) v^2 w,
// but T stays Jacobian, so a step has no inversion and every line comes out multiplied by a factor in Fq2 (2 Y Z^3 for a
// tangent, Z3 for a chord).  The final exponentiation kills such factors: device Miller values equal the host's only
// after it.
//
// Shape: one pair (P, Q) per LANE PAIR.  Every Fq2 value is an Fq2P (field28.hpp): its two components live in two
// adjacent lanes, so f in Fq12 costs a lane 6 x 14 registers and T 3 x 14.  The Fq2 products are out-of-line routines
// shared by all call sites: the loop body of ~45 products stays a few thousand instructions instead of ~40 000.
// The 63 steps of |x| = 0xd201000000010000 and its 5 additions run as ONE loop of 68 rounds whose kind (tangent after
// squaring f / chord) is wave-uniform; for Q in the r-order subgroup T = [k]Q with 1 < k < |x| < r never meets +-Q or
// O, so neither step has an exceptional case.  A lane pair whose inputs are garbage or infinite keeps computing on
// values nobody reads (an infinite member writes 1 at the end); lane pairs past the end redo the last pair and write
// nothing.
//
// Magnitudes: field28.hpp's products return (-p/2, 3p/2) only for operands below ~16 p, and the tower formulas add a
// few dozen products before the next one.  shrink() subtracts the multiple of p that the top limb names (one
// multiply-add per limb) and brings a value back below 2 p in absolute value; every coefficient of f and every
// coordinate of T passes through it once per round, which keeps all operands of products below 32 p.
//
// The final exponentiation (final_exp_chain, k_final_exp: zkmi_pairing_batch_dev, zkmi_groth16_verify_each) is written over
// the same tower template; see the comment above final_exp_chain.
#include "pairing_dev.hpp"
#include "field28.hpp"

namespace zkmi {

namespace {

#define PD_CALL __device__ __attribute__((noinline))
PD_CALL Fq28 fq_mul(Fq28 a, Fq28 b) { return Fq28::mul_inline(a, b); }
PD_CALL Fq2P e2_mul(Fq2P a, Fq2P b) { return a * b; }
PD_CALL Fq2P e2_sqr(Fq2P a) { return a.sqr(); }
PD_CALL Fq2P e2_mul_sub_mul(Fq2P a, Fq2P b, Fq2P c, Fq2P d) { return f_mul_sub_mul(a, b, c, d); }  // a b - c d, one reduction
#define PD_INL __device__ __forceinline__

PD_INL Fq2P e2_mul_fq(const Fq2P& a, const Fq28& k) { return {fq_mul(a.v, k)}; }
// xi = 1 + u: (c0 - c1) + (c0 + c1) u
PD_INL Fq2P e2_mul_xi(const Fq2P& a) {
  const Fq28 p = Fq2P::partner(a.v);
  return {a.v + Fq2P::sel(Fq2P::odd(), p, Fq2P::negl(p))};
}
// a - k p for the k the top limb names: |result| < 2 p for |a| < 2^10 p (p = 0x1a011 * 2^364 + ...: the quotient of the
// top limbs is within one of the true one, a float holds a top limb below 2^24 exactly)
PD_INL Fq28 shrink(const Fq28& a) {
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
PD_INL Fq28 limbs_from_words(const uint32_t* __restrict__ q, bool* all_zero) {
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
PD_INL void limbs_to_words(const Fq28& a, uint32_t* __restrict__ q, bool write) {
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
// one Miller value: coefficient k of the tower basis at words 24 k (c0) and 24 k + 12 (c1)
PD_INL E12P e12_load(const uint32_t* __restrict__ m) {
  const uint32_t* q = m + (Fq2P::odd() ? 12 : 0);
  bool z;
  E12P f;
  f.c0.a0 = {limbs_from_words(q, &z)};
  f.c0.a1 = {limbs_from_words(q + 24, &z)};
  f.c0.a2 = {limbs_from_words(q + 48, &z)};
  f.c1.a0 = {limbs_from_words(q + 72, &z)};
  f.c1.a1 = {limbs_from_words(q + 96, &z)};
  f.c1.a2 = {limbs_from_words(q + 120, &z)};
  return f;
}
PD_INL void e12_store(const E12P& f, uint32_t* __restrict__ m, bool write) {
  uint32_t* q = m + (Fq2P::odd() ? 12 : 0);
  limbs_to_words(f.c0.a0.v, q, write);
  limbs_to_words(f.c0.a1.v, q + 24, write);
  limbs_to_words(f.c0.a2.v, q + 48, write);
  limbs_to_words(f.c1.a0.v, q + 72, write);
  limbs_to_words(f.c1.a1.v, q + 96, write);
  limbs_to_words(f.c1.a2.v, q + 120, write);
}
PD_INL E12P e12_select(bool c, const E12P& a, const E12P& b) {
  return {{{E2::sel(c, a.c0.a0.v, b.c0.a0.v)}, {E2::sel(c, a.c0.a1.v, b.c0.a1.v)}, {E2::sel(c, a.c0.a2.v, b.c0.a2.v)}},
          {{E2::sel(c, a.c1.a0.v, b.c1.a0.v)}, {E2::sel(c, a.c1.a1.v, b.c1.a1.v)}, {E2::sel(c, a.c1.a2.v, b.c1.a2.v)}}};
}

// g1: n x 24 words (x | y), g2: n x 48 words (x.c0 x.c1 y.c0 y.c1), out: n x 144 words
__global__ __launch_bounds__(64, 1) void k_miller(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2,
                                                  uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t pair = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = pair < n;
  const uint64_t idx = live ? pair : n - 1;  // n >= 1 (host); tail lane pairs shadow the last pair
  const uint32_t comp = threadIdx.x & 1u;

  bool zx, zy;
  const Fq28 xp = limbs_from_words(g1 + idx * 24, &zx);
  const Fq28 nyp = limbs_from_words(g1 + idx * 24 + 12, &zy).neg();
  bool inf = zx && zy;
  const E2 xq = {limbs_from_words(g2 + idx * 48 + 12 * comp, &zx)};
  const E2 yq = {limbs_from_words(g2 + idx * 48 + 24 + 12 * comp, &zy)};
  const int mine = (zx && zy) ? 1 : 0;
  inf = inf || ((mine & __builtin_amdgcn_mov_dpp(mine, 0xB1, 0xF, 0xF, true)) != 0);

  E12P f = miller_rounds(xq, yq, xp, nyp);
  f = e12_select(inf, e12_one<E2>(), f);
  e12_store(f, out + idx * 144, live);
}

// partial product j < np: prod of m[i], i = j, j + np, j + 2 np, ... < n   (np <= n)
__global__ __launch_bounds__(64, 1) void k_miller_product(const uint32_t* __restrict__ m, uint64_t n, uint32_t np,
                                                          uint32_t* __restrict__ out) {
  const uint32_t gj = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = gj < np;
  const uint32_t j = live ? gj : np - 1;
  E12P acc = e12_load(m + (uint64_t)j * 144);
  const uint64_t rounds = (n + np - 1) / np;
#pragma unroll 1
  for (uint64_t k = 1; k < rounds; k++) {
    const uint64_t i = j + k * np;
    const bool have = i < n;
    const E12P prod = e12_mul(acc, e12_load(m + (have ? i : (uint64_t)j) * 144));
    acc = e12_select(have, prod, acc);
  }
  e12_store(acc, out + (uint64_t)j * 144, live);
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
// sums of a few products: no operand of a product exceeds ~16 p.
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

// One group of Miller values per lane pair: group i < n is the product of the g values at index i gs + k ms (k < g) and,
// when `shared` is given, of the one value there; conjugated once (x < 0), raised to (p^12 - 1)/r.  out_gt: n x 144 words
// (the bytes of zkmi_pairing); otherwise out_status: one byte per group, 0 when the result is 1, else ZKMI_PROOF_PAIRING.
// Tail lane pairs shadow the last group and write nothing.
__global__ __launch_bounds__(64, 1) void k_final_exp(const uint32_t* __restrict__ m, uint64_t n, uint32_t g, uint64_t gs,
                                                     uint64_t ms, const uint32_t* __restrict__ shared,
                                                     uint32_t* __restrict__ out_gt, uint8_t* __restrict__ out_status) {
  const uint64_t pair = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = pair < n;
  const uint64_t idx = live ? pair : n - 1;  // n >= 1 (host)
  E12P f = e12_load(m + idx * gs * 144);
  const uint32_t members = g + (shared ? 1u : 0u);
#pragma unroll 1
  for (uint32_t k = 1; k < members; k++)
    f = e12_mul_o(f, e12_load(k < g ? m + (idx * gs + k * ms) * 144 : shared));
  f = final_exp_chain(e12_conj(f));
  if (out_gt) {
    e12_store(f, out_gt + idx * 144, live);
  } else {
    // f == 1: every coefficient of f - 1 is zero (is_zero is exact for |v| <= 4 p; f is shrunk below 2 p)
    int mine = (f.c0.a0 - E2::one()).v.is_zero() ? 1 : 0;
    mine &= (f.c0.a1.v.is_zero() && f.c0.a2.v.is_zero() && f.c1.a0.v.is_zero() && f.c1.a1.v.is_zero() && f.c1.a2.v.is_zero()) ? 1 : 0;
    const int both = mine & __builtin_amdgcn_mov_dpp(mine, 0xB1, 0xF, 0xF, true);
    if (live && !Fq2P::odd()) out_status[idx] = both ? (uint8_t)ZKMI_PROOF_OK : (uint8_t)ZKMI_PROOF_PAIRING;
  }
}

bool fq12_from_words(const uint8_t* b, Fq12* out) {
  Fq2* a[6] = {&out->c0.a0, &out->c0.a1, &out->c0.a2, &out->c1.a0, &out->c1.a1, &out->c1.a2};
  bool ok = true;
  for (int k = 0; k < 6; k++) {
    ok = fq_from_wire(b + 96 * k, &a[k]->c0) && ok;
    ok = fq_from_wire(b + 96 * k + 48, &a[k]->c1) && ok;
  }
  return ok;
}

}  // namespace

hipError_t miller_values_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, void* d_miller) {
  const dim3 grid((unsigned)((2 * n + 63) / 64)), block(64);
  hipLaunchKernelGGL(k_miller, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(d_g1),
                     static_cast<const uint32_t*>(d_g2), n, static_cast<uint32_t*>(d_miller));
  return hipGetLastError();
}

int32_t miller_product_dev(zkmi_ctx* ctx, const void* d_miller, uint64_t n, void* d_partials, Fq12* out) {
  const uint32_t np = (uint32_t)((n + 1) / 2 < MILLER_PARTIALS ? (n + 1) / 2 : MILLER_PARTIALS);
  const dim3 grid((2 * np + 63) / 64), block(64);
  hipLaunchKernelGGL(k_miller_product, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(d_miller), n, np,
                     static_cast<uint32_t*>(d_partials));
  hipError_t e = hipGetLastError();
  std::vector<uint8_t> host(np * MILLER_BYTES);
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_partials, host.size(), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return ctx->hip_fail(e, "Miller product");
  Fq12 acc = Fq12::one();
  for (uint32_t j = 0; j < np; j++) {
    Fq12 v;
    if (!fq12_from_words(host.data() + j * MILLER_BYTES, &v)) return ctx->fail(ZKMI_ERR_HIP, "Miller product: a coefficient >= p came back");
    acc = acc * v;
  }
  *out = acc;
  return ZKMI_OK;
}

hipError_t final_exp_dev(zkmi_ctx* ctx, const void* d_miller, uint64_t n, uint32_t g, uint64_t group_stride,
                         uint64_t member_stride, const void* d_shared, void* d_out_gt, void* d_out_status) {
  const dim3 grid((unsigned)((2 * n + 63) / 64)), block(64);
  hipLaunchKernelGGL(k_final_exp, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(d_miller), n, g, group_stride,
                     member_stride, static_cast<const uint32_t*>(d_shared), static_cast<uint32_t*>(d_out_gt),
                     static_cast<uint8_t*>(d_out_status));
  return hipGetLastError();
}

}  // namespace zkmi

extern "C" int32_t zkmi_pairing_batch_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, void* d_out_gt) {
  using namespace zkmi;
  ZK_ENTER(ctx);
  if (n >= (1ull << 30)) return ZKMI_ERR_BAD_ARG;
  if (n == 0) return ZKMI_OK;
  if (!d_g1 || !d_g2 || !d_out_gt || (reinterpret_cast<uintptr_t>(d_g1) & 3u) || (reinterpret_cast<uintptr_t>(d_g2) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_out_gt) & 3u))
    return ZKMI_ERR_BAD_ARG;
  ZK_HIP(ctx, ctx->staging(n * MILLER_BYTES));
  hipError_t e = miller_values_dev(ctx, d_g1, d_g2, n, ctx->d_tmp);
  if (e == hipSuccess) e = final_exp_dev(ctx, ctx->d_tmp, n, 1, 1, 0, nullptr, d_out_gt, nullptr);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // also on an error path: nothing may still use the staging buffer
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? ZKMI_OK : ctx->hip_fail(e, "pairing batch");
}

extern "C" int32_t zkmi_pairing_product_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, uint8_t out_fq12[576]) {
  using namespace zkmi;
  ZK_ENTER(ctx);
  if (!out_fq12 || n >= (1ull << 30)) return ZKMI_ERR_BAD_ARG;
  if (n == 0) {
    fq12_to_wire(Fq12::one(), out_fq12);
    return ZKMI_OK;
  }
  if (!d_g1 || !d_g2 || (reinterpret_cast<uintptr_t>(d_g1) & 3u) || (reinterpret_cast<uintptr_t>(d_g2) & 3u)) return ZKMI_ERR_BAD_ARG;
  ZK_HIP(ctx, ctx->staging((n + MILLER_PARTIALS) * MILLER_BYTES));
  uint8_t* d_miller = static_cast<uint8_t*>(ctx->d_tmp);
  const hipError_t e = miller_values_dev(ctx, d_g1, d_g2, n, d_miller);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return ctx->hip_fail(e, "Miller loops");
  }
  Fq12 f;
  const int32_t rc = miller_product_dev(ctx, d_miller, n, d_miller + n * MILLER_BYTES, &f);
  if (rc != ZKMI_OK) return rc;
  fq12_to_wire(final_exponentiation(f.conj()), out_fq12);  // x < 0: one conjugation for the whole product
  return ZKMI_OK;
}

#ifdef ZKMI_TESTING  // test scaffolding: libzkmi_exp.so only (include/zkmi_testing.h)
extern "C" int32_t zkmi_selftest_miller_formulas(const uint8_t g1_affine[96], const uint8_t g2_affine[192], uint8_t out_fq12[576]) {
  using namespace zkmi;
  if (!g1_affine || !g2_affine || !out_fq12) return ZKMI_ERR_BAD_ARG;
  G1Affine p;
  G2Affine q;
  if (!g1_from_wire(g1_affine, &p, true) || !g2_from_wire(g2_affine, &q, true)) return ZKMI_ERR_NON_CANONICAL;
  Fq12 f = Fq12::one();
  if (!p.is_inf() && !q.is_inf()) {
    const E12<Fq2> m = miller_rounds<Fq2, Fq>(q.x, q.y, p.x, p.y.neg());
    f = {{m.c0.a0, m.c0.a1, m.c0.a2}, {m.c1.a0, m.c1.a1, m.c1.a2}};
  }
  fq12_to_wire(final_exponentiation(f.conj()), out_fq12);
  return ZKMI_OK;
}
extern "C" int32_t zkmi_selftest_final_exp_formulas(const uint8_t in_fq12[576], uint8_t out_chain[576], uint8_t out_plain[576]) {
  using namespace zkmi;
  if (!in_fq12 || !out_chain || !out_plain) return ZKMI_ERR_BAD_ARG;
  Fq12 f;
  if (!fq12_from_words(in_fq12, &f)) return ZKMI_ERR_NON_CANONICAL;
  if (f.c0 == Fq6::zero() && f.c1 == Fq6::zero()) return ZKMI_ERR_BAD_ARG;
  const E12<Fq2> c = final_exp_chain<Fq2>({{f.c0.a0, f.c0.a1, f.c0.a2}, {f.c1.a0, f.c1.a1, f.c1.a2}});
  fq12_to_wire({{c.c0.a0, c.c0.a1, c.c0.a2}, {c.c1.a0, c.c1.a1, c.c1.a2}}, out_chain);
  fq12_to_wire(final_exponentiation(f), out_plain);
  return ZKMI_OK;
}
#endif  // ZKMI_TESTING
