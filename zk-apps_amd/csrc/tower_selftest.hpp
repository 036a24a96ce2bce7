// zkmi — TEST SCAFFOLDING over tower_dev.hpp (include/zkmi_testing.h): nothing here is compiled into the product library.
//   * the tower's Fq2 primitives over Fq2_28 (both components in one lane): the HOST path of zkmi_selftest_tower_ops and of
//     oracle/tower_ubsan.cpp -- the same templated bodies the lane pairs run;
//   * the same primitives over an INTERVAL type (units of p): where every operand of a product, of shrink and of is_zero may
//     lie and what every column sums up to (zkmi_selftest_tower_bounds);
//   * one operation of the tower on a tuple of RAW limb arrays, over an element-access policy (host: HostIO, lane pair: PairIO).
// The overloads live in namespace zkmi proper, not in tower_dev.hpp's unnamed namespace: the templates find them by
// argument-dependent lookup at their point of instantiation.
#pragma once
#include <math.h>
#include <mutex>
#include "tower_dev.hpp"
#include "../../include/zkmi.h"

namespace zkmi {

// ---- the tower's Fq2 primitives over Fq2_28 (both components in one lane; the host path) --------------------------------
static inline Fq2_28 e2_mul(const Fq2_28& a, const Fq2_28& b) { return a * b; }
static inline Fq2_28 e2_sqr(const Fq2_28& a) { return a.sqr(); }
static inline Fq2_28 e2_mul_sub_mul(const Fq2_28& a, const Fq2_28& b, const Fq2_28& c, const Fq2_28& d) { return f_mul_sub_mul(a, b, c, d); }
static inline Fq2_28 e2_mul_fq(const Fq2_28& a, const Fq28& k) { return {fq_mul(a.c0, k), fq_mul(a.c1, k)}; }
static inline Fq2_28 e2_mul_xi(const Fq2_28& a) { return a.mul_xi(); }
static inline Fq2_28 e2_conj(const Fq2_28& a) { return a.conj(); }
static inline Fq2_28 shrink(const Fq2_28& a) { return {shrink(a.c0), shrink(a.c1)}; }
// as the lane pair does it: both squares, one inversion in Fq, each component scaled, c1 negated
static inline Fq2_28 e2_inv(const Fq2_28& a) {
  const Fq28 d = (fq_mul(a.c0, a.c0) + fq_mul(a.c1, a.c1)).inv();
  return {fq_mul(a.c0, d), fq_mul(a.c1, d).neg()};
}
template <int K>
static inline Fq2_28 frob_p1(const Fq2_28*) {
  bool z;
  return {limbs_from_words(FrobK::P1[K][0], &z), limbs_from_words(FrobK::P1[K][1], &z)};
}
template <int K>
static inline Fq28 frob_p2(const Fq2_28*) {
  bool z;
  return limbs_from_words(FrobK::P2[K], &z);
}
static inline E12<Fq2_28> e12_mul_o(const E12<Fq2_28>& a, const E12<Fq2_28>& b) { return e12_mul(a, b); }
static inline E12<Fq2_28> e12_sqr_o(const E12<Fq2_28>& a) { return e12_sqr(a); }
static inline bool e12_is_one(const E12<Fq2_28>& f) {
  return (f.c0.a0 - Fq2_28::one()).is_zero() && f.c0.a1.is_zero() && f.c0.a2.is_zero() && f.c1.a0.is_zero() && f.c1.a1.is_zero() &&
         f.c1.a2.is_zero();
}

// ---- the interval instantiation ---------------------------------------------------------------------------------------
// An Iv2 is a closed interval, in units of p, that holds BOTH components of an Fq2 value; IvQ the same for a value of Fq.
// Sums propagate it; a product records what it was given and returns the (-1/2, 3/2) that a Montgomery product promises
// while its column sum stays below R p / 2 -- which tests/test_cpu_tower.py asserts of the recorded maximum.  Intervals
// ignore correlation (x - x is not 0 here), so every figure is an over-estimate.
enum IvSite : int {
  IV_PROD_OPERAND = 0,  // |a| of an operand of a Montgomery product as the multiplier sees it (the lazy 2 a of a squaring)
  IV_PROD_BUDGET,       // sum over the partial products of one reduction of |a| |b|, in p^2
  IV_COLUMN_LOG2,       // log2 of the bound on a 64-bit column: 14 limb products per partial product + the reduction's 14 + carry
  IV_SHRINK_IN,         // |a| handed to shrink
  IV_IS_ZERO_IN,        // |a| handed to is_zero
  IV_STORED,            // |a| of any value held in limbs
  IV_SITES
};
enum IvClass : int {
  IVC_F = 0,     // coefficient of an Fq12 value between tower operations
  IVC_T_XY,      // x, y of T
  IVC_T_Z,       // z of T
  IVC_Q,         // xQ, yQ
  IVC_P,         // xP, -yP
  IVC_L0,        // line coefficients
  IVC_L1,
  IVC_L2,
  IVC_E6_MUL,    // coefficient of an operand of e6_mul
  IVC_E6_INV,    // ... of e6_inv
  IVC_E2_XI,     // operand of e2_mul_xi
  IVC_E2_CONJ,   // ... of e2_conj
  IVC_E2_INV,    // ... of e2_inv
  IVC_SHRINK,    // ... of shrink
  IVC_WORDS,     // ... of limbs_to_words
  IVC_CLASSES
};
struct IvState {
  double site[IV_SITES];
  double lo[IVC_CLASSES], hi[IVC_CLASSES];
};
static IvState* iv_state = nullptr;  // set by zkmi_selftest_tower_bounds for the duration of a run (under its mutex)
static inline void iv_site(int k, double m) {
  if (m > iv_state->site[k]) iv_state->site[k] = m;
}
static inline void iv_class(int k, double lo, double hi) {
  if (lo < iv_state->lo[k]) iv_state->lo[k] = lo;
  if (hi > iv_state->hi[k]) iv_state->hi[k] = hi;
}
struct IvQ {
  double lo, hi;
  double mag() const { return fmax(fabs(lo), fabs(hi)); }
  IvQ neg() const { return {-hi, -lo}; }
};
struct Iv2 {
  double lo, hi;
  double mag() const { return fmax(fabs(lo), fabs(hi)); }
  static Iv2 held(double lo, double hi) {
    iv_site(IV_STORED, fmax(fabs(lo), fabs(hi)));
    return {lo, hi};
  }
  static Iv2 one() { return {0.0, 1.0}; }  // canonical: R mod p
  static Iv2 zero() { return {0.0, 0.0}; }
  friend Iv2 operator+(const Iv2& a, const Iv2& b) { return held(a.lo + b.lo, a.hi + b.hi); }
  friend Iv2 operator-(const Iv2& a, const Iv2& b) { return held(a.lo - b.hi, a.hi - b.lo); }
  Iv2 neg() const { return held(-hi, -lo); }
  Iv2 dbl() const { return held(2 * lo, 2 * hi); }
};
// the largest limb of a value of magnitude m (units of p) whose low limbs are `lazy` times a normalised limb: p's top limb
// is 0x1a011 = 106513 and a carried value's top limb is floor(v / 2^364)
static inline double iv_limb(double m, double lazy) { return fmax(lazy * 268435456.0, m * 106514.0 + 2.0); }
// one reduction over the partial products (a_i, b_i): operands as the multiplier sees them
static inline Iv2 iv_product(int np, const double* a, const double* b, const double* lazy_a, const double* lazy_b) {
  double budget = 0, col = 14.0 * 268435456.0 * 268435456.0;  // the reduction's m_k MOD[j]
  for (int i = 0; i < np; i++) {
    iv_site(IV_PROD_OPERAND, fmax(a[i], b[i]));
    budget += a[i] * b[i];
    col += 14.0 * iv_limb(a[i], lazy_a[i]) * iv_limb(b[i], lazy_b[i]);
  }
  col += col / 268435456.0 + 1.0;  // the carry from the column below
  iv_site(IV_PROD_BUDGET, budget);
  iv_site(IV_COLUMN_LOG2, log2(col));
  return Iv2::held(-0.5, 1.5);
}
static const double IV_ONES[4] = {1, 1, 1, 1};
// Fq2P::operator*: each lane sums two partial products, a0 b0 - a1 b1 or a0 b1 + a1 b0
static inline Iv2 e2_mul(const Iv2& a, const Iv2& b) {
  const double x[2] = {a.mag(), a.mag()}, y[2] = {b.mag(), b.mag()};
  return iv_product(2, x, y, IV_ONES, IV_ONES);
}
// Fq2P::sqr: ONE product per lane of lazy operands, (a0 + a1)(a0 - a1) or (2 a0) a1
static inline Iv2 e2_sqr(const Iv2& a) {
  const double x[1] = {2 * a.mag()}, two[1] = {2};
  return iv_product(1, x, x, two, two);
}
// f_mul_sub_mul(Fq2P): four partial products per lane under one reduction
static inline Iv2 e2_mul_sub_mul(const Iv2& a, const Iv2& b, const Iv2& c, const Iv2& d) {
  const double x[4] = {a.mag(), a.mag(), c.mag(), c.mag()}, y[4] = {b.mag(), b.mag(), d.mag(), d.mag()};
  return iv_product(4, x, y, IV_ONES, IV_ONES);
}
static inline Iv2 iv_fq_mul(double a, double b) {
  const double x[1] = {a}, y[1] = {b};
  return iv_product(1, x, y, IV_ONES, IV_ONES);
}
static inline Iv2 e2_mul_fq(const Iv2& a, const IvQ& k) { return iv_fq_mul(a.mag(), k.mag()); }
static inline Iv2 e2_mul_xi(const Iv2& a) {  // (c0 - c1, c0 + c1)
  iv_class(IVC_E2_XI, a.lo, a.hi);
  return Iv2::held(fmin(a.lo - a.hi, 2 * a.lo), fmax(a.hi - a.lo, 2 * a.hi));
}
static inline Iv2 e2_conj(const Iv2& a) {  // (c0, -c1)
  iv_class(IVC_E2_CONJ, a.lo, a.hi);
  return Iv2::held(fmin(a.lo, -a.hi), fmax(a.hi, -a.lo));
}
static inline Iv2 shrink(const Iv2& a) {
  iv_site(IV_SHRINK_IN, a.mag());
  iv_class(IVC_SHRINK, a.lo, a.hi);
  return Iv2::held(-2.0, 2.0);
}
// e2_inv(Fq2P): s = v^2, the sum of both squares, Fp28::inv (squarings and products by its argument, all of them products
// of a product by a value in s + partner(s)), a product by v, one negation
static inline Iv2 e2_inv(const Iv2& a) {
  iv_class(IVC_E2_INV, a.lo, a.hi);
  const Iv2 s = iv_fq_mul(a.mag(), a.mag());
  const Iv2 n = s + s;
  (void)iv_fq_mul(n.mag(), n.mag());  // first squaring of the ladder: its argument itself
  (void)iv_fq_mul(1.5, 1.5);
  (void)iv_fq_mul(1.5, n.mag());
  const Iv2 t = iv_fq_mul(a.mag(), 1.5);
  return Iv2::held(fmin(t.lo, -t.hi), fmax(t.hi, -t.lo));
}
template <int K>
static inline Iv2 frob_p1(const Iv2*) {
  return Iv2::held(-0.5, 1.5);  // limbs_from_words: a product
}
template <int K>
static inline IvQ frob_p2(const Iv2*) {
  return {-0.5, 1.5};
}
static inline E12<Iv2> e12_mul_o(const E12<Iv2>& a, const E12<Iv2>& b) { return e12_mul(a, b); }
static inline E12<Iv2> e12_sqr_o(const E12<Iv2>& a) { return e12_sqr(a); }
static inline bool e12_is_one(const E12<Iv2>& f) {
  iv_site(IV_IS_ZERO_IN, (f.c0.a0 - Iv2::one()).mag());
  const Iv2* c[5] = {&f.c0.a1, &f.c0.a2, &f.c1.a0, &f.c1.a1, &f.c1.a2};
  for (int k = 0; k < 5; k++) iv_site(IV_IS_ZERO_IN, c[k]->mag());
  return false;
}
// recorders of operand classes: non-template overloads that argument-dependent lookup prefers over the templates for Iv2
static inline void iv_class6(int k, const E6<Iv2>& a) {
  iv_class(k, a.a0.lo, a.a0.hi);
  iv_class(k, a.a1.lo, a.a1.hi);
  iv_class(k, a.a2.lo, a.a2.hi);
}
static inline E6<Iv2> e6_mul(const E6<Iv2>& a, const E6<Iv2>& b) {
  iv_class6(IVC_E6_MUL, a);
  iv_class6(IVC_E6_MUL, b);
  return e6_mul<Iv2>(a, b);
}
static inline E6<Iv2> e6_inv(const E6<Iv2>& a) {
  iv_class6(IVC_E6_INV, a);
  return e6_inv<Iv2>(a);
}
static inline E12<Iv2> e12_mul_line(const E12<Iv2>& f, const Iv2& l0, const Iv2& l1, const Iv2& l2) {
  iv_class(IVC_L0, l0.lo, l0.hi);
  iv_class(IVC_L1, l1.lo, l1.hi);
  iv_class(IVC_L2, l2.lo, l2.hi);
  return e12_mul_line<Iv2>(f, l0, l1, l2);
}
static inline void iv_class12(int k, const E12<Iv2>& a) {
  iv_class6(k, a.c0);
  iv_class6(k, a.c1);
}

// ---- one operation on raw limbs -----------------------------------------------------------------------------------------
namespace {
enum TowerOp : int {
  TOP_SHRINK = 0, TOP_E2_MUL_XI, TOP_E2_CONJ, TOP_E2_INV, TOP_E6_MUL, TOP_E12_SQR, TOP_E12_MUL, TOP_E12_MUL_LINE, TOP_E12_CONJ,
  TOP_E12_FROB_P, TOP_E12_FROB_P2, TOP_E6_INV, TOP_E12_INV, TOP_STEP_TANGENT, TOP_STEP_CHORD, TOP_MILLER_ROUNDS,
  TOP_FINAL_EXP_CHAIN, TOP_WORDS_ROUND_TRIP, TOP_IS_ONE, TOP_COUNT
};
// Fq elements (14 limbs) per tuple
constexpr int TOP_IN[TOP_COUNT] = {1, 2, 2, 2, 12, 12, 24, 18, 12, 12, 12, 6, 12, 8, 12, 6, 12, 1, 12};
constexpr int TOP_OUT[TOP_COUNT] = {1, 2, 2, 2, 6, 12, 12, 12, 12, 12, 12, 6, 12, 12, 12, 12, 12, 2, 0};
constexpr int TNL = Fq28::NL;

PD_HD Fq28 tower_ld(const int32_t* p) {
  Fq28 r;
#pragma unroll
  for (int i = 0; i < TNL; i++) r.l[i] = p[i];
  return r;
}
PD_HD void tower_st(int32_t* p, const Fq28& v) {
#pragma unroll
  for (int i = 0; i < TNL; i++) p[i] = v.l[i];
}
// element access of one tuple: an Fq2 value is the two Fq elements k (c0), k + 1 (c1)
struct HostIO {
  using E2 = Fq2_28;
  const int32_t* in;
  int32_t* out;
  uint8_t* flag;
  Fq28 ldq(int k) const { return tower_ld(in + k * TNL); }
  E2 ld2(int k) const { return {tower_ld(in + k * TNL), tower_ld(in + (k + 1) * TNL)}; }
  void stq(int k, const Fq28& v) const { tower_st(out + k * TNL, v); }
  void st2(int k, const E2& v) const {
    tower_st(out + k * TNL, v.c0);
    tower_st(out + (k + 1) * TNL, v.c1);
  }
  void stw(int k, const uint32_t* w) const {
    for (int i = 0; i < TNL; i++) out[k * TNL + i] = i < 12 ? (int32_t)w[i] : 0;
  }
  void set_flag(bool b) const { *flag = b ? 1 : 0; }
};
#if defined(__HIPCC__)  // (Fq2P exists under hipcc only)
struct PairIO {  // one lane of a lane pair: its component of every Fq2 value; the even lane writes what is not split
  using E2 = Fq2P;
  const int32_t* in;
  int32_t* out;
  uint8_t* flag;
  uint32_t comp;
  bool live;
  __device__ Fq28 ldq(int k) const { return tower_ld(in + k * TNL); }
  __device__ E2 ld2(int k) const { return {tower_ld(in + (k + comp) * TNL)}; }
  __device__ void stq(int k, const Fq28& v) const {
    if (live && comp == 0) tower_st(out + k * TNL, v);
  }
  __device__ void st2(int k, const E2& v) const {
    if (live) tower_st(out + (k + comp) * TNL, v.v);
  }
  __device__ void stw(int k, const uint32_t* w) const {
    if (live && comp == 0)
      for (int i = 0; i < TNL; i++) out[k * TNL + i] = i < 12 ? (int32_t)w[i] : 0;
  }
  __device__ void set_flag(bool b) const {
    if (live && comp == 0) *flag = b ? 1 : 0;
  }
};
#endif
template <class IO>
PD_HD E6<typename IO::E2> tower_ld6(const IO& io, int k) {
  return {io.ld2(k), io.ld2(k + 2), io.ld2(k + 4)};
}
template <class IO>
PD_HD E12<typename IO::E2> tower_ld12(const IO& io, int k) {  // the coefficient order of e12_load
  return {tower_ld6(io, k), tower_ld6(io, k + 6)};
}
template <class IO>
PD_HD void tower_st6(const IO& io, int k, const E6<typename IO::E2>& a) {
  io.st2(k, a.a0);
  io.st2(k + 2, a.a1);
  io.st2(k + 4, a.a2);
}
template <class IO>
PD_HD void tower_st12(const IO& io, int k, const E12<typename IO::E2>& a) {
  tower_st6(io, k, a.c0);
  tower_st6(io, k + 6, a.c1);
}
template <int OP, class IO>
PD_HD void tower_op_body(const IO& io) {
  using E2 = typename IO::E2;
  if constexpr (OP == TOP_SHRINK) io.stq(0, shrink(io.ldq(0)));
  if constexpr (OP == TOP_E2_MUL_XI) io.st2(0, e2_mul_xi(io.ld2(0)));
  if constexpr (OP == TOP_E2_CONJ) io.st2(0, e2_conj(io.ld2(0)));
  if constexpr (OP == TOP_E2_INV) io.st2(0, e2_inv(io.ld2(0)));
  if constexpr (OP == TOP_E6_MUL) tower_st6(io, 0, e6_mul(tower_ld6(io, 0), tower_ld6(io, 6)));
  if constexpr (OP == TOP_E12_SQR) tower_st12(io, 0, e12_sqr(tower_ld12(io, 0)));
  if constexpr (OP == TOP_E12_MUL) tower_st12(io, 0, e12_mul(tower_ld12(io, 0), tower_ld12(io, 12)));
  if constexpr (OP == TOP_E12_MUL_LINE) tower_st12(io, 0, e12_mul_line(tower_ld12(io, 0), io.ld2(12), io.ld2(14), io.ld2(16)));
  if constexpr (OP == TOP_E12_CONJ) tower_st12(io, 0, e12_conj(tower_ld12(io, 0)));
  if constexpr (OP == TOP_E12_FROB_P) tower_st12(io, 0, e12_frob_p(tower_ld12(io, 0)));
  if constexpr (OP == TOP_E12_FROB_P2) tower_st12(io, 0, e12_frob_p2(tower_ld12(io, 0)));
  if constexpr (OP == TOP_E6_INV) tower_st6(io, 0, e6_inv(tower_ld6(io, 0)));
  if constexpr (OP == TOP_E12_INV) tower_st12(io, 0, e12_inv(tower_ld12(io, 0)));
  if constexpr (OP == TOP_STEP_TANGENT || OP == TOP_STEP_CHORD) {
    Jac<E2> t = {io.ld2(0), io.ld2(2), io.ld2(4)};
    E2 l0, l1, l2;
    if constexpr (OP == TOP_STEP_TANGENT) step_tangent(t, io.ldq(6), io.ldq(7), l0, l1, l2);
    else step_chord(t, io.ld2(6), io.ld2(8), io.ldq(10), io.ldq(11), l0, l1, l2);
    io.st2(0, t.x);
    io.st2(2, t.y);
    io.st2(4, t.z);
    io.st2(6, l0);
    io.st2(8, l1);
    io.st2(10, l2);
  }
  if constexpr (OP == TOP_MILLER_ROUNDS) tower_st12(io, 0, miller_rounds(io.ld2(0), io.ld2(2), io.ldq(4), io.ldq(5)));
  if constexpr (OP == TOP_FINAL_EXP_CHAIN) tower_st12(io, 0, final_exp_chain(tower_ld12(io, 0)));
  if constexpr (OP == TOP_WORDS_ROUND_TRIP) {
    uint32_t w[12];
    limbs_to_words(io.ldq(0), w, true);
    io.stw(0, w);
    bool z;
    io.stq(1, limbs_from_words(w, &z));
  }
  if constexpr (OP == TOP_IS_ONE) io.set_flag(e12_is_one(tower_ld12(io, 0)));
}

template <int OP>
static inline void tower_run_host(uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  for (uint32_t t = 0; t < n; t++) {
    const HostIO io = {in + (size_t)t * TOP_IN[OP] * TNL, out + (size_t)t * TOP_OUT[OP] * TNL, OP == TOP_IS_ONE ? out_flag + t : nullptr};
    tower_op_body<OP>(io);
  }
}
}  // namespace

// out_sites[6]: the IvSite maxima; out_classes[2 x 15]: lo, hi of every IvClass
static inline int32_t tower_bounds_run(double* out_sites, uint32_t n_sites, double* out_classes, uint32_t n_classes) {
  if (!out_sites || !out_classes || n_sites != (uint32_t)IV_SITES || n_classes != (uint32_t)IVC_CLASSES) return ZKMI_ERR_BAD_ARG;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  IvState st;
  for (int k = 0; k < IV_SITES; k++) st.site[k] = 0;
  for (int k = 0; k < IVC_CLASSES; k++) st.lo[k] = 1e300, st.hi[k] = -1e300;
  iv_state = &st;
  // entry conditions of the kernels: limbs_from_words returns a product, -yP is the negation of one, one() is canonical
  const Iv2 prod = Iv2::held(-0.5, 1.5), shrunk = Iv2::held(-2.0, 2.0);
  const IvQ xp = {-0.5, 1.5}, nyp = xp.neg();
  iv_class(IVC_Q, prod.lo, prod.hi);
  iv_class(IVC_P, xp.lo, xp.hi);
  iv_class(IVC_P, nyp.lo, nyp.hi);
  // k_miller
  const E12<Iv2> m = miller_rounds<Iv2, IvQ>(prod, prod, xp, nyp);
  iv_class12(IVC_F, m);
  iv_class12(IVC_WORDS, m);
  // T between rounds: (x, y) shrunk or Q's, z = 1, a doubled product (tangent) or a product (chord); one more step of each
  // kind from the whole class, so that the line classes hold every round's
  iv_class(IVC_T_XY, prod.lo, prod.hi);
  iv_class(IVC_T_XY, shrunk.lo, shrunk.hi);
  iv_class(IVC_T_Z, 0.0, 1.0);
  for (int round = 0; round < 2; round++) {
    const Jac<Iv2> t0 = {{st.lo[IVC_T_XY], st.hi[IVC_T_XY]}, {st.lo[IVC_T_XY], st.hi[IVC_T_XY]}, {st.lo[IVC_T_Z], st.hi[IVC_T_Z]}};
    const E12<Iv2> f = {{shrunk, shrunk, shrunk}, {shrunk, shrunk, shrunk}};
    for (int chord = 0; chord < 2; chord++) {
      Jac<Iv2> t = t0;
      Iv2 l0, l1, l2;
      if (chord) step_chord(t, prod, prod, xp, nyp, l0, l1, l2);
      else step_tangent(t, xp, nyp, l0, l1, l2);
      iv_class(IVC_T_XY, t.x.lo, t.x.hi);
      iv_class(IVC_T_XY, t.y.lo, t.y.hi);
      iv_class(IVC_T_Z, t.z.lo, t.z.hi);
      iv_class12(IVC_F, e12_mul_line(f, l0, l1, l2));
    }
  }
  // k_miller_product / k_final_exp: products of loaded (product) or shrunk values, one conjugation, the chain, the status
  const E12<Iv2> f = {{shrunk, shrunk, shrunk}, {shrunk, shrunk, shrunk}};
  const E12<Iv2> prod12 = e12_mul_o(f, f);
  iv_class12(IVC_F, prod12);
  const E12<Iv2> r = final_exp_chain(e12_conj(f));
  iv_class12(IVC_F, r);
  iv_class12(IVC_WORDS, r);
  (void)e12_is_one(r);
  iv_state = nullptr;
  for (int k = 0; k < IV_SITES; k++) out_sites[k] = st.site[k];
  for (int k = 0; k < IVC_CLASSES; k++) out_classes[2 * k] = st.lo[k], out_classes[2 * k + 1] = st.hi[k];
  return ZKMI_OK;
}

}  // namespace zkmi
