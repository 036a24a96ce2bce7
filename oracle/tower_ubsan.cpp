// The pairing tower of zk-apps_amd/csrc/tower_dev.hpp over Fq2_28 (both components in one lane: the host instantiation of
// zkmi_selftest_tower_ops) under UndefinedBehaviorSanitizer, host only, stand-alone (own main; `make -C oracle tower-ubsan`).
// Every op of the hook over operands at the ENDS of the interval the interval instantiation (tower_bounds_run) reports for
// their class: k p + x with k the extreme multiples the class admits and x in {0, 1, 2, p - 2, p - 1, (p +- 1) / 2, seeded
// draws} -- all high, all low, alternating, seeded mixtures.  A signed overflow of a limb or of a 64-bit column aborts
// (-fno-sanitize-recover).  Every result is also compared, as a field element, with the same template over the host's
// canonical Fq2 (32-bit limbs): a wrong value counts as a mismatch and fails the run.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../zk-apps_amd/csrc/tower_selftest.hpp"

using namespace zkmi;

static uint64_t g_bad = 0, g_checks = 0;

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

// x + k p: limb-wise sum with the normalised limbs of k p, then one carry sweep
static Fq28 shifted(const Fq28& x, int k) {
  Fq28 r;
  for (int i = 0; i < Fq28::NL; i++) r.l[i] = x.l[i] + Fq28::kp_limb(k, i);
  r.carry();
  return r;
}
static Fq28 small(int32_t v) {
  Fq28 r = Fq28::zero();
  r.l[0] = v;
  return r;
}
static Fq28 half_p(bool up) {  // (p - 1) / 2 or (p + 1) / 2 as an integer in limbs
  Fq28 r;
  for (int i = 0; i < Fq28::NL; i++) {
    const int32_t hi = i + 1 < Fq28::NL ? (Fq28Params::MOD[i + 1] & 1) : 0;
    r.l[i] = (Fq28Params::MOD[i] >> 1) | (hi << 27);
  }
  return up ? r + small(1) : r;
}
static Fq28 draw(Rng& rng) {  // an integer in [0, p): 13 random limbs under a top limb below p's
  Fq28 r;
  for (int i = 0; i < Fq28::NL - 1; i++) r.l[i] = (int32_t)(rng.next() & (uint32_t)Fq28::MASK);
  r.l[Fq28::NL - 1] = (int32_t)(rng.next() % (uint32_t)Fq28Params::MOD[Fq28::NL - 1]);
  return r;
}

// the values of a class (lo, hi), open, ends multiples of 1/2: [0] the largest few, [1] the smallest few, [2] others
struct ClassValues {
  std::vector<Fq28> hi, lo, mid;
};
static ClassValues class_values(double lo, double hi, Rng& rng) {
  ClassValues c;
  const int khi = (int)floor(hi), klo = (int)ceil(lo);
  const bool half_hi = hi != floor(hi), half_lo = lo != ceil(lo);
  const Fq28 pm1 = shifted(small(-1), 1), pm2 = shifted(small(-2), 1);  // p - 1, p - 2
  if (half_hi) {
    c.hi = {shifted(half_p(false), khi), shifted(half_p(false) - small(1), khi)};
  } else {
    c.hi = {shifted(pm1, khi - 1), shifted(pm2, khi - 1)};
  }
  if (half_lo) {
    c.lo = {shifted(half_p(true), klo - 1), shifted(half_p(true) + small(1), klo - 1)};
  } else {
    c.lo = {shifted(small(1), klo), shifted(small(2), klo)};
  }
  for (int i = 0; i < 6; i++) {
    c.hi.push_back(shifted(draw(rng), khi - 1));
    c.lo.push_back(shifted(draw(rng), klo));
  }
  for (int k = klo; k < khi; k++) {
    c.mid.push_back(shifted(small(0), k));
    c.mid.push_back(shifted(draw(rng), k));
  }
  c.mid.push_back(shifted(small(0), khi));  // k p for every k inside, the top one included when the end is a half
  if (!half_hi) c.mid.pop_back();
  return c;
}

// the same op over the host's canonical field: operands converted on the way in
struct CanonIO {
  using E2 = Fq2;
  const int32_t* in;
  Fq2* out;  // result Fq2 values, indexed by element / 2
  Fq ldq(int k) const { return fq_from_fq28(tower_ld(in + k * TNL)); }
  Fq2 ld2(int k) const { return {ldq(k), ldq(k + 1)}; }
  void st2(int k, const Fq2& v) const { out[k / 2] = v; }
};

template <int OP>
static void run_op(const char* name, const std::vector<int>& cls, const std::vector<ClassValues>& values, uint32_t tuples,
                   uint64_t seed, bool compare) {
  constexpr int NI = TOP_IN[OP], NO = TOP_OUT[OP];
  Rng rng{seed};
  std::vector<int32_t> in((size_t)tuples * NI * TNL), out((size_t)tuples * (NO ? NO : 1) * TNL);
  std::vector<uint8_t> flag(tuples);
  for (uint32_t t = 0; t < tuples; t++) {
    const uint64_t w = rng.next();
    for (int j = 0; j < NI; j++) {
      const ClassValues& c = values[cls[j]];
      int side;  // 1 high, 0 low, 2 anything
      if (t == 0) side = 1;
      else if (t == 1) side = 0;
      else if (t == 2) side = j & 1;
      else if (t == 3) side = (j + 1) & 1;
      else if (t < tuples / 2) side = (int)((w >> (j % 60)) & 1);
      else side = (int)((w >> (j % 60)) % 3);
      const std::vector<Fq28>& pool = side == 1 ? c.hi : side == 0 ? c.lo : c.mid;
      const Fq28& v = pool[t < 4 ? 0 : (size_t)(rng.next() % pool.size())];
      tower_st(&in[((size_t)t * NI + j) * TNL], v);
    }
  }
  tower_run_host<OP>(tuples, in.data(), out.data(), flag.data());
  uint64_t bad = 0;
  if constexpr (OP != TOP_SHRINK && OP != TOP_WORDS_ROUND_TRIP && OP != TOP_IS_ONE) {
    if (compare) {
      for (uint32_t t = 0; t < tuples; t++) {
        Fq2 want[NO / 2];
        const CanonIO io = {&in[(size_t)t * NI * TNL], want};
        tower_op_body<OP>(io);
        const HostIO got = {&out[(size_t)t * NO * TNL], nullptr, nullptr};
        for (int k = 0; k < NO; k += 2) {
          g_checks++;
          if (!(fq_from_fq28(got.ld2(k)) == want[k / 2])) bad++;
        }
      }
    }
  }
  g_bad += bad;
  printf("tower-ubsan: %-16s %u tuples%s, %llu mismatches\n", name, tuples, compare ? " against the canonical field" : "",
         (unsigned long long)bad);
}

int main() {
  double sites[IV_SITES], classes[2 * IVC_CLASSES];
  if (tower_bounds_run(sites, IV_SITES, classes, IVC_CLASSES) != ZKMI_OK) return 2;
  printf("tower-ubsan: interval maxima: product operand %.1f p, column budget %.1f p^2 (limit 1260), 64-bit column 2^%.2f, shrink input %.1f p, "
         "is_zero input %.1f p, any value %.1f p\n", sites[0], sites[1], sites[2], sites[3], sites[4], sites[5]);
  Rng rng{0x7031};
  std::vector<ClassValues> values;
  for (int k = 0; k < IVC_CLASSES; k++) values.push_back(class_values(classes[2 * k], classes[2 * k + 1], rng));
  auto rep = [](int c, int n) { return std::vector<int>((size_t)n, c); };
  auto cat = [](std::vector<int> a, const std::vector<int>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
  };
  const std::vector<int> T = cat(rep(IVC_T_XY, 4), rep(IVC_T_Z, 2)), Pq = rep(IVC_P, 2), Q = rep(IVC_Q, 4);
  run_op<TOP_SHRINK>("shrink", rep(IVC_SHRINK, 1), values, 512, 1, false);
  run_op<TOP_E2_MUL_XI>("e2_mul_xi", rep(IVC_E2_XI, 2), values, 512, 2, true);
  run_op<TOP_E2_CONJ>("e2_conj", rep(IVC_E2_CONJ, 2), values, 512, 3, true);
  run_op<TOP_E2_INV>("e2_inv", rep(IVC_E2_INV, 2), values, 64, 4, true);
  run_op<TOP_E6_MUL>("e6_mul", rep(IVC_E6_MUL, 12), values, 512, 5, true);
  run_op<TOP_E12_SQR>("e12_sqr", rep(IVC_F, 12), values, 512, 6, true);
  run_op<TOP_E12_MUL>("e12_mul", rep(IVC_F, 24), values, 512, 7, true);
  run_op<TOP_E12_MUL_LINE>("e12_mul_line", cat(rep(IVC_F, 12), cat(rep(IVC_L0, 2), cat(rep(IVC_L1, 2), rep(IVC_L2, 2)))), values, 512, 8, true);
  run_op<TOP_E12_CONJ>("e12_conj", rep(IVC_F, 12), values, 512, 9, true);
  run_op<TOP_E12_FROB_P>("e12_frob_p", rep(IVC_F, 12), values, 256, 10, true);
  run_op<TOP_E12_FROB_P2>("e12_frob_p2", rep(IVC_F, 12), values, 256, 11, true);
  run_op<TOP_E6_INV>("e6_inv", rep(IVC_E6_INV, 6), values, 64, 12, true);
  run_op<TOP_E12_INV>("e12_inv", rep(IVC_F, 12), values, 64, 13, true);
  // the steps and the loop on arbitrary field elements, not curve points: the formulas are polynomial identities in the
  // coordinates either way, and magnitudes do not depend on the curve equation
  run_op<TOP_STEP_TANGENT>("step_tangent", cat(T, Pq), values, 512, 14, true);
  run_op<TOP_STEP_CHORD>("step_chord", cat(T, cat(Q, Pq)), values, 512, 15, true);
  run_op<TOP_MILLER_ROUNDS>("miller_rounds", cat(Q, Pq), values, 16, 16, true);
  run_op<TOP_FINAL_EXP_CHAIN>("final_exp_chain", rep(IVC_F, 12), values, 16, 17, true);
  run_op<TOP_WORDS_ROUND_TRIP>("words_round_trip", rep(IVC_WORDS, 1), values, 512, 18, false);
  run_op<TOP_IS_ONE>("is_one", rep(IVC_F, 12), values, 512, 19, false);
  printf("tower-ubsan: %llu checks, %llu mismatches\n", (unsigned long long)g_checks, (unsigned long long)g_bad);
  return g_bad ? 1 : 0;
}
