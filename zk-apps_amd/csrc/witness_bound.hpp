// zkmi — where the values of the witness map may lie between the mat-vec and the first inverse transforms, decided from the
// SHAPE of a relation at key build.  Host only, a pure function of the row pointers.
//
// The mat-vec kernels add k products of (-r/2, 3r/2) without reducing: a row of k terms leaves |v| < 3/2 k r.  The first
// inverse transform (ntt.hip, decimation in frequency) adds such values without reducing either: within one pass, the node
// that only ever took the sum path holds the integer sum of all 2^S inputs of its sub-transform.  Plans of two passes multiply
// every element by a twist behind the first pass, which brings it back to (-r/2, 3r/2); plans of three passes (N > 2^20) and of
// one pass do not, so the whole vector is one coherent set.  What a node may hold is the signed 32-bit top limb:
// |v| < 2^31 2^252.  A matrix whose worst-case coherent sum reaches that is NORMALISED: its mat-vec multiplies each row sum by
// one() (k_matvec<S, NORM>, k_matvec_long<NORM>), after which every row is in (-r/2, 3r/2) and a coherent sum is at most
// 3/2 N r (N = 2^26: 2^26.6 r).  The worst case takes 3/2 r for every term; tests/witness28.py restates the rule over
// Python integers and tests/test_cpu_witness_bounds.py holds this function to it.
#pragma once
#include <stdint.h>
#include <vector>
#include "field28.hpp"

namespace zkmi {

constexpr int NTT_MAX_PASS_STAGES = 10;  // ntt.hip run_passes: a pass owns at most 10 stages

struct WitnessBound {
  uint32_t normalise = 0;     // bit m: matrix m (A, B, C) is normalised
  uint64_t half_r[3] = {};    // the largest coherent sum of the first inverse transform of matrix m, in units of r / 2
};

// rowptr[m]: nc + 1 entries.  Rows [nc, nc + n_pub) of A hold the instance variables themselves (one term each).
inline WitnessBound witness_bound(uint32_t log_n, uint32_t n_pub, uint32_t nc, const uint32_t* const rowptr[3]) {
  WitnessBound out;
  const int np = ((int)log_n + NTT_MAX_PASS_STAGES - 1) / NTT_MAX_PASS_STAGES;
  // coherent sets: two passes -> the stride classes i mod 2^10 of the first (high-stage) pass; otherwise the whole vector
  const uint32_t class_bits = np == 2 ? (uint32_t)NTT_MAX_PASS_STAGES : 0u;
  const uint32_t first_stages = np == 2 ? log_n - class_bits : log_n;
  const uint64_t N = 1ull << log_n;
  // |v| <= b r / 2 fits when b r + 2^253 <= 2^284: one unit of the top limb stays free at either end (a lazy difference is not
  // carried).  r's top 64 bits, rounded up, decide it as b (r_hi + 1) + 2^61 <= 2^92 -- never later than the exact test.
  const unsigned __int128 r_hi1 = (((unsigned __int128)Fr28Params::MOD32[7] << 32) | Fr28Params::MOD32[6]) + 1u;
  const unsigned __int128 limit = ((unsigned __int128)1 << 92) - ((unsigned __int128)1 << 61);
  std::vector<uint64_t> sum((size_t)1 << class_bits);
  for (int m = 0; m < 3; m++) {
    std::fill(sum.begin(), sum.end(), 0);
    const uint32_t mask = (1u << class_bits) - 1u;
    for (uint64_t i = 0; i < nc && i < N; i++) sum[i & mask] += rowptr[m][i + 1] - rowptr[m][i];
    if (m == 0)
      for (uint64_t i = nc; i < (uint64_t)nc + n_pub && i < N; i++) sum[i & mask] += 1;
    uint64_t terms = 0;
    for (uint64_t s : sum) terms = s > terms ? s : terms;
    out.half_r[m] = 3 * terms;
    // (the difference path -- a product behind a stage, sums only from there -- stays below 3/2 r 2^(stages - 1))
    const uint64_t diff = first_stages ? 3ull << (first_stages - 1) : 0;
    const unsigned __int128 b = 3 * terms > diff ? 3 * terms : diff;
    if (b * r_hi1 > limit) out.normalise |= 1u << m;
  }
  return out;
}

}  // namespace zkmi
