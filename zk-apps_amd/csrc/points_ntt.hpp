// zkmi — group-element transforms (points_ntt.hip): a radix-2 transform over Fr's 2^log_n domain whose elements are curve
// points, and the resident phase-1 transcript it is meant for.
#pragma once
#include <vector>
#include "ctx.hpp"

// a phase-1 transcript ("powers of tau" with alpha and beta), resident form (Affine<Fq> / Affine<Fq2>, Montgomery R = 2^384)
struct zkmi_srs {
  zkmi_ctx* ctx = nullptr;
  int device = -1;
  zkmi::G1Affine *tau_g1 = nullptr, *alpha_tau_g1 = nullptr, *beta_tau_g1 = nullptr;
  zkmi::G2Affine* tau_g2 = nullptr;
  zkmi::G2Affine beta_g2;
  uint64_t n_tau_g1 = 0, n_tau_g2 = 0, n_ab = 0;
  int32_t checks = 0;  // ZKMI_CHECK_* every point was read under (zkmi_srs_generate: all of them); zkmi_srs_verify asks for SUBGROUP
  ~zkmi_srs() {
    if (device >= 0) (void)hipSetDevice(device);
    for (void* p : {(void*)tau_g1, (void*)alpha_tau_g1, (void*)beta_tau_g1, (void*)tau_g2})
      if (p) (void)hipFree(p);
  }
};

namespace zkmi {

// groth16.hip: table[w * 256 + d] = d * 2^(8w) * base in HBM (the caller frees it), and out[i] = scalars[i] * base
template <class F>
hipError_t fixed_base_table(const Affine<F>& base, Affine<F>** d_table);
template <class F>
hipError_t fixed_base_batch(zkmi_ctx* ctx, const Affine<F>* d_table, const std::vector<Fr>& scalars_mont, Affine<F>* d_out);

// w^k for k < max(1, 2^(log_n - 1)), canonical 8-word scalars in HBM (the caller frees them); w = fr_root_of_unity(log_n).
// One table serves both directions: w^(-k) = -w^(N/2 - k).
hipError_t points_ntt_twiddles(uint32_t log_n, uint32_t** d_tw);

// `count` arrays of 2^log_n points in the resident form, array a at d_pts + a * stride, transformed in place (natural
// order in and out; the inverse scaled by N^-1).  One launch per level covers all the arrays.  Queued on ctx->stream;
// returns after the stream has drained.
template <class F>
hipError_t points_ntt_resident(zkmi_ctx* ctx, Affine<F>* d_pts, uint64_t stride, uint32_t count, uint32_t log_n,
                               bool inverse, const uint32_t* d_tw);

}  // namespace zkmi
