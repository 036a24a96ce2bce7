// zkmi — verification of ceremony outputs (ceremony.hip): the same-ratio checks of a phase-1 transcript and of a phase-2
// contribution, as random linear combinations whose weights are derived on the device.
#pragma once
#include "ctx.hpp"

namespace zkmi {

// domains of the weight derivation w(seed, dom, i): the section numbers of zkmi_srs_load in phase 1, 16 + the query number
// of zkmi_pk_export_query in phase 2
constexpr uint32_t RLC_DOM_PK = 16;

// what zkmi_pk_verify_contribution reads of a key (groth16.hip owns zkmi_pk): resident queries, their 28-bit limb forms
// in natural order, the single elements
struct PkCeremonyView {
  uint32_t n_vars, n_pub, log_n;
  const G1Affine *a, *b_g1;
  const G2Affine* b_g2;
  const Affine<Fq28>*h28, *l28;  // N and n_vars entries
  G1Affine alpha_g1, beta_g1, delta_g1;
  G2Affine beta_g2, delta_g2;
};

// The four checks of a contribution (ZKMI_PK2_*) on an idle context; both keys have the same shape (the caller checked).
// ZKMI_OK with *out_failed = 0, ZKMI_ERR_VERIFICATION with the mask, or an error code with ctx->err set.
int32_t pk_verify_contribution(zkmi_ctx* ctx, const PkCeremonyView& before, const PkCeremonyView& after, const uint8_t seed[32],
                               uint32_t* out_failed);

}  // namespace zkmi
