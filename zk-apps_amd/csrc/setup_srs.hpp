// zkmi — a relation's Groth16 key from a phase-1 transcript (setup_srs.hip): Lagrange bases by the point transform, the
// R1CS column sums, the h query, and the scaling a phase-2 contribution applies.  groth16.hip owns zkmi_pk and the entry
// points; this file fills the five query arrays.
#pragma once
#include "colsum_plan.hpp"
#include "ctx.hpp"
#include "points_ntt.hpp"
#include "r1cs.hpp"

namespace zkmi {

// groth16.hip: [L_i(tau)] for the 2^log_n domain and Z(tau) = tau^N - 1; false when tau lies in the domain
bool lagrange_basis_at(uint32_t log_n, const Fr& tau, std::vector<Fr>* L, Fr* zt);

// The plan of one column query, numbered as zkmi_pk_export_query numbers them: 0 a, 1 b_g1, 2 b_g2, 4 l (all n_vars slots;
// the first n_pub of l are the verifying key's gamma_abc_g1).  Base-array selectors: 0 [L_i], 1 [alpha L_i], 2 [beta L_i].
// false: which is none of these, or the relation has 2^31 terms or more.
bool setup_colsum_plan(const zkmi_r1cs& r, int which, ColsumPlan* plan);

struct SetupQueries {
  G1Affine *a, *b_g1, *l, *h;  // n_vars, n_vars, n_vars (public part included), N (h[N - 1] blank)
  G2Affine* b_g2;
};
// Fills the five resident query arrays of a key from the transcript (gamma = delta = 1) and reads alpha_g1 / beta_g1.
// The transcript is only read.  ZKMI_OK or an error code with ctx->err set.
int32_t setup_queries_from_srs(zkmi_ctx* ctx, const zkmi_r1cs* r, const zkmi_srs* srs, const SetupQueries& out,
                               G1Affine* alpha_g1, G1Affine* beta_g1);

// d_pts[i] <- k * d_pts[i] for one canonical 8-word scalar, in place (resident form); returns after the stream has drained
template <class F>
int32_t points_scale_resident(zkmi_ctx* ctx, Affine<F>* d_pts, uint64_t n, const uint32_t k[8]);

}  // namespace zkmi
