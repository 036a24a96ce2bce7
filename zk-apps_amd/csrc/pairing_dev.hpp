// zkmi — Miller loops and their product on the device (pairing_dev.hip): the pairing side of proof verification.
#pragma once
#include "ctx.hpp"
#include "pairing.hpp"

namespace zkmi {

// bytes of one Miller value in HBM: 12 canonical Fq coefficients of 48 B in the order of fq12_to_wire, BEFORE the
// conjugation (x < 0) and the final exponentiation
constexpr uint64_t MILLER_BYTES = 576;

// f_{|x|,Q_i}(P_i) for n >= 1 pairs in HBM (affine WIRE form, 4-byte aligned) -> d_miller (n x MILLER_BYTES).  A pair
// with an infinite member gives 1.  Queued on ctx->stream; does not wait.
hipError_t miller_values_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, void* d_miller);

// prod_i d_miller[i] for n >= 1 values: the device multiplies down to at most MILLER_PARTIALS partial products in
// d_partials (room for that many values), the host multiplies those.  Waits for ctx->stream.
constexpr uint64_t MILLER_PARTIALS = 256;
int32_t miller_product_dev(zkmi_ctx* ctx, const void* d_miller, uint64_t n, void* d_partials, Fq12* out);

}  // namespace zkmi
