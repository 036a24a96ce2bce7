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

// n >= 1 groups of Miller values -> conj, ^((p^12 - 1)/r) on the device.  Group i is the product of the g values at index
// i * group_stride + k * member_stride (k < g) of d_miller and, when d_shared is given, of the one value there.  Either
// d_out_gt (n x MILLER_BYTES: the bytes of zkmi_pairing) or d_out_status (n bytes: ZKMI_PROOF_OK when the result is 1,
// else ZKMI_PROOF_PAIRING) is written.  Queued on ctx->stream; does not wait.
hipError_t final_exp_dev(zkmi_ctx* ctx, const void* d_miller, uint64_t n, uint32_t g, uint64_t group_stride,
                         uint64_t member_stride, const void* d_shared, void* d_out_gt, void* d_out_status);

}  // namespace zkmi
