// zkmi — every point of an array times a scalar of its own (points_mul.hip): the arithmetic of a phase-1 contribution
// (DESIGN.md 5.9).
#pragma once
#include "ctx.hpp"

namespace zkmi {

constexpr uint32_t PM_WINDOW = 4;         // bits per signed digit of the multiplication body
constexpr uint32_t FR_POWERS_CHUNK = 64;  // consecutive powers one lane of k_fr_powers walks
constexpr uint64_t PM_MAX_POINTS = 1ull << 28;

// d_out[i] = d_k[i] * d_in[i]: n points in the resident form, n canonical 8-word scalars in HBM (the caller has checked
// them < r); d_out may equal d_in.  Queued on ctx->stream; returns after the stream has drained.
template <class F>
int32_t points_mul_each_resident(zkmi_ctx* ctx, const Affine<F>* d_in, const uint32_t* d_k, uint64_t n, Affine<F>* d_out);

// d_out[i] = the canonical words of c * q^i for i < n (c, q in Montgomery form), made on the device.  The q^(2^t) table
// is overwritten on the host and on the device before it is freed; d_out is the caller's to wipe.  Waits.
int32_t fr_powers_dev(zkmi_ctx* ctx, const Fr& c, const Fr& q, uint64_t n, uint32_t* d_out);

// zeros over secret bytes: the host form is not elided by the compiler, the device form is queued on `st`
void wipe_host(void* p, size_t bytes);
hipError_t wipe_dev(void* d, uint64_t bytes, hipStream_t st);

// ZKMI_TESTING: the accumulators behind zkmi_points_mul_phases start again (the product library compiles this to nothing)
void points_mul_phases_reset();

}  // namespace zkmi
