// zkmi — point arrays parsed, decompressed and checked on the device (points.hip): the ingest side of keys and bases.
#pragma once
#include "ctx.hpp"

namespace zkmi {

// a fourth, internal encoding beside ZKMI_ENC_*: the resident form keys and bases hold (Affine<Fq> / Affine<Fq2>,
// Montgomery R = 2^384) -- what zkmi_pk_check reads
constexpr int32_t PT_ENC_RESIDENT = 3;

// bytes per element of `group` (1 | 2) in `enc`
uint64_t point_bytes(int group, int32_t enc);
// encoding known, no unknown check bit; *checks comes back with the implied bits set
bool point_args_ok(int32_t enc, int32_t* checks);

// n elements at d_in (HBM, 4-byte aligned) -> d_out (NULL, or n elements: affine WIRE form, or the resident form when
// `out_resident`), d_status (NULL or n bytes).  Runs on ctx->stream and waits for it.  *first_bad: smallest failing
// index (UINT64_MAX when none), *bad_status: its status byte.  ZKMI_OK also when elements fail: the caller decides.
int32_t points_read(zkmi_ctx* ctx, int group, const void* d_in, uint64_t n, int32_t enc, int32_t checks, void* d_out,
                    bool out_resident, void* d_status, uint64_t* first_bad, uint32_t* bad_status);

// the same for n elements in HOST memory, uploaded through the context's staging buffer in bounded chunks; d_out is the
// resident form (n elements in HBM).  Stops at the first chunk with a failing element.
int32_t points_read_host(zkmi_ctx* ctx, int group, const uint8_t* host, uint64_t n, int32_t enc, int32_t checks,
                         void* d_out_resident, uint64_t* first_bad, uint32_t* bad_status);

const char* point_status_name(uint32_t st);

// groth16.hip: a proving key for `r` from its five single elements (WIRE form; the caller has validated what it wants
// validated) and its five queries (a, b_g1, b_g2, h, l) in HOST memory in `enc`, every query point read by the kernels
// above under `checks`.  A refused point: ZKMI_ERR_NON_CANONICAL, where[0] = query, where[1] = index, no key.
int32_t pk_load_encoded(zkmi_ctx* ctx, const zkmi_r1cs* r, const uint8_t alpha_g1[96], const uint8_t beta_g1[96],
                        const uint8_t beta_g2[192], const uint8_t delta_g1[96], const uint8_t delta_g2[192],
                        const uint8_t* const queries[5], int32_t enc, int32_t checks, zkmi_pk** out_pk, uint64_t where[2]);

}  // namespace zkmi
