// zkmi — the prepared verifying key shared by the two device verifiers (verify_batch.hip, verify_each.hip).
#pragma once
#include <mutex>
#include <vector>
#include "curve.hpp"
#include "field28.hpp"

// a verifying key validated once (zkmi_vk_prepare, verify_batch.hip)
struct zkmi_vk {
  uint32_t n_pub = 0;
  zkmi::G1Affine alpha;
  zkmi::G2Affine beta, gamma, delta;
  std::vector<zkmi::G1Affine> ic;
  // zkmi_groth16_verify_each: the window table of ic_1.. (verify_each.hip public_sum_table), a function of the key alone,
  // built by the first call that needs it (callers of one key may run on several threads)
  mutable std::once_flag sum_tab_once;
  mutable std::vector<zkmi::Affine<zkmi::Fq28>> sum_tab;
};
