// zkmi — testing hooks of the witness map (include/zkmi_testing.h): the key's mat-vec alone with raw limbs out, the map stage
// by stage with the largest |top limb| of every vector behind each stage, the key's normalisation mask, and the shape rule
// that sets it (witness_bound.hpp).  Included by groth16.hip inside its extern "C" block, after witness_map_dev, so that the
// hooks launch the product's own kernels through the product's own launch_matvec().
// TEST SCAFFOLDING: compiled into libzkmi_exp.so only.
#pragma once

static void wm_matset(const zkmi_pk* pk, MatSet* ms) {
  for (int m = 0; m < 3; m++) {
    ms->rowptr[m] = pk->d_rowptr[m];
    ms->col[m] = pk->d_col[m];
    ms->val[m] = pk->d_val[m];
  }
}

int32_t zkmi_selftest_witness_bound(uint32_t log_n, uint32_t n_pub, uint32_t n_constraints, const uint32_t* rowptr_a,
                                    const uint32_t* rowptr_b, const uint32_t* rowptr_c, uint32_t* out_mask, double out_bound[3]) {
  if (!rowptr_a || !rowptr_b || !rowptr_c || !out_mask || !out_bound || log_n > 26 ||
      (uint64_t)n_constraints + n_pub > (1ull << log_n))
    return ZKMI_ERR_BAD_ARG;
  const uint32_t* rps[3] = {rowptr_a, rowptr_b, rowptr_c};
  const WitnessBound wb = witness_bound(log_n, n_pub, n_constraints, rps);
  *out_mask = wb.normalise;
  for (int m = 0; m < 3; m++) out_bound[m] = 0.5 * (double)wb.half_r[m];
  return ZKMI_OK;
}

int32_t zkmi_selftest_pk_normalise(zkmi_pk* pk, int32_t force_mask, uint32_t* out_mask) {
  if (!pk || force_mask > 7) return ZKMI_ERR_BAD_ARG;
  if (force_mask >= 0) pk->norm_mask = (uint32_t)force_mask;
  if (out_mask) *out_mask = pk->norm_mask;
  return ZKMI_OK;
}

int32_t zkmi_selftest_matvec_dev(zkmi_ctx* ctx, const zkmi_pk* pk, const void* d_z, int32_t form, int32_t* out_limbs) {
  ZK_ENTER(ctx);
  if (!pk || !d_z || !out_limbs || (form != 0 && form != 1)) return ZKMI_ERR_BAD_ARG;
  const uint32_t N = 1u << pk->log_n;
  ZK_HIP(ctx, ntt_from_canonical(static_cast<const uint32_t*>(d_z), pk->d_zm, pk->n_vars, ctx->stream));
  MatSet ms;
  wm_matset(pk, &ms);
  launch_matvec(pk, ms, form == 1, 1, ctx->stream);
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, hipMemcpyAsync(out_limbs, pk->d_a, 3ull * N * sizeof(Fr28), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int32_t zkmi_selftest_witness_map_stages(zkmi_ctx* ctx, const zkmi_pk* pk, const void* d_z, uint32_t out_max[18]) {
  ZK_ENTER(ctx);
  if (!pk || !d_z || !out_max) return ZKMI_ERR_BAD_ARG;
  const uint32_t N = 1u << pk->log_n, nv = pk->n_vars;
  hipStream_t st = ctx->stream;
  hipError_t e;
  NttDomain* dom = ctx->domain((int)pk->log_n, &e);
  if (!dom) return ctx->hip_fail(e, "ntt domain");
  uint32_t* d_max = nullptr;
  ZK_HIP(ctx, hipMalloc(&d_max, 18 * sizeof(uint32_t)));
  auto run = [&]() -> hipError_t {
    hipError_t r;
    if ((r = hipMemsetAsync(d_max, 0, 18 * sizeof(uint32_t), st)) != hipSuccess) return r;
    auto measure = [&](int stage, int slot, const Fr28* v, uint32_t n) {
      const uint32_t blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
      hipLaunchKernelGGL(k_max_top_limb, dim3(blocks), dim3(256), 0, st, v, n, d_max + 3 * stage + slot);
    };
    auto measure_abc = [&](int stage) {
      for (int m = 0; m < 3; m++) measure(stage, m, pk->d_a + (size_t)m * N, N);
    };
    Fr28* const d_b = pk->d_a + (size_t)N;
    Fr28* const d_c = pk->d_a + 2 * (size_t)N;
    // 0: z in limb form (the one vector in all three slots)
    if ((r = ntt_from_canonical(static_cast<const uint32_t*>(d_z), pk->d_zm, nv, st)) != hipSuccess) return r;
    for (int m = 0; m < 3; m++) measure(0, m, pk->d_zm, nv);
    // 1: the mat-vec, in the form witness_map_dev picks for one proof of this key
    MatSet ms;
    wm_matset(pk, &ms);
    launch_matvec(pk, ms, pk->log_n <= 16, 1, st);
    measure_abc(1);
    // 2: the three inverse transforms with their post products; 3: the two forward transforms
    if ((r = dom->inverse_to_rev(pk->d_a, dom->rev_coset_n, nullptr, st, 3)) != hipSuccess) return r;
    measure_abc(2);
    if ((r = dom->forward_from_rev(pk->d_a, st, 2)) != hipSuccess) return r;
    measure_abc(3);
    // 4: k_quotient's outputs (a <- a b, c <- N c): the input of the last transform
    hipLaunchKernelGGL(k_quotient, dim3((N + 63) / 64), dim3(64), 0, st, pk->d_a, d_b, d_c, dom->n_host, N);
    measure_abc(4);
    // 5: the last transform without its epilogue: slot 0 holds the x of (x - sub) * post
    if ((r = dom->inverse_to_rev(pk->d_a, nullptr, nullptr, st, 1)) != hipSuccess) return r;
    measure_abc(5);
    if ((r = hipMemcpyAsync(out_max, d_max, 18 * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return r;
    if ((r = hipStreamSynchronize(st)) != hipSuccess) return r;
    return hipGetLastError();
  };
  e = run();
  (void)hipFree(d_max);
  ZK_HIP(ctx, e);
  return ZKMI_OK;
}
