// zkmi — one operation of the limb arithmetic (field28.hpp) on caller-chosen RAW limb arrays, on the device (one lane per
// tuple; a lane pair per tuple for the Fq2P forms) or, with the same templated body, on the host; and the prover's
// decimation-in-frequency transform alone.  The callers (tests/test_cpu_field28.py, tests/test_gpu_field28.py) place every
// residue in the representations x + k p up to the bounds field28.hpp states and compare with big integers.
// TEST SCAFFOLDING (include/zkmi_testing.h): compiled into libzkmi_exp.so only.
#include "ctx.hpp"
#include "field28.hpp"
#include "ntt.hpp"

#ifdef ZKMI_TESTING
using namespace zkmi;

namespace {
enum Op : int {
  OP_ADD = 0, OP_SUB, OP_NEG, OP_DBL, OP_CARRY, OP_MUL, OP_SQR, OP_LAZY_MUL, OP_MSM, OP_X3, OP_SSUB_MUL, OP_IS_ZERO,
  OP_FROM_CANON, OP_TO_CANON, OP_INV,
  OP_FQ2_MUL = 15, OP_FQ2_SQR, OP_FQ2_MSM, OP_FQ2_X3,
  OP_P_MUL = 19, OP_P_SQR, OP_P_MSM, OP_P_SSUB, OP_P_IS_ZERO,
  OP_MUL_FIPS = 24, OP_SQR_FIPS, OP_FIPS2, OP_FIPS4,
  OP_COUNT
};
// elements per tuple: operands, results (OP_IS_ZERO / OP_P_IS_ZERO write flags instead)
constexpr int N_IN[OP_COUNT] = {2, 2, 1, 1, 2, 2, 1, 4, 6, 3, 3, 1, 1, 1, 1, 4, 2, 8, 6, 4, 2, 8, 4, 2, 2, 1, 4, 8};
constexpr int N_OUT[OP_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 4, 0, 1, 1, 1, 1};

template <class F>
ZK_HD F ld(const int32_t* p) {
  F r;
#pragma unroll
  for (int i = 0; i < F::NL; i++) r.l[i] = p[i];
  return r;
}
template <class F>
ZK_HD void st(int32_t* p, const F& v) {
#pragma unroll
  for (int i = 0; i < F::NL; i++) p[i] = v.l[i];
}

// ops every field has: tuple t of `in` -> tuple t of `out` (or flag[t])
template <class P, int OP>
ZK_HD void op_body(const int32_t* in, int32_t* out, uint8_t* flag, uint32_t t) {
  using F = Fp28<P>;
  constexpr int NL = F::NL;
  const int32_t* a = in + (size_t)t * N_IN[OP] * NL;
  int32_t* o = out + (size_t)t * N_OUT[OP] * NL;
  auto A = [&](int k) { return ld<F>(a + k * NL); };
  if constexpr (OP == OP_ADD) st(o, A(0) + A(1));
  if constexpr (OP == OP_SUB) st(o, A(0) - A(1));
  if constexpr (OP == OP_NEG) st(o, A(0).neg());
  if constexpr (OP == OP_DBL) st(o, A(0).dbl());
  if constexpr (OP == OP_CARRY) {
    F r = A(0).add_lazy(A(1));
    r.carry();
    st(o, r);
  }
  if constexpr (OP == OP_MUL) st(o, A(0) * A(1));
  if constexpr (OP == OP_SQR) st(o, A(0).sqr());
  if constexpr (OP == OP_LAZY_MUL) st(o, A(0).add_lazy(A(1)) * A(2).sub_lazy(A(3)));
  if constexpr (OP == OP_MSM) st(o, f_mul_sub_mul(A(0).sub_lazy(A(1)), A(2).sub_lazy(A(3)), A(4), A(5)));
  if constexpr (OP == OP_X3) st(o, f_x3(A(0), A(1), A(2)));
  if constexpr (OP == OP_SSUB_MUL) {
    st(o, f_signed_sub_lazy(A(0), 0u, A(1)) * A(2));
    st(o + NL, f_signed_sub_lazy(A(0), 0xffffffffu, A(1)) * A(2));
  }
  if constexpr (OP == OP_IS_ZERO) flag[t] = A(0).is_zero() ? 1 : 0;
  if constexpr (OP == OP_FROM_CANON) {
    uint32_t w[P::N32];
#pragma unroll
    for (int i = 0; i < P::N32; i++) w[i] = (uint32_t)a[i];
    st(o, F::from_canonical(w));
  }
  if constexpr (OP == OP_TO_CANON) {
    uint32_t w[P::N32];
    A(0).to_canonical(w);
#pragma unroll
    for (int i = 0; i < NL; i++) o[i] = i < P::N32 ? (int32_t)w[i] : 0;
  }
  if constexpr (OP == OP_INV) st(o, A(0).inv());
  if constexpr (OP == OP_MUL_FIPS) st(o, F::mul_fips(A(0), A(1)));
  if constexpr (OP == OP_SQR_FIPS) st(o, A(0).sqr_fips());
  if constexpr (OP == OP_FIPS2) st(o, F::template fips<true>(A(0), A(1), A(2), A(3)));
  if constexpr (OP == OP_FIPS4) {
    const F v[8] = {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7)};
    const F* x[4] = {&v[0], &v[2], &v[4], &v[6]};
    const F* y[4] = {&v[1], &v[3], &v[5], &v[7]};
    st(o, F::template fipsn<4>(x, y));
  }
}

// Fq2 over the limbs, both components in one lane
template <int OP>
ZK_HD void op_body_fq2(const int32_t* in, int32_t* out, uint32_t t) {
  constexpr int NL = Fq28::NL;
  const int32_t* a = in + (size_t)t * N_IN[OP] * NL;
  int32_t* o = out + (size_t)t * N_OUT[OP] * NL;
  auto A = [&](int k) { return Fq2_28{ld<Fq28>(a + 2 * k * NL), ld<Fq28>(a + (2 * k + 1) * NL)}; };
  Fq2_28 r;
  if constexpr (OP == OP_FQ2_MUL) r = A(0) * A(1);
  if constexpr (OP == OP_FQ2_SQR) r = A(0).sqr();
  if constexpr (OP == OP_FQ2_MSM) r = f_mul_sub_mul(A(0), A(1), A(2), A(3));
  if constexpr (OP == OP_FQ2_X3) r = f_x3(A(0), A(1), A(2));
  st(o, r.c0);
  st(o + NL, r.c1);
}

template <class P, int OP>
__global__ void __launch_bounds__(64) k_op(const int32_t* in, int32_t* out, uint8_t* flag, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  if constexpr (OP >= OP_FQ2_MUL && OP <= OP_FQ2_X3) op_body_fq2<OP>(in, out, t);
  else op_body<P, OP>(in, out, flag, t);
}

// Fq2 split over a lane pair: lane 2 t holds the c0 of tuple t's operands and writes the c0 of its results, lane 2 t + 1 the
// c1.  The guard is per PAIR (both lanes share t), so the partner of an active lane is always active.
template <int OP>
__global__ void __launch_bounds__(64) k_op_pair(const int32_t* in, int32_t* out, uint8_t* flag, uint32_t n) {
  constexpr int NL = Fq28::NL;
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = lane >> 1, comp = lane & 1u;
  if (t >= n) return;
  const int32_t* a = in + (size_t)t * N_IN[OP] * NL;
  int32_t* o = out + (size_t)t * N_OUT[OP] * NL;
  auto A = [&](int k) { return Fq2P{ld<Fq28>(a + (2 * k + comp) * NL)}; };
  if constexpr (OP == OP_P_MUL) st(o + comp * NL, (A(0) * A(1)).v);
  if constexpr (OP == OP_P_SQR) st(o + comp * NL, A(0).sqr().v);
  if constexpr (OP == OP_P_MSM) st(o + comp * NL, f_mul_sub_mul(A(0), A(1), A(2), A(3)).v);
  if constexpr (OP == OP_P_SSUB) {
    st(o + comp * NL, f_signed_sub_lazy(A(0), 0u, A(1)).v);
    st(o + (2 + comp) * NL, f_signed_sub_lazy(A(0), 0xffffffffu, A(1)).v);
  }
  if constexpr (OP == OP_P_IS_ZERO) flag[2 * (size_t)t + comp] = A(0).is_zero() ? 1 : 0;
}

template <class P, int OP>
int32_t run_op(zkmi_ctx* ctx, uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  constexpr int NL = P::NL;
  constexpr bool PAIR = OP >= OP_P_MUL && OP <= OP_P_IS_ZERO;
  constexpr bool FQ2 = OP >= OP_FQ2_MUL && OP <= OP_FQ2_X3;
  constexpr bool FIPS = OP >= OP_MUL_FIPS;
  constexpr uint32_t n_flag = OP == OP_IS_ZERO ? 1 : OP == OP_P_IS_ZERO ? 2 : 0;
  if ((N_OUT[OP] && !out) || (n_flag && !out_flag)) return ZKMI_ERR_BAD_ARG;
  if (!ctx) {
    if constexpr (PAIR) {
      return ZKMI_ERR_BAD_ARG;
    } else {
      for (uint32_t t = 0; t < n; t++) {
        if constexpr (FQ2) op_body_fq2<OP>(in, out, t);
        else op_body<P, OP>(in, out, out_flag, t);
      }
      return ZKMI_OK;
    }
  }
  if constexpr (FIPS) {
    return ZKMI_ERR_BAD_ARG;
  } else {
    ZK_ENTER(ctx);
    const size_t in_bytes = sizeof(int32_t) * NL * N_IN[OP] * (size_t)n, out_bytes = sizeof(int32_t) * NL * N_OUT[OP] * (size_t)n;
    int32_t *d_in = nullptr, *d_out = nullptr;
    uint8_t* d_flag = nullptr;
    hipError_t e = hipMalloc(&d_in, in_bytes);
    if (e == hipSuccess && out_bytes) e = hipMalloc(&d_out, out_bytes);
    if (e == hipSuccess && n_flag) e = hipMalloc(&d_flag, (size_t)n_flag * n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
      if constexpr (PAIR) hipLaunchKernelGGL(k_op_pair<OP>, dim3((2 * n + 63) / 64), dim3(64), 0, ctx->stream, d_in, d_out, d_flag, n);
      else hipLaunchKernelGGL((k_op<P, OP>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_in, d_out, d_flag, n);
      e = hipGetLastError();
    }
    if (e == hipSuccess && out_bytes) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && n_flag) e = hipMemcpyAsync(out_flag, d_flag, (size_t)n_flag * n, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_flag);
    return e == hipSuccess ? ZKMI_OK : ctx->hip_fail(e, "fp28 ops self-test");
  }
}

#define ZK_OP_CASE(OP) \
  case OP: return run_op<P, OP>(ctx, n, in, out, out_flag);
template <class P>
int32_t dispatch(zkmi_ctx* ctx, int32_t op, uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  switch (op) {
    ZK_OP_CASE(OP_ADD) ZK_OP_CASE(OP_SUB) ZK_OP_CASE(OP_NEG) ZK_OP_CASE(OP_DBL) ZK_OP_CASE(OP_CARRY) ZK_OP_CASE(OP_MUL)
    ZK_OP_CASE(OP_SQR) ZK_OP_CASE(OP_LAZY_MUL) ZK_OP_CASE(OP_MSM) ZK_OP_CASE(OP_X3) ZK_OP_CASE(OP_SSUB_MUL)
    ZK_OP_CASE(OP_IS_ZERO) ZK_OP_CASE(OP_FROM_CANON) ZK_OP_CASE(OP_TO_CANON) ZK_OP_CASE(OP_INV)
    ZK_OP_CASE(OP_MUL_FIPS) ZK_OP_CASE(OP_SQR_FIPS) ZK_OP_CASE(OP_FIPS2) ZK_OP_CASE(OP_FIPS4)
    default: break;
  }
  if constexpr (std::is_same<P, Fq28Params>::value) {
    switch (op) {
      ZK_OP_CASE(OP_FQ2_MUL) ZK_OP_CASE(OP_FQ2_SQR) ZK_OP_CASE(OP_FQ2_MSM) ZK_OP_CASE(OP_FQ2_X3)
      ZK_OP_CASE(OP_P_MUL) ZK_OP_CASE(OP_P_SQR) ZK_OP_CASE(OP_P_MSM) ZK_OP_CASE(OP_P_SSUB) ZK_OP_CASE(OP_P_IS_ZERO)
      default: break;
    }
  }
  return ZKMI_ERR_BAD_ARG;
}
#undef ZK_OP_CASE

template <class F, class Dom>
int32_t ntt_dif(zkmi_ctx* ctx, Dom* dom, void* d_data, uint32_t log_n, int32_t post) {
  const uint32_t n = 1u << log_n;
  const uint64_t bytes = (uint64_t)n * sizeof(F);
  if (ctx->d_work_cap < bytes) {
    if (ctx->d_work) (void)hipFree(ctx->d_work);
    ctx->d_work = nullptr;
    ctx->d_work_cap = 0;
    ZK_HIP(ctx, hipMalloc(&ctx->d_work, bytes));
    ctx->d_work_cap = bytes;
  }
  F* work = static_cast<F*>(ctx->d_work);
  ZK_HIP(ctx, ntt_from_canonical(static_cast<const uint32_t*>(d_data), work, n, ctx->stream));
  ZK_HIP(ctx, dom->inverse_to_rev(work, post ? dom->rev_coset_n : nullptr, nullptr, ctx->stream));
  ZK_HIP(ctx, ntt_to_canonical(work, static_cast<uint32_t*>(d_data), n, ctx->stream));
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}
}  // namespace

extern "C" int32_t zkmi_selftest_fp28_ops(zkmi_ctx* ctx, int32_t field, int32_t op, uint32_t n, const int32_t* in, int32_t* out,
                                          uint8_t* out_flag) {
  if (!in || n == 0 || n > (1u << 20) || op < 0 || op >= OP_COUNT) return ZKMI_ERR_BAD_ARG;
  switch (field) {
    case 0: return dispatch<Fq28Params>(ctx, op, n, in, out, out_flag);
    case 1: return dispatch<Fr28Params>(ctx, op, n, in, out, out_flag);
    case 2: return dispatch<BnFq28Params>(ctx, op, n, in, out, out_flag);
    case 3: return dispatch<BnFr28Params>(ctx, op, n, in, out, out_flag);
    default: return ZKMI_ERR_BAD_ARG;
  }
}

extern "C" int32_t zkmi_selftest_ntt_dif_dev(zkmi_ctx* ctx, int32_t field, void* d_data, uint32_t log_n, int32_t post) {
  ZK_ENTER(ctx);
  if (!d_data || log_n == 0 || log_n > 26 || (field != 1 && field != 3)) return ZKMI_ERR_BAD_ARG;
  hipError_t e;
  if (field == 1) {
    NttDomain* dom = ctx->domain((int)log_n, &e);
    if (!dom) return ctx->hip_fail(e, "ntt domain init");
    return ntt_dif<Fr28>(ctx, dom, d_data, log_n, post);
  }
  NttDomainBn* dom = ctx->domain_bn((int)log_n, &e);
  if (!dom) return ctx->hip_fail(e, "bn254 ntt domain init");
  return ntt_dif<BnFr28>(ctx, dom, d_data, log_n, post);
}

// the same transform on RAW limbs, in place: what the witness map hands it (unreduced mat-vec sums) is the caller's to choose
extern "C" int32_t zkmi_selftest_ntt_dif_raw_dev(zkmi_ctx* ctx, int32_t field, void* d_limbs, uint32_t log_n, int32_t post) {
  ZK_ENTER(ctx);
  if (!d_limbs || log_n == 0 || log_n > 26 || (field != 1 && field != 3)) return ZKMI_ERR_BAD_ARG;
  hipError_t e;
  if (field == 1) {
    NttDomain* dom = ctx->domain((int)log_n, &e);
    if (!dom) return ctx->hip_fail(e, "ntt domain init");
    ZK_HIP(ctx, dom->inverse_to_rev(static_cast<Fr28*>(d_limbs), post ? dom->rev_coset_n : nullptr, nullptr, ctx->stream));
  } else {
    NttDomainBn* dom = ctx->domain_bn((int)log_n, &e);
    if (!dom) return ctx->hip_fail(e, "bn254 ntt domain init");
    ZK_HIP(ctx, dom->inverse_to_rev(static_cast<BnFr28*>(d_limbs), post ? dom->rev_coset_n : nullptr, nullptr, ctx->stream));
  }
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}
#endif  // ZKMI_TESTING
