// zkmi — prod_i e(P_i, Q_i) with the Miller loops and their product on the device and ONE final exponentiation on the
// host (zkmi_pairing_product_dev).  pairing.hip is the specification: the same M-twist line embedding
//   -yP*xi + (yT - l*xT) v w + (l*xP) v^2 w,
// but T stays Jacobian, so a step has no inversion and every line comes out multiplied by a factor in Fq2 (2 Y Z^3 for a
// tangent, Z3 for a chord).  The final exponentiation kills such factors: device Miller values equal the host's only
// after it.
//
// Shape: one pair (P, Q) per LANE PAIR.  Every Fq2 value is an Fq2P (field28.hpp): its two components live in two
// adjacent lanes, so f in Fq12 costs a lane 6 x 14 registers and T 3 x 14.  The Fq2 products are out-of-line routines
// shared by all call sites: the loop body of ~45 products stays a few thousand instructions instead of ~40 000.
// The 63 steps of |x| = 0xd201000000010000 and its 5 additions run as ONE loop of 68 rounds whose kind (tangent after
// squaring f / chord) is wave-uniform; for Q in the r-order subgroup T = [k]Q with 1 < k < |x| < r never meets +-Q or
// O, so neither step has an exceptional case.  A lane pair whose inputs are garbage or infinite keeps computing on
// values nobody reads (an infinite member writes 1 at the end); lane pairs past the end redo the last pair and write
// nothing.
//
// Magnitudes: nothing between two products is reduced modulo p; tower_dev.hpp states the one bound everything rests on
// (sum over a reduction's partial products of |a||b| < 1260 p^2) and what the tower reaches (operands up to 22.5 p, sums up
// to 202.5 p^2, shrink() once per round on every coefficient of f and on x, y of T).
//
// The final exponentiation (final_exp_chain, k_final_exp: zkmi_pairing_batch_dev, zkmi_groth16_verify_each) is written over
// the same tower template; see the comment above final_exp_chain.
#include "pairing_dev.hpp"
#include "tower_dev.hpp"

namespace zkmi {

namespace {

// one Miller value: coefficient k of the tower basis at words 24 k (c0) and 24 k + 12 (c1)
PD_INL E12P e12_load(const uint32_t* __restrict__ m) {
  const uint32_t* q = m + (Fq2P::odd() ? 12 : 0);
  bool z;
  E12P f;
  f.c0.a0 = {limbs_from_words(q, &z)};
  f.c0.a1 = {limbs_from_words(q + 24, &z)};
  f.c0.a2 = {limbs_from_words(q + 48, &z)};
  f.c1.a0 = {limbs_from_words(q + 72, &z)};
  f.c1.a1 = {limbs_from_words(q + 96, &z)};
  f.c1.a2 = {limbs_from_words(q + 120, &z)};
  return f;
}
PD_INL void e12_store(const E12P& f, uint32_t* __restrict__ m, bool write) {
  uint32_t* q = m + (Fq2P::odd() ? 12 : 0);
  limbs_to_words(f.c0.a0.v, q, write);
  limbs_to_words(f.c0.a1.v, q + 24, write);
  limbs_to_words(f.c0.a2.v, q + 48, write);
  limbs_to_words(f.c1.a0.v, q + 72, write);
  limbs_to_words(f.c1.a1.v, q + 96, write);
  limbs_to_words(f.c1.a2.v, q + 120, write);
}
PD_INL E12P e12_select(bool c, const E12P& a, const E12P& b) {
  return {{{E2::sel(c, a.c0.a0.v, b.c0.a0.v)}, {E2::sel(c, a.c0.a1.v, b.c0.a1.v)}, {E2::sel(c, a.c0.a2.v, b.c0.a2.v)}},
          {{E2::sel(c, a.c1.a0.v, b.c1.a0.v)}, {E2::sel(c, a.c1.a1.v, b.c1.a1.v)}, {E2::sel(c, a.c1.a2.v, b.c1.a2.v)}}};
}

// g1: n x 24 words (x | y), g2: n x 48 words (x.c0 x.c1 y.c0 y.c1), out: n x 144 words
__global__ __launch_bounds__(64, 1) void k_miller(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2,
                                                  uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t pair = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = pair < n;
  const uint64_t idx = live ? pair : n - 1;  // n >= 1 (host); tail lane pairs shadow the last pair
  const uint32_t comp = threadIdx.x & 1u;

  bool zx, zy;
  const Fq28 xp = limbs_from_words(g1 + idx * 24, &zx);
  const Fq28 nyp = limbs_from_words(g1 + idx * 24 + 12, &zy).neg();
  bool inf = zx && zy;
  const E2 xq = {limbs_from_words(g2 + idx * 48 + 12 * comp, &zx)};
  const E2 yq = {limbs_from_words(g2 + idx * 48 + 24 + 12 * comp, &zy)};
  const int mine = (zx && zy) ? 1 : 0;
  inf = inf || ((mine & __builtin_amdgcn_mov_dpp(mine, 0xB1, 0xF, 0xF, true)) != 0);

  E12P f = miller_rounds(xq, yq, xp, nyp);
  f = e12_select(inf, e12_one<E2>(), f);
  e12_store(f, out + idx * 144, live);
}

// partial product j < np: prod of m[i], i = j, j + np, j + 2 np, ... < n   (np <= n)
__global__ __launch_bounds__(64, 1) void k_miller_product(const uint32_t* __restrict__ m, uint64_t n, uint32_t np,
                                                          uint32_t* __restrict__ out) {
  const uint32_t gj = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = gj < np;
  const uint32_t j = live ? gj : np - 1;
  E12P acc = e12_load(m + (uint64_t)j * 144);
  const uint64_t rounds = (n + np - 1) / np;
#pragma unroll 1
  for (uint64_t k = 1; k < rounds; k++) {
    const uint64_t i = j + k * np;
    const bool have = i < n;
    const E12P prod = e12_mul(acc, e12_load(m + (have ? i : (uint64_t)j) * 144));
    acc = e12_select(have, prod, acc);
  }
  e12_store(acc, out + (uint64_t)j * 144, live);
}

// One group of Miller values per lane pair: group i < n is the product of the g values at index i gs + k ms (k < g) and,
// when `shared` is given, of the one value there; conjugated once (x < 0), raised to (p^12 - 1)/r.  out_gt: n x 144 words
// (the bytes of zkmi_pairing); otherwise out_status: one byte per group, 0 when the result is 1, else ZKMI_PROOF_PAIRING.
// Tail lane pairs shadow the last group and write nothing.
__global__ __launch_bounds__(64, 1) void k_final_exp(const uint32_t* __restrict__ m, uint64_t n, uint32_t g, uint64_t gs,
                                                     uint64_t ms, const uint32_t* __restrict__ shared,
                                                     uint32_t* __restrict__ out_gt, uint8_t* __restrict__ out_status) {
  const uint64_t pair = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = pair < n;
  const uint64_t idx = live ? pair : n - 1;  // n >= 1 (host)
  E12P f = e12_load(m + idx * gs * 144);
  const uint32_t members = g + (shared ? 1u : 0u);
#pragma unroll 1
  for (uint32_t k = 1; k < members; k++)
    f = e12_mul_o(f, e12_load(k < g ? m + (idx * gs + k * ms) * 144 : shared));
  f = final_exp_chain(e12_conj(f));
  if (out_gt) {
    e12_store(f, out_gt + idx * 144, live);
  } else {
    const bool both = e12_is_one(f);
    if (live && !Fq2P::odd()) out_status[idx] = both ? (uint8_t)ZKMI_PROOF_OK : (uint8_t)ZKMI_PROOF_PAIRING;
  }
}

bool fq12_from_words(const uint8_t* b, Fq12* out) {
  Fq2* a[6] = {&out->c0.a0, &out->c0.a1, &out->c0.a2, &out->c1.a0, &out->c1.a1, &out->c1.a2};
  bool ok = true;
  for (int k = 0; k < 6; k++) {
    ok = fq_from_wire(b + 96 * k, &a[k]->c0) && ok;
    ok = fq_from_wire(b + 96 * k + 48, &a[k]->c1) && ok;
  }
  return ok;
}

}  // namespace

hipError_t miller_values_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, void* d_miller) {
  const dim3 grid((unsigned)((2 * n + 63) / 64)), block(64);
  hipLaunchKernelGGL(k_miller, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(d_g1),
                     static_cast<const uint32_t*>(d_g2), n, static_cast<uint32_t*>(d_miller));
  return hipGetLastError();
}

int32_t miller_product_dev(zkmi_ctx* ctx, const void* d_miller, uint64_t n, void* d_partials, Fq12* out) {
  const uint32_t np = (uint32_t)((n + 1) / 2 < MILLER_PARTIALS ? (n + 1) / 2 : MILLER_PARTIALS);
  const dim3 grid((2 * np + 63) / 64), block(64);
  hipLaunchKernelGGL(k_miller_product, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(d_miller), n, np,
                     static_cast<uint32_t*>(d_partials));
  hipError_t e = hipGetLastError();
  std::vector<uint8_t> host(np * MILLER_BYTES);
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_partials, host.size(), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return ctx->hip_fail(e, "Miller product");
  Fq12 acc = Fq12::one();
  for (uint32_t j = 0; j < np; j++) {
    Fq12 v;
    if (!fq12_from_words(host.data() + j * MILLER_BYTES, &v)) return ctx->fail(ZKMI_ERR_HIP, "Miller product: a coefficient >= p came back");
    acc = acc * v;
  }
  *out = acc;
  return ZKMI_OK;
}

hipError_t final_exp_dev(zkmi_ctx* ctx, const void* d_miller, uint64_t n, uint32_t g, uint64_t group_stride,
                         uint64_t member_stride, const void* d_shared, void* d_out_gt, void* d_out_status) {
  const dim3 grid((unsigned)((2 * n + 63) / 64)), block(64);
  hipLaunchKernelGGL(k_final_exp, grid, block, 0, ctx->stream, static_cast<const uint32_t*>(d_miller), n, g, group_stride,
                     member_stride, static_cast<const uint32_t*>(d_shared), static_cast<uint32_t*>(d_out_gt),
                     static_cast<uint8_t*>(d_out_status));
  return hipGetLastError();
}

}  // namespace zkmi

extern "C" int32_t zkmi_pairing_batch_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, void* d_out_gt) {
  using namespace zkmi;
  ZK_ENTER(ctx);
  if (n >= (1ull << 30)) return ZKMI_ERR_BAD_ARG;
  if (n == 0) return ZKMI_OK;
  if (!d_g1 || !d_g2 || !d_out_gt || (reinterpret_cast<uintptr_t>(d_g1) & 3u) || (reinterpret_cast<uintptr_t>(d_g2) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_out_gt) & 3u))
    return ZKMI_ERR_BAD_ARG;
  ZK_HIP(ctx, ctx->staging(n * MILLER_BYTES));
  hipError_t e = miller_values_dev(ctx, d_g1, d_g2, n, ctx->d_tmp);
  if (e == hipSuccess) e = final_exp_dev(ctx, ctx->d_tmp, n, 1, 1, 0, nullptr, d_out_gt, nullptr);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // also on an error path: nothing may still use the staging buffer
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? ZKMI_OK : ctx->hip_fail(e, "pairing batch");
}

extern "C" int32_t zkmi_pairing_product_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, uint8_t out_fq12[576]) {
  using namespace zkmi;
  ZK_ENTER(ctx);
  if (!out_fq12 || n >= (1ull << 30)) return ZKMI_ERR_BAD_ARG;
  if (n == 0) {
    fq12_to_wire(Fq12::one(), out_fq12);
    return ZKMI_OK;
  }
  if (!d_g1 || !d_g2 || (reinterpret_cast<uintptr_t>(d_g1) & 3u) || (reinterpret_cast<uintptr_t>(d_g2) & 3u)) return ZKMI_ERR_BAD_ARG;
  ZK_HIP(ctx, ctx->staging((n + MILLER_PARTIALS) * MILLER_BYTES));
  uint8_t* d_miller = static_cast<uint8_t*>(ctx->d_tmp);
  const hipError_t e = miller_values_dev(ctx, d_g1, d_g2, n, d_miller);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return ctx->hip_fail(e, "Miller loops");
  }
  Fq12 f;
  const int32_t rc = miller_product_dev(ctx, d_miller, n, d_miller + n * MILLER_BYTES, &f);
  if (rc != ZKMI_OK) return rc;
  fq12_to_wire(final_exponentiation(f.conj()), out_fq12);  // x < 0: one conjugation for the whole product
  return ZKMI_OK;
}

#ifdef ZKMI_TESTING  // test scaffolding: libzkmi_exp.so only (include/zkmi_testing.h)
#include "tower_selftest.hpp"
namespace zkmi {
namespace {
// the launch of the product's kernels: 64 lanes per block, one tuple per lane pair, tail pairs shadow the last tuple
template <int OP>
__global__ __launch_bounds__(64, 1) void k_tower_op(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                    uint8_t* __restrict__ flag, uint32_t n) {
  const uint32_t pair = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = pair < n;
  const uint32_t idx = live ? pair : n - 1;  // n >= 1 (host)
  const PairIO io = {in + (size_t)idx * TOP_IN[OP] * TNL, out + (size_t)idx * TOP_OUT[OP] * TNL, flag + idx, threadIdx.x & 1u, live};
  tower_op_body<OP>(io);
}

template <int OP>
int32_t tower_run(zkmi_ctx* ctx, uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  constexpr bool FLAG = OP == TOP_IS_ONE;
  if ((TOP_OUT[OP] && !out) || (FLAG && !out_flag)) return ZKMI_ERR_BAD_ARG;
  if (!ctx) {
    tower_run_host<OP>(n, in, out, out_flag);
    return ZKMI_OK;
  }
  ZK_ENTER(ctx);
  const size_t in_bytes = sizeof(int32_t) * TNL * TOP_IN[OP] * (size_t)n, out_bytes = sizeof(int32_t) * TNL * TOP_OUT[OP] * (size_t)n;
  int32_t *d_in = nullptr, *d_out = nullptr;
  uint8_t* d_flag = nullptr;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes ? out_bytes : 4);
  if (e == hipSuccess) e = hipMalloc(&d_flag, n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_tower_op<OP>, dim3((2 * n + 63) / 64), dim3(64), 0, ctx->stream, d_in, d_out, d_flag, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess && out_bytes) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && FLAG) e = hipMemcpyAsync(out_flag, d_flag, n, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_flag);
  return e == hipSuccess ? ZKMI_OK : ctx->hip_fail(e, "tower ops self-test");
}
}  // namespace
}  // namespace zkmi

extern "C" int32_t zkmi_selftest_tower_ops(zkmi_ctx* ctx, int32_t op, uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  using namespace zkmi;
  if (!in || n == 0 || n > (1u << 16)) return ZKMI_ERR_BAD_ARG;
  switch (op) {
#define ZK_TOP_CASE(OP) \
  case OP: return tower_run<OP>(ctx, n, in, out, out_flag);
    ZK_TOP_CASE(TOP_SHRINK) ZK_TOP_CASE(TOP_E2_MUL_XI) ZK_TOP_CASE(TOP_E2_CONJ) ZK_TOP_CASE(TOP_E2_INV) ZK_TOP_CASE(TOP_E6_MUL)
    ZK_TOP_CASE(TOP_E12_SQR) ZK_TOP_CASE(TOP_E12_MUL) ZK_TOP_CASE(TOP_E12_MUL_LINE) ZK_TOP_CASE(TOP_E12_CONJ)
    ZK_TOP_CASE(TOP_E12_FROB_P) ZK_TOP_CASE(TOP_E12_FROB_P2) ZK_TOP_CASE(TOP_E6_INV) ZK_TOP_CASE(TOP_E12_INV)
    ZK_TOP_CASE(TOP_STEP_TANGENT) ZK_TOP_CASE(TOP_STEP_CHORD) ZK_TOP_CASE(TOP_MILLER_ROUNDS) ZK_TOP_CASE(TOP_FINAL_EXP_CHAIN)
    ZK_TOP_CASE(TOP_WORDS_ROUND_TRIP) ZK_TOP_CASE(TOP_IS_ONE)
#undef ZK_TOP_CASE
    default: return ZKMI_ERR_BAD_ARG;
  }
}

extern "C" int32_t zkmi_selftest_tower_bounds(double* out_sites, uint32_t n_sites, double* out_classes, uint32_t n_classes) {
  return zkmi::tower_bounds_run(out_sites, n_sites, out_classes, n_classes);
}
extern "C" int32_t zkmi_selftest_miller_formulas(const uint8_t g1_affine[96], const uint8_t g2_affine[192], uint8_t out_fq12[576]) {
  using namespace zkmi;
  if (!g1_affine || !g2_affine || !out_fq12) return ZKMI_ERR_BAD_ARG;
  G1Affine p;
  G2Affine q;
  if (!g1_from_wire(g1_affine, &p, true) || !g2_from_wire(g2_affine, &q, true)) return ZKMI_ERR_NON_CANONICAL;
  Fq12 f = Fq12::one();
  if (!p.is_inf() && !q.is_inf()) {
    const E12<Fq2> m = miller_rounds<Fq2, Fq>(q.x, q.y, p.x, p.y.neg());
    f = {{m.c0.a0, m.c0.a1, m.c0.a2}, {m.c1.a0, m.c1.a1, m.c1.a2}};
  }
  fq12_to_wire(final_exponentiation(f.conj()), out_fq12);
  return ZKMI_OK;
}
extern "C" int32_t zkmi_selftest_final_exp_formulas(const uint8_t in_fq12[576], uint8_t out_chain[576], uint8_t out_plain[576]) {
  using namespace zkmi;
  if (!in_fq12 || !out_chain || !out_plain) return ZKMI_ERR_BAD_ARG;
  Fq12 f;
  if (!fq12_from_words(in_fq12, &f)) return ZKMI_ERR_NON_CANONICAL;
  if (f.c0 == Fq6::zero() && f.c1 == Fq6::zero()) return ZKMI_ERR_BAD_ARG;
  const E12<Fq2> c = final_exp_chain<Fq2>({{f.c0.a0, f.c0.a1, f.c0.a2}, {f.c1.a0, f.c1.a1, f.c1.a2}});
  fq12_to_wire({{c.c0.a0, c.c0.a1, c.c0.a2}, {c.c1.a0, c.c1.a1, c.c1.a2}}, out_chain);
  fq12_to_wire(final_exponentiation(f), out_plain);
  return ZKMI_OK;
}
#endif  // ZKMI_TESTING
