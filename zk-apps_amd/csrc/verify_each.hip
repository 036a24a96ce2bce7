// zkmi — every Groth16 proof of one key checked by its own equation on the device (zkmi_groth16_verify_each):
//
//   e(A_i, B_i) * e(X_i, -gamma) * e(C_i, -delta) * e(-alpha, beta) = 1,   X_i = ic_0 + sum_j pub_ij ic_j.
//
// No weights, no error term, no bisection: the launches are the same whatever the verdicts.  What runs where:
//   device  upload once, strided copies split A | B | C, k_points_read decompresses and subgroup-checks each array (the
//           acceptance rules of the host verifier by construction), k_public_sum_g1 forms X_i, ONE k_miller launch over
//           3 n + 1 pairs, k_final_exp multiplies each proof's three values with the shared fourth, raises the product to
//           (p^12 - 1)/r and writes one status byte
//   host    publics < r, -alpha, -gamma, -delta; the window table of the ic_j (n_pub - 1 times 64 x 15 additions) once
//           per key, kept in the zkmi_vk and uploaded at every call
// Pair layout (planar, so that the point readers write straight into it):
//   g1 = [A_0..A_{n-1} | X_0.. | C_0.. | -alpha],  g2 = [B_0.. | -gamma x n | -delta x n | beta].
// A malformed proof keeps its status 1-4; its lanes compute on values nobody reads.
#include <string.h>
#include <chrono>
#include <vector>
#include "pairing_dev.hpp"
#include "verify.hpp"
#include "points.hpp"
#include "field28.hpp"

namespace zkmi {

namespace {

constexpr uint32_t PS_WINDOWS = 64, PS_DIGITS = 15;  // 4-bit windows of a 256-bit scalar, digits 1..15

// X_i = ic_0 + sum_j pub_ij ic_j, one lane per proof: tab[(j * 64 + w) * 15 + d - 1] = d 16^w ic_{j+1} (affine), so a
// public input costs at most 64 mixed additions and no doubling.  The sums are arbitrary: a key may hold equal or
// opposite ic_j (or O), publics may cancel each other, so every addition is XYZZ::madd, complete by case analysis
// (infinite accumulator, equal points -> doubling, opposite points -> O, infinite table entry); a cheaper incomplete
// addition would be wrong for such keys.  Output: affine WIRE form, all zero = infinity.
__global__ __launch_bounds__(64) void k_public_sum_g1(const Affine<Fq28>* __restrict__ tab, const uint32_t* __restrict__ ic0,
                                                      const uint32_t* __restrict__ pub, uint32_t np1, uint64_t n,
                                                      uint32_t* __restrict__ out) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = gid < n;
  const uint64_t idx = live ? gid : n - 1;  // n >= 1 (host)
  uint32_t xw[12], yw[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    xw[i] = ic0[i];
    yw[i] = ic0[12 + i];
  }
  XYZZ<Fq28> acc = XYZZ<Fq28>::from_affine({Fq28::from_canonical(xw), Fq28::from_canonical(yw)});
#pragma unroll 1
  for (uint32_t j = 0; j < np1; j++) {
    const uint32_t* k = pub + (idx * np1 + j) * 8;
#pragma unroll 1
    for (uint32_t w = 0; w < PS_WINDOWS; w++) {
      const uint32_t d = (k[w >> 3] >> ((w & 7u) * 4u)) & 15u;
      if (d) acc.madd(tab[((uint64_t)j * PS_WINDOWS + w) * PS_DIGITS + d - 1]);
    }
  }
  const Affine<Fq28> r = acc.to_affine();
  r.x.to_canonical(xw);
  r.y.to_canonical(yw);
  if (live) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
      out[gid * 24 + i] = xw[i];
      out[gid * 24 + 12 + i] = yw[i];
    }
  }
}

// g2[n + i] = two[0], g2[2 n + i] = two[1] for i < n (192-byte elements as 48 words)
__global__ __launch_bounds__(256) void k_replicate_g2(const uint32_t* __restrict__ two, uint64_t n, uint32_t* __restrict__ g2) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * n * 48) return;
  const uint64_t el = t / 48;
  g2[n * 48 + t] = two[(el >= n ? 48 : 0) + t % 48];
}

// the window table of ic_1 .. ic_{n_pub-1} in the device limb form
void public_sum_table(const zkmi_vk* vk, std::vector<Affine<Fq28>>* out) {
  const uint32_t np1 = vk->n_pub - 1;
  const size_t per = (size_t)PS_WINDOWS * PS_DIGITS;
  std::vector<G1XYZZ> t(np1 * per);
  for (uint32_t j = 0; j < np1; j++) {
    G1XYZZ base = G1XYZZ::from_affine(vk->ic[j + 1]);
    for (uint32_t w = 0; w < PS_WINDOWS; w++) {
      G1XYZZ* row = t.data() + j * per + (size_t)w * PS_DIGITS;
      row[0] = base;
      for (uint32_t d = 1; d < PS_DIGITS; d++) {
        row[d] = row[d - 1];
        row[d].add(base);
      }
      base = row[PS_DIGITS - 1];
      base.add(row[0]);  // 16 * (16^w ic_j)
    }
  }
  std::vector<G1Affine> a(t.size());
  if (!t.empty()) batch_to_affine(t.data(), t.size(), a.data());
  out->resize(a.size());
  for (size_t i = 0; i < a.size(); i++) (*out)[i] = {fq28_from_fq(a[i].x), fq28_from_fq(a[i].y)};
}

#ifdef ZKMI_TESTING
float g_each_ms[3];  // the last call: k_public_sum_g1, k_final_exp by HIP events, the table build by the host clock (0: kept)
#endif

}  // namespace

hipError_t public_sums_dev(zkmi_ctx* ctx, const void* d_tab, const void* d_ic0, const void* d_pub, uint32_t np1, uint64_t n,
                           void* d_out) {
  hipLaunchKernelGGL(k_public_sum_g1, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream,
                     static_cast<const Affine<Fq28>*>(d_tab), static_cast<const uint32_t*>(d_ic0),
                     static_cast<const uint32_t*>(d_pub), np1, n, static_cast<uint32_t*>(d_out));
  return hipGetLastError();
}

}  // namespace zkmi

extern "C" int32_t zkmi_groth16_verify_each(zkmi_ctx* ctx, const zkmi_vk* vk, uint64_t n, const uint8_t* publics,
                                            const uint8_t* proofs, uint8_t* out_status, uint64_t* out_first_bad) {
  using namespace zkmi;
  ZK_ENTER(ctx);
  if (!vk || !out_status || n > (1ull << 24)) return ZKMI_ERR_BAD_ARG;
  if (out_first_bad) *out_first_bad = UINT64_MAX;
  if (n == 0) return ZKMI_OK;
  const uint32_t np1 = vk->n_pub - 1;
  if (!proofs || (np1 && !publics)) return ZKMI_ERR_BAD_ARG;

#ifdef ZKMI_TESTING
  g_each_ms[2] = 0;
#endif
  std::call_once(vk->sum_tab_once, [vk] {
#ifdef ZKMI_TESTING
    const auto t0 = std::chrono::steady_clock::now();
#endif
    public_sum_table(vk, &vk->sum_tab);
#ifdef ZKMI_TESTING
    g_each_ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
#endif
  });
  const std::vector<Affine<Fq28>>& tab = vk->sum_tab;
  uint8_t g1tail[96], g2tail[192], ic0[96], neg2[2 * 192];
  g1_to_wire(vk->alpha.neg(), g1tail);
  g2_to_wire(vk->beta, g2tail);
  g1_to_wire(vk->ic[0], ic0);
  g2_to_wire(vk->gamma.neg(), neg2);
  g2_to_wire(vk->delta.neg(), neg2 + 192);

  // one workspace: [proofs | A, C compressed | B compressed | g1 (3 n + 1) | g2 (3 n + 1) | Miller values (3 n + 1) |
  //                 window table | publics | ic_0 | -gamma, -delta | point statuses (3 n) | equation statuses (n)]
  const uint64_t np = 3 * n + 1, tab_bytes = tab.size() * sizeof(Affine<Fq28>);
  auto up = [](uint64_t v) { return (v + 255) & ~255ull; };
  const uint64_t o_proofs = 0, o_ac = o_proofs + up(192 * n), o_cc = o_ac + up(48 * n), o_bc = o_cc + up(48 * n),
                 o_g1 = o_bc + up(96 * n), o_g2 = o_g1 + up(96 * np), o_m = o_g2 + up(192 * np),
                 o_tab = o_m + up(MILLER_BYTES * np), o_pub = o_tab + up(tab_bytes), o_ic0 = o_pub + up(32ull * np1 * n),
                 o_neg = o_ic0 + up(96), o_st = o_neg + up(384), o_eq = o_st + up(3 * n), total = o_eq + up(n);
  ZK_HIP(ctx, ctx->staging(total));
  uint8_t* d = static_cast<uint8_t*>(ctx->d_tmp);
  hipStream_t st = ctx->stream;
  std::vector<uint8_t> pst(3 * n), eq(n);
#ifdef ZKMI_TESTING
  hipEvent_t ev[4] = {};
  struct Events {
    hipEvent_t* e;
    ~Events() {
      for (int i = 0; i < 4; i++)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  } events{ev};
#endif
  // declared after every host buffer and event the stream touches: destroyed first, so every return below, HIP error
  // paths included, waits for the stream before any of them goes away
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{st};

  ZK_HIP(ctx, hipMemcpyAsync(d + o_proofs, proofs, 192 * n, hipMemcpyHostToDevice, st));
  ZK_HIP(ctx, hipMemcpy2DAsync(d + o_ac, 48, d + o_proofs, 192, 48, n, hipMemcpyDeviceToDevice, st));
  ZK_HIP(ctx, hipMemcpy2DAsync(d + o_bc, 96, d + o_proofs + 48, 192, 96, n, hipMemcpyDeviceToDevice, st));
  ZK_HIP(ctx, hipMemcpy2DAsync(d + o_cc, 48, d + o_proofs + 144, 192, 48, n, hipMemcpyDeviceToDevice, st));
  if (tab_bytes) {
    ZK_HIP(ctx, hipMemcpyAsync(d + o_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d + o_pub, publics, 32ull * np1 * n, hipMemcpyHostToDevice, st));
  }
  ZK_HIP(ctx, hipMemcpyAsync(d + o_ic0, ic0, sizeof(ic0), hipMemcpyHostToDevice, st));
  ZK_HIP(ctx, hipMemcpyAsync(d + o_neg, neg2, sizeof(neg2), hipMemcpyHostToDevice, st));
  ZK_HIP(ctx, hipMemcpyAsync(d + o_g1 + 96 * 3 * n, g1tail, sizeof(g1tail), hipMemcpyHostToDevice, st));
  ZK_HIP(ctx, hipMemcpyAsync(d + o_g2 + 192 * 3 * n, g2tail, sizeof(g2tail), hipMemcpyHostToDevice, st));

  const int32_t enc = ZKMI_ENC_ZCASH_COMPRESSED, chk = ZKMI_CHECK_SUBGROUP;
  int32_t rc;
  if ((rc = points_read(ctx, 1, d + o_ac, n, enc, chk, d + o_g1, false, d + o_st, nullptr, nullptr)) != ZKMI_OK) return rc;
  if ((rc = points_read(ctx, 2, d + o_bc, n, enc, chk, d + o_g2, false, d + o_st + n, nullptr, nullptr)) != ZKMI_OK) return rc;
  if ((rc = points_read(ctx, 1, d + o_cc, n, enc, chk, d + o_g1 + 96 * 2 * n, false, d + o_st + 2 * n, nullptr, nullptr)) != ZKMI_OK)
    return rc;
  ZK_HIP(ctx, hipMemcpyAsync(pst.data(), d + o_st, 3 * n, hipMemcpyDeviceToHost, st));

#ifdef ZKMI_TESTING
  for (hipEvent_t& e : ev) ZK_HIP(ctx, hipEventCreate(&e));
  ZK_HIP(ctx, hipEventRecord(ev[0], st));
#endif
  ZK_HIP(ctx, public_sums_dev(ctx, d + o_tab, d + o_ic0, d + o_pub, np1, n, d + o_g1 + 96 * n));
#ifdef ZKMI_TESTING
  ZK_HIP(ctx, hipEventRecord(ev[1], st));
#endif
  hipLaunchKernelGGL(k_replicate_g2, dim3((unsigned)((2 * n * 48 + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint32_t*>(d + o_neg), n, reinterpret_cast<uint32_t*>(d + o_g2));
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, miller_values_dev(ctx, d + o_g1, d + o_g2, np, d + o_m));
#ifdef ZKMI_TESTING
  ZK_HIP(ctx, hipEventRecord(ev[2], st));
#endif
  // proof i: values i, n + i, 2 n + i and the shared one at 3 n
  ZK_HIP(ctx, final_exp_dev(ctx, d + o_m, n, 3, 1, n, d + o_m + MILLER_BYTES * 3 * n, nullptr, d + o_eq));
#ifdef ZKMI_TESTING
  ZK_HIP(ctx, hipEventRecord(ev[3], st));
#endif
  ZK_HIP(ctx, hipMemcpyAsync(eq.data(), d + o_eq, n, hipMemcpyDeviceToHost, st));
  ZK_HIP(ctx, hipStreamSynchronize(st));
#ifdef ZKMI_TESTING
  ZK_HIP(ctx, hipEventElapsedTime(&g_each_ms[0], ev[0], ev[1]));
  ZK_HIP(ctx, hipEventElapsedTime(&g_each_ms[1], ev[2], ev[3]));
#endif

  bool malformed = false, failed = false;
  for (uint64_t i = 0; i < n; i++) {
    uint8_t s = pst[i] ? pst[i] : pst[n + i] ? pst[n + i] : pst[2 * n + i];  // A, B, C: ZKMI_PT_* = ZKMI_PROOF_*
    for (uint32_t j = 0; j < np1 && !s; j++)
      if (!fr_is_canonical(publics + 32 * (i * np1 + j))) s = ZKMI_PROOF_BAD_PUBLIC;
    if (s) malformed = true;
    else if ((s = eq[i]) != ZKMI_PROOF_OK) failed = true;
    out_status[i] = s;
    if (s && out_first_bad && *out_first_bad == UINT64_MAX) *out_first_bad = i;
  }
  if (malformed) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "verify each: a malformed proof");
  return failed ? ctx->fail(ZKMI_ERR_VERIFICATION, "verify each: a pairing equation does not hold") : ZKMI_OK;
}

#ifdef ZKMI_TESTING  // test scaffolding: libzkmi_exp.so only (include/zkmi_testing.h)
extern "C" int32_t zkmi_verify_each_kernel_ms(float out_ms[3]) {
  if (!out_ms) return ZKMI_ERR_BAD_ARG;
  for (int k = 0; k < 3; k++) out_ms[k] = zkmi::g_each_ms[k];
  return ZKMI_OK;
}
#endif  // ZKMI_TESTING
