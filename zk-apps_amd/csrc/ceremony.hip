// zkmi — verifying what a ceremony hands over: the same-ratio checks of a phase-1 transcript
// (zkmi_srs_verify), of a phase-1 contribution (zkmi_srs_verify_contribution: the same checks of the new transcript plus one
// step equation per contributed scalar) and of a phase-2 contribution (zkmi_pk_verify_contribution), and the
// layer below them, the weighted sums of a point array and of the array shifted by one
// (zkmi_g{1,2}_points_adjacent_sums_dev).
//
// A chain P_0, P_1, ... has one ratio tau iff e(P_{i+1}, G2) = e(P_i, [tau]G2) for every i.  The m - 1 equations are taken
// as ONE random linear combination: with lo = sum w_i P_i and hi = sum w_i P_{i+1}, e(hi, G2) = e(lo, [tau]G2).  The weights
//   w(seed, dom, i) = the first 16 bytes of SHA-256(seed[32] | LE32(dom) | LE64(i)), a little-endian 128-bit integer
// are derived on the device, one lane per index (k_rlc_weights: one SHA-256 block per weight), straight into the scalar
// vectors the library's MSM reads.  The sums are two runs of that MSM over the same 28-bit bases.  On the pairing side every
// named equation is its own two-pair product under its own final exponentiation; the equations of a call share one launch
// of Miller loops and one of final exponentiations (pairing_dev.hip).
//
// Nothing waits.  k_rlc_weights and k_points_differ are one-lane-per-item kernels: a range check, then plain vector
// stores to the lane's own entries; no lane reads what another lane of the same launch writes, there are no atomics,
// flags or counters, and every loop has a compile-time trip count.  k_points_differ raises a status word nothing reads
// inside a launch: the host reads it after the last one.  The only ordering is launch order on ctx->stream.
#include <string.h>
#include <sys/random.h>
#include <chrono>
#include <string>
#include <vector>
#include "ceremony.hpp"
#include "pairing_dev.hpp"
#include "points.hpp"
#include "points_ntt.hpp"
#include "sha256.hpp"

namespace zkmi {

namespace {

// the seed as SHA-256 reads it: eight big-endian words
struct RlcSeed {
  uint32_t w[8];
};

RlcSeed rlc_seed(const uint8_t seed[32]) {
  RlcSeed s;
  for (int k = 0; k < 8; k++)
    s.w[k] = ((uint32_t)seed[4 * k] << 24) | ((uint32_t)seed[4 * k + 1] << 16) | ((uint32_t)seed[4 * k + 2] << 8) | seed[4 * k + 3];
  return s;
}

// w(seed, dom, i) as four little-endian words.  The message is 44 bytes: one block, padded with 0x80 and the bit length 352.
__host__ __device__ inline void rlc_weight_body(const RlcSeed& seed, uint32_t dom, uint64_t i, uint32_t out[4]) {
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = seed.w[k];
  w[8] = sha_bswap(dom);
  w[9] = sha_bswap((uint32_t)i);
  w[10] = sha_bswap((uint32_t)(i >> 32));
  w[11] = 0x80000000u;
  w[12] = 0;
  w[13] = 0;
  w[14] = 0;
  w[15] = 352u;
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  sha256_compress(h, w);
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] = sha_bswap(h[k]);
}

constexpr unsigned RLC_BLOCK = 128;

// Scalars are 32 bytes (two uint4): the weight below, zeros above.  Lane i < count writes lo[i] = w_i.  With `hi` given both
// vectors have count + 1 entries: hi[i + 1] = w_i as well, lane 0 adds hi[0] = 0 and the last lane lo[count] = 0 -- every
// entry of both vectors is written by exactly one lane.  Without `hi`, lo has count entries.
__global__ __launch_bounds__(RLC_BLOCK) void k_rlc_weights(RlcSeed seed, uint32_t dom, uint64_t count, uint4* __restrict__ lo,
                                                           uint4* __restrict__ hi) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t w[4];
  rlc_weight_body(seed, dom, i, w);
  const uint4 v = make_uint4(w[0], w[1], w[2], w[3]), z = make_uint4(0, 0, 0, 0);
  lo[2 * i] = v;
  lo[2 * i + 1] = z;
  if (hi) {
    hi[2 * i + 2] = v;
    hi[2 * i + 3] = z;
    if (i == 0) {
      hi[0] = z;
      hi[1] = z;
    }
    if (i + 1 == count) {
      lo[2 * count] = z;
      lo[2 * count + 1] = z;
    }
  }
}

// two arrays of n 32-bit words, one lane per word: a lane that sees a difference stores 1 to *status
__global__ __launch_bounds__(256) void k_points_differ(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t n,
                                                       uint32_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (a[i] != b[i]) *status = 1u;
}

struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(uint64_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Where a call spends its time (testing library only: zkmi_ceremony_phases): the host clock at points where the stream is
// waited for; the product library compiles lap() to nothing and adds no synchronisation.
enum { CP_WEIGHTS, CP_CONVERT, CP_MSM, CP_PAIRING, CP_NPHASE };
#ifdef ZKMI_TESTING
double g_phase_ms[CP_NPHASE];
struct PhaseLog {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(zkmi_ctx* ctx, int k) {
    (void)hipStreamSynchronize(ctx->stream);
    const auto t = std::chrono::steady_clock::now();
    g_phase_ms[k] += std::chrono::duration<double, std::milli>(t - t0).count();
    t0 = t;
  }
};
void phases_reset() {
  for (double& v : g_phase_ms) v = 0;
}
#else
struct PhaseLog {
  void lap(zkmi_ctx*, int) {}
};
void phases_reset() {}
#endif

template <int G>
struct Group;
template <>
struct Group<1> {
  using A = G1Affine;
  using F28 = Fq28;
  using Bases = zkmi_bases_g1;
  static constexpr uint64_t WIRE = 96;
  static int32_t msm(zkmi_ctx* ctx, const void* d_scal, uint64_t n, const Bases* b, uint8_t* out) {
    return zkmi_msm_g1_dev(ctx, d_scal, n, b, out);
  }
};
template <>
struct Group<2> {
  using A = G2Affine;
  using F28 = Fq2_28;
  using Bases = zkmi_bases_g2;
  static constexpr uint64_t WIRE = 192;
  static int32_t msm(zkmi_ctx* ctx, const void* d_scal, uint64_t n, const Bases* b, uint8_t* out) {
    return zkmi_msm_g2_dev(ctx, d_scal, n, b, out);
  }
};

// m >= 1 points of the r-order subgroup, resident form at d_res and / or 28-bit limb form at d28 (nullptr: converted here).
//   adjacent:  out_lo = sum_{i < m-1} w_i P[i], out_hi = sum_{i < m-1} w_i P[i + 1]   (affine WIRE form)
//   otherwise: out_lo = sum_{i < m} w_i P[i]; out_hi is not touched
// Two scalar vectors against one base array, both written by one launch; the MSM returns after its result has landed, so
// the buffers are free when this returns.
template <int G>
int32_t weighted_sums(zkmi_ctx* ctx, const typename Group<G>::A* d_res, const Affine<typename Group<G>::F28>* d28, uint64_t m,
                      const uint8_t seed[32], uint32_t dom, bool adjacent, uint8_t* out_lo, uint8_t* out_hi) {
  using GR = Group<G>;
  using A28 = Affine<typename GR::F28>;
  if (m == 0 || m > MSM_MAX_TERMS) return ctx->fail(ZKMI_ERR_BAD_ARG, "weighted sums: point count out of range");
  const uint64_t count = adjacent ? m - 1 : m;
  memset(out_lo, 0, GR::WIRE);
  if (adjacent) memset(out_hi, 0, GR::WIRE);
  if (count == 0) return ZKMI_OK;
  hipStream_t st = ctx->stream;
  PhaseLog log;
  DevBuf conv, scal;
  if (!d28) {
    ZK_HIP(ctx, conv.alloc(sizeof(A28) * m));
    ZK_HIP(ctx, bases_convert<typename GR::F28>(d_res, conv.as<A28>(), m, st));
    d28 = conv.as<A28>();
  }
  log.lap(ctx, CP_CONVERT);
  ZK_HIP(ctx, scal.alloc(32 * m * (adjacent ? 2 : 1)));
  uint4* d_lo = scal.as<uint4>();
  uint4* d_hi = adjacent ? d_lo + 2 * m : nullptr;
  hipLaunchKernelGGL(k_rlc_weights, dim3((unsigned)((count + RLC_BLOCK - 1) / RLC_BLOCK)), dim3(RLC_BLOCK), 0, st, rlc_seed(seed),
                     dom, count, d_lo, d_hi);
  ZK_HIP(ctx, hipGetLastError());
  log.lap(ctx, CP_WEIGHTS);
  typename GR::Bases bases;
  bases.ctx = ctx;
  bases.d = const_cast<typename GR::A*>(d_res);
  bases.d28 = const_cast<A28*>(d28);
  bases.n = m;
  int32_t rc = GR::msm(ctx, d_lo, m, &bases, out_lo);
  if (rc == ZKMI_OK && adjacent) rc = GR::msm(ctx, d_hi, m, &bases, out_hi);
  if (rc != ZKMI_OK) (void)ctx->drain();  // the buffers go when this returns
  log.lap(ctx, CP_MSM);
  return rc;
}

template <int G>
int32_t adjacent_sums_dev(zkmi_ctx* ctx, const void* d_points, uint64_t m, const uint8_t seed[32], uint32_t dom, uint8_t* out_lo,
                          uint8_t* out_hi) {
  ZK_ENTER(ctx);
  if (!d_points || !seed || !out_lo || !out_hi || m == 0 || m > MSM_MAX_TERMS || (reinterpret_cast<uintptr_t>(d_points) & 3u))
    return ZKMI_ERR_BAD_ARG;
  DevBuf res;
  ZK_HIP(ctx, res.alloc(sizeof(typename Group<G>::A) * m));
  uint64_t bad = UINT64_MAX;
  uint32_t stt = 0;
  const int32_t rc = points_read(ctx, G, d_points, m, ZKMI_ENC_WIRE, 0, res.p, true, nullptr, &bad, &stt);
  if (rc != ZKMI_OK) return rc;
  if (bad != UINT64_MAX) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "point " + std::to_string(bad) + ": " + point_status_name(stt));
  return weighted_sums<G>(ctx, res.as<typename Group<G>::A>(), nullptr, m, seed, dom, true, out_lo, out_hi);
}

// One named equation e(p0, q0) e(p1, q1) = 1
struct PairEq {
  G1Affine p0;
  G2Affine q0;
  G1Affine p1;
  G2Affine q1;
  uint32_t bit;
};

// Every equation is its own product of two Miller values under its own final exponentiation, so the one that fails is
// named; what they share is the launches: one of Miller loops over all the pairs, one of final exponentiations over all
// the groups (pairing_dev.hip: group e = values 2e and 2e + 1), one status byte per equation.  *failed |= the bits of the
// equations that do not hold.
int32_t pair_equations(zkmi_ctx* ctx, const std::vector<PairEq>& eqs, uint32_t* failed) {
  const uint64_t k = eqs.size();
  if (!k) return ZKMI_OK;
  PhaseLog log;
  auto up = [](uint64_t v) { return (v + 255) & ~255ull; };
  const uint64_t o_g1 = 0, o_g2 = up(192 * k), o_m = o_g2 + up(384 * k), o_st = o_m + up(2 * k * MILLER_BYTES), total = o_st + up(k);
  std::vector<uint8_t> host(o_m, 0), status(k, 0);
  for (uint64_t e = 0; e < k; e++) {
    g1_to_wire(eqs[e].p0, host.data() + o_g1 + 192 * e);
    g1_to_wire(eqs[e].p1, host.data() + o_g1 + 192 * e + 96);
    g2_to_wire(eqs[e].q0, host.data() + o_g2 + 384 * e);
    g2_to_wire(eqs[e].q1, host.data() + o_g2 + 384 * e + 192);
  }
  DevBuf buf;
  ZK_HIP(ctx, buf.alloc(total));
  uint8_t* d = buf.as<uint8_t>();
  hipStream_t st = ctx->stream;
  hipError_t err = hipMemcpyAsync(d, host.data(), o_m, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = miller_values_dev(ctx, d + o_g1, d + o_g2, 2 * k, d + o_m);
  if (err == hipSuccess) err = final_exp_dev(ctx, d + o_m, k, 2, 2, 1, nullptr, nullptr, d + o_st);
  if (err == hipSuccess) err = hipMemcpyAsync(status.data(), d + o_st, k, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // also on an error path: the buffers go when this returns
  if (err == hipSuccess) err = es;
  if (err != hipSuccess) return ctx->hip_fail(err, "ceremony: pairing equations");
  for (uint64_t e = 0; e < k; e++)
    if (status[e] != ZKMI_PROOF_OK) *failed |= eqs[e].bit;
  log.lap(ctx, CP_PAIRING);
  return ZKMI_OK;
}

bool wire_g1(const uint8_t* b, G1Affine* out) { return g1_from_wire(b, out, false); }
bool wire_g2(const uint8_t* b, G2Affine* out) { return g2_from_wire(b, out, false); }

int32_t draw_seed(zkmi_ctx* ctx, const uint8_t* seed, uint8_t drawn[32], const uint8_t** out) {
  *out = seed;
  if (seed) return ZKMI_OK;
  for (size_t off = 0; off < 32;) {
    const ssize_t got = getrandom(drawn + off, 32 - off, 0);
    if (got <= 0) return ctx->fail(ZKMI_ERR_BAD_ARG, "ceremony: getrandom failed");
    off += (size_t)got;
  }
  *out = drawn;
  return ZKMI_OK;
}

// the points the equations of a transcript are anchored on (infinity where the transcript has no such entry)
struct SrsAnchors {
  G1Affine tau1 = G1Affine::infinity(), alpha0 = G1Affine::infinity(), beta0 = G1Affine::infinity();
  G2Affine tau2 = G2Affine::infinity();
};

int32_t srs_anchors(zkmi_ctx* ctx, const zkmi_srs* srs, SrsAnchors* a) {
  if (srs->n_tau_g1 > 1) ZK_HIP(ctx, hipMemcpy(&a->tau1, srs->tau_g1 + 1, sizeof(G1Affine), hipMemcpyDeviceToHost));
  if (srs->n_tau_g2 > 1) ZK_HIP(ctx, hipMemcpy(&a->tau2, srs->tau_g2 + 1, sizeof(G2Affine), hipMemcpyDeviceToHost));
  ZK_HIP(ctx, hipMemcpy(&a->alpha0, srs->alpha_tau_g1, sizeof(G1Affine), hipMemcpyDeviceToHost));
  ZK_HIP(ctx, hipMemcpy(&a->beta0, srs->beta_tau_g1, sizeof(G1Affine), hipMemcpyDeviceToHost));
  return ZKMI_OK;
}

// a transcript the checks may be run on: of this context and device, every point read under ZKMI_CHECK_SUBGROUP
int32_t srs_verifiable(zkmi_ctx* ctx, const zkmi_srs* srs) {
  if (srs->ctx != ctx || srs->device != ctx->device) return ctx->fail(ZKMI_ERR_BAD_ARG, "transcript of another context");
  if (!(srs->checks & ZKMI_CHECK_SUBGROUP))
    return ctx->fail(ZKMI_ERR_BAD_ARG, "transcript was loaded without ZKMI_CHECK_SUBGROUP: its sums prove nothing");
  return ZKMI_OK;
}

// The five same-ratio equations of a resident transcript, appended to *eqs for the caller's one launch of pairings; a
// degenerate transcript raises ZKMI_SRS_DEGENERATE in *failed and appends nothing.  *an: the anchors that were read.
int32_t srs_consistency(zkmi_ctx* ctx, const zkmi_srs* srs, const uint8_t* seed, SrsAnchors* an, uint32_t* failed,
                        std::vector<PairEq>* eqs) {
  int32_t rc = srs_anchors(ctx, srs, an);
  if (rc != ZKMI_OK) return rc;
  const bool has_tau = srs->n_tau_g1 > 1 || srs->n_tau_g2 > 1 || srs->n_ab > 1;  // any power of tau above tau^0
  const G1Affine &tau1 = an->tau1, &alpha0 = an->alpha0, &beta0 = an->beta0;
  const G2Affine& tau2 = an->tau2;
  if ((has_tau && (tau1.is_inf() || tau2.is_inf())) || alpha0.is_inf() || beta0.is_inf() || srs->beta_g2.is_inf()) {
    *failed |= ZKMI_SRS_DEGENERATE;
    return ZKMI_OK;
  }
  if (has_tau) {
    // the three G1 chains against [tau]G2:  e(hi, G2) e(-lo, tau_g2[1]) = 1
    struct {
      const G1Affine* chain;
      uint64_t m;
      uint32_t dom, bit;
    } const chains[3] = {{srs->tau_g1, srs->n_tau_g1, 0, ZKMI_SRS_BAD_TAU_G1},
                         {srs->alpha_tau_g1, srs->n_ab, 2, ZKMI_SRS_BAD_ALPHA},
                         {srs->beta_tau_g1, srs->n_ab, 3, ZKMI_SRS_BAD_BETA}};
    for (const auto& c : chains) {
      uint8_t lo_w[96], hi_w[96];
      if ((rc = weighted_sums<1>(ctx, c.chain, nullptr, c.m, seed, c.dom, true, lo_w, hi_w)) != ZKMI_OK) return rc;
      G1Affine lo, hi;
      if (!wire_g1(lo_w, &lo) || !wire_g1(hi_w, &hi)) return ctx->fail(ZKMI_ERR_HIP, "ceremony: the MSM returned a non-canonical point");
      eqs->push_back({hi, g2_generator(), lo.neg(), tau2, c.bit});
    }
    // the G2 chain against [tau]G1:  e(tau_g1[1], lo) e(-G1, hi) = 1; its term i = 0 ties tau in G1 to tau in G2
    uint8_t lo_w[192], hi_w[192];
    if ((rc = weighted_sums<2>(ctx, srs->tau_g2, nullptr, srs->n_tau_g2, seed, 1, true, lo_w, hi_w)) != ZKMI_OK) return rc;
    G2Affine lo, hi;
    if (!wire_g2(lo_w, &lo) || !wire_g2(hi_w, &hi)) return ctx->fail(ZKMI_ERR_HIP, "ceremony: the MSM returned a non-canonical point");
    eqs->push_back({tau1, lo, g1_generator().neg(), hi, ZKMI_SRS_BAD_TAU_G2});
  }
  // beta in G1 and in G2:  e(beta_tau_g1[0], G2) e(-G1, beta_g2) = 1
  eqs->push_back({beta0, g2_generator(), g1_generator().neg(), srs->beta_g2, ZKMI_SRS_BAD_BETA_G2});
  return ZKMI_OK;
}

}  // namespace

int32_t pk_verify_contribution(zkmi_ctx* ctx, const PkCeremonyView& before, const PkCeremonyView& after, const uint8_t seed_in[32],
                               uint32_t* out_failed) {
  uint8_t drawn[32];
  const uint8_t* seed = nullptr;
  int32_t rc = draw_seed(ctx, seed_in, drawn, &seed);
  if (rc != ZKMI_OK) return rc;
  phases_reset();
  hipStream_t st = ctx->stream;
  const uint64_t N = 1ull << after.log_n, nv = after.n_vars, np = after.n_pub;
  uint32_t failed = 0;
  // the part a contribution must not touch: three single elements on the host, three queries word by word on the device
  const bool singles_same = before.alpha_g1.x == after.alpha_g1.x && before.alpha_g1.y == after.alpha_g1.y &&
                            before.beta_g1.x == after.beta_g1.x && before.beta_g1.y == after.beta_g1.y &&
                            before.beta_g2.x == after.beta_g2.x && before.beta_g2.y == after.beta_g2.y;
  DevBuf d_status;
  ZK_HIP(ctx, d_status.alloc(sizeof(uint32_t)));
  ZK_HIP(ctx, hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  struct {
    const void *a, *b;
    uint64_t words;
  } const fixed[3] = {{before.a, after.a, nv * (sizeof(G1Affine) / 4)},
                      {before.b_g1, after.b_g1, nv * (sizeof(G1Affine) / 4)},
                      {before.b_g2, after.b_g2, nv * (sizeof(G2Affine) / 4)}};
  for (const auto& f : fixed) {
    if (!f.words) continue;
    hipLaunchKernelGGL(k_points_differ, dim3((unsigned)((f.words + 255) / 256)), dim3(256), 0, st, static_cast<const uint32_t*>(f.a),
                       static_cast<const uint32_t*>(f.b), f.words, d_status.as<uint32_t>());
    ZK_HIP(ctx, hipGetLastError());
  }
  uint32_t differ = 0;
  ZK_HIP(ctx, hipMemcpyAsync(&differ, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  ZK_HIP(ctx, hipStreamSynchronize(st));
  if (!singles_same || differ) failed |= ZKMI_PK2_FIXED_PART_DIFFERS;
  std::vector<PairEq> eqs;
  // delta' is one non-zero scalar in both groups:  e(delta'_1, G2) e(-G1, delta'_2) = 1
  if (after.delta_g1.is_inf() || after.delta_g2.is_inf()) failed |= ZKMI_PK2_BAD_DELTA;
  else eqs.push_back({after.delta_g1, g2_generator(), g1_generator().neg(), after.delta_g2, ZKMI_PK2_BAD_DELTA});
  // h and the non-public l moved by the inverse of what delta moved by:  e(S', delta'_2) e(-S, delta_2) = 1
  struct {
    const Affine<Fq28>*b, *a;
    uint64_t count;
    uint32_t dom, bit;
  } const moved[2] = {{before.h28, after.h28, N - 1, RLC_DOM_PK + 3, ZKMI_PK2_BAD_H},
                      {before.l28 + np, after.l28 + np, nv - np, RLC_DOM_PK + 4, ZKMI_PK2_BAD_L}};
  for (const auto& q : moved) {
    if (!q.count) continue;
    uint8_t sb_w[96], sa_w[96];
    if ((rc = weighted_sums<1>(ctx, nullptr, q.b, q.count, seed, q.dom, false, sb_w, nullptr)) != ZKMI_OK) return rc;
    if ((rc = weighted_sums<1>(ctx, nullptr, q.a, q.count, seed, q.dom, false, sa_w, nullptr)) != ZKMI_OK) return rc;
    G1Affine sb, sa;
    if (!wire_g1(sb_w, &sb) || !wire_g1(sa_w, &sa)) return ctx->fail(ZKMI_ERR_HIP, "ceremony: the MSM returned a non-canonical point");
    eqs.push_back({sa, after.delta_g2, sb.neg(), before.delta_g2, q.bit});
  }
  if ((rc = pair_equations(ctx, eqs, &failed)) != ZKMI_OK) return rc;
  *out_failed = failed;
  return failed ? ctx->fail(ZKMI_ERR_VERIFICATION, "contribution: failed checks, mask " + std::to_string(failed)) : ZKMI_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int32_t zkmi_g1_points_adjacent_sums_dev(zkmi_ctx* ctx, const void* d_points, uint64_t m, const uint8_t seed[32], uint32_t dom,
                                         uint8_t out_lo[96], uint8_t out_hi[96]) {
  return adjacent_sums_dev<1>(ctx, d_points, m, seed, dom, out_lo, out_hi);
}

int32_t zkmi_g2_points_adjacent_sums_dev(zkmi_ctx* ctx, const void* d_points, uint64_t m, const uint8_t seed[32], uint32_t dom,
                                         uint8_t out_lo[192], uint8_t out_hi[192]) {
  return adjacent_sums_dev<2>(ctx, d_points, m, seed, dom, out_lo, out_hi);
}

int32_t zkmi_srs_verify(zkmi_ctx* ctx, const zkmi_srs* srs, const uint8_t seed_in[32], uint32_t* out_failed) {
  ZK_ENTER(ctx);
  if (!srs || !out_failed) return ZKMI_ERR_BAD_ARG;
  *out_failed = 0;
  int32_t rc = srs_verifiable(ctx, srs);
  if (rc != ZKMI_OK) return rc;
  uint8_t drawn[32];
  const uint8_t* seed = nullptr;
  if ((rc = draw_seed(ctx, seed_in, drawn, &seed)) != ZKMI_OK) return rc;
  ZK_HIP(ctx, ctx->drain());
  phases_reset();
  uint32_t failed = 0;
  std::vector<PairEq> eqs;
  SrsAnchors an;
  if ((rc = srs_consistency(ctx, srs, seed, &an, &failed, &eqs)) != ZKMI_OK) return rc;
  if (failed & ZKMI_SRS_DEGENERATE) {
    *out_failed = failed;
    return ctx->fail(ZKMI_ERR_VERIFICATION, "transcript: degenerate (an anchor point is infinity, or there is no tau to compare against)");
  }
  if ((rc = pair_equations(ctx, eqs, &failed)) != ZKMI_OK) return rc;
  *out_failed = failed;
  return failed ? ctx->fail(ZKMI_ERR_VERIFICATION, "transcript: failed checks, mask " + std::to_string(failed)) : ZKMI_OK;
}

int32_t zkmi_srs_verify_contribution(zkmi_ctx* ctx, const zkmi_srs* before, const zkmi_srs* after, const uint8_t step_g2[576],
                                     const uint8_t seed_in[32], uint32_t* out_failed) {
  ZK_ENTER(ctx);
  if (!before || !after || !step_g2 || !out_failed) return ZKMI_ERR_BAD_ARG;
  *out_failed = 0;
  int32_t rc = srs_verifiable(ctx, before);
  if (rc == ZKMI_OK) rc = srs_verifiable(ctx, after);
  if (rc != ZKMI_OK) return rc;
  if (before->n_tau_g1 != after->n_tau_g1 || before->n_tau_g2 != after->n_tau_g2 || before->n_ab != after->n_ab)
    return ctx->fail(ZKMI_ERR_BAD_ARG, "transcripts of different shape");
  // the step elements [s]G2 | [a]G2 | [b]G2: on the curve and in the subgroup, or the pairing says nothing
  G2Affine step[3];
  bool step_inf = false;
  for (int j = 0; j < 3; j++) {
    if (!g2_from_wire(step_g2 + 192 * j, &step[j], true) || !g2_in_subgroup(step[j]))
      return ctx->fail(ZKMI_ERR_NON_CANONICAL, "step element " + std::to_string(j) + ": not a point of the G2 subgroup");
    step_inf = step_inf || step[j].is_inf();
  }
  uint8_t drawn[32];
  const uint8_t* seed = nullptr;
  if ((rc = draw_seed(ctx, seed_in, drawn, &seed)) != ZKMI_OK) return rc;
  ZK_HIP(ctx, ctx->drain());
  phases_reset();
  uint32_t failed = 0;
  std::vector<PairEq> eqs;
  SrsAnchors a, b;
  if ((rc = srs_consistency(ctx, after, seed, &a, &failed, &eqs)) != ZKMI_OK) return rc;
  if ((rc = srs_anchors(ctx, before, &b)) != ZKMI_OK) return rc;
  // after = before moved by the logarithms of the step elements: one equation per element, anchored on the first point of
  // each chain that carries it.  The domain of size 1 has no tau_g1[1]: no tau step to compare.
  const bool has_tau1 = before->n_tau_g1 > 1;
  if (step_inf || (has_tau1 && b.tau1.is_inf()) || b.alpha0.is_inf() || b.beta0.is_inf()) {
    failed |= ZKMI_SRS_STEP_DEGENERATE;
  } else {
    struct {
      const G1Affine *now, *was;
      const G2Affine* by;
      uint32_t bit;
      bool present;
    } const steps[3] = {{&a.tau1, &b.tau1, &step[0], ZKMI_SRS_STEP_BAD_TAU, has_tau1},
                        {&a.alpha0, &b.alpha0, &step[1], ZKMI_SRS_STEP_BAD_ALPHA, true},
                        {&a.beta0, &b.beta0, &step[2], ZKMI_SRS_STEP_BAD_BETA, true}};
    for (const auto& s : steps) {
      if (!s.present) continue;
      // e(now, G2) e(-was, step) = 1.  `was` and `step` are finite here, so e(was, step) != 1: an infinite `now` fails
      // the equation without a Miller loop.
      if (s.now->is_inf()) failed |= s.bit;
      else eqs.push_back({*s.now, g2_generator(), s.was->neg(), *s.by, s.bit});
    }
  }
  if ((rc = pair_equations(ctx, eqs, &failed)) != ZKMI_OK) return rc;
  *out_failed = failed;
  return failed ? ctx->fail(ZKMI_ERR_VERIFICATION, "transcript contribution: failed checks, mask " + std::to_string(failed)) : ZKMI_OK;
}

}  // extern "C"

#ifdef ZKMI_TESTING  // test scaffolding: libzkmi_exp.so only (include/zkmi_testing.h)
extern "C" {

int32_t zkmi_selftest_rlc_weights_host(const uint8_t seed[32], uint32_t dom, uint64_t first, uint64_t count, uint8_t* out16) {
  if (!seed || (count && !out16) || first + count < first) return ZKMI_ERR_BAD_ARG;
  const RlcSeed s = rlc_seed(seed);
  for (uint64_t k = 0; k < count; k++) {
    uint32_t w[4];
    rlc_weight_body(s, dom, first + k, w);
    memcpy(out16 + 16 * k, w, 16);
  }
  return ZKMI_OK;
}

int32_t zkmi_ceremony_phases(double out_ms[4]) {
  if (!out_ms) return ZKMI_ERR_BAD_ARG;
  for (int k = 0; k < CP_NPHASE; k++) out_ms[k] = g_phase_ms[k];
  return ZKMI_OK;
}

}  // extern "C"
#endif  // ZKMI_TESTING
