// zkmi — batch verification of Groth16 proofs of one key (zkmi_vk_prepare, zkmi_groth16_verify_batch).
//
//   prod_i e(w_i A_i, B_i) * e(-(sum w_i) alpha, beta) * e(-sum_i w_i X_i, gamma) * e(-sum_i w_i C_i, delta) = 1
//
// with X_i = ic_0 + sum_j pub_ij ic_j and caller-drawn 128-bit weights w_i: n + 3 Miller loops on the device
// (pairing_dev.hip) and one final exponentiation, where zkmi_groth16_verify spends four loops and one exponentiation
// per proof.  What runs where:
//   device  upload once, strided copies split A | B | C, k_points_read decompresses and subgroup-checks each array
//           (the acceptance rules of the host verifier by construction), k_scale_g1 forms w_i A_i, the library's G1 MSM
//           forms sum w_i C_i over the decompressed C_i, k_miller / k_miller_product the pairing product
//   host    sum w_i and sum_i w_i pub_ij in Fr, n_pub + 1 scalar multiplications for the alpha and gamma pairs, the
//           final exponentiation
// A malformed proof keeps its status, gets A_i = O (its Miller value is 1) and weight 0 in every sum.  Localisation
// re-runs the same path on index ranges: the per-proof Miller values stay in HBM, a range costs its three sums, three
// Miller loops and one final exponentiation.
#include <string.h>
#include <sys/random.h>
#include <chrono>
#include <new>
#include <vector>
#include "pairing_dev.hpp"
#include "verify.hpp"
#include "points.hpp"
#include "field28.hpp"

namespace zkmi {

namespace {

// out_i = [w_i] P_i for n G1 points in affine WIRE form and 128-bit little-endian w_i, one lane per point: 128 steps of
// double-and-add on the lane's own bit.  For P in the r-order subgroup the running multiple k P, k < 2^128 < r, never
// meets +-P, so the rare cases of the complete addition are reached only from infinity (the leading zeros of w_i, an
// infinite P) or by garbage nobody reads.  One inversion per lane brings the result back to affine.
__global__ __launch_bounds__(64) void k_scale_g1(const uint32_t* __restrict__ in, const uint32_t* __restrict__ w, uint64_t n,
                                                 uint32_t* __restrict__ out) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = gid < n;
  const uint64_t idx = live ? gid : n - 1;  // n >= 1 (host)
  uint32_t xw[12], yw[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    xw[i] = in[idx * 24 + i];
    yw[i] = in[idx * 24 + 12 + i];
  }
  const Affine<Fq28> p = {Fq28::from_canonical(xw), Fq28::from_canonical(yw)};
  const uint32_t k0 = w[idx * 4], k1 = w[idx * 4 + 1], k2 = w[idx * 4 + 2], k3 = w[idx * 4 + 3];
  XYZZ<Fq28> acc = XYZZ<Fq28>::infinity();
#pragma unroll 1
  for (int b = 127; b >= 0; b--) {
    acc.dbl_inplace();
    const int wi = b >> 5;
    const uint32_t word = wi == 0 ? k0 : wi == 1 ? k1 : wi == 2 ? k2 : k3;
    if ((word >> (b & 31)) & 1u) acc.madd(p);
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

bool parse_vk(const uint8_t* vk, uint32_t n_pub, zkmi_vk* out) {
  out->n_pub = n_pub;
  if (!g1_from_wire(vk, &out->alpha, true) || !g2_from_wire(vk + 96, &out->beta, true) ||
      !g2_from_wire(vk + 288, &out->gamma, true) || !g2_from_wire(vk + 480, &out->delta, true))
    return false;
  if (!g1_in_subgroup(out->alpha) || !g2_in_subgroup(out->beta) || !g2_in_subgroup(out->gamma) || !g2_in_subgroup(out->delta))
    return false;
  out->ic.resize(n_pub);
  for (uint32_t j = 0; j < n_pub; j++)
    if (!g1_from_wire(vk + 672 + 96ull * j, &out->ic[j], true) || !g1_in_subgroup(out->ic[j])) return false;
  return true;
}

// Where a call spends its time (testing library only: zkmi_verify_batch_phases): the host clock at points where the
// stream is waited for; the product library compiles lap() to nothing and adds no synchronisation.
enum { VB_UPLOAD, VB_POINTS, VB_SCALE, VB_MILLER, VB_SUMS, VB_PRODUCT, VB_FINAL_EXP, VB_NPHASE };
#ifdef ZKMI_TESTING
double g_phase_ms[VB_NPHASE];
struct PhaseLog {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(zkmi_ctx* ctx, int k) {
    (void)hipStreamSynchronize(ctx->stream);
    const auto t = std::chrono::steady_clock::now();
    g_phase_ms[k] += std::chrono::duration<double, std::milli>(t - t0).count();
    t0 = t;
  }
};
#else
struct PhaseLog {
  void lap(zkmi_ctx*, int) {}
};
#endif

Fr fr_from_u128(const uint8_t* b) {
  Fr a = Fr::zero();
  memcpy(a.l, b, 16);
  return a.to_mont();
}

struct Batch {
  zkmi_ctx* ctx;
  const zkmi_vk* vk;
  uint64_t n;
  const uint8_t* weights;          // n x 16
  std::vector<Fr> pub;             // n x (n_pub - 1), Montgomery; unspecified for malformed proofs
  std::vector<uint8_t> status;     // per proof
  std::vector<uint8_t> c_inf;      // C_i = O: kept out of the MSM (its term is O)
  // device
  uint8_t *d_g1, *d_g2, *d_miller, *d_partials, *d_scal;
  G1Affine* d_c;
  Affine<Fq28>* d_c28;
  std::vector<uint8_t> scal;  // host image of the MSM scalars of one range
  uint64_t checks = 0;
  PhaseLog log;

  // the equation over the well-formed proofs of [lo, hi)
  int32_t check(uint64_t lo, uint64_t hi, bool* ok) {
    const uint32_t np1 = vk->n_pub - 1;
    Fr sw = Fr::zero();
    std::vector<Fr> sp(np1, Fr::zero());
    memset(scal.data() + 32 * lo, 0, 32 * (hi - lo));
    uint64_t members = 0;
    for (uint64_t i = lo; i < hi; i++) {
      if (status[i] != ZKMI_PROOF_OK) continue;
      members++;
      const Fr w = fr_from_u128(weights + 16 * i);
      sw = sw + w;
      for (uint32_t j = 0; j < np1; j++) sp[j] = sp[j] + w * pub[i * np1 + j];
      if (!c_inf[i]) memcpy(scal.data() + 32 * i, weights + 16 * i, 16);
    }
    *ok = true;
    if (!members) return ZKMI_OK;
    checks++;
    // sum w_i C_i: the library's G1 MSM over the decompressed points of the range
    ZK_HIP(ctx, hipMemcpyAsync(d_scal + 32 * lo, scal.data() + 32 * lo, 32 * (hi - lo), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    zkmi_bases_g1 bases;
    bases.ctx = ctx;
    bases.d = d_c + lo;
    bases.d28 = d_c28 + lo;
    bases.n = hi - lo;
    uint8_t tail[3 * 96];
    int32_t rc = zkmi_msm_g1_dev(ctx, d_scal + 32 * lo, hi - lo, &bases, tail + 192);
    if (rc != ZKMI_OK) return rc;
    G1Affine csum;
    if (!g1_from_wire(tail + 192, &csum, false)) return ctx->fail(ZKMI_ERR_HIP, "verify batch: the MSM returned a non-canonical point");
    const Fr swc = sw.from_mont();
    g1_to_wire(scalar_mul(G1XYZZ::from_affine(vk->alpha), swc.l, 8).to_affine().neg(), tail);
    G1XYZZ x = scalar_mul(G1XYZZ::from_affine(vk->ic[0]), swc.l, 8);
    for (uint32_t j = 0; j < np1; j++) x.add(scalar_mul(G1XYZZ::from_affine(vk->ic[j + 1]), sp[j].from_mont().l, 8));
    g1_to_wire(x.to_affine().neg(), tail + 96);
    g1_to_wire(csum.neg(), tail + 192);
    log.lap(ctx, VB_SUMS);
    ZK_HIP(ctx, hipMemcpyAsync(d_g1 + 96 * n, tail, sizeof(tail), hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = miller_values_dev(ctx, d_g1 + 96 * n, d_g2 + 192 * n, 3, d_miller + MILLER_BYTES * n);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      return ctx->hip_fail(e, "verify batch: Miller loops");
    }
    Fq12 t, s;
    if ((rc = miller_product_dev(ctx, d_miller + MILLER_BYTES * n, 3, d_partials, &t)) != ZKMI_OK) return rc;
    if ((rc = miller_product_dev(ctx, d_miller + MILLER_BYTES * lo, hi - lo, d_partials, &s)) != ZKMI_OK) return rc;
    log.lap(ctx, VB_PRODUCT);
    *ok = final_exponentiation((s * t).conj()) == Fq12::one();
    log.lap(ctx, VB_FINAL_EXP);
    return ZKMI_OK;
  }

  // [lo, hi) is known to fail: halve until single proofs are left
  int32_t mark(uint64_t lo, uint64_t hi) {
    uint64_t members = 0, last = lo;
    for (uint64_t i = lo; i < hi; i++)
      if (status[i] == ZKMI_PROOF_OK) {
        members++;
        last = i;
      }
    if (members == 1) {
      status[last] = ZKMI_PROOF_PAIRING;
      return ZKMI_OK;
    }
    const uint64_t mid = lo + (hi - lo) / 2;
    bool left_ok = true, right_ok = false;
    int32_t rc = check(lo, mid, &left_ok);
    if (rc != ZKMI_OK) return rc;
    // the product of the halves is the product of the whole: a passing left half leaves the fault to the right one
    if (!left_ok && (rc = check(mid, hi, &right_ok)) != ZKMI_OK) return rc;
    if (!left_ok && (rc = mark(lo, mid)) != ZKMI_OK) return rc;
    if (!right_ok && (rc = mark(mid, hi)) != ZKMI_OK) return rc;
    return ZKMI_OK;
  }
};

}  // namespace

}  // namespace zkmi

extern "C" {

int32_t zkmi_vk_prepare(const uint8_t* vk, uint32_t n_pub, zkmi_vk** out) {
  if (!vk || !out || n_pub == 0) return ZKMI_ERR_BAD_ARG;
  *out = nullptr;
  zkmi_vk* v = new (std::nothrow) zkmi_vk();
  if (!v) return ZKMI_ERR_BAD_ARG;
  if (!zkmi::parse_vk(vk, n_pub, v)) {
    delete v;
    return ZKMI_ERR_NON_CANONICAL;
  }
  *out = v;
  return ZKMI_OK;
}

int32_t zkmi_vk_free(zkmi_vk* vk) {
  if (!vk) return ZKMI_ERR_BAD_ARG;
  delete vk;
  return ZKMI_OK;
}

int32_t zkmi_groth16_verify_batch(zkmi_ctx* ctx, const zkmi_vk* vk, uint64_t n, const uint8_t* publics,
                                  const uint8_t* proofs, const uint8_t* weights, uint8_t* out_status,
                                  uint64_t* out_first_bad) {
  using namespace zkmi;
  ZK_ENTER(ctx);
  if (!vk || n > (1ull << 24)) return ZKMI_ERR_BAD_ARG;
  if (out_first_bad) *out_first_bad = UINT64_MAX;
  if (n == 0) return ZKMI_OK;
  const uint32_t np1 = vk->n_pub - 1;
  if (!proofs || (np1 && !publics)) return ZKMI_ERR_BAD_ARG;
  std::vector<uint8_t> drawn;
  if (weights) {
    for (uint64_t i = 0; i < n; i++) {
      uint8_t acc = 0;
      for (int k = 0; k < 16; k++) acc |= weights[16 * i + k];
      if (!acc) return ctx->fail(ZKMI_ERR_BAD_ARG, "verify batch: weight " + std::to_string(i) + " is zero");
    }
  } else {
    drawn.resize(16 * n);
    for (uint64_t off = 0; off < drawn.size();) {
      const ssize_t got = getrandom(drawn.data() + off, drawn.size() - off, 0);
      if (got <= 0) return ctx->fail(ZKMI_ERR_BAD_ARG, "verify batch: getrandom failed");
      off += (uint64_t)got;
    }
    for (uint64_t i = 0; i < n; i++) {
      uint8_t acc = 0;
      for (int k = 0; k < 16; k++) acc |= drawn[16 * i + k];
      if (!acc) drawn[16 * i] = 1;  // probability 2^-128
    }
    weights = drawn.data();
  }

  // one allocation: [proofs | A, C compressed | B compressed | A wire | g1 (n + 3) | g2 (n + 3) | C resident | C limbs |
  //                  Miller values (n + 3) | partial products | MSM scalars | weights | status (3 n)]
  auto up = [](uint64_t v) { return (v + 255) & ~255ull; };
  const uint64_t o_proofs = 0, o_ac = o_proofs + up(192 * n), o_cc = o_ac + up(48 * n), o_bc = o_cc + up(48 * n),
                 o_aw = o_bc + up(96 * n), o_g1 = o_aw + up(96 * n), o_g2 = o_g1 + up(96 * (n + 3)),
                 o_c = o_g2 + up(192 * (n + 3)), o_c28 = o_c + up(sizeof(G1Affine) * n),
                 o_m = o_c28 + up(sizeof(Affine<Fq28>) * n), o_part = o_m + up(MILLER_BYTES * (n + 3)),
                 o_scal = o_part + up(MILLER_BYTES * MILLER_PARTIALS), o_w = o_scal + up(32 * n), o_st = o_w + up(16 * n),
                 total = o_st + up(3 * n);
  uint8_t* d = nullptr;
  ZK_HIP(ctx, hipMalloc(&d, total));
  struct Free {
    zkmi_ctx* c;
    uint8_t* p;
    ~Free() {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(p);
    }
  } guard{ctx, d};
  hipStream_t st = ctx->stream;
  PhaseLog log;
#ifdef ZKMI_TESTING
  for (double& v : g_phase_ms) v = 0;
#endif
  ZK_HIP(ctx, hipMemcpyAsync(d + o_proofs, proofs, 192 * n, hipMemcpyHostToDevice, st));
  ZK_HIP(ctx, hipMemcpyAsync(d + o_w, weights, 16 * n, hipMemcpyHostToDevice, st));
  uint8_t g2tail[3 * 192];
  g2_to_wire(vk->beta, g2tail);
  g2_to_wire(vk->gamma, g2tail + 192);
  g2_to_wire(vk->delta, g2tail + 384);
  ZK_HIP(ctx, hipMemcpyAsync(d + o_g2 + 192 * n, g2tail, sizeof(g2tail), hipMemcpyHostToDevice, st));
  ZK_HIP(ctx, hipMemcpy2DAsync(d + o_ac, 48, d + o_proofs, 192, 48, n, hipMemcpyDeviceToDevice, st));
  ZK_HIP(ctx, hipMemcpy2DAsync(d + o_bc, 96, d + o_proofs + 48, 192, 96, n, hipMemcpyDeviceToDevice, st));
  ZK_HIP(ctx, hipMemcpy2DAsync(d + o_cc, 48, d + o_proofs + 144, 192, 48, n, hipMemcpyDeviceToDevice, st));
  log.lap(ctx, VB_UPLOAD);
  const int32_t enc = ZKMI_ENC_ZCASH_COMPRESSED, chk = ZKMI_CHECK_SUBGROUP;
  int32_t rc;
  if ((rc = points_read(ctx, 1, d + o_ac, n, enc, chk, d + o_aw, false, d + o_st, nullptr, nullptr)) != ZKMI_OK) return rc;
  if ((rc = points_read(ctx, 2, d + o_bc, n, enc, chk, d + o_g2, false, d + o_st + n, nullptr, nullptr)) != ZKMI_OK) return rc;
  if ((rc = points_read(ctx, 1, d + o_cc, n, enc, chk, d + o_c, true, d + o_st + 2 * n, nullptr, nullptr)) != ZKMI_OK) return rc;
  std::vector<uint8_t> pst(3 * n);
  ZK_HIP(ctx, hipMemcpyAsync(pst.data(), d + o_st, 3 * n, hipMemcpyDeviceToHost, st));
  ZK_HIP(ctx, hipStreamSynchronize(st));

  log.lap(ctx, VB_POINTS);

  Batch b;
  b.ctx = ctx;
  b.vk = vk;
  b.n = n;
  b.weights = weights;
  b.status.assign(n, ZKMI_PROOF_OK);
  b.c_inf.assign(n, 0);
  b.pub.assign(n * np1, Fr::zero());
  b.scal.assign(32 * n, 0);
  b.d_g1 = d + o_g1;
  b.d_g2 = d + o_g2;
  b.d_miller = d + o_m;
  b.d_partials = d + o_part;
  b.d_scal = d + o_scal;
  b.d_c = reinterpret_cast<G1Affine*>(d + o_c);
  b.d_c28 = reinterpret_cast<Affine<Fq28>*>(d + o_c28);
  bool malformed = false;
  for (uint64_t i = 0; i < n; i++) {
    uint8_t s = pst[i] ? pst[i] : pst[n + i] ? pst[n + i] : pst[2 * n + i];  // A, B, C: ZKMI_PT_* = ZKMI_PROOF_*
    for (uint32_t j = 0; j < np1 && !s; j++)
      if (!fr_from_wire(publics + 32 * (i * np1 + j), &b.pub[i * np1 + j])) s = ZKMI_PROOF_BAD_PUBLIC;
    b.status[i] = s;
    b.c_inf[i] = (proofs[192 * i + 144] & 0x40) ? 1 : 0;
    if (s) {
      malformed = true;
      // the outputs of a refused point are unspecified: A_i = O (Miller value 1), C_i = O
      ZK_HIP(ctx, hipMemsetAsync(d + o_aw + 96 * i, 0, 96, st));
      ZK_HIP(ctx, hipMemsetAsync(d + o_c + sizeof(G1Affine) * i, 0, sizeof(G1Affine), st));
    }
  }
  hipLaunchKernelGGL(k_scale_g1, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, reinterpret_cast<const uint32_t*>(d + o_aw),
                     reinterpret_cast<const uint32_t*>(d + o_w), n, reinterpret_cast<uint32_t*>(d + o_g1));
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, bases_convert<Fq28>(b.d_c, b.d_c28, n, st));
  log.lap(ctx, VB_SCALE);
  ZK_HIP(ctx, miller_values_dev(ctx, b.d_g1, b.d_g2, n, b.d_miller));
  log.lap(ctx, VB_MILLER);
  b.log = log;

  bool ok = true;
  if ((rc = b.check(0, n, &ok)) != ZKMI_OK) return rc;
  if (!ok && (out_status || out_first_bad) && (rc = b.mark(0, n)) != ZKMI_OK) return rc;
  if (out_status) memcpy(out_status, b.status.data(), n);
  if (out_first_bad)
    for (uint64_t i = 0; i < n; i++)
      if (b.status[i]) {
        *out_first_bad = i;
        break;
      }
  if (malformed) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "verify batch: a malformed proof");
  return ok ? ZKMI_OK : ctx->fail(ZKMI_ERR_VERIFICATION, "verify batch: a pairing equation does not hold");
}

}  // extern "C"

#ifdef ZKMI_TESTING  // test scaffolding: libzkmi_exp.so only (include/zkmi_testing.h)
extern "C" int32_t zkmi_verify_batch_phases(double out_ms[7]) {
  if (!out_ms) return ZKMI_ERR_BAD_ARG;
  for (int k = 0; k < zkmi::VB_NPHASE; k++) out_ms[k] = zkmi::g_phase_ms[k];
  return ZKMI_OK;
}
#endif  // ZKMI_TESTING
