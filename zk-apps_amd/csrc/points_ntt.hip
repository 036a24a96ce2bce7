// zkmi — transforms whose elements are curve points, and the phase-1 transcript ("powers of tau" with alpha and beta)
// they are meant for: the first layers of a Groth16 setup that never sees the toxic waste.
//
// Reference locus: none in /root/reference; the specification is oracle/groth16.py lagrange_at(): [L_i(tau)]G is the
// inverse DFT of [tau^k]G "in the exponent", in exactly the convention of zkmi_ntt_fr(inverse = 1, coset = 0) (natural
// order in and out, scaled by N^-1).
//
// Kernels (one lane per element, F = Fq for G1 and Fq2 for G2, the 32-bit-limb fields k_fixed_base runs on):
//   k_pn_load   resident affine -> XYZZ at the bit-reversed position (inverse: times N^-1 on the way, by mixed additions)
//   k_pn_level  one radix-2 level, one lane per butterfly (P, Q) -> (P + wQ, P - wQ); blockIdx.y = array.  wQ is a
//               255-bit double-and-add, so a level is arithmetic-bound by orders of magnitude and takes no LDS tile.
//               w = 1 (every butterfly of level 0, the first of every group later) multiplies nothing; the inverse
//               reads w^-k = -w^(N/2 - k) from the same table.  Both additions are the complete one (curve.hpp
//               XYZZ::add): P = wQ, P = -wQ and infinity all occur on legitimate inputs.
//   k_pn_store  XYZZ -> resident affine, PN_INV_BATCH points per lane under one inversion
//
// A phase-1 contribution (zkmi_srs_contribute) is four calls of the per-point multiplication of points_mul.hip over the
// transcript's arrays, under powers made on the device; no kernel of its own lives here.
#include <string.h>
#include <algorithm>
#include <new>
#include <string>
#include <type_traits>
#include "points_ntt.hpp"
#include "group_dev.hpp"
#include "points.hpp"
#include "points_mul.hpp"

namespace zkmi {

namespace {

template <class F>
__global__ void __launch_bounds__(64)
k_pn_load(const Affine<F>* __restrict__ in, uint64_t stride, XYZZ<F>* __restrict__ work, uint32_t log_n,
          const uint32_t* __restrict__ scale) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = 1u << log_n;
  if (i >= n) return;
  const Affine<F> p = ldv(in + (size_t)blockIdx.y * stride + i);
  XYZZ<F> v = XYZZ<F>::from_affine(p);
  if (scale) mul_words(&p, scale, &v);
  const uint32_t r = log_n ? (__brev(i) >> (32 - log_n)) : 0u;
  stv(work + (size_t)blockIdx.y * n + r, v);
}

template <class F>
__global__ void __launch_bounds__(64)
k_pn_level(XYZZ<F>* __restrict__ work, const uint32_t* __restrict__ tw, uint32_t log_n, uint32_t s, int inverse) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t half_n = 1u << (log_n - 1);
  if (j >= half_n) return;
  XYZZ<F>* arr = work + ((size_t)blockIdx.y << log_n);
  const uint32_t k = j & ((1u << s) - 1u);
  const uint32_t i0 = ((j >> s) << (s + 1)) + k, i1 = i0 + (1u << s);  // i1 < 2^log_n
  XYZZ<F> q = ldv(arr + i1);
  if (k) {
    uint32_t t = k << (log_n - 1 - s);  // 0 < t < N/2
    if (inverse) t = half_n - t;
    const XYZZ<F> q0 = q;
    mul_words(&q0, tw + (size_t)t * 8, &q);
    if (inverse) q = q.neg();
  }
  XYZZ<F> p = ldv(arr + i0);
  XYZZ<F> d = p;
  g_add(&p, &q);
  q = q.neg();
  g_add(&d, &q);
  stv(arr + i0, p);
  stv(arr + i1, d);
}

template <class F>
__global__ void __launch_bounds__(64)
k_pn_store(const XYZZ<F>* __restrict__ work, Affine<F>* __restrict__ out, uint64_t stride, uint32_t log_n) {
  const uint32_t n = 1u << log_n;
  const uint32_t first = (blockIdx.x * blockDim.x + threadIdx.x) * PN_INV_BATCH;
  if (first >= n) return;
  const XYZZ<F>* src = work + (size_t)blockIdx.y * n;
  Affine<F>* dst = out + (size_t)blockIdx.y * stride;
  const uint32_t cnt = n - first < (uint32_t)PN_INV_BATCH ? n - first : (uint32_t)PN_INV_BATCH;
  store_affine_batch(src, dst, first, cnt);
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
  hipError_t upload(const void* host, uint64_t bytes) {
    hipError_t e = alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

inline unsigned blocks64(uint64_t n) { return (unsigned)((n + 63) / 64); }

// canonical words of a Montgomery-form scalar
void fr_words(const Fr& mont, uint32_t k[8]) {
  const Fr c = mont.from_mont();
  memcpy(k, c.l, 32);
}
}  // namespace

hipError_t points_ntt_twiddles(uint32_t log_n, uint32_t** d_tw) {
  const uint64_t cnt = log_n ? (1ull << (log_n - 1)) : 1;
  std::vector<uint32_t> tw(cnt * 8);
  Fr w = Fr::one(), run = Fr::one();
  if (log_n) w = fr_root_of_unity((int)log_n);
  for (uint64_t k = 0; k < cnt; k++) {
    fr_words(run, &tw[k * 8]);
    run = run * w;
  }
  hipError_t e = hipMalloc(d_tw, 32 * cnt);
  if (e != hipSuccess) return e;
  return hipMemcpy(*d_tw, tw.data(), 32 * cnt, hipMemcpyHostToDevice);
}

template <class F>
hipError_t points_ntt_resident(zkmi_ctx* ctx, Affine<F>* d_pts, uint64_t stride, uint32_t count, uint32_t log_n,
                               bool inverse, const uint32_t* d_tw) {
  hipStream_t st = ctx->stream;
  const uint64_t n = 1ull << log_n;
  hipError_t e;
  DevBuf work, d_scale;
  if ((e = work.alloc(sizeof(XYZZ<F>) * n * count)) != hipSuccess) return e;
  if (inverse && log_n) {
    Fr nf = Fr::zero();
    nf.l[0] = (uint32_t)n;
    uint32_t k[8];
    fr_words(nf.to_mont().inv(), k);
    if ((e = d_scale.upload(k, 32)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_pn_load<F>, dim3(blocks64(n), count), dim3(64), 0, st, d_pts, stride, work.as<XYZZ<F>>(), log_n,
                     d_scale.as<uint32_t>());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (uint32_t s = 0; s < log_n; s++) {
    hipLaunchKernelGGL(k_pn_level<F>, dim3(blocks64(n / 2), count), dim3(64), 0, st, work.as<XYZZ<F>>(), d_tw, log_n, s,
                       inverse ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_pn_store<F>, dim3(blocks64((n + PN_INV_BATCH - 1) / PN_INV_BATCH), count), dim3(64), 0, st,
                     work.as<XYZZ<F>>(), d_pts, stride, log_n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}
template hipError_t points_ntt_resident<Fq>(zkmi_ctx*, G1Affine*, uint64_t, uint32_t, uint32_t, bool, const uint32_t*);
template hipError_t points_ntt_resident<Fq2>(zkmi_ctx*, G2Affine*, uint64_t, uint32_t, uint32_t, bool, const uint32_t*);

}  // namespace zkmi

using namespace zkmi;

static int32_t points_ntt_dev(zkmi_ctx* ctx, int group, void* d_points, uint32_t log_n, int32_t inverse) {
  if (!ctx || !d_points || log_n > 26 || (reinterpret_cast<uintptr_t>(d_points) & 3u)) return ZKMI_ERR_BAD_ARG;
  ZK_ENTER(ctx);
  const uint64_t n = 1ull << log_n;
  DevBuf res, tw;
  ZK_HIP(ctx, res.alloc((group == 1 ? sizeof(G1Affine) : sizeof(G2Affine)) * n));
  uint64_t bad = UINT64_MAX;
  uint32_t stt = 0;
  int32_t rc = points_read(ctx, group, d_points, n, ZKMI_ENC_WIRE, 0, res.p, true, nullptr, &bad, &stt);
  if (rc != ZKMI_OK) return rc;
  if (bad != UINT64_MAX) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "point " + std::to_string(bad) + ": " + point_status_name(stt));
  uint32_t* d_tw = nullptr;
  ZK_HIP(ctx, points_ntt_twiddles(log_n, &d_tw));
  tw.p = d_tw;
  if (group == 1) ZK_HIP(ctx, points_ntt_resident<Fq>(ctx, res.as<G1Affine>(), n, 1, log_n, inverse != 0, d_tw));
  else ZK_HIP(ctx, points_ntt_resident<Fq2>(ctx, res.as<G2Affine>(), n, 1, log_n, inverse != 0, d_tw));
  return points_read(ctx, group, res.p, n, PT_ENC_RESIDENT, 0, d_points, false, nullptr, &bad, &stt);
}

// one section of a transcript: host bytes -> resident points, checked on the device
static int32_t srs_section(zkmi_ctx* ctx, int section, int group, const uint8_t* host, uint64_t n, int32_t enc, int32_t checks,
                           void** d_out, uint64_t where[2]) {
  static const char* const NAME[5] = {"tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"};
  ZK_HIP(ctx, hipMalloc(d_out, (group == 1 ? sizeof(G1Affine) : sizeof(G2Affine)) * n));
  uint64_t bad = UINT64_MAX;
  uint32_t stt = 0;
  const int32_t rc = points_read_host(ctx, group, host, n, enc, checks, *d_out, &bad, &stt);
  if (rc != ZKMI_OK) return rc;
  if (bad != UINT64_MAX) {
    if (where) where[0] = (uint64_t)section, where[1] = bad;
    return ctx->fail(ZKMI_ERR_NON_CANONICAL, std::string("transcript: ") + NAME[section] + "[" + std::to_string(bad) + "]: " +
                                                 point_status_name(stt));
  }
  return ZKMI_OK;
}

extern "C" {

int32_t zkmi_g1_points_ntt_dev(zkmi_ctx* ctx, void* d_points, uint32_t log_n, int32_t inverse) {
  return points_ntt_dev(ctx, 1, d_points, log_n, inverse);
}
int32_t zkmi_g2_points_ntt_dev(zkmi_ctx* ctx, void* d_points, uint32_t log_n, int32_t inverse) {
  return points_ntt_dev(ctx, 2, d_points, log_n, inverse);
}

int32_t zkmi_srs_load(zkmi_ctx* ctx, int32_t encoding, int32_t checks, const uint8_t* tau_g1, uint64_t n_tau_g1,
                      const uint8_t* tau_g2, uint64_t n_tau_g2, const uint8_t* alpha_tau_g1, const uint8_t* beta_tau_g1,
                      uint64_t n_ab, const uint8_t* beta_g2, zkmi_srs** out, uint64_t out_where[2]) {
  if (out) *out = nullptr;
  if (out_where) out_where[0] = out_where[1] = UINT64_MAX;
  if (!ctx || !tau_g1 || !tau_g2 || !alpha_tau_g1 || !beta_tau_g1 || !beta_g2 || !out || !n_tau_g1 || !n_tau_g2 || !n_ab ||
      encoding == PT_ENC_RESIDENT || !point_args_ok(encoding, &checks))
    return ZKMI_ERR_BAD_ARG;
  ZK_ENTER(ctx);
  zkmi_srs* s = new (std::nothrow) zkmi_srs();
  if (!s) return ZKMI_ERR_BAD_ARG;
  s->ctx = ctx;
  s->device = ctx->device;
  s->n_tau_g1 = n_tau_g1, s->n_tau_g2 = n_tau_g2, s->n_ab = n_ab;
  s->checks = checks;  // with the implied bits (point_args_ok)
  void* d_beta = nullptr;
  int32_t rc = srs_section(ctx, 0, 1, tau_g1, n_tau_g1, encoding, checks, reinterpret_cast<void**>(&s->tau_g1), out_where);
  if (rc == ZKMI_OK) rc = srs_section(ctx, 1, 2, tau_g2, n_tau_g2, encoding, checks, reinterpret_cast<void**>(&s->tau_g2), out_where);
  if (rc == ZKMI_OK) rc = srs_section(ctx, 2, 1, alpha_tau_g1, n_ab, encoding, checks, reinterpret_cast<void**>(&s->alpha_tau_g1), out_where);
  if (rc == ZKMI_OK) rc = srs_section(ctx, 3, 1, beta_tau_g1, n_ab, encoding, checks, reinterpret_cast<void**>(&s->beta_tau_g1), out_where);
  if (rc == ZKMI_OK) rc = srs_section(ctx, 4, 2, beta_g2, 1, encoding, checks, &d_beta, out_where);
  G1Affine first1;
  G2Affine first2;
  hipError_t e = hipSuccess;
  if (rc == ZKMI_OK) e = hipMemcpy(&s->beta_g2, d_beta, sizeof(G2Affine), hipMemcpyDeviceToHost);
  if (rc == ZKMI_OK && e == hipSuccess) e = hipMemcpy(&first1, s->tau_g1, sizeof(G1Affine), hipMemcpyDeviceToHost);
  if (rc == ZKMI_OK && e == hipSuccess) e = hipMemcpy(&first2, s->tau_g2, sizeof(G2Affine), hipMemcpyDeviceToHost);
  if (d_beta) (void)hipFree(d_beta);
  if (rc == ZKMI_OK && e != hipSuccess) rc = ctx->hip_fail(e, "transcript read-back");
  if (rc == ZKMI_OK) {
    const G1Affine g1 = g1_generator();
    const G2Affine g2 = g2_generator();
    const bool ok1 = first1.x == g1.x && first1.y == g1.y;
    const bool ok2 = first2.x.c0 == g2.x.c0 && first2.x.c1 == g2.x.c1 && first2.y.c0 == g2.y.c0 && first2.y.c1 == g2.y.c1;
    if (!ok1 || !ok2) {
      if (out_where) out_where[0] = ok1 ? 1 : 0, out_where[1] = 0;
      rc = ctx->fail(ZKMI_ERR_NON_CANONICAL, ok1 ? "transcript: tau_g2[0] is not the G2 generator" : "transcript: tau_g1[0] is not the G1 generator");
    }
  }
  if (rc != ZKMI_OK) {
    delete s;
    return rc;
  }
  *out = s;
  return ZKMI_OK;
}

int32_t zkmi_srs_generate(zkmi_ctx* ctx, const uint8_t toxic[96], uint32_t log_n, zkmi_srs** out) {
  if (out) *out = nullptr;
  if (!ctx || !toxic || !out || log_n > 26) return ZKMI_ERR_BAD_ARG;
  ZK_ENTER(ctx);
  Fr tau, alpha, beta;
  if (!fr_from_wire(toxic, &tau) || !fr_from_wire(toxic + 32, &alpha) || !fr_from_wire(toxic + 64, &beta))
    return ctx->fail(ZKMI_ERR_NON_CANONICAL, "toxic waste >= r");
  const uint64_t N = 1ull << log_n, n1 = 2 * N - 1;
  zkmi_srs* s = new (std::nothrow) zkmi_srs();
  if (!s) return ZKMI_ERR_BAD_ARG;
  s->ctx = ctx;
  s->device = ctx->device;
  s->n_tau_g1 = n1, s->n_tau_g2 = N, s->n_ab = N;
  s->checks = ZKMI_CHECK_CURVE | ZKMI_CHECK_SUBGROUP;  // multiples of the generators
  std::vector<Fr> p(n1), pa(N), pb(N);
  Fr run = Fr::one();
  for (uint64_t i = 0; i < n1; i++) {
    p[i] = run;
    if (i < N) pa[i] = run * alpha, pb[i] = run * beta;
    run = run * tau;
  }
  G1Affine* t1 = nullptr;
  G2Affine* t2 = nullptr;
  const G1Affine g1 = g1_generator();
  const G2Affine g2 = g2_generator();
  hipError_t e = hipMalloc(&s->tau_g1, sizeof(G1Affine) * n1);
  if (e == hipSuccess) e = hipMalloc(&s->alpha_tau_g1, sizeof(G1Affine) * N);
  if (e == hipSuccess) e = hipMalloc(&s->beta_tau_g1, sizeof(G1Affine) * N);
  if (e == hipSuccess) e = hipMalloc(&s->tau_g2, sizeof(G2Affine) * N);
  if (e == hipSuccess) e = fixed_base_table<Fq>(g1, &t1);
  if (e == hipSuccess) e = fixed_base_table<Fq2>(g2, &t2);
  if (e == hipSuccess) e = fixed_base_batch<Fq>(ctx, t1, p, s->tau_g1);
  if (e == hipSuccess) e = fixed_base_batch<Fq>(ctx, t1, pa, s->alpha_tau_g1);
  if (e == hipSuccess) e = fixed_base_batch<Fq>(ctx, t1, pb, s->beta_tau_g1);
  p.resize(N);
  if (e == hipSuccess) e = fixed_base_batch<Fq2>(ctx, t2, p, s->tau_g2);
  if (t1) (void)hipFree(t1);
  if (t2) (void)hipFree(t2);
  if (e != hipSuccess) {
    delete s;
    return ctx->hip_fail(e, "srs generate");
  }
  uint32_t k[8];
  fr_words(beta, k);
  s->beta_g2 = scalar_mul(G2XYZZ::from_affine(g2), k, 8).to_affine();
  *out = s;
  return ZKMI_OK;
}

// Where the toxic waste lives during the call, and where it ends:
//   `sec` below     the Montgomery forms of s, a, b and the canonical words handed to the host scalar multiplications;
//                   its destructor overwrites the whole struct on every return path
//   pw (HBM)        the n powers c s^i of the array being multiplied, reused for the three weights 1, a, b; overwritten
//                   with zeros (wipe_dev, then a stream wait) before the buffer is freed, on the error paths as well
//   fr_powers_dev   the table c | s^(2^t) in pinned host memory and in HBM: wiped inside that call (points_mul.hip)
// Not reachable from here: registers and scratch of the kernels, which the next launch overwrites.
int32_t zkmi_srs_contribute(zkmi_ctx* ctx, zkmi_srs* srs, const uint8_t sab[96], uint8_t out_step_g2[576]) {
  ZK_ENTER(ctx);
  if (!srs || !sab || !out_step_g2) return ZKMI_ERR_BAD_ARG;
  if (srs->ctx != ctx || srs->device != ctx->device) return ctx->fail(ZKMI_ERR_BAD_ARG, "transcript of another context");
  struct Secrets {
    Fr s, a, b;
    uint32_t k[8];
    ~Secrets() { wipe_host(this, sizeof(*this)); }
  } sec;
  if (!fr_from_wire(sab, &sec.s) || !fr_from_wire(sab + 32, &sec.a) || !fr_from_wire(sab + 64, &sec.b))
    return ctx->fail(ZKMI_ERR_NON_CANONICAL, "contribution >= r");
  if (sec.s.is_zero() || sec.a.is_zero() || sec.b.is_zero()) return ctx->fail(ZKMI_ERR_BAD_ARG, "contribution must be non-zero");
  ZK_HIP(ctx, ctx->drain());  // the transcript is idle: nothing queued earlier still reads its arrays
  points_mul_phases_reset();
  const uint64_t n1 = srs->n_tau_g1, n2 = srs->n_tau_g2, nab = srs->n_ab;
  const uint64_t n_pw = std::max(std::max(n1, n2), nab);
  // fresh arrays, swapped in at the end: a failure on the way leaves the transcript as it was
  DevBuf t1, t2, al, be, pw;
  ZK_HIP(ctx, t1.alloc(sizeof(G1Affine) * n1));
  ZK_HIP(ctx, t2.alloc(sizeof(G2Affine) * n2));
  ZK_HIP(ctx, al.alloc(sizeof(G1Affine) * nab));
  ZK_HIP(ctx, be.alloc(sizeof(G1Affine) * nab));
  ZK_HIP(ctx, pw.alloc(32 * n_pw));
  uint32_t* d_pw = pw.as<uint32_t>();
  int32_t rc = fr_powers_dev(ctx, Fr::one(), sec.s, std::max(n1, n2), d_pw);
  if (rc == ZKMI_OK) rc = points_mul_each_resident<Fq>(ctx, srs->tau_g1, d_pw, n1, t1.as<G1Affine>());
  if (rc == ZKMI_OK) rc = points_mul_each_resident<Fq2>(ctx, srs->tau_g2, d_pw, n2, t2.as<G2Affine>());
  if (rc == ZKMI_OK) rc = fr_powers_dev(ctx, sec.a, sec.s, nab, d_pw);
  if (rc == ZKMI_OK) rc = points_mul_each_resident<Fq>(ctx, srs->alpha_tau_g1, d_pw, nab, al.as<G1Affine>());
  if (rc == ZKMI_OK) rc = fr_powers_dev(ctx, sec.b, sec.s, nab, d_pw);
  if (rc == ZKMI_OK) rc = points_mul_each_resident<Fq>(ctx, srs->beta_tau_g1, d_pw, nab, be.as<G1Affine>());
  const hipError_t ew = wipe_dev(pw.p, 32 * n_pw, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (rc != ZKMI_OK) return rc;
  ZK_HIP(ctx, ew);
  ZK_HIP(ctx, es);
  // the single elements on the host: b beta_g2 and the three step elements
  const G2XYZZ g2 = G2XYZZ::from_affine(g2_generator());
  const Fr* const step[3] = {&sec.s, &sec.a, &sec.b};
  for (int j = 0; j < 3; j++) {
    fr_words(*step[j], sec.k);
    g2_to_wire(scalar_mul(g2, sec.k, 8).to_affine(), out_step_g2 + 192 * j);
  }
  srs->beta_g2 = scalar_mul(G2XYZZ::from_affine(srs->beta_g2), sec.k, 8).to_affine();  // sec.k holds b
  auto swap_in = [](auto*& held, DevBuf& fresh) {  // the old array goes with the DevBuf
    void* old = held;
    held = static_cast<std::remove_reference_t<decltype(held)>>(fresh.p);
    fresh.p = old;
  };
  swap_in(srs->tau_g1, t1);
  swap_in(srs->tau_g2, t2);
  swap_in(srs->alpha_tau_g1, al);
  swap_in(srs->beta_tau_g1, be);
  return ZKMI_OK;
}

int32_t zkmi_srs_shape(const zkmi_srs* s, uint64_t out[3]) {
  if (!s || !out) return ZKMI_ERR_BAD_ARG;
  out[0] = s->n_tau_g1, out[1] = s->n_tau_g2, out[2] = s->n_ab;
  return ZKMI_OK;
}

int32_t zkmi_srs_read(zkmi_ctx* ctx, const zkmi_srs* s, int32_t section, uint64_t first, uint64_t count, uint8_t* out_wire) {
  if (!ctx || !s || !out_wire || section < 0 || section > 4) return ZKMI_ERR_BAD_ARG;
  ZK_ENTER(ctx);
  if (ctx->device != s->device) return ZKMI_ERR_BAD_ARG;
  const uint64_t len = section == 0 ? s->n_tau_g1 : section == 1 ? s->n_tau_g2 : section == 4 ? 1 : s->n_ab;
  if (first > len || count > len - first) return ZKMI_ERR_BAD_ARG;
  if (section == 4) {
    if (count) g2_to_wire(s->beta_g2, out_wire);
    return ZKMI_OK;
  }
  if (section == 1) {
    std::vector<G2Affine> h(count);
    ZK_HIP(ctx, hipMemcpy(h.data(), s->tau_g2 + first, sizeof(G2Affine) * count, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < count; i++) g2_to_wire(h[i], out_wire + 192 * i);
    return ZKMI_OK;
  }
  const G1Affine* src = section == 0 ? s->tau_g1 : section == 2 ? s->alpha_tau_g1 : s->beta_tau_g1;
  std::vector<G1Affine> h(count);
  ZK_HIP(ctx, hipMemcpy(h.data(), src + first, sizeof(G1Affine) * count, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < count; i++) g1_to_wire(h[i], out_wire + 96 * i);
  return ZKMI_OK;
}

int32_t zkmi_srs_free(zkmi_srs* s) {
  if (!s) return ZKMI_ERR_BAD_ARG;
  delete s;
  return ZKMI_OK;
}

}  // extern "C"
