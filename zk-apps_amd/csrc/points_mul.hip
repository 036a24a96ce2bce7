// zkmi — every point of an array times a scalar of its own: out[i] = k[i] * P[i] (zkmi_g{1,2}_points_mul_each_dev), and
// the same with k[i] = c * q^i made on the device (zkmi_g{1,2}_points_mul_powers_dev): the arithmetic of a phase-1
// contribution.
//
// Kernels (one lane per item; F = Fq for G1 and Fq2 for G2, the 32-bit-limb fields and the out-of-line group operations of
// group_dev.hpp: a lane spends its time inside g_dbl / g_add, which the point transforms already run on, and the resident
// form is read and written as it is; the 28-bit forms of the MSM would need a conversion both ways, and their group
// operations are bodies inlined into the accumulation kernels, not functions a second kernel can share):
//   k_scalars_check   one lane per scalar: >= r raises the status word
//   k_fr_powers       one lane per chunk of FR_POWERS_CHUNK indices: c * q^first from the table of q^(2^t), then the
//                     chunk by one product per index
//   k_points_mul      one lane per point, a fixed SIGNED window of PM_WINDOW = 4 bits: k = sum d_j 16^j, -8 <= d_j <= 8,
//                     64 digits.  The lane writes P .. 8P to its own column of an HBM workspace (one doubling, six mixed
//                     additions), then runs 64 rounds of four doublings and one addition of +-|d_j| P, the entry selected
//                     by address and negated by a word-wise select.  The only branch on the scalar skips a zero digit.
//                     Every addition is the complete one (curve.hpp add / madd, by case analysis): with small scalars
//                     and infinity inputs the accumulator does meet +-(table entry) and infinity, and no incomplete
//                     formula is used anywhere in this file.
//   k_points_mul_plain  A/B library only (ZKMI_POINTS_MUL_PLAIN=1): one lane per point around mul_words, the yardstick
//   k_pm_store        XYZZ -> resident affine through store_affine_batch (four points per inversion)
//
// Nothing waits.  No lane reads what another lane of the same launch writes: a lane's table column is written and read by
// that lane alone.  There are no atomics, flags or counters in memory and no cross-lane or cross-workgroup operations.
// Every loop count is a constant (64 digits, 4 doublings, 8 table entries, 40 table bits) or a host-passed value that is
// range-checked before the loop (a chunk's count <= FR_POWERS_CHUNK): an out-of-range value ends the lane and raises a
// status word nothing reads inside a launch.  The only ordering is launch order on ctx->stream.
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include "group_dev.hpp"
#include "points.hpp"
#include "points_mul.hpp"
#include "tune.hpp"

namespace zkmi {

namespace {

constexpr uint32_t PM_TABLE = 1u << (PM_WINDOW - 1);           // |d| = 1 .. 8
constexpr uint32_t PM_DIGITS = (256 + PM_WINDOW - 1) / PM_WINDOW;  // 64
constexpr uint32_t PW_BITS = 40;                                // indices below 2^40
constexpr uint64_t PM_SLICE = 1ull << 18;                       // lanes per launch: bounds the table workspace
static_assert(PM_WINDOW == 4, "the digit extraction below reads nibbles");

// the group operations of a body: the out-of-line device functions on the device, the methods themselves on the host
template <class F>
__host__ __device__ inline void pm_dbl(XYZZ<F>* a) {
#ifdef __HIP_DEVICE_COMPILE__
  g_dbl(a);
#else
  a->dbl_inplace();
#endif
}
template <class F>
__host__ __device__ inline void pm_add(XYZZ<F>* a, const XYZZ<F>* o) {
#ifdef __HIP_DEVICE_COMPILE__
  g_add(a, o);
#else
  a->add(*o);
#endif
}
template <class F>
__host__ __device__ inline void pm_madd(XYZZ<F>* a, const Affine<F>* p) {
#ifdef __HIP_DEVICE_COMPILE__
  g_madd(a, p);
#else
  a->madd(*p);
#endif
}
template <class T>
__host__ __device__ inline T pm_load(const T* p) {
#ifdef __HIP_DEVICE_COMPILE__
  return ldv(p);
#else
  return *p;
#endif
}
template <class T>
__host__ __device__ inline void pm_store(T* p, const T& v) {
#ifdef __HIP_DEVICE_COMPILE__
  stv(p, v);
#else
  *p = v;
#endif
}

// pick ? b : a, word by word: no branch
template <class F>
__host__ __device__ inline F pm_select(const F& a, const F& b, bool pick) {
  static_assert(sizeof(F) % 4 == 0, "fields are arrays of 32-bit words");
  F r;
  const uint32_t* pa = reinterpret_cast<const uint32_t*>(&a);
  const uint32_t* pb = reinterpret_cast<const uint32_t*>(&b);
  uint32_t* pr = reinterpret_cast<uint32_t*>(&r);
  const uint32_t m = pick ? 0xffffffffu : 0u;
#pragma unroll
  for (unsigned i = 0; i < sizeof(F) / 4; i++) pr[i] = (pa[i] & ~m) | (pb[i] & m);
  return r;
}

__host__ __device__ inline uint32_t pm_nibble(const uint32_t k[8], uint32_t j) { return (k[j >> 3] >> ((j & 7u) * 4u)) & 15u; }

// acc = k * p for a canonical scalar k < r < 2^255.  tab: PM_TABLE entries of this lane, entry e at tab[e * stride].
//
// Recoding: v_j = nibble_j + carry_j; v_j > 8 gives the digit v_j - 16 and carry_{j+1} = 1, else the digit v_j.  The top
// nibble of k is at most 7, so v_63 <= 8 and no carry leaves the top.  The carries are found from the bottom up first (64
// steps of integer work, two words of state); the digits are then consumed from the top down.
template <class F>
__host__ __device__ inline void points_mul_body(const Affine<F>& p, const uint32_t k[8], XYZZ<F>* tab, size_t stride, XYZZ<F>* acc) {
  // the lane's multiples P, 2P, .. 8P.  madd is complete: P = infinity gives eight infinities, and (e)P + P never doubles
  // for a point of odd prime order, but would be handled if it did.
  XYZZ<F> t = XYZZ<F>::from_affine(p);
  pm_store(tab, t);
  pm_dbl(&t);
  pm_store(tab + stride, t);
#pragma unroll 1
  for (uint32_t e = 2; e < PM_TABLE; e++) {
    pm_madd(&t, &p);
    pm_store(tab + (size_t)e * stride, t);
  }
  uint32_t cin[2] = {0, 0};  // bit j: the carry into nibble j
  uint32_t c = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < PM_DIGITS; j++) {
    cin[j >> 5] |= c << (j & 31u);
    c = (pm_nibble(k, j) + c) > PM_TABLE ? 1u : 0u;
  }
  *acc = XYZZ<F>::infinity();
#pragma unroll 1
  for (uint32_t j = PM_DIGITS; j-- > 0;) {
#pragma unroll 1
    for (uint32_t d = 0; d < PM_WINDOW; d++) pm_dbl(acc);
    const uint32_t v = pm_nibble(k, j) + ((cin[j >> 5] >> (j & 31u)) & 1u);  // 0 .. 16
    const bool neg = v > PM_TABLE;
    const uint32_t mag = neg ? 16u - v : v;  // 0 .. 8
    if (mag) {                                // the one branch on the scalar: a zero digit adds nothing
      XYZZ<F> o = pm_load(tab + (size_t)(mag - 1u) * stride);
      o.y = pm_select(o.y, o.y.neg(), neg);
      pm_add(acc, &o);
    }
  }
}

// pw[0] = c, pw[1 + t] = q^(2^t) for t < PW_BITS (Montgomery form).  out[8 m .. 8 m + 8) = the canonical words of
// c * q^(first + m) for m < count.  Returns non-zero, with nothing written, for a count or an index out of range.
__host__ __device__ inline uint32_t fr_powers_body(const Fr* pw, uint64_t first, uint32_t count, uint32_t* out) {
  if (count > FR_POWERS_CHUNK || (first >> PW_BITS) != 0) return 1u;
  Fr acc = pw[0];
#pragma unroll 1
  for (uint32_t t = 0; t < PW_BITS; t++)
    if ((first >> t) & 1u) acc = acc * pw[1 + t];
  const Fr q = pw[1];
#pragma unroll 1
  for (uint32_t m = 0; m < count; m++) {
    const Fr cn = acc.from_mont();
#pragma unroll
    for (int w = 0; w < 8; w++) out[8 * (size_t)m + w] = cn.l[w];
    acc = acc * q;
  }
  return 0u;
}

__global__ void __launch_bounds__(64) k_fr_powers(const Fr* __restrict__ pw, uint64_t n, uint32_t* __restrict__ out,
                                                  uint32_t* __restrict__ status) {
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * FR_POWERS_CHUNK;
  if (first >= n) return;
  const uint32_t count = n - first < FR_POWERS_CHUNK ? (uint32_t)(n - first) : FR_POWERS_CHUNK;
  if (fr_powers_body(pw, first, count, out + 8 * first)) *status = 1u;
}

// scalar i >= r: the status word is raised (every lane that raises it stores the same value)
__global__ void __launch_bounds__(256) k_scalars_check(const uint32_t* __restrict__ k, uint64_t n, uint32_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool below = false;  // k < r, decided at the highest word that differs
#pragma unroll
  for (int w = 7; w >= 0; w--) {
    const uint32_t v = k[8 * i + w], m = FrParams::MOD[w];
    if (v != m) {
      below = v < m;
      break;
    }
  }
  if (!below) *status = 1u;
}

template <class F>
__global__ void __launch_bounds__(64)
k_points_mul(const Affine<F>* __restrict__ in, const uint32_t* __restrict__ k, uint32_t n, XYZZ<F>* __restrict__ tab,
             XYZZ<F>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kw[8];
#pragma unroll
  for (int w = 0; w < 8; w++) kw[w] = k[8 * (size_t)i + w];
  const Affine<F> p = ldv(in + i);
  XYZZ<F> acc;
  points_mul_body(p, kw, tab + i, (size_t)n, &acc);
  stv(out + i, acc);
}

#ifdef ZKMI_EXPERIMENTS
// the yardstick: the bit-by-bit double-and-add of the point transforms, one lane per point
template <class F>
__global__ void __launch_bounds__(64)
k_points_mul_plain(const Affine<F>* __restrict__ in, const uint32_t* __restrict__ k, uint32_t n, XYZZ<F>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = ldv(in + i);
  XYZZ<F> acc;
  mul_words(&p, k + 8 * (size_t)i, &acc);
  stv(out + i, acc);
}
int g_plain_override = -1;
bool use_plain_kernel() { return g_plain_override >= 0 ? g_plain_override != 0 : ZK_TUNE("ZKMI_POINTS_MUL_PLAIN", 0) != 0; }
#endif

template <class F>
__global__ void __launch_bounds__(64) k_pm_store(const XYZZ<F>* __restrict__ src, Affine<F>* __restrict__ dst, uint32_t n) {
  const uint32_t first = (blockIdx.x * blockDim.x + threadIdx.x) * PN_INV_BATCH;
  if (first >= n) return;
  store_affine_batch(src, dst, first, n - first < (uint32_t)PN_INV_BATCH ? n - first : (uint32_t)PN_INV_BATCH);
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

inline unsigned blocks_of(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

// Where the multiplications spend their time (testing library only: zkmi_points_mul_phases): the host clock at points
// where the stream is waited for; the product library compiles lap() to nothing and adds no synchronisation.
#ifdef ZKMI_TESTING
double g_pm_ms[4] = {0, 0, 0, 0};
struct PmLog {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(zkmi_ctx* ctx, int k) {
    (void)hipStreamSynchronize(ctx->stream);
    const auto t = std::chrono::steady_clock::now();
    g_pm_ms[k] += std::chrono::duration<double, std::milli>(t - t0).count();
    t0 = t;
  }
};
#else
struct PmLog {
  void lap(zkmi_ctx*, int) {}
};
#endif

template <class F>
struct GroupOf;
template <>
struct GroupOf<Fq> {
  static constexpr int G = 1;
};
template <>
struct GroupOf<Fq2> {
  static constexpr int G = 2;
};

// n canonical scalars in HBM: ZKMI_OK with *bad = whether one of them is >= r
int32_t scalars_check_dev(zkmi_ctx* ctx, const uint32_t* d_k, uint64_t n, bool* bad) {
  hipStream_t st = ctx->stream;
  DevBuf d_status;
  ZK_HIP(ctx, d_status.alloc(sizeof(uint32_t)));
  ZK_HIP(ctx, hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_scalars_check, dim3(blocks_of(n, 256)), dim3(256), 0, st, d_k, n, d_status.as<uint32_t>());
  ZK_HIP(ctx, hipGetLastError());
  uint32_t status = 0;
  ZK_HIP(ctx, hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  ZK_HIP(ctx, hipStreamSynchronize(st));
  *bad = status != 0;
  return ZKMI_OK;
}

}  // namespace

void wipe_host(void* p, size_t bytes) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < bytes; i++) v[i] = 0;
}

hipError_t wipe_dev(void* d, uint64_t bytes, hipStream_t st) { return (d && bytes) ? hipMemsetAsync(d, 0, bytes, st) : hipSuccess; }

void points_mul_phases_reset() {
#ifdef ZKMI_TESTING
  for (double& v : g_pm_ms) v = 0;
#endif
}

template <class F>
int32_t points_mul_each_resident(zkmi_ctx* ctx, const Affine<F>* d_in, const uint32_t* d_k, uint64_t n, Affine<F>* d_out) {
  if (!n) return ZKMI_OK;
  if (n > PM_MAX_POINTS) return ctx->fail(ZKMI_ERR_BAD_ARG, "point multiplication: too many points");
  hipStream_t st = ctx->stream;
  PmLog log;
  const uint64_t slice = n < PM_SLICE ? n : PM_SLICE;
  bool plain = false;
#ifdef ZKMI_EXPERIMENTS
  plain = use_plain_kernel();
#endif
  DevBuf work, tab;
  ZK_HIP(ctx, work.alloc(sizeof(XYZZ<F>) * n));
  if (!plain) ZK_HIP(ctx, tab.alloc(sizeof(XYZZ<F>) * PM_TABLE * slice));
  log.lap(ctx, 3);
  for (uint64_t first = 0; first < n; first += slice) {
    const uint32_t cnt = (uint32_t)(n - first < slice ? n - first : slice);
#ifdef ZKMI_EXPERIMENTS
    if (plain) {
      hipLaunchKernelGGL(k_points_mul_plain<F>, dim3(blocks_of(cnt, 64)), dim3(64), 0, st, d_in + first, d_k + 8 * first, cnt,
                         work.as<XYZZ<F>>() + first);
      ZK_HIP(ctx, hipGetLastError());
      continue;
    }
#endif
    hipLaunchKernelGGL(k_points_mul<F>, dim3(blocks_of(cnt, 64)), dim3(64), 0, st, d_in + first, d_k + 8 * first, cnt,
                       tab.as<XYZZ<F>>(), work.as<XYZZ<F>>() + first);
    ZK_HIP(ctx, hipGetLastError());
  }
  log.lap(ctx, GroupOf<F>::G);
  hipLaunchKernelGGL(k_pm_store<F>, dim3(blocks_of((n + PN_INV_BATCH - 1) / PN_INV_BATCH, 64)), dim3(64), 0, st, work.as<XYZZ<F>>(),
                     d_out, (uint32_t)n);
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, hipStreamSynchronize(st));  // the buffers go when this returns
  log.lap(ctx, 3);
  return ZKMI_OK;
}
template int32_t points_mul_each_resident<Fq>(zkmi_ctx*, const G1Affine*, const uint32_t*, uint64_t, G1Affine*);
template int32_t points_mul_each_resident<Fq2>(zkmi_ctx*, const G2Affine*, const uint32_t*, uint64_t, G2Affine*);

// The table pw (c and the q^(2^t): as secret as c and q themselves) lives in pinned host memory this call owns, so the copy
// engine reads it in place, and in one device buffer; both are overwritten with zeros before they are freed, on every path.
int32_t fr_powers_dev(zkmi_ctx* ctx, const Fr& c, const Fr& q, uint64_t n, uint32_t* d_out) {
  if (!n) return ZKMI_OK;
  if (n > PM_MAX_POINTS) return ctx->fail(ZKMI_ERR_BAD_ARG, "powers: too many indices");
  hipStream_t st = ctx->stream;
  PmLog log;
  constexpr size_t BYTES = sizeof(Fr) * (1 + PW_BITS);
  Fr* h_pw = nullptr;
  ZK_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&h_pw), BYTES, hipHostMallocDefault));
  h_pw[0] = c;
  h_pw[1] = q;
  for (uint32_t t = 1; t < PW_BITS; t++) h_pw[1 + t] = h_pw[t].sqr();
  DevBuf d_pw, d_status;
  uint32_t status = 0;
  hipError_t e = d_pw.alloc(BYTES);
  if (e == hipSuccess) e = d_status.alloc(sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_pw.p, h_pw, BYTES, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fr_powers, dim3(blocks_of((n + FR_POWERS_CHUNK - 1) / FR_POWERS_CHUNK, 64)), dim3(64), 0, st, d_pw.as<Fr>(), n,
                       d_out, d_status.as<uint32_t>());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  // the wipes run on the error paths too: after the stream has drained nothing reads the table any more
  const hipError_t ew = wipe_dev(d_pw.p, BYTES, st);
  const hipError_t es = hipStreamSynchronize(st);
  wipe_host(h_pw, BYTES);
  (void)hipHostFree(h_pw);
  if (e == hipSuccess) e = ew;
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return ctx->hip_fail(e, "powers of a scalar");
  if (status) return ctx->fail(ZKMI_ERR_HIP, "powers of a scalar: chunk out of range");
  log.lap(ctx, 0);
  return ZKMI_OK;
}

namespace {

template <class F>
int32_t mul_dev_checked_args(zkmi_ctx* ctx, const void* d_points, uint64_t n, DevBuf* res) {
  using A = Affine<F>;
  ZK_HIP(ctx, res->alloc(sizeof(A) * n));
  uint64_t bad = UINT64_MAX;
  uint32_t stt = 0;
  const int32_t rc = points_read(ctx, GroupOf<F>::G, d_points, n, ZKMI_ENC_WIRE, 0, res->p, true, nullptr, &bad, &stt);
  if (rc != ZKMI_OK) return rc;
  if (bad != UINT64_MAX) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "point " + std::to_string(bad) + ": " + point_status_name(stt));
  return ZKMI_OK;
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

template <class F>
int32_t mul_each_dev(zkmi_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out) {
  ZK_ENTER(ctx);
  if (!d_points || !d_scalars || !d_out || n == 0 || n > PM_MAX_POINTS || misaligned(d_points) || misaligned(d_scalars) ||
      misaligned(d_out))
    return ZKMI_ERR_BAD_ARG;
  using A = Affine<F>;
  DevBuf res;
  int32_t rc = mul_dev_checked_args<F>(ctx, d_points, n, &res);
  if (rc != ZKMI_OK) return rc;
  bool bad_scalar = false;
  const uint32_t* d_k = static_cast<const uint32_t*>(d_scalars);
  if ((rc = scalars_check_dev(ctx, d_k, n, &bad_scalar)) != ZKMI_OK) return rc;
  if (bad_scalar) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "a scalar >= r");
  if ((rc = points_mul_each_resident<F>(ctx, res.as<A>(), d_k, n, res.as<A>())) != ZKMI_OK) return rc;
  uint64_t bad = UINT64_MAX;
  uint32_t stt = 0;
  return points_read(ctx, GroupOf<F>::G, res.p, n, PT_ENC_RESIDENT, 0, d_out, false, nullptr, &bad, &stt);
}

// Secrets: the Montgomery forms of c and q on this frame and the n powers in HBM; both are overwritten before they go.
template <class F>
int32_t mul_powers_dev(zkmi_ctx* ctx, void* d_points, uint64_t n, const uint8_t c[32], const uint8_t q[32]) {
  ZK_ENTER(ctx);
  if (!d_points || !c || !q || n == 0 || n > PM_MAX_POINTS || misaligned(d_points)) return ZKMI_ERR_BAD_ARG;
  using A = Affine<F>;
  Fr cq[2];
  int32_t rc = ZKMI_OK;
  DevBuf res, d_k;
  if (!fr_from_wire(c, &cq[0]) || !fr_from_wire(q, &cq[1])) rc = ctx->fail(ZKMI_ERR_NON_CANONICAL, "scalar >= r");
  if (rc == ZKMI_OK) rc = mul_dev_checked_args<F>(ctx, d_points, n, &res);
  if (rc == ZKMI_OK) {
    const hipError_t e = d_k.alloc(32 * n);
    if (e != hipSuccess) rc = ctx->hip_fail(e, "powers: allocation");
  }
  if (rc == ZKMI_OK) rc = fr_powers_dev(ctx, cq[0], cq[1], n, d_k.as<uint32_t>());
  if (rc == ZKMI_OK) rc = points_mul_each_resident<F>(ctx, res.as<A>(), d_k.as<uint32_t>(), n, res.as<A>());
  wipe_host(cq, sizeof(cq));
  if (d_k.p) {
    (void)wipe_dev(d_k.p, 32 * n, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (rc != ZKMI_OK) return rc;
  uint64_t bad = UINT64_MAX;
  uint32_t stt = 0;
  return points_read(ctx, GroupOf<F>::G, res.p, n, PT_ENC_RESIDENT, 0, d_points, false, nullptr, &bad, &stt);
}

}  // namespace

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int32_t zkmi_g1_points_mul_each_dev(zkmi_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out) {
  return mul_each_dev<Fq>(ctx, d_points, d_scalars, n, d_out);
}
int32_t zkmi_g2_points_mul_each_dev(zkmi_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out) {
  return mul_each_dev<Fq2>(ctx, d_points, d_scalars, n, d_out);
}
int32_t zkmi_g1_points_mul_powers_dev(zkmi_ctx* ctx, void* d_points, uint64_t n, const uint8_t c[32], const uint8_t q[32]) {
  return mul_powers_dev<Fq>(ctx, d_points, n, c, q);
}
int32_t zkmi_g2_points_mul_powers_dev(zkmi_ctx* ctx, void* d_points, uint64_t n, const uint8_t c[32], const uint8_t q[32]) {
  return mul_powers_dev<Fq2>(ctx, d_points, n, c, q);
}

}  // extern "C"

#ifdef ZKMI_TESTING  // test scaffolding: libzkmi_exp.so only (include/zkmi_testing.h)
namespace {

template <class F>
void mul_each_host(const std::vector<Affine<F>>& pts, const uint8_t* scalars, std::vector<Affine<F>>* out) {
  std::vector<XYZZ<F>> tab(PM_TABLE);
  out->resize(pts.size());
  for (size_t i = 0; i < pts.size(); i++) {
    uint32_t k[8];
    memcpy(k, scalars + 32 * i, 32);
    XYZZ<F> acc;
    points_mul_body(pts[i], k, tab.data(), 1, &acc);
    (*out)[i] = acc.to_affine();
  }
}

}  // namespace

extern "C" {

int32_t zkmi_selftest_points_mul_each_host(int32_t group, const uint8_t* wire_points, const uint8_t* scalars, uint64_t n,
                                           uint8_t* out_wire) {
  if ((group != 1 && group != 2) || !wire_points || !scalars || !out_wire || n == 0 || n > (1u << 20)) return ZKMI_ERR_BAD_ARG;
  for (uint64_t i = 0; i < n; i++)
    if (!fr_is_canonical(scalars + 32 * i)) return ZKMI_ERR_NON_CANONICAL;
  if (group == 1) {
    std::vector<G1Affine> pts(n), out;
    for (uint64_t i = 0; i < n; i++)
      if (!g1_from_wire(wire_points + 96 * i, &pts[i], false)) return ZKMI_ERR_NON_CANONICAL;
    mul_each_host<Fq>(pts, scalars, &out);
    for (uint64_t i = 0; i < n; i++) g1_to_wire(out[i], out_wire + 96 * i);
  } else {
    std::vector<G2Affine> pts(n), out;
    for (uint64_t i = 0; i < n; i++)
      if (!g2_from_wire(wire_points + 192 * i, &pts[i], false)) return ZKMI_ERR_NON_CANONICAL;
    mul_each_host<Fq2>(pts, scalars, &out);
    for (uint64_t i = 0; i < n; i++) g2_to_wire(out[i], out_wire + 192 * i);
  }
  return ZKMI_OK;
}

int32_t zkmi_selftest_fr_powers_host(const uint8_t c[32], const uint8_t q[32], uint64_t first, uint64_t count, uint8_t* out) {
  if (!c || !q || (count && !out) || first + count < first || first + count > (1ull << PW_BITS)) return ZKMI_ERR_BAD_ARG;
  Fr pw[1 + PW_BITS];
  if (!fr_from_wire(c, &pw[0]) || !fr_from_wire(q, &pw[1])) return ZKMI_ERR_NON_CANONICAL;
  for (uint32_t t = 1; t < PW_BITS; t++) pw[1 + t] = pw[t].sqr();
  uint64_t done = 0;
  while (done < count) {  // cut at the multiples of the chunk, as the kernel's lanes are
    const uint64_t at = first + done, to_edge = FR_POWERS_CHUNK - at % FR_POWERS_CHUNK;
    const uint32_t take = (uint32_t)(count - done < to_edge ? count - done : to_edge);
    uint32_t words[8 * FR_POWERS_CHUNK];
    if (fr_powers_body(pw, at, take, words)) return ZKMI_ERR_BAD_ARG;
    memcpy(out + 32 * done, words, 32 * (size_t)take);
    done += take;
  }
  return ZKMI_OK;
}

int32_t zkmi_selftest_points_mul_shape(uint32_t* out_chunk, uint32_t* out_window) {
  if (!out_chunk || !out_window) return ZKMI_ERR_BAD_ARG;
  *out_chunk = FR_POWERS_CHUNK, *out_window = PM_WINDOW;
  return ZKMI_OK;
}

int32_t zkmi_points_mul_kernel(int32_t which) {
  if (which < -1 || which > 1) return ZKMI_ERR_BAD_ARG;
  g_plain_override = which;
  return ZKMI_OK;
}

int32_t zkmi_points_mul_phases(double out_ms[4], int32_t reset) {
  if (!out_ms) return ZKMI_ERR_BAD_ARG;
  for (int k = 0; k < 4; k++) out_ms[k] = g_pm_ms[k];
  if (reset) points_mul_phases_reset();
  return ZKMI_OK;
}

}  // extern "C"
#endif  // ZKMI_TESTING
