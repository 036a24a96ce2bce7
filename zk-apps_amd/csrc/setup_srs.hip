// zkmi — the circuit-specific step of a Groth16 setup that never sees the toxic waste: the five queries of a relation's
// key from a phase-1 transcript, gamma = delta = 1.
//
// The specification is oracle/groth16.py setup() with gamma = delta = 1, taken "in the exponent" over the transcript's
// points.
//
//   Lagrange bases   the first N points of tau_g1 | alpha_tau_g1 | beta_tau_g1 (one chain) and of tau_g2, copied to scratch
//                    and run through the inverse point transform (points_ntt.hip)
//   column sums      colsum_plan.hpp cuts every column into items of at most COLSUM_FAN inputs, level by level
//     k_colsum_terms     level 0, one lane per item: for each term a double-and-add of bitlen(k) steps on the (negated) base
//                        point, the results summed by the complete addition
//     k_colsum_partials  levels >= 1, one lane per item: the sum of at most COLSUM_FAN partial sums of the level before
//   h query          k_h_query, one lane per point: tau_g1[i + N] - tau_g1[i] (mixed addition of the negated point)
//   contribution     k_points_scale, one lane per point: one scalar for every lane (zkmi_pk_contribute)
//   k_xyzz_store     XYZZ -> resident affine, the store of the point transform (four points per inversion)
//
// Nothing waits.  No lane reads what another lane of the same launch writes, there are no atomics, flags or counters, and
// the only ordering is launch order on ctx->stream.  Every loop count is an item's `count` or a term's bit length: both
// come from the host plan and are range-checked before the loop -- an out-of-range value ends the lane and raises the
// status word the host reads after the last launch.  The per-item bodies are __host__ __device__ templates: the kernels
// call them, and so does the host loop run_plan_host() the CPU tests run over the same plan.
#include <string.h>
#include <chrono>
#include <string>
#include "group_dev.hpp"
#include "setup_srs.hpp"

namespace zkmi {

namespace {

enum : uint32_t { CS_OK = 0, CS_BAD_ITEM = 1, CS_BAD_TERM = 2, CS_BAD_OUT = 3, CS_BAD_BITS = 4 };

// the group operations of a body: the out-of-line device functions on the device, the methods themselves on the host
template <class F>
__host__ __device__ inline void cs_dbl(XYZZ<F>* a) {
#ifdef __HIP_DEVICE_COMPILE__
  g_dbl(a);
#else
  a->dbl_inplace();
#endif
}
template <class F>
__host__ __device__ inline void cs_add(XYZZ<F>* a, const XYZZ<F>* o) {
#ifdef __HIP_DEVICE_COMPILE__
  g_add(a, o);
#else
  a->add(*o);
#endif
}
template <class F>
__host__ __device__ inline void cs_madd(XYZZ<F>* a, const Affine<F>* p) {
#ifdef __HIP_DEVICE_COMPILE__
  g_madd(a, p);
#else
  a->madd(*p);
#endif
}
template <class T>
__host__ __device__ inline T cs_load(const T* p) {
#ifdef __HIP_DEVICE_COMPILE__
  return ldv(p);
#else
  return *p;
#endif
}
template <class T>
__host__ __device__ inline void cs_store(T* p, const T& v) {
#ifdef __HIP_DEVICE_COMPILE__
  stv(p, v);
#else
  *p = v;
#endif
}

// k * p for the low `bits` bits of a little-endian scalar, from the top bit down; the caller has checked bits <= 256
template <class F>
__host__ __device__ inline void mul_bits(const Affine<F>* p, const uint32_t* k, uint32_t bits, XYZZ<F>* acc) {
  *acc = XYZZ<F>::infinity();
#pragma unroll 1
  for (uint32_t b = bits; b-- > 0;) {
    cs_dbl(acc);
    if ((k[b >> 5] >> (b & 31u)) & 1u) cs_madd(acc, p);
  }
}

// where an item writes: a final slot or a partial of its level; nullptr when the index is out of range
template <class F>
__host__ __device__ inline XYZZ<F>* colsum_dst(const ColsumItem& it, XYZZ<F>* finals, uint32_t n_slots, XYZZ<F>* partials,
                                               uint32_t n_partials) {
  if (it.out & COLSUM_FINAL) {
    const uint32_t j = it.out & ~COLSUM_FINAL;
    return j < n_slots ? finals + j : nullptr;
  }
  return it.out < n_partials ? partials + it.out : nullptr;
}

// level 0: sum of k * (+-)base[sel][point] over the item's terms
template <class F>
__host__ __device__ inline uint32_t colsum_terms_body(const ColsumItem& it, const ColsumTerm* terms, uint32_t n_terms,
                                                      const Affine<F>* bases, uint32_t n_points, uint32_t n_sel, XYZZ<F>* sum) {
  if (it.count - 1u >= COLSUM_FAN || it.first > n_terms || it.count > n_terms - it.first) return CS_BAD_ITEM;
  *sum = XYZZ<F>::infinity();
#pragma unroll 1
  for (uint32_t q = 0; q < it.count; q++) {
    const ColsumTerm t = terms[it.first + q];
    const uint32_t bits = t.bits();
    if (bits - 1u >= 255u || t.point >= n_points || t.base() >= n_sel) return CS_BAD_TERM;
    Affine<F> p = cs_load(bases + (size_t)t.base() * n_points + t.point);
    if (t.neg()) p = p.neg();
    if (bits == 1) {  // k = 1: most coefficients of real relations are +-1
      cs_madd(sum, &p);
    } else {
      XYZZ<F> m;
      mul_bits(&p, t.k, bits, &m);
      cs_add(sum, &m);
    }
  }
  return CS_OK;
}

// levels >= 1: sum of the item's partial sums of the level before
template <class F>
__host__ __device__ inline uint32_t colsum_partials_body(const ColsumItem& it, const XYZZ<F>* prev, uint32_t n_prev, XYZZ<F>* sum) {
  if (it.count - 1u >= COLSUM_FAN || it.first > n_prev || it.count > n_prev - it.first) return CS_BAD_ITEM;
  *sum = cs_load(prev + it.first);
#pragma unroll 1
  for (uint32_t q = 1; q < it.count; q++) {
    const XYZZ<F> o = cs_load(prev + it.first + q);
    cs_add(sum, &o);
  }
  return CS_OK;
}

template <class F>
__global__ void __launch_bounds__(64)
k_colsum_terms(const ColsumItem* __restrict__ items, uint32_t n_items, const ColsumTerm* __restrict__ terms, uint32_t n_terms,
               const Affine<F>* __restrict__ bases, uint32_t n_points, uint32_t n_sel, XYZZ<F>* __restrict__ finals,
               uint32_t n_slots, XYZZ<F>* __restrict__ partials, uint32_t n_partials, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const ColsumItem it = items[i];
  XYZZ<F>* dst = colsum_dst(it, finals, n_slots, partials, n_partials);
  XYZZ<F> sum;
  const uint32_t st = dst ? colsum_terms_body(it, terms, n_terms, bases, n_points, n_sel, &sum) : (uint32_t)CS_BAD_OUT;
  if (st != CS_OK) {
    *status = st;
    return;
  }
  stv(dst, sum);
}

template <class F>
__global__ void __launch_bounds__(64)
k_colsum_partials(const ColsumItem* __restrict__ items, uint32_t n_items, const XYZZ<F>* __restrict__ prev, uint32_t n_prev,
                  XYZZ<F>* __restrict__ finals, uint32_t n_slots, XYZZ<F>* __restrict__ partials, uint32_t n_partials,
                  uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const ColsumItem it = items[i];
  XYZZ<F>* dst = colsum_dst(it, finals, n_slots, partials, n_partials);
  XYZZ<F> sum;
  const uint32_t st = dst ? colsum_partials_body(it, prev, n_prev, &sum) : (uint32_t)CS_BAD_OUT;
  if (st != CS_OK) {
    *status = st;
    return;
  }
  stv(dst, sum);
}

// out[i] = tau[i + n] - tau[i] for i < n - 1, out[n - 1] = infinity; tau holds at least 2n - 1 points
template <class F>
__global__ void __launch_bounds__(64) k_h_query(const Affine<F>* __restrict__ tau, uint32_t n, XYZZ<F>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  XYZZ<F> v = XYZZ<F>::infinity();
  if (i + 1 < n) {
    v = XYZZ<F>::from_affine(ldv(tau + (size_t)n + i));
    const Affine<F> m = ldv(tau + i).neg();
    g_madd(&v, &m);
  }
  stv(out + i, v);
}

// out[i] = k * pts[i], the low `bits` bits of k: every lane runs the same loop
template <class F>
__global__ void __launch_bounds__(64)
k_points_scale(const Affine<F>* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ k, uint32_t bits,
               XYZZ<F>* __restrict__ out, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (bits > 255u) {
    *status = CS_BAD_BITS;
    return;
  }
  uint32_t kw[8];
#pragma unroll
  for (int w = 0; w < 8; w++) kw[w] = k[w];
  const Affine<F> p = ldv(pts + i);
  XYZZ<F> v;
  mul_bits(&p, kw, bits, &v);
  stv(out + i, v);
}

template <class F>
__global__ void __launch_bounds__(64) k_xyzz_store(const XYZZ<F>* __restrict__ src, Affine<F>* __restrict__ dst, uint32_t n) {
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

template <class F>
hipError_t store_affine(hipStream_t st, const XYZZ<F>* src, Affine<F>* dst, uint64_t n) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_xyzz_store<F>, dim3(blocks64((n + PN_INV_BATCH - 1) / PN_INV_BATCH)), dim3(64), 0, st, src, dst, (uint32_t)n);
  return hipGetLastError();
}

const char* cs_status_name(uint32_t s) {
  switch (s) {
    case CS_BAD_ITEM: return "item count or input range out of bounds";
    case CS_BAD_TERM: return "term bit length, point or base selector out of bounds";
    case CS_BAD_OUT: return "output slot out of bounds";
    case CS_BAD_BITS: return "scalar bit length out of bounds";
    default: return "unknown status";
  }
}

// One query on the device: d_out[j] = column sum j (n_slots resident affine points).  *status: what the kernels raised.
template <class F>
hipError_t run_plan_dev(zkmi_ctx* ctx, const ColsumPlan& plan, const Affine<F>* d_bases, uint32_t n_points, uint32_t n_sel,
                        Affine<F>* d_out, uint32_t* status) {
  hipStream_t st = ctx->stream;
  hipError_t e;
  *status = CS_OK;
  const size_t nl = plan.levels.size();
  uint32_t max_part = 0;
  for (uint32_t c : plan.n_partials) max_part = c > max_part ? c : max_part;
  DevBuf terms, finals, part[2], d_status;
  std::vector<DevBuf> items(nl);
  if ((e = terms.upload(plan.terms.data(), sizeof(ColsumTerm) * plan.terms.size())) != hipSuccess) return e;
  for (size_t l = 0; l < nl; l++)
    if ((e = items[l].upload(plan.levels[l].data(), sizeof(ColsumItem) * plan.levels[l].size())) != hipSuccess) return e;
  if ((e = finals.alloc(sizeof(XYZZ<F>) * plan.n_slots)) != hipSuccess) return e;
  if ((e = part[0].alloc(sizeof(XYZZ<F>) * max_part)) != hipSuccess) return e;
  if ((e = part[1].alloc(sizeof(XYZZ<F>) * max_part)) != hipSuccess) return e;
  if ((e = d_status.alloc(sizeof(uint32_t))) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st)) != hipSuccess) return e;
  // every slot starts as infinity (all-zero XYZZ): the slots of variables no row mentions stay so
  if ((e = hipMemsetAsync(finals.p, 0, sizeof(XYZZ<F>) * plan.n_slots, st)) != hipSuccess) return e;
  for (size_t l = 0; l < nl; l++) {
    const uint32_t n_items = (uint32_t)plan.levels[l].size();
    XYZZ<F>* cur = part[l & 1].as<XYZZ<F>>();
    if (l == 0)
      hipLaunchKernelGGL(k_colsum_terms<F>, dim3(blocks64(n_items)), dim3(64), 0, st, items[0].as<ColsumItem>(), n_items,
                         terms.as<ColsumTerm>(), (uint32_t)plan.terms.size(), d_bases, n_points, n_sel, finals.as<XYZZ<F>>(),
                         plan.n_slots, cur, plan.n_partials[0], d_status.as<uint32_t>());
    else
      hipLaunchKernelGGL(k_colsum_partials<F>, dim3(blocks64(n_items)), dim3(64), 0, st, items[l].as<ColsumItem>(), n_items,
                         part[(l - 1) & 1].as<XYZZ<F>>(), plan.n_partials[l - 1], finals.as<XYZZ<F>>(), plan.n_slots, cur,
                         plan.n_partials[l], d_status.as<uint32_t>());
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = store_affine<F>(st, finals.as<XYZZ<F>>(), d_out, plan.n_slots)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

// The same plan through the same bodies in a host loop; false when a body refused an item
template <class F>
bool run_plan_host(const ColsumPlan& plan, const Affine<F>* bases, uint32_t n_points, uint32_t n_sel, std::vector<XYZZ<F>>* finals) {
  finals->assign(plan.n_slots, XYZZ<F>::infinity());
  std::vector<XYZZ<F>> prev, cur;
  for (size_t l = 0; l < plan.levels.size(); l++) {
    cur.assign(plan.n_partials[l], XYZZ<F>::infinity());
    for (const ColsumItem& it : plan.levels[l]) {
      XYZZ<F>* dst = colsum_dst(it, finals->data(), plan.n_slots, cur.data(), plan.n_partials[l]);
      if (!dst) return false;
      XYZZ<F> sum;
      const uint32_t st = l == 0 ? colsum_terms_body(it, plan.terms.data(), (uint32_t)plan.terms.size(), bases, n_points, n_sel, &sum)
                                 : colsum_partials_body(it, prev.data(), (uint32_t)prev.size(), &sum);
      if (st != CS_OK) return false;
      *dst = sum;
    }
    prev.swap(cur);
  }
  return true;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
#ifdef ZKMI_TESTING
double g_setup_phase_ms[3] = {0, 0, 0};  // zkmi_setup_from_srs_phases: transform, column sums, h (last call wins)
#endif

}  // namespace

bool setup_colsum_plan(const zkmi_r1cs& r, int which, ColsumPlan* plan) {
  if (which != 0 && which != 1 && which != 2 && which != 4) return false;
  uint64_t total = 3ull * r.n_pub;
  for (int m = 0; m < 3; m++) total += r.m[m].col.size();
  if (total >= (1ull << 31)) return false;
  std::vector<uint32_t> canon[3];
  auto src = [&](int m, uint32_t sel) {
    const auto& M = r.m[m];
    canon[m].resize(8 * M.val.size());
    for (size_t k = 0; k < M.val.size(); k++) {
      const Fr c = M.val[k].from_mont();
      memcpy(&canon[m][8 * k], c.l, 32);
    }
    return ColsumSource{M.rowptr.data(), M.col.data(), canon[m].data(), sel};
  };
  std::vector<ColsumSource> srcs;
  std::vector<uint32_t> inst;
  if (which == 0) {
    srcs = {src(0, 0)};
    inst = {0};
  } else if (which == 4) {
    srcs = {src(0, 2), src(1, 1), src(2, 0)};  // beta A + alpha B + C
    inst = {2};
  } else {
    srcs = {src(1, 0)};
  }
  *plan = colsum_plan(r.n_vars, r.n_constraints, srcs, r.n_pub, inst, FrParams::MOD);
  return true;
}

int32_t setup_queries_from_srs(zkmi_ctx* ctx, const zkmi_r1cs* r, const zkmi_srs* srs, const SetupQueries& out,
                               G1Affine* alpha_g1, G1Affine* beta_g1) {
  const uint64_t N = 1ull << r->log_n;
  hipStream_t st = ctx->stream;
  ColsumPlan plans[4];
  static const int WHICH[4] = {0, 1, 2, 4};
  for (int q = 0; q < 4; q++)
    if (!setup_colsum_plan(*r, WHICH[q], &plans[q])) return ctx->fail(ZKMI_ERR_BAD_ARG, "relation too large for the column plan");
  ZK_HIP(ctx, hipMemcpy(alpha_g1, srs->alpha_tau_g1, sizeof(G1Affine), hipMemcpyDeviceToHost));
  ZK_HIP(ctx, hipMemcpy(beta_g1, srs->beta_tau_g1, sizeof(G1Affine), hipMemcpyDeviceToHost));
  // Lagrange bases: [L_i]G1 | [alpha L_i]G1 | [beta L_i]G1 in one chain, [L_i]G2; the transcript stays as it is
  auto t0 = std::chrono::steady_clock::now();
  DevBuf l1, l2, tw;
  ZK_HIP(ctx, l1.alloc(sizeof(G1Affine) * 3 * N));
  ZK_HIP(ctx, l2.alloc(sizeof(G2Affine) * N));
  const G1Affine* s1[3] = {srs->tau_g1, srs->alpha_tau_g1, srs->beta_tau_g1};
  for (int a = 0; a < 3; a++)
    ZK_HIP(ctx, hipMemcpyAsync(l1.as<G1Affine>() + a * N, s1[a], sizeof(G1Affine) * N, hipMemcpyDeviceToDevice, st));
  ZK_HIP(ctx, hipMemcpyAsync(l2.p, srs->tau_g2, sizeof(G2Affine) * N, hipMemcpyDeviceToDevice, st));
  uint32_t* d_tw = nullptr;
  ZK_HIP(ctx, points_ntt_twiddles(r->log_n, &d_tw));
  tw.p = d_tw;
  ZK_HIP(ctx, points_ntt_resident<Fq>(ctx, l1.as<G1Affine>(), N, 3, r->log_n, true, d_tw));
  ZK_HIP(ctx, points_ntt_resident<Fq2>(ctx, l2.as<G2Affine>(), N, 1, r->log_n, true, d_tw));
  const double ms_transform = ms_since(t0);
  // column sums
  t0 = std::chrono::steady_clock::now();
  uint32_t status[4] = {0, 0, 0, 0};
  ZK_HIP(ctx, run_plan_dev<Fq>(ctx, plans[0], l1.as<G1Affine>(), (uint32_t)N, 1, out.a, &status[0]));
  ZK_HIP(ctx, run_plan_dev<Fq>(ctx, plans[1], l1.as<G1Affine>(), (uint32_t)N, 1, out.b_g1, &status[1]));
  ZK_HIP(ctx, run_plan_dev<Fq2>(ctx, plans[2], l2.as<G2Affine>(), (uint32_t)N, 1, out.b_g2, &status[2]));
  ZK_HIP(ctx, run_plan_dev<Fq>(ctx, plans[3], l1.as<G1Affine>(), (uint32_t)N, 3, out.l, &status[3]));
  for (int q = 0; q < 4; q++)
    if (status[q] != CS_OK)
      return ctx->fail(ZKMI_ERR_HIP, std::string("column sums, query ") + std::to_string(WHICH[q]) + ": " + cs_status_name(status[q]));
  const double ms_columns = ms_since(t0);
  // h[i] = [tau^(i + N) - tau^i]G1 = [tau^i Z(tau)]G1
  t0 = std::chrono::steady_clock::now();
  DevBuf hw;
  ZK_HIP(ctx, hw.alloc(sizeof(G1XYZZ) * N));
  hipLaunchKernelGGL(k_h_query<Fq>, dim3(blocks64(N)), dim3(64), 0, st, srs->tau_g1, (uint32_t)N, hw.as<G1XYZZ>());
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, store_affine<Fq>(st, hw.as<G1XYZZ>(), out.h, N));
  ZK_HIP(ctx, hipStreamSynchronize(st));
#ifdef ZKMI_TESTING
  g_setup_phase_ms[0] = ms_transform, g_setup_phase_ms[1] = ms_columns, g_setup_phase_ms[2] = ms_since(t0);
#else
  (void)ms_transform, (void)ms_columns;
#endif
  return ZKMI_OK;
}

template <class F>
int32_t points_scale_resident(zkmi_ctx* ctx, Affine<F>* d_pts, uint64_t n, const uint32_t k[8]) {
  if (!n) return ZKMI_OK;
  hipStream_t st = ctx->stream;
  DevBuf work, d_k, d_status;
  ZK_HIP(ctx, work.alloc(sizeof(XYZZ<F>) * n));
  ZK_HIP(ctx, d_k.upload(k, 32));
  ZK_HIP(ctx, d_status.alloc(sizeof(uint32_t)));
  ZK_HIP(ctx, hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_points_scale<F>, dim3(blocks64(n)), dim3(64), 0, st, d_pts, (uint32_t)n, d_k.as<uint32_t>(),
                     colsum_detail::bitlen8(k), work.as<XYZZ<F>>(), d_status.as<uint32_t>());
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, store_affine<F>(st, work.as<XYZZ<F>>(), d_pts, n));
  uint32_t status = 0;
  ZK_HIP(ctx, hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  ZK_HIP(ctx, hipStreamSynchronize(st));
  if (status != CS_OK) return ctx->fail(ZKMI_ERR_HIP, std::string("point scaling: ") + cs_status_name(status));
  return ZKMI_OK;
}
template int32_t points_scale_resident<Fq>(zkmi_ctx*, G1Affine*, uint64_t, const uint32_t*);

}  // namespace zkmi

#ifdef ZKMI_TESTING
using namespace zkmi;

extern "C" {

int32_t zkmi_selftest_colsum_plan(const zkmi_r1cs* r1cs, int32_t which, uint64_t out_counts[5], uint32_t* out_terms,
                                  uint64_t cap_terms, uint32_t* out_items, uint64_t cap_items, uint32_t* out_empty,
                                  uint64_t cap_empty) {
  if (!r1cs || !out_counts) return ZKMI_ERR_BAD_ARG;
  ColsumPlan p;
  if (!setup_colsum_plan(*r1cs, which, &p)) return ZKMI_ERR_BAD_ARG;
  uint64_t n_items = 0;
  for (const auto& l : p.levels) n_items += l.size();
  out_counts[0] = COLSUM_FAN, out_counts[1] = p.terms.size(), out_counts[2] = n_items, out_counts[3] = p.levels.size();
  out_counts[4] = p.empty_slots.size();
  if (out_terms) {
    if (cap_terms < p.terms.size()) return ZKMI_ERR_BAD_ARG;
    for (size_t i = 0; i < p.terms.size(); i++) {
      const ColsumTerm& t = p.terms[i];
      uint32_t* o = out_terms + 12 * i;
      o[0] = t.point, o[1] = t.base(), o[2] = t.neg() ? 1u : 0u, o[3] = t.bits();
      memcpy(o + 4, t.k, 32);
    }
  }
  if (out_items) {
    if (cap_items < n_items) return ZKMI_ERR_BAD_ARG;
    uint32_t* o = out_items;
    for (size_t l = 0; l < p.levels.size(); l++)
      for (const ColsumItem& it : p.levels[l]) {
        o[0] = (uint32_t)l, o[1] = it.out, o[2] = it.first, o[3] = it.count;
        o += 4;
      }
  }
  if (out_empty) {
    if (cap_empty < p.empty_slots.size()) return ZKMI_ERR_BAD_ARG;
    for (size_t i = 0; i < p.empty_slots.size(); i++) out_empty[i] = p.empty_slots[i];
  }
  return ZKMI_OK;
}

int32_t zkmi_selftest_setup_columns_host(const zkmi_r1cs* r1cs, const uint8_t toxic3[96], int32_t which, uint8_t* out_wire) {
  if (!r1cs || !toxic3 || !out_wire || r1cs->log_n > 6) return ZKMI_ERR_BAD_ARG;
  Fr tau, alpha, beta, zt;
  if (!fr_from_wire(toxic3, &tau) || !fr_from_wire(toxic3 + 32, &alpha) || !fr_from_wire(toxic3 + 64, &beta)) return ZKMI_ERR_NON_CANONICAL;
  ColsumPlan plan;
  if (!setup_colsum_plan(*r1cs, which, &plan)) return ZKMI_ERR_BAD_ARG;
  std::vector<Fr> L;
  if (!lagrange_basis_at(r1cs->log_n, tau, &L, &zt)) return ZKMI_ERR_BAD_ARG;
  const uint32_t N = 1u << r1cs->log_n, nv = r1cs->n_vars;
  auto words = [](const Fr& mont, uint32_t k[8]) {
    const Fr c = mont.from_mont();
    memcpy(k, c.l, 32);
  };
  uint32_t k[8];
  if (which == 2) {
    const G2XYZZ g = G2XYZZ::from_affine(g2_generator());
    std::vector<G2Affine> bases(N);
    for (uint32_t i = 0; i < N; i++) {
      words(L[i], k);
      bases[i] = scalar_mul(g, k, 8).to_affine();
    }
    std::vector<G2XYZZ> fin;
    if (!run_plan_host<Fq2>(plan, bases.data(), N, 1, &fin)) return ZKMI_ERR_BAD_ARG;
    for (uint32_t j = 0; j < nv; j++) g2_to_wire(fin[j].to_affine(), out_wire + 192ull * j);
    return ZKMI_OK;
  }
  const G1XYZZ g = G1XYZZ::from_affine(g1_generator());
  std::vector<G1Affine> bases(3 * N);
  const Fr scale[3] = {Fr::one(), alpha, beta};
  for (uint32_t s = 0; s < 3; s++)
    for (uint32_t i = 0; i < N; i++) {
      words(L[i] * scale[s], k);
      bases[s * N + i] = scalar_mul(g, k, 8).to_affine();
    }
  std::vector<G1XYZZ> fin;
  if (!run_plan_host<Fq>(plan, bases.data(), N, which == 4 ? 3 : 1, &fin)) return ZKMI_ERR_BAD_ARG;
  for (uint32_t j = 0; j < nv; j++) g1_to_wire(fin[j].to_affine(), out_wire + 96ull * j);
  return ZKMI_OK;
}

int32_t zkmi_setup_from_srs_phases(double out_ms[3]) {
  if (!out_ms) return ZKMI_ERR_BAD_ARG;
  for (int i = 0; i < 3; i++) out_ms[i] = g_setup_phase_ms[i];
  return ZKMI_OK;
}

}  // extern "C"
#endif
