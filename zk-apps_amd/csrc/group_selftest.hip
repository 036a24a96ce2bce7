// zkmi — the group law between the field and the MSM on caller-chosen RAW limb arrays (zkmi_selftest_group_ops): one body of
// msm_impl.hpp, curve.hpp or quad.hpp per call, in the lane layout the accumulation kernels use, on the device or -- where the
// body is host-callable -- in a host loop (group_selftest.hpp).  The callers (tests/test_cpu_group28.py,
// tests/test_gpu_group28.py) place every coordinate in the representations x + k p its class admits, the ends included, and
// compare with the big-integer model of tests/group28.py.
// TEST SCAFFOLDING (include/zkmi_testing.h): compiled into libzkmi_exp.so only.
#ifdef ZKMI_TESTING
#include "ctx.hpp"
#include "group_selftest.hpp"
#include "quad.hpp"
using namespace zkmi;

namespace {
// 64-lane blocks like the accumulation kernels; tail lanes (pairs, quads, octets) shadow the last tuple and write nothing,
// so every DPP source lane is enabled
template <int OP, class F>
__global__ void __launch_bounds__(64) k_group_lane(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                   uint8_t* __restrict__ flag, uint32_t n) {
  constexpr int W = GroupCoord<F>::W;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = t < n;
  const uint32_t idx = live ? t : n - 1;  // n >= 1 (host)
  const GroupLaneIO<F> io = {in + idx * group_in_words<OP, W>(), out + (size_t)idx * GOP_OUT * W, flag + idx, live};
  group_op_body<OP>(io);
}
template <int OP>
__global__ void __launch_bounds__(64) k_group_pair(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                   uint8_t* __restrict__ flag, uint32_t n) {
  constexpr int W = GroupPairIO::W;
  const uint32_t pair = (blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  const bool live = pair < n;
  const uint32_t idx = live ? pair : n - 1;
  const GroupPairIO io = {in + idx * group_in_words<OP, W>(), out + (size_t)idx * GOP_OUT * W, flag + idx, threadIdx.x & 1u, live};
  group_op_body<OP>(io);
}
// XYZZQ::add: a quad (G2: an octet) of lanes per point, one coordinate (component) per lane; a tuple is the two points a, o in
// the memory form XYZZQ::load reads
template <class PT>
__global__ void __launch_bounds__(64) k_group_quad(const int32_t* __restrict__ in, int32_t* __restrict__ out, uint32_t n) {
  using Point = typename PT::Point;
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / PT::LANES;
  const bool live = i < n;
  const uint32_t idx = live ? i : n - 1;
  const Point* a = reinterpret_cast<const Point*>(in) + 2 * (size_t)idx;
  PT r = PT::load(a);
  r.add(PT::load(a + 1));
  if (live) r.store(reinterpret_cast<Point*>(out) + idx);
}

enum Layout { LANE, PAIR, QUAD };

// From here on host code only, compiled without optimisation: the host loop inlines every body once more per op and curve, and
// optimising those copies cost this file more build time than its kernels.  The bodies are the same source either way.
#pragma clang optimize off

// F: the coordinate type of the one-lane layout (and of the host path); PAIR runs Fq2P, QUAD the XYZZQ form over BF
template <int OP, class F, class BF, Layout L, bool EXT2>
int32_t run(zkmi_ctx* ctx, uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  constexpr int W = GroupCoord<F>::W;
  constexpr bool FLAG = gop_has_flag(OP);
  if (!out || (FLAG && !out_flag)) return ZKMI_ERR_BAD_ARG;
  if (!ctx) {
    if constexpr (L == QUAD || (L == PAIR && OP != GOP_ADD_GENERIC)) {
      return ZKMI_ERR_BAD_ARG;  // DPP forms; (+-a) - b has no Fq2_28 form
    } else {
      uint8_t sink = 0;
      for (uint32_t t = 0; t < n; t++) {  // group_run_host's loop, inside this unoptimised function
        const GroupLaneIO<F> io = {in + t * group_in_words<OP, W>(), out + (size_t)t * GOP_OUT * W, out_flag ? out_flag + t : &sink, true};
        group_op_body<OP>(io);
      }
      return ZKMI_OK;
    }
  }
  ZK_ENTER(ctx);
  const size_t in_bytes = sizeof(int32_t) * group_in_words<OP, W>() * n, out_bytes = sizeof(int32_t) * GOP_OUT * W * (size_t)n;
  int32_t *d_in = nullptr, *d_out = nullptr;
  uint8_t* d_flag = nullptr;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_flag, n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if constexpr (L == LANE) {
      hipLaunchKernelGGL((k_group_lane<OP, F>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_in, d_out, d_flag, n);
    } else if constexpr (L == PAIR) {
      hipLaunchKernelGGL(k_group_pair<OP>, dim3((2 * n + 63) / 64), dim3(64), 0, ctx->stream, d_in, d_out, d_flag, n);
    } else {
      using PT = XYZZQ<BF, OP == GOP_QUAD_BPERMUTE ? 1 : 0, EXT2>;
      hipLaunchKernelGGL(k_group_quad<PT>, dim3((PT::LANES * n + 63) / 64), dim3(64), 0, ctx->stream, d_in, d_out, n);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && FLAG) e = hipMemcpyAsync(out_flag, d_flag, n, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_flag);
  return e == hipSuccess ? ZKMI_OK : ctx->hip_fail(e, "group ops self-test");
}

// F: one-lane coordinate type; BF: its base field; G2: the accumulation layout is the lane pair, the quad form an octet
template <class F, class BF, bool G2>
int32_t dispatch(zkmi_ctx* ctx, int32_t op, uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  constexpr Layout ACC = G2 ? PAIR : LANE;
  switch (op) {
#define ZK_GOP_CASE(OP, L) \
  case OP: return run<OP, F, BF, L, G2>(ctx, n, in, out, out_flag);
    ZK_GOP_CASE(GOP_MADD, ACC) ZK_GOP_CASE(GOP_MADD_NEG, ACC) ZK_GOP_CASE(GOP_PAIR, ACC) ZK_GOP_CASE(GOP_PAIR_NEG, ACC)
    ZK_GOP_CASE(GOP_ADD_GENERIC, ACC) ZK_GOP_CASE(GOP_CHAIN, ACC)
    ZK_GOP_CASE(GOP_ADD, LANE) ZK_GOP_CASE(GOP_MADD_COMPLETE, LANE) ZK_GOP_CASE(GOP_DBL, LANE)
    ZK_GOP_CASE(GOP_QUAD_DPP, QUAD) ZK_GOP_CASE(GOP_QUAD_BPERMUTE, QUAD)
#undef ZK_GOP_CASE
    default: return ZKMI_ERR_BAD_ARG;
  }
}
}  // namespace

extern "C" int32_t zkmi_selftest_group_ops(zkmi_ctx* ctx, int32_t curve, int32_t op, uint32_t n, const int32_t* in, int32_t* out,
                                           uint8_t* out_flag) {
  if (!in || n == 0 || n > (1u << 16)) return ZKMI_ERR_BAD_ARG;
  switch (curve) {
    case 0: return dispatch<Fq28, Fq28, false>(ctx, op, n, in, out, out_flag);
    case 1: return dispatch<Fq2_28, Fq28, true>(ctx, op, n, in, out, out_flag);
    case 2: return dispatch<BnFq28, BnFq28, false>(ctx, op, n, in, out, out_flag);
    default: return ZKMI_ERR_BAD_ARG;
  }
}
#pragma clang optimize on
#endif  // ZKMI_TESTING
