// zkmi — one body of the device group law on caller-chosen RAW limb arrays: the mixed and general additions of the bucket
// kernels (msm_impl.hpp madd_generic, madd_affine_pair, add_generic), the complete one-lane forms of curve.hpp (XYZZ::add,
// XYZZ::madd, XYZZ::dbl_inplace) and a short accumulation chain, each as the body the product runs.  Shared by
// group_selftest.hip (zkmi_selftest_group_ops: device kernels and the host loop) and oracle/group_ubsan.cpp (the host loop
// under UndefinedBehaviorSanitizer).  tests/group28.py is the big-integer model.
// TEST SCAFFOLDING (include/zkmi_testing.h): compiled into libzkmi_exp.so only.
#pragma once
#include "msm_impl.hpp"

namespace zkmi {

enum GroupOp : int {
  GOP_MADD = 0, GOP_MADD_NEG, GOP_PAIR, GOP_PAIR_NEG, GOP_ADD_GENERIC, GOP_ADD, GOP_MADD_COMPLETE, GOP_DBL, GOP_QUAD_DPP,
  GOP_QUAD_BPERMUTE, GOP_CHAIN,
  GOP_COUNT
};
constexpr int GROUP_CHAIN_K = 16;  // points of a chain: the first entry and K - 1 behind it
// coordinates per tuple in (the chain: + K sign words behind them); every op writes the four coordinates of a point
constexpr int GOP_IN[GOP_COUNT] = {6, 6, 4, 4, 8, 8, 6, 4, 8, 8, 2 * GROUP_CHAIN_K};
constexpr int GOP_OUT = 4;
constexpr int GOP_SIGNS[GOP_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, GROUP_CHAIN_K};
constexpr bool gop_has_flag(int op) { return op <= GOP_ADD_GENERIC || op == GOP_CHAIN; }

// int32 words of one coordinate of the curve's points
template <class F>
struct GroupCoord {
  static constexpr int W = F::NL;
  ZK_HD static F ld(const int32_t* p) {
    F r;
#pragma unroll
    for (int i = 0; i < F::NL; i++) r.l[i] = p[i];
    return r;
  }
  ZK_HD static void st(int32_t* p, const F& v) {
#pragma unroll
    for (int i = 0; i < F::NL; i++) p[i] = v.l[i];
  }
};
template <class B>
struct GroupCoord<Fq2T<B>> {
  static constexpr int W = 2 * B::NL;
  ZK_HD static Fq2T<B> ld(const int32_t* p) { return {GroupCoord<B>::ld(p), GroupCoord<B>::ld(p + B::NL)}; }
  ZK_HD static void st(int32_t* p, const Fq2T<B>& v) {
    GroupCoord<B>::st(p, v.c0);
    GroupCoord<B>::st(p + B::NL, v.c1);
  }
};

// a tuple as ONE lane sees it: every coordinate whole
template <class F_>
struct GroupLaneIO {
  using F = F_;
  static constexpr int W = GroupCoord<F>::W;
  const int32_t* in;
  int32_t* out;
  uint8_t* flag;
  bool live;
  ZK_HD F ld(int k) const { return GroupCoord<F>::ld(in + k * W); }
  ZK_HD int32_t word(int k) const { return in[k]; }
  ZK_HD void st(int k, const F& v) const {
    if (live) GroupCoord<F>::st(out + k * W, v);
  }
  ZK_HD void st_flag(uint8_t v) const {
    if (live) *flag = v;
  }
};
#if defined(__HIPCC__)
// ... and as lane `comp` of a lane pair sees it: its component of every Fq2 coordinate (c0 then c1 in memory)
struct GroupPairIO {
  using F = Fq2P;
  static constexpr int W = 2 * Fq28::NL;
  const int32_t* in;
  int32_t* out;
  uint8_t* flag;
  uint32_t comp;
  bool live;
  __device__ __forceinline__ Fq2P ld(int k) const { return {GroupCoord<Fq28>::ld(in + k * W + comp * Fq28::NL)}; }
  __device__ __forceinline__ int32_t word(int k) const { return in[k]; }
  __device__ __forceinline__ void st(int k, const Fq2P& v) const {
    if (live) GroupCoord<Fq28>::st(out + k * W + comp * Fq28::NL, v.v);
  }
  __device__ __forceinline__ void st_flag(uint8_t v) const {
    if (live && comp == 0) *flag = v;
  }
};
#endif

template <class IO>
ZK_HD XYZZ<typename IO::F> group_ld_point(const IO& io, int k) {
  return {io.ld(k), io.ld(k + 1), io.ld(k + 2), io.ld(k + 3)};
}
template <class IO>
ZK_HD void group_st_point(const IO& io, const XYZZ<typename IO::F>& p) {
  io.st(0, p.x);
  io.st(1, p.y);
  io.st(2, p.zz);
  io.st(3, p.zzz);
}

// ops 0 - 7 and 10 (8 and 9 are kernels of their own: group_selftest.hip)
template <int OP, class IO>
ZK_HD void group_op_body(const IO& io) {
  using F = typename IO::F;
  if constexpr (OP == GOP_MADD || OP == GOP_MADD_NEG) {
    XYZZ<F> acc = group_ld_point(io, 0);
    const Affine<F> p = {io.ld(4), io.ld(5)};
    const bool ok = madd_generic(acc, p, OP == GOP_MADD_NEG ? 0xffffffffu : 0u);
    group_st_point(io, acc);
    io.st_flag(ok ? 1 : 0);
  }
  if constexpr (OP == GOP_PAIR || OP == GOP_PAIR_NEG) {
    // zz and zzz of an affine accumulator are implied and never read: zeros here, so that the false branch has bytes to show
    XYZZ<F> acc = {io.ld(0), io.ld(1), F::zero(), F::zero()};
    const Affine<F> p = {io.ld(2), io.ld(3)};
    const bool ok = madd_affine_pair(acc, p, OP == GOP_PAIR_NEG ? 0xffffffffu : 0u);
    group_st_point(io, acc);
    io.st_flag(ok ? 1 : 0);
  }
  if constexpr (OP == GOP_ADD_GENERIC) {
    XYZZ<F> a = group_ld_point(io, 0);
    const bool ok = add_generic(a, group_ld_point(io, 4));
    group_st_point(io, a);
    io.st_flag(ok ? 1 : 0);
  }
  if constexpr (OP == GOP_ADD) {
    XYZZ<F> a = group_ld_point(io, 0);
    a.add(group_ld_point(io, 4));
    group_st_point(io, a);
  }
  if constexpr (OP == GOP_MADD_COMPLETE) {
    XYZZ<F> a = group_ld_point(io, 0);
    const Affine<F> p = {io.ld(4), io.ld(5)};
    a.madd(p);
    group_st_point(io, a);
  }
  if constexpr (OP == GOP_DBL) {
    XYZZ<F> a = group_ld_point(io, 0);
    a.dbl_inplace();
    group_st_point(io, a);
  }
  if constexpr (OP == GOP_CHAIN) {
    // what accum_first and accum_chain<FIRST_IS_AFFINE> do to the entries of one bucket, without the table and the sort:
    // the first entry with its sign applied, the pair step, generic additions until one needs the complete law
    constexpr int K = GROUP_CHAIN_K;
    const int signs = 2 * K * IO::W;
    XYZZ<F> acc = {io.ld(0), io.ld(1), F::zero(), F::zero()};
    if (io.word(signs) != 0) acc.y = acc.y.neg();
    uint32_t bad = 0xFFu;
    {
      const Affine<F> p = {io.ld(2), io.ld(3)};
      if (!madd_affine_pair(acc, p, io.word(signs + 1) != 0 ? 0xffffffffu : 0u)) bad = 1;
    }
#pragma unroll 1
    for (int k = 2; k < K && bad == 0xFFu; k++) {
      const Affine<F> p = {io.ld(2 * k), io.ld(2 * k + 1)};
      if (!madd_generic(acc, p, io.word(signs + k) != 0 ? 0xffffffffu : 0u)) bad = (uint32_t)k;
    }
    group_st_point(io, acc);
    io.st_flag((uint8_t)bad);
  }
}

// words per tuple
template <int OP, int W>
constexpr size_t group_in_words() { return (size_t)GOP_IN[OP] * W + GOP_SIGNS[OP]; }

// the host path: tuple after tuple through the same body
template <int OP, class F>
static inline void group_run_host(uint32_t n, const int32_t* in, int32_t* out, uint8_t* out_flag) {
  constexpr int W = GroupCoord<F>::W;
  uint8_t sink = 0;
  for (uint32_t t = 0; t < n; t++) {
    const GroupLaneIO<F> io = {in + t * group_in_words<OP, W>(), out + (size_t)t * GOP_OUT * W, out_flag ? out_flag + t : &sink, true};
    group_op_body<OP>(io);
  }
}

}  // namespace zkmi
