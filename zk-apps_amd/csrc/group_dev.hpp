// zkmi — the group operations of the 32-bit-limb fields as out-of-line device functions, shared by the kernels that are
// thin loops around them: the point transforms (points_ntt.hip) and the key derivation from a transcript (setup_srs.hip).
//
// A call costs a scratch frame, which a 255-step double-and-add does not notice, and a file compiles in a fraction of the
// time the inlined bodies take (the accumulation kernels of msm_impl.hpp make the opposite trade).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "curve.hpp"

namespace zkmi {
namespace {

constexpr int PN_INV_BATCH = 4;  // points per lane of the affine stores (Montgomery's trick: one inversion for all of them)

template <class T>
__device__ __forceinline__ T ldv(const T* p) {
  T r;
  const uint4* s = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
  return r;
}
template <class T>
__device__ __forceinline__ void stv(T* p, const T& v) {
  const uint4* s = reinterpret_cast<const uint4*>(&v);
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
}

// The group operations, one body per field.
template <class F>
__device__ __noinline__ void g_dbl(XYZZ<F>* a) {
  a->dbl_inplace();
}
template <class F>
__device__ __noinline__ void g_add(XYZZ<F>* a, const XYZZ<F>* o) {
  a->add(*o);
}
template <class F>
__device__ __noinline__ void g_madd(XYZZ<F>* a, const Affine<F>* p) {
  a->madd(*p);
}
template <class F>
__device__ __noinline__ void f_inv(const F* a, F* out) {
  *out = a->inv();
}

// k * p for a canonical 8-word scalar in HBM, from the top bit down; the word is loaded once per 32 steps
template <class F>
__device__ __noinline__ void mul_words(const Affine<F>* p, const uint32_t* __restrict__ k, XYZZ<F>* acc) {
  *acc = XYZZ<F>::infinity();
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = k[w];
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      g_dbl(acc);
      if ((word >> b) & 1u) g_madd(acc, p);
    }
  }
}
template <class F>
__device__ __noinline__ void mul_words(const XYZZ<F>* p, const uint32_t* __restrict__ k, XYZZ<F>* acc) {
  *acc = XYZZ<F>::infinity();
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = k[w];
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      g_dbl(acc);
      if ((word >> b) & 1u) g_add(acc, p);
    }
  }
}

// src[first .. first + cnt) -> affine at dst[first ..], cnt <= PN_INV_BATCH points under one inversion: prefix products of the
// zzz coordinates (infinity counts as one), one inversion, and back
template <class F>
__device__ __forceinline__ void store_affine_batch(const XYZZ<F>* __restrict__ src, Affine<F>* __restrict__ dst, uint32_t first,
                                                   uint32_t cnt) {
  F pre[PN_INV_BATCH];
  F run = F::one();
#pragma unroll 1
  for (uint32_t k = 0; k < cnt; k++) {
    pre[k] = run;
    const F zzz = ldv(&src[first + k].zzz);
    if (!zzz.is_zero()) run = run * zzz;
  }
  F inv;
  f_inv(&run, &inv);
#pragma unroll 1
  for (uint32_t k = cnt; k-- > 0;) {
    const XYZZ<F> v = ldv(src + first + k);
    Affine<F> a = Affine<F>::infinity();
    if (!v.is_inf()) {
      const F zi = inv * pre[k];  // 1 / zzz
      inv = inv * v.zzz;
      const F zz_inv = (zi * v.zz).sqr();  // (zz / zzz)^2 = 1 / zz
      a = {v.x * zz_inv, v.y * zi};
    }
    stv(dst + first + k, a);
  }
}

}  // namespace
}  // namespace zkmi
