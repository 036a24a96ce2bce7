// zkmi — point arrays on the device: parse (three byte encodings + the resident form), decompress (square roots in
// Fq / Fq2), curve equation, prime-order subgroup ([r]P = O).  What zkmi_{g1,g2}_points_read_dev, the *_load_encoded
// entry points, zkmi_ark_pk_load_validated and zkmi_pk_check run; the host functions of wire.hip are the specification
// of every acceptance rule here and stay the comparison baseline.
//
// Shape: one lane per point, G1 on Fq28, G2 on Fq2_28 (DESIGN.md "Key ingest" has the register report).  Every
// exponent (the three of the square roots, r of the subgroup check) is a constant in the constant address space and
// the bit that steers square-and-multiply / double-and-add is read with a wave-uniform index: no lane branches on its
// own data in those loops except into the exceptional cases of the complete addition (P = +-Q, infinity), which a
// point of small order does reach.  A lane whose element is refused keeps computing on whatever it parsed and only
// records its status; lanes past the end of the array redo the last element and write nothing.
#include "points.hpp"
#include "field28.hpp"

namespace zkmi {

namespace {

// (p+1)/4, (p-3)/4, (p-1)/2 and r, little-endian 32-bit words
__constant__ const uint32_t EXP_P14[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                           0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
__constant__ const uint32_t EXP_P34[12] = {0xffffeaaau, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                           0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
__constant__ const uint32_t EXP_P12[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                           0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};
__constant__ const uint32_t EXP_R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                        0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
constexpr int EXP_P14_TOP = 378, EXP_P34_TOP = 378, EXP_P12_TOP = 379, EXP_R_TOP = 254;  // index of the leading one

// (p-1)/2 as an integer: y is "lexicographically larger" iff its canonical value exceeds it
__device__ __forceinline__ bool words_gt_half(const uint32_t* w) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint64_t d = (uint64_t)EXP_P12[i] - w[i] - borrow;
    borrow = (d >> 63) & 1;
  }
  return borrow != 0;
}
__device__ __forceinline__ bool words_lt_p(const uint32_t* w) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint64_t d = (uint64_t)w[i] - FqParams::MOD[i] - borrow;
    borrow = (d >> 63) & 1;
  }
  return borrow != 0;
}
__device__ __forceinline__ bool words_zero(const uint32_t* w) {
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) acc |= w[i];
  return acc == 0;
}
// p - w for 0 < w < p
__device__ __forceinline__ void words_neg(uint32_t* w) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint64_t d = (uint64_t)FqParams::MOD[i] - w[i] - borrow;
    w[i] = (uint32_t)d;
    borrow = (d >> 63) & 1;
  }
}

// 4 R mod p (R = 2^392) in 28-bit limbs: the curve constant b = 4 (G1), 4 + 4u (G2)
__device__ __forceinline__ Fq28 fq28_four() {
  constexpr int32_t L[14] = {0xd1ff2e0, 0x6000000, 0x00ac467, 0x3379b48, 0x1c84b80, 0x0e88243, 0x0dd9a7e,
                             0x683dcf8, 0x6c26d0b, 0x4a5eec2, 0x457663c, 0x04b29f1, 0x967f3e8, 0x0015de9};
  Fq28 r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.l[i] = L[i];
  return r;
}

// ---- the two coordinate fields behind one set of names ----------------------------------------------------------
// W<NC>: canonical words of one coordinate, component c at w[c] (Fq2: c0, c1)
template <int NC>
struct Words {
  uint32_t w[NC][12];
};
template <int NC>
struct FieldOf;
template <>
struct FieldOf<1> {
  using F = Fq28;
  __device__ __forceinline__ static F from_words(const Words<1>& a) { return Fq28::from_canonical(a.w[0]); }
  __device__ __forceinline__ static void to_words(const F& a, Words<1>* o) { a.to_canonical(o->w[0]); }
  __device__ __forceinline__ static F curve_b() { return fq28_four(); }
  __device__ __forceinline__ static bool is_zero(const F& a) { return a.is_zero(); }
};
template <>
struct FieldOf<2> {
  using F = Fq2_28;
  __device__ __forceinline__ static F from_words(const Words<2>& a) {
    return {Fq28::from_canonical(a.w[0]), Fq28::from_canonical(a.w[1])};
  }
  __device__ __forceinline__ static void to_words(const F& a, Words<2>* o) {
    a.c0.to_canonical(o->w[0]);
    a.c1.to_canonical(o->w[1]);
  }
  __device__ __forceinline__ static F curve_b() { return {fq28_four(), fq28_four()}; }
  __device__ __forceinline__ static bool is_zero(const F& a) { return a.c0.is_zero() && a.c1.is_zero(); }
};

template <int NC>
__device__ __forceinline__ bool coord_zero(const Words<NC>& a) {
  bool z = true;
#pragma unroll
  for (int c = 0; c < NC; c++) z = z && words_zero(a.w[c]);
  return z;
}
template <int NC>
__device__ __forceinline__ bool coord_lt_p(const Words<NC>& a) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < NC; c++) ok = ok && words_lt_p(a.w[c]);
  return ok;
}
// Fq2 orders by c1, then c0 (wire.hip Fq2T::lex_larger)
template <int NC>
__device__ __forceinline__ bool coord_lex_larger(const Words<NC>& a) {
  if (NC == 2 && !words_zero(a.w[NC - 1])) return words_gt_half(a.w[NC - 1]);
  return words_gt_half(a.w[0]);
}
template <int NC>
__device__ __forceinline__ void coord_neg(Words<NC>* a) {
#pragma unroll
  for (int c = 0; c < NC; c++)
    if (!words_zero(a->w[c])) words_neg(a->w[c]);
}

// a^e for one of the constant exponents: plain square-and-multiply from the leading one down, the bit is wave-uniform
template <int WHICH, class F>
__device__ __forceinline__ F pow_const(const F& a) {
  constexpr int top = WHICH == 0 ? EXP_P14_TOP : WHICH == 1 ? EXP_P34_TOP : EXP_P12_TOP;
  F r = a;
#pragma unroll 1
  for (int b = top - 1; b >= 0; b--) {
    r = r.sqr();
    const uint32_t word = WHICH == 0 ? EXP_P14[b >> 5] : WHICH == 1 ? EXP_P34[b >> 5] : EXP_P12[b >> 5];
    if ((word >> (b & 31)) & 1u) r = r * a;
  }
  return r;
}

// a square root of a, *ok = it squares back to a (the caller's sign bit picks between it and its negative)
__device__ __forceinline__ Fq28 sqrt_verified(const Fq28& a, bool* ok) {
  const Fq28 s = pow_const<0>(a);
  *ok = (s.sqr() - a).is_zero();
  return s;
}
// Adj & Rodriguez-Henriquez, algorithm 9 (p = 3 mod 4) as wire.hip fq2_sqrt states it, without its branches: both
// candidate roots are formed, the test alpha = -1 selects, and squaring decides whether a root exists at all
__device__ __forceinline__ Fq2_28 sqrt_verified(const Fq2_28& a, bool* ok) {
  const Fq2_28 a1 = pow_const<1>(a);
  const Fq2_28 x0 = a1 * a;
  const Fq2_28 alpha = a1 * x0;
  const Fq2_28 one_alpha = Fq2_28::one() + alpha;
  const bool alpha_m1 = one_alpha.c0.is_zero() && alpha.c1.is_zero();
  const Fq2_28 b = pow_const<2>(one_alpha);
  Fq2_28 res = b * x0;
  const Fq2_28 ux0 = {x0.c1.neg(), x0.c0};
#pragma unroll
  for (int i = 0; i < Fq28::NL; i++) {
    res.c0.l[i] = alpha_m1 ? ux0.c0.l[i] : res.c0.l[i];
    res.c1.l[i] = alpha_m1 ? ux0.c1.l[i] : res.c1.l[i];
  }
  const Fq2_28 d = res.sqr() - a;
  *ok = d.c0.is_zero() && d.c1.is_zero();
  return res;
}

__device__ __forceinline__ void load_words_le(const uint32_t* q, uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = q[i];
}
__device__ __forceinline__ void load_words_be(const uint32_t* q, uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = __builtin_bswap32(q[11 - i]);
}
__device__ __forceinline__ void store_words(uint32_t* q, const uint32_t* w, bool mont) {
  Fq t;
#pragma unroll
  for (int i = 0; i < 12; i++) t.l[i] = w[i];
  if (mont) t = t.to_mont();
#pragma unroll
  for (int i = 0; i < 12; i++) q[i] = t.l[i];
}

// acc += p for acc != O by the mixed addition of curve.hpp, without its out-of-line doubling case (a call inside a
// kernel costs it the callee's register count and a scratch frame: msm_impl.hpp "call-free accumulation kernels").
// Returns false and leaves acc alone when p.x = acc.x, i.e. acc = +-p; *opposite then tells acc = -p.
template <class F>
__device__ __forceinline__ bool madd_or_meet(XYZZ<F>& acc, const Affine<F>& p, bool* opposite) {
  const F pp_ = f_sub_lazy(p.x * acc.zz, acc.x);
  const F r = f_sub_lazy(p.y * acc.zzz, acc.y);
  const F pp = pp_.sqr();
  const F rr = r.sqr();
  if (pp.is_zero()) {
    *opposite = !rr.is_zero();
    return false;
  }
  const F ppp = pp_ * pp;
  acc.zz = acc.zz * pp;
  acc.zzz = acc.zzz * ppp;
  const F q = acc.x * pp;
  acc.x = f_x3(rr, ppp, q);
  acc.y = f_mul_sub_mul(r, f_sub_lazy(q, acc.x), acc.y, ppp);
  return true;
}

// [r]P = O for a finite point P of the curve, by double-and-add over the bits of r from its leading one.  With
// k the multiple reached so far (1 < k < r), the running value can only meet +-P or O when the order of P divides
// k -+ 1 or k -- a number below r, so the order is not r and, r being prime and P not O, [r]P is not O either.  The one
// meeting that membership asks for is the last: r is odd, its final step adds P to [r-1]P = -P.  So the loop needs no
// doubling case and no addition to infinity: a lane that meets P early is outside the subgroup, says so, and goes on
// computing on a value nobody reads.  (Points of small order do meet it within a few steps.)
template <class F>
__device__ __forceinline__ bool mul_r_is_infinity(const Affine<F>& P) {
  XYZZ<F> acc = {P.x, P.y, F::one(), F::one()};
  bool early = false, closes = false;
#pragma unroll 1
  for (int b = EXP_R_TOP - 1; b >= 0; b--) {
    acc.dbl_inplace();
    if ((EXP_R[b >> 5] >> (b & 31)) & 1u) {
      bool opposite = false;
      const bool met = acc.is_inf() || !madd_or_meet(acc, P, &opposite);
      if (b == 0) closes = met && opposite;
      else early = early || met;
    }
  }
  return closes && !early;
}

// NC = 1: G1, 2: G2.  ENC = ZKMI_ENC_* or PT_ENC_RESIDENT.
template <int NC, int ENC>
__global__ __launch_bounds__(64, NC == 1 ? 2 : 1) void k_points_read(const uint32_t* __restrict__ in, uint64_t n, int checks,
                                                    uint32_t* __restrict__ out, int out_resident,
                                                    uint8_t* __restrict__ status, unsigned long long* first_bad,
                                                    uint64_t index_base) {
  using FO = FieldOf<NC>;
  using F = typename FO::F;
  constexpr bool COMPRESSED = ENC == ZKMI_ENC_ZCASH_COMPRESSED;
  constexpr bool BE_ENC = ENC == ZKMI_ENC_ZCASH_COMPRESSED || ENC == ZKMI_ENC_ZCASH_UNCOMPRESSED;
  constexpr int IN_WORDS = 12 * NC * (COMPRESSED ? 1 : 2);
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = gid < n;
  const uint64_t idx = live ? gid : n - 1;  // n >= 1 (host); tail lanes shadow the last element
  const uint32_t* q = in + idx * IN_WORDS;

  uint32_t st = ZKMI_PT_OK;
  bool inf = false, sort_flag = false;
  Words<NC> xw, yw;
  if (!BE_ENC) {
    // x.c0 (x.c1) y.c0 (y.c1), little-endian; infinity = all zero
#pragma unroll
    for (int c = 0; c < NC; c++) {
      load_words_le(q + 12 * c, xw.w[c]);
      load_words_le(q + 12 * (NC + c), yw.w[c]);
      if (ENC == PT_ENC_RESIDENT) {
        Fq t;
#pragma unroll
        for (int i = 0; i < 12; i++) t.l[i] = xw.w[c][i];
        t = t.from_mont();
#pragma unroll
        for (int i = 0; i < 12; i++) xw.w[c][i] = t.l[i];
#pragma unroll
        for (int i = 0; i < 12; i++) t.l[i] = yw.w[c][i];
        t = t.from_mont();
#pragma unroll
        for (int i = 0; i < 12; i++) yw.w[c][i] = t.l[i];
      }
    }
    inf = coord_zero(xw) && coord_zero(yw);
    if (!coord_lt_p(xw) || !coord_lt_p(yw)) st = ZKMI_PT_BAD_ENCODING;
  } else {
    // big-endian, the high component first (Fq2: c1 || c0); byte 0 carries the flags
#pragma unroll
    for (int c = 0; c < NC; c++) {
      load_words_be(q + 12 * c, xw.w[NC - 1 - c]);
      if (!COMPRESSED) load_words_be(q + 12 * (NC + c), yw.w[NC - 1 - c]);
      else
#pragma unroll
        for (int i = 0; i < 12; i++) yw.w[c][i] = 0;
    }
    const uint32_t top = xw.w[NC - 1][11];
    const uint32_t flags = top >> 29;  // bit 2: compressed, bit 1: infinity, bit 0: sort
    if (((flags >> 2) & 1u) != (COMPRESSED ? 1u : 0u)) st = ZKMI_PT_BAD_ENCODING;
    if (flags & 2u) {
      // the one encoding of infinity: the flag byte alone (0xC0 / 0x40), every other bit zero
      inf = true;
      xw.w[NC - 1][11] = top & 0x00ffffffu;
      if ((top >> 24) != (COMPRESSED ? 0xC0u : 0x40u) || !coord_zero(xw) || !coord_zero(yw)) st = ZKMI_PT_BAD_ENCODING;
    } else {
      sort_flag = (flags & 1u) != 0;
      if (COMPRESSED) xw.w[NC - 1][11] = top & 0x1fffffffu;
      else if (flags & 1u) st = ZKMI_PT_BAD_ENCODING;
      if (!coord_lt_p(xw) || !coord_lt_p(yw)) st = ZKMI_PT_BAD_ENCODING;
    }
  }
  if (inf) {
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
      for (int i = 0; i < 12; i++) xw.w[c][i] = yw.w[c][i] = 0;
  }

  const F x = FO::from_words(xw);
  F y;
  if (COMPRESSED) {
    bool ok;
    const F a = x.sqr() * x + FO::curve_b();
    y = sqrt_verified(a, &ok);
    if (!ok && !inf && st == ZKMI_PT_OK) st = ZKMI_PT_NOT_ON_CURVE;
    FO::to_words(y, &yw);
    if (coord_lex_larger(yw) != sort_flag) coord_neg(&yw);
    if (inf) {
#pragma unroll
      for (int c = 0; c < NC; c++)
#pragma unroll
        for (int i = 0; i < 12; i++) yw.w[c][i] = 0;
    }
    y = FO::from_words(yw);
  } else {
    y = FO::from_words(yw);
    if (checks & ZKMI_CHECK_CURVE) {
      const F d = y.sqr() - (x.sqr() * x + FO::curve_b());
      if (!FO::is_zero(d) && !inf && st == ZKMI_PT_OK) st = ZKMI_PT_NOT_ON_CURVE;
    }
  }

  // outputs before the long loop: the canonical words are dead after this
  if (out && live) {
    uint32_t* o = out + gid * (24 * NC);
#pragma unroll
    for (int c = 0; c < NC; c++) {
      store_words(o + 12 * c, xw.w[c], out_resident != 0);
      store_words(o + 12 * (NC + c), yw.w[c], out_resident != 0);
    }
  }

  if (checks & ZKMI_CHECK_SUBGROUP) {
    const Affine<F> P = {x, y};
    if (!mul_r_is_infinity(P) && !inf && st == ZKMI_PT_OK) st = ZKMI_PT_NOT_IN_SUBGROUP;
  }

  if (live) {
    if (status) status[gid] = (uint8_t)st;
    if (st != ZKMI_PT_OK) atomicMin(first_bad, (unsigned long long)(((index_base + gid) << 2) | st));
  }
}

template <int NC>
void launch(int32_t enc, const void* d_in, uint64_t n, int32_t checks, void* d_out, bool out_resident, void* d_status,
            unsigned long long* d_first, uint64_t index_base, hipStream_t st) {
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  const uint32_t* in = static_cast<const uint32_t*>(d_in);
  uint32_t* out = static_cast<uint32_t*>(d_out);
  uint8_t* stat = static_cast<uint8_t*>(d_status);
  const int res = out_resident ? 1 : 0;
  switch (enc) {
    case ZKMI_ENC_WIRE:
      hipLaunchKernelGGL((k_points_read<NC, ZKMI_ENC_WIRE>), grid, block, 0, st, in, n, checks, out, res, stat, d_first, index_base);
      break;
    case ZKMI_ENC_ZCASH_COMPRESSED:
      hipLaunchKernelGGL((k_points_read<NC, ZKMI_ENC_ZCASH_COMPRESSED>), grid, block, 0, st, in, n, checks, out, res, stat, d_first, index_base);
      break;
    case ZKMI_ENC_ZCASH_UNCOMPRESSED:
      hipLaunchKernelGGL((k_points_read<NC, ZKMI_ENC_ZCASH_UNCOMPRESSED>), grid, block, 0, st, in, n, checks, out, res, stat, d_first, index_base);
      break;
    default:
      hipLaunchKernelGGL((k_points_read<NC, PT_ENC_RESIDENT>), grid, block, 0, st, in, n, checks, out, res, stat, d_first, index_base);
      break;
  }
}

// one launch; *d_first is the caller's device word, already set
hipError_t run(zkmi_ctx* ctx, int group, const void* d_in, uint64_t n, int32_t enc, int32_t checks, void* d_out,
               bool out_resident, void* d_status, unsigned long long* d_first, uint64_t index_base) {
  PhaseTimer* t = ctx->timer();  // device events around the launch when profiling is on (zkmi_prof_get, phase "misc")
  if (t) t->begin(PH_MISC, ctx->stream);
  if (group == 1) launch<1>(enc, d_in, n, checks, d_out, out_resident, d_status, d_first, index_base, ctx->stream);
  else launch<2>(enc, d_in, n, checks, d_out, out_resident, d_status, d_first, index_base, ctx->stream);
  const hipError_t e = hipGetLastError();
  if (t) t->end(PH_MISC, ctx->stream);
  return e;
}

void split_key(unsigned long long key, uint64_t* first_bad, uint32_t* bad_status) {
  const bool none = key == ~0ull;
  if (first_bad) *first_bad = none ? UINT64_MAX : (uint64_t)(key >> 2);
  if (bad_status) *bad_status = none ? (uint32_t)ZKMI_PT_OK : (uint32_t)(key & 3u);
}

}  // namespace

uint64_t point_bytes(int group, int32_t enc) {
  const uint64_t full = group == 1 ? 96 : 192;
  return enc == ZKMI_ENC_ZCASH_COMPRESSED ? full / 2 : full;
}

bool point_args_ok(int32_t enc, int32_t* checks) {
  if (enc != ZKMI_ENC_WIRE && enc != ZKMI_ENC_ZCASH_COMPRESSED && enc != ZKMI_ENC_ZCASH_UNCOMPRESSED && enc != PT_ENC_RESIDENT)
    return false;
  if (*checks & ~(ZKMI_CHECK_CURVE | ZKMI_CHECK_SUBGROUP)) return false;
  if ((*checks & ZKMI_CHECK_SUBGROUP) || enc == ZKMI_ENC_ZCASH_COMPRESSED) *checks |= ZKMI_CHECK_CURVE;
  return true;
}

const char* point_status_name(uint32_t st) {
  switch (st) {
    case ZKMI_PT_OK: return "ok";
    case ZKMI_PT_BAD_ENCODING: return "bad encoding";
    case ZKMI_PT_NOT_ON_CURVE: return "not on the curve";
    default: return "not in the prime-order subgroup";
  }
}

int32_t points_read(zkmi_ctx* ctx, int group, const void* d_in, uint64_t n, int32_t enc, int32_t checks, void* d_out,
                    bool out_resident, void* d_status, uint64_t* first_bad, uint32_t* bad_status) {
  if (!ctx || !d_in || n == 0 || n >= (1ull << 40) || (group != 1 && group != 2) || !point_args_ok(enc, &checks) ||
      (reinterpret_cast<uintptr_t>(d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & 3u))
    return ZKMI_ERR_BAD_ARG;
  unsigned long long* d_first = nullptr;
  ZK_HIP(ctx, hipMalloc(&d_first, sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(d_first, 0xff, sizeof(unsigned long long), ctx->stream);
  if (e == hipSuccess) e = run(ctx, group, d_in, n, enc, checks, d_out, out_resident, d_status, d_first, 0);
  unsigned long long key = ~0ull;
  if (e == hipSuccess) e = hipMemcpyAsync(&key, d_first, sizeof(key), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // also on an error path: nothing may still use d_first
  if (e == hipSuccess) e = es;
  (void)hipFree(d_first);
  if (e != hipSuccess) return ctx->hip_fail(e, "points read");
  split_key(key, first_bad, bad_status);
  return ZKMI_OK;
}

int32_t points_read_host(zkmi_ctx* ctx, int group, const uint8_t* host, uint64_t n, int32_t enc, int32_t checks,
                         void* d_out_resident, uint64_t* first_bad, uint32_t* bad_status) {
  if (!ctx || !host || !d_out_resident || n == 0 || (group != 1 && group != 2) || !point_args_ok(enc, &checks))
    return ZKMI_ERR_BAD_ARG;
  const uint64_t CH = 1ull << 20;  // elements per upload: at most 192 MiB of staging
  const uint64_t w = point_bytes(group, enc), wout = group == 1 ? 96 : 192;
  ZK_HIP(ctx, ctx->staging((n < CH ? n : CH) * w + sizeof(unsigned long long)));
  // the result word lives in front of the chunk (8 bytes keep the elements aligned)
  unsigned long long* d_first = static_cast<unsigned long long*>(ctx->d_tmp);
  uint8_t* d_chunk = static_cast<uint8_t*>(ctx->d_tmp) + sizeof(unsigned long long);
  unsigned long long key = ~0ull;
  hipError_t e = hipMemsetAsync(d_first, 0xff, sizeof(unsigned long long), ctx->stream);
  for (uint64_t first = 0; first < n && e == hipSuccess && key == ~0ull; first += CH) {
    const uint64_t c = n - first < CH ? n - first : CH;
    e = hipMemcpyAsync(d_chunk, host + first * w, c * w, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
      e = run(ctx, group, d_chunk, c, enc, checks, static_cast<uint8_t*>(d_out_resident) + first * wout, true, nullptr, d_first, first);
    if (e == hipSuccess) e = hipMemcpyAsync(&key, d_first, sizeof(key), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return ctx->hip_fail(e, "points upload / read");
  }
  split_key(key, first_bad, bad_status);
  return ZKMI_OK;
}

}  // namespace zkmi
