// zkmi — Pippenger bucket-method MSM on gfx950, templated on the base field
// (F = Fq -> G1, F = Fq2 -> G2).
//
// Reference locus: none in /root/reference.  The
// value computed is sum_i s_i * P_i, the same group element
// ark_ec::VariableBaseMSM::msm_bigint / halo2curves::msm::best_multiexp
// return; any correct bucket schedule is bit-exact after affine normalisation.
//
// HBM layout
//   scalars   : n x 32 B canonical little-endian integers < r (NOT Montgomery)
//   bases     : n x Affine<F>, F = 14 x 28-bit limbs (field28.hpp), (0,0) = infinity
//   blockhist : nwin*nch*nb x u32  per-(window, chunk) tile histograms -> tile base slots
//   count/begin : nwin*nb x u32    points per bucket / first slot in sorted[]
//   sorted    : nwin*n x u32       point index | sign<<31, grouped by bucket
//   buckets   : nwin*nb x XYZZ<F>
//   segsum / segw : nwin*nb/SEG x XYZZ<F>
//   partial   : nwin*(1+log2(nb/SEG)) x XYZZ<host field>   -> host
//
// Kernel chain (all on one stream):
//   1 k_bucket_pass<false>  (window, chunk) tile: carry-free signed digits, LDS histogram
//                           (2^15 u32 counters = 128 KiB of the CU's 160 KiB LDS)
//   2 k_bucket_totals / k_window_scan / k_bucket_bases   prefix sums -> slots
//   3 k_bucket_pass<true>   same tiles: LDS cursors (ds_add_rtn) -> sorted[]   (bucket scatter)
//   4 k_accum_g1_nc / k_accum_g2_nc   thread (lane pair) per bucket : gather affine points, XYZZ mixed adds   <- dominant
//     k_accum_heavy[_g2_split]  workgroups per heavy bucket (the last one of a split bucket adds the sub-range sums),
//     k_accum_redo[_g2_split]   buckets that met P + P, with the complete addition
//   5 k_segreduce thread/2..16 buckets : running-sum  sum (i+1) B_i  and  sum B_i
//   5b k_segreduce2 (one-lane reductions of shared-bucket plans with >= 256 segments per window): the same running sums
//                 over 16 consecutive segsum entries -- segsum2 and segt2, see TreeLevel2
//   6 k_treesum   block/(window, job[, slice]) : plain sums (LDS tree) of segw, and of
//                 segsum over {t : bit j of t set}; small plans: slices + k_treesum_final
//   Steps 4 - 6 have ONE body per algorithm, over a lane layout (OneLane<F>: a lane per point; LanePair: a G2 point across a
//   lane pair): see "Lane layouts" and "The two accumulation chains" below.
//   host: window_w = P[w][0] + SEG * sum_j 2^j P[w][1+j];  result = sum_w 2^(c w) window_w
//         (with 5b: window_w = P[w][0] + SEG * (T[w] + 16 * sum_j 2^j P2[w][1+j]), windows_from_partials)
#pragma once
#include <stdlib.h>
#include <functional>
#include <type_traits>
#include <vector>
#include "curve.hpp"
#include "host_pool.hpp"
#include "msm.hpp"

namespace zkmi {

// segment arrays: 16-bucket segments for big plans, down to 1-bucket segments for plans of <= 2^16 buckets
static inline uint64_t msm_max_segments(uint64_t buckets) { return (buckets / 16 > (1u << 16) ? buckets / 16 : (1u << 16)) + 1; }
constexpr int MSM_SEG2_LOG = 4;             // k_segreduce2: segment sums per super-segment (log2)
constexpr uint32_t MSM_SEG2_MIN_SEGS = 256;  // ... where a window has at least this many segments
constexpr int MSM_TREE_T = 128;  // k_treesum block: 128 x XYZZ<Fq2> = 56 KiB LDS
constexpr uint32_t MSM_STAGE_PTS = 16384;  // slices of one slot's tree-sum job lists (k_treesum_q; the one-lane k_treesum uses the first MSM_STAGE_PTS_1)
constexpr uint32_t MSM_STAGE_PTS_1 = 4096;
constexpr uint32_t MSM_HEAVY = 256;  // load-ordering key range; the heavy threshold itself is plan.heavy_thr

template <class T>
__device__ __forceinline__ T load_vec(const T* p) {
  static_assert(sizeof(T) % 16 == 0, "16-byte multiple");
  T r;
  const uint4* s = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
  return r;
}
template <class T>
__device__ __forceinline__ void store_vec(T* p, const T& v) {
  static_assert(sizeof(T) % 16 == 0, "16-byte multiple");
  const uint4* s = reinterpret_cast<const uint4*>(&v);
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;


// G2 accumulation with every Fq2 value split across a lane pair (field28.hpp Fq2P):
// two adjacent lanes own one bucket; per-lane state is that of a G1 addition, so the
// kernel runs at 2 waves per SIMD instead of 1.  Memory layouts are the unsplit ones
// (x.c0, x.c1, y.c0, y.c1, ...): a lane simply reads / writes its own components.
__device__ __forceinline__ Fq28 ld_comp(const Fq28* p) {
  Fq28 r;
  const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const uint2 w = q[i];
    r.l[2 * i] = (int32_t)w.x;
    r.l[2 * i + 1] = (int32_t)w.y;
  }
  return r;
}
__device__ __forceinline__ void st_comp(Fq28* p, const Fq28& v) {
  uint2* q = reinterpret_cast<uint2*>(p);
#pragma unroll
  for (int i = 0; i < 7; i++) q[i] = make_uint2((uint32_t)v.l[2 * i], (uint32_t)v.l[2 * i + 1]);
}


// ---------------------------------------------------------------------------------------------
// Call-free accumulation kernels.  XYZZ::madd keeps its rare doubling case in an out-of-line function;
// a call inside the hot kernel costs more than code size: the kernel's register count becomes the
// callee's (231-248 VGPRs whatever __launch_bounds__ asks for) and the frame needs scratch.  Here the
// doubling case (two equal points in one bucket: repeated bases with equal digits) never happens in
// the kernel: the lane appends its bucket to a redo list and stops; k_accum_redo recomputes the
// listed buckets with the complete addition afterwards.  The list holds bucket ids, so it cannot
// overflow (capacity = number of buckets).
// ---------------------------------------------------------------------------------------------
// acc += p for acc != O, p != O; returns false when the sum needs the complete group law (p = +-acc):
// the caller hands the bucket to k_accum_redo.  No state besides acc: the loop around it has one path.
// negmask = 0xffffffff adds -p instead of p (the sign of the digit): folded into the lazy difference R = +-(y zzz) - Y
template <class F>
__host__ __device__ __forceinline__ bool madd_generic(XYZZ<F>& acc, const Affine<F>& p, uint32_t negmask = 0) {
  F pp_ = f_sub_lazy(p.x * acc.zz, acc.x);
  F r = f_signed_sub_lazy(p.y * acc.zzz, negmask, acc.y);
  F pp = pp_.sqr();
  F rr = r.sqr();
  if (pp.is_zero()) return false;
  F ppp = pp_ * pp;
  acc.zz = acc.zz * pp;
  acc.zzz = acc.zzz * ppp;
  F q = acc.x * pp;
  acc.x = f_x3(rr, ppp, q);
  acc.y = f_mul_sub_mul(r, f_sub_lazy(q, acc.x), acc.y, ppp);
  return true;
}
// The same for an accumulator that is still ONE affine point (x, y set; zz = zzz = 1 implied and never read): EFD "xyzz"
// mmadd-2008-s, 4M + 2S.  madd_generic would multiply p.x, p.y, pp and ppp by one here: four products of the ten, once per
// bucket.  Same contract (false: p = +-acc, nothing written) and the same lazy differences; sets all four coordinates.
template <class F>
__host__ __device__ __forceinline__ bool madd_affine_pair(XYZZ<F>& acc, const Affine<F>& p, uint32_t negmask = 0) {
  F pp_ = f_sub_lazy(p.x, acc.x);
  F r = f_signed_sub_lazy(p.y, negmask, acc.y);
  F pp = pp_.sqr();
  F rr = r.sqr();
  if (pp.is_zero()) return false;
  F ppp = pp_ * pp;
  F q = acc.x * pp;
  acc.x = f_x3(rr, ppp, q);
  acc.y = f_mul_sub_mul(r, f_sub_lazy(q, acc.x), acc.y, ppp);
  acc.zz = pp;
  acc.zzz = ppp;
  return true;
}
// device table entries at infinity are exact zeros (k_bases_convert, k_build_table); one limb decides for all but
// 2^-28 of the finite entries, the full test runs behind that branch
template <class P>
__device__ __forceinline__ bool affine_is_zero_words(const Affine<Fp28<P>>& p) {
  if (p.y.l[0] != 0) return false;
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < P::NL; i++) o |= (uint32_t)p.x.l[i] | (uint32_t)p.y.l[i];
  return o == 0;
}

// ---------------------------------------------------------------------------------------------
// Lane layouts.  The accumulation chains and every reduction-side algorithm (redo, heavy buckets, segment sums, tree sums)
// have ONE body each, written over a layout L that says how a point lies across lanes; the __global__ entry points around a
// body differ in layout, stride and __launch_bounds__ only.
//   OneLane<F>  a lane per point (G1, BN254 G1; the unsplit G2 tree sum of the A/B library)
//   LanePair    a lane pair per G2 point, one Fq2 component per lane (field28.hpp Fq2P, see k_accum_g2_nc): per-lane state
//               is that of a G1 addition.  The unsplit forms are 330-register kernels with 45-75 us per dependent addition:
//               0.8 ms for one 600-point bucket of a 2^14 proof, on the critical path of the G2 reduction; and 0.1 ms to
//               place an EMPTY redo kernel.
// Memory layouts are the unsplit ones for both.  Thread i (of the workgroup, or of the grid) is lane `comp` = i % LANES of
// point i / LANES, and every branch around an addition is uniform over the lanes of a point.
// ---------------------------------------------------------------------------------------------
template <class F>
struct OneLane {
  typedef XYZZ<F> Stored;                             // the point in memory
  typedef XYZZ<F> P;                                  // what a lane holds of it
  typedef XYZZ<typename HostFieldOf<F>::type> Host;   // the host-representation point
  typedef Affine<F> Base;                             // a table entry in memory
  static constexpr uint32_t LANES = 1;
  __device__ __forceinline__ static P load(const Stored* p, uint32_t) { return load_vec(p); }
  __device__ __forceinline__ static void store(Stored* p, const P& v, uint32_t) { store_vec(p, v); }
  __device__ __forceinline__ static void store_host(Host* p, const P& v, uint32_t) {
    const Host o = {fq_from_fq28(v.x), fq_from_fq28(v.y), fq_from_fq28(v.zz), fq_from_fq28(v.zzz)};
    store_vec(p, o);
  }
  // the table entry of a sorted[] word, negated where the word's sign bit is set
  __device__ __forceinline__ static Affine<F> load_affine(const Base* bases, uint32_t v, uint32_t) {
    Affine<F> p = load_vec(bases + (v & 0x7fffffffu));
    if (v >> 31) p.y = p.y.neg();
    return p;
  }
  // heavy_marker() left by k_accum_heavy_nc: "infinity" with zzz word 0 set; *empty: all zz words zero, marker or not
  __device__ __forceinline__ static bool is_marker(const P& v, uint32_t, bool* empty) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < F::NL; i++) o |= (uint32_t)v.zz.l[i];
    *empty = o == 0;
    return o == 0 && v.zzz.l[0] == 1;
  }
  // a coordinate as the lane at distance `dist` holds it
  __device__ __forceinline__ static F shfl_xor(const F& a, int dist) {
    F r;
#pragma unroll
    for (int i = 0; i < F::NL; i++) r.l[i] = __shfl_xor(a.l[i], dist);
    return r;
  }
};
struct LanePair {
  typedef XYZZ<Fq2_28> Stored;  // x.c0 x.c1 y.c0 y.c1 zz.c0 zz.c1 zzz.c0 zzz.c1: lane `comp` reads / writes every second one
  typedef XYZZ<Fq2P> P;
  typedef XYZZ<Fq2> Host;
  typedef Affine<Fq2_28> Base;
  static constexpr uint32_t LANES = 2;
  __device__ __forceinline__ static P load(const Stored* p, uint32_t comp) {
    const Fq28* s = reinterpret_cast<const Fq28*>(p);
    P r;
    r.x.v = ld_comp(s + comp);
    r.y.v = ld_comp(s + 2 + comp);
    r.zz.v = ld_comp(s + 4 + comp);
    r.zzz.v = ld_comp(s + 6 + comp);
    return r;
  }
  __device__ __forceinline__ static void store(Stored* p, const P& v, uint32_t comp) {
    Fq28* d = reinterpret_cast<Fq28*>(p);
    st_comp(d + comp, v.x.v);
    st_comp(d + 2 + comp, v.y.v);
    st_comp(d + 4 + comp, v.zz.v);
    st_comp(d + 6 + comp, v.zzz.v);
  }
  // what a pair of k_accum_heavy_nc_g2 without a partial sum leaves: infinity, and `marked` -- it met P + P or P - P,
  // k_accum_heavy_g2_split recomputes the pair's points -- with zzz.c0 word 0 = 1 (ONE store path for both: a branch of
  // its own for the plain infinity cost the kernel 8 - 52 bytes of scratch)
  __device__ __forceinline__ static void store_marker(Stored* p, bool marked, uint32_t comp) {
    P m = P::infinity();
    m.zzz.v.l[0] = (marked && comp == 0) ? 1 : 0;
    store(p, m, comp);
  }
  __device__ __forceinline__ static void store_host(Host* p, const P& v, uint32_t comp) {
    Fq* d = reinterpret_cast<Fq*>(p);
    d[comp] = fq_from_fq28(v.x.v);
    d[2 + comp] = fq_from_fq28(v.y.v);
    d[4 + comp] = fq_from_fq28(v.zz.v);
    d[6 + comp] = fq_from_fq28(v.zzz.v);
  }
  // The lane's component of the table entry of a sorted[] word, NO sign applied (the caller does: first point, or folded
  // into the addition); true = the point at infinity.  Infinity = all four components exact zeros: OR of this lane's words,
  // combined with the partner's; the lowest limb of y decides for all but 2^-56 of the finite entries, the full test runs
  // behind that (pair-uniform) branch.  Each DPP swap stands in front of the branch that depends on it.
  __device__ __forceinline__ static bool load_entry(const Base* bases, uint32_t v, uint32_t comp, Affine<Fq2P>& p) {
    const Fq28* src = reinterpret_cast<const Fq28*>(bases + (v & 0x7fffffffu));  // x.c0 x.c1 y.c0 y.c1
    p.x.v = ld_comp(src + comp);
    p.y.v = ld_comp(src + 2 + comp);
    uint32_t o = (uint32_t)p.y.v.l[0];
    o |= (uint32_t)__builtin_amdgcn_mov_dpp((int)o, 0xB1, 0xF, 0xF, true);
    if (o != 0) return false;
#pragma unroll
    for (int i = 0; i < Fq28::NL; i++) o |= (uint32_t)p.x.v.l[i] | (uint32_t)p.y.v.l[i];
    o |= (uint32_t)__builtin_amdgcn_mov_dpp((int)o, 0xB1, 0xF, 0xF, true);
    return o == 0;
  }
  __device__ __forceinline__ static Affine<Fq2P> load_affine(const Base* bases, uint32_t v, uint32_t comp) {
    const Fq28* src = reinterpret_cast<const Fq28*>(bases + (v & 0x7fffffffu));  // x.c0 x.c1 y.c0 y.c1
    Affine<Fq2P> p;
    p.x.v = ld_comp(src + comp);
    p.y.v = ld_comp(src + 2 + comp);
    if (v >> 31) p.y = p.y.neg();
    return p;
  }
  // the marker of k_accum_heavy_nc_g2 is zzz.c0 word 0: both tests ORed over the pair with one DPP swap each
  __device__ __forceinline__ static bool is_marker(const P& v, uint32_t comp, bool* empty) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < Fq28::NL; i++) o |= (uint32_t)v.zz.v.l[i];
    uint32_t mk = (comp == 0 && v.zzz.v.l[0] == 1) ? 1u : 0u;
    o |= (uint32_t)__builtin_amdgcn_mov_dpp((int)o, 0xB1, 0xF, 0xF, true);
    mk |= (uint32_t)__builtin_amdgcn_mov_dpp((int)mk, 0xB1, 0xF, 0xF, true);
    *empty = o == 0;
    return o == 0 && mk == 1;
  }
  __device__ __forceinline__ static Fq2P shfl_xor(const Fq2P& a, int dist) { return {OneLane<Fq28>::shfl_xor(a.v, dist)}; }
};

// ---------------------------------------------------------------------------------------------
// The two accumulation chains.  accum_first starts a sum with the first finite entry of sorted[j], sorted[j + STRIDE], ...
// (x and y, the digit's sign applied; j ends up behind that entry; false: there was none), accum_chain adds the finite
// entries behind it and returns true when an addition met P + P or P - P (the caller hands the bucket to the redo list, or
// leaves a marker), through ONE exit behind its loops.  FIRST_IS_AFFINE: acc holds x and y of one affine point, and the
// first finite entry behind it is added with madd_affine_pair (4M + 2S); otherwise all four coordinates are set.  They are
// two bodies because they are two loop shapes, each the one its kernels' allocation stands on:
//   OneLane   the next entry prefetched through the wave's LDS column (PrefetchTile), the pair step ONE peeled iteration,
//             a count-down of `rem` entries (the light kernel's zero-scratch allocation needs the count)
//   LanePair  entries loaded through registers (LanePair::load_entry), the pair step a search loop, j < end (wave-uniform
//             in the heavy kernel, where a per-lane count costs 4 - 5 registers)
// ---------------------------------------------------------------------------------------------
// The per-wave prefetch column of the one-lane chain: one table entry per lane, fetched by seven (BLS12-381 Fq) or five
// (BN254 Fq) direct-to-LDS loads of 16 bytes (per-lane source address, destination = wave-uniform LDS base + 16 B x lane).
// ONE buffer: take() reads the entry into registers at the top of an iteration, so the column is free for the next fetch()
// straight away: 7 KB per wave.  What orders take()'s reads behind the fetch is the compiler's own wait for the LDS-DMA, and
// it places that wait only where it believes the two may alias: NO __restrict__ on the pointer parameters of a function that
// fetches (inlined, they become no-alias scopes, the reads count as independent of the DMA and are issued in front of the
// vmcnt wait -- stale entries, wrong sums, no fault).  The rule covers the functions that fetch through this tile; the
// lane-pair chain below loads through registers and keeps its qualifiers.
template <class F>
struct PrefetchTile {
  static constexpr int CHUNKS = sizeof(Affine<F>) / 16;
  typedef uint4 Column[CHUNKS][64];  // [chunk][lane], in LDS
  uint4 (*col)[64];
  uint32_t lane;
  __device__ __forceinline__ void fetch(const Affine<F>* bases, uint32_t v) const {
    const char* src = reinterpret_cast<const char*>(bases + (v & 0x7fffffffu));
#pragma unroll
    for (int q = 0; q < CHUNKS; q++)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + 16 * q), (lds_ptr_t)&col[q][0], 16, 0, 0);
  }
  __device__ __forceinline__ void take(Affine<F>& p) const {  // LDS -> registers; the compiler waits for the outstanding LDS-DMA first
    uint4* d = reinterpret_cast<uint4*>(&p);
#pragma unroll
    for (int q = 0; q < CHUNKS; q++) d[q] = col[q][lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads have left the LDS: the buffer may be refilled
  }
};
template <class F, bool FIRST_IS_AFFINE, uint32_t STRIDE>
__device__ __forceinline__ bool accum_chain(XYZZ<F>& acc, const Affine<F>* bases, const uint32_t* sorted, uint32_t j, uint32_t rem,
                                            const PrefetchTile<F>& tile) {
  bool bad = false;
  uint32_t v_cur = 0, v_next = 0;
  if (rem > 0) {
    v_cur = sorted[j];
    tile.fetch(bases, v_cur);
    if (rem > 1) v_next = sorted[j + STRIDE];
  }
  if constexpr (FIRST_IS_AFFINE) {
    // The entry behind the first meets an accumulator that is still affine.  Lanes of a wave own buckets of near-equal load,
    // so the wave takes this step together.  It is one peeled iteration of the loop below (same tile, same prefetch), not a
    // loop of its own: an entry at infinity HERE (exceptional) leaves zz = zzz = 1 and the generic additions take over.  A
    // search loop for "the next finite entry" spilt 144 - 228 bytes per lane.
    bool paired = false;
    if (rem > 0) {
      Affine<F> p;
      tile.take(p);
      const uint32_t v = v_cur;
      if (rem > 1) {
        tile.fetch(bases, v_next);
        v_cur = v_next;
        if (rem > 2) v_next = sorted[j + 2 * STRIDE];
      }
      rem--;
      j += STRIDE;
      if (!affine_is_zero_words(p)) {
        bad = !madd_affine_pair(acc, p, 0u - (v >> 31));
        paired = true;
      }
    }
    if (!paired) {
      acc.zz = F::one();
      acc.zzz = F::one();
    }
    if (bad) rem = 0;
  }
  // ONE exit behind the loop for both outcomes, and a count-down instead of (j, end): with a return to the redo list inside
  // the loop or in front of it the register allocator spilt 12 - 124 bytes per lane around the pair step; this form needs
  // no scratch in the light kernel (tests/test_cpu_host.py::test_kernel_register_budgets holds it to that).
  for (; rem > 0; rem--, j += STRIDE) {
    Affine<F> p;
    tile.take(p);
    const uint32_t v = v_cur;
    if (rem > 1) {
      tile.fetch(bases, v_next);
      v_cur = v_next;
      if (rem > 2) v_next = sorted[j + 2 * STRIDE];
    }
    if (affine_is_zero_words(p)) continue;
    if (!madd_generic(acc, p, 0u - (v >> 31))) {
      bad = true;
      break;
    }
  }
  return bad;
}
// (plain loads: runs once per chain)
template <class F, uint32_t STRIDE>
__device__ __forceinline__ bool accum_first(XYZZ<F>& acc, const Affine<F>* bases, const uint32_t* sorted, uint32_t& j, uint32_t& rem) {
  bool have = false;
  for (; rem > 0 && !have; rem--, j += STRIDE) {
    const uint32_t v = sorted[j];
    Affine<F> p = load_vec(bases + (v & 0x7fffffffu));
    if (affine_is_zero_words(p)) continue;
    if (v >> 31) p.y = p.y.neg();
    acc.x = p.x;
    acc.y = p.y;
    have = true;
  }
  return have;
}
template <uint32_t STRIDE>
__device__ __forceinline__ bool accum_first(XYZZ<Fq2P>& acc, const LanePair::Base* __restrict__ bases, const uint32_t* __restrict__ sorted,
                                            uint32_t& j, uint32_t end, uint32_t comp) {
  bool have = false;
  for (; j < end && !have; j += STRIDE) {
    Affine<Fq2P> p;
    const uint32_t v = sorted[j];
    if (LanePair::load_entry(bases, v, comp, p)) continue;
    acc.x = p.x;
    acc.y = (v >> 31) ? p.y.neg() : p.y;
    have = true;
  }
  return have;
}
template <uint32_t STRIDE, bool FIRST_IS_AFFINE>
__device__ __forceinline__ bool accum_chain(XYZZ<Fq2P>& acc, const LanePair::Base* __restrict__ bases, const uint32_t* __restrict__ sorted,
                                            uint32_t j, uint32_t end, uint32_t comp) {
  bool bad = false, paired = !FIRST_IS_AFFINE;
  for (; j < end && !paired && !bad; j += STRIDE) {
    Affine<Fq2P> p;
    const uint32_t v = sorted[j];
    if (LanePair::load_entry(bases, v, comp, p)) continue;
    if (madd_affine_pair(acc, p, 0u - (v >> 31))) paired = true;  // pair-uniform (Fq2P::is_zero exchanges the halves)
    else bad = true;
  }
  if (!paired) {  // one finite entry (or bad)
    acc.zz = Fq2P::one();
    acc.zzz = Fq2P::one();
  }
  for (; j < end && !bad; j += STRIDE) {
    Affine<Fq2P> p;
    const uint32_t v = sorted[j];
    if (LanePair::load_entry(bases, v, comp, p)) continue;
    if (!madd_generic(acc, p, 0u - (v >> 31))) bad = true;  // pair-uniform
  }
  return bad;
}

// G1 (and BN254 G1): thread per bucket, the one-lane chain over the bucket's entries.
// What one launch accumulates: one MSM (table, bucket array, redo list + the digit sort it reads), or up to four MSMs of
// the same shape, one per blockIdx.y -- the A, B1, L queries of a proof over the sort of z and the H query over the sort of
// h.  One small proof uses the second form: 256-wave grids on separate streams did not start together (a kernel that
// cannot place all its workgroups at once holds its dispatch pipe, and the other streams of that pipe wait).
constexpr int MSM_MULTI_MAX = 4;
struct SortView {
  const uint32_t *begin, *count, *perm, *sorted;
  uint32_t heavy_thr;
};
template <class F, bool MULTI>
struct AccumArgs;
template <class F>
struct AccumArgs<F, false> {
  const Affine<F>* bases_;
  XYZZ<F>* buckets_;
  uint32_t* redo_;
  SortView sort_;
  __device__ __forceinline__ const Affine<F>* bases() const { return bases_; }
  __device__ __forceinline__ XYZZ<F>* buckets() const { return buckets_; }
  __device__ __forceinline__ uint32_t* redo() const { return redo_; }
  __device__ __forceinline__ const SortView& sort() const { return sort_; }
};
template <class F>
struct AccumArgs<F, true> {
  const Affine<F>* bases_[MSM_MULTI_MAX];
  XYZZ<F>* buckets_[MSM_MULTI_MAX];
  uint32_t* redo_[MSM_MULTI_MAX];
  SortView sort_[MSM_MULTI_MAX];
  __device__ __forceinline__ const Affine<F>* bases() const { return bases_[blockIdx.y]; }
  __device__ __forceinline__ XYZZ<F>* buckets() const { return buckets_[blockIdx.y]; }
  __device__ __forceinline__ uint32_t* redo() const { return redo_[blockIdx.y]; }
  __device__ __forceinline__ const SortView& sort() const { return sort_[blockIdx.y]; }
};
// INTO: the bucket array already holds the sums of an earlier MSM over the same bucket set (another query whose result is
// only ever ADDED to this one's: the prover's L and H queries both end up in C).  The accumulator then
// starts from the bucket's value instead of the first entry, an empty entry list leaves the bucket alone, and one
// reduction serves both MSMs.  A bucket the earlier MSM left EMPTY (exact zeros; probability e^-(mean load)) needs no
// test of its own: with acc = (0, 0, 0, 0) the first addition computes P = x zz - X = 0, which is the "needs the complete
// group law" exit below -- the bucket goes to the redo pass, whose complete addition starts from infinity.
// (Any early exit through the redo list IN FRONT of the chain made the register allocator spill 120 dwords inside its
// loop; with the chain's one exit behind the loop this form spills 3, and the plain kernel needs no scratch.)
// The body is a function because the occupancy-capped k_accum_g1_nc_w2 of the A/B library (msm_impl_exp.hpp) is the same
// code under other attributes.
template <class F, int BW, bool MULTI, bool INTO>
__device__ __forceinline__ void accum_g1_nc_body(const AccumArgs<F, MULTI>& args, uint32_t total_buckets) {
  const Affine<F>* __restrict__ const bases = args.bases();
  XYZZ<F>* __restrict__ const buckets = args.buckets();
  uint32_t* __restrict__ const redo = args.redo();
  const uint32_t* __restrict__ const begin = args.sort().begin;
  const uint32_t* __restrict__ const count = args.sort().count;
  const uint32_t* __restrict__ const perm = args.sort().perm;
  const uint32_t* __restrict__ const sorted = args.sort().sorted;
  const uint32_t heavy_thr = args.sort().heavy_thr;
  __shared__ typename PrefetchTile<F>::Column tile[BW];  // [wave]
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const PrefetchTile<F> pf = {tile[threadIdx.x >> 6], threadIdx.x & 63};
  if (t >= total_buckets) return;
  const uint32_t b = perm[t];  // lanes of a wave own buckets of near-equal load
  const uint32_t cnt = count[b];
  if (cnt > heavy_thr) return;  // k_accum_heavy owns it
  const uint32_t beg = begin[b], end = beg + cnt;
  XYZZ<F> acc;
  uint32_t j = beg;
  // first entry that is not the point at infinity starts the accumulator (plain loads: runs once per bucket)
  for (;; j++) {
    if (j >= end) {
      if constexpr (!INTO) store_vec(buckets + b, XYZZ<F>::infinity());  // (INTO: nothing to add, the bucket keeps its sum)
      return;
    }
    const uint32_t v = sorted[j];
    Affine<F> p = load_vec(bases + (v & 0x7fffffffu));
    if (affine_is_zero_words(p)) continue;
    if constexpr (INTO) {
      acc = load_vec(buckets + b);  // entry j itself is added by the chain
      break;
    }
    if (v >> 31) p.y = p.y.neg();
    acc.x = p.x;
    acc.y = p.y;  // (zz = zzz = 1 are the chain's to set, where the entry behind this one does not make them)
    j++;
    break;
  }
  if (accum_chain<F, !INTO, 1>(acc, bases, sorted, j, end - j, pf)) {
    // doubling or cancellation met: k_accum_redo recomputes the bucket (INTO: from the value it still holds -- nothing has
    // been written)
    redo[1 + atomicAdd(redo, 1u)] = b;
    return;
  }
  store_vec(buckets + b, acc);
}
template <class F, int W, int BW, bool MULTI = false, bool INTO = false>
__global__ void __launch_bounds__(64 * BW, W)
k_accum_g1_nc(const AccumArgs<F, MULTI> args, uint32_t total_buckets) {
  accum_g1_nc_body<F, BW, MULTI, INTO>(args, total_buckets);
}
// acc += o for acc, o != O; false when the sum needs the complete group law (o = +-acc): same contract as madd_generic
template <class F>
__host__ __device__ __forceinline__ bool add_generic(XYZZ<F>& a, const XYZZ<F>& o) {
  F u1 = a.x * o.zz;
  F u2 = o.x * a.zz;
  F s1 = a.y * o.zzz;
  F s2 = o.y * a.zzz;
  F pp_ = f_sub_lazy(u2, u1);
  F r = f_sub_lazy(s2, s1);
  F pp = pp_.sqr();
  F rr = r.sqr();
  if (pp.is_zero()) return false;
  F ppp = pp_ * pp;
  F q = u1 * pp;
  F x3 = f_x3(rr, ppp, q);
  a.y = f_mul_sub_mul(r, f_sub_lazy(q, x3), s1, ppp);
  a.x = x3;
  a.zz = a.zz * o.zz * pp;
  a.zzz = a.zzz * o.zzz * ppp;
  return true;
}
// The tail of a two-halves-per-bucket kernel (k_accum_g2_split2; written over the layout): half `sub` of a bucket has the partial sum acc (has: it met a finite entry;
// bad: it met P + P or P - P).  The halves hold the same component L::LANES lanes apart; half 0 adds the two sums and stores
// the bucket, or appends it to the redo list where either half or this addition needs the complete group law.
template <class L>
__device__ __forceinline__ void accum_split2_tail(typename L::P& acc, bool has, bool bad, uint32_t sub, uint32_t comp,
                                                  typename L::Stored* buckets, uint32_t* redo, uint32_t b) {
  const uint32_t flags = (has ? 1u : 0u) | (bad ? 2u : 0u);
  const uint32_t pflags = (uint32_t)__shfl_xor((int)flags, L::LANES);
  typename L::P o;
  o.x = L::shfl_xor(acc.x, L::LANES);
  o.y = L::shfl_xor(acc.y, L::LANES);
  o.zz = L::shfl_xor(acc.zz, L::LANES);
  o.zzz = L::shfl_xor(acc.zzz, L::LANES);
  if (sub != 0) return;
  bool redo_it = ((flags | pflags) & 2u) != 0;
  if (!redo_it) {
    if (has && (pflags & 1u)) redo_it = !add_generic(acc, o);  // uniform over the lanes of the point
    else if (!has) acc = (pflags & 1u) ? o : L::P::infinity();
  }
  if (redo_it) {
    if (comp == 0) redo[1 + atomicAdd(redo, 1u)] = b;  // k_accum_redo recomputes the bucket with the complete addition
  } else {
    L::store(buckets + b, acc, comp);
  }
}
// Two adjacent lanes per bucket (even lane: entries beg, beg + 2, ...; odd lane: beg + 1, beg + 3, ...), the even lane adds
// the two partial sums at the end.  For ONE small proof: its accumulation launch is 0.3 ms of chip time but lasts as long as
// the fullest bucket's chain of dependent additions (25-35 of them, 0.65 ms); two lanes halve the chain (section 4.11).
// Always the multi form (table / bucket array / redo list / sort per blockIdx.y); a doubling in either half or in the
// final addition sends the bucket to the redo list like the one-lane kernel does.  (No pair step: every addition is generic.)
// Spelt out, not a call site of accum_chain and accum_split2_tail: with either of them shared the BN254 instantiation needs
// 149 - 167 registers instead of 148 (profiles/r13/accum_chain_refactor.txt), in every form tried.
template <class F, int BW>
__global__ void __launch_bounds__(64 * BW, 2)
k_accum_g1_split2(const AccumArgs<F, true> args, uint32_t total_buckets) {
  const Affine<F>* __restrict__ const bases = args.bases();
  XYZZ<F>* __restrict__ const buckets = args.buckets();
  uint32_t* __restrict__ const redo = args.redo();
  const uint32_t* __restrict__ const begin = args.sort().begin;
  const uint32_t* __restrict__ const count = args.sort().count;
  const uint32_t* __restrict__ const perm = args.sort().perm;
  const uint32_t* __restrict__ const sorted = args.sort().sorted;
  const uint32_t heavy_thr = args.sort().heavy_thr;
  constexpr int CHUNKS = sizeof(Affine<F>) / 16;
  __shared__ uint4 tile[BW][CHUNKS][64];  // [wave][chunk][lane]
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = gt >> 1, sub = gt & 1u;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (t >= total_buckets) return;  // pair-uniform from here on
  const uint32_t b = perm[t];
  const uint32_t cnt = count[b];
  if (cnt > heavy_thr) return;  // k_accum_heavy owns it
  const uint32_t beg = begin[b], end = beg + cnt;
  auto fetch = [&](uint32_t v) {
    const char* src = reinterpret_cast<const char*>(bases + (v & 0x7fffffffu));
#pragma unroll
    for (int q = 0; q < CHUNKS; q++)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + 16 * q), (lds_ptr_t)&tile[wave][q][0], 16, 0, 0);
  };
  auto take = [&](Affine<F>& p) {
    uint4* d = reinterpret_cast<uint4*>(&p);
#pragma unroll
    for (int q = 0; q < CHUNKS; q++) d[q] = tile[wave][q][lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  XYZZ<F> acc = XYZZ<F>::infinity();
  bool has = false, bad = false;
  uint32_t j = beg + sub;
  for (; j < end; j += 2) {  // first entry of this lane that is not the point at infinity starts its accumulator
    const uint32_t v = sorted[j];
    Affine<F> p = load_vec(bases + (v & 0x7fffffffu));
    if (affine_is_zero_words(p)) continue;
    if (v >> 31) p.y = p.y.neg();
    acc.x = p.x;
    acc.y = p.y;
    acc.zz = F::one();
    acc.zzz = F::one();
    has = true;
    j += 2;
    break;
  }
  uint32_t v_cur = 0, v_next = 0;
  if (j < end) {
    v_cur = sorted[j];
    fetch(v_cur);
    if (j + 2 < end) v_next = sorted[j + 2];
  }
  for (; j < end; j += 2) {
    Affine<F> p;
    take(p);
    const uint32_t v = v_cur;
    if (j + 2 < end) {
      fetch(v_next);
      v_cur = v_next;
      if (j + 4 < end) v_next = sorted[j + 4];
    }
    if (affine_is_zero_words(p)) continue;
    if (!madd_generic(acc, p, 0u - (v >> 31))) {
      bad = true;
      break;
    }
  }
  // the partner's state and partial sum
  const uint32_t flags = (has ? 1u : 0u) | (bad ? 2u : 0u);
  const uint32_t pflags = (uint32_t)__shfl_xor((int)flags, 1);
  XYZZ<F> o;
#pragma unroll
  for (int i = 0; i < F::NL; i++) {
    o.x.l[i] = __shfl_xor(acc.x.l[i], 1);
    o.y.l[i] = __shfl_xor(acc.y.l[i], 1);
    o.zz.l[i] = __shfl_xor(acc.zz.l[i], 1);
    o.zzz.l[i] = __shfl_xor(acc.zzz.l[i], 1);
  }
  if (sub != 0) return;
  bool redo_it = ((flags | pflags) & 2u) != 0;
  if (!redo_it) {
    if (has && (pflags & 1u)) redo_it = !add_generic(acc, o);
    else if (!has) acc = (pflags & 1u) ? o : XYZZ<F>::infinity();
  }
  if (redo_it)
    redo[1 + atomicAdd(redo, 1u)] = b;  // k_accum_redo recomputes the bucket with the complete addition
  else
    store_vec(buckets + b, acc);
}

// G2, lane pair per bucket (see LanePair)
template <int W, int BW>
__global__ void __launch_bounds__(64 * BW, W)
k_accum_g2_nc(const Affine<Fq2_28>* __restrict__ bases, const uint32_t* __restrict__ begin,
              const uint32_t* __restrict__ count, const uint32_t* __restrict__ perm,
              const uint32_t* __restrict__ sorted, XYZZ<Fq2_28>* __restrict__ buckets, uint32_t total_buckets,
              uint32_t heavy_thr, uint32_t* __restrict__ redo) {
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = gt >> 1, comp = gt & 1u;
  if (t >= total_buckets) return;  // pair-uniform
  const uint32_t b = perm[t];
  const uint32_t cnt = count[b];
  if (cnt > heavy_thr) return;
  XYZZ<Fq2P> acc;
  uint32_t j = begin[b];
  const uint32_t end = j + cnt;
  bool bad = false;
  if (accum_first<1>(acc, bases, sorted, j, end, comp)) bad = accum_chain<1, true>(acc, bases, sorted, j, end, comp);
  else acc = XYZZ<Fq2P>::infinity();
  if (bad) {
    if (comp == 0) redo[1 + atomicAdd(redo, 1u)] = b;
  } else {
    LanePair::store(buckets + b, acc, comp);
  }
}

// G2, TWO lane pairs per bucket (pair 0: entries beg, beg + 2, ...; pair 1: beg + 1, beg + 3, ...), pair 0 adds the two partial
// sums at the end: k_accum_g1_split2's idea for the G2 launch of ONE small proof, which is 0.3 ms of chip time but lasts as long
// as the fullest bucket's chain of dependent mixed additions (17 per bucket at 2^14: 0.65 ms, the longest link of a 1.9 ms
// proof).  One wave per SIMD (the general addition on top of the loop's state does not fit 256 registers); only for plans of
// <= 2^16 buckets on an otherwise idle chip.  A doubling in either half or in the final addition sends the bucket to the redo list.
template <int UNUSED = 0>
__global__ void __launch_bounds__(64, 1)
k_accum_g2_split2(const Affine<Fq2_28>* __restrict__ bases, const uint32_t* __restrict__ begin, const uint32_t* __restrict__ count,
                  const uint32_t* __restrict__ perm, const uint32_t* __restrict__ sorted, XYZZ<Fq2_28>* __restrict__ buckets,
                  uint32_t total_buckets, uint32_t heavy_thr, uint32_t* __restrict__ redo) {
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = gt >> 2, sub = (gt >> 1) & 1u, comp = gt & 1u;
  if (t >= total_buckets) return;  // quad-uniform
  const uint32_t b = perm[t];
  const uint32_t cnt = count[b];
  if (cnt > heavy_thr) return;
  XYZZ<Fq2P> acc = XYZZ<Fq2P>::infinity();
  const uint32_t beg = begin[b], end = beg + cnt;
  uint32_t j = beg + sub;  // this pair's entries: every second one
  bool bad = false;
  acc.zz = Fq2P::one();  // (in front of the search: behind it, 2 registers more; the tail does not read the sum of a half without a finite entry)
  acc.zzz = Fq2P::one();
  const bool has = accum_first<2>(acc, bases, sorted, j, end, comp);
  if (has) bad = accum_chain<2, false>(acc, bases, sorted, j, end, comp);
  accum_split2_tail<LanePair>(acc, has, bad, sub, comp, buckets, redo, b);
}

// LDS tree over the npt points a workgroup holds (a power of two; sh: npt x Stored): the sum ends in the lanes of point 0
template <class L>
__device__ __forceinline__ typename L::P lanes_tree_sum(typename L::P acc, typename L::Stored* sh, uint32_t pt, uint32_t npt, uint32_t comp) {
  L::store(sh + pt, acc, comp);
  __syncthreads();
  for (uint32_t s = npt / 2; s > 0; s >>= 1) {
    if (pt < s) {
      acc.add(L::load(sh + pt + s, comp));
      L::store(sh + pt, acc, comp);
    }
    __syncthreads();
  }
  return acc;
}

// the listed buckets again, with the complete addition (rare: repeated bases with equal digits)
// The kernel also CLEARS the list for the slot's next MSM: every workgroup reads the length first, and the last one to
// finish (a ticket word behind the list) resets length and ticket -- no hipMemsetAsync launch in front of an accumulation
// (a kernel of its own that waited up to 0.8 ms for a slot on a full chip).  The buffer is zeroed once when it is allocated.
// Round 5: one WAVE per listed bucket (point l of its 64 / LANES adds entries l, l + 64 / LANES, ...; LDS tree of the partial
// sums) instead of one lane: the synthetic bases of the benchmarks and tests, P_i = G + i Q, meet P + P by arithmetic
// coincidence (a running sum P_a - P_b + P_c IS P_(a - b + c)) about once per 10^7 insertions, and the one lane that then
// walked its bucket's ~32 entries with 16 us per dependent addition held the whole reduction back by 0.2 - 0.5 ms per MSM.
template <class L>
__device__ __forceinline__ void accum_redo_body(const typename L::Base* __restrict__ bases, const uint32_t* __restrict__ begin,
                                                const uint32_t* __restrict__ count, const uint32_t* __restrict__ sorted,
                                                typename L::Stored* __restrict__ buckets, uint32_t* __restrict__ redo,
                                                uint32_t* __restrict__ ticket, uint32_t into) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  typename L::Stored* sh = reinterpret_cast<typename L::Stored*>(lds_raw);
  const uint32_t pt = threadIdx.x / L::LANES, comp = threadIdx.x % L::LANES, npt = blockDim.x / L::LANES;
  const uint32_t n = redo[0];
  for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {  // block-uniform
    const uint32_t b = redo[1 + k];
    const uint32_t beg = begin[b], end = beg + count[b];
    typename L::P acc = L::P::infinity();
    for (uint32_t j = beg + pt; j < end; j += npt) acc.madd(L::load_affine(bases, sorted[j], comp));
    acc = lanes_tree_sum<L>(acc, sh, pt, npt, comp);
    if (pt == 0) {
      // into: the accumulation was adding to an earlier MSM's bucket sums and left the listed buckets untouched
      if (into) acc.add(L::load(buckets + b, comp));
      L::store(buckets + b, acc, comp);
    }
    __syncthreads();
  }
  // every workgroup has read the length by now; the last one to get here clears the list for the slot's next MSM
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
    redo[0] = 0;
    *ticket = 0;
  }
}
template <class F>
__global__ void __launch_bounds__(64)
k_accum_redo(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ begin,
             const uint32_t* __restrict__ count, const uint32_t* __restrict__ sorted,
             XYZZ<F>* __restrict__ buckets, uint32_t* __restrict__ redo, uint32_t* __restrict__ ticket, uint32_t into) {
  accum_redo_body<OneLane<F>>(bases, begin, count, sorted, buckets, redo, ticket, into);
}
template <int UNUSED = 0>
__global__ void __launch_bounds__(64, 2)
k_accum_redo_g2_split(const Affine<Fq2_28>* __restrict__ bases, const uint32_t* __restrict__ begin,
                      const uint32_t* __restrict__ count, const uint32_t* __restrict__ sorted,
                      XYZZ<Fq2_28>* __restrict__ buckets, uint32_t* __restrict__ redo, uint32_t* __restrict__ ticket) {
  accum_redo_body<LanePair>(bases, begin, count, sorted, buckets, redo, ticket, 0u);  // (no accumulate-into form for G2)
}

// Heavy buckets (repeated scalars, booleans: one bucket can hold 20 % of all points):
// MSM_HSPLIT workgroups share one bucket, each reduces a sub-range with an LDS tree into
// heavy_partial[h][r]; the last of them to finish adds the partials.  Buckets beyond the
// partial-slot capacity (pathological inputs) fall back to one workgroup per bucket.
constexpr uint32_t MSM_HSPLIT = 64;
constexpr uint32_t MSM_HEAVY_CAP = 1024;

// ---------------------------------------------------------------------------------------------
// Round 5: the heavy buckets' additions in a kernel that RUNS BESIDE the light accumulation.
// k_accum_heavy (below) adds with the complete group law: 320 registers and scratch, one wave per SIMD (1.6 G additions/s
// against the light kernel's 6.5), and -- two-wave workgroups of that size -- it is not placed while the light kernel
// still has workgroups to issue: the heavy buckets of a witness-like MSM started when the light ones
// had finished.  Now the additions of POINTS into partial sums -- all but a few per cent of the work -- are made by
// one-wave workgroups with the light kernel's own loop (call-free mixed additions, next table entry prefetched through
// LDS: 168 registers, no scratch), every lane on its own stride of a sub-range:
//   k_heavy_plan       one workgroup: list entry h -> (bucket, first entry, points, first wave-item); points per lane
//                      chosen so that the partial sums fit the pool
//   k_accum_heavy_nc   wave-item = 64 x PL consecutive entries of a heavy bucket; lane l adds entries l, l + 64, ... and
//                      stores ONE partial sum (G2: 32 lane pairs); a lane that meets P + P stores a marker instead
//   k_accum_heavy<..>  in PARTIAL mode: sums each bucket's partials with the complete law (LDS trees, ticket for split
//                      buckets: the code that used to add the points); a marked partial is recomputed there, serially,
//                      from its <= PL points.  In POINT mode (plan too long for the pool, partitioned big windows,
//                      A/B accumulate-into forms) it is the kernel of rounds 1-4.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t MSM_HNC_ENT = 1024;        // list entries the plan holds (= k_heavy_plan's block, <= MSM_HEAVY_CAP ticket words)
constexpr uint32_t MSM_HNC_POOL = 131072;     // first-level partial sums per MSM slot
constexpr uint32_t MSM_HNC_MIN_PL = 8;        // points per lane at least (the tree behind costs ~1.4 additions per partial)
constexpr uint32_t MSM_HPLAN_WORDS = 4 + 4 * (MSM_HNC_ENT + 1);
// hplan: [0] wave-items, [1] points per lane PL, [2] entries, [3] mode (0 = partial sums by k_accum_heavy_nc, 1 = point mode),
// then per entry {bucket, first slot in sorted[], points, first wave-item}; entry [entries] = {.., .., .., wave-items}
// ONE WAVE (16 entries per lane): a 1 024-thread workgroup is not placed while accumulation waves hold 504 of a SIMD's 512
// registers (it sat 0.66 - 2.2 ms in front of the heavy kernels in the first traces of this round); a wave fits the slot
// one retiring accumulation wave frees.
template <int UNUSED = 0>
__global__ void __launch_bounds__(64)
k_heavy_plan(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ count, const uint32_t* __restrict__ begin,
             uint32_t* __restrict__ hplan, uint32_t lanes, uint32_t force_point_mode) {
  constexpr uint32_t PER = MSM_HNC_ENT / 64;
  const uint32_t lane = threadIdx.x, n = heavy[0];
  if (force_point_mode || n > MSM_HNC_ENT) {
    if (lane == 0) {
      hplan[0] = 0;
      hplan[1] = 0;
      hplan[2] = 0;
      hplan[3] = 1;
    }
    return;
  }
  // lane owns entries [lane * PER, (lane + 1) * PER)
  uint32_t c[PER], mine = 0;
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    const uint32_t h = lane * PER + k;
    c[k] = h < n ? count[heavy[1 + h]] : 0u;
    mine += c[k];
  }
  auto wave_incl = [&](uint32_t v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)v, off);
      if ((int)lane >= off) v += t;
    }
    return v;
  };
  const uint32_t total = (uint32_t)__shfl((int)wave_incl(mine), 63);  // (entries < 2^32: the sort's slot arithmetic)
  // partial sums = lanes x wave-items <= total / PL + lanes x n
  const uint32_t room = MSM_HNC_POOL - lanes * MSM_HNC_ENT;
  uint32_t pl = (total + room - 1) / room;
  if (pl < MSM_HNC_MIN_PL) pl = MSM_HNC_MIN_PL;
  const uint32_t per_item = lanes * pl;
  uint32_t items[PER], my_items = 0;
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    items[k] = (c[k] + per_item - 1) / per_item;
    my_items += items[k];
  }
  const uint32_t incl = wave_incl(my_items);
  uint32_t run = incl - my_items;
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    const uint32_t h = lane * PER + k;
    if (h < n) {
      const uint32_t b = heavy[1 + h];
      uint32_t* e = hplan + 4 + 4 * h;
      e[0] = b;
      e[1] = begin[b];
      e[2] = c[k];
      e[3] = run;
    }
    run += items[k];
  }
  if (lane == 63) {
    hplan[0] = incl;
    hplan[1] = pl;
    hplan[2] = n;
    hplan[3] = 0;
    hplan[4 + 4 * n + 3] = incl;
  }
}
// the plan entry that owns wave-item `it` (last e with first_item[e] <= it): uniform over the wave
__device__ __forceinline__ uint32_t heavy_plan_entry(const uint32_t* __restrict__ ent, uint32_t n_ent, uint32_t it) {
  uint32_t lo = 0, hi = n_ent;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ent[4 * mid + 3] <= it) lo = mid;
    else hi = mid;
  }
  return lo;
}
// what a lane that met P + P (or P - P) leaves instead of its partial sum: "infinity" with a non-zero zzz word
template <class F>
__device__ __forceinline__ XYZZ<F> heavy_marker() {
  XYZZ<F> m = XYZZ<F>::infinity();
  m.zzz.l[0] = 1;
  return m;
}

template <class F, int W>
__global__ void __launch_bounds__(64, W)
k_accum_heavy_nc(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ hplan,
                 XYZZ<F>* __restrict__ pool) {
  __shared__ typename PrefetchTile<F>::Column tile;
  if (hplan[3] != 0) return;  // point mode: k_accum_heavy takes the list
  const uint32_t n_items = hplan[0], pl = hplan[1], n_ent = hplan[2];
  const uint32_t* __restrict__ const ent = hplan + 4;
  const uint32_t lane = threadIdx.x;
  const PrefetchTile<F> pf = {tile, lane};
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint32_t e = heavy_plan_entry(ent, n_ent, it);
    const uint32_t beg = ent[4 * e + 1], cnt = ent[4 * e + 2], first = ent[4 * e + 3];
    const uint32_t w0 = beg + (it - first) * 64u * pl;
    const uint32_t w1 = (w0 + 64u * pl < beg + cnt) ? w0 + 64u * pl : beg + cnt;
    XYZZ<F> acc;
    uint32_t j = w0 + lane;  // the lane's entries: w0 + lane, + 64, ... below w1
    uint32_t rem = w0 + lane < w1 ? (w1 - w0 - lane + 63) / 64 : 0u;
    if (!accum_first<F, 64>(acc, bases, sorted, j, rem)) {
      store_vec(pool + (size_t)it * 64 + lane, XYZZ<F>::infinity());
      continue;
    }
    // the light kernel's chain; k_accum_heavy recomputes the <= PL points of a lane that met P + P with the complete law
    const bool bad = accum_chain<F, true, 64>(acc, bases, sorted, j, rem, pf);
    XYZZ<F>* const dst = pool + (size_t)it * 64 + lane;
    if (bad) store_vec(dst, heavy_marker<F>());
    else store_vec(dst, acc);
    // (a lane that left the chain early still has a direct-to-LDS load in flight into its own column of the tile: the next
    // item's first fetch into the same column is ordered behind it, and take() waits for both)
  }
}

// G2: 32 lane pairs per wave-item (field28.hpp Fq2P), the light G2 kernel's chain
template <int W>
__global__ void __launch_bounds__(64, W)
k_accum_heavy_nc_g2(const Affine<Fq2_28>* __restrict__ bases, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ hplan,
                    XYZZ<Fq2_28>* __restrict__ pool) {
  if (hplan[3] != 0) return;
  const uint32_t n_items = hplan[0], pl = hplan[1], n_ent = hplan[2];
  const uint32_t* __restrict__ const ent = hplan + 4;
  const uint32_t pair = threadIdx.x >> 1, comp = threadIdx.x & 1u;
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint32_t e = heavy_plan_entry(ent, n_ent, it);
    const uint32_t beg = ent[4 * e + 1], cnt = ent[4 * e + 2], first = ent[4 * e + 3];
    const uint32_t w0 = beg + (it - first) * 32u * pl;
    const uint32_t w1 = (w0 + 32u * pl < beg + cnt) ? w0 + 32u * pl : beg + cnt;
    XYZZ<Fq2_28>* const dst = pool + (size_t)it * 32 + pair;
    XYZZ<Fq2P> acc;
    uint32_t j = w0 + pair;  // the pair's entries: w0 + pair, + 32, ... below w1
    bool bad = false;
    const bool have = accum_first<32>(acc, bases, sorted, j, w1, comp);
    if (have) bad = accum_chain<32, true>(acc, bases, sorted, j, w1, comp);
    if (!have || bad) LanePair::store_marker(dst, bad, comp);
    else LanePair::store(dst, acc, comp);
  }
}

// grid = (MSM_HSPLIT, groups).  The sub-ranges of a split bucket are added up by whichever of its workgroups finishes
// last (ticket word per heavy bucket, left at zero for the slot's next MSM): there is no separate combine launch -- a
// kernel of 330-register waves (G2) that found no SIMD until the accumulation beside it had drained, with the reduction
// waiting behind it (0.23 ms of one 2^14 proof's critical path for a list in which no bucket was split at all).
//
// Round 5: a bucket is cut into as many sub-ranges as it can feed (~4 points per thread), up to MSM_HSPLIT_MAX -- no longer
// at most 64.  A witness of bits puts 630 000 points into ONE bucket per query; 64 sub-ranges x 64 lane pairs left every
// lane pair of the G2 kernel a chain of 154 dependent additions on an otherwise empty chip: 5.3 ms of a 9.5 ms proof
// (profiles/r05/experiments/heavy_bucket_before.txt).  The partial sums live in one pool per MSM slot (MSM_HEAVY_CAP x
// MSM_HSPLIT entries as before), handed out in list order: entry h owns [item0, item0 + nsplit) where item0 = the
// sub-ranges of the entries before it -- the number every workgroup already computes to deal the work items.
constexpr uint32_t MSM_HSPLIT_MAX = 1024;
constexpr uint32_t MSM_HPOOL = MSM_HEAVY_CAP * MSM_HSPLIT;  // partial-sum slots per MSM slot
// sub-ranges of list entry h (count points, pts points per workgroup pass), given the pool slots already handed out
__device__ __forceinline__ uint32_t heavy_nsplit(uint32_t h, uint32_t count, uint32_t pts, uint32_t item0) {
  if (h >= MSM_HEAVY_CAP) return 1u;  // beyond the ticket words: one workgroup per bucket
  uint32_t n = (count + pts - 1) / pts;
  n = n < 1 ? 1 : (n > MSM_HSPLIT_MAX ? MSM_HSPLIT_MAX : n);
  if (item0 + n > MSM_HPOOL) n = 1;  // pool exhausted (thousands of split buckets: pathological): unsplit
  return n;
}
// The ticket of a split bucket: every lane of point 0 stores its part of the partial and fences, a barrier, then thread 0
// takes the ticket -- a sequence that holds for any LANES ("thread 0 stores, fences and takes it" would for one lane only).
template <class L>
__device__ __forceinline__ void accum_heavy_body(const typename L::Base* __restrict__ bases, const uint32_t* __restrict__ begin,
                                                 const uint32_t* __restrict__ count, const uint32_t* __restrict__ heavy,
                                                 const uint32_t* __restrict__ sorted, typename L::Stored* __restrict__ buckets,
                                                 typename L::Stored* __restrict__ heavy_partial, uint32_t* __restrict__ ticket,
                                                 uint32_t into, uint32_t h_first, uint32_t h_limit, const uint32_t* __restrict__ hplan,
                                                 const typename L::Stored* __restrict__ pool_nc) {
  typedef typename L::P P;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  typename L::Stored* sh = reinterpret_cast<typename L::Stored*>(lds_raw);
  __shared__ uint32_t is_last;
  const uint32_t pt = threadIdx.x / L::LANES, comp = threadIdx.x % L::LANES, npt = blockDim.x / L::LANES;
  // PARTIAL mode (hplan given and its mode word 0): the "points" of list entry h are the partial sums k_accum_heavy_nc[_g2]
  // left in pool_nc -- one per point of a wave, in wave-item order -- and the list is the plan's; POINT mode: the kernel of
  // rounds 1-4
  constexpr uint32_t PER_ITEM = 64 / L::LANES;
  const bool pmode = hplan != nullptr && hplan[3] == 0;
  const uint32_t* __restrict__ const ent = hplan + 4;
  const uint32_t pl_nc = pmode ? hplan[1] : 0u;
  // a partial sum, or -- where its lane (pair) met P + P -- that lane's points again with the complete law
  auto partial_at = [&](uint32_t h, uint32_t j) {
    P v = L::load(pool_nc + j, comp);
    bool empty;
    if (L::is_marker(v, comp, &empty)) {
      const uint32_t it = j / PER_ITEM, ln = j % PER_ITEM;
      const uint32_t beg = ent[4 * h + 1], cnt = ent[4 * h + 2], first = ent[4 * h + 3];
      const uint32_t w0 = beg + (it - first) * PER_ITEM * pl_nc;
      const uint32_t w1 = (w0 + PER_ITEM * pl_nc < beg + cnt) ? w0 + PER_ITEM * pl_nc : beg + cnt;
      v = P::infinity();
      for (uint32_t jj = w0 + ln; jj < w1; jj += PER_ITEM) v.madd(L::load_affine(bases, sorted[jj], comp));
    } else if (empty) {
      v = P::infinity();  // (what add() takes it for anyway; without it k_accum_heavy<Fq28> allocates 315 registers, not 308)
    }
    return v;
  };
  // list entries [h_first, min(length, h_limit)): one launch takes the whole list, or -- plans whose partial top window
  // puts thousands of buckets above the threshold (windowed c = 20: 2^14 buckets of 4 500 points at 2^26 terms) -- the
  // first MSM_HEAVY_CAP entries go to a (MSM_HSPLIT, 8) grid and the rest to a second launch with one workgroup per
  // list entry (a (MSM_HSPLIT, 8) grid would walk them with 8 workgroups)
  const uint32_t n_heavy = pmode ? hplan[2] : (heavy[0] < h_limit ? heavy[0] : h_limit);
  // Work items = (bucket, sub-range) pairs, numbered through the list and dealt round-robin to ALL workgroups of the grid.
  // (Rounds 1-3 gave grid row y the buckets y, y + 8, ... and column x the sub-range x: the 64 buckets of a group of small
  // proofs -- one per proof, ~600 points = 2 sub-ranges each -- were walked 8 at a time by 2 of the 64 columns: 5.8 ms per
  // launch at 2^14, a quarter of the group's kernel time; dealt flat the same list is one round of 128 workgroups.)
  const uint32_t n_wg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  uint32_t item0 = 0;  // number of the bucket's first work item = its first pool slot
  // (a launch for the entries beyond the split capacity -- one item per bucket -- strides the list directly)
  const bool tail = h_first >= MSM_HEAVY_CAP;
  for (uint32_t h = tail ? h_first + wg : h_first; h < n_heavy; h += tail ? n_wg : 1u) {
    const uint32_t b = pmode ? ent[4 * h] : heavy[1 + h];
    // (partial mode: positions in pool_nc -- PER_ITEM partial sums per wave-item of the entry)
    const uint32_t cnt = pmode ? (ent[4 * (h + 1) + 3] - ent[4 * h + 3]) * PER_ITEM : count[b];
    const uint32_t beg0 = pmode ? ent[4 * h + 3] * PER_ITEM : begin[b];
    // as many sub-ranges as the bucket can feed: ~4 points per thread (lane pair) of the MSM_TREE_T before the tree (a
    // bucket of 400 points on all 64 x 128 threads is 64 trees of points at infinity: measured 10 % of all instructions of
    // a 2^14 group).
    // (8 points per thread -- one workgroup, no partials and no second tree for the 600 bit variables of a small
    // proof -- measured no better: 2^14 2 501 against 2 554-2 573 proofs/s.)
    const uint32_t nsplit = tail ? 1u : heavy_nsplit(h, cnt, 4 * MSM_TREE_T / L::LANES, item0);
    const uint32_t base = item0;
    // this workgroup's sub-ranges of the bucket: item numbers base + r = wg (mod n_wg)
    const uint32_t r0 = tail ? 0u : (wg + n_wg - base % n_wg) % n_wg;
    item0 += nsplit;
    for (uint32_t r = r0; r < nsplit; r += n_wg) {  // block-uniform
      uint32_t beg = beg0, end = beg0 + cnt;
      if (nsplit > 1) {
        const uint32_t len = (cnt + nsplit - 1) / nsplit;
        const uint32_t sb = beg + r * len;
        end = (sb + len < end) ? sb + len : end;
        beg = sb < end ? sb : end;
      }
      P acc = P::infinity();
      if (pmode) {
        for (uint32_t j = beg + pt; j < end; j += npt) acc.add(partial_at(h, j));
      } else {
        for (uint32_t j = beg + pt; j < end; j += npt) acc.madd(L::load_affine(bases, sorted[j], comp));
      }
      acc = lanes_tree_sum<L>(acc, sh, pt, npt, comp);
      if (nsplit == 1) {
        if (pt == 0) {
          // into: the bucket's sum is added to what an earlier MSM left in the bucket (complete addition, the lanes of point 0)
          // (spelt out here and below: behind a lambda the same two lines cost 944 B of scratch per lane in the lane-pair kernel)
          if (into) acc.add(L::load(buckets + b, comp));
          L::store(buckets + b, acc, comp);
        }
      } else {
        if (pt == 0) {
          L::store(heavy_partial + (size_t)base + r, acc, comp);
          __threadfence();  // each lane's part of the partial is visible device-wide ...
        }
        __syncthreads();  // ... before the ticket is taken
        if (threadIdx.x == 0) is_last = atomicAdd(ticket + h, 1u) == nsplit - 1 ? 1u : 0u;
        __syncthreads();
        if (is_last) {  // block-uniform
          __threadfence();
          P v = P::infinity();
          for (uint32_t k = pt; k < nsplit; k += npt) v.add(L::load(heavy_partial + (size_t)base + k, comp));
          v = lanes_tree_sum<L>(v, sh, pt, npt, comp);
          if (pt == 0) {
            if (into) v.add(L::load(buckets + b, comp));
            L::store(buckets + b, v, comp);
          }
          if (threadIdx.x == 0) ticket[h] = 0;
        }
      }
      __syncthreads();
    }
  }
}
template <class F>
__global__ void __launch_bounds__(MSM_TREE_T)
k_accum_heavy(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ begin,
              const uint32_t* __restrict__ count, const uint32_t* __restrict__ heavy,
              const uint32_t* __restrict__ sorted, XYZZ<F>* __restrict__ buckets,
              XYZZ<F>* __restrict__ heavy_partial, uint32_t* __restrict__ ticket, uint32_t into, uint32_t h_first,
              uint32_t h_limit, const uint32_t* __restrict__ hplan, const XYZZ<F>* __restrict__ pool_nc) {
  accum_heavy_body<OneLane<F>>(bases, begin, count, heavy, sorted, buckets, heavy_partial, ticket, into, h_first, h_limit, hplan, pool_nc);
}
template <int UNUSED = 0>
__global__ void __launch_bounds__(MSM_TREE_T, 2)
k_accum_heavy_g2_split(const Affine<Fq2_28>* __restrict__ bases, const uint32_t* __restrict__ begin,
                       const uint32_t* __restrict__ count, const uint32_t* __restrict__ heavy,
                       const uint32_t* __restrict__ sorted, XYZZ<Fq2_28>* __restrict__ buckets,
                       XYZZ<Fq2_28>* __restrict__ heavy_partial, uint32_t* __restrict__ ticket, uint32_t h_first,
                       uint32_t h_limit, const uint32_t* __restrict__ hplan, const XYZZ<Fq2_28>* __restrict__ pool_nc) {
  accum_heavy_body<LanePair>(bases, begin, count, heavy, sorted, buckets, heavy_partial, ticket, 0u, h_first, h_limit, hplan, pool_nc);
}

// point t handles buckets [t*SEG, (t+1)*SEG) of one window (global segment id)
// buckets2 (optional): the bucket array of a SECOND MSM over the same bucket set whose result is only ever added to this
// one's (the prover's L and H queries: C = ... + L + H).  Its buckets join the running sum here -- three additions per bucket
// for the pair instead of two each, and one tree sum / host combine instead of two -- and nothing else of the two MSMs
// knows about the other: both accumulate into their own arrays with the ordinary kernels.
template <class L>
__device__ __forceinline__ void segreduce_body(const typename L::Stored* __restrict__ buckets, typename L::Stored* __restrict__ segsum,
                                               typename L::Stored* __restrict__ segw, uint32_t total_segs, int seg,
                                               const typename L::Stored* __restrict__ buckets2,
                                               const typename L::Stored* __restrict__ buckets3) {
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = gt / L::LANES, comp = gt % L::LANES;
  if (t >= total_segs) return;
  typename L::P run = L::P::infinity();
  typename L::P acc = L::P::infinity();
  for (int i = seg - 1; i >= 0; i--) {
    typename L::P bk = L::load(buckets + (size_t)t * seg + i, comp);
    run.add(bk);
    if (buckets2) {
      bk = L::load(buckets2 + (size_t)t * seg + i, comp);
      run.add(bk);
    }
    if (buckets3) {
      bk = L::load(buckets3 + (size_t)t * seg + i, comp);
      run.add(bk);
    }
    acc.add(run);
  }
  L::store(segsum + t, run, comp);
  L::store(segw + t, acc, comp);
}
template <class F>
__global__ void __launch_bounds__(256)
k_segreduce(const XYZZ<F>* __restrict__ buckets, XYZZ<F>* __restrict__ segsum, XYZZ<F>* __restrict__ segw,
            uint32_t total_segs, int seg, const XYZZ<F>* __restrict__ buckets2, const XYZZ<F>* __restrict__ buckets3) {
  segreduce_body<OneLane<F>>(buckets, segsum, segw, total_segs, seg, buckets2, buckets3);
}
// The same at two waves per SIMD (256 registers, 656 B of scratch instead of 464): for the reductions that have the chip to
// themselves and enough waves to use the room -- the 13 x 2^19 buckets of the big windowed plans, 5.66 -> 4.98 ms at 2^26 terms.
// (The prover's and the small plans' reductions keep the form above: they run beside accumulations or are latency chains.)
template <class F>
__global__ void __launch_bounds__(256, 2)
k_segreduce_w2(const XYZZ<F>* __restrict__ buckets, XYZZ<F>* __restrict__ segsum, XYZZ<F>* __restrict__ segw,
            uint32_t total_segs, int seg, const XYZZ<F>* __restrict__ buckets2, const XYZZ<F>* __restrict__ buckets3) {
  segreduce_body<OneLane<F>>(buckets, segsum, segw, total_segs, seg, buckets2, buckets3);
}
template <int UNUSED = 0>
__global__ void __launch_bounds__(256, 2)
k_segreduce_g2_split(const XYZZ<Fq2_28>* __restrict__ buckets, XYZZ<Fq2_28>* __restrict__ segsum,
                     XYZZ<Fq2_28>* __restrict__ segw, uint32_t total_segs, int seg) {
  segreduce_body<LanePair>(buckets, segsum, segw, total_segs, seg, nullptr, nullptr);
}

// Second running-sum level.  The tree sums below weight segment t of a window by t through bit decomposition: every
// segsum entry is added ~ log2(segments) / 2 times.  With t = 16 u + k,
//   sum_t t segsum_t = 16 sum_u u segsum2_u + sum_u segt2_u,   segsum2_u = sum_k segsum_(16u+k),  segt2_u = sum_k k segsum_(16u+k),
// so a point per super-segment u forms both by the running sums of k_segreduce (31 additions per 16 segments) and the bit
// jobs walk the 16 x shorter list segsum2; segt2 is one more plain job.  (The plain sum of segw stays what it was: every
// entry is added once either way.)  The segment lists of the windows lie back to back and are multiples of 16 long, so
// super-segment u of the array is super-segment u mod (segments / 16) of its window.
template <class L>
__device__ __forceinline__ void segreduce2_body(const typename L::Stored* __restrict__ segsum, typename L::Stored* __restrict__ segsum2,
                                                typename L::Stored* __restrict__ segt2, uint32_t total_segs2) {
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t u = gt / L::LANES, comp = gt % L::LANES;
  if (u >= total_segs2) return;
  typename L::P run = L::P::infinity();
  typename L::P acc = L::P::infinity();
  for (int k = (1 << MSM_SEG2_LOG) - 1; k >= 0; k--) {
    typename L::P v = L::load(segsum + ((size_t)u << MSM_SEG2_LOG) + k, comp);
    run.add(v);
    if (k) acc.add(run);  // weight k, not k + 1: segment 0 of a super-segment counts in the plain sum only
  }
  L::store(segsum2 + u, run, comp);
  L::store(segt2 + u, acc, comp);
}
template <class F>
__global__ void __launch_bounds__(256)
k_segreduce2(const XYZZ<F>* __restrict__ segsum, XYZZ<F>* __restrict__ segsum2, XYZZ<F>* __restrict__ segt2, uint32_t total_segs2) {
  segreduce2_body<OneLane<F>>(segsum, segsum2, segt2, total_segs2);
}
template <int UNUSED = 0>
__global__ void __launch_bounds__(256, 2)
k_segreduce2_g2_split(const XYZZ<Fq2_28>* __restrict__ segsum, XYZZ<Fq2_28>* __restrict__ segsum2, XYZZ<Fq2_28>* __restrict__ segt2,
                      uint32_t total_segs2) {
  segreduce2_body<LanePair>(segsum, segsum2, segt2, total_segs2);
}

// What the tree-sum kernels read when a second level ran (t_job < 0: none): the bit jobs and the plain job walk segsum2
// (segs2 entries per window), job t_job is the plain sum of segt2, job 0 stays the plain sum of segw (segs_per_win entries).
template <class P>
struct TreeLevel2 {
  const P* segsum2;
  const P* segt2;
  uint32_t segs2;
  int t_job;
};
// the list of (window w, job): first entry, length (whole lists; a bit job enumerates half of that), whole or bit job
template <class P>
__device__ __forceinline__ const P* tree_job_list(int job, int w, const P* segsum, const P* segw, uint32_t segs_per_win, int plain_job,
                                                  const TreeLevel2<P>& l2, uint32_t* len, bool* whole) {
  *whole = job == 0 || job == plain_job || job == l2.t_job;
  if (job == 0) {
    *len = segs_per_win;
    return segw + (size_t)w * segs_per_win;
  }
  if (l2.t_job < 0) {
    *len = *whole ? segs_per_win : segs_per_win / 2;
    return segsum + (size_t)w * segs_per_win;
  }
  *len = *whole ? l2.segs2 : l2.segs2 / 2;
  return (job == l2.t_job ? l2.segt2 : l2.segsum2) + (size_t)w * l2.segs2;
}

// grid = (njobs, nwin, nchunk).  job 0: sum_t segw[w][t]; job j>=1: sum_{t: bit (j-1)} segsum[w][t];
// job plain_job (shared-bucket mode only): sum_t segsum[w][t].  With a second level (l2): see TreeLevel2.
// nchunk = 1: the workgroup sums the job's whole list and writes the result in the host representation.
// nchunk > 1 (small plans, where the reduction is a latency chain and the chip is empty): workgroup z sums the z-th
// slice of the list into stage[(w * njobs + job) * nchunk + z]; k_treesum_final adds the slices.  A list of 2^13 segments
// then costs 2 + 7 + 5 dependent additions instead of 64 + 7.
// One loop over the list for whole jobs and bit jobs, with a select on `whole`: k_treesum<Fq28> is 24 471 instructions
// with it, 33 592 with a loop per kind of job.
template <class L>
__device__ __forceinline__ void treesum_body(const typename L::Stored* __restrict__ segsum, const typename L::Stored* __restrict__ segw,
                                             uint32_t segs_per_win, typename L::Host* __restrict__ partial, int plain_job,
                                             typename L::Stored* __restrict__ stage, typename L::Host* __restrict__ partial_host,
                                             const TreeLevel2<typename L::Stored>& l2) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  typename L::Stored* sh = reinterpret_cast<typename L::Stored*>(lds_raw);
  const int job = blockIdx.x;
  const int w = blockIdx.y;
  const uint32_t nchunk = gridDim.z, z = blockIdx.z;
  const uint32_t pt = threadIdx.x / L::LANES, comp = threadIdx.x % L::LANES, npt = blockDim.x / L::LANES;
  uint32_t len;
  bool whole;
  const typename L::Stored* src = tree_job_list(job, w, segsum, segw, segs_per_win, plain_job, l2, &len, &whole);
  const uint32_t per = (len + nchunk - 1) / nchunk;
  // (a list shorter than the slices of job 0 leaves the last slices empty: lo >= hi)
  const uint32_t lo = z * per, hi = lo + per < len ? lo + per : len;
  // bit job: enumerate only the segments whose bit (job - 1) is set, so that no lane idles through an addition
  const uint32_t b = whole ? 0u : (uint32_t)(job - 1), lowmask = (1u << b) - 1u;
  typename L::P acc = L::P::infinity();
  for (uint32_t u = lo + pt; u < hi; u += npt) {
    const uint32_t t = whole ? u : (((u & ~lowmask) << 1) | (1u << b) | (u & lowmask));
    typename L::P v = L::load(src + t, comp);
    acc.add(v);
  }
  acc = lanes_tree_sum<L>(acc, sh, pt, npt, comp);
  if (pt == 0) {
    if (nchunk == 1) {
      // device copy (the RCCL exchange gathers it) and, directly, the pinned host slot the combining thread reads: no
      // device-to-host copy behind the reduction (it ran as a blit kernel, 0.3 ms of waiting for SIMDs per MSM)
      L::store_host(partial + (size_t)w * gridDim.x + job, acc, comp);
      L::store_host(partial_host + (size_t)w * gridDim.x + job, acc, comp);
    } else {
      L::store(stage + ((size_t)w * gridDim.x + job) * nchunk + z, acc, comp);
    }
  }
}
// grid = (njobs, nwin), nchunk <= points per workgroup (a power of two) <= MSM_TREE_T: adds the slices of one (window, job)
template <class L>
__device__ __forceinline__ void treesum_final_body(const typename L::Stored* __restrict__ stage, uint32_t nchunk,
                                                   typename L::Host* __restrict__ partial, typename L::Host* __restrict__ partial_host) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  typename L::Stored* sh = reinterpret_cast<typename L::Stored*>(lds_raw);
  const size_t idx = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const uint32_t pt = threadIdx.x / L::LANES, comp = threadIdx.x % L::LANES, npt = blockDim.x / L::LANES;
  typename L::P acc = L::P::infinity();
  if (pt < nchunk) acc = L::load(stage + idx * nchunk + pt, comp);
  acc = lanes_tree_sum<L>(acc, sh, pt, npt, comp);
  if (pt == 0) {
    L::store_host(partial + idx, acc, comp);
    L::store_host(partial_host + idx, acc, comp);
  }
}
template <class F>
__global__ void __launch_bounds__(MSM_TREE_T)
k_treesum(const XYZZ<F>* __restrict__ segsum, const XYZZ<F>* __restrict__ segw, uint32_t segs_per_win,
          XYZZ<typename HostFieldOf<F>::type>* __restrict__ partial, int plain_job, XYZZ<F>* __restrict__ stage,
          XYZZ<typename HostFieldOf<F>::type>* __restrict__ partial_host, TreeLevel2<XYZZ<F>> l2) {
  treesum_body<OneLane<F>>(segsum, segw, segs_per_win, partial, plain_job, stage, partial_host, l2);
}
template <class F>
__global__ void __launch_bounds__(MSM_TREE_T)
k_treesum_final(const XYZZ<F>* __restrict__ stage, uint32_t nchunk, XYZZ<typename HostFieldOf<F>::type>* __restrict__ partial,
                XYZZ<typename HostFieldOf<F>::type>* __restrict__ partial_host) {
  treesum_final_body<OneLane<F>>(stage, nchunk, partial, partial_host);
}
// The lane-pair tree sums for G2: a pair owns one list element, so the unsplit form's 330-register additions (one wave per
// SIMD, 45-60 us each in a latency chain) become G1-sized ones.  For the sliced (small-plan) case, where the tree sums ARE
// the latency of a proof, and for the big plans; blockDim.x / 2 pairs per workgroup.
template <int UNUSED = 0>
__global__ void __launch_bounds__(2 * MSM_TREE_T, 2)
k_treesum_g2_split(const XYZZ<Fq2_28>* __restrict__ segsum, const XYZZ<Fq2_28>* __restrict__ segw, uint32_t segs_per_win,
                   XYZZ<Fq2>* __restrict__ partial, int plain_job, XYZZ<Fq2_28>* __restrict__ stage, XYZZ<Fq2>* __restrict__ partial_host,
                   TreeLevel2<XYZZ<Fq2_28>> l2) {
  treesum_body<LanePair>(segsum, segw, segs_per_win, partial, plain_job, stage, partial_host, l2);
}
template <int UNUSED = 0>
__global__ void __launch_bounds__(2 * MSM_TREE_T, 2)
k_treesum_final_g2_split(const XYZZ<Fq2_28>* __restrict__ stage, uint32_t nchunk, XYZZ<Fq2>* __restrict__ partial,
                         XYZZ<Fq2>* __restrict__ partial_host) {
  treesum_final_body<LanePair>(stage, nchunk, partial, partial_host);
}

}  // namespace zkmi
#include "msm_quad.hpp"
namespace zkmi {

template <class F>
__global__ void __launch_bounds__(256)
k_bases_convert(const Affine<typename HostFieldOf<F>::type>* __restrict__ in, Affine<F>* __restrict__ out,
                uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<typename HostFieldOf<F>::type> p = load_vec(in + i);
  Affine<F> q = {fq28_from_fq(p.x), fq28_from_fq(p.y)};  // (0,0) stays exactly (0,0)
  store_vec(out + i, q);
}

// ---------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------
template <class F>
void MsmEngine<F>::release() {
  if (buckets) (void)hipFree(buckets);
  if (segsum) (void)hipFree(segsum);
  if (segw) (void)hipFree(segw);
  if (seg2) (void)hipFree(seg2);
  seg2 = nullptr;
  if (partial) (void)hipFree(partial);
  if (tree_stage) (void)hipFree(tree_stage);
  tree_stage = nullptr;
  if (heavy_partial) (void)hipFree(heavy_partial);
  heavy_partial = nullptr;
  if (heavy_plan) (void)hipFree(heavy_plan);
  heavy_plan = nullptr;
  if (heavy_ticket) (void)hipFree(heavy_ticket);
  heavy_ticket = nullptr;
  if (redo) (void)hipFree(redo);
  redo = nullptr;
  if (h_partial) (void)hipHostFree(h_partial);
  // the events outlive a re-allocation: MsmSort::readers may still hold some of them (destroy_events() runs
  // from the destructor only)
  buckets = segsum = segw = nullptr;
  partial = h_partial = nullptr;
  cap_buckets = 0;
}

uint64_t msm_max_buckets(uint64_t n);

template <class F>
hipError_t MsmEngine<F>::reset_transients() {
  if (!redo || !heavy_ticket) return hipSuccess;
  hipError_t e = hipMemset(redo, 0, sizeof(uint32_t) * (cap_buckets + 2) * nslots);
  if (e != hipSuccess) return e;
  return hipMemset(heavy_ticket, 0, sizeof(uint32_t) * MSM_HEAVY_CAP * nslots);
}

template <class F>
void MsmEngine<F>::destroy_events() {
  for (int i = 0; i < SLOTS; i++) {
    hipEvent_t* evs[] = {&done[i], &acc_done[i], &pre[i], &heavy_done[i], &redo_done[i]};
    for (hipEvent_t* e : evs) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  }
}

template <class F>
hipError_t MsmEngine<F>::ensure_slots(int n) {
  if (n > SLOTS) return hipErrorInvalidValue;
  if (n <= nslots) return hipSuccess;
  const bool sh = has_shared;
  const uint64_t mb = min_buckets;
  release();
  has_shared = sh;
  min_buckets = mb;
  nslots = n;
  return hipSuccess;
}

template <class F>
hipError_t MsmEngine<F>::reserve_buckets(uint64_t buckets) {
  if (buckets <= cap_buckets) return hipSuccess;
  const bool sh = has_shared;
  release();
  has_shared = sh;
  min_buckets = buckets;
  return reserve(1, sh);
}

template <class F>
hipError_t MsmEngine<F>::reserve(uint64_t n, bool shared_too) {
  uint64_t need = msm_max_buckets(n);
  if (need < min_buckets) need = min_buckets;
  const uint64_t forced = (uint64_t)(255 / 16 + 1) * (1u << 15);  // plan_override = 16 for any n
  if (need < forced) need = forced;
  shared_too = shared_too || has_shared;
  if (shared_too) {
    const MsmPlan sp = msm_make_plan_shared(n);  // shared-bucket plan of the same n
    const uint64_t sb = (uint64_t)sp.nwin * sp.nb;
    if (need < sb) need = sb;
  }
  has_shared = shared_too;
  if (need <= cap_buckets) return hipSuccess;
  release();
  hipError_t e;
  if ((e = hipMalloc(&buckets, sizeof(XYZZ<F>) * need * nslots)) != hipSuccess) return e;
  seg_cap = msm_max_segments(need);
  if ((e = hipMalloc(&segsum, sizeof(XYZZ<F>) * seg_cap * nslots)) != hipSuccess) return e;
  if ((e = hipMalloc(&segw, sizeof(XYZZ<F>) * seg_cap * nslots)) != hipSuccess) return e;
  if ((e = hipMalloc(&seg2, sizeof(XYZZ<F>) * 2 * (seg_cap >> MSM_SEG2_LOG) * nslots)) != hipSuccess) return e;
  if ((e = hipMalloc(&partial, sizeof(XYZZ<HF>) * SLOTS * SLOT_PTS)) != hipSuccess) return e;
  if ((e = hipMalloc(&tree_stage, sizeof(XYZZ<F>) * MSM_STAGE_PTS * nslots)) != hipSuccess) return e;
  // per slot: MSM_HPOOL partial sums of split buckets (k_accum_heavy) + MSM_HNC_POOL first-level ones (k_accum_heavy_nc)
  if ((e = hipMalloc(&heavy_partial, sizeof(XYZZ<F>) * ((size_t)MSM_HPOOL + MSM_HNC_POOL) * nslots)) != hipSuccess) return e;
  if ((e = hipMalloc(&heavy_plan, sizeof(uint32_t) * MSM_HPLAN_WORDS * nslots)) != hipSuccess) return e;
  if ((e = hipMalloc(&heavy_ticket, sizeof(uint32_t) * MSM_HEAVY_CAP * nslots)) != hipSuccess) return e;
  if ((e = hipMemset(heavy_ticket, 0, sizeof(uint32_t) * MSM_HEAVY_CAP * nslots)) != hipSuccess) return e;  // every use leaves zeros behind
  if ((e = hipMalloc(&redo, sizeof(uint32_t) * (need + 2) * nslots)) != hipSuccess) return e;  // one list per slot
  if ((e = hipMemset(redo, 0, sizeof(uint32_t) * (need + 2) * nslots)) != hipSuccess) return e;  // lengths and tickets start at zero
  if ((e = hipHostMalloc(&h_partial, sizeof(XYZZ<HF>) * SLOTS * SLOT_PTS, hipHostMallocCoherent)) != hipSuccess) return e;
  for (int i = 0; i < SLOTS; i++) {
    hipEvent_t* evs[] = {&done[i], &acc_done[i], &pre[i], &heavy_done[i], &redo_done[i]};
    for (hipEvent_t* ev : evs)
      if (!*ev && (e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return e;
  }
  cap_buckets = need;
  return hipSuccess;
}

static inline int msm_seg_bits(const MsmPlan& pl) {
  const uint32_t segs_per_win = pl.nb >> pl.seg_log;
  int seg_bits = 0;
  while ((1u << seg_bits) < segs_per_win) seg_bits++;
  return seg_bits;
}
// partial sums a reduction leaves per window: [0] plain sum of segw, [1 ..] the bit jobs, then (shared-bucket plans) the plain
// sum of segsum, last.  With a second level (pl.seg2_log, shared plans only): the bit jobs of segsum2, the plain sum of
// segt2, the plain sum of segsum2.
static inline int msm_njobs(const MsmPlan& pl) {
  if (pl.seg2_log) return 3 + msm_seg_bits(pl) - pl.seg2_log;
  return 1 + msm_seg_bits(pl) + (pl.shared ? 1 : 0);
}

// points a wave of the quad (G1, BN254 G1) / octet (G2) kernels holds
static inline uint32_t msm_quad_per_wave(MsmEngineKind kind) {
  return kind == MSM_ENGINE_G2 ? XYZZQ<Fq28, 0, true>::PER_WAVE : XYZZQ<Fq28, 0, false>::PER_WAVE;
}

// The launch schedule of one run_device_multi call (msm.hpp MsmRunSchedule), from the plan all its MSMs share, the engine,
// MsmEngine::host_spin (ONE MSM or ONE proof by itself: the latency path; false: the batch prover's pipeline), the number
// of MSMs, the MSM_RUN_* flags, and whether an MSM adds INTO another one's bucket array (A/B library).
inline MsmRunSchedule msm_run_schedule(const MsmPlan& pl, MsmEngineKind kind, bool host_spin, int nm, int flags, bool any_into) {
  // Every tuning switch of the engine, read here and nowhere else; the product compiles each to its default (tune.hpp).
  //   ZKMI_ACCUM (msm.hpp) / ZKMI_ACCUM_G2 = 0 | 1: the retired accumulation generations (madd with an out-of-line doubling
  //     path; ZKMI_ACCUM_BLOCK = 64 | 256 threads per workgroup, ZKMI_ACCUM_ROUNDS = R load-ordered bucket groups per wave),
  //     2 | 3: the call-free kernels at 2 / 3 waves per SIMD (the product: 3 for G1, 2 for G2)
  //   ZKMI_QUAD / ZKMI_QUAD_BATCH (G2, the octet form: ZKMI_QUAD_G2 / ZKMI_QUAD_G2_BATCH): the reduction-side kernels with every
  //     complete addition split over a lane quad (msm_quad.hpp): bit 0 = segment sums, 1 = tree sums, 2 = redo pass, 3 = the
  //     summing of heavy-bucket partials, 4 = (A/B) the accumulation itself.  One-wave workgroups at the accumulation
  //     kernels' register count, placed beside them.  The latency path takes all four: a chain of 4 products per dependent
  //     addition instead of 14; the pipeline only redo and heavy: the quad form issues 1.37 x the instructions
  //   ZKMI_HEAVY_ON (msm.hpp), ZKMI_HEAVY_NC = 0: the complete-law heavy kernel of rounds 1-4 for everything, ZKMI_HEAVY_DEFER
  //     = 1: round 6, no gain (g2_split2_ab.txt)
  //   ZKMI_FORCE_MULTI = 1: a lone MSM through the fused launch too (so that the generic entry points, with their degenerate
  //     inputs, reach k_accum_g1_split2 and the MULTI kernel form)
  //   ZKMI_SOLO_SPLIT / ZKMI_SOLO_SPLIT_G2 = 0: one lane (pair) per bucket for small plans too
  //   ZKMI_ACCUM_W2 = 1: every lone G1 accumulation capped at two waves (12 % slower)
  //   ZKMI_G2_TREE_SPLIT = 0: the unsplit G2 tree sum;  ZKMI_GATHER_MASK_BITS: TIMING ONLY, see k_mask_sorted
  MsmRunSchedule s = {};
  const bool g2 = kind == MSM_ENGINE_G2;
  s.exp_accum_mode = g2 ? ZK_TUNE("ZKMI_ACCUM_G2", 2) : msm_tune_accum();
  const int quad_mask = g2 ? (host_spin ? ZK_TUNE("ZKMI_QUAD_G2", 15) : ZK_TUNE("ZKMI_QUAD_G2_BATCH", 12))
                           : (host_spin ? ZK_TUNE("ZKMI_QUAD", 15) : ZK_TUNE("ZKMI_QUAD_BATCH", 12));
  s.exp_accum_block = ZK_TUNE("ZKMI_ACCUM_BLOCK", 64) == 256 ? 256 : 64;
  s.exp_accum_rounds = ZK_TUNE("ZKMI_ACCUM_ROUNDS", 0);
  s.exp_mask_bits = ZK_TUNE("ZKMI_GATHER_MASK_BITS", 0);
  s.exp_two_waves = (flags & MSM_RUN_TWO_WAVES) || ZK_TUNE("ZKMI_ACCUM_W2", 0) == 1;
  s.exp_g2_tree_unsplit = ZK_TUNE("ZKMI_G2_TREE_SPLIT", 1) == 0;
  s.heavy_on = msm_tune_heavy_on();
  const bool t_heavy_nc = ZK_TUNE("ZKMI_HEAVY_NC", 1) != 0, t_heavy_defer = ZK_TUNE("ZKMI_HEAVY_DEFER", 0) != 0;
  const bool t_solo_split = ZK_TUNE("ZKMI_SOLO_SPLIT", 1) != 0, t_solo_split_g2 = ZK_TUNE("ZKMI_SOLO_SPLIT_G2", 1) != 0;
  const bool t_force_multi = ZK_TUNE("ZKMI_FORCE_MULTI", 0) != 0;

  const uint32_t lanes = g2 ? 2 : 1;  // lanes per point of the one-lane / lane-pair kernels
  const uint32_t point_bytes = g2 ? sizeof(XYZZ<Fq2_28>) : kind == MSM_ENGINE_BN254 ? sizeof(XYZZ<BnFq28>) : sizeof(XYZZ<Fq28>);
  s.nocall = s.exp_accum_mode == 2 || s.exp_accum_mode == 3;
  s.tot_b = pl.nwin * pl.nb;
  s.segs_per_win = pl.nb >> pl.seg_log;
  s.tot_segs = pl.nwin * s.segs_per_win;
  s.seg = 1 << pl.seg_log;
  s.seg_bits = msm_seg_bits(pl);
  // the partitioned big windows keep the one-lane segment and tree sums: their reduction has the chip to itself
  s.wide = !pl.shared && pl.c > 16;
  s.quad_seg = (quad_mask & 1) && !s.wide;
  s.quad_tree = (quad_mask & 2) && !s.wide;
  s.quad_redo = (quad_mask & 4) != 0;
  // the quad / octet kernels, the windowed plans and their exchange layouts keep the single level
  s.level2 = pl.shared && !s.quad_seg && !s.quad_tree && s.segs_per_win >= MSM_SEG2_MIN_SEGS;
  s.seg2_log = s.level2 ? MSM_SEG2_LOG : 0;
  s.segs2 = s.segs_per_win >> MSM_SEG2_LOG;
  s.tot_segs2 = s.tot_segs >> MSM_SEG2_LOG;
  MsmPlan reduced = pl;
  reduced.seg2_log = s.seg2_log;
  s.njobs = msm_njobs(reduced);
  s.plain_job = pl.shared ? s.njobs - 1 : -1;
  s.t_job = s.level2 ? s.njobs - 2 : -1;

  // One small G2 MSM by itself (the G2 launch of a single small proof): two lane pairs per bucket halve the chain (2^13 1.99
  // -> 1.74 ms, 2^14 1.92 -> 1.77, 2^15 2.38 -> 2.2; at 2^16 buckets the chip is full and it costs 0.08 ms:
  // profiles/r06/experiments/g2_split2_ab.txt).  G1: a fused launch of small plans (one small proof) takes two lanes per bucket.
  s.fused = !g2 && s.nocall && (nm > 1 || (t_force_multi && !any_into));
  if (g2) s.accum = host_spin && s.tot_b <= (1u << 15) && t_solo_split_g2 ? MSM_ACCUM_G2_SPLIT2 : MSM_ACCUM_G2;
  else if (s.fused) s.accum = t_solo_split && s.tot_b <= (1u << 16) ? MSM_ACCUM_G1_SPLIT2 : MSM_ACCUM_G1_MULTI;
  else s.accum = MSM_ACCUM_G1;
  s.exp_accum_q = (quad_mask & 16) && s.tot_b <= (1u << 16);  // (G2 and the fused G1 launch, in front of split2)

  // the call-free kernels take the additions of points (DESIGN.md 4.1 "heavy buckets"); not for lists the plan cannot hold
  // (decided on the device), the partitioned big windows' thousands of entries, or the A/B accumulate-into forms
  s.heavy_nc = t_heavy_nc && !s.wide && !any_into;
  s.quad_heavy = (quad_mask & 8) && s.heavy_nc;
  s.heavy_deferred = host_spin && s.tot_b <= (1u << 16) && (quad_mask & 8) && s.heavy_on == 2 && t_heavy_defer;

  // One-lane / lane-pair tree sums: a workgroup of MSM_TREE_T threads takes two segments per point.  Job lists longer than
  // that are cut into nchunk slices (k_treesum_final adds them), as many as leave no slice empty, within a cap:
  //   plans of at most 2^16 buckets: all of them, or none where the stage cannot hold them (fewer, longer slices -- at most
  //     16, 8 or 4 -- measured the same group rates and single-proof latencies: profiles/r05/experiments/tree_slices_ab.txt);
  //   one windowed MSM of up to 2^19 buckets: as many as the chip holds at once (1024 workgroups; 16 windows x 13 jobs: 16;
  //     3 328 workgroups of 9 dependent additions each, in three rounds, took longer than 208 of 23; see plan_set_heavy);
  //   partitioned big windows: 2^(c-5) segments per list on ONE workgroup are a chain of 2^(c-12) dependent additions (5 ms
  //     at c = 20); as many as the stage holds (16 at 13 windows x 16 jobs);
  //   every other plan: unsliced.
  const uint32_t per_block = 2 * MSM_TREE_T / lanes;
  const uint64_t lists = (uint64_t)s.njobs * pl.nwin;
  const uint32_t fit = s.segs_per_win / per_block < MSM_TREE_T ? s.segs_per_win / per_block : MSM_TREE_T;
  s.nchunk = 1;
  if (fit > 1 && s.tot_b <= (1u << 16)) {
    if (lists * fit <= MSM_STAGE_PTS_1) s.nchunk = fit;
  } else if (fit > 1 && ((!pl.shared && s.tot_b <= (1u << 19)) || s.wide)) {
    const uint32_t cap = s.tot_b <= (1u << 19) ? 1024 : MSM_STAGE_PTS_1;
    for (s.nchunk = fit; s.nchunk > 1 && lists * s.nchunk > cap;) s.nchunk >>= 1;
  }
  // sliced: MSM_TREE_T / lanes points per workgroup (G2: 64 lane pairs); unsliced: MSM_TREE_T points (G2: 128 pairs -- the
  // unsplit form's 330-register additions made this the slowest link of a proof's tail)
  const uint32_t tree_points = s.nchunk > 1 ? MSM_TREE_T / lanes : MSM_TREE_T;
  s.exp_g2_tree_unsplit = s.exp_g2_tree_unsplit && g2 && s.nchunk == 1;  // (then by the one-lane kernel)
  s.tree_block = tree_points * (s.exp_g2_tree_unsplit ? 1 : lanes);
  s.tree_lds = tree_points * point_bytes;
  // the final sum: a point per slice, at least a wave
  for (s.final_block = 64; s.final_block < lanes * s.nchunk;) s.final_block <<= 1;
  s.final_lds = s.final_block / lanes * point_bytes;
  // Quad / octet tree sums: one wave (16 quads / 8 octets) per slice; as many slices as make the two levels equally deep (a
  // point walks len / (PER_WAVE slices) segments, the final sum slices / PER_WAVE), within the stage and none empty
  const uint32_t per_wave = msm_quad_per_wave(kind);
  for (s.nq = 1; (uint64_t)s.nq * s.nq * 4 <= s.segs_per_win;) s.nq <<= 1;  // ~ sqrt(segs_per_win), rounded to a power of two
  while (s.nq > 1 && (lists * s.nq > MSM_STAGE_PTS || s.nq * per_wave > s.segs_per_win)) s.nq >>= 1;
  return s;
}

// One run_device_multi call: its arguments, and per MSM what the stages below share.
template <class F>
struct MsmRunCall {
  // (the arguments, in their order)
  const MsmSort* const* sorts;
  const Affine<F>* const* bases;
  int nm;
  hipStream_t st;
  const hipStream_t* st_reduces;
  PhaseTimer* prof;
  int ph_accum, ph_reduce;
  const int* slots;
  hipStream_t st_heavy;
  const int* bucket_slots;
  int flags, third_slot;
  bool any_into;
  // per MSM: the bucket array its kernels write; its slot's redo list ([0] length, [1 ..] list, [cap_buckets + 1] ticket:
  // k_accum_redo); the stream of its heavy-bucket kernels, and whether that is another one than the accumulation's (then
  // they are queued in front of it)
  XYZZ<F>* bk[MSM_MULTI_MAX];
  uint32_t* redo[MSM_MULTI_MAX];
  hipStream_t heavy_stream[MSM_MULTI_MAX];
  bool heavy_first[MSM_MULTI_MAX];
  // bucket_slots[m] != slots[m] names another MSM's array.  MSM_RUN_ADD_AT_REDUCE (the product): a second SOURCE of this
  // MSM's reduction (k_segreduce adds both arrays); without the flag (A/B library): the array its kernels add INTO
  bool add_at_reduce() const { return (flags & MSM_RUN_ADD_AT_REDUCE) != 0; }
  int bslot(int m) const { return bucket_slots ? bucket_slots[m] : slots[m]; }
  bool into(int m) const { return !add_at_reduce() && bslot(m) != slots[m]; }
  bool second(int m) const { return add_at_reduce() && bslot(m) != slots[m]; }
  SortView view(int m) const { return SortView{sorts[m]->begin, sorts[m]->count, sorts[m]->perm, sorts[m]->sorted, sorts[m]->plan.heavy_thr}; }
  // the argument block of a fused accumulation launch (slots past nm repeat the first MSM)
  AccumArgs<F, true> fused_args() const {
    AccumArgs<F, true> set;
    for (int m = 0; m < MSM_MULTI_MAX; m++) {
      const int k = m < nm ? m : 0;
      set.bases_[m] = bases[k];
      set.buckets_[m] = bk[k];
      set.redo_[m] = redo[k];
      set.sort_[m] = view(k);
    }
    return set;
  }
};

// What the engine's steps launch: the kernels of its lane layout with LANES lanes per point (msm_impl.hpp "Lane layouts"),
// the quad / octet point type, and the accumulation's waves per SIMD.  Grid, block and LDS sizes below are expressions in LANES.
template <class F, int U = 0>
struct MsmEngineKernels {  // OneLane<F>: G1, BN254 G1
  static constexpr uint32_t LANES = 1, ACCUM_WAVES = 3;
  static constexpr MsmEngineKind KIND = std::is_same<F, BnFq28>::value ? MSM_ENGINE_BN254 : MSM_ENGINE_G1;
  using QPT = XYZZQ<F, 0, false>;
  static constexpr auto heavy_nc = &k_accum_heavy_nc<F, 3>;
  static constexpr auto segreduce2 = &k_segreduce2<F>;
  static constexpr auto treesum = &k_treesum<F>;
  static constexpr auto treesum_final = &k_treesum_final<F>;
};
template <int U>
struct MsmEngineKernels<Fq2_28, U> {  // LanePair: G2
  static constexpr uint32_t LANES = 2, ACCUM_WAVES = 2;
  static constexpr MsmEngineKind KIND = MSM_ENGINE_G2;
  using QPT = XYZZQ<Fq28, 0, true>;
  static constexpr auto heavy_nc = &k_accum_heavy_nc_g2<2 + U>;
  static constexpr auto segreduce2 = &k_segreduce2_g2_split<U>;
  static constexpr auto treesum = &k_treesum_g2_split<U>;
  static constexpr auto treesum_final = &k_treesum_final_g2_split<U>;
};

#ifdef ZKMI_EXPERIMENTS
}  // namespace zkmi
#include "msm_impl_exp.hpp"  // A/B library only: the retired kernel generations and what selects them
namespace zkmi {
#endif

// ---- stages of run_device_multi, in the order it runs them ----

// Records `ev` on stream `on`; `waiter`, where that is another stream, waits for it; `reads`: the sort whose buffers the
// kernels in front of `ev` read keeps it for the next sort into them, which may be queued on another stream (MsmSort::readers).
static inline hipError_t msm_signal(hipEvent_t ev, hipStream_t on, hipStream_t waiter, const MsmSort* reads = nullptr) {
  hipError_t e = hipEventRecord(ev, on);
  if (e == hipSuccess && waiter != on) e = hipStreamWaitEvent(waiter, ev, 0);
  if (e == hipSuccess && reads) reads->readers.push_back(ev);
  return e;
}

// The heavy-bucket kernels of one MSM.  Heavy and light buckets are disjoint, so they only have to see the sort complete.
template <class F>
static void msm_launch_heavy(const MsmEngine<F>& eng, const MsmRunCall<F>& c, const MsmRunSchedule& s, int m) {
  using K = MsmEngineKernels<F>;
  const MsmSort& sort = *c.sorts[m];
  const hipStream_t hs = c.heavy_stream[m];
  // MSMs of different slots may overlap: partial sums, plan and tickets per slot
  XYZZ<F>* const hp = eng.heavy_partial + (size_t)c.slots[m] * ((size_t)MSM_HPOOL + MSM_HNC_POOL);
  XYZZ<F>* const pool_nc = hp + MSM_HPOOL;
  uint32_t* const hplan = eng.heavy_plan + (size_t)c.slots[m] * MSM_HPLAN_WORDS;
  uint32_t* const tk = eng.heavy_ticket + (size_t)c.slots[m] * MSM_HEAVY_CAP;
  if (s.heavy_nc) {
    hipLaunchKernelGGL(k_heavy_plan<0>, dim3(1), dim3(64), 0, hs, sort.heavy, sort.count, sort.begin, hplan, 64u / K::LANES, 0u);
    // one-wave workgroups, grid-strided over the wave-items: twice the chip's wave slots (an empty list costs one placement)
    hipLaunchKernelGGL(K::heavy_nc, dim3(2048 * K::ACCUM_WAVES), dim3(64), 0, hs, c.bases[m], sort.sorted, hplan, pool_nc);
  }
  if (s.quad_heavy) {
    // both modes of the plan in one-wave workgroups of quads / octets: nothing of 300 registers has to find a SIMD beside the accumulation
    hipLaunchKernelGGL(k_heavy_q<typename K::QPT>, dim3(1024), dim3(64), 0, hs, c.bases[m], sort.begin, sort.count, sort.heavy,
                       sort.sorted, c.bk[m], hp, tk, hplan, pool_nc);
    return;
  }
  // the complete-law kernel; partitioned big windows: the tail of the list in a launch of its own (see k_accum_heavy)
  const uint32_t* const plan_arg = s.heavy_nc ? hplan : nullptr;
  const size_t lds = sizeof(XYZZ<F>) * MSM_TREE_T / K::LANES;
  for (int tail = 0; tail <= (s.wide ? 1 : 0); tail++) {
    const dim3 grid = tail ? dim3(1, 4096) : dim3(MSM_HSPLIT, 8);
    const uint32_t first = tail ? MSM_HEAVY_CAP : 0u, last = !tail && s.wide ? MSM_HEAVY_CAP : 0xffffffffu;
    if constexpr (K::LANES == 2)
      hipLaunchKernelGGL(k_accum_heavy_g2_split<0>, grid, dim3(MSM_TREE_T), lds, hs, c.bases[m], sort.begin, sort.count, sort.heavy,
                         sort.sorted, c.bk[m], hp, tk, first, last, tail ? nullptr : plan_arg, pool_nc);
    else
      hipLaunchKernelGGL(k_accum_heavy<F>, grid, dim3(MSM_TREE_T), lds, hs, c.bases[m], sort.begin, sort.count, sort.heavy,
                         sort.sorted, c.bk[m], hp, tk, c.into(m) ? 1u : 0u, first, last, tail ? nullptr : plan_arg, pool_nc);
  }
}

// In front of the accumulation: where MSM m's heavy-bucket kernels run, and their launch where that is another stream.
// They run at the head of the REDUCTION's stream.  With uniform scalars the heavy list is empty, but an empty 512-workgroup
// launch still has to be placed: on a normal-priority stream it queued behind the next accumulation's workgroups (0.9 ms G1 /
// 9.8 ms G2 average in the round-2 trace) and every reduction waited for it.  The reduction streams have high priority, so
// there the launch is placed as soon as any workgroup retires, and no cross-stream event sits between it and the
// reduction.  On another stream they are queued BEFORE the accumulation: their workgroups (two waves of up to 330 registers,
// 28-56 KB of LDS) are then placed while the SIMDs are still free; queued behind it they waited for the accumulation to drain.
template <class F>
static hipError_t msm_queue_heavy_in_front(MsmEngine<F>& eng, MsmRunCall<F>& c, const MsmRunSchedule& s, int m) {
  hipError_t e;
  const hipStream_t st = c.st, st_reduce = c.st_reduces[m];
  const bool on_reduce = s.heavy_on == 2 && st_reduce != st;
  const bool side = !on_reduce && s.heavy_on != 0 && c.st_heavy && c.st_heavy != st;
  c.heavy_first[m] = side || on_reduce;
  c.heavy_stream[m] = on_reduce ? st_reduce : side ? c.st_heavy : st;
  if (c.into(m)) {
    // the bucket array is complete once the first MSM's redo pass has run (it follows that MSM's accumulation and
    // heavy-bucket kernels on its reduction stream)
    const hipEvent_t filled = eng.redo_done[c.bslot(m)];
    if ((e = hipStreamWaitEvent(st, filled, 0)) != hipSuccess) return e;
    if (c.heavy_stream[m] != st && (e = hipStreamWaitEvent(c.heavy_stream[m], filled, 0)) != hipSuccess) return e;
    if (st_reduce != st && st_reduce != c.heavy_stream[m] && (e = hipStreamWaitEvent(st_reduce, filled, 0)) != hipSuccess) return e;
  }
  if (!c.heavy_first[m]) return hipSuccess;
  e = msm_signal(eng.pre[c.slots[m]], st, c.heavy_stream[m]);
  if (e == hipSuccess && !s.heavy_deferred) msm_launch_heavy(eng, c, s, m);
  return e;
}

// The accumulation: one of the product's five launches (MsmAccumForm), per MSM or fused.
template <class F>
static void msm_launch_accum(const MsmRunCall<F>& c, const MsmRunSchedule& s) {
  const uint32_t tot_b = s.tot_b;
  for (int m = 0; m < (s.fused ? 1 : c.nm); m++) {
#ifdef ZKMI_EXPERIMENTS
    if (msm_exp_launch_accum(c, s, m)) continue;
#endif
    if constexpr (MsmEngineKernels<F>::LANES == 2) {
      // a lane pair per bucket, or two (split2)
      const MsmSort& sort = *c.sorts[m];
      const bool split2 = s.accum == MSM_ACCUM_G2_SPLIT2;
      hipLaunchKernelGGL((split2 ? &k_accum_g2_split2<0> : &k_accum_g2_nc<2, 1>), dim3(((split2 ? 4 : 2) * tot_b + 63) / 64), dim3(64), 0, c.st,
                         c.bases[m], sort.begin, sort.count, sort.perm, sort.sorted, c.bk[m], tot_b, sort.plan.heavy_thr, c.redo[m]);
    } else if (s.fused) {
      // a lane per bucket, or two (split2); blockIdx.y = the MSM
      const bool split2 = s.accum == MSM_ACCUM_G1_SPLIT2;
      hipLaunchKernelGGL((split2 ? &k_accum_g1_split2<F, 1> : &k_accum_g1_nc<F, 3, 1, true>), dim3(((split2 ? 2 : 1) * tot_b + 63) / 64, c.nm),
                         dim3(64), 0, c.st, c.fused_args(), tot_b);
    } else {
      const AccumArgs<F, false> one = {c.bases[m], c.bk[m], c.redo[m], c.view(m)};
      hipLaunchKernelGGL((k_accum_g1_nc<F, 3, 1>), dim3((tot_b + 63) / 64), dim3(64), 0, c.st, one, tot_b);
    }
  }
}

// Behind the accumulation, MSM m: heavy kernels that run in line, the events that order the reduction stream behind both,
// and the redo pass.  Everything that still reads the sort leaves an event in sort.readers: the next sort into these
// buffers may be queued on another stream and must not overwrite what these kernels read.
template <class F>
static hipError_t msm_order_and_redo(MsmEngine<F>& eng, const MsmRunCall<F>& c, const MsmRunSchedule& s, int m) {
  using K = MsmEngineKernels<F>;
  hipError_t e;
  const MsmSort& sort = *c.sorts[m];
  const int slot = c.slots[m];
  const hipStream_t st = c.st, st_reduce = c.st_reduces[m];
  if (!c.heavy_first[m]) msm_launch_heavy(eng, c, s, m);
  if ((e = msm_signal(eng.acc_done[slot], st, st_reduce, &sort)) != hipSuccess) return e;
  // heavy kernels on a side stream; on the reduction's own stream redo_done below covers them too (same stream, later),
  // which only the call-free kernels record
  if (c.heavy_first[m] && (c.heavy_stream[m] != st_reduce || !s.nocall) &&
      (e = msm_signal(eng.heavy_done[slot], c.heavy_stream[m], st_reduce, &sort)) != hipSuccess)
    return e;
  if (!s.nocall) return hipSuccess;
  // after the accumulation (it writes the list), in front of the reduction (it reads the buckets);
  // heavy buckets are never listed, so the heavy kernels may still be running
  uint32_t* const redo = c.redo[m];
  uint32_t* const ticket = redo + eng.cap_buckets + 1;
  if (s.quad_redo)
    hipLaunchKernelGGL(k_accum_redo_q<typename K::QPT>, dim3(64), dim3(64), 0, st_reduce, c.bases[m], sort.begin, sort.count, sort.sorted,
                       c.bk[m], redo, ticket, c.into(m) ? 1u : 0u);
  else if constexpr (K::LANES == 2)
    hipLaunchKernelGGL(k_accum_redo_g2_split<0>, dim3(64), dim3(64), sizeof(XYZZ<F>) * 64 / K::LANES, st_reduce, c.bases[m], sort.begin,
                       sort.count, sort.sorted, c.bk[m], redo, ticket);
  else
    hipLaunchKernelGGL(k_accum_redo<F>, dim3(64), dim3(64), sizeof(XYZZ<F>) * 64 / K::LANES, st_reduce, c.bases[m], sort.begin,
                       sort.count, sort.sorted, c.bk[m], redo, ticket, c.into(m) ? 1u : 0u);
  return msm_signal(eng.redo_done[slot], st_reduce, st_reduce, &sort);  // (the list reads the sort)
}

// The reduction of MSM m on its stream: segment sums, the optional second level, tree sums, the slot's `done` event.
template <class F>
static hipError_t msm_launch_reduction(MsmEngine<F>& eng, const MsmRunCall<F>& c, const MsmRunSchedule& s, int m) {
  using K = MsmEngineKernels<F>;
  using QPT = typename K::QPT;
  using HF = typename MsmEngine<F>::HF;
  constexpr int T = 256;
  constexpr uint32_t SLOT_PTS = MsmEngine<F>::SLOT_PTS;
  hipError_t e;
  const int slot = c.slots[m];
  const hipStream_t st_reduce = c.st_reduces[m];
  const dim3 lists(s.njobs, c.sorts[0]->plan.nwin);
  if (c.prof) c.prof->begin(c.ph_reduce, st_reduce);
  XYZZ<F>* const bk = c.bk[m];
  XYZZ<F>* const ssum = eng.segsum + (size_t)slot * eng.seg_cap;
  XYZZ<F>* const sw = eng.segw + (size_t)slot * eng.seg_cap;
  const XYZZ<F>*bk2 = nullptr, *bk3 = nullptr;
  if (c.second(m)) {
    // the other MSM's bucket array is complete behind its redo pass (which follows its accumulation and heavy-bucket kernels)
    if ((e = hipStreamWaitEvent(st_reduce, eng.redo_done[c.bslot(m)], 0)) != hipSuccess) return e;
    bk2 = eng.buckets + (size_t)c.bslot(m) * eng.cap_buckets;
    if (c.third_slot >= 0) {
      if ((e = hipStreamWaitEvent(st_reduce, eng.redo_done[c.third_slot], 0)) != hipSuccess) return e;
      bk3 = eng.buckets + (size_t)c.third_slot * eng.cap_buckets;
    }
  }
  if (s.quad_seg)
    hipLaunchKernelGGL(k_segreduce_q<QPT>, dim3((s.tot_segs + QPT::PER_WAVE - 1) / QPT::PER_WAVE), dim3(64), 0, st_reduce, bk, ssum, sw,
                       s.tot_segs, s.seg, bk2, bk3);
  else if constexpr (K::LANES == 2)  // (the lane-pair segment sums have no second source)
    hipLaunchKernelGGL(k_segreduce_g2_split<0>, dim3((K::LANES * s.tot_segs + T - 1) / T), dim3(T), 0, st_reduce, bk, ssum, sw, s.tot_segs, s.seg);
  else  // (partitioned big windows: the two-wave build)
    hipLaunchKernelGGL((s.wide ? &k_segreduce_w2<F> : &k_segreduce<F>), dim3((K::LANES * s.tot_segs + T - 1) / T), dim3(T), 0, st_reduce, bk,
                       ssum, sw, s.tot_segs, s.seg, bk2, bk3);
  TreeLevel2<XYZZ<F>> l2 = {nullptr, nullptr, 0u, -1};
  if (s.level2) {
    XYZZ<F>* const s2 = eng.seg2 + (size_t)slot * 2 * (eng.seg_cap >> MSM_SEG2_LOG);
    XYZZ<F>* const t2 = s2 + (eng.seg_cap >> MSM_SEG2_LOG);
    hipLaunchKernelGGL(K::segreduce2, dim3((K::LANES * s.tot_segs2 + T - 1) / T), dim3(T), 0, st_reduce, ssum, s2, t2, s.tot_segs2);
    l2 = {s2, t2, s.segs2, s.t_job};
  }
  XYZZ<HF>* const dp = eng.partial + (size_t)slot * SLOT_PTS;
  XYZZ<HF>* const hp_out = eng.h_partial + (size_t)slot * SLOT_PTS;  // pinned host slot, written by the tree-sum kernels themselves
  XYZZ<F>* const stg = eng.tree_stage + (size_t)slot * MSM_STAGE_PTS;
  if (s.quad_tree) {
    hipLaunchKernelGGL(k_treesum_q<QPT>, dim3(lists.x, lists.y, s.nq), dim3(64), 0, st_reduce, ssum, sw, s.segs_per_win, dp, s.plain_job, stg, hp_out);
    if (s.nq > 1) hipLaunchKernelGGL(k_treesum_final_q<QPT>, lists, dim3(64), 0, st_reduce, stg, s.nq, dp, hp_out);
  } else {
    auto treesum = K::treesum;
#ifdef ZKMI_EXPERIMENTS
    msm_exp_treesum_unsplit<F>(s, &treesum);
#endif
    hipLaunchKernelGGL(treesum, dim3(lists.x, lists.y, s.nchunk), dim3(s.tree_block), s.tree_lds, st_reduce, ssum, sw, s.segs_per_win, dp,
                       s.plain_job, stg, hp_out, l2);
    if (s.nchunk > 1)
      hipLaunchKernelGGL(K::treesum_final, lists, dim3(s.final_block), s.final_lds, st_reduce, stg, s.nchunk, dp, hp_out);
  }
  if (c.prof) c.prof->end(c.ph_reduce, st_reduce);
  // (the partials are in the pinned host slot when the last tree-sum kernel has finished: the event is all that is left)
  return hipEventRecord(eng.done[slot], st_reduce);
}

template <class F>
hipError_t MsmEngine<F>::run_device(const MsmSort& sort, const Affine<F>* d_bases, hipStream_t st,
                                    hipStream_t st_reduce, PhaseTimer* prof, int ph_accum, int ph_reduce, int slot,
                                    hipStream_t st_heavy, int bucket_slot, int flags, int bucket_slot3) {
  const MsmSort* sp = &sort;
  return run_device_multi(&sp, &d_bases, 1, st, &st_reduce, prof, ph_accum, ph_reduce, &slot, st_heavy,
                          bucket_slot >= 0 ? &bucket_slot : nullptr, flags, bucket_slot3);
}

// nm MSMs of the same plan shape (sorts[m] may repeat: different tables over one digit sort): one fused accumulation
// launch where the kernel has a fused form (the call-free G1 kernels), otherwise nm launches in line; each MSM keeps
// its own slot and reduction stream.  All sorts must be complete on `st` (stream order or events) when this is called.
//
// Two MSMs whose results are only ever added (the prover's L and H queries: C = ... + L + H) can share one reduction: the
// first runs with MSM_RUN_NO_REDUCE (accumulation, heavy buckets and redo list only; its slot's `done` event is NOT recorded
// and it has no host result), the second names the first one's slot in bucket_slots[m] and
//   MSM_RUN_ADD_AT_REDUCE (the product): accumulates into its OWN array with the ordinary kernels; its k_segreduce adds both
//     arrays behind the first one's redo_done event -- the accumulations stay independent of each other;
//   without the flag (A/B library): its kernels add INTO the first one's array (k_accum_g1_nc<.., INTO>, k_accum_heavy /
//     k_accum_redo with into = 1) behind that event.
// Either way its reduction yields the sum of both.  Both sorts must plan the same bucket set (checked by the caller: the
// arrays are indexed by bucket id, and the ids mean the same digit values only under equal plans).
//
// Two invariants of the stages (stated here once):
//   - every refusal happens before the first launch or event record: an early return between the accumulation and
//     k_accum_redo would leave a redo list behind that the slot's next MSM appends to;
//   - sort.readers receives, per MSM and in this order: acc_done; heavy_done where the heavy kernels ran on a side stream
//     (or, with the retired accumulation kernels, on the reduction stream); redo_done.
template <class F>
hipError_t MsmEngine<F>::run_device_multi(const MsmSort* const* sorts, const Affine<F>* const* d_bases, int nm, hipStream_t st,
                                          const hipStream_t* st_reduces, PhaseTimer* prof, int ph_accum, int ph_reduce,
                                          const int* slots, hipStream_t st_heavy, const int* bucket_slots, int flags, int third_slot) {
  constexpr bool is_g2 = MsmEngineKernels<F>::LANES == 2;
  MsmRunCall<F> c = {sorts, d_bases, nm, st, st_reduces, prof, ph_accum, ph_reduce, slots, st_heavy, bucket_slots, flags, third_slot};
  // ---- the arguments ----
  if (nm < 1 || nm > MSM_MULTI_MAX) return hipErrorInvalidValue;
  // third_slot >= 0 (with MSM_RUN_ADD_AT_REDUCE, one MSM): a THIRD bucket array joins the segment sums
  if (third_slot >= nslots || (third_slot >= 0 && (nm != 1 || !c.add_at_reduce() || !bucket_slots))) return hipErrorInvalidValue;
  c.any_into = false;
  for (int m = 0; m < nm; m++) {
    if (slots[m] < 0 || slots[m] >= nslots) return hipErrorInvalidValue;
    if (bucket_slots && (bucket_slots[m] < 0 || bucket_slots[m] >= nslots)) return hipErrorInvalidValue;
    c.any_into = c.any_into || c.into(m);
  }
  if (c.add_at_reduce() && is_g2) return hipErrorInvalidValue;  // (the lane-pair segment sums have no second source)
  // the accumulate-into forms exist for the call-free G1 kernels, one MSM per launch
  if (c.any_into && (nm != 1 || is_g2)) return hipErrorInvalidValue;
  const MsmPlan& pl = sorts[0]->plan;  // bucket count, windows, segment length: common to all (checked); heavy_thr is per sort
  for (int m = 1; m < nm; m++) {
    const MsmPlan& q = sorts[m]->plan;
    if (q.nwin != pl.nwin || q.nb != pl.nb || q.seg_log != pl.seg_log || q.shared != pl.shared || q.c != pl.c) return hipErrorInvalidValue;
  }
  // ---- the schedule, and what the buffers cannot hold ----
  const MsmRunSchedule s = msm_run_schedule(pl, MsmEngineKernels<F>::KIND, host_spin, nm, flags, c.any_into);
  if (c.any_into && !s.nocall) return hipErrorInvalidValue;
  if (s.tot_segs > seg_cap || (uint64_t)(2 + s.seg_bits) * pl.nwin > SLOT_PTS || s.tot_b > cap_buckets) return hipErrorInvalidValue;
  for (int m = 0; m < nm; m++) {
    c.bk[m] = buckets + (size_t)(c.into(m) ? c.bslot(m) : slots[m]) * cap_buckets;
    c.redo[m] = redo + (size_t)slots[m] * (cap_buckets + 2);
  }
#ifdef ZKMI_EXPERIMENTS
  msm_exp_mask_sorted(c, s);
#else
  // (the retired accumulation kernels and the accumulate-into kernel are A/B variants: the product adds at the reduction)
  if (!s.nocall || c.any_into) return hipErrorInvalidValue;
#endif
  hipError_t e;
  // ---- in front of the accumulation: heavy-bucket kernels of every MSM that runs them on another stream ----
  for (int m = 0; m < nm; m++) {
    slot_plan[slots[m]] = sorts[m]->plan;
    slot_plan[slots[m]].seg2_log = s.seg2_log;
    if ((e = msm_queue_heavy_in_front(*this, c, s, m)) != hipSuccess) return e;
  }
  // ---- the accumulation (the phase brackets its launches only: roofline leg of bench.py) ----
  if (prof) prof->begin(ph_accum, st);
  msm_launch_accum(c, s);
  if (prof) prof->end(ph_accum, st);
  for (int m = 0; m < nm && s.heavy_deferred; m++)
    if (c.heavy_first[m]) msm_launch_heavy(*this, c, s, m);
  // ---- behind it, per MSM: heavy kernels that run in line, events, redo pass, reduction ----
  for (int m = 0; m < nm; m++) {
    if ((e = msm_order_and_redo(*this, c, s, m)) != hipSuccess) return e;
    // MSM_RUN_NO_REDUCE: a later MSM takes these buckets into its reduction (bucket_slots); the slot's `done` event is not recorded
    if (flags & MSM_RUN_NO_REDUCE) continue;
    if ((e = msm_launch_reduction(*this, c, s, m)) != hipSuccess) return e;
  }
  return hipGetLastError();
}

template <class F>
hipError_t MsmEngine<F>::finish_host_windows(XYZZ<HF>* out_windows, int slot) {
  hipError_t e = wait_event(done[slot], host_spin);  // (host_pool.hpp: the batch prover's driving thread polls, then sleeps)
  if (e != hipSuccess) return e;
  // (host_spin = one MSM or one proof by itself: the latency path)
  windows_from_partials(slot_plan[slot], h_partial + (size_t)slot * SLOT_PTS, out_windows, host_spin);
  return hipSuccess;
}

// the per-(window, job) sums a reduction leaves behind -> one sum per window (host arithmetic).  `h` may come from this
// device's pinned slot or from another rank's copy of the same array (comm.hip: the all-gathered partials of a point split).
template <class F>
int MsmEngine<F>::partials_per_msm(const MsmPlan& pl) { return pl.nwin * msm_njobs(pl); }
template <class F>
void MsmEngine<F>::windows_from_partials(const MsmPlan& pl, const XYZZ<HF>* h, XYZZ<HF>* out_windows, bool parallel) {
  const int seg_bits = msm_seg_bits(pl) - pl.seg2_log;  // bit jobs: over the segments, or over the second level's super-segments
  const int njobs = msm_njobs(pl);
  const std::function<void(uint32_t)> one = [&](uint32_t w) {
    XYZZ<HF> u = XYZZ<HF>::infinity();
    // (top window of a partitioned big-window plan: the top bits of the segment index number the partition its entries
    // were spread to, not the digit -- MsmPlan::top_spread_log)
    const int bits = (pl.win_first + (int)w == pl.total_windows() - 1 && pl.top_spread_log > 0) ? seg_bits - pl.top_spread_log : seg_bits;
    for (int j = bits - 1; j >= 0; j--) {
      u.dbl_inplace();
      u.add(h[(size_t)w * njobs + 1 + j]);
    }
    if (pl.seg2_log) {
      // sum_t t segsum_t = 2^seg2_log sum_u u segsum2_u + sum_u segt2_u (k_segreduce2)
      for (int i = 0; i < pl.seg2_log; i++) u.dbl_inplace();
      u.add(h[(size_t)w * njobs + njobs - 2]);
    }
    for (int i = 0; i < pl.seg_log; i++) u.dbl_inplace();
    u.add(h[(size_t)w * njobs]);
    out_windows[w] = u;
  };
  // One MSM by itself: its 13-16 windows (or partitions) are ~30 group operations each -- 0.3 ms on one thread between the
  // last kernel and the result, a seventh of a witness-like 2^20-term MSM; on the process's pool they run side by side.
  if (parallel && pl.nwin >= 8) {
    HostPool::instance().run((uint32_t)pl.nwin, host_cpu_budget(), one);
  } else {
    for (int w = 0; w < pl.nwin; w++) one((uint32_t)w);
  }
}

// shared buckets: partition q of a vector holds buckets q*nb + j (digit value q*nb + j + 1):
//   sum_b (b+1) B_b = sum_q U_q + nb * sum_q q * S_q,   U_q = weighted sum, S_q = plain sum of partition q
template <class HF>
static XYZZ<HF> msm_combine_partitions(const XYZZ<HF>* win, const XYZZ<HF>* h, int parts, int njobs, uint32_t nb) {
  XYZZ<HF> run = XYZZ<HF>::infinity(), t = XYZZ<HF>::infinity(), total = XYZZ<HF>::infinity();
  for (int q = parts - 1; q >= 1; q--) {
    run.add(h[(size_t)q * njobs + (njobs - 1)]);
    t.add(run);
  }
  for (uint32_t b = nb; b > 1; b >>= 1) t.dbl_inplace();
  for (int q = 0; q < parts; q++) total.add(win[q]);
  total.add(t);
  return total;
}

template <class F>
hipError_t MsmEngine<F>::finish_host_batch(XYZZ<HF>* out, int slot) {
  // the batched plan holds, per scalar vector, the vec_parts partitions of that vector's own bucket set
  const MsmPlan& pl = slot_plan[slot];
  if (pl.vec_parts <= 1) return finish_host_windows(out, slot);
  std::vector<XYZZ<HF>> win(pl.nwin);
  hipError_t e = finish_host_windows(win.data(), slot);
  if (e != hipSuccess) return e;
  const int njobs = msm_njobs(pl);
  const XYZZ<HF>* h = h_partial + (size_t)slot * SLOT_PTS;
  for (int v = 0; v * pl.vec_parts < pl.nwin; v++)
    out[v] = msm_combine_partitions<HF>(win.data() + (size_t)v * pl.vec_parts, h + (size_t)v * pl.vec_parts * njobs, pl.vec_parts,
                                        njobs, pl.nb);
  return hipSuccess;
}

template <class F>
hipError_t MsmEngine<F>::wait_slot(int slot) {
  return wait_event(done[slot], host_spin);
}
template <class F>
XYZZ<typename MsmEngine<F>::HF> MsmEngine<F>::host_result_vec(int slot, int v) const {
  const MsmPlan& pl = slot_plan[slot];
  const int vp = pl.vec_parts > 1 ? pl.vec_parts : 1;
  const int njobs = msm_njobs(pl);
  const XYZZ<HF>* h = h_partial + (size_t)slot * SLOT_PTS + (size_t)v * vp * njobs;
  MsmPlan mine = pl;  // the partitions of this vector only
  mine.nwin = vp;
  XYZZ<HF> win[64];
  windows_from_partials(mine, h, win);
  if (vp == 1) return win[0];
  return msm_combine_partitions<HF>(win, h, vp, njobs, pl.nb);
}

template <class HF>
XYZZ<HF> msm_combine_windows(const XYZZ<HF>* windows, int nwin, int c) {
  XYZZ<HF> total = XYZZ<HF>::infinity();
  for (int w = nwin - 1; w >= 0; w--) {
    for (int i = 0; i < c; i++) total.dbl_inplace();
    total.add(windows[w]);
  }
  return total;
}

template <class F>
hipError_t MsmEngine<F>::finish_host(XYZZ<HF>* out, int slot) {
  const MsmPlan& pl = slot_plan[slot];
  std::vector<XYZZ<HF>> win(pl.nwin);
  hipError_t e = finish_host_windows(win.data(), slot);
  if (e != hipSuccess) return e;
  if (!pl.shared) {
    *out = msm_combine_windows(win.data(), pl.nwin, pl.c);
    return hipSuccess;
  }
  *out = msm_combine_partitions<HF>(win.data(), h_partial + (size_t)slot * SLOT_PTS, pl.nwin, msm_njobs(pl), pl.nb);
  return hipSuccess;
}

// table[w * n + i] = 2^(c w) * bases[i]: one thread per base point walks the digits
template <class F>
__global__ void __launch_bounds__(64)
k_build_table(const Affine<F>* __restrict__ bases, Affine<F>* __restrict__ table, uint32_t n, int ndigits, int c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = load_vec(bases + i);
  XYZZ<F> cur = XYZZ<F>::from_affine(p);
  store_vec(table + i, p);
  for (int w = 1; w < ndigits; w++) {
    for (int k = 0; k < c; k++) cur.dbl_inplace();
    const Affine<F> a = cur.to_affine();
    // points at infinity must be exact zeros (the accumulate kernels test limbs)
    Affine<F> o = cur.is_inf() ? Affine<F>::infinity() : a;
    store_vec(table + (size_t)w * n + i, o);
  }
}

template <class F>
hipError_t msm_build_table(const Affine<F>* d_bases, uint64_t n, const MsmPlan& plan, Affine<F>** out_table,
                           hipStream_t st) {
  *out_table = nullptr;
  hipError_t e = hipMalloc(out_table, sizeof(Affine<F>) * (size_t)plan.ndigits * (n ? n : 1));
  if (e != hipSuccess) return e;
  if (n) {
    hipLaunchKernelGGL(k_build_table<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_bases, *out_table,
                       (uint32_t)n, plan.ndigits, plan.c);
    e = hipGetLastError();
  }
  return e;
}

template <class F>
hipError_t bases_convert(const Affine<typename HostFieldOf<F>::type>* d_in, Affine<F>* d_out, uint64_t n,
                         hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_bases_convert<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_in, d_out, (uint32_t)n);
  return hipGetLastError();
}

}  // namespace zkmi
