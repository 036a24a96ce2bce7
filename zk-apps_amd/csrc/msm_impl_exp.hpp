// zkmi — A/B LIBRARY ONLY (-DZKMI_EXPERIMENTS): the retired generations of the MSM accumulation kernels that the switches of
// tune.hpp still select in libzkmi_exp.so -- the first thread-per-bucket kernels with an out-of-line doubling path (ZKMI_ACCUM
// = 0 / 1), the first lane-pair G2 kernel (ZKMI_ACCUM_G2 = 0), and the occupancy-capped two-wave build of the call-free G1
// kernel (the pipelined big MSM, msm_pipe.hpp: measured neutral; ZKMI_ACCUM_W2 = 1).  The two-wave kernel is an entry point
// around msm_impl.hpp's accum_g1_nc_body, the product kernel's own body: it has no copy of the loop here, and with the
// shared body it takes the first-pair step (madd_affine_pair) too -- the bytes of its results do not change.  Nothing here
// is compiled into the product library; the variants test (tests/test_gpu_sizes.py::
// test_ab_switches_do_not_change_any_result) holds every one of them to its bytes.
// Included by msm_impl.hpp behind the definitions it uses (load_vec / store_vec, ld_comp / st_comp, AccumArgs,
// accum_g1_nc_body).
#pragma once

namespace zkmi {

// ---- retired accumulation kernels (A/B library only: ZKMI_ACCUM=0|1, ZKMI_ACCUM_G2=0|1) ----
// G1 (14-limb coordinates): 248 VGPRs -> 2 waves per SIMD.  G2 needs ~330 registers
// (accumulator 112 + point 56 + columns 56 + temporaries) and runs at 1 wave per SIMD with
// cheap AGPR spills; forcing 2 waves sends 350+ values to scratch and is 2x slower.
template <class F>
struct AccumWaves {
  static constexpr int value = (sizeof(F) <= 64) ? 2 : 1;  // measured: forcing 3 for G1 spills around the rare-path calls and is 25 % slower
};
template <class F>
__global__ void __launch_bounds__(256, AccumWaves<F>::value)
k_accum(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ begin,
        const uint32_t* __restrict__ count, const uint32_t* __restrict__ perm,
        const uint32_t* __restrict__ sorted, XYZZ<F>* __restrict__ buckets, uint32_t total_buckets,
        uint32_t heavy_thr) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total_buckets) return;
  const uint32_t b = perm[t];  // lanes of a wave own buckets of near-equal load
  const uint32_t cnt = count[b];
  if (cnt > heavy_thr) return;  // k_accum_heavy owns it
  const uint32_t beg = begin[b], end = beg + cnt;
  XYZZ<F> acc = XYZZ<F>::infinity();
  // (prefetching the next point into registers costs 28 VGPRs and gains nothing; the G1 path of
  // the prover prefetches through LDS instead: k_accum_g1_glds below)
  for (uint32_t j = beg; j < end; j++) {
    const uint32_t v = sorted[j];
    Affine<F> p = load_vec(bases + (v & 0x7fffffffu));
    if (v >> 31) p.y = p.y.neg();
    acc.madd(p);
  }
  store_vec(buckets + b, acc);
}

// G1 accumulation with the gather of the NEXT point in flight during the current mixed addition,
// at no register cost: the 112-byte (BLS12-381) or 80-byte (BN254) table entry is fetched by seven direct-to-LDS loads
// (global_load_lds_dwordx4: per-lane source address, destination = wave-uniform LDS base + 16 B x lane),
// into one of two LDS buffers.  Order inside an iteration: wait -> read point j from LDS -> issue the
// loads of point j+1 and of index j+2 -> mixed addition (no memory operation inside it).
// LDS: 2 buffers x 256 threads x 112 B = 56 KB per block, two blocks per CU (VGPR-limited anyway).
// BW = waves per workgroup.  One-wave workgroups (BW = 1) free their slot the moment the wave retires; a
// 4-wave workgroup can only start once all four SIMDs of a CU have a free slot at the same time.
// The loop strides the load-ordered bucket list by the grid size: with a grid of one wave per bucket group
// it runs once (dynamic dispatch, heaviest groups first); with a smaller grid every wave takes a heavy, a
// medium and a light group in turn (ZKMI_ACCUM_ROUNDS) and nothing depends on the dispatcher's refill rate.
template <class F, int BW>
__global__ void __launch_bounds__(64 * BW, AccumWaves<F>::value)
k_accum_g1_glds(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ begin,
                const uint32_t* __restrict__ count, const uint32_t* __restrict__ perm,
                const uint32_t* __restrict__ sorted, XYZZ<F>* __restrict__ buckets, uint32_t total_buckets,
                uint32_t heavy_thr) {
  constexpr int CHUNKS = sizeof(Affine<F>) / 16;  // 7 (BLS12-381 Fq), 5 (BN254 Fq)
  __shared__ uint4 tile[2][BW][CHUNKS][64];           // [buffer][wave][chunk][lane]
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total_buckets; t += stride) {
    const uint32_t b = perm[t];  // lanes of a wave own buckets of near-equal load
    const uint32_t cnt = count[b];
    if (cnt > heavy_thr) continue;  // k_accum_heavy owns it
    const uint32_t beg = begin[b], end = beg + cnt;
    XYZZ<F> acc = XYZZ<F>::infinity();
    auto fetch = [&](uint32_t v, int buf) {
      const char* src = reinterpret_cast<const char*>(bases + (v & 0x7fffffffu));
#pragma unroll
      for (int q = 0; q < CHUNKS; q++)
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + 16 * q), (lds_ptr_t)&tile[buf][wave][q][0], 16, 0, 0);
    };
    uint32_t v_cur = 0, v_next = 0;
    if (cnt) {
      v_cur = sorted[beg];
      fetch(v_cur, 0);
      if (cnt > 1) v_next = sorted[beg + 1];
    }
    int buf = 0;
    for (uint32_t j = beg; j < end; j++) {
      // the compiler waits for the outstanding LDS-DMA (vmcnt) before these LDS reads
      Affine<F> p;
      uint4* d = reinterpret_cast<uint4*>(&p);
#pragma unroll
      for (int q = 0; q < CHUNKS; q++) d[q] = tile[buf][wave][q][lane];
      const uint32_t v = v_cur;
      if (j + 1 < end) {
        fetch(v_next, buf ^ 1);
        v_cur = v_next;
        if (j + 2 < end) v_next = sorted[j + 2];
      }
      buf ^= 1;
      if (v >> 31) p.y = p.y.neg();
      acc.madd(p);
    }
    store_vec(buckets + b, acc);
  }
}

template <int BW>
__global__ void __launch_bounds__(64 * BW, 2)
k_accum_g2_split(const Affine<Fq2_28>* __restrict__ bases, const uint32_t* __restrict__ begin,
                 const uint32_t* __restrict__ count, const uint32_t* __restrict__ perm,
                 const uint32_t* __restrict__ sorted, XYZZ<Fq2_28>* __restrict__ buckets, uint32_t total_buckets,
                 uint32_t heavy_thr) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x; (gt >> 1) < total_buckets; gt += stride) {
    const uint32_t t = gt >> 1, comp = gt & 1u;
    const uint32_t b = perm[t];
    const uint32_t cnt = count[b];
    if (cnt > heavy_thr) continue;  // pair-uniform
    const uint32_t beg = begin[b], end = beg + cnt;
    XYZZ<Fq2P> acc = XYZZ<Fq2P>::infinity();
    for (uint32_t j = beg; j < end; j++) {
      const uint32_t v = sorted[j];
      const Fq28* src = reinterpret_cast<const Fq28*>(bases + (v & 0x7fffffffu));  // x.c0 x.c1 y.c0 y.c1
      Affine<Fq2P> p;
      p.x.v = ld_comp(src + comp);
      p.y.v = ld_comp(src + 2 + comp);
      if (v >> 31) p.y = p.y.neg();
      acc.madd(p);
    }
    Fq28* dst = reinterpret_cast<Fq28*>(buckets + b);  // x.c0 x.c1 y.c0 y.c1 zz.c0 zz.c1 zzz.c0 zzz.c1
    st_comp(dst + comp, acc.x.v);
    st_comp(dst + 2 + comp, acc.y.v);
    st_comp(dst + 4 + comp, acc.zz.v);
    st_comp(dst + 6 + comp, acc.zzz.v);
  }
}

// k_accum_g1_nc's body (msm_impl.hpp accum_g1_nc_body) CAPPED at two waves per SIMD with at most 176 registers (352 of a
// SIMD's 512: the kernel descriptor is padded to the occupancy limit): it leaves 160 registers per SIMD, ~100 KB of LDS per
// CU and six wave slots per SIMD to OTHER kernels.  The three-wave kernel above fills 504 registers and nothing runs beside
// it; the issue rate of the additions is the same at two and at three waves (round 2).  Used by the
// pipelined form of one big windowed MSM (BASELINE config 3): the digit sort of the second window group runs beside the
// first group's accumulation.
template <class F>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2), amdgpu_num_vgpr(176)))
k_accum_g1_nc_w2(const AccumArgs<F, false> args, uint32_t total_buckets) {
  accum_g1_nc_body<F, 1, false, false>(args, total_buckets);
}

// TIMING ONLY (ZKMI_GATHER_MASK_BITS = k > 0): every table index of a sort is cut to its low k bits before the accumulation
// reads it, so that all gathers hit a sub-table of 2^k entries that stays in L2.  The sums are WRONG by design: what is left
// of a launch's time and held clock is the arithmetic alone, the bound of what any change to the fetch path can give.
template <int UNUSED = 0>
__global__ void k_mask_sorted(uint32_t* __restrict__ sorted, uint64_t n, uint32_t keep) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) sorted[i] &= keep;
}

// ---- what selects them: the A/B library's side of MsmEngine::run_device_multi (msm_impl.hpp) ----
// In front of everything a call queues (all cap_entries words of the buffer: idempotent, and a sort may serve several MSMs).
template <class F>
static void msm_exp_mask_sorted(const MsmRunCall<F>& c, const MsmRunSchedule& s) {
  if (s.exp_mask_bits <= 0 || s.exp_mask_bits >= 31) return;
  for (int m = 0; m < c.nm; m++)
    hipLaunchKernelGGL(k_mask_sorted<0>, dim3(1024), dim3(256), 0, c.st, c.sorts[m]->sorted, c.sorts[m]->cap_entries,
                       0x80000000u | ((1u << s.exp_mask_bits) - 1u));
}

// The accumulation of MSM m (s.fused: of all MSMs of the call, m = 0) where a switch selects another launch than the
// product's; false: the product's launch follows.
//   ZKMI_ACCUM_G2 = 3: the G2 kernel at three waves; ZKMI_ACCUM / ZKMI_ACCUM_G2 = 0 | 1: the retired kernels above, in
//   workgroups of ZKMI_ACCUM_BLOCK threads, every wave walking ZKMI_ACCUM_ROUNDS bucket groups; ZKMI_ACCUM = 2: two waves;
//   ZKMI_QUAD* bit 4: a quad / octet per bucket (msm_quad.hpp k_accum_q: the complete law in line, no redo list) for plans of at
//   most 2^16 buckets; bucket_slots without MSM_RUN_ADD_AT_REDUCE: the accumulate-INTO kernel; MSM_RUN_TWO_WAVES (the pipelined
//   big MSM, msm_pipe.hpp: measured neutral) or ZKMI_ACCUM_W2 = 1: the occupancy-capped kernel.
template <class F>
static bool msm_exp_launch_accum(const MsmRunCall<F>& c, const MsmRunSchedule& s, int m) {
  using K = MsmEngineKernels<F>;
  using QPT = typename K::QPT;
  const MsmSort& sort = *c.sorts[m];
  const uint32_t tot_b = s.tot_b, heavy_thr = sort.plan.heavy_thr, block = s.exp_accum_block;
  const hipStream_t st = c.st;
  // grid of the retired kernels: one thread per bucket (G2: two), the waves striped over ZKMI_ACCUM_ROUNDS groups
  auto striped = [&s, block](uint32_t threads) {
    const uint32_t g = (threads + block - 1) / block, rounds = s.exp_accum_rounds > 1 ? s.exp_accum_rounds : 1;
    return g ? (g + rounds - 1) / rounds : 1u;
  };
  // a quad / octet per bucket; blockIdx.y = the MSM of a fused launch (slots past nm repeat the first MSM)
  auto launch_q = [&c, &s, m, tot_b, st] {
    AccumQArgs<QPT> qa;
    for (int k = 0; k < MSM_MULTI_MAX; k++) {
      const int j = s.fused ? (k < c.nm ? k : 0) : m;
      qa.bases[k] = c.bases[j];
      qa.buckets[k] = c.bk[j];
      qa.sort[k] = c.view(j);
    }
    hipLaunchKernelGGL(k_accum_q<QPT>, dim3((tot_b + QPT::PER_WAVE - 1) / QPT::PER_WAVE, s.fused ? c.nm : 1), dim3(64), 0, st, qa, tot_b);
  };
  if constexpr (K::LANES == 2) {
    if (s.exp_accum_mode == 3)
      hipLaunchKernelGGL((k_accum_g2_nc<3, 1>), dim3((2 * tot_b + 63) / 64), dim3(64), 0, st, c.bases[m], sort.begin, sort.count, sort.perm,
                         sort.sorted, c.bk[m], tot_b, heavy_thr, c.redo[m]);
    else if (s.exp_accum_mode != 2)
      hipLaunchKernelGGL((block == 64 ? &k_accum_g2_split<1> : &k_accum_g2_split<4>), dim3(striped(2 * tot_b)), dim3(block), 0, st, c.bases[m],
                         sort.begin, sort.count, sort.perm, sort.sorted, c.bk[m], tot_b, heavy_thr);
    else if (s.exp_accum_q)
      launch_q();
    else
      return false;
  } else if (s.fused) {
    if (s.exp_accum_q)
      launch_q();
    else if (s.accum != MSM_ACCUM_G1_SPLIT2 && s.exp_accum_mode != 3)
      hipLaunchKernelGGL((k_accum_g1_nc<F, 2, 1, true>), dim3((tot_b + 63) / 64, c.nm), dim3(64), 0, st, c.fused_args(), tot_b);
    else
      return false;
  } else {
    const AccumArgs<F, false> one = {c.bases[m], c.bk[m], c.redo[m], c.view(m)};
    if (c.into(m))
      hipLaunchKernelGGL((k_accum_g1_nc<F, 3, 1, false, true>), dim3((tot_b + 63) / 64), dim3(64), 0, st, one, tot_b);
    else if (s.exp_accum_mode == 2)
      hipLaunchKernelGGL((k_accum_g1_nc<F, 2, 1>), dim3((tot_b + 63) / 64), dim3(64), 0, st, one, tot_b);
    else if (s.exp_accum_mode == 1)
      hipLaunchKernelGGL(k_accum<F>, dim3((tot_b + 255) / 256), dim3(256), 0, st, c.bases[m], sort.begin, sort.count, sort.perm, sort.sorted,
                         c.bk[m], tot_b, heavy_thr);
    else if (s.exp_accum_mode != 3)
      hipLaunchKernelGGL((block == 64 ? &k_accum_g1_glds<F, 1> : &k_accum_g1_glds<F, 4>), dim3(striped(tot_b)), dim3(block), 0, st, c.bases[m],
                         sort.begin, sort.count, sort.perm, sort.sorted, c.bk[m], tot_b, heavy_thr);
    else if (s.exp_two_waves)
      hipLaunchKernelGGL(k_accum_g1_nc_w2<F>, dim3((tot_b + 63) / 64), dim3(64), 0, st, one, tot_b);
    else
      return false;
  }
  return true;
}

// ZKMI_G2_TREE_SPLIT = 0: the unsliced G2 tree sum by the one-lane kernel (a lane per point: 330-register additions; the
// schedule sizes the workgroup for it); true: *kernel is that kernel
template <class F, class Kernel>
static bool msm_exp_treesum_unsplit(const MsmRunSchedule& s, Kernel* kernel) {
  if (s.exp_g2_tree_unsplit) *kernel = &k_treesum<F>;
  return s.exp_g2_tree_unsplit;
}

}  // namespace zkmi
