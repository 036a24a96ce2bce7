// zkmi — the resident Poseidon note tree: batched appends, the root after each leaf, and paths, all in HBM
// (include/zkmi.h "note tree"; layout and the padding rule: note_tree.hpp).
//
// This is the relation's tree of merkle_proof.rs:38-61 at the heights the relation admits, not the contract's SHA-256
// tree (sha_merkle.hip).  An append of m leaves behind n0 stored ones recomputes, at level l, exactly the nodes
// (n0 >> l) .. ((n0 + m - 1) >> l): one launch per level while a level has more than 256 nodes to compute, then ONE
// single-workgroup launch for all remaining levels up to the root, with a workgroup barrier between levels.  No kernel
// waits on another workgroup; a dependence wider than a workgroup is the launch boundary on the context's stream.
#include <string.h>
#include <new>
#include "ctx.hpp"
#include "note_tree.hpp"
#include "poseidon.hpp"

namespace zkmi {
namespace {

constexpr uint32_t NT_BLOCK = 256;  // lanes per workgroup = nodes the tail computes per level

struct ModWords {
  uint32_t w[8];
};

__device__ __forceinline__ void nt_load(const uint32_t* p, uint32_t* w) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
  w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}
__device__ __forceinline__ void nt_store(uint32_t* p, const uint32_t* w) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// out = H(left, right), canonical words in and out
template <class F>
__device__ __forceinline__ void nt_hash(const uint32_t* left, const uint32_t* right, const PoseidonConsts<F>* __restrict__ c,
                                        int32_t* col, uint32_t* out) {
  uint32_t pair[16];
  nt_load(left, pair);
  nt_load(right, pair + 8);
  const F h = poseidon_hash_words_lds<F>(pair, 2, c, col);
  h.to_canonical(out);
}

// node p of `level` >= 1 from its children; cnt_below = nodes the level below stores (a right child behind them is Z)
template <class F>
__device__ __forceinline__ void nt_node(const NoteTreeView& t, uint32_t level, uint64_t p, uint64_t cnt_below,
                                        const PoseidonConsts<F>* __restrict__ c, int32_t* col) {
  const uint32_t* left = t.node(level - 1, 2 * p);
  const uint32_t* right = 2 * p + 1 < cnt_below ? t.node(level - 1, 2 * p + 1) : t.z(level - 1);
  uint32_t w[8];
  nt_hash<F>(left, right, c, col, w);
  nt_store(t.node(level, p), w);
}

// Z_0 = 0, Z_{l+1} = H(Z_l, Z_l): one lane, once per tree
template <class F>
__global__ __launch_bounds__(NT_BLOCK, 3) void k_nt_zinit(NoteTreeView t, const PoseidonConsts<F>* __restrict__ c) {
  __shared__ int32_t tile[POS_LDS_WORDS];
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  nt_store(t.base + 8 * t.z_off, w);
#pragma unroll 1
  for (uint32_t l = 0; l < t.height; l++) {
    nt_hash<F>(t.z(l), t.z(l), c, tile, w);
    nt_store(t.base + 8 * (t.z_off + l + 1), w);
  }
}

// flag = 1 when some leaf is >= the modulus (nothing else is written)
__global__ __launch_bounds__(NT_BLOCK) void k_nt_check(const uint32_t* __restrict__ leaves, uint64_t m, ModWords mod,
                                                       uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * NT_BLOCK + threadIdx.x;
  if (i >= m) return;
  uint32_t w[8];
  nt_load(leaves + 8 * i, w);
  bool lt = false, decided = false;
#pragma unroll
  for (int k = 7; k >= 0; k--)
    if (!decided && w[k] != mod.w[k]) {
      lt = w[k] < mod.w[k];
      decided = true;
    }
  if (!lt) *flag = 1u;
}

// nodes lo .. lo + count - 1 of `level`, one lane per node
template <class F>
__global__ __launch_bounds__(NT_BLOCK, 3) void k_nt_level(NoteTreeView t, uint32_t level, uint64_t lo, uint64_t count,
                                                          uint64_t cnt_below, const PoseidonConsts<F>* __restrict__ c) {
  __shared__ int32_t tile[POS_LDS_WORDS];
  const uint64_t i = (uint64_t)blockIdx.x * NT_BLOCK + threadIdx.x;
  if (i >= count) return;
  nt_node<F>(t, level, lo + i, cnt_below, c, tile + threadIdx.x);
}

// every level from first_level to the root, each with at most NT_BLOCK nodes to compute, in one workgroup: the nodes a
// level writes are the children the next one reads, so a fence and a workgroup barrier stand between them
template <class F>
__global__ __launch_bounds__(NT_BLOCK, 3) void k_nt_tail(NoteTreeView t, uint32_t first_level, uint64_t n0, uint64_t n_new,
                                                         const PoseidonConsts<F>* __restrict__ c) {
  __shared__ int32_t tile[POS_LDS_WORDS];
#pragma unroll 1
  for (uint32_t level = first_level; level <= t.height; level++) {
    const uint64_t lo = n0 >> level, hi = (n_new - 1) >> level;
    if (threadIdx.x <= hi - lo) nt_node<F>(t, level, lo + threadIdx.x, NoteTreeView::count(n_new, level - 1), c, tile + threadIdx.x);
    __threadfence();
    __syncthreads();
  }
}

// out[j] = the root of the tree holding leaves 0 .. n0 + j, for the m leaves just appended.  The lane of leaf g walks up
// with its own running node: where its position p = g >> l is odd the left sibling p - 1 covers only leaves < g and is
// final as stored; where p is even everything to its right is padding, Z_l.
template <class F>
__global__ __launch_bounds__(NT_BLOCK, 3) void k_nt_leaf_roots(NoteTreeView t, uint64_t n0, uint64_t m, uint32_t* __restrict__ out,
                                                               const PoseidonConsts<F>* __restrict__ c) {
  __shared__ int32_t tile[POS_LDS_WORDS];
  const uint64_t j = (uint64_t)blockIdx.x * NT_BLOCK + threadIdx.x;
  if (j >= m) return;
  const uint64_t g = n0 + j;
  uint32_t cur[8], pair[16];
  nt_load(t.node(0, g), cur);
#pragma unroll 1
  for (uint32_t level = 0; level < t.height; level++) {
    const uint64_t p = g >> level;
    const bool odd = (p & 1) != 0;
    uint32_t other[8];
    nt_load(odd ? t.node(level, p - 1) : t.z(level), other);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      pair[k] = odd ? other[k] : cur[k];
      pair[8 + k] = odd ? cur[k] : other[k];
    }
    const F h = poseidon_hash_words_lds<F>(pair, 2, c, tile + threadIdx.x);
    h.to_canonical(cur);
  }
  nt_store(out + 8 * j, cur);
}

// thread (i, l): sibling of leaf idx[i] at level l and its shape byte (k_merkle_paths' convention: 0 = the sibling is
// the left input), leaf level first
__global__ __launch_bounds__(NT_BLOCK) void k_nt_paths(NoteTreeView t, uint64_t n, const uint64_t* __restrict__ idx, uint32_t k,
                                                       uint8_t* __restrict__ shape, uint32_t* __restrict__ paths) {
  const uint64_t q = (uint64_t)blockIdx.x * NT_BLOCK + threadIdx.x;
  if (q >= (uint64_t)k * t.height) return;
  const uint32_t i = (uint32_t)(q / t.height), level = (uint32_t)(q % t.height);
  const uint64_t pos = idx[i] >> level;
  uint32_t w[8];
  nt_load(t.node_or_z(n, level, pos ^ 1), w);
  shape[q] = (uint8_t)(1u - (uint32_t)(pos & 1));
  nt_store(paths + 8 * q, w);
}

hipError_t ensure_consts(zkmi_ctx* ctx, int field) {
  if (ctx->d_pos[field]) return hipSuccess;
  const size_t bytes = field == ZKMI_FIELD_BLS12_381_FR ? sizeof(PoseidonConsts<Fr28>) : sizeof(PoseidonConsts<BnFr28>);
  const void* host = field == ZKMI_FIELD_BLS12_381_FR ? static_cast<const void*>(poseidon_consts_bls())
                                                      : static_cast<const void*>(poseidon_consts_bn());
  hipError_t e = hipMalloc(&ctx->d_pos[field], bytes);
  if (e != hipSuccess) return e;
  e = hipMemcpy(ctx->d_pos[field], host, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(ctx->d_pos[field]);
    ctx->d_pos[field] = nullptr;
  }
  return e;
}

const uint32_t* mod_of(int field) { return field == ZKMI_FIELD_BLS12_381_FR ? Fr28Params::MOD32 : BnFr28Params::MOD32; }

bool words_lt(const uint32_t* w, const uint32_t* mod) {
  for (int k = 7; k >= 0; k--)
    if (w[k] != mod[k]) return w[k] < mod[k];
  return false;
}

bool tree_ok(const zkmi_ctx* ctx, const zkmi_note_tree* t) { return t && t->ctx == ctx && t->device == ctx->device; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// launch F's instantiation of a kernel template for the tree's field
#define NT_LAUNCH(kernel, field, grid, block, stream, ...)                                                              \
  do {                                                                                                                  \
    if ((field) == ZKMI_FIELD_BLS12_381_FR)                                                                             \
      hipLaunchKernelGGL(kernel<Fr28>, grid, block, 0, stream, __VA_ARGS__,                                             \
                         static_cast<const PoseidonConsts<Fr28>*>(ctx->d_pos[ZKMI_FIELD_BLS12_381_FR]));                \
    else                                                                                                                \
      hipLaunchKernelGGL(kernel<BnFr28>, grid, block, 0, stream, __VA_ARGS__,                                           \
                         static_cast<const PoseidonConsts<BnFr28>*>(ctx->d_pos[ZKMI_FIELD_BN254_FR]));                  \
  } while (0)

// The launches of one append (arguments already checked, leaves canonical): leaves into level 0, the level updates, the
// tail, the per-leaf roots when asked.  The count advances only after the stream has been waited for.
int32_t append_launches(zkmi_ctx* ctx, zkmi_note_tree* t, const void* d_leaves, uint64_t m, uint8_t* out_root, void* d_roots,
                        uint8_t* host_roots) {
  const NoteTreeView& v = t->view;
  const uint64_t n0 = t->n, n_new = n0 + m;
  if (ctx->timer()) ctx->timer()->begin(PH_WITNESS, ctx->stream);
  ZK_HIP(ctx, hipMemcpyAsync(v.node(0, n0), d_leaves, 32 * m, hipMemcpyDeviceToDevice, ctx->stream));
  uint32_t level = 1;
  for (; level <= v.height; level++) {
    const uint64_t lo = n0 >> level, count = ((n_new - 1) >> level) - lo + 1;
    if (count <= NT_BLOCK) break;  // from here on one workgroup covers a level: the tail takes over
    NT_LAUNCH(k_nt_level, t->field, dim3((uint32_t)((count + NT_BLOCK - 1) / NT_BLOCK)), dim3(NT_BLOCK), ctx->stream, v, level, lo,
              count, NoteTreeView::count(n_new, level - 1));
    ZK_HIP(ctx, hipGetLastError());
  }
  // (the root level computes one node, so the loop always leaves at least that level to the tail)
  NT_LAUNCH(k_nt_tail, t->field, dim3(1), dim3(NT_BLOCK), ctx->stream, v, level, n0, n_new);
  ZK_HIP(ctx, hipGetLastError());
  if (d_roots) {
    NT_LAUNCH(k_nt_leaf_roots, t->field, dim3((uint32_t)((m + NT_BLOCK - 1) / NT_BLOCK)), dim3(NT_BLOCK), ctx->stream, v, n0, m,
              static_cast<uint32_t*>(d_roots));
    ZK_HIP(ctx, hipGetLastError());
    if (host_roots) ZK_HIP(ctx, hipMemcpyAsync(host_roots, d_roots, 32 * m, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (ctx->timer()) ctx->timer()->end(PH_WITNESS, ctx->stream);
  if (out_root) ZK_HIP(ctx, hipMemcpyAsync(out_root, v.node(v.height, 0), 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  t->n = n_new;
  return ZKMI_OK;
}

// k paths into device buffers; the indices (host, already checked) travel through d_idx
int32_t paths_launch(zkmi_ctx* ctx, const zkmi_note_tree* t, const uint64_t* leaf_idx, uint32_t k, uint64_t* d_idx, void* d_shape,
                     void* d_paths) {
  ZK_HIP(ctx, hipMemcpyAsync(d_idx, leaf_idx, 8 * (uint64_t)k, hipMemcpyHostToDevice, ctx->stream));
  const uint64_t cnt = (uint64_t)k * t->view.height;
  hipLaunchKernelGGL(k_nt_paths, dim3((uint32_t)((cnt + NT_BLOCK - 1) / NT_BLOCK)), dim3(NT_BLOCK), 0, ctx->stream, t->view, t->n,
                     d_idx, k, static_cast<uint8_t*>(d_shape), static_cast<uint32_t*>(d_paths));
  ZK_HIP(ctx, hipGetLastError());
  return ZKMI_OK;
}

bool indices_ok(const zkmi_note_tree* t, const uint64_t* leaf_idx, uint32_t k) {
  for (uint32_t i = 0; i < k; i++)
    if (leaf_idx[i] >= t->n) return false;
  return true;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int32_t zkmi_note_tree_create(zkmi_ctx* ctx, int32_t field, uint32_t height, uint64_t capacity, zkmi_note_tree** out) {
  if (out) *out = nullptr;
  ZK_ENTER(ctx);
  if (!out || (field != ZKMI_FIELD_BLS12_381_FR && field != ZKMI_FIELD_BN254_FR) || height < 1 || height > ZKMI_MAX_TREE_HEIGHT ||
      capacity < 1 || capacity > (1ull << height))
    return ZKMI_ERR_BAD_ARG;
  zkmi_note_tree* t = new (std::nothrow) zkmi_note_tree();
  if (!t) return ZKMI_ERR_BAD_ARG;
  t->ctx = ctx;
  t->device = ctx->device;
  t->field = field;
  t->capacity = capacity;
  NoteTreeView& v = t->view;
  v.height = height;
  uint64_t nodes = 0;
  for (uint32_t l = 0; l <= ZKMI_MAX_TREE_HEIGHT; l++) {
    v.off[l] = nodes;
    if (l <= height) nodes += NoteTreeView::count(capacity, l);
  }
  v.z_off = nodes;
  nodes += height + 1;
  hipError_t e = ensure_consts(ctx, field);
  if (e == hipSuccess) e = hipMalloc(&t->d_mem, 32 * (nodes + 1));  // + the flag's slot
  if (e != hipSuccess) {
    delete t;
    return ctx->hip_fail(e, "note tree allocation");
  }
  v.base = static_cast<uint32_t*>(t->d_mem);
  t->d_flag = v.base + 8 * nodes;
  NT_LAUNCH(k_nt_zinit, field, dim3(1), dim3(64), ctx->stream, v);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(t->d_mem);
    delete t;
    return ctx->hip_fail(e, "note tree padding table");
  }
  *out = t;
  return ZKMI_OK;
}

int32_t zkmi_note_tree_free(zkmi_note_tree* t) {
  if (!t) return ZKMI_ERR_BAD_ARG;
  (void)hipSetDevice(t->device);
  if (t->d_mem) (void)hipFree(t->d_mem);
  delete t;
  return ZKMI_OK;
}

int32_t zkmi_note_tree_shape(const zkmi_note_tree* t, uint64_t out[3]) {
  if (!t || !out) return ZKMI_ERR_BAD_ARG;
  out[0] = t->view.height;
  out[1] = t->capacity;
  out[2] = t->n;
  return ZKMI_OK;
}

int32_t zkmi_note_tree_root(zkmi_ctx* ctx, const zkmi_note_tree* t, uint8_t out_root[32]) {
  ZK_ENTER(ctx);
  if (!tree_ok(ctx, t) || !out_root) return ZKMI_ERR_BAD_ARG;
  const NoteTreeView& v = t->view;
  const uint32_t* root = t->n ? v.node(v.height, 0) : v.z(v.height);  // the empty tree is all padding
  ZK_HIP(ctx, hipMemcpyAsync(out_root, root, 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int32_t zkmi_note_tree_append(zkmi_ctx* ctx, zkmi_note_tree* t, const uint8_t* leaves, uint64_t m, uint8_t out_root[32],
                              uint8_t* out_roots) {
  ZK_ENTER(ctx);
  if (!tree_ok(ctx, t) || !leaves || m == 0 || m > t->capacity - t->n) return ZKMI_ERR_BAD_ARG;
  const uint32_t* mod = mod_of(t->field);
  for (uint64_t i = 0; i < m; i++) {
    uint32_t w[8];
    memcpy(w, leaves + 32 * i, 32);
    if (!words_lt(w, mod)) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "note tree leaf >= field modulus");
  }
  ZK_HIP(ctx, ctx->staging(32 * m * (out_roots ? 2 : 1)));
  uint8_t* d = static_cast<uint8_t*>(ctx->d_tmp);
  ZK_HIP(ctx, hipMemcpyAsync(d, leaves, 32 * m, hipMemcpyHostToDevice, ctx->stream));
  return append_launches(ctx, t, d, m, out_root, out_roots ? d + 32 * m : nullptr, out_roots);
}

int32_t zkmi_note_tree_append_dev(zkmi_ctx* ctx, zkmi_note_tree* t, const void* d_leaves, uint64_t m, uint8_t out_root[32],
                                  void* d_roots) {
  ZK_ENTER(ctx);
  if (!tree_ok(ctx, t) || !d_leaves || m == 0 || m > t->capacity - t->n || !aligned16(d_leaves) || !aligned16(d_roots))
    return ZKMI_ERR_BAD_ARG;
  // canonicity on the device, before any node is written: one flag, read back
  ModWords mod;
  memcpy(mod.w, mod_of(t->field), 32);
  uint32_t flag = 0;
  ZK_HIP(ctx, hipMemsetAsync(t->d_flag, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_nt_check, dim3((uint32_t)((m + NT_BLOCK - 1) / NT_BLOCK)), dim3(NT_BLOCK), 0, ctx->stream,
                     static_cast<const uint32_t*>(d_leaves), m, mod, t->d_flag);
  ZK_HIP(ctx, hipGetLastError());
  ZK_HIP(ctx, hipMemcpyAsync(&flag, t->d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (flag) return ctx->fail(ZKMI_ERR_NON_CANONICAL, "note tree leaf >= field modulus");
  return append_launches(ctx, t, d_leaves, m, out_root, d_roots, nullptr);
}

int32_t zkmi_note_tree_paths_dev(zkmi_ctx* ctx, const zkmi_note_tree* t, const uint64_t* leaf_idx, uint32_t k, void* d_shape,
                                 void* d_paths) {
  ZK_ENTER(ctx);
  if (!tree_ok(ctx, t) || !leaf_idx || !d_shape || !d_paths || !aligned16(d_paths) || !indices_ok(t, leaf_idx, k))
    return ZKMI_ERR_BAD_ARG;
  if (k == 0) return ZKMI_OK;
  ZK_HIP(ctx, ctx->staging(8 * (uint64_t)k));
  const int32_t rc = paths_launch(ctx, t, leaf_idx, k, static_cast<uint64_t*>(ctx->d_tmp), d_shape, d_paths);
  if (rc != ZKMI_OK) return rc;
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int32_t zkmi_note_tree_paths(zkmi_ctx* ctx, const zkmi_note_tree* t, const uint64_t* leaf_idx, uint32_t k, uint8_t* out_shape,
                             uint8_t* out_paths) {
  ZK_ENTER(ctx);
  if (!tree_ok(ctx, t) || !leaf_idx || !out_shape || !out_paths || !indices_ok(t, leaf_idx, k)) return ZKMI_ERR_BAD_ARG;
  if (k == 0) return ZKMI_OK;
  const uint64_t cnt = (uint64_t)k * t->view.height;
  const uint64_t off_shape = (8 * (uint64_t)k + 255) & ~255ull, off_paths = (off_shape + cnt + 255) & ~255ull;
  ZK_HIP(ctx, ctx->staging(off_paths + 32 * cnt));
  uint8_t* d = static_cast<uint8_t*>(ctx->d_tmp);
  const int32_t rc = paths_launch(ctx, t, leaf_idx, k, reinterpret_cast<uint64_t*>(d), d + off_shape, d + off_paths);
  if (rc != ZKMI_OK) return rc;
  ZK_HIP(ctx, hipMemcpyAsync(out_shape, d + off_shape, cnt, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, hipMemcpyAsync(out_paths, d + off_paths, 32 * cnt, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

}  // extern "C"
