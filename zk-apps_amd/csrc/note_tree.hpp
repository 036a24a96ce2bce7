// zkmi — the resident Poseidon note tree (include/zkmi.h "note tree"): its handle and the view of it a kernel takes.
//
// A tree of height h holding n leaves is the dense tree of zkmi_poseidon_merkle_tree_dev over those n leaves followed by
// 2^h - n zero leaves.  Level l (0 = leaves, h = root) stores only its filled prefix cnt_l = ceil(n / 2^l) nodes; a node
// at index >= cnt_l is Z_l, with Z_0 = 0 and Z_{l+1} = H(Z_l, Z_l).  Nodes are 32-byte canonical little-endian elements,
// as in the dense tree.  One allocation holds every level (ceil(capacity / 2^l) nodes each), the table Z_0..Z_h and one
// flag word; note_tree.hip owns it, relation.hip reads paths out of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/zkmi.h"

namespace zkmi {

struct NoteTreeView {
  uint32_t* base;                            // node i of the allocation starts at word 8 i
  uint64_t off[ZKMI_MAX_TREE_HEIGHT + 1];    // first node of level l
  uint64_t z_off;                            // first node of the Z table
  uint32_t height;

  __host__ __device__ uint32_t* node(uint32_t level, uint64_t i) const { return base + 8 * (off[level] + i); }
  __host__ __device__ const uint32_t* z(uint32_t level) const { return base + 8 * (z_off + level); }
  // nodes level l stores for n leaves
  __host__ __device__ static uint64_t count(uint64_t n, uint32_t level) { return (n + ((1ull << level) - 1)) >> level; }
  // node i of level l of the tree over n leaves: the stored one, or Z_l behind the filled prefix
  __host__ __device__ const uint32_t* node_or_z(uint64_t n, uint32_t level, uint64_t i) const {
    return i < count(n, level) ? node(level, i) : z(level);
  }
};

}  // namespace zkmi

struct zkmi_note_tree {
  zkmi_ctx* ctx = nullptr;
  int device = 0;
  int32_t field = 0;
  uint64_t capacity = 0, n = 0;
  void* d_mem = nullptr;      // the allocation behind view.base
  uint32_t* d_flag = nullptr;  // the device canonicity check of zkmi_note_tree_append_dev
  zkmi::NoteTreeView view;
};
