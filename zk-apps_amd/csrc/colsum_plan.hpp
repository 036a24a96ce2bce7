// zkmi — the host plan of the column sums a Groth16 key derivation from a transcript needs (setup_srs.hip):
//   out[j] = sum over the terms of column j of  c * base[sel][point]
// for the columns of sparse matrices given by rows.  Plain C++: no device, no field type -- a coefficient is its canonical
// 8-word value and the modulus is an argument, so a CPU build can include this file.
//
// Every column is cut into work items of at most COLSUM_FAN inputs.  Level-0 items read terms; a level-l item reads the
// contiguous partial sums level l-1 wrote for its column.  The level at which one item remains writes the column's final
// slot.  An item depends on nothing but the output of the launch before it: nothing in the plan waits.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "tune.hpp"

namespace zkmi {

struct ColsumTerm {
  uint32_t point;  // index into the base array
  uint32_t meta;   // bits 0..7 base-array selector, bit 8 negate, bits 16..24 bit length of k (1 .. 255)
  uint32_t k[8];   // min(c, r - c), canonical words
  constexpr uint32_t base() const { return meta & 0xffu; }
  constexpr bool neg() const { return (meta >> 8) & 1u; }
  constexpr uint32_t bits() const { return meta >> 16; }
};
static_assert(sizeof(ColsumTerm) == 40, "term layout");

constexpr uint32_t COLSUM_FINAL = 0x80000000u;  // bit 31 of ColsumItem::out: the slot is a final one (else: a partial of this level)
struct ColsumItem {
  uint32_t out, first, count;  // count in [1, COLSUM_FAN]
};

// one source matrix of a query: CSR by rows, canonical 8-word values, all its terms taken from base array `sel`
struct ColsumSource {
  const uint32_t* rowptr;
  const uint32_t* col;
  const uint32_t* val;  // 8 words per entry
  uint32_t sel;
};

struct ColsumPlan {
  uint32_t n_slots = 0;                         // final slots (variables)
  std::vector<ColsumTerm> terms;                // column after column
  std::vector<std::vector<ColsumItem>> levels;  // levels[0] reads terms
  std::vector<uint32_t> n_partials;             // partial sums level l writes
  std::vector<uint32_t> empty_slots;            // variables no row mentions: infinity
};

namespace colsum_detail {
inline int cmp8(const uint32_t* a, const uint32_t* b) {
  for (int i = 7; i >= 0; i--)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
inline void sub8(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint64_t borrow = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
    out[i] = (uint32_t)d;
    borrow = (d >> 32) & 1u;
  }
}
inline uint32_t bitlen8(const uint32_t* a) {
  for (int i = 7; i >= 0; i--)
    if (a[i]) return 32u * i + (32u - (uint32_t)__builtin_clz(a[i]));
  return 0;
}
}  // namespace colsum_detail

// c (canonical, < r) -> term with k = min(c, r - c); false for c = 0 (the term is dropped)
inline bool colsum_make_term(const uint32_t c[8], const uint32_t r[8], uint32_t point, uint32_t sel, ColsumTerm* t) {
  using namespace colsum_detail;
  if (bitlen8(c) == 0) return false;
  uint32_t n[8];
  sub8(r, c, n);
  const bool neg = cmp8(n, c) < 0;
  memcpy(t->k, neg ? n : c, 32);
  t->point = point;
  t->meta = (sel & 0xffu) | (neg ? 0x100u : 0u) | (bitlen8(t->k) << 16);
  return true;
}

// The plan of one query: `srcs` are merged column by column (source after source, rows ascending within one); variable
// j < n_instance gets one more term per entry of inst_sel: 1 * base[inst_sel][n_rows + j] (the instance rows of the QAP).
inline ColsumPlan colsum_plan(uint32_t n_slots, uint32_t n_rows, const std::vector<ColsumSource>& srcs, uint32_t n_instance,
                              const std::vector<uint32_t>& inst_sel, const uint32_t r[8]) {
  constexpr uint32_t FAN = COLSUM_FAN;
  ColsumPlan p;
  p.n_slots = n_slots;
  // counting sort of the entries (zero coefficients included: they are dropped when the terms are made) by column
  std::vector<uint64_t> start(n_slots + 1, 0);
  for (const ColsumSource& s : srcs)
    for (uint32_t k = 0; k < s.rowptr[n_rows]; k++) start[s.col[k] + 1]++;
  for (uint32_t j = 0; j < n_instance && j < n_slots; j++) start[j + 1] += inst_sel.size();
  for (uint32_t j = 0; j < n_slots; j++) start[j + 1] += start[j];
  struct Entry {
    uint32_t point, sel;
    const uint32_t* val;
  };
  static const uint32_t ONE[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  std::vector<Entry> ent(start[n_slots]);
  {
    std::vector<uint64_t> fill(start.begin(), start.end() - 1);
    for (const ColsumSource& s : srcs)
      for (uint32_t i = 0; i < n_rows; i++)
        for (uint32_t k = s.rowptr[i]; k < s.rowptr[i + 1]; k++) ent[fill[s.col[k]]++] = {i, s.sel, s.val + 8ull * k};
    for (uint32_t j = 0; j < n_instance && j < n_slots; j++)
      for (uint32_t sel : inst_sel) ent[fill[j]++] = {n_rows + j, sel, ONE};
  }
  // terms, column after column; len[j] = live terms of column j
  std::vector<uint32_t> first(n_slots), len(n_slots);
  p.terms.reserve(ent.size());
  for (uint32_t j = 0; j < n_slots; j++) {
    first[j] = (uint32_t)p.terms.size();
    for (uint64_t e = start[j]; e < start[j + 1]; e++) {
      ColsumTerm t;
      if (colsum_make_term(ent[e].val, r, ent[e].point, ent[e].sel, &t)) p.terms.push_back(t);
    }
    len[j] = (uint32_t)p.terms.size() - first[j];
    if (!len[j]) p.empty_slots.push_back(j);
  }
  // levels: a column with `len` inputs left becomes ceil(len / FAN) items; one item -> the final slot
  for (bool more = true; more;) {
    more = false;
    std::vector<ColsumItem> items;
    uint32_t written = 0;
    for (uint32_t j = 0; j < n_slots; j++) {
      if (!len[j]) continue;
      const uint32_t cnt = (len[j] + FAN - 1) / FAN;
      const uint32_t out0 = written;
      for (uint32_t q = 0; q < cnt; q++) {
        const uint32_t c = len[j] - q * FAN < FAN ? len[j] - q * FAN : FAN;
        items.push_back({cnt == 1 ? (COLSUM_FINAL | j) : written++, first[j] + q * FAN, c});
      }
      if (cnt == 1) {
        len[j] = 0;  // finished
      } else {
        first[j] = out0;
        len[j] = cnt;
        more = true;
      }
    }
    if (items.empty()) break;
    p.levels.push_back(std::move(items));
    p.n_partials.push_back(written);
  }
  return p;
}

}  // namespace zkmi
