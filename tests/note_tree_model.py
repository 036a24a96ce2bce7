"""Model of the resident Poseidon note tree (zkmi_note_tree_*), in Python integers over oracle.poseidon.hash_fix_len: the
shared inputs of tests/test_{cpu,gpu}_note_tree.py.

The rule it restates: a tree of height h holding n leaves is the dense tree over those leaves followed by 2^h - n zero
leaves.  Level l keeps its filled prefix of ceil(n / 2^l) nodes; a node behind it is Z_l, with Z_0 = 0 and
Z_{l+1} = H(Z_l, Z_l); the root of the empty tree is Z_h.  An append recomputes, at level l, the nodes
(n0 >> l) .. ((n0 + m - 1) >> l) and nothing else.

One hash costs about 0.65 ms here, so two-input hashes are remembered per field (the function is pure), and per-leaf
roots, which the model takes by their definition, one single-leaf append each, are for a few leaves at height 32 only.

`python tests/note_tree_model.py` writes tests/golden/note_tree.json."""
import json
import os
import sys
from functools import lru_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import poseidon as ps  # noqa: E402

FIELD_NAMES = {0: "bls12_381_fr", 1: "bn254_fr"}  # ZKMI_FIELD_*
MAX_HEIGHT = 32


def modulus(field):
    return ps.FIELDS[FIELD_NAMES[field]][0]


@lru_cache(maxsize=None)
def hash2(field, left, right):
    return ps.hash_fix_len([left, right], FIELD_NAMES[field])


@lru_cache(maxsize=None)
def zeros(field, height=MAX_HEIGHT):
    """[Z_0 .. Z_height]"""
    z = [0]
    for _ in range(height):
        z.append(hash2(field, z[-1], z[-1]))
    return z


def frs(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def unfrs(b):
    return [int.from_bytes(b[32 * i : 32 * i + 32], "little") for i in range(len(b) // 32)]


def count(n, level):
    """nodes level `level` stores for n leaves"""
    return (n + (1 << level) - 1) >> level


def n_hashes(n0, m, height):
    """hashes of an append of m leaves behind n0"""
    return sum(((n0 + m - 1) >> l) - (n0 >> l) + 1 for l in range(1, height + 1))


class NoteTree:
    def __init__(self, height, field=0, capacity=None):
        assert 1 <= height <= MAX_HEIGHT
        self.height, self.field = height, field
        self.capacity = (1 << height) if capacity is None else capacity
        assert 1 <= self.capacity <= 1 << height
        self.z = zeros(field)[: height + 1]
        self.levels = [[] for _ in range(height + 1)]

    @property
    def n(self):
        return len(self.levels[0])

    def node(self, level, i):
        return self.levels[level][i] if i < len(self.levels[level]) else self.z[level]

    def root(self):
        return self.node(self.height, 0)

    def _append(self, leaves):
        n0, m = self.n, len(leaves)
        self.levels[0].extend(leaves)
        for level in range(1, self.height + 1):
            row = self.levels[level]
            for p in range(n0 >> level, ((n0 + m - 1) >> level) + 1):
                h = hash2(self.field, self.node(level - 1, 2 * p), self.node(level - 1, 2 * p + 1))
                if p < len(row):
                    row[p] = h
                else:
                    assert p == len(row)
                    row.append(h)
            assert len(row) == count(n0 + m, level)

    def append(self, leaves, per_leaf=False):
        """-> (root, [root after each leaf] or None); refused (ValueError, nothing changed) like the library refuses"""
        leaves = list(leaves)
        if not leaves or self.n + len(leaves) > self.capacity:
            raise ValueError("BAD_ARG")
        if any(not 0 <= v < modulus(self.field) for v in leaves):
            raise ValueError("NON_CANONICAL")
        if not per_leaf:
            self._append(leaves)
            return self.root(), None
        roots = []
        for v in leaves:
            self._append([v])
            roots.append(self.root())
        return self.root(), roots

    def path(self, i):
        """(shape, siblings) of leaf i, leaf level first; shape 0 = the sibling is the left input"""
        if not 0 <= i < self.n:
            raise ValueError("BAD_ARG")
        return ([1 - ((i >> level) & 1) for level in range(self.height)],
                [self.node(level, (i >> level) ^ 1) for level in range(self.height)])

    def paths_bytes(self, idx):
        """what zkmi_note_tree_paths returns for idx: (shape bytes, path bytes)"""
        shape, paths = bytearray(), bytearray()
        for i in idx:
            s, p = self.path(i)
            shape += bytes(s)
            paths += frs(p)
        return bytes(shape), bytes(paths)


def golden():
    def record(leaves):
        t = NoteTree(MAX_HEIGHT, 0)
        t.append(leaves)
        shape, path = t.path(4)
        return {"field": FIELD_NAMES[0], "leaves": leaves, "root": hex(t.root()), "leaf": 4, "shape": shape,
                "path": [hex(v) for v in path]}

    return {
        "comment": "tests/note_tree_model.py: Z_0..Z_32 per field (Z_0 = 0, Z_{l+1} = hash_fix_len([Z_l, Z_l])); root and path "
                   "of leaf 4 of the height-32 BLS12-381 Fr tree over the leaves 1..5, and the same once a sixth leaf, 6, "
                   "stands beside leaf 4.  Integers as 0x-prefixed hex.",
        "zeros": {FIELD_NAMES[f]: [hex(v) for v in zeros(f)] for f in (0, 1)},
        "height32_leaves_1_to_5": record([1, 2, 3, 4, 5]),
        "height32_leaves_1_to_6": record([1, 2, 3, 4, 5, 6]),
    }


if __name__ == "__main__":
    with open(os.path.join(ROOT, "tests", "golden", "note_tree.json"), "w") as f:
        json.dump(golden(), f, indent=1)
        f.write("\n")
