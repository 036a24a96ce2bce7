"""The note tree's model (tests/note_tree_model.py) against the oracle's dense tree and path recomputation, the golden
file against the model, and the public surface of the feature.  No GPU."""
import os
import re

import pytest

import note_tree_model as ntm
from conftest import ROOT, golden
from oracle import poseidon as ps

FUNCTIONS = ("zkmi_note_tree_create", "zkmi_note_tree_free", "zkmi_note_tree_shape", "zkmi_note_tree_root", "zkmi_note_tree_append",
             "zkmi_note_tree_append_dev", "zkmi_note_tree_paths", "zkmi_note_tree_paths_dev", "zkmi_update_note_witness_batch_tree_dev")


def _leaves(field, n):
    """distinct, reproducible, canonical; the largest element of the field among them"""
    p = ntm.modulus(field)
    return [p - 1 if i == 2 else (0x9E3779B97F4A7C15 * (i + 1) + (i << 200)) % p for i in range(n)]


@pytest.fixture(scope="module")
def dense():
    """levels of oracle.poseidon.merkle_tree over the first n leaves and 2^h - n zeros, per (field, height, n)"""
    made = {}

    def get(field, height, n):
        key = (field, height, n)
        if key not in made:
            made[key] = ps.merkle_tree(_leaves(field, n) + [0] * ((1 << height) - n), ntm.FIELD_NAMES[field])
        return made[key]

    return get


def _same_as_dense(t, levels):
    n = t.n
    assert t.root() == levels[t.height][0]
    for level in range(t.height + 1):
        assert len(t.levels[level]) == ntm.count(n, level)  # the filled prefix and nothing else
        assert [t.node(level, i) for i in range(len(levels[level]))] == levels[level]  # stored nodes, and Z behind them


@pytest.mark.parametrize("field", [0, 1], ids=["bls12_381_fr", "bn254_fr"])
@pytest.mark.parametrize("height", [1, 2, 3, 4])
def test_model_is_the_dense_tree_over_zero_padded_leaves(dense, field, height):
    """Every (n0, m) with n0 + m <= 2^h: after appending n0 and then m leaves the model holds the dense tree's nodes, every
    per-leaf root of the second append is the dense root of that prefix, and every path recomputes the root."""
    cap = 1 << height
    name = ntm.FIELD_NAMES[field]
    empty = ntm.NoteTree(height, field)
    assert empty.root() == ntm.zeros(field)[height] == dense(field, height, 0)[height][0]
    for n0 in range(cap):
        for m in range(1, cap - n0 + 1):
            leaves = _leaves(field, n0 + m)
            t, u = ntm.NoteTree(height, field), ntm.NoteTree(height, field)
            if n0:
                assert t.append(leaves[:n0])[0] == u.append(leaves[:n0])[0] == dense(field, height, n0)[height][0]
            root, none = t.append(leaves[n0:])
            root_u, roots = u.append(leaves[n0:], per_leaf=True)
            assert none is None and root == root_u == roots[-1]
            assert roots == [dense(field, height, n0 + j + 1)[height][0] for j in range(m)]
            assert t.levels == u.levels
            _same_as_dense(t, dense(field, height, n0 + m))
            for i in range(n0 + m):
                shape, path = t.path(i)
                assert ps.merkle_root(leaves[i], shape, path, name) == root, (n0, m, i)
            # full: the padding is not used any more, and one more leaf is refused
            if n0 + m == cap:
                assert all(len(t.levels[level]) == cap >> level for level in range(height + 1))
                with pytest.raises(ValueError):
                    t.append([1])
                assert t.root() == root


def test_model_refusals_change_nothing():
    t = ntm.NoteTree(3, 0, capacity=5)
    t.append([7, 8, 9])
    before = (t.n, t.root(), t.path(2))
    for bad in ([], [1, 2, 3], [ntm.modulus(0)], [1, ntm.modulus(0)]):
        with pytest.raises(ValueError):
            t.append(bad)
        assert (t.n, t.root(), t.path(2)) == before
    with pytest.raises(ValueError):
        t.path(3)
    assert ntm.n_hashes(0, 8, 3) == 7 and ntm.n_hashes(3, 1, 3) == 3 and ntm.n_hashes(0, 1, 32) == 32


def test_golden_file_is_what_the_model_computes():
    gd = golden("note_tree.json")
    assert gd == ntm.golden()
    z = gd["zeros"]
    assert len(z["bls12_381_fr"]) == len(z["bn254_fr"]) == 33 and z["bls12_381_fr"][0] == z["bn254_fr"][0] == "0x0"
    assert z["bls12_381_fr"][1].startswith("0x306786380fad37d3")
    assert int(z["bls12_381_fr"][1], 16) == ps.hash_fix_len([0, 0])
    assert int(z["bn254_fr"][32], 16) == ps.hash_fix_len([int(z["bn254_fr"][31], 16)] * 2, "bn254_fr")
    g = gd["height32_leaves_1_to_5"]
    assert ps.merkle_root(5, g["shape"], [int(v, 16) for v in g["path"]]) == int(g["root"], 16)
    # leaf 4 = 0b100: a left child twice with padding to its right, then the right child of the node over leaves 0..3
    assert g["shape"] == [1, 1, 0] + [1] * 29
    assert g["path"][:2] == z["bls12_381_fr"][:2] and g["path"][3:] == z["bls12_381_fr"][3:32]
    # a sixth leaf changes the root and nothing of leaf 4's path but its neighbour
    g6 = gd["height32_leaves_1_to_6"]
    assert g6["root"] != g["root"] and g6["shape"] == g["shape"] and g6["path"] == ["0x6"] + g["path"][1:]
    assert ps.merkle_root(5, g6["shape"], [int(v, 16) for v in g6["path"]]) == int(g6["root"], 16)


def test_kernel_allocations():
    """What DESIGN.md 5.10 states about the new kernels, read from the product library's code objects, for both fields: the
    hashing kernels hold the Poseidon state in 50 KB of LDS and at most 168 registers, as k_poseidon_hash does (three
    workgroups of 256 lanes per CU); the level kernel uses no scratch; the copying kernels use neither LDS nor scratch."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    ks = kr.kernels(os.path.join(ROOT, "zk-apps_amd", "libzkmi.so"))
    seen = set()
    for name, k in ks.items():
        short = kr.short_name(name).split("<")[0]
        if short in ("k_nt_level", "k_nt_tail", "k_nt_leaf_roots", "k_nt_zinit"):
            seen.add((short, "Bn" in name))
            assert k["vgpr"] + k["agpr"] <= 168 and k["lds"] == 51200 and k["max_wg"] == 256 and not k["dynamic_stack"], (name, k)
            assert k["scratch"] <= (0 if short in ("k_nt_level", "k_nt_zinit") else 160), (name, k)
        elif short.startswith(("k_nt_paths", "k_nt_check", "k_note_paths_fill")):
            seen.add((short[:10], False))
            assert k["vgpr"] <= 32 and k["lds"] == 0 and k["scratch"] == 0 and not k["dynamic_stack"], (name, k)
    assert len(seen) == 4 * 2 + 3, sorted(seen)


def test_public_surface(zk, pkg):
    """The nine functions are declared in include/zkmi.h, exported by both libraries, bound in integration/ffi.rs and wrapped by
    the binding."""
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    rs = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    assert "typedef struct zkmi_note_tree zkmi_note_tree;" in hdr
    for fn in FUNCTIONS:
        assert re.search(r"\bint32_t %s\s*\(" % fn, hdr), fn
        assert hasattr(zk.lib, fn) and hasattr(zk.tlib, fn), fn
        assert re.search(r"pub fn %s\s*\(" % fn, rs), fn
    for method in ("note_tree", "append", "append_dev", "root", "shape", "paths", "paths_dev", "update_note_witness_batch_tree_dev"):
        assert callable(getattr(pkg.Context, method)), method
    for method in ("append", "append_dev", "root", "shape", "paths", "paths_dev", "free"):
        assert callable(getattr(pkg.NoteTree, method)), method
    # the header states the rule and what a refused call leaves behind
    assert "followed by 2^h - n zero leaves" in hdr and "A refused append changes nothing" in hdr
