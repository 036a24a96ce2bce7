"""The resident Poseidon note tree (zkmi_note_tree_*, note_tree.hip) against the model of tests/note_tree_model.py, against
the dense builder and the path kernels that predate it, and as the source of the witness generator's Merkle inputs.
Everything is byte for byte; every device output buffer holds 0xA5 first and is checked untouched behind its end."""
import random

import pytest
import torch

import note_tree_model as ntm
import note_update_cases as nc
from conftest import golden

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SLACK = 64  # canary bytes behind every device output
BAD_ARG, NON_CANONICAL = -1, -2


def dev(b):
    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def canary(nbytes):
    t = torch.full((nbytes + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def written(t, nbytes):
    """the first nbytes of a canary buffer; the rest must still be canary"""
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    assert (host[nbytes:] == CANARY).all(), "bytes behind the end of an output buffer were written"
    return host[:nbytes].tobytes()


def untouched(t):
    torch.cuda.synchronize()
    return bool((t.cpu().numpy() == CANARY).all())


def rand_leaves(seed, n, field=0):
    rng = random.Random(seed)
    return [rng.randrange(ntm.modulus(field)) for _ in range(n)]


def refused(pkg, code, call, *args, **kw):
    with pytest.raises(pkg.ZkmiError) as e:
        call(*args, **kw)
    assert e.value.code == code, e.value
    return True


def append_dev(tree, leaves, want_roots=False):
    """through zkmi_note_tree_append_dev: (root, per-leaf roots or None) as integers"""
    m = len(leaves)
    d_leaves = dev(ntm.frs(leaves))
    d_roots = canary(32 * m) if want_roots else None
    root = tree.append_dev(d_leaves.data_ptr(), m, d_roots.data_ptr() if want_roots else None)
    return ntm.unfrs(root)[0], (ntm.unfrs(written(d_roots, 32 * m)) if want_roots else None)


def append_host(tree, leaves, want_roots=False):
    root, roots = tree.append(ntm.frs(leaves), want_roots)
    return ntm.unfrs(root)[0], (ntm.unfrs(roots) if want_roots else None)


def state(tree, leaf):
    return tree.shape(), tree.root(), tree.paths([leaf])


# ---- range arithmetic ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,field", [(1, 0), (2, 0), (3, 0), (4, 0), (3, 1)], ids=["h1", "h2", "h3", "h4", "h3-bn254"])
def test_every_append_range_of_a_small_tree(ctx, pkg, height, field):
    """Every (n0, m) with n0 + m <= 2^h: n0 leaves, then m, into a fresh tree.  The root, the per-leaf roots of the second call and
    the paths of leaves 0, n0 - 1, n0 and n0 + m - 1 are the model's.  The second call alternates between the two append entries.
    At n0 + m = 2^h the padding is not used at the last append any more, and one more leaf is refused."""
    cap = 1 << height
    leaves = rand_leaves(0x7EE0 + 16 * height + field, cap, field)
    leaves[0], leaves[cap - 1] = ntm.modulus(field) - 1, 0
    for n0 in range(cap):
        for m in range(1, cap - n0 + 1):
            what = "n0 = %d, m = %d" % (n0, m)
            model = ntm.NoteTree(height, field)
            tree = ctx.note_tree(height, cap, field)
            assert tree.shape() == (height, cap, 0) and ntm.unfrs(tree.root()) == [model.root()], what
            if n0:
                assert append_host(tree, leaves[:n0])[0] == model.append(leaves[:n0])[0], what
            want_root, want_roots = model.append(leaves[n0 : n0 + m], per_leaf=True)
            got_root, got_roots = (append_dev if (n0 + m) & 1 else append_host)(tree, leaves[n0 : n0 + m], True)
            assert got_root == want_root and got_roots == want_roots, what
            assert tree.shape() == (height, cap, n0 + m) and ntm.unfrs(tree.root()) == [want_root], what
            idx = [i for i in (0, n0 - 1, n0, n0 + m - 1) if i >= 0]
            assert tree.paths(idx) == model.paths_bytes(idx), what
            if n0 + m == cap:
                before = state(tree, cap - 1)
                assert refused(pkg, BAD_ARG, tree.append, ntm.frs([1]))
                assert state(tree, cap - 1) == before
            tree.free()


# ---- against the dense builder on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [0, 1, 255, 256])
def test_height_12_against_the_dense_builder(ctx, n0):
    """The workgroup ends and both sides of the switch between level launches and the tail: root against
    zkmi_poseidon_merkle_tree_dev over the zero-padded leaves, paths of 64 spread leaves against zkmi_poseidon_merkle_paths_dev."""
    lg, cap = 12, 1 << 12
    for m in (1, 255, 256, 257, 511, 513, 1025):
        n = n0 + m
        leaves = ntm.frs(rand_leaves(0xD0 + 4096 * n0 + m, n))
        d_leaves = dev(leaves)
        tree = ctx.note_tree(lg, cap)
        if n0:
            tree.append_dev(d_leaves.data_ptr(), n0)
        root = tree.append_dev(d_leaves.data_ptr() + 32 * n0, m)
        nodes = torch.zeros((2 * cap - 1, 32), dtype=torch.uint8, device="cuda")
        nodes[:n] = d_leaves.view(n, 32)
        torch.cuda.synchronize()
        ctx.poseidon_merkle_tree_dev(nodes.data_ptr(), lg)
        assert root == tree.root() == bytes(nodes[-1].cpu().numpy().tobytes()), (n0, m)
        idx = sorted({(i * n) // 64 for i in range(64)} | {0, n - 1, n0, max(n0 - 1, 0)})
        assert tree.paths(idx) == ctx.poseidon_merkle_paths_dev(nodes.data_ptr(), lg, idx), (n0, m)
        tree.free()


# ---- height 32 -------------------------------------------------------------------------------------------------------------------
def test_height_32_on_one_tree_of_capacity_1000(ctx, pkg):
    """1, 5, 300 and 1 leaves, then up to exactly 1000.  The first six leaves are 1..6: the root after the fifth (a per-leaf root
    of the second append) and, after the sixth, the root and leaf 4's path are the golden file's.  Per-leaf roots are taken for the
    1 + 5 + 1 leaves of the small appends only (the model pays 32 hashes for each)."""
    gd = golden("note_tree.json")
    H = lambda v: int(v, 16)
    rest = rand_leaves(0x32, 994)
    model = ntm.NoteTree(32, 0, capacity=1000)
    tree = ctx.note_tree(32, 1000)
    assert tree.shape() == (32, 1000, 0) and ntm.unfrs(tree.root()) == [model.root()] == [H(gd["zeros"]["bls12_381_fr"][32])]

    assert append_host(tree, [1], True) == model.append([1], per_leaf=True)
    got = append_dev(tree, [2, 3, 4, 5, 6], True)
    assert got == model.append([2, 3, 4, 5, 6], per_leaf=True)
    g5, g6 = gd["height32_leaves_1_to_5"], gd["height32_leaves_1_to_6"]
    assert got[1][3] == H(g5["root"]) and got[0] == H(g6["root"])
    assert tree.paths([4]) == (bytes(g6["shape"]), ntm.frs([H(v) for v in g6["path"]]))

    assert append_dev(tree, rest[:300]) == model.append(rest[:300])
    sample = [0, 4, 5, 6, 255, 256, 305]
    assert tree.paths(sample) == model.paths_bytes(sample)
    assert append_host(tree, rest[300:301], True) == model.append(rest[300:301], per_leaf=True)
    assert tree.shape() == (32, 1000, 307)
    sample = [306, 0, 128, 300]
    assert tree.paths(sample) == model.paths_bytes(sample)

    assert append_dev(tree, rest[301:]) == model.append(rest[301:])
    assert tree.shape() == (32, 1000, 1000) and ntm.unfrs(tree.root()) == [model.root()]
    sample = [999, 998, 0, 511, 512, 767, 768]
    assert tree.paths(sample) == model.paths_bytes(sample)
    before = state(tree, 999)
    assert refused(pkg, BAD_ARG, tree.append, ntm.frs([7]))
    d_one, d_roots = dev(ntm.frs([7])), canary(32)
    assert refused(pkg, BAD_ARG, tree.append_dev, d_one.data_ptr(), 1, d_roots.data_ptr())
    assert untouched(d_roots) and state(tree, 999) == before
    tree.free()


# ---- per-leaf roots --------------------------------------------------------------------------------------------------------------
def test_per_leaf_roots_are_the_roots_of_single_appends(ctx):
    leaves = rand_leaves(0x70, 75)
    batch, single = ctx.note_tree(7, 128), ctx.note_tree(7, 128)
    assert append_host(batch, leaves[:5])[0] == append_host(single, leaves[:5])[0]
    root, roots = append_dev(batch, leaves[5:], True)
    one_by_one = [append_host(single, [v])[0] for v in leaves[5:]]
    assert len(roots) == 70 and roots == one_by_one and roots[-1] == root
    assert batch.root() == single.root() and batch.paths([0, 74]) == single.paths([0, 74])
    batch.free(), single.free()


# ---- paths -----------------------------------------------------------------------------------------------------------------------
def test_paths_recompute_the_root_for_any_list_of_leaves(ctx):
    """Duplicated, unsorted, first and last indices; zkmi_poseidon_merkle_roots_dev over (leaf, shape, path) straight from
    paths_dev gives the tree's root for every queried leaf; the host variant gives the same bytes."""
    height, n = 9, 333
    leaves = rand_leaves(0x9A, n)
    tree = ctx.note_tree(height, 400)
    append_dev(tree, leaves)
    idx = [332, 0, 17, 17, 331, 1, 0, 256, 255, 332, 100]
    k = len(idx)
    d_shape, d_paths = canary(k * height), canary(32 * k * height)
    tree.paths_dev(idx, d_shape.data_ptr(), d_paths.data_ptr())
    shape, paths = written(d_shape, k * height), written(d_paths, 32 * k * height)
    assert (shape, paths) == tree.paths(idx)
    assert shape == bytes(1 - ((i >> lv) & 1) for i in idx for lv in range(height))
    d_leaves, d_roots = dev(ntm.frs([leaves[i] for i in idx])), canary(32 * k)
    ctx.poseidon_merkle_roots_dev(d_leaves.data_ptr(), d_shape.data_ptr(), d_paths.data_ptr(), height, k, d_roots.data_ptr())
    assert written(d_roots, 32 * k) == tree.root() * k
    assert tree.paths([]) == (b"", b"")
    tree.free()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [0, 1], ids=["bls12_381_fr", "bn254_fr"])
def test_refused_calls_leave_the_tree_as_it_was(ctx, pkg, field):
    """Every refusal with its code; afterwards shape, root and a path are unchanged, and a following valid append gives what a
    tree that never saw the refused calls gives."""
    p = ntm.modulus(field)
    first, block = rand_leaves(0xBAD, 20, field), rand_leaves(0xB10C, 130, field)
    tree, twin = ctx.note_tree(8, 151, field), ctx.note_tree(8, 151, field)
    assert append_host(tree, first) == append_host(twin, first)
    before = state(tree, 19)
    m = len(block)
    for pos in (0, 63, 64, m - 1):
        bad = list(block)
        bad[pos] = p
        assert refused(pkg, NON_CANONICAL, tree.append, ntm.frs(bad), True), pos
        d_bad, d_roots = dev(ntm.frs(bad)), canary(32 * m)
        assert refused(pkg, NON_CANONICAL, tree.append_dev, d_bad.data_ptr(), m, d_roots.data_ptr()), pos
        assert untouched(d_roots) and state(tree, 19) == before, pos
    d_block, d_roots = dev(ntm.frs(block + [1, 2])), canary(32 * (m + 2))
    assert refused(pkg, BAD_ARG, tree.append, b"")  # m = 0
    assert refused(pkg, BAD_ARG, tree.append_dev, d_block.data_ptr(), 0, d_roots.data_ptr())
    assert refused(pkg, BAD_ARG, tree.append, ntm.frs(block + [1, 2]))  # 20 + 132 = capacity + 1
    assert refused(pkg, BAD_ARG, tree.append_dev, d_block.data_ptr(), m + 2, d_roots.data_ptr())
    assert refused(pkg, BAD_ARG, tree.paths, [20])  # leaf_idx = n
    assert refused(pkg, BAD_ARG, tree.paths, [3, 20, 4])
    d_shape, d_paths = canary(8), canary(32 * 8)
    assert refused(pkg, BAD_ARG, tree.paths_dev, [20], d_shape.data_ptr(), d_paths.data_ptr())
    assert refused(pkg, BAD_ARG, twin.paths, [1 << 63])
    assert untouched(d_roots) and untouched(d_shape) and untouched(d_paths) and state(tree, 19) == before
    for height, capacity in ((0, 1), (33, 1), (8, 0), (8, 257), (32, (1 << 32) + 1)):
        assert refused(pkg, BAD_ARG, ctx.note_tree, height, capacity, field), (height, capacity)
    assert refused(pkg, BAD_ARG, ctx.note_tree, 8, 8, 2)  # no such field
    assert state(tree, 19) == before
    assert append_dev(tree, block + [1], True) == append_dev(twin, block + [1], True)  # up to the capacity exactly
    assert state(tree, 150) == state(twin, 150) and tree.shape() == (8, 151, 151)
    tree.free(), twin.free()


# ---- the witness generator fed from the tree -------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,log_n", [(10, 13), (32, 14)])
@pytest.mark.parametrize("op_kind", [nc.DEPOSIT, nc.WITHDRAW], ids=["deposit", "withdraw"])
def test_witness_batch_takes_its_paths_from_the_tree(ctx, zk, pkg, op_kind, height, log_n):
    """70 instances (two workgroups of the witness kernel) whose old-note hashes stand among other leaves: the assignments of
    update_note_witness_batch_tree_dev, called with garbage in tree_height / path_shape / path, equal those of
    update_note_witness_batch_dev fed with the tree's paths; public input 4 of each is the tree's root; one of them satisfies the
    relation."""
    n = 70
    rng = random.Random(0x717E + 2 * height + op_kind)
    base = nc.base(op_kind, height, log_n)
    cases = [dict(base, amount=1 + j, old_note=tuple(rng.randrange(nc.R) for _ in range(3)),
                  new_note=tuple(rng.randrange(nc.R) for _ in range(3))) for j in range(n)]
    acc_hash = ntm.unfrs(ctx.poseidon_hash_batch(ntm.frs(base["account"]), 1, 4))[0]
    hashes = ntm.unfrs(ctx.poseidon_hash_batch(b"".join(ntm.frs(c["old_note"] + (acc_hash,)) for c in cases), n, 4))
    leaves = rand_leaves(0x1EAF + height, 300)
    where = [4 * j + 1 for j in range(n)]
    where[0], where[-1] = 0, 299  # the first and the last leaf too
    for j, i in enumerate(where):
        leaves[i] = hashes[j]
    tree = ctx.note_tree(height, 500)
    append_host(tree, leaves[:7])
    append_dev(tree, leaves[7:])
    root = tree.root()

    size = 32 << log_n
    garbage = [nc.to_input(pkg, dict(c, shape=[2] * 32, path=[nc.R + j] * 32)) for j, c in enumerate(cases)]
    for j, g in enumerate(garbage):
        g.tree_height = (j * 7) % 41  # mixed, 0 and beyond the maximum among them
    through_tree = torch.full((n, size + SLACK), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    status = ctx.update_note_witness_batch_tree_dev(log_n, op_kind, garbage, tree, where, [through_tree[j].data_ptr() for j in range(n)])
    assert status == [0] * n

    shape, paths = tree.paths(where)
    fed = []
    for j, c in enumerate(cases):
        s = list(shape[height * j : height * (j + 1)]) + [0] * (32 - height)
        p = ntm.unfrs(paths[32 * height * j : 32 * height * (j + 1)]) + [0] * (32 - height)
        fed.append(nc.to_input(pkg, dict(c, shape=s, path=p)))
    by_hand = torch.full((n, size + SLACK), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.update_note_witness_batch_dev(log_n, op_kind, fed, [by_hand[j].data_ptr() for j in range(n)]) == [0] * n
    torch.cuda.synchronize()
    a, b = through_tree.cpu().numpy(), by_hand.cpu().numpy()
    assert (a[:, size:] == CANARY).all() and (b[:, size:] == CANARY).all()
    differ = [j for j in range(n) if not (a[j] == b[j]).all()]
    assert not differ, "instances %s differ from the ones fed with the tree's paths" % differ
    for j in range(n):
        assert a[j, 32 * 5 : 32 * 6].tobytes() == root, j  # z = (1, amount, token, user, new_note_hash, merkle_root, ...)
    r1 = zk.update_note_r1cs(log_n, op_kind, height)
    assert r1.is_satisfied(a[n - 1, :size].tobytes()) is True
    r1.free()
    tree.free()


def test_witness_batch_refuses_a_bn254_tree_and_a_leaf_behind_the_end(ctx, pkg):
    base = nc.base(nc.WITHDRAW, 10)
    buf = torch.full((32 << 13,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bn = ctx.note_tree(10, 16, field=1)
    append_host(bn, [1, 2, 3])
    assert refused(pkg, BAD_ARG, ctx.update_note_witness_batch_tree_dev, 13, nc.WITHDRAW, [nc.to_input(pkg, base)], bn, [1], [buf.data_ptr()])
    bls = ctx.note_tree(10, 16)
    append_host(bls, [1, 2, 3])
    assert refused(pkg, BAD_ARG, ctx.update_note_witness_batch_tree_dev, 13, nc.WITHDRAW, [nc.to_input(pkg, base)], bls, [3], [buf.data_ptr()])
    assert untouched(buf)
    assert ctx.update_note_witness_batch_tree_dev(13, nc.WITHDRAW, [nc.to_input(pkg, base)], bls, [2], [buf.data_ptr()]) == [0]
    assert not untouched(buf)
    bn.free(), bls.free()
