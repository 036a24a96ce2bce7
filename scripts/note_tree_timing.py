#!/usr/bin/env python3
"""The resident Poseidon note tree timed (csrc/note_tree.hip; results in profiles/rNN/note_tree.txt).

    python scripts/note_tree_timing.py             # -> the next profiles/rNN/note_tree.txt
    python scripts/note_tree_timing.py --out FILE  # into FILE

One MI355X, one process, run under a time limit.  Host clock around calls that end in a synchronise; one warm-up of each
call, then the median of 3 (all times stand beside it).

(a) Appends of 2^20, 2^10 and 1 leaves, in this order, into a fresh height-32 tree per repetition (leaves in HBM,
    zkmi_note_tree_append_dev), with and without per-leaf roots, alternated.  The yardstick of the 2^20 append is
    zkmi_poseidon_merkle_tree_dev at log_leaves = 20 over the same leaves: the same 2^20 - 1 hashes; the tree adds the 12
    levels above them, one node each, and the small launches.  Before a time is quoted the tree's root is held to the dense
    root folded with Z_20 .. Z_31 by zkmi_poseidon_hash_batch.
(b) Paths of 2^10 and 2^16 leaves of that tree, into HBM and to the host.
(c) 512 update_note instances, height 10, 2^13: zkmi_update_note_witness_batch_tree_dev beside today's route,
    zkmi_poseidon_merkle_paths_dev -> host -> the structs patched in Python -> zkmi_update_note_witness_batch_dev, over the
    same leaves; the two sets of assignments are compared byte for byte first."""
import ctypes as C
import os
import random
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zkmi_loader import load_pkg  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
REPS = 3


def frs(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def report(name, times, unit_hashes=None):
    med = statistics.median(times)
    tail = "" if not unit_hashes else "   %d hashes, %.1f M hashes/s" % (unit_hashes, unit_hashes / med / 1e3)
    return "%-58s %10.3f ms   (%s)%s" % (name, med, " ".join("%.3f" % t for t in times), tail)


def n_hashes(n0, m, height):
    return sum(((n0 + m - 1) >> l) - (n0 >> l) + 1 for l in range(1, height + 1))


def appends(ctx, torch, out):
    lg, height = 20, 32
    n_big, n_mid = 1 << lg, 1 << 10
    total = n_big + n_mid + 1
    gen = torch.Generator(device="cpu").manual_seed(0x7EE)
    leaves = torch.randint(0, 256, (total, 32), dtype=torch.uint8, generator=gen)
    leaves[:, 31] &= 0x3F  # < 2^254 < r
    d_leaves = leaves.cuda()
    d_roots = torch.zeros((n_big, 32), dtype=torch.uint8, device="cuda")
    nodes = torch.zeros((2 * n_big - 1, 32), dtype=torch.uint8, device="cuda")
    nodes[:n_big] = d_leaves[:n_big]
    torch.cuda.synchronize()
    t_dense = []
    for rep in range(REPS + 1):
        _, ms = timed(lambda: ctx.poseidon_merkle_tree_dev(nodes.data_ptr(), lg))
        if rep:
            t_dense.append(ms)
    # the dense root under the 12 levels of padding above it
    want = bytes(nodes[-1].cpu().numpy().tobytes())
    z = bytes(32)
    for _ in range(lg):
        z = ctx.poseidon_hash_batch(z + z, 1, 2)
    for _ in range(lg, height):
        want = ctx.poseidon_hash_batch(want + z, 1, 2)
        z = ctx.poseidon_hash_batch(z + z, 1, 2)
    t = {(m, r): [] for m in (n_big, n_mid, 1) for r in (False, True)}
    kept = None
    for rep in range(REPS + 1):
        for with_roots in (False, True):
            tree = ctx.note_tree(height, total)
            first = 0
            for m in (n_big, n_mid, 1):
                ptr = d_leaves.data_ptr() + 32 * first
                root, ms = timed(lambda: tree.append_dev(ptr, m, d_roots.data_ptr() if with_roots else None))
                if m == n_big:
                    assert root == want, "the tree's root differs from the dense builder's"
                    if with_roots:
                        torch.cuda.synchronize()
                        assert bytes(d_roots[-1].cpu().numpy().tobytes()) == want
                if rep:
                    t[(m, with_roots)].append(ms)
                first += m
            if rep == REPS and not with_roots:
                kept = tree
            else:
                tree.free()
    out("(a) appends into a height-32 tree (n0 = 0, 2^20, 2^20 + 2^10), leaves in HBM; root == dense root under Z_20..Z_31: True")
    first = 0
    for m in (n_big, n_mid, 1):
        h = n_hashes(first, m, height)
        out("  " + report("append %7d leaves" % m, t[(m, False)], h))
        out("  " + report("append %7d leaves + per-leaf roots" % m, t[(m, True)], h + m * height))
        first += m
    d = statistics.median(t_dense)
    a = statistics.median(t[(n_big, False)])
    out("  " + report("yardstick: zkmi_poseidon_merkle_tree_dev, log_leaves = 20", t_dense, n_big - 1))
    out("  append of 2^20 / dense build of 2^20 = %.3f (%+.3f ms)" % (a / d, a - d))
    return kept, total


def paths(ctx, torch, tree, n_leaves, out):
    out("(b) paths against the current root of that tree (%d leaves, height 32)" % n_leaves)
    rng = random.Random(0xA7)
    for k in (1 << 10, 1 << 16):
        idx = [rng.randrange(n_leaves) for _ in range(k)]
        d_shape = torch.zeros(k * 32, dtype=torch.uint8, device="cuda")
        d_paths = torch.zeros(k * 32 * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # the ctypes index array is made outside the window: the call is what is timed
        arr = (C.c_uint64 * k)(*idx)
        shape_h, paths_h = (C.c_uint8 * (k * 32))(), (C.c_uint8 * (k * 32 * 32))()
        t_dev, t_host = [], []
        for rep in range(REPS + 1):
            _, ms = timed(lambda: ctx._chk(ctx.lib.zkmi_note_tree_paths_dev(ctx.h, tree.h, arr, C.c_uint32(k), C.c_void_p(d_shape.data_ptr()),
                                                                            C.c_void_p(d_paths.data_ptr()))))
            _, ms2 = timed(lambda: ctx._chk(ctx.lib.zkmi_note_tree_paths(ctx.h, tree.h, arr, C.c_uint32(k), shape_h, paths_h)))
            if rep:
                t_dev.append(ms)
                t_host.append(ms2)
        torch.cuda.synchronize()
        assert bytes(d_paths.cpu().numpy().tobytes()) == bytes(paths_h) and bytes(d_shape.cpu().numpy().tobytes()) == bytes(shape_h)
        out("  " + report("paths of %6d leaves into HBM (%d MB)" % (k, k * 32 * 33 >> 20), t_dev))
        out("  " + report("paths of %6d leaves to the host" % k, t_host))


def witness(z, ctx, torch, out):
    n, height, log_n, op_kind = 512, 10, 13, 1
    rng = random.Random(0x512)
    fr = lambda: rng.randrange(R)
    t0, t1 = fr(), fr()
    account = (t0, 900, t1, 40)
    acc_hash = int.from_bytes(ctx.poseidon_hash_batch(frs(account), 1, 4), "little")
    notes = [dict(old=(fr(), fr(), fr()), new=(fr(), fr(), fr()), user=fr(), amount=1 + j % 800) for j in range(n)]
    hashes = ctx.poseidon_hash_batch(b"".join(frs(c["old"] + (acc_hash,)) for c in notes), n, 4)
    where = rng.sample(range(1 << height), n)
    leaves = [fr() for _ in range(1 << height)]
    for j, i in enumerate(where):
        leaves[i] = int.from_bytes(hashes[32 * j : 32 * j + 32], "little")
    blob = frs(leaves)
    tree = ctx.note_tree(height, 1 << height)
    tree.append(blob)
    nodes = torch.zeros(((2 << height) - 1, 32), dtype=torch.uint8, device="cuda")
    nodes[: 1 << height] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).view(-1, 32).cuda()
    torch.cuda.synchronize()
    ctx.poseidon_merkle_tree_dev(nodes.data_ptr(), height)
    assert bytes(nodes[-1].cpu().numpy().tobytes()) == tree.root()
    bufs = [torch.zeros((n, 32 << log_n), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    ptrs = [[b[j].data_ptr() for j in range(n)] for b in bufs]
    blank = [z.note_update(c["amount"], t0, c["user"], c["new"], c["old"], [0] * height, [0] * height, c["user"], account) for c in notes]

    def through_tree():
        return ctx.update_note_witness_batch_tree_dev(log_n, op_kind, blank, tree, where, ptrs[0])

    split = []

    def todays_route():
        (shape, pth), ms_paths = timed(lambda: ctx.poseidon_merkle_paths_dev(nodes.data_ptr(), height, where))

        def patch():
            for j, inp in enumerate(blank_b):
                C.memmove(inp.path_shape, shape[height * j : height * (j + 1)], height)
                C.memmove(inp.path, pth[32 * height * j : 32 * height * (j + 1)], 32 * height)

        _, ms_patch = timed(patch)
        st, ms_wit = timed(lambda: ctx.update_note_witness_batch_dev(log_n, op_kind, blank_b, ptrs[1]))
        split.append((ms_paths, ms_patch, ms_wit))
        return st

    blank_b = [z.note_update(c["amount"], t0, c["user"], c["new"], c["old"], [0] * height, [0] * height, c["user"], account) for c in notes]
    t_tree, t_today = [], []
    for rep in range(REPS + 1):
        st_a, ms_a = timed(through_tree)
        st_b, ms_b = timed(todays_route)
        assert st_a == st_b == [0] * n
        if rep == 0:
            torch.cuda.synchronize()
            assert torch.equal(bufs[0], bufs[1]), "assignments differ between the two routes"
        else:
            t_tree.append(ms_a)
            t_today.append(ms_b)
    out("(c) %d update_note instances, height %d, 2^%d, withdraw; assignments of the two routes byte-equal: True" % (n, height, log_n))
    out("  " + report("zkmi_update_note_witness_batch_tree_dev", t_tree))
    out("  " + report("merkle_paths_dev -> host -> Python structs -> batch_dev", t_today))
    out("    of that: paths to the host %.3f ms | structs patched in Python %.3f ms | zkmi_update_note_witness_batch_dev %.3f ms"
        % tuple(statistics.median(s[k] for s in split[1:]) for k in range(3)))
    tree.free()


def next_profile_dir():
    base = os.path.join(ROOT, "profiles")
    rounds = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(base)) if m]
    return os.path.join(base, "r%02d" % (max(rounds or [0]) + 1))


def main():
    args = sys.argv[1:]
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(next_profile_dir(), "note_tree.txt")
    import torch

    pkg = load_pkg()
    z = pkg.Zkmi()
    ctx = z.context(0)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        out("note tree on %s, library %s; host clock around synchronised calls, median of %d after one warm-up" % (
            z.host_info(), z.version(), REPS))
        tree, n_leaves = appends(ctx, torch, out)
        paths(ctx, torch, tree, n_leaves, out)
        tree.free()
        witness(z, ctx, torch, out)
    ctx.close()


if __name__ == "__main__":
    main()
