"""Launch shapes of the MSM driver (csrc/msm_impl.hpp run_device_multi) for two builds of the library, compared kernel by kernel.

  run      a small seeded workload that reaches every branch of the driver's schedule: G1 MSMs plain and prepared with uniform
           and witness-like scalars at 2^12 (small-plan slicing) and 2^16, the 2^24 plan over 2^12 points (partitioned big
           windows: wide heavy tail, two-wave segment sums), a G2 MSM at or below 2^15 buckets and one above, a BN254 MSM, at
           2^13 a single proof (fused four-MSM launch, split2 forms), a grouped batch and a batch of one-proof groups (no-reduce,
           add-at-reduce, third array), and a batch at the smallest domain where the second running-sum level runs.  Prints
           RESULT_DIGEST over every result.  Run it once per build under `rocprofv3 --kernel-trace --output-format csv -d DIR --
           python scripts/launch_shapes.py run` (no counters, no other tracing); ZKMI_LIB selects the library.
  compare A_kernel_trace.csv B_kernel_trace.csv
           per kernel name: the number of launches and the list of (grid, workgroup, LDS) must be equal; per-queue order of
           kernel names is compared where both traces have the same queue ids with the same launch counts, and said not to
           correspond otherwise.  Exit status 1 on a difference in names, counts or shapes.

scripts/trace_timeline.py reads its CSV in a loop inside main(), not in a function: what is shared with it is the kernel-name
shortening (`short`); the rows are read here, with every grid / workgroup / LDS column the trace has."""
import collections
import csv
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trace_timeline import short  # noqa: E402  (the kernel-name shortening of the timeline report)


def read_trace(path):
    """[(queue, kernel name, shape)] in start order; shape = every grid / workgroup / LDS column the trace has."""
    rows = []
    for r in csv.DictReader(open(path)):
        shape = tuple((k, r[k]) for k in sorted(r) if k.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size")))
        rows.append((int(r["Start_Timestamp"]), r.get("Queue_Id", "?"), short(r["Kernel_Name"]), shape))
    rows.sort(key=lambda x: x[0])
    return [x[1:] for x in rows]


def compare(path_a, path_b):
    a, b = read_trace(path_a), read_trace(path_b)
    bad = 0
    shapes = [collections.defaultdict(list), collections.defaultdict(list)]
    for t, rows in zip(shapes, (a, b)):
        for _, name, shape in rows:
            t[name].append(shape)
    print("%d launches of %d kernels in A, %d launches of %d kernels in B" % (len(a), len(shapes[0]), len(b), len(shapes[1])))
    for name in sorted(set(shapes[0]) | set(shapes[1])):
        la, lb = shapes[0].get(name, []), shapes[1].get(name, [])
        if len(la) != len(lb):
            bad += 1
            print("COUNT  %-60s %d vs %d" % (name, len(la), len(lb)))
        elif la != lb and sorted(la) != sorted(lb):
            bad += 1
            print("SHAPE  %-60s %d launches, shapes differ" % (name, len(la)))
        elif la != lb:
            print("order  %-60s same multiset of shapes, other order in time (streams overlap)" % name)
    print("names, counts and shapes equal: %s" % (bad == 0))
    qa, qb = collections.defaultdict(list), collections.defaultdict(list)
    for q, name, _ in a:
        qa[q].append(name)
    for q, name, _ in b:
        qb[q].append(name)
    if sorted(qa) == sorted(qb) and all(len(qa[q]) == len(qb[q]) for q in qa):
        same = [q for q in sorted(qa) if qa[q] == qb[q]]
        print("queues correspond (%s); per-queue order of kernel names equal on %d of %d" % (", ".join(sorted(qa)), len(same), len(qa)))
    else:
        print("queue ids of the two runs do not correspond (A: %s; B: %s): per-queue order not compared"
              % ({q: len(v) for q, v in sorted(qa.items())}, {q: len(v) for q, v in sorted(qb.items())}))
    return 1 if bad else 0


def run():
    import numpy as np
    import torch

    import bench

    z = bench.load_pkg().Zkmi()
    ctx = z.context(0)
    h = hashlib.sha256()
    rng = np.random.default_rng(14)

    def scalars(n, witness_like):
        a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        a[:, 31] &= 0x3F
        if witness_like:
            kind = rng.random(n)
            a[kind < 0.5] = 0
            a[(kind >= 0.3) & (kind < 0.5), 0] = 1
        return a

    def buckets(n):
        c, nd, nwin, nb = z.msm_plan_query(n)[:4]
        return nwin * nb

    for lg in (12, 16):
        n = (1 << lg) - 3
        sc = [scalars(n, False), scalars(n, True)]
        b = ctx.bases_g1_synthetic(n)
        for s_ in sc:
            h.update(ctx.msm_g1(s_.tobytes(), b))
        if lg == 12:
            for s_ in sc:
                d_ = torch.from_numpy(s_).cuda()
                torch.cuda.synchronize()
                h.update(ctx.msm_g1_windows_dev(d_.data_ptr(), n, b, 1 << 24)[0])
        b.prepare()
        for s_ in sc:
            h.update(ctx.msm_g1(s_.tobytes(), b))
        b.free()
    below = max(k for k in range(8, 20) if buckets(1 << k) <= 1 << 15)
    above = min(k for k in range(8, 20) if buckets(1 << k) > 1 << 15)
    for lg in (below, above):
        b = ctx.bases_g2_synthetic(1 << lg)
        h.update(ctx.msm_g2(scalars(1 << lg, True).tobytes(), b))
        b.free()
    b = ctx.bn254_bases_synthetic(1 << 12)
    sc = scalars(1 << 12, False)
    sc[:, 31] &= 0x1F  # below BN254's r (2^253.6)
    h.update(ctx.bn254_msm_g1(sc.tobytes(), b))
    b.free()

    def prove(r1, wits, count, group):
        prng = bench.SplitMix64(r1.log_n)
        toxic = b"".join(prng.fr_bytes() for _ in range(5))
        ctx.set_group_size(group)
        pk, vk = ctx.groth16_setup(r1, toxic)
        ctx.set_group_size(0)
        d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
        rs = [prng.fr_bytes() for _ in range(count)]
        ss = [prng.fr_bytes() for _ in range(count)]
        torch.cuda.synchronize()
        h.update(ctx.groth16_prove_dev(pk, d[0].data_ptr(), rs[0], ss[0]))
        for p in ctx.groth16_prove_batch_dev(pk, [d[i % len(d)].data_ptr() for i in range(count)], rs, ss):
            h.update(p)
        pk.free()

    r1, wits = bench.relation_and_witness(z, "poseidon", 13, [13, 14])
    prove(r1, wits, 9, 0)
    prove(r1, wits, 3, 1)
    r1.free()
    # the smallest domain whose prover plans both have a second level (tests/test_gpu_reduction_levels.py): z_i * 1 = z_i
    n_pub, min_segs = 2, 256
    segs = lambda n: (lambda p: p[3] >> p[4])(z.msm_plan_query(n, shared=True))
    lg = min(k for k in range(7, 17) if segs((1 << k) - n_pub - 1) >= min_segs and segs(1 << k) >= min_segs)
    n_vars = (1 << lg) - n_pub
    nc = n_vars - n_pub
    one = (1).to_bytes(32, "little")
    rp, cols = list(range(nc + 1)), list(range(n_pub, n_vars))
    r1 = z.r1cs_create(n_vars, n_pub, [(rp, cols, one * nc), (rp, [0] * nc, one * nc), (rp, cols, one * nc)])
    dense = scalars(n_vars, False)
    dense[0] = 0
    dense[0, 0] = 1
    prove(r1, [dense.tobytes()], 3, 0)
    r1.free()
    ctx.close()
    print("cases: G1 2^12 / 2^16 plain, prepared, 2^24 plan; G2 2^%d, 2^%d; BN254 2^12; proofs 2^13 single, grouped, one-proof groups; "
          "second level 2^%d" % (below, above, lg))
    print("RESULT_DIGEST", h.hexdigest())


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
