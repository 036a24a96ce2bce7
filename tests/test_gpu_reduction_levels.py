"""The second running-sum level of the bucket reduction (msm_impl.hpp k_segreduce2): shared-bucket plans whose partitions
have at least 256 segments sum 16 consecutive segment sums first and weight the 16 x shorter list by bit decomposition;
below that the single level stays.  Result points must not change: every MSM here is compared with the C++ oracle's bytes.

Which kernels reduce depends on the caller: one MSM by itself takes the quad / octet kernels (single level, whatever the
size), the batch prover the one-lane kernels (the second level).  So the MSM cases run twice -- in this process through the
product library, and in ONE child process through the A/B library with the one-lane kernels selected for single MSMs too
(ZKMI_QUAD = ZKMI_QUAD_G2 = 0: the switches are read once per process) -- and the batch prover runs in this process.
Sizes come from the plan (zkmi_msm_plan_query), never guessed: the largest 2^k with fewer than 256 segments per partition,
the smallest with at least 256 (one super-segment list of 16 entries: tree sums of one slice), and 8 x that, where the job
lists are cut into slices (k_treesum_final) and the second level's lists are shorter than a slice of the first's."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bls12_381 as ec  # noqa: E402
from oracle.bls12_381 import R  # noqa: E402

pytestmark = pytest.mark.gpu
MIN_SEGS = 256  # msm_impl.hpp MSM_SEG2_MIN_SEGS
EXP_LIB = os.path.join(ROOT, "zk-apps_amd", "libzkmi_exp.so")
KINDS = ["uniform", "ones", "top_bucket", "witness_like"]


def frs(vals):
    return b"".join(ec.fr_to_bytes(v) for v in vals)


def segs_per_partition(zk, n):
    c, nd, nwin, nb, seg_log, thr = zk.msm_plan_query(n, shared=True)
    return nb >> seg_log


def sizes_around_the_threshold(zk):
    """{side: n}: largest 2^k below the threshold, smallest 2^k at or above it (k in 5 .. 16), and 8 x the latter"""
    below = [k for k in range(5, 17) if segs_per_partition(zk, 1 << k) < MIN_SEGS]
    above = [k for k in range(5, 17) if segs_per_partition(zk, 1 << k) >= MIN_SEGS]
    assert below and above and max(below) < min(above), (below, above)
    sliced = 8 << min(above)
    assert segs_per_partition(zk, sliced) >= 4 * MIN_SEGS
    return {"below": 1 << max(below), "above": 1 << min(above), "sliced": sliced}


def scalars(zk, kind, n, seed, r=R, top_mask=0x3F):
    """32-byte scalars below r; top_mask keeps the uniform draws below it (0x3F: 2^254 < BLS12-381's r, the default)"""
    assert (top_mask + 1) << 248 <= r
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= top_mask
    if kind == "ones":  # only the bucket of weight 1 is loaded: every other term of the running sums is infinity
        a[:] = 0
        a[:, 0] = 1
    elif kind == "top_bucket":
        # every digit that can be non-zero at its maximum 2^(c-1) (msm_sort.hip: d_w = e_w - (2^(c-1) - 1) over the digits e_w
        # of k + bias, so k = sum_w 2^(c w + c - 1)); the last digit position stays empty where it would pass r
        c, nd = zk.msm_plan_query(n, shared=True)[:2]
        k = 0
        for w in range(nd):
            if k + (1 << (c * w + c - 1)) < r:
                k += 1 << (c * w + c - 1)
        a[:] = np.frombuffer(k.to_bytes(32, "little"), dtype=np.uint8)
    elif kind == "witness_like":  # bench.py's mix: 40 % zero, 20 % one, 10 % below 2^16, 30 % uniform
        u = rng.random(n)
        a[u < 0.4] = 0
        one = (u >= 0.4) & (u < 0.6)
        a[one] = 0
        a[one, 0] = 1
        a[(u >= 0.6) & (u < 0.7), 2:] = 0
    return a.tobytes()


def check_msms(zk, ctx, ocpp, group, n, kinds=KINDS):
    b = ctx.bases_g1_synthetic(n) if group == 1 else ctx.bases_g2_synthetic(n)
    pts = b.read(0, n)
    b.prepare()
    for i, kind in enumerate(kinds):
        sc = scalars(zk, kind, n, 1000 * group + i)
        got = ctx.msm_g1(sc, b) if group == 1 else ctx.msm_g2(sc, b)
        want = ocpp.msm_g1(sc, pts) if group == 1 else ocpp.msm_g2(sc, pts)
        assert got == want, (group, n, kind)
    b.free()


def check_degenerate_msms(ctx, group):
    """The point and scalar patterns of test_gpu_parity.py::test_msm_degenerate_bases_and_scalars at reps 1 (9 points: P + P in
    a light bucket, so the redo pass runs with a non-empty list; P - P; infinity) and 400 (3 600 points per bucket: the heavy
    kernels), against the same closed form over oracle/bls12_381.py."""
    F, G = (ec.Fq, ec.G1) if group == 1 else (ec.Fq2, ec.G2)
    mul = ec.g1_mul if group == 1 else ec.g2_mul
    to_b = ec.g1_to_bytes if group == 1 else ec.g2_to_bytes
    width = 96 if group == 1 else 192
    neg = lambda p: ec.pt_neg(F, p)
    P2, P3 = mul(2), mul(3)
    pts = [G, G, neg(G), G, None, P2, neg(P2), P3, P3]
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890AB % R
    for reps, sc in ((1, [k] * 9), (1, [k, k, k, R - 1, 5, 0, 1, R - 1, R - 1]), (400, [k] * 9)):
        want = None
        for s, p in zip(sc, pts):
            if p is not None and s:
                want = ec.pt_add(F, want, ec.pt_mul(F, p, s))
        want = ec.pt_mul(F, want, reps) if want is not None else None
        raw_b = b"".join(to_b(p) if p is not None else bytes(width) for p in pts * reps)
        b = ctx.bases_g1(raw_b) if group == 1 else ctx.bases_g2(raw_b)
        got = (ctx.msm_g1 if group == 1 else ctx.msm_g2)(frs(sc * reps), b)
        assert got == (to_b(want) if want is not None else bytes(width)), (group, reps, sc[:4])
        b.free()


@pytest.fixture(scope="module")
def ocpp():
    from oracle import cpp

    cpp.build()
    return cpp


@pytest.mark.parametrize("side", ["below", "above", "sliced"])
@pytest.mark.parametrize("group", [1, 2])
def test_prepared_msm_on_both_sides_of_the_threshold_vs_cpp_oracle(ctx, zk, ocpp, group, side):
    check_msms(zk, ctx, ocpp, group, sizes_around_the_threshold(zk)[side])


def test_prepared_msm_through_the_one_lane_reduction_vs_cpp_oracle(zk):
    """The same cases in a child process over the A/B library with ZKMI_QUAD = ZKMI_QUAD_G2 = 0: a single MSM then reduces
    with k_segreduce / k_treesum (G2: the lane-pair forms) and, above the threshold, with the second level.  The child also
    feeds the one-lane and lane-pair k_accum_redo and k_accum_heavy a redo list that is not empty and heavy buckets
    (check_degenerate_msms); a second child adds ZKMI_HEAVY_NC=0, the point mode of k_accum_heavy."""
    assert os.path.exists(EXP_LIB), "zk-apps_amd/libzkmi_exp.so missing: run __graft_entry__.build() (make experiments)"
    for extra in ({}, {"ZKMI_HEAVY_NC": "0"}):
        env = dict(os.environ, ZKMI_LIB=EXP_LIB, ZKMI_QUAD="0", ZKMI_QUAD_G2="0", **extra)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert p.returncode == 0 and "ONE_LANE_MSMS_OK" in p.stdout and "DEGENERATE_MSMS_OK" in p.stdout, (
            extra, p.stdout[-1500:], p.stderr[-3000:])


def test_group_of_three_proofs_with_a_second_level_fold_and_no_fold_vs_cpp_oracle(ctx, zk, ocpp):
    """A group of three proofs at the smallest domain whose prover plans (over the n_vars - 1 assignment terms and over the N
    quotient terms) both have a second level.  The relation z_i * 1 = z_i holds for any assignment, so one key proves a dense
    assignment (the key folds r B1 into the merged L + H reduction: three bucket arrays into one running sum) and
    assignments of bits (after which it stops folding: zkmi_pk_schedule_state) -- byte for byte against the oracle's prover."""
    import random

    import torch

    n_pub = 2
    lg = min(k for k in range(7, 17)
             if segs_per_partition(zk, (1 << k) - n_pub - 1) >= MIN_SEGS and segs_per_partition(zk, 1 << k) >= MIN_SEGS)
    n_vars = (1 << lg) - n_pub
    nc = n_vars - n_pub
    one = (1).to_bytes(32, "little")
    rp, cols = list(range(nc + 1)), list(range(n_pub, n_vars))
    mats = [(rp, cols, one * nc), (rp, [0] * nc, one * nc), (rp, cols, one * nc)]
    r1 = zk.r1cs_create(n_vars, n_pub, mats)
    assert r1.log_n == lg
    rng = ec.SplitMix64(0x2E7E15)
    toxic = frs([rng.fr() for _ in range(5)])
    pk, vk = ctx.groth16_setup(r1, toxic)
    emats = [r1.export(m) for m in range(3)]
    ovk, okey = ocpp.groth16_setup(n_vars, n_pub, nc, lg, emats, toxic)
    assert vk == ovk
    assert pk.schedule_state()[0] is True  # a fresh key folds
    rnd = random.Random(lg)
    G = 3
    dense = [frs([1, 5] + [rnd.randrange(R) for _ in range(n_vars - 2)]) for _ in range(G)]
    bits = [frs([1, 1] + [1 if rnd.random() < 0.6 else 0 for _ in range(n_vars - 2)]) for _ in range(G)]
    seen = []
    for wits, is_dense in ((dense, True), (bits, False), (bits, False), (dense, True)):
        rs = [ec.fr_to_bytes(rng.fr()) for _ in range(G)]
        ss = [ec.fr_to_bytes(rng.fr()) for _ in range(G)]
        want = [ocpp.groth16_prove(n_vars, n_pub, nc, lg, emats, okey, w, r_, s_) for w, r_, s_ in zip(wits, rs, ss)]
        d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
        torch.cuda.synchronize()
        seen.append(pk.schedule_state()[0])  # the route THIS group takes
        assert ctx.groth16_prove_batch_dev(pk, [t.data_ptr() for t in d], rs, ss) == want, (lg, is_dense, seen)
        assert pk.schedule_state()[0] is is_dense
    assert seen == [True, True, False, False]  # both routes were taken, with dense and with sparse assignments
    pk.free()
    r1.free()


if __name__ == "__main__":
    # the child of test_prepared_msm_through_the_one_lane_reduction_vs_cpp_oracle
    from zkmi_loader import load_pkg
    from oracle import cpp

    cpp.build()
    z = load_pkg().Zkmi()
    c = z.context(0)
    sizes = sizes_around_the_threshold(z)
    for grp in (1, 2):
        for size in sizes.values():
            check_msms(z, c, cpp, grp, size)
    print("ONE_LANE_MSMS_OK", sizes)
    for grp in (1, 2):
        check_degenerate_msms(c, grp)
    print("DEGENERATE_MSMS_OK")
    c.close()
