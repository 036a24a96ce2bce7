"""The BN254 G1 MSM (csrc/msm_bn.hip: every kernel of msm_impl.hpp, msm_quad.hpp and quad.hpp compiled for the 10-limb field)
held to the edge cases the BLS12-381 MSM is held to: first-pair cases in 1 % of the buckets, heavy buckets with every tail
of the last wave-item, degenerate bases up to 54 000 per bucket, witness-like scalars, irregular sizes, digits at their
maximum, the second reduction level, the two-level record sort and the 20-bit plan.

Every result is compared byte for byte with the sum of discrete logs (bn254_msm_cases.py): one scalar multiplication by
oracle/bn254.py, made by no bucket method; test_cpu_bn254_msm.py pins it to the oracle's double-and-add sum.  No tolerances.

The product library runs the quad kernels and 16-bit windows below 2^24 terms; test_the_one_lane_kernels_and_the_big_plan_
at_small_sizes sends the same inputs through the one-lane reduction, the point mode of the heavy kernel and the 20-bit plan
in child processes over the A/B library (its switches are read once per process)."""
import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bn254_msm_cases as cases  # noqa: E402
from oracle import bn254 as bn  # noqa: E402
from test_first_pair import CASES, census, plan_of  # noqa: E402
from test_gpu_reduction_levels import scalars as kind_scalars, sizes_around_the_threshold  # noqa: E402

pytestmark = pytest.mark.gpu
EXP_LIB = os.path.join(ROOT, "zk-apps_amd", "libzkmi_exp.so")


def bn_scalars(zk, kind, n, seed):
    return kind_scalars(zk, kind, n, seed, r=bn.R, top_mask=cases.TOP_MASK)


def check(ctx, sc, b, want, tag, plain=True, prepared=True):
    """The MSM over b's bases as they are and over the prepared ones (b is prepared on the way) against the reference bytes."""
    if plain:
        got = ctx.bn254_msm_g1(sc, b)
        assert got == want, (tag, "plain", got.hex(), want.hex())
    if prepared:
        b.prepare()
        got = ctx.bn254_msm_g1(sc, b)
        assert got == want, (tag, "prepared", got.hex(), want.hex())


def check_synthetic(ctx, sc, n, tag, **kw):
    b = ctx.bn254_bases_synthetic(n)
    check(ctx, sc, b, cases.want(cases.unfrs(sc), cases.synthetic_logs(n)), tag, **kw)
    b.free()


def check_first_pair(zk, ctx, n, shared):
    plan = plan_of(zk, n, shared)
    terms, points, bases, sc, logs = cases.designed(n, plan)
    got = census(terms, plan)
    assert all(got[case] * 100 >= plan["buckets"] for case in CASES), (got, plan)
    b = ctx.bn254_bases(bases)
    check(ctx, sc, b, cases.want([s for _, _, s in terms], logs), ("first pair", n, plan), plain=not shared, prepared=shared)
    b.free()


def check_heavy_tail(zk, ctx, n, distinct):
    """One scalar on n bases: a heavy bucket of n entries per window (plain) / one of n entries per digit value (prepared)."""
    sc = cases.frs([cases.K]) * n
    if distinct:
        check_synthetic(ctx, sc, n, ("heavy tail, distinct bases", n))
    else:
        bases, logs = cases.nine_pattern(n)
        b = ctx.bn254_bases(bases)
        check(ctx, sc, b, cases.want([cases.K] * n, logs), ("heavy tail, nine-point pattern", n))
        b.free()


def check_degenerate(ctx, reps, prepared):
    """Both scalar rows over the nine-point pattern repeated reps times, over the bases as given and then over prepared ones."""
    bases, _ = cases.nine_pattern(9 * reps)
    b = ctx.bn254_bases(bases)
    for over_prepared in (False, True) if prepared else (False,):
        for row in cases.NINE_ROWS:
            want = cases.want([s * reps % bn.R for s in row], cases.NINE)
            assert want != bytes(64)
            check(ctx, cases.frs(row * reps), b, want, ("degenerate", reps, row[3:5]), plain=not over_prepared, prepared=over_prepared)
    b.free()


@pytest.mark.parametrize("shared", [False, True], ids=["windowed", "prepared"])
def test_first_pair_cases(zk, ctx, shared):
    """madd_affine_pair<BnFq28> on P + P, P - P (redo list), a base at infinity beside one or two entries, buckets of one and of
    two entries, with every combination of digit sign and stored sign: 4 000 designed terms, each case in >= 1 % of the buckets."""
    check_first_pair(zk, ctx, 4000, shared)


@pytest.mark.parametrize("distinct", [False, True], ids=["nine_points", "distinct_bases"])
@pytest.mark.parametrize("n", cases.HEAVY_TAILS)
def test_heavy_bucket_chains_with_every_tail_of_the_last_wave_item(zk, ctx, n, distinct):
    """k_accum_heavy_nc<BnFq28, 3>: five full wave-items and a last one of 1 / 63 / 64 / 65 entries, so the lanes whose entry
    count differs by one sit in that item.  With the nine-point pattern the lanes meet infinity, P + P and P - P in the pair
    step; with n DISTINCT bases the reference is K x the sum of their logs, which a skipped, repeated or stale table entry
    cannot leave unchanged -- and no lane meets P + P there, so no partial sum is a marker that k_accum_heavy recomputes
    from its points with the complete law (a pattern whose period divides 64 gives every lane ONE point over and over: all
    markers, and the chain under test never adds).  Plain and prepared (there a heavy bucket holds n entries per digit
    value: another tail)."""
    assert cases.heavy_plan_picks_the_minimum(n, zk.msm_plan_query(n, False)), zk.msm_plan_query(n, False)
    check_heavy_tail(zk, ctx, n, distinct)


@pytest.mark.parametrize("reps", [1, 400, 6000])
def test_degenerate_bases_and_scalars(ctx, reps):
    """test_msm_degenerate_bases_and_scalars over BN254: G, G, -G, G, infinity, 2G, -2G, 3G, 3G with one scalar on all and with
    K, K, K, r - 1, 5, 0, 1, r - 1, r - 1; 9 points (light buckets, a redo list that is not empty), 3 600 and 54 000 per bucket
    (several wave-items per heavy bucket, marked partial sums, split buckets and tickets); at 6 000 also over prepared bases."""
    check_degenerate(ctx, reps, prepared=reps >= 6000)


@pytest.mark.parametrize("n", [5000, 70000])
def test_witness_like_scalars(zk, ctx, n):
    """bench.py's mix (40 % zero, 20 % one, 10 % below 2^16, 30 % uniform) -- the columns a halo2 prover commits: heavy buckets
    of distinct points beside light ones, plain and prepared."""
    check_synthetic(ctx, bn_scalars(zk, "witness_like", n, 254 + n), n, ("witness-like", n))


@functools.lru_cache(maxsize=None)
def irregular_cases():
    """[(n, scalars, reference)] for the G1 size list of test_msm_random_sizes_vs_cpp_oracle, computed once"""
    sizes, rnd = cases.irregular_sizes()
    logs = cases.synthetic_logs(max(sizes))
    out = []
    for n in sizes:
        sc = cases.random_scalars(rnd, n)
        out.append((n, sc, cases.want(cases.unfrs(sc), logs[:n])))
    return out


def test_irregular_sizes(ctx):
    """1 ... 40 000, powers of two and their neighbours: every plan boundary of the windowed schedule, over a prefix of one
    base set."""
    todo = irregular_cases()
    b = ctx.bn254_bases_synthetic(max(n for n, _, _ in todo))
    for n, sc, want in todo:
        got = ctx.bn254_msm_g1(sc, b)
        assert got == want, (n, got.hex(), want.hex())
    b.free()


def test_irregular_sizes_over_prepared_bases(ctx):
    """The sizes up to 4 097 once more, each over a prepared base set of exactly its length (the shared-bucket plans)."""
    for n, sc, want in irregular_cases():
        if n <= 4097:
            b = ctx.bn254_bases_synthetic(n)
            check(ctx, sc, b, want, ("irregular", n), plain=False)
            b.free()


def check_threshold_kinds(zk, ctx, n, kinds, plain):
    b = ctx.bn254_bases_synthetic(n)
    logs = cases.synthetic_logs(n)
    b.prepare()
    for i, kind in enumerate(kinds):
        sc = bn_scalars(zk, kind, n, 2540 + i)
        want = cases.want(cases.unfrs(sc), logs)
        got = ctx.bn254_msm_g1(sc, b)
        assert got == want, (kind, n, "prepared", got.hex(), want.hex())
        if plain:  # fewer scalars than bases: the windowed schedule
            got = ctx.bn254_msm_g1(sc[: 32 * (n - 1)], b)
            want = cases.want(cases.unfrs(sc)[: n - 1], logs[: n - 1])
            assert got == want, (kind, n, "windowed", got.hex(), want.hex())
    b.free()


@pytest.mark.parametrize("side", ["below", "above"])
def test_digits_at_their_maximum_and_the_ones_vector(zk, ctx, side):
    """Prepared bases on both sides of the second-level threshold (test_gpu_reduction_levels.py): every digit below r at its
    maximum 2^(c-1) (the last bucket of every partition, the carry into the next digit), all scalars one (a single loaded
    bucket: every other term of the running sums is infinity), and the witness-like mix."""
    check_threshold_kinds(zk, ctx, sizes_around_the_threshold(zk)[side], ["top_bucket", "ones", "witness_like"], plain=True)


def torch_scalars(n, seed, witness_like):
    """n canonical scalars (< 2^253) generated in HBM and the closed form's log: sum s_i (1 + i STEP) mod r."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= cases.TOP_MASK
    if witness_like:
        kind = torch.rand(n, device="cuda", generator=g)
        raw[kind < 0.6] = 0
        raw[(kind >= 0.4) & (kind < 0.6), 0] = 1
        raw[(kind >= 0.6) & (kind < 0.7), 2:] = 0
        del kind
    s0, s1 = [0] * 32, [0] * 32
    for lo in range(0, n, 1 << 22):  # (byte sums below 2^56 per column; a slice at a time bounds the 64-bit copies)
        part = raw[lo : lo + (1 << 22)].to(torch.int64)
        idx = torch.arange(lo, lo + part.shape[0], dtype=torch.int64, device="cuda")
        s0 = [a + b for a, b in zip(s0, part.sum(dim=0).cpu().tolist())]
        s1 = [a + b for a, b in zip(s1, (part * idx[:, None]).sum(dim=0).cpu().tolist())]
        del part, idx
    tot = sum(v << (8 * k) for k, v in enumerate(s0))
    wtot = sum(v << (8 * k) for k, v in enumerate(s1))
    torch.cuda.synchronize()
    return raw, bn.g1_to_bytes(bn.pt_mul(bn.G1, (tot + cases.STEP * wtot) % bn.R))


def test_two_level_sort_of_16_bit_windows(zk, ctx):
    """n = 2^21 + 4097: the record sort of the big plans over 254-bit scalars (top window one bit shorter than over BLS12-381's
    Fr), uniform scalars and the witness-like mix (420 000 records in one bucket), against the closed form."""
    import torch

    n = (1 << 21) + 4097
    assert zk.msm_plan_query(n)[0] == 16 and zk.msm_plan_query((1 << 21) - 1)[0] == 16
    b = ctx.bn254_bases_synthetic(n)
    for witness_like in (False, True):
        raw, want = torch_scalars(n, 2121 + witness_like, witness_like)
        got = ctx.bn254_msm_g1_dev(raw.data_ptr(), n, b)
        assert got == want, (witness_like, got.hex(), want.hex())
        del raw
    b.free()
    torch.cuda.empty_cache()


def test_20_bit_plan_in_the_product(zk, ctx):
    """2^24 is the smallest n at which the product library picks 20-bit windows: run_windowed_big over BN254 scalars, the one-lane
    k_segreduce / k_treesum / k_treesum_final<BnFq28>, and -- a fifth of the scalars equal one -- the complete-law heavy
    kernel (the call-free one is off for wide plans).  The one large test of this file."""
    import torch

    n = 1 << 24
    assert zk.msm_plan_query(n)[0] == 20 and zk.msm_plan_query(n - 1)[0] == 16
    raw, want = torch_scalars(n, 2424, True)
    b = ctx.bn254_bases_synthetic(n)
    got = ctx.bn254_msm_g1_dev(raw.data_ptr(), n, b)
    b.free()
    del raw
    torch.cuda.empty_cache()
    assert got == want, (got.hex(), want.hex())


CHILDREN = [
    # (mode, switches of the A/B library, token, seconds: a process start, a context and a few dozen small MSMs)
    ("one_lane", {"ZKMI_QUAD": "0"}, "BN254_ONE_LANE_OK", 300),
    ("point_mode", {"ZKMI_QUAD": "0", "ZKMI_HEAVY_NC": "0"}, "BN254_POINT_MODE_OK", 300),
    ("big_plan", {"ZKMI_WINDOW_BITS": "20"}, "BN254_BIG_PLAN_OK", 300),
]


def test_the_one_lane_kernels_and_the_big_plan_at_small_sizes(zk):
    """Three child processes over the A/B library:
    ZKMI_QUAD=0                    k_segreduce, k_treesum and the second level for BnFq28 (threshold sizes, prepared, four
                                   scalar kinds); the one-lane k_accum_redo and k_accum_heavy (degenerate pattern, reps 1, 400)
    ZKMI_QUAD=0 ZKMI_HEAVY_NC=0    the point mode of k_accum_heavy (degenerate pattern, heavy tails)
    ZKMI_WINDOW_BITS=20            the 20-bit plan on 2^17 terms: uniform, witness-like, scalars drawn from 600 values"""
    assert os.path.exists(EXP_LIB), "zk-apps_amd/libzkmi_exp.so missing: run __graft_entry__.build() (make experiments)"
    for mode, switches, token, seconds in CHILDREN:
        env = dict(os.environ, ZKMI_LIB=EXP_LIB, **switches)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=seconds, cwd=ROOT, env=env)
        assert p.returncode == 0 and token in p.stdout, (mode, switches, p.stdout[-1500:], p.stderr[-3000:])


def child(mode):
    from zkmi_loader import load_pkg

    z = load_pkg().Zkmi()
    c = z.context(0)
    if mode == "one_lane":
        sizes = sizes_around_the_threshold(z)
        for n in sizes.values():
            check_threshold_kinds(z, c, n, ["uniform", "ones", "top_bucket", "witness_like"], plain=False)
        for reps in (1, 400):
            check_degenerate(c, reps, prepared=False)
        print("BN254_ONE_LANE_OK", sizes)
    elif mode == "point_mode":
        for reps in (1, 400):
            check_degenerate(c, reps, prepared=False)
        for n in cases.HEAVY_TAILS:
            for distinct in (False, True):
                check_heavy_tail(z, c, n, distinct)
        print("BN254_POINT_MODE_OK")
    elif mode == "big_plan":
        n = 1 << 17
        assert z.msm_plan_query(n)[0] == 20, z.msm_plan_query(n)
        for name, sc in (("uniform", bn_scalars(z, "uniform", n, 77)), ("witness-like", bn_scalars(z, "witness_like", n, 78)),
                         ("600 values", cases.few_values(n, 600, 79))):
            check_synthetic(c, sc, n, ("20-bit plan", name), prepared=False)
        print("BN254_BIG_PLAN_OK", z.msm_plan_query(n))
    else:
        raise SystemExit("unknown mode " + mode)
    c.close()


if __name__ == "__main__":
    child(sys.argv[1])
