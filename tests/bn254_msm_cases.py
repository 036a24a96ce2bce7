"""Inputs and the reference of the BN254 MSM edge tests (test_cpu_bn254_msm.py, test_gpu_bn254_msm.py).  Built from the
oracle (oracle/bn254.py) alone: nothing here calls the library.

THE REFERENCE: the sum of discrete logs.  Every base these tests use is a known multiple of the generator --

    synthetic bases      P_i = [1 + i 0xC0FFEE] G   (zkmi_bn254_bases_synthetic = oracle/bn254.py synthetic_bases)
    a negated base       [-k] G
    a base at infinity   k = 0
    the nine-point pattern of test_msm_degenerate_bases_and_scalars   [1, 1, -1, 1, 0, 2, -2, 3, 3] G

-- so for ANY scalars  sum_i s_i P_i = [sum_i s_i k_i mod r] G : one scalar multiplication by the oracle, exact, and made by
no bucket method.  test_cpu_bn254_msm.py pins this bookkeeping to the oracle's double-and-add sum (bn.msm_naive).

The designed first-pair inputs (design, census, signed_digits, KINDS) are test_first_pair.py's: they are curve-agnostic,
their scalars are below 2^250 < r of BN254."""
import random

import numpy as np

from oracle import bn254 as bn
from test_first_pair import HNC_ENT, HNC_MIN_PL, HNC_POOL, design, materialise

STEP = 0xC0FFEE
NINE = [1, 1, -1, 1, 0, 2, -2, 3, 3]  # G, G, -G, G, infinity, 2G, -2G, 3G, 3G
K = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890AB % bn.R
# the two scalar rows of test_msm_degenerate_bases_and_scalars over BN254's r
NINE_ROWS = [[K] * 9, [K, K, K, bn.R - 1, 5, 0, 1, bn.R - 1, bn.R - 1]]
HEAVY_TAILS = [5 * 64 * HNC_MIN_PL + t for t in (1, 63, 64, 65)]  # test_first_pair.py HEAVY_TAILS, the G1 sizes
TOP_MASK = 0x1F  # 2^253 < r: uniform 32-byte draws with the top byte masked are canonical


def frs(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def unfrs(raw):
    raw = bytes(raw)
    return [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]


def synthetic_logs(n):
    return [1 + i * STEP for i in range(n)]


def point_of_log(k):
    """[k] G for a signed k"""
    pt = bn.pt_mul(bn.G1, abs(k) % bn.R)
    return bn.pt_neg(pt) if k < 0 else pt


def want(scalars, logs):
    """The MSM's wire bytes from the scalars (integers) and the discrete logs of the bases."""
    assert len(scalars) == len(logs)
    return bn.g1_to_bytes(bn.pt_mul(bn.G1, sum(s * k for s, k in zip(scalars, logs)) % bn.R))


def nine_pattern(n):
    """(wire bytes of the bases, their logs): the nine points repeated and cut to n terms"""
    wire = [bn.g1_to_bytes(point_of_log(k)) if k else bytes(64) for k in NINE]
    return b"".join(wire[i % 9] for i in range(n)), [NINE[i % 9] for i in range(n)]


def designed(n, plan):
    """The designed first-pair input of test_first_pair.py for `plan` over the synthetic bases:
    (terms, points [affine or None per term], wire bytes of the bases, wire bytes of the scalars, logs per term)"""
    terms, npts = design(n, plan, bn.R)
    pts = bn.synthetic_bases(npts)
    bases, scalars = materialise(terms, b"".join(bn.g1_to_bytes(p) for p in pts), 64, bn.P, 32)
    logs = [0 if pid is None else (-(1 + pid * STEP) if negated else 1 + pid * STEP) for pid, negated, _ in terms]
    points = [None if pid is None else (bn.pt_neg(pts[pid]) if negated else pts[pid]) for pid, negated, _ in terms]
    return terms, points, bases, scalars, logs


def random_scalars(rnd, n):
    """n canonical scalars from random.Random rnd, as wire bytes (the draw of test_msm_random_sizes_vs_cpp_oracle)"""
    sc = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        sc[i] &= TOP_MASK
    return bytes(sc)


def irregular_sizes():
    """The G1 list of test_msm_random_sizes_vs_cpp_oracle and the generator behind it (for the scalars)"""
    rnd = random.Random(2718)
    sizes = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097] + [rnd.randrange(5, 40000) for _ in range(8)]
    return sizes, rnd


def few_values(n, k, seed):
    """n scalars drawn from k uniform values (thousands of buckets above the heavy threshold), as wire bytes"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    vals[:, 31] &= TOP_MASK
    return vals[rng.integers(0, k, size=n)].tobytes()


def heavy_plan_picks_the_minimum(n, plan_query):
    """test_heavy_bucket_chains_with_every_tail_of_the_last_wave_item's condition on msm_plan_query(n, False): one scalar on n
    bases is a heavy bucket per window, and k_heavy_plan's points per lane stay at the minimum (64 lanes per wave-item)"""
    c, nd, parts, nb, seg_log, heavy_thr = plan_query
    return n > heavy_thr and max(nd, parts) * n <= HNC_MIN_PL * (HNC_POOL - 64 * HNC_ENT)
