"""The reference of the BN254 MSM edge tests (bn254_msm_cases.py: the sum of discrete logs) pinned to the oracle's
double-and-add sum, and the designed first-pair inputs counted against the plans the library picks.  No GPU."""
import pytest

import bn254_msm_cases as cases
from oracle import bn254 as bn
from oracle.bls12_381 import SplitMix64
from test_first_pair import CASES, KINDS, census, plan_of


def wire_points(raw):
    out = []
    for i in range(0, len(raw), 64):
        x, y = int.from_bytes(raw[i : i + 32], "little"), int.from_bytes(raw[i + 32 : i + 64], "little")
        out.append(None if x == 0 and y == 0 else (x, y))
    return out


@pytest.mark.parametrize("shared", [False, True], ids=["windowed", "shared"])
def test_bookkeeping_equals_the_naive_sum_on_a_designed_input(zk, shared):
    """47 designed terms (every kind of bucket three times + a remainder): negated bases, bases at infinity, the borrow of a
    negative digit.  The wire bytes decode to the points the logs describe, and the log sum is the double-and-add sum."""
    n = 3 * len(KINDS) + 5
    terms, points, bases, scalars, logs = cases.designed(n, plan_of(zk, n, shared))
    assert len(terms) == n and any(p is None for p in points) and any(k < 0 for k in logs)
    assert wire_points(bases) == points and all(bn.on_curve(p) for p in points)
    sc = cases.unfrs(scalars)
    assert sc == [s for _, _, s in terms] and all(0 < s < bn.R for s in sc)
    assert cases.want(sc, logs) == bn.g1_to_bytes(bn.msm_naive(sc, points))


def test_bookkeeping_equals_the_naive_sum_on_the_degenerate_pattern():
    """Both scalar rows over the nine points (and the pattern cut inside its second repetition): P + P, P - P, infinity, the
    scalars 0, 1 and r - 1."""
    for n in (9, 13):
        bases, logs = cases.nine_pattern(n)
        points = wire_points(bases)
        assert [p is None for p in points] == [k == 0 for k in logs] and all(bn.on_curve(p) for p in points)
        for row in cases.NINE_ROWS:
            sc = (row * 2)[:n]
            assert cases.want(sc, logs) == bn.g1_to_bytes(bn.msm_naive(sc, points))
    # the first row cancels nothing by accident: the reference is a finite point, and so is the second's
    assert all(cases.want(row, cases.NINE) != bytes(64) for row in cases.NINE_ROWS)


def test_bookkeeping_equals_the_naive_sum_on_seeded_scalars():
    rng = SplitMix64(0xB254ED6E)
    n = 40
    sc = [rng.next() * rng.next() * rng.next() * rng.next() % bn.R for _ in range(n)]
    sc[0], sc[1], sc[2] = 0, 1, bn.R - 1
    assert cases.unfrs(cases.frs(sc)) == sc
    assert cases.want(sc, cases.synthetic_logs(n)) == bn.g1_to_bytes(bn.msm_naive(sc, bn.synthetic_bases(n)))


@pytest.mark.parametrize("shared", [False, True], ids=["windowed", "shared"])
def test_designed_inputs_hit_every_case_in_one_percent_of_the_buckets(zk, shared):
    """test_first_pair.py's condition for the inputs the BN254 GPU test runs: 4 000 terms, the plan the library picks, every
    first-pair case in at least 1 % of ALL its buckets -- with every scalar below BN254's r."""
    n = 4000
    plan = plan_of(zk, n, shared)
    terms, points, bases, scalars, logs = cases.designed(n, plan)
    assert len(terms) == n and len(bases) == 64 * n and len(scalars) == 32 * n
    assert all(0 < s < bn.R for _, _, s in terms)
    got = census(terms, plan)
    print(plan, got)
    for case in CASES:
        assert got[case] * 100 >= plan["buckets"], (case, got, plan)


def test_heavy_tail_sizes_are_heavy_in_the_plan_the_library_picks(zk):
    for n in cases.HEAVY_TAILS:
        assert cases.heavy_plan_picks_the_minimum(n, zk.msm_plan_query(n, False)), n
    assert cases.HEAVY_TAILS == [2561, 2623, 2624, 2625]
