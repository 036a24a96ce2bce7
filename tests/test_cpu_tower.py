"""The device pairing tower (zk-apps_amd/csrc/pairing_dev.hip) at its magnitude bounds, without a GPU.

Part 1: where operands may lie.  zkmi_selftest_tower_bounds runs the tower's own templates over intervals from the kernels'
entry conditions; the maxima it records are held to limits DERIVED in DESIGN.md 5.6.1 (not to the comments they replace).
Part 2: every op of zkmi_selftest_tower_ops on the HOST path (Fq2_28: the same templated bodies the lane pairs run) against
the big integers of tests/tower28.py, every operand at the ends of the class interval part 1 reports."""
import numpy as np
import pytest

import limbs28 as lb
import tower28 as tw
from oracle import bls12_381 as ec

F, P = tw.F, tw.P


@pytest.fixture(scope="module")
def classes(zk):
    return tw.bounds(zk)[1]


# ---- part 1: the bounds -------------------------------------------------------------------------------------------------
# DESIGN.md 5.6.1 derives each of these.
BUDGET_LIMIT = F.R // (2 * P)      # 1260: sum |a||b| < R/(2p) keeps T/R inside (-p/2, p/2), the result in (-p/2, 3p/2)
SHRINK_LIMIT = 1 << 14             # |v| < 2^14 p: top limb < 2^31, float and truncation errors of the quotient sum to < 0.03
IS_ZERO_LIMIT = 4                  # is_zero compares with k p, |k| <= 4
STORED_LIMIT = (1 << 31) // 106514  # 20161: the top limb floor(v / 2^364) must fit int32
OPERAND_LIMIT = (1 << 28) // 106514  # 2520: a top limb no larger than a normalised limb, which the column bound assumes


def test_recorded_maxima_stay_below_the_derived_limits(zk):
    sites, classes = tw.bounds(zk)
    print("tower bounds: sites", {k: round(v, 3) for k, v in sites.items()})
    print("tower bounds: classes", classes)
    assert 0 < sites["prod_budget"] < BUDGET_LIMIT
    assert sites["column_log2"] < 63
    assert 0 < sites["prod_operand"] < OPERAND_LIMIT
    assert 0 < sites["shrink_in"] < SHRINK_LIMIT
    assert 0 < sites["is_zero_in"] <= IS_ZERO_LIMIT
    assert sites["stored"] < STORED_LIMIT
    # every figure is an over-estimate of a real run, and none is vacuous: the analysis did reach the deep sites
    assert sites["prod_operand"] >= 16 and sites["shrink_in"] >= 8 and sites["stored"] >= sites["shrink_in"]
    # the classes the kernels' contracts name
    assert classes["F"] == (-2.0, 2.0) and classes["T_XY"] == (-2.0, 2.0) and classes["Q"] == (-0.5, 1.5)
    assert classes["P"] == (-1.5, 1.5) and classes["T_Z"] == (-1.0, 3.0) and classes["WORDS"] == (-2.0, 2.0)
    assert classes["E2_INV"] == (-2.0, 2.0) and max(-classes["SHRINK"][0], classes["SHRINK"][1]) == sites["shrink_in"]
    for name, (lo, hi) in classes.items():
        assert lo < 0 < hi and max(-lo, hi) <= sites["stored"], name


def test_the_montgomery_range_promise_holds_to_the_budget_limit():
    """mont(T) = (T + m p) / R with 0 <= m < R lies in [T/R, T/R + p): inside (-p/2, 3p/2) exactly while |T| < R p / 2.  With
    Field.mont: at the hand-found and the measured budget and at the limit."""
    assert BUDGET_LIMIT == 1260 and F.R * 2 > 2520 * P * 2 and F.R < 2521 * P
    rng = lb.SplitMix64(0xB0D)
    for budget in (203, 457, BUDGET_LIMIT):
        for sign in (1, -1):
            for _ in range(8):
                t = sign * (budget * P * P - rng.below(P))
                v = F.mont(t)
                assert t <= v * F.R < t + P * F.R and -P < 2 * v < 3 * P, (budget, sign)


def test_shrink_to_the_derived_limit_on_the_host(zk):
    """Beyond the tower's own operands (host path only): up to |v| < 2^14 p the float quotient is within one of floor(v / p)
    and the result below 2 p; exact against the single-precision program of tower28.shrink_ref."""
    rng = lb.SplitMix64(0x5121)
    vs = []
    for k in [0, 1, -1, 2, -2, 157, -158, 158, 1023, -1024, 1024, 2521, -2521, (1 << 14) - 1, -(1 << 14)]:
        vs += [k * P, k * P + 1, k * P + P - 1, k * P + rng.below(P)]
    vs += [rng.below(P << 15) - (P << 14) for _ in range(200)]
    # quotients where float32(top limb) / 106513 lands next to an integer: top limb = q * 106513 and its neighbours
    for q in (1, 2, 3, 7, 100, 157, 158, 1000, 16000, -1, -2, -3, -100, -16000):
        for d in (-1, 0, 1):
            vs.append(((q * 106513 + d) << 364) + rng.below(1 << 364))
    vs = [v for v in vs if abs(v) < (P << 14)]
    out = tw.call(zk, None, "shrink", tw.block_of([(v,) for v in vs]))
    got = [r[0] for r in tw.ints_of(out)]
    for v, g in zip(vs, got):
        assert g == tw.shrink_ref(v) and (v - g) % P == 0, v
        assert abs((v - g) // P - v // P) <= 1 and -2 * P < g < 2 * P, v


# ---- part 2: every op against the reference -----------------------------------------------------------------------------
GENERIC = ("shrink", "e2_mul_xi", "e2_conj", "e2_inv", "e6_mul", "e12_sqr", "e12_mul", "e12_mul_line", "e12_conj", "e12_frob_p",
           "e12_frob_p2", "e6_inv", "e12_inv", "words_round_trip")
CAPS = {"e2_inv": 128, "e6_inv": 96, "e12_inv": 96}


def test_vectors_reach_the_ends_of_every_class(classes):
    for op in GENERIC:
        cls = tw.OPS[op]["cls"]
        tuples = tw.generic_tuples(op, classes, CAPS.get(op, 512))
        assert len(tuples) == CAPS.get(op, 512) and len(set(tuples)) > len(tuples) // 2
        for j, c in enumerate(cls):
            lo, hi = tw.span(c, classes)
            col = [t[j] for t in tuples]
            assert min(col) == lo and max(col) == hi, (op, j)
            ks = {v // P for v in col}
            assert {0, -1, 1} <= ks, (op, j)
        assert tuples[0] == tuple(tw.span(c, classes)[1] for c in cls) and tuples[2] == tuple(tw.span(c, classes)[0] for c in cls)


@pytest.mark.parametrize("op", GENERIC)
def test_host_op(zk, classes, op):
    tw.run_generic(zk, None, op, classes, cap=CAPS.get(op, 512))


def test_frobenius_reference_is_the_oracles_power(classes):
    """tower28.frob_ref is linear algebra over the oracle's f12_pow of w; here against f12_pow of the whole element."""
    for t in tw.generic_tuples("e12_frob_p", classes, cap=70)[-2:]:
        x = tw.tower_to_poly(tw.vals(t))
        assert tw.frob_ref(x, 1) == ec.f12_pow(x, P)
        assert tw.frob_ref(x, 2) == ec.f12_pow(x, P * P)
    assert tw.poly_to_tower(tw.tower_to_poly(list(range(1, 13)))) == list(range(1, 13))


@pytest.mark.parametrize("op", ["e12_mul", "e12_inv"])
def test_host_coefficients_that_are_zero_but_held_as_multiples_of_p(zk, classes, op):
    tw.run_generic(zk, None, op, classes, tuples=tw.zero_held_tuples(op, classes))


def test_host_words_of_multiples_of_p(zk, classes):
    tuples = [(k * P + d,) for k in range(-2, 3) for d in (0, 1, -1) if abs(k * P + d) <= 2 * P]
    _, raw = tw.run_generic(zk, None, "words_round_trip", classes, tuples=tuples)
    assert not raw[[i for i, t in enumerate(tuples) if t[0] % P == 0], :12].any()


@pytest.mark.parametrize("op", ["e2_inv", "e6_inv", "e12_inv"])
def test_host_inversions_of_zero_and_one(zk, classes, op):
    tuples = tw.inv_special_tuples(op, classes)
    _, raw = tw.run_generic(zk, None, op, classes, tuples=tuples)
    outs = tw.ints_of(raw)
    assert all(v % P == 0 for v in outs[0] + outs[1] + outs[2])  # 0, p, -p -> 0
    assert tw.vals(outs[3])[0] == 1 and not any(tw.vals(outs[3])[1:])


@pytest.mark.parametrize("op", ["e12_sqr", "e12_inv", "final_exp_chain"])
def test_host_subfield_elements(zk, classes, op):
    tuples = tw.subfield_tuples(classes)
    if op == "final_exp_chain":
        tuples = tuples[::2]
    _, raw = tw.run_generic(zk, None, op, classes, tuples=tuples)
    if op == "final_exp_chain":  # a^(p^6 - 1) = 1 in every proper subfield of even index
        assert all(tw.vals(r) == [1] + [0] * 11 for r in tw.ints_of(raw))


def test_host_is_one(zk, classes):
    tuples, want = tw.is_one_tuples(classes)
    assert sum(want) >= 12 and len(want) - sum(want) >= 100
    got = tw.call(zk, None, "is_one", tw.block_of(tuples), flag=True)
    bad = [(i, int(g), w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]


@pytest.mark.parametrize("op", ["step_tangent", "step_chord"])
def test_host_steps(zk, classes, op):
    tuples = tw.step_tuples(op, classes)
    assert len(tuples) >= 36
    tw.run_generic(zk, None, op, classes, tuples=tuples)


def test_host_miller_rounds(zk, classes):
    tw.run_generic(zk, None, "miller_rounds", classes, tuples=tw.miller_tuples(classes, 4))


def test_host_final_exp_chain(zk, classes):
    tuples = tw.generic_tuples("final_exp_chain", classes, cap=70)
    tw.run_generic(zk, None, "final_exp_chain", classes, tuples=tuples[:4] + tuples[-4:])


def test_bad_arguments(zk):
    import ctypes as C

    block = np.zeros((1, 24 * 14), dtype=np.int32)
    out = np.zeros((1, 12 * 14), dtype=np.int32)
    flag = np.zeros(1, dtype=np.uint8)
    f = zk.tlib.zkmi_selftest_tower_ops
    args = lambda op, n=1, i=block, o=out, fl=flag: (C.c_void_p(None), C.c_int32(op), C.c_uint32(n),
                                                     i.ctypes.data_as(C.c_void_p) if i is not None else None,
                                                     o.ctypes.data_as(C.c_void_p) if o is not None else None,
                                                     fl.ctypes.data_as(C.c_void_p) if fl is not None else None)
    assert f(*args(0)) == 0
    assert f(*args(19)) == -1 and f(*args(-1)) == -1 and f(*args(0, n=0)) == -1 and f(*args(0, i=None)) == -1
    assert f(*args(5, o=None)) == -1 and f(*args(18, fl=None)) == -1 and f(*args(18, o=None)) == 0
    s, c = (C.c_double * 6)(), (C.c_double * 30)()
    g = zk.tlib.zkmi_selftest_tower_bounds
    assert g(s, C.c_uint32(5), c, C.c_uint32(15)) == -1 and g(None, C.c_uint32(6), c, C.c_uint32(15)) == -1
