"""The digit sort's model and its designed inputs, without a GPU (tests/sort_model.py, tests/sort_cases.py).

The census is the check that matters: from the model alone every named vector must produce the loads, partition totals, run
positions and oversized counts its name promises, under the plan the library's planners return today and around the constants
zkmi_selftest_msm_sort_shape returns -- so that a planner change that moves a threshold fails HERE, and test_gpu_msm_sort.py
never goes quietly vacuous."""
import ctypes as C
import random

import numpy as np
import pytest

import sort_cases as sc_
import sort_model as sm
from oracle.bls12_381 import R

# every digit width a planner can return: pick_window's, the shared plan's candidates (6 .. 22), the big plans' (17 .. 22)
WIDTHS = sorted(set([5, 8, 10, 13, 16, 20]) | set(range(6, 23)))


@pytest.fixture(scope="module")
def shape(zk):
    return zk.selftest_msm_sort_shape()


def test_shape_constants_are_the_ones_the_cases_stand_on(shape):
    assert len(shape) == 13
    assert shape["FSORT_RPT"] * 1024 == shape["FINE_STAGE"] > shape["FINE_ROUND"] > 0
    assert shape["BIG_THR"] > shape["FINE_STAGE"] and shape["BIG_MAX"] > 0 and shape["SPLIT_B"] % 1024 == 0
    assert shape["WRITE_BATCH"] == 1024 and 1 << shape["FINE_LOG"] == 1024


@pytest.mark.parametrize("c", WIDTHS)
def test_recoding_identity(c):
    npos = 255 // c + 1
    rnd = random.Random(c)
    vals = [rnd.randrange(R) for _ in range(300)] + [0, 1, R - 1, R - 2, (1 << 254) - 1, 1 << 254]
    vals += [(1 << (c * w)) * m % R for w in range(npos) for m in (1, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1)]
    d = sm.recode(sm.scalars_from_ints(vals), c, npos)
    lo, hi = -((1 << (c - 1)) - 1), 1 << (c - 1)
    assert d.min() >= lo and d.max() <= hi
    for v, row in zip(vals, d):
        assert sum(int(x) << (c * w) for w, x in enumerate(row)) == v
    assert sm.scalars_to_ints(sm.scalars_from_ints(vals)) == vals


def _plan(c, shared, n, nwin=None, nb=None, tsl=0, vec_parts=1):
    return {"c": c, "nwin": nwin if nwin else 255 // c + 1, "nb": nb if nb else 1 << (c - 1), "ndigits": 255 // c + 1 if shared else 0,
            "shared": int(shared), "vec_parts": vec_parts, "heavy_thr": 256, "heavy_shift": 0, "top_spread_log": tsl, "n": n}


def test_bucket_and_entry_conventions_on_hand_computed_scalars():
    S = 0x80000000
    # windowed, c = 10 (512 buckets per window): 5 = digit +5 at 0; 2^10 - 5 = digit -5 at 0 and +1 at 1; 2^9 = the digit +2^(c-1);
    # 2^9 + 1 = 2^10 - 511: digit -511 at 0 and +1 at 1
    sc = sm.scalars_from_ints([5, (1 << 10) - 5, 0, 7 << 20, 1 << 9, (1 << 9) + 1])
    bk, en = sm.records(_plan(10, False, 6), sc)
    got = sorted(zip(bk.tolist(), en.tolist()))
    assert got == sorted([(4, 0), (4, 1 | S), (512 + 0, 1), (2 * 512 + 6, 3), (511, 4), (510, 5 | S), (512, 5)])
    # shared, c = 10, one bucket set of 512, n = 6: the entry is the table index w n + i
    bk, en = sm.records(_plan(10, True, 6, nwin=1), sc)
    assert sorted(zip(bk.tolist(), en.tolist())) == sorted([(4, 0), (4, 1 | S), (0, 6 + 1), (6, 12 + 3), (511, 4), (510, 5 | S), (0, 6 + 5)])
    # batch of 2 vectors x 3 scalars: vector 1's buckets behind vector 0's, indices per vector
    bk, en = sm.records(_plan(10, True, 3, nwin=2, vec_parts=1), sc, batch=2)
    assert sorted(zip(bk.tolist(), en.tolist())) == sorted([(4, 0), (4, 1 | S), (0, 3 + 1), (512 + 6, 6 + 0), (512 + 511, 1), (512 + 510, 2 | S),
                                                            (512 + 0, 3 + 2)])
    # c = 20, top window (position 12) spread over 16 groups of 2^15 by point index: scalar i = 3 with top digit +9
    sc = sm.scalars_from_ints([0, 0, 0, (9 << 240) + (6 << 20), (9 << 240)])
    bk, en = sm.records(_plan(20, False, 5, tsl=4), sc)
    assert sorted(zip(bk.tolist(), en.tolist())) == sorted([(12 * (1 << 19) + 3 * 32768 + 8, 3), ((1 << 19) + 5, 3), (12 * (1 << 19) + 4 * 32768 + 8, 4)])


def test_check_refuses_what_it_should(zk):
    """the checker on a sort made by numpy -- and on the same sort with one word wrong in each array"""
    plan = dict(_plan(10, False, 3000), heavy_thr=48)
    sc = sm.dense(3000, R, 5)
    sc[:200] = sm.scalars_from_ints([77 << 30] * 200)  # one heavy bucket
    good = _numpy_sort(plan, sc)
    sm.check(*good)
    for which, pos in ((2, 0), (3, 5), (4, 7), (5, 0), (5, -1), (6, 1)):
        bad = [a.copy() if isinstance(a, np.ndarray) else a for a in good]
        if which == 5 and pos == 0:  # swap a loaded bucket's slot with the slot of a lighter one: the key increases
            bad[5][[0, 1000]] = bad[5][[1000, 0]]
            assert good[2][good[5][0]] != good[2][good[5][1000]]
        else:
            bad[which][pos] ^= 1
        with pytest.raises(AssertionError):
            sm.check(*bad)


def test_check_refuses_a_heavy_list_that_takes_the_threshold_itself(zk):
    """`>` written `>=` in the ordering key (msm_sort.hip order_key), on the vector with a bucket of exactly heavy_thr entries"""
    case = sc_.get("windowed_heavy_edge", zk)
    sm.check(*_numpy_sort(case["plan"], case["sc"]))
    with pytest.raises(AssertionError):
        sm.check(*_numpy_sort(case["plan"], case["sc"], heavy_from=case["plan"]["heavy_thr"]))


def _numpy_sort(plan, sc, path=sm.PATH_WINDOWED, heavy_from=None):
    """a correct sort of the windowed plain layout, made by numpy: the arguments of sort_model.check (heavy_from: the smallest
    load the heavy list takes, heavy_thr + 1 in a correct sort)"""
    n, tot = len(sc), plan["nwin"] * plan["nb"]
    bk, en = sm.records(plan, sc)
    count = np.bincount(bk, minlength=tot).astype(np.uint32)
    begin = np.zeros(tot, dtype=np.uint32)
    srt = np.zeros(plan["nwin"] * n, dtype=np.uint32)
    o = np.argsort(bk, kind="stable")
    for w in range(plan["nwin"]):
        c = count[w * plan["nb"] : (w + 1) * plan["nb"]].astype(np.int64)
        begin[w * plan["nb"] : (w + 1) * plan["nb"]] = w * n + np.cumsum(c) - c
    ne = np.nonzero(count)[0]
    cnt = count[ne].astype(np.int64)
    pos = np.repeat(begin[ne].astype(np.int64) - (np.cumsum(cnt) - cnt), cnt) + np.arange(cnt.sum())
    srt[pos] = en[o]
    heavy_ids = np.nonzero(count >= (plan["heavy_thr"] + 1 if heavy_from is None else heavy_from))[0]
    light = np.setdiff1d(np.arange(tot), heavy_ids)
    light = light[np.argsort(-(count[light].astype(np.int64) >> plan["heavy_shift"]), kind="stable")]
    perm = np.concatenate([light, heavy_ids]).astype(np.uint32)
    heavy = np.concatenate([[len(heavy_ids)], heavy_ids]).astype(np.uint32)
    info = dict(plan, buckets=tot, words=plan["nwin"] * n, n_heavy=len(heavy_ids), path=path)
    return info, sc, count, begin, srt, perm, heavy


@pytest.mark.parametrize("name", list(sc_.CASES))
def test_census_every_named_vector_hits_what_its_name_promises(zk, shape, name):
    case = sc_.get(name, zk)
    plan, sc = case["plan"], case["sc"]
    batch = max(case["batch"], 1)
    assert sc.shape == (case["n"] * batch, 8) and case["n"] <= 1 << 21
    # the chain the case is named for is the one the product's rules pick for this plan
    assert case["path"] == case["named_path"], (name, case["path"], plan)
    ints_ok = (sc[:, 7] <= (R >> 224)).all()  # a cheap canonicity screen, then exactly for the rows at the top limb's edge
    assert ints_ok and all(v < R for v in sm.scalars_to_ints(sc[sc[:, 7] == (R >> 224)]))
    if case["promise"] is None:
        assert not case["designed"]
        return
    bk, en = sm.records(plan, sc, batch)
    assert len(bk) <= 6_500_000
    case["promise"](bk, en)
    if name in ("big_thr_exact", "big_thr_plus_1", "big_list_overflow", "two_level_16"):
        fl = sc_.fine_log_big(plan, shape)
        over = np.count_nonzero(np.bincount(bk >> fl) > shape["BIG_THR"])
        assert (min(over, shape["BIG_MAX"]), over) == case["big"]


def test_dense_vectors_carry_their_special_scalars(zk):
    case = sc_.get("one_dense_2p14", zk)
    plan = case["plan"]
    assert (plan["c"], plan["ndigits"]) == (15, 18)  # 17 x 15 = 255: the top position holds the bias and a carry, no scalar bit
    d = sm.recode(case["sc"][:6], plan["c"], plan["ndigits"])
    top = sm.recode(case["sc"], 15, 18)[:, 17]
    assert not d[0].any() and d[1].tolist() == [1] + [0] * 17 and set(top.tolist()) == {0, 1}  # (the carry of a negative digit below it)
    half = 1 << (plan["c"] - 1)
    assert d[4][:16].tolist() == [half] * 16 and d[5][:16].tolist() == [-(half - 1)] * 16 and d[5][16] == 1
    case = sc_.get("one_dense_2p16", zk)
    assert (case["plan"]["c"], case["plan"]["ndigits"]) == (16, 16)  # a 15-bit top digit
    top = sm.recode(case["sc"], 16, 16)[:, 15]
    assert top.max() > 0 and top.max() < 1 << 15 and top.min() >= 0


def test_closed_form_log_is_the_sum_over_the_synthetic_bases(zk):
    case = sc_.get("windowed_heavy_edge", zk)
    vals = sm.scalars_to_ints(case["sc"])
    assert sc_.closed_form_log(case["sc"]) == sum(s * (1 + i * sc_.STEP) for i, s in enumerate(vals)) % R


def test_read_out_refuses_bad_arguments_without_a_device(zk):
    t = zk.tlib
    out = (C.c_uint32 * 13)()
    assert t.zkmi_selftest_msm_sort_shape(None, C.c_uint32(13)) == -1
    assert t.zkmi_selftest_msm_sort_shape(out, C.c_uint32(12)) == -1 and t.zkmi_selftest_msm_sort_shape(out, C.c_uint32(14)) == -1
    assert t.zkmi_selftest_msm_sort_shape(out, C.c_uint32(13)) == 0
    info = (C.c_uint32 * 16)()
    rc = t.zkmi_selftest_msm_sort_dev(None, C.c_int32(0), None, C.c_uint64(4), C.c_uint64(0), C.c_uint32(0), info, C.c_uint32(16), None, None,
                                      None, None, C.c_uint64(0), None, C.c_uint64(0))
    assert rc == -1  # no context
