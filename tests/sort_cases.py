"""The named inputs of the digit-sort tests (test_cpu_msm_sort.py counts them, test_gpu_msm_sort.py sorts them): scalar vectors
designed around the thresholds of csrc/msm_sort.hip, each with the kernel chain (sort_model.PATH_*) it is built for and a
`promise`: what the vector must produce -- loads, partition totals, run positions, oversized counts -- checked from
sort_model's records alone, so that a planner change that moves a threshold fails the CPU census instead of leaving the GPU
test quietly vacuous.  Plans come from the library's planners (zkmi_msm_plan_query, zkmi_selftest_msm_run_schedule), the
constants from zkmi_selftest_msm_sort_shape (`shape`).

A case is a dict: mode / n / plan_n / batch (the arguments of zkmi_selftest_msm_sort_dev), path, sc (uint32 (batch n, 8)),
plan (sort_model's plan dict), designed (one designed digit per scalar: the whole MSM is run over it too), promise(bk, en)."""
import ctypes as C
import functools

import numpy as np

import sort_model as sm
from oracle.bls12_381 import R

STEP = 0xC0FFEE  # synthetic bases: P_i = [1 + i STEP] G


# ---- plans ---------------------------------------------------------------------------------------------------------------------
def heavy_rule(buckets, items):
    """msm_sort.hip plan_set_heavy restated: (heavy_thr, heavy_shift)"""
    mean = -(-items // buckets)
    thr = 256
    while thr < 8 * mean:
        thr <<= 1
    if buckets <= 1 << 16:
        thr = max(3 * mean, 48)
    shift = 0
    while (thr >> shift) > 256:
        shift += 1
    return thr, shift


def plan_windowed(zk, n, plan_n=0):
    """The windowed plan of n terms; plan_n: under the window width of the plan of plan_n terms (a slice of a split MSM)."""
    c = zk.msm_plan_query(plan_n or n, False)[0]
    nwin, nb = 255 // c + 1, 1 << (c - 1)
    thr, shift = heavy_rule(nwin * nb, nwin * n)
    out = (C.c_int32 * 37)()
    rc = zk.tlib.zkmi_selftest_msm_run_schedule(C.c_uint64(n), C.c_int32(0), C.c_uint64(plan_n), C.c_int32(0), C.c_int32(1), C.c_int32(1),
                                                C.c_int32(0), out, C.c_uint32(37))
    assert rc == 0 and (out[0], out[1], out[2]) == (nwin, c, nwin * nb), (rc, list(out[:3]))
    if not plan_n:
        q = zk.msm_plan_query(n, False)
        assert (q[1], q[2], q[3], q[5]) == (nwin, nwin, nb, thr), (q, thr)
    return {"c": c, "nwin": nwin, "nb": nb, "ndigits": 0, "shared": 0, "vec_parts": 1, "heavy_thr": thr, "heavy_shift": shift,
            "top_spread_log": c - 16 if c > 16 else 0, "n": n}


def plan_shared(zk, n, batch=0):
    c, nd, parts, nb, _, thr = zk.msm_plan_query(n, True)
    assert parts * nb == 1 << (c - 1) and nd == 255 // c + 1
    t, shift = heavy_rule(parts * nb * max(batch, 1), nd * n * max(batch, 1))
    assert batch or t == thr, (t, thr)
    return {"c": c, "nwin": parts * max(batch, 1), "nb": nb, "ndigits": nd, "shared": 1, "vec_parts": parts if batch else 1,
            "heavy_thr": t, "heavy_shift": shift, "top_spread_log": 0, "n": n}


def expected_path(plan, shape, batch=0):
    """The kernel chain the product runs for this plan (msm_sort.hip run / run_shared / run_shared_batch), restated."""
    n = plan["n"]
    if batch:
        return sm.PATH_SHARED_BATCH
    if not plan["shared"]:
        return sm.PATH_BIG_FINE if plan["c"] > 16 or (plan["c"] == 16 and n >= 1 << 21) else sm.PATH_WINDOWED
    if plan["nwin"] == 1:
        return sm.PATH_SHARED_ONE
    parts = (plan["nwin"] * plan["nb"]) >> shape["FINE_LOG"]
    return sm.PATH_SHARED_FINE if plan["ndigits"] * n // parts <= 2 * shape["FINE_ROUND"] and plan["ndigits"] <= 16 else sm.PATH_SHARED_RECORDS


def fine_log_big(plan, shape):
    """log2 of the buckets per fine partition of the two-level sort (run_windowed_big)"""
    fl = shape["FINE_LOG"]
    while fl > 7 and (plan["n"] >> (plan["c"] - 1 - fl)) > shape["FINE_ROUND"]:
        fl -= 1
    return fl


def plan_matches_info(plan, info):
    return all(plan[k] == info[k] for k in ("c", "nwin", "nb", "ndigits", "shared", "vec_parts", "heavy_thr", "heavy_shift", "top_spread_log"))


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def spread(m, neg, k, wmax, w0=0):
    """a load of k scalars with the designed digit (m, neg), dealt over the positions w0 .. wmax - 1 (the entry words differ)"""
    ws = list(range(w0, wmax))
    per, extra = divmod(k, len(ws))
    return [(w, m, neg, per + (1 if j < extra else 0)) for j, w in enumerate(ws) if per + (1 if j < extra else 0)]


def pad(parts, n):
    sc = np.concatenate(parts) if parts else np.zeros((0, 8), dtype=np.uint32)
    assert len(sc) <= n, (len(sc), n)
    out = np.zeros((n, 8), dtype=np.uint32)
    out[: len(sc)] = sc
    return out


def fine_totals(hist, fine_log):
    return hist.reshape(-1, 1 << fine_log).sum(axis=1)


def closed_form_log(sc, r=R):
    """sum_i s_i (1 + i STEP) mod r: the discrete log of the MSM over the synthetic bases"""
    sc = np.asarray(sc, dtype=np.uint32).reshape(-1, 8)
    nz = np.nonzero(sc.any(axis=1))[0]
    rows, inv = np.unique(sc[nz], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert len(sc) < 1 << 26  # the index sums below are exact in float64
    cnt, isum = np.bincount(inv, minlength=len(rows)), np.bincount(inv, weights=nz.astype(np.float64), minlength=len(rows))
    return sum(v * (int(k) + STEP * int(t)) for v, k, t in zip(sm.scalars_to_ints(rows), cnt, isum)) % r


SPECIALS = (0, 1, R - 1, R - 2)


def dense_case(zk, shape, mode, n, plan_n=0, batch=0, seed=1, zero_vector=None, live=None):
    plan = plan_shared(zk, n, batch) if mode else plan_windowed(zk, n, plan_n)
    sp = SPECIALS + (sm.all_digits(plan, 1 << (plan["c"] - 1), R), sm.all_digits(plan, -((1 << (plan["c"] - 1)) - 1), R))
    vecs = []
    for v in range(max(batch, 1)):
        s = sm.dense(n, R, seed + 977 * v, sp if v == 0 else ())
        if live is not None:
            s[live:] = 0
        if zero_vector == v:
            s[:] = 0
        vecs.append(s)
    return {"mode": mode, "n": n, "plan_n": plan_n, "batch": batch, "sc": np.concatenate(vecs), "plan": plan,
            "path": expected_path(plan, shape, batch), "designed": False, "promise": None}


def designed_case(zk, shape, mode, n, sc, plan_n=0, promise=None):
    plan = plan_shared(zk, n) if mode else plan_windowed(zk, n, plan_n)
    return {"mode": mode, "n": n, "plan_n": plan_n, "batch": 0, "sc": sc, "plan": plan, "path": expected_path(plan, shape), "designed": True,
            "promise": promise}


# ---- shared plan, fine-partition form: k_fpart_sort ---------------------------------------------------------------------------
N17 = 1 << 17


def _fine_plan(zk, shape):
    plan = plan_shared(zk, N17)
    # from the planner: c = 17, 16 digits, 2 partitions, 64 fine partitions of 1 024 buckets
    assert (plan["c"], plan["ndigits"], plan["nwin"], plan["nb"]) == (17, 16, 2, 1 << 15) and shape["FINE_LOG"] == 10
    assert shape["FSORT_RPT"] * 1024 == shape["FINE_STAGE"] and shape["FINE_ROUND"] < shape["FINE_STAGE"]
    return plan, plan["ndigits"] - 2  # positions 0 .. wmax - 1: a negative digit's carry stays below the top digit


def fm(q, l):
    """the digit magnitude of local bucket l of fine partition q (2^10 buckets each)"""
    return q * 1024 + l + 1


def _runs(hist, q):
    """(local bucket, first position, load) of the non-empty buckets of fine partition q"""
    h = hist[q * 1024 : (q + 1) * 1024]
    beg = np.cumsum(h) - h
    return [(int(l), int(beg[l]), int(h[l])) for l in np.nonzero(h)[0]]


def case_fine_stage_edges(zk, shape):
    """partition 2: exactly FINE_STAGE records (the register form's largest); partition 3: FINE_STAGE + 1 (round form, two
    rounds) with a run that starts at FINE_ROUND - 1 and ends at the stage's LAST slot, and a last non-empty bucket followed by
    empty ones only; partition 4: FINE_STAGE + 1 with the same run one longer: its last entry is written directly; every other
    fine partition is empty"""
    plan, wmax = _fine_plan(zk, shape)
    ST, RD = shape["FINE_STAGE"], shape["FINE_ROUND"]
    slack = ST - RD
    loads = spread(fm(2, 0), False, 20000, wmax) + spread(fm(2, 511), False, ST - 20000 - 864, wmax) + spread(fm(2, 1023), False, 864, wmax)
    loads += spread(fm(3, 0), False, RD - 1, wmax) + spread(fm(3, 1), False, slack + 1, wmax) + spread(fm(3, 5), False, 1, wmax)
    loads += spread(fm(4, 0), False, RD - 1, wmax) + spread(fm(4, 1), False, slack + 2, wmax)
    sc = pad([sm.design(plan, loads, R)], N17)

    def promise(bk, en):
        hist = np.bincount(bk, minlength=1 << 16)
        tot = fine_totals(hist, 10)
        assert tot[2] == ST and tot[2] % 1024 == 0 and tot[3] == ST + 1 and tot[4] == ST + 1 and tot.sum() == tot[2] + tot[3] + tot[4]
        assert -(-int(tot[3]) // RD) == 2
        assert _runs(hist, 3) == [(0, 0, RD - 1), (1, RD - 1, slack + 1), (5, ST, 1)] and RD - 1 + slack + 1 == ST
        assert _runs(hist, 4) == [(0, 0, RD - 1), (1, RD - 1, slack + 2)]

    return designed_case(zk, shape, 1, N17, sc, promise=promise)


def case_fine_long_run(zk, shape):
    """partition 5: one bucket of more than 3 FINE_ROUND records in front of small ones -- rounds 1 and 2 own no bucket, the
    next_rd jump --; partition 6: every record names ONE bucket (the aggregated counter path, register form); partition 7: the
    same total over two buckets alternating by point index (the mixed path); partition 0: the stray +1 digits of partition
    6's negative digits, one bucket again"""
    plan, wmax = _fine_plan(zk, shape)
    RD = shape["FINE_ROUND"]
    big = 3 * RD + 5
    a = sm.design(plan, spread(fm(5, 0), False, big, wmax) + spread(fm(5, 1), False, 10, wmax) + spread(fm(5, 7), True, 3, wmax), R)
    b = sm.design(plan, spread(fm(6, 100), True, 6000, wmax), R)
    c = sm.design(plan, [(2, fm(7, 200), False, 3000), (2, fm(7, 900), False, 3000)], R, interleave=True)
    sc = pad([a, b, c], N17)
    first_c = len(a) + len(b)

    def promise(bk, en):
        hist = np.bincount(bk, minlength=1 << 16)
        tot = fine_totals(hist, 10)
        assert _runs(hist, 5) == [(0, 0, big), (1, big, 10), (7, big + 10, 3)]
        assert -(-int(tot[5]) // RD) == 4 and big // RD == 3  # four rounds; the first bucket behind the run begins in round 3
        assert _runs(hist, 6) == [(100, 0, 6000)] and _runs(hist, 0) == [(0, 0, 6003)]
        assert _runs(hist, 7) == [(200, 0, 3000), (900, 3000, 3000)]
        i = (en[bk == fm(7, 200) - 1] & 0x7FFFFFFF) % N17
        assert ((i - first_c) % 2 == 0).all()  # alternating by point index
        assert tot.sum() == tot[0] + tot[5] + tot[6] + tot[7]

    return designed_case(zk, shape, 1, N17, sc, promise=promise)


def case_fine_round_multiple(zk, shape):
    """partition 8: FINE_STAGE + 1 records, its second bucket begins exactly at FINE_ROUND; partitions 9 .. 13: totals 1 024,
    1 023, 1 025, 2 048 and 1 (whole waves walk the records: a multiple of 1 024 and one off it), negative digits, whose
    strays fill bucket 0"""
    plan, wmax = _fine_plan(zk, shape)
    ST, RD = shape["FINE_STAGE"], shape["FINE_ROUND"]
    loads = spread(fm(8, 0), False, RD, wmax) + spread(fm(8, 1), False, ST + 1 - RD, wmax)
    small = [(9, 1024), (10, 1023), (11, 1025), (12, 2048), (13, 1)]
    for q, k in small:
        loads += spread(fm(q, 17), True, k // 2, wmax) + spread(fm(q, 1000), True, k - k // 2, wmax)
    sc = pad([sm.design(plan, loads, R)], N17)

    def promise(bk, en):
        hist = np.bincount(bk, minlength=1 << 16)
        tot = fine_totals(hist, 10)
        assert _runs(hist, 8) == [(0, 0, RD), (1, RD, ST + 1 - RD)] and tot[8] == ST + 1
        assert [int(tot[q]) for q, _ in small] == [k for _, k in small]
        assert _runs(hist, 0) == [(0, 0, sum(k for _, k in small))]
        assert (en[bk >= 9 * 1024] >> 31).all() and not (en[bk < 9 * 1024] >> 31).any()

    return designed_case(zk, shape, 1, N17, sc, promise=promise)


# ---- heavy threshold and ordering key ------------------------------------------------------------------------------------------
def _heavy_loads(plan, wmax, where):
    """loads heavy_thr (negative digits: the strays stay below the threshold) and heavy_thr + 1, and pairs 2k, 2k + 1 that share
    an ordering key where heavy_shift = 1; where(j) -> (w, m) of designed bucket j"""
    thr, shift = plan["heavy_thr"], plan["heavy_shift"]
    sizes = [(thr, True), (thr + 1, False)]
    for k in (3, thr // 4, thr // 2 - 1):
        sizes += [(2 * k, False), (2 * k + 1, False)]
    loads = []
    for j, (k, neg) in enumerate(sizes):
        w, m = where(j)
        loads.append((w, m, neg, k))
    return loads, sizes


def case_windowed_heavy_edge(zk, shape):
    """plain windowed chain, n = 4097: loads of exactly heavy_thr and heavy_thr + 1 in two buckets of different windows"""
    n = 4097
    plan = plan_windowed(zk, n)
    where = lambda j: (1 + 2 * j, 7 + j)
    loads, sizes = _heavy_loads(plan, None, where)
    sc = pad([sm.design(plan, loads, R)], n)

    def promise(bk, en):
        hist = np.bincount(bk, minlength=plan["nwin"] * plan["nb"])
        for j, (k, neg) in enumerate(sizes):
            w, m = where(j)
            assert hist[w * plan["nb"] + m - 1] == k
        assert np.count_nonzero(hist > plan["heavy_thr"]) == 1 and np.count_nonzero(hist == plan["heavy_thr"]) == 2  # (the strays of the first)

    return designed_case(zk, shape, 0, n, sc, promise=promise)


def case_records_heavy_edge(zk, shape):
    """shared record form, n = 2^19 (heavy_shift = 1): loads heavy_thr, heavy_thr + 1, and pairs 2k, 2k + 1 of one ordering key"""
    n = 1 << 19
    plan = plan_shared(zk, n)
    assert plan["heavy_shift"] == 1
    wmax = plan["ndigits"] - 2
    where = lambda j: (j % wmax, 40000 + 1000 * j)
    loads, sizes = _heavy_loads(plan, wmax, where)
    sc = pad([sm.design(plan, loads, R)], n)

    def promise(bk, en):
        hist = np.bincount(bk, minlength=plan["nwin"] * plan["nb"])
        assert [int(hist[where(j)[1] - 1]) for j in range(len(sizes))] == [k for k, _ in sizes]
        assert np.count_nonzero(hist > plan["heavy_thr"]) == 1
        keys = [k >> 1 for k, _ in sizes[2:]]
        assert keys[0::2] == keys[1::2]

    return designed_case(zk, shape, 1, n, sc, promise=promise)


def heavy_cap_vector(zk, shape, heavies):
    """plain windowed plan, n just above 2^18: exactly `heavies` heavy buckets of heavy_thr + 1 entries each"""
    n = (shape["MSM_HEAVY_CAP"] + 1) * 257
    plan = plan_windowed(zk, n)
    assert plan["c"] == 16 and plan["heavy_thr"] == 256 and n > 1 << 18 and heavies * 257 <= n
    loads = [(j % 14, 2 + j // 14, False, plan["heavy_thr"] + 1) for j in range(heavies)]
    return plan, pad([sm.design(plan, loads, R)], n)


def case_heavy_cap(zk, shape, delta):
    heavies = shape["MSM_HEAVY_CAP"] + delta
    plan, sc = heavy_cap_vector(zk, shape, heavies)

    def promise(bk, en):
        hist = np.bincount(bk, minlength=plan["nwin"] * plan["nb"])
        assert np.count_nonzero(hist > plan["heavy_thr"]) == heavies and hist.max() == plan["heavy_thr"] + 1 and hist.sum() == heavies * 257

    return designed_case(zk, shape, 0, len(sc), sc, promise=promise)


# ---- big windowed plan (plan_n = 2^24), fine form ------------------------------------------------------------------------------
PLAN_BIG = 1 << 24


def _big_plan(zk, shape, n):
    plan = plan_windowed(zk, n, PLAN_BIG)
    assert (plan["c"], plan["nwin"], plan["top_spread_log"]) == (20, 13, 4) and fine_log_big(plan, shape) == 10
    return plan


def case_big_split_batches(zk, shape):
    """groups (window, 2^15 buckets) of exactly SPLIT_B, SPLIT_B + 1 and 16 SPLIT_B + 1 records, each spread over the group's 32
    fine partitions"""
    SB = shape["SPLIT_B"]
    n = SB + SB + 1 + 16 * SB + 1
    plan = _big_plan(zk, shape, n)
    groups = [(1, 2, SB), (2, 3, SB + 1), (4, 5, 16 * SB + 1)]  # (window, group of the window, records)
    loads = []
    for w, g, k in groups:
        per, extra = divmod(k, 4096)
        loads += [(w, g * 32768 + 8 * j + 1, j % 2 == 1, per + (1 if j < extra else 0)) for j in range(4096) if per + (1 if j < extra else 0)]
    sc = sm.design(plan, loads, R, n=n)

    def promise(bk, en):
        tot = np.bincount(bk >> 15, minlength=13 * 16)
        # (the negative digits' strays: bucket 0 of the next window, group 0 of it)
        assert [int(tot[w * 16 + g]) for w, g, _ in groups] == [k for _, _, k in groups]
        assert np.bincount(bk >> 10).max() <= shape["BIG_THR"]

    return designed_case(zk, shape, 0, n, sc, PLAN_BIG, promise)


def _one_fine_partition(plan, n, w, q, nbuckets):
    """n scalars whose digit at position w walks the first nbuckets buckets of fine partition q of that window"""
    per, extra = divmod(n, nbuckets)
    return sm.design(plan, [(w, q * 1024 + j + 1, False, per + (1 if j < extra else 0)) for j in range(nbuckets)], R, interleave=True)


def case_big_thr(zk, shape, over):
    """every scalar's digit at position 3, inside fine partition 5 of that window: BIG_THR records (not listed: the round form of
    k_fpart_sort takes them) or BIG_THR + 1 (listed: the k_big_* kernels)"""
    n = shape["BIG_THR"] + over
    plan = _big_plan(zk, shape, n)
    sc = _one_fine_partition(plan, n, 3, 5, 700)

    def promise(bk, en):
        tot = np.bincount(bk >> 10, minlength=13 * 512)
        assert tot[3 * 512 + 5] == n == tot.sum()
        assert np.count_nonzero(tot > shape["BIG_THR"]) == over

    out = designed_case(zk, shape, 0, n, sc, PLAN_BIG, promise)
    out["big"] = (over, over)
    return out


def case_big_list_overflow(zk, shape):
    """n = 3 (BIG_THR + 1) scalars in three groups, every scalar with a digit in each of the twelve full windows, group g inside
    fine partition 7 + g: 36 fine partitions above BIG_THR, four more than the list holds -- those stay with k_fpart_sort.  The
    top window only covers 15 bits and is spread over 16 groups by point index: it cannot be oversized here (its digits are 0)"""
    per = shape["BIG_THR"] + 1
    n = 3 * per
    plan = _big_plan(zk, shape, n)
    assert shape["BIG_MAX"] == 32
    # scalar i of group g: the digit of window w is local bucket (i + 37 w) mod 600 of fine partition 7 + g
    table = [sum(((7 + g) * 1024 + (j + 37 * w) % 600 + 1) << (20 * w) for w in range(12)) for g in range(3) for j in range(600)]
    assert max(table) < 1 << 240
    i = np.arange(per)
    sc = sm.scalars_from_ints(table)[np.concatenate([600 * g + i % 600 for g in range(3)])]

    def promise(bk, en):
        tot = np.bincount(bk >> 10, minlength=13 * 512)
        big = np.nonzero(tot > shape["BIG_THR"])[0]
        assert len(big) == 36 > shape["BIG_MAX"] and (tot[big] == per).all() and (big // 512 < 12).all() and tot.sum() == 12 * n

    out = designed_case(zk, shape, 0, n, sc, PLAN_BIG, promise)
    out["big"] = (shape["BIG_MAX"], 36)
    return out


def case_two_level_16(zk, shape):
    """the two-level sort of 16-bit windows at its smallest product size, n = 2^21: BIG_THR + 1 scalars are non-zero, their digit
    at position 3 inside one fine partition (2^9 buckets here), which is listed"""
    n = 1 << 21
    plan = plan_windowed(zk, n)
    fl = fine_log_big(plan, shape)
    assert plan["c"] == 16 and fl == 9
    live = shape["BIG_THR"] + 1
    per, extra = divmod(live, 300)
    loads = [(3, 5 * 512 + j + 1, j % 3 == 0, per + (1 if j < extra else 0)) for j in range(300)]
    sc = pad([sm.design(plan, loads, R, interleave=True)], n)

    def promise(bk, en):
        tot = np.bincount(bk >> fl, minlength=16 * 64)
        assert tot[3 * 64 + 5] == live and np.count_nonzero(tot > shape["BIG_THR"]) == 1

    out = designed_case(zk, shape, 0, n, sc, promise=promise)
    out["big"] = (1, 1)
    return out


# ---- the table -----------------------------------------------------------------------------------------------------------------
P = sm
CASES = {
    # shared, fine-partition form
    "fine_stage_edges": (P.PATH_SHARED_FINE, case_fine_stage_edges),
    "fine_long_run": (P.PATH_SHARED_FINE, case_fine_long_run),
    "fine_round_multiple": (P.PATH_SHARED_FINE, case_fine_round_multiple),
    "fine_dense_past_a_batch": (P.PATH_SHARED_FINE, lambda zk, sh: dense_case(zk, sh, 1, N17 + 1, seed=11)),
    # shared, one partition
    "one_dense_2p14": (P.PATH_SHARED_ONE, lambda zk, sh: dense_case(zk, sh, 1, 1 << 14, seed=12)),
    "one_dense_2p16": (P.PATH_SHARED_ONE, lambda zk, sh: dense_case(zk, sh, 1, 1 << 16, seed=13)),
    # shared, record form (2^19: the first 2^18 scalars are dense, the others 0 -- 3.9 M records)
    # (the planner leaves the fine form where ndigits n / 64 -- an integer division -- exceeds 2 FINE_ROUND: 2^18 + 1 .. 2^18 + 3
    # still run the fine form, at its largest mean partition; 2^18 + 4 is the smallest size of the record form)
    "fine_dense_2p18_1": (P.PATH_SHARED_FINE, lambda zk, sh: dense_case(zk, sh, 1, (1 << 18) + 1, seed=14)),
    "records_dense_2p18_4": (P.PATH_SHARED_RECORDS, lambda zk, sh: dense_case(zk, sh, 1, (1 << 18) + 4, seed=14)),
    "records_dense_2p19": (P.PATH_SHARED_RECORDS, lambda zk, sh: dense_case(zk, sh, 1, 1 << 19, seed=15, live=1 << 18)),
    "records_heavy_edge": (P.PATH_SHARED_RECORDS, case_records_heavy_edge),
    # shared batch
    "batch3_2p13": (P.PATH_SHARED_BATCH, lambda zk, sh: dense_case(zk, sh, 2, 1 << 13, batch=3, seed=16, zero_vector=1)),
    "batch2_2p17": (P.PATH_SHARED_BATCH, lambda zk, sh: dense_case(zk, sh, 2, N17, batch=2, seed=17, zero_vector=0)),
    # plain windowed
    **{"windowed_dense_%d" % n: (P.PATH_WINDOWED, functools.partial(lambda zk, sh, n: dense_case(zk, sh, 0, n, seed=18 + n), n=n))
       for n in (1, 1023, 1024, 1025, 4097, N17, N17 + 1)},
    "windowed_heavy_edge": (P.PATH_WINDOWED, case_windowed_heavy_edge),
    "heavy_cap_minus_1": (P.PATH_WINDOWED, functools.partial(case_heavy_cap, delta=-1)),
    "heavy_cap": (P.PATH_WINDOWED, functools.partial(case_heavy_cap, delta=0)),
    "heavy_cap_plus_1": (P.PATH_WINDOWED, functools.partial(case_heavy_cap, delta=1)),
    # big windowed, fine form
    **{"big_dense_%d" % n: (P.PATH_BIG_FINE, functools.partial(lambda zk, sh, n: dense_case(zk, sh, 0, n, PLAN_BIG, seed=30 + n), n=n))
       for n in (1, 1025, (1 << 16) + 1)},
    "big_split_batches": (P.PATH_BIG_FINE, case_big_split_batches),
    "big_thr_exact": (P.PATH_BIG_FINE, functools.partial(case_big_thr, over=0)),
    "big_thr_plus_1": (P.PATH_BIG_FINE, functools.partial(case_big_thr, over=1)),
    "big_list_overflow": (P.PATH_BIG_FINE, case_big_list_overflow),
    # two-level sort of 16-bit windows
    "two_level_16": (P.PATH_BIG_FINE, case_two_level_16),
}
# the vectors whose MSM also runs in G2 and over BN254
HEAVY_MSM_CASES = ("windowed_heavy_edge", "heavy_cap_minus_1", "heavy_cap", "heavy_cap_plus_1")


@functools.lru_cache(maxsize=4)
def build(name, zk, shape_items):
    shape = dict(shape_items)
    path, fn = CASES[name]
    case = fn(zk, shape)
    case["name"], case["named_path"] = name, path
    case.setdefault("big", (0, 0))
    return case


def get(name, zk):
    return build(name, zk, tuple(sorted(zk.selftest_msm_sort_shape().items())))
