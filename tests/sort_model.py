"""A numpy model of the MSM digit sort's contract (csrc/msm_sort.hip), for test_cpu_msm_sort.py and test_gpu_msm_sort.py.

It works from the scalars and the plan fields alone and calls nothing of the library: `plan` is a dict with the keys of
zkmi_selftest_msm_sort_dev's out_info that describe a plan (c, nwin, nb, ndigits, shared, vec_parts, heavy_thr, heavy_shift,
top_spread_log); tests/sort_cases.py builds the same dict from the library's planners.

RECODING.  k' = k + M over nine 32-bit limbs, M = sum_w (2^(c-1) - 1) 2^(c w) over all digit positions of the plan;
d_w = ((k' >> c w) & (2^c - 1)) - (2^(c-1) - 1), in [-(2^(c-1) - 1), 2^(c-1)]; a zero digit makes no record.

RECORDS.  One per non-zero digit: (bucket, entry word).
    windowed     bucket w 2^(c-1) + |d| - 1, entry i | sign << 31; in the top window of a plan with top_spread_log > 0 the
                 bucket is w 2^(c-1) + (i mod 2^top_spread_log) 2^15 + |d| - 1 (csrc/msm.hpp MsmPlan::top_spread_log)
    shared       bucket |d| - 1, entry (w n + i) | sign << 31
    batch        vector v's buckets sit behind those of the vectors before it (vec_parts x nb each), entries per vector

Scalars travel as uint32 arrays of shape (n, 8), little-endian limbs (scalars_from_ints / scalars_to_bytes)."""
import numpy as np

SIGN = np.uint32(0x80000000)
# MsmSortPath (csrc/msm.hpp)
PATH_WINDOWED, PATH_BIG_FINE, PATH_BIG_RECORDS, PATH_SHARED_ONE, PATH_SHARED_FINE, PATH_SHARED_RECORDS, PATH_SHARED_BATCH = 1, 2, 3, 4, 5, 6, 7
PACKED = (PATH_BIG_FINE, PATH_BIG_RECORDS, PATH_SHARED_ONE, PATH_SHARED_FINE, PATH_SHARED_RECORDS, PATH_SHARED_BATCH)


def scalars_from_ints(vals):
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u4").reshape(-1, 8).copy()


def scalars_to_ints(sc):
    raw = np.ascontiguousarray(sc, dtype="<u4").tobytes()
    return [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]


def scalars_to_bytes(sc):
    return np.ascontiguousarray(sc, dtype="<u4").tobytes()


def positions(plan):
    """digit positions of a scalar under the plan"""
    return plan["ndigits"] if plan["shared"] else 255 // plan["c"] + 1


def recode(sc, c, npos):
    """signed digits of every scalar: int64 array (n, npos)"""
    sc = np.asarray(sc, dtype=np.uint32).reshape(-1, 8)
    bias = (1 << (c - 1)) - 1
    m = sum(bias << (c * w) for w in range(npos))
    k = np.zeros((sc.shape[0], 10), dtype=np.uint64)  # nine limbs of k', and a zero behind them for the last extraction
    carry = np.zeros(sc.shape[0], dtype=np.uint64)
    for j in range(9):
        v = (sc[:, j].astype(np.uint64) if j < 8 else np.uint64(0)) + np.uint64((m >> (32 * j)) & 0xFFFFFFFF) + carry
        k[:, j] = v & np.uint64(0xFFFFFFFF)
        carry = v >> np.uint64(32)
    assert m >> 288 == 0 and not carry.any()
    out = np.empty((sc.shape[0], npos), dtype=np.int64)
    for w in range(npos):
        limb, sh = (c * w) >> 5, (c * w) & 31
        v = k[:, limb] | (k[:, limb + 1] << np.uint64(32))
        out[:, w] = ((v >> np.uint64(sh)) & np.uint64((1 << c) - 1)).astype(np.int64) - bias
    return out


def records(plan, sc, batch=1):
    """(bucket ids int64, entry words uint32) of every non-zero digit; sc: (batch * n, 8), vector after vector"""
    c, nb, tsl = plan["c"], plan["nb"], plan["top_spread_log"]
    sc = np.asarray(sc, dtype=np.uint32).reshape(-1, 8)
    assert sc.shape[0] % batch == 0
    n = sc.shape[0] // batch
    npos = positions(plan)
    bk, en = [], []
    for v in range(batch):
        vec = sc[v * n : (v + 1) * n]
        live = np.nonzero(vec.any(axis=1))[0]  # (a zero scalar makes no record)
        d = recode(vec[live], c, npos)
        i, w = np.nonzero(d)
        dv = d[i, w]
        i = live[i]
        mag = np.abs(dv)
        sign = np.where(dv < 0, SIGN, np.uint32(0)).astype(np.uint32)
        if plan["shared"]:
            assert n * npos < 1 << 31
            bucket = mag - 1 + v * plan["vec_parts"] * nb
            entry = (w * n + i).astype(np.uint32) | sign
        else:
            assert batch == 1 and nb == 1 << (c - 1)
            bucket = w * nb + mag - 1
            if tsl:
                top = w == npos - 1
                assert (mag[top] <= 1 << 15).all()
                bucket = np.where(top, bucket + (i & ((1 << tsl) - 1)) * (1 << 15), bucket)
            entry = i.astype(np.uint32) | sign
        bk.append(bucket.astype(np.int64))
        en.append(entry)
    return np.concatenate(bk), np.concatenate(en)


def histogram(plan, sc, batch=1):
    bk, _ = records(plan, sc, batch)
    return np.bincount(bk, minlength=plan["nwin"] * plan["nb"])


def check(info, sc, count, begin, srt, perm, heavy, batch=1):
    """The sort's contract: info = the dict of zkmi_selftest_msm_sort_dev, the arrays as it returned them."""
    u32 = lambda a: np.frombuffer(a, dtype=np.uint32) if not isinstance(a, np.ndarray) else a.astype(np.uint32, copy=False)
    count, begin, srt, perm, heavy = (u32(a) for a in (count, begin, srt, perm, heavy))
    sc = np.asarray(sc, dtype=np.uint32).reshape(-1, 8)
    n = sc.shape[0] // batch
    tot_b, words, path = info["buckets"], info["words"], info["path"]
    assert tot_b == info["nwin"] * info["nb"] and len(count) == len(begin) == len(perm) == tot_b
    mb, me = records(info, sc, batch)
    # 1. the histogram
    want = np.bincount(mb, minlength=tot_b)
    assert len(want) == tot_b, "the model names a bucket beyond the plan's"
    bad = np.nonzero(want != count)[0]
    assert bad.size == 0, ("count[] differs from the model's histogram", bad[:8], count[bad[:8]], want[bad[:8]])
    # 2. the ranges of the non-empty buckets
    ne = np.nonzero(count)[0]
    lo = begin[ne].astype(np.int64)
    hi = lo + count[ne]
    order = np.argsort(lo, kind="stable")
    slo, shi = lo[order], hi[order]
    if path in PACKED:
        assert words == len(mb), ("records in sorted[]", words, len(mb))
        if ne.size:
            assert slo[0] == 0 and shi[-1] == words and (shi[:-1] == slo[1:]).all(), "the ranges do not tile [0, records)"
    else:
        assert path == PATH_WINDOWED and words == info["nwin"] * n
        w = ne // info["nb"]
        assert (shi[:-1] <= slo[1:]).all(), "ranges overlap"
        assert (lo >= w * n).all() and (hi <= (w + 1) * n).all(), "a range leaves its window's region"
    # 3. the multiset of entry words per bucket
    cnt = count[ne].astype(np.int64)
    pos = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(cnt.sum())
    got_b, got_e = np.repeat(ne, cnt), srt[pos]
    o1, o2 = np.lexsort((got_e, got_b)), np.lexsort((me, mb))
    assert (got_b[o1] == mb[o2]).all()
    bad = np.nonzero(got_e[o1] != me[o2])[0]
    assert bad.size == 0, ("a bucket's entries differ from the model's", got_b[o1][bad[:8]], got_e[o1][bad[:8]], me[o2][bad[:8]])
    # 4. the heavy list
    nh = int(heavy[0])
    hv = heavy[1 : 1 + nh]
    want_h = np.nonzero(count > info["heavy_thr"])[0]
    assert nh == info["n_heavy"] == want_h.size, ("heavy buckets", nh, info["n_heavy"], want_h.size)
    assert (np.sort(hv) == want_h).all(), "heavy[] is not the set of buckets above the threshold"
    # 5. the load order
    assert (np.sort(perm) == np.arange(tot_b)).all(), "perm is not a permutation of the bucket ids"
    assert (np.sort(perm[tot_b - nh :]) == want_h).all(), "the heavy buckets are not perm's last slots"
    key = count[perm[: tot_b - nh]] >> np.uint32(info["heavy_shift"])
    assert (key[:-1] >= key[1:]).all(), "the ordering key increases along perm"
    return {"records": len(mb), "heavy": nh, "max_load": int(count.max()) if tot_b else 0}


# ---- designed inputs -----------------------------------------------------------------------------------------------------------
def design(plan, loads, r, n=None, interleave=False):
    """Scalars with ONE designed signed digit each, in the writing of test_first_pair.py: m << c w, or 2^(c (w + 1)) - (m << c w)
    for a negative digit (its stray +1 digit lands in bucket 1 - 1 = 0 of the next position: put no designed load there).
    loads: [(w, m, negative, how many)], laid out one run after another (interleave: dealt round-robin while they last);
    the scalars behind them, up to n, are 0 and make no record.  -> uint32 array (n, 8)."""
    c = plan["c"]
    vals, idx = [], []
    for j, (w, m, neg, k) in enumerate(loads):
        assert 1 <= m <= (1 << (c - 1)) - (1 if neg else 0) and k >= 0
        s = (1 << (c * (w + 1))) - (m << (c * w)) if neg else m << (c * w)
        assert 0 < s < r and s < 1 << 250, (w, m, neg)
        vals.append(s)
        idx.append(np.full(k, j, dtype=np.int64))
    if interleave:
        kmax = max(len(a) for a in idx)
        grid = np.full((kmax, len(idx)), -1, dtype=np.int64)
        for j, a in enumerate(idx):
            grid[: len(a), j] = j
        flat = grid.reshape(-1)
        flat = flat[flat >= 0]
    else:
        flat = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
    total = len(flat)
    n = total if n is None else n
    assert total <= n, (total, n)
    out = np.zeros((n, 8), dtype=np.uint32)
    if total:
        out[:total] = scalars_from_ints(vals)[flat]
    return out


def dense(n, r, seed, specials=()):
    """n uniform canonical scalars (top byte masked to stay below r), the given special values first"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    top = (r >> 248) >> 1  # a mask below r's top byte
    mask = 1
    while mask * 2 - 1 <= top:
        mask *= 2
    raw[:, 31] &= mask - 1
    out = np.frombuffer(raw.tobytes(), dtype="<u4").reshape(n, 8).copy()
    sp = [s % r for s in specials][:n]
    if sp:
        out[: len(sp)] = scalars_from_ints(sp)
    return out


def all_digits(plan, value, r):
    """the scalar whose digit positions below 2^250 (and below the plan's top one) all hold the signed digit `value`"""
    c = plan["c"]
    k = min(positions(plan) - 1, 250 // c)
    s = sum(value << (c * w) for w in range(k))
    if value < 0:
        s += 1 << (c * k)  # (a +1 digit above them: the scalar is positive)
    assert 0 < s < r
    return s
