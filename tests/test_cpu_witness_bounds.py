"""The witness map's value-range model (tests/witness28.py) against an integer simulation of the transforms, and the library's
key-build verdict (zkmi_selftest_witness_bound, csrc/witness_bound.hpp) against the model's.  No GPU.

Part 1 runs the decimation-in-frequency and decimation-in-time butterflies of ntt.hip's k_ntt_pass on Python integers, Montgomery
products predicted exactly (limbs28.Field.mont), on small synthetic plans -- 2^9 as 3 + 3 + 3 stages without twists (the shape of
a three-pass plan), 2^8 as 4 + 4 with a twist, one pass of 6 -- with inputs in random signed representations x + k r, and asserts
that the model's bound dominates every node and that the constant vector attains it within a factor 2 (the model is not
vacuous).  Part 2 compares verdicts on a grid of shapes."""
import ctypes as C

import numpy as np
import pytest

import limbs28 as lb
import witness28 as wm

F28 = {1: lb.FIELDS[1], 3: lb.FIELDS[3]}
PLANS = {
    "3+3+3": [(3, False), (3, False), (3, False)],
    "4+4 twist": [(4, True), (4, False)],
    "6": [(6, False)],
    "2+5 twist, post": [(2, True), (5, True)],
    "3+3+3, post": [(3, False), (3, False), (3, True)],
}


def _rev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _reps(rng, lf, x, spread):
    """A representation of the residue x's Montgomery form inside (-r/2, 3r/2), moved by `spread` moduli either way."""
    return lf.rep(x) + (rng.below(2 * spread + 1) - spread) * lf.p if spread else lf.rep(x)


def simulate_dif(lf, plan, vals, om, rng):
    """k_ntt_pass<DIF> on integers.  Plans with a twist run their passes with local twiddles and the twist behind the strided
    pass; the others gather the global twiddle.  -> (outputs, every stored node's value, position by position per stage)."""
    r = lf.p
    log_n = sum(s for s, _ in plan)
    n = 1 << log_n
    twisted = len(plan) == 2 and plan[0][1]
    v = list(vals)
    nodes = [list(v)]
    t_hi = log_n
    for k, (stages, mul) in enumerate(plan):
        t0 = t_hi - stages
        for u in range(stages - 1, -1, -1):
            t = t0 + u
            d = 1 << t
            for i in range(n):
                if i & d:
                    continue
                if twisted:  # w_{2^S}^((e mod 2^u) 2^(S-1-u)), e = the element's row inside the pass
                    e = (i >> t0) & ((1 << stages) - 1)
                    ex = ((e & ((1 << u) - 1)) << (stages - 1 - u)) << (log_n - stages)
                else:
                    ex = (i & (d - 1)) << (log_n - 1 - t)
                w = _reps(rng, lf, pow(om, ex, r), 0)
                x, y = v[i], v[i | d]
                v[i] = x + y
                v[i | d] = lf.mont((x - y) * w)
            nodes.append(list(v))
        if mul and k + 1 < len(plan):  # the twist: w^(column * rev_S(row))
            for i in range(n):
                e, col = i >> t0, i & ((1 << t0) - 1)
                v[i] = lf.mont(v[i] * lf.rep(pow(om, col * _rev(e, stages), r)))
            nodes.append(list(v))
        elif mul:  # a post table: any factor in (-r/2, 3r/2) serves the bound; this one is g^rev(p)
            for i in range(n):
                v[i] = lf.mont(v[i] * lf.rep(pow(7, _rev(i, log_n), r)))
            nodes.append(list(v))
        t_hi = t0
    return v, nodes


def _input_bounds(rng, n, kind):
    if kind == "uniform":
        return [3] * n
    if kind == "rows":  # mat-vec row sums of 0 .. 40 terms, some rows empty
        return [3 * (rng.below(41) if rng.below(4) else 0) for _ in range(n)]
    return [3 * 1000 if i % 16 == 5 else 3 for i in range(n)]  # one heavy stride class


@pytest.mark.parametrize("fid", [1, 3], ids=["Fr28", "BnFr28"])
@pytest.mark.parametrize("name", list(PLANS))
def test_dif_bounds_dominate_an_integer_simulation(fid, name):
    lf, f = F28[fid], (wm.FR if fid == 1 else wm.BN_FR)
    plan = PLANS[name]
    log_n = sum(s for s, _ in plan)
    n, r = 1 << log_n, lf.p
    om = pow(lb.ntt_root(lf, log_n), -1, r)
    rng = lb.SplitMix64(0x3157 + fid + 16 * log_n)
    for kind in ("uniform", "rows", "class"):
        bound = _input_bounds(rng, n, kind)
        out_b, peak, _ = wm.dif_node_bounds(f, plan, bound)
        for trial in range(2):
            xs = [rng.below(r) for _ in range(n)]
            vals = []
            for x, h in zip(xs, bound):  # a representation with |v| <= h r / 2 (h = 0: the structural zero)
                k_max = (h * r // 2 - r) // r if h else 0
                v = lf.rep(x) + (rng.below(2 * k_max + 1) - k_max) * r if h >= 3 else 0
                assert 2 * abs(v) <= h * r
                vals.append(v)
                xs[len(vals) - 1] = lf.value(v)
            out, nodes = simulate_dif(lf, plan, vals, om, rng)
            # it is the transform: position p holds sum_i x_i om^(i rev(p)), times the post factor where the plan has one
            for p in (0, 1, n // 2 + 1, n - 1):
                want = sum(x * pow(om, i * _rev(p, log_n), r) for i, x in enumerate(xs)) % r
                if plan[-1][1]:
                    want = want * pow(7, _rev(p, log_n), r) % r
                assert lf.value(out[p]) == want, (name, kind, p)
            # the position-by-position bounds hold for the final vector, the peak for every stored node
            assert all(2 * abs(v) <= h * r for v, h in zip(out, out_b)), (name, kind)
            assert all(2 * abs(v) <= peak * r for vec in nodes for v in vec), (name, kind)
    # the class-sum closed form dominates the per-node peak, and a constant vector attains it within a factor 2
    h = 3 * 25
    _, peak, _ = wm.dif_node_bounds(f, plan, [h] * n)
    closed, _ = wm.dif_bound_uniform(f, plan, h)
    assert closed >= peak
    c = lf.rep(1) + 36 * r  # in [36 r, 37.5 r): |c| <= h r / 2
    assert 2 * c <= h * r
    _, nodes = simulate_dif(lf, plan, [c] * n, om, rng)
    attained = max(abs(v) for vec in nodes for v in vec)
    assert 2 * attained <= closed * r and 4 * attained >= closed * r, (name, closed, attained)


@pytest.mark.parametrize("log_n", [6, 8])
def test_dit_bounds_dominate_an_integer_simulation(log_n):
    """Forward transforms: y = tile[L1] * w, then x + y and x - y: one product's width per stage."""
    lf, f = F28[1], wm.FR
    n, r = 1 << log_n, lf.p
    om = lb.ntt_root(lf, log_n)
    rng = lb.SplitMix64(0xD17 + log_n)
    plan = [(log_n, False)]
    _, peak = wm.dit_node_bounds(f, plan, [3] * n)
    assert peak == 3 * (1 + log_n)
    for vec in ([lf.rep(rng.below(r)) for _ in range(n)], [lf.rep(r - 1)] * n):
        xs = [lf.value(v) for v in vec]
        v = [vec[_rev(i, log_n)] for i in range(n)]  # bit-reversed in, natural out
        worst = 0
        for t in range(log_n):
            d = 1 << t
            for i in range(n):
                if i & d:
                    continue
                w = lf.rep(pow(om, (i & (d - 1)) << (log_n - 1 - t), r))
                x, y = v[i], lf.mont(v[i | d] * w)
                v[i], v[i | d] = x + y, x - y
            worst = max(worst, max(abs(e) for e in v))
        for k in (0, 1, n - 1):
            assert lf.value(v[k]) == sum(x * pow(om, i * k, r) for i, x in enumerate(xs)) % r
        assert 2 * worst <= peak * r


def test_capacity_and_product_constants():
    """The constants of the model against the figures the sources quote: 2^28.1 r (BLS12-381) and 2^29.4 r (BN254) of limb
    capacity (ntt.hip), and R r / 2 = 2^24.1 r^2 of product budget (field28.hpp's condition) for Fr28."""
    import math

    assert abs(math.log2(wm.FR.capacity() / 2) - 28.14) < 0.01
    assert abs(math.log2(wm.BN_FR.capacity() / 2) - 29.40) < 0.01
    assert wm.FR.fits(wm.FR.capacity()) and not wm.FR.fits(wm.FR.capacity() + 1)
    # 3r/2 times 2^23.5 r is inside the condition, times 2^23.6 r is not
    assert wm.FR.prod_ok(3, int(2 * 2**23.5)) and not wm.FR.prod_ok(3, int(2 * 2**23.6))
    assert wm.FR.prod(3, 3) == 3 and wm.FR.prod(0, 3) == 0
    # beyond the condition the result is still bounded: capacity times a twiddle stays below 16 r
    assert 3 < wm.FR.prod(wm.FR.capacity(), 3) < 32


# ---- the key-build verdict ----------------------------------------------------------------------------------------------
def _lib_verdict(zk, log_n, n_pub, rowptrs):
    rps = [np.ascontiguousarray(rp, dtype=np.uint32) for rp in rowptrs]
    nc = len(rps[0]) - 1
    mask = C.c_uint32(0xFF)
    bound = (C.c_double * 3)()
    rc = zk.tlib.zkmi_selftest_witness_bound(C.c_uint32(log_n), C.c_uint32(n_pub), C.c_uint32(nc),
                                             rps[0].ctypes.data_as(C.c_void_p), rps[1].ctypes.data_as(C.c_void_p),
                                             rps[2].ctypes.data_as(C.c_void_p), C.byref(mask), bound)
    assert rc == 0
    return mask.value, list(bound)


def _uniform(rows, k):
    return np.arange(rows + 1, dtype=np.int64) * k


def _update_note_rowptrs(zk, lg):
    r1 = zk.update_note_r1cs(lg, 1)
    assert r1.log_n == lg
    out = r1.n_pub, [np.array(r1.export(m)[0], dtype=np.int64) for m in range(3)]
    r1.free()
    return out


GRID = [
    # name, log_n, n_pub, rows, terms per row (A, B, C), must the verdict be "nothing normalised"
    ("bench 2^20", 20, 7, (1 << 20) - 7, (3, 3, 3), True),
    ("2^22 x 3", 22, 7, (1 << 22) - 7, (3, 3, 3), True),
    ("2^22 x 40", 22, 7, (1 << 22) - 7, (40, 40, 1), None),
    ("2^22 x 150", 22, 7, (1 << 22) - 7, (150, 2, 150), None),
    ("2^24 x 8", 24, 7, (1 << 24) - 7, (8, 8, 8), None),
    ("2^24 x 40", 24, 7, (1 << 24) - 7, (40, 1, 40), None),
]


@pytest.mark.parametrize("case", GRID, ids=[g[0] for g in GRID])
def test_verdict_matches_the_model_on_a_grid_of_shapes(zk, case):
    """The library's verdict (which matrices a key normalises, and the bound it computed) equals the model's on every shape.
    The model's verdict is the WORST case -- 3r/2 for every term of every row, all of one sign -- not what an assignment would
    reach: the key is built before any assignment exists."""
    _, log_n, n_pub, rows, terms, none = case
    rps = [_uniform(rows, k) for k in terms]
    want_mask, want_bounds = wm.verdict(log_n, n_pub, rps)
    mask, bounds = _lib_verdict(zk, log_n, n_pub, rps)
    assert mask == want_mask, (case[0], mask, want_mask)
    assert bounds == [b / 2 for b in want_bounds]
    if none:
        assert mask == 0
    cap = wm.FR.capacity()
    assert all(((mask >> m) & 1) == (want_bounds[m] > cap) for m in range(3))


def test_verdict_expected_flags():
    """What the model itself says about the grid, from the capacity alone: 2^28.14 r / (3r/2) = 1.98 10^8 terms."""
    cap_terms = wm.FR.capacity() // 3
    assert 197_000_000 < cap_terms < 198_000_000
    for _, log_n, n_pub, rows, terms, _ in GRID:
        mask, _ = wm.verdict(log_n, n_pub, [_uniform(rows, k) for k in terms])
        want = sum(1 << m for m, k in enumerate(terms) if rows * k + (n_pub if m == 0 else 0) > cap_terms)
        assert mask == want, (log_n, terms)


@pytest.mark.parametrize("lg", [13, 14])
def test_verdict_update_note(zk, lg):
    n_pub, rps = _update_note_rowptrs(zk, lg)
    mask, bounds = _lib_verdict(zk, lg, n_pub, rps)
    want_mask, want_bounds = wm.verdict(lg, n_pub, rps)
    assert mask == want_mask == 0 and bounds == [b / 2 for b in want_bounds]


def test_verdict_one_stride_class_of_a_two_pass_plan(zk):
    """2^20 runs two passes: only the rows of one stride class i mod 2^10 add up before the twist.  1 024 rows of 2^18 terms in
    ONE class (2^28 terms: over capacity) against the same rows spread over all classes (2^18 terms each: far inside)."""
    log_n, n_pub, rows = 20, 1, (1 << 20) - 1
    lens_one = np.zeros(rows, dtype=np.int64)
    lens_one[5 :: 1 << 10] = 1 << 18
    assert int((lens_one > 0).sum()) == 1024
    lens_spread = np.zeros(rows, dtype=np.int64)
    lens_spread[:1024] = 1 << 18
    c = _uniform(rows, 1)
    for lens, want in ((lens_one, 1), (lens_spread, 0)):
        rp = np.concatenate([[0], np.cumsum(lens)])
        for m in range(3):  # the heavy matrix in each place
            rps = [rp if k == m else c for k in range(3)]
            mask, bounds = _lib_verdict(zk, log_n, n_pub, rps)
            want_mask, want_bounds = wm.verdict(log_n, n_pub, rps)
            assert mask == want_mask == (want << m), (m, mask, want_mask)
            assert bounds == [b / 2 for b in want_bounds]


@pytest.mark.parametrize("log_n,count_pub", [(22, True), (22, False), (20, True)])
def test_verdict_one_term_apart(zk, log_n, count_pub):
    """A shape whose worst-case coherent sum is the last that fits, and the same shape with ONE more term: the model flips
    between them, and the library is never more permissive than the model (it rounds r up in its 64-bit comparison, so it
    may flip at most a few parts in 2^62 earlier: not on these shapes).  With count_pub the last terms that fit are A's
    instance rows, so a bound that ignored n_pub -- or one that counted rows instead of terms -- lands on the wrong side."""
    cap_terms = wm.FR.capacity() // 3
    n_pub = 1000 if count_pub else 1
    classes = 1 << wm.dif_first_pass_classes(log_n)[0]
    rows = (1 << log_n) - n_pub
    # all terms in the rows of class 0; the instance rows of A follow the constraint rows and are dealt over the classes too
    pub_in_class = sum(1 for i in range(rows, rows + n_pub) if i % classes == 0)
    lens = np.zeros(rows, dtype=np.int64)
    in_class = np.arange(0, rows, classes)
    budget = cap_terms - pub_in_class
    lens[in_class] = budget // len(in_class)
    lens[in_class[: budget % len(in_class)]] += 1
    c = _uniform(rows, 1)
    for extra, want in ((0, 0), (1, 1)):
        lens2 = lens.copy()
        lens2[0] += extra
        rp = np.concatenate([[0], np.cumsum(lens2)])
        rps = [rp, c, c]
        want_mask, want_bounds = wm.verdict(log_n, n_pub, rps)
        assert want_mask == want and want_bounds[0] == 3 * (cap_terms + extra)
        mask, bounds = _lib_verdict(zk, log_n, n_pub, rps)
        assert mask | want_mask == mask, "the library is more permissive than the model"
        assert mask == want_mask and bounds[0] == want_bounds[0] / 2
