"""The group law between the field and the MSM at its representation bounds, without a GPU.
Part 1: the big-integer model of tests/group28.py against the affine group law of the oracles on real points, the exceptional
cases included.  Part 2: the coordinate classes are closed and every vector lies inside them.  Part 3: every
host-callable op of zkmi_selftest_group_ops (ctx == NULL: the bodies the kernels run, compiled for the host) with exact
integer equality to the model."""
import numpy as np
import pytest

import group28 as g
import limbs28 as lb

CURVE_IDS = [c.name for c in g.CURVES]
HOST_CASES = [(c, op) for c in g.CURVES for op in g.OPS if g.host_has(c, op)]
NO_HOST_CASES = [(c, op) for c in g.CURVES for op in g.OPS if not g.host_has(c, op)]


def _ids(cases):
    return ["%s-%s" % (c.name, op) for c, op in cases]


# ---- part 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", g.CURVES, ids=CURVE_IDS)
def test_model_is_the_group_law_on_real_points(curve):
    """64 pairs (P, Q) per curve -- Q another point, P, -P, infinity (zeros, and ZZ = ZZZ = p), P itself at infinity, both --
    in varying representations and scalings: every body of the model, taken to affine, against the oracle's chord and tangent."""
    m = g.Model(curve)
    pts = g.points(curve)
    rng = lb.SplitMix64(0x0AC1E + curve.id)
    zero = m.zero()
    for i in range(64):
        P, other = pts[i % 12], pts[12 + i % 11]
        case = i % 8
        Q = [other, P, curve.neg(P), None, other, None, other, P][case]
        if case in (4, 5):
            P = None
        lam, mu = g._lam(curve, rng, i), g._lam(curve, rng, i + 1)

        def xyzz(pt, l, rep):
            if pt is None:
                if rep % 2:
                    return [zero, zero, zero, zero]
                fin = g._lift_point(curve, g.xyzz_of(curve, pts[rep % 5], l), g.POINT, rep)
                return [fin[0], fin[1], (curve.f.p,) * curve.ext, (0,) * curve.ext]
            return g._lift_point(curve, g.xyzz_of(curve, pt, l), g.POINT, rep)

        a, o = xyzz(P, lam, i // 8), xyzz(Q, mu, i // 8 + 1)
        want = curve.add(P, Q)
        assert m.to_affine(m.add_complete(tuple(a), tuple(o))) == want, (i, "add")
        assert m.to_affine(m.quad_add(tuple(a), tuple(o))) == want, (i, "quad")
        if P is not None:
            assert m.to_affine(m.dbl_inplace(tuple(a))) == curve.add(P, P), (i, "dbl")
        q_aff = [zero, zero] if Q is None else g._lift_point(curve, g.aff_of(curve, Q), g.AFFINE, i // 8)
        assert m.to_affine(m.madd_complete(tuple(a), tuple(q_aff))) == want, (i, "madd")
        if P is None or Q is None:
            continue
        # the bodies of the accumulation kernels: the sum where they return true, false exactly for Q = +-P
        for neg in (False, True):
            signed = curve.neg(Q) if neg else Q
            acc, ok = m.madd_generic(tuple(a), tuple(q_aff), neg)
            assert ok == (case not in (1, 2, 7)), (i, "madd_generic")
            if ok:
                assert m.to_affine(acc) == curve.add(P, signed)
            p_aff = g._lift_point(curve, g.aff_of(curve, P), g.AFFINE, i // 8 + 2)
            acc, ok = m.madd_affine_pair((p_aff[0], p_aff[1], zero, zero), tuple(q_aff), neg)
            assert ok == (case not in (1, 2, 7)), (i, "madd_affine_pair")
            if ok:
                assert m.to_affine(acc) == curve.add(P, signed)
        acc, ok = m.add_generic(tuple(a), tuple(o))
        assert ok == (case not in (1, 2, 7)) and (not ok or m.to_affine(acc) == want), (i, "add_generic")


@pytest.mark.parametrize("curve", g.CURVES, ids=CURVE_IDS)
def test_model_chain_is_the_signed_sum(curve):
    """The chains of real points: the sum of the signed entries before the one that meets it, as the oracle adds them; where
    the pair step itself returns false (flag 1), the first entry with its sign applied and ZZ = ZZZ = 0."""
    tuples, signs, flags = g.chain_tuples(curve)
    pts, got_flags = g.expected(curve, "chain", "chain", tuples, signs)[:2]
    m = g.Model(curve)
    met = {1: 0, 7: 0}
    for t, s, want, pt, fl in zip(tuples, signs, flags, pts, got_flags):
        if want is None:
            continue
        assert fl == want
        if want == 1:
            assert pt == (t[0], m.neg(t[1]) if s[0] else t[1], m.zero(), m.zero())
        else:
            acc = None
            for k in range(want):
                q = tuple(tuple(curve.f.value(v) for v in co) for co in (t[2 * k], t[2 * k + 1]))
                acc = curve.add(acc, curve.neg(q) if s[k] else q)
            assert m.to_affine(pt) == acc
        met[want] += 1
    assert met == {1: 2, 7: 3}  # positions 9, 41 and 5, 37, 69: one of each in every 32 chains


# ---- part 2 -------------------------------------------------------------------------------------------------------------
def test_classes_are_closed():
    assert g.closure_violations() == []
    # ... and no wider than needed: some producer reaches each end of every class
    for c in g.POINT:
        assert g._union(*(out[c] for out in g.OUT.values())) == g.CLASSES[c], c
    for c in g.AFFINE:
        assert g.ENTRY[c] == g.CLASSES[c], c


@pytest.mark.parametrize("curve", g.CURVES, ids=CURVE_IDS)
def test_vectors_stay_inside_the_classes_and_reach_their_ends(curve):
    for op in g.OPS:
        if op == "chain":
            tuples = g.chain_tuples(curve)[0]
        else:
            tuples = g.generic_tuples(curve, op) + g.exceptional_tuples(curve, op)[0]
        assert 0 < len(tuples) <= 1 << 15
        g.check_inputs(curve, op, tuples)
        for j, cls in enumerate(g.IN[op][:8]):
            lo, hi = g.ends(curve.f, cls)
            seen = {v for t in tuples for v in t[j]}
            assert lo in seen and hi in seen, (op, j, cls)


@pytest.mark.parametrize("curve", g.CURVES, ids=CURVE_IDS)
def test_model_holds_its_conditions_at_the_class_ends(curve):
    """Every op over all its vectors in the model alone: the column condition at every reduction, |v| <= 4 p at every
    is_zero(), lazy differences into products only, the promised class at every output (asserted inside expected()); the
    exceptional vectors take the branches they were built for; and every body that returns a flag met a square that is zero
    but held as p, not 0."""
    budget = 0
    for op in g.OPS:
        if op == "chain":
            tuples, signs, _ = g.chain_tuples(curve)
            _, flags, b, kp_zeros = g.expected(curve, op, "chain", tuples, signs)
            budget = max(budget, b)
            assert kp_zeros > 0 and {1, 7, 0xFF} <= set(flags), (op, kp_zeros, set(flags))
            continue
        budget = max(budget, g.expected(curve, op, "generic", g.generic_tuples(curve, op))[2])
        tuples, what = g.exceptional_tuples(curve, op)
        pts, flags, b, kp_zeros = g.expected(curve, op, "exceptional", tuples)
        budget = max(budget, b)
        if g.has_flag(op):  # is_zero() is read on P^2 alone there
            assert kp_zeros > 0, op
        for t, w, pt, fl in zip(tuples, what, pts, flags):
            if fl is not None:
                assert fl == (1 if w == "sum" else 0), (op, w)
            elif w == "opposite" or w == "inf_both":
                assert all(v % curve.f.p == 0 for v in pt[2]), (op, w)
            elif w == "inf_o":
                assert pt == tuple(t[0:4]), (op, w)
            elif w == "inf_a" and op not in ("dbl", "madd_complete"):
                assert pt == tuple(t[4:8]), (op, w)
    # sum |a| |b| of one reduction, in p^2: below what the classes allow, and that below the limit
    # R / (2 p) (1260 for Fq28)
    assert budget < g.COLUMN_BOUND[curve.ext]
    assert g.COLUMN_BOUND[curve.ext] < curve.f.R // (2 * curve.f.p)


# ---- part 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,op", HOST_CASES, ids=_ids(HOST_CASES))
def test_host_op_equals_the_model(zk, curve, op):
    if op == "chain":
        tuples, signs, _ = g.chain_tuples(curve)
        out, flag = g.check(zk, None, curve, op, "chain", tuples, signs)
    else:
        signs = None
        tuples = g.generic_tuples(curve, op)
        out, flag = g.check(zk, None, curve, op, "generic", tuples)
        exc = g.exceptional_tuples(curve, op)[0]
        g.check(zk, None, curve, op, "exceptional", exc)
    one, flag1 = g.call(zk, None, curve, op, g.block_of(curve, tuples[:1], None if signs is None else signs[:1]))
    assert np.array_equal(one, out[:1])
    if g.has_flag(op):
        assert flag1[0] == flag[0]


@pytest.mark.parametrize("curve,op", NO_HOST_CASES, ids=_ids(NO_HOST_CASES))
def test_host_path_refuses_the_lane_exchange_forms(zk, curve, op):
    tuples = g.chain_tuples(curve) if op == "chain" else (g.generic_tuples(curve, op)[:1], None)
    g.call(zk, None, curve, op, g.block_of(curve, tuples[0][:1], None if tuples[1] is None else tuples[1][:1]), expect_rc=-1)


def test_hook_refuses_what_it_does_not_have(zk):
    curve = g.CURVES[0]
    block = g.block_of(curve, g.generic_tuples(curve, "dbl")[:1])
    out = np.zeros(4 * curve.W, dtype=np.int32)
    f = zk.tlib.zkmi_selftest_group_ops
    assert f(None, 3, 7, 1, block.ctypes.data, out.ctypes.data, None) == -1  # no such curve
    assert f(None, 0, 11, 1, block.ctypes.data, out.ctypes.data, None) == -1  # no such op
    assert f(None, 0, -1, 1, block.ctypes.data, out.ctypes.data, None) == -1
    assert f(None, 0, 7, 0, block.ctypes.data, out.ctypes.data, None) == -1  # no tuples
    assert f(None, 0, 7, 1, None, out.ctypes.data, None) == -1
    assert f(None, 0, 7, 1, block.ctypes.data, None, None) == -1
    assert f(None, 0, 7, 1, block.ctypes.data, out.ctypes.data, None) == 0  # dbl writes no flag
    assert f(None, 0, 0, 1, block.ctypes.data, out.ctypes.data, None) == -1  # madd_generic does
