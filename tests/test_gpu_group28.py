"""The gfx950 compilation of the group law between the field and the MSM at its representation bounds: every op of
zkmi_selftest_group_ops on the DEVICE, in the lane layout the product's kernels use (one lane, a lane pair over Fq2P, a quad or
an octet per point), with exact integer equality to the big-integer model of tests/group28.py, and limb for limb equal to
the host path wherever both exist.  The vectors are those of test_cpu_group28.py: every coordinate in every representation of
its class, every combination of class ends, real points in the exceptional branches.  Tuple counts leave the last wave partly
filled for every layout, and n = 1 runs alone."""
import numpy as np
import pytest

import group28 as g

pytestmark = pytest.mark.gpu

CASES = [(c, op) for c in g.CURVES for op in g.OPS if op != "chain"]
CURVE_IDS = [c.name for c in g.CURVES]


def _vectors(curve, op):
    tuples = g.generic_tuples(curve, op)
    if len(tuples) % 16 == 0:  # points per wave: 64 lanes, 32 pairs, 16 quads, 8 octets
        tuples = tuples[:-1]
    return tuples


@pytest.mark.parametrize("curve,op", CASES, ids=["%s-%s" % (c.name, op) for c, op in CASES])
def test_device_op_equals_the_model(zk, ctx, curve, op):
    tuples = _vectors(curve, op)
    assert len(tuples) % 16
    out, flag = g.check(zk, ctx, curve, op, "generic-gpu", tuples)
    exc = g.exceptional_tuples(curve, op)[0]
    out_e, flag_e = g.check(zk, ctx, curve, op, "exceptional", exc)
    if g.host_has(curve, op):
        for t, o, f in ((tuples, out, flag), (exc, out_e, flag_e)):
            host, hflag = g.call(zk, None, curve, op, g.block_of(curve, t))
            assert np.array_equal(o, host), (curve.name, op)
            if g.has_flag(op):
                assert np.array_equal(f, hflag), (curve.name, op)
    # one tuple alone, and counts around a wave of every layout: the same tuples give the same words
    for n in (1, 7, 17, 33, 65):
        part, pflag = g.call(zk, ctx, curve, op, g.block_of(curve, exc[:n]))
        assert np.array_equal(part, out_e[:n]), (curve.name, op, n)
        if g.has_flag(op):
            assert np.array_equal(pflag, flag_e[:n]), (curve.name, op, n)


@pytest.mark.parametrize("curve", g.CURVES, ids=CURVE_IDS)
def test_quad_forms_agree_with_each_other_and_with_the_one_lane_addition(zk, ctx, curve):
    """The DPP form and the ds_bpermute form limb for limb; both against XYZZ::add as field elements, coordinate by coordinate
    (the quad form reduces Y3 in two reductions and multiplies ZZZ3 in another order: the same residue, not always the same
    representation -- each is pinned to its own model above)."""
    p = curve.f.p
    for tuples in (_vectors(curve, "add"), g.exceptional_tuples(curve, "add")[0]):
        block = g.block_of(curve, tuples)
        dpp, _ = g.call(zk, ctx, curve, "quad_dpp", block)
        bperm, _ = g.call(zk, ctx, curve, "quad_bpermute", block)
        one, _ = g.call(zk, ctx, curve, "add", block)
        assert np.array_equal(dpp, bperm)
        for i, (a, b) in enumerate(zip(g.points_of(curve, dpp), g.points_of(curve, one))):
            assert all((x - y) % p == 0 for ca, cb in zip(a, b) for x, y in zip(ca, cb)), (curve.name, i)


@pytest.mark.parametrize("curve", g.CURVES, ids=CURVE_IDS)
def test_device_chain_equals_the_model(zk, ctx, curve):
    tuples, signs, flags = g.chain_tuples(curve)
    assert len(tuples) % 32 and len(tuples) > 64
    out, flag = g.check(zk, ctx, curve, "chain", "chain", tuples, signs)
    for i, want in enumerate(flags):
        if want is not None:
            assert flag[i] == want  # one chain in every wave meets its negative (or itself) at step 7, one at the pair step
    if g.host_has(curve, "chain"):
        host, hflag = g.call(zk, None, curve, "chain", g.block_of(curve, tuples, signs))
        assert np.array_equal(out, host) and np.array_equal(flag, hflag)
    one, flag1 = g.call(zk, ctx, curve, "chain", g.block_of(curve, tuples[5:6], signs[5:6]))
    assert np.array_equal(one, out[5:6]) and flag1[0] == 7
    one, flag1 = g.call(zk, ctx, curve, "chain", g.block_of(curve, tuples[9:10], signs[9:10]))
    assert np.array_equal(one, out[9:10]) and flag1[0] == 1 and not one[0, 2 * curve.W:].any()
