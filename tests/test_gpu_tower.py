"""The gfx950 compilation of the pairing tower (zk-apps_amd/csrc/pairing_dev.hip) at its magnitude bounds: every op of
zkmi_selftest_tower_ops on the DEVICE -- one tuple per lane pair over Fq2P, the product's types and launch shape -- against
the big integers of tests/tower28.py, and its residues against the host path's (Fq2_28).  The operands are those of
test_cpu_tower.py: every residue at the ends of the interval zkmi_selftest_tower_bounds reports for its class, never beyond.
Tuple counts cross a wave: 31, 32 and 33 lane pairs, and the capped vector set."""
import ctypes as C

import numpy as np
import pytest

import tower28 as tw

pytestmark = pytest.mark.gpu
P = tw.P

GENERIC = ("shrink", "e2_mul_xi", "e2_conj", "e2_inv", "e6_mul", "e12_sqr", "e12_mul", "e12_mul_line", "e12_conj", "e12_frob_p",
           "e12_frob_p2", "e6_inv", "e12_inv", "words_round_trip")
CAPS = {"e2_inv": 128, "e6_inv": 96, "e12_inv": 96}


@pytest.fixture(scope="module")
def classes(zk):
    return tw.bounds(zk)[1]


def _both(zk, ctx, op, classes, tuples):
    """Device against the reference, and its residues against the host path's."""
    _, dev = tw.run_generic(zk, ctx, op, classes, tuples=tuples)
    host = tw.call(zk, None, op, tw.block_of(tuples))
    if op == "words_round_trip":
        assert np.array_equal(dev, host)  # canonical words and an exact product: one answer
    else:
        assert tw.residues_equal(dev, host), op
    return dev


@pytest.mark.parametrize("op", GENERIC)
def test_device_op(zk, ctx, classes, op):
    tuples = tw.generic_tuples(op, classes, CAPS.get(op, 512))
    dev = _both(zk, ctx, op, classes, tuples)
    # a last wave with one lane pair, a full wave, and one pair less: the same tuples give the same words
    for n in (33, 32, 31):
        part = tw.call(zk, ctx, op, tw.block_of(tuples[:n]))
        assert np.array_equal(part, dev[:n]), (op, n)


@pytest.mark.parametrize("op", ["e12_mul", "e12_inv"])
def test_device_coefficients_that_are_zero_but_held_as_multiples_of_p(zk, ctx, classes, op):
    _both(zk, ctx, op, classes, tw.zero_held_tuples(op, classes))


def test_device_words_of_multiples_of_p(zk, ctx, classes):
    tuples = [(k * P + d,) for k in range(-2, 3) for d in (0, 1, -1) if abs(k * P + d) <= 2 * P]
    raw = _both(zk, ctx, "words_round_trip", classes, tuples)
    assert not raw[[i for i, t in enumerate(tuples) if t[0] % P == 0], :12].any()


@pytest.mark.parametrize("op", ["e2_inv", "e6_inv", "e12_inv"])
def test_device_inversions_of_zero_and_one(zk, ctx, classes, op):
    tuples = tw.inv_special_tuples(op, classes)
    outs = tw.ints_of(_both(zk, ctx, op, classes, tuples))
    assert all(v % P == 0 for v in outs[0] + outs[1] + outs[2])
    assert tw.vals(outs[3])[0] == 1 and not any(tw.vals(outs[3])[1:])


@pytest.mark.parametrize("op", ["e12_sqr", "e12_inv"])
def test_device_subfield_elements(zk, ctx, classes, op):
    _both(zk, ctx, op, classes, tw.subfield_tuples(classes))


def test_device_is_one(zk, ctx, classes):
    tuples, want = tw.is_one_tuples(classes)
    assert (2 * len(tuples)) % 64 != 0
    block = tw.block_of(tuples)
    got = tw.call(zk, ctx, "is_one", block, flag=True)
    bad = [(i, int(g), w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]
    assert np.array_equal(got, tw.call(zk, None, "is_one", block, flag=True))


@pytest.mark.parametrize("op", ["step_tangent", "step_chord"])
def test_device_steps(zk, ctx, classes, op):
    _both(zk, ctx, op, classes, tw.step_tuples(op, classes))


def test_device_miller_rounds(zk, ctx, classes):
    """8 tuples against the oracle (after its final exponentiation: the line factors differ), 33 against the host path."""
    tuples = tw.miller_tuples(classes, 33)
    dev = tw.call(zk, ctx, "miller_rounds", tw.block_of(tuples))
    tw.check("miller_rounds", tuples[:8], tw.ints_of(dev[:8]), classes)
    assert all(tw.is_shrunk(v) for row in tw.ints_of(dev) for v in row)
    assert tw.residues_equal(dev, tw.call(zk, None, "miller_rounds", tw.block_of(tuples)))


def test_device_final_exp_chain(zk, ctx, classes):
    """8 tuples against the oracle's f12_pow, the subfield elements, and 64 more against out_plain of
    zkmi_selftest_final_exp_formulas, the host's unchanged square-and-multiply."""
    gen = tw.generic_tuples("final_exp_chain", classes, cap=130)
    tuples = gen[:3] + gen[-2:] + tw.subfield_tuples(classes)[::4] + gen[66:130]
    dev = tw.call(zk, ctx, "final_exp_chain", tw.block_of(tuples))
    outs = tw.ints_of(dev)
    tw.check("final_exp_chain", tuples[:8], outs[:8], classes)
    assert all(tw.vals(r) == [1] + [0] * 11 for r in outs[5:8])
    chain, plain = (C.c_uint8 * 576)(), (C.c_uint8 * 576)()
    for t, got in zip(tuples[8:], outs[8:]):
        f = tw.tower_bytes(tw.vals(t))
        rc = zk.tlib.zkmi_selftest_final_exp_formulas((C.c_uint8 * 576).from_buffer_copy(f), chain, plain)
        assert rc == 0 and tw.tower_bytes(tw.vals(got)) == bytes(plain)
        assert all(tw.is_shrunk(v) for v in got)
    assert tw.residues_equal(dev, tw.call(zk, None, "final_exp_chain", tw.block_of(tuples)))
