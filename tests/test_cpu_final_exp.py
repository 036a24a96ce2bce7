"""CPU suite: the final-exponentiation chain the device runs (csrc/pairing_dev.hip final_exp_chain: easy part with a tower
inversion, the hard part as ((x-1)^2/3) (x+p) (x^2+p^2-1) + 1 with the p and p^2 Frobenius maps) instantiated over the HOST
field types, against the unchanged square-and-multiply final_exponentiation and against oracle/bls12_381.py.  Pins the
Frobenius constants and the exponent identity without a GPU."""
import ctypes as C
import random

from conftest import golden
from oracle import bls12_381 as ec

ONE = (1).to_bytes(48, "little") + bytes(528)


def _buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(bytes(b))


def _tower_to_poly(gt):
    """576 bytes in the tower basis -> the oracle's Fq[w]/(w^12 - 2w^6 + 2): u = w^6 - 1, v = w^2."""
    co = [int.from_bytes(gt[48 * i : 48 * i + 48], "little") for i in range(12)]
    poly = [0] * 12
    idx = 0
    for i in range(2):
        for j in range(3):
            for u in range(2):
                c = co[idx]
                idx += 1
                e = 2 * j + i
                if u == 0:
                    poly[e] = (poly[e] + c) % ec.P
                else:
                    poly[e + 6] = (poly[e + 6] + c) % ec.P
                    poly[e] = (poly[e] - c) % ec.P
    return poly


def _poly_to_tower(poly):
    """The inverse map: coefficient of v^j w^i is (poly[e] + poly[e + 6]) + poly[e + 6] u with e = 2 j + i."""
    out = b""
    for i in range(2):
        for j in range(3):
            e = 2 * j + i
            out += ((poly[e] + poly[e + 6]) % ec.P).to_bytes(48, "little") + (poly[e + 6] % ec.P).to_bytes(48, "little")
    return out


def _both(zk, f):
    chain, plain = (C.c_uint8 * 576)(), (C.c_uint8 * 576)()
    rc = zk.tlib.zkmi_selftest_final_exp_formulas(_buf(f), chain, plain)
    return rc, bytes(chain), bytes(plain)


def _random_fq12(rnd):
    return b"".join(rnd.randrange(ec.P).to_bytes(48, "little") for _ in range(12))


def test_chain_equals_the_plain_exponentiation_on_random_elements(zk):
    rnd = random.Random(901)
    seen = set()
    for k in range(12):
        f = _random_fq12(rnd)
        rc, chain, plain = _both(zk, f)
        assert rc == 0
        assert chain == plain
        assert chain != ONE
        seen.add(chain)
        if k < 3:  # the oracle's own final exponentiation on the same element
            assert _tower_to_poly(f) == _tower_to_poly(_poly_to_tower(_tower_to_poly(f)))
            assert ec.final_exponentiation(_tower_to_poly(f)) == _tower_to_poly(chain)
    assert len(seen) == 12


def test_one_and_base_field_elements_go_to_one(zk):
    assert _both(zk, ONE) == (0, ONE, ONE)
    rnd = random.Random(902)
    for _ in range(2):
        f = rnd.randrange(1, ec.P).to_bytes(48, "little") + bytes(528)  # Fq inside Fq12: killed by p^6 - 1
        assert _both(zk, f) == (0, ONE, ONE)
    # an Fq2 element as well (a^(p^6 - 1) = 1 for every a in a proper subfield of even degree)
    f = rnd.randrange(1, ec.P).to_bytes(48, "little") + rnd.randrange(1, ec.P).to_bytes(48, "little") + bytes(480)
    assert _both(zk, f) == (0, ONE, ONE)


def test_an_element_of_gt_is_raised_like_the_plain_path(zk):
    pg = golden("pairing.json")
    gt = zk.pairing(ec.g1_to_bytes(ec.g1_mul(pg["a"])), ec.g2_to_bytes(ec.g2_mul(pg["b"])))
    rc, chain, plain = _both(zk, gt)
    assert rc == 0 and chain == plain and chain != ONE
    assert ec.final_exponentiation(_tower_to_poly(gt)) == _tower_to_poly(chain)


def test_a_miller_value_of_the_oracle_becomes_the_pairing(zk):
    rnd = random.Random(903)
    a, b = rnd.randrange(1, ec.R), rnd.randrange(1, ec.R)
    p, q = ec.g1_mul(a), ec.g2_mul(b)
    m = ec.miller_loop(p, q)
    f = _poly_to_tower(m)
    assert _tower_to_poly(f) == [c % ec.P for c in m]
    rc, chain, plain = _both(zk, f)
    assert rc == 0 and chain == plain
    assert _tower_to_poly(chain) == ec.final_exponentiation(m)
    # the library's own Miller formulas (Jacobian T, scaled lines) end in the same bytes through the plain path
    out = (C.c_uint8 * 576)()
    assert zk.tlib.zkmi_selftest_miller_formulas(_buf(ec.g1_to_bytes(p)), _buf(ec.g2_to_bytes(q)), out) == 0
    assert bytes(out) == zk.pairing(ec.g1_to_bytes(p), ec.g2_to_bytes(q))
    assert _tower_to_poly(bytes(out)) == _tower_to_poly(chain)


def test_refused_inputs(zk):
    rnd = random.Random(904)
    chain, plain = (C.c_uint8 * 576)(), (C.c_uint8 * 576)()
    f = bytearray(_random_fq12(rnd))
    for k in (0, 7, 11):
        g = bytearray(f)
        g[48 * k : 48 * k + 48] = (ec.P + k).to_bytes(48, "little")
        assert _both(zk, g)[0] == -2  # ZKMI_ERR_NON_CANONICAL
    assert _both(zk, bytes(576))[0] == -1  # zero has no inverse: ZKMI_ERR_BAD_ARG
    assert zk.tlib.zkmi_selftest_final_exp_formulas(None, chain, plain) == -1
    assert zk.tlib.zkmi_selftest_final_exp_formulas(_buf(f), None, plain) == -1
    assert zk.tlib.zkmi_selftest_final_exp_formulas(_buf(f), chain, None) == -1


def test_the_two_entry_points_are_bound(zk):
    """The binding carries the new calls (their GPU behaviour: tests/test_gpu_verify_each.py)."""
    assert hasattr(zk.lib, "zkmi_pairing_batch_dev") and hasattr(zk.lib, "zkmi_groth16_verify_each")
    import importlib

    mod = importlib.import_module(type(zk).__module__)
    assert hasattr(mod.Context, "pairing_batch_dev") and hasattr(mod.Context, "groth16_verify_each")
