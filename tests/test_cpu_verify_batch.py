"""CPU suite for the host side of batch verification: the prepared verifying key (zkmi_vk_prepare validates exactly what
zkmi_groth16_verify validates at every call), and the Miller-loop formulas the device kernel runs (csrc/pairing_dev.hip),
instantiated over the host field types by the testing library and held to the host pairing."""
import ctypes as C

import pytest

from conftest import golden
from oracle import bls12_381 as ec

H = bytes.fromhex
N_PUB = 7


def _buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(b)


def _prepare_rc(zk, vk, n_pub=N_PUB):
    h = C.c_void_p()
    rc = zk.lib.zkmi_vk_prepare(_buf(vk), C.c_uint32(n_pub), C.byref(h))
    if rc == 0:
        assert h.value
        assert zk.lib.zkmi_vk_free(h) == 0
    else:
        assert not h.value
    return rc


def test_vk_prepare_accepts_the_golden_key(zk):
    vk = H(golden("groth16_n128.json")["vk"])
    assert len(vk) == 672 + 96 * N_PUB
    assert _prepare_rc(zk, vk) == 0
    pv = zk.vk_prepare(vk)
    assert pv.n_pub == N_PUB
    pv.free()


def test_vk_prepare_refuses_what_the_verifier_refuses(zk, pkg):
    gd = golden("groth16_n128.json")
    vk, proof = H(gd["vk"]), H(gd["proof"])
    publics = H(gd["witness"])[32 : 32 * N_PUB]

    def verify_rc(key):
        return zk.lib.zkmi_groth16_verify(_buf(key), C.c_uint32(N_PUB), _buf(publics), _buf(proof))

    assert verify_rc(vk) == 0
    # a G2 curve point outside the subgroup, found as test_verifier_rejects_non_canonical_and_small_order_points finds it
    off = None
    for x in range(1, 200):
        enc = bytearray(bytes(48) + x.to_bytes(48, "big"))
        enc[0] |= 0x80
        try:
            aff = zk.g2_decompress(bytes(enc))
        except pkg.ZkmiError:
            continue
        if not zk.g2_in_subgroup(aff):
            off = aff
            break
    assert off is not None
    bad_delta = vk[:480] + off + vk[672:]
    # one gamma_abc coordinate >= p
    bad_ic = bytearray(vk)
    bad_ic[672 + 96 * 3 + 48 : 672 + 96 * 3 + 96] = (ec.P + 5).to_bytes(48, "little")
    # alpha off the curve
    bad_alpha = bytearray(vk)
    bad_alpha[0] ^= 1
    for key in (bad_delta, bytes(bad_ic), bytes(bad_alpha)):
        assert verify_rc(key) == -2
        assert _prepare_rc(zk, key) == -2
        with pytest.raises(pkg.ZkmiError) as e:
            zk.vk_prepare(key)
        assert e.value.code == -2


def test_vk_prepare_bad_arguments(zk):
    vk = H(golden("groth16_n128.json")["vk"])
    h = C.c_void_p()
    assert zk.lib.zkmi_vk_prepare(None, C.c_uint32(N_PUB), C.byref(h)) == -1
    assert zk.lib.zkmi_vk_prepare(_buf(vk), C.c_uint32(N_PUB), None) == -1
    assert zk.lib.zkmi_vk_prepare(_buf(vk), C.c_uint32(0), C.byref(h)) == -1
    assert zk.lib.zkmi_vk_free(None) == -1


def test_device_miller_formulas_match_the_host_pairing(zk):
    """Jacobian steps, scaled sparse lines, complex squaring and the merged 68-round loop of the device kernel, run over
    the host's Fq2: equal to zkmi_pairing after the final exponentiation (which test_pairing_matches_oracle holds to the
    oracle), infinity included."""
    g1, g2 = zk.g1_generator(), zk.g2_generator()
    cases = [(g1, g2)]
    for a, b in ((3, 5), (0xDEADBEEF12345, 0x1234567890ABCDEF0123)):
        cases.append((zk.g1_mul(g1, a.to_bytes(32, "little")), zk.g2_mul(g2, b.to_bytes(32, "little"))))
    cases += [(bytes(96), g2), (g1, bytes(192))]
    for p, q in cases:
        out = (C.c_uint8 * 576)()
        assert zk.tlib.zkmi_selftest_miller_formulas(_buf(p), _buf(q), out) == 0
        assert bytes(out) == zk.pairing(p, q)
    one = (1).to_bytes(48, "little") + bytes(528)
    assert zk.pairing(bytes(96), g2) == one
