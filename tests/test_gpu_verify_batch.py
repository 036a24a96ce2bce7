"""GPU suite for the pairing product on the device (csrc/pairing_dev.hip) and batch verification on top of it
(csrc/verify_batch.hip).  Exact bytes and verdicts: expected values come from oracle/bls12_381.py, oracle/groth16.py,
tests/points_corpus.py and the unchanged host verifier zkmi_groth16_verify, never from the code under test."""
import ctypes as C
import random

import pytest

import points_corpus as pc
from conftest import golden
from oracle import bls12_381 as ec
from oracle import groth16 as g16

pytestmark = pytest.mark.gpu

H = bytes.fromhex
ONE = (1).to_bytes(48, "little") + bytes(528)
NO_INDEX = (1 << 64) - 1
N = 130
FAULTS = (0, 64, 129)  # first lane, wave boundary, last lane


def _dev(b):
    import torch

    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _product(ctx, pairs):
    """zkmi_pairing_product_dev over oracle points (None = infinity)."""
    g1 = _dev(b"".join(ec.g1_to_bytes(p) for p, _ in pairs))
    g2 = _dev(b"".join(ec.g2_to_bytes(q) for _, q in pairs))
    return ctx.pairing_product_dev(g1.data_ptr(), g2.data_ptr(), len(pairs))


def _tower_to_poly(gt):
    """The 576 bytes of zkmi_pairing -> the oracle's Fq[w]/(w^12 - 2w^6 + 2) (as test_pairing_matches_oracle does)."""
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


# ---- pairing product ------------------------------------------------------------------------------------------------


def test_pairing_product_of_three_matches_the_oracle(ctx):
    rnd = random.Random(31)
    pairs = [(ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R))),
             (None, ec.g2_mul(rnd.randrange(1, ec.R))),
             (ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R)))]
    f = ec.f12_one()
    for p, q in pairs:
        f = ec.f12_mul(f, ec.miller_loop(p, q))
    assert _tower_to_poly(_product(ctx, pairs)) == ec.final_exponentiation(f)


def test_pairing_product_of_one_equals_the_host_pairing(ctx, zk):
    rnd = random.Random(32)
    for _ in range(2):
        p, q = ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R))
        assert _product(ctx, [(p, q)]) == zk.pairing(ec.g1_to_bytes(p), ec.g2_to_bytes(q))
    assert _product(ctx, [(ec.G1, None)]) == ONE
    assert ctx.pairing_product_dev(None, None, 0) == ONE


def test_pairing_product_bilinearity_across_a_wave(ctx):
    """67 pairs: more than one 64-lane wave, and an odd tail.  prod e(a_i G1, b_i G2) * e(-(sum a_i b_i) G1, G2) = 1."""
    rnd = random.Random(33)
    ab = [(rnd.randrange(1, 1 << 64), rnd.randrange(1, 1 << 64)) for _ in range(66)]
    pairs = [(ec.g1_mul(a), ec.g2_mul(b)) for a, b in ab]
    closing = (ec.g1_mul((-sum(a * b for a, b in ab)) % ec.R), ec.G2)
    assert _product(ctx, pairs + [closing]) == ONE
    for i in (0, 40, 65):
        moved = list(pairs)
        moved[i] = (ec.g1_mul(ab[i][0] + 1), pairs[i][1])
        assert _product(ctx, moved + [closing]) != ONE


# ---- batch verdicts -------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def batch(ctx, zk):
    """130 proofs of distinct witnesses of the N = 128 golden relation under the golden key."""
    import torch

    gd = golden("groth16_n128.json")
    lg = gd["log_n"]
    r1 = zk.shielder_r1cs(lg)
    pk, vk = ctx.groth16_setup(r1, H(gd["toxic"]))
    assert vk == H(gd["vk"])
    wits = [zk.shielder_witness(lg, 7000 + i) for i in range(N)]
    rng = ec.SplitMix64(4242)
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(N)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(N)]
    d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
    torch.cuda.synchronize()
    proofs = ctx.groth16_prove_batch_dev(pk, [t.data_ptr() for t in d], rs, ss)
    publics = [w[32 : 32 * r1.n_pub] for w in wits]
    assert len(set(publics)) == N and len(set(proofs)) == N
    pk.free()
    pv = zk.vk_prepare(vk)
    rnd = random.Random(77)
    weights = [rnd.randrange(1, 1 << 128).to_bytes(16, "little") for _ in range(N)]
    yield {"vk": vk, "pv": pv, "proofs": proofs, "publics": publics, "weights": weights, "n_pub": r1.n_pub}
    pv.free()
    r1.free()


def _verify(ctx, pv, publics, proofs, weights, want_status=True):
    """(return code, status bytes, first_bad) of zkmi_groth16_verify_batch."""
    n = len(proofs)
    buf = lambda b: (C.c_uint8 * max(1, len(b))).from_buffer_copy(b) if len(b) else (C.c_uint8 * 1)()
    st = (C.c_uint8 * max(1, n))(*([0xEE] * max(1, n)))
    bad = C.c_uint64(12345)
    rc = ctx.lib.zkmi_groth16_verify_batch(ctx.h, pv.h, C.c_uint64(n), buf(b"".join(publics)), buf(b"".join(proofs)),
                                           buf(b"".join(weights)) if weights is not None else None,
                                           st if want_status else None, C.byref(bad))
    return rc, bytes(st)[:n], bad.value


def test_batch_of_valid_proofs_is_accepted(ctx, zk, batch):
    pv, proofs, publics = batch["pv"], batch["proofs"], batch["publics"]
    for weights in (batch["weights"], None):
        rc, st, bad = _verify(ctx, pv, publics, proofs, weights)
        assert (rc, st, bad) == (0, bytes(N), NO_INDEX)
    assert _verify(ctx, pv, publics, proofs, None, want_status=False)[0] == 0
    assert ctx.groth16_verify_batch(pv, b"".join(publics), b"".join(proofs)) == (True, bytes(N), None)
    # the same proofs under the host verifier and the oracle
    for i in (0, 64, 129):
        assert zk.groth16_verify(batch["vk"], publics[i], proofs[i]) is True
    vk = batch["vk"]
    ovk = {"alpha_g1": ec.g1_from_bytes(vk[:96]), "beta_g2": ec.g2_from_bytes(vk[96:288]),
           "gamma_g2": ec.g2_from_bytes(vk[288:480]), "delta_g2": ec.g2_from_bytes(vk[480:672]),
           "gamma_abc_g1": [ec.g1_from_bytes(vk[672 + 96 * j : 768 + 96 * j]) for j in range(batch["n_pub"])]}
    pub = [int.from_bytes(publics[5][32 * j : 32 * j + 32], "little") for j in range(batch["n_pub"] - 1)]
    assert g16.verify(ovk, pub, g16.proof_from_bytes(proofs[5])) is True


def test_batch_of_one_and_of_none(ctx, batch):
    pv = batch["pv"]
    assert _verify(ctx, pv, batch["publics"][:1], batch["proofs"][:1], batch["weights"][:1]) == (0, b"\x00", NO_INDEX)
    rc, _, bad = _verify(ctx, pv, [], [], [])
    assert (rc, bad) == (0, NO_INDEX)


def _expect(statuses):
    st = bytearray(N)
    for i, s in statuses.items():
        st[i] = s
    return bytes(st)


def test_swapped_c_is_localised(ctx, zk, batch):
    pv, publics, weights = batch["pv"], batch["publics"], batch["weights"]
    proofs = list(batch["proofs"])
    for i in FAULTS:
        proofs[i] = proofs[i][:144] + batch["proofs"][(i + 7) % N][144:]
        assert zk.groth16_verify(batch["vk"], publics[i], proofs[i]) is False
    rc, st, bad = _verify(ctx, pv, publics, proofs, weights)
    assert (rc, st, bad) == (-5, _expect({i: 5 for i in FAULTS}), 0)
    # without the status array the verdict alone
    assert _verify(ctx, pv, publics, proofs, weights, want_status=False)[0] == -5
    assert ctx.groth16_verify_batch(pv, b"".join(publics), b"".join(proofs), b"".join(weights)) == (False, st, 0)


def test_foreign_public_input_is_localised(ctx, batch):
    publics = list(batch["publics"])
    for i in FAULTS:
        publics[i] = batch["publics"][(i + 3) % N]
    rc, st, bad = _verify(ctx, batch["pv"], publics, batch["proofs"], batch["weights"])
    assert (rc, st, bad) == (-5, _expect({i: 5 for i in FAULTS}), 0)


def test_public_input_not_below_r_is_malformed(ctx, batch):
    publics = list(batch["publics"])
    for k, i in enumerate(FAULTS):
        p = bytearray(publics[i])
        p[32 * k : 32 * k + 32] = (ec.R + (0 if k == 0 else 1 << (8 * k))).to_bytes(32, "little")
        publics[i] = bytes(p)
    rc, st, bad = _verify(ctx, batch["pv"], publics, batch["proofs"], batch["weights"])
    assert (rc, st, bad) == (-2, _expect({i: 4 for i in FAULTS}), 0)


def test_malformed_points_get_their_point_status(ctx, batch):
    enc, chk = pc.ENC_COMPRESSED, pc.CHECK_SUBGROUP
    first = lambda group, cls: next(b for c, b in pc.corpus(group, enc) if c == cls)
    proofs = list(batch["proofs"])
    want = {}
    for i, cls in zip(FAULTS, ("x_ge_p", "no_root", "off_subgroup")):
        proofs[i] = first(1, cls) + proofs[i][48:]
        want[i] = pc.class_status(cls, enc, chk)
    assert want == {0: 1, 64: 2, 129: 3}
    order_cls = "order_%d" % pc.SMALL_ORDERS[2][0][0]
    proofs[65] = proofs[65][:48] + first(2, order_cls) + proofs[65][144:]
    want[65] = pc.class_status(order_cls, enc, chk)
    proofs[1] = proofs[1][:144] + first(1, "off_subgroup")
    want[1] = 3
    rc, st, bad = _verify(ctx, batch["pv"], batch["publics"], proofs, batch["weights"])
    assert (rc, st, bad) == (-2, _expect(want), 0)
    # a malformed proof does not hide a failing equation elsewhere, and the other way round
    proofs[100] = proofs[100][:144] + batch["proofs"][101][144:]
    want[100] = 5
    rc, st, bad = _verify(ctx, batch["pv"], batch["publics"], proofs, batch["weights"])
    assert (rc, st, bad) == (-2, _expect(want), 0)


def test_infinite_points_are_legal_encodings(ctx, zk, batch):
    """A, B or C at infinity parse; the equation then fails exactly as under the host verifier."""
    inf1, inf2 = bytes([0xC0]) + bytes(47), bytes([0xC0]) + bytes(95)
    proofs = list(batch["proofs"])
    proofs[0] = inf1 + proofs[0][48:]
    proofs[64] = proofs[64][:48] + inf2 + proofs[64][144:]
    proofs[129] = proofs[129][:144] + inf1
    for i in FAULTS:
        assert zk.groth16_verify(batch["vk"], batch["publics"][i], proofs[i]) is False
    rc, st, bad = _verify(ctx, batch["pv"], batch["publics"], proofs, batch["weights"])
    assert (rc, st, bad) == (-5, _expect({i: 5 for i in FAULTS}), 0)


def test_the_weights_are_used(ctx, batch):
    """Swapping the C of two proofs keeps sum C_i: weights (1, 1) accept the pair, (1, 2) refuse it."""
    i, j = 10, 20
    p, q = batch["proofs"][i], batch["proofs"][j]
    proofs = [p[:144] + q[144:], q[:144] + p[144:]]
    publics = [batch["publics"][i], batch["publics"][j]]
    w = lambda *ks: [k.to_bytes(16, "little") for k in ks]
    assert _verify(ctx, batch["pv"], publics, proofs, w(1, 1)) == (0, bytes(2), NO_INDEX)
    assert _verify(ctx, batch["pv"], publics, proofs, w(1, 2)) == (-5, b"\x05\x05", 0)


def test_a_zero_weight_is_a_bad_argument(ctx, batch):
    weights = list(batch["weights"])
    weights[77] = bytes(16)
    rc, st, _ = _verify(ctx, batch["pv"], batch["publics"], batch["proofs"], weights)
    assert rc == -1 and st == bytes([0xEE] * N)
