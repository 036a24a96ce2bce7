"""GPU suite: a relation's Groth16 key from a phase-1 transcript (zkmi_groth16_setup_from_srs) and phase-2 contributions to
its delta (zkmi_pk_contribute).  Affine wire form is unique: every comparison is byte for byte."""
import pytest

from oracle import bls12_381 as ec
from oracle import cpp as ocpp

import setup_key_model as model

pytestmark = pytest.mark.gpu

R = ec.R
frs = model.frs
TOXIC3 = frs([model.TAU, model.ALPHA, model.BETA])
D1, D2 = 0xD1_0000_0000_0000_0000_0000_0005 % R, (R - 0xD2D2D2) % R
RS, SS = frs([0x1234567]), frs([R - 77])


def queries(pk, log_n, n_vars, n_pub):
    """a, b_g1, b_g2, h, l as zkmi_pk_export_query reads them."""
    n = 1 << log_n
    return [pk.export_query(0, 0, n_vars), pk.export_query(1, 0, n_vars), pk.export_query(2, 0, n_vars),
            pk.export_query(3, 0, n - 1), pk.export_query(4, 0, n_vars - n_pub)]


def oracle_key(rel, delta=1):
    """oracle.cpp's setup with gamma = 1: (vk, [a, b_g1, b_g2, h, l], key dict)."""
    toxic = frs([model.TAU, model.ALPHA, model.BETA, 1, delta])
    vk, key = ocpp.groth16_setup(rel.n_vars, rel.n_pub, rel.nc, rel.log_n, rel.mats(), toxic)
    return vk, [key[k] for k in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")], key


def sections(srs):
    n1, n2, nab = srs.shape()
    return [srs.read(0, 0, n1), srs.read(1, 0, n2), srs.read(2, 0, nab), srs.read(3, 0, nab), srs.read(4, 0, 1)]


@pytest.fixture(scope="module")
def rel8(zk):
    rel = model.Relation(8, 0x5E7 + 8)  # the relation of the CPU plan test: three levels at FAN = 8
    r1 = zk.r1cs_create(rel.n_vars, rel.n_pub, rel.mats())
    assert r1.log_n == 8 and r1.is_satisfied(rel.witness())
    yield rel, r1
    r1.free()


@pytest.fixture(scope="module")
def rel3(zk):
    rel = model.Relation(3, 0x5E7 + 3)
    r1 = zk.r1cs_create(rel.n_vars, rel.n_pub, rel.mats())
    assert r1.log_n == 3
    yield rel, r1
    r1.free()


def test_key_at_n8_matches_the_python_oracle(ctx, rel3):
    """N = 8: vk and all five queries against oracle.groth16.setup(gamma = delta = 1), from zkmi_srs_generate and from a
    loaded transcript five powers longer in every array."""
    import setup_srs_model as srs_model

    rel, r1 = rel3
    want_vk, want_q = model.oracle_setup_bytes(rel)
    srs = ctx.srs_generate(TOXIC3, 3)
    pk, vk = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()  # the transcript may go once the key stands
    got = queries(pk, 3, rel.n_vars, rel.n_pub)
    for k in range(5):
        assert got[k] == want_q[k], "query %d" % k
    assert vk == want_vk
    pk.free()
    tr = srs_model.transcript(model.TAU, model.ALPHA, model.BETA, 3, extra=5)
    g = srs_model.points_bytes
    long_srs = ctx.srs_load(0, g(1, tr["tau_g1"]), g(2, tr["tau_g2"]), g(1, tr["alpha_tau_g1"]), g(1, tr["beta_tau_g1"]),
                            ec.g2_to_bytes(tr["beta_g2"]))
    assert long_srs.shape() == (20, 13, 13)
    pk2, vk2 = ctx.groth16_setup_from_srs(r1, long_srs)
    assert queries(pk2, 3, rel.n_vars, rel.n_pub) == want_q and vk2 == want_vk
    pk2.free()
    long_srs.free()


def test_random_relation_at_2p8_matches_the_oracle(ctx, rel8):
    """N = 2^8, n_pub = 3: columns of length 0, 1, FAN, FAN + 1, FAN^2, FAN^2 + 1 and one of every row (three levels),
    coefficients 1, r-1, 2, r-2, 2^16 and full-width, a variable A, B and C mention on one row, one no row mentions:
    vk and all five queries against oracle.cpp.groth16_setup with gamma = delta = 1."""
    rel, r1 = rel8
    want_vk, want_q, _ = oracle_key(rel)
    srs = ctx.srs_generate(TOXIC3, 8)
    pk, vk = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    got = queries(pk, 8, rel.n_vars, rel.n_pub)
    pk.free()
    for k in range(5):
        assert got[k] == want_q[k], "query %d" % k
    assert vk == want_vk
    assert got[0][96 * model.V_NONE : 96 * model.V_NONE + 96] == bytes(96)


def test_real_relation_matches_the_trapdoor_setup(ctx, zk):
    """zkmi_create_note_r1cs(11): full-width Poseidon constants and a constant-one column of thousands of entries.  The key
    from the transcript equals zkmi_groth16_setup(tau, alpha, beta, 1, 1) on the same context."""
    r1 = zk.create_note_r1cs(11)
    assert r1.log_n == 11
    pk0, vk0 = ctx.groth16_setup(r1, frs([model.TAU, model.ALPHA, model.BETA, 1, 1]))
    want = queries(pk0, 11, r1.n_vars, r1.n_pub)
    want_elems = pk0.export_g1_elems()
    pk0.free()
    srs = ctx.srs_generate(TOXIC3, 11)
    pk, vk = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    got = queries(pk, 11, r1.n_vars, r1.n_pub)
    for k in range(5):
        assert got[k] == want[k], "query %d" % k
    assert vk == vk0 and pk.export_g1_elems() == want_elems
    pk.free()
    r1.free()


def test_contributions_give_the_key_of_the_product(ctx, zk, rel8):
    """d1 then d2 on the key of the 2^8 relation: queries, beta_g1 / delta_g1, delta_g2 and the patched vk equal the oracle's
    setup with delta = d1 d2; a proof from the contributed key verifies under the patched vk and not under the unpatched one."""
    rel, r1 = rel8
    srs = ctx.srs_generate(TOXIC3, 8)
    pk, vk = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    _, q1, key1 = oracle_key(rel, D1)
    dg1, dg2 = pk.contribute(ec.fr_to_bytes(D1))
    assert queries(pk, 8, rel.n_vars, rel.n_pub) == q1 and dg1 == key1["delta_g1"] and dg2 == key1["delta_g2"]
    want_vk, want_q, key = oracle_key(rel, D1 * D2 % R)
    dg1, dg2 = pk.contribute(ec.fr_to_bytes(D2))
    got = queries(pk, 8, rel.n_vars, rel.n_pub)
    for k in range(5):
        assert got[k] == want_q[k], "query %d" % k
    assert pk.export_g1_elems() == (key["beta_g1"], key["delta_g1"]) and dg1 == key["delta_g1"] and dg2 == key["delta_g2"]
    patched = vk[:480] + dg2 + vk[672:]
    assert patched == want_vk and patched != vk
    wit = rel.witness()
    proof = ctx.groth16_prove(pk, wit, RS, SS)
    assert proof == ocpp.groth16_prove(rel.n_vars, rel.n_pub, rel.nc, rel.log_n, rel.mats(), key, wit, RS, SS)
    publics = wit[32 : 32 * rel.n_pub]
    assert zk.groth16_verify(patched, publics, proof) is True
    assert zk.groth16_verify(vk, publics, proof) is False
    pk.free()


def test_refusals_leave_context_and_key_intact(ctx, zk, pkg, rel3):
    """A transcript one power short in each of the three length conditions, vk_cap one byte short, d = 0, d = r: refused
    with the documented code; after each the key's l query is unchanged and the context still proves."""
    rel, r1 = rel3
    n, wit = 8, rel.witness()
    full = ctx.srs_generate(TOXIC3, 3)
    sec = sections(full)
    pk, vk = ctx.groth16_setup_from_srs(r1, full)
    l_before = pk.export_query(4, 0, rel.n_vars - rel.n_pub)
    proof = ctx.groth16_prove(pk, wit, RS, SS)
    assert zk.groth16_verify(vk, wit[32 : 32 * rel.n_pub], proof) is True

    def still_fine():
        assert pk.export_query(4, 0, rel.n_vars - rel.n_pub) == l_before
        assert ctx.groth16_prove(pk, wit, RS, SS) == proof

    cuts = ((96 * (2 * n - 2), 192 * n, 96 * n), (96 * (2 * n - 1), 192 * (n - 1), 96 * n), (96 * (2 * n - 1), 192 * n, 96 * (n - 1)))
    for c1, c2, cab in cuts:
        short = ctx.srs_load(0, sec[0][:c1], sec[1][:c2], sec[2][:cab], sec[3][:cab], sec[4])
        with pytest.raises(pkg.ZkmiError) as e:
            ctx.groth16_setup_from_srs(r1, short)
        assert e.value.code == -1
        short.free()
        still_fine()
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.groth16_setup_from_srs(r1, full, vk_cap=672 + 96 * rel.n_pub - 1)
    assert e.value.code == -1
    still_fine()
    for d, code in ((0, -1), (R, -2)):
        with pytest.raises(pkg.ZkmiError) as e:
            pk.contribute(d.to_bytes(32, "little"))
        assert e.value.code == code
        still_fine()
    assert pk.export_g1_elems()[1] == zk.g1_generator()  # delta_g1 untouched
    full.free()
    pk.free()
