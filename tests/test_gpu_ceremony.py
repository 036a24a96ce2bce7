"""GPU suite: verifying a ceremony -- the adjacent weighted sums of a point array (zkmi_g{1,2}_points_adjacent_sums_dev), the
same-ratio checks of a phase-1 transcript (zkmi_srs_verify) and of a phase-2 contribution (zkmi_pk_verify_contribution).
Every input comes from zkmi_srs_generate / zkmi_srs_read; tampered points are other subgroup points ([k]P from the oracle),
so ingest accepts them and only the pairing equations can refuse.  Affine wire form is unique: sums compare byte for byte."""
import hashlib
import struct

import pytest

from oracle import bls12_381 as ec
from oracle import cpp as ocpp

import points_corpus as pc
import setup_key_model as key_model
import setup_srs_model as model

pytestmark = pytest.mark.gpu

R = ec.R
frs = model.frs
TAU, ALPHA, BETA = key_model.TAU, key_model.ALPHA, key_model.BETA
TAU_B, BETA_B = (TAU * 7 + 11) % R, (BETA * 3 + 5) % R
TOXIC3 = frs([TAU, ALPHA, BETA])
TOXIC3_B = frs([TAU_B, ALPHA, BETA_B])  # another tau and another beta, the same alpha
SEED_A, SEED_B = bytes(range(32)), hashlib.sha256(b"ceremony seed two").digest()
D1, D2 = 0xD1_0000_0000_0000_0000_0000_0005 % R, (R - 0xD2D2D2) % R
RS, SS = frs([0x1234567]), frs([R - 77])
WIRE = model.WIRE
FROM_BYTES, TO_BYTES = model.FROM_BYTES, model.TO_BYTES
T1, T2, AL, BE, BG2, DEG = 1, 2, 4, 8, 16, 32  # ZKMI_SRS_*
FIXED, DELTA, BAD_H, BAD_L = 1, 2, 4, 8  # ZKMI_PK2_*


def upload(b):
    import torch

    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def weights32(seed, dom, count):
    """count 32-byte canonical scalars: the weight in the low 16 bytes."""
    return [hashlib.sha256(seed + struct.pack("<IQ", dom, i)).digest()[:16] + bytes(16) for i in range(count)]


def sections(srs):
    n1, n2, nab = srs.shape()
    return [srs.read(0, 0, n1), srs.read(1, 0, n2), srs.read(2, 0, nab), srs.read(3, 0, nab), srs.read(4, 0, 1)]


def scaled(group, buf, idx, k=5):
    """buf with point idx replaced by [k] of itself: another point of the subgroup."""
    w = WIRE[group]
    pt = FROM_BYTES[group](buf[w * idx : w * idx + w])
    assert pt is not None
    new = TO_BYTES[group]((ec.g1_mul if group == 1 else ec.g2_mul)(k, pt))
    assert new != buf[w * idx : w * idx + w]
    return buf[: w * idx] + new + buf[w * idx + w :]


# ---- the layer below: adjacent sums ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points9(ctx):
    """The first 300 powers of tau in both groups, from a transcript for 2^9."""
    srs = ctx.srs_generate(TOXIC3, 9)
    out = {1: srs.read(0, 0, 300), 2: srs.read(1, 0, 300)}
    srs.free()
    return out


@pytest.mark.parametrize("group", (1, 2))
def test_adjacent_sums_match_the_oracle(ctx, points9, group):
    """m = 1, 2, 3, 64, 65, 257 and 300 (k_rlc_weights runs 128 lanes a workgroup: one, exactly two and more than two
    workgroups), infinity entries mixed in at m = 65 (in the middle and at the end): lo and hi against hashlib weights and
    the oracle's MSM."""
    w = WIRE[group]
    msm = ocpp.msm_g1 if group == 1 else ocpp.msm_g2
    for m, seed, dom in ((1, SEED_A, 0), (2, SEED_A, 1), (3, SEED_B, 2), (64, SEED_A, 3), (65, SEED_B, 19), (257, SEED_A, 20), (300, SEED_B, 0)):
        pts = points9[group][: w * m]
        if m == 65:
            pts = pts[: w * 7] + bytes(w) + pts[w * 8 : w * 64] + bytes(w)
        d = upload(pts)
        lo, hi = ctx.points_adjacent_sums_dev(group, d.data_ptr(), m, seed, dom)
        if m == 1:
            assert lo == bytes(w) and hi == bytes(w)
            continue
        sc = b"".join(weights32(seed, dom, m - 1))
        assert lo == msm(sc, pts[: w * (m - 1)]), (m, "lo")
        assert hi == msm(sc, pts[w:]), (m, "hi")


def test_adjacent_sums_refuse_bad_arguments(ctx, pkg, points9):
    d = upload(points9[1][: 96 * 4])
    for args in ((0, 4, SEED_A), (d.data_ptr(), 0, SEED_A), (d.data_ptr(), 4, None)):
        with pytest.raises(pkg.ZkmiError) as e:
            ctx.points_adjacent_sums_dev(1, args[0], args[1], args[2], 0)
        assert e.value.code == -1
    bad = upload(bytes([0xFF]) * 96 + points9[1][96 : 96 * 4])  # a coordinate >= p
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.points_adjacent_sums_dev(1, bad.data_ptr(), 4, SEED_A, 0)
    assert e.value.code == -2
    lo, hi = ctx.points_adjacent_sums_dev(1, d.data_ptr(), 4, SEED_A, 0)  # the context is as usable as before
    sc = b"".join(weights32(SEED_A, 0, 3))
    assert lo == ocpp.msm_g1(sc, points9[1][: 96 * 3]) and hi == ocpp.msm_g1(sc, points9[1][96 : 96 * 4])


# ---- phase 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", (0, 1, 3, 5, 8))
def test_generated_transcripts_verify(ctx, log_n):
    """Two seeds and a drawn one.  log_n = 0 holds no power of tau: nothing to compare, the anchors and beta only."""
    srs = ctx.srs_generate(TOXIC3, log_n)
    for seed in (SEED_A, SEED_B, None):
        assert srs.verify(seed) == (True, 0), seed
    srs.free()


@pytest.fixture(scope="module")
def sec3(ctx):
    srs = ctx.srs_generate(TOXIC3, 3)
    sec = sections(srs)
    srs.free()
    return sec


@pytest.fixture(scope="module")
def sec3_other(ctx):
    srs = ctx.srs_generate(TOXIC3_B, 3)
    sec = sections(srs)
    srs.free()
    return sec


def test_reloaded_and_longer_transcripts_verify(ctx, sec3):
    """The transcript for N = 8 through the compressed encoding; and the one for N = 16 cut to what N = 8 needs in G2, alpha
    and beta, which leaves 31 > 2 N - 1 powers in tau_g1."""
    groups = (1, 2, 1, 1, 2)
    comp = [b"".join(pc.encode(g, 1, p) for p in model.points_from_bytes(g, s)) for g, s in zip(groups, sec3)]
    srs = ctx.srs_load(1, *comp)
    assert srs.verify(SEED_A) == (True, 0) and srs.verify(None) == (True, 0)
    srs.free()
    gen = ctx.srs_generate(TOXIC3, 4)
    s4 = sections(gen)
    gen.free()
    srs = ctx.srs_load(0, s4[0], s4[1][: 192 * 8], s4[2][: 96 * 8], s4[3][: 96 * 8], s4[4])
    assert srs.shape() == (31, 8, 8)
    assert srs.verify(SEED_B) == (True, 0)
    srs.free()


def swap(buf, w, i, j):
    pts = [buf[w * k : w * k + w] for k in range(len(buf) // w)]
    pts[i], pts[j] = pts[j], pts[i]
    return b"".join(pts)


# name -> (section changed, how, expected mask).  N = 8: tau_g1 has 15 points, the others 8.
BAD_TRANSCRIPTS = {
    # eq. TAU_G2 reads tau_g1[1] as its G1 anchor: a wrong tau_g1[1] breaks the tie between the groups as well
    "tau_g1[1]": (0, lambda s, o: scaled(1, s[0], 1), T1 | T2),
    "tau_g1[7]": (0, lambda s, o: scaled(1, s[0], 7), T1),
    "tau_g1[last]": (0, lambda s, o: scaled(1, s[0], 14), T1),
    "tau_g2[last]": (1, lambda s, o: scaled(2, s[1], 7), T2),
    "alpha_tau_g1[0]": (2, lambda s, o: scaled(1, s[2], 0), AL),
    "alpha_tau_g1[last]": (2, lambda s, o: scaled(1, s[2], 7), AL),
    # beta_tau_g1[0] is also the G1 side of BETA_G2
    "beta_tau_g1[0]": (3, lambda s, o: scaled(1, s[3], 0), BE | BG2),
    "beta_tau_g1[last]": (3, lambda s, o: scaled(1, s[3], 7), BE),
    "tau_g1[4] <-> tau_g1[5]": (0, lambda s, o: swap(s[0], 96, 4, 5), T1),
    # tau_g2[1] is the ratio every G1 chain is held to, and tau_g2 no longer continues tau_g1[1]
    "tau_g2 of another tau": (1, lambda s, o: o[1], T1 | T2 | AL | BE),
    "beta_g2 of another beta": (4, lambda s, o: o[4], BG2),
    # a chain that is consistent in itself, in another tau
    "alpha_tau_g1 of another tau": (2, lambda s, o: o[2], AL),
    # reported alone: the equations are not evaluated without their anchor
    "tau_g1[1] = infinity": (0, lambda s, o: s[0][:96] + bytes(96) + s[0][192:], DEG),
}


@pytest.mark.parametrize("name", sorted(BAD_TRANSCRIPTS))
def test_bad_transcript_is_refused_with_its_mask(ctx, sec3, sec3_other, name):
    which, change, mask = BAD_TRANSCRIPTS[name]
    sec = list(sec3)
    sec[which] = change(sec3, sec3_other)
    assert sec[which] != sec3[which] and len(sec[which]) == len(sec3[which])
    srs = ctx.srs_load(0, *sec)  # every point is in the subgroup: ingest accepts
    for seed in (SEED_A, None):
        assert srs.verify(seed) == (False, mask), (name, seed)
    srs.free()


def test_transcript_without_subgroup_checks_is_refused(ctx, pkg, sec3):
    srs = ctx.srs_load(0, *sec3, checks=pkg.CHECK_CURVE)
    with pytest.raises(pkg.ZkmiError) as e:
        srs.verify(SEED_A)
    assert e.value.code == -1
    srs.free()
    good = ctx.srs_load(0, *sec3)
    assert good.verify(SEED_A) == (True, 0)  # the context stays usable
    good.free()


# ---- phase 2 ---------------------------------------------------------------------------------------------------------
def key_parts(pk, vk, rel, delta_g1, delta_g2):
    """Everything zkmi_pk_load takes, as a dict."""
    n = 1 << rel.log_n
    beta_g1, _ = pk.export_g1_elems()
    return dict(alpha_g1=vk[:96], beta_g1=beta_g1, beta_g2=vk[96:288], delta_g1=delta_g1, delta_g2=delta_g2,
                a=pk.export_query(0, 0, rel.n_vars), b1=pk.export_query(1, 0, rel.n_vars), b2=pk.export_query(2, 0, rel.n_vars),
                h=pk.export_query(3, 0, n - 1), l=pk.export_query(4, 0, rel.n_vars - rel.n_pub))


def load_parts(ctx, r1, p):
    return ctx.pk_load(r1, p["alpha_g1"], p["beta_g1"], p["beta_g2"], p["delta_g1"], p["delta_g2"], p["a"], p["b1"], p["b2"], p["h"], p["l"])


def first_finite(buf, w, start=0):
    return next(i for i in range(start, len(buf) // w) if buf[w * i : w * i + w] != bytes(w))


@pytest.fixture(scope="module")
def phase2(ctx, zk):
    """The relation of test_gpu_setup_key.py at N = 2^5; `before` is the key of the transcript, `after` the same key with
    the contribution D1, `after2` with D1 then D2; the parts of `before` and `after` for rebuilding tampered keys."""
    rel = key_model.Relation(5, 0x5E7 + 5)
    r1 = zk.r1cs_create(rel.n_vars, rel.n_pub, rel.mats())
    srs = ctx.srs_generate(TOXIC3, 5)
    before, vk = ctx.groth16_setup_from_srs(r1, srs)
    after, _ = ctx.groth16_setup_from_srs(r1, srs)
    after2, _ = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    dg1, dg2 = after.contribute(ec.fr_to_bytes(D1))
    assert after2.contribute(ec.fr_to_bytes(D1)) == (dg1, dg2)
    after2.contribute(ec.fr_to_bytes(D2))
    st = dict(rel=rel, r1=r1, before=before, after=after, after2=after2, vk=vk,
              parts_before=key_parts(before, vk, rel, zk.g1_generator(), zk.g2_generator()), parts_after=key_parts(after, vk, rel, dg1, dg2))
    yield st
    for k in (before, after, after2):
        k.free()
    r1.free()


def test_contributions_verify(ctx, phase2):
    """One contribution, a second one chained on top, and a key against itself (d = 1); two seeds and a drawn one."""
    b, a, a2 = phase2["before"], phase2["after"], phase2["after2"]
    for seed in (SEED_A, SEED_B, None):
        assert a.verify_contribution(b, seed) == (True, 0)
    assert a2.verify_contribution(a, SEED_A) == (True, 0)
    assert b.verify_contribution(b, SEED_A) == (True, 0)
    # the two contributions as one step are a contribution too (d = D1 D2); backwards as well (d^-1)
    assert a2.verify_contribution(b, SEED_B) == (True, 0)
    assert b.verify_contribution(a, SEED_B) == (True, 0)


def test_rebuilt_key_verifies(ctx, phase2):
    """`after` exported and loaded again is the same contribution: the comparison of the fixed part is between a key this
    library derived and one it parsed from bytes."""
    pk = load_parts(ctx, phase2["r1"], phase2["parts_after"])
    assert pk.verify_contribution(phase2["before"], SEED_A) == (True, 0)
    pk.free()


def other_delta(group):
    return (ec.g1_to_bytes(ec.g1_mul(D2)) if group == 1 else ec.g2_to_bytes(ec.g2_mul(D2)))


# name -> (change of the parts of `after`, given those of `before` as well; expected mask): exactly one thing each
BAD_CONTRIBUTIONS = {
    "one h entry": (lambda a, b: dict(a, h=scaled(1, a["h"], first_finite(a["h"], 96, 5))), BAD_H),
    "the last l entry": (lambda a, b: dict(a, l=scaled(1, a["l"], len(a["l"]) // 96 - 1)), BAD_L),
    "one a entry": (lambda a, b: dict(a, a=scaled(1, a["a"], first_finite(a["a"], 96))), FIXED),
    "one b_g2 entry": (lambda a, b: dict(a, b2=scaled(2, a["b2"], first_finite(a["b2"], 192, 1))), FIXED),
    "beta_g1": (lambda a, b: dict(a, beta_g1=scaled(1, a["beta_g1"], 0)), FIXED),
    # delta_g1 and delta_g2 of different d.  h and l are held to delta_g2: when delta_g1 is the odd one out they still pass,
    # when delta_g2 is, they moved by another factor than it did
    "delta_g1 of another d": (lambda a, b: dict(a, delta_g1=other_delta(1)), DELTA),
    "delta_g2 of another d": (lambda a, b: dict(a, delta_g2=other_delta(2)), DELTA | BAD_H | BAD_L),
    "h scaled, l left alone": (lambda a, b: dict(a, l=b["l"]), BAD_L),
}


@pytest.mark.parametrize("name", sorted(BAD_CONTRIBUTIONS))
def test_bad_contribution_is_refused_with_its_mask(ctx, phase2, name):
    change, mask = BAD_CONTRIBUTIONS[name]
    parts = change(phase2["parts_after"], phase2["parts_before"])
    assert parts != phase2["parts_after"]
    pk = load_parts(ctx, phase2["r1"], parts)
    for seed in (SEED_A, None):
        assert pk.verify_contribution(phase2["before"], seed) == (False, mask), (name, seed)
    pk.free()


def test_contribution_of_another_shape_is_refused(ctx, zk, pkg, phase2):
    rel = key_model.Relation(3, 0x5E7 + 3)
    r1 = zk.r1cs_create(rel.n_vars, rel.n_pub, rel.mats())
    srs = ctx.srs_generate(TOXIC3, 3)
    small, _ = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    with pytest.raises(pkg.ZkmiError) as e:
        small.verify_contribution(phase2["before"], SEED_A)
    assert e.value.code == -1
    assert phase2["after"].verify_contribution(phase2["before"], SEED_A) == (True, 0)  # nothing was disturbed
    small.free()
    r1.free()


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_ceremony_end_to_end(ctx, zk, phase2):
    """generate, verify, derive the key, contribute, verify the contribution, prove with the contributed key: the proof
    verifies under the vk patched with the new delta_g2, and not under the unpatched one."""
    rel, r1 = phase2["rel"], phase2["r1"]
    srs = ctx.srs_generate(TOXIC3, 5)
    assert srs.verify() == (True, 0)
    before, vk = ctx.groth16_setup_from_srs(r1, srs)
    pk, _ = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    _, dg2 = pk.contribute(ec.fr_to_bytes(D2))
    assert pk.verify_contribution(before) == (True, 0)
    wit = rel.witness()
    proof = ctx.groth16_prove(pk, wit, RS, SS)
    patched = vk[:480] + dg2 + vk[672:]
    publics = wit[32 : 32 * rel.n_pub]
    assert zk.groth16_verify(patched, publics, proof) is True
    assert zk.groth16_verify(vk, publics, proof) is False
    before.free()
    pk.free()
