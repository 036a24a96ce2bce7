"""GPU suite: a phase-1 contribution -- every point of an array times a scalar of its own (zkmi_g{1,2}_points_mul_each_dev,
zkmi_g{1,2}_points_mul_powers_dev), the contribution to a resident transcript (zkmi_srs_contribute) and its check
(zkmi_srs_verify_contribution).  Multiplications compare with the oracle's point arithmetic (oracle.cpp's MSM of one term
is k * P); a contributed transcript compares with zkmi_srs_generate of the product waste, the fixed-base path, which
shares no kernel with the multiplication; altered transcripts hold other subgroup points, so ingest accepts them and only
the pairing equations can refuse."""
import hashlib
import random

import pytest

from oracle import bls12_381 as ec
from oracle import cpp as ocpp

import points_corpus as pc
import setup_key_model as key_model
import setup_srs_model as model
import srs_contribute_model as cm

pytestmark = pytest.mark.gpu

R = ec.R
frs = model.frs
WIRE, FROM_BYTES, TO_BYTES = model.WIRE, model.FROM_BYTES, model.TO_BYTES
TAU, ALPHA, BETA = key_model.TAU, key_model.ALPHA, key_model.BETA
S1, A1, B1 = 0x5151_0000_0000_0000_0000_0000_0000_0007 % R, (R - 0xA1A1A1) % R, 0xB1B1_B1B1_B1B1_B1B1 * 0x10001 % R
S2, A2, B2 = (R - 0x5252) % R, 0xA2A2_0000_0000_0003 % R, 0xB2_0000_0000_0000_0000_0000_0000_0000_0000_0011 % R
TOXIC3 = frs([TAU, ALPHA, BETA])
SEED_A, SEED_B = bytes(range(32)), hashlib.sha256(b"ceremony seed two").digest()
T1, T2, AL, BE, BG2, DEG = 1, 2, 4, 8, 16, 32  # ZKMI_SRS_*
ST_TAU, ST_ALPHA, ST_BETA, ST_DEG = 256, 512, 1024, 2048  # ZKMI_SRS_STEP_*
MSM = {1: ocpp.msm_g1, 2: ocpp.msm_g2}


def upload(b):
    import torch

    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def download(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def sections(srs):
    n1, n2, nab = srs.shape()
    return [srs.read(0, 0, n1), srs.read(1, 0, n2), srs.read(2, 0, nab), srs.read(3, 0, nab), srs.read(4, 0, 1)]


def step_bytes(s, a, b):
    return b"".join(ec.g2_to_bytes(ec.g2_mul(k)) for k in (s, a, b))


def oracle_mul_each(group, pts, scalars):
    """k[i] * P[i] by the C++ oracle: an MSM of one term per point."""
    w = WIRE[group]
    return b"".join(MSM[group](ec.fr_to_bytes(k), pts[w * i : w * i + w]) for i, k in enumerate(scalars))


@pytest.fixture(scope="module")
def window(zk):
    return zk.selftest_points_mul_shape()[1]


@pytest.fixture(scope="module")
def points12(ctx):
    """Powers of tau of a transcript for 2^12: 4097 in G1, 65 in G2."""
    srs = ctx.srs_generate(TOXIC3, 12)
    out = {1: srs.read(0, 0, 4097), 2: srs.read(1, 0, 65)}
    srs.free()
    return out


def mixed_scalars(window, n, seed):
    """n scalars: the edge scalars in a seeded order first, random ones behind them."""
    rnd = random.Random(seed)
    ks = cm.edge_scalars(window)
    rnd.shuffle(ks)
    return (ks + [rnd.randrange(R) for _ in range(n)])[:n]


# ---- the layer below: out[i] = k[i] * P[i] ---------------------------------------------------------------------------
@pytest.mark.parametrize("group,n", [(1, 1), (1, 3), (1, 64), (1, 65), (1, 257), (2, 1), (2, 3), (2, 64), (2, 65)])
def test_mul_each_matches_the_oracle(ctx, points12, window, group, n):
    """One lane, a partly filled store group (n = 1, 3, 65, 257 are no multiples of the four points an inversion serves), one
    workgroup exactly, and more than one.  Edge scalars first (all of them at 257; across the sizes every one is met),
    infinity entries in the middle and at the end; out of place, then in place."""
    w = WIRE[group]
    pts = points12[group][: w * n]
    if n >= 3:
        pts = pts[:w] + bytes(w) + pts[2 * w : w * (n - 1)] + bytes(w)
    ks = mixed_scalars(window, n, 100 * group + n)
    if n == 64:
        ks = ks[::-1][:n]  # the other end of the shuffled edge scalars
    sc = b"".join(ec.fr_to_bytes(k) for k in ks)
    want = oracle_mul_each(group, pts, ks)
    d_p, d_k, d_o = upload(pts), upload(sc), upload(bytes([0xAB]) * (w * n))
    ctx.points_mul_each_dev(group, d_p.data_ptr(), d_k.data_ptr(), n, d_o.data_ptr())
    got = download(d_o)
    for i in range(n):
        assert got[w * i : w * i + w] == want[w * i : w * i + w], (group, n, i, hex(ks[i]))
    assert download(d_p) == pts and download(d_k) == sc  # the inputs are only read
    ctx.points_mul_each_dev(group, d_p.data_ptr(), d_k.data_ptr(), n, d_p.data_ptr())
    assert download(d_p) == want


def test_mul_each_meets_every_edge_scalar(window):
    """The sizes above draw from one shuffled list: 257 entries hold all of it."""
    assert len(cm.edge_scalars(window)) <= 257


@pytest.mark.parametrize("group,n", [(1, 1), (1, 2), (1, 65), (1, 4097), (2, 1), (2, 2), (2, 65)])
def test_mul_powers_equals_mul_each_and_the_oracle(ctx, zk, points12, group, n):
    """P[i] <- (c q^i) P[i]: equal to mul_each under powers made in Python; at 65 (more than one chunk of powers) equal to
    the oracle as well.  4097 spans many workgroups and many chunks."""
    chunk, _ = zk.selftest_points_mul_shape()
    assert 65 > chunk and 4097 > 64 * chunk // 2
    w = WIRE[group]
    pts = points12[group][: w * n]
    c, q = (A1, S1) if n != 2 else (1, R - 1)
    ks = [c * pow(q, i, R) % R for i in range(n)]
    d_p, d_e = upload(pts), upload(pts)
    ctx.points_mul_powers_dev(group, d_p.data_ptr(), n, ec.fr_to_bytes(c), ec.fr_to_bytes(q))
    d_k = upload(b"".join(ec.fr_to_bytes(k) for k in ks))
    ctx.points_mul_each_dev(group, d_e.data_ptr(), d_k.data_ptr(), n, d_e.data_ptr())
    got = download(d_p)
    assert got == download(d_e)
    if n <= 65:
        assert got == oracle_mul_each(group, pts, ks)


@pytest.mark.parametrize("group", (1, 2))
def test_mul_refusals_leave_the_output_untouched(ctx, pkg, points12, group):
    w, n = WIRE[group], 4
    pts = points12[group][: w * n]
    sc = b"".join(ec.fr_to_bytes(k) for k in (3, 5, R - 1, 7))
    filler = bytes([0xAB]) * (w * n)
    d_p, d_k, d_o = upload(pts), upload(sc), upload(filler)
    d_bad_k = upload(sc[:32] + R.to_bytes(32, "little") + sc[64:])  # a scalar equal to r
    d_bad_p = upload(pts[:w] + ec.P.to_bytes(48, "little") + pts[w + 48 :])  # a coordinate equal to p
    P_, K_, O_ = d_p.data_ptr(), d_k.data_ptr(), d_o.data_ptr()
    cases = [((P_, d_bad_k.data_ptr(), n, O_), -2), ((d_bad_p.data_ptr(), K_, n, O_), -2), ((0, K_, n, O_), -1), ((P_, 0, n, O_), -1),
             ((P_, K_, n, 0), -1), ((P_, K_, 0, O_), -1), ((P_ + 1, K_, n - 1, O_), -1), ((P_, K_ + 2, n - 1, O_), -1),
             ((P_, K_, n - 1, O_ + 1), -1)]
    for args, code in cases:
        with pytest.raises(pkg.ZkmiError) as e:
            ctx.points_mul_each_dev(group, *args)
        assert e.value.code == code, args
        assert download(d_o) == filler
    one, two = ec.fr_to_bytes(1), ec.fr_to_bytes(2)
    pcases = [((d_bad_p.data_ptr(), n, one, two), -2), ((P_, n, R.to_bytes(32, "little"), two), -2), ((P_, n, one, R.to_bytes(32, "little")), -2),
              ((0, n, one, two), -1), ((P_, n, None, two), -1), ((P_, n, one, None), -1), ((P_, 0, one, two), -1), ((P_ + 2, n - 1, one, two), -1)]
    for args, code in pcases:
        with pytest.raises(pkg.ZkmiError) as e:
            ctx.points_mul_powers_dev(group, *args)
        assert e.value.code == code, args
        assert download(d_p) == pts
    ctx.points_mul_each_dev(group, P_, K_, n, O_)  # the context is as usable as before
    assert download(d_o) == oracle_mul_each(group, pts, (3, 5, R - 1, 7))


# ---- the contribution ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", (0, 1, 3, 6, 12))
def test_contribution_equals_the_generated_product_transcript(ctx, log_n):
    """generate(t, a, b) then contribute(s, x, y) is generate(t s, a x, b y), every section byte for byte; 2^12 spans many
    workgroups and many chunks of powers.  The step elements are the oracle's."""
    srs = ctx.srs_generate(TOXIC3, log_n)
    step = srs.contribute(frs([S1, A1, B1]))
    want = ctx.srs_generate(frs([TAU * S1 % R, ALPHA * A1 % R, BETA * B1 % R]), log_n)
    assert srs.shape() == want.shape()
    for k, (got, exp) in enumerate(zip(sections(srs), sections(want))):
        assert got == exp, (log_n, k)
    assert step == step_bytes(S1, A1, B1)
    srs.free()
    want.free()


def test_two_contributions_are_the_contribution_of_the_products(ctx):
    a, b = ctx.srs_generate(TOXIC3, 3), ctx.srs_generate(TOXIC3, 3)
    a.contribute(frs([S1, A1, B1]))
    a.contribute(frs([S2, A2, B2]))
    step = b.contribute(frs([S1 * S2 % R, A1 * A2 % R, B1 * B2 % R]))
    assert sections(a) == sections(b)
    assert step == step_bytes(S1 * S2, A1 * A2, B1 * B2)
    a.free()
    b.free()


def test_the_unit_contribution_changes_no_byte(ctx):
    srs = ctx.srs_generate(TOXIC3, 3)
    before = sections(srs)
    step = srs.contribute(frs([1, 1, 1]))
    assert sections(srs) == before
    assert step == ec.g2_to_bytes(ec.G2) * 3
    srs.free()


def test_contribution_to_a_loaded_transcript_of_odd_lengths(ctx):
    """Lengths (100, 7, 33) cut from a 2^6 transcript and loaded zcash-compressed: more G1 than G2 powers, neither a power
    of two; the result is the matching prefix of the generated product transcript."""
    gen = ctx.srs_generate(TOXIC3, 6)
    s6 = sections(gen)
    gen.free()
    cut = [s6[0][: 96 * 100], s6[1][: 192 * 7], s6[2][: 96 * 33], s6[3][: 96 * 33], s6[4]]
    comp = [b"".join(pc.encode(g, 1, p) for p in model.points_from_bytes(g, s)) for g, s in zip((1, 2, 1, 1, 2), cut)]
    srs = ctx.srs_load(1, *comp)
    assert srs.shape() == (100, 7, 33)
    srs.contribute(frs([S1, A1, B1]))
    want = ctx.srs_generate(frs([TAU * S1 % R, ALPHA * A1 % R, BETA * B1 % R]), 6)
    w6 = sections(want)
    want.free()
    assert sections(srs) == [w6[0][: 96 * 100], w6[1][: 192 * 7], w6[2][: 96 * 33], w6[3][: 96 * 33], w6[4]]
    assert srs.verify(SEED_A) == (True, 0)  # `checks` was kept: the transcript is still verifiable
    srs.free()


def test_refused_contributions_leave_the_transcript_unchanged(ctx, pkg):
    srs = ctx.srs_generate(TOXIC3, 3)
    before = sections(srs)
    r32 = R.to_bytes(32, "little")
    for sab, code in ((frs([0, A1, B1]), -1), (frs([S1, 0, B1]), -1), (frs([S1, A1, 0]), -1), (frs([S1]) + r32 + frs([B1]), -2), (None, -1)):
        with pytest.raises(pkg.ZkmiError) as e:
            srs.contribute(sab)
        assert e.value.code == code
        assert sections(srs) == before
    srs.contribute(frs([S1, A1, B1]))  # and it still takes a good one
    assert sections(srs) != before
    srs.free()


# ---- the check -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain3(ctx):
    """A 2^3 transcript, the same after (S1, A1, B1), and after (S2, A2, B2) on top; the sections of each."""
    s0, s1, s2 = (ctx.srs_generate(TOXIC3, 3) for _ in range(3))
    step1 = s1.contribute(frs([S1, A1, B1]))
    assert s2.contribute(frs([S1, A1, B1])) == step1
    step2 = s2.contribute(frs([S2, A2, B2]))
    st = dict(s0=s0, s1=s1, s2=s2, step1=step1, step2=step2, sec0=sections(s0), sec1=sections(s1))
    yield st
    for s in (s0, s1, s2):
        s.free()


def test_genuine_contributions_verify(ctx, chain3):
    """One contribution under two fixed seeds and a drawn one; a chain of two, link by link; and the two as one step."""
    for seed in (SEED_A, SEED_B, None):
        assert chain3["s1"].verify_contribution(chain3["s0"], chain3["step1"], seed) == (True, 0), seed
    assert chain3["s2"].verify_contribution(chain3["s1"], chain3["step2"], SEED_A) == (True, 0)
    both = step_bytes(S1 * S2, A1 * A2, B1 * B2)
    assert chain3["s2"].verify_contribution(chain3["s0"], both, SEED_B) == (True, 0)


def test_contribution_to_the_domain_of_size_one_verifies(ctx):
    """No tau_g1[1]: no tau step to compare, and whatever stands in its place is not held against anything."""
    a, b = ctx.srs_generate(TOXIC3, 0), ctx.srs_generate(TOXIC3, 0)
    step = b.contribute(frs([S1, A1, B1]))
    assert b.verify_contribution(a, step, SEED_A) == (True, 0)
    assert b.verify_contribution(a, step_bytes(S2, A1, B1), SEED_A) == (True, 0)
    assert b.verify_contribution(a, step_bytes(S1, A2, B1), SEED_A) == (False, ST_ALPHA)
    a.free()
    b.free()


def scaled(group, buf, idx, k=5):
    """buf with point idx replaced by [k] of itself: another point of the subgroup."""
    w = WIRE[group]
    new = TO_BYTES[group]((ec.g1_mul if group == 1 else ec.g2_mul)(k, FROM_BYTES[group](buf[w * idx : w * idx + w])))
    assert new != buf[w * idx : w * idx + w]
    return buf[: w * idx] + new + buf[w * idx + w :]


# name -> (step elements, expected mask) against the genuine `after`
BAD_STEPS = {
    "s of another scalar": (lambda: step_bytes(S2, A1, B1), ST_TAU),
    "a of another scalar": (lambda: step_bytes(S1, A2, B1), ST_ALPHA),
    "b of another scalar": (lambda: step_bytes(S1, A1, B2), ST_BETA),
    "s at infinity": (lambda: bytes(192) + step_bytes(S1, A1, B1)[192:], ST_DEG),
    "b at infinity": (lambda: step_bytes(S1, A1, B1)[:384] + bytes(192), ST_DEG),
}


@pytest.mark.parametrize("name", sorted(BAD_STEPS))
def test_bad_step_element_is_refused_with_its_mask(ctx, chain3, name):
    make, mask = BAD_STEPS[name]
    for seed in (SEED_A, None):
        assert chain3["s1"].verify_contribution(chain3["s0"], make(), seed) == (False, mask), (name, seed)


# name -> (section of `after` changed, how, expected mask).  N = 8: tau_g1 has 15 points, the others 8.
BAD_AFTER = {
    "tau_g1[7]": (0, lambda s: scaled(1, s[0], 7), T1),
    "tau_g2[4]": (1, lambda s: scaled(2, s[1], 4), T2),
    "alpha_tau_g1[4]": (2, lambda s: scaled(1, s[2], 4), AL),
    "beta_tau_g1[4]": (3, lambda s: scaled(1, s[3], 4), BE),
}


@pytest.mark.parametrize("name", sorted(BAD_AFTER))
def test_altered_entry_is_refused_with_its_section(ctx, chain3, name):
    which, change, mask = BAD_AFTER[name]
    sec = list(chain3["sec1"])
    sec[which] = change(sec)
    srs = ctx.srs_load(0, *sec)
    for seed in (SEED_A, None):
        assert srs.verify_contribution(chain3["s0"], chain3["step1"], seed) == (False, mask), (name, seed)
        assert srs.verify(seed) == (False, mask)  # the low bits are what zkmi_srs_verify reports
    srs.free()


def test_unmoved_beta_g2_is_refused(ctx, chain3):
    sec = list(chain3["sec1"])
    sec[4] = chain3["sec0"][4]
    srs = ctx.srs_load(0, *sec)
    assert srs.verify_contribution(chain3["s0"], chain3["step1"], SEED_A) == (False, BG2)
    srs.free()


def test_contribution_from_another_predecessor_is_refused(ctx, chain3):
    """`after` is consistent in itself, but descends from a transcript of another tau, alpha and beta."""
    other = ctx.srs_generate(frs([(TAU * 7 + 11) % R, (ALPHA * 3 + 1) % R, (BETA * 3 + 5) % R]), 3)
    assert other.verify(SEED_A) == (True, 0)
    assert chain3["s1"].verify_contribution(other, chain3["step1"], SEED_A) == (False, ST_TAU | ST_ALPHA | ST_BETA)
    other.free()


def test_step_element_outside_the_subgroup_is_refused(ctx, pkg, chain3):
    rnd = random.Random(77)
    pt = pc.random_curve_point(2, rnd)
    assert ec.pt_mul(ec.Fq2, pt, R) is not None  # on the curve, outside the r-order subgroup
    bad = chain3["step1"][:192] + ec.g2_to_bytes(pt) + chain3["step1"][384:]
    with pytest.raises(pkg.ZkmiError) as e:
        chain3["s1"].verify_contribution(chain3["s0"], bad, SEED_A)
    assert e.value.code == -2
    with pytest.raises(pkg.ZkmiError) as e:  # a coordinate >= p
        chain3["s1"].verify_contribution(chain3["s0"], ec.P.to_bytes(48, "little") + chain3["step1"][48:], SEED_A)
    assert e.value.code == -2


def test_verify_contribution_refuses_bad_arguments(ctx, pkg, chain3):
    small = ctx.srs_generate(TOXIC3, 2)
    unchecked = ctx.srs_load(0, *chain3["sec1"], checks=pkg.CHECK_CURVE)
    s0, s1, step = chain3["s0"], chain3["s1"], chain3["step1"]
    for before, after, st in ((small, s1, step), (s0, small, step), (s0, unchecked, step), (unchecked, s1, step), (s0, s1, None)):
        with pytest.raises(pkg.ZkmiError) as e:
            ctx.srs_verify_contribution(before, after, st, SEED_A)
        assert e.value.code == -1
    assert s1.verify_contribution(s0, step, SEED_A) == (True, 0)  # nothing was disturbed
    small.free()
    unchecked.free()


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_ceremony_phase_one_end_to_end(ctx, zk):
    """generate, contribute twice with every link verified, derive the key of a small random relation (2^5): the key is
    zkmi_groth16_setup's for the product waste and gamma = delta = 1, byte for byte."""
    rel = key_model.Relation(5, 0x5E7 + 5)
    r1 = zk.r1cs_create(rel.n_vars, rel.n_pub, rel.mats())
    srs, prev = ctx.srs_generate(TOXIC3, 5), ctx.srs_generate(TOXIC3, 5)
    assert srs.verify() == (True, 0)
    step = srs.contribute(frs([S1, A1, B1]))
    assert srs.verify_contribution(prev, step) == (True, 0)
    prev.contribute(frs([S1, A1, B1]))
    step = srs.contribute(frs([S2, A2, B2]))
    assert srs.verify_contribution(prev, step) == (True, 0)
    prev.free()
    pk, vk = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    pk0, vk0 = ctx.groth16_setup(r1, frs([TAU * S1 * S2 % R, ALPHA * A1 * A2 % R, BETA * B1 * B2 % R, 1, 1]))
    n = 1 << rel.log_n
    for which, count in ((0, rel.n_vars), (1, rel.n_vars), (2, rel.n_vars), (3, n - 1), (4, rel.n_vars - rel.n_pub)):
        assert pk.export_query(which, 0, count) == pk0.export_query(which, 0, count), which
    assert vk == vk0 and pk.export_g1_elems() == pk0.export_g1_elems()
    pk.free()
    pk0.free()
    r1.free()
