"""GPU suite: the point transform (zkmi_g{1,2}_points_ntt_dev) and the phase-1 transcript handle (zkmi_srs_*).
Affine wire form is unique: every comparison is byte for byte."""
import json
import os
import random

import pytest

from conftest import ROOT
from oracle import bls12_381 as ec
from oracle import groth16 as g16

import points_corpus as pc
import setup_srs_model as model

pytestmark = pytest.mark.gpu

R = ec.R
frs = model.frs
TAU, ALPHA, BETA = 0x1D0C5A7E5EED0001 % R, 0x2A11FA0000000007 * 0x10001 % R, (R - 0xBE7A) % R
TOXIC3 = frs([TAU, ALPHA, BETA])


def upload(b):
    import torch

    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def download(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def transform(ctx, group, pts_bytes, log_n, inverse):
    d = upload(pts_bytes)
    (ctx.g1_points_ntt_dev if group == 1 else ctx.g2_points_ntt_dev)(d.data_ptr(), log_n, inverse)
    return download(d)


def host_mul(zk, group, pt_bytes, k):
    return (zk.g1_mul if group == 1 else zk.g2_mul)(pt_bytes, ec.fr_to_bytes(k))


# ---- the transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", (1, 2))
def test_transform_matches_the_definition(ctx, group):
    """log_n = 0, 1, 3, forward and inverse, against the O(N^2) definition in the oracle's point arithmetic: random subgroup
    points mixed with infinity entries."""
    rnd = random.Random(100 + group)
    mul = ec.g1_mul if group == 1 else ec.g2_mul
    for log_n in (0, 1, 3):
        n = 1 << log_n
        pts = [None if (n > 1 and i % 3 == 1) else mul(rnd.randrange(1, R)) for i in range(n)]
        raw = model.points_bytes(group, pts)
        for inverse in (False, True):
            want = model.points_bytes(group, model.dft_points(group, pts, inverse=inverse))
            assert transform(ctx, group, raw, log_n, inverse) == want, (log_n, inverse)


@pytest.mark.parametrize("group", (1, 2))
def test_transform_constant_and_delta_arrays(ctx, zk, group):
    """[P] * N at log_n = 5 -> [N P, O, O, ...]: every butterfly of every level meets P + P or P - P.  [P, O, ...] -> all P."""
    w = model.WIRE[group]
    gen = zk.g1_generator() if group == 1 else zk.g2_generator()
    p = host_mul(zk, group, gen, 0xABCDEF12345)
    n = 32
    assert transform(ctx, group, p * n, 5, False) == host_mul(zk, group, p, n) + bytes(w * (n - 1))
    assert transform(ctx, group, p + bytes(w * (n - 1)), 5, False) == p * n
    # and back: the inverse scales by N^-1
    assert transform(ctx, group, p * n, 5, True) == p + bytes(w * (n - 1))


@pytest.mark.parametrize("group", (1, 2))
def test_inverse_transform_of_powers_is_the_lagrange_basis(ctx, zk, group):
    """log_n = 7: the inverse transform of the first N powers zkmi_srs_generate makes is [L_i(tau)]G for every i (L_i from
    oracle.groth16.lagrange_at, the points from the host's scalar multiplication)."""
    log_n, n = 7, 128
    srs = ctx.srs_generate(TOXIC3, log_n)
    assert srs.shape() == (2 * n - 1, n, n)
    got = transform(ctx, group, srs.read(0 if group == 1 else 1, 0, n), log_n, True)
    srs.free()
    gen = zk.g1_generator() if group == 1 else zk.g2_generator()
    assert got == b"".join(host_mul(zk, group, gen, v) for v in g16.lagrange_at(log_n, TAU))


@pytest.mark.parametrize("group", (1, 2))
def test_transform_round_trip_2p13(ctx, group):
    """inverse(forward(x)) == x on 2^13 synthetic points: the smallest update_note domain, many workgroups per level."""
    n = 1 << 13
    b = ctx.bases_g1_synthetic(n) if group == 1 else ctx.bases_g2_synthetic(n)
    raw = b.read(0, n)
    b.free()
    d = upload(raw)
    fn = ctx.g1_points_ntt_dev if group == 1 else ctx.g2_points_ntt_dev
    fn(d.data_ptr(), 13, False)
    mid = download(d)
    assert mid != raw
    fn(d.data_ptr(), 13, True)
    assert download(d) == raw


# ---- the transcript --------------------------------------------------------------------------------------------------
def test_srs_generate_matches_the_oracle(ctx):
    """log_n = 3: every section against the Python oracle's scalar multiplications."""
    tr = model.transcript(TAU, ALPHA, BETA, 3)
    srs = ctx.srs_generate(TOXIC3, 3)
    assert srs.shape() == (15, 8, 8)
    assert srs.read(0, 0, 15) == model.points_bytes(1, tr["tau_g1"])
    assert srs.read(1, 0, 8) == model.points_bytes(2, tr["tau_g2"])
    assert srs.read(2, 0, 8) == model.points_bytes(1, tr["alpha_tau_g1"])
    assert srs.read(3, 0, 8) == model.points_bytes(1, tr["beta_tau_g1"])
    assert srs.read(4, 0, 1) == ec.g2_to_bytes(tr["beta_g2"])
    assert srs.read(0, 13, 2) == model.points_bytes(1, tr["tau_g1"][13:])
    srs.free()


def sections(srs):
    n1, n2, nab = srs.shape()
    return [srs.read(0, 0, n1), srs.read(1, 0, n2), srs.read(2, 0, nab), srs.read(3, 0, nab), srs.read(4, 0, 1)]


def reencode(sec, enc):
    groups = (1, 2, 1, 1, 2)
    return [b"".join(pc.encode(g, enc, p) for p in model.points_from_bytes(g, s)) for g, s in zip(groups, sec)]


def test_ingest_encodings_give_identical_transcripts(ctx):
    """The same transcript through WIRE, ZCASH_COMPRESSED and ZCASH_UNCOMPRESSED: identical resident sections."""
    gen = ctx.srs_generate(TOXIC3, 3)
    sec = sections(gen)
    gen.free()
    for enc in (0, 1, 2):
        s = ctx.srs_load(enc, *(sec if enc == 0 else reencode(sec, enc)))
        assert s.shape() == (15, 8, 8) and sections(s) == sec, enc
        s.free()


def test_ingest_refusals(ctx, zk, pkg):
    """tau_g1[5] replaced by an on-curve point outside the subgroup: refused with where = (0, 5), no handle.  tau_g2[0] != G2
    and tau_g1[0] != G1: refused."""
    gen = ctx.srs_generate(TOXIC3, 3)
    sec = sections(gen)
    gen.free()
    rnd = random.Random(77)
    bad_pt = pc.random_curve_point(1, rnd)
    bad = pc.encode(1, 0, bad_pt)
    assert not zk.g1_in_subgroup(bad)
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.srs_load(0, sec[0][: 96 * 5] + bad + sec[0][96 * 6 :], *sec[1:])
    assert e.value.code == -2 and e.value.where == (0, 5)
    g2x2 = zk.g2_add(zk.g2_generator(), zk.g2_generator())
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.srs_load(0, sec[0], g2x2 + sec[1][192:], *sec[2:])
    assert e.value.code == -2 and e.value.where == (1, 0)
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.srs_load(0, sec[0][96:192] + sec[0][96:], *sec[1:])
    assert e.value.code == -2 and e.value.where == (0, 0)
    # a non-subgroup point passes when the caller asks for the curve check only: the checks are the caller's choice
    s = ctx.srs_load(0, sec[0][: 96 * 5] + bad + sec[0][96 * 6 :], *sec[1:], checks=1)
    s.free()


def test_context_stays_usable(ctx, zk):
    """After transforms and a transcript: zkmi_ctx_sync is clean and an ordinary zkmi_groth16_prove_dev on a key made BEFORE
    them still gives its golden bytes (the workspaces are intact)."""
    with open(os.path.join(ROOT, "tests", "golden", "groth16_n128.json")) as f:
        gd = json.load(f)
    H = bytes.fromhex
    r_old = zk.shielder_r1cs(gd["log_n"])
    wit = zk.shielder_witness(gd["log_n"], gd["witness_seed"])
    pk_old, _ = ctx.groth16_setup(r_old, H(gd["toxic"]))
    srs = ctx.srs_generate(TOXIC3, 3)
    transform(ctx, 1, srs.read(0, 0, 8), 3, True)
    transform(ctx, 2, srs.read(1, 0, 8), 3, False)
    ctx.srs_load(0, *sections(srs)).free()
    srs.free()
    ctx.sync()
    d = upload(wit)
    assert ctx.groth16_prove_dev(pk_old, d.data_ptr(), H(gd["r"]), H(gd["s"])) == H(gd["proof"])
    ctx.sync()
    pk_old.free()
