"""GPU suite for the device point readers (csrc/points.hip) and the entry points built on them: decompression and verdict
parity with the oracle and with the product's host functions, the size the keys have, resident bases from encoded
bytes, and proving keys loaded and checked through them.  Expected values come from oracle/bls12_381.py and from the
corpus tests/test_cpu_points.py holds to it; none is computed by the code under test."""
import random

import numpy as np
import pytest

import points_corpus as pc
from conftest import golden
from oracle import bls12_381 as ec

pytestmark = pytest.mark.gpu

H = bytes.fromhex
HALF_BE = np.frombuffer(((ec.P - 1) // 2).to_bytes(48, "big"), dtype=np.uint8)


def _dev(b):
    import torch

    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _read(ctx, group, enc, data, checks, want_out=True):
    """(first_bad or None, wire bytes, status bytes) of one launch over host bytes `data`."""
    import torch

    n = len(data) // pc.point_bytes(group, enc)
    d_in = _dev(data)
    d_out = torch.zeros(n * (96 if group == 1 else 192), dtype=torch.uint8, device="cuda") if want_out else None
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fn = ctx.g1_points_read_dev if group == 1 else ctx.g2_points_read_dev
    bad = fn(d_in.data_ptr(), n, enc, checks, d_out.data_ptr() if want_out else None, d_st.data_ptr())
    return bad, (d_out.cpu().numpy().tobytes() if want_out else None), d_st.cpu().numpy().tobytes()


def _gt_half(be):
    """Row-wise: big-endian 48-byte integer > (p - 1) / 2."""
    diff = be != HALF_BE
    first = diff.argmax(axis=1)
    rows = np.arange(be.shape[0])
    return diff.any(axis=1) & (be[rows, first] > HALF_BE[first])


def np_compress(group, wire):
    """zcash compressed form of n affine wire points, with numpy only (no oracle loop at 2^20)."""
    nc = group
    a = np.frombuffer(wire, dtype=np.uint8).reshape(-1, 2 * nc, 48)[:, :, ::-1]  # big-endian components: x.c0 (x.c1) y.c0 (y.c1)
    inf = ~a.reshape(a.shape[0], -1).any(axis=1)
    out = np.ascontiguousarray(a[:, :nc][:, ::-1]).reshape(-1, 48 * nc).copy()  # x.c1 || x.c0
    if group == 1:
        larger = _gt_half(a[:, 1])
    else:
        c1_nonzero = a[:, 3].any(axis=1)
        larger = np.where(c1_nonzero, _gt_half(a[:, 3]), _gt_half(a[:, 2]))
    out[:, 0] |= 0x80
    out[larger, 0] |= 0x20
    out[inf] = 0
    out[inf, 0] = 0xC0
    return out.tobytes()


def np_big_endian(group, wire):
    """zcash uncompressed form: every component big-endian, the high component of Fq2 first."""
    nc = group
    a = np.frombuffer(wire, dtype=np.uint8).reshape(-1, 2, nc, 48)[:, :, ::-1, ::-1]
    inf = ~a.reshape(a.shape[0], -1).any(axis=1)
    out = np.ascontiguousarray(a).reshape(-1, 96 * nc).copy()
    out[inf, 0] = 0x40
    return out.tobytes()


def _to_wire(group, pt):
    return ec.g1_to_bytes(pt) if group == 1 else ec.g2_to_bytes(pt)


def _first_of(group, enc, cls):
    return next(b for c, b in pc.corpus(group, enc) if c == cls)


def test_numpy_encoders_agree_with_the_oracle():
    rnd = random.Random(5)
    for group in (1, 2):
        F, _, _ = pc.field(group)
        gen = ec.G1 if group == 1 else ec.G2
        pts = [None] + [ec.pt_mul(F, gen, rnd.randrange(1, ec.R)) for _ in range(12)]
        wire = b"".join(_to_wire(group, p) for p in pts)
        assert np_compress(group, wire) == b"".join(pc.encode(group, pc.ENC_COMPRESSED, p) for p in pts)
        assert np_big_endian(group, wire) == b"".join(pc.encode(group, pc.ENC_UNCOMPRESSED, p) for p in pts)


@pytest.mark.parametrize("group,n", [(1, 4096), (2, 1024)])
def test_decompression_parity(ctx, zk, group, n):
    """Compressed encodings of oracle-made subgroup points, both sort bits, infinity included -> the device's wire output
    is the oracle's decompression byte for byte, and the host path's."""
    F, _, _ = pc.field(group)
    gen = ec.G1 if group == 1 else ec.G2
    rnd = random.Random(100 + group)
    pts, cur, step = [], ec.pt_mul(F, gen, rnd.randrange(1, ec.R)), ec.pt_mul(F, gen, rnd.randrange(1, ec.R))
    for i in range(n):
        pts.append(None if i % 257 == 100 else cur)
        cur = ec.pt_add(F, cur, step)
    comp = [ec.g1_compress(p) if group == 1 else ec.g2_compress(p) for p in pts]
    sort_bits = [bool(c[0] & 0x20) for c, p in zip(comp, pts) if p is not None]
    assert sum(sort_bits) > n // 8 and sum(not s for s in sort_bits) > n // 8
    dec = ec.g1_decompress if group == 1 else ec.g2_decompress
    want = b"".join(_to_wire(group, dec(c)) for c in comp)
    assert want == b"".join(_to_wire(group, p) for p in pts)
    host = zk.g1_decompress if group == 1 else zk.g2_decompress
    assert b"".join(host(c) for c in comp) == want
    for checks in (pc.CHECK_CURVE, pc.CHECK_SUBGROUP):
        bad, out, st = _read(ctx, group, pc.ENC_COMPRESSED, b"".join(comp), checks)
        assert bad is None and st == bytes(n)
        assert out == want


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("enc", [pc.ENC_WIRE, pc.ENC_COMPRESSED, pc.ENC_UNCOMPRESSED])
def test_verdict_parity_on_the_mixed_corpus(ctx, group, enc):
    """Every element's status byte is its class's, the first failing index is the smallest expected one, the call fails
    iff an element does; the accepted elements alone pass, and their wire output is the oracle's point."""
    items = pc.corpus(group, enc)
    data = b"".join(b for _, b in items)
    w = 96 if group == 1 else 192
    for checks in ((pc.CHECK_CURVE,) if enc == pc.ENC_COMPRESSED else (0, pc.CHECK_CURVE)) + (pc.CHECK_SUBGROUP,):
        want = bytes(pc.class_status(cls, enc, checks) for cls, _ in items)
        bad, out, st = _read(ctx, group, enc, data, checks)
        wrong = [(i, items[i][0], st[i], want[i]) for i in range(len(items)) if st[i] != want[i]]
        print("group %d enc %d checks %d: %d elements, %d failing expected, %d status bytes differ" %
              (group, enc, checks, len(items), sum(1 for s in want if s), len(wrong)))
        assert not wrong, wrong[:8]
        first = next(i for i, s in enumerate(want) if s)
        assert bad == first
        good = [i for i, s in enumerate(want) if s == 0]
        bad2, out2, st2 = _read(ctx, group, enc, b"".join(items[i][1] for i in good), checks)
        assert bad2 is None and st2 == bytes(len(good))
        # wire output of the accepted elements: the oracle's reading of the same bytes
        for k, i in enumerate(good):
            cls, b = items[i]
            if cls == "no_root":
                continue  # accepted only unchecked (status 0 under checks = 0): the bytes go through as they are
            if enc == pc.ENC_COMPRESSED:
                pt = ec.g1_decompress(b) if group == 1 else ec.g2_decompress(b)
                exp = _to_wire(group, pt)
            elif enc == pc.ENC_WIRE:
                exp = b
            else:
                exp = np_wire_from_be(group, b)
            assert out2[w * k : w * k + w] == exp, (cls, i)
            assert out[w * i : w * i + w] == exp, (cls, i)


def np_wire_from_be(group, b):
    if b[0] & 0x40:
        return bytes(len(b))
    nc = group
    a = np.frombuffer(b, dtype=np.uint8).reshape(2, nc, 48)[:, ::-1, ::-1]
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("group,log_n", [(1, 20), (2, 18)])
def test_key_sized_arrays_and_planted_faults(ctx, group, log_n):
    """2^20 G1 / 2^18 G2 points (the testing library's synthetic bases, compressed on the host with numpy): the
    decompressed bytes are the originals and all pass the subgroup check; then three planted elements, one per failing
    status -> exactly those statuses, and the smallest index reported."""
    n = 1 << log_n
    b = ctx.bases_g1_synthetic(n) if group == 1 else ctx.bases_g2_synthetic(n)
    wire = b.read(0, n)
    b.free()
    comp = np_compress(group, wire)
    bad, out, st = _read(ctx, group, pc.ENC_COMPRESSED, comp, pc.CHECK_SUBGROUP)
    assert bad is None
    assert st == bytes(n)
    assert out == wire
    del out
    w = pc.point_bytes(group, pc.ENC_COMPRESSED)
    rnd = random.Random(77 + group)
    pos = sorted(rnd.sample(range(64, n), 3))
    while pos[0] % 64 == 0:
        pos[0] += 1
    faults = {pc.BAD_ENCODING: _first_of(group, pc.ENC_COMPRESSED, "noncanon_inf"),
              pc.NOT_ON_CURVE: _first_of(group, pc.ENC_COMPRESSED, "no_root"),
              pc.NOT_IN_SUBGROUP: _first_of(group, pc.ENC_COMPRESSED, "mixed_%d" % pc.SMALL_ORDERS[group][1][0])}
    order = [pc.NOT_IN_SUBGROUP, pc.BAD_ENCODING, pc.NOT_ON_CURVE]
    planted = bytearray(comp)
    for p, s in zip(pos, order):
        planted[w * p : w * p + w] = faults[s]
    bad, _, st = _read(ctx, group, pc.ENC_COMPRESSED, bytes(planted), pc.CHECK_SUBGROUP, want_out=False)
    got = {i: s for i, s in enumerate(st) if s}
    assert got == dict(zip(pos, order)), (got, pos)
    assert bad == pos[0] and pos[0] >= 64 and pos[0] % 64 != 0


def _scalars(n, seed):
    raw = bytearray(random.Random(seed).randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    return bytes(raw)


@pytest.mark.parametrize("group", [1, 2])
def test_bases_from_encoded_bytes(ctx, group):
    """bases_g{1,2}_encoded from the compressed and the big-endian form: read() returns the original bytes and an MSM
    over them is the MSM over the bases loaded the old way; a planted small-order point is refused with its index."""
    n = 1 << 16
    syn = ctx.bases_g1_synthetic(n) if group == 1 else ctx.bases_g2_synthetic(n)
    wire = syn.read(0, n)
    syn.free()
    load = ctx.bases_g1 if group == 1 else ctx.bases_g2
    load_enc = ctx.bases_g1_encoded if group == 1 else ctx.bases_g2_encoded
    msm = ctx.msm_g1 if group == 1 else ctx.msm_g2
    sc = _scalars(n, 9)
    ref = load(wire)
    want = msm(sc, ref)
    ref.free()
    forms = {pc.ENC_COMPRESSED: np_compress(group, wire), pc.ENC_UNCOMPRESSED: np_big_endian(group, wire), pc.ENC_WIRE: wire}
    for enc, data in forms.items():
        b = load_enc(data, enc, pc.CHECK_SUBGROUP)
        assert b.read(0, n) == wire
        assert msm(sc, b) == want
        b.free()
    q = pc.SMALL_ORDERS[group][0][0]
    for enc, data in forms.items():
        w = pc.point_bytes(group, enc)
        bad = bytearray(data)
        at = 40001
        bad[w * at : w * at + w] = _first_of(group, enc, "order_%d" % q)
        with pytest.raises(Exception) as ei:
            load_enc(bytes(bad), enc, pc.CHECK_SUBGROUP)
        assert ei.value.code == -2 and ei.value.first_bad == at, (ei.value, enc)
        assert "40001" in str(ei.value)
        if enc != pc.ENC_COMPRESSED:
            load_enc(bytes(bad), enc, pc.CHECK_CURVE).free()  # on the curve: only the subgroup check refuses it


def _code(fn):
    try:
        pk, _ = fn()
    except Exception as e:  # ZkmiError
        return e.code
    pk.free()
    return 0


def test_arkworks_key_validated_load(ctx, zk):
    """The golden N = 128 key through arkworks' layout, compressed and not: the validated load proves the golden proof and
    writes the blob back; a query point outside the subgroup (a G1 query, then the G2 query) refuses the key and names
    the point; malformed blobs get the error codes of the host path."""
    from oracle import ark_serialize as ark

    gd = golden("groth16_n128.json")
    r1 = zk.shielder_r1cs(gd["log_n"])
    key = {k: H(v) for k, v in gd["pk"].items()}
    vk, z = H(gd["vk"]), H(gd["witness"])
    for compressed in (False, True):
        blob = ark.proving_key(vk, r1.n_pub, key, compressed)
        for checks in (pc.CHECK_CURVE, pc.CHECK_SUBGROUP):
            pk, vk_back = ctx.ark_pk_load_validated(r1, blob, compressed, checks)
            assert vk_back == vk
            assert ctx.groth16_prove(pk, z, H(gd["r"]), H(gd["s"])) == H(gd["proof"])
            assert ctx.ark_pk_write(pk, vk, compressed) == blob
            assert pk.check(pc.CHECK_SUBGROUP) is None
            pk.free()
        # one point of a query replaced by an on-curve point outside the subgroup
        for section, name, group, at in ((0, "a_query", 1, 37), (3, "h_query", 1, 70), (4, "l_query", 1, 5), (2, "b_g2_query", 2, 66)):
            w = 96 if group == 1 else 192
            off = _first_of(group, pc.ENC_WIRE, "off_subgroup")
            bad_key = dict(key)
            bad_key[name] = key[name][: w * at] + off + key[name][w * at + w :]
            assert len(bad_key[name]) == len(key[name])
            bad_blob = ark.proving_key(vk, r1.n_pub, bad_key, compressed)
            with pytest.raises(Exception) as ei:
                ctx.ark_pk_load_validated(r1, bad_blob, compressed, pc.CHECK_SUBGROUP)
            assert ei.value.code == -2 and ei.value.where == (section, at), (ei.value, ei.value.where)
            assert "section %d" % section in str(ei.value) and "[%d]" % at in str(ei.value)
            # the curve check alone lets it through (that is what zkmi_ark_pk_load stops at)
            pk, _ = ctx.ark_pk_load_validated(r1, bad_blob, compressed, pc.CHECK_CURVE)
            assert pk.check(pc.CHECK_CURVE) is None
            assert pk.check(pc.CHECK_SUBGROUP) == (section, at)
            pk.free()
        # malformed blobs: the same codes as the host path
        head = len(ark.verifying_key(vk, r1.n_pub, compressed)) + 2 * (48 if compressed else 96)
        wrong_len = bytearray(blob)
        wrong_len[head : head + 8] = (r1.n_vars + 1).to_bytes(8, "little")
        huge_len = bytearray(blob)
        huge_len[head : head + 8] = (1 << 62).to_bytes(8, "little")
        for broken in (blob[: len(blob) - 1], blob[: len(blob) // 2], blob[: head + 3], blob[:40], bytes(wrong_len), bytes(huge_len)):
            c_host = _code(lambda: ctx.ark_pk_load(r1, broken, compressed))
            c_new = _code(lambda: ctx.ark_pk_load_validated(r1, broken, compressed, pc.CHECK_SUBGROUP))
            assert c_new == c_host and c_new in (-1, -2), (len(broken), c_host, c_new)
    r1.free()


def test_key_at_the_relations_own_size(ctx, zk):
    """update_note at 2^13, set up on the device -> arkworks bytes (compressed) -> validated load: same proof bytes as
    the original key; both keys pass the resident check; a key loaded by the host path with one h_query point replaced
    by [k]G + T (T of small order) is caught by it, with the point's place."""
    from test_cpu_host import _note_update_case

    lg = 13
    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(0x13130000)
    toxic = b"".join(ec.fr_to_bytes(rng.fr()) for _ in range(5))
    pk, vk = ctx.groth16_setup(r1, toxic)
    inp, _ = _note_update_case(zk, 4242, 1)
    wit, _, _ = zk.update_note_witness(lg, 1, inp)
    r_, s_ = ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr())
    want = ctx.groth16_prove(pk, wit, r_, s_)
    blob = ctx.ark_pk_write(pk, vk, True)
    pk2, vk2 = ctx.ark_pk_load_validated(r1, blob, True, pc.CHECK_SUBGROUP)
    assert vk2 == vk
    assert ctx.groth16_prove(pk2, wit, r_, s_) == want
    assert pk.check(pc.CHECK_SUBGROUP) is None and pk2.check(pc.CHECK_SUBGROUP) is None
    n, N = r1.n_vars, 1 << lg
    q = [pk.export_query(which, 0, cnt) for which, cnt in ((0, n), (1, n), (2, n), (3, N - 1), (4, n - r1.n_pub))]
    head = len(zk.ark_vk_write(vk, r1.n_pub, True))
    beta_g1, delta_g1 = zk.g1_decompress(blob[head : head + 48]), zk.g1_decompress(blob[head + 48 : head + 96])
    at = 5003
    mixed = _first_of(1, pc.ENC_WIRE, "mixed_11")
    hq = q[3][: 96 * at] + mixed + q[3][96 * at + 96 :]
    pk3 = ctx.pk_load(r1, vk[:96], beta_g1, vk[96:288], delta_g1, vk[480:672], q[0], q[1], q[2], hq, q[4])
    assert pk3.check(pc.CHECK_CURVE) is None
    assert pk3.check(pc.CHECK_SUBGROUP) == (3, at)
    for k in (pk, pk2, pk3):
        k.free()
    r1.free()
