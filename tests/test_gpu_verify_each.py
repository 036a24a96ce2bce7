"""GPU suite for the final exponentiation on the device (csrc/pairing_dev.hip k_final_exp), the batch of reduced pairings
on top of it (zkmi_pairing_batch_dev) and per-proof verification (csrc/verify_each.hip: zkmi_groth16_verify_each).  Exact
bytes and verdicts: expected values come from oracle/bls12_381.py, tests/points_corpus.py and the unchanged host functions
zkmi_pairing and zkmi_groth16_verify, never from the code under test.  32 lane pairs fill a wave: 33 crosses one."""
import ctypes as C
import random

import pytest

import points_corpus as pc
from conftest import golden
from oracle import bls12_381 as ec
from tower28 import _tower_to_poly

pytestmark = pytest.mark.gpu

H = bytes.fromhex
ONE = (1).to_bytes(48, "little") + bytes(528)
NO_INDEX = (1 << 64) - 1
N = 130
FAULTS = (0, 64, 129)  # first lane, wave boundary of the one-lane kernels, last lane


def _dev(b):
    import torch

    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


# ---- pairing batch --------------------------------------------------------------------------------------------------

CANARY = 0xA5


def _pairings(ctx, pairs, room=None):
    """zkmi_pairing_batch_dev over oracle points (None = infinity): the n outputs, and the bytes behind them."""
    import torch

    n = len(pairs)
    room = n if room is None else room
    g1 = _dev(b"".join(ec.g1_to_bytes(p) for p, _ in pairs) or bytes(4))
    g2 = _dev(b"".join(ec.g2_to_bytes(q) for _, q in pairs) or bytes(4))
    out = _dev(bytes([CANARY]) * (576 * max(room, 1)))
    ctx.pairing_batch_dev(g1.data_ptr(), g2.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    raw = bytes(out.cpu().numpy().tobytes())
    return [raw[576 * i : 576 * i + 576] for i in range(n)], raw[576 * n :]


@pytest.fixture(scope="module")
def pairs33():
    rnd = random.Random(41)
    a, b = rnd.randrange(2, 1 << 64), rnd.randrange(2, 1 << 64)
    pairs = [(ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R))) for _ in range(33)]
    pairs[0] = (ec.g1_mul(a), ec.g2_mul(b))
    pairs[32] = (ec.g1_mul(a * b % ec.R), ec.G2)
    pairs[31] = (ec.g1_mul((a * b + 1) % ec.R), ec.G2)
    pairs[5] = (None, pairs[5][1])
    pairs[6] = (pairs[6][0], None)
    return pairs


@pytest.mark.parametrize("n", [1, 2])
def test_pairing_batch_equals_the_host_pairing(ctx, zk, n):
    rnd = random.Random(42 + n)
    pairs = [(ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R))) for _ in range(n)]
    got, rest = _pairings(ctx, pairs)
    assert rest == b""
    for (p, q), g in zip(pairs, got):
        assert g == zk.pairing(ec.g1_to_bytes(p), ec.g2_to_bytes(q))
    assert _tower_to_poly(got[0]) == ec.final_exponentiation(ec.miller_loop(*pairs[0]))


def test_pairing_batch_across_a_wave(ctx, zk, pairs33):
    got, rest = _pairings(ctx, pairs33, room=35)
    for i in (0, 31, 32):
        p, q = pairs33[i]
        assert got[i] == zk.pairing(ec.g1_to_bytes(p), ec.g2_to_bytes(q)), i
    assert got[5] == ONE and got[6] == ONE  # P = O, Q = O
    assert rest == bytes([CANARY]) * (576 * 2)  # nothing written at index n and beyond
    # bilinearity across the wave boundary: e(a G1, b G2) = e(a b G1, G2) != e((a b + 1) G1, G2)
    assert got[0] == got[32] and got[0] != got[31] and got[0] != ONE
    assert len(set(got)) == 33 - 2  # {0, 32} and {5, 6} coincide, nothing else does


def test_pairing_batch_of_negated_points(ctx, zk):
    """(P, Q), (-P, Q), (P, -Q), (-P, -Q): in the oracle's arithmetic the first is the inverse of the second and of the third
    and equal to the fourth, so the four outputs multiply to one; none of them is one."""
    rnd = random.Random(47)
    p, q = ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R))
    np_, nq = ec.pt_neg(ec.Fq, p), ec.pt_neg(ec.Fq2, q)
    got, rest = _pairings(ctx, [(p, q), (np_, q), (p, nq), (np_, nq)])
    assert rest == b""
    e = [_tower_to_poly(g) for g in got]
    one = ec.f12_one()
    assert e[0] == ec.pairing(p, q) and e[0] != one
    assert ec.f12_mul(e[0], e[1]) == one and ec.f12_mul(e[0], e[2]) == one and e[1] == e[2] and e[3] == e[0]
    assert e[1] == ec.f12_inv(e[0])
    acc = one
    for x in e:
        acc = ec.f12_mul(acc, x)
    assert acc == one
    assert got[1] == zk.pairing(ec.g1_to_bytes(np_), ec.g2_to_bytes(q))


def test_pairing_batch_of_one_pair_32_times(ctx, zk):
    """A whole wave of lane pairs on the same operands: 32 equal outputs, the host's bytes."""
    rnd = random.Random(48)
    p, q = ec.g1_mul(rnd.randrange(1, ec.R)), ec.g2_mul(rnd.randrange(1, ec.R))
    got, rest = _pairings(ctx, [(p, q)] * 32, room=33)
    assert rest == bytes([CANARY]) * 576
    assert set(got) == {zk.pairing(ec.g1_to_bytes(p), ec.g2_to_bytes(q))}


def test_pairing_batch_of_none_writes_nothing(ctx):
    got, rest = _pairings(ctx, [], room=1)
    assert got == [] and rest == bytes([CANARY]) * 576
    out = _dev(bytes([CANARY]) * 576)
    assert ctx.lib.zkmi_pairing_batch_dev(ctx.h, None, None, C.c_uint64(0), C.c_void_p(out.data_ptr())) == 0
    assert bytes(out.cpu().numpy().tobytes()) == bytes([CANARY]) * 576
    # n > 0 with a missing array is a bad argument, and the context stays usable
    assert ctx.lib.zkmi_pairing_batch_dev(ctx.h, None, None, C.c_uint64(1), C.c_void_p(out.data_ptr())) == -1
    g1, g2 = _dev(ec.g1_to_bytes(ec.G1)), _dev(ec.g2_to_bytes(ec.G2))
    assert ctx.lib.zkmi_pairing_batch_dev(ctx.h, C.c_void_p(g1.data_ptr()), C.c_void_p(g2.data_ptr()), C.c_uint64(1), None) == -1
    assert bytes(out.cpu().numpy().tobytes()) == bytes([CANARY]) * 576


# ---- verification: helpers ------------------------------------------------------------------------------------------


def _each(ctx, pv, publics, proofs, want_status=True):
    """(return code, status bytes, first_bad) of zkmi_groth16_verify_each."""
    n = len(proofs)
    buf = lambda b: (C.c_uint8 * max(1, len(b))).from_buffer_copy(b) if len(b) else (C.c_uint8 * 1)()
    st = (C.c_uint8 * max(1, n))(*([0xEE] * max(1, n)))
    bad = C.c_uint64(12345)
    rc = ctx.lib.zkmi_groth16_verify_each(ctx.h, pv.h, C.c_uint64(n), buf(b"".join(publics)), buf(b"".join(proofs)),
                                          st if want_status else None, C.byref(bad))
    return rc, bytes(st)[:n], bad.value


def _host_status(zk, vk, public, proof):
    """The verdict of zkmi_groth16_verify on one proof as 'ok' / 'pairing' / 'malformed'."""
    try:
        return "ok" if zk.groth16_verify(vk, public, proof) else "pairing"
    except Exception as e:  # ZkmiError
        assert getattr(e, "code", None) == -2, e
        return "malformed"


def _kind(s):
    return "ok" if s == 0 else "pairing" if s == 5 else "malformed"


def _check_against_host(ctx, zk, vk, pv, publics, proofs, want=None, host_on=None):
    """Statuses of verify_each against the host verifier proof by proof (on `host_on`, default all), the exact bytes against
    `want` when given, and against the unchanged batch call with fixed weights."""
    n = len(proofs)
    rc, st, bad = _each(ctx, pv, publics, proofs)
    for i in (range(n) if host_on is None else host_on):
        assert _kind(st[i]) == _host_status(zk, vk, publics[i], proofs[i]), (i, st[i])
    if want is not None:
        assert st == want
    failing = [i for i in range(n) if st[i]]
    assert bad == (failing[0] if failing else NO_INDEX)
    assert rc == (0 if not failing else -2 if any(0 < s < 5 for s in st) else -5)
    rnd = random.Random(78)
    weights = b"".join(rnd.randrange(1, 1 << 128).to_bytes(16, "little") for _ in range(n))
    ok_b, st_b, bad_b = ctx.groth16_verify_batch(pv, b"".join(publics), b"".join(proofs), weights)
    assert (ok_b, st_b, bad_b) == (rc == 0, st, None if bad == NO_INDEX else bad)
    assert ctx.groth16_verify_each(pv, b"".join(publics), b"".join(proofs)) == (rc == 0, st, None if bad == NO_INDEX else bad)
    return rc, st, bad


# ---- public sums, through the whole call ----------------------------------------------------------------------------


def test_public_sums_with_a_crafted_key(ctx, zk):
    """The golden key with ic_0 = G, ic_1 = G, ic_2 = -2 G and the rest random multiples of G: publics that make the sum
    double a point, cancel to O, stay at ic_0, or run through every window.  With the key's exponents known a proof that
    PASSES can be made for any X = x G: A = (alpha beta + x gamma + c delta) G, B = G2, C = c G -- so a wrong X_i shows as
    status 5 where the host verifier accepts."""
    gd = golden("groth16_n128.json")
    vk0 = H(gd["vk"])
    tox = H(gd["toxic"])
    _, alpha, beta, gamma, delta = (int.from_bytes(tox[32 * k : 32 * k + 32], "little") for k in range(5))
    n_pub = (len(vk0) - 672) // 96
    np1 = n_pub - 1
    assert np1 >= 3
    rnd = random.Random(55)
    ks = [1, 1, ec.R - 2] + [rnd.randrange(1, ec.R) for _ in range(n_pub - 3)]
    vk = vk0[:672] + b"".join(ec.g1_to_bytes(ec.g1_mul(k)) for k in ks)
    pv = zk.vk_prepare(vk)
    rows = [[1] + [0] * (np1 - 1),            # G + G: the doubling case of the addition
            [1, 1] + [0] * (np1 - 2),         # G + G - 2 G = O
            [0] * np1,                        # ic_0 alone
            [ec.R - 1] * np1,                 # every window of every scalar
            [rnd.randrange(ec.R) for _ in range(np1)],
            [2, 1] + [0] * (np1 - 2),         # 3 G - 2 G: opposite-sign partial sums, a finite result
            [ec.R - 1] + [0] * (np1 - 1)]     # G - G = O through a full-length scalar
    rows += [[rnd.randrange(ec.R) for _ in range(np1)] for _ in range(66 - len(rows))]  # past one wave of the one-lane kernel
    xs = [(ks[0] + sum(p * k for p, k in zip(row, ks[1:]))) % ec.R for row in rows]
    assert xs[1] == 0 and xs[6] == 0 and xs[0] == 2 and xs[5] == 1
    publics = [b"".join(p.to_bytes(32, "little") for p in row) for row in rows]
    g2 = zk.g2_compress(ec.g2_to_bytes(ec.G2))

    def proof(x, c):
        a = (alpha * beta + x * gamma + c * delta) % ec.R
        return zk.g1_compress(ec.g1_to_bytes(ec.g1_mul(a))) + g2 + zk.g1_compress(ec.g1_to_bytes(ec.g1_mul(c)))

    good = [proof(x, rnd.randrange(1, ec.R)) for x in xs]
    host_on = list(range(8)) + [63, 64, 65]
    for i in host_on:
        assert zk.groth16_verify(vk, publics[i], good[i]) is True
    _check_against_host(ctx, zk, vk, pv, publics, good, want=bytes(len(rows)), host_on=host_on)
    # the same proofs against X + G: every equation fails, here and under the host verifier
    off = [proof((x + 1) % ec.R, 7) for x in xs]
    _check_against_host(ctx, zk, vk, pv, publics, off, want=bytes([5]) * len(rows), host_on=host_on)
    # arbitrary well-formed proofs and one public input >= r: status 4 there, 5 elsewhere
    pubs5 = publics[:4] + [publics[4][:32] + ec.R.to_bytes(32, "little") + publics[4][64:]]
    any5 = [proof(rnd.randrange(ec.R), 3) for _ in range(5)]
    _check_against_host(ctx, zk, vk, pv, pubs5, any5, want=bytes([5, 5, 5, 5, 4]))
    pv.free()


def test_a_product_that_is_one_because_two_members_cancel(ctx, zk):
    """The status path (f == 1 on the device) where e(A, B) alone equals e(alpha, beta) and the members of X and of C are
    each other's inverses: C = c G with c = -x gamma / delta, A = alpha beta G.  Accepted, as the host verifier accepts it;
    with any other c for the same A it is rejected; and with x gamma + c delta = 0 reached through A = -alpha beta G, B = -G2
    (both remaining members negated) it is accepted again."""
    gd = golden("groth16_n128.json")
    vk0 = H(gd["vk"])
    tox = H(gd["toxic"])
    _, alpha, beta, gamma, delta = (int.from_bytes(tox[32 * k : 32 * k + 32], "little") for k in range(5))
    n_pub = (len(vk0) - 672) // 96
    rnd = random.Random(56)
    ks = [rnd.randrange(1, ec.R) for _ in range(n_pub)]
    vk = vk0[:672] + b"".join(ec.g1_to_bytes(ec.g1_mul(k)) for k in ks)
    pv = zk.vk_prepare(vk)
    g2 = zk.g2_compress(ec.g2_to_bytes(ec.G2))
    ng2 = zk.g2_compress(ec.g2_to_bytes(ec.pt_neg(ec.Fq2, ec.G2)))
    g1c = lambda k: zk.g1_compress(ec.g1_to_bytes(ec.g1_mul(k % ec.R)))
    publics, proofs, want = [], [], []
    for i in range(33):  # past one wave of lane pairs
        row = [rnd.randrange(ec.R) for _ in range(n_pub - 1)]
        x = (ks[0] + sum(p * k for p, k in zip(row, ks[1:]))) % ec.R
        c = (-x * gamma * pow(delta, -1, ec.R)) % ec.R
        assert x and c and (x * gamma + c * delta) % ec.R == 0
        publics.append(b"".join(p.to_bytes(32, "little") for p in row))
        kind = i % 3
        if kind == 0:
            proofs.append(g1c(alpha * beta) + g2 + g1c(c)), want.append(0)
        elif kind == 1:
            proofs.append(g1c(alpha * beta) + g2 + g1c(c + 1)), want.append(5)
        else:
            proofs.append(g1c(-alpha * beta) + ng2 + g1c(c)), want.append(0)
    _check_against_host(ctx, zk, vk, pv, publics, proofs, want=bytes(want), host_on=(0, 1, 2, 31, 32))
    pv.free()


# ---- verdicts on real proofs ----------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def batch(ctx, zk):
    """130 proofs of distinct witnesses of the N = 128 golden relation under the golden key, proved on the device."""
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
    yield {"vk": vk, "pv": pv, "proofs": proofs, "publics": publics, "n_pub": r1.n_pub}
    pv.free()
    r1.free()


def test_all_good_proofs_are_accepted(ctx, zk, batch):
    rc, st, bad = _check_against_host(ctx, zk, batch["vk"], batch["pv"], batch["publics"], batch["proofs"], host_on=FAULTS)
    assert (rc, st, bad) == (0, bytes(N), NO_INDEX)
    assert ctx.groth16_verify_each(batch["pv"], b"".join(batch["publics"]), b"".join(batch["proofs"])) == (True, bytes(N), None)


def test_one_fault_of_each_kind(ctx, zk, batch):
    """Index 0: a public input of another proof; 64: C of another proof; 129: A replaced by a corrupted compressed point."""
    enc, chk = pc.ENC_COMPRESSED, pc.CHECK_SUBGROUP
    first = lambda cls: next(b for c, b in pc.corpus(1, enc) if c == cls)
    for cls in ("x_ge_p", "no_root", "off_subgroup"):
        publics, proofs = list(batch["publics"]), list(batch["proofs"])
        publics[0] = batch["publics"][3]
        proofs[64] = proofs[64][:144] + batch["proofs"][71][144:]
        proofs[129] = first(cls) + proofs[129][48:]
        want = bytearray(N)
        want[0], want[64], want[129] = 5, 5, pc.class_status(cls, enc, chk)
        assert 1 <= want[129] <= 3
        rc, st, bad = _check_against_host(ctx, zk, batch["vk"], batch["pv"], publics, proofs, want=bytes(want),
                                          host_on=(0, 1, 64, 65, 129))
        assert (rc, bad) == (-2, 0)
    # the two equation faults alone: a rejected batch, not a malformed one; first_bad is the smallest failing index
    publics, proofs = list(batch["publics"]), list(batch["proofs"])
    proofs[64] = proofs[64][:144] + batch["proofs"][71][144:]
    publics[129] = batch["publics"][3]
    want = bytearray(N)
    want[64] = want[129] = 5
    rc, st, bad = _check_against_host(ctx, zk, batch["vk"], batch["pv"], publics, proofs, want=bytes(want), host_on=(63, 64, 129))
    assert (rc, bad) == (-5, 64)


def test_every_proof_bad(ctx, zk, batch):
    publics = batch["publics"][1:] + batch["publics"][:1]  # proof i gets the publics of proof i + 1
    rc, st, bad = _check_against_host(ctx, zk, batch["vk"], batch["pv"], publics, batch["proofs"], want=bytes([5]) * N,
                                      host_on=FAULTS)  # (the batch call bisects: 2 N - 1 host exponentiations)
    assert (rc, bad) == (-5, 0)


@pytest.mark.parametrize("n", [1, 2])
def test_small_batches(ctx, zk, batch, n):
    vk, pv, publics, proofs = batch["vk"], batch["pv"], batch["publics"][:n], batch["proofs"][:n]
    rc, st, bad = _check_against_host(ctx, zk, vk, pv, publics, proofs)
    assert (rc, st, bad) == (0, bytes(n), NO_INDEX)
    bad_last = proofs[:-1] + [proofs[-1][:144] + batch["proofs"][9][144:]]
    rc, st, bad = _check_against_host(ctx, zk, vk, pv, publics, bad_last)
    assert (rc, st, bad) == (-5, bytes(n - 1) + b"\x05", n - 1)


# ---- arguments ------------------------------------------------------------------------------------------------------


def test_bad_arguments_launch_nothing(ctx, zk, batch):
    pv, publics, proofs = batch["pv"], batch["publics"][:2], batch["proofs"][:2]
    assert _each(ctx, pv, publics, proofs, want_status=False)[0] == -1  # out_status is required
    st = (C.c_uint8 * 2)(0xEE, 0xEE)
    pub = (C.c_uint8 * len(b"".join(publics))).from_buffer_copy(b"".join(publics))
    prf = (C.c_uint8 * 384).from_buffer_copy(b"".join(proofs))
    lib = ctx.lib
    assert lib.zkmi_groth16_verify_each(ctx.h, pv.h, C.c_uint64(2), pub, None, st, None) == -1
    assert lib.zkmi_groth16_verify_each(ctx.h, pv.h, C.c_uint64(2), None, prf, st, None) == -1
    assert lib.zkmi_groth16_verify_each(ctx.h, None, C.c_uint64(2), pub, prf, st, None) == -1
    assert lib.zkmi_groth16_verify_each(None, pv.h, C.c_uint64(2), pub, prf, st, None) == -1
    assert lib.zkmi_groth16_verify_each(ctx.h, pv.h, C.c_uint64(0), None, None, None, None) == -1
    assert bytes(st) == b"\xee\xee"
    bad = C.c_uint64(5)
    assert lib.zkmi_groth16_verify_each(ctx.h, pv.h, C.c_uint64(0), None, None, st, C.byref(bad)) == 0  # n = 0
    assert bytes(st) == b"\xee\xee" and bad.value == NO_INDEX
    # a key of another n_pub: the binding refuses the publics' length before the library is called
    vk = batch["vk"]
    shorter = zk.vk_prepare(vk[: len(vk) - 96])
    with pytest.raises(Exception) as ei:
        ctx.groth16_verify_each(shorter, b"".join(publics), b"".join(proofs))
    assert getattr(ei.value, "code", None) == -1
    shorter.free()
    # a good call on the same context afterwards
    assert _each(ctx, pv, publics, proofs) == (0, bytes(2), NO_INDEX)
