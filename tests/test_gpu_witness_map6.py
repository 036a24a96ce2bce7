"""The six-transform witness map (groth16.hip witness_map_dev): c stays in coefficient form and is subtracted in the
epilogue of the last inverse transform, h = (coset-iNTT(a_c * b_c) - c) / (g^N - 1).  Both forms compute
(a b mod (X^N - g^N) - c) / (g^N - 1), so h must equal the oracle's seven-transform map word for word -- for witnesses
that satisfy the relation and for one that does not.

Sizes: 2^1 (one butterfly, the single-pass edge), 2^4, 2^10 (the largest one-pass plan), 2^11 and 2^12 (two passes with a
short second pass).  The shielder relation starts at 2^7, so the two smallest domains use a chain of products
z_(i+1) = (3 z_i + 1) z_i with padding rows; from 2^10 on it is shielder_r1cs(log_n)."""
import pytest

from oracle import bls12_381 as ec
from oracle.bls12_381 import R

pytestmark = pytest.mark.gpu


def frs(vals):
    return b"".join(ec.fr_to_bytes(v) for v in vals)


def _chain_relation(zk, lg, seed):
    """(r1cs, witness bytes): nc constraints (3 z_i + z_0) * z_i = z_(i+1) over n_pub = 1; nc + 1 < 2^lg for lg > 1, so the
    domain has padding rows"""
    nc = 1 if lg == 1 else (1 << lg) - 4
    n_vars = nc + 2
    one, three = (1).to_bytes(32, "little"), (3).to_bytes(32, "little")
    rp2, rp1 = [2 * i for i in range(nc + 1)], list(range(nc + 1))
    a = (rp2, [c for i in range(nc) for c in (0, i + 1)], (one + three) * nc)
    b = (rp1, [i + 1 for i in range(nc)], one * nc)
    c = (rp1, [i + 2 for i in range(nc)], one * nc)
    r1 = zk.r1cs_create(n_vars, 1, [a, b, c])
    assert r1.log_n == lg
    z = [1, ec.SplitMix64(seed).fr()]
    for i in range(nc):
        z.append((3 * z[-1] + 1) * z[-1] % R)
    return r1, frs(z)


def _relation(zk, lg, seed):
    if lg < 7:
        return _chain_relation(zk, lg, seed)
    return zk.shielder_r1cs(lg), zk.shielder_witness(lg, seed)


@pytest.fixture(scope="module")
def ocpp():
    from oracle import cpp

    cpp.build()
    return cpp


@pytest.mark.parametrize("lg", [1, 4, 10, 11, 12])
def test_witness_map_words_vs_cpp_oracle(ctx, zk, ocpp, lg):
    rng = ec.SplitMix64(0x6E77 + lg)
    r1 = _relation(zk, lg, 1)[0]
    pk, _ = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    mats = [r1.export(m) for m in range(3)]
    for seed in (61 + lg, 0xC0FFEE + lg):
        z = _relation(zk, lg, seed)[1]
        assert r1.is_satisfied(z)
        want = ocpp.witness_map(r1.n_vars, r1.n_pub, r1.n_constraints, lg, mats, z)
        assert ctx.groth16_witness_map(pk, z) == want, (lg, seed)
    pk.free()
    r1.free()


def test_witness_map_of_an_unsatisfied_witness_vs_cpp_oracle(ctx, zk, ocpp):
    """One variable of a valid assignment replaced: a b - c is no multiple of X^N - 1 any more, and the six-transform form
    must still give the words of the seven-transform one (the quotient of the division by X^N - g^N on the coset)."""
    lg = 11
    r1, z = _relation(zk, lg, 77)
    rng = ec.SplitMix64(0xBAD5EED)
    pk, _ = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    k = r1.n_vars // 2
    bad = z[: 32 * k] + ec.fr_to_bytes((int.from_bytes(z[32 * k: 32 * k + 32], "little") + 12345) % R) + z[32 * k + 32:]
    assert r1.is_satisfied(z) and not r1.is_satisfied(bad)
    mats = [r1.export(m) for m in range(3)]
    want = ocpp.witness_map(r1.n_vars, r1.n_pub, r1.n_constraints, lg, mats, bad)
    assert want != ocpp.witness_map(r1.n_vars, r1.n_pub, r1.n_constraints, lg, mats, z)
    assert ctx.groth16_witness_map(pk, bad) == want
    pk.free()
    r1.free()


def test_group_of_five_proofs_vs_cpp_oracle(ctx, zk, ocpp):
    """The batched route: five different witnesses at 2^11 through groth16_prove_batch_dev go through the map as ONE group
    (a | b | c vectors of the group back to back, the layout follows the group size); all 192 bytes of every proof against
    the oracle's prover over the oracle's own setup."""
    import torch

    lg, G = 11, 5
    r1 = zk.shielder_r1cs(lg)
    rng = ec.SplitMix64(0x6F1E)
    toxic = frs([rng.fr() for _ in range(5)])
    pk, vk = ctx.groth16_setup(r1, toxic)
    mats = [r1.export(m) for m in range(3)]
    ovk, okey = ocpp.groth16_setup(r1.n_vars, r1.n_pub, r1.n_constraints, lg, mats, toxic)
    assert vk == ovk
    wits = [zk.shielder_witness(lg, 1100 + i) for i in range(G)]
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(G)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(G)]
    want = [ocpp.groth16_prove(r1.n_vars, r1.n_pub, r1.n_constraints, lg, mats, okey, w, r_, s_) for w, r_, s_ in zip(wits, rs, ss)]
    assert len(set(want)) == G
    d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
    torch.cuda.synchronize()
    got = ctx.groth16_prove_batch_dev(pk, [t.data_ptr() for t in d], rs, ss)
    assert got == want
    pk.free()
    r1.free()
