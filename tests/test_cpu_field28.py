"""The limb arithmetic of zk-apps_amd/csrc/field28.hpp on the HOST path of zkmi_selftest_fp28_ops (ctx == NULL: the same
templated body the device kernels run), all four parameter sets, every operand a RAW limb array in a representation
x + k p up to the |v| < 16 p bound the header states, against Python integers (tests/limbs28.py).  Exact, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import limbs28 as lb

FIELD_IDS = [f.name for f in lb.FIELDS]


def test_limb_helpers_and_constants():
    for f in lb.FIELDS:
        for v in (0, 1, -1, f.p, -16 * f.p + 1, 16 * f.p - 1, f.R1, f.R2):
            limbs = lb.to_limbs(v, f.NL)
            assert lb.normalised(limbs) and lb.from_limbs(limbs) == v
        assert lb.to_limbs(-1, f.NL) == [lb.MASK] * (f.NL - 1) + [-1]
        assert (f.p * f.INV + 1) % (1 << 28) == 0
        assert f.mont(f.R2) == f.R1 and f.value(f.rep(5)) == 5
    fq, fr, bq, br = lb.FIELDS
    # the constants field28.hpp carries (INV of every parameter set; top limbs of p)
    assert (fq.INV, fr.INV, bq.INV, br.INV) == (0xFFCFFFD, 0xFFFFFFF, 0x4866389, 0xFFFFFFF)
    assert lb.to_limbs(fq.p, 14)[-1] == 0x1A011 and lb.to_limbs(fr.p, 10)[-1] == 7 and lb.to_limbs(br.p, 10)[-1] == 3


def test_vectors_cover_what_they_claim():
    for f in lb.FIELDS:
        vec = lb.vectors(f)
        nk = len(lb.KS)
        assert len(vec.vals) == vec.nr * nk - 1  # only 0 - 16 p is dropped
        assert max(vec.vals) == 16 * f.p - 1 and min(vec.vals) == -16 * f.p + 1
        rev = {i: key for key, i in vec.index.items()}
        for arity in (2, 4, 8):
            tuples = vec.tuples(arity)
            assert len(tuples) <= 1 << 15
            first = {rev[t[0]] for t in tuples}
            assert first == set(vec.index)  # every residue meets every k
            pairs = {(rev[t[0]][1], rev[t[1]][1]) for t in tuples}
            assert len(pairs) == nk * nk  # every (k_a, k_b)
        if f.id == 0:
            assert any((1 << 380) < x < f.p for x in vec.res)
        assert sum(1 for x in vec.res if x >= 1 << (f.p.bit_length() - 1)) >= 8  # draws over all of [0, p)


@pytest.mark.parametrize("f", lb.FIELDS, ids=FIELD_IDS)
def test_host_ops(zk, f):
    for name in lb.op_names(f, device=False):
        lb.check_op(zk, None, f, name)


@pytest.mark.parametrize("f", lb.FIELDS, ids=FIELD_IDS)
def test_host_is_zero_and_conversions(zk, f):
    lb.check_is_zero(zk, None, f)
    lb.check_from_canonical(zk, None, f)
    lb.check_to_canonical(zk, None, f)


def test_ops_a_field_or_path_lacks_are_refused(zk):
    fq, fr = lb.FIELDS[0], lb.FIELDS[1]
    block = np.zeros((1, 8 * 14), dtype=np.int32)
    out = np.zeros((1, 4 * 14), dtype=np.int32)
    flag = np.zeros(2, dtype=np.uint8)

    def rc(f, op):
        return zk.tlib.zkmi_selftest_fp28_ops(C.c_void_p(None), C.c_int32(f.id), C.c_int32(op), C.c_uint32(1),
                                              block.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                              flag.ctypes.data_as(C.c_void_p))

    for op in (15, 16, 17, 18):
        assert rc(fq, op) == 0 and rc(fr, op) == -1  # Fq2 forms: Fq28 only
    for op in (19, 20, 21, 22, 23):
        assert rc(fq, op) == -1  # lane-pair forms: device only
    assert rc(fq, 28) == -1 and rc(fq, -1) == -1 and rc(lb.Field(4, "none", 7, 10, 8), 0) == -1


def test_lane_pair_tuple_counts_leave_a_partial_wave():
    """The device test runs the Fq2P forms on 2 n lanes in 64-lane blocks: the last wave must be partly filled."""
    f = lb.FIELDS[0]
    for name in ("pair_mul", "pair_sqr", "pair_mul_sub_mul", "pair_signed_sub"):
        n = len(lb.vectors(f).tuples(lb.OPS[name]["n_in"]))
        assert (2 * n) % 64 != 0, (name, n)


@pytest.mark.parametrize("f", [lb.FIELDS[1], lb.FIELDS[3]], ids=["Fr28", "BnFr28"])
def test_ntt_closed_forms_match_the_oracle_at_16_points(f):
    """The closed forms test_gpu_field28.py holds the device to, against the oracle's transforms (oracle/ntt.py, oracle/bn254.py)
    and, for the bit-reversed decimation-in-frequency hook, against the defining sum."""
    from oracle import bn254 as bn
    from oracle import ntt as ontt

    log_n, n, r = 4, 16, f.p

    def transform(a, inverse, coset):
        if f.id == 3:
            return bn.ntt(a, inverse=inverse, coset=coset)
        if coset:
            return ontt.coset_intt(a) if inverse else ontt.coset_ntt(a)
        return ontt.ntt(a, inverse=inverse)

    w_inv = pow(lb.ntt_root(f, log_n), -1, r)
    rev = [int(format(i, "04b")[::-1], 2) for i in range(n)]
    for c in lb.ntt_constants(f):
        for vec in ("const", "alt"):
            pat = lb.ntt_input(vec, c, r)
            a = [pat[i % len(pat)] for i in range(n)]
            for way in ("fwd", "inv", "fwd_coset", "inv_coset", "dif0", "dif1"):
                want = lb.ntt_closed_form(f, vec + "_" + way, log_n, c)
                if way.startswith("dif"):
                    ref = [sum(a[i] * pow(w_inv, i * rev[p], r) for i in range(n)) % r for p in range(n)]
                    if way == "dif1":
                        ref = [v * pow(lb.NTT_G, rev[p], r) * pow(n, -1, r) % r for p, v in enumerate(ref)]
                else:
                    ref = transform(a, way.startswith("inv"), way.endswith("coset"))
                got = [want(k) for k in range(n)] if callable(want) else [want.get(k, 0) for k in range(n)]
                assert got == ref, (f.name, vec, way, c)
