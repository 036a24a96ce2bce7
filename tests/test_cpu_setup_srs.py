"""CPU suite: phase-1 transcripts and the transform of point arrays.  The big-integer model of tests/setup_srs_model.py --
the reference the GPU tests lean on -- against oracle.groth16.lagrange_at, and the new entry points' refusals without a
context."""
import ctypes as C

from oracle import bls12_381 as ec
from oracle import groth16 as g16
from oracle import ntt as nt

import setup_srs_model as model

R = ec.R
TAU, ALPHA, BETA = 0x1D0C5A7E5EED0001 % R, 0x2A11FA0000000007 * 0x10001 % R, (R - 0xBE7A) % R


def test_idft_of_powers_is_the_lagrange_basis():
    """The convention the point transform has to follow: the inverse DFT of the powers of tau, natural order in and out and
    scaled by N^-1, is [L_i(tau)] -- in the field (oracle.ntt) and in the exponent (the model's O(N^2) definition)."""
    for log_n in (1, 3):
        n = 1 << log_n
        L = g16.lagrange_at(log_n, TAU)
        assert nt.ntt([pow(TAU, i, R) for i in range(n)], inverse=True) == L
        for group, mul in ((1, ec.g1_mul), (2, ec.g2_mul)):
            assert model.dft_points(group, [mul(pow(TAU, i, R)) for i in range(n)], inverse=True) == [mul(v) for v in L]
    # forward and inverse are inverses of each other, infinity entries included
    pts = [ec.g1_mul(3), None, ec.g1_mul(R - 5), ec.g1_mul(3)]
    assert model.dft_points(1, model.dft_points(1, pts), inverse=True) == pts


def test_new_entry_points_refuse_null_arguments(zk):
    """NULL context / NULL out pointers: ZKMI_ERR_BAD_ARG, not a crash (no device is touched)."""
    lib = zk.lib
    buf = (C.c_uint8 * 1024)()
    h = C.c_void_p()
    out3 = (C.c_uint64 * 3)()
    where = (C.c_uint64 * 2)()
    u64, u32, i32 = C.c_uint64, C.c_uint32, C.c_int32
    fake = C.c_void_p(8)  # never dereferenced: every call below is refused before it looks at it
    assert lib.zkmi_g1_points_ntt_dev(None, fake, u32(3), i32(0)) == -1
    assert lib.zkmi_g2_points_ntt_dev(None, fake, u32(3), i32(1)) == -1
    assert lib.zkmi_srs_load(None, i32(0), i32(2), buf, u64(1), buf, u64(1), buf, buf, u64(1), buf, C.byref(h), where) == -1
    assert h.value is None
    assert lib.zkmi_srs_generate(None, buf, u32(3), C.byref(h)) == -1 and h.value is None
    assert lib.zkmi_srs_shape(None, out3) == -1
    assert lib.zkmi_srs_read(None, None, i32(0), u64(0), u64(1), buf) == -1
    assert lib.zkmi_srs_free(None) == -1
