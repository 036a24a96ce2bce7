"""CPU suite for the device point readers (csrc/points.hip): the C ABI's argument checks without a GPU, the test-vector
corpus of tests/points_corpus.py held to the oracle and to the product's host functions, and the register / scratch
allocation DESIGN.md states for the new kernels."""
import ctypes as C
import os
import re
import sys
from collections import Counter

import pytest

import points_corpus as pc
from conftest import ROOT
from oracle import bls12_381 as ec

NEW = ["zkmi_g1_points_read_dev", "zkmi_g2_points_read_dev", "zkmi_bases_g1_load_encoded", "zkmi_bases_g2_load_encoded",
       "zkmi_ark_pk_load_validated", "zkmi_pk_check"]


def test_new_entry_points_are_declared_exported_and_bound(zk, pkg):
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    declared = set(re.findall(r"\b(zkmi_[a-z0-9_]+)\s*\(", hdr))
    rs = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    for n in NEW:
        assert n in declared and hasattr(zk.lib, n) and hasattr(zk.tlib, n), n
    for n in ("zkmi_ark_pk_load_validated", "zkmi_pk_check"):
        assert re.search(r"pub fn %s\s*\(" % n, rs), n
    # the constants of the header, the binding and the corpus are one set
    for name, val in (("ENC_WIRE", 0), ("ENC_ZCASH_COMPRESSED", 1), ("ENC_ZCASH_UNCOMPRESSED", 2), ("CHECK_CURVE", 1),
                      ("CHECK_SUBGROUP", 2), ("PT_OK", 0), ("PT_BAD_ENCODING", 1), ("PT_NOT_ON_CURVE", 2),
                      ("PT_NOT_IN_SUBGROUP", 3)):
        assert re.search(r"#define ZKMI_%s %d\b" % (name, val), hdr), name
        assert getattr(pkg, name) == val
    assert (pc.ENC_WIRE, pc.ENC_COMPRESSED, pc.ENC_UNCOMPRESSED) == (0, 1, 2)
    assert (pc.OK, pc.BAD_ENCODING, pc.NOT_ON_CURVE, pc.NOT_IN_SUBGROUP) == (0, 1, 2, 3)
    for m in ("g1_points_read_dev", "g2_points_read_dev", "bases_g1_encoded", "bases_g2_encoded", "ark_pk_load_validated"):
        assert callable(getattr(pkg.Context, m))
    from zk_apps_amd import binding

    assert callable(binding.ProvingKey.check)


def test_shape_errors_are_bad_arg_before_any_gpu_work(zk):
    """NULL / zero / unknown arguments: ZKMI_ERR_BAD_ARG, with no context and no device (this process has neither)."""
    lib = zk.lib
    bad = C.c_uint64(7)
    buf = (C.c_uint8 * 192)()
    h = C.c_void_p()
    where = (C.c_uint64 * 2)()
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below is refused on its other arguments
    for fn in (lib.zkmi_g1_points_read_dev, lib.zkmi_g2_points_read_dev):
        assert fn(None, buf, C.c_uint64(1), 0, 0, None, None, C.byref(bad)) == -1  # no context
        assert fn(fake, None, C.c_uint64(1), 0, 0, None, None, C.byref(bad)) == -1  # no input
        assert fn(fake, fake, C.c_uint64(0), 0, 0, None, None, C.byref(bad)) == -1  # n == 0
        assert fn(fake, fake, C.c_uint64(1), 3, 0, None, None, C.byref(bad)) == -1  # unknown encoding
        assert fn(fake, fake, C.c_uint64(1), -1, 0, None, None, C.byref(bad)) == -1
        assert fn(fake, fake, C.c_uint64(1), 1, 4, None, None, C.byref(bad)) == -1  # unknown check bit
        assert fn(fake, C.c_void_p(0x1001), C.c_uint64(1), 0, 0, None, None, C.byref(bad)) == -1  # misaligned input
    for fn in (lib.zkmi_bases_g1_load_encoded, lib.zkmi_bases_g2_load_encoded):
        assert fn(None, buf, C.c_uint64(1), 0, 0, C.byref(h), C.byref(bad)) == -1
        assert fn(fake, None, C.c_uint64(1), 0, 0, C.byref(h), C.byref(bad)) == -1
        assert fn(fake, buf, C.c_uint64(0), 0, 0, C.byref(h), C.byref(bad)) == -1
        assert fn(fake, buf, C.c_uint64(1), 0, 0, None, C.byref(bad)) == -1
        assert fn(fake, buf, C.c_uint64(1), 5, 0, C.byref(h), C.byref(bad)) == -1
        assert fn(fake, buf, C.c_uint64(1), 0, 8, C.byref(h), C.byref(bad)) == -1
    assert not h.value
    f = lib.zkmi_ark_pk_load_validated
    assert f(None, fake, buf, C.c_uint64(192), 1, 2, C.byref(h), None, C.c_uint64(0), where) == -1
    assert f(fake, None, buf, C.c_uint64(192), 1, 2, C.byref(h), None, C.c_uint64(0), where) == -1
    assert f(fake, fake, None, C.c_uint64(192), 1, 2, C.byref(h), None, C.c_uint64(0), where) == -1
    assert f(fake, fake, buf, C.c_uint64(192), 1, 2, None, None, C.c_uint64(0), where) == -1
    assert f(fake, fake, buf, C.c_uint64(192), 1, 16, C.byref(h), None, C.c_uint64(0), where) == -1
    assert lib.zkmi_pk_check(None, fake, 2, where) == -1
    assert lib.zkmi_pk_check(fake, None, 2, where) == -1
    assert lib.zkmi_pk_check(fake, fake, 0, where) == -1
    assert lib.zkmi_pk_check(fake, fake, 4, where) == -1
    assert bad.value == 7 and not h.value


def test_cofactors_and_small_order_recipe():
    """The facts the corpus stands on, from the oracle: [r h]P = O on both curves, a random curve point is outside the
    subgroup, T = [r h / q^e]P has order q, and [k]G + T is on the curve and fails [r]."""
    import random

    rnd = random.Random(11)
    for group in (1, 2):
        F, b, h = pc.field(group)
        gen = ec.G1 if group == 1 else ec.G2
        p = pc.random_curve_point(group, rnd)
        assert ec.on_curve(F, b, p) and ec.pt_mul(F, p, pc.R * h) is None and ec.pt_mul(F, p, pc.R) is not None
        for q, e in pc.SMALL_ORDERS[group]:
            t = pc.small_order_point(group, q, e, rnd)
            assert t is not None and ec.pt_mul(F, t, q) is None and ec.on_curve(F, b, t)
            m = ec.pt_add(F, ec.pt_mul(F, gen, rnd.randrange(1, pc.R)), t)
            assert ec.on_curve(F, b, m) and ec.pt_mul(F, m, pc.R) is not None


@pytest.mark.parametrize("group", [1, 2])
def test_corpus_classes_get_the_oracles_status(zk, group):
    """Every element of the corpus, in every encoding and for both check levels: the status its class stands for is the
    one the oracle computes from the bytes, and the one the product's host functions imply.  Every class is there, with
    at least 64 (G1) / 16 (G2) members: a corpus of valid points alone would test nothing."""
    host_decompress = zk.g1_decompress if group == 1 else zk.g2_decompress
    host_in_subgroup = zk.g1_in_subgroup if group == 1 else zk.g2_in_subgroup
    for enc in (pc.ENC_WIRE, pc.ENC_COMPRESSED, pc.ENC_UNCOMPRESSED):
        items = pc.corpus(group, enc)
        counts = Counter(cls for cls, _ in items)
        assert set(counts) == pc.expected_classes(group, enc), (enc, sorted(counts))
        for cls, n in counts.items():
            assert n >= pc.MIN_MEMBERS[group], (group, enc, cls, n)
        sort_bits = Counter()
        for cls, b in items:
            assert len(b) == pc.point_bytes(group, enc)
            for checks in (0, pc.CHECK_CURVE, pc.CHECK_SUBGROUP):
                assert pc.oracle_status(group, enc, b, checks) == pc.class_status(cls, enc, checks), (group, enc, cls, checks)
            if enc == pc.ENC_COMPRESSED:
                # host path: zkmi_g{1,2}_decompress accepts exactly what is canonical and on the curve, and returns the
                # oracle's point; zkmi_g{1,2}_in_subgroup then separates status 0 from 3
                want = pc.class_status(cls, enc, pc.CHECK_SUBGROUP)
                try:
                    wire = host_decompress(b)
                except Exception:
                    wire = None
                assert (wire is None) == (want in (pc.BAD_ENCODING, pc.NOT_ON_CURVE)), (group, cls)
                if wire is not None:
                    pt = ec.g1_decompress(b) if group == 1 else ec.g2_decompress(b)
                    assert wire == (ec.g1_to_bytes(pt) if group == 1 else ec.g2_to_bytes(pt))
                    assert bool(host_in_subgroup(wire)) == (want == pc.OK), (group, cls)
                    if cls == "valid" and pt is not None:
                        sort_bits[bool(b[0] & 0x20)] += 1
        if enc == pc.ENC_COMPRESSED:
            assert sort_bits[True] >= 4 and sort_bits[False] >= 4, sort_bits
            assert sum(1 for cls, b in items if cls == "valid" and b[0] == 0xC0) >= 2  # infinity is among the valid ones


def test_point_reader_kernel_allocations():
    """What DESIGN.md ("Key ingest") states about the new kernels, read from the code objects of the built library: the
    G1 readers fit two waves per SIMD (256 registers) with no scratch; the G2 readers (one lane per point on Fq2_28) take
    a whole SIMD's 512 registers and at most 64 bytes of scratch per lane.  None of them uses LDS or a dynamic stack."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    ks = {kr.short_name(n): v for n, v in kr.kernels(os.path.join(ROOT, "zk-apps_amd", "libzkmi.so")).items()}
    for enc in range(4):  # the three encodings and the resident form
        g1, g2 = ks["k_points_read<1,%d>" % enc], ks["k_points_read<2,%d>" % enc]
        assert g1["vgpr"] + g1["agpr"] <= 256 and g1["scratch"] == 0, g1
        assert g2["vgpr"] <= 512 and g2["scratch"] <= 64, g2
        for k in (g1, g2):
            assert k["lds"] == 0 and not k["dynamic_stack"] and k["max_wg"] == 64, k
