"""CPU suite: the weight derivation of the ceremony checks (zkmi_srs_verify, zkmi_pk_verify_contribution) and their public
surface.  The per-index body k_rlc_weights runs is held to hashlib through the host loop of the testing library before
anything reaches a GPU."""
import hashlib
import os
import re
import struct

from conftest import ROOT

SEEDS = (bytes(range(32)), hashlib.sha256(b"ceremony seed two").digest())
DOMS = (0, 3, 20)
INDICES = (0, 1, 63, 64, 255, 256, 1 << 32, (1 << 40) + 5)


def weight(seed, dom, i):
    """include/zkmi.h: the first 16 bytes of SHA-256(seed | LE32(dom) | LE64(i))."""
    return hashlib.sha256(seed + struct.pack("<IQ", dom, i)).digest()[:16]


def test_weights_equal_hashlib(zk):
    for seed in SEEDS:
        for dom in DOMS:
            for i in INDICES:
                assert zk.selftest_rlc_weights_host(seed, dom, i, 1) == weight(seed, dom, i), (dom, i)


def test_weight_ranges_are_the_single_weights_in_order(zk):
    """first / count walk consecutive indices, across the 2^32 carry of LE64(i) as well."""
    seed = SEEDS[1]
    for first, count in ((0, 300), ((1 << 32) - 2, 5)):
        got = zk.selftest_rlc_weights_host(seed, 1, first, count)
        assert got == b"".join(weight(seed, 1, first + k) for k in range(count))
    assert zk.selftest_rlc_weights_host(seed, 1, 7, 0) == b""


def test_different_domain_or_index_gives_a_different_weight(zk):
    seed = SEEDS[0]
    seen = {}
    for dom in (0, 1, 2, 3, 19, 20):
        for i in range(64):
            w = zk.selftest_rlc_weights_host(seed, dom, i, 1)
            assert w not in seen, ((dom, i), seen[w])
            seen[w] = (dom, i)
    # (dom, i) is not a concatenation that another pair can spell: LE32(1) | LE64(0) against LE32(0) | LE64(1 << 32) differ
    assert zk.selftest_rlc_weights_host(seed, 1, 0, 1) != zk.selftest_rlc_weights_host(seed, 0, 1 << 32, 1)
    assert zk.selftest_rlc_weights_host(SEEDS[1], 0, 0, 1) != zk.selftest_rlc_weights_host(seed, 0, 0, 1)


def test_public_surface(zk, pkg):
    """The four functions and the masks are declared in include/zkmi.h, exported, and wrapped by the binding; the header no
    longer leaves the checks to the caller."""
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    for fn in ("zkmi_g1_points_adjacent_sums_dev", "zkmi_g2_points_adjacent_sums_dev", "zkmi_srs_verify", "zkmi_pk_verify_contribution"):
        assert re.search(r"\bint32_t %s\s*\(" % fn, hdr), fn
        assert hasattr(zk.lib, fn) and hasattr(zk.tlib, fn), fn
    masks = {"ZKMI_SRS_BAD_TAU_G1": 1, "ZKMI_SRS_BAD_TAU_G2": 2, "ZKMI_SRS_BAD_ALPHA": 4, "ZKMI_SRS_BAD_BETA": 8, "ZKMI_SRS_BAD_BETA_G2": 16,
             "ZKMI_SRS_DEGENERATE": 32, "ZKMI_PK2_FIXED_PART_DIFFERS": 1, "ZKMI_PK2_BAD_DELTA": 2, "ZKMI_PK2_BAD_H": 4, "ZKMI_PK2_BAD_L": 8}
    for name, value in masks.items():
        m = re.search(r"#define\s+%s\s+(\d+)u\b" % name, hdr)
        assert m and int(m.group(1)) == value, name
        assert getattr(pkg, name[len("ZKMI_"):]) == value, name
    for method in ("srs_verify", "pk_verify_contribution", "points_adjacent_sums_dev"):
        assert callable(getattr(pkg.Context, method)), method
    assert callable(pkg.Srs.verify) and callable(pkg.ProvingKey.verify_contribution)
    assert "are the caller's. */" not in hdr and "verify it before it gets here" not in hdr
    thdr = open(os.path.join(ROOT, "include", "zkmi_testing.h")).read()
    assert "zkmi_selftest_rlc_weights_host" in thdr and not hasattr(zk.lib, "zkmi_selftest_rlc_weights_host")
