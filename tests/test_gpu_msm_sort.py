"""The digit sort every MSM starts with (csrc/msm_sort.hip) against tests/sort_model.py, at its partition and round edges.

One parameter per named vector of tests/sort_cases.py: upload, read the context's own sort out through the testing library
(zkmi_selftest_msm_sort_dev), assert the kernel chain the vector is built for, and hold count / begin / sorted / perm / heavy
to the model.  test_cpu_msm_sort.py proves without a GPU that each vector hits the threshold it is named for.

For the designed vectors the whole MSM runs too, through the product's entry points over the synthetic bases P_i = [1 + i
0xC0FFEE] G, against the closed form [sum_i s_i (1 + i 0xC0FFEE)] G: the accumulation's handling of these bucket shapes, tied to
the sort's."""
import pytest

import sort_cases as sc_
import sort_model as sm
from oracle import bls12_381 as ec

pytestmark = pytest.mark.gpu


def _upload(sc):
    import torch

    d = torch.frombuffer(bytearray(sm.scalars_to_bytes(sc)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", list(sc_.CASES))
def test_sort_matches_the_model(zk, ctx, name):
    case = sc_.get(name, zk)
    shape = zk.selftest_msm_sort_shape()
    d = _upload(case["sc"])
    info, count, begin, perm, heavy, srt = ctx.selftest_msm_sort_dev(d.data_ptr(), case["n"], case["mode"], case["plan_n"], case["batch"])
    print(name, info)
    assert info["path"] == case["named_path"] == case["path"], (name, info)
    assert sc_.plan_matches_info(case["plan"], info), (case["plan"], info)
    if info["path"] == sm.PATH_BIG_FINE:
        assert info["fine_log"] == sc_.fine_log_big(case["plan"], shape)
        assert (info["big_listed"], info["big_total"]) == case["big"], (info, case["big"])
    elif info["path"] == sm.PATH_SHARED_FINE:
        assert info["fine_log"] == shape["FINE_LOG"]
    got = sm.check(info, case["sc"], count, begin, srt, perm, heavy, max(case["batch"], 1))
    print(name, got)
    if not case["designed"]:
        return
    # the whole MSM over the same scalars
    n = case["n"]
    want = ec.g1_to_bytes(ec.g1_mul(sc_.closed_form_log(case["sc"])))
    b = ctx.bases_g1_synthetic(n)
    try:
        if case["plan_n"]:
            w, nwin, cb = ctx.msm_g1_windows_dev(d.data_ptr(), n, b, case["plan_n"])
            assert (nwin, cb) == (info["nwin"], info["c"])
            assert zk.msm_g1_combine(w, 1, nwin, cb) == want, (name, "windows + combine")
        else:
            assert ctx.msm_g1_dev(d.data_ptr(), n, b) == want, (name, "plain")
            b.prepare()
            assert ctx.msm_g1_dev(d.data_ptr(), n, b) == want, (name, "prepared bases")
    finally:
        b.free()


@pytest.mark.parametrize("name", sc_.HEAVY_MSM_CASES)
def test_heavy_edge_vectors_in_g2_and_over_bn254(zk, ctx, name):
    """Buckets of exactly heavy_thr and heavy_thr + 1 entries, and MSM_HEAVY_CAP - 1, MSM_HEAVY_CAP, MSM_HEAVY_CAP + 1 heavy
    buckets: the same scalars through the G2 and the BN254 engines.  References: one scalar multiplication of the G2 oracle,
    and bn254_msm_cases' sum of discrete logs."""
    import bn254_msm_cases as bc
    from oracle import bn254 as bn

    case = sc_.get(name, zk)
    n, sc = case["n"], case["sc"]
    assert all(v < bn.R for v in sm.scalars_to_ints(sc[sc[:, 7] != 0])) and (sc[:, 7] >> 26 == 0).all()
    d = _upload(sc)
    b2 = ctx.bases_g2_synthetic(n)
    try:
        assert ctx.msm_g2_dev(d.data_ptr(), n, b2) == ec.g2_to_bytes(ec.g2_mul(sc_.closed_form_log(sc)))
    finally:
        b2.free()
    bb = ctx.bn254_bases_synthetic(n)
    try:
        assert ctx.bn254_msm_g1_dev(d.data_ptr(), n, bb) == bn.g1_to_bytes(bn.pt_mul(bn.G1, sc_.closed_form_log(sc, bn.R)))
    finally:
        bb.free()


def test_read_out_refuses_bad_arguments(zk, ctx):
    import ctypes as C

    d = _upload(sm.dense(64, ec.R, 3))
    fn = zk.tlib.zkmi_selftest_msm_sort_dev
    info = (C.c_uint32 * 16)()
    few = (C.c_uint32 * 4)()

    def call(mode=0, ptr=d.data_ptr(), n=64, plan_n=0, batch=0, n_info=16, count=None, cap_b=0, srt=None, cap_s=0):
        return fn(ctx.h, C.c_int32(mode), C.c_void_p(ptr), C.c_uint64(n), C.c_uint64(plan_n), C.c_uint32(batch), info, C.c_uint32(n_info),
                  count, None, None, None, C.c_uint64(cap_b), srt, C.c_uint64(cap_s))

    assert call() == 0 and info[15] == sm.PATH_WINDOWED
    assert call(n=0) == -1 and call(ptr=None) == -1 and call(n_info=15) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(n=1 << 28) == -1 and call(plan_n=1 << 28) == -1
    assert call(mode=1, plan_n=64) == -1 and call(mode=0, batch=2) == -1 and call(mode=2, batch=0) == -1 and call(mode=2, n=16, batch=65) == -1
    assert call(count=few, cap_b=4) == -1 and call(srt=few, cap_s=4) == -1  # capacities below the need
    assert call(mode=2, n=16, batch=4) == 0 and info[15] == sm.PATH_SHARED_BATCH and info[5] == 1
