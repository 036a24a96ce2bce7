"""CPU suite: a relation's Groth16 key from a phase-1 transcript (zkmi_groth16_setup_from_srs, zkmi_pk_contribute).  The host
plan of the column sums and the per-item bodies the kernels call, run by the host loop of the testing library, before
anything runs on a device; and the new entry points' refusals without a context."""
import ctypes as C

import pytest

import setup_key_model as model

TOXIC3 = model.frs([model.TAU, model.ALPHA, model.BETA])
QUERIES = (0, 1, 2, 4)  # a, b_g1, b_g2, l as zkmi_pk_export_query numbers them


@pytest.fixture(scope="module")
def relations(zk):
    out = {}
    for log_n in (3, 5, 8):
        rel = model.Relation(log_n, 0x5E7 + log_n)
        r1 = zk.r1cs_create(rel.n_vars, rel.n_pub, rel.mats())
        assert (r1.log_n, r1.n_constraints) == (log_n, rel.nc) and r1.is_satisfied(rel.witness())
        out[log_n] = (rel, r1)
    yield out
    for _, r1 in out.values():
        r1.free()


@pytest.mark.parametrize("log_n", (3, 5, 8))
def test_plan_invariants(zk, relations, log_n):
    """Columns of length 0, 1, FAN, FAN + 1, FAN^2, FAN^2 + 1 (those the domain has room for) and one every row mentions:
    every final slot written exactly once (by an item or the infinity fill), every partial written once and read once at
    the next level, counts in [1, FAN], levels within ceil(log_FAN(longest column)), zero coefficients dropped, and
    min(c, r - c) with its flag reproducing c."""
    rel, r1 = relations[log_n]
    fan = model.FAN
    for which in QUERIES:
        want = rel.expected_terms(which)
        lens = {len(t) for t in want.values()}
        assert {0, 1} <= lens
        if log_n == 8:
            assert {fan, fan + 1, fan * fan, fan * fan + 1} <= lens, sorted(lens)
        plan = zk.selftest_colsum_plan(r1, which)
        assert plan["empty"] == [j for j, t in want.items() if not t] and model.V_NONE in plan["empty"]
        levels = model.check_plan(plan, want)
        if log_n == 8 and which in (0, 4):
            assert levels == 3  # the constant's column: 254 terms -> 32 -> 4 -> 1
        # the model drops the zero entries the matrices carry: the plan holds exactly the live ones
        assert len(plan["terms"]) == sum(len(t) for t in want.values())
    # a query that is none: refused
    with pytest.raises(Exception):
        zk.selftest_colsum_plan(r1, 3)


@pytest.mark.parametrize("log_n", (3, 5))
def test_host_run_of_the_plan_matches_the_oracle(zk, relations, log_n):
    """All four column queries from the host loop over the kernels' per-item bodies, Lagrange bases from explicit tau, alpha,
    beta, against oracle.groth16.setup(r1cs, tau, alpha, beta, 1, 1)."""
    rel, r1 = relations[log_n]
    vk, q = model.oracle_setup_bytes(rel)
    np_ = rel.n_pub
    got = {w: zk.selftest_setup_columns_host(r1, TOXIC3, w, rel.n_vars) for w in QUERIES}
    assert got[0] == q[0]
    assert got[1] == q[1]
    assert got[2] == q[2]
    assert got[4][96 * np_ :] == q[4]
    assert got[4][: 96 * np_] == vk[672:]  # gamma_abc_g1
    assert got[0][96 * model.V_NONE : 96 * model.V_NONE + 96] == bytes(96)  # the variable no row mentions: infinity


def test_new_entry_points_refuse_null_arguments(zk):
    """NULL context / handles: ZKMI_ERR_BAD_ARG, not a crash (no device is touched), *out_pk NULL."""
    lib = zk.lib
    buf = (C.c_uint8 * 1024)()
    h = C.c_void_p(1)
    fake = C.c_void_p(8)  # never dereferenced: every call below is refused before it looks at it
    assert lib.zkmi_groth16_setup_from_srs(None, fake, fake, C.byref(h), buf, C.c_uint64(1024)) == -1
    assert h.value is None
    assert lib.zkmi_groth16_setup_from_srs(None, None, None, None, None, C.c_uint64(0)) == -1
    assert lib.zkmi_pk_contribute(None, fake, buf, buf, buf) == -1
    assert lib.zkmi_pk_contribute(None, None, None, None, None) == -1
