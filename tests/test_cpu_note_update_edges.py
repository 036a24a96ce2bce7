"""The update_note witness generator at its value and batch edges, on the host: the constraint builder (relation.hip's
synthesize, canonical Fr) and the device code executed on the host (relation_values.hpp's rv_update_note, lazily reduced
Fr28) against the model of note_update_cases.py, against each other byte for byte, against the exported constraint system,
and -- for the accepted edges -- against an assignment the product did not compute (oracle/relation_witness.py)."""
import json
import os
import subprocess
import sys

import pytest

import note_update_cases as nc
from note_update_cases import CASES, SOLVER_CASES, case_id, model_status, mock_status, to_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def r1cs_of(zk):
    """update_note_r1cs per (op_kind, height, log_n), built once"""
    made = {}

    def get(op_kind, height, log_n):
        key = (op_kind, height, log_n)
        if key not in made:
            made[key] = zk.update_note_r1cs(log_n, op_kind, tree_height=height)
        return made[key]

    yield get
    for r1 in made.values():
        r1.free()


@pytest.fixture(scope="module")
def built(zk, pkg):
    """(bytes, status) of the constraint builder per case, computed once"""
    made = {}

    def get(c):
        if case_id(c) not in made:
            w, _, rc = zk.update_note_witness(c["log_n"], c["op_kind"], to_input(pkg, c), check=False)
            made[case_id(c)] = (w, rc)
        return made[case_id(c)]

    return get


def test_case_table_covers_every_status_in_both_kinds_and_mock_agrees():
    """The table is not vacuous, and where the mock's u128 Account::update is defined it decides as the model does:
    b + a < 2^129 < r, and b - a < 0 lands above 2^128, so checked arithmetic and the range check coincide."""
    for op_kind in (nc.DEPOSIT, nc.WITHDRAW):
        seen = {model_status(c) for c in nc.group(op_kind, 10, 13)}
        assert seen == {nc.OK, nc.NON_CANONICAL, nc.ACCOUNT_UPDATE, nc.COMBINE}
    defined = 0
    for c in CASES:
        m = mock_status(c)
        if m is not None:
            defined += 1
            assert m == model_status(c), case_id(c)
    assert defined > len(CASES) // 3
    by = {case_id(c): model_status(c) for c in CASES}
    # the model's verdict on the named edges of the case table, spelled out
    for name, want in (("withdraw-h10-withdraw_whole_balance", nc.OK), ("withdraw-h10-withdraw_balance_plus_1", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-withdraw_0_from_0", nc.OK), ("withdraw-h10-withdraw_1_from_0", nc.ACCOUNT_UPDATE),
                       ("deposit-h10-deposit_to_u128_max", nc.OK), ("deposit-h10-deposit_past_u128_max", nc.ACCOUNT_UPDATE),
                       ("deposit-h10-balance_u128_max_amount_u128_max", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-balance_u128_max_amount_u128_max", nc.OK),
                       ("deposit-h10-amount_2p128", nc.ACCOUNT_UPDATE), ("withdraw-h10-amount_2p128", nc.ACCOUNT_UPDATE),
                       ("deposit-h10-deposit_r_minus_1_on_5", nc.OK), ("withdraw-h10-withdraw_r_minus_5_from_0", nc.OK),
                       ("withdraw-h10-old_balance_2p128_plus_3_withdraw_4", nc.OK),
                       ("deposit-h10-untouched_balance_u128_max", nc.OK), ("withdraw-h10-untouched_balance_2p128", nc.ACCOUNT_UPDATE),
                       ("deposit-h10-balances_r_minus_1_deposit_r_minus_1", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-tokens_all_equal", nc.ACCOUNT_UPDATE), ("deposit-h10-slots_equal_token_differs", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-token_t0_zero", nc.OK), ("deposit-h10-token_t1_r_minus_1", nc.OK),
                       ("withdraw-h10-t0_token_plus_2p224", nc.ACCOUNT_UPDATE), ("withdraw-h10-users_differ", nc.COMBINE),
                       ("deposit-h10-users_differ_token_missing", nc.ACCOUNT_UPDATE), ("withdraw-h10-users_r_minus_1", nc.OK),
                       ("withdraw-h10-users_differ_touched_out_of_range", nc.ACCOUNT_UPDATE),
                       ("deposit-h10-users_differ_touched_out_of_range", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-users_differ_untouched_out_of_range", nc.ACCOUNT_UPDATE),
                       ("deposit-h10-users_differ_untouched_out_of_range", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-users_differ_tokens_all_equal", nc.ACCOUNT_UPDATE),
                       ("withdraw-h10-shape_2_at_last", nc.NON_CANONICAL), ("withdraw-h10-shape_2_behind_height", nc.OK),
                       ("deposit-h10-path_r_behind_height", nc.OK), ("withdraw-h10-all_zero", nc.OK),
                       ("withdraw-h32-max_lazy_seed", nc.ACCOUNT_UPDATE), ("deposit-h32-max_lazy_seed", nc.ACCOUNT_UPDATE)):
        assert by[name] == want, name


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_builder_and_value_code_agree_with_the_model(zk, pkg, r1cs_of, built, c):
    """Both generators return the model's status; unless the instance is non-canonical their assignments are
    byte-identical, and the assignment satisfies the relation's constraint system EXACTLY when the status is OK."""
    want = model_status(c)
    inp = to_input(pkg, c)
    if want == nc.NON_CANONICAL:
        for call in (lambda: zk.update_note_witness(c["log_n"], c["op_kind"], inp, check=False),
                     lambda: zk.update_note_witness_values_host(c["log_n"], c["op_kind"], inp)):
            with pytest.raises(pkg.ZkmiError) as e:
                call()
            assert e.value.code == nc.NON_CANONICAL
        return
    w, rc = built(c)
    wv, rcv = zk.update_note_witness_values_host(c["log_n"], c["op_kind"], inp)
    assert rc == want, "constraint builder: status %d, the model says %d" % (rc, want)
    assert rcv == want, "value code: status %d, the model says %d" % (rcv, want)
    assert wv == w, "value code and constraint builder differ in variable %d" % next(
        i for i in range(1 << c["log_n"]) if wv[32 * i : 32 * i + 32] != w[32 * i : 32 * i + 32])
    satisfied = r1cs_of(c["op_kind"], c["height"], c["log_n"]).is_satisfied(w)
    assert satisfied == (want == nc.OK), ("status OK on an UNSATISFIED assignment" if want == nc.OK
                                          else "status %d on a SATISFIED assignment" % want)
    if c["name"].endswith("_behind_height"):
        assert w == built(nc.base(c["op_kind"], c["height"], c["log_n"]))[0], "an entry behind the height reached the assignment"


@pytest.fixture(scope="module")
def oracle_rows(r1cs_of):
    made = {}

    def get(op_kind, height):
        if (op_kind, height) not in made:
            made[(op_kind, height)] = nc.oracle_r1cs(r1cs_of(op_kind, height, 13))
        return made[(op_kind, height)]

    return get


@pytest.mark.parametrize("c", SOLVER_CASES, ids=case_id)
def test_accepted_edges_equal_an_assignment_the_product_did_not_compute(built, oracle_rows, c):
    """Loaded values with oracle/poseidon.py hashes + the generic solver over the exported rows reproduce the builder's
    bytes at the accepted edges."""
    from oracle import relation_witness as rw

    assert model_status(c) == nc.OK and c["log_n"] == 13 and c["account"][0] != c["account"][2]
    H = c["height"]
    loaded = rw.update_note_loaded(c["op_kind"], c["amount"], c["token"], c["user"], c["new_note"], c["old_note"], c["shape"][:H],
                                   c["path"][:H], c["op_priv_user"], c["account"])
    orc = oracle_rows(c["op_kind"], H)
    z = rw.solve(orc.n_vars, orc.A, orc.B, orc.C, loaded)
    assert orc.is_satisfied(z)
    w, rc = built(c)
    assert rc == nc.OK and w == b"".join(v.to_bytes(32, "little") for v in z)


def test_solver_cases_cover_the_named_edges():
    names = {c["name"] for c in SOLVER_CASES}
    assert {"amount_0", "withdraw_whole_balance", "deposit_to_u128_max", "balance_u128_max_amount_0", "deposit_r_minus_1_on_5",
            "withdraw_r_minus_5_from_0", "token_t0_zero", "all_zero", "siblings_all_r_minus_1"} <= names
    assert {c["height"] for c in SOLVER_CASES} >= {1, 2, 10}


_FIT_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from zkmi_loader import load_pkg
import note_update_cases as nc
pkg = load_pkg(); zk = pkg.Zkmi()
order, warm, op_kind = sys.argv[1].split(","), sys.argv[2] == "warm", int(sys.argv[3])
def code(f):
    try:
        r = f()
    except pkg.ZkmiError as e:
        return e.code
    if hasattr(r, "free"):
        r.free()
    return 0
out = {}
for h in range(1, 33):
    inp = nc.to_input(pkg, nc.base(op_kind, h))
    calls = {"r1cs": lambda: zk.update_note_r1cs(13, op_kind, tree_height=h),
             "builder": lambda: zk.update_note_witness(13, op_kind, inp),
             "values": lambda: zk.update_note_witness_values_host(13, op_kind, inp)}
    if warm:  # a larger domain first: the value code's padding shape is then remembered for this (kind, height)
        assert code(lambda: zk.update_note_witness_values_host(14, op_kind, inp)) == 0
    out[h] = {name: code(calls[name]) for name in order}
print(json.dumps(out))
"""


_FIT_RUNS = [(order, warm, op_kind) for order, warm in ((("r1cs", "builder", "values"), False), (("values", "builder", "r1cs"), True))
             for op_kind in (nc.DEPOSIT, nc.WITHDRAW)]


def test_whether_a_height_fits_2p13_has_one_answer():
    """Heights 1..32, both kinds: update_note_r1cs, update_note_witness and update_note_witness_values_host all accept or
    all refuse with the bad-argument code, whichever is asked first and whether or not the value code has already seen the
    (kind, height) at a larger domain -- chain_shape remembers the relation's size per process (and then tests
    N < v + 16 where pad_chain tests v + 8 > N and c + n_pub + 8 > N), hence fresh children: one per call order and kind,
    side by side."""
    script = _FIT_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    children = [subprocess.Popen([sys.executable, "-c", script, ",".join(order), "warm" if warm else "cold", str(op_kind)],
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for order, warm, op_kind in _FIT_RUNS]
    results = [ch.communicate(timeout=600) + (ch.returncode,) for ch in children]
    for (order, warm, op_kind), (out, err, rc) in zip(_FIT_RUNS, results):
        assert rc == 0, err[-2000:]
        got = json.loads(out.strip().splitlines()[-1])
        for h in range(1, 33):
            codes = got[str(h)]
            assert set(codes.values()) in ({nc.OK}, {nc.BAD_ARG}), "kind %d height %d, asked in the order %s%s: %r" % (
                op_kind, h, order, " after a larger domain" if warm else "", codes)
        assert [h for h in range(1, 33) if got[str(h)]["values"] == nc.OK] == list(range(1, nc.HEIGHT_MAX_13 + 1))
