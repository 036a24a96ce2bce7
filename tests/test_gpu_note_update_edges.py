"""The update_note witness kernel (k_update_note_values, one lane per instance) at the value and batch edges of
note_update_cases.py.  Expected bytes and statuses come from the constraint builder on the host, once per module; every
comparison is byte for byte, and every device buffer holds 0xA5 before the call."""
import pytest
import torch

import note_update_cases as nc
from note_update_cases import case_id, model_status, to_input

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope="module")
def expected(zk, pkg):
    """(assignment bytes, status) of the host builder per case; (None, NON_CANONICAL) where it refuses the instance."""
    made = {}

    def get(c):
        if case_id(c) not in made:
            try:
                w, _, rc = zk.update_note_witness(c["log_n"], c["op_kind"], to_input(pkg, c), check=False)
                made[case_id(c)] = (w, rc)
            except pkg.ZkmiError as e:
                assert e.code == nc.NON_CANONICAL
                made[case_id(c)] = (None, e.code)
        return made[case_id(c)]

    return get


def _call(ctx, pkg, inputs, log_n, op_kind, buf_log_n=None):
    """One call of update_note_witness_batch_dev over canary-filled buffers of 2^buf_log_n elements each: (statuses, or the
    ZkmiError the call raised; the buffers as an (n, bytes) uint8 array; the device tensor)."""
    bufs = torch.full((len(inputs), 32 << (buf_log_n or log_n)), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        status = ctx.update_note_witness_batch_dev(log_n, op_kind, inputs, [bufs[i].data_ptr() for i in range(len(inputs))])
    except pkg.ZkmiError as e:
        status = e
    torch.cuda.synchronize()
    return status, bufs.cpu().numpy(), bufs


def _run(ctx, pkg, cases):
    status, host, bufs = _call(ctx, pkg, [to_input(pkg, c) for c in cases], cases[0]["log_n"], cases[0]["op_kind"])
    if isinstance(status, Exception):
        raise status
    return status, host, bufs


def _check(cases, status, host, expected):
    for i, c in enumerate(cases):
        w, rc = expected(c)
        assert status[i] == rc == model_status(c), "%s (lane %d): kernel %d, builder %d, model %d" % (
            case_id(c), i, status[i], rc, model_status(c))
        if w is None:
            assert (host[i] == CANARY).all(), "%s (lane %d): a non-canonical instance's buffer was written" % (case_id(c), i)
        else:
            got = host[i].tobytes()
            assert got == w, "%s (lane %d): differs from the builder in variable %d" % (
                case_id(c), i, next(k for k in range(len(w) // 32) if got[32 * k : 32 * k + 32] != w[32 * k : 32 * k + 32]))


def _interleaved(op_kind):
    """The whole (kind, 10, 2^13) group, accepted / refused / non-canonical in turn, so that the lanes of the first wave
    return different statuses and leave rv_update_note at different points.  The group is longer than a workgroup of 64
    lanes, so its tail runs in a second one."""
    g = nc.group(op_kind, 10, 13)
    kinds = [[c for c in g if model_status(c) == nc.OK], [c for c in g if model_status(c) in (nc.ACCOUNT_UPDATE, nc.COMBINE)],
             [c for c in g if model_status(c) == nc.NON_CANONICAL]]
    out = []
    for k in range(max(len(v) for v in kinds)):
        out += [v[k] for v in kinds if k < len(v)]
    assert len(out) == len(g) >= 65
    return out


@pytest.fixture(scope="module")
def whole(ctx, pkg):
    """(cases, statuses, buffers) of the whole group of a kind in one call, made once"""
    made = {}

    def get(op_kind):
        if op_kind not in made:
            cases = _interleaved(op_kind)
            status, host, _ = _run(ctx, pkg, cases)
            made[op_kind] = (cases, status, host)
        return made[op_kind]

    return get


@pytest.mark.parametrize("op_kind", [nc.DEPOSIT, nc.WITHDRAW], ids=["deposit", "withdraw"])
def test_whole_table_in_one_batch(whole, expected, op_kind):
    cases, status, host = whole(op_kind)
    want = [model_status(c) for c in cases]
    assert {nc.OK, nc.ACCOUNT_UPDATE, nc.COMBINE, nc.NON_CANONICAL} == set(want[:64])
    assert sum(a != b for a, b in zip(want[:64], want[1:64])) >= 40  # neighbouring lanes of the first wave disagree
    _check(cases, status, host, expected)
    # a lane that returns at the canonicity check writes nothing, between two lanes that write everything
    between = [i for i in range(1, len(cases) - 1) if want[i] == nc.NON_CANONICAL and nc.NON_CANONICAL not in (want[i - 1], want[i + 1])]
    assert len(between) >= 10
    for i in between:
        assert (host[i] == CANARY).all() and not (host[i - 1] == CANARY).all() and not (host[i + 1] == CANARY).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_an_instance_does_not_depend_on_its_batch(ctx, pkg, whole, expected, n):
    """The first n instances of the whole-table batch, called alone: each buffer and status equals what the same instance
    got in the whole batch (canary bytes included), and, as there, the builder's."""
    for op_kind in (nc.DEPOSIT, nc.WITHDRAW):
        cases, whole_status, whole_host = whole(op_kind)
        status, host, _ = _run(ctx, pkg, cases[:n])
        assert status == whole_status[:n]
        differ = [case_id(c) for i, c in enumerate(cases[:n]) if not (host[i] == whole_host[i]).all()]
        assert not differ, "bytes depend on the batch size: %s" % differ
        _check(cases[:n], status, host, expected)


@pytest.mark.parametrize("height,log_n", [(1, 13), (2, 13), (nc.HEIGHT_MAX_13, 13), (32, 14)])
def test_other_tree_heights(ctx, pkg, expected, height, log_n):
    ran = 0
    for op_kind in (nc.DEPOSIT, nc.WITHDRAW):
        cases = nc.group(op_kind, height, log_n)
        if cases:
            status, host, _ = _run(ctx, pkg, cases)
            _check(cases, status, host, expected)
            ran += len(cases)
    assert ran >= 3
    if height == 32:
        assert ran == 3 and sorted(c["name"] for op_kind in (0, 1) for c in nc.group(op_kind, 32, 14)) == [
            "base", "max_lazy_seed", "max_lazy_seed"]


def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, pkg, expected):
    good = nc.base(nc.WITHDRAW, 10)
    too_high = to_input(pkg, good)
    too_high.tree_height = nc.MAX_HEIGHT + 1
    no_fit = nc.base(nc.WITHDRAW, nc.HEIGHT_MAX_13 + 1)
    for what, inputs, log_n in (
        ("mixed heights in one batch", [to_input(pkg, good), to_input(pkg, nc.base(nc.WITHDRAW, 2)), to_input(pkg, good)], 13),
        ("height 33 behind a good instance", [to_input(pkg, good), too_high], 13),
        ("height 33", [too_high], 13),
        ("log_n 12", [to_input(pkg, good)], 12),
        ("a height that does not fit 2^13", [to_input(pkg, no_fit), to_input(pkg, no_fit)], 13),
    ):
        status, host, _ = _call(ctx, pkg, inputs, log_n, nc.WITHDRAW, buf_log_n=13)
        assert isinstance(status, pkg.ZkmiError) and status.code == nc.BAD_ARG, "%s: %r" % (what, status)
        assert (host == CANARY).all(), "%s: a refused call wrote to a buffer" % what
        status, host, _ = _run(ctx, pkg, [good])  # the context still works
        _check([good], status, host, expected)


def test_edge_witnesses_go_from_hbm_through_the_batch_prover(ctx, zk, pkg, expected):
    """The whole-balance withdrawal and the deposit to 2^128 - 1, each beside its base instance, proved from the buffers
    the kernel wrote under a 2^13 key of their kind; the proofs verify against publics computed by oracle/poseidon.py."""
    from oracle import bls12_381 as ec
    from oracle import relation_witness as rw

    frs = lambda vals: b"".join(v.to_bytes(32, "little") for v in vals)
    for op_kind, name in ((nc.WITHDRAW, "withdraw_whole_balance"), (nc.DEPOSIT, "deposit_to_u128_max")):
        cases = [c for c in nc.group(op_kind, 10, 13) if c["name"] in (name, "base")]
        assert [c["name"] for c in cases] == ["base", name]
        status, host, bufs = _run(ctx, pkg, cases)
        _check(cases, status, host, expected)
        assert status == [0, 0]
        r1 = zk.update_note_r1cs(13, op_kind)
        rng = ec.SplitMix64(0xED6E + op_kind)
        pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
        rs = [ec.fr_to_bytes(rng.fr()) for _ in cases]
        ss = [ec.fr_to_bytes(rng.fr()) for _ in cases]
        proofs = ctx.groth16_prove_batch_dev(pk, [bufs[i].data_ptr() for i in range(len(cases))], rs, ss)
        for c, pf in zip(cases, proofs):
            publics = rw.update_note_loaded(op_kind, c["amount"], c["token"], c["user"], c["new_note"], c["old_note"],
                                            c["shape"][:10], c["path"][:10], c["op_priv_user"], c["account"])[1:7]
            assert zk.groth16_verify(vk, frs(publics), pf) is True, case_id(c)
            wrong = list(publics)
            wrong[3] = (wrong[3] + 1) % ec.R
            assert zk.groth16_verify(vk, frs(wrong), pf) is False, case_id(c)
        pk.free()
        r1.free()
