"""The named instances of the update_note edge tests (test_cpu_note_update_edges.py pins the constraint builder and the host
execution of the device code to them, test_gpu_note_update_edges.py the kernel) and a model of the status they must get,
written from the statement of the relation (csrc/relation.hip's header) in Python integers, without the library.

A case is a dict: name, op_kind (0 = deposit, 1 = withdraw), height, log_n and the fields of zkmi_note_update as integers:
amount, token, user, op_priv_user, new_note / old_note (zk_id, trapdoor, nullifier), account (token_0, balance_0, token_1,
balance_1), shape and path (ZKMI_MAX_TREE_HEIGHT entries each: the relation uses the first `height`, and what lies behind
them must not matter).  Every case is a named variation of one seeded base instance per (op_kind, height): distinct random
tokens T0, T1, balances (900, 40), amount 25 on slot 0, equal users, random notes and a random path."""
import ctypes as C

from oracle.bls12_381 import R, SplitMix64

DEPOSIT, WITHDRAW = 0, 1
OK, BAD_ARG, NON_CANONICAL, ACCOUNT_UPDATE, COMBINE = 0, -1, -2, -6, -7
MAX_HEIGHT = 32
U128 = 1 << 128
# The largest tree height whose relation (each path level adds an is_zero, two selects and a Poseidon 2 -> 1) still fits
# 2^13 rows with its 8 rows of padding; test_cpu_note_update_edges.py finds the same number from the three entry points.
HEIGHT_MAX_13 = 19
HEIGHTS_13 = (1, 2, HEIGHT_MAX_13, 10)


def _base_fields(seed=0x0DD5):
    rng = SplitMix64(seed)
    t0 = rng.fr()
    while not 1 < t0 < R - (1 << 224):  # T0 - 1, T0 + 1 and T0 + 2^224 are field elements too
        t0 = rng.fr()
    t1 = rng.fr()
    user = rng.fr()
    return {"amount": 25, "token": t0, "user": user, "op_priv_user": user,
            "new_note": tuple(rng.fr() for _ in range(3)), "old_note": tuple(rng.fr() for _ in range(3)),
            "account": (t0, 900, t1, 40),
            "shape": [rng.next() & 1 for _ in range(MAX_HEIGHT)], "path": [rng.fr() for _ in range(MAX_HEIGHT)],
            "other": rng.fr()}  # a field element that is neither token nor user


_BASE = _base_fields()
T0, T1, OTHER = _BASE["account"][0], _BASE["account"][2], _BASE.pop("other")
assert len({T0, T1, OTHER, _BASE["user"], T0 - 1, T0 + 1, T0 + (1 << 224)}) == 7


def base(op_kind, height, log_n=13, name="base"):
    """The base instance: entries behind `height` are zero, as Zkmi.note_update leaves them."""
    c = dict(_BASE, name=name, op_kind=op_kind, height=height, log_n=log_n)
    c["shape"] = _BASE["shape"][:height] + [0] * (MAX_HEIGHT - height)
    c["path"] = _BASE["path"][:height] + [0] * (MAX_HEIGHT - height)
    return c


def _with(case, name, **over):
    c = dict(case, name=name)
    for k, v in over.items():
        if k in ("b0", "b1", "t0", "t1"):
            acc = list(c["account"])
            acc[{"t0": 0, "b0": 1, "t1": 2, "b1": 3}[k]] = v
            c["account"] = tuple(acc)
        else:
            c[k] = v
    return c


def _set(seq, i, v):
    s = list(seq)
    s[i] = v
    return type(seq)(s)


def _value_cases(b):
    """Amounts, balances, tokens, users: independent of the height."""
    D, W = b["op_kind"] == DEPOSIT, b["op_kind"] == WITHDRAW
    out = [b, _with(b, "amount_0", amount=0)]
    if W:
        out += [_with(b, "withdraw_whole_balance", amount=900), _with(b, "withdraw_balance_plus_1", amount=901),
                _with(b, "withdraw_0_from_0", amount=0, b0=0), _with(b, "withdraw_1_from_0", amount=1, b0=0),
                # the relation does not range-check the amount (the u128 type of OpPub does, a layer above): 0 - (r - 5) = 5
                _with(b, "withdraw_r_minus_5_from_0", amount=R - 5, b0=0),
                # old balances are not range-checked either: 2^128 + 3 - 4 fits
                _with(b, "old_balance_2p128_plus_3_withdraw_4", amount=4, b0=U128 + 3)]
    if D:
        out += [_with(b, "deposit_to_u128_max", b0=U128 - 1 - 25), _with(b, "deposit_past_u128_max", b0=U128 - 25),
                _with(b, "deposit_r_minus_1_on_5", amount=R - 1, b0=5),
                _with(b, "balances_r_minus_1_deposit_r_minus_1", amount=R - 1, b0=R - 1, b1=R - 1)]
    out += [_with(b, "balance_u128_max_amount_0", amount=0, b0=U128 - 1),
            _with(b, "balance_u128_max_amount_u128_max", amount=U128 - 1, b0=U128 - 1),
            _with(b, "amount_2p128", amount=U128),
            _with(b, "untouched_balance_u128_max", b1=U128 - 1), _with(b, "untouched_balance_2p128", b1=U128),
            # too large in the top limb only, as 2^128 is in the lowest limb above the range only
            _with(b, "untouched_balance_2p224", b1=1 << 224)]
    # tokens ("hit in slot 0" is the base)
    out += [_with(b, "hit_slot_1", token=T1), _with(b, "hit_neither", token=OTHER),
            _with(b, "tokens_all_equal", t1=T0), _with(b, "slots_equal_token_differs", t1=T0, token=T1),
            _with(b, "token_t0_zero", token=0, t0=0), _with(b, "token_t1_r_minus_1", token=R - 1, t1=R - 1),
            _with(b, "t0_token_plus_1", t0=T0 + 1), _with(b, "t0_token_minus_1", t0=T0 - 1),
            _with(b, "t0_token_plus_2p224", t0=T0 + (1 << 224))]
    # users
    out += [_with(b, "users_differ", op_priv_user=OTHER),
            _with(b, "users_differ_token_missing", op_priv_user=OTHER, token=OTHER),
            _with(b, "users_zero", user=0, op_priv_user=0), _with(b, "users_r_minus_1", user=R - 1, op_priv_user=R - 1)]
    # differing users together with each further failure of Account::update: the account's error comes first
    touched = {"amount": 901} if W else {"b0": U128 - 25}
    out += [_with(b, "users_differ_touched_out_of_range", op_priv_user=OTHER, **touched),
            _with(b, "users_differ_untouched_out_of_range", op_priv_user=OTHER, b1=U128),
            _with(b, "users_differ_tokens_all_equal", op_priv_user=OTHER, t1=T0)]
    return out


def _path_cases(b):
    H = b["height"]
    behind = [0] * (MAX_HEIGHT - H)
    out = [_with(b, "shape_all_0", shape=[0] * MAX_HEIGHT), _with(b, "shape_all_1", shape=[1] * H + behind),
           _with(b, "shape_alternating", shape=[i & 1 for i in range(H)] + behind),
           _with(b, "siblings_all_0", path=[0] * MAX_HEIGHT), _with(b, "siblings_all_r_minus_1", path=[R - 1] * H + behind),
           _with(b, "shape_2_at_0", shape=_set(b["shape"], 0, 2)), _with(b, "shape_2_at_last", shape=_set(b["shape"], H - 1, 2))]
    if H < MAX_HEIGHT:  # behind the height: ignored, the assignment is the base's
        out += [_with(b, "shape_2_behind_height", shape=_set(b["shape"], H, 2)),
                _with(b, "path_r_behind_height", path=_set(b["path"], H, R))]
    return out


def _non_canonical_cases(b, value_fields=True):
    H = b["height"]
    out = []
    for tag, v in (("r", R), ("all_ones", (1 << 256) - 1)):
        if value_fields:
            for f in ("amount", "token", "user", "op_priv_user"):
                out.append(_with(b, "%s_%s" % (f, tag), **{f: v}))
            for k in range(3):
                out.append(_with(b, "new_note%d_%s" % (k, tag), new_note=_set(b["new_note"], k, v)))
                out.append(_with(b, "old_note%d_%s" % (k, tag), old_note=_set(b["old_note"], k, v)))
            for k in range(4):
                out.append(_with(b, "account%d_%s" % (k, tag), account=_set(b["account"], k, v)))
        out.append(_with(b, "path_first_%s" % tag, path=_set(b["path"], 0, v)))
        out.append(_with(b, "path_last_%s" % tag, path=_set(b["path"], H - 1, v)))
    return out


def _height_group(op_kind, height):
    """What depends on the height: the path, its shape bytes and where the used part of both ends, with one accepted
    and one refused value edge."""
    b = base(op_kind, height)
    edge = ([_with(b, "withdraw_whole_balance", amount=900), _with(b, "withdraw_balance_plus_1", amount=901)] if op_kind == WITHDRAW
            else [_with(b, "deposit_to_u128_max", b0=U128 - 1 - 25), _with(b, "deposit_past_u128_max", b0=U128 - 25)])
    return [b] + edge + _path_cases(b) + _non_canonical_cases(b, value_fields=False)


def _extremes(op_kind):
    zero = dict(base(op_kind, 10), name="all_zero", amount=0, token=0, user=0, op_priv_user=0, new_note=(0, 0, 0),
                old_note=(0, 0, 0), account=(0, 0, 1, 0), shape=[0] * MAX_HEIGHT, path=[0] * MAX_HEIGHT)
    # the largest lazy chain seed: every loaded field r - 1 (T1 = r - 2 keeps the tokens distinct), all shape bytes 1, height 32
    big = dict(base(op_kind, 32, 14), name="max_lazy_seed", amount=R - 1 if op_kind == DEPOSIT else 0, token=R - 1, user=R - 1,
               op_priv_user=R - 1, new_note=(R - 1,) * 3, old_note=(R - 1,) * 3, account=(R - 1, R - 1, R - 2, R - 1),
               shape=[1] * MAX_HEIGHT, path=[R - 1] * MAX_HEIGHT)
    return zero, big


def _table():
    out = []
    for op_kind in (DEPOSIT, WITHDRAW):
        b = base(op_kind, 10)
        zero, big = _extremes(op_kind)
        out += _value_cases(b) + _path_cases(b) + _non_canonical_cases(b) + [zero]
        for h in HEIGHTS_13:
            if h != 10:
                out += _height_group(op_kind, h)
    # height 32 at 2^14: the extreme seed as withdraw 0 and as deposit, and one base instance
    out += [_extremes(WITHDRAW)[1], _extremes(DEPOSIT)[1], base(WITHDRAW, 32, 14)]
    return out


CASES = _table()


def case_id(c):
    return "%s-h%d-%s" % ("deposit" if c["op_kind"] == DEPOSIT else "withdraw", c["height"], c["name"])


assert len({case_id(c) for c in CASES}) == len(CASES)


def group(op_kind, height, log_n):
    return [c for c in CASES if (c["op_kind"], c["height"], c["log_n"]) == (op_kind, height, log_n)]


GROUPS = sorted({(c["op_kind"], c["height"], c["log_n"]) for c in CASES})

# accepted edges that the oracle-side solver (oracle/relation_witness.py) reproduces, all at 2^13
SOLVER_IDS = (
    "withdraw-h10-amount_0", "withdraw-h10-withdraw_whole_balance", "withdraw-h10-withdraw_0_from_0",
    "withdraw-h10-balance_u128_max_amount_0", "withdraw-h10-untouched_balance_u128_max", "withdraw-h10-withdraw_r_minus_5_from_0",
    "withdraw-h10-token_t0_zero", "withdraw-h10-all_zero", "withdraw-h10-siblings_all_r_minus_1", "withdraw-h1-base", "withdraw-h2-base",
    "deposit-h10-deposit_to_u128_max", "deposit-h10-deposit_r_minus_1_on_5", "deposit-h10-all_zero",
)
SOLVER_CASES = [c for c in CASES if case_id(c) in SOLVER_IDS]
assert len(SOLVER_CASES) == len(SOLVER_IDS) == 14 and all(c["log_n"] == 13 for c in SOLVER_CASES)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def used_fields(c):
    return ([c["amount"], c["token"], c["user"], c["op_priv_user"]] + list(c["new_note"]) + list(c["old_note"])
            + list(c["account"]) + list(c["path"][: c["height"]]))


def model_status(c):
    """The status of one instance, from the statement of the relation:
      NON_CANONICAL   a used field >= r or a used shape byte > 1 (there is no assignment to speak of);
      ACCOUNT_UPDATE  no slot holds the token (m_0 + m_1 = 1 fails at 0), both slots hold equal tokens (the account is
                      malformed: with the token in both, m_0 + m_1 = 2), or a new balance (b +- [slot hit] amount) mod r
                      does not fit the 128-bit range check -- BOTH new balances are range-checked, the old ones are not;
      COMBINE         op_priv's user differs from op_pub's, and nothing above applies;
      OK              otherwise.
    The precedence (every failure of Account::update before combine) is the witness generator's, as synthesize() in
    relation.hip documents it where it compares the users; the mock-facing zkmi_shielder_prove_update runs zkmi_operation_combine FIRST, as the mock's
    ZkProof::update_account does, so there differing users win over a missing token."""
    H = c["height"]
    if any(v >= R for v in used_fields(c)) or any(s > 1 for s in c["shape"][:H]):
        return NON_CANONICAL
    t0, b0, t1, b1 = c["account"]
    sign = 1 if c["op_kind"] == DEPOSIT else -1
    hit = [int(t0 == c["token"]), int(t1 == c["token"])]
    new = [(b0 + sign * hit[0] * c["amount"]) % R, (b1 + sign * hit[1] * c["amount"]) % R]
    if hit == [0, 0] or t0 == t1 or new[0] >= U128 or new[1] >= U128:
        return ACCOUNT_UPDATE
    if c["user"] != c["op_priv_user"]:
        return COMBINE
    return OK


def mock_status(c):
    """Account::update of the mock (u128 checked_add / checked_sub on the first slot that holds the token), then the users,
    in the generator's precedence.  None where the mock's types do not reach: a non-canonical instance, an amount or a
    balance that is no u128, equal tokens in both slots."""
    t0, b0, t1, b1 = c["account"]
    if model_status(c) == NON_CANONICAL or max(c["amount"], b0, b1) >= U128 or t0 == t1:
        return None
    for token, balance in ((t0, b0), (t1, b1)):
        if token == c["token"]:
            upd = balance + c["amount"] if c["op_kind"] == DEPOSIT else balance - c["amount"]
            if not 0 <= upd < U128:
                return ACCOUNT_UPDATE
            break
    else:
        return ACCOUNT_UPDATE
    return COMBINE if c["user"] != c["op_priv_user"] else OK


# ---- to the library ---------------------------------------------------------------------------------------------------------------
def to_input(pkg, c):
    """zkmi_note_update of a case: all ZKMI_MAX_TREE_HEIGHT path entries are written, also those behind the height."""
    i = pkg.binding.NoteUpdate()
    put = lambda dst, v: C.memmove(dst, int(v).to_bytes(32, "little"), 32)
    put(i.amount, c["amount"]), put(i.token, c["token"]), put(i.user, c["user"]), put(i.op_priv_user, c["op_priv_user"])
    for k in range(3):
        put(i.new_note[k], c["new_note"][k]), put(i.old_note[k], c["old_note"][k])
    i.tree_height = c["height"]
    for k in range(MAX_HEIGHT):
        i.path_shape[k] = c["shape"][k]
        put(i.path[k], c["path"][k])
    for k in range(4):
        put(i.account[k], c["account"][k])
    return i


def oracle_r1cs(r1):
    """The exported matrices of an R1cs handle as oracle/groth16.py's R1CS (rows of (column, coefficient) in Python integers)."""
    from oracle import groth16 as g16

    rows = []
    for m in range(3):
        rp, cl, vl = r1.export(m)
        vals = [int.from_bytes(vl[32 * k : 32 * k + 32], "little") for k in range(len(cl))]
        rows.append([[(cl[k], vals[k]) for k in range(rp[i], rp[i + 1])] for i in range(r1.n_constraints)])
    return g16.R1CS(r1.n_vars, r1.n_pub, *rows)
