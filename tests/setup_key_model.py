"""Shared inputs of tests/test_{cpu,gpu}_setup_key.py: random satisfiable relations whose columns have prescribed lengths
(the edges of the column-sum plan of zkmi_groth16_setup_from_srs), their expected column terms, and the checker of a plan's
invariants.  Big integers only; the oracle supplies the keys."""
import random

from oracle import bls12_381 as ec
from oracle import groth16 as g16

R = ec.R
FAN = 8  # csrc/tune.hpp COLSUM_FAN; test_cpu_setup_key.py holds the library to it
TAU, ALPHA, BETA = 0x1D0C5A7E5EED0001 % R, 0x2A11FA0000000007 * 0x10001 % R, (R - 0xBE7A) % R  # as test_cpu_setup_srs.py
FINAL = 1 << 31
N_PUB = 3
# variables: 0 the constant (A and C mention it on every row), 1 2 public, then
V_NONE, V_ONE_ROW, V_SAME_ROW, V_ZEROS, V_LEN0 = 3, 4, 5, 6, 7  # V_LEN0 + k: the k-th prescribed length > 1
LENGTHS = (FAN, FAN + 1, FAN * FAN, FAN * FAN + 1)


def frs(vals):
    return b"".join(ec.fr_to_bytes(v) for v in vals)


def coefficient(rnd):
    """1, r-1, 2, r-2, 2^16 and full-width values, none of them 0."""
    return rnd.choice((1, R - 1, 2, R - 2, 1 << 16, rnd.randrange(1 << 200, R)))


class Relation:
    """rows[m][i] = sorted [(column, coefficient)] of matrix m (A, B, C), zero coefficients included; z satisfies it."""

    def __init__(self, log_n, seed):
        rnd = random.Random(seed)
        self.log_n, self.n_pub = log_n, N_PUB
        n = 1 << log_n
        nc = self.nc = n - N_PUB
        lengths = [k for k in LENGTHS if k <= nc]
        a_only = V_LEN0 + len(lengths)  # 1 + len(lengths) variables only A mentions: the same lengths in the merged lists of l
        self.n_vars = a_only + 1 + len(lengths) + 6
        z = self.z = [1] + [rnd.randrange(R) for _ in range(self.n_vars - 1)]
        rows = [[dict() for _ in range(nc)] for _ in range(3)]
        for k, length in enumerate([1] + lengths):
            for i in rnd.sample(range(nc), length):
                rows[0][i][a_only + k] = coefficient(rnd)
        for m in range(3):
            rows[m][rnd.randrange(nc)][V_ONE_ROW] = coefficient(rnd)
            rows[m][min(2, nc - 1)][V_SAME_ROW] = coefficient(rnd)  # A, B and C on one row: l merges three lists on one point
            for i in rnd.sample(range(nc), min(3, nc)):
                rows[m][i][V_ZEROS] = 0  # dropped by the plan
            rows[m][rnd.randrange(nc)][V_ZEROS] = coefficient(rnd)
            for k, length in enumerate(lengths):
                for i in rnd.sample(range(nc), length):
                    rows[m][i][V_LEN0 + k] = coefficient(rnd)
                if length < nc:  # a zero entry beside a column of exactly `length` live terms
                    free = [i for i in range(nc) if V_LEN0 + k not in rows[m][i]]
                    rows[m][rnd.choice(free)][V_LEN0 + k] = 0
            for v in range(a_only + 1 + len(lengths), self.n_vars):  # filler, the public variables among its rows
                for i in rnd.sample(range(nc), min(4, nc)):
                    rows[m][i][v] = coefficient(rnd)
                    rows[m][i][rnd.choice((1, 2))] = coefficient(rnd)
        for i in range(nc):
            rows[0][i][0] = coefficient(rnd)  # the column every row mentions
            if not any(c for j, c in rows[1][i].items()):
                rows[1][i][1] = coefficient(rnd)
            ev = lambda row: sum(c * z[j] for j, c in row.items()) % R
            rows[2][i].pop(0, None)
            rows[2][i][0] = (ev(rows[0][i]) * ev(rows[1][i]) - ev(rows[2][i])) % R  # z[0] = 1 balances the row
        self.rows = [[sorted(r.items()) for r in mat] for mat in rows]
        self.oracle = g16.R1CS(self.n_vars, N_PUB, *self.rows)
        assert self.oracle.log_n == log_n and self.oracle.is_satisfied(z)

    def mats(self):
        """[(rowptr, col, val bytes)] * 3 for zkmi_r1cs_create and oracle.cpp."""
        out = []
        for mat in self.rows:
            rp, cl, vl = [0], [], []
            for row in mat:
                cl += [j for j, _ in row]
                vl += [c for _, c in row]
                rp.append(len(cl))
            out.append((rp, cl, frs(vl)))
        return out

    def witness(self):
        return frs(self.z)

    def expected_terms(self, which):
        """{column: sorted [(point, base selector, coefficient != 0)]} of query `which` (0 a, 1 b_g1, 2 b_g2, 4 l): base 0
        [L_i], 1 [alpha L_i], 2 [beta L_i]; the instance rows nc + j for j < n_pub in a and (on the beta base) in l."""
        src = {0: ((0, 0),), 1: ((1, 0),), 2: ((1, 0),), 4: ((0, 2), (1, 1), (2, 0))}[which]
        cols = {j: [] for j in range(self.n_vars)}
        for m, base in src:
            for i, row in enumerate(self.rows[m]):
                for j, c in row:
                    if c:
                        cols[j].append((i, base, c))
        if which in (0, 4):
            for j in range(self.n_pub):
                cols[j].append((self.nc + j, 2 if which == 4 else 0, 1))
        return {j: sorted(t) for j, t in cols.items()}


def check_plan(plan, expected):
    """Every invariant of a column-sum plan against the expected terms of its query; returns the number of levels used."""
    fan, terms, items = plan["fan"], plan["terms"], plan["items"]
    assert fan == FAN
    n_levels = plan["levels"]
    by_level = [[it for it in items if it[0] == l] for l in range(n_levels)]
    assert sum(len(b) for b in by_level) == len(items) and all(by_level)
    for _, _, _, count in items:
        assert 1 <= count <= fan
    # what every term stands for: k = min(c, r - c) with its flag and bit length, never 0
    coeff = []
    for point, base, neg, bits, k in terms:
        assert 0 < k <= (R - 1) // 2 and bits == k.bit_length() and neg in (0, 1)
        coeff.append((point, base, (R - k) if neg else k))
    # every partial written exactly once, outputs of a level dense from 0
    writer = []
    for l, level in enumerate(by_level):
        outs = [it[1] for it in level if not it[1] & FINAL]
        assert sorted(outs) == list(range(len(outs))), "a partial written twice or never"
        writer.append({it[1]: it for it in level if not it[1] & FINAL})
    finals = [it[1] & ~FINAL for it in items if it[1] & FINAL]
    assert len(set(finals)) == len(finals) and not set(finals) & set(plan["empty"])
    assert sorted(finals + plan["empty"]) == list(range(len(expected))), "a final slot written twice or never"
    reads = [[0] * len(terms)] + [[0] * len(w) for w in writer]

    def leaves(it):
        level, _, first, count = it
        out = []
        for q in range(first, first + count):
            reads[level][q] += 1
            out += [coeff[q]] if level == 0 else leaves(writer[level - 1][q])
        return out

    for it in items:
        if it[1] & FINAL:
            assert sorted(leaves(it)) == expected[it[1] & ~FINAL], it
    for j in plan["empty"]:
        assert expected[j] == []
    for l, r in enumerate(reads[: n_levels + 1]):
        assert all(c == 1 for c in r), "level %d: an input read twice or never" % l
    assert not writer[-1], "the last level writes partials nobody reads"
    longest = max(len(t) for t in expected.values())
    bound, p = 0, 1
    while p < longest:
        p, bound = p * fan, bound + 1
    assert n_levels <= max(1, bound)
    return n_levels


def oracle_setup_bytes(rel, delta=1):
    """The Python oracle's key with gamma = 1: (vk bytes, [a, b_g1, b_g2, h, l] wire bytes) as zkmi_pk_export_query numbers them."""
    pk, vk = g16.setup(rel.oracle, TAU, ALPHA, BETA, 1, delta)
    g1s = lambda pts: b"".join(ec.g1_to_bytes(p) for p in pts)
    q = [g1s(pk["a_query"]), g1s(pk["b_g1_query"]), b"".join(ec.g2_to_bytes(p) for p in pk["b_g2_query"]), g1s(pk["h_query"]),
         g1s(pk["l_query"])]
    vkb = ec.g1_to_bytes(vk["alpha_g1"]) + b"".join(ec.g2_to_bytes(vk[k]) for k in ("beta_g2", "gamma_g2", "delta_g2"))
    return vkb + g1s(vk["gamma_abc_g1"]), q
