"""Big-integer reference and test vectors for the device pairing tower (zk-apps_amd/csrc/pairing_dev.hip), shared by
test_cpu_tower.py (host path of zkmi_selftest_tower_ops, Fq2_28) and test_gpu_tower.py (device path, Fq2P lane pairs).

Every operand is a RAW limb array (tests/limbs28.py): the integer v it holds stands for v R^-1 mod p, in whatever
representation x + k p the caller chose.  Where an operand may lie is NOT written down here: zkmi_selftest_tower_bounds runs
the tower's own templates over intervals and returns, per operand class, the interval the kernels can produce; the vectors
put every residue at both ends of that interval, at k = 0, +-1 and in between.  Results are compared modulo p through
Field.value with oracle/bls12_381.py (a different representation of Fq12: Fq[w]/(w^12 - 2 w^6 + 2)), plus the range the op
promises (shrunk: |v| < 2 p; product: (-p/2, 3p/2)), plus normalised limbs."""
import ctypes as C

import numpy as np

import limbs28 as lb
from oracle import bls12_381 as ec

F = lb.FIELDS[0]
P, NL = F.p, F.NL

SITES = ("prod_operand", "prod_budget", "column_log2", "shrink_in", "is_zero_in", "stored")
CLASSES = ("F", "T_XY", "T_Z", "Q", "P", "L0", "L1", "L2", "E6_MUL", "E6_INV", "E2_XI", "E2_CONJ", "E2_INV", "SHRINK", "WORDS")


# ---- tower basis <-> the oracle's polynomial basis ----------------------------------------------------------------------
def tower_to_poly(co):
    """12 canonical integers in the order of e12_load (c0.a0.c0, c0.a0.c1, c0.a1.c0, ...) -> the oracle's
    Fq[w]/(w^12 - 2w^6 + 2): u = w^6 - 1, v = w^2."""
    poly = [0] * 12
    idx = 0
    for i in range(2):
        for j in range(3):
            for u in range(2):
                c = co[idx]
                idx += 1
                e = 2 * j + i
                if u == 0:
                    poly[e] = (poly[e] + c) % P
                else:
                    poly[e + 6] = (poly[e + 6] + c) % P
                    poly[e] = (poly[e] - c) % P
    return poly


def poly_to_tower(poly):
    """The inverse map: the coefficient of v^j w^i is (poly[e] + poly[e + 6]) + poly[e + 6] u with e = 2 j + i."""
    out = []
    for i in range(2):
        for j in range(3):
            e = 2 * j + i
            out += [(poly[e] + poly[e + 6]) % P, poly[e + 6] % P]
    return out


def _tower_to_poly(gt):
    """The 576 bytes of zkmi_pairing -> the oracle's basis."""
    return tower_to_poly([int.from_bytes(gt[48 * i : 48 * i + 48], "little") for i in range(12)])


def tower_bytes(co):
    return b"".join(int(c).to_bytes(48, "little") for c in co)


# ---- the hooks ----------------------------------------------------------------------------------------------------------
_BOUNDS = None


def bounds(zk):
    """(sites, classes) of zkmi_selftest_tower_bounds: {site: maximum}, {class: (lo, hi)} in units of p."""
    global _BOUNDS
    if _BOUNDS is None:
        s = (C.c_double * len(SITES))()
        c = (C.c_double * (2 * len(CLASSES)))()
        rc = zk.tlib.zkmi_selftest_tower_bounds(s, C.c_uint32(len(SITES)), c, C.c_uint32(len(CLASSES)))
        assert rc == 0, rc
        _BOUNDS = (dict(zip(SITES, s)), {n: (c[2 * i], c[2 * i + 1]) for i, n in enumerate(CLASSES)})
    return _BOUNDS


def call(zk, ctx, op, block, flag=False):
    """zkmi_selftest_tower_ops on an (n, n_in * 14) int32 block -> (n, n_out * 14) int32 array, or the n flag bytes."""
    o = OPS[op]
    n = block.shape[0]
    assert block.dtype == np.int32 and block.flags["C_CONTIGUOUS"] and block.shape[1] == len(o["cls"]) * NL, op
    out = np.zeros((n, max(o["n_out"], 1) * NL), dtype=np.int32)
    fl = np.full(n, 0xFF, dtype=np.uint8)
    rc = zk.tlib.zkmi_selftest_tower_ops(ctx.h if ctx is not None else C.c_void_p(None), C.c_int32(o["id"]), C.c_uint32(n),
                                         block.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                         fl.ctypes.data_as(C.c_void_p))
    assert rc == 0, (op, rc)
    return fl if flag else out


# ---- the operations: id, operand classes (one per Fq element), result elements -----------------------------------------
OPS = {}


def _op(name, oid, cls, n_out):
    OPS[name] = dict(id=oid, cls=tuple(cls), n_out=n_out)


_op("shrink", 0, ["SHRINK"], 1)
_op("e2_mul_xi", 1, ["E2_XI"] * 2, 2)
_op("e2_conj", 2, ["E2_CONJ"] * 2, 2)
_op("e2_inv", 3, ["E2_INV"] * 2, 2)
_op("e6_mul", 4, ["E6_MUL"] * 12, 6)
_op("e12_sqr", 5, ["F"] * 12, 12)
_op("e12_mul", 6, ["F"] * 24, 12)
_op("e12_mul_line", 7, ["F"] * 12 + ["L0"] * 2 + ["L1"] * 2 + ["L2"] * 2, 12)
_op("e12_conj", 8, ["F"] * 12, 12)
_op("e12_frob_p", 9, ["F"] * 12, 12)
_op("e12_frob_p2", 10, ["F"] * 12, 12)
_op("e6_inv", 11, ["E6_INV"] * 6, 6)
_op("e12_inv", 12, ["F"] * 12, 12)
_op("step_tangent", 13, ["T_XY"] * 4 + ["T_Z"] * 2 + ["P"] * 2, 12)
_op("step_chord", 14, ["T_XY"] * 4 + ["T_Z"] * 2 + ["Q"] * 4 + ["P"] * 2, 12)
_op("miller_rounds", 15, ["Q"] * 4 + ["P"] * 2, 12)
_op("final_exp_chain", 16, ["F"] * 12, 12)
_op("words_round_trip", 17, ["WORDS"], 2)
_op("is_one", 18, ["F"] * 12, 0)


# ---- representations ----------------------------------------------------------------------------------------------------
def span(cls, classes):
    """The integers a class admits: a closed range [lo, hi].  The class intervals are those of open promises ((-p/2, 3p/2),
    |v| < 2 p) and sums of them, so the ends themselves are left out."""
    lo, hi = classes[cls]
    num_lo, num_hi = int(round(lo * 2)), int(round(hi * 2))  # the hook's ends are multiples of 1/2
    assert num_lo == lo * 2 and num_hi == hi * 2, (cls, lo, hi)
    return num_lo * P // 2 + 1, -((-num_hi * P) // 2) - 1


def ks_of(x, cls, classes):
    """Every k with x + k p inside the class, x a residue in [0, p)."""
    lo, hi = span(cls, classes)
    k0, k1 = -((x - lo) // P), (hi - x) // P
    return list(range(k0, k1 + 1))


def pick_k(x, cls, classes, sel):
    """sel "lo" / "hi": the extreme k; an integer: walks both ends, 0, +-1 and the interior."""
    ks = ks_of(x, cls, classes)
    if sel == "lo":
        return ks[0]
    if sel == "hi":
        return ks[-1]
    menu = [ks[0], ks[-1]] + [k for k in (0, -1, 1) if k in ks] + ks[1:-1]
    return menu[sel % len(menu)]


def lift(val, cls, classes, sel):
    """The raw integer of the field element `val` (canonical) in the representation `sel` chooses."""
    x = val * F.R % P
    return x + pick_k(x, cls, classes, sel) * P


_RES = None


def residues():
    global _RES
    if _RES is None:
        _RES = lb.residues(F)
    return _RES


def generic_tuples(op, classes, cap=512, seed=0x70):
    """Raw-integer operand tuples of an op.  First every element at an end of its class: all high, all low, the two
    alternations, then per group of 12 elements every combination (2^groups), then seeded patterns (as Vectors.tuples puts
    2^arity combinations first, capped); the ends themselves (lo + 1 .. hi - 1 are the class's extreme integers) ride on the
    residues p - 1 and 1.  Then strided mixtures: element j of tuple t takes residue (t (2 j + 1) + j) and walks the k's of
    its class at another stride."""
    cls = OPS[op]["cls"]
    n = len(cls)
    res = residues()
    nr = len(res)
    rng = lb.SplitMix64(seed + OPS[op]["id"])
    pats = [[1] * n, [0] * n, [j & 1 for j in range(n)], [(j + 1) & 1 for j in range(n)], [(j >> 1) & 1 for j in range(n)]]
    groups = max(1, n // 12)
    for bits in range(1 << groups):
        pats.append([(bits >> min(j // 12, groups - 1)) & 1 for j in range(n)])
    for _ in range(24):
        w = rng.next() | (rng.next() << 64)
        pats.append([(w >> j) & 1 for j in range(n)])
    out = []
    for pi, pat in enumerate(pats):
        for far in (True, False):  # the extreme integers of the class, then other residues at the extreme k
            tup = []
            for j, b in enumerate(pat):
                lo, hi = span(cls[j], classes)
                if far:
                    tup.append(hi if b else lo)
                else:
                    x = res[(pi * 5 + 3 * j + 1) % nr]
                    tup.append(x + pick_k(x, cls[j], classes, "hi" if b else "lo") * P)
            out.append(tuple(tup))
    t = 0
    while len(out) < cap:
        tup = []
        for j in range(n):
            x = res[(t * (2 * j + 1) + j) % nr]
            tup.append(x + pick_k(x, cls[j], classes, t + 3 * j + t // 7) * P)
        out.append(tuple(tup))
        t += 1
    for tup in out:
        for v, c in zip(tup, cls):
            lo, hi = span(c, classes)
            assert lo <= v <= hi
    return out[:cap]


def block_of(tuples):
    flat = [v for t in tuples for v in t]
    return np.ascontiguousarray(lb.limbs_array(flat, NL).reshape(len(tuples), -1))


def ints_of(out):
    rows = out.reshape(-1, NL)
    assert lb.rows_normalised(rows)
    return np.array(lb.ints_of(rows), dtype=object).reshape(out.shape[0], -1).tolist()


def val(v):
    return F.value(v)


def vals(vs):
    return [F.value(v) for v in vs]


def is_shrunk(v):
    return -2 * P < v < 2 * P


def is_product(v):
    return -P < 2 * v < 3 * P


def in_class(v, cls, classes):
    lo, hi = span(cls, classes)
    return lo <= v <= hi


# ---- references ---------------------------------------------------------------------------------------------------------
def shrink_ref(v):
    """a - q p with q = floor(float32(top limb) * float32(1 / 106513)): the float program itself, in IEEE single precision."""
    top = v >> (28 * (NL - 1))
    q = int(np.floor(np.float32(top) * (np.float32(1.0) / np.float32(106513.0))))
    return v - q * P


def e6_to_poly(co6):
    return tower_to_poly(list(co6) + [0] * 6)


def poly_to_e6(poly):
    t = poly_to_tower(poly)
    assert not any(t[6:])
    return t[:6]


_FROB = {}


def frob_ref(poly, power):
    """a -> a^(p^power) as the Fq-linear map it is: the images of w^k under the oracle's f12_pow(., p^power)."""
    if power not in _FROB:
        wp = ec.f12_pow([0, 1] + [0] * 10, P**power)
        img, acc = [], ec.f12_one()
        for _ in range(12):
            img.append(acc)
            acc = ec.f12_mul(acc, wp)
        _FROB[power] = img
    out = [0] * 12
    for k, a in enumerate(poly):
        if a:
            out = [(o + a * c) % P for o, c in zip(out, _FROB[power][k])]
    return out


def f12_inv0(poly):
    return ec.f12_inv(poly) if any(poly) else [0] * 12


def line_poly(l0, l1, l2):
    """l0 + (l1 v + l2 v^2) w in the oracle's basis."""
    return tower_to_poly(list(l0) + [0] * 6 + list(l1) + list(l2))


XI = (1, 1)


def scaled_oracle_line(t_aff, q_aff, p_aff, factor):
    """The oracle's affine line through the untwisted t and q at P, times `factor` in Fq2 and times xi: with x = x'/w^2,
    y = y'/w^3 the oracle's l = lambda (xP - x) - (yP - y) satisfies
    l w^6 = -yP w^6 + (y' - lambda' x') w^3 + lambda' xP w^5, pairing_dev.hip's embedding (xi = w^6, v w = w^3)."""
    l = ec._line(ec._untwist(t_aff), ec._untwist(q_aff), (ec._f12_scalar(p_aff[0]), ec._f12_scalar(p_aff[1])))
    return ec.f12_mul(l, ec.fq2_to_f12(ec.Fq2.mul(factor, XI)))


def jac_to_affine(x, y, z):
    zi = ec.Fq2.inv(z)
    zi2 = ec.Fq2.sqr(zi)
    return ec.Fq2.mul(x, zi2), ec.Fq2.mul(y, ec.Fq2.mul(zi2, zi))


def fq2s(vs):
    v = vals(vs)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def check(op, tuples, outs, classes):
    """Asserts the raw outputs `outs` (rows of integers) of `op` on the raw operand `tuples`."""
    for t, (ins, got) in enumerate(zip(tuples, outs)):
        ctx = (op, t)
        a, g = vals(ins), vals(got)
        if op == "shrink":
            assert got[0] == shrink_ref(ins[0]) and is_shrunk(got[0]), ctx
        elif op == "e2_mul_xi":
            assert got == [ins[0] - ins[1], ins[0] + ins[1]], ctx
        elif op == "e2_conj":
            assert got == [ins[0], -ins[1]], ctx
        elif op == "e2_inv":
            assert tuple(g) == (ec.Fq2.inv(tuple(a)) if any(a) else (0, 0)), ctx
            assert is_product(got[0]) and is_product(-got[1]), ctx
        elif op == "e6_mul":
            assert g == poly_to_e6(ec.f12_mul(e6_to_poly(a[:6]), e6_to_poly(a[6:]))), ctx
            # sums of at most five products and one product times xi: c0 in (-6.5 p, 7.5 p), the others inside that
            assert all(-8 * P < v < 8 * P for v in got), ctx
        elif op == "e6_inv":
            assert g == poly_to_e6(f12_inv0(e6_to_poly(a))), ctx
            assert all(is_product(v) for v in got), ctx
        elif op in ("e12_sqr", "e12_mul", "e12_mul_line", "e12_inv"):
            x = tower_to_poly(a[:12])
            if op == "e12_sqr":
                want = ec.f12_mul(x, x)
            elif op == "e12_mul":
                want = ec.f12_mul(x, tower_to_poly(a[12:]))
            elif op == "e12_mul_line":
                want = ec.f12_mul(x, line_poly(a[12:14], a[14:16], a[16:18]))
            else:
                want = f12_inv0(x)
            assert tower_to_poly(g) == want, ctx
            assert all(is_shrunk(v) for v in got), ctx
        elif op == "e12_conj":
            assert got == list(ins[:6]) + [-v for v in ins[6:]], ctx
            assert tower_to_poly(g) == ec.f12_conj(tower_to_poly(a)), ctx
        elif op == "e12_frob_p":
            assert tower_to_poly(g) == frob_ref(tower_to_poly(a), 1), ctx
            assert got[:2] == [ins[0], -ins[1]] and all(is_product(v) for v in got[2:]), ctx
        elif op == "e12_frob_p2":
            assert tower_to_poly(g) == frob_ref(tower_to_poly(a), 2), ctx
            assert got[:2] == list(ins[:2]) and all(is_product(v) for v in got[2:]), ctx
        elif op in ("step_tangent", "step_chord"):
            T = fq2s(ins[:6])
            t_aff = jac_to_affine(*T)
            if op == "step_tangent":
                q_aff, (xp, nyp) = t_aff, a[6:8]
                factor = ec.Fq2.mul(ec.Fq2.muli(T[1], 2), ec.Fq2.mul(T[2], ec.Fq2.sqr(T[2])))  # 2 Y Z^3 of the old T
            else:
                q_aff, (xp, nyp) = fq2s(ins[6:10]), a[10:12]
                q_aff = (q_aff[0], q_aff[1])
            G = fq2s(got)
            assert jac_to_affine(*G[:3]) == ec.pt_add(ec.Fq2, t_aff, q_aff), ctx
            if op == "step_chord":
                factor = G[2]  # Z3
            want = scaled_oracle_line(t_aff, q_aff, (xp, (-nyp) % P), factor)
            assert line_poly(G[3], G[4], G[5]) == want, ctx
            assert all(is_shrunk(v) for v in got[:4]), ctx
            for k, c in ((4, "T_Z"), (6, "L0"), (8, "L1"), (10, "L2")):
                assert in_class(got[k], c, classes) and in_class(got[k + 1], c, classes), (ctx, c)
        elif op == "miller_rounds":
            q_aff, (xp, nyp) = fq2s(ins[:4]), a[4:6]
            want = ec.f12_conj(ec.miller_loop((xp, (-nyp) % P), (q_aff[0], q_aff[1])))  # the oracle conjugates: undo it
            ratio = ec.f12_mul(tower_to_poly(g), ec.f12_inv(want))
            assert ec.f12_pow(ratio, ec.FINAL_EXP) == ec.f12_one(), ctx  # the line factors lie in Fq2: killed
            assert all(is_shrunk(v) for v in got), ctx
        elif op == "final_exp_chain":
            x = tower_to_poly(a)
            assert tower_to_poly(g) == (ec.f12_pow(x, ec.FINAL_EXP) if any(x) else [0] * 12), ctx
            assert all(is_shrunk(v) for v in got), ctx
        else:
            raise ValueError(op)


def check_words(raw_out, ins):
    """limbs_to_words: the unique canonical integer in [0, p), slots 12 and 13 zero; limbs_from_words of it: the exact
    product mont(c R^2)."""
    words = raw_out[:, :NL].view(np.uint32)
    assert not words[:, 12:].any()
    back = lb.ints_of(raw_out[:, NL:])
    assert lb.rows_normalised(raw_out[:, NL:])
    for v, row, b in zip(ins, words, back):
        c = sum(int(w) << (32 * i) for i, w in enumerate(row[:12]))
        assert c == F.value(v) and 0 <= c < P, (v, c)
        assert b == F.rep(c) and is_product(b), (v, b)


def run_generic(zk, ctx, op, classes, tuples=None, cap=512):
    """One op over its vectors: reference, ranges, normalised limbs.  Returns (tuples, raw output)."""
    tuples = generic_tuples(op, classes, cap) if tuples is None else tuples
    raw = call(zk, ctx, op, block_of(tuples))
    if op == "words_round_trip":
        check_words(raw, [t[0] for t in tuples])
    else:
        check(op, tuples, ints_of(raw), classes)
    return tuples, raw


def residues_equal(a, b):
    """Two raw outputs hold the same field elements (Fq2P and Fq2_28 products may reduce to different representations)."""
    x, y = lb.ints_of(a.reshape(-1, NL)), lb.ints_of(b.reshape(-1, NL))
    return all((u - v) % P == 0 for u, v in zip(x, y))


# ---- special vectors ----------------------------------------------------------------------------------------------------
def zero_held_tuples(op, classes, seed=0x5A):
    """Tuples of an Fq12 op whose coefficients are = 0 but held as +-p and +-2 p (the closed ends of the class): every
    coefficient in turn, every other one, all of them."""
    cls = OPS[op]["cls"]
    n = len(cls)
    base = generic_tuples(op, classes, cap=64, seed=seed)[-8:]
    reps = [P, -P, 0, 2 * P, -2 * P]
    out = []
    for bi, b in enumerate(base):
        for j in range(0, n, 1 if bi == 0 else 5):
            t = list(b)
            t[j] = reps[(j + bi) % 5]
            out.append(tuple(t))
        out.append(tuple(reps[(j + bi) % 5] if (j + bi) % 2 else v for j, v in enumerate(b)))
    out.append(tuple(reps[j % 2] for j in range(n)))
    out.append(tuple(reps[(j + 1) % 2] for j in range(n)))
    return out


def subfield_tuples(classes, seed=0x5B):
    """f in Fq, Fq2 and Fq6 inside Fq12 (the other coefficients 0 held as 0 or +-p), every live coefficient at an end of F."""
    res = residues()
    out = []
    for live in (1, 2, 6):
        for s, sel in enumerate(("hi", "lo", 3, 4)):
            t = []
            for j in range(12):
                if j < live:
                    x = res[(7 * j + 11 * s + live + 9) % len(res)] or 5
                    t.append(x + pick_k(x, "F", classes, sel) * P)
                else:
                    t.append((0, P, -P)[(j + s) % 3])
            out.append(tuple(t))
    return out


def inv_special_tuples(op, classes):
    """0 and 1 in their representations: zero must come back as zero with no special path."""
    cls = OPS[op]["cls"]
    n = len(cls)
    one = F.R1
    out = []
    for z in (0, P, -P):
        out.append(tuple([z] * n))
    for k in ks_of(one, cls[0], classes):
        out.append(tuple([one + k * P] + [0] * (n - 1)))
        out.append(tuple([one + k * P] + [(P, -P)[j % 2] for j in range(n - 1)]))
    return out


def is_one_tuples(classes):
    """(tuples, expected flag): coefficient 0 as ONE + k p for every k the class admits and the others = 0 held as 0, +-p,
    +-2 p -> 1; near misses (one unit off in one limb of one coefficient, a coefficient = 1, ONE in the wrong slot) -> 0."""
    one = F.R1
    zeros = (0, P, -P, 2 * P, -2 * P)
    lo, hi = span("F", classes)
    zeros_in = [z for z in zeros if lo - 1 <= z <= hi + 1]  # +-2 p: the closed end of the class, exact for is_zero (<= 4 p)
    tuples, want = [], []
    ks = list(range(-2, 2))
    for k in ks:
        assert -2 * P <= one + k * P <= 2 * P
        for s in range(len(zeros_in)):
            tuples.append(tuple([one + k * P] + [zeros_in[(s + j) % len(zeros_in)] for j in range(11)]))
            want.append(1)
    for k in ks:
        for j in range(12):
            for d in (1, -1, 1 << 28, -(1 << (28 * 13))):
                t = [one + k * P] + [zeros_in[(j + i) % len(zeros_in)] for i in range(11)]
                t[j] += d
                if abs(t[j]) < 2 * P:
                    tuples.append(tuple(t))
                    want.append(0)
    tuples.append(tuple([0] * 12)), want.append(0)
    tuples.append(tuple([0, one] + [0] * 10)), want.append(0)
    tuples.append(tuple([one, one] + [0] * 10)), want.append(0)
    tuples.append(tuple([one] + [0] * 10 + [one])), want.append(0)
    tuples.append(tuple([1] + [0] * 11)), want.append(0)  # the integer 1 is not the field's one
    return tuples, want


# ---- points for the steps and the Miller loop ---------------------------------------------------------------------------
X_ABS = -ec.X
_POINTS = None


def points():
    """Real subgroup points: (P, Q) pairs and, per Q, T = [k] Q for k in {1, 2, 3, |x| >> 1}."""
    global _POINTS
    if _POINTS is None:
        rng = lb.SplitMix64(0x7031)
        out = []
        for _ in range(2):
            p = ec.g1_mul(rng.below(ec.R - 1) + 1)
            q = ec.g2_mul(rng.below(ec.R - 1) + 1)
            ts = [(k, ec.g2_mul(k, q)) for k in (1, 2, 3, X_ABS >> 1)]
            out.append((p, q, ts))
        _POINTS = out
    return _POINTS


def _lift2(v2, cls, classes, sel):
    return [lift(v2[0], cls, classes, sel), lift(v2[1], cls, classes, sel if isinstance(sel, str) else sel + 1)]


def step_tuples(op, classes, seed=0x7E):
    """T = [k] Q re-scaled by a random z to make it Jacobian, and T = Q with z = 1 in the representations of one its class
    admits; every coordinate lifted to the ends of its class, to k = 0, +-1 and in between.  A z held as a negative integer
    is among them (the class of z reaches down to -p: the tangent step doubles a product)."""
    rng = lb.SplitMix64(seed)
    out = []
    sels = ("hi", "lo", 2, 3, 4, 5)
    flip = {"hi": "lo", "lo": "hi"}
    for p, q, ts in points():
        xp, nyp = p[0], (-p[1]) % P
        for k, t in ts:
            if op == "step_chord" and k == 1:
                continue  # T = Q has no chord; the loop never adds Q to +-Q
            for si, sel in enumerate(sels):
                z = (1, 0) if k == 1 and si < 3 else (rng.below(P - 1) + 1, rng.below(P - 1) + 1)
                z2 = ec.Fq2.sqr(z)
                X, Y = ec.Fq2.mul(t[0], z2), ec.Fq2.mul(t[1], ec.Fq2.mul(z2, z))
                other = flip.get(sel, sel)
                tup = _lift2(X, "T_XY", classes, sel) + _lift2(Y, "T_XY", classes, other)
                tup += _lift2(z, "T_Z", classes, other if si < 2 else "lo" if si % 2 else sel)
                if op == "step_chord":
                    tup += _lift2(q[0], "Q", classes, sel) + _lift2(q[1], "Q", classes, other)
                tup += [lift(xp, "P", classes, other), lift(nyp, "P", classes, sel)]
                out.append(tuple(tup))
    assert any(t[4] < 0 and t[5] < 0 for t in out)
    return out


def miller_tuples(classes, n=8):
    out = []
    sels = ("hi", "lo", 2, 3, 4, 5, 6, 7)
    pts = points()
    for i in range(n):
        p, q, _ = pts[i % len(pts)]
        sel = sels[i % len(sels)]
        other = "lo" if sel == "hi" else "hi" if sel == "lo" else sel + 1
        tup = _lift2(q[0], "Q", classes, sel) + _lift2(q[1], "Q", classes, other)
        tup += [lift(p[0], "P", classes, other), lift((-p[1]) % P, "P", classes, sel)]
        out.append(tuple(tup))
    return out
