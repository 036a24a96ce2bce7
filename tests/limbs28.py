"""Big-integer reference and test vectors for the device limb arithmetic (zk-apps_amd/csrc/field28.hpp), shared by
test_cpu_field28.py (host path of zkmi_selftest_fp28_ops) and test_gpu_field28.py (device path, NTT closed forms).

A field element is NL signed 28-bit limbs; the integer it holds is v = sum l[i] 2^(28 i), limbs 0..NL-2 in [0, 2^28), the top
limb signed.  v is a Montgomery form with R = 2^(28 NL): it stands for v R^-1 mod p, in ANY representation v + k p with
|v| < 16 p.  Every reference here is Python int arithmetic; a Montgomery reduction's result is predicted exactly:
mont(T) = (T + m p) / R with m = -T p^-1 mod R, the one m in [0, R) the limb-wise reduction can produce."""
import ctypes as C

import numpy as np

from oracle import bls12_381 as bls
from oracle import bn254 as bn

MASK = (1 << 28) - 1
KS = (-16, -15, -8, -4, -1, 0, 1, 4, 8, 14, 15)


class Field:
    def __init__(self, fid, name, p, nl, n32):
        self.id, self.name, self.p, self.NL, self.N32 = fid, name, p, nl, n32
        self.R = 1 << (28 * nl)
        self.R1 = self.R % p  # one()
        self.R2 = self.R * self.R % p
        self.Rinv = pow(self.R, -1, p)
        self.pinv = pow(p, -1, self.R)
        self.INV = (-self.pinv) % (1 << 28)  # -p^-1 mod 2^28

    def mont(self, t):
        """The exact integer a Montgomery reduction of the column sum t returns."""
        m = (-t * self.pinv) % self.R
        q, rem = divmod(t + m * self.p, self.R)
        assert rem == 0
        return q

    def rep(self, c):
        """from_canonical(c): the representation the library holds for the canonical integer c."""
        return self.mont(c * self.R2)

    def value(self, v):
        """The canonical integer the Montgomery form v stands for."""
        return v * self.Rinv % self.p

    def __repr__(self):
        return self.name


FIELDS = (Field(0, "Fq28", bls.P, 14, 12), Field(1, "Fr28", bls.R, 10, 8), Field(2, "BnFq28", bn.P, 10, 8),
          Field(3, "BnFr28", bn.R, 10, 8))


def to_limbs(v, nl):
    return [(v >> (28 * i)) & MASK for i in range(nl - 1)] + [v >> (28 * (nl - 1))]


def from_limbs(limbs):
    return sum(int(x) << (28 * i) for i, x in enumerate(limbs))


def normalised(limbs):
    return all(0 <= int(x) <= MASK for x in limbs[:-1])


def limbs_array(values, nl):
    """(len(values), nl) int32 array; a top limb that does not fit int32 is the caller's mistake."""
    rows = [to_limbs(v, nl) for v in values]
    for r in rows:
        assert -(1 << 31) <= r[-1] < (1 << 31)
    return np.array(rows, dtype=np.int64).astype(np.int32)


def ints_of(arr):
    """Rows of an (n, nl) int32 limb array as Python ints."""
    a = arr.astype(np.int64).astype(object)
    acc = a[:, 0]
    for i in range(1, a.shape[1]):
        acc = acc + (a[:, i] << (28 * i))
    return [int(x) for x in acc]


def rows_normalised(arr):
    low = arr[:, :-1]
    return bool(((low >= 0) & (low <= MASK)).all())


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & (2**64 - 1)

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return z ^ (z >> 31)

    def below(self, p):
        """Uniform over [0, p) by rejection."""
        words = (p.bit_length() + 63) // 64
        while True:
            v = 0
            for i in range(words):
                v |= self.next() << (64 * i)
            v &= (1 << p.bit_length()) - 1
            if v < p:
                return v


def residues(f, seed=0x28):
    p = f.p
    out = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, f.R1, f.R2]
    for i in range(1, f.NL):
        if (1 << (28 * i)) < p:
            out += [(1 << (28 * i)) - 1, 1 << (28 * i)]
    if f.id == 0:
        out += [(1 << 380) - 1, 1 << 380, (1 << 380) + ((p - (1 << 380)) // 3)]
        assert (1 << 380) < out[-1] < p
    rng = SplitMix64(seed + f.id)
    out += [rng.below(p) for _ in range(32)]
    seen, uniq = set(), []
    for x in out:
        if x not in seen:
            seen.add(x)
            uniq.append(x)
    return uniq


class Vectors:
    """The representations x + k p of a field's residues (|v| < 16 p), as integers and as limb rows, and index tuples over them."""

    def __init__(self, f):
        self.f = f
        self.res = residues(f)
        self.nr = len(self.res)
        self.vals, self.index = [], {}
        for ri, x in enumerate(self.res):
            for ki, k in enumerate(KS):
                v = x + k * f.p
                if abs(v) >= 16 * f.p:
                    continue
                self.index[(ri, ki)] = len(self.vals)
                self.vals.append(v)
        # the two ends of the representation range, for the tuples that put every operand at a bound
        self.hi = self.index[(self.res.index(f.p - 1), KS.index(15))]  # 16 p - 1
        self.lo = self.index[(self.res.index(1), KS.index(-16))]  # -16 p + 1
        self.limbs = limbs_array(self.vals, f.NL)

    def tuples(self, arity):
        """Index tuples into vals.  One operand: every representation.  More: for every (k_a, k_b) of the first two operands
        every residue as the first operand (the others walk the residues and the k's at other strides), then every way of
        putting each operand at one of the two ends of the range (2^arity tuples).  At most 2^15 tuples."""
        nk = len(KS)
        out = []
        if arity == 1:
            return [(i,) for i in range(len(self.vals))]
        for t in range(nk * nk * self.nr):
            pair, blk = t % (nk * nk), t // (nk * nk)
            tup = []
            for j in range(arity):
                ki = ((pair // nk if j % 2 else pair % nk) + (j // 2) * (1 + blk + 3 * (pair // nk))) % nk
                ri = (blk * (2 * j + 1) + pair * 3 * j + j) % self.nr
                tup.append(self.index.get((ri, ki)))
            if None not in tup:
                out.append(tuple(tup))
        for bits in range(1 << arity):
            out.append(tuple(self.hi if (bits >> j) & 1 else self.lo for j in range(arity)))
        assert len(out) <= 1 << 15
        return out

    def gather(self, tuples):
        """(n, arity * NL) int32 input block and the operands as integers."""
        idx = np.array(tuples, dtype=np.int64)
        block = self.limbs[idx.reshape(-1)].reshape(len(tuples), -1)
        ints = [[self.vals[i] for i in t] for t in tuples]
        return np.ascontiguousarray(block), ints


_VECTORS = {}


def vectors(f):
    if f.id not in _VECTORS:
        _VECTORS[f.id] = Vectors(f)
    return _VECTORS[f.id]


# ---- the operations of zkmi_selftest_fp28_ops (include/zkmi_testing.h) -------------------------------------------------
# name -> (op id, operand elements, result elements, kind)
#   kind "exact": ref(f, ops) -> the exact result integers
#   kind "mont" : ref(f, ops) -> the column sums T; the result is f.mont(T), promised in (-p/2, 3p/2) unless `wide`
OPS = {}


def _op(name, oid, n_in, n_out, kind, ref, wide=False, fields=(0, 1, 2, 3), where="both"):
    OPS[name] = dict(id=oid, n_in=n_in, n_out=n_out, kind=kind, ref=ref, wide=wide, fields=fields, where=where)


def _fq2_mul(a0, a1, b0, b1):
    return [a0 * b0 - a1 * b1, a0 * b1 + a1 * b0]


_op("add", 0, 2, 1, "exact", lambda f, o: [o[0] + o[1]])
_op("sub", 1, 2, 1, "exact", lambda f, o: [o[0] - o[1]])
_op("neg", 2, 1, 1, "exact", lambda f, o: [-o[0]])
_op("dbl", 3, 1, 1, "exact", lambda f, o: [2 * o[0]])
_op("carry", 4, 2, 1, "exact", lambda f, o: [o[0] + o[1]])
_op("mul", 5, 2, 1, "mont", lambda f, o: [o[0] * o[1]])
_op("sqr", 6, 1, 1, "mont", lambda f, o: [o[0] * o[0]])
_op("lazy_mul", 7, 4, 1, "mont", lambda f, o: [(o[0] + o[1]) * (o[2] - o[3])])
# two lazy differences of values at +-16 p and a second product: |T| / R reaches 1280 p^2 / R = 0.508 p in Fq28, so the
# range is (-p, 2p) there, not the (-p/2, 3p/2) of a single product (field28.hpp says so at f_mul_sub_mul)
_op("mul_sub_mul", 8, 6, 1, "mont", lambda f, o: [(o[0] - o[1]) * (o[2] - o[3]) - o[4] * o[5]], wide=True)
_op("x3", 9, 3, 1, "exact", lambda f, o: [o[0] - o[1] - 2 * o[2]])
_op("signed_sub_mul", 10, 3, 2, "mont", lambda f, o: [(o[0] - o[1]) * o[2], (-o[0] - o[1]) * o[2]])
_op("inv", 14, 1, 1, "inv", None)
_op("fq2_mul", 15, 4, 2, "mont", lambda f, o: _fq2_mul(*o), fields=(0,))
_op("fq2_sqr", 16, 2, 2, "mont", lambda f, o: [(o[0] + o[1]) * (o[0] - o[1]), 2 * o[0] * o[1]], fields=(0,))
_op("fq2_mul_sub_mul", 17, 8, 2, "mont",
    lambda f, o: [x - y for x, y in zip(_fq2_mul(*o[0:4]), _fq2_mul(*o[4:8]))], fields=(0,))
_op("fq2_x3", 18, 6, 2, "exact", lambda f, o: [o[0] - o[2] - 2 * o[4], o[1] - o[3] - 2 * o[5]], fields=(0,))
_op("pair_mul", 19, 4, 2, "mont", lambda f, o: _fq2_mul(*o), fields=(0,), where="device")
_op("pair_sqr", 20, 2, 2, "mont", lambda f, o: [(o[0] + o[1]) * (o[0] - o[1]), 2 * o[0] * o[1]], fields=(0,), where="device")
_op("pair_mul_sub_mul", 21, 8, 2, "mont",
    lambda f, o: [x - y for x, y in zip(_fq2_mul(*o[0:4]), _fq2_mul(*o[4:8]))], fields=(0,), where="device")
_op("pair_signed_sub", 22, 4, 4, "exact", lambda f, o: [o[0] - o[2], o[1] - o[3], -o[0] - o[2], -o[1] - o[3]],
    fields=(0,), where="device")
_op("mul_fips", 24, 2, 1, "mont", lambda f, o: [o[0] * o[1]], where="host")
_op("sqr_fips", 25, 1, 1, "mont", lambda f, o: [o[0] * o[0]], where="host")
_op("fips2", 26, 4, 1, "mont", lambda f, o: [o[0] * o[1] + o[2] * o[3]], where="host")
_op("fips4", 27, 8, 1, "mont", lambda f, o: [o[0] * o[1] + o[2] * o[3] + o[4] * o[5] + o[6] * o[7]], where="host")
OP_IS_ZERO, OP_FROM_CANON, OP_TO_CANON, OP_PAIR_IS_ZERO = 11, 12, 13, 23


def op_names(f, device):
    return [n for n, o in OPS.items() if f.id in o["fields"] and o["where"] in ("both", "device" if device else "host")]


def call(zk, ctx, f, op_id, block, n_out, n_flag=0):
    """zkmi_selftest_fp28_ops on an (n, n_in * NL) int32 block -> ((n, n_out * NL) int32 array, (n, n_flag) uint8 array)."""
    n = block.shape[0]
    assert block.dtype == np.int32 and block.flags["C_CONTIGUOUS"]
    out = np.zeros((n, max(n_out, 1) * f.NL), dtype=np.int32)
    flag = np.full((n, max(n_flag, 1)), 0xFF, dtype=np.uint8)
    rc = zk.tlib.zkmi_selftest_fp28_ops(ctx.h if ctx is not None else C.c_void_p(None), C.c_int32(f.id), C.c_int32(op_id),
                                        C.c_uint32(n), block.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                        flag.ctypes.data_as(C.c_void_p))
    assert rc == 0, (f.name, op_id, rc)
    return out, flag


def check_op(zk, ctx, f, name):
    """Runs one op of OPS over the field's vectors and asserts (a) the residue, (b) normalised limbs, (c) the promised range
    -- all three through the exact expected integer where the op determines it.  Returns the raw output for a word-for-word
    comparison between the two paths."""
    o, vec, p = OPS[name], vectors(f), f.p
    tuples = vec.tuples(o["n_in"])
    block, ints = vec.gather(tuples)
    out, _ = call(zk, ctx, f, o["id"], block, o["n_out"])
    assert rows_normalised(out.reshape(-1, f.NL)), name
    got = np.array(ints_of(out.reshape(-1, f.NL)), dtype=object).reshape(len(tuples), o["n_out"])
    for t, ops in enumerate(ints):
        if o["kind"] == "inv":
            (x,) = ops
            (v,) = got[t]
            assert 2 * v > -p and 2 * v < 3 * p, (name, x, v)
            if x % p == 0:
                assert v % p == 0, (name, x, v)
            else:
                assert v * x * f.Rinv % p == f.R1 and f.value(v) * f.value(x) % p == 1, (name, x, v)
            continue
        want = o["ref"](f, ops)
        for j, w in enumerate(want):
            v = got[t][j]
            if o["kind"] == "exact":
                assert v == w, (name, ops, j, v, w)
            else:
                assert v == f.mont(w) and (v - w * f.Rinv) % p == 0, (name, ops, j, v, f.mont(w))
                if o["wide"]:
                    assert -p < v < 2 * p, (name, ops, j, v)
                else:
                    assert 2 * v > -p and 2 * v < 3 * p, (name, ops, j, v)
    return out


def is_zero_vectors(f):
    """(values, expected flag): (d) k p, |k| <= 4 -> true; (e) k p +- 1, k p +- 2^(28 i) for every limb i, values that share
    the top limb of some k p, and every representation within 4 p of a non-zero residue -> false."""
    p, nl = f.p, f.NL
    vals, want = [], []
    for k in range(-4, 5):
        vals.append(k * p), want.append(1)
        for d in [1] + [1 << (28 * i) for i in range(nl)]:
            for s in (1, -1):
                vals.append(k * p + s * d), want.append(0)
        top = (k * p) >> (28 * (nl - 1))
        rng = SplitMix64(0x15 + k + 9 * f.id)
        for _ in range(4):
            v = (top << (28 * (nl - 1))) | (rng.below(1 << (28 * (nl - 1))))
            if v != k * p:
                vals.append(v), want.append(0)
        # only one lower limb differs from k p
        for i in range(nl - 1):
            vals.append(k * p ^ (1 << (28 * i + 27))), want.append(0)
    vec = vectors(f)
    for v in vec.vals:
        if abs(v) <= 4 * p and v % p:
            vals.append(v), want.append(0)
    return vals, want


def check_is_zero(zk, ctx, f):
    vals, want = is_zero_vectors(f)
    _, flag = call(zk, ctx, f, OP_IS_ZERO, limbs_array(vals, f.NL), 0, 1)
    got = flag[:, 0].tolist()
    bad = [(v // f.p, v % f.p, g, w) for v, g, w in zip(vals, got, want) if g != w]
    assert not bad, (f.name, bad[:4])
    return flag


def canonical_values(f):
    return vectors(f).res


def check_from_canonical(zk, ctx, f):
    """Canonical words in -> the exact representation mont(w R^2), in (-p/2, 3p/2)."""
    xs = canonical_values(f)
    block = np.zeros((len(xs), f.NL), dtype=np.uint32)
    for t, x in enumerate(xs):
        for i in range(f.N32):
            block[t, i] = (x >> (32 * i)) & 0xFFFFFFFF
    out, _ = call(zk, ctx, f, OP_FROM_CANON, block.view(np.int32), 1)
    assert rows_normalised(out)
    for x, v in zip(xs, ints_of(out)):
        assert v == f.rep(x) and f.value(v) == x and 2 * v > -f.p and 2 * v < 3 * f.p, (f.name, x, v)
    return out


def check_to_canonical(zk, ctx, f):
    """Every representation -> the unique canonical integer in [0, p), the slots past N32 zero."""
    vec = vectors(f)
    out, _ = call(zk, ctx, f, OP_TO_CANON, np.ascontiguousarray(vec.limbs), 1)
    words = out.view(np.uint32)
    assert not words[:, f.N32:].any()
    for v, row in zip(vec.vals, words):
        got = sum(int(w) << (32 * i) for i, w in enumerate(row[: f.N32]))
        assert got == f.value(v) and 0 <= got < f.p, (f.name, v, got)
    return out


# ---- NTT closed forms ---------------------------------------------------------------------------------------------------
# Transforms of the constant vector (c, c, ...) and of the alternating vector (c, -c, c, ...): the inputs whose entries add
# up coherently, so that intermediate values grow like N (random vectors: like sqrt N).  `kind` -> the sparse output
# {index: value} (every other entry 0), or for the forward coset transform of a constant, which is dense, a function of k.
NTT_G = 7


def ntt_root(f, log_n):
    from oracle import ntt as bls_ntt

    return bls_ntt.root_of_unity(log_n) if f.id == 1 else bn.root_of_unity(log_n)


def ntt_input(kind, c, r):
    """The repeating pattern of the input vector: (c,) or (c, r - c)."""
    return (c,) if kind.startswith("const") else (c, (r - c) % r)


def ntt_closed_form(f, kind, log_n, c):
    """kind: "<const|alt>_<fwd|inv>[_coset]" for the natural-order entry points (oracle/ntt.py's definitions), or
    "<const|alt>_dif<0|1>" for zkmi_selftest_ntt_dif_dev (bit-reversed positions, post 0 / 1)."""
    r, n = f.p, 1 << log_n
    vec, way = kind.split("_", 1)
    half = n // 2
    if way == "fwd":
        return {0 if vec == "const" else half: n * c % r}
    if way == "inv":
        return {0 if vec == "const" else half: c}
    if way == "inv_coset":  # the inverse transform's entry j, times g^-j
        return {0: c} if vec == "const" else {half: c * pow(NTT_G, -half, r) % r}
    if way == "fwd_coset":  # sum_i c x^i = c (x^N - 1) / (x - 1) with x = +-g w^k, x^N = g^N: dense
        w, gn = ntt_root(f, log_n), pow(NTT_G, n, r)
        sign = 1 if vec == "const" else -1
        return lambda k: c * (gn - 1) * pow(sign * NTT_G * pow(w, k, r) - 1, -1, r) % r
    if way == "dif0":  # unscaled sums, bit-reversed: index 0 stays, index N/2 lands on position 1
        return {0 if vec == "const" else 1: n * c % r}
    if way == "dif1":  # ... times g^rev(p) / N
        return {0: c} if vec == "const" else {1: c * pow(NTT_G, half, r) % r}
    raise ValueError(kind)


def ntt_constants(f, seed=0x4E5454, candidates=4096):
    """The canonical c whose library representation from_canonical(c) -- the integer that doubles along a sum path -- is the
    largest, the smallest, and the one with the largest rep(c) - rep(r - c) (the alternating vector's last lazy difference),
    among seeded candidates and the edge residues; plus r - 1 and 1."""
    rng = SplitMix64(seed + f.id)
    cand = [x for x in residues(f) if x] + [rng.below(f.p - 1) + 1 for _ in range(candidates)]
    hi = max(cand, key=f.rep)
    lo = min(cand, key=f.rep)
    diff = max(cand, key=lambda c: f.rep(c) - f.rep(f.p - c))
    out = []
    for c in (hi, lo, diff, f.p - 1, 1):
        if c not in out:
            out.append(c)
    return out
