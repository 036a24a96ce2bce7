"""Test vectors for the device point readers (csrc/points.hip): a mixed corpus of BLS12-381 G1 / G2 encodings, every
element labelled with the class it was built as.  Built from the oracle only (oracle/bls12_381.py); nothing here calls
the code under test.  tests/test_cpu_points.py holds the corpus itself to the oracle and to the product's host
functions, tests/test_gpu_points.py holds the device to the corpus.

Classes (not every class exists in every encoding: the wire form has no flag bits and one way to write infinity):
  valid         subgroup points, both values of the sort bit, infinity among them
  bad_flags     compression / sort flag that the encoding does not allow
  noncanon_inf  infinity flag with anything else set
  x_ge_p        a coordinate that is not reduced
  no_root       x for which x^3 + b is not a square (uncompressed forms: with some y)
  off_subgroup  random points of the curve (the cofactors are huge: none is in the subgroup)
  order_<q>     points of small prime order q
  mixed_<q>     [k]G + T with T of order q: on the curve, outside the subgroup, nothing small about it
"""
import functools
import random

from oracle import bls12_381 as ec

ENC_WIRE, ENC_COMPRESSED, ENC_UNCOMPRESSED = 0, 1, 2
CHECK_CURVE, CHECK_SUBGROUP = 1, 2
OK, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = 0, 1, 2, 3

P, R = ec.P, ec.R
X_PARAM = -0xD201000000010000
H1 = (X_PARAM - 1) ** 2 // 3
H2 = (X_PARAM**8 - 4 * X_PARAM**7 + 5 * X_PARAM**6 - 4 * X_PARAM**4 + 6 * X_PARAM**3 - 4 * X_PARAM**2 - 4 * X_PARAM + 13) // 9
# (q, e): q^e is the full power of q in the cofactor
SMALL_ORDERS = {1: [(3, 1), (11, 2), (10177, 2)], 2: [(13, 2), (23, 2), (2713, 1)]}
MIN_MEMBERS = {1: 64, 2: 16}


def field(group):
    return (ec.Fq, ec.B_G1, H1) if group == 1 else (ec.Fq2, ec.B_G2, H2)


def point_bytes(group, enc):
    return (96 if group == 1 else 192) // (2 if enc == ENC_COMPRESSED else 1)


def _rand_fe(group, rnd):
    return rnd.randrange(P) if group == 1 else (rnd.randrange(P), rnd.randrange(P))


def _step(group, x):
    return (x + 1) % P if group == 1 else ((x[0] + 1) % P, x[1])


def _rhs(group, x):
    F, b, _ = field(group)
    return F.add(F.mul(F.sqr(x), x), b)


def _sqrt(group, a):
    return ec.fq_sqrt(a) if group == 1 else ec.fq2_sqrt(a)


def random_curve_point(group, rnd):
    """x at random, stepped until x^3 + b has a root; the root or its negative at random."""
    F, _, _ = field(group)
    x = _rand_fe(group, rnd)
    while True:
        y = _sqrt(group, _rhs(group, x))
        if y is not None:
            return (x, F.neg(y) if rnd.getrandbits(1) else y)
        x = _step(group, x)


def x_without_root(group, rnd):
    x = _rand_fe(group, rnd)
    while _sqrt(group, _rhs(group, x)) is not None:
        x = _step(group, x)
    return x


def small_order_point(group, q, e, rnd):
    """T = [r h / q^e] P for a random curve point P: order q (or O: try again)."""
    F, _, h = field(group)
    assert h % q**e == 0 and h % q ** (e + 1) != 0
    while True:
        t = ec.pt_mul(F, random_curve_point(group, rnd), R * h // q**e)
        if t is not None:
            return t


# ---- encoders (the three byte forms as the issue and csrc/wire.hip state them) ---------------------------------------
def _coords(group, pt):
    """Coordinates as the big-endian forms order them: the high component of Fq2 first."""
    if group == 1:
        return [pt[0]], [pt[1]]
    return [pt[0][1], pt[0][0]], [pt[1][1], pt[1][0]]


def encode(group, enc, pt):
    if enc == ENC_WIRE:
        return ec.g1_to_bytes(pt) if group == 1 else ec.g2_to_bytes(pt)
    if enc == ENC_COMPRESSED:
        return ec.g1_compress(pt) if group == 1 else ec.g2_compress(pt)
    if pt is None:
        return bytes([0x40]) + bytes(point_bytes(group, enc) - 1)
    xs, ys = _coords(group, pt)
    return b"".join(v.to_bytes(48, "big") for v in xs + ys)


def _raw(group, enc, xs, ys, flags=0):
    """Element from raw coordinate integers (each < 2^384), components low first, and extra flag bits for byte 0."""
    if enc == ENC_WIRE:
        return b"".join(v.to_bytes(48, "little") for v in xs + ys)
    vals = list(reversed(xs)) + ([] if enc == ENC_COMPRESSED else list(reversed(ys)))
    out = bytearray(b"".join(v.to_bytes(48, "big") for v in vals))
    out[0] |= flags
    return bytes(out)


def _comps(group, fe):
    return [fe] if group == 1 else [fe[0], fe[1]]


# ---- the oracle's verdict on one element ---------------------------------------------------------------------------
def oracle_status(group, enc, b, checks):
    """Status byte from the oracle's arithmetic and the encoding rules, smallest fault first."""
    F, bcurve, _ = field(group)
    nc = group
    assert len(b) == point_bytes(group, enc)
    if checks & CHECK_SUBGROUP or enc == ENC_COMPRESSED:
        checks |= CHECK_CURVE
    if enc == ENC_WIRE:
        if b == bytes(len(b)):
            return OK
        v = [int.from_bytes(b[48 * i : 48 * i + 48], "little") for i in range(2 * nc)]
        if any(c >= P for c in v):
            return BAD_ENCODING
        pt = (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))
    else:
        compressed = enc == ENC_COMPRESSED
        if bool(b[0] & 0x80) != compressed:
            return BAD_ENCODING
        if b[0] & 0x40:
            return OK if b == bytes([0xC0 if compressed else 0x40]) + bytes(len(b) - 1) else BAD_ENCODING
        if not compressed and b[0] & 0x20:
            return BAD_ENCODING
        body = bytes([b[0] & 0x1F]) + b[1:] if compressed else b
        v = [int.from_bytes(body[48 * i : 48 * i + 48], "big") for i in range(len(b) // 48)]
        if any(c >= P for c in v):
            return BAD_ENCODING
        if compressed:
            try:
                pt = ec.g1_decompress(b) if group == 1 else ec.g2_decompress(b)
            except ValueError:
                return NOT_ON_CURVE
        else:
            pt = (v[0], v[1]) if group == 1 else ((v[1], v[0]), (v[3], v[2]))
    if checks & CHECK_CURVE and not ec.on_curve(F, bcurve, pt):
        return NOT_ON_CURVE
    if checks & CHECK_SUBGROUP and ec.pt_mul(F, pt, R) is not None:
        return NOT_IN_SUBGROUP
    return OK


def class_status(cls, enc, checks):
    """The status an element gets by the class it was built as."""
    if checks & CHECK_SUBGROUP or enc == ENC_COMPRESSED:
        checks |= CHECK_CURVE
    if cls == "valid":
        return OK
    if cls in ("bad_flags", "noncanon_inf", "x_ge_p"):
        return BAD_ENCODING
    if cls == "no_root":
        return NOT_ON_CURVE if checks & CHECK_CURVE else OK
    assert cls == "off_subgroup" or cls.startswith(("order_", "mixed_")), cls
    return NOT_IN_SUBGROUP if checks & CHECK_SUBGROUP else OK


# ---- the corpus -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logical(group, seed=2024):
    """[(class, payload)]: points for the point classes, a recipe for the encoding faults (made per encoding)."""
    rnd = random.Random(seed * 10 + group)
    F, _, _ = field(group)
    m = MIN_MEMBERS[group]
    gen = ec.G1 if group == 1 else ec.G2
    items = []
    base = ec.pt_mul(F, gen, rnd.randrange(1, R))
    stepq = ec.pt_mul(F, gen, rnd.randrange(1, R))
    for i in range(m + 8):
        items.append(("valid", None if i % 9 == 4 else base))
        base = ec.pt_add(F, base, stepq)
    for i in range(m):
        items.append(("bad_flags", (i, ec.pt_mul(F, gen, i + 2))))
        items.append(("noncanon_inf", (i, rnd.randrange(1, 1 << 64))))
        items.append(("x_ge_p", (i, random_curve_point(group, rnd), rnd.randrange(0, 1 << 40))))
        items.append(("no_root", (x_without_root(group, rnd), _rand_fe(group, rnd), rnd.getrandbits(1))))
        items.append(("off_subgroup", random_curve_point(group, rnd)))
    for q, e in SMALL_ORDERS[group]:
        ts = [small_order_point(group, q, e, rnd) for _ in range(4)]
        for i in range(m):
            t = ts[i % 4]
            items.append(("order_%d" % q, ec.pt_mul(F, t, 1 + i % (q - 1))))
            items.append(("mixed_%d" % q, ec.pt_add(F, ec.pt_mul(F, gen, rnd.randrange(1, R)), t)))
    rnd.shuffle(items)
    return tuple(items)


def _fault(group, enc, cls, payload):
    """Bytes of an encoding-fault element, or None when the class does not exist in `enc`."""
    nc = group
    w = point_bytes(group, enc)
    if cls == "bad_flags":
        i, pt = payload
        if enc == ENC_WIRE:
            return None
        b = bytearray(encode(group, enc, pt))
        if enc == ENC_COMPRESSED:
            b[0] &= 0x7F  # a compressed element must say so
        elif i % 2:
            b[0] |= 0x80  # an uncompressed one must not
        else:
            b[0] |= 0x20  # and has no sort bit
        return bytes(b)
    if cls == "noncanon_inf":
        i, junk = payload
        if enc == ENC_WIRE:
            return None
        b = bytearray(w)
        b[0] = 0xC0 if enc == ENC_COMPRESSED else 0x40
        if i % 3 == 0:
            b[0] |= 0x20  # sort flag on infinity
        elif i % 3 == 1:
            b[1 + junk % (w - 1)] = 1 + junk % 255
        else:
            b[0] |= 1 + junk % 31  # coordinate bits in the flag byte
        return bytes(b)
    if cls == "x_ge_p":
        i, pt, k = payload
        xs, ys = _comps(group, pt[0]), _comps(group, pt[1])
        # which coordinate component is left unreduced; the compressed form only has x.  The top component of the
        # big-endian forms shares its byte with the flags, so there the excess stays below 2^381
        slots = nc if enc == ENC_COMPRESSED else 2 * nc
        s = i % slots
        top_of_be = enc != ENC_WIRE and s == nc - 1
        big = P + k if (top_of_be or i % 4 == 0) else (1 << 384) - 1 - k
        if s < nc:
            xs[s] = big
        else:
            ys[s - nc] = big
        flags = 0 if enc != ENC_COMPRESSED else 0x80 | (0x20 if i % 2 else 0)
        return _raw(group, enc, xs, ys, flags)
    if cls == "no_root":
        x, y, sort = payload
        flags = 0 if enc != ENC_COMPRESSED else 0x80 | (0x20 if sort else 0)
        return _raw(group, enc, _comps(group, x), _comps(group, y), flags)
    raise AssertionError(cls)


@functools.lru_cache(maxsize=None)
def corpus(group, enc, seed=2024):
    """[(class, element bytes)] in one encoding, in the shuffled order of logical()."""
    out = []
    for cls, payload in logical(group, seed):
        if cls in ("bad_flags", "noncanon_inf", "x_ge_p", "no_root"):
            b = _fault(group, enc, cls, payload)
            if b is None:
                continue
        else:
            b = encode(group, enc, payload)
        out.append((cls, b))
    return tuple(out)


def expected_classes(group, enc):
    cls = {"valid", "x_ge_p", "no_root", "off_subgroup"}
    if enc != ENC_WIRE:
        cls |= {"bad_flags", "noncanon_inf"}
    for q, _ in SMALL_ORDERS[group]:
        cls |= {"order_%d" % q, "mixed_%d" % q}
    return cls
