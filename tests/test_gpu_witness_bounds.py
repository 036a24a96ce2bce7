"""The prover's witness map at the ends of what its limbs can hold: the mat-vec kernels store UNREDUCED row
sums, the first inverse transform adds them up without reducing, and the signed 32-bit top limb is what bounds the result.
tests/witness28.py is the big-integer model: which inputs are legal, and how large every class of value may become.

Part 1: the decimation-in-frequency transform on RAW limbs (zkmi_selftest_ntt_dif_raw_dev), fed constant and alternating
        vectors whose representation x = c + K r the model puts just inside capacity.
Part 2: the three mat-vec forms on one crafted relation, raw limbs out, with and without normalisation.
Part 3: the largest |top limb| behind every stage of the map, measured on four keys, against the model's bound.
Part 4: proofs and h words with normalisation forced on equal the C++ oracle's bytes.
Every operand is one the model calls legal: nothing here is meant to wrap."""
import ctypes as C
import random

import numpy as np
import pytest

import limbs28 as lb
import witness28 as wm
from oracle import bls12_381 as ec
from oracle.bls12_381 import R

pytestmark = pytest.mark.gpu
NTT_FIELDS = [(lb.FIELDS[1], wm.FR), (lb.FIELDS[3], wm.BN_FR)]
NTT_IDS = [f.name for f, _ in NTT_FIELDS]


def frs(vals):
    return b"".join(ec.fr_to_bytes(v) for v in vals)


# ---- part 1: the raw DIF at capacity -------------------------------------------------------------------------------------
def _raw_tensor(torch, f, pattern, n):
    """n raw elements repeating `pattern` (1 or 2 integers), built on the device from its 40 or 80 bytes."""
    w = lb.limbs_array(list(pattern), f.NL).reshape(-1)
    return torch.from_numpy(w).cuda().repeat(n // len(pattern)).view(n, f.NL).contiguous()


def _ints(t, rows):
    return lb.ints_of(t[rows].cpu().numpy())


def _input_bound(mf, log_n):
    """The largest per-element bound h (half moduli) of a uniform input whose transform the model lets through, and the
    model's bound on the outputs (post 0)."""
    plan = wm.dif_plan(log_n, post=False)
    first = plan[0][0] if len(plan) == 2 else log_n  # stages that add before anything multiplies
    h = mf.capacity() >> first
    peak, out = wm.dif_bound_uniform(mf, plan, h)
    assert mf.fits(peak) and not mf.fits(wm.dif_bound_uniform(mf, plan, h + 1)[0])
    return h, out


def _vectors(f, h):
    """Constant and alternating patterns at +-h r / 2: (name, pattern, canonical c of the closed form's "const" or "alt")."""
    r = f.p
    c_hi, c_lo = lb.ntt_constants(f)[:2]  # the canonical c with the largest and the smallest library representation
    up = lambda v: v + (h * r // 2 - v) // r * r  # the largest representation of v's residue that is <= h r / 2
    down = lambda v: v - (h * r // 2 + v) // r * r  # the smallest that is >= -h r / 2
    out = [("const+", (up(f.rep(c_hi)),), c_hi), ("const-", (down(f.rep(c_lo)),), c_lo),
           # both entries at the top: position 0 holds N/2 (x + y), a non-zero multiple of r of full size
           ("alt++", (up(f.rep(c_hi)), up(f.rep(r - c_hi))), c_hi),
           # the entries at opposite ends: the last stage's lazy difference x - y is the value of full size
           ("alt+-", (up(f.rep(c_hi)), down(f.rep(r - c_hi))), c_hi)]
    for _, pat, _ in out:
        assert all(h * r - 2 * r < 2 * abs(v) <= h * r for v in pat)
    return out


@pytest.mark.parametrize("log_n", [20, 21, 22])
@pytest.mark.parametrize("f,mf", NTT_FIELDS, ids=NTT_IDS)
def test_raw_dif_at_capacity(zk, ctx, f, mf, log_n):
    """2^21 and 2^22 run three passes and multiply nothing on the sum path: with post 0 position 0 must hold the exact INTEGER
    sum of the inputs, N x -- just inside 2^31 2^252.  2^20 runs two passes: the inputs sit at the capacity of one stride class
    of the first pass (2^10 of them add up) and the twist must bring every element back.  Residues at position 0, 1 and 16
    further positions against the closed forms of tests/limbs28.py; magnitudes against the model's output bound."""
    import torch

    n, r = 1 << log_n, f.p
    h, out_bound = _input_bound(mf, log_n)
    three_pass = len(wm.plan_stages(log_n)) >= 3
    rng = lb.SplitMix64(0xD1F + log_n)
    rows = [0, 1, 2, n // 2, n - 1] + [rng.below(n) for _ in range(13)]
    for name, pat, c in _vectors(f, h):
        kind = "const" if name.startswith("const") else "alt"
        for post in (0, 1):
            t = _raw_tensor(torch, f, pat, n)
            rc = zk.tlib.zkmi_selftest_ntt_dif_raw_dev(ctx.h, C.c_int32(f.id), C.c_void_p(t.data_ptr()), C.c_uint32(log_n), C.c_int32(post))
            assert rc == 0, (name, post, rc)
            got = _ints(t, rows)
            want = lb.ntt_closed_form(f, "%s_dif%d" % (kind, post), log_n, c)
            for p, v in zip(rows, got):
                assert f.value(v) == want.get(p, 0), (f.name, log_n, name, post, p)
            low = t[:, : f.NL - 1]
            assert bool(((low >= 0) & (low <= lb.MASK)).all()), "limbs not normalised"
            if post == 0 and three_pass:
                assert got[0] == (n // len(pat)) * sum(pat), (f.name, log_n, name)
                if kind == "const":  # and that sum IS at capacity: within three vectors' worth of r
                    assert (mf.capacity() - 3 * n) * r < 2 * abs(got[0]) <= mf.capacity() * r
            bound = wm.top_limb_bound(mf, out_bound if post == 0 else mf.prod(out_bound, wm.PROD))
            assert int(t[:, f.NL - 1].abs().max().item()) <= bound, (f.name, log_n, name, post)
            del t


# ---- part 2: the mat-vec forms -------------------------------------------------------------------------------------------
ROW_TERMS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 5000)  # both sides of the 8-lane split and of MATVEC_LONG_ROW


def _crafted_relation(zk, seed=0x3A7):
    """log_n = 10: 600 rows; A's first rows have ROW_TERMS terms, B's the same lengths in reverse order, the others 0 .. 12;
    C_i is one product variable.  0, 1 and r - 1 are frequent among the coefficients and the assignment."""
    rnd = random.Random(seed)
    n_pub, n_free, n_rows = 3, 6000, 600
    special = [0, 1, R - 1]
    pick = lambda: rnd.choice(special) if rnd.random() < 0.3 else rnd.randrange(R)
    vals = [1] + [pick() for _ in range(n_pub - 1 + n_free)]
    n_in = len(vals)
    rows = []
    for i in range(n_rows):
        ka = ROW_TERMS[i] if i < len(ROW_TERMS) else rnd.randrange(13)
        kb = ROW_TERMS[len(ROW_TERMS) - 1 - i] if i < len(ROW_TERMS) else rnd.randrange(13)
        lc = lambda k: (sorted(rnd.sample(range(n_in), k)), [pick() for _ in range(k)])
        (ac, av), (bc, bv) = lc(ka), lc(kb)
        a = sum(v * vals[c] for c, v in zip(ac, av)) % R
        b = sum(v * vals[c] for c, v in zip(bc, bv)) % R
        rows.append((ac, av, bc, bv))
        vals.append(a * b % R)
    mats = []
    for which in range(3):
        rp, cl, vl = [0], [], []
        for i, (ac, av, bc, bv) in enumerate(rows):
            cols, cv = ((ac, av), (bc, bv), ([n_in + i], [1]))[which]
            cl += cols
            vl += cv
            rp.append(len(cl))
        mats.append((rp, cl, vl))
    r1 = zk.r1cs_create(len(vals), n_pub, [(rp, cl, frs(vl)) for rp, cl, vl in mats])
    assert r1.log_n == 10 and r1.is_satisfied(frs(vals))
    return r1, mats, vals


def _toxic(seed):
    rng = ec.SplitMix64(seed)
    return frs([rng.fr() for _ in range(5)])


def _normalise(zk, pk, force=-1):
    mask = C.c_uint32(0xFF)
    assert zk.tlib.zkmi_selftest_pk_normalise(pk.h, C.c_int32(force), C.byref(mask)) == 0
    return mask.value


def test_matvec_forms_raw_rows(zk, ctx):
    """k_matvec<1>, k_matvec<8> and k_matvec_long (rows of 1 025 and 5 000 terms) store the raw sum of k products: every row's
    residue against Python, its magnitude against the model's 3/2 k r, an empty row exactly 0; with normalisation forced on,
    every row inside (-r/2, 3r/2)."""
    import torch

    f = lb.FIELDS[1]
    r1, mats, vals = _crafted_relation(zk)
    pk, _ = ctx.groth16_setup(r1, _toxic(0x3A70))
    n, nc, n_pub = 1 << r1.log_n, r1.n_constraints, r1.n_pub
    assert _normalise(zk, pk) == 0  # the shape is far inside capacity: the key normalises nothing by itself
    want = []
    for rp, cl, vl in mats:
        want.append([sum(vl[k] * vals[cl[k]] for k in range(rp[i], rp[i + 1])) % R for i in range(nc)] + [0] * (n - nc))
    want[0][nc : nc + n_pub] = vals[:n_pub]
    terms = [[rp[i + 1] - rp[i] for i in range(nc)] for rp, _, _ in mats]
    d = torch.frombuffer(bytearray(frs(vals)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    raw = {}
    for mask in (0, 7):
        assert _normalise(zk, pk, mask) == mask
        model = wm.WitnessModel(r1.log_n, n_pub, terms, normalise=mask)
        for form in (0, 1):
            out = np.zeros((3 * n, f.NL), dtype=np.int32)
            rc = zk.tlib.zkmi_selftest_matvec_dev(ctx.h, pk.h, C.c_void_p(d.data_ptr()), C.c_int32(form), out.ctypes.data_as(C.c_void_p))
            assert rc == 0, (mask, form, rc)
            assert lb.rows_normalised(out)
            got = lb.ints_of(out)
            for m in range(3):
                for i in range(n):
                    v = got[m * n + i]
                    assert f.value(v) == want[m][i], (mask, form, m, i)
                    assert 2 * abs(v) <= int(model.rows[m][i]) * R, (mask, form, m, i, v // R)
                    if mask:
                        assert -R < 2 * v < 3 * R, (form, m, i)
                    if model.rows[m][i] == 0:
                        assert v == 0
            raw[(mask, form)] = got
    # the unnormalised sums really are sums: a row of 5 000 terms is far outside (-r/2, 3r/2) -- what the flag is for
    long_row = ROW_TERMS.index(5000)
    assert abs(raw[(0, 0)][long_row]) > 100 * R and abs(raw[(0, 1)][long_row]) > 100 * R
    _normalise(zk, pk, 0)
    pk.free()
    r1.free()


# ---- part 3: measured maxima against the model -----------------------------------------------------------------------------
def _stages(zk, ctx, pk, d):
    out = (C.c_uint32 * 18)()
    rc = zk.tlib.zkmi_selftest_witness_map_stages(ctx.h, pk.h, C.c_void_p(d.data_ptr()), out)
    assert rc == 0, rc
    return [list(out[3 * s : 3 * s + 3]) for s in range(6)]


def _row_terms(zk, r1):
    """Row lengths of A, B, C from the library's own copy of the relation (row pointers only: no columns, no values)."""
    out = []
    for m in range(3):
        rp = np.zeros(r1.n_constraints + 1, dtype=np.uint32)
        assert zk.lib.zkmi_r1cs_export(r1.h, C.c_int32(m), rp.ctypes.data_as(C.c_void_p), None, None, None) == 0
        out.append(np.diff(rp.astype(np.int64)))
    return out


def _check_stages(zk, ctx, name, r1, pk, wit, row_terms):
    import torch

    f = wm.FR
    mask = _normalise(zk, pk)
    model = wm.WitnessModel(r1.log_n, r1.n_pub, row_terms, normalise=mask)
    # every bound fits the limbs, or the key carries the flag for the matrix that does not
    unflagged = wm.WitnessModel(r1.log_n, r1.n_pub, row_terms, normalise=0)
    assert unflagged.exceeds() & ~mask == 0, (name, unflagged.exceeds(), mask)
    assert model.exceeds() == 0 and all(f.fits(b) for b in model.all_bounds().values()), name
    assert model.is_zero_operand <= 8  # is_zero() is exact up to 4 r
    d = torch.frombuffer(bytearray(wit), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = _stages(zk, ctx, pk, d)
    bounds = model.stage_bounds()
    line = []
    for s, stage in enumerate(wm.STAGES):
        for m in range(3):
            limit = wm.top_limb_bound(f, bounds[stage][m])
            assert got[s][m] <= limit, (name, stage, "abc"[m], got[s][m], limit)
        line.append("%s %s / %s" % (stage, max(got[s]), max(wm.top_limb_bound(f, b) for b in bounds[stage])))
    print("witness map %s, max |top limb| measured / bound: %s" % (name, "; ".join(line)))


def test_stage_maxima_update_note(zk, ctx):
    from test_cpu_host import _note_update_case

    lg = 13
    r1 = zk.update_note_r1cs(lg, 1)
    pk, _ = ctx.groth16_setup(r1, _toxic(0x57A6E))
    inp, _ = _note_update_case(zk, 99, 1, amount=33, balances=(5, 40), slot=1)
    wit, _, rc = zk.update_note_witness(lg, 1, inp)
    assert rc == 0
    terms = _row_terms(zk, r1)
    assert max(int(t.max()) for t in terms) > 60  # the Poseidon rows
    _check_stages(zk, ctx, "update_note 2^13", r1, pk, wit, terms)
    pk.free()
    r1.free()


def test_stage_maxima_crafted_relation(zk, ctx):
    r1, mats, vals = _crafted_relation(zk)
    pk, _ = ctx.groth16_setup(r1, _toxic(0x3A71))
    terms = [np.diff(np.array(rp, dtype=np.int64)) for rp, _, _ in mats]
    _check_stages(zk, ctx, "crafted rows 2^10", r1, pk, frs(vals), terms)
    assert _normalise(zk, pk, 7) == 7
    _check_stages(zk, ctx, "crafted rows 2^10, normalised", r1, pk, frs(vals), terms)
    pk.free()
    r1.free()


def test_stage_maxima_bits_relation(zk, ctx):
    """b_i b_i = b_i for 2^12 bits and one row that sums them all into the public input: a k_matvec_long row of 2^12 ones."""
    nbits, n_pub = 1 << 12, 2
    rnd = random.Random(12)
    bits = [1 if rnd.random() < 0.6 else 0 for _ in range(nbits)]
    zv = [1, sum(bits)] + bits
    cols = list(range(n_pub, n_pub + nbits))
    rp = list(range(nbits + 2))
    one = (1).to_bytes(32, "little")
    a = (rp[:-1] + [2 * nbits], cols + cols, one * (2 * nbits))  # last row: (b_0 + b_1 + ...) * 1 = z_1
    b = (rp, cols + [0], one * (nbits + 1))
    c = (rp, cols + [1], one * (nbits + 1))
    r1 = zk.r1cs_create(len(zv), n_pub, [a, b, c])
    wit = frs(zv)
    assert r1.log_n == 13 and r1.is_satisfied(wit)
    pk, _ = ctx.groth16_setup(r1, _toxic(0xB175))
    terms = [np.diff(np.array(m[0], dtype=np.int64)) for m in (a, b, c)]
    _check_stages(zk, ctx, "bits 2^13 with a row of 2^12 terms", r1, pk, wit, terms)
    pk.free()
    r1.free()


def test_stage_maxima_chain_relation_three_passes(zk, ctx):
    """The smallest three-pass plan: the whole vector is one coherent set."""
    lg = 21
    r1 = zk.shielder_r1cs(lg)
    pk, _ = ctx.groth16_setup(r1, _toxic(0xC4A1))
    wit = zk.shielder_witness(lg, 21)
    terms = _row_terms(zk, r1)
    _check_stages(zk, ctx, "chain 2^21", r1, pk, wit, terms)
    pk.free()
    r1.free()


# ---- part 4: bytes do not depend on the flag ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ocpp():
    from oracle import cpp

    cpp.build()
    return cpp


def test_proofs_with_normalisation_forced_vs_cpp_oracle(zk, ctx, ocpp):
    """The relations of test_random_relations_vs_cpp_oracle (same seeds, same generator): proof bytes with every matrix
    normalised equal the C++ oracle's, as they do without."""
    import torch

    for seed, n_free, n_rows, n_pub in ((1, 40, 200, 3), (2, 300, 900, 1), (3, 1700, 2300, 5)):
        rnd = random.Random(9000 + seed)
        special = [0, 1, R - 1, 2, R - 2]
        vals = [1] + [rnd.choice(special) if rnd.random() < 0.2 else rnd.randrange(R) for _ in range(n_pub - 1 + n_free)]
        n_in = len(vals)
        rows = []

        def lc(max_len):
            k = rnd.choice([0, 1, 1, 2, 3, 5, 8, max_len])
            cols = sorted(rnd.sample(range(n_in), min(k, n_in)))
            return cols, [rnd.choice([1, R - 1, 2]) if rnd.random() < 0.5 else rnd.randrange(1, R) for _ in cols]

        for i in range(n_rows):
            big = 1500 if (seed == 3 and i == 7) else (200 if i % 97 == 0 else 12)
            (ac, av), (bc, bv) = lc(big), lc(12)
            a = sum(v * vals[c] for c, v in zip(ac, av)) % R
            b = sum(v * vals[c] for c, v in zip(bc, bv)) % R
            rows.append((ac, av, bc, bv))
            vals.append(a * b % R)
        mats = []
        for which in range(3):
            rp, cl, vl = [0], [], b""
            for i, (ac, av, bc, bv) in enumerate(rows):
                cols, cv = ((ac, av), (bc, bv), ([n_in + i], [1]))[which]
                cl += cols
                vl += b"".join(v.to_bytes(32, "little") for v in cv)
                rp.append(len(cl))
            mats.append((rp, cl, vl))
        r1 = zk.r1cs_create(len(vals), n_pub, mats)
        wit = frs(vals)
        assert r1.is_satisfied(wit)
        rng = ec.SplitMix64(0xABCD00 + seed)
        toxic = frs([rng.fr() for _ in range(5)])
        ovk, okey = ocpp.groth16_setup(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, toxic)
        r_, s_ = ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr())
        want = ocpp.groth16_prove(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, okey, wit, r_, s_)
        d = torch.frombuffer(bytearray(wit), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        pk, vk = ctx.groth16_setup(r1, toxic)
        assert vk == ovk
        for mask in (7, 1, 0):
            assert _normalise(zk, pk, mask) == mask
            assert ctx.groth16_prove_dev(pk, d.data_ptr(), r_, s_) == want, (seed, mask)
        assert _normalise(zk, pk, 7) == 7  # and the grouped route, whose mat-vec is always the one-lane form
        assert ctx.groth16_prove_batch_dev(pk, [d.data_ptr()] * 3, [r_] * 3, [s_] * 3) == [want] * 3, seed
        pk.free()
        r1.free()


@pytest.mark.parametrize("lg", [4, 10, 12])
def test_witness_map_words_with_normalisation_forced_vs_cpp_oracle(zk, ctx, ocpp, lg):
    """The shapes of test_gpu_witness_map6.py: h words through zkmi_groth16_witness_map with every matrix normalised."""
    from test_gpu_witness_map6 import _relation

    rng = ec.SplitMix64(0x6E77 + lg)
    r1 = _relation(zk, lg, 1)[0]
    pk, _ = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    assert _normalise(zk, pk, 7) == 7
    mats = [r1.export(m) for m in range(3)]
    for seed in (61 + lg, 0xC0FFEE + lg):
        z = _relation(zk, lg, seed)[1]
        want = ocpp.witness_map(r1.n_vars, r1.n_pub, r1.n_constraints, lg, mats, z)
        assert ctx.groth16_witness_map(pk, z) == want, (lg, seed)
    pk.free()
    r1.free()
