"""GPU parity tests proper: HIP path (through the C ABI) vs the oracle, on the
committed golden fixtures and on seeded inputs.  Bit-exact (integer work)."""
import os

import pytest

from conftest import golden
from oracle import bls12_381 as ec
from oracle import groth16 as g16
from oracle import ntt as ont
from oracle.bls12_381 import R

pytestmark = pytest.mark.gpu

H = bytes.fromhex


def frs(vals):
    return b"".join(ec.fr_to_bytes(v) for v in vals)


def unfrs(b):
    return [int.from_bytes(b[i : i + 32], "little") for i in range(0, len(b), 32)]


def test_library_before_torch_shares_one_hip_runtime():
    """Import order must not matter: a fresh process that creates a zkmi context BEFORE importing torch still gets a
    working torch.cuda (the wheel bundles its own HIP runtime; binding.py makes both resolve to one copy), and
    the library can consume a torch allocation afterwards.  First GPU test of the file on purpose: this process
    does not hold a context yet."""
    import subprocess
    import sys

    from conftest import ROOT

    code = (
        "import faulthandler, sys; faulthandler.dump_traceback_later(150, exit=True)\n"
        "sys.path.insert(0, %r)\n"
        "from zkmi_loader import load_pkg\n"
        "z = load_pkg().Zkmi(); c = z.context(0)\n"
        "assert 'torch' not in sys.modules\n"
        "import torch\n"
        "t = torch.arange(64, dtype=torch.uint8, device='cuda'); torch.cuda.synchronize()\n"
        "d = torch.zeros(32 << 10, dtype=torch.uint8, device='cuda')\n"
        "d[0] = 1; torch.cuda.synchronize()\n"
        "c.ntt_dev(d.data_ptr(), 10); c.sync(); torch.cuda.synchronize()\n"
        "assert bytes(d[32:64].cpu().numpy()) == bytes(d[0:32].cpu().numpy())  # NTT of (1, 0, 0, ...) is all ones\n"
        "print('ok', int(t.sum()))\n"
    ) % ROOT
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=400)
    except subprocess.TimeoutExpired as e:
        # a hang in context creation is a defect of the product path, never a skip (the child dumps its Python
        # stacks after 150 s through faulthandler: they are in e.stderr)
        pytest.fail("child process did not finish in 400 s: %r" % ((e.stderr or b"")[-3000:],))
    assert r.returncode == 0 and "ok 2016" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- NTT (row a6)
@pytest.mark.parametrize("case", golden("ntt_small.json"), ids=lambda c: f"log{c['log_n']}")
def test_ntt_golden(ctx, case):
    lg = case["log_n"]
    x = H(case["input"])
    assert ctx.ntt(x, lg) == H(case["forward"])
    assert ctx.ntt(x, lg, inverse=True) == H(case["inverse"])
    assert ctx.ntt(x, lg, coset=True) == H(case["coset_forward"])
    assert ctx.ntt(x, lg, inverse=True, coset=True) == H(case["coset_inverse"])


@pytest.mark.parametrize("lg", [4, 9, 11, 12, 13, 14])
def test_ntt_vs_oracle_seeded(ctx, lg):
    rng = ec.SplitMix64(1000 + lg)
    a = [rng.fr() for _ in range(1 << lg)]
    assert unfrs(ctx.ntt(frs(a), lg)) == ont.ntt(a)
    assert unfrs(ctx.ntt(frs(a), lg, inverse=True, coset=True)) == ont.coset_intt(a)


def test_ntt_rejects_non_canonical(ctx, pkg):
    bad = (R).to_bytes(32, "little") + bytes(32)
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.ntt(bad, 1)
    assert e.value.code == -2


@pytest.mark.parametrize("lg", [16, 20])
def test_ntt_large_properties(ctx, lg):
    """Full-size checks through size-independent properties: round trip, coset
    round trip, linearity, and the transform of a delta / constant."""
    n = 1 << lg
    rng = ec.SplitMix64(77 + lg)
    # cheap pseudo-random canonical input: 31 random bytes per element
    import random

    rnd = random.Random(lg)
    a = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        a[i] &= 0x3F
    a = bytes(a)
    fwd = ctx.ntt(a, lg)
    assert ctx.ntt(fwd, lg, inverse=True) == a
    cf = ctx.ntt(a, lg, coset=True)
    assert ctx.ntt(cf, lg, inverse=True, coset=True) == a
    # delta at position 1 -> powers of w
    d = bytearray(32 * n)
    d[32] = 1
    wpow = unfrs(ctx.ntt(bytes(d), lg))
    w = ont.root_of_unity(lg)
    for k in (0, 1, 2, 3, n // 2, n - 1, 12345 % n):
        assert wpow[k] == pow(w, k, R)
    # sum of outputs == n * a[0]
    s = sum(unfrs(fwd)) % R
    assert s == n * int.from_bytes(a[:32], "little") % R
    # out[0] == sum of inputs
    assert int.from_bytes(fwd[:32], "little") == sum(unfrs(a)) % R


# ---------------------------------------------------------- MSM (rows a8, a9)
@pytest.mark.parametrize("case", golden("msm_small.json"), ids=lambda c: c["name"])
def test_msm_golden(ctx, case):
    sc, bs = H(case["scalars"]), H(case["bases"])
    if case["group"] == 1:
        b = ctx.bases_g1(bs)
        assert ctx.msm_g1(sc, b) == H(case["expected"])
    else:
        b = ctx.bases_g2(bs)
        assert ctx.msm_g2(sc, b) == H(case["expected"])
    b.free()


def test_msm_empty(ctx):
    b = ctx.bases_g1(ec.g1_to_bytes(ec.G1))
    assert ctx.msm_g1(b"", b) == bytes(96)
    b.free()


def test_synthetic_bases_match_recipe(ctx):
    c = golden("constants.json")
    b = ctx.bases_g1_synthetic(2000)
    assert [b.read(i, 1).hex() for i in range(4)] == c["synthetic_g1_first4"]
    assert b.read(1000, 1).hex() == c["synthetic_g1_index_1000"]
    b.free()
    b2 = ctx.bases_g2_synthetic(130)
    assert [b2.read(i, 1).hex() for i in range(4)] == c["synthetic_g2_first4"]
    p129 = ec.pt_add(ec.Fq2, ec.G2, ec.g2_mul(129 * 0xC0FFEE))
    assert b2.read(129, 1) == ec.g2_to_bytes(p129)
    b2.free()


@pytest.mark.parametrize("n", [300, 3000, 20000])
def test_msm_g1_structured_vs_closed_form(ctx, n):
    """With P_i = G + i*Q the MSM has a closed form:
    sum s_i P_i = (sum s_i) G + (sum i*s_i) Q — checks every plan size."""
    rng = ec.SplitMix64(n)
    s = [rng.fr() for _ in range(n)]
    b = ctx.bases_g1_synthetic(n)
    got = ctx.msm_g1(frs(s), b)
    q = ec.g1_mul(0xC0FFEE)
    exp = ec.pt_add(ec.Fq, ec.g1_mul(sum(s) % R), ec.g1_mul(sum(i * v for i, v in enumerate(s)) % R, q))
    assert got == ec.g1_to_bytes(exp)
    b.free()


@pytest.mark.parametrize("n", [5000, 70000])
def test_msm_g1_witness_like_heavy_buckets(ctx, n):
    """Witness-like scalars: 40 % zero, 20 % one, 10 % < 2^16,
    one value repeated in 10 %, rest uniform — drives single buckets far above
    the mean load (the workgroup-per-heavy-bucket path)."""
    rng = ec.SplitMix64(31 * n)
    rep = rng.fr()
    s = []
    for _ in range(n):
        t = rng.next() % 10
        s.append(0 if t < 4 else 1 if t < 6 else (rng.next() & 0xFFFF) if t < 7 else rep if t < 8 else rng.fr())
    b = ctx.bases_g1_synthetic(n)
    got = ctx.msm_g1(frs(s), b)
    q = ec.g1_mul(0xC0FFEE)
    exp = ec.pt_add(ec.Fq, ec.g1_mul(sum(s) % R), ec.g1_mul(sum(i * v for i, v in enumerate(s)) % R, q))
    assert got == ec.g1_to_bytes(exp)
    b.free()


def test_msm_g1_all_scalars_equal(ctx):
    """Every point lands in the same bucket of every window."""
    n = 4096
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF
    b = ctx.bases_g1_synthetic(n)
    got = ctx.msm_g1(ec.fr_to_bytes(k) * n, b)
    q = ec.g1_mul(0xC0FFEE)
    exp = ec.pt_add(ec.Fq, ec.g1_mul(n * k % R), ec.g1_mul(k * (n * (n - 1) // 2) % R, q))
    assert got == ec.g1_to_bytes(exp)
    b.free()


@pytest.mark.parametrize("n", [3000, 40000])
def test_msm_g2_witness_like_heavy_buckets(ctx, n):
    """The G2 twin of test_msm_g1_witness_like_heavy_buckets: buckets of thousands of points go through the lane-pair
    heavy-bucket kernel, the biggest ones split over several workgroups whose last one adds the partials."""
    rng = ec.SplitMix64(37 * n)
    rep = rng.fr()
    s = []
    for _ in range(n):
        t = rng.next() % 10
        s.append(0 if t < 4 else 1 if t < 6 else (rng.next() & 0xFFFF) if t < 7 else rep if t < 8 else rng.fr())
    b = ctx.bases_g2_synthetic(n)
    q = ec.g2_mul(0xC0FFEE)
    exp = ec.pt_add(ec.Fq2, ec.g2_mul(sum(s) % R), ec.g2_mul(sum(i * v for i, v in enumerate(s)) % R, q))
    for _ in range(2):  # the second run finds the tickets of the first one reset
        assert ctx.msm_g2(frs(s), b) == ec.g2_to_bytes(exp)
    b.free()


@pytest.mark.parametrize("n", [300, 5000])
def test_msm_g2_structured_vs_closed_form(ctx, n):
    rng = ec.SplitMix64(7 * n)
    s = [rng.fr() for _ in range(n)]
    b = ctx.bases_g2_synthetic(n)
    got = ctx.msm_g2(frs(s), b)
    q = ec.g2_mul(0xC0FFEE)
    exp = ec.pt_add(ec.Fq2, ec.g2_mul(sum(s) % R), ec.g2_mul(sum(i * v for i, v in enumerate(s)) % R, q))
    assert got == ec.g2_to_bytes(exp)
    b.free()


def test_msm_g1_full_size_closed_form(ctx):
    """BASELINE config 1 size (2^20) through the closed form above."""
    import random

    n = 1 << 20
    rnd = random.Random(5)
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    s = unfrs(bytes(raw))
    b = ctx.bases_g1_synthetic(n)
    got = ctx.msm_g1(bytes(raw), b)
    q = ec.g1_mul(0xC0FFEE)
    exp = ec.pt_add(ec.Fq, ec.g1_mul(sum(s) % R), ec.g1_mul(sum(i * v for i, v in enumerate(s)) % R, q))
    assert got == ec.g1_to_bytes(exp)
    b.free()


# ------------------------------------------------- Groth16 (rows a7, a10, a11)
def test_groth16_golden_n128(ctx, zk):
    gd = golden("groth16_n128.json")
    r1 = zk.shielder_r1cs(gd["log_n"])
    z = zk.shielder_witness(gd["log_n"], gd["witness_seed"])
    assert z == H(gd["witness"])
    pk, vk = ctx.groth16_setup(r1, H(gd["toxic"]))
    assert vk == H(gd["vk"])
    for which, name in ((0, "a_query"), (1, "b_g1_query"), (2, "b_g2_query"), (3, "h_query"), (4, "l_query")):
        exp = H(gd["pk"][name])
        w = 192 if which == 2 else 96
        assert pk.export_query(which, 0, len(exp) // w) == exp, name
    assert ctx.groth16_witness_map(pk, z) == H(gd["h"])
    proof = ctx.groth16_prove(pk, z, H(gd["r"]), H(gd["s"]))
    assert proof == H(gd["proof"])
    publics = z[32 : 32 * r1.n_pub]
    assert zk.groth16_verify(vk, publics, proof) is True
    bad = bytearray(publics)
    bad[0] ^= 1
    assert zk.groth16_verify(vk, bytes(bad), proof) is False
    # key loaded from wire arrays gives the same proof (drop-in key format)
    p = gd["pk"]
    pk2 = ctx.pk_load(r1, H(p["alpha_g1"]), H(p["beta_g1"]), H(p["beta_g2"]), H(p["delta_g1"]), H(p["delta_g2"]),
                      H(p["a_query"]), H(p["b_g1_query"]), H(p["b_g2_query"]), H(p["h_query"]), H(p["l_query"]))
    assert ctx.groth16_prove(pk2, z, H(gd["r"]), H(gd["s"])) == H(gd["proof"])
    pk.free()
    pk2.free()


@pytest.mark.parametrize("lg", [10, 14])
def test_groth16_self_verifies(ctx, zk, lg):
    """BASELINE config 0 size (2^14): proof must pass the pairing verifier."""
    r1 = zk.shielder_r1cs(lg)
    z = zk.shielder_witness(lg, 0x5A4B0000 + lg)
    assert r1.is_satisfied(z)
    rng = ec.SplitMix64(lg)
    toxic = frs([rng.fr() for _ in range(5)])
    pk, vk = ctx.groth16_setup(r1, toxic)
    proof = ctx.groth16_prove(pk, z, ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr()))
    assert zk.groth16_verify(vk, z[32 : 32 * r1.n_pub], proof) is True
    pk.free()


def test_groth16_batch_matches_single(ctx, zk):
    """Pipelined batch (two proofs in flight) returns the same bytes as one-at-a-time proving."""
    import torch

    lg = 12
    r1 = zk.shielder_r1cs(lg)
    rng = ec.SplitMix64(99)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    wits = [zk.shielder_witness(lg, 500 + i) for i in range(5)]
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(5)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(5)]
    single = [ctx.groth16_prove(pk, w, r, s) for w, r, s in zip(wits, rs, ss)]
    d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
    torch.cuda.synchronize()
    batch = ctx.groth16_prove_batch_dev(pk, [t.data_ptr() for t in d], rs, ss)
    assert batch == single
    for w, pf in zip(wits, batch):
        assert zk.groth16_verify(vk, w[32 : 32 * r1.n_pub], pf) is True
    pk.free()


def _torch_scalars(n, seed):
    """n canonical scalars (< 2^254) generated in HBM + the two sums the closed form needs."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= 0x3F
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    s0 = raw.to(torch.int64).sum(dim=0).cpu().tolist()
    s1 = (raw.to(torch.int64) * idx[:, None]).sum(dim=0).cpu().tolist()
    tot = sum(v << (8 * k) for k, v in enumerate(s0)) % R
    wtot = sum(v << (8 * k) for k, v in enumerate(s1)) % R
    return raw, tot, wtot


def _closed_form_g1(tot, wtot):
    q = ec.g1_mul(0xC0FFEE)
    return ec.g1_to_bytes(ec.pt_add(ec.Fq, ec.g1_mul(tot), ec.g1_mul(wtot, q)))


@pytest.mark.gpu
def test_msm_g1_two_level_sort_of_16_bit_windows(ctx):
    """16-bit windows from 2^21 terms on are sorted like the big plans (msm_sort.hip run_windowed_big with one group per
    window: records -> fine partitions -> one workgroup per partition, oversized partitions by 64 workgroups).  An odd
    size just above 2^21, uniform scalars and the witness-like mix (a fifth of the scalars equal to one: 420 000 records
    in one bucket -- the k_big_* kernels), each against the closed form over the synthetic bases."""
    import torch

    n = (1 << 21) + 4097
    raw, tot, wtot = _torch_scalars(n, 2121)
    b = ctx.bases_g1_synthetic(n)
    assert ctx.msm_g1_dev(raw.data_ptr(), n, b) == _closed_form_g1(tot, wtot)
    g = torch.Generator(device="cuda").manual_seed(2122)
    kind = torch.rand(n, device="cuda", generator=g)
    raw[kind < 0.6] = 0
    raw[(kind >= 0.4) & (kind < 0.6), 0] = 1
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    s0 = raw.to(torch.int64).sum(dim=0).cpu().tolist()
    s1 = (raw.to(torch.int64) * idx[:, None]).sum(dim=0).cpu().tolist()
    tot = sum(v << (8 * k) for k, v in enumerate(s0)) % R
    wtot = sum(v << (8 * k) for k, v in enumerate(s1)) % R
    torch.cuda.synchronize()
    assert ctx.msm_g1_dev(raw.data_ptr(), n, b) == _closed_form_g1(tot, wtot)
    b.free()
    del raw, kind, idx
    torch.cuda.empty_cache()


def test_msm_g1_point_split_matches_full(ctx, zk):
    """BASELINE config 3 logic on one GPU: two point-slices -> per-window partials ->
    zkmi_msm_g1_combine == the unsplit MSM == the closed form."""
    import torch

    n = 1 << 18
    raw, tot, wtot = _torch_scalars(n, 11)
    b = ctx.bases_g1_synthetic(n)
    full = ctx.msm_g1_dev(raw.data_ptr(), n, b)
    assert full == _closed_form_g1(tot, wtot)
    half = n // 2
    lo = ctx.bases_g1(b.read(0, half), check=False)
    hi = ctx.bases_g1(b.read(half, half), check=False)
    w0, nwin, cb = ctx.msm_g1_windows_dev(raw.data_ptr(), half, lo, n)
    w1, nwin1, cb1 = ctx.msm_g1_windows_dev(raw[half:].data_ptr(), half, hi, n)
    assert (nwin, cb) == (nwin1, cb1)
    assert zk.msm_g1_combine(w0 + w1, 2, nwin, cb) == full
    for x in (b, lo, hi):
        x.free()


def test_msm_g1_big_window_plan_on_small_slices(ctx, zk):
    """The windowed schedule of >= 2^24 terms uses 20-bit windows, each sorted as 16 partitions of 2^15 buckets
    (MsmSort::run_windowed_big).  A rank of a point-split MSM runs that plan on its slice whatever the slice's size: here
    two slices of 2^17 terms under the plan of a 2^24-term MSM -- uniform scalars (every bucket nearly empty), the
    witness-like mix (one bucket holds 20 % of the points: the cooperative kernel), and scalars drawn from 600 values
    (7 800 buckets above the heavy threshold: the wide tail launch of the cooperative kernel) -- must combine to the
    result of the 16-bit plan, which is compared with the C++ oracle."""
    import torch

    from oracle import cpp as ocpp

    assert zk.msm_plan_query(1 << 24)[0] == 20 and zk.msm_plan_query((1 << 24) - 1)[0] == 16
    n = 1 << 18
    half = n // 2
    b = ctx.bases_g1_synthetic(n)
    pts = b.read(0, n)
    lo = ctx.bases_g1(pts[: 96 * half], check=False)
    hi = ctx.bases_g1(pts[96 * half :], check=False)
    g = torch.Generator().manual_seed(77)
    uni = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    uni[:, 31] &= 0x3F
    mix = uni.clone()
    kind = torch.rand(n, generator=g)
    mix[kind < 0.4] = 0
    one = (kind >= 0.4) & (kind < 0.6)
    mix[one] = 0
    mix[one, 0] = 1
    few = uni[:600][torch.randint(0, 600, (n,), generator=g)]
    for name, sc in (("uniform", uni), ("witness-like", mix), ("600 values", few)):
        d = sc.contiguous().cuda()
        torch.cuda.synchronize()
        full = ctx.msm_g1_dev(d.data_ptr(), n, b)
        assert full == ocpp.msm_g1(sc.numpy().tobytes(), pts), name
        w0, nwin, cb = ctx.msm_g1_windows_dev(d.data_ptr(), half, lo, 1 << 24)
        w1, nwin1, cb1 = ctx.msm_g1_windows_dev(d[half:].data_ptr(), half, hi, 1 << 24)
        assert (nwin, cb, nwin1, cb1) == (13, 20, 13, 20), name
        assert zk.msm_g1_combine(w0 + w1, 2, nwin, cb) == full, name
    for x in (b, lo, hi):
        x.free()


def test_msm_g1_multi_ctx_matches_full(ctx, zk):
    """zkmi_msm_g1_multi: one process, one ctx per slice (second ctx on GPU 1 when the box has one,
    otherwise a second ctx on GPU 0); uneven slices, result == unsplit MSM == closed form."""
    import torch

    n = (1 << 17) + 12345
    raw, tot, wtot = _torch_scalars(n, 12)
    b = ctx.bases_g1_synthetic(n)
    full = ctx.msm_g1_dev(raw.data_ptr(), n, b)
    assert full == _closed_form_g1(tot, wtot)
    dev1 = 1 if torch.cuda.device_count() > 1 else 0
    ctx1 = zk.context(dev1)
    cut = 50001
    lo = ctx.bases_g1(b.read(0, cut), check=False)
    hi = ctx1.bases_g1(b.read(cut, n - cut), check=False)
    raw_hi = raw[cut:].to("cuda:%d" % dev1).contiguous()
    torch.cuda.synchronize()
    got = zk.msm_g1_multi([ctx, ctx1], [raw.data_ptr(), raw_hi.data_ptr()], [cut, n - cut], [lo, hi])
    assert got == full
    # degenerate slices: one device holds everything, the other nothing
    got = zk.msm_g1_multi([ctx, ctx1], [raw.data_ptr(), 0], [cut, 0], [lo, hi])
    assert got == ctx.msm_g1_dev(raw.data_ptr(), cut, lo)
    for x in (b, lo, hi):
        x.free()
    ctx1.close()


def test_msm_g1_2p26_single_gpu(ctx):
    """BASELINE config 3 size (n = 2^26, 8 GiB of algorithmic bytes) on one GPU."""
    import torch

    n = 1 << 26
    raw, tot, wtot = _torch_scalars(n, 26)
    b = ctx.bases_g1_synthetic(n)
    got = ctx.msm_g1_dev(raw.data_ptr(), n, b)
    assert got == _closed_form_g1(tot, wtot)
    b.free()
    del raw
    torch.cuda.empty_cache()


def test_groth16_2p22_with_g2_and_pairing(ctx, zk):
    """BASELINE config 4: full proof at N = 2^22 (G2 MSM of 2^22 - 1 terms on the Fq2
    path), checked by the CPU pairing verifier."""
    lg = 22
    r1 = zk.shielder_r1cs(lg)
    z = zk.shielder_witness(lg, 0x5A4B0004)
    rng = ec.SplitMix64(0x5A4B0044)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    proof = ctx.groth16_prove(pk, z, ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr()))
    assert zk.groth16_verify(vk, z[32 : 32 * r1.n_pub], proof) is True
    # ... and by the oracle's own verifier on the decoded proof (Python big integers, polynomial-basis Fq12)
    vkd = {
        "alpha_g1": ec.g1_from_bytes(vk[:96]), "beta_g2": ec.g2_from_bytes(vk[96:288]), "gamma_g2": ec.g2_from_bytes(vk[288:480]),
        "delta_g2": ec.g2_from_bytes(vk[480:672]), "gamma_abc_g1": [ec.g1_from_bytes(vk[672 + 96 * i: 768 + 96 * i]) for i in range(r1.n_pub)],
    }
    assert g16.verify(vkd, unfrs(z[32: 32 * r1.n_pub]), g16.proof_from_bytes(proof))
    pk.free()


def test_mock_flow_with_real_proofs(ctx, zk, pkg):
    """The reference's wallet flow (drink_tests/mod.rs:11-68, utils/shielder.rs:43-134: create note ->
    deposit -> withdraw) through the ZkProof-shaped entry points with REAL proofs of the Poseidon
    relations: zkmi_shielder_prove_creation / _verify_creation (relations.rs:37-55, 127-136) and
    _prove_update / _verify_update (relations.rs:79-98, 138-155).  The note tree is a Poseidon Merkle tree
    built on the device; the values the prover returns equal the oracle's Poseidon hashes; the mock's error
    codes come back for impossible updates before any GPU work; tampered publics are rejected."""
    import torch
    from oracle import poseidon as ps

    lg_tree = 10
    rng = ec.SplitMix64(2024)
    fr = lambda: ec.fr_to_bytes(rng.fr())
    r1c = zk.create_note_r1cs(12)
    r1d, r1w = zk.update_note_r1cs(14, 0), zk.update_note_r1cs(14, 1)
    pkc, vkc = ctx.groth16_setup(r1c, frs([rng.fr() for _ in range(5)]))
    pkd, vkd = ctx.groth16_setup(r1d, frs([rng.fr() for _ in range(5)]))
    pkw, vkw = ctx.groth16_setup(r1w, frs([rng.fr() for _ in range(5)]))
    user = (1).to_bytes(16, "little") + bytes(16)
    token = bytes([228] * 32)  # MOCKED_TOKEN (mocked_zk/src/lib.rs:18): exceeds r, enters the relation mod r
    tokens = [token, bytes(32)]
    tok_fr = [int.from_bytes(zk.fr_reduce(t), "little") for t in tokens]
    ident, trap0, null0 = (7).to_bytes(32, "little"), (12).to_bytes(32, "little"), (11).to_bytes(32, "little")
    know = zk.zkproof_new(ident, trap0, null0, zk.op_priv(user), zk.account_new(tokens))

    # ---- create_account / add_note
    h0, pf0 = ctx.shielder_prove_creation(pkc, know, tokens, fr(), fr())
    acc0 = ps.hash_fix_len([tok_fr[0], 0, tok_fr[1], 0])
    assert int.from_bytes(h0, "little") == ps.hash_fix_len([7, 12, 11, acc0])
    zk.shielder_verify_creation(vkc, h0, tokens, pf0)
    for bad_args in ((h0, [bytes(32), token]), (ec.fr_to_bytes(5), tokens)):
        with pytest.raises(pkg.ZkmiError) as e:
            zk.shielder_verify_creation(vkc, bad_args[0], bad_args[1], pf0)
        assert e.value.code == -5  # ZkpError::VerificationError

    # ---- the contract's note tree, Poseidon flavour, on the device
    n = 1 << lg_tree
    nodes = torch.zeros((2 * n - 1, 32), dtype=torch.uint8, device="cuda")

    def add_leaf(i, leaf):
        nodes[i] = torch.frombuffer(bytearray(leaf), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        ctx.poseidon_merkle_tree_dev(nodes.data_ptr(), lg_tree)
        return bytes(nodes[-1].cpu().numpy().tobytes())

    def path_of(i):
        _, paths = ctx.poseidon_merkle_paths_dev(nodes.data_ptr(), lg_tree, [i])
        return [paths[32 * k : 32 * k + 32] for k in range(lg_tree)]

    root = add_leaf(0, h0)
    balance, leaf_id, nullifier_old = 0, 0, null0
    for step, (kind, amount) in enumerate((("deposit", 10), ("withdraw", 9))):
        op = zk.op_pub(kind, amount, token, user)
        trap, null = (20 + step).to_bytes(32, "little"), (30 + step).to_bytes(32, "little")
        h_new, root_got, know_new, pf = ctx.shielder_prove_update(pkd, pkw, know, op, zk.op_priv(user), trap, null,
                                                                  path_of(leaf_id), leaf_id, fr(), fr())
        assert root_got == root  # the relation's recomputed root is the device tree's root
        balance += amount if kind == "deposit" else -amount
        acc = ps.hash_fix_len([tok_fr[0], balance, tok_fr[1], 0])
        assert int.from_bytes(h_new, "little") == ps.hash_fix_len([7, 20 + step, 30 + step, acc])
        zk.shielder_verify_update(vkd, vkw, op, h_new, root, nullifier_old, pf)
        # what the contract would reject: another amount, the other operation kind, a stale root, a replayed nullifier
        other_kind = zk.op_pub("withdraw" if kind == "deposit" else "deposit", amount, token, user)
        for bad in ((zk.op_pub(kind, amount + 1, token, user), h_new, root, nullifier_old), (other_kind, h_new, root, nullifier_old),
                    (op, h_new, ec.fr_to_bytes(1), nullifier_old), (op, h_new, root, ec.fr_to_bytes(99))):
            with pytest.raises(pkg.ZkmiError) as e:
                zk.shielder_verify_update(vkd, vkw, *bad, pf)
            assert e.value.code == -5
        # the mock's own state machine saw the same transition
        assert bytes(know_new.trapdoor_old.bytes) == bytes(know.trapdoor_new.bytes)
        assert int.from_bytes(bytes(know_new.acc_new.balances[0][1].bytes), "little") == balance
        know, nullifier_old, leaf_id = know_new, null, leaf_id + 1
        root = add_leaf(leaf_id, h_new)
    # impossible updates: the mock's error codes, no proof
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.shielder_prove_update(pkd, pkw, know, zk.op_pub("withdraw", 2, token, user), zk.op_priv(user), trap0, null0,
                                  path_of(leaf_id), leaf_id, fr(), fr())
    assert e.value.code == -6  # AccountUpdateError: balance is 1
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.shielder_prove_update(pkd, pkw, know, zk.op_pub("withdraw", 1, token, user), zk.op_priv(bytes([9]) + bytes(31)),
                                  trap0, null0, path_of(leaf_id), leaf_id, fr(), fr())
    assert e.value.code == -7  # OperationCombineError
    for x in (pkc, pkd, pkw, r1c, r1d, r1w):
        x.free()


# ---- Poseidon-5 ------------------------------------------------------------


@pytest.mark.parametrize("field,name", [(0, "bls12_381_fr"), (1, "bn254_fr")])
def test_poseidon_hash_batch_matches_oracle(ctx, zk, field, name):
    """hash_fix_len_array on the GPU == oracle/poseidon.py for every framing case: empty input,
    partial chunk, exactly RATE (extra padding permutation), more than one chunk; edge values."""
    from oracle import poseidon as ps

    p, _ = ps.FIELDS[name]
    rng = ec.SplitMix64(77 + field)
    for arity in (0, 1, 2, 3, 4, 5, 8, 9):
        n = 67
        vals = [[rng.next() * rng.next() * rng.next() * rng.next() % p for _ in range(arity)] for _ in range(n)]
        if arity:
            vals[0] = [0] * arity
            vals[1] = [p - 1] * arity
        raw = b"".join(v.to_bytes(32, "little") for row in vals for v in row)
        got = ctx.poseidon_hash_batch(raw, n, arity, field)
        want = b"".join(ps.hash_fix_len(row, name).to_bytes(32, "little") for row in vals)
        assert got == want, "arity %d" % arity
    # inputs must be canonical
    with pytest.raises(Exception):
        ctx.poseidon_hash_batch(p.to_bytes(32, "little") * 2, 1, 2, field)
    assert ctx.poseidon_hash_batch(b"", 0, 2, field) == b""


def test_poseidon_merkle_tree_dev_matches_oracle(ctx, zk):
    """Device-built Poseidon tree (256 leaves) == oracle tree; a path taken from the device nodes
    recomputes the root with the selector convention of merkle_proof.rs:38-61."""
    import torch
    from oracle import poseidon as ps

    lg = 8
    n = 1 << lg
    leaves = [ps.hash_fix_len([i]) for i in range(n)]
    nodes = torch.zeros((2 * n - 1, 32), dtype=torch.uint8, device="cuda")
    nodes[:n] = torch.frombuffer(bytearray(b"".join(v.to_bytes(32, "little") for v in leaves)), dtype=torch.uint8).view(n, 32).cuda()
    torch.cuda.synchronize()
    ctx.poseidon_merkle_tree_dev(nodes.data_ptr(), lg)
    got = bytes(nodes.cpu().numpy().tobytes())
    levels = ps.merkle_tree(leaves)
    want = b"".join(v.to_bytes(32, "little") for lv in levels for v in lv)
    assert got == want
    ints = [int.from_bytes(got[32 * i : 32 * i + 32], "little") for i in range(2 * n - 1)]
    idx, off, width = 201, 0, n
    shape, path = [], []
    for lv in range(lg):
        shape.append(1 - ((idx >> lv) & 1))
        path.append(ints[off + ((idx >> lv) ^ 1)])
        off += width
        width //= 2
    assert ps.merkle_root(leaves[idx], shape, path) == ints[-1]


def test_poseidon_hash_large_batch_self_consistent(ctx, zk):
    """2^18 two-to-one hashes resident in HBM: equal inputs give equal digests, the batch equals
    the same rows hashed in two halves, and sampled rows equal the oracle."""
    import torch
    from oracle import poseidon as ps

    n = 1 << 18
    g = torch.Generator(device="cuda").manual_seed(5)
    raw = torch.randint(0, 256, (n, 2, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, :, 31] &= 0x3F
    raw[n // 2] = raw[3]
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    ctx.poseidon_hash_batch_dev(raw.data_ptr(), n, 2, out.data_ptr())
    ctx.poseidon_hash_batch_dev(raw.data_ptr(), n // 2, 2, out2.data_ptr())
    ctx.poseidon_hash_batch_dev(raw[n // 2 :].data_ptr(), n // 2, 2, out2[n // 2 :].data_ptr())
    assert torch.equal(out, out2)
    assert torch.equal(out[n // 2], out[3])
    host_in, host_out = raw.cpu().numpy(), out.cpu().numpy()
    for i in (0, 3, 12345, n - 1):
        a, b = (int.from_bytes(host_in[i, k].tobytes(), "little") for k in (0, 1))
        assert int.from_bytes(host_out[i].tobytes(), "little") == ps.hash_fix_len([a, b])


def _wire_key(zk, pk, vk, toxic, r1):
    """Proving key in wire format for the C++ oracle prover (as bench.py's cpu_baseline does)."""
    n, N = r1.n_vars, 1 << r1.log_n
    return {
        "alpha_g1": vk[:96], "beta_g2": vk[96:288], "delta_g2": vk[480:672],
        "beta_g1": zk.g1_mul(zk.g1_generator(), toxic[64:96]), "delta_g1": zk.g1_mul(zk.g1_generator(), toxic[128:160]),
        "a_query": pk.export_query(0, 0, n), "b_g1_query": pk.export_query(1, 0, n),
        "b_g2_query": pk.export_query(2, 0, n), "h_query": pk.export_query(3, 0, N - 1),
        "l_query": pk.export_query(4, 0, n - r1.n_pub),
    }


def test_update_note_poseidon_relation_proof(ctx, zk):
    """The reference's update_note relation with real Poseidon hashing (N = 2^14): the GPU proof
    (a) verifies against publics computed independently by oracle/poseidon.py, (b) is byte-identical
    to the C++ oracle prover's proof over the same key, (c) fails for any other public input."""
    from oracle import cpp as ocpp
    from test_cpu_host import _note_update_case

    ocpp.build()
    lg = 14
    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(4242)
    toxic = frs([rng.fr() for _ in range(5)])
    pk, vk = ctx.groth16_setup(r1, toxic)
    inp, publics = _note_update_case(zk, 99, 1, amount=33, balances=(5, 40), slot=1)
    wit, pub, rc = zk.update_note_witness(lg, 1, inp)
    assert rc == 0 and pub == publics
    r_, s_ = ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr())
    proof = ctx.groth16_prove(pk, wit, r_, s_)
    assert zk.groth16_verify(vk, frs(publics), proof) is True
    for k in range(6):
        bad = list(publics)
        bad[k] = (bad[k] + 1) % R
        assert zk.groth16_verify(vk, frs(bad), proof) is False
    mats = [r1.export(m) for m in range(3)]
    want = ocpp.groth16_prove(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, _wire_key(zk, pk, vk, toxic, r1), wit, r_, s_)
    assert proof == want
    pk.free()
    r1.free()


def test_update_note_witness_batch_on_device(ctx, zk):
    """assignments of a batch generated by one GPU thread per instance equal the host
    generator byte for byte (valid and impossible updates, both operation kinds), and feed the
    pipelined batch prover straight from HBM."""
    import copy
    import ctypes as C
    import torch
    from test_cpu_host import _note_update_case

    lg = 14
    n = 1 << lg
    cases = [_note_update_case(zk, 700 + i, 1, amount=10 + i, slot=i & 1) for i in range(6)]
    inputs = [c[0] for c in cases]
    bad = copy.deepcopy(inputs[0])
    C.memmove(bad.amount, (10**6).to_bytes(32, "little"), 32)  # underflow
    inputs.append(bad)
    bufs = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in inputs]
    torch.cuda.synchronize()
    status = ctx.update_note_witness_batch_dev(lg, 1, inputs, [b.data_ptr() for b in bufs])
    assert status == [0] * 6 + [-6]
    for inp, buf in zip(inputs, bufs):
        w, _, _ = zk.update_note_witness(lg, 1, inp, check=False)
        assert bytes(buf.cpu().numpy().tobytes()) == w
    # deposits use the same kernel with the other sign
    dep, dep_pub = _note_update_case(zk, 31, 0, amount=5, slot=0)
    dbuf = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    assert ctx.update_note_witness_batch_dev(lg, 0, [dep], [dbuf.data_ptr()]) == [0]
    assert bytes(dbuf.cpu().numpy().tobytes()) == zk.update_note_witness(lg, 0, dep)[0]
    # device-generated witnesses -> batch prover, no host copy of the assignment
    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(8080)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(6)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(6)]
    proofs = ctx.groth16_prove_batch_dev(pk, [b.data_ptr() for b in bufs[:6]], rs, ss)
    for (_, publics), pf in zip(cases, proofs):
        assert zk.groth16_verify(vk, frs(publics), pf) is True
    pk.free()
    r1.free()


# ---- the contract's SHA-256 Merkle tree (pinned by the reference's own test) ----


def _contract_tree(depth, leaves):
    """MerkleTree::add_leaf replayed with hashlib (contract/merkle.rs:48-81): nodes[] keyed like the
    contract (root = 1, leaf i = 2^depth + i), missing nodes read as zero; returns the node map."""
    import hashlib

    size = 1 << depth
    nodes = {}
    for i, leaf in enumerate(leaves):
        idx = size + i
        nodes[idx] = leaf
        idx //= 2
        while idx > 0:
            left, right = nodes.get(2 * idx, bytes(32)), nodes.get(2 * idx + 1, bytes(32))
            nodes[idx] = hashlib.sha256(left + right).digest()
            idx //= 2
    return nodes


def test_sha256_pairs_match_hashlib(ctx):
    import hashlib
    import random

    rnd = random.Random(9)
    n = 1000
    raw = rnd.randbytes(64 * n)
    want = b"".join(hashlib.sha256(raw[64 * i : 64 * i + 64]).digest() for i in range(n))
    assert ctx.sha256_pairs(raw, n) == want
    assert ctx.sha256_pairs(b"", 0) == b""


def test_sha256_merkle_tree_matches_contract_semantics(ctx):
    """Device tree == the reference's own pinned value (merkle.rs:115-132, two leaves, depth 10) and ==
    add_leaf replayed leaf by leaf for partially filled trees (untouched nodes read as zero)."""
    import torch

    depth = 10
    size = 1 << depth
    two = [(1).to_bytes(32, "little"), (2).to_bytes(32, "little")]
    for leaves in (two, [i.to_bytes(32, "little") for i in range(10)], [bytes([i % 251] * 32) for i in range(size)], []):
        buf = torch.full((2 * size - 1, 32), 0xEE, dtype=torch.uint8, device="cuda")  # stale contents must not leak
        if leaves:
            buf[: len(leaves)] = torch.frombuffer(bytearray(b"".join(leaves)), dtype=torch.uint8).view(-1, 32).cuda()
        torch.cuda.synchronize()
        ctx.sha256_merkle_tree_dev(buf.data_ptr(), depth, len(leaves))
        got = bytes(buf.cpu().numpy().tobytes())
        nodes = _contract_tree(depth, leaves)
        off, width, level = 0, size, depth
        while width >= 1:
            for j in range(width):
                assert got[32 * (off + j) : 32 * (off + j + 1)] == nodes.get((1 << level) + j, bytes(32)), (level, j)
            off += width
            width //= 2
            level -= 1
        if leaves is two:
            assert got[-32:].hex() == golden("mock_boundary.json")["merkle_root_two_leaves"]


@pytest.mark.parametrize("group", [1, 2])
def test_msm_degenerate_bases_and_scalars(ctx, group):
    """Exceptional cases of the bucket additions, forced into the same buckets by equal scalars:
    P + P (doubling path), P + (-P) (cancellation to infinity, then restart), points at infinity
    among the bases, scalars 0, 1, r - 1; in the light-bucket kernel (n = 9), across the heavy-bucket
    kernels (the pattern repeated 400 times) and through the signed-digit borrow (r - 1)."""
    F, G = (ec.Fq, ec.G1) if group == 1 else (ec.Fq2, ec.G2)
    mul = ec.g1_mul if group == 1 else ec.g2_mul
    to_b = ec.g1_to_bytes if group == 1 else ec.g2_to_bytes
    width = 96 if group == 1 else 192
    neg = lambda p: ec.pt_neg(F, p)
    P2, P3 = mul(2), mul(3)
    pts = [G, G, neg(G), G, None, P2, neg(P2), P3, P3]
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890AB % R
    # (6 000 repetitions: 54 000 points per bucket -- several wave-items per heavy bucket in k_accum_heavy_nc, lanes that meet
    # P + P and leave a marker, split buckets and tickets in the partial-sum mode of k_accum_heavy; also over prepared bases)
    for reps, scalars in (
        (1, [k] * 9),
        (1, [k, k, k, R - 1, 5, 0, 1, R - 1, R - 1]),
        (400, [k] * 9),
        (6000, [k] * 9),
        (6000, [k, k, k, R - 1, 5, 0, 1, R - 1, R - 1]),
    ):
        bases = pts * reps
        sc = scalars * reps
        want = None
        for s, p in zip(scalars, pts):
            if p is not None and s:
                want = ec.pt_add(F, want, ec.pt_mul(F, p, s))
        want = ec.pt_mul(F, want, reps) if want is not None else None
        raw_b = b"".join(to_b(p) if p is not None else bytes(width) for p in bases)
        b = ctx.bases_g1(raw_b) if group == 1 else ctx.bases_g2(raw_b)
        got = (ctx.msm_g1 if group == 1 else ctx.msm_g2)(frs(sc), b)
        assert got == (to_b(want) if want is not None else bytes(width)), (reps, scalars[:3])
        if reps >= 6000:
            b.prepare()
            got = (ctx.msm_g1 if group == 1 else ctx.msm_g2)(frs(sc), b)
            assert got == (to_b(want) if want is not None else bytes(width)), (reps, scalars[:3], "prepared")
        b.free()


def test_msm_two_queries_through_one_bucket_set(ctx, zk):
    """The mechanism behind the prover's L + H merge, exercised on inputs a proving key never produces:
    MSM(a) left unreduced in its bucket array, MSM(b) accumulated INTO it, one reduction -- against the C++ oracle's MSM over
    the concatenation.  a is sparse (90 % zero scalars: most buckets are EMPTY when b's kernel arrives and take the redo
    pass from infinity) with a heavy bucket (5 % ones); b repeats a's non-zero scalars on the same points (P + P across the
    two MSMs: the doubling exit of the accumulate-into kernel), holds a 20 %-heavy bucket of its own (the cooperative kernel
    adds into the bucket) and opposite points (P - P: cancellation).  Windowed plan, and prepared bases (shared-bucket plan)."""
    import torch

    from oracle import cpp as ocpp

    n = 1 << 14
    g = torch.Generator().manual_seed(99)
    base = ctx.bases_g1_synthetic(n)
    pts = bytearray(base.read(0, n))
    base.free()
    # points 1000..1999 repeat points 0..999; points 2000..2499 are the NEGATIVES of points 0..499 (y -> p - y)
    P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    for i in range(1000):
        pts[96 * (1000 + i) : 96 * (1001 + i)] = pts[96 * i : 96 * (i + 1)]
    for i in range(500):
        y = int.from_bytes(pts[96 * i + 48 : 96 * i + 96], "little")
        pts[96 * (2000 + i) : 96 * (2000 + i) + 48] = pts[96 * i : 96 * i + 48]
        pts[96 * (2000 + i) + 48 : 96 * (2001 + i)] = (P - y).to_bytes(48, "little")
    pts = bytes(pts)
    uni = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    uni[:, 31] &= 0x3F
    a = uni.clone()
    kind = torch.rand(n, generator=g)
    a[kind < 0.90] = 0
    one = (kind >= 0.90) & (kind < 0.95)
    a[one] = 0
    a[one, 0] = 1
    b = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    b[:, 31] &= 0x3F
    b[:1000] = a[:1000]            # same scalar on the same point in both MSMs
    b[1000:2000] = a[:1000]        # ... and on its repeated copy
    a[2000:2500] = b[:500]         # a adds s P, b adds s P: with the negated copies below everything cancels pairwise
    b[2000:2500] = b[:500]
    heavy = torch.rand(n, generator=g) < 0.20
    heavy[:2500] = False
    b[heavy] = 0
    b[heavy, 0] = 7
    want = ocpp.msm_g1(a.numpy().tobytes() + b.numpy().tobytes(), pts + pts)
    da, db = a.contiguous().cuda(), b.contiguous().cuda()
    torch.cuda.synchronize()
    for prepared in (False, True):
        bs = ctx.bases_g1(pts, check=False)
        if prepared:
            bs.prepare()
        assert ctx.selftest_msm_g1_sum2_dev(da.data_ptr(), db.data_ptr(), n, bs) == want, prepared
        assert ctx.selftest_msm_g1_sum2_dev(db.data_ptr(), da.data_ptr(), n, bs) == want, prepared  # roles swapped
        bs.free()


# ---- BN254 MSM / NTT / KZG commit ---------------------------------------------


def _bn_frs(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def test_bn254_ntt_matches_oracle(ctx):
    from oracle import bn254 as bn

    for lg in (0, 1, 4, 9, 11, 13):
        rng = ec.SplitMix64(50 + lg)
        a = [rng.next() * rng.next() * rng.next() * rng.next() % bn.R for _ in range(1 << lg)]
        a[0] = bn.R - 1
        raw = _bn_frs(a)
        assert ctx.bn254_ntt(raw, lg) == _bn_frs(bn.ntt(a))
        assert ctx.bn254_ntt(raw, lg, inverse=True) == _bn_frs(bn.ntt(a, inverse=True))
        assert ctx.bn254_ntt(raw, lg, coset=True) == _bn_frs(bn.ntt(a, coset=True))
        assert ctx.bn254_ntt(raw, lg, inverse=True, coset=True) == _bn_frs(bn.ntt(a, inverse=True, coset=True))
    with pytest.raises(Exception):
        ctx.bn254_ntt(bn.R.to_bytes(32, "little") * 2, 1)


def test_bn254_ntt_large_round_trip(ctx):
    import torch

    lg = 20
    n = 1 << lg
    g = torch.Generator(device="cuda").manual_seed(20)
    raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= 0x1F
    x = raw.clone()
    torch.cuda.synchronize()
    ctx.bn254_ntt_dev(x.data_ptr(), lg)
    assert not torch.equal(x, raw)
    ctx.bn254_ntt_dev(x.data_ptr(), lg, inverse=True)
    assert torch.equal(x, raw)
    ctx.bn254_ntt_dev(x.data_ptr(), lg, coset=True)
    ctx.bn254_ntt_dev(x.data_ptr(), lg, inverse=True, coset=True)
    assert torch.equal(x, raw)


def test_bn254_msm_matches_oracle(ctx):
    """Seeded MSM vs double-and-add; edge scalars; infinity / repeated / opposite bases; on-curve check."""
    from oracle import bn254 as bn

    rng = ec.SplitMix64(254)
    n = 300
    pts = bn.synthetic_bases(n)
    b = ctx.bn254_bases_synthetic(n)
    assert b.read(0, 4) == b"".join(bn.g1_to_bytes(p) for p in pts[:4])
    assert b.read(n - 1, 1) == bn.g1_to_bytes(pts[-1])
    sc = [rng.next() * rng.next() * rng.next() * rng.next() % bn.R for _ in range(n)]
    sc[0], sc[1], sc[2] = 0, 1, bn.R - 1
    assert ctx.bn254_msm_g1(_bn_frs(sc), b) == bn.g1_to_bytes(bn.msm_naive(sc, pts))
    assert ctx.bn254_msm_g1(b"", b) == bytes(64)
    b.free()
    g, g2 = bn.G1, bn.pt_mul(bn.G1, 2)
    odd = [g, g, bn.pt_neg(g), None, g2, bn.pt_neg(g2), g2, g]
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890AB % bn.R
    for reps, scalars in ((1, [k] * 8), (300, [k] * 8), (1, [k, bn.R - 1, 5, 7, 0, 1, bn.R - 1, k])):
        bb = ctx.bn254_bases(b"".join(bn.g1_to_bytes(p) for p in odd * reps))
        want = bn.pt_mul(bn.msm_naive(scalars, odd), reps)
        assert ctx.bn254_msm_g1(_bn_frs(scalars * reps), bb) == bn.g1_to_bytes(want)
        bb.free()
    with pytest.raises(Exception):
        ctx.bn254_bases((1).to_bytes(32, "little") + (3).to_bytes(32, "little"))  # (1, 3) is not on the curve


def test_bn254_msm_full_size_closed_form(ctx):
    """n = 2^20 on the synthetic bases: sum s_i [1 + i c] G = [sum s_i + c sum i s_i] G."""
    import torch
    from oracle import bn254 as bn

    n = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(99)
    raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= 0x1F
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    s0 = raw.to(torch.int64).sum(dim=0).cpu().tolist()
    s1 = (raw.to(torch.int64) * idx[:, None]).sum(dim=0).cpu().tolist()
    tot = sum(v << (8 * k) for k, v in enumerate(s0))
    wtot = sum(v << (8 * k) for k, v in enumerate(s1))
    b = ctx.bn254_bases_synthetic(n)
    got = ctx.bn254_msm_g1_dev(raw.data_ptr(), n, b)
    assert got == bn.g1_to_bytes(bn.pt_mul(bn.G1, (tot + 0xC0FFEE * wtot) % bn.R))
    b.free()


def test_bn254_kzg_commit(ctx):
    """commit(evaluations) = MSM(SRS, iNTT(evaluations)) = [p(tau)] G for an SRS [tau^i] G."""
    import torch
    from oracle import bn254 as bn

    lg = 8
    n = 1 << lg
    tau = 0xDEADBEEFCAFEF00D1234567 % bn.R
    srs = [bn.pt_mul(bn.G1, pow(tau, i, bn.R)) for i in range(n)]
    rng = ec.SplitMix64(88)
    coeffs = [rng.next() * rng.next() * rng.next() * rng.next() % bn.R for _ in range(n)]
    evals = bn.ntt(coeffs)
    b = ctx.bn254_bases(b"".join(bn.g1_to_bytes(p) for p in srs))
    d = torch.frombuffer(bytearray(_bn_frs(evals)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = ctx.bn254_kzg_commit_dev(d.data_ptr(), lg, b)
    p_tau = sum(c * pow(tau, i, bn.R) for i, c in enumerate(coeffs)) % bn.R
    assert got == bn.g1_to_bytes(bn.pt_mul(bn.G1, p_tau))
    assert bytes(d.cpu().numpy().tobytes()) == _bn_frs(coeffs)  # the coefficients are left in place
    b.free()


def test_bn254_kzg_open_matches_oracle(ctx):
    """zkmi_bn254_kzg_open_dev = eval_polynomial + kate_division + commit: evaluation, every quotient coefficient and the
    opening proof against the oracle for lengths around the block sizes of the scan (1, 2, 1023..1025 coefficients), at
    zeta in {0, 1, r - 1, random}; against an SRS with a known tau the proof is [q(tau)] G, through the plain and the
    prepared SRS."""
    import torch
    from oracle import bn254 as bn

    rng = ec.SplitMix64(2540)
    fr = lambda: rng.next() * rng.next() * rng.next() * rng.next() % bn.R
    nmax = 1030
    pts = bn.synthetic_bases(300)
    b = ctx.bn254_bases_synthetic(nmax)
    for n in (1, 2, 5, 300, 1023, 1024, 1025, 1030):
        p = [fr() for _ in range(n)]
        d = torch.frombuffer(bytearray(_bn_frs(p)), dtype=torch.uint8).cuda()
        dq = torch.zeros(32 * max(n - 1, 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for z in (fr(), 0, 1, bn.R - 1):
            ev, pf = ctx.bn254_kzg_open_dev(d.data_ptr(), n, _bn_frs([z]), b, dq.data_ptr())
            q = bn.kate_division(p, z)
            assert ev == _bn_frs([bn.eval_polynomial(p, z)]), (n, z)
            assert bytes(dq.cpu().numpy().tobytes())[: 32 * (n - 1)] == _bn_frs(q), (n, z)
            if n <= 300:
                assert pf == bn.g1_to_bytes(bn.msm_naive(q, pts[: n - 1])), (n, z)
            else:  # the synthetic bases' closed form: sum q_i [1 + i c] G
                k = (sum(q) + 0xC0FFEE * sum(i * v for i, v in enumerate(q))) % bn.R
                assert pf == bn.g1_to_bytes(bn.pt_mul(bn.G1, k)), (n, z)
    b.free()
    tau, n = 0xDEADBEEFCAFEF00D1234567 % bn.R, 256
    srs_pts = [bn.pt_mul(bn.G1, pow(tau, i, bn.R)) for i in range(n)]
    p = [fr() for _ in range(n)]
    z = fr()
    d = torch.frombuffer(bytearray(_bn_frs(p)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    srs = ctx.bn254_bases(b"".join(bn.g1_to_bytes(x) for x in srs_pts))
    want = bn.g1_to_bytes(bn.pt_mul(bn.G1, bn.eval_polynomial(bn.kate_division(p, z), tau)))
    ev, pf = ctx.bn254_kzg_open_dev(d.data_ptr(), n, _bn_frs([z]), srs)
    assert pf == want and ev == _bn_frs([bn.eval_polynomial(p, z)])
    srs.prepare()
    assert ctx.bn254_kzg_open_dev(d.data_ptr(), n, _bn_frs([z]), srs) == (ev, pf)
    assert ctx.bn254_kzg_open_dev(d.data_ptr(), n - 7, _bn_frs([z]), srs)[1] == bn.g1_to_bytes(
        bn.pt_mul(bn.G1, bn.eval_polynomial(bn.kate_division(p[: n - 7], z), tau)))
    with pytest.raises(Exception):
        ctx.bn254_kzg_open_dev(d.data_ptr(), n, _bn_frs([z])[:31] + b"\xff", srs)  # zeta >= r
    srs.free()


def test_bn254_kzg_open_full_size(ctx):
    """2^20 + 3 coefficients (1 025 blocks of the first level: all three levels of the scan run): evaluation and every
    quotient coefficient equal the oracle's Horner chain; the proof equals the synthetic bases' closed form."""
    import torch
    from oracle import bn254 as bn

    n = (1 << 20) + 3
    g = torch.Generator(device="cuda").manual_seed(2541)
    raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= 0x1F
    host = raw.cpu().numpy().tobytes()
    p = [int.from_bytes(host[32 * i: 32 * i + 32], "little") for i in range(n)]
    z = 0x2B1C5E9F00D1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234 % bn.R
    b = ctx.bn254_bases_synthetic(n - 1)
    dq = torch.zeros(32 * (n - 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ev, pf = ctx.bn254_kzg_open_dev(raw.data_ptr(), n, _bn_frs([z]), b, dq.data_ptr())
    q = bn.kate_division(p, z)
    assert ev == _bn_frs([bn.eval_polynomial(p, z)])
    assert dq.cpu().numpy().tobytes() == _bn_frs(q)
    k = (sum(q) + 0xC0FFEE * sum(i * v for i, v in enumerate(q))) % bn.R
    assert pf == bn.g1_to_bytes(bn.pt_mul(bn.G1, k))
    b.free()


def test_poseidon_and_bn254_golden_fixtures_on_gpu(ctx, zk):
    """HIP path vs the committed fixtures (tests/golden/poseidon.json, bn254.json)."""
    g = golden("poseidon.json")
    for field, name in ((0, "bls12_381_fr"), (1, "bn254_fr")):
        for c in g[name]["hashes"]:
            vals = [int(v, 16) for v in c["inputs"]]
            got = ctx.poseidon_hash_batch(b"".join(v.to_bytes(32, "little") for v in vals), 1, len(vals), field)
            assert hex(int.from_bytes(got, "little")) == c["hash"]
    b = golden("bn254.json")
    bases = ctx.bn254_bases(H(b["msm"]["bases"]))
    assert bases.read(0, 4) == b"".join(H(x) for x in b["synthetic_first4"])
    assert ctx.bn254_msm_g1(H(b["msm"]["scalars"]), bases).hex() == b["msm"]["expected"]
    bases.free()
    n = b["ntt"]
    x = H(n["input"])
    assert ctx.bn254_ntt(x, n["log_n"]).hex() == n["forward"]
    assert ctx.bn254_ntt(x, n["log_n"], inverse=True).hex() == n["inverse"]
    assert ctx.bn254_ntt(x, n["log_n"], coset=True).hex() == n["coset_forward"]
    assert ctx.bn254_ntt(x, n["log_n"], inverse=True, coset=True).hex() == n["coset_inverse"]
    import torch

    k = b["kzg"]
    srs = ctx.bn254_bases(H(k["srs"]))
    d = torch.frombuffer(bytearray(H(k["evaluations"])), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert ctx.bn254_kzg_commit_dev(d.data_ptr(), k["log_n"], srs).hex() == k["commitment"]
    assert bytes(d.cpu().numpy().tobytes()).hex() == k["coefficients"]
    o = b["kzg_open"]  # d now holds the coefficients
    dq = torch.zeros(32 * 15, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ev, pf = ctx.bn254_kzg_open_dev(d.data_ptr(), 16, H(o["zeta"]), srs, dq.data_ptr())
    assert (ev.hex(), pf.hex(), dq.cpu().numpy().tobytes().hex()) == (o["eval"], o["proof"], o["quotient"])
    srs.free()
    gp = b["grand_product"]
    dn = torch.frombuffer(bytearray(H(gp["num"])), dtype=torch.uint8).cuda()
    dd = torch.frombuffer(bytearray(H(gp["den"])), dtype=torch.uint8).cuda()
    out = torch.zeros(32 * 12, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.bn254_grand_product_dev(dn.data_ptr(), dd.data_ptr(), 12, out.data_ptr()).hex() == gp["total"]
    assert out.cpu().numpy().tobytes().hex() == gp["z"]


def test_bn254_prepared_srs_matches_plain_msm(ctx):
    """zkmi_bn254_srs_prepare (fixed-base table, shared buckets) gives the same MSM / commitment as the
    windowed schedule, for small, odd and large lengths and for edge scalars.

    Above 77 terms this compares the prepared path with the plain one only: both run the same kernels, so an error they
    share passes here.  The prepared path meets an independent reference (the sum of discrete logs, bn254_msm_cases.py) in
    test_gpu_bn254_msm.py: designed first-pair inputs at 4 000 terms, heavy buckets at 2 561 ... 2 625 and 54 000, witness-like
    scalars at 5 000 and 70 000, every irregular size up to 4 097, and both sides of the second-level threshold."""
    import torch
    from oracle import bn254 as bn

    rng = ec.SplitMix64(1313)
    for n in (1, 16, 77, 1000, 5000):
        sc = [rng.next() * rng.next() * rng.next() * rng.next() % bn.R for _ in range(n)]
        sc[0] = bn.R - 1
        if n > 2:
            sc[1], sc[2] = 0, 1
        b = ctx.bn254_bases_synthetic(n)
        plain = ctx.bn254_msm_g1(_bn_frs(sc), b)
        b.prepare()
        assert ctx.bn254_msm_g1(_bn_frs(sc), b) == plain
        if n <= 77:
            assert plain == bn.g1_to_bytes(bn.msm_naive(sc, bn.synthetic_bases(n)))
        # a shorter MSM over prepared bases falls back to the windowed schedule
        if n > 16:
            assert ctx.bn254_msm_g1(_bn_frs(sc[:16]), b) == bn.g1_to_bytes(bn.msm_naive(sc[:16], bn.synthetic_bases(16)))
        b.free()
    n = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(7)
    raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= 0x1F
    b = ctx.bn254_bases_synthetic(n)
    plain = ctx.bn254_msm_g1_dev(raw.data_ptr(), n, b)
    b.prepare()
    assert ctx.bn254_msm_g1_dev(raw.data_ptr(), n, b) == plain
    b.free()


def test_prepared_bases_match_plain_msm(ctx):
    """zkmi_bases_g{1,2}_prepare (table of 2^(c w) multiples, shared buckets) gives the same MSM as the windowed
    schedule: small, odd and plan-boundary lengths, edge scalars (0, 1, r - 1, equal scalars on equal points force the
    P + P redo path), a shorter MSM over prepared bases, and 2^22 terms against the closed form."""
    from oracle import cpp as ocpp

    rng = ec.SplitMix64(4242)
    for group in (1, 2):
        for n in (1, 2, 33, 1000, (1 << 13) + 5, 70000 if group == 1 else 9000):
            sc = [rng.fr() for _ in range(n)]
            sc[0] = R - 1
            if n > 3:
                sc[1], sc[2], sc[3] = 0, 1, sc[0]
            raw = frs(sc)
            b = ctx.bases_g1_synthetic(n) if group == 1 else ctx.bases_g2_synthetic(n)
            msm = ctx.msm_g1 if group == 1 else ctx.msm_g2
            plain = msm(raw, b)
            assert msm(raw, b.prepare()) == plain
            if n <= 9000:
                want = (ocpp.msm_g1 if group == 1 else ocpp.msm_g2)(raw, b.read(0, n))
                assert plain == want
            if n > 33:  # fewer scalars than bases: windowed schedule again
                short = (ocpp.msm_g1 if group == 1 else ocpp.msm_g2)(raw[: 32 * 33], b.read(0, 33))
                assert msm(raw[: 32 * 33], b) == short
            b.free()
    n = 1 << 22
    raw, tot, wtot = _torch_scalars(n, 23)
    b = ctx.bases_g1_synthetic(n).prepare()
    assert ctx.msm_g1_dev(raw.data_ptr(), n, b) == _closed_form_g1(tot, wtot)
    b.free()


def test_msm_random_sizes_vs_cpp_oracle(ctx):
    """A sweep over irregular lengths (1 ... 40 000, powers of two and their neighbours included) of G1
    and G2 MSMs against the C++ oracle on the same seeded inputs; every plan boundary of the window /
    chunk selection is crossed somewhere in the sweep."""
    import random

    from oracle import cpp as ocpp

    ocpp.build()
    rnd = random.Random(2718)
    sizes = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097] + [rnd.randrange(5, 40000) for _ in range(8)]
    nmax = max(sizes)
    b1 = ctx.bases_g1_synthetic(nmax)
    raw_b1 = b1.read(0, nmax)
    for n in sizes:
        sc = bytearray(rnd.randbytes(32 * n))
        for i in range(31, 32 * n, 32):
            sc[i] &= 0x3F
        sc = bytes(sc)
        assert ctx.msm_g1(sc, b1) == ocpp.msm_g1(sc, raw_b1[: 96 * n]), n
    b1.free()
    g2_sizes = [1, 2, 65, 257, 1025, rnd.randrange(1500, 6000)]
    nmax2 = max(g2_sizes)
    b2 = ctx.bases_g2_synthetic(nmax2)
    raw_b2 = b2.read(0, nmax2)
    for n in g2_sizes:
        sc = bytearray(rnd.randbytes(32 * n))
        for i in range(31, 32 * n, 32):
            sc[i] &= 0x3F
        sc = bytes(sc)
        assert ctx.msm_g2(sc, b2) == ocpp.msm_g2(sc, raw_b2[: 192 * n]), n
    b2.free()


def test_ntt_every_size_round_trip_and_definition(ctx):
    """Every domain size 2^0 ... 2^22 (one-, two- and three-pass plans, every tile shape of the register-blocked passes):
    forward and coset-inverse transforms against the C++ oracle, inverse(forward(x)) == x and the coset round trip."""
    import torch
    from oracle import cpp as ocpp

    ocpp.build()
    g = torch.Generator(device="cuda").manual_seed(314)
    for lg in range(0, 23):
        n = 1 << lg
        raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
        raw[:, 31] &= 0x3F
        x = raw.clone()
        torch.cuda.synchronize()
        host = bytes(raw.cpu().numpy().tobytes())
        ctx.ntt_dev(x.data_ptr(), lg)
        assert bytes(x.cpu().numpy().tobytes()) == ocpp.ntt(host, lg), lg
        ctx.ntt_dev(x.data_ptr(), lg, inverse=True)
        assert torch.equal(x, raw), lg
        ctx.ntt_dev(x.data_ptr(), lg, coset=True)
        ctx.ntt_dev(x.data_ptr(), lg, inverse=True, coset=True)
        assert torch.equal(x, raw), lg
        ctx.ntt_dev(x.data_ptr(), lg, inverse=True, coset=True)
        assert bytes(x.cpu().numpy().tobytes()) == ocpp.ntt(host, lg, inverse=True, coset=True), lg


@pytest.mark.parametrize("lg", [7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21])
def test_groth16_every_domain_size_verifies(ctx, zk, lg):
    """Setup + prove + pairing-verify at every domain size between the golden 2^7 and 2^21: crosses the
    one/two/three-pass NTT plans and every shared-bucket digit width (c = log2 n clamped to 6..22)."""
    r1 = zk.shielder_r1cs(lg)
    z = zk.shielder_witness(lg, 900 + lg)
    rng = ec.SplitMix64(70 + lg)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    proof = ctx.groth16_prove(pk, z, ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr()))
    publics = z[32 : 32 * r1.n_pub]
    assert zk.groth16_verify(vk, publics, proof) is True
    bad = bytearray(publics)
    bad[33] ^= 1
    assert zk.groth16_verify(vk, bytes(bad), proof) is False
    pk.free()
    r1.free()


def test_poseidon_merkle_paths_and_roots_on_device(ctx, zk):
    """Note tree on the device -> paths of chosen leaves -> (a) the batch root kernel recomputes the
    tree's root for every path, (b) the oracle agrees, (c) the paths feed the update_note witness
    generator, whose public merkle_root is then the root of the device-built tree."""
    import torch
    from oracle import poseidon as ps

    lg = 10  # TREE_HEIGHT of the relation
    n = 1 << lg
    rng = ec.SplitMix64(4711)
    # leaf 77 is a real old note; the others are arbitrary field elements
    tok = [rng.fr(), rng.fr()]
    bal = [500, 9]
    old_id, ot, on = rng.fr(), rng.fr(), rng.fr()
    old_acc = ps.hash_fix_len([tok[0], bal[0], tok[1], bal[1]])
    leaves = [rng.fr() for _ in range(n)]
    leaves[77] = ps.hash_fix_len([old_id, ot, on, old_acc])
    nodes = torch.zeros((2 * n - 1, 32), dtype=torch.uint8, device="cuda")
    nodes[:n] = torch.frombuffer(bytearray(frs(leaves)), dtype=torch.uint8).view(n, 32).cuda()
    torch.cuda.synchronize()
    ctx.poseidon_merkle_tree_dev(nodes.data_ptr(), lg)
    root = int.from_bytes(bytes(nodes[-1].cpu().numpy().tobytes()), "little")
    idx = [77, 0, 1, 1023, 512, 333]
    shape, paths = ctx.poseidon_merkle_paths_dev(nodes.data_ptr(), lg, idx)
    for k, i in enumerate(idx):
        sh = list(shape[lg * k : lg * (k + 1)])
        pa = unfrs(paths[32 * lg * k : 32 * lg * (k + 1)])
        assert sh == [1 - ((i >> lv) & 1) for lv in range(lg)]
        assert ps.merkle_root(leaves[i], sh, pa) == root
    d_leaves = torch.frombuffer(bytearray(frs([leaves[i] for i in idx])), dtype=torch.uint8).cuda()
    d_shape = torch.frombuffer(bytearray(shape), dtype=torch.uint8).cuda()
    d_paths = torch.frombuffer(bytearray(paths), dtype=torch.uint8).cuda()
    d_roots = torch.zeros(32 * len(idx), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.poseidon_merkle_roots_dev(d_leaves.data_ptr(), d_shape.data_ptr(), d_paths.data_ptr(), lg, len(idx), d_roots.data_ptr())
    assert unfrs(bytes(d_roots.cpu().numpy().tobytes())) == [root] * len(idx)
    # a wrong sibling gives a different root
    bad = bytearray(paths)
    bad[5] ^= 1
    d_bad = torch.frombuffer(bad, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    ctx.poseidon_merkle_roots_dev(d_leaves.data_ptr(), d_shape.data_ptr(), d_bad.data_ptr(), lg, len(idx), d_roots.data_ptr())
    got = unfrs(bytes(d_roots.cpu().numpy().tobytes()))
    assert got[0] != root and got[1:] == [root] * (len(idx) - 1)
    # the path of leaf 77 drives the relation's witness generator
    user, nt, nn, new_id = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    inp = zk.note_update(40, tok[0], user, (new_id, nt, nn), (old_id, ot, on), list(shape[:lg]), unfrs(paths[: 32 * lg]), user,
                         (tok[0], bal[0], tok[1], bal[1]))
    _, pub, rc = zk.update_note_witness(14, 1, inp)
    assert rc == 0 and pub[4] == root


def test_c_example_proves_and_verifies(tmp_path):
    """examples/prove_withdraw.c (plain C against include/zkmi.h) on the GPU: proof verified, tampered
    public input rejected, impossible update reported with the mock's error code."""
    import subprocess

    from test_cpu_host import _build_c_example

    p = subprocess.run([_build_c_example(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "proof of the withdraw: verified" in p.stdout
    assert "amount tampered: rejected" in p.stdout
    assert "-> -6 (ZKMI_ERR_ACCOUNT_UPDATE = -6)" in p.stdout


def test_c_bench_under_the_native_runtime_matches_the_python_path(ctx, zk, tmp_path):
    """examples/bench_prove.c in a fresh process WITHOUT Python or PyTorch: libzkmi.so bound to the /opt/rocm runtime it
    was built for (every other GPU test runs on the PyTorch wheel's bundled HIP runtime, which the binding preloads).
    Short form of profiles/r05's run: 6 + 1 proofs at 2^14 from device-generated assignments, every proof verified by
    pairing inside the program, 80 churn operations (setups 2^13..2^17, forced group sizes, batches, single and
    host-witness proofs, error path, MSMs, NTTs, second contexts); the dumped proof bytes must equal this process's
    proofs from the same seeds."""
    import json
    import subprocess

    import bench
    from test_cpu_host import _build_c_bench

    exe = _build_c_bench(tmp_path)
    dump = str(tmp_path / "proofs.bin")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZKMI_")}
    p = subprocess.run([exe, "--log-n", "14", "--proofs", "6", "--warmup", "1", "--churn", "80", "--dump", dump], capture_output=True,
                       text=True, timeout=1200, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "same release" in p.stdout and "clean" in p.stdout
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert line["failed"] == 0 and line["verified_by_pairing"] == 7 and line["hip_build"] // 100000 == line["hip_runtime"] // 100000
    # the same seven proofs through the Python binding (bench.py's generator: seeds 0x5A4B0000 + i, toxic + (r, s) drawn
    # from SplitMix64(0x5A4B0001))
    r1, wits = bench.relation_and_witness(zk, "poseidon", 14, [0x5A4B0000 + i for i in range(7)])
    rng = bench.SplitMix64(0x5A4B0001)
    toxic = b"".join(rng.fr_bytes() for _ in range(5))
    pk, vk = ctx.groth16_setup(r1, toxic)
    want = b""
    for w in wits:
        r, s = rng.fr_bytes(), rng.fr_bytes()
        want += ctx.groth16_prove(pk, w, r, s)
    pk.free()
    r1.free()
    assert open(dump, "rb").read() == want


# ---- the headline configuration inside the suite (BASELINE configs 1 and 2) ----------------------


@pytest.fixture(scope="module")
def key_2p20(ctx, zk):
    """update_note (withdraw, Poseidon-5) at N = 2^20: relation, resident key, verifying key."""
    r1 = zk.update_note_r1cs(20, 1)
    rng = ec.SplitMix64(0x5A4B2020)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    yield r1, pk, vk
    pk.free()
    r1.free()


def test_groth16_2p20_poseidon_relation_proof(ctx, zk, key_2p20):
    """BASELINE config 1's size with the real relation: a 2^20-constraint update_note proof from a host
    witness verifies against publics the oracle's Poseidon computed independently; every tampered public
    input is rejected."""
    from test_cpu_host import _note_update_case

    r1, pk, vk = key_2p20
    assert (r1.n_vars, r1.n_constraints + r1.n_pub, r1.log_n) == (1 << 20, 1 << 20, 20)
    inp, publics = _note_update_case(zk, 2020, 1, amount=123, balances=(1000, 7), slot=0)
    wit, pub, rc = zk.update_note_witness(20, 1, inp)
    assert rc == 0 and pub == publics
    rng = ec.SplitMix64(77)
    proof = ctx.groth16_prove(pk, wit, ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr()))
    assert zk.groth16_verify(vk, frs(publics), proof) is True
    for k in range(6):
        bad = list(publics)
        bad[k] = (bad[k] + 1) % R
        assert zk.groth16_verify(vk, frs(bad), proof) is False


def test_groth16_batch_of_8_at_2p20_device_resident(ctx, zk, key_2p20):
    """BASELINE config 2's per-GPU share (and drink_tests/mod.rs:133-207's 8 actors): 8 withdraw instances,
    assignments generated on the device, proved as one pipelined batch straight from HBM; every proof
    verifies against its own oracle-computed publics and equals one-at-a-time proving byte for byte."""
    import torch
    from test_cpu_host import _note_update_case

    r1, pk, vk = key_2p20
    n = 1 << 20
    cases = [_note_update_case(zk, 8000 + i, 1, amount=1 + i, balances=(50 + i, 3), slot=0) for i in range(8)]
    bufs = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in cases]
    torch.cuda.synchronize()
    assert ctx.update_note_witness_batch_dev(20, 1, [c[0] for c in cases], [b.data_ptr() for b in bufs]) == [0] * 8
    rng = ec.SplitMix64(8181)
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(8)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(8)]
    proofs = ctx.groth16_prove_batch_dev(pk, [b.data_ptr() for b in bufs], rs, ss)
    assert len(set(proofs)) == 8
    for (_, publics), pf in zip(cases, proofs):
        assert zk.groth16_verify(vk, frs(publics), pf) is True
    assert zk.groth16_verify(vk, frs(cases[1][1]), proofs[0]) is False
    for i in (0, 3, 7):
        assert ctx.groth16_prove_dev(pk, bufs[i].data_ptr(), rs[i], ss[i]) == proofs[i]
    # the host-witness entry point gives the same bytes as the device-resident one
    w0, _, _ = zk.update_note_witness(20, 1, cases[0][0])
    assert ctx.groth16_prove(pk, w0, rs[0], ss[0]) == proofs[0]


def test_prover_reports_unsatisfied_assignments(ctx, zk, pkg):
    """A witness that does not satisfy the relation (an impossible withdraw; a corrupted variable; z[0] != 1)
    yields ZKMI_ERR_UNSATISFIED from every prove entry point instead of an unverifiable proof, also from
    inside a pipelined batch, and the context stays usable."""
    import copy
    import ctypes as C
    import torch
    from test_cpu_host import _note_update_case

    lg = 14
    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(31337)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    good_inp, publics = _note_update_case(zk, 5150, 1)
    good, _, _ = zk.update_note_witness(lg, 1, good_inp)
    bad_inp = copy.deepcopy(good_inp)
    C.memmove(bad_inp.amount, (10**9).to_bytes(32, "little"), 32)
    under, _, rc = zk.update_note_witness(lg, 1, bad_inp, check=False)
    assert rc == -6
    flipped = bytearray(good)
    flipped[32 * 5000] ^= 1
    not_one = (2).to_bytes(32, "little") + good[32:]
    r_, s_ = ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr())
    for w in (under, bytes(flipped), not_one):
        with pytest.raises(pkg.ZkmiError) as e:
            ctx.groth16_prove(pk, w, r_, s_)
        assert e.value.code == -8
    d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in (good, under, good)]
    torch.cuda.synchronize()
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.groth16_prove_batch_dev(pk, [t.data_ptr() for t in d], [r_] * 3, [s_] * 3)
    assert e.value.code == -8
    proof = ctx.groth16_prove_dev(pk, d[0].data_ptr(), r_, s_)
    assert zk.groth16_verify(vk, frs(publics), proof) is True
    pk.free()
    r1.free()


def test_setup_matches_cpp_oracle_at_2p16(ctx, zk):
    """The product's trusted setup against the C++ oracle's own setup (arkworks generator shape, pinned to the
    Python oracle at N = 128 in the CPU suite) at N = 2^16 with the Poseidon relation: verifying key and all
    five queries byte for byte; then the oracle prover over the ORACLE's key and the GPU prover over the
    PRODUCT's key give the same 192 bytes."""
    from oracle import cpp as ocpp
    from test_cpu_host import _note_update_case

    ocpp.build()
    lg = 16
    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(161616)
    toxic = frs([rng.fr() for _ in range(5)])
    pk, vk = ctx.groth16_setup(r1, toxic)
    mats = [r1.export(m) for m in range(3)]
    ovk, okey = ocpp.groth16_setup(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, toxic)
    assert vk == ovk
    n, N = r1.n_vars, 1 << lg
    for which, name, cnt in ((0, "a_query", n), (1, "b_g1_query", n), (2, "b_g2_query", n), (3, "h_query", N - 1),
                             (4, "l_query", n - r1.n_pub)):
        assert pk.export_query(which, 0, cnt) == okey[name], name
    inp, publics = _note_update_case(zk, 1616, 1)
    wit, _, _ = zk.update_note_witness(lg, 1, inp)
    r_, s_ = ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr())
    want = ocpp.groth16_prove(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, okey, wit, r_, s_)
    assert ctx.groth16_prove(pk, wit, r_, s_) == want
    assert zk.groth16_verify(ovk, frs(publics), want) is True
    pk.free()
    r1.free()


def test_update_note_relation_other_tree_height_on_device(ctx, zk):
    """tree_height as a run-time field on the device path: the batch kernel at height 20 equals the host
    generator, a mixed-height batch is refused, and the proof verifies."""
    import torch
    from test_cpu_host import _note_update_case

    lg, height = 15, 20
    r1 = zk.update_note_r1cs(lg, 1, tree_height=height)
    cases = [_note_update_case(zk, 6100 + i, 1, height=height) for i in range(3)]
    bufs = [torch.zeros(32 << lg, dtype=torch.uint8, device="cuda") for _ in cases]
    torch.cuda.synchronize()
    assert ctx.update_note_witness_batch_dev(lg, 1, [c[0] for c in cases], [b.data_ptr() for b in bufs]) == [0] * 3
    for (inp, _), buf in zip(cases, bufs):
        assert bytes(buf.cpu().numpy().tobytes()) == zk.update_note_witness(lg, 1, inp)[0]
    mixed = [cases[0][0], _note_update_case(zk, 1, 1)[0]]
    with pytest.raises(Exception):
        ctx.update_note_witness_batch_dev(lg, 1, mixed, [bufs[0].data_ptr(), bufs[1].data_ptr()])
    rng = ec.SplitMix64(2323)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    proof = ctx.groth16_prove_dev(pk, bufs[2].data_ptr(), ec.fr_to_bytes(rng.fr()), ec.fr_to_bytes(rng.fr()))
    assert zk.groth16_verify(vk, frs(cases[2][1]), proof) is True
    pk.free()
    r1.free()


def _run_multigpu(nproc, extra):
    import json
    import os
    import socket
    import subprocess
    import sys

    from conftest import ROOT

    if "--one-gpu" in extra:  # the all-gather double for ranks that share a GPU (tests/fake_rccl/fake_rccl.cpp)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], stdout=subprocess.DEVNULL)

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "scripts", "run_multigpu.py")] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def test_multigpu_script_world1():
    """scripts/run_multigpu.py under torch.distributed.run with one rank (RCCL group of size 1): config 2
    (sharded proofs, all verified, gathered) and config 3 (point-split MSM == closed form) execute on hardware."""
    out = _run_multigpu(1, ["--log-n", "16", "--proofs", "6", "--msm-log-n", "20"])
    c2, c3 = out[0], out[1]
    assert c2["config"] == 2 and c2["all_verified"] and c2["proofs_gathered"] == 6
    assert c3["config"] == 3 and c3["matches_closed_form_on_every_rank"]
    # the exchange behind the C ABI (zkmi_comm + zkmi_msm_g1_allgather_combine over RCCL) == the Python exchange == closed form
    by = {o.get("workload", ""): o for o in out}
    assert next(o for w, o in by.items() if "zkmi_msm_g1_allgather_combine" in w)["matches_closed_form_and_python_path_on_every_rank"]
    # BASELINE configs[3] as worded: the windows split over the ranks
    assert next(o for w, o in by.items() if "WINDOWS split" in w)["matches_closed_form_on_every_rank"]


def test_rccl_exchange_behind_the_c_abi_world1(ctx, zk):
    """zkmi_comm_unique_id / zkmi_comm_init / zkmi_msm_g1_allgather_combine in THIS process (a world of one rank, no
    torch.distributed involved): the RCCL all-gather of the device-resident partial sums + combination gives the plain
    MSM's result, under the 16-bit plan and under the partitioned 20-bit plan of a 2^24-term global size."""
    import torch

    n = (1 << 17) + 77
    raw, tot, wtot = _torch_scalars(n, 21)
    b = ctx.bases_g1_synthetic(n)
    want = ctx.msm_g1_dev(raw.data_ptr(), n, b)
    assert want == _closed_form_g1(tot, wtot)
    comm = ctx.comm_init(1, 0, zk.comm_unique_id())
    assert ctx.msm_g1_allgather_combine(comm, raw.data_ptr(), n, b, n) == want
    assert ctx.msm_g1_allgather_combine(comm, raw.data_ptr(), n, b, 1 << 24) == want
    comm.free()
    b.free()


def test_msm_g1_window_split_matches_full(ctx, zk):
    """BASELINE configs[3] as worded -- the WINDOWS of one MSM split over the ranks, every rank over all points: two
    window ranges computed separately (zkmi_msm_g1_window_range_dev) and concatenated give the unsplit MSM, under the
    16-bit plan (16 windows) and under the partitioned 20-bit plan of a 2^24-term size (13 windows; the range that holds
    the top window exercises its partition spread); and the collective form over a one-rank zkmi_comm."""
    n = (1 << 17) + 5
    raw, tot, wtot = _torch_scalars(n, 31)
    b = ctx.bases_g1_synthetic(n)
    want = ctx.msm_g1_dev(raw.data_ptr(), n, b)
    assert want == _closed_form_g1(tot, wtot)
    for plan_n, cut in ((n, 5), (1 << 24, 7), (1 << 24, 12)):
        nwin = zk.msm_plan_query(plan_n)[2]
        lo, tot_w, cb = ctx.msm_g1_window_range_dev(raw.data_ptr(), n, b, plan_n, 0, cut)
        hi, tot_w2, cb2 = ctx.msm_g1_window_range_dev(raw.data_ptr(), n, b, plan_n, cut, nwin - cut)
        assert (tot_w, cb) == (tot_w2, cb2) == (nwin, zk.msm_plan_query(plan_n)[0])
        zero = bytes(96)
        ranks = lo + zero * (nwin - cut) + zero * cut + hi  # rank 0 owns [0, cut), rank 1 the rest; infinity elsewhere
        assert zk.msm_g1_combine(ranks, 2, nwin, cb) == want, (plan_n, cut)
    comm = ctx.comm_init(1, 0, zk.comm_unique_id())
    assert ctx.msm_g1_window_split_allgather(comm, raw.data_ptr(), n, b) == want
    comm.free()
    b.free()


def test_multigpu_script_world2():
    """The same with two ranks over RCCL (BASELINE configs 2 and 3); needs two GPUs on the box."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (the driver's multi-GPU box); the gloo world-2 test covers the exchange on CPU")
    out = _run_multigpu(2, ["--log-n", "16", "--proofs", "6", "--msm-log-n", "20"])
    assert out[0]["all_verified"] and out[0]["proofs_gathered"] == 6 and out[0]["n_gpus"] == 2
    assert out[1]["matches_closed_form_on_every_rank"] and out[1]["n_gpus"] == 2
    by = {o.get("workload", ""): o for o in out}
    a = next(o for w, o in by.items() if "zkmi_msm_g1_allgather_combine" in w)
    assert a["matches_closed_form_and_python_path_on_every_rank"] and a["n_gpus"] == 2
    assert next(o for w, o in by.items() if "WINDOWS split" in w)["matches_closed_form_on_every_rank"]


@pytest.mark.parametrize("world", [2, 4, 8])
def test_multigpu_script_ranks_sharing_one_gpu(world):
    """Ranks > 0 on hardware.  The pool has one GPU per box and RCCL refuses two ranks on one device, so the multi-rank legs
    never ran: here `world` processes share GPU 0, torch.distributed runs over gloo and libzkmi's exchange over the
    all-gather double of tests/fake_rccl (ZKMI_RCCL_LIB).  Everything else is the product path of BASELINE configs 2 and 3:
    every rank proves its share of the proofs (all verified, all gathered), owns its slice of the 2^20-point MSM under the
    plan of the global size, exchanges its partial sums through zkmi_comm (point split, window split with ranks that own
    one, two or NO window at world 8 x 16 windows ... ) and combines; every rank must reach the closed form."""
    out = _run_multigpu(world, ["--one-gpu", "--log-n", "14", "--proofs", str(3 * world + 1), "--msm-log-n", "20"])
    c2 = out[0]
    assert c2["config"] == 2 and c2["all_verified"] and c2["proofs_gathered"] == 3 * world + 1 and c2["ranks"] == world
    assert all(o["ranks"] == world and o["n_gpus"] == 1 for o in out)
    by = {o.get("workload", ""): o for o in out}
    assert out[1]["config"] == 3 and out[1]["matches_closed_form_on_every_rank"]
    assert next(o for w, o in by.items() if "zkmi_msm_g1_allgather_combine" in w)["matches_closed_form_and_python_path_on_every_rank"]
    assert next(o for w, o in by.items() if "WINDOWS split" in w)["matches_closed_form_on_every_rank"]
    assert next(o for w, o in by.items() if "prepared bases" in w)["matches_closed_form_on_every_rank"]
    # round 6: the 2-D split (point groups x 2 window ranges) on the same slices
    assert next(o for w, o in by.items() if "2-D split" in w)["matches_closed_form_on_every_rank"]


def test_exchange_under_the_big_window_plan_with_ranks_sharing_one_gpu():
    """The same with the plan of BASELINE config 3's size: 4 ranks, 2^24 points (the partitioned 20-bit windows: 13 windows
    x 16 partial sums per rank, the top window spread over its partitions)."""
    out = _run_multigpu(4, ["--one-gpu", "--config", "3", "--msm-log-n", "24"])
    assert all(o.get("matches_closed_form_on_every_rank", o.get("matches_closed_form_and_python_path_on_every_rank")) for o in out)
    assert all(o["ranks"] == 4 for o in out) and len(out) >= 3


@pytest.mark.parametrize("window_groups", [2, 4])
def test_2d_split_under_the_big_window_plan_at_world_8(window_groups):
    """BASELINE configs[3] at its rank count: 8 ranks as 4 point groups x 2 window ranges and as 2 x 4
    (zkmi_msm_g1_split2d_allgather), 2^24 points under their own plan -- the partitioned 20-bit windows, 13 windows, so the
    ranges own 6 + 7 resp. 3 + 3 + 3 + 4 windows and the spread top window sits in the last range -- over the all-gather
    double; every rank must reach the closed form.  (Ranks share GPU 0: nothing here says anything about RCCL or xGMI.)"""
    # (only the 2-D leg: eight contexts with the workspaces of a 2^24 plan -- 12 bucket arrays of 13 x 2^19 buckets each -- already
    # take most of the one GPU they share)
    out = _run_multigpu(8, ["--one-gpu", "--config", "3", "--msm-log-n", "24", "--window-groups", str(window_groups), "--legs", "2d"])
    two_d = [o for o in out if "2-D split" in o.get("workload", "")]
    assert len(two_d) == 1 and two_d[0]["matches_closed_form_on_every_rank"] and two_d[0]["ranks"] == 8
    assert "%d point groups x %d window ranges" % (8 // window_groups, window_groups) in two_d[0]["workload"]


def test_arkworks_key_layout_load_and_write(ctx, zk):
    """Proving key through arkworks' CanonicalSerialize layout (csrc/arkworks.hip vs oracle/ark_serialize.py, both
    restated from memory: oracle/README.md rows 8, 10): the oracle's setup serialised by the Python restatement loads
    into a resident key that proves byte-identically to the directly loaded key; writing it back reproduces the blob."""
    from oracle import ark_serialize as ark
    from oracle import cpp as ocpp

    gd = golden("groth16_n128.json")
    r1 = zk.shielder_r1cs(gd["log_n"])
    key = {k: H(v) for k, v in gd["pk"].items()}
    vk = H(gd["vk"])
    z = H(gd["witness"])
    for compressed in (False, True):
        blob = ark.proving_key(vk, r1.n_pub, key, compressed)
        pk, vk_back = ctx.ark_pk_load(r1, blob, compressed)
        assert vk_back == vk
        assert ctx.groth16_prove(pk, z, H(gd["r"]), H(gd["s"])) == H(gd["proof"])
        assert ctx.ark_pk_write(pk, vk, compressed) == blob
        pk.free()
    r1.free()


@pytest.mark.parametrize("sub", ["arkworks", "arkworks_2p13"])
def test_arkworks_fixture_if_present(ctx, zk, sub):
    """Consumes what integration/ark_fixture (a Rust program a maintainer with cargo builds; it cannot be built in
    this image) writes to tests/golden/arkworks/: the relation, an ark-groth16 proving key, the witness, (r, s) and
    arkworks' own proof.  With it, proof bytes are pinned against the real arkworks prover; without it this test
    skips and parity stays unpinned (oracle/README.md)."""
    import os

    from conftest import ROOT

    d = os.path.join(ROOT, "tests", "golden", sub)
    need = ["relation.bin", "pk_uncompressed.bin", "witness.bin", "rs.bin", "proof.bin"]
    if not all(os.path.exists(os.path.join(d, f)) for f in need):
        pytest.skip("no arkworks fixture under tests/golden/arkworks (build integration/ark_fixture with cargo to create it)")
    rd = lambda f: open(os.path.join(d, f), "rb").read()
    rel = rd("relation.bin")
    n_vars, n_pub, nc = (int.from_bytes(rel[4 * i : 4 * i + 4], "little") for i in range(3))
    off, mats = 12, []
    for _ in range(3):
        rowptr = [int.from_bytes(rel[off + 4 * i : off + 4 * i + 4], "little") for i in range(nc + 1)]
        off += 4 * (nc + 1)
        nnz = rowptr[-1]
        col = [int.from_bytes(rel[off + 4 * i : off + 4 * i + 4], "little") for i in range(nnz)]
        off += 4 * nnz
        mats.append((rowptr, col, rel[off : off + 32 * nnz]))
        off += 32 * nnz
    r1 = zk.r1cs_create(n_vars, n_pub, mats)
    pk, vk = ctx.ark_pk_load(r1, rd("pk_uncompressed.bin"), False)
    rs = rd("rs.bin")
    wit = rd("witness.bin")
    proof = ctx.groth16_prove(pk, wit, rs[:32], rs[32:64])
    assert proof == rd("proof.bin"), "proof bytes differ from ark-groth16's"
    assert zk.groth16_verify(vk, wit[32 : 32 * n_pub], proof) is True
    pk.free()
    r1.free()


def test_soak_script_short_run():
    """scripts/soak.py (the same batches proved over and over must give the same bytes; partial groups and single
    proofs interleaved) in a short configuration; the long run is `python scripts/soak.py`."""
    import subprocess
    import sys

    from conftest import ROOT

    p = subprocess.run([sys.executable, "scripts/soak.py", "8", "3"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "SOAK OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_grouped_small_domain_prover_matches_one_by_one(ctx, zk):
    """Small domains (the relation's natural size, BASELINE config 0): the batch entry point proves up to 64 proofs as
    ONE group (one digit sort, one accumulation launch per query, batched NTT passes).  70 proofs at N = 2^13 (two
    groups, the second partial) must equal, byte for byte, a key that never groups (zkmi_ctx_set_group_size 1) and verify."""
    import os

    import torch
    from test_cpu_host import _note_update_case

    lg, count = 13, 70
    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(1313)
    toxic = frs([rng.fr() for _ in range(5)])
    cases = [_note_update_case(zk, 4000 + i, 1, amount=1 + i % 7, balances=(100 + i, 9)) for i in range(count)]
    bufs = [torch.zeros(32 << lg, dtype=torch.uint8, device="cuda") for _ in cases]
    torch.cuda.synchronize()
    for k in range(0, count, 32):
        chunk = list(range(k, min(count, k + 32)))
        assert ctx.update_note_witness_batch_dev(lg, 1, [cases[i][0] for i in chunk], [bufs[i].data_ptr() for i in chunk]) == [0] * len(chunk)
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(count)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(count)]
    pk, vk = ctx.groth16_setup(r1, toxic)
    grouped = ctx.groth16_prove_batch_dev(pk, [b.data_ptr() for b in bufs], rs, ss)
    pk.free()
    ctx.set_group_size(1)
    try:
        pk1, vk1 = ctx.groth16_setup(r1, toxic)
    finally:
        ctx.set_group_size(0)
    assert vk1 == vk
    single = ctx.groth16_prove_batch_dev(pk1, [b.data_ptr() for b in bufs], rs, ss)
    pk1.free()
    assert grouped == single
    for (_, publics), pf in zip(cases, grouped):
        assert zk.groth16_verify(vk, frs(publics), pf) is True
    r1.free()


@pytest.mark.parametrize("lg,count", [(14, 48), (15, 21), (16, 9), (17, 11), (18, 7), (19, 5)])
def test_grouped_prover_partial_groups(ctx, zk, lg, count):
    """Groups smaller than the key's capacity (they use more histogram tiles per proof) at every grouped size
    (from 2^17 on a proof owns several 2^15-bucket partitions of the group's bucket array):
    each proof verifies and equals the single-proof entry point."""
    import torch
    from test_cpu_host import _note_update_case

    r1 = zk.update_note_r1cs(lg, 1)
    rng = ec.SplitMix64(500 + lg)
    pk, vk = ctx.groth16_setup(r1, frs([rng.fr() for _ in range(5)]))
    cases = [_note_update_case(zk, 70 * lg + i, 1) for i in range(3)]
    wits = [zk.update_note_witness(lg, 1, c[0])[0] for c in cases]
    d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
    torch.cuda.synchronize()
    idx = [i % 3 for i in range(count)]
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(count)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(count)]
    proofs = ctx.groth16_prove_batch_dev(pk, [d[j].data_ptr() for j in idx], rs, ss)
    for i in (0, count // 2, count - 1):
        assert zk.groth16_verify(vk, frs(cases[idx[i]][1]), proofs[i]) is True
        assert ctx.groth16_prove_dev(pk, d[idx[i]].data_ptr(), rs[i], ss[i]) == proofs[i]
    # the host-witness entry point (uploads on the copy stream, group by group) gives the same bytes
    hw = [torch.frombuffer(bytearray(w), dtype=torch.uint8).pin_memory() for w in wits]
    assert ctx.groth16_prove_batch_host(pk, [hw[j].data_ptr() for j in idx], rs, ss) == proofs
    pk.free()
    r1.free()


def test_groth16_witness_of_bits_and_edge_blinding_factors_vs_cpp_oracle(ctx, zk):
    """The B1 MSM is taken over r z and enters the proof through the reduction L and H share (groth16.hip, "r B1 fold"):
    proof bytes against the C++ oracle's prover for r in {0, 1, r_mod - 1, random} on a relation of bit constraints --
    every 1 of the witness becomes the SAME full-width scalar r (one heavy bucket per digit position), every 0 stays 0,
    r = 0 empties the B1 MSM altogether -- through the single-proof call (no fold), the grouped batch and the batch of
    one-proof groups (what a 2^20 key runs).  Such a witness is also the one the prover stops folding for."""
    import random

    import torch
    from oracle import cpp as ocpp

    ocpp.build()
    one = (1).to_bytes(32, "little")
    nbits, n_pub = 3000, 2
    n_vars = n_pub + nbits + 40  # 1, the public count of ones, the bits, a tail of full-width values
    rnd = random.Random(77)
    bits = [1 if rnd.random() < 0.6 else 0 for _ in range(nbits)]
    tail = [rnd.randrange(R) for _ in range(40)]
    zv = [1, sum(bits) % R] + bits + tail
    # rows: b_i * b_i = b_i;  (sum b_i) * 1 = z[1];  t_k * 1 = t_k
    a_rp, a_c, b_rp, b_c, c_rp, c_c = [0], [], [0], [], [0], []
    for i in range(nbits):
        a_c.append(n_pub + i), b_c.append(n_pub + i), c_c.append(n_pub + i)
        a_rp.append(len(a_c)), b_rp.append(len(b_c)), c_rp.append(len(c_c))
    a_c += [n_pub + i for i in range(nbits)]
    b_c.append(0), c_c.append(1)
    a_rp.append(len(a_c)), b_rp.append(len(b_c)), c_rp.append(len(c_c))
    for k in range(40):
        a_c.append(n_pub + nbits + k), b_c.append(0), c_c.append(n_pub + nbits + k)
        a_rp.append(len(a_c)), b_rp.append(len(b_c)), c_rp.append(len(c_c))
    mats = [(rp, cl, one * len(cl)) for rp, cl in ((a_rp, a_c), (b_rp, b_c), (c_rp, c_c))]
    wit = frs(zv)
    rng = ec.SplitMix64(0xB175)
    toxic = frs([rng.fr() for _ in range(5)])
    blind = [0, 1, R - 1, rng.fr(), 0, rng.fr(), 1]
    rs = [ec.fr_to_bytes(v) for v in blind]
    ss = [ec.fr_to_bytes(v) for v in (rng.fr(), 0, rng.fr(), R - 1, 0, 1, rng.fr())]
    r1 = zk.r1cs_create(n_vars, n_pub, mats)
    assert r1.is_satisfied(wit)
    ovk, okey = ocpp.groth16_setup(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, toxic)
    want = [ocpp.groth16_prove(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, okey, wit, r_, s_) for r_, s_ in zip(rs, ss)]
    d = torch.frombuffer(bytearray(wit), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for group in (0, 1):
        ctx.set_group_size(group)
        pk, vk = ctx.groth16_setup(r1, toxic)
        ctx.set_group_size(0)
        assert vk == ovk
        # the batch FIRST: a fresh key folds until the first finished proof has reported how few of its digits this witness
        # fills (groth16.hip fold_dense) -- the proofs in flight by then are the ones with r = 0, 1, r_mod - 1
        assert ctx.groth16_prove_batch_dev(pk, [d.data_ptr()] * len(rs), rs, ss) == want
        assert [ctx.groth16_prove_dev(pk, d.data_ptr(), r_, s_) for r_, s_ in zip(rs, ss)] == want
        assert ctx.groth16_prove_batch_dev(pk, [d.data_ptr()] * len(rs), rs, ss) == want  # and without the fold
        pk.free()
    assert all(zk.groth16_verify(ovk, wit[32: 32 * n_pub], p) for p in want)
    r1.free()


def test_fold_decision_follows_the_digit_density(ctx, zk):
    """The prover folds B1 into the L + H reduction only while the assignments of a key fill at least 9 in 10 of their digits
    (groth16.hip note_density).  The count comes from the digit sort of z -- on EVERY sort path: round 4's fine-partition
    sort (one-proof groups at 2^17 .. 2^21, the bench's path) never wrote it and the decision read stale memory.  Here:
    one-proof groups at 2^17 (the fine path), a relation any assignment satisfies (z_i * 1 = z_i), so ONE key sees a witness
    of bits and a dense one; the reported count must equal the host's count of non-zero signed digits both times."""
    import random

    import torch

    lg, n_pub = 17, 2
    n_vars = (1 << lg) - n_pub
    nc = n_vars - n_pub
    one = (1).to_bytes(32, "little")
    rp = list(range(nc + 1))
    cols = list(range(n_pub, n_vars))
    mats = [(rp, cols, one * nc), (rp, [0] * nc, one * nc), (rp, cols, one * nc)]
    r1 = zk.r1cs_create(n_vars, n_pub, mats)
    assert r1.log_n == lg
    c, nd = zk.msm_plan_query(n_vars - 1, shared=True)[:2]
    bias = sum(((1 << (c - 1)) - 1) << (c * w) for w in range(nd))
    live = nd - (1 if (nd - 1) * c >= 255 else 0)

    def nonzero_digits(vals):
        tot = 0
        for v in vals:
            k = v + bias
            for w in range(nd):
                tot += ((k >> (c * w)) & ((1 << c) - 1)) != (1 << (c - 1)) - 1
        return tot

    rnd = random.Random(1717)
    z_bits = [1, 1] + [1 if rnd.random() < 0.6 else 0 for _ in range(n_vars - 2)]
    z_dense = [1, 5] + [rnd.randrange(R) for _ in range(n_vars - 2)]
    rng = ec.SplitMix64(0xF01D)
    toxic = frs([rng.fr() for _ in range(5)])
    ctx.set_group_size(1)
    pk, vk = ctx.groth16_setup(r1, toxic)
    ctx.set_group_size(0)
    assert pk.schedule_state()[0] is True  # a fresh key folds
    rs = [ec.fr_to_bytes(rng.fr()) for _ in range(4)]
    ss = [ec.fr_to_bytes(rng.fr()) for _ in range(4)]
    full = (n_vars - 1) * live
    for zv, dense in ((z_bits, False), (z_dense, True), (z_bits, False)):
        wit = frs(zv)
        d = torch.frombuffer(bytearray(wit), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        proofs = ctx.groth16_prove_batch_dev(pk, [d.data_ptr()] * 4, rs, ss)
        assert zk.groth16_verify(vk, wit[32: 32 * n_pub], proofs[0]) and zk.groth16_verify(vk, wit[32: 32 * n_pub], proofs[-1])
        folding, entries, want_full = pk.schedule_state()
        assert want_full == full
        assert entries == nonzero_digits(zv[1:]), "the digit sort's count of non-zero digits differs from the host's"
        assert folding is dense
        # the bytes do not depend on the decision: the single-proof call never folds
        assert ctx.groth16_prove_dev(pk, d.data_ptr(), rs[0], ss[0]) == proofs[0]
    pk.free()
    r1.free()


def test_bn254_grand_product_matches_oracle(ctx, pkg):
    """zkmi_bn254_grand_product_dev (PLONK's z: batch inversion of the denominators + running product) against the oracle's
    chain for lengths around the block sizes (1 .. 1 030 terms; 8 per thread in the inversion kernel, 1 024 per block in the
    scan) and for 2^20 + 3 terms (all three levels); a permutation's product telescopes to 1; a zero denominator is refused."""
    import random

    import torch
    from oracle import bn254 as bn

    rnd = random.Random(2542)
    up = lambda v: torch.frombuffer(bytearray(_bn_frs(v)), dtype=torch.uint8).cuda()
    for n in (1, 2, 7, 8, 9, 513, 1023, 1024, 1025, 1030, (1 << 20) + 3):
        num = [rnd.randrange(bn.R) for _ in range(n)]
        den = [rnd.randrange(1, bn.R) for _ in range(n)]
        if n > 4:
            num[3], den[2] = 0 if n < 100 else 1, 1  # a zero numerator zeroes everything behind it
        dn, dd = up(num), up(den)
        out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        tot = ctx.bn254_grand_product_dev(dn.data_ptr(), dd.data_ptr(), n, out.data_ptr())
        z, last = bn.grand_product(num, den)
        assert out.cpu().numpy().tobytes() == _bn_frs(z), n
        assert tot == _bn_frs([last]), n
    # the permutation argument's shape: num_i = f(i), den_i = f(sigma(i)) -> the product over the whole domain is 1
    n = 4096
    vals = [rnd.randrange(1, bn.R) for _ in range(n)]
    sigma = list(range(n))
    rnd.shuffle(sigma)
    dn, dd = up(vals), up([vals[j] for j in sigma])
    out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.bn254_grand_product_dev(dn.data_ptr(), dd.data_ptr(), n, out.data_ptr()) == _bn_frs([1])
    dd = up([vals[j] if k != 77 else 0 for k, j in enumerate(sigma)])
    torch.cuda.synchronize()
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.bn254_grand_product_dev(dn.data_ptr(), dd.data_ptr(), n, out.data_ptr())
    assert e.value.code == -1


def test_random_relations_vs_cpp_oracle(ctx, zk):
    """Differential test on relations nobody designed: random sparse A and B rows (empty rows, rows that are one constant,
    rows of hundreds of terms and one of 1 500, variables no row mentions, zero and one and r - 1 among the values), C_i one
    product variable per row.  Setup (verifying key) and proof bytes against the C++ oracle's setup and prover from the same
    toxic waste, witness, r and s -- single proofs, grouped batches and one-proof groups."""
    import random

    import torch
    from oracle import cpp as ocpp

    ocpp.build()
    one = (1).to_bytes(32, "little")
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
            vals.append(a * b % R)  # the product variable of row i: column n_in + i
        n_vars = len(vals)
        mats = []
        for which in range(3):
            rp, cl, vl = [0], [], b""
            for i, (ac, av, bc, bv) in enumerate(rows):
                cols, cv = ((ac, av), (bc, bv), ([n_in + i], [1]))[which]
                cl += cols
                vl += b"".join(v.to_bytes(32, "little") for v in cv)
                rp.append(len(cl))
            mats.append((rp, cl, vl))
        r1 = zk.r1cs_create(n_vars, n_pub, mats)
        wit = frs(vals)
        assert r1.is_satisfied(wit)
        rng = ec.SplitMix64(0xABCD00 + seed)
        toxic = frs([rng.fr() for _ in range(5)])
        ovk, okey = ocpp.groth16_setup(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, toxic)
        rs = [ec.fr_to_bytes(rng.fr()) for _ in range(5)]
        ss = [ec.fr_to_bytes(rng.fr()) for _ in range(5)]
        want = [ocpp.groth16_prove(r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n, mats, okey, wit, r_, s_) for r_, s_ in zip(rs, ss)]
        d = torch.frombuffer(bytearray(wit), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        for group in (0, 1):
            ctx.set_group_size(group)
            pk, vk = ctx.groth16_setup(r1, toxic)
            ctx.set_group_size(0)
            assert vk == ovk, (seed, group)
            assert ctx.groth16_prove_batch_dev(pk, [d.data_ptr()] * 5, rs, ss) == want, (seed, group)
            assert ctx.groth16_prove_dev(pk, d.data_ptr(), rs[0], ss[0]) == want[0], (seed, group)
            assert ctx.groth16_prove(pk, wit, rs[1], ss[1]) == want[1], (seed, group)
            pk.free()
        assert zk.groth16_verify(ovk, wit[32: 32 * n_pub], want[0])
        bad = bytearray(wit)
        bad[32 * (n_in + 3)] ^= 1  # a wrong product variable: refused, not proved
        with pytest.raises(Exception):
            ctx2_pk, _ = ctx.groth16_setup(r1, toxic)
            try:
                ctx.groth16_prove(ctx2_pk, bytes(bad), rs[0], ss[0])
            finally:
                ctx2_pk.free()
        r1.free()


def test_bn254_polynomial_entry_points_refuse_bad_arguments(ctx, pkg):
    """The ABI promises an error code, not a crash: no coefficients, an SRS shorter than the quotient, null buffers."""
    import torch
    from oracle import bn254 as bn

    n = 40
    d = torch.frombuffer(bytearray(_bn_frs(list(range(1, n + 1)))), dtype=torch.uint8).cuda()
    out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    z = _bn_frs([5])
    short = ctx.bn254_bases_synthetic(n - 2)  # the quotient has n - 1 coefficients
    exact = ctx.bn254_bases_synthetic(n - 1)
    for call in (lambda: ctx.bn254_kzg_open_dev(d.data_ptr(), 0, z, exact),
                 lambda: ctx.bn254_kzg_open_dev(d.data_ptr(), n, z, short),
                 lambda: ctx.bn254_kzg_open_dev(0, n, z, exact),
                 lambda: ctx.bn254_grand_product_dev(d.data_ptr(), d.data_ptr(), 0, out.data_ptr()),
                 lambda: ctx.bn254_grand_product_dev(d.data_ptr(), 0, n, out.data_ptr()),
                 lambda: ctx.bn254_grand_product_dev(d.data_ptr(), d.data_ptr(), n, 0)):
        with pytest.raises(pkg.ZkmiError) as e:
            call()
        assert e.value.code == -1
    ev, pf = ctx.bn254_kzg_open_dev(d.data_ptr(), n, z, exact)  # the context is still usable, and n - 1 points suffice
    p = list(range(1, n + 1))
    assert ev == _bn_frs([bn.eval_polynomial(p, 5)])
    assert pf == bn.g1_to_bytes(bn.msm_naive(bn.kate_division(p, 5), bn.synthetic_bases(n - 1)))
    assert ctx.bn254_grand_product_dev(d.data_ptr(), d.data_ptr(), n, out.data_ptr()) == _bn_frs([1])
    short.free()
    exact.free()


def test_bits_relation_script_short():
    """scripts/bits_relation_ab.py (a witness of bits with a row that sums them all: the long-row mat-vec kernel, the heavy
    buckets of a one-value witness and the density switch of the B1 fold) proves and verifies at 2^12."""
    import subprocess
    import sys

    from conftest import ROOT

    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bits_relation_ab.py"), "12", "12", "sum"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "verified True" in p.stdout, p.stdout[-500:]


def test_bn254_kzg_open_many_matches_oracle(ctx, pkg):
    """zkmi_bn254_kzg_open_many_dev (k polynomials at one point: all evaluations + ONE proof for f = sum_j v^j p_j) against
    the oracle: k in {1, 3, 8} x lengths around the block size, v in {0, 1, random}; against an SRS with a known tau the proof
    is [q_f(tau)] G and satisfies the folded check (tau - z) q_f(tau) = sum_j v^j (p_j(tau) - p_j(z)); and three polynomials of
    2^20 + 3 coefficients (every level of the scan, one launch per level for all three)."""
    import torch
    from oracle import bn254 as bn

    rng = ec.SplitMix64(2543)
    fr = lambda: rng.next() * rng.next() * rng.next() * rng.next() % bn.R
    up = lambda vals: torch.frombuffer(bytearray(_bn_frs(vals)), dtype=torch.uint8).cuda()
    b = ctx.bn254_bases_synthetic(1030)
    for k in (1, 3, 8):
        for n in (1, 2, 300, 1024, 1027):
            polys = [[fr() for _ in range(n)] for _ in range(k)]
            d = [up(p) for p in polys]
            torch.cuda.synchronize()
            for z, v in ((fr(), fr()), (fr(), 0), (0, 1), (bn.R - 1, fr())):
                evs, pf = ctx.bn254_kzg_open_many_dev([t.data_ptr() for t in d], n, _bn_frs([z]), _bn_frs([v]), b)
                f = [0] * n
                for p in reversed(polys):
                    f = [(a * v + c) % bn.R for a, c in zip(f, p)]
                q = bn.kate_division(f, z)
                assert evs == [_bn_frs([bn.eval_polynomial(p, z)]) for p in polys], (k, n)
                kk = (sum(q) + 0xC0FFEE * sum(i * x for i, x in enumerate(q))) % bn.R
                assert pf == bn.g1_to_bytes(bn.pt_mul(bn.G1, kk)), (k, n)
                if k == 1:
                    assert (evs[0], pf) == ctx.bn254_kzg_open_dev(d[0].data_ptr(), n, _bn_frs([z]), b)
    b.free()
    tau, n, k = 0xDEADBEEFCAFEF00D1234567 % bn.R, 64, 5
    srs_pts = [bn.pt_mul(bn.G1, pow(tau, i, bn.R)) for i in range(n)]
    srs = ctx.bn254_bases(b"".join(bn.g1_to_bytes(x) for x in srs_pts))
    polys = [[fr() for _ in range(n)] for _ in range(k)]
    d = [up(p) for p in polys]
    z, v = fr(), fr()
    torch.cuda.synchronize()
    evs, pf = ctx.bn254_kzg_open_many_dev([t.data_ptr() for t in d], n, _bn_frs([z]), _bn_frs([v]), srs)
    want_evs, want_pf = bn.kzg_open_many(polys, z, v, srs_pts)
    assert evs == [_bn_frs([y]) for y in want_evs] and pf == bn.g1_to_bytes(want_pf)
    folded = sum(pow(v, j, bn.R) * (bn.eval_polynomial(p, tau) - y) for j, (p, y) in enumerate(zip(polys, want_evs))) % bn.R
    f = [sum(pow(v, j, bn.R) * p[i] for j, p in enumerate(polys)) % bn.R for i in range(n)]
    q_tau = bn.eval_polynomial(bn.kate_division(f, z), tau)
    assert (tau - z) * q_tau % bn.R == folded and pf == bn.g1_to_bytes(bn.pt_mul(bn.G1, q_tau))
    with pytest.raises(pkg.ZkmiError) as e:
        ctx.bn254_kzg_open_many_dev([], n, _bn_frs([z]), _bn_frs([v]), srs)
    assert e.value.code == -1
    srs.free()
    # full size
    n, k = (1 << 20) + 3, 3
    g = torch.Generator(device="cuda").manual_seed(2544)
    raws = []
    for _ in range(k):
        raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
        raw[:, 31] &= 0x1F
        raws.append(raw)
    hosts = [r.cpu().numpy().tobytes() for r in raws]
    polys = [[int.from_bytes(h[32 * i: 32 * i + 32], "little") for i in range(n)] for h in hosts]
    b = ctx.bn254_bases_synthetic(n - 1)
    torch.cuda.synchronize()
    evs, pf = ctx.bn254_kzg_open_many_dev([r.data_ptr() for r in raws], n, _bn_frs([z]), _bn_frs([v]), b)
    assert evs == [_bn_frs([bn.eval_polynomial(p, z)]) for p in polys]
    f = [0] * n
    for p in reversed(polys):
        f = [(a * v + c) % bn.R for a, c in zip(f, p)]
    q = bn.kate_division(f, z)
    kk = (sum(q) + 0xC0FFEE * sum(i * x for i, x in enumerate(q))) % bn.R
    assert pf == bn.g1_to_bytes(bn.pt_mul(bn.G1, kk))
    b.free()


def test_quad_split_addition_selftest(ctx, zk):
    """csrc/quad.hpp -- the complete XYZZ addition with one coordinate per lane of a quad (the segment sums, tree sums, redo
    pass and heavy-bucket sums of the G1 MSM run on it: csrc/msm_quad.hpp) -- against curve.hpp's one-lane addition on the
    device and the host's 32-bit-limb arithmetic: 4 096 pairs with every special case (o = a and o = -a in the same and in
    another representation, either operand at infinity, both), and 16-point sums over the quads of a wave from XYZZ and
    from affine sources (signs, entries at infinity, a doubling and a cancellation inside the tree).  Three instantiations,
    4 096 pairs each: BLS12-381 G1 quads, G2 octets, and the quads of the 10-limb BN254 field (csrc/msm_bn.hip)."""
    import ctypes as C

    bad = C.c_uint32(99)
    assert zk.tlib.zkmi_selftest_quad_add(ctx.h, C.c_uint64(0xA11CE), C.c_uint32(4096), C.byref(bad)) == 0
    assert bad.value == 0
