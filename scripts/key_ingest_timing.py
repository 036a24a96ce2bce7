#!/usr/bin/env python3
"""Key ingest on the device, timed (csrc/points.hip; DESIGN.md "Key ingest"; results in profiles/r07/key_ingest.txt).

    python scripts/key_ingest_timing.py kernels          # each kernel family alone, 2^20 G1 / 2^18 G2 points
    python scripts/key_ingest_timing.py keys 13 16       # compressed update_note keys: host path against the device path
    python scripts/key_ingest_timing.py big 20           # the validated load of a compressed 2^20 key (device path only)

Run the steps as separate processes, each under its own time limit, chained with && (a step that faults ends the job).

kernels: device events around the launch (the library's own phase timer, zkmi_prof_get "misc"), 3 warm-ups, median of
10.  Products per second come from the operation count below and are set against the flat issue peak of DESIGN.md
section 4 (614.4 G wave-instructions/s) at 500 instructions per Fq product (field28.hpp).
keys: zkmi_ark_pk_load (one host thread, curve membership only) against zkmi_ark_pk_load_validated with CURVE and with
SUBGROUP: same blob, same process, alternated, host clock around calls that end in a synchronise."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from zkmi_loader import load_pkg  # noqa: E402

PEAK = 614.4e9  # wave-instructions / s
INSTR_PER_PRODUCT = 500
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HALF_BE = np.frombuffer(((P - 1) // 2).to_bytes(48, "big"), dtype=np.uint8)


def ones(e):
    return bin(e).count("1")


# Fq-product equivalents per point.  A product is 196 + 196 multiply-adds and a carry sweep (500 instructions); a square
# does 105 + 196 of them and is priced at 0.8 product.  In Fq2 a product is 4 limb products under 2 reductions (priced 3),
# a square 2 products.  Square-and-multiply from the leading one: bits - 1 squares, ones - 1 products.  Doubling
# (dbl-2008-s-1): 3 squares + 6 products; mixed addition (madd-2008-s): 2 squares + 7 products + one a b - c d under one
# reduction (one product in Fq, two in Fq2).
SQ = 0.8


def chain(e, sqr, mul):
    return (e.bit_length() - 1) * sqr + (ones(e) - 1) * mul


OPS = {
    (1, "decompress"): chain((P + 1) // 4, SQ, 1) + 6,
    (1, "subgroup"): (R.bit_length() - 1) * (3 * SQ + 6) + (ones(R) - 1) * (2 * SQ + 8) + 5,
    (2, "decompress"): chain((P - 3) // 4, 2, 3) + chain((P - 1) // 2, 2, 3) + 25,
    (2, "subgroup"): (R.bit_length() - 1) * (3 * 2 + 6 * 3) + (ones(R) - 1) * (2 * 2 + 7 * 3 + 6) + 12,
}


def gt_half(be):
    diff = be != HALF_BE
    first = diff.argmax(axis=1)
    return diff.any(axis=1) & (be[np.arange(be.shape[0]), first] > HALF_BE[first])


def np_compress(group, wire):
    """zcash compressed form of n finite affine wire points."""
    a = np.frombuffer(wire, dtype=np.uint8).reshape(-1, 2 * group, 48)[:, :, ::-1]
    out = np.ascontiguousarray(a[:, :group][:, ::-1]).reshape(-1, 48 * group).copy()
    larger = gt_half(a[:, 1]) if group == 1 else np.where(a[:, 3].any(axis=1), gt_half(a[:, 3]), gt_half(a[:, 2]))
    out[:, 0] |= 0x80
    out[larger, 0] |= 0x20
    return out.tobytes()


def kernels(pkg, z, ctx):
    import torch

    for group, log_n in ((1, 20), (2, 18)):
        n = 1 << log_n
        b = ctx.bases_g1_synthetic(n) if group == 1 else ctx.bases_g2_synthetic(n)
        wire = b.read(0, n)
        b.free()
        forms = {pkg.ENC_WIRE: wire, pkg.ENC_ZCASH_COMPRESSED: np_compress(group, wire)}
        dev = {e: torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda() for e, v in forms.items()}
        out = torch.empty(len(wire), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fn = ctx.g1_points_read_dev if group == 1 else ctx.g2_points_read_dev
        cases = (("decompress", pkg.ENC_ZCASH_COMPRESSED, pkg.CHECK_CURVE, OPS[group, "decompress"]),
                 ("curve + subgroup, wire in", pkg.ENC_WIRE, pkg.CHECK_SUBGROUP, OPS[group, "subgroup"]),
                 ("decompress + subgroup", pkg.ENC_ZCASH_COMPRESSED, pkg.CHECK_SUBGROUP,
                  OPS[group, "decompress"] + OPS[group, "subgroup"]))
        for name, enc, checks, ops in cases:
            ms = []
            ctx.prof_enable(True)
            for it in range(13):
                ctx.prof_reset()
                assert fn(dev[enc].data_ptr(), n, enc, checks, out.data_ptr(), None) is None
                t, cnt = ctx.prof_get("misc")
                assert cnt == 1
                if it >= 3:
                    ms.append(t)
            ctx.prof_enable(False)
            med = statistics.median(ms)
            prod_s = n * ops / (med * 1e-3)
            frac = prod_s / 64 * INSTR_PER_PRODUCT / PEAK
            print("kernel G%d 2^%d %-26s median %8.3f ms (min %.3f max %.3f, 10 launches)  %7.0f product-equivalents/point  "
                  "%.3e products/s  %.2f of issue peak" % (group, log_n, name, med, min(ms), max(ms), ops, prod_s, frac), flush=True)
        assert out.cpu().numpy().tobytes() == wire
        del dev, out


def make_key(z, ctx, lg):
    toxic = b"".join(((0x1234567 + 977 * i) % R).to_bytes(32, "little") for i in range(5))
    r1 = z.update_note_r1cs(lg, 1)
    t0 = time.perf_counter()
    pk, vk = ctx.groth16_setup(r1, toxic)
    t1 = time.perf_counter()
    blob = ctx.ark_pk_write(pk, vk, True)
    t2 = time.perf_counter()
    print("key 2^%d: n_vars %d, setup on the device %.2f s, ark_pk_write(compressed) %.2f s, blob %.1f MiB"
          % (lg, r1.n_vars, t1 - t0, t2 - t1, len(blob) / 2**20), flush=True)
    return r1, pk, vk, blob


def timed(f):
    t0 = time.perf_counter()
    pk, vk = f()
    dt = time.perf_counter() - t0
    pk.free()
    return dt, vk


def keys(pkg, z, ctx, sizes, rounds=3):
    for lg in sizes:
        r1, pk, vk, blob = make_key(z, ctx, lg)
        pk.free()
        t = {"host": [], "curve": [], "subgroup": []}
        for _ in range(rounds):
            for name, f in (("host", lambda: ctx.ark_pk_load(r1, blob, True)),
                            ("curve", lambda: ctx.ark_pk_load_validated(r1, blob, True, pkg.CHECK_CURVE)),
                            ("subgroup", lambda: ctx.ark_pk_load_validated(r1, blob, True, pkg.CHECK_SUBGROUP))):
                dt, vk_back = timed(f)
                assert vk_back == vk
                t[name].append(dt)
        med = {k: statistics.median(v) for k, v in t.items()}
        for k, v in t.items():
            print("load 2^%d %-8s %s  median %.3f s" % (lg, k, " ".join("%.3f" % x for x in v), med[k]), flush=True)
        print("load 2^%d: host path / validated(CURVE) = %.1fx, host path / validated(SUBGROUP) = %.1fx"
              % (lg, med["host"] / med["curve"], med["host"] / med["subgroup"]), flush=True)
        r1.free()


def big(pkg, z, ctx, lg):
    r1, pk, vk, blob = make_key(z, ctx, lg)
    pk.free()
    for checks, name in ((pkg.CHECK_CURVE, "curve"), (pkg.CHECK_SUBGROUP, "subgroup"), (pkg.CHECK_SUBGROUP, "subgroup")):
        dt, vk_back = timed(lambda: ctx.ark_pk_load_validated(r1, blob, True, checks))
        assert vk_back == vk
        print("load 2^%d validated(%s) %.3f s (device path; includes building the MSM tables of the key)" % (lg, name, dt), flush=True)
    # the part that is the point readers: the five queries alone, from HBM
    import torch

    n, N = r1.n_vars, 1 << lg
    head = len(z.ark_vk_write(vk, r1.n_pub, True)) + 96
    ctx.prof_enable(True)
    off, total = head, 0.0
    for group, cnt in ((1, n), (1, n), (2, n), (1, N - 1), (1, n - r1.n_pub)):
        w = 48 * group
        sec = torch.frombuffer(bytearray(blob[off + 8 : off + 8 + w * cnt]), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        ctx.prof_reset()
        fn = ctx.g1_points_read_dev if group == 1 else ctx.g2_points_read_dev
        assert fn(sec.data_ptr(), cnt, pkg.ENC_ZCASH_COMPRESSED, pkg.CHECK_SUBGROUP) is None
        total += ctx.prof_get("misc")[0]
        off += 8 + w * cnt
    ctx.prof_enable(False)
    print("load 2^%d: the point-reader kernels over the five queries (decompress + subgroup): %.1f ms of GPU time" % (lg, total), flush=True)
    r1.free()


def main():
    pkg = load_pkg()
    z = pkg.Zkmi(os.environ.get("ZKMI_LIB"))
    ctx = z.context(0)
    step = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if step == "kernels":
        kernels(pkg, z, ctx)
    elif step == "keys":
        keys(pkg, z, ctx, [int(a) for a in sys.argv[2:]] or [13, 16])
    elif step == "big":
        big(pkg, z, ctx, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        raise SystemExit("unknown step " + step)
    ctx.close()


if __name__ == "__main__":
    main()
