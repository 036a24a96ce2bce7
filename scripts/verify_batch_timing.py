#!/usr/bin/env python3
"""Batch verification timed against the host verifier (csrc/verify_batch.hip; results in
profiles/r08/verify_batch.txt).

    python scripts/verify_batch_timing.py batch 64 1024 16384     # zkmi_groth16_verify_batch, phase split included
    python scripts/verify_batch_timing.py host 64                 # the loop of zkmi_groth16_verify, 1 and 16 threads

Run the steps as separate processes, each under its own time limit, chained with && (a step that faults ends the job).

Proofs of the 2^14 update_note key (two distinct witnesses, a fresh (r, s) per proof, so all proofs differ).
batch: the whole call on the product library (host clock, median of 3 after one warm-up), then ONE call on the testing
library, which waits for the stream at every phase boundary and reports the split (zkmi_verify_batch_phases).
host: the unchanged zkmi_groth16_verify over the first `count` proofs on one thread and on 16 threads (ctypes releases
the GIL for the call); rates for larger batches are this rate extrapolated, and labelled so."""
import ctypes as C
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (relation_and_witness, SplitMix64)

LOG_N = 14
PHASES = ("upload + split", "decompress + subgroup", "w_i A_i, MSM bases", "n Miller loops", "sums (Fr, MSM, scalar muls)",
          "3 Miller loops + products", "final exponentiation")


def make_proofs(z, ctx, count):
    import torch

    r1, wits = bench.relation_and_witness(z, "poseidon", LOG_N, [0x5A4B0100, 0x5A4B0101])
    rng = bench.SplitMix64(0x5A4B0102)
    pk, vk = ctx.groth16_setup(r1, b"".join(rng.fr_bytes() for _ in range(5)))
    d = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
    torch.cuda.synchronize()
    idx = [i % 2 for i in range(count)]
    proofs = ctx.groth16_prove_batch_dev(pk, [d[j].data_ptr() for j in idx], [rng.fr_bytes() for _ in idx], [rng.fr_bytes() for _ in idx])
    ctx.sync()
    pk.free()
    publics = [wits[j][32 : 32 * r1.n_pub] for j in idx]
    n_pub = r1.n_pub
    r1.free()
    return vk, n_pub, proofs, publics


def batch(pkg, z, ctx, sizes):
    vk, n_pub, proofs, publics = make_proofs(z, ctx, max(sizes))
    assert len(set(proofs)) == len(proofs)
    rng = bench.SplitMix64(0x77)
    weights = [rng.fr_bytes()[:15] + b"\x01" for _ in proofs]
    zt = pkg.Zkmi(os.path.join(os.path.dirname(pkg.lib_path()), "libzkmi_exp.so"))
    ctx_t = zt.context(0)
    pv, pv_t = z.vk_prepare(vk), zt.vk_prepare(vk)
    print("key 2^%d update_note, n_pub %d; %d distinct proofs" % (LOG_N, n_pub, len(proofs)), flush=True)
    for n in sizes:
        pub, prf, w = b"".join(publics[:n]), b"".join(proofs[:n]), b"".join(weights[:n])
        ts = []
        for it in range(4):
            t0 = time.perf_counter()
            ok, st, bad = ctx.groth16_verify_batch(pv, pub, prf, w)
            dt = time.perf_counter() - t0
            assert ok and bad is None and st == bytes(n)
            if it:
                ts.append(dt)
        med = statistics.median(ts)
        print("batch n=%6d  median %9.3f ms (min %.3f max %.3f, 3 calls)  %9.0f proofs/s" % (n, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), n / med), flush=True)
        assert ctx_t.groth16_verify_batch(pv_t, pub, prf, w)[0]
        t0 = time.perf_counter()
        assert ctx_t.groth16_verify_batch(pv_t, pub, prf, w)[0]
        dt = time.perf_counter() - t0
        ph = (C.c_double * 7)()
        assert zt.lib.zkmi_verify_batch_phases(ph) == 0
        print("  split n=%d (testing library, stream waited for at every boundary; whole call %.3f ms):" % (n, 1e3 * dt))
        for name, v in zip(PHASES, ph):
            print("    %-30s %9.3f ms" % (name, v))
        sys.stdout.flush()
    # one planted fault: what localisation costs
    n = sizes[0] if len(sizes) == 1 else sizes[1]
    prf = list(proofs[:n])
    prf[n // 3] = prf[n // 3][:144] + prf[n // 3 + 1][144:]
    t0 = time.perf_counter()
    ok, st, bad = ctx.groth16_verify_batch(pv, b"".join(publics[:n]), b"".join(prf), b"".join(weights[:n]))
    dt = time.perf_counter() - t0
    assert not ok and bad == n // 3 and st.count(5) == 1
    print("batch n=%6d with one failing proof, localised by bisection: %.3f ms" % (n, 1e3 * dt), flush=True)
    pv.free()
    pv_t.free()
    ctx_t.close()


def host(pkg, z, ctx, count):
    vk, n_pub, proofs, publics = make_proofs(z, ctx, count)

    def one(i):
        return z.groth16_verify(vk, publics[i], proofs[i])

    t0 = time.perf_counter()
    assert all(one(i) for i in range(count))
    t1 = time.perf_counter() - t0
    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        assert all(ex.map(one, range(count)))
        t16 = time.perf_counter() - t0
    print("host loop of zkmi_groth16_verify over %d proofs: 1 thread %.1f ms/proof (%.1f proofs/s), 16 threads %.1f proofs/s"
          % (count, 1e3 * t1 / count, count / t1, count / t16), flush=True)
    for n in (64, 1024, 16384):
        print("  n=%6d: 1 thread %10.1f ms, 16 threads %10.1f ms%s" % (n, 1e3 * t1 / count * n, 1e3 * t16 / count * n,
                                                                      "" if n <= count else "  (extrapolated from %d proofs)" % count))


def main():
    pkg = bench.load_pkg()
    z = pkg.Zkmi(os.environ.get("ZKMI_LIB"))
    ctx = z.context(0)
    step = sys.argv[1] if len(sys.argv) > 1 else "batch"
    if step == "batch":
        batch(pkg, z, ctx, [int(a) for a in sys.argv[2:]] or [64, 1024, 16384])
    elif step == "host":
        host(pkg, z, ctx, int(sys.argv[2]) if len(sys.argv) > 2 else 64)
    else:
        raise SystemExit("unknown step " + step)
    ctx.close()


if __name__ == "__main__":
    main()
