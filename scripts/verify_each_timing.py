#!/usr/bin/env python3
"""Per-proof verification on the device timed against the batch call (csrc/verify_each.hip, csrc/pairing_dev.hip
k_final_exp; results in profiles/r09/verify_each.txt).

    python scripts/verify_each_timing.py each 64 1024 16384      # zkmi_groth16_verify_each: good / one bad / all bad
    python scripts/verify_each_timing.py batch 64 1024 16384     # zkmi_groth16_verify_batch with statuses, same inputs
    python scripts/verify_each_timing.py pairing 1 64 1024       # zkmi_pairing_batch_dev (Miller loops + k_final_exp)

Every line printed is also appended to profiles/r09/verify_each.txt (ZKMI_TIMING_OUT names another file).

Run the steps as separate processes, each under its own time limit, chained with && (a step that faults ends the job).

Proofs of the 2^14 update_note key as in scripts/verify_batch_timing.py (two distinct witnesses, a fresh (r, s) per proof).
Inputs: no bad proof; one bad proof (C of its neighbour at n // 3); every proof bad (the publics of the other witness).
each: the whole call on the product library by the host clock, median of 3 after one warm-up; then one call on the testing
library, which records HIP events around k_public_sum_g1 and k_final_exp (zkmi_verify_each_kernel_ms).
batch: the unchanged batch call with statuses and fixed weights on the same inputs; its all-bad case bisects with one HOST
final exponentiation per range (2 n - 1 ranges), so it runs only for n <= 1024 and ONCE; larger n are extrapolated from
the per-range cost and labelled so."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from verify_batch_timing import LOG_N, make_proofs  # noqa: E402

ALL_BAD_BATCH_MAX = 1024
OUT = os.environ.get("ZKMI_TIMING_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                        "profiles", "r09", "verify_each.txt")


def say(line):
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def inputs(proofs, publics, n, kind):
    prf, pub = list(proofs[:n]), list(publics[:n])
    if kind == "one bad" and n > 1:
        k = n // 3
        prf[k] = prf[k][:144] + prf[k + 1][144:]
    elif kind == "one bad":
        pub[0] = publics[1]
    elif kind == "all bad":
        pub = [publics[i + 1] for i in range(n)]  # the two witnesses alternate: every proof gets the other one's publics
    return b"".join(pub), b"".join(prf)


def expect(n, kind):
    if kind == "no bad":
        return True, bytes(n), None
    if kind == "all bad":
        return False, bytes([5]) * n, 0
    k = n // 3 if n > 1 else 0
    return False, bytes(k) + b"\x05" + bytes(n - k - 1), k


def timed(fn, want, calls):
    ts = []
    for it in range(calls + 1):
        t0 = time.perf_counter()
        got = fn()
        dt = time.perf_counter() - t0
        assert got == want, (got[0], got[2])
        if it or calls == 0:
            ts.append(dt)
    return ts


def each(pkg, z, ctx, sizes):
    vk, n_pub, proofs, publics = make_proofs(z, ctx, max(sizes) + 1)
    zt = pkg.Zkmi(os.path.join(os.path.dirname(pkg.lib_path()), "libzkmi_exp.so"))
    ctx_t = zt.context(0)
    pv, pv_t = z.vk_prepare(vk), zt.vk_prepare(vk)
    say("key 2^%d update_note, n_pub %d; %d distinct proofs" % (LOG_N, n_pub, len(proofs)))
    for n in sizes:
        for kind in ("no bad", "one bad", "all bad"):
            pub, prf = inputs(proofs, publics, n, kind)
            ts = timed(lambda: ctx.groth16_verify_each(pv, pub, prf), expect(n, kind), 3)
            med = statistics.median(ts)
            assert ctx_t.groth16_verify_each(pv_t, pub, prf) == expect(n, kind)
            ms = (C.c_float * 3)()
            assert zt.lib.zkmi_verify_each_kernel_ms(ms) == 0
            if ms[2]:
                say("      (the first call with this key built its window table on the host: %.3f ms, once per key)" % ms[2])
            say("each  n=%6d %-8s median %9.3f ms (min %.3f max %.3f, 3 calls) %9.0f proofs/s | k_public_sum_g1 %8.3f ms, "
                  "k_final_exp %8.3f ms (HIP events, testing library)"
                  % (n, kind, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), n / med, ms[0], ms[1]))
    pv.free()
    pv_t.free()
    ctx_t.close()


def batch(pkg, z, ctx, sizes):
    vk, n_pub, proofs, publics = make_proofs(z, ctx, max(sizes) + 1)
    rng = bench.SplitMix64(0x77)
    weights = [rng.fr_bytes()[:15] + b"\x01" for _ in proofs]
    pv = z.vk_prepare(vk)
    per_range = None
    for n in sizes:
        w = b"".join(weights[:n])
        for kind in ("no bad", "one bad", "all bad"):
            pub, prf = inputs(proofs, publics, n, kind)
            if kind == "all bad" and n > ALL_BAD_BATCH_MAX:
                if per_range is not None:
                    say("batch n=%6d all bad  NOT RUN: (2 n - 1) ranges x %.2f ms per range (measured at n = %d) = %.0f s, extrapolated"
                          % (n, 1e3 * per_range[0], per_range[1], (2 * n - 1) * per_range[0]))
                continue
            calls = 0 if kind == "all bad" else 3
            ts = timed(lambda: ctx.groth16_verify_batch(pv, pub, prf, w), expect(n, kind), calls)
            med = statistics.median(ts)
            if kind == "all bad":
                per_range = (med / (2 * n - 1), n)
            say("batch n=%6d %-8s median %9.3f ms (min %.3f max %.3f, %d call%s) %9.0f proofs/s"
                  % (n, kind, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), len(ts), "s" if len(ts) > 1 else "", n / med))
    pv.free()


def pairing(pkg, z, ctx, sizes):
    import torch

    g1, g2 = z.g1_generator(), z.g2_generator()
    one = z.pairing(g1, g2)
    for n in sizes:
        d1 = torch.frombuffer(bytearray(g1 * n), dtype=torch.uint8).cuda()
        d2 = torch.frombuffer(bytearray(g2 * n), dtype=torch.uint8).cuda()
        out = torch.zeros(576 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ts = []
        for it in range(4):
            t0 = time.perf_counter()
            ctx.pairing_batch_dev(d1.data_ptr(), d2.data_ptr(), n, out.data_ptr())
            dt = time.perf_counter() - t0
            if it:
                ts.append(dt)
        raw = out.cpu().numpy().tobytes()
        assert raw[:576] == one and raw[-576:] == one
        med = statistics.median(ts)
        say("pairing batch n=%6d  median %9.3f ms (min %.3f max %.3f, 3 calls) %9.0f pairings/s"
              % (n, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), n / med))
    t0 = time.perf_counter()
    for _ in range(4):
        z.pairing(g1, g2)
    say("host zkmi_pairing (Miller loop + square-and-multiply final exponentiation): %.2f ms each" % (1e3 * (time.perf_counter() - t0) / 4))


def main():
    pkg = bench.load_pkg()
    z = pkg.Zkmi(os.environ.get("ZKMI_LIB"))
    ctx = z.context(0)
    step = sys.argv[1] if len(sys.argv) > 1 else "each"
    sizes = [int(a) for a in sys.argv[2:]]
    if step == "each":
        each(pkg, z, ctx, sizes or [64, 1024, 16384])
    elif step == "batch":
        batch(pkg, z, ctx, sizes or [64, 1024, 16384])
    elif step == "pairing":
        pairing(pkg, z, ctx, sizes or [1, 64, 1024])
    else:
        raise SystemExit("unknown step " + step)
    ctx.close()


if __name__ == "__main__":
    main()
