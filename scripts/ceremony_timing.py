#!/usr/bin/env python3
"""zkmi_srs_verify and zkmi_pk_verify_contribution against the other thing a verifier must run, timed (csrc/ceremony.hip;
DESIGN.md 5.8; results in profiles/r13/ceremony.txt).

    python scripts/ceremony_timing.py                 # domains 2^13, 2^16, 2^20, then phase 2 at 2^13
    python scripts/ceremony_timing.py 13 16           # these domains only
    python scripts/ceremony_timing.py --no-phase2 20

One MI355X, one process, run under a time limit (a step that faults ends the job).  Host clock around calls that end in a
synchronise; one warm-up of each call, then the median of 3, alternated.

Phase 1: the transcript is made by zkmi_srs_generate and read back to host bytes outside the clock.  zkmi_srs_verify on the
resident transcript is set beside zkmi_srs_load of the same bytes (wire form) under ZKMI_CHECK_SUBGROUP: the load is the
yardstick, since a verifier runs both.  Phase 2: `after` is the update_note key of the transcript with one contribution;
zkmi_pk_verify_contribution(before, after) is set beside zkmi_pk_check(after) under ZKMI_CHECK_SUBGROUP.  The breakdown comes
from the testing library's zkmi_ceremony_phases (host clock between stream waits): weights, conversion to the MSM's base
form, MSMs, pairing products; "rest" is what remains of the call -- allocation, the reads of the anchor points, and in
phase 2 the comparison of the fixed part."""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zkmi_loader import load_pkg  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU, ALPHA, BETA = 0x1D0C5A7E5EED0001 % R, 0x2A11FA0000000007 * 0x10001 % R, (R - 0xBE7A) % R
REPS = 3


def frs(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def seed(k):
    return hashlib.sha256(b"ceremony timing %d" % k).digest()


def report(name, times):
    return "%-34s %10.1f ms   (%s)" % (name, statistics.median(times), " ".join("%.1f" % t for t in times))


def breakdown(phases, total):
    ph = [statistics.median(p[k] for p in phases) for k in range(4)]
    return ("    weights %8.2f ms | conversion %8.2f ms | MSMs %9.1f ms | pairing products %8.1f ms | rest %8.1f ms"
            % (ph[0], ph[1], ph[2], ph[3], total - sum(ph)))


def phase1(ctx, log_n):
    srs = ctx.srs_generate(frs([TAU, ALPHA, BETA]), log_n)
    n1, n2, nab = srs.shape()
    sec = [srs.read(0, 0, n1), srs.read(1, 0, n2), srs.read(2, 0, nab), srs.read(3, 0, nab), srs.read(4, 0, 1)]
    t_verify, t_load, phases = [], [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        ok, failed = srs.verify(seed(rep))
        t1 = time.perf_counter()
        ph = ctx.ceremony_phases()
        loaded = ctx.srs_load(0, *sec)
        t2 = time.perf_counter()
        assert ok and failed == 0
        if rep == 0:  # the loaded transcript is the generated one: it verifies too
            assert loaded.verify(seed(99)) == (True, 0)
        else:
            t_verify.append((t1 - t0) * 1e3)
            t_load.append((t2 - t1) * 1e3)
            phases.append(ph)
        loaded.free()
    srs.free()
    v, l = statistics.median(t_verify), statistics.median(t_load)
    print("transcript for 2^%d: %d + %d + %d G1 points, %d G2 points" % (log_n, n1, nab, nab, n2))
    print("  " + report("zkmi_srs_verify", t_verify) + "   ratio to the load %.2f" % (v / l))
    print(breakdown(phases, v))
    print("  " + report("zkmi_srs_load, ZKMI_CHECK_SUBGROUP", t_load), flush=True)


def phase2(z, ctx, log_n):
    r1 = z.update_note_r1cs(log_n, 1)
    srs = ctx.srs_generate(frs([TAU, ALPHA, BETA]), r1.log_n)
    before, _ = ctx.groth16_setup_from_srs(r1, srs)
    after, _ = ctx.groth16_setup_from_srs(r1, srs)
    srs.free()
    after.contribute(frs([0xD1_0000_0000_0000_0000_0000_0005 % R]))
    t_verify, t_check, phases = [], [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        ok, failed = after.verify_contribution(before, seed(rep))
        t1 = time.perf_counter()
        ph = ctx.ceremony_phases()
        where = after.check()
        t2 = time.perf_counter()
        assert ok and failed == 0 and where is None
        if rep:
            t_verify.append((t1 - t0) * 1e3)
            t_check.append((t2 - t1) * 1e3)
            phases.append(ph)
    v, c = statistics.median(t_verify), statistics.median(t_check)
    print("update_note 2^%d: n_vars %d, n_pub %d" % (r1.log_n, r1.n_vars, r1.n_pub))
    print("  " + report("zkmi_pk_verify_contribution", t_verify) + "   ratio to the check %.2f" % (v / c))
    print(breakdown(phases, v))
    print("  " + report("zkmi_pk_check, ZKMI_CHECK_SUBGROUP", t_check), flush=True)
    before.free()
    after.free()
    r1.free()


def main():
    args = sys.argv[1:]
    with_phase2 = "--no-phase2" not in args
    sizes = [int(a) for a in args if not a.startswith("--")] or [13, 16, 20]
    pkg = load_pkg()
    # the A/B + testing library: the product's kernels, plus the phase record
    z = pkg.Zkmi(os.path.join(ROOT, "zk-apps_amd", "libzkmi_exp.so"))
    ctx = z.context(0)
    for log_n in sizes:
        phase1(ctx, log_n)
    if with_phase2:
        phase2(z, ctx, 13)
    ctx.close()


if __name__ == "__main__":
    main()
