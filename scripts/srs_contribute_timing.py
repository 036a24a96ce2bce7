#!/usr/bin/env python3
"""zkmi_srs_contribute timed, with its breakdown and three yardsticks (csrc/points_mul.hip, csrc/points_ntt.hip; DESIGN.md
5.9; results in profiles/rNN/srs_contribute.txt).

    python scripts/srs_contribute_timing.py                   # domains 2^13, 2^16, 2^20 -> the next profiles/rNN/
    python scripts/srs_contribute_timing.py --out FILE 13 16  # these domains only, into FILE
    python scripts/srs_contribute_timing.py --once 16         # one contribution per kernel and nothing else: the run a
                                                              # profiler wraps (rocprofv3 ... -- python scripts/... --once 16)

One MI355X, one process, run under a time limit (a step that faults ends the job).  Host clock around calls that end in a
synchronise; one warm-up of each call, then the median of 3.

Two transcripts of the same waste take the same contributions, one through the windowed multiplication kernel and one
through the plain one (the testing library's switch), alternated; their five sections are compared byte for byte after
the first pair, before any time is quoted.  A third transcript takes the same contributions through the product library,
which records no phases, and is held to the same last points.  The spread of the repeated identical runs (max - min) stands next to the
difference of the medians.  The breakdown is the testing library's zkmi_points_mul_phases (host clock between stream
waits): powers, G1 multiplication kernels, G2 multiplication kernels, affine stores and allocation; "rest" is what remains
of the call -- the wipes, the host's four G2 multiplications and the swap.  Yardsticks: (a) the plain kernel, (b)
zkmi_srs_generate at the same size, (c) zkmi_srs_verify_contribution beside zkmi_srs_verify of the same transcript."""
import hashlib
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zkmi_loader import load_pkg  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU, ALPHA, BETA = 0x1D0C5A7E5EED0001 % R, 0x2A11FA0000000007 * 0x10001 % R, (R - 0xBE7A) % R
REPS = 3
WINDOWED, PLAIN = 0, 1


def frs(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def waste(k):
    """Three full-width non-zero scalars per repetition."""
    h = [int.from_bytes(hashlib.sha256(b"contribution %d %d" % (k, j)).digest(), "little") % (R - 1) + 1 for j in range(3)]
    return frs(h)


def seed(k):
    return hashlib.sha256(b"contribute timing %d" % k).digest()


def sections(srs):
    n1, n2, nab = srs.shape()
    return [srs.read(0, 0, n1), srs.read(1, 0, n2), srs.read(2, 0, nab), srs.read(3, 0, nab), srs.read(4, 0, 1)]


def report(name, times):
    return "%-40s %10.1f ms   (%s)" % (name, statistics.median(times), " ".join("%.1f" % t for t in times))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def one_size(z, ctx, ctx_product, log_n, out):
    toxic = frs([TAU, ALPHA, BETA])
    t_gen = []
    for rep in range(REPS + 1):  # (b) the fixed-base path that makes a transcript from waste in the clear
        s, ms = timed(lambda: ctx.srs_generate(toxic, log_n))
        s.free()
        if rep:
            t_gen.append(ms)
    a, b = ctx.srs_generate(toxic, log_n), ctx.srs_generate(toxic, log_n)
    n1, n2, nab = a.shape()
    t = {WINDOWED: [], PLAIN: []}
    phases = []
    for rep in range(REPS + 1):
        for kernel, srs in ((WINDOWED, a), (PLAIN, b)):
            z.points_mul_kernel(kernel)
            step, ms = timed(lambda: srs.contribute(waste(rep)))
            if kernel == WINDOWED:
                ph = z.points_mul_phases()
            if rep:
                t[kernel].append(ms)
                if kernel == WINDOWED:
                    phases.append(ph)
        if rep == 0:  # the two kernels agree on every byte before a time is quoted
            same = sections(a) == sections(b)
            out("transcript for 2^%d: %d + %d + %d G1 points, %d G2 points; windowed and plain kernels byte-equal: %s"
                % (log_n, n1, nab, nab, n2, same))
            assert same
    z.points_mul_kernel(WINDOWED)
    b.free()
    # the product library (no phase record: it adds no stream waits) takes the same contributions and ends on the same bytes
    c = ctx_product.srs_generate(toxic, log_n)
    t_prod = []
    for rep in range(REPS + 1):
        _, ms = timed(lambda: c.contribute(waste(rep)))
        if rep:
            t_prod.append(ms)
    n_tail = min(n2, 4096)
    same = (c.read(0, n1 - n_tail, n_tail), c.read(1, n2 - n_tail, n_tail), c.read(4, 0, 1)) == (
        a.read(0, n1 - n_tail, n_tail), a.read(1, n2 - n_tail, n_tail), a.read(4, 0, 1))
    c.free()
    assert same
    w, p = statistics.median(t[WINDOWED]), statistics.median(t[PLAIN])
    spread = max(max(v) - min(v) for v in t.values())
    out("  " + report("zkmi_srs_contribute (windowed kernel)", t[WINDOWED]))
    ph = [statistics.median(x[k] for x in phases) for k in range(4)]
    out("    powers %8.2f ms | G1 kernels %9.1f ms | G2 kernels %9.1f ms | stores and allocation %8.1f ms | rest %8.1f ms"
        % (ph[0], ph[1], ph[2], ph[3], w - sum(ph)))
    out("  " + report("the product library, same contributions", t_prod) + "   last points byte-equal: %s" % same)
    out("  " + report("(a) the same, plain mul_words kernel", t[PLAIN]))
    out("    plain - windowed %+.1f ms (%.2fx); spread of repeated identical runs %.1f ms" % (p - w, p / w, spread))
    out("  " + report("(b) zkmi_srs_generate", t_gen))
    # (c) the check of the contribution beside the check of the transcript alone
    before = ctx.srs_generate(toxic, log_n)
    after = ctx.srs_generate(toxic, log_n)
    step = after.contribute(waste(100))
    t_vc, t_v = [], []
    for rep in range(REPS + 1):
        r1, ms1 = timed(lambda: after.verify_contribution(before, step, seed(rep)))
        r2, ms2 = timed(lambda: after.verify(seed(rep)))
        assert r1 == (True, 0) and r2 == (True, 0)
        if rep:
            t_vc.append(ms1)
            t_v.append(ms2)
    out("  " + report("(c) zkmi_srs_verify_contribution", t_vc))
    out("  " + report("    zkmi_srs_verify", t_v))
    for s in (a, before, after):
        s.free()


def once(z, ctx, log_n):
    toxic = frs([TAU, ALPHA, BETA])
    for kernel in (WINDOWED, PLAIN):
        srs = ctx.srs_generate(toxic, log_n)
        z.points_mul_kernel(kernel)
        srs.contribute(waste(0))
        srs.free()
    z.points_mul_kernel(WINDOWED)


def next_profile_dir():
    base = os.path.join(ROOT, "profiles")
    rounds = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(base)) if m]
    return os.path.join(base, "r%02d" % (max(rounds or [0]) + 1))


def main():
    args = sys.argv[1:]
    path = None
    if "--out" in args:
        i = args.index("--out")
        path = args[i + 1]
        del args[i : i + 2]
    only_once = "--once" in args
    sizes = [int(a) for a in args if not a.startswith("--")] or [13, 16, 20]
    pkg = load_pkg()
    # the A/B + testing library: the product's kernels, plus the plain kernel, the switch and the phase record
    z = pkg.Zkmi(os.path.join(ROOT, "zk-apps_amd", "libzkmi_exp.so"))
    ctx = z.context(0)
    ctx_product = None if only_once else pkg.Zkmi(os.path.join(ROOT, "zk-apps_amd", "libzkmi.so")).context(0)
    if only_once:
        for log_n in sizes:
            once(z, ctx, log_n)
        ctx.close()
        return
    if path is None:
        path = os.path.join(next_profile_dir(), "srs_contribute.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        def out(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        out("zkmi_srs_contribute on %s, library %s; median of %d after one warm-up" % (z.host_info(), z.version(), REPS))
        for log_n in sizes:
            one_size(z, ctx, ctx_product, log_n, out)
    ctx_product.close()
    ctx.close()


if __name__ == "__main__":
    main()
