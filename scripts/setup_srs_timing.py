#!/usr/bin/env python3
"""zkmi_groth16_setup_from_srs against zkmi_groth16_setup at the same size, timed (csrc/setup_srs.hip; DESIGN.md 5.7;
results in profiles/r12/setup_from_srs.txt).

    python scripts/setup_srs_timing.py update_note 13
    python scripts/setup_srs_timing.py update_note 14
    python scripts/setup_srs_timing.py synthetic 16

Run the sizes as separate processes, each under its own time limit, chained with && (a step that faults ends the job).

Host clock around calls that end in a synchronise; one warm-up of each setup, then the median of 3, alternated.  The
transcript is made by zkmi_srs_generate outside the clock (a deployment loads it once).  The breakdown of the transcript
path comes from the testing library's zkmi_setup_from_srs_phases (host clock between stream waits): Lagrange transforms,
column sums, h query; "rest" is what remains of the call -- key allocation, the conversion to the 28-bit forms and the
digit tables, which the trapdoor setup runs too."""
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


def main():
    kind, log_n = sys.argv[1], int(sys.argv[2])
    pkg = load_pkg()
    # the A/B + testing library: the product's kernels, plus the phase record
    z = pkg.Zkmi(os.path.join(ROOT, "zk-apps_amd", "libzkmi_exp.so"))
    ctx = z.context(0)
    r1 = z.update_note_r1cs(log_n, 1) if kind == "update_note" else z.shielder_r1cs(log_n)
    nnz = sum(len(r1.export(m)[1]) for m in range(3))
    srs = ctx.srs_generate(frs([TAU, ALPHA, BETA]), r1.log_n)
    toxic = frs([TAU, ALPHA, BETA, 1, 1])
    t_trap, t_srs, phases = [], [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        pk0, vk0 = ctx.groth16_setup(r1, toxic)
        t1 = time.perf_counter()
        pk1, vk1 = ctx.groth16_setup_from_srs(r1, srs)
        t2 = time.perf_counter()
        if rep == 0:  # the two keys are one key
            assert vk0 == vk1
            for which, cnt in ((0, r1.n_vars), (1, r1.n_vars), (2, r1.n_vars), (3, (1 << r1.log_n) - 1), (4, r1.n_vars - r1.n_pub)):
                assert pk0.export_query(which, 0, cnt) == pk1.export_query(which, 0, cnt), which
        else:
            t_trap.append((t1 - t0) * 1e3)
            t_srs.append((t2 - t1) * 1e3)
            phases.append(ctx.setup_from_srs_phases())
        pk0.free()
        pk1.free()
    trap, from_srs = statistics.median(t_trap), statistics.median(t_srs)
    ph = [statistics.median(p[k] for p in phases) for k in range(3)]
    print("%s 2^%d: n_vars %d, n_pub %d, constraints %d, non-zeros %d; keys identical" % (kind, r1.log_n, r1.n_vars, r1.n_pub, r1.n_constraints, nnz))
    print("  zkmi_groth16_setup (trapdoor)   %9.1f ms   (%s)" % (trap, " ".join("%.1f" % t for t in t_trap)))
    print("  zkmi_groth16_setup_from_srs     %9.1f ms   (%s)   ratio %.2f" % (from_srs, " ".join("%.1f" % t for t in t_srs), from_srs / trap))
    print("    Lagrange transforms %9.1f ms | column sums %9.1f ms | h query %7.1f ms | rest (allocation, conversion, tables) %9.1f ms"
          % (ph[0], ph[1], ph[2], from_srs - sum(ph)))
    srs.free()
    r1.free()
    ctx.close()


if __name__ == "__main__":
    main()
