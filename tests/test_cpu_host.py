"""CPU suite, part 2: the product's host logic through the C ABI (no compute
kernels are launched; the library must load and export every declared symbol
without a GPU)."""
import ctypes as C
import os
import re
import sys

import pytest

from conftest import ROOT, golden
from oracle import bls12_381 as ec
from oracle import groth16 as g16

H = bytes.fromhex


def test_library_exports_every_declared_symbol(zk):
    """The product library exports exactly the product ABI: everything include/zkmi.h declares, and NONE of the test
    scaffolding of include/zkmi_testing.h (synthetic bases, the chain stand-in relation, host self-tests: round 4 exported
    those from libzkmi.so); the A/B + testing library libzkmi_exp.so exports both."""
    import subprocess

    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    names = set(re.findall(r"\b(zkmi_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) > 50
    for n in sorted(names):
        assert hasattr(zk.lib, n), f"{n} declared in include/zkmi.h but not exported"
    thdr = open(os.path.join(ROOT, "include", "zkmi_testing.h")).read()
    tnames = set(re.findall(r"\b(zkmi_[a-z0-9_]+)\s*\(", thdr))
    assert len(tnames) >= 12 and not (tnames & names)
    assert zk.tlib is not zk.lib
    for n in sorted(tnames):
        assert not hasattr(zk.lib, n), f"{n} is test scaffolding but the product library exports it"
        assert hasattr(zk.tlib, n), f"{n} declared in include/zkmi_testing.h but not exported by the testing library"
    for n in sorted(names):
        assert hasattr(zk.tlib, n), f"{n}: the A/B + testing library must carry the whole product ABI too"
    # nothing exported that no header declares
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zk-apps_amd", "libzkmi.so")], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (zkmi_[a-z0-9_]+)$", out, re.M))
    assert exported == names, (sorted(exported - names), sorted(names - exported))


def test_reference_side_bindings_name_only_exported_functions(zk):
    """integration/ffi.rs (the extern block a maintainer adds to mocked_zk) and the C example bind nothing the
    library does not export, and every function they bind is declared in include/zkmi.h with the same argument count."""
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(zkmi_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, re.S)}
    rs = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    fns = re.findall(r"pub fn (zkmi_[a-z0-9_]+)\s*\(([^;]*?)\)\s*(?:->[^;]*)?;", rs, re.S)
    assert len(fns) >= 50
    for name, args in fns:
        assert hasattr(zk.lib, name), f"{name} bound in integration/ffi.rs but not exported"
        assert name in decl, f"{name} bound in integration/ffi.rs but not declared in include/zkmi.h"
        n_rs = 0 if not args.strip() else args.count(",") + 1
        c_args = decl[name].strip()
        n_c = 0 if c_args in ("", "void") else c_args.count(",") + 1
        assert n_rs == n_c, f"{name}: {n_rs} arguments in ffi.rs, {n_c} in zkmi.h"
    ex = open(os.path.join(ROOT, "examples", "prove_withdraw.c")).read()
    for name in set(re.findall(r"\b(zkmi_[a-z0-9_]+)\s*\(", ex)):
        assert hasattr(zk.lib, name), f"{name} called in examples/prove_withdraw.c but not exported"


def _impl_pub_fns(src, type_name):
    """{name: [argument names]} of the `pub fn`s inside `impl <type_name> { ... }` blocks of a Rust source."""
    out = {}
    for m in re.finditer(r"\bimpl\s+(?:super::)?%s\s*\{" % type_name, src):
        depth, i = 1, m.end()
        while depth and i < len(src):
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        body = src[m.end(): i]
        for f in re.finditer(r"\bpub fn (\w+)\s*\(([^)]*)\)\s*(?:->\s*([^{]+?))?\s*\{", body, re.S):
            args = [a.strip().split(":")[0].strip() for a in f.group(2).split(",") if a.strip()]
            out[f.group(1)] = (args, re.sub(r"\s+", " ", (f.group(3) or "").strip()))
    return out


# Every public method of the reference's `impl ZkProof` (mocked_zk/src/relations.rs:36-155): argument names and return
# type, as _impl_pub_fns reads them.  SURVEY.md 8b describes the four call-site methods; verify_acccount_update
# (relations.rs:100-104, the reference's spelling) completes the set.
REFERENCE_ZKPROOF_API = {
    "new": (["id", "trapdoor", "nullifier", "op_priv", "acc"], "Self"),
    "update_account": (["&self", "operation", "trapdoor", "nullifier", "merkle_proof", "merkle_proof_leaf_id"],
                       "Result<(Scalar, Self), ZkpError>"),
    "verify_acccount_update": (["&self", "op", "h_acc_old"], "Result<Account, ZkpError>"),
    "verify_creation": (["&self", "h_note_new", "tokens_list"], "Result<(), ZkpError>"),
    "verify_update": (["&self", "op_pub", "h_note_new", "merkle_root", "nullifier_old"], "Result<(), ZkpError>"),
}


def test_rust_shim_is_drop_in_by_name_and_arity(zk):
    """integration/zkproof_shim.rs replaces mocked_zk::relations::ZkProof: every public method of the reference's
    `impl ZkProof` (relations.rs:36-155) exists in the shim as a METHOD with the same argument names, arity and return
    type, so the call sites (contract/lib.rs:56,74; drink_tests/utils/shielder.rs:60,105-114) compile unchanged.
    Every zkmi_* function the shim calls is bound in ffi.rs and exported by the library.  The expected shapes of all
    five methods are recorded in REFERENCE_ZKPROOF_API above, so the test needs nothing outside this repository."""
    shim_src = open(os.path.join(ROOT, "integration", "zkproof_shim.rs")).read()
    ffi_src = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    shim = _impl_pub_fns(shim_src, "ZkProof")
    for name, (args, ret) in REFERENCE_ZKPROOF_API.items():
        assert name in shim, f"reference method ZkProof::{name} is missing from the shim"
        assert shim[name][0] == args, f"ZkProof::{name}: arguments {shim[name][0]} != reference {args}"
        assert shim[name][1] == ret, f"ZkProof::{name}: return type {shim[name][1]!r} != reference {ret!r}"
    bound = set(re.findall(r"pub fn (zkmi_[a-z0-9_]+)", ffi_src))
    for name in set(re.findall(r"\b(zkmi_[a-z0-9_]+)\s*\(", shim_src)):
        assert name in bound, f"{name} called by the shim but not bound in ffi.rs"
        assert hasattr(zk.lib, name), f"{name} called by the shim but not exported"


def test_bench_never_reports_a_line_for_another_gpu_count():
    """bench.py --gpus N: a launcher with another world size is refused, and without a launcher N > 1 starts N fresh
    ranks before anything touches the GPU (here, without GPUs, the ranks fail and so does the parent): in neither case
    does a JSON line come out."""
    import subprocess
    import sys

    env = dict(os.environ, RANK="0", WORLD_SIZE="2", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 2 and "refusing" in p.stderr and "{" not in p.stdout
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if zk_has_gpu():
        pytest.skip("a GPU is visible: the spawn path is exercised by the GPU suite")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--log-n", "13"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode != 0 and '"n_gpus"' not in p.stdout
    assert "starting 2 ranks" in p.stderr


def zk_has_gpu():
    from zkmi_loader import load_pkg

    return load_pkg().Zkmi().device_count() > 0


def test_public_point_encoding_known_answers_on_the_product(zk):
    """The published encodings of test_cpu_oracle.PUBLIC_KATS through the product's host code (wire.hip, curve.hpp)."""
    from test_cpu_oracle import PUBLIC_KATS

    g1, g2 = zk.g1_generator(), zk.g2_generator()
    k = lambda v: int(v).to_bytes(32, "little")
    assert zk.g1_compress(g1).hex() == PUBLIC_KATS["g1_x1"]
    assert zk.g1_compress(zk.g1_mul(g1, k(2))).hex() == PUBLIC_KATS["g1_x2"]
    assert zk.g1_compress(zk.g1_add(zk.g1_mul(g1, k(2)), g1)).hex() == PUBLIC_KATS["g1_x3"]
    assert zk.g1_compress(zk.g1_mul(g1, k(ec.R - 1))).hex() == PUBLIC_KATS["g1_neg"]
    assert zk.g2_compress(zk.g2_mul(g2, k(2))).hex() == PUBLIC_KATS["g2_x2"]
    assert zk.g2_compress(zk.g2_add(g2, g2)).hex() == PUBLIC_KATS["g2_x2"]
    assert zk.g1_decompress(H(PUBLIC_KATS["g1_x3"])) == zk.g1_mul(g1, k(3))


def test_ctx_create_without_gpu_fails_loudly(zk, pkg):
    if zk.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(pkg.ZkmiError) as e:
        zk.context(0)
    assert e.value.code == -4  # ZKMI_ERR_NO_DEVICE: no silent CPU fallback


def test_wire_and_compression(zk):
    c = golden("constants.json")
    assert zk.g1_generator().hex() == c["g1"] and zk.g2_generator().hex() == c["g2"]
    assert zk.g1_compress(H(c["g1"])).hex() == c["g1_compressed"]
    assert zk.g2_compress(H(c["g2"])).hex() == c["g2_compressed"]
    assert zk.g1_decompress(H(c["g1_compressed"])).hex() == c["g1"]
    assert zk.g2_decompress(H(c["g2_compressed"])).hex() == c["g2"]
    assert zk.g1_mul(H(c["g1"]), (0xC0FFEE).to_bytes(32, "little")).hex() == c["g1_times_c0ffee"]
    assert zk.g2_mul(H(c["g2"]), (0xC0FFEE).to_bytes(32, "little")).hex() == c["g2_times_c0ffee"]
    assert zk.g1_mul(H(c["g1"]), ec.fr_to_bytes(ec.R - 1)).hex() == c["g1_times_r_minus_1"]
    # P + (-P) = infinity, infinity encodings
    assert zk.g1_add(H(c["g1"]), H(c["g1_times_r_minus_1"])) == bytes(96)
    assert zk.g1_compress(bytes(96)) == bytes([0xC0]) + bytes(47)
    assert zk.g1_decompress(bytes([0xC0]) + bytes(47)) == bytes(96)
    assert zk.g2_compress(bytes(192)) == bytes([0xC0]) + bytes(95)


def test_rejects_bad_points_and_scalars(zk, pkg):
    g = bytearray(zk.g1_generator())
    g[0] ^= 1
    with pytest.raises(pkg.ZkmiError) as e:
        zk.g1_compress(bytes(g))
    assert e.value.code == -2
    with pytest.raises(pkg.ZkmiError) as e:
        zk.g1_mul(zk.g1_generator(), ec.R.to_bytes(32, "little"))
    assert e.value.code == -2


def test_pairing_matches_oracle(zk):
    pg = golden("pairing.json")
    p = ec.g1_to_bytes(ec.g1_mul(pg["a"]))
    q = ec.g2_to_bytes(ec.g2_mul(pg["b"]))
    gt = zk.pairing(p, q)
    co = [int.from_bytes(gt[48 * i : 48 * i + 48], "little") for i in range(12)]
    poly = [0] * 12  # tower basis -> Fq[w]/(w^12 - 2w^6 + 2): u = w^6 - 1, v = w^2
    idx = 0
    for i in range(2):
        for j in range(3):
            for u in range(2):
                c = co[idx]
                idx += 1
                e = 2 * j + i
                if u == 0:
                    poly[e] = (poly[e] + c) % ec.P
                else:
                    poly[e + 6] = (poly[e + 6] + c) % ec.P
                    poly[e] = (poly[e] - c) % ec.P
    assert [hex(v) for v in poly] == pg["e_aG1_bG2"]


def test_shielder_relation_matches_oracle(zk):
    lg = 7
    r = zk.shielder_r1cs(lg)
    ro = g16.shielder_r1cs(lg)
    assert (r.n_vars, r.n_pub, r.n_constraints, r.log_n) == (ro.n_vars, ro.n_pub, ro.n_constraints, ro.log_n)
    for m, M in enumerate((ro.A, ro.B, ro.C)):
        rp, cl, vl = r.export(m)
        rows = [
            [(cl[k], int.from_bytes(vl[32 * k : 32 * k + 32], "little")) for k in range(rp[i], rp[i + 1])]
            for i in range(r.n_constraints)
        ]
        assert rows == [[(j, c % ec.R) for j, c in row] for row in M]
    w = zk.shielder_witness(lg, 42)
    assert w == b"".join(ec.fr_to_bytes(v) for v in g16.shielder_witness(lg, 42))
    assert r.is_satisfied(w)
    bad = bytearray(w)
    bad[32 * 50] ^= 1
    assert not r.is_satisfied(bytes(bad))
    # round trip through the generic CSR constructor
    r2 = zk.r1cs_create(r.n_vars, r.n_pub, [r.export(m) for m in range(3)])
    assert r2.is_satisfied(w) and r2.log_n == r.log_n
    r.free()
    r2.free()


def test_shielder_relation_shape_at_config0_size(zk):
    r = zk.shielder_r1cs(14)
    assert r.n_vars == 1 << 14 and r.n_constraints + r.n_pub == 1 << 14 and r.log_n == 14
    assert r.is_satisfied(zk.shielder_witness(14, 1))
    r.free()


def test_msm_plans_are_consistent(zk):
    """Host logic of the bucket plans for every size the ABI admits: the digits cover 255 bits, the bucket array is
    2^(c-1) wide, a partition fits the 2^15-counter LDS histogram, the prover's table index (digit * n + point) leaves
    bit 31 to the sign up to 2^26 terms, a group of proofs has at most 64 partitions, and the digit widths are the
    ones DESIGN.md 4.1 quotes."""
    import ctypes as C

    out = (C.c_uint32 * 6)()
    quoted = {12: 13, 13: 13, 14: 15, 15: 15, 16: 16, 17: 17, 18: 17, 19: 17, 20: 20, 22: 20, 26: 20}
    for lg in range(0, 28):
        for n in {1 << lg, (1 << lg) - 1, (1 << lg) + 1} - {0}:
            for shared in (0, 1):
                if n > (1 << 28) - 1:
                    continue
                assert zk.lib.zkmi_msm_plan_query(C.c_uint64(n), C.c_int32(shared), out) == 0
                c, nd, parts, nb, seg_log, heavy = list(out)
                assert 4 <= c <= 22 and nd * c >= 255 and (nb & (nb - 1)) == 0
                assert (1 << seg_log) <= nb and heavy >= 1
                # a tile histogram holds 2^15 counters: shared plans cut the bucket set into partitions of that size, and
                # so does the windowed plan of >= 2^24 terms (20-bit windows = 16 partitions each, at most 256 groups)
                if shared or n < 1 << 24:
                    assert nb <= 1 << 15
                else:
                    assert c == 20 and nb == 1 << 19 and parts * (nb >> 15) <= 256
                if shared:
                    assert parts * nb == 1 << (c - 1) and parts <= 64
                    if lg <= 26:
                        assert nd * n < 1 << 31
                    if n == 1 << lg and lg in quoted:
                        assert c == quoted[lg], (lg, c)
                    if lg <= 19:  # groups of 2^(20 - lg) proofs (at most 64) keep within 64 partitions
                        assert min(64, 1 << max(0, 20 - lg)) * parts <= 64 or lg < 14
                else:
                    assert nb == 1 << (c - 1) and parts == nd and parts * c >= 255
    assert zk.lib.zkmi_msm_plan_query(C.c_uint64(0), C.c_int32(0), out) != 0


RUN_SCHEDULE_FIELDS = (
    "nwin c tot_b segs_per_win tot_segs seg seg_bits njobs plain_job t_job level2 segs2 tot_segs2 wide quad_seg quad_tree "
    "quad_redo quad_heavy nchunk nq tree_block tree_lds final_block final_lds accum fused heavy_nc partials_per_msm "
    "lanes slice_segs quad_per_wave SLOT_PTS STAGE_PTS_1 STAGE_PTS TREE_T SEG2_MIN_SEGS SEG2_LOG").split()


def _msm_hpp_enum(name, prefix):
    """{enumerator without `prefix`: value} of `enum name { A = 0, ... };` as csrc/msm.hpp writes it (every value explicit)."""
    src = open(os.path.join(ROOT, "zk-apps_amd", "csrc", "msm.hpp")).read()
    body = re.search(r"\benum %s \{([^}]*)\};" % name, src).group(1)
    return {k[len(prefix):]: int(v) for k, v in re.findall(r"\b(%s\w+) = (\d+)" % prefix, body)}


_FORMS, _KINDS = _msm_hpp_enum("MsmAccumForm", "MSM_ACCUM_"), _msm_hpp_enum("MsmEngineKind", "MSM_ENGINE_")
ACCUM_G1, ACCUM_G1_MULTI, ACCUM_G1_SPLIT2, ACCUM_G2, ACCUM_G2_SPLIT2 = (_FORMS[k] for k in ("G1", "G1_MULTI", "G1_SPLIT2", "G2", "G2_SPLIT2"))
ENGINE_G1, ENGINE_G2, ENGINE_BN254 = (_KINDS[k] for k in ("G1", "G2", "BN254"))
assert len(_FORMS) == 5 and len(_KINDS) == 3


def run_schedule(zk, n, shared, engine, host_spin, nm, plan_n=0, flags=0):
    import types

    out = (C.c_int32 * len(RUN_SCHEDULE_FIELDS))()
    rc = zk.tlib.zkmi_selftest_msm_run_schedule(C.c_uint64(n), C.c_int32(shared), C.c_uint64(plan_n), C.c_int32(engine),
                                                C.c_int32(host_spin), C.c_int32(nm), C.c_int32(flags), out, C.c_uint32(len(out)))
    assert rc == 0, (rc, n, shared, engine, host_spin, nm, plan_n)
    return types.SimpleNamespace(**dict(zip(RUN_SCHEDULE_FIELDS, out)))


def test_msm_run_schedules_fit_their_buffers_and_kernels(zk):
    """The launch schedule MsmEngine::run_device_multi decides up front (csrc/msm_impl.hpp msm_run_schedule), read through the
    testing library without a GPU, for every engine, both callers (one MSM or proof by itself / the batch pipeline), windowed
    and shared-bucket plans, one and four MSMs per call, n = 2^5 .. 2^26 and the 2^24 plan over a small n.  The bounds are
    those of the buffers (MsmEngine::reserve: SLOT_PTS partials per slot, MSM_STAGE_PTS staged slices of which the one-lane
    tree sums use the first MSM_STAGE_PTS_1) and of the kernels (treesum_final_body: one point per slice in ONE workgroup of
    at most MSM_TREE_T points; treesum_body: a slice workgroup takes slice_segs segments at once; k_segreduce2: 16 segment
    sums per super-segment; TreeLevel2 is a parameter of the one-lane / lane-pair tree sums only), all exported by the hook.
    The quad / octet final sum strides over its slices a wave at a time (msm_quad.hpp k_treesum_final_q), so its slices are
    held to the stage and to "none empty", not to a workgroup's points."""
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    cases = [(1 << k, shared, 0) for k in range(5, 27) for shared in (0, 1)] + [((1 << 12) - 3, 0, 1 << 24)]
    seen = set()
    for n, shared, plan_n in cases:
        for engine in (ENGINE_G1, ENGINE_G2, ENGINE_BN254):
            for host_spin in (0, 1):
                for nm in (1, 4):
                    s = run_schedule(zk, n, shared, engine, host_spin, nm, plan_n)
                    what = (n, shared, plan_n, engine, host_spin, nm, vars(s))
                    lists = s.njobs * s.nwin
                    assert s.lanes == (2 if engine == ENGINE_G2 else 1)
                    assert lists <= s.SLOT_PTS and (2 + s.seg_bits) * s.nwin <= s.SLOT_PTS, what
                    assert s.njobs * s.nwin == s.partials_per_msm, what
                    assert s.segs_per_win == 1 << s.seg_bits and s.tot_segs == s.nwin * s.segs_per_win, what
                    # one-lane / lane-pair slices
                    assert pow2(s.nchunk) and s.nchunk <= s.TREE_T and lists * s.nchunk <= s.STAGE_PTS_1, what
                    assert s.final_block // s.lanes >= s.nchunk and s.final_block <= s.lanes * s.TREE_T, what
                    assert s.nchunk == 1 or s.nchunk * s.slice_segs <= s.segs_per_win, what
                    assert s.tree_block <= s.lanes * s.TREE_T and s.tree_block % 64 == 0 and s.final_block % 64 == 0, what
                    # quad / octet slices
                    assert pow2(s.nq) and lists * s.nq <= s.STAGE_PTS, what
                    assert s.nq == 1 or s.nq * s.quad_per_wave <= s.segs_per_win, what
                    # second level
                    if s.level2:
                        assert shared and s.segs_per_win >= s.SEG2_MIN_SEGS and s.segs_per_win % 16 == 0, what
                        assert not s.quad_seg and not s.quad_tree, what
                        assert s.segs2 << s.SEG2_LOG == s.segs_per_win and s.tot_segs2 == s.nwin * s.segs2, what
                        assert s.t_job == s.njobs - 2 and s.plain_job == s.njobs - 1, what
                    else:
                        assert s.t_job == -1 and s.plain_job == (s.njobs - 1 if shared else -1), what
                    assert s.wide == (not shared and s.c > 16), what
                    if s.wide:
                        assert not s.quad_seg and not s.quad_tree, what
                    # what the documents say in words
                    if not s.wide:  # one MSM by itself takes all four quad stages, the batch pipeline only redo and heavy
                        assert (s.quad_seg, s.quad_tree, s.quad_redo, s.quad_heavy) == ((1, 1, 1, 1) if host_spin else (0, 0, 1, 1)), what
                    if engine == ENGINE_G2:
                        assert s.accum == (ACCUM_G2_SPLIT2 if host_spin and s.tot_b <= 1 << 15 else ACCUM_G2) and not s.fused, what
                    else:
                        assert s.fused == (nm > 1), what
                        assert s.accum == ((ACCUM_G1_SPLIT2 if s.tot_b <= 1 << 16 else ACCUM_G1_MULTI) if nm > 1 else ACCUM_G1), what
                    seen.add((s.accum, bool(s.level2), s.nchunk > 1, s.nq > 1, bool(s.wide)))
    assert {a for a, *_ in seen} == {ACCUM_G1, ACCUM_G1_MULTI, ACCUM_G1_SPLIT2, ACCUM_G2, ACCUM_G2_SPLIT2}
    assert any(l2 for _, l2, *_ in seen) and any(w for *_, w in seen)
    # the 13-window, 20-bit plan: two-wave segment sums (no quad form) and 16 tree slices (13 windows x 16 jobs x 16 <= 4096)
    for n, plan_n in ((1 << 24, 0), ((1 << 12) - 3, 1 << 24)):
        s = run_schedule(zk, n, 0, ENGINE_G1, 1, 1, plan_n)
        assert (s.c, s.nwin, s.wide, s.quad_seg, s.quad_tree, s.nchunk) == (20, 13, 1, 0, 0, 16), vars(s)
        assert s.quad_redo and not s.heavy_nc and not s.quad_heavy  # (the partitioned windows' heavy lists stay with the complete-law kernel)
    for bad in ((0, 0, 0, 0, 1, 1), (1 << 12, 0, 0, 3, 1, 1), (1 << 12, 0, 0, 0, 1, 5), (1 << 12, 1, 1 << 24, 0, 1, 1)):
        n, shared, plan_n, engine, host_spin, nm = bad
        out = (C.c_int32 * len(RUN_SCHEDULE_FIELDS))()
        assert zk.tlib.zkmi_selftest_msm_run_schedule(C.c_uint64(n), C.c_int32(shared), C.c_uint64(plan_n), C.c_int32(engine),
                                                      C.c_int32(host_spin), C.c_int32(nm), C.c_int32(0), out, C.c_uint32(len(out))) != 0


def test_assembly_scalar_multiplications_selftest(zk):
    """Host arithmetic of proof assembly: fixed-base delta tables and the joint s*A + r*B1 multiplication equal
    plain double-and-add in G1 and G2 (scalars 0, 1, r - 1 and random; P + P and P - P in the joint form)."""
    import ctypes as C

    bad = C.c_uint32(99)
    assert zk.tlib.zkmi_selftest_assembly(C.c_uint64(21), C.c_uint32(12), C.byref(bad)) == 0
    assert bad.value == 0


def test_host_pool_and_cpu_budget(zk):
    """The prover's host side (csrc/host_pool.hpp): the persistent assembly pool runs every item exactly once under
    concurrent callers, and the thread budget follows what the process is granted, divided by the ranks of the node."""
    import ctypes as C
    import subprocess
    import sys

    bad = C.c_uint32(99)
    assert zk.tlib.zkmi_selftest_host_pool(C.c_uint32(6), C.c_uint32(300), C.byref(bad)) == 0
    assert bad.value == 0
    info = zk.host_info()
    assert 1 <= info["threads"] <= min(16, info["cpus_granted"]) and info["pool_workers"] <= 16
    assert info["cpus_granted"] <= os.cpu_count()
    zk.set_host_threads(3)
    assert zk.host_info()["threads"] == 3
    zk.set_host_threads(0)
    assert zk.host_info()["threads"] == info["threads"]
    # a rank of an 8-process job gets an eighth of the grant (at least one thread); ZKMI_HOST_THREADS overrides
    code = ("import sys; sys.path.insert(0, %r)\nfrom zkmi_loader import load_pkg\n"
            "print(sorted(load_pkg().Zkmi().host_info().items()))\n" % ROOT)
    def child(**env):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZKMI_SHARE_TORCH_HIP="0", **env),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return dict(eval(out.stdout.strip().splitlines()[-1]))
    eight = child(LOCAL_WORLD_SIZE="8")
    assert eight["local_ranks"] == 8 and eight["threads"] == max(1, min(16, eight["cpus_granted"] // 8))
    assert child(LOCAL_WORLD_SIZE="8", ZKMI_HOST_THREADS="5")["threads"] == 5


def test_host_verifier_on_golden_proof(zk):
    gd = golden("groth16_n128.json")
    wit = H(gd["witness"])
    publics = wit[32 : 32 * 7]
    assert zk.groth16_verify(H(gd["vk"]), publics, H(gd["proof"])) is True
    bad = bytearray(publics)
    bad[5] ^= 0x10
    assert zk.groth16_verify(H(gd["vk"]), bytes(bad), H(gd["proof"])) is False
    # proof with A and C swapped is rejected
    pr = H(gd["proof"])
    assert zk.groth16_verify(H(gd["vk"]), publics, pr[144:] + pr[48:144] + pr[:48]) is False


def test_msm_window_combine_host(zk):
    """zkmi_msm_g1_combine (the local step after the all-gather of SURVEY §8e)."""
    c, nwin = 13, 255 // 13 + 1
    rng = ec.SplitMix64(5)
    ks = [[rng.fr() for _ in range(nwin)] for _ in range(2)]
    wins = b"".join(ec.g1_to_bytes(ec.g1_mul(k)) for r in ks for k in r)
    exp = sum((ks[0][w] + ks[1][w]) << (c * w) for w in range(nwin)) % ec.R
    assert zk.msm_g1_combine(wins, 2, nwin, c) == ec.g1_to_bytes(ec.g1_mul(exp))


def _xyzz_host_bytes(pt, lam):
    """An affine oracle point as the XYZZ value (x lam^2, y lam^3, lam^2, lam^3) in the library's host form: four 48-byte
    little-endian Montgomery residues (R = 2^384); None = infinity = zeros."""
    if pt is None:
        return bytes(192)
    x, y = pt
    mont = lambda v: ((v % ec.P) * pow(2, 384, ec.P) % ec.P).to_bytes(48, "little")
    l2, l3 = lam * lam % ec.P, lam * lam * lam % ec.P
    return mont(x * l2) + mont(y * l3) + mont(l2) + mont(l3)


@pytest.mark.parametrize("n_ranks", [1, 2, 8])
def test_exchange_combine_at_the_real_slot_layout(zk, n_ranks):
    """What every rank computes behind ncclAllGather (csrc/comm.hip), at the slot geometry of BASELINE config 3 -- the plan of
    2^26 terms: 13 windows of 20 bits, 14 partial sums per window, the partial top window spread over 16 partitions --
    with up to 8 synthetic ranks, in both partitions (points / windows).  The slots hold known multiples of the
    generator in non-trivial XYZZ form (and some points at infinity); the expected scalar follows from the reduction's
    definition: window = job_0 + 2^seg_log * sum_j 2^j job_(1+j), the top window without its top_spread_log top bits."""
    plan_n = 1 << 26
    lay = zk.msm_exchange_layout(plan_n, n_ranks)
    # (64-bucket segments since round 5: 2^19 / 64 = 2^13 segments per window -> 1 + 13 partial sums)
    assert (lay["nwin"], lay["per_window"], lay["c"], lay["seg_log"], lay["top_spread_log"]) == (13, 14, 20, 6, 4)
    assert lay["slot_pts_points"] == 13 * 14 and lay["point_bytes"] == 192
    nwin, per, c, seg_log = lay["nwin"], lay["per_window"], lay["c"], lay["seg_log"]
    rng = ec.SplitMix64(0x5A4B0003 + n_ranks)
    small = lambda: rng.fr() & ((1 << 48) - 1)

    def window_value(w, jobs):
        bits = per - 1 - (lay["top_spread_log"] if w == nwin - 1 else 0)
        return jobs[0] + (1 << seg_log) * sum(jobs[1 + j] << j for j in range(bits))

    # --- point split: every rank holds all windows
    total, slots = 0, []
    for k in range(n_ranks):
        for w in range(nwin):
            jobs = [small() if (k + w + j) % 7 else 0 for j in range(per)]
            total += window_value(w, jobs) << (c * w)
            slots += [_xyzz_host_bytes(ec.g1_mul(v) if v else None, 2 + rng.fr() % ec.P) for v in jobs]
    got = zk.msm_g1_combine_partials(b"".join(slots), n_ranks, plan_n, window_split=False)
    assert got == ec.g1_to_bytes(ec.g1_mul(total % ec.R))
    # --- window split: rank k holds windows [k nwin / R, (k + 1) nwin / R) at the head of an equal-sized slot
    first = lambda k: k * nwin // n_ranks
    max_w = max(first(k + 1) - first(k) for k in range(n_ranks))
    assert lay["slot_pts_windows"] == per * max_w
    total, slots = 0, []
    for k in range(n_ranks):
        mine = []
        for w in range(first(k), first(k + 1)):
            jobs = [small() if (k + w + j) % 5 else 0 for j in range(per)]
            total += window_value(w, jobs) << (c * w)
            mine += [_xyzz_host_bytes(ec.g1_mul(v) if v else None, 2 + rng.fr() % ec.P) for v in jobs]
        # whatever lies behind a rank's own windows is ignored by the readers: fill it with a valid but wrong point
        mine += [_xyzz_host_bytes(ec.g1_mul(12345), 1)] * (per * max_w - len(mine))
        slots += mine
    got = zk.msm_g1_combine_partials(b"".join(slots), n_ranks, plan_n, window_split=True)
    assert got == ec.g1_to_bytes(ec.g1_mul(total % ec.R))
    # --- 2-D split (round 6): rank k = g Q + q holds window range q of Q over point group g; a window's value is the sum
    # over the point groups.  Every Q that divides the rank count (Q = 1 is the point split's arithmetic in window-range
    # slots, Q = n_ranks the window split's).
    for Q in [q for q in (2, 4, 8) if n_ranks % q == 0 and q <= n_ranks]:
        firstq = lambda q: q * nwin // Q
        max_wq = max(firstq(q + 1) - firstq(q) for q in range(Q))
        assert zk.msm_exchange_layout(plan_n, Q)["slot_pts_windows"] == per * max_wq
        total, slots = 0, []
        for k in range(n_ranks):
            q = k % Q
            mine = []
            for w in range(firstq(q), firstq(q + 1)):
                jobs = [small() if (k + w + j) % 6 else 0 for j in range(per)]
                total += window_value(w, jobs) << (c * w)
                mine += [_xyzz_host_bytes(ec.g1_mul(v) if v else None, 2 + rng.fr() % ec.P) for v in jobs]
            mine += [_xyzz_host_bytes(ec.g1_mul(54321), 1)] * (per * max_wq - len(mine))
            slots += mine
        got = zk.msm_g1_combine_partials(b"".join(slots), n_ranks, plan_n, window_split=Q)
        assert got == ec.g1_to_bytes(ec.g1_mul(total % ec.R)), Q
    # a window-range count that does not divide the ranks is refused
    if n_ranks == 8:
        with pytest.raises(Exception):
            zk.msm_g1_combine_partials(bytes(192 * per * 13 * 8), 8, plan_n, window_split=3)


def test_rccl_not_found_is_an_error_code_not_a_crash(tmp_path):
    """include/zkmi.h: a host without RCCL loads the library and gets ZKMI_ERR_RCCL from the zkmi_comm_* calls only
    (round 4 dereferenced a null dlerror() here).  Fresh process: the lookup is cached."""
    import subprocess
    import sys

    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "from zkmi_loader import load_pkg\n"
        "pkg = load_pkg(); zk = pkg.Zkmi()\n"
        "try:\n"
        "    zk.comm_unique_id()\n"
        "except pkg.ZkmiError as e:\n"
        "    print('code', e.code)\n"
        "print('plan', zk.msm_plan_query(1 << 20)[0])\n" % ROOT
    )
    env = dict(os.environ, ZKMI_RCCL_LIB=str(tmp_path / "no_such_librccl.so"), ZKMI_SHARE_TORCH_HIP="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "code -9" in out.stdout and "plan 16" in out.stdout, out.stdout
    # the product does not dlopen whatever the environment names: a relative path, and a world-writable
    # file, are refused with the same error code -- and never fall back to another RCCL
    fake = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
    loose = tmp_path / "libloose.so"
    loose.write_bytes(open(fake, "rb").read() if os.path.exists(fake) else b"\x7fELF")
    os.chmod(loose, 0o777)
    for bad in ("tests/fake_rccl/libfake_rccl.so", str(loose)):
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, ZKMI_RCCL_LIB=bad, ZKMI_DEBUG="1"), capture_output=True,
                             text=True, timeout=120, cwd=ROOT)
        assert out.returncode == 0 and "code -9" in out.stdout and "ZKMI_RCCL_LIB refused" in out.stderr, (bad, out.stdout, out.stderr)


# ------------------------------------------------ mocked_zk mirror (row a12)
def _tokens():
    return [bytes([228] * 32), bytes(32)]  # MOCKED_TOKEN, shielder/mocked_zk/src/lib.rs:18


def _empty_note_proof(zk, id_, nullifier, trapdoor):
    acc = zk.account_new(_tokens())
    h = zk.note_hash(id_, trapdoor, nullifier, zk.account_hash(acc))
    user = (1).to_bytes(16, "little") + bytes(16)  # mocked_user()
    return h, zk.zkproof_new(id_, trapdoor, nullifier, zk.op_priv(user), acc)


def test_mock_boundary_golden_vectors(zk):
    m = golden("mock_boundary.json")
    acc = zk.account_new(_tokens())
    assert zk.account_hash(acc).hex() == m["account_hash_empty"]
    z32 = bytes(32)
    assert zk.note_hash(z32, z32, z32, zk.account_hash(acc)).hex() == m["empty_note_hash"]
    s1 = (1).to_bytes(16, "little") + bytes(16)
    s2 = (2).to_bytes(16, "little") + bytes(16)
    cur = zk.combine_merkle_hash(s1, s2)
    for _ in range(9):
        cur = zk.combine_merkle_hash(cur, z32)
    assert cur.hex() == m["merkle_root_two_leaves"]


def test_create_note(zk):
    """shielder/mocked_zk/src/tests.rs:27-35"""
    z32 = bytes(32)
    h, proof = _empty_note_proof(zk, z32, z32, z32)
    zk.zkproof_verify_creation(proof, h, _tokens())


def test_create_note_fails(zk, pkg):
    """shielder/mocked_zk/src/tests.rs:37-51"""
    z32 = bytes(32)
    _, proof = _empty_note_proof(zk, z32, z32, z32)
    h_other, _ = _empty_note_proof(zk, (1).to_bytes(16, "little") + bytes(16), z32, z32)
    with pytest.raises(pkg.ZkmiError) as e:
        zk.zkproof_verify_creation(proof, h_other, _tokens())
    assert e.value.name == "VerificationError"


def test_deposit_withdraw_flow(zk, pkg):
    """Prove-side sequence of drink_tests/utils/shielder.rs:78-134 against the
    verify side of contract/lib.rs:63-78, with the Merkle path semantics of
    contract/merkle.rs:89-102 (missing sibling = zero scalar)."""
    z32 = bytes(32)
    user = (1).to_bytes(16, "little") + bytes(16)
    token = _tokens()[0]
    ident = (7).to_bytes(16, "little") + bytes(16)
    h0, p0 = _empty_note_proof(zk, ident, (11).to_bytes(32, "little"), (12).to_bytes(32, "little"))
    path = [z32] * 10  # single-leaf tree: zero siblings, leaf id 0
    root = h0
    for s in path:
        root = zk.combine_merkle_hash(root, s)
    dep = zk.op_pub("deposit", 10, token, user)
    h1, p1 = zk.zkproof_update_account(p0, dep, zk.op_priv(user), (13).to_bytes(32, "little"), (14).to_bytes(32, "little"), path, 0)
    zk.zkproof_verify_update(p1, dep, h1, root, (11).to_bytes(32, "little"))
    with pytest.raises(pkg.ZkmiError) as e:  # wrong old nullifier
        zk.zkproof_verify_update(p1, dep, h1, root, (99).to_bytes(32, "little"))
    assert e.value.name == "VerificationError"
    other = zk.op_pub("deposit", 10, token, (2).to_bytes(16, "little") + bytes(16))
    with pytest.raises(pkg.ZkmiError) as e:  # ops.rs:47-63
        zk.zkproof_verify_update(p1, other, h1, root, (11).to_bytes(32, "little"))
    assert e.value.name == "OperationCombineError"
    wd = zk.op_pub("withdraw", 11, token, user)
    with pytest.raises(pkg.ZkmiError) as e:  # account.rs:57-62 checked_sub
        zk.zkproof_update_account(p1, wd, zk.op_priv(user), z32, z32, path, 0)
    assert e.value.name == "AccountUpdateError"
    unk = zk.op_pub("deposit", 1, bytes([9] * 32), user)
    with pytest.raises(pkg.ZkmiError) as e:  # unknown token
        zk.zkproof_update_account(p1, unk, zk.op_priv(user), z32, z32, path, 0)
    assert e.value.name == "AccountUpdateError"
    wd9 = zk.op_pub("withdraw", 9, token, user)
    h2, p2 = zk.zkproof_update_account(p1, wd9, zk.op_priv(user), z32, z32, path, 0)
    assert bytes(p2.acc_new.balances[0][1].bytes)[:16] == (1).to_bytes(16, "little")


def test_account_hash_quirk_only_second_balance(zk):
    """account.rs:16-24 hashes only balances[1].1 — token-0 deposits do not change it."""
    user = (1).to_bytes(16, "little") + bytes(16)
    acc = zk.account_new(_tokens())
    acc2 = zk.account_update(acc, zk.op_pub("deposit", 5, _tokens()[0], user), zk.op_priv(user))
    assert zk.account_hash(acc) == zk.account_hash(acc2)


def test_device_limb_representation_selftest(zk):
    """field28.hpp (the MSM kernels' 28-bit-limb Fq) executed on the host
    against the 32-bit-limb arithmetic: mixed-add-shaped chains, zero tests."""
    import ctypes as C

    bad = C.c_uint32(1)
    assert zk.tlib.zkmi_selftest_fq28(C.c_uint64(7), C.c_uint32(5000), C.byref(bad)) == 0
    assert bad.value == 0


def test_witness_from_semantic_inputs(zk):
    """Row a1: the assignment built from the relation's semantic inputs (order of
    UpdateNoteInput::new, update_note.rs:47-88) equals the seeded generator's and satisfies the relation."""
    lg = 8
    w = zk.shielder_witness(lg, 77)
    f = lambda i: w[32 * i : 32 * i + 32]
    shape = [f(14 + i)[0] for i in range(10)]
    inp = zk.update_note_input(f(1), f(2), f(3), f(6), [f(7 + k) for k in range(4)], f(12), f(13), shape,
                               [f(24 + i) for i in range(10)], [f(35), f(36)])
    w2 = zk.shielder_witness_from_input(lg, inp)
    assert w2 == w
    r = zk.shielder_r1cs(lg)
    assert r.is_satisfied(w2)
    r.free()


def test_fr_reduce(zk, pkg):
    import hashlib

    h = hashlib.sha256(b"note").digest()
    v = int.from_bytes(h, "little")
    assert int.from_bytes(zk.fr_reduce(h), "little") == v % ec.R
    assert zk.fr_reduce(bytes(32)) == bytes(32)
    assert int.from_bytes(zk.fr_reduce(b"\xff" * 32), "little") == (2**256 - 1) % ec.R
    # a non-canonical scalar is rejected by the witness builder
    inp = zk.update_note_input(*([b"\xff" * 32] * 4), [bytes(32)] * 4, bytes(32), bytes(32), [0] * 10, [bytes(32)] * 10, [bytes(32)] * 2)
    with pytest.raises(pkg.ZkmiError) as e:
        zk.shielder_witness_from_input(8, inp)
    assert e.value.code == -2


def test_poseidon_constants_match_oracle(zk):
    """The library's Grain/Cauchy generator (host code in poseidon.hip) == oracle/poseidon.py for
    both fields; the oracle in turn is pinned by published BN254 vectors (test_cpu_oracle.py)."""
    from oracle import poseidon as ps

    for field, name in ((0, "bls12_381_fr"), (1, "bn254_fr")):
        rc, mds = zk.poseidon_spec(field)
        orc, omds = ps.spec(name)
        assert rc == [list(r) for r in orc]
        assert mds == [list(r) for r in omds]
    assert zk.poseidon_spec(1)[0][0][0] != zk.poseidon_spec(0)[0][0][0]


def _note_update_case(zk, seed, op_kind, amount=250, balances=(1000, 77), slot=0, height=10):
    """A valid update_note instance + the values the oracle's Poseidon gives for its hashes."""
    from oracle import bls12_381 as ec
    from oracle import poseidon as ps

    rng = ec.SplitMix64(seed)
    tok = [rng.fr(), rng.fr()]
    bal = list(balances)
    new_id, old_id, ot, on, nt, nn, user = (rng.fr() for _ in range(7))
    old_acc = ps.hash_fix_len([tok[0], bal[0], tok[1], bal[1]])
    old_note = ps.hash_fix_len([old_id, ot, on, old_acc])
    shape = [rng.next() & 1 for _ in range(height)]
    path = [rng.fr() for _ in range(height)]
    root = ps.merkle_root(old_note, shape, path)
    nb = list(bal)
    nb[slot] += amount if op_kind == 0 else -amount
    new_acc = ps.hash_fix_len([tok[0], nb[0], tok[1], nb[1]])
    new_note = ps.hash_fix_len([new_id, nt, nn, new_acc])
    inp = zk.note_update(amount, tok[slot], user, (new_id, nt, nn), (old_id, ot, on), shape, path, user,
                         (tok[0], bal[0], tok[1], bal[1]))
    publics = [amount, tok[slot], user, new_note, root, on]
    return inp, publics


def test_update_note_relation_hashes_match_oracle(zk):
    """The Poseidon relation (update_note.rs:106-149 as R1CS): the witness generator's note hash and
    Merkle root equal oracle/poseidon.py, the assignment satisfies the exported matrices under the
    oracle's own R1CS evaluation, and tampering any public input breaks it."""
    from oracle import groth16 as g16
    from oracle.bls12_381 import R

    lg = 14
    for op_kind, slot in ((1, 0), (0, 1)):
        r1 = zk.update_note_r1cs(lg, op_kind)
        assert (r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n) == (1 << lg, 7, (1 << lg) - 7, lg)
        inp, publics = _note_update_case(zk, 40 + op_kind, op_kind, slot=slot)
        w, pub, rc = zk.update_note_witness(lg, op_kind, inp)
        assert rc == 0 and pub == publics
        assert w[32:224] == b"".join(v.to_bytes(32, "little") for v in publics)
        assert r1.is_satisfied(w)
        # independent evaluation by the oracle's R1CS class on the exported CSR
        rows = []
        for m in range(3):
            rp, cl, vl = r1.export(m)
            vals = [int.from_bytes(vl[32 * k : 32 * k + 32], "little") for k in range(len(cl))]
            rows.append([[(cl[k], vals[k]) for k in range(rp[i], rp[i + 1])] for i in range(r1.n_constraints)])
        z_int = [int.from_bytes(w[32 * i : 32 * i + 32], "little") for i in range(1 << lg)]
        oracle_r1 = g16.R1CS(r1.n_vars, r1.n_pub, *rows)
        assert oracle_r1.is_satisfied(z_int)
        for k in range(1, 7):
            bad = list(z_int)
            bad[k] = (bad[k] + 1) % R
            assert not oracle_r1.is_satisfied(bad), "public %d not bound" % k
        r1.free()


from note_update_cases import oracle_r1cs as _oracle_r1cs  # noqa: E402  (shared with test_cpu_note_update_edges.py)


def test_update_note_relation_tree_height_is_a_runtime_field(zk, pkg):
    """TREE_HEIGHT is a const generic of the reference (merkle_proof.rs:11): heights other than the
    mock's 10 give a relation of another shape whose root still equals the oracle's fold, the builder and
    the value-only synthesis agree, and a key for one height does not accept another height's witness."""
    lg = 14
    r10 = zk.update_note_r1cs(lg, 1)
    for height in (1, 4, 20):
        r1 = zk.update_note_r1cs(lg, 1, tree_height=height)
        assert (r1.n_vars, r1.n_pub, r1.n_constraints) == (1 << lg, 7, (1 << lg) - 7)
        inp, publics = _note_update_case(zk, 900 + height, 1, height=height)
        assert inp.tree_height == height
        w, pub, rc = zk.update_note_witness(lg, 1, inp)
        assert rc == 0 and pub == publics
        assert r1.is_satisfied(w) and not r10.is_satisfied(w)
        wv, rcv = zk.update_note_witness_values_host(lg, 1, inp)
        assert rcv == 0 and wv == w
        r1.free()
    # height 32 does not fit 2^13 rows; an out-of-range height is an argument error
    with pytest.raises(pkg.ZkmiError) as e:
        zk.update_note_r1cs(13, 1, tree_height=32)
    assert e.value.code == -1
    with pytest.raises(pkg.ZkmiError) as e:
        zk.update_note_r1cs(14, 1, tree_height=33)
    assert e.value.code == -1
    r13 = zk.update_note_r1cs(13, 1)  # the relation proper fits 2^13 (config 0 is quoted at 2^14)
    inp, publics = _note_update_case(zk, 77, 1)
    w, pub, rc = zk.update_note_witness(13, 1, inp)
    assert rc == 0 and pub == publics and r13.is_satisfied(w)
    r13.free()
    r10.free()


def test_create_note_relation_matches_oracle(zk):
    """The creation relation (what ZkProof::verify_creation stands for, relations.rs:127-136):
    publics h_note_new | token_0 | token_1, h_note_new = Poseidon(id, trapdoor, nullifier,
    Poseidon(token_0, 0, token_1, 0)) as oracle/poseidon.py computes it; the assignment satisfies the
    exported matrices under the oracle's evaluator and every public input is bound."""
    from oracle import bls12_381 as ec
    from oracle import poseidon as ps
    from oracle.bls12_381 import R

    lg = 12
    r1 = zk.create_note_r1cs(lg)
    assert (r1.n_vars, r1.n_pub, r1.n_constraints, r1.log_n) == (1 << lg, 4, (1 << lg) - 4, lg)
    rng = ec.SplitMix64(4242)
    tok = (rng.fr(), rng.fr())
    note = (rng.fr(), rng.fr(), rng.fr())
    w, pub = zk.create_note_witness(lg, zk.note_create(tok, note))
    acc_hash = ps.hash_fix_len([tok[0], 0, tok[1], 0])
    assert pub == [ps.hash_fix_len([note[0], note[1], note[2], acc_hash]), tok[0], tok[1]]
    assert w[32:128] == b"".join(v.to_bytes(32, "little") for v in pub)
    assert r1.is_satisfied(w)
    orc = _oracle_r1cs(r1)
    z_int = [int.from_bytes(w[32 * i : 32 * i + 32], "little") for i in range(1 << lg)]
    assert orc.is_satisfied(z_int)
    for k in range(1, 4):
        bad = list(z_int)
        bad[k] = (bad[k] + 1) % R
        assert not orc.is_satisfied(bad), "public %d not bound" % k
    # another note under the same tokens: different hash, same shape
    w2, pub2 = zk.create_note_witness(lg, zk.note_create(tok, (note[0], note[1], note[2] + 1)))
    assert pub2[0] != pub[0] and r1.is_satisfied(w2)
    r1.free()


def test_oracle_side_witness_solver_reproduces_both_relations(zk):
    """oracle/relation_witness.py: loaded values by the reference's load order with oracle/poseidon.py hashes + a generic
    solver over the exported matrices (products, is_zero pairs, range-check bits).  The solved assignment satisfies the
    oracle's evaluator and equals the product generator's bytes for deposit, withdraw (2^13) and the creation relation (2^12);
    a loaded hash that is off by one makes the solver raise (the constraint system computes the oracle's Poseidon)."""
    from oracle import bls12_381 as ec
    from oracle import relation_witness as rw

    height = 10
    for op_kind in (0, 1):
        r1 = zk.update_note_r1cs(13, op_kind)
        rng = ec.SplitMix64(0xA11 + op_kind)
        tok = [rng.fr(), rng.fr()]
        bal, amount, slot = [900, 40], 25, 1 - op_kind
        new_note, old_note = (rng.fr(), rng.fr(), rng.fr()), (rng.fr(), rng.fr(), rng.fr())
        user = rng.fr()
        shape = [rng.next() & 1 for _ in range(height)]
        path = [rng.fr() for _ in range(height)]
        acct = (tok[0], bal[0], tok[1], bal[1])
        loaded = rw.update_note_loaded(op_kind, amount, tok[slot], user, new_note, old_note, shape, path, user, acct)
        orc = _oracle_r1cs(r1)
        z_int = rw.solve(r1.n_vars, orc.A, orc.B, orc.C, loaded)
        assert orc.is_satisfied(z_int)
        inp = zk.note_update(amount, tok[slot], user, new_note, old_note, shape, path, user, acct)
        w, pub, rc = zk.update_note_witness(13, op_kind, inp)
        assert rc == 0 and w == b"".join(v.to_bytes(32, "little") for v in z_int)
        bad = list(loaded)
        bad[5] = (bad[5] + 1) % ec.R  # merkle_root
        with pytest.raises(ValueError):
            rw.solve(r1.n_vars, orc.A, orc.B, orc.C, bad)
        r1.free()
    r1 = zk.create_note_r1cs(12)
    rng = ec.SplitMix64(0xC4EA7E)
    tok, note = (rng.fr(), rng.fr()), (rng.fr(), rng.fr(), rng.fr())
    pubs, acc_hash = rw.create_note_loaded(tok, note)
    orc = _oracle_r1cs(r1)
    z_int = rw.solve(r1.n_vars, orc.A, orc.B, orc.C, pubs + [note[0], note[1], note[2], acc_hash])
    assert orc.is_satisfied(z_int)
    w, pub = zk.create_note_witness(12, zk.note_create(tok, note))
    assert w == b"".join(v.to_bytes(32, "little") for v in z_int) and pub == pubs[1:]
    r1.free()


def test_verifier_rejects_non_canonical_and_small_order_points(zk, pkg):
    """zkmi_groth16_verify is a validating verifier (as arkworks' deserialisation and the zcash format are):
    one encoding of infinity, and every proof point must lie in the r-order subgroup."""
    gd = golden("groth16_n128.json")
    vk, proof = H(gd["vk"]), H(gd["proof"])
    publics = H(gd["witness"])[32 : 32 * 7]
    assert zk.groth16_verify(vk, publics, proof) is True

    def rc_of(pr):
        import ctypes as C

        buf = lambda b: (C.c_uint8 * len(b)).from_buffer_copy(b)
        return zk.lib.zkmi_groth16_verify(buf(vk), C.c_uint32(7), buf(publics), buf(pr))

    # infinity with stray bits / bytes / the sort flag: not canonical
    inf1 = bytes([0xC0]) + bytes(47)
    for bad_inf in (bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01", bytes([0xC1]) + bytes(47)):
        assert rc_of(bad_inf + proof[48:]) == -2
        with pytest.raises(pkg.ZkmiError):
            zk.g1_decompress(bad_inf)
    assert rc_of(inf1 + proof[48:]) == -5  # canonical infinity parses; the pairing equation then fails
    assert rc_of(proof[:48] + bytes([0xC0]) + bytes(94) + b"\x01" + proof[144:]) == -2
    # a curve point outside G1: x = 4 gives y^2 = 68... search small x until decompression succeeds,
    # the cofactor makes a random curve point miss the subgroup with overwhelming probability
    found = None
    for x in range(1, 200):
        enc = bytearray(x.to_bytes(48, "big"))
        enc[0] |= 0x80
        try:
            aff = zk.g1_decompress(bytes(enc))
        except pkg.ZkmiError:
            continue
        if not zk.g1_in_subgroup(aff):
            found = bytes(enc)
            break
    assert found is not None
    assert zk.g1_in_subgroup(zk.g1_generator()) and zk.g2_in_subgroup(zk.g2_generator())
    assert rc_of(found + proof[48:]) == -2          # A outside the subgroup
    assert rc_of(proof[:144] + found) == -2         # C outside the subgroup
    # same for G2: x = (k, 0)
    found2 = None
    for x in range(1, 200):
        enc = bytearray(bytes(48) + x.to_bytes(48, "big"))
        enc[0] |= 0x80
        try:
            aff = zk.g2_decompress(bytes(enc))
        except pkg.ZkmiError:
            continue
        if not zk.g2_in_subgroup(aff):
            found2 = bytes(enc)
            break
    assert found2 is not None
    assert rc_of(proof[:48] + found2 + proof[144:]) == -2


def test_arkworks_vk_layout_round_trip(zk, pkg):
    """VerifyingKey in arkworks' CanonicalSerialize layout (restated in csrc/arkworks.hip and, independently, in
    oracle/ark_serialize.py): both restatements emit the same bytes, compressed and uncompressed, and the reader
    returns the original key; truncated or corrupted input is an error, not a crash."""
    from oracle import ark_serialize as ark

    gd = golden("groth16_n128.json")
    vk = H(gd["vk"])
    n_pub = (len(vk) - 672) // 96
    for compressed in (True, False):
        blob = zk.ark_vk_write(vk, n_pub, compressed)
        assert blob == ark.verifying_key(vk, n_pub, compressed)
        assert len(blob) == (48 + 3 * 96 + 8 + 48 * n_pub) * (1 if compressed else 2) - (0 if compressed else 8)
        back, n, used = zk.ark_vk_read(blob + b"tail", compressed)
        assert (back, n, used) == (vk, n_pub, len(blob))
        with pytest.raises(pkg.ZkmiError):
            zk.ark_vk_read(blob[:-1], compressed)
        bad = bytearray(blob)
        bad[5] ^= 1  # alpha_g1.x: no longer on the curve / not a valid x
        with pytest.raises(pkg.ZkmiError):
            zk.ark_vk_read(bytes(bad), compressed)
    # a compressed arkworks Proof is the 192-byte proof as is: A | B | C
    pr = H(gd["proof"])
    assert zk.g1_compress(zk.g1_decompress(pr[:48])) == pr[:48] and zk.g2_compress(zk.g2_decompress(pr[48:144])) == pr[48:144]


def test_r1cs_create_rejects_malformed_csr(zk, pkg):
    """The ABI promises an error code, not a crash: decreasing row pointers, columns out of range and
    domains beyond what the NTT supports are argument errors."""
    one = (1).to_bytes(32, "little")
    good = ([0, 1, 2], [1, 2], one + one)
    r = zk.r1cs_create(4, 2, [good, good, good])
    assert r.n_constraints == 2
    r.free()
    for bad in (([0, 2, 1], [1, 2], one + one), ([1, 1, 2], [1, 2], one + one), ([0, 1, 2], [1, 7], one + one)):
        with pytest.raises(pkg.ZkmiError) as e:
            zk.r1cs_create(4, 2, [bad, good, good])
        assert e.value.code == -1


def test_update_note_relation_rejects_impossible_updates(zk):
    """Account::update / Operation::combine failure modes of the mock (account.rs:37-82,
    ops.rs:47-63) come back as the same error codes and as unsatisfied assignments."""
    lg = 14
    r1 = zk.update_note_r1cs(lg, 1)
    base, _ = _note_update_case(zk, 7, 1)
    import copy

    def variant(**kw):
        i = copy.deepcopy(base)
        for name, v in kw.items():
            import ctypes as C
            C.memmove(getattr(i, name), int(v).to_bytes(32, "little"), 32)
        return i

    for inp, code in (
        (variant(amount=1001), -6),          # checked_sub underflow
        (variant(token=123456789), -6),      # token not in the account
        (variant(op_priv_user=5), -7),       # users differ
    ):
        w, _, rc = zk.update_note_witness(lg, 1, inp, check=False)
        assert rc == code
        assert not r1.is_satisfied(w)
    w, _, rc = zk.update_note_witness(lg, 1, variant(amount=1000))  # withdraw everything: fine
    assert rc == 0 and r1.is_satisfied(w)
    r1.free()


def test_poseidon_sparse_form_equals_definition(zk):
    """The kernels run the partial rounds in the sparse form (one scalar constant + a sparse matrix
    per round); host execution of the same code must equal the plain 64-round definition."""
    import ctypes as C

    for field in (0, 1):
        bad = C.c_uint32(1)
        assert zk.tlib.zkmi_selftest_poseidon(C.c_int32(field), C.c_uint64(11 + field), C.c_uint32(40), C.byref(bad)) == 0
        assert bad.value == 0


def test_update_note_value_synthesis_equals_constraint_builder(zk):
    """The value-only synthesis the GPU runs (relation_values.hpp, executed on the host here) yields
    the same assignment, byte for byte, as the constraint builder — valid and impossible updates."""
    import copy
    import ctypes as C

    lg = 14
    for op_kind, slot in ((1, 0), (1, 1), (0, 1)):
        inp, _ = _note_update_case(zk, 300 + 2 * op_kind + slot, op_kind, amount=50, slot=slot)
        w, _, rc = zk.update_note_witness(lg, op_kind, inp)
        wv, rcv = zk.update_note_witness_values_host(lg, op_kind, inp)
        assert rc == rcv == 0
        assert wv == w
    base, _ = _note_update_case(zk, 8, 1)
    for field, value, code in (("amount", 1001, -6), ("token", 99, -6), ("op_priv_user", 5, -7)):
        i = copy.deepcopy(base)
        C.memmove(getattr(i, field), int(value).to_bytes(32, "little"), 32)
        w, _, rc = zk.update_note_witness(lg, 1, i, check=False)
        wv, rcv = zk.update_note_witness_values_host(lg, 1, i)
        assert rc == rcv == code
        assert wv == w


def test_update_note_witness_matches_golden_publics(zk):
    """The seeded update_note instance of tests/golden/poseidon.json: the library's witness generator
    (host code) returns exactly the committed public inputs (note hash and Merkle root = Poseidon-5)."""
    from conftest import golden

    g = golden("poseidon.json")["update_note_withdraw"]
    i = lambda v: int(v, 16) if isinstance(v, str) else int(v)
    inp = zk.note_update(g["amount"], i(g["token"]), i(g["user"]), [i(v) for v in g["new_note"]], [i(v) for v in g["old_note"]],
                         g["path_shape"], [i(v) for v in g["path"]], i(g["user"]), [i(v) for v in g["account"]])
    _, pub, rc = zk.update_note_witness(14, 1, inp)
    assert rc == 0 and [hex(v) for v in pub] == g["publics"]
    rc_first = zk.poseidon_spec(0)[0][0][0]
    assert hex(rc_first) == golden("poseidon.json")["bls12_381_fr"]["rc_first"]
    import hashlib

    for field, name in ((0, "bls12_381_fr"), (1, "bn254_fr")):
        rc_, mds = zk.poseidon_spec(field)
        flat = b"".join(v.to_bytes(32, "little") for row in rc_ for v in row) + b"".join(v.to_bytes(32, "little") for row in mds for v in row)
        assert hashlib.sha256(flat).hexdigest() == golden("poseidon.json")[name]["constants_sha256"]


def _build_c_example(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "prove_withdraw")
    lib_dir = os.path.join(root, "zk-apps_amd")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "prove_withdraw.c"), "-L" + lib_dir, "-lzkmi",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def _build_c_bench(tmp_path):
    """examples/bench_prove.c: plain C that also calls the HIP runtime directly (hipMalloc), linked against /opt/rocm --
    the runtime libzkmi.so was built for; no Python, no PyTorch in that process."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bench_prove")
    lib_dir = os.path.join(root, "zk-apps_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"),
                           "-I/opt/rocm/include", os.path.join(root, "examples", "bench_prove.c"), "-L" + lib_dir, "-lzkmi",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_c_bench_builds_and_fails_loudly_without_gpu(tmp_path):
    """examples/bench_prove.c (the torch-free twin of bench.py + scripts/churn.py) compiles with -Wall -Werror against the
    header; without a GPU it stops at zkmi_ctx_create."""
    import subprocess

    import torch

    exe = _build_c_bench(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the GPU test")
    p = subprocess.run([exe, "--proofs", "1"], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


def test_c_example_builds_against_the_header_and_fails_loudly_without_gpu(tmp_path):
    """include/zkmi.h is plain C: examples/prove_withdraw.c compiles with gcc -Wall -Werror and links
    libzkmi.so; on a machine without a GPU it stops at zkmi_ctx_create (no CPU fallback)."""
    import subprocess

    import torch

    exe = _build_c_example(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the GPU test")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no CPU fallback" in p.stderr


def test_library_carries_the_digest_of_its_sources(zk):
    """zkmi_version() returns the digest of the sources the binary was BUILT from (Makefile: src_digest.o); it must equal the
    digest of the files beside it -- the .so files are git-ignored and travel prebuilt, and bench.py / smoke() print the same
    comparison as `library_matches_sources`.  Both libraries."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import src_digest
    finally:
        sys.path.pop(0)
    want = src_digest.csrc_digest(ROOT)
    assert re.fullmatch(r"zkmi 0\.1 \(gfx950\) src:[0-9a-f]{16}", zk.version()), zk.version()
    assert zk.src_digest() == want, "libzkmi.so is stale: run __graft_entry__.build()"
    zk.tlib.zkmi_version.restype = C.c_char_p
    assert zk.tlib.zkmi_version().decode() == "zkmi 0.1 (gfx950) src:%s exp" % want
    import bench

    assert bench.csrc_digest() == want
    rev = bench.source_revision(zk)
    assert rev["library_matches_sources"] is True and rev["library_src_sha256_16"] == want


def test_struct_layouts_agree_between_product_and_testing_library(zk):
    """Tests and bench.py create inputs in libzkmi_exp.so on a context made by libzkmi.so (Zkmi.tlib): both export a
    fingerprint of the struct layouts involved, the binding refuses to pair them when they differ."""
    a, b = zk.abi_layout(zk.lib), zk.abi_layout(zk.tlib)
    assert a == b and len(a) >= 20 and a[0] > 1000  # (sizeof(zkmi_ctx) first)
    n = C.c_uint32(0)
    assert zk.lib.zkmi_abi_layout_probe((C.c_uint64 * 2)(), C.c_uint32(2), C.byref(n)) == -1 and n.value == len(a)


def test_kernel_register_budgets():
    """The allocations the design stands on, read from the code objects inside the built library (scripts/kernel_resources.py;
    no GPU needed): the accumulation kernels and the quad-split reduction kernels are one-wave workgroups of at most 168
    VGPRs -- three waves per SIMD, each placed in the slot another one frees -- and the hot ones have
    no scratch.  k_accum_g1_nc's zero-spill allocation at exactly 168 is, by msm_impl.hpp's own comment, a draw of the register
    allocator that an edit nearby can lose: this test is what notices."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    ks = {kr.short_name(n): v for n, v in kr.kernels(os.path.join(ROOT, "zk-apps_amd", "libzkmi.so")).items()}
    assert len(ks) > 100
    # kernel: (max VGPRs + AGPRs, max scratch bytes per lane)
    budgets = {
        "k_accum_g1_nc<Fq28,3,1,0,0>": (168, 0), "k_accum_g1_nc<Fq28,3,1,1,0>": (168, 0),
        "k_accum_g1_nc<BnFq28,3,1,0,0>": (168, 0), "k_accum_g2_nc<Fq2,2,1>": (256, 0),
        "k_accum_heavy_nc<Fq28,3>": (168, 96), "k_accum_heavy_nc_g2<Fq2,2>": (256, 0),
        "k_accum_g2_split2<Fq2,0>": (320, 0),  # one wave per SIMD by design (one small G2 MSM by itself)
        # quad (G1, BN254 G1: <F, 0, 0>) and octet (G2: <Fq28, 0, 1>, two waves per SIMD) forms of the reduction-side kernels
        "k_segreduce_q<Fq28,0,0>": (168, 0), "k_treesum_q<Fq28,0,0>": (168, 0), "k_treesum_final_q<Fq28,0,0>": (168, 0),
        "k_accum_redo_q<Fq28,0,0>": (168, 0), "k_heavy_q<Fq28,0,0>": (168, 64),
        "k_segreduce_q<BnFq28,0,0>": (168, 0), "k_treesum_q<BnFq28,0,0>": (168, 0), "k_heavy_q<BnFq28,0,0>": (168, 0),
        "k_segreduce_q<Fq28,0,1>": (256, 0), "k_treesum_q<Fq28,0,1>": (256, 0), "k_treesum_final_q<Fq28,0,1>": (256, 0),
        "k_accum_redo_q<Fq28,0,1>": (256, 0), "k_heavy_q<Fq28,0,1>": (256, 0),
    }
    for name, (regs, scratch) in budgets.items():
        assert name in ks, (name, sorted(k for k in ks if k.startswith(name.split("<")[0])))
        k = ks[name]
        assert k["vgpr"] + k["agpr"] <= regs and k["scratch"] <= scratch and not k["dynamic_stack"], (name, k)
