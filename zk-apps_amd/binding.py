"""ctypes binding of include/zkmi.h (one Python method per C entry point).

Mirrors the reference's caller-side conventions: scalars are
32-byte little-endian `bytes`, points are affine wire bytes, errors surface as
`ZkmiError(code)` with the code names of `ZkpError`
(shielder/mocked_zk/src/errors.rs:3-7) where they apply.
"""
import ctypes as C
import os

ERR = {
    0: "OK",
    -1: "BAD_ARG",
    -2: "NON_CANONICAL",
    -3: "HIP",
    -4: "NO_DEVICE",
    -5: "VerificationError",
    -6: "AccountUpdateError",
    -7: "OperationCombineError",
    -8: "UNSATISFIED",
    -9: "RCCL",
}
PHASES = {
    "msm_sort": 0,
    "msm_accum_g1": 1,
    "msm_reduce_g1": 2,
    "msm_accum_g2": 3,
    "msm_reduce_g2": 4,
    "ntt": 5,
    "witness": 6,
    "misc": 7,
}
# point encodings, checks and per-element status bytes of the device point readers (include/zkmi.h)
ENC_WIRE, ENC_ZCASH_COMPRESSED, ENC_ZCASH_UNCOMPRESSED = 0, 1, 2
CHECK_CURVE, CHECK_SUBGROUP = 1, 2
PT_OK, PT_BAD_ENCODING, PT_NOT_ON_CURVE, PT_NOT_IN_SUBGROUP = 0, 1, 2, 3
NO_INDEX = (1 << 64) - 1
# masks of Context.srs_verify / Context.pk_verify_contribution (include/zkmi.h)
SRS_BAD_TAU_G1, SRS_BAD_TAU_G2, SRS_BAD_ALPHA, SRS_BAD_BETA, SRS_BAD_BETA_G2, SRS_DEGENERATE = 1, 2, 4, 8, 16, 32
PK2_FIXED_PART_DIFFERS, PK2_BAD_DELTA, PK2_BAD_H, PK2_BAD_L = 1, 2, 4, 8
# on top of the SRS_* mask of `after`: Context.srs_verify_contribution
SRS_STEP_BAD_TAU, SRS_STEP_BAD_ALPHA, SRS_STEP_BAD_BETA, SRS_STEP_DEGENERATE = 256, 512, 1024, 2048
MERKLE_TREE_DEPTH = 10
MAX_TREE_HEIGHT = 32
TOKENS_NUMBER = 2


class ZkmiError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        self.name = ERR.get(code, str(code))
        super().__init__(f"zkmi error {code} ({self.name}) {detail}".strip())


def lib_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libzkmi.so")


class Scalar(C.Structure):
    _fields_ = [("bytes", C.c_uint8 * 32)]


class Account(C.Structure):
    _fields_ = [("balances", (Scalar * 2) * TOKENS_NUMBER)]


class OpPub(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("amount", C.c_uint8 * 16), ("token", Scalar), ("user", Scalar)]


class OpPriv(C.Structure):
    _fields_ = [("user", Scalar)]


class NoteUpdate(C.Structure):
    """zkmi_note_update (include/zkmi.h): semantic inputs of the Poseidon update_note relation."""

    _fields_ = [
        ("amount", C.c_uint8 * 32), ("token", C.c_uint8 * 32), ("user", C.c_uint8 * 32),
        ("new_note", (C.c_uint8 * 32) * 3), ("old_note", (C.c_uint8 * 32) * 3),
        ("tree_height", C.c_uint32),
        ("path_shape", C.c_uint8 * MAX_TREE_HEIGHT), ("path", (C.c_uint8 * 32) * MAX_TREE_HEIGHT),
        ("op_priv_user", C.c_uint8 * 32), ("account", (C.c_uint8 * 32) * 4),
    ]


class NoteCreate(C.Structure):
    """zkmi_note_create: semantic inputs of the creation relation."""

    _fields_ = [("tokens", (C.c_uint8 * 32) * TOKENS_NUMBER), ("note", (C.c_uint8 * 32) * 3)]


class UpdateNoteInput(C.Structure):
    """zkmi_update_note_input: semantic inputs of the withdraw-shaped relation (row a1)."""

    _fields_ = [
        ("amount", Scalar), ("token", Scalar), ("user", Scalar),
        ("old_nullifier", Scalar),
        ("new_note", Scalar * 4),
        ("old_trapdoor", Scalar), ("old_account_hash", Scalar),
        ("path_shape", C.c_uint8 * MERKLE_TREE_DEPTH),
        ("path", Scalar * MERKLE_TREE_DEPTH),
        ("old_account", Scalar * TOKENS_NUMBER),
    ]


class ZkProof(C.Structure):
    _fields_ = [
        ("id", Scalar),
        ("trapdoor_new", Scalar),
        ("trapdoor_old", Scalar),
        ("nullifier_new", Scalar),
        ("acc_old", Account),
        ("acc_new", Account),
        ("op_priv", OpPriv),
        ("merkle_proof", Scalar * MERKLE_TREE_DEPTH),
        ("merkle_proof_leaf_id", C.c_uint32),
    ]


def scalar(b):
    s = Scalar()
    b = bytes(b)
    assert len(b) == 32
    C.memmove(s.bytes, b, 32)
    return s


def scalar_u128(v):
    return scalar(int(v).to_bytes(16, "little") + bytes(16))


def _buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(bytes(b)) if len(b) else (C.c_uint8 * 1)()


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels carry their own libamdhip64.so / libhsa-runtime64.so (RPATH $ORIGIN) and ask for them by
    the unversioned name, so a process that loads libzkmi.so (NEEDED libamdhip64.so.7 -> /opt/rocm) BEFORE importing
    torch ends up with two HIP runtimes, and the second one to initialise finds no GPU.  Loading torch's copy first
    (its SONAME is libamdhip64.so.7 too) makes both sides resolve to the same runtime whatever the import order.
    No torch installed, or torch already imported: nothing to do."""
    import importlib.util
    import sys

    if os.environ.get("ZKMI_SHARE_TORCH_HIP", "1") == "0":  # opt-out: a host that never imports torch in this process
        return
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


class Zkmi:
    """Loads libzkmi.so.  Fails loudly if it is missing (no fallback path)."""

    def __init__(self, path=None):
        path = path or os.environ.get("ZKMI_LIB") or lib_path()
        if not os.path.exists(path):
            raise ZkmiError(-4, f"{path} not built; run __graft_entry__.build()")
        _share_hip_runtime_with_torch()
        self.lib = C.CDLL(path)
        self.lib.zkmi_version.restype = C.c_char_p
        self.lib.zkmi_last_error.restype = C.c_char_p
        self.lib.zkmi_last_error.argtypes = [C.c_void_p]
        self._tlib = None

    @property
    def tlib(self):
        """The TESTING library (include/zkmi_testing.h: synthetic bases, the chain stand-in relation, host self-tests) --
        test scaffolding the product library does not export.  It is the A/B + testing build libzkmi_exp.so; the objects it
        creates are the product's own types, and a context made by the product library is the same struct there (one
        source tree), so tests manufacture inputs here and hand them to libzkmi.so."""
        if self._tlib is None:
            if hasattr(self.lib, "zkmi_selftest_fq28"):
                self._tlib = self.lib  # ZKMI_LIB selected the A/B + testing library itself
            else:
                path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libzkmi_exp.so")
                if not os.path.exists(path):
                    raise ZkmiError(-4, f"{path} (testing library) not built; run __graft_entry__.build()")
                self._tlib = C.CDLL(path)
                # objects cross between the two libraries (a product context drives testing-library code and back): refuse
                # to pair builds whose struct layouts differ instead of corrupting memory silently
                mine, theirs = self.abi_layout(self.lib), self.abi_layout(self._tlib)
                if mine != theirs:
                    self._tlib = None
                    raise ZkmiError(-1, f"libzkmi.so and libzkmi_exp.so disagree on struct layouts: {mine} vs {theirs}; rebuild both")
            self._tlib.zkmi_selftest_group_ops.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                           C.c_void_p]
        return self._tlib

    @staticmethod
    def abi_layout(lib):
        """zkmi_abi_layout_probe of `lib` as a tuple."""
        out, n = (C.c_uint64 * 64)(), C.c_uint32(0)
        rc = lib.zkmi_abi_layout_probe(out, C.c_uint32(64), C.byref(n))
        if rc != 0:
            raise ZkmiError(rc, "zkmi_abi_layout_probe")
        return tuple(out[: n.value])

    def src_digest(self):
        """The source digest compiled into the loaded library (zkmi_version(): 'src:<digest>')."""
        v = self.version()
        return v.split("src:", 1)[1].split()[0] if "src:" in v else None

    def hip_versions(self):
        """(HIP_VERSION of the build, version of the HIP runtime this process bound the library to)."""
        b, r = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.zkmi_hip_versions(C.byref(b), C.byref(r)))
        return b.value, r.value

    def host_info(self):
        """zkmi_host_info: dict(cpus_granted, local_ranks, threads, pool_workers)."""
        out = (C.c_uint32 * 4)()
        self._chk(self.lib.zkmi_host_info(out))
        return dict(zip(("cpus_granted", "local_ranks", "threads", "pool_workers"), out))

    def set_host_threads(self, n):
        self._chk(self.lib.zkmi_set_host_threads(C.c_uint32(n)))

    def version(self):
        return self.lib.zkmi_version().decode()

    def device_count(self):
        n = C.c_int32(0)
        self.lib.zkmi_device_count(C.byref(n))
        return n.value

    def _chk(self, rc, ctx=None):
        if rc != 0:
            detail = ""
            if ctx is not None:
                detail = (self.lib.zkmi_last_error(ctx) or b"").decode()
            raise ZkmiError(rc, detail)

    # ---- host-only helpers --------------------------------------------------
    def g1_generator(self):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_g1_generator(out))
        return bytes(out)

    def g2_generator(self):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_g2_generator(out))
        return bytes(out)

    def g1_compress(self, a):
        out = (C.c_uint8 * 48)()
        self._chk(self.lib.zkmi_g1_compress(_buf(a), out))
        return bytes(out)

    def g1_decompress(self, a):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_g1_decompress(_buf(a), out))
        return bytes(out)

    def g2_compress(self, a):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_g2_compress(_buf(a), out))
        return bytes(out)

    def g2_decompress(self, a):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_g2_decompress(_buf(a), out))
        return bytes(out)

    def g1_mul(self, a, k):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_g1_mul(_buf(a), _buf(k), out))
        return bytes(out)

    def g2_mul(self, a, k):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_g2_mul(_buf(a), _buf(k), out))
        return bytes(out)

    def g1_add(self, a, b):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_g1_add(_buf(a), _buf(b), out))
        return bytes(out)

    def g2_add(self, a, b):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_g2_add(_buf(a), _buf(b), out))
        return bytes(out)

    def pairing(self, p, q):
        out = (C.c_uint8 * 576)()
        self._chk(self.lib.zkmi_pairing(_buf(p), _buf(q), out))
        return bytes(out)

    def msm_plan_query(self, n, shared=False):
        """(digit bits, digits, windows | partitions, buckets per window | partition, log2 segment length, heavy threshold)"""
        out = (C.c_uint32 * 6)()
        self._chk(self.lib.zkmi_msm_plan_query(C.c_uint64(n), C.c_int32(1 if shared else 0), out))
        return tuple(out)

    def comm_unique_id(self):
        """128 bytes from ncclGetUniqueId (rank 0 calls; the host layer hands them to every rank)"""
        out = (C.c_uint8 * 128)()
        self._chk(self.lib.zkmi_comm_unique_id(out))
        return bytes(out)

    def msm_g1_combine(self, windows, n_ranks, nwin, window_bits):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1_combine(_buf(windows), C.c_uint32(n_ranks), C.c_uint32(nwin), C.c_uint32(window_bits), out))
        return bytes(out)

    def msm_exchange_layout(self, plan_n, n_ranks=1):
        """zkmi_msm_exchange_layout: dict of the slot geometry of the two RCCL exchanges for a plan of plan_n terms."""
        out = (C.c_uint32 * 8)()
        self._chk(self.lib.zkmi_msm_exchange_layout(C.c_uint64(plan_n), C.c_uint32(n_ranks), out))
        keys = ("nwin", "per_window", "slot_pts_points", "slot_pts_windows", "point_bytes", "c", "seg_log", "top_spread_log")
        return dict(zip(keys, out))

    def msm_g1_combine_partials(self, partials, n_ranks, plan_n, window_split=False):
        """zkmi_msm_g1_combine_partials: the host combination behind the all-gather, on caller-supplied slots."""
        out = (C.c_uint8 * 96)()
        # window_split: False / 0 = point split, True / 1 = window split, Q >= 2 = the 2-D split with Q window ranges
        self._chk(self.lib.zkmi_msm_g1_combine_partials(_buf(partials), C.c_uint32(n_ranks), C.c_uint64(plan_n),
                                                        C.c_int32(int(window_split)), out))
        return bytes(out)

    def host_info_string(self):
        self.lib.zkmi_host_info_string.restype = C.c_char_p
        return self.lib.zkmi_host_info_string().decode()

    def msm_g1_multi(self, ctxs, dptrs, counts, bases):
        """One MSM split by points over several contexts (one per GPU) of this process."""
        k = len(ctxs)
        assert k == len(dptrs) == len(counts) == len(bases) and k > 0
        a_ctx = (C.c_void_p * k)(*[c.h.value for c in ctxs])
        a_ptr = (C.c_void_p * k)(*[int(p) for p in dptrs])
        a_cnt = (C.c_uint64 * k)(*counts)
        a_bas = (C.c_void_p * k)(*[b.h.value for b in bases])
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1_multi(a_ctx, C.c_uint32(k), a_ptr, a_cnt, a_bas, out))
        return bytes(out)

    def groth16_prove_batch_multi(self, ctxs, pks, z_ptrs, on_device, rs, ss):
        """zkmi_groth16_prove_batch_multi: proof i runs on ctxs[i % len(ctxs)] with the key replica pks[i % len(ctxs)]."""
        nd, n = len(ctxs), len(z_ptrs)
        cs = (C.c_void_p * nd)(*[c.h.value for c in ctxs])
        ks = (C.c_void_p * nd)(*[k.h.value for k in pks])
        ptrs = (C.c_void_p * max(1, n))(*z_ptrs)
        out = (C.c_uint8 * max(1, 192 * n))()
        rc = self.lib.zkmi_groth16_prove_batch_multi(cs, ks, C.c_uint32(nd), C.c_uint32(n), ptrs, C.c_int32(int(on_device)),
                                                     _buf(b"".join(rs)), _buf(b"".join(ss)), out)
        if rc != 0:
            msgs = "; ".join((self.lib.zkmi_last_error(c.h) or b"").decode() for c in ctxs)
            raise ZkmiError(rc, msgs)
        raw = bytes(out)
        return [raw[192 * i: 192 * i + 192] for i in range(n)]

    def groth16_verify(self, vk, publics, proof):
        n_pub = (len(vk) - 672) // 96
        assert len(publics) == 32 * (n_pub - 1)
        rc = self.lib.zkmi_groth16_verify(_buf(vk), C.c_uint32(n_pub), _buf(publics), _buf(proof))
        if rc == 0:
            return True
        if rc == -5:
            return False
        raise ZkmiError(rc)

    def vk_prepare(self, vk):
        """zkmi_vk_prepare: the verifying key validated once (what zkmi_groth16_verify re-checks at every call), for
        Context.groth16_verify_batch.  A refused key raises ZkmiError (NON_CANONICAL)."""
        n_pub = (len(vk) - 672) // 96
        h = C.c_void_p()
        self._chk(self.lib.zkmi_vk_prepare(_buf(vk), C.c_uint32(n_pub), C.byref(h)))
        return PreparedVk(self, h, n_pub)

    # ---- R1CS ---------------------------------------------------------------
    def shielder_r1cs(self, log_n):
        h = C.c_void_p()
        self._chk(self.tlib.zkmi_shielder_r1cs(C.c_uint32(log_n), C.byref(h)))
        return R1cs(self, h)

    def shielder_witness(self, log_n, seed):
        out = (C.c_uint8 * (32 << log_n))()
        self._chk(self.tlib.zkmi_shielder_witness(C.c_uint32(log_n), C.c_uint64(seed), out))
        return bytes(out)

    # ---- Poseidon-5 ---------------------------------------
    def poseidon_spec(self, field=0):
        """(round constants [64][5], mds [5][5]) as ints, straight from the library's generator."""
        rc = (C.c_uint8 * (32 * 64 * 5))()
        mds = (C.c_uint8 * (32 * 25))()
        self._chk(self.lib.zkmi_poseidon_spec(C.c_int32(field), rc, mds))
        r, m = bytes(rc), bytes(mds)
        ints = lambda raw, n: [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(n)]
        rl, ml = ints(r, 320), ints(m, 25)
        return [rl[5 * i : 5 * i + 5] for i in range(64)], [ml[5 * i : 5 * i + 5] for i in range(5)]

    # ---- update_note relation with real Poseidon hashing --------------------
    def update_note_r1cs(self, log_n, op_kind, tree_height=MERKLE_TREE_DEPTH):
        h = C.c_void_p()
        self._chk(self.lib.zkmi_update_note_r1cs_h(C.c_uint32(log_n), C.c_int32(op_kind), C.c_uint32(tree_height), C.byref(h)))
        return R1cs(self, h)

    def create_note_r1cs(self, log_n):
        h = C.c_void_p()
        self._chk(self.lib.zkmi_create_note_r1cs(C.c_uint32(log_n), C.byref(h)))
        return R1cs(self, h)

    def note_create(self, tokens, note):
        """Integers in: tokens = (token_0, token_1), note = (zk_id, trapdoor, nullifier)."""
        i = NoteCreate()
        for k in range(2):
            C.memmove(i.tokens[k], int(tokens[k]).to_bytes(32, "little"), 32)
        for k in range(3):
            C.memmove(i.note[k], int(note[k]).to_bytes(32, "little"), 32)
        return i

    def create_note_witness(self, log_n, inp):
        """(z bytes, [h_note_new, token_0, token_1] as ints)."""
        out = (C.c_uint8 * (32 << log_n))()
        pub = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_create_note_witness(C.c_uint32(log_n), C.byref(inp), out, pub))
        p = bytes(pub)
        return bytes(out), [int.from_bytes(p[32 * k : 32 * k + 32], "little") for k in range(3)]

    def g1_in_subgroup(self, a):
        return self.lib.zkmi_g1_in_subgroup(_buf(a)) == 0

    def g2_in_subgroup(self, a):
        return self.lib.zkmi_g2_in_subgroup(_buf(a)) == 0

    # ---- keys in arkworks' CanonicalSerialize layout --------------------------
    def ark_vk_read(self, buf, compressed):
        cap = 672 + 96 * 64
        out = (C.c_uint8 * cap)()
        n_pub, used = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.zkmi_ark_vk_read(_buf(buf), C.c_uint64(len(buf)), C.c_int32(int(compressed)), out, C.c_uint64(cap),
                                            C.byref(n_pub), C.byref(used)))
        return bytes(out)[: 672 + 96 * n_pub.value], n_pub.value, used.value

    def ark_vk_write(self, vk, n_pub, compressed):
        need = C.c_uint64()
        self.lib.zkmi_ark_vk_write(_buf(vk), C.c_uint32(n_pub), C.c_int32(int(compressed)), None, C.c_uint64(0), C.byref(need))
        out = (C.c_uint8 * need.value)()
        self._chk(self.lib.zkmi_ark_vk_write(_buf(vk), C.c_uint32(n_pub), C.c_int32(int(compressed)), out, need, C.byref(need)))
        return bytes(out)

    # ---- the ZkProof surface with real proofs ---------------
    def shielder_verify_creation(self, vk_create, h_note_new, tokens, proof):
        arr = (Scalar * TOKENS_NUMBER)(*[scalar(t) for t in tokens])
        h = scalar(h_note_new)
        self._chk(self.lib.zkmi_shielder_verify_creation(_buf(vk_create), C.byref(h), arr, _buf(proof)))

    def shielder_verify_update(self, vk_deposit, vk_withdraw, op_pub, h_note_new, merkle_root, nullifier_old, proof):
        a = [scalar(x) for x in (h_note_new, merkle_root, nullifier_old)]
        vd = _buf(vk_deposit) if vk_deposit else None
        vw = _buf(vk_withdraw) if vk_withdraw else None
        self._chk(self.lib.zkmi_shielder_verify_update(vd, vw, C.byref(op_pub), *[C.byref(x) for x in a], _buf(proof)))

    def note_update(self, amount, token, user, new_note, old_note, path_shape, path, op_priv_user, account):
        """Integers in, zkmi_note_update out (new_note / old_note = (zk_id, trapdoor, nullifier),
        account = (token_0, balance_0, token_1, balance_1))."""
        i = NoteUpdate()
        put = lambda dst, v: C.memmove(dst, int(v).to_bytes(32, "little"), 32)
        put(i.amount, amount), put(i.token, token), put(i.user, user), put(i.op_priv_user, op_priv_user)
        for k in range(3):
            put(i.new_note[k], new_note[k]), put(i.old_note[k], old_note[k])
        height = len(path)
        assert len(path_shape) == height and 1 <= height <= MAX_TREE_HEIGHT
        i.tree_height = height
        for k in range(height):
            i.path_shape[k] = int(path_shape[k])
            put(i.path[k], path[k])
        for k in range(4):
            put(i.account[k], account[k])
        return i

    def update_note_witness(self, log_n, op_kind, inp, check=True):
        """(z bytes, [6 public ints], status); raises on a non-zero status unless check=False."""
        out = (C.c_uint8 * (32 << log_n))()
        pub = (C.c_uint8 * (32 * 6))()
        rc = self.lib.zkmi_update_note_witness(C.c_uint32(log_n), C.c_int32(op_kind), C.byref(inp), out, pub)
        if check or rc in (-1, -2):
            self._chk(rc)
        p = bytes(pub)
        return bytes(out), [int.from_bytes(p[32 * k : 32 * k + 32], "little") for k in range(6)], rc

    def update_note_witness_values_host(self, log_n, op_kind, inp):
        """The device code path (value-only synthesis) executed on the host; test hook."""
        out = (C.c_uint8 * (32 << log_n))()
        rc = self.lib.zkmi_update_note_witness_values_host(C.c_uint32(log_n), C.c_int32(op_kind), C.byref(inp), out)
        if rc in (-1, -2):
            self._chk(rc)
        return bytes(out), rc

    def fr_reduce(self, b32):
        out = (C.c_uint8 * 32)()
        self._chk(self.lib.zkmi_fr_reduce(_buf(b32), out))
        return bytes(out)

    def update_note_input(self, amount, token, user, old_nullifier, new_note, old_trapdoor, old_account_hash,
                          path_shape, path, old_account):
        """All scalar arguments are 32-byte canonical LE values (use fr_reduce for SHA-256 outputs)."""
        i = UpdateNoteInput()
        i.amount, i.token, i.user, i.old_nullifier = scalar(amount), scalar(token), scalar(user), scalar(old_nullifier)
        for k in range(4):
            i.new_note[k] = scalar(new_note[k])
        i.old_trapdoor, i.old_account_hash = scalar(old_trapdoor), scalar(old_account_hash)
        for k in range(MERKLE_TREE_DEPTH):
            i.path_shape[k] = int(path_shape[k])
            i.path[k] = scalar(path[k])
        for k in range(TOKENS_NUMBER):
            i.old_account[k] = scalar(old_account[k])
        return i

    def shielder_witness_from_input(self, log_n, inp):
        out = (C.c_uint8 * (32 << log_n))()
        self._chk(self.tlib.zkmi_shielder_witness_from_input(C.c_uint32(log_n), C.byref(inp), out))
        return bytes(out)

    def r1cs_create(self, n_vars, n_pub, mats):
        """mats = [(rowptr list, col list, val bytes)] * 3"""
        args = []
        keep = []
        nc = len(mats[0][0]) - 1
        for rowptr, col, val in mats:
            rp = (C.c_uint32 * len(rowptr))(*rowptr)
            cl = (C.c_uint32 * max(1, len(col)))(*col)
            vl = _buf(val)
            keep += [rp, cl, vl]
            args += [rp, cl, vl]
        h = C.c_void_p()
        self._chk(self.lib.zkmi_r1cs_create(C.c_uint32(n_vars), C.c_uint32(n_pub), C.c_uint32(nc), *args, C.byref(h)))
        return R1cs(self, h)

    def selftest_colsum_plan(self, r1cs, which):
        """Testing library: the host plan of one column query of groth16_setup_from_srs (which: 0 a, 1 b_g1, 2 b_g2, 4 l) ->
        dict(fan, terms [(point, base, neg, bits, k)], items [(level, out, first, count)], empty [slot])."""
        cnt = (C.c_uint64 * 5)()
        fn = self.tlib.zkmi_selftest_colsum_plan
        self._chk(fn(r1cs.h, C.c_int32(which), cnt, None, C.c_uint64(0), None, C.c_uint64(0), None, C.c_uint64(0)))
        nt, ni, ne = int(cnt[1]), int(cnt[2]), int(cnt[4])
        t, i, e = (C.c_uint32 * max(1, 12 * nt))(), (C.c_uint32 * max(1, 4 * ni))(), (C.c_uint32 * max(1, ne))()
        self._chk(fn(r1cs.h, C.c_int32(which), cnt, t, C.c_uint64(nt), i, C.c_uint64(ni), e, C.c_uint64(ne)))
        terms = [(t[12 * q], t[12 * q + 1], t[12 * q + 2], t[12 * q + 3], sum(t[12 * q + 4 + w] << (32 * w) for w in range(8)))
                 for q in range(nt)]
        items = [tuple(i[4 * q : 4 * q + 4]) for q in range(ni)]
        return {"fan": int(cnt[0]), "levels": int(cnt[3]), "terms": terms, "items": items, "empty": list(e[:ne])}

    def selftest_setup_columns_host(self, r1cs, toxic3, which, n_vars):
        """Testing library: one column query of the key from explicit tau|alpha|beta, the plan run by the host loop -> wire bytes."""
        assert len(toxic3) == 96
        w = 192 if which == 2 else 96
        out = (C.c_uint8 * (w * n_vars))()
        self._chk(self.tlib.zkmi_selftest_setup_columns_host(r1cs.h, _buf(toxic3), C.c_int32(which), out))
        return bytes(out)

    def selftest_rlc_weights_host(self, seed, dom, first, count):
        """Testing library: w(seed, dom, i) for i in [first, first + count) through the body k_rlc_weights runs, in a host
        loop -> count x 16 bytes (little-endian weights)."""
        assert len(seed) == 32
        out = (C.c_uint8 * (16 * max(1, count)))()
        self._chk(self.tlib.zkmi_selftest_rlc_weights_host(_buf(seed), C.c_uint32(dom), C.c_uint64(first), C.c_uint64(count), out))
        return bytes(out)[: 16 * count]

    def selftest_points_mul_each_host(self, group, wire_points, scalars):
        """Testing library: out[i] = k[i] * P[i] through the per-point body k_points_mul runs, in a host loop -> wire bytes."""
        w = 96 if group == 1 else 192
        n = len(scalars) // 32
        assert len(wire_points) == w * n and len(scalars) == 32 * n
        out = (C.c_uint8 * (w * max(1, n)))()
        self._chk(self.tlib.zkmi_selftest_points_mul_each_host(C.c_int32(group), _buf(wire_points), _buf(scalars), C.c_uint64(n), out))
        return bytes(out)[: w * n]

    def selftest_fr_powers_host(self, c, q, first, count):
        """Testing library: c * q^i for i in [first, first + count) through the body k_fr_powers runs, in a host loop cut at
        the chunk boundaries -> count x 32 bytes (canonical scalars)."""
        assert len(c) == 32 and len(q) == 32
        out = (C.c_uint8 * (32 * max(1, count)))()
        self._chk(self.tlib.zkmi_selftest_fr_powers_host(_buf(c), _buf(q), C.c_uint64(first), C.c_uint64(count), out))
        return bytes(out)[: 32 * count]

    def selftest_points_mul_shape(self):
        """Testing library: (indices a lane of k_fr_powers walks, window width of the multiplication body in bits)."""
        chunk, window = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.tlib.zkmi_selftest_points_mul_shape(C.byref(chunk), C.byref(window)))
        return int(chunk.value), int(window.value)

    MSM_SORT_SHAPE = ("FINE_LOG", "FINE_STAGE", "FINE_ROUND", "FSORT_RPT", "BIG_THR", "BIG_MAX", "BIG_NCH", "SPLIT_B", "PART_MAX",
                      "FPART_BLOCKS", "MSM_HEAVY", "MSM_HEAVY_CAP", "WRITE_BATCH")
    MSM_SORT_INFO = ("c", "nwin", "nb", "ndigits", "shared", "vec_parts", "heavy_thr", "heavy_shift", "top_spread_log", "buckets",
                     "words", "n_heavy", "fine_log", "big_listed", "big_total", "path")

    def selftest_msm_sort_shape(self):
        """Testing library: the constants the digit sort's kernel chains switch on (csrc/msm_sort.hip), as a dict."""
        out = (C.c_uint32 * len(self.MSM_SORT_SHAPE))()
        self._chk(self.tlib.zkmi_selftest_msm_sort_shape(out, C.c_uint32(len(self.MSM_SORT_SHAPE))))
        return dict(zip(self.MSM_SORT_SHAPE, (int(v) for v in out)))

    def points_mul_kernel(self, which):
        """Testing library: the multiplication kernel ITS calls launch from now on: 0 windowed, 1 plain, -1 as the environment said."""
        self._chk(self.tlib.zkmi_points_mul_kernel(C.c_int32(which)))

    def points_mul_phases(self, reset=False):
        """Testing library: ms of its multiplications since the last contribution began (powers, G1 kernels, G2 kernels, stores
        and allocation)."""
        out = (C.c_double * 4)()
        self._chk(self.tlib.zkmi_points_mul_phases(out, C.c_int32(int(reset))))
        return tuple(out)

    # ---- reference prove/verify surface (mocked_zk mirror) -------------------
    def account_new(self, tokens):
        arr = (Scalar * TOKENS_NUMBER)(*[scalar(t) for t in tokens])
        acc = Account()
        self._chk(self.lib.zkmi_account_new(arr, C.byref(acc)))
        return acc

    def account_hash(self, acc):
        out = Scalar()
        self._chk(self.lib.zkmi_account_hash(C.byref(acc), C.byref(out)))
        return bytes(out.bytes)

    def account_update(self, acc, op_pub, op_priv):
        out = Account()
        self._chk(self.lib.zkmi_account_update(C.byref(acc), C.byref(op_pub), C.byref(op_priv), C.byref(out)))
        return out

    def note_hash(self, id_, trapdoor, nullifier, acc_hash):
        out = Scalar()
        a = [scalar(x) for x in (id_, trapdoor, nullifier, acc_hash)]
        self._chk(self.lib.zkmi_note_hash(*[C.byref(x) for x in a], C.byref(out)))
        return bytes(out.bytes)

    def combine_merkle_hash(self, first, second):
        out = Scalar()
        a, b = scalar(first), scalar(second)
        self._chk(self.lib.zkmi_combine_merkle_hash(C.byref(a), C.byref(b), C.byref(out)))
        return bytes(out.bytes)

    def op_pub(self, kind, amount, token, user):
        o = OpPub()
        o.kind = {"deposit": 0, "withdraw": 1}[kind]
        C.memmove(o.amount, int(amount).to_bytes(16, "little"), 16)
        o.token = scalar(token)
        o.user = scalar(user)
        return o

    def op_priv(self, user):
        o = OpPriv()
        o.user = scalar(user)
        return o

    def operation_combine(self, op_pub, op_priv):
        self._chk(self.lib.zkmi_operation_combine(C.byref(op_pub), C.byref(op_priv)))

    def zkproof_new(self, id_, trapdoor, nullifier, op_priv, acc):
        out = ZkProof()
        a = [scalar(x) for x in (id_, trapdoor, nullifier)]
        self._chk(self.lib.zkmi_zkproof_new(*[C.byref(x) for x in a], C.byref(op_priv), C.byref(acc), C.byref(out)))
        return out

    def zkproof_update_account(self, proof, op_pub, op_priv, trapdoor, nullifier, merkle_proof, leaf_id):
        out = ZkProof()
        h = Scalar()
        mp = (Scalar * MERKLE_TREE_DEPTH)(*[scalar(x) for x in merkle_proof])
        t, n = scalar(trapdoor), scalar(nullifier)
        self._chk(
            self.lib.zkmi_zkproof_update_account(
                C.byref(proof), C.byref(op_pub), C.byref(op_priv), C.byref(t), C.byref(n), mp, C.c_uint32(leaf_id), C.byref(h), C.byref(out)
            )
        )
        return bytes(h.bytes), out

    def zkproof_verify_creation(self, proof, h_note_new, tokens):
        arr = (Scalar * TOKENS_NUMBER)(*[scalar(t) for t in tokens])
        h = scalar(h_note_new)
        self._chk(self.lib.zkmi_zkproof_verify_creation(C.byref(proof), C.byref(h), arr))

    def zkproof_verify_update(self, proof, op_pub, h_note_new, merkle_root, nullifier_old):
        a = [scalar(x) for x in (h_note_new, merkle_root, nullifier_old)]
        self._chk(self.lib.zkmi_zkproof_verify_update(C.byref(proof), C.byref(op_pub), *[C.byref(x) for x in a]))

    def context(self, device=0):
        return Context(self, device)


class R1cs:
    def __init__(self, z, handle):
        self.z, self.h = z, handle
        nv, npub, nc, lg = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        z._chk(z.lib.zkmi_r1cs_shape(handle, C.byref(nv), C.byref(npub), C.byref(nc), C.byref(lg)))
        self.n_vars, self.n_pub, self.n_constraints, self.log_n = nv.value, npub.value, nc.value, lg.value

    def export(self, m):
        nnz = C.c_uint64()
        self.z._chk(self.z.lib.zkmi_r1cs_export(self.h, C.c_int32(m), None, None, None, C.byref(nnz)))
        rp = (C.c_uint32 * (self.n_constraints + 1))()
        cl = (C.c_uint32 * max(1, nnz.value))()
        vl = (C.c_uint8 * max(1, 32 * nnz.value))()
        self.z._chk(self.z.lib.zkmi_r1cs_export(self.h, C.c_int32(m), rp, cl, vl, None))
        return list(rp), list(cl)[: nnz.value], bytes(vl)[: 32 * nnz.value]

    def is_satisfied(self, zbytes):
        rc = self.z.lib.zkmi_r1cs_is_satisfied(self.h, _buf(zbytes))
        if rc == 0:
            return True
        if rc == -8:
            return False
        raise ZkmiError(rc)

    def free(self):
        if self.h:
            self.z.lib.zkmi_r1cs_free(self.h)
            self.h = None


class Comm:
    """zkmi_comm: an RCCL communicator behind the C ABI (include/zkmi.h)."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def free(self):
        if self.h:
            self.ctx.lib.zkmi_comm_destroy(self.h)
            self.h = None


class PreparedVk:
    """zkmi_vk: a validated verifying key (host memory only)."""

    def __init__(self, z, h, n_pub):
        self.z, self.h, self.n_pub = z, h, n_pub

    def free(self):
        if self.h:
            self.z.lib.zkmi_vk_free(self.h)
            self.h = None


class Context:
    """One HIP device + stream + resident workspaces (zkmi_ctx)."""

    def __init__(self, z, device=0):
        self.z = z
        self.lib = z.lib
        self.h = C.c_void_p()
        z._chk(self.lib.zkmi_ctx_create(C.c_int32(device), C.byref(self.h)))

    def _chk(self, rc):
        self.z._chk(rc, self.h)

    def close(self):
        if self.h:
            self.lib.zkmi_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        self._chk(self.lib.zkmi_ctx_sync(self.h))

    def prof_enable(self, on=True):
        self._chk(self.lib.zkmi_prof_enable(self.h, C.c_int32(1 if on else 0)))

    def prof_reset(self):
        self._chk(self.lib.zkmi_prof_reset(self.h))

    def prof_get(self, phase):
        ms, cnt = C.c_double(), C.c_uint64()
        self._chk(self.lib.zkmi_prof_get(self.h, C.c_int32(PHASES[phase]), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    # NTT
    def ntt(self, data, log_n, inverse=False, coset=False):
        assert len(data) == 32 << log_n
        buf = _buf(data)
        self._chk(self.lib.zkmi_ntt_fr(self.h, buf, C.c_uint32(log_n), C.c_int32(inverse), C.c_int32(coset)))
        return bytes(buf)

    def ntt_dev(self, dptr, log_n, inverse=False, coset=False):
        self._chk(self.lib.zkmi_ntt_fr_dev(self.h, C.c_void_p(dptr), C.c_uint32(log_n), C.c_int32(inverse), C.c_int32(coset)))

    # bases
    def bases_g1(self, affine, check=True):
        h = C.c_void_p()
        self._chk(self.lib.zkmi_bases_g1_load(self.h, _buf(affine), C.c_uint64(len(affine) // 96), C.c_int32(check), C.byref(h)))
        return Bases(self, h, 1, len(affine) // 96)

    def bases_g2(self, affine, check=True):
        h = C.c_void_p()
        self._chk(self.lib.zkmi_bases_g2_load(self.h, _buf(affine), C.c_uint64(len(affine) // 192), C.c_int32(check), C.byref(h)))
        return Bases(self, h, 2, len(affine) // 192)

    def _bases_encoded(self, group, points, encoding, checks):
        w = (96 if group == 1 else 192) // (2 if encoding == ENC_ZCASH_COMPRESSED else 1)
        h, bad = C.c_void_p(), C.c_uint64(NO_INDEX)
        fn = self.lib.zkmi_bases_g1_load_encoded if group == 1 else self.lib.zkmi_bases_g2_load_encoded
        rc = fn(self.h, _buf(points), C.c_uint64(len(points) // w), C.c_int32(encoding), C.c_int32(checks), C.byref(h), C.byref(bad))
        if rc != 0:
            err = ZkmiError(rc, (self.lib.zkmi_last_error(self.h) or b"").decode())
            err.first_bad = None if bad.value == NO_INDEX else bad.value
            raise err
        return Bases(self, h, group, len(points) // w)

    def bases_g1_encoded(self, points, encoding, checks=CHECK_SUBGROUP):
        """Resident G1 bases from host bytes in any ENC_* form, parsed / decompressed / checked on the device.  A refused
        load raises ZkmiError (NON_CANONICAL) whose `first_bad` is the smallest failing index."""
        return self._bases_encoded(1, points, encoding, checks)

    def bases_g2_encoded(self, points, encoding, checks=CHECK_SUBGROUP):
        return self._bases_encoded(2, points, encoding, checks)

    def _points_read_dev(self, group, d_in, n, encoding, checks, d_out_wire, d_status):
        bad = C.c_uint64(NO_INDEX)
        fn = self.lib.zkmi_g1_points_read_dev if group == 1 else self.lib.zkmi_g2_points_read_dev
        rc = fn(self.h, C.c_void_p(d_in), C.c_uint64(n), C.c_int32(encoding), C.c_int32(checks),
                C.c_void_p(d_out_wire) if d_out_wire else None, C.c_void_p(d_status) if d_status else None, C.byref(bad))
        if rc not in (0, -2):
            self._chk(rc)
        assert (rc == 0) == (bad.value == NO_INDEX)
        return None if rc == 0 else bad.value

    def g1_points_read_dev(self, d_in, n, encoding, checks, d_out_wire=None, d_status=None):
        """n G1 points at device address d_in in `encoding` -> affine wire form at d_out_wire (optional), one status byte
        each at d_status (optional).  Returns None when every element passes, else the smallest failing index."""
        return self._points_read_dev(1, d_in, n, encoding, checks, d_out_wire, d_status)

    def g2_points_read_dev(self, d_in, n, encoding, checks, d_out_wire=None, d_status=None):
        return self._points_read_dev(2, d_in, n, encoding, checks, d_out_wire, d_status)

    def pairing_product_dev(self, d_g1, d_g2, n):
        """prod_i e(P_i, Q_i) of n pairs in HBM (affine wire form, subgroup points): the 576 bytes Zkmi.pairing returns."""
        out = (C.c_uint8 * 576)()
        self._chk(self.lib.zkmi_pairing_product_dev(self.h, C.c_void_p(d_g1) if d_g1 else None, C.c_void_p(d_g2) if d_g2 else None,
                                                    C.c_uint64(n), out))
        return bytes(out)

    def groth16_verify_batch(self, vk, publics, proofs, weights=None, want_status=True):
        """zkmi_groth16_verify_batch over host bytes: vk from Zkmi.vk_prepare, proofs n x 192 B, publics n x (n_pub - 1) x 32 B,
        weights n x 16 B or None (drawn from the OS).  Returns (ok, status bytes or None, first_bad or None); a rejected
        batch is a result, not an exception.  Anything else (bad argument, HIP error) raises ZkmiError."""
        n = len(proofs) // 192
        assert len(proofs) == 192 * n and len(publics) == 32 * (vk.n_pub - 1) * n
        assert weights is None or len(weights) == 16 * n
        st = (C.c_uint8 * max(1, n))() if want_status else None
        bad = C.c_uint64(NO_INDEX)
        rc = self.lib.zkmi_groth16_verify_batch(self.h, vk.h, C.c_uint64(n), _buf(publics), _buf(proofs),
                                                _buf(weights) if weights is not None else None, st, C.byref(bad))
        if rc not in (0, -2, -5):
            self._chk(rc)
        return rc == 0, (bytes(st)[:n] if want_status else None), (None if bad.value == NO_INDEX else bad.value)

    def pairing_batch_dev(self, d_g1, d_g2, n, d_out):
        """zkmi_pairing_batch_dev: n reduced pairings e(P_i, Q_i) of pairs in HBM (affine wire form, subgroup points), Miller
        loop and final exponentiation on the device; d_out receives n x 576 B, each the bytes Zkmi.pairing returns."""
        self._chk(self.lib.zkmi_pairing_batch_dev(self.h, C.c_void_p(d_g1) if d_g1 else None, C.c_void_p(d_g2) if d_g2 else None,
                                                  C.c_uint64(n), C.c_void_p(d_out) if d_out else None))

    def groth16_verify_each(self, vk, publics, proofs):
        """zkmi_groth16_verify_each over host bytes: every proof checked by its own equation on the device, the same work
        whatever the verdicts (the call for proofs from outside; groth16_verify_batch is the one for trusted input).  vk from
        Zkmi.vk_prepare, proofs n x 192 B, publics n x (n_pub - 1) x 32 B.  Returns (ok, status bytes, first_bad or None); a
        rejected batch is a result, not an exception.  Lengths that do not fit the key raise ZkmiError (BAD_ARG) before the
        library is called; anything else (HIP error) raises ZkmiError too."""
        n = len(proofs) // 192
        if len(proofs) != 192 * n or len(publics) != 32 * (vk.n_pub - 1) * n:
            raise ZkmiError(-1, "groth16_verify_each: %d bytes of proofs and %d of publics do not fit a key with n_pub = %d"
                            % (len(proofs), len(publics), vk.n_pub))
        st = (C.c_uint8 * max(1, n))()
        bad = C.c_uint64(NO_INDEX)
        rc = self.lib.zkmi_groth16_verify_each(self.h, vk.h, C.c_uint64(n), _buf(publics), _buf(proofs), st, C.byref(bad))
        if rc not in (0, -2, -5):
            self._chk(rc)
        return rc == 0, bytes(st)[:n], (None if bad.value == NO_INDEX else bad.value)

    def bases_g1_synthetic_range(self, first, n):
        h = C.c_void_p()
        self._chk(self.z.tlib.zkmi_bases_g1_synthetic_range(self.h, C.c_uint64(first), C.c_uint64(n), C.byref(h)))
        return Bases(self, h, 1, n)

    def bases_g1_synthetic(self, n):
        h = C.c_void_p()
        self._chk(self.z.tlib.zkmi_bases_g1_synthetic(self.h, C.c_uint64(n), C.byref(h)))
        return Bases(self, h, 1, n)

    def bases_g2_synthetic(self, n):
        h = C.c_void_p()
        self._chk(self.z.tlib.zkmi_bases_g2_synthetic(self.h, C.c_uint64(n), C.byref(h)))
        return Bases(self, h, 2, n)

    # MSM
    def msm_g1(self, scalars, bases):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1(self.h, _buf(scalars), C.c_uint64(len(scalars) // 32), bases.h, out))
        return bytes(out)

    def msm_g2(self, scalars, bases):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_msm_g2(self.h, _buf(scalars), C.c_uint64(len(scalars) // 32), bases.h, out))
        return bytes(out)

    def msm_g1_dev(self, dptr, n, bases):
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1_dev(self.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, out))
        return bytes(out)

    def msm_g2_dev(self, dptr, n, bases):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_msm_g2_dev(self.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, out))
        return bytes(out)

    def update_note_witness_batch_dev(self, log_n, op_kind, inputs, d_ptrs):
        """Assignments of len(inputs) instances generated on the GPU into the device buffers d_ptrs
        (each 2^log_n x 32 B); returns the per-instance status codes."""
        n = len(inputs)
        assert n == len(d_ptrs)
        arr = (NoteUpdate * max(1, n))(*inputs)
        ptrs = (C.c_void_p * max(1, n))(*[int(p) for p in d_ptrs])
        st = (C.c_int32 * max(1, n))()
        self._chk(self.lib.zkmi_update_note_witness_batch_dev(self.h, C.c_uint32(log_n), C.c_int32(op_kind), arr, C.c_uint32(n), ptrs, st))
        return list(st)[:n]

    # ---- the resident Poseidon note tree (include/zkmi.h "note tree") ---------
    def note_tree(self, height, capacity, field=0):
        h = C.c_void_p()
        self._chk(self.lib.zkmi_note_tree_create(self.h, C.c_int32(field), C.c_uint32(height), C.c_uint64(capacity), C.byref(h)))
        return NoteTree(self, h, field)

    def append(self, tree, leaves, want_roots=False):
        """m = len(leaves) / 32 leaves (bytes) behind the tree's last one -> (new root, m x 32 B per-leaf roots or None)."""
        assert len(leaves) % 32 == 0
        m = len(leaves) // 32
        root = (C.c_uint8 * 32)()
        roots = (C.c_uint8 * (32 * max(1, m)))() if want_roots else None
        self._chk(self.lib.zkmi_note_tree_append(self.h, tree.h, _buf(leaves), C.c_uint64(m), root, roots))
        return bytes(root), (bytes(roots)[: 32 * m] if want_roots else None)

    def append_dev(self, tree, d_leaves, m, d_roots=None):
        """m leaves from the device buffer d_leaves; d_roots (optional device buffer, m x 32 B) receives the per-leaf roots."""
        root = (C.c_uint8 * 32)()
        self._chk(self.lib.zkmi_note_tree_append_dev(self.h, tree.h, C.c_void_p(d_leaves), C.c_uint64(m), root,
                                                     C.c_void_p(d_roots) if d_roots else None))
        return bytes(root)

    def root(self, tree):
        out = (C.c_uint8 * 32)()
        self._chk(self.lib.zkmi_note_tree_root(self.h, tree.h, out))
        return bytes(out)

    def shape(self, tree):
        """(height, capacity, n_leaves)"""
        out = (C.c_uint64 * 3)()
        self._chk(self.lib.zkmi_note_tree_shape(tree.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def paths(self, tree, leaf_idx):
        """(shape bytes k x height, path bytes k x height x 32) of the given leaves against the current root."""
        k, height = len(leaf_idx), self.shape(tree)[0]
        idx = (C.c_uint64 * max(1, k))(*leaf_idx)
        shape = (C.c_uint8 * max(1, k * height))()
        paths = (C.c_uint8 * max(1, 32 * k * height))()
        self._chk(self.lib.zkmi_note_tree_paths(self.h, tree.h, idx, C.c_uint32(k), shape, paths))
        return bytes(shape)[: k * height], bytes(paths)[: 32 * k * height]

    def paths_dev(self, tree, leaf_idx, d_shape, d_paths):
        """The same into device buffers (k x height bytes, k x height x 32 B)."""
        k = len(leaf_idx)
        idx = (C.c_uint64 * max(1, k))(*leaf_idx)
        self._chk(self.lib.zkmi_note_tree_paths_dev(self.h, tree.h, idx, C.c_uint32(k), C.c_void_p(d_shape), C.c_void_p(d_paths)))

    def update_note_witness_batch_tree_dev(self, log_n, op_kind, inputs, tree, leaf_idx, d_ptrs):
        """update_note_witness_batch_dev with the Merkle inputs of inputs[i] taken on the device from the path of
        leaf_idx[i] in `tree`; returns the per-instance status codes."""
        n = len(inputs)
        assert n == len(d_ptrs) == len(leaf_idx)
        arr = (NoteUpdate * max(1, n))(*inputs)
        idx = (C.c_uint64 * max(1, n))(*leaf_idx)
        ptrs = (C.c_void_p * max(1, n))(*[int(p) for p in d_ptrs])
        st = (C.c_int32 * max(1, n))()
        self._chk(self.lib.zkmi_update_note_witness_batch_tree_dev(self.h, C.c_uint32(log_n), C.c_int32(op_kind), arr, tree.h, idx,
                                                                   C.c_uint32(n), ptrs, st))
        return list(st)[:n]

    # ---- BN254 MSM / NTT / KZG commit -----------------------
    def bn254_bases(self, affine, check=True):
        h = C.c_void_p()
        self._chk(self.lib.zkmi_bn254_bases_load(self.h, _buf(affine), C.c_uint64(len(affine) // 64), C.c_int32(check), C.byref(h)))
        return BnBases(self, h, len(affine) // 64)

    def bn254_bases_synthetic(self, n):
        h = C.c_void_p()
        self._chk(self.z.tlib.zkmi_bn254_bases_synthetic(self.h, C.c_uint64(n), C.byref(h)))
        return BnBases(self, h, n)

    def bn254_msm_g1(self, scalars, bases):
        out = (C.c_uint8 * 64)()
        self._chk(self.lib.zkmi_bn254_msm_g1(self.h, _buf(scalars), C.c_uint64(len(scalars) // 32), bases.h, out))
        return bytes(out)

    def bn254_msm_g1_dev(self, dptr, n, bases):
        out = (C.c_uint8 * 64)()
        self._chk(self.lib.zkmi_bn254_msm_g1_dev(self.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, out))
        return bytes(out)

    def bn254_ntt(self, data, log_n, inverse=False, coset=False):
        buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
        self._chk(self.lib.zkmi_bn254_ntt_fr(self.h, buf, C.c_uint32(log_n), C.c_int32(inverse), C.c_int32(coset)))
        return bytes(buf)

    def bn254_ntt_dev(self, dptr, log_n, inverse=False, coset=False):
        self._chk(self.lib.zkmi_bn254_ntt_fr_dev(self.h, C.c_void_p(dptr), C.c_uint32(log_n), C.c_int32(inverse), C.c_int32(coset)))

    def bn254_kzg_commit_dev(self, d_evals, log_n, srs):
        out = (C.c_uint8 * 64)()
        self._chk(self.lib.zkmi_bn254_kzg_commit_dev(self.h, C.c_void_p(d_evals), C.c_uint32(log_n), srs.h, out))
        return bytes(out)

    def bn254_kzg_open_dev(self, d_coeffs, n, zeta, srs, d_quotient=None):
        """(p(zeta) as 32 bytes, commit(q) as 64 bytes); d_quotient: device pointer that receives the n - 1 quotient coefficients."""
        ev, pf = (C.c_uint8 * 32)(), (C.c_uint8 * 64)()
        self._chk(self.lib.zkmi_bn254_kzg_open_dev(self.h, C.c_void_p(d_coeffs), C.c_uint64(n), _buf(zeta), srs.h,
                                                   C.c_void_p(d_quotient) if d_quotient else None, ev, pf))
        return bytes(ev), bytes(pf)

    def bn254_kzg_open_many_dev(self, d_polys, n, zeta, v, srs):
        """([p_j(zeta) as 32 bytes], commit(q of sum_j v^j p_j) as 64 bytes) for a list of device pointers."""
        k = len(d_polys)
        tab = (C.c_void_p * max(k, 1))(*d_polys)
        ev, pf = (C.c_uint8 * (32 * max(k, 1)))(), (C.c_uint8 * 64)()
        self._chk(self.lib.zkmi_bn254_kzg_open_many_dev(self.h, tab, C.c_uint32(k), C.c_uint64(n), _buf(zeta), _buf(v), srs.h, ev, pf))
        raw = bytes(ev)
        return [raw[32 * j: 32 * j + 32] for j in range(k)], bytes(pf)

    def bn254_grand_product_dev(self, d_num, d_den, n, d_out):
        """d_out[i] = prod_{j < i} num_j / den_j; returns the product over all n terms (32 bytes)."""
        tot = (C.c_uint8 * 32)()
        self._chk(self.lib.zkmi_bn254_grand_product_dev(self.h, C.c_void_p(d_num), C.c_void_p(d_den), C.c_uint64(n), C.c_void_p(d_out), tot))
        return bytes(tot)

    def sha256_pairs(self, inputs, n_hashes):
        assert len(inputs) == 64 * n_hashes
        out = (C.c_uint8 * (32 * max(1, n_hashes)))()
        self._chk(self.lib.zkmi_sha256_pairs(self.h, _buf(inputs), C.c_uint64(n_hashes), out))
        return bytes(out)[: 32 * n_hashes]

    def sha256_pairs_dev(self, d_in, n_hashes, d_out):
        self._chk(self.lib.zkmi_sha256_pairs_dev(self.h, C.c_void_p(d_in), C.c_uint64(n_hashes), C.c_void_p(d_out)))

    def sha256_merkle_tree_dev(self, d_nodes, log_leaves, n_filled):
        self._chk(self.lib.zkmi_sha256_merkle_tree_dev(self.h, C.c_void_p(d_nodes), C.c_uint32(log_leaves), C.c_uint64(n_filled)))

    def poseidon_hash_batch(self, inputs, n_hashes, arity, field=0):
        """n_hashes x arity canonical 32-byte inputs (bytes) -> n_hashes x 32 bytes, hashed on the GPU."""
        assert len(inputs) == 32 * n_hashes * arity
        out = (C.c_uint8 * (32 * max(1, n_hashes)))()
        self._chk(self.lib.zkmi_poseidon_hash_batch(self.h, C.c_int32(field), _buf(inputs), C.c_uint64(n_hashes), C.c_uint32(arity), out))
        return bytes(out)[: 32 * n_hashes]

    def poseidon_hash_batch_dev(self, d_in, n_hashes, arity, d_out, field=0):
        self._chk(self.lib.zkmi_poseidon_hash_batch_dev(self.h, C.c_int32(field), C.c_void_p(d_in), C.c_uint64(n_hashes), C.c_uint32(arity), C.c_void_p(d_out)))

    def poseidon_merkle_tree_dev(self, d_nodes, log_leaves, field=0):
        self._chk(self.lib.zkmi_poseidon_merkle_tree_dev(self.h, C.c_int32(field), C.c_void_p(d_nodes), C.c_uint32(log_leaves)))

    def poseidon_merkle_paths_dev(self, d_nodes, log_leaves, leaf_idx):
        """(shape bytes n x log_leaves, path bytes n x log_leaves x 32) for the given leaf indices."""
        n = len(leaf_idx)
        idx = (C.c_uint32 * max(1, n))(*leaf_idx)
        shape = (C.c_uint8 * max(1, n * log_leaves))()
        paths = (C.c_uint8 * max(1, 32 * n * log_leaves))()
        self._chk(self.lib.zkmi_poseidon_merkle_paths_dev(self.h, C.c_void_p(d_nodes), C.c_uint32(log_leaves), idx, C.c_uint32(n), shape, paths))
        return bytes(shape)[: n * log_leaves], bytes(paths)[: 32 * n * log_leaves]

    def poseidon_merkle_roots_dev(self, d_leaves, d_shape, d_paths, depth, n, d_roots, field=0):
        self._chk(self.lib.zkmi_poseidon_merkle_roots_dev(self.h, C.c_int32(field), C.c_void_p(d_leaves), C.c_void_p(d_shape), C.c_void_p(d_paths), C.c_uint32(depth), C.c_uint64(n), C.c_void_p(d_roots)))

    def comm_init(self, n_ranks, rank, unique_id):
        """RCCL communicator of this context's device (collective: every rank calls it with rank 0's id)."""
        h = C.c_void_p()
        self._chk(self.lib.zkmi_comm_init(self.h, C.c_uint32(n_ranks), C.c_uint32(rank), _buf(unique_id), C.byref(h)))
        return Comm(self, h)

    def msm_g1_allgather_combine(self, comm, dptr, n, bases, plan_n):
        """This rank's slice of a point-split MSM + the RCCL exchange + combination (collective); the full result."""
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1_allgather_combine(self.h, comm.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, C.c_uint64(plan_n), out))
        return bytes(out)

    def selftest_msm_g1_sum2_dev(self, dptr_a, dptr_b, n, bases):
        """MSM(a) + MSM(b) over the same bases through ONE shared bucket set (test hook of the L + H merge)."""
        out = (C.c_uint8 * 96)()
        self._chk(self.z.tlib.zkmi_selftest_msm_g1_sum2_dev(self.h, C.c_void_p(dptr_a), C.c_void_p(dptr_b), C.c_uint64(n), bases.h, out))
        return bytes(out)

    def selftest_msm_sort_dev(self, dptr, n, mode=0, plan_n=0, batch=0, arrays=True):
        """Testing library: one run of this context's digit sort over n canonical scalars in HBM, read out (mode 0 windowed --
        plan_n: under the window width of that many terms --, 1 shared, 2 shared batch of `batch` vectors).  Returns
        (info dict, count, begin, perm, heavy, sorted) as ctypes uint32 arrays (numpy reads them with np.frombuffer); heavy is
        [n_heavy, ids ...].  arrays=False: the info dict alone.  An error code raises ZkmiError."""
        fn = self.z.tlib.zkmi_selftest_msm_sort_dev
        keys = self.z.MSM_SORT_INFO
        info = (C.c_uint32 * len(keys))()
        head = (self.h, C.c_int32(mode), C.c_void_p(dptr), C.c_uint64(n), C.c_uint64(plan_n), C.c_uint32(batch), info, C.c_uint32(len(keys)))
        self._chk(fn(*head, None, None, None, None, C.c_uint64(0), None, C.c_uint64(0)))
        d = dict(zip(keys, (int(v) for v in info)))
        if not arrays:
            return d
        nb, nw = d["buckets"], d["words"]
        count, begin, perm = (C.c_uint32 * nb)(), (C.c_uint32 * nb)(), (C.c_uint32 * nb)()
        heavy, srt = (C.c_uint32 * (nb + 1))(), (C.c_uint32 * max(1, nw))()
        self._chk(fn(*head, count, begin, perm, heavy, C.c_uint64(nb), srt, C.c_uint64(nw)))
        # (the sort ran twice: the order inside a bucket aside, the same result)
        assert dict(zip(keys, (int(v) for v in info))) == d, (d, list(info))
        return d, count, begin, perm, heavy, srt

    def msm_g1_window_range_dev(self, dptr, n, bases, plan_n, w_first, w_count):
        """(w_count x 96 B window sums over ALL n points, total windows of the plan, window bits): a rank of a WINDOW split"""
        out = (C.c_uint8 * (96 * max(1, w_count)))()
        tot, cbits = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.zkmi_msm_g1_window_range_dev(self.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, C.c_uint64(plan_n),
                                                        C.c_uint32(w_first), C.c_uint32(w_count), out, C.byref(tot), C.byref(cbits)))
        return bytes(out)[: 96 * w_count], tot.value, cbits.value

    def msm_g1_window_split_allgather(self, comm, dptr, n, bases):
        """BASELINE configs[3] as worded: windows split over the ranks of `comm`, RCCL all-gather, the full result (collective)"""
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1_window_split_allgather(self.h, comm.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, out))
        return bytes(out)

    def msm_g1_split2d_allgather(self, comm, dptr, n, bases, plan_n, window_groups):
        """The 2-D split: rank k = g * window_groups + q holds point group g's slice (dptr / n / bases) and computes window
        range q of the plan of plan_n terms; RCCL all-gather, the full result on every rank (collective)"""
        out = (C.c_uint8 * 96)()
        self._chk(self.lib.zkmi_msm_g1_split2d_allgather(self.h, comm.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, C.c_uint64(plan_n),
                                                         C.c_uint32(window_groups), out))
        return bytes(out)

    def msm_g1_windows_dev(self, dptr, n, bases, plan_n):
        out = (C.c_uint8 * (96 * 64))()
        nwin, cbits = C.c_uint32(), C.c_uint32()
        self._chk(
            self.lib.zkmi_msm_g1_windows_dev(self.h, C.c_void_p(dptr), C.c_uint64(n), bases.h, C.c_uint64(plan_n), out, C.byref(nwin), C.byref(cbits))
        )
        return bytes(out)[: 96 * nwin.value], nwin.value, cbits.value

    # Groth16
    def set_group_size(self, group):
        """proofs per group for keys created next on this context (0 = automatic, 1 = never group)"""
        self._chk(self.lib.zkmi_ctx_set_group_size(self.h, C.c_uint32(group)))

    def groth16_setup(self, r1cs, toxic):
        assert len(toxic) == 160
        cap = 672 + 96 * r1cs.n_pub
        vk = (C.c_uint8 * cap)()
        h = C.c_void_p()
        self._chk(self.lib.zkmi_groth16_setup(self.h, r1cs.h, _buf(toxic), C.byref(h), vk, C.c_uint64(cap)))
        return ProvingKey(self, h, r1cs), bytes(vk)

    def g1_points_ntt_dev(self, d_points, log_n, inverse=False):
        """zkmi_g1_points_ntt_dev: 2^log_n G1 points at device address d_points (affine wire form, subgroup points)
        transformed in place, natural order in and out; the inverse is scaled by N^-1."""
        self._chk(self.lib.zkmi_g1_points_ntt_dev(self.h, C.c_void_p(d_points) if d_points else None, C.c_uint32(log_n), C.c_int32(int(inverse))))

    def g2_points_ntt_dev(self, d_points, log_n, inverse=False):
        self._chk(self.lib.zkmi_g2_points_ntt_dev(self.h, C.c_void_p(d_points) if d_points else None, C.c_uint32(log_n), C.c_int32(int(inverse))))

    def srs_load(self, encoding, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, checks=CHECK_SUBGROUP):
        """Phase-1 transcript from host bytes in any ENC_* form, every point parsed and checked on the device under `checks`.
        A refused transcript raises ZkmiError (NON_CANONICAL) whose `where` is (section, index) of the refused point
        (sections: 0 tau_g1, 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1, 4 beta_g2), or None."""
        w1 = 96 // (2 if encoding == ENC_ZCASH_COMPRESSED else 1)
        assert len(alpha_tau_g1) == len(beta_tau_g1) and len(beta_g2) == 2 * w1
        h = C.c_void_p()
        where = (C.c_uint64 * 2)(NO_INDEX, NO_INDEX)
        rc = self.lib.zkmi_srs_load(self.h, C.c_int32(encoding), C.c_int32(checks), _buf(tau_g1), C.c_uint64(len(tau_g1) // w1),
                                    _buf(tau_g2), C.c_uint64(len(tau_g2) // (2 * w1)), _buf(alpha_tau_g1), _buf(beta_tau_g1),
                                    C.c_uint64(len(alpha_tau_g1) // w1), _buf(beta_g2), C.byref(h), where)
        if rc != 0:
            err = ZkmiError(rc, (self.lib.zkmi_last_error(self.h) or b"").decode())
            err.where = None if where[0] == NO_INDEX else (int(where[0]), int(where[1]))
            assert not h.value
            raise err
        return Srs(self, h)

    def srs_generate(self, toxic, log_n):
        """The transcript of explicit toxic waste tau|alpha|beta (96 bytes) for a domain of 2^log_n: tests and benches only."""
        assert len(toxic) == 96
        h = C.c_void_p()
        self._chk(self.lib.zkmi_srs_generate(self.h, _buf(toxic), C.c_uint32(log_n), C.byref(h)))
        return Srs(self, h)

    def _verdict(self, rc, failed):
        """(ok, failed_mask) of a verification call: a failed check is an answer, every other refusal raises."""
        if rc == -5:
            return False, int(failed.value)
        self._chk(rc)
        return True, int(failed.value)

    def srs_verify(self, srs, seed=None):
        """zkmi_srs_verify: the same-ratio checks of a resident transcript under the weights of `seed` (32 bytes; None: drawn
        by the library) -> (ok, failed_mask of SRS_*).  Raises ZkmiError (BAD_ARG) for a transcript of another context or one
        that was not loaded under CHECK_SUBGROUP."""
        assert seed is None or len(seed) == 32
        failed = C.c_uint32(0)
        rc = self.lib.zkmi_srs_verify(self.h, srs.h, _buf(seed) if seed is not None else None, C.byref(failed))
        return self._verdict(rc, failed)

    def pk_verify_contribution(self, before, after, seed=None):
        """zkmi_pk_verify_contribution: `after` is `before` with one phase-2 contribution applied -> (ok, failed_mask of PK2_*).
        Raises ZkmiError (BAD_ARG) for keys of different shape or of another context."""
        assert seed is None or len(seed) == 32
        failed = C.c_uint32(0)
        rc = self.lib.zkmi_pk_verify_contribution(self.h, before.h, after.h, _buf(seed) if seed is not None else None, C.byref(failed))
        return self._verdict(rc, failed)

    def points_adjacent_sums_dev(self, group, d_points, m, seed, dom):
        """zkmi_g{1,2}_points_adjacent_sums_dev: m subgroup points at device address d_points (affine wire form) ->
        (lo, hi) = (sum w_i P[i], sum w_i P[i + 1]) over i < m - 1, wire bytes."""
        w = 96 if group == 1 else 192
        lo, hi = (C.c_uint8 * w)(), (C.c_uint8 * w)()
        fn = self.lib.zkmi_g1_points_adjacent_sums_dev if group == 1 else self.lib.zkmi_g2_points_adjacent_sums_dev
        self._chk(fn(self.h, C.c_void_p(d_points) if d_points else None, C.c_uint64(m), _buf(seed) if seed is not None else None,
                     C.c_uint32(dom), lo, hi))
        return bytes(lo), bytes(hi)

    def points_mul_each_dev(self, group, d_points, d_scalars, n, d_out):
        """zkmi_g{1,2}_points_mul_each_dev: out[i] = k[i] * P[i] for n subgroup points (affine wire form) and n canonical
        32-byte scalars at device addresses; d_out may equal d_points."""
        fn = self.lib.zkmi_g1_points_mul_each_dev if group == 1 else self.lib.zkmi_g2_points_mul_each_dev
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        self._chk(fn(self.h, ptr(d_points), ptr(d_scalars), C.c_uint64(n), ptr(d_out)))

    def points_mul_powers_dev(self, group, d_points, n, c, q):
        """zkmi_g{1,2}_points_mul_powers_dev: P[i] <- (c q^i) P[i] in place, the scalars made on the device (c, q: 32 bytes
        canonical)."""
        fn = self.lib.zkmi_g1_points_mul_powers_dev if group == 1 else self.lib.zkmi_g2_points_mul_powers_dev
        self._chk(fn(self.h, C.c_void_p(d_points) if d_points else None, C.c_uint64(n), _buf(c) if c is not None else None,
                     _buf(q) if q is not None else None))

    def srs_contribute(self, srs, sab):
        """zkmi_srs_contribute: one phase-1 contribution s | a | b (96 bytes canonical, each non-zero) in place ->
        step_g2 = [s]G2 | [a]G2 | [b]G2 (576 bytes), what srs_verify_contribution takes."""
        step = (C.c_uint8 * 576)()
        self._chk(self.lib.zkmi_srs_contribute(self.h, srs.h, _buf(sab) if sab is not None else None, step))
        return bytes(step)

    def srs_verify_contribution(self, before, after, step_g2, seed=None):
        """zkmi_srs_verify_contribution: `after` is `before` moved by the contribution whose step elements are step_g2 ->
        (ok, failed_mask: the SRS_* mask of `after` plus SRS_STEP_*).  It does not prove that anybody knows s, a, b."""
        assert seed is None or len(seed) == 32
        failed = C.c_uint32(0)
        rc = self.lib.zkmi_srs_verify_contribution(self.h, before.h, after.h, _buf(step_g2) if step_g2 is not None else None,
                                                   _buf(seed) if seed is not None else None, C.byref(failed))
        return self._verdict(rc, failed)

    def ceremony_phases(self):
        """Testing library: ms of the last srs_verify / pk_verify_contribution made through it (weights, conversion, MSMs,
        pairing products)."""
        out = (C.c_double * 4)()
        self._chk(self.z.tlib.zkmi_ceremony_phases(out))
        return tuple(out)

    def groth16_setup_from_srs(self, r1cs, srs, vk_cap=None):
        """zkmi_groth16_setup_from_srs: the relation's key from a phase-1 transcript, gamma = delta = 1 -> (ProvingKey, vk)."""
        cap = 672 + 96 * r1cs.n_pub if vk_cap is None else vk_cap
        vk = (C.c_uint8 * max(1, cap))()
        h = C.c_void_p()
        rc = self.lib.zkmi_groth16_setup_from_srs(self.h, r1cs.h, srs.h, C.byref(h), vk, C.c_uint64(cap))
        if rc != 0:
            assert not h.value
        self._chk(rc)
        return ProvingKey(self, h, r1cs), bytes(vk)

    def setup_from_srs_phases(self):
        """Testing library: ms of the last groth16_setup_from_srs made through it (transforms, column sums, h query)."""
        out = (C.c_double * 3)()
        self._chk(self.z.tlib.zkmi_setup_from_srs_phases(out))
        return tuple(out)

    def pk_load(self, r1cs, alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, a_q, b1_q, b2_q, h_q, l_q):
        h = C.c_void_p()
        self._chk(
            self.lib.zkmi_pk_load(
                self.h, r1cs.h, _buf(alpha_g1), _buf(beta_g1), _buf(beta_g2), _buf(delta_g1), _buf(delta_g2),
                _buf(a_q), _buf(b1_q), _buf(b2_q), _buf(h_q), _buf(l_q), C.byref(h),
            )
        )
        return ProvingKey(self, h, r1cs)

    def shielder_prove_creation(self, pk_create, knowledge, tokens, r, s):
        """(h_note_new bytes, proof bytes) from the ZkProof `knowledge` built by zkproof_new."""
        arr = (Scalar * TOKENS_NUMBER)(*[scalar(t) for t in tokens])
        h = Scalar()
        out = (C.c_uint8 * 192)()
        self._chk(self.z.lib.zkmi_shielder_prove_creation(self.h, pk_create.h, C.byref(knowledge), arr, _buf(r), _buf(s), C.byref(h), out))
        return bytes(h.bytes), bytes(out)

    def shielder_prove_update(self, pk_deposit, pk_withdraw, knowledge, op_pub, op_priv, trapdoor, nullifier, merkle_proof,
                              leaf_id, r, s):
        """ZkProof::update_account with a real proof: (h_note_new, merkle_root, new ZkProof, proof bytes)."""
        height = len(merkle_proof)
        mp = (Scalar * height)(*[scalar(x) for x in merkle_proof])
        t, n = scalar(trapdoor), scalar(nullifier)
        h, root, new = Scalar(), Scalar(), ZkProof()
        out = (C.c_uint8 * 192)()
        self._chk(self.z.lib.zkmi_shielder_prove_update(
            self.h, pk_deposit.h if pk_deposit else None, pk_withdraw.h if pk_withdraw else None, C.byref(knowledge),
            C.byref(op_pub), C.byref(op_priv), C.byref(t), C.byref(n), mp, C.c_uint32(height), C.c_uint32(leaf_id),
            _buf(r), _buf(s), C.byref(h), C.byref(root), C.byref(new), out))
        return bytes(h.bytes), bytes(root.bytes), new, bytes(out)

    def ark_pk_load(self, r1cs, buf, compressed, check_curve=True):
        """Proving key from arkworks' ProvingKey::serialize_{compressed,uncompressed} bytes -> (ProvingKey, vk bytes)."""
        h = C.c_void_p()
        cap = 672 + 96 * r1cs.n_pub
        vk = (C.c_uint8 * cap)()
        self._chk(self.lib.zkmi_ark_pk_load(self.h, r1cs.h, _buf(buf), C.c_uint64(len(buf)), C.c_int32(int(compressed)),
                                            C.c_int32(int(check_curve)), C.byref(h), vk, C.c_uint64(cap)))
        return ProvingKey(self, h, r1cs), bytes(vk)

    def ark_pk_load_validated(self, r1cs, buf, compressed, checks=CHECK_SUBGROUP):
        """ark_pk_load for keys from outside: every query point is parsed and checked on the device under `checks`.
        A refused key raises ZkmiError (NON_CANONICAL) whose `where` is (section, index) of the refused point, or None."""
        h = C.c_void_p()
        cap = 672 + 96 * r1cs.n_pub
        vk = (C.c_uint8 * cap)()
        where = (C.c_uint64 * 2)(NO_INDEX, NO_INDEX)
        rc = self.lib.zkmi_ark_pk_load_validated(self.h, r1cs.h, _buf(buf), C.c_uint64(len(buf)), C.c_int32(int(compressed)),
                                                 C.c_int32(checks), C.byref(h), vk, C.c_uint64(cap), where)
        if rc != 0:
            err = ZkmiError(rc, (self.lib.zkmi_last_error(self.h) or b"").decode())
            err.where = None if where[0] == NO_INDEX else (int(where[0]), None if where[1] == NO_INDEX else int(where[1]))
            assert not h.value
            raise err
        return ProvingKey(self, h, r1cs), bytes(vk)

    def ark_pk_write(self, pk, vk, compressed):
        need = C.c_uint64()
        self.lib.zkmi_ark_pk_write(self.h, pk.h, _buf(vk), C.c_int32(int(compressed)), None, C.c_uint64(0), C.byref(need))
        out = (C.c_uint8 * need.value)()
        self._chk(self.lib.zkmi_ark_pk_write(self.h, pk.h, _buf(vk), C.c_int32(int(compressed)), out, need, C.byref(need)))
        return bytes(out)

    def groth16_prove(self, pk, z, r, s):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_groth16_prove(self.h, pk.h, _buf(z), _buf(r), _buf(s), out))
        return bytes(out)

    def groth16_prove_dev(self, pk, d_z_ptr, r, s):
        out = (C.c_uint8 * 192)()
        self._chk(self.lib.zkmi_groth16_prove_dev(self.h, pk.h, C.c_void_p(d_z_ptr), _buf(r), _buf(s), out))
        return bytes(out)

    def groth16_prove_batch_dev(self, pk, d_z_ptrs, rs, ss):
        n = len(d_z_ptrs)
        ptrs = (C.c_void_p * n)(*d_z_ptrs)
        out = (C.c_uint8 * (192 * n))()
        self._chk(self.lib.zkmi_groth16_prove_batch_dev(self.h, pk.h, C.c_uint32(n), ptrs, _buf(b"".join(rs)), _buf(b"".join(ss)), out))
        raw = bytes(out)
        return [raw[192 * i : 192 * i + 192] for i in range(n)]

    def groth16_prove_batch_host(self, pk, z_ptrs, rs, ss):
        """z_ptrs: HOST addresses of the witnesses (pinned for an asynchronous upload)."""
        n = len(z_ptrs)
        ptrs = (C.c_void_p * n)(*z_ptrs)
        out = (C.c_uint8 * (192 * n))()
        self._chk(self.lib.zkmi_groth16_prove_batch(self.h, pk.h, C.c_uint32(n), ptrs, _buf(b"".join(rs)), _buf(b"".join(ss)), out))
        raw = bytes(out)
        return [raw[192 * i : 192 * i + 192] for i in range(n)]

    def groth16_witness_map(self, pk, z):
        out = (C.c_uint8 * (32 << pk.r1cs.log_n))()
        self._chk(self.lib.zkmi_groth16_witness_map(self.h, pk.h, _buf(z), out))
        return bytes(out)


class BnBases:
    def __init__(self, ctx, h, n):
        self.ctx, self.h, self.n = ctx, h, n

    def prepare(self):
        """Fixed-base table for repeated commitments against this SRS (zkmi_bn254_srs_prepare)."""
        self.ctx._chk(self.ctx.lib.zkmi_bn254_srs_prepare(self.ctx.h, self.h))
        return self

    def read(self, first, count):
        out = (C.c_uint8 * (64 * max(1, count)))()
        self.ctx._chk(self.ctx.lib.zkmi_bn254_bases_read(self.ctx.h, self.h, C.c_uint64(first), C.c_uint64(count), out))
        return bytes(out)[: 64 * count]

    def free(self):
        if self.h:
            self.ctx.lib.zkmi_bn254_bases_free(self.h)
            self.h = None


class Bases:
    def __init__(self, ctx, h, group, n):
        self.ctx, self.h, self.group, self.n = ctx, h, group, n

    def read(self, first, count):
        w = 96 if self.group == 1 else 192
        out = (C.c_uint8 * (w * count))()
        fn = self.ctx.lib.zkmi_bases_g1_read if self.group == 1 else self.ctx.lib.zkmi_bases_g2_read
        self.ctx._chk(fn(self.ctx.h, self.h, C.c_uint64(first), C.c_uint64(count), out))
        return bytes(out)

    def prepare(self):
        """Table of 2^(c w) multiples for repeated full-length MSMs over these bases (zkmi_bases_g{1,2}_prepare)."""
        fn = self.ctx.lib.zkmi_bases_g1_prepare if self.group == 1 else self.ctx.lib.zkmi_bases_g2_prepare
        self.ctx._chk(fn(self.ctx.h, self.h))
        return self

    def free(self):
        if self.h:
            fn = self.ctx.lib.zkmi_bases_g1_free if self.group == 1 else self.ctx.lib.zkmi_bases_g2_free
            fn(self.h)
            self.h = None


class Srs:
    """A resident phase-1 transcript (zkmi_srs): sections 0 tau_g1, 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1, 4 beta_g2."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def shape(self):
        out = (C.c_uint64 * 3)()
        self.ctx._chk(self.ctx.lib.zkmi_srs_shape(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def read(self, section, first, count):
        w = 192 if section in (1, 4) else 96
        out = (C.c_uint8 * (w * max(1, count)))()
        self.ctx._chk(self.ctx.lib.zkmi_srs_read(self.ctx.h, self.h, C.c_int32(section), C.c_uint64(first), C.c_uint64(count), out))
        return bytes(out)[: w * count]

    def verify(self, seed=None):
        """zkmi_srs_verify -> (ok, failed_mask)."""
        return self.ctx.srs_verify(self, seed)

    def contribute(self, sab):
        """zkmi_srs_contribute in place -> step_g2 (576 bytes)."""
        return self.ctx.srs_contribute(self, sab)

    def verify_contribution(self, before, step_g2, seed=None):
        """zkmi_srs_verify_contribution of this transcript against its predecessor `before` -> (ok, failed_mask)."""
        return self.ctx.srs_verify_contribution(before, self, step_g2, seed)

    def free(self):
        if self.h:
            self.ctx.lib.zkmi_srs_free(self.h)
            self.h = None


class NoteTree:
    """A resident append-only Poseidon note tree (zkmi_note_tree): batched appends, per-leaf roots and paths in HBM."""

    def __init__(self, ctx, h, field):
        self.ctx, self.h, self.field = ctx, h, field

    def shape(self):
        return self.ctx.shape(self)

    def root(self):
        return self.ctx.root(self)

    def append(self, leaves, want_roots=False):
        return self.ctx.append(self, leaves, want_roots)

    def append_dev(self, d_leaves, m, d_roots=None):
        return self.ctx.append_dev(self, d_leaves, m, d_roots)

    def paths(self, leaf_idx):
        return self.ctx.paths(self, leaf_idx)

    def paths_dev(self, leaf_idx, d_shape, d_paths):
        return self.ctx.paths_dev(self, leaf_idx, d_shape, d_paths)

    def free(self):
        if self.h:
            self.ctx.lib.zkmi_note_tree_free(self.h)
            self.h = None


class ProvingKey:
    def __init__(self, ctx, h, r1cs):
        self.ctx, self.h, self.r1cs = ctx, h, r1cs

    def export_query(self, which, first, count):
        w = 192 if which == 2 else 96
        out = (C.c_uint8 * (w * count))()
        self.ctx._chk(self.ctx.lib.zkmi_pk_export_query(self.ctx.h, self.h, C.c_int32(which), C.c_uint64(first), C.c_uint64(count), out))
        return bytes(out)

    def check(self, checks=CHECK_SUBGROUP):
        """zkmi_pk_check: every point of the resident key under `checks`.  None when all pass, else (section, index) of the
        first refused point (sections 0..4 = a, b_g1, b_g2, h, l queries; 5 = alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2)."""
        where = (C.c_uint64 * 2)(NO_INDEX, NO_INDEX)
        rc = self.ctx.lib.zkmi_pk_check(self.ctx.h, self.h, C.c_int32(checks), where)
        if rc == -2:
            return int(where[0]), int(where[1])
        self.ctx._chk(rc)
        return None

    def contribute(self, d):
        """zkmi_pk_contribute: one phase-2 contribution d (32 B canonical, 0 < d < r) in place -> (delta_g1, delta_g2), the
        new elements; the caller patches vk[480:672] with delta_g2."""
        assert len(d) == 32
        d1, d2 = (C.c_uint8 * 96)(), (C.c_uint8 * 192)()
        self.ctx._chk(self.ctx.lib.zkmi_pk_contribute(self.ctx.h, self.h, _buf(d), d1, d2))
        return bytes(d1), bytes(d2)

    def verify_contribution(self, before, seed=None):
        """zkmi_pk_verify_contribution of this key against its predecessor `before` -> (ok, failed_mask)."""
        return self.ctx.pk_verify_contribution(before, self, seed)

    def export_g1_elems(self):
        """zkmi_pk_export_g1_elems: (beta_g1, delta_g1)."""
        b, d = (C.c_uint8 * 96)(), (C.c_uint8 * 96)()
        self.ctx._chk(self.ctx.lib.zkmi_pk_export_g1_elems(self.h, b, d))
        return bytes(b), bytes(d)

    def schedule_state(self):
        """zkmi_pk_schedule_state: (B1 folded into the L + H reduction?, non-zero digits of the last finished proof's
        assignment(s), digits a dense assignment would have placed)."""
        out = (C.c_uint64 * 3)()
        self.ctx._chk(self.ctx.lib.zkmi_pk_schedule_state(self.h, out))
        return bool(out[0]), int(out[1]), int(out[2])

    def free(self):
        if self.h:
            self.ctx.lib.zkmi_pk_free(self.h)
            self.h = None
