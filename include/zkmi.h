/* zkmi — C ABI of the MI355X-native proving backend for the Shielder
 * proof-generation hot path (BLS12-381, Groth16-shaped workload).
 *
 * The reference (/root/reference = Cardinal-Cryptography/zk-apps @ v2) has no
 * FFI of its own.  Each entry point below is what a Rust
 * shim behind the reference's only "prover API" would bind — the inherent
 * methods of mocked_zk::relations::ZkProof
 *   new              shielder/mocked_zk/src/relations.rs:37-55
 *   update_account   shielder/mocked_zk/src/relations.rs:79-98   (prove step,
 *                    called at shielder/contract/drink_tests/utils/shielder.rs:105-114)
 *   verify_creation  shielder/mocked_zk/src/relations.rs:127-136 (contract/lib.rs:56)
 *   verify_update    shielder/mocked_zk/src/relations.rs:138-155 (contract/lib.rs:74)
 * and the arithmetic stages they stand in for.
 * INTEGRATION.md shows the reference-side `extern "C"` block.
 *
 * Conventions
 *   - every function returns int32_t: 0 = ZKMI_OK, negative = error; no
 *     exceptions or aborts cross the ABI; zkmi_last_error() gives a string.
 *   - Fr  : 32-byte little-endian canonical integer < r   (= Scalar{bytes:[u8;32]},
 *           shielder/mocked_zk/src/scalar.rs:1-30)
 *   - Fq  : 48-byte little-endian canonical integer < p
 *   - G1 affine : x || y (96 B);  G2 affine : x.c0 || x.c1 || y.c0 || y.c1 (192 B);
 *     all-zero bytes = point at infinity
 *   - proof : 192 B = compressed A (48) || B (96) || C (48), zcash/IETF big-endian
 *   - caller owns every buffer; the library never frees caller memory; device
 *     state lives behind opaque handles bound to one HIP device; a ctx is not
 *     thread-safe (one ctx per host thread / process / GPU).
 *   - *_dev entry points take pointers into HBM (e.g. torch tensors'
 *     data_ptr()); all other pointers are host memory.
 */
#ifndef ZKMI_H
#define ZKMI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ZKMI_OK 0
#define ZKMI_ERR_BAD_ARG (-1)
#define ZKMI_ERR_NON_CANONICAL (-2)   /* Fr/Fq >= modulus, point not on curve */
#define ZKMI_ERR_HIP (-3)             /* HIP runtime error (see zkmi_last_error) */
#define ZKMI_ERR_NO_DEVICE (-4)       /* no gfx950 device / HIP extension unusable */
#define ZKMI_ERR_VERIFICATION (-5)    /* = ZkpError::VerificationError   (mocked_zk/src/errors.rs:3-7) */
#define ZKMI_ERR_ACCOUNT_UPDATE (-6)  /* = ZkpError::AccountUpdateError */
#define ZKMI_ERR_OPERATION_COMBINE (-7) /* = ZkpError::OperationCombineError */
#define ZKMI_ERR_UNSATISFIED (-8)     /* witness does not satisfy the relation */
#define ZKMI_ERR_RCCL (-9)            /* RCCL missing or a collective failed (see zkmi_last_error) */

typedef struct zkmi_ctx zkmi_ctx;
typedef struct zkmi_bases_g1 zkmi_bases_g1;
typedef struct zkmi_bases_g2 zkmi_bases_g2;
typedef struct zkmi_r1cs zkmi_r1cs;
typedef struct zkmi_pk zkmi_pk;

/* ---- library / context -------------------------------------------------- */
/* "zkmi 0.1 (gfx950) src:<16 hex digits>": the digits are the sha256 digest of the sources the binary was built from
 * (scripts/src_digest.py; bench.py and smoke() compare it with the files beside the library: `library_matches_sources`). */
const char* zkmi_version(void);
/* Where the host-side numbers of zkmi_host_info came from, e.g. "cpus=16 (cgroup2 /sys/fs/cgroup/cpu.max) ranks=8
 * (LOCAL_WORLD_SIZE) threads=2": the CPU grant is min(logical CPUs, affinity mask, the smallest cgroup quota between the
 * process's own cgroup and the root); the ranks sharing it come from LOCAL_WORLD_SIZE (torchrun), OMPI_COMM_WORLD_LOCAL_SIZE,
 * SLURM_NTASKS_PER_NODE or MPI_LOCALNRANKS. */
const char* zkmi_host_info_string(void);
/* Fingerprint of the library's internal struct layouts (sizes and member offsets of the context, the MSM workspaces and the
 * handle types): two builds of this source tree may only share objects (a context made by one, bases made by the other --
 * what the test suite does with the testing library) when their fingerprints are equal.  out_n = values written / needed. */
int32_t zkmi_abi_layout_probe(uint64_t* out, uint32_t cap, uint32_t* out_n);
/* HIP_VERSION the library was built with / hipRuntimeGetVersion of the runtime it is bound to (diagnostics) */
int32_t zkmi_hip_versions(int32_t* out_build, int32_t* out_runtime);
/* The prover's host side: proof assembly (row a10: O(1) scalar multiplications, compression) runs on one persistent pool
 * of threads per process, sized by what the process may actually use -- min(logical CPUs, affinity mask, cgroup CPU quota)
 * divided by the processes of the job on this node (LOCAL_WORLD_SIZE, as torch.distributed.run exports it), at most 16.
 * ZKMI_HOST_THREADS=<n> (environment) or zkmi_set_host_threads override it; n = 0: the library's choice again.
 * zkmi_host_info: out[0] = CPUs granted, out[1] = local ranks, out[2] = threads per process (the caller's included),
 * out[3] = pool workers started so far.  The batch prover's driving thread sleeps between polls while it waits. */
int32_t zkmi_host_info(uint32_t out[4]);
int32_t zkmi_set_host_threads(uint32_t n);
int32_t zkmi_device_count(int32_t* out_count);
int32_t zkmi_ctx_create(int32_t device, zkmi_ctx** out_ctx);
int32_t zkmi_ctx_destroy(zkmi_ctx* ctx);
const char* zkmi_last_error(const zkmi_ctx* ctx);
int32_t zkmi_ctx_sync(zkmi_ctx* ctx);

/* per-phase HIP-event timers on the ctx stream (bench.py's roofline leg) */
#define ZKMI_PH_MSM_SORT 0
#define ZKMI_PH_MSM_ACCUM_G1 1
#define ZKMI_PH_MSM_REDUCE_G1 2
#define ZKMI_PH_MSM_ACCUM_G2 3
#define ZKMI_PH_MSM_REDUCE_G2 4
#define ZKMI_PH_NTT 5
#define ZKMI_PH_WITNESS 6
#define ZKMI_PH_MISC 7
int32_t zkmi_prof_enable(zkmi_ctx* ctx, int32_t on);
int32_t zkmi_prof_reset(zkmi_ctx* ctx);
int32_t zkmi_prof_get(zkmi_ctx* ctx, int32_t phase, double* out_total_ms, uint64_t* out_launches);

/* ---- row a6: Fr NTT ------------------------------------------------------ */
/* In-place radix-2 transform of 2^log_n Fr elements, natural order in/out.
 * inverse: 0 forward, 1 inverse (scaled by N^-1); coset: 0/1 (generator 7).
 * Replaces ark_poly::Radix2EvaluationDomain::{fft,ifft}_in_place + coset
 * variants [not in reference tree; SURVEY.md row a6]. */
int32_t zkmi_ntt_fr(zkmi_ctx* ctx, uint8_t* data, uint32_t log_n, int32_t inverse, int32_t coset);
/* Same on a device buffer of 2^log_n x 32 B canonical LE elements (in place). */
int32_t zkmi_ntt_fr_dev(zkmi_ctx* ctx, void* d_data, uint32_t log_n, int32_t inverse, int32_t coset);

/* ---- rows a8 / a9: multi-scalar multiplication --------------------------- */
/* Upload n affine points (wire format) and keep them resident in HBM in
 * Montgomery form.  check != 0 additionally verifies y^2 = x^3 + b on the host. */
int32_t zkmi_bases_g1_load(zkmi_ctx* ctx, const uint8_t* affine, uint64_t n, int32_t check, zkmi_bases_g1** out);
int32_t zkmi_bases_g1_free(zkmi_bases_g1* b);
int32_t zkmi_bases_g2_load(zkmi_ctx* ctx, const uint8_t* affine, uint64_t n, int32_t check, zkmi_bases_g2** out);
int32_t zkmi_bases_g2_free(zkmi_bases_g2* b);
/* Bases used for many MSMs of their full length (an SRS, a proving-key query): build the table 2^(c w) * P_i once
 * (ceil(255 / c) x n points of HBM).  Afterwards zkmi_msm_g{1,2}[_dev] with n == the number of bases run the prover's
 * shared-bucket schedule (12-13 insertions per scalar instead of 16); other n, and the *_windows entry points, keep the
 * windowed schedule.  Same results either way. */
int32_t zkmi_bases_g1_prepare(zkmi_ctx* ctx, zkmi_bases_g1* b);
int32_t zkmi_bases_g2_prepare(zkmi_ctx* ctx, zkmi_bases_g2* b);
int32_t zkmi_bases_g1_read(zkmi_ctx* ctx, const zkmi_bases_g1* b, uint64_t first, uint64_t count, uint8_t* out_affine);
int32_t zkmi_bases_g2_read(zkmi_ctx* ctx, const zkmi_bases_g2* b, uint64_t first, uint64_t count, uint8_t* out_affine);

/* sum_i scalars[i] * bases[i]; scalars are n x 32 B canonical LE in host memory.
 * Replaces ark_ec::VariableBaseMSM::msm_bigint / halo2curves::msm::best_multiexp
 * [not in reference tree; SURVEY.md rows a8, a9]. */
int32_t zkmi_msm_g1(zkmi_ctx* ctx, const uint8_t* scalars, uint64_t n, const zkmi_bases_g1* bases, uint8_t out_affine[96]);
int32_t zkmi_msm_g2(zkmi_ctx* ctx, const uint8_t* scalars, uint64_t n, const zkmi_bases_g2* bases, uint8_t out_affine[192]);
/* scalars already resident in HBM (n x 32 B canonical LE) */
int32_t zkmi_msm_g1_dev(zkmi_ctx* ctx, const void* d_scalars, uint64_t n, const zkmi_bases_g1* bases, uint8_t out_affine[96]);
int32_t zkmi_msm_g2_dev(zkmi_ctx* ctx, const void* d_scalars, uint64_t n, const zkmi_bases_g2* bases, uint8_t out_affine[192]);

/* Multi-GPU split of one large MSM (BASELINE config 3): each
 * rank runs the bucket method over its slice of the points and emits one
 * partial sum per window (nwin x 96 B affine, nwin <= 64); the ranks exchange
 * these few KiB (RCCL all-gather of raw bytes, done by the host layer) and
 * every rank combines locally.  *out_window_bits receives c. */
int32_t zkmi_msm_g1_windows_dev(zkmi_ctx* ctx, const void* d_scalars, uint64_t n, const zkmi_bases_g1* bases,
                                uint64_t plan_n, uint8_t* out_windows_affine, uint32_t* out_nwin, uint32_t* out_window_bits);
int32_t zkmi_msm_g1_combine(const uint8_t* windows_affine, uint32_t n_ranks, uint32_t nwin, uint32_t window_bits,
                            uint8_t out_affine[96]);

/* The same exchange behind the C ABI, one process per GPU over RCCL ("ncclAllGather, dtype ncclUint8,
 * + local EC summation and Horner combine on each rank"): the rank's partial sums stay in HBM, are all-gathered on the
 * reduction stream and combined on every rank.  libzkmi.so resolves RCCL at first use (the copy already in the process,
 * else librccl.so.1): nothing here is needed to load the library on a host without RCCL.
 *   zkmi_comm_unique_id   rank 0 draws the 128-byte id (ncclGetUniqueId); the HOST distributes the bytes to all ranks
 *   zkmi_comm_init        every rank: ncclCommInitRank on ctx's device (collective call)
 *   zkmi_comm_from_nccl   wrap an ncclComm_t the host created itself (same RCCL instance; not destroyed with the handle)
 *   zkmi_msm_g1_allgather_combine  this rank's n terms (plan from plan_n = the GLOBAL number of terms, equal on all ranks),
 *                         all-gather, combination: the FULL result on every rank.  Collective: all ranks call it.
 * ZKMI_ERR_RCCL: RCCL not found, or a call failed (zkmi_last_error).
 * Failure semantics of the two collectives: arguments, the plan and every allocation are checked before anything is
 * launched, so ZKMI_ERR_BAD_ARG never leaves the other ranks waiting PROVIDED all ranks pass consistent arguments (the same
 * plan_n, n <= their bases).  After ZKMI_ERR_HIP / ZKMI_ERR_RCCL from a collective the communicator is unusable and the
 * peers may be blocked inside ncclAllGather: abort all ranks (as after any failed NCCL collective).
 * Lifetime: zkmi_comm_destroy may run before or after zkmi_ctx_destroy of the context the handle was made on.
 * Environment: ZKMI_RCCL_LIB=<file> makes that file the only RCCL candidate (deployments with RCCL outside the loader's
 * search path; a missing file yields ZKMI_ERR_RCCL). */
typedef struct zkmi_comm zkmi_comm;
int32_t zkmi_comm_unique_id(uint8_t out_id[128]);
int32_t zkmi_comm_init(zkmi_ctx* ctx, uint32_t n_ranks, uint32_t rank, const uint8_t id[128], zkmi_comm** out);
int32_t zkmi_comm_from_nccl(zkmi_ctx* ctx, void* nccl_comm, uint32_t n_ranks, uint32_t rank, zkmi_comm** out);
int32_t zkmi_comm_destroy(zkmi_comm* comm);
int32_t zkmi_msm_g1_allgather_combine(zkmi_ctx* ctx, zkmi_comm* comm, const void* d_scalars, uint64_t n,
                                      const zkmi_bases_g1* bases, uint64_t plan_n, uint8_t out_affine[96]);

/* The WINDOW split (BASELINE configs[3] as worded: "windows split across 8 GPUs"): every rank holds ALL n scalars and
 * bases and computes the sums of a contiguous range of the plan's windows; the ranks' windows are disjoint, so the
 * exchange is a concatenation.  zkmi_msm_g1_window_range_dev: windows [w_first, w_first + w_count) of the plan of plan_n
 * terms -> w_count x 96 B (the caller combines: zkmi_msm_g1_combine over n_ranks x nwin_total windows with all-zero =
 * infinity entries where a rank owns nothing).  zkmi_msm_g1_window_split_allgather: the collective form over a zkmi_comm
 * (rank k takes windows [k nwin / R, (k + 1) nwin / R)); the full result on every rank.  The POINT split above moves 1 / R
 * of the scalars and bases per rank and is what bench.py measures by default. */
int32_t zkmi_msm_g1_window_range_dev(zkmi_ctx* ctx, const void* d_scalars, uint64_t n, const zkmi_bases_g1* bases,
                                     uint64_t plan_n, uint32_t w_first, uint32_t w_count, uint8_t* out_windows_affine,
                                     uint32_t* out_nwin_total, uint32_t* out_window_bits);
int32_t zkmi_msm_g1_window_split_allgather(zkmi_ctx* ctx, zkmi_comm* comm, const void* d_scalars, uint64_t n,
                                           const zkmi_bases_g1* bases, uint8_t out_affine[96]);
/* The 2-D split: n_ranks = P x window_groups; rank k = g * window_groups + q holds the points of group g (d_scalars / bases
 * are its slice of n points, as in the point split; plan_n = the size of the whole MSM) and computes only the windows of
 * range q of window_groups (range q: windows [q nwin / Q, (q + 1) nwin / Q)).  Per rank: 1 / n_ranks of the bucket
 * insertions like both 1-D splits, 1 / P of the points resident, 1 / Q of the buckets to reduce -- the share of a rank's
 * time that the point split leaves unscaled.  window_groups = 1 is the point split, = n_ranks the window split (over a
 * slice that is then the whole input).  window_groups must divide the communicator's size (else ZKMI_ERR_BAD_ARG, before
 * anything is launched).  The full result on every rank. */
int32_t zkmi_msm_g1_split2d_allgather(zkmi_ctx* ctx, zkmi_comm* comm, const void* d_scalars, uint64_t n, const zkmi_bases_g1* bases,
                                      uint64_t plan_n, uint32_t window_groups, uint8_t out_affine[96]);

/* What every rank computes AFTER the all-gather, on caller-supplied slots (host arithmetic; no GPU, no RCCL): partials =
 * n_ranks slots of XYZZ points in the form the reductions leave in HBM (4 x 48-byte LE Montgomery coordinates x, y, zz, zzz;
 * all-zero zz = infinity).  window_split = 0: rank k's slot holds the partial sums of ALL windows over its points (the
 * point split); 1: the partial sums of its windows [k nwin / R, (k + 1) nwin / R); Q >= 2 (Q divides n_ranks): the 2-D split
 * with Q window ranges -- rank k's slot holds the partial sums of window range k mod Q over its point group's points.  zkmi_msm_exchange_layout reports the
 * slot geometry for a plan of plan_n terms: out[0] windows, [1] partial sums per window, [2] points per slot (point
 * split), [3] points per slot (window split over n_ranks), [4] bytes per point, [5] window bits, [6] log2 of the
 * reduction's segment length, [7] log2 of the partitions the partial top window is spread over. */
int32_t zkmi_msm_g1_combine_partials(const uint8_t* partials, uint32_t n_ranks, uint64_t plan_n, int32_t window_split,
                                     uint8_t out_affine[96]);
int32_t zkmi_msm_exchange_layout(uint64_t plan_n, uint32_t n_ranks, uint32_t out[8]);

/* Same split driven from ONE process holding one ctx per GPU (SURVEY.md §8b
 * "zkmi_msm_g1_multi", BASELINE config 3): device d holds counts[d] scalars at
 * d_scalars[d] and the matching slice of the points in bases[d] (loaded on
 * ctxs[d]).  All devices are enqueued before any is waited for, then the
 * per-window partial sums are added on the host.  n_dev <= 64. */
int32_t zkmi_msm_g1_multi(zkmi_ctx* const* ctxs, uint32_t n_dev, const void* const* d_scalars, const uint64_t* counts,
                          const zkmi_bases_g1* const* bases, uint8_t out_affine[96]);

/* The bucket plan the library would use for an MSM of n terms (host logic, no GPU): shared != 0 = the prover's
 * shared-bucket schedule over precomputed tables, 0 = the windowed schedule.  out[0..5] = digit bits c, digits per
 * scalar, partitions (shared) or windows (windowed), buckets per partition/window, log2 of the reduction segment
 * length, heavy-bucket threshold. */
int32_t zkmi_msm_plan_query(uint64_t n, int32_t shared, uint32_t out[6]);

/* ---- group / encoding helpers (host) -------------------------------------- */
int32_t zkmi_g1_compress(const uint8_t affine[96], uint8_t out[48]);
int32_t zkmi_g1_decompress(const uint8_t in[48], uint8_t out_affine[96]);
int32_t zkmi_g2_compress(const uint8_t affine[192], uint8_t out[96]);
int32_t zkmi_g2_decompress(const uint8_t in[96], uint8_t out_affine[192]);
int32_t zkmi_g1_mul(const uint8_t affine[96], const uint8_t scalar[32], uint8_t out_affine[96]);
int32_t zkmi_g2_mul(const uint8_t affine[192], const uint8_t scalar[32], uint8_t out_affine[192]);
int32_t zkmi_g1_add(const uint8_t a[96], const uint8_t b[96], uint8_t out_affine[96]);
int32_t zkmi_g2_add(const uint8_t a[192], const uint8_t b[192], uint8_t out_affine[192]);
/* [r]P = O (points on the curve but outside the prime-order subgroup exist on both curves) */
int32_t zkmi_g1_in_subgroup(const uint8_t affine[96]);   /* ZKMI_OK / ZKMI_ERR_NON_CANONICAL */
int32_t zkmi_g2_in_subgroup(const uint8_t affine[192]);
int32_t zkmi_g1_generator(uint8_t out_affine[96]);
int32_t zkmi_g2_generator(uint8_t out_affine[192]);
/* reduced optimal-ate pairing e(P,Q) as 12 x 48-byte LE Fq coefficients in the
 * tower basis c0.c0.c0, c0.c0.c1, c0.c1.c0, ... (Fq12 = Fq6[w], Fq6 = Fq2[v]) */
int32_t zkmi_pairing(const uint8_t g1_affine[96], const uint8_t g2_affine[192], uint8_t out_fq12[576]);
/* prod_i e(P_i, Q_i) for n pairs in HBM: d_g1 = n x 96 B, d_g2 = n x 192 B, affine WIRE form (all zero = infinity;
 * a pair with an infinite member contributes 1).  Miller loops and their product on the device, ONE final
 * exponentiation on the host.  out_fq12: the 576 bytes zkmi_pairing writes.  The points must be in the r-order
 * subgroups (the caller's duty here, as for zkmi_pairing; use zkmi_g{1,2}_points_read_dev). n = 0: out = 1. */
int32_t zkmi_pairing_product_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, uint8_t out_fq12[576]);
/* n reduced pairings e(P_i, Q_i), Miller loop AND final exponentiation on the device: d_out_gt = n x 576 B in HBM
 * (4-byte aligned), each the bytes zkmi_pairing writes; a pair with an infinite member gives 1.  Same input form and
 * caller's duties as zkmi_pairing_product_dev.  Waits for the results.  n = 0: ZKMI_OK, nothing written. */
int32_t zkmi_pairing_batch_dev(zkmi_ctx* ctx, const void* d_g1, const void* d_g2, uint64_t n, void* d_out_gt);

/* ---- rows a1-a5, a7: relation + witness ---------------------------------- */
/* R1CS in CSR form; column 0 is the constant 1, columns [0, n_pub) are the
 * instance variables; values are 32-byte canonical LE Fr. */
int32_t zkmi_r1cs_create(uint32_t n_vars, uint32_t n_pub, uint32_t n_constraints,
                         const uint32_t* a_rowptr, const uint32_t* a_col, const uint8_t* a_val,
                         const uint32_t* b_rowptr, const uint32_t* b_col, const uint8_t* b_val,
                         const uint32_t* c_rowptr, const uint32_t* c_col, const uint8_t* c_val,
                         zkmi_r1cs** out);
int32_t zkmi_r1cs_free(zkmi_r1cs* r);
/* Semantic inputs of the hash-free chain stand-in of the first builds (the relation itself and its assignment
 * generators are test scaffolding now: include/zkmi_testing.h; the relation with real hashing is zkmi_update_note_*). */
typedef struct {
  uint8_t bytes[32];
} zkmi_fr;
typedef struct {
  zkmi_fr amount, token, user; /* op_pub.into()                                  */
  zkmi_fr old_nullifier;       /* public: old_note.nullifier                     */
  zkmi_fr new_note[4];         /* zk_id, trapdoor, nullifier, account_hash       */
  zkmi_fr old_trapdoor, old_account_hash;
  uint8_t path_shape[10];      /* MerkleProof::path_shape (0/1)                  */
  zkmi_fr path[10];            /* MerkleProof::path                              */
  zkmi_fr old_account[2];      /* TOKENS_NUMBER balances                         */
} zkmi_update_note_input;
/* value mod r (SHA-256 outputs used as Scalars by the mock can exceed r) */
int32_t zkmi_fr_reduce(const uint8_t in[32], uint8_t out[32]);
int32_t zkmi_r1cs_shape(const zkmi_r1cs* r, uint32_t* n_vars, uint32_t* n_pub, uint32_t* n_constraints, uint32_t* log_n);
/* export matrix m (0=A,1=B,2=C) as CSR; pass NULL buffers to query nnz */
int32_t zkmi_r1cs_export(const zkmi_r1cs* r, int32_t m, uint32_t* rowptr, uint32_t* col, uint8_t* val, uint64_t* nnz);
int32_t zkmi_r1cs_is_satisfied(const zkmi_r1cs* r, const uint8_t* z);

/* ---- BN254 (halo2curves::bn256) MSM / NTT, KZG-commit-shaped driver ------ *
 * The reference's relations are halo2 circuits over bn256 (shielder/Cargo.toml:26,
 * shielder/Cargo.lock:436-492); a halo2/KZG prover's hot loops are best_fft and best_multiexp
 * (crates not in tree).  Same kernels as above over the 254-bit fields.
 * Fr / Fq: 32-byte LE canonical; G1 affine: x || y (64 B), all-zero = infinity;
 * curve y^2 = x^3 + 3, generator (1, 2); NTT root = 7^((r-1)/2^28) (bn256::Fr::ROOT_OF_UNITY),
 * coset shift 7 (bn256::Fr::MULTIPLICATIVE_GENERATOR). */
typedef struct zkmi_bn_bases zkmi_bn_bases;
int32_t zkmi_bn254_bases_load(zkmi_ctx* ctx, const uint8_t* affine, uint64_t n, int32_t check, zkmi_bn_bases** out);
int32_t zkmi_bn254_bases_read(zkmi_ctx* ctx, const zkmi_bn_bases* b, uint64_t first, uint64_t count, uint8_t* out);
int32_t zkmi_bn254_bases_free(zkmi_bn_bases* b);
/* Fixed-base preparation of an SRS that is committed to many times (a halo2 prover commits every
 * column against the same ParamsKZG): builds the table 2^(c w) * P_i; MSMs / commitments of exactly
 * b->n terms then use one shared set of buckets (13 instead of 16 insertions per scalar). */
int32_t zkmi_bn254_srs_prepare(zkmi_ctx* ctx, zkmi_bn_bases* b);
int32_t zkmi_bn254_msm_g1(zkmi_ctx* ctx, const uint8_t* scalars, uint64_t n, const zkmi_bn_bases* bases, uint8_t out_affine[64]);
int32_t zkmi_bn254_msm_g1_dev(zkmi_ctx* ctx, const void* d_scalars, uint64_t n, const zkmi_bn_bases* bases, uint8_t out_affine[64]);
int32_t zkmi_bn254_ntt_fr(zkmi_ctx* ctx, uint8_t* data, uint32_t log_n, int32_t inverse, int32_t coset);
int32_t zkmi_bn254_ntt_fr_dev(zkmi_ctx* ctx, void* d_data, uint32_t log_n, int32_t inverse, int32_t coset);
/* KZG commitment from evaluations: coefficients = iNTT(evaluations) (written back to d_evals),
 * commitment = MSM(srs, coefficients); srs holds at least 2^log_n points [tau^i] G. */
int32_t zkmi_bn254_kzg_commit_dev(zkmi_ctx* ctx, void* d_evals, uint32_t log_n, const zkmi_bn_bases* srs,
                                  uint8_t out_commitment[64]);
/* KZG opening of one polynomial at one point -- halo2_proofs::arithmetic::eval_polynomial + kate_division and the
 * commitment to the quotient (poly::kzg::multiopen's inner step; halo2_proofs is a git dependency of the reference,
 * shielder/Cargo.toml:26, not in the tree): d_coeffs = n coefficients in HBM (32-byte LE canonical, constant term first),
 * *out_eval = p(zeta), out_proof = commit(q) for q(X) = (p(X) - p(zeta)) / (X - zeta).  srs holds at least n - 1 points
 * [tau^i] G (a prepared SRS is used through its table).  d_quotient: NULL, or n - 1 x 32 B in HBM that receive q. */
int32_t zkmi_bn254_kzg_open_dev(zkmi_ctx* ctx, const void* d_coeffs, uint64_t n, const uint8_t zeta[32], const zkmi_bn_bases* srs,
                                void* d_quotient, uint8_t out_eval[32], uint8_t out_proof[64]);

/* k polynomials of n coefficients each opened at ONE point (a rotation set of poly::kzg::multiopen): d_polys = k device
 * pointers (a host array), out_evals = k x 32 B, out_evals[j] = p_j(zeta); out_proof = commit((f - f(zeta)) / (X - zeta)) for
 * f = sum_j v^j p_j (the verifier folds commitments and evaluations with the same powers of v). */
int32_t zkmi_bn254_kzg_open_many_dev(zkmi_ctx* ctx, const void* const* d_polys, uint32_t k, uint64_t n, const uint8_t zeta[32],
                                     const uint8_t v[32], const zkmi_bn_bases* srs, uint8_t* out_evals, uint8_t out_proof[64]);
/* Grand product of a permutation argument (halo2_proofs::plonk::permutation::prover::commit: batch_invert of the
 * denominators + running product; PLONK's z(X)): d_out[0] = 1, d_out[i] = prod_{j < i} d_num[j] / d_den[j] for i < n,
 * out_total = the product over all n terms.  All arrays: n x 32-byte LE canonical Fr in HBM.  ZKMI_ERR_BAD_ARG on a zero
 * denominator (d_out is then unspecified). */
int32_t zkmi_bn254_grand_product_dev(zkmi_ctx* ctx, const void* d_num, const void* d_den, uint64_t n, void* d_out,
                                     uint8_t out_total[32]);

/* ---- the contract's SHA-256 Merkle tree, batched ------------ *
 * compute_hash / combine_merkle_hash = SHA-256(first.bytes || second.bytes)
 * (shielder/contract/merkle.rs:24-28, shielder/mocked_zk/src/lib.rs:24-28).
 * in: n_hashes x 2 x 32 B, out: n_hashes x 32 B. */
int32_t zkmi_sha256_pairs(zkmi_ctx* ctx, const uint8_t* in, uint64_t n_hashes, uint8_t* out);
int32_t zkmi_sha256_pairs_dev(zkmi_ctx* ctx, const void* d_in, uint64_t n_hashes, void* d_out);
/* MerkleTree<DEPTH> after its first n_filled add_leaf calls (merkle.rs:48-81): d_nodes holds
 * 2^(log_leaves+1) - 1 elements of 32 B, leaves first, then each level, root last; the caller
 * writes the first n_filled leaves.  A node no inserted leaf has touched does not exist in the
 * contract's mapping and reads as Scalar 0 (not as a hash of zeros) - reproduced here. */
int32_t zkmi_sha256_merkle_tree_dev(zkmi_ctx* ctx, void* d_nodes, uint32_t log_leaves, uint64_t n_filled);

/* ---- Poseidon-5 ------------------------------------------ *
 * T_WIDTH = 5, RATE = 4, R_F = 8, R_P = 56, S-box x^5
 * (shielder/relations/src/lib.rs:17-26); hashing = PoseidonHasher::hash_fix_len_array
 * (update_note.rs:100,131; update_account.rs:62; merkle_proof.rs:56): state
 * [2^64,0,0,0,0], inputs added to state[1..], a 1 added behind the last input,
 * an extra padding-only permutation when len % 4 == 0, output state[1].
 * Constants are generated with the Grain LFSR procedure of the Poseidon paper
 * (what halo2-base's OptimizedPoseidonSpec::new::<8,56,0>() runs; crate not in
 * tree).  field: the scalar field of BLS12-381 (the prover's) or of BN254 (the
 * field the reference's relations are written over). */
#define ZKMI_FIELD_BLS12_381_FR 0
#define ZKMI_FIELD_BN254_FR 1
/* constants in canonical LE form: out_rc = 64 x 5 x 32 B (round-major), out_mds = 5 x 5 x 32 B (row-major) */
int32_t zkmi_poseidon_spec(int32_t field, uint8_t* out_rc, uint8_t* out_mds);
/* n_hashes independent hash_fix_len_array calls of `arity` (0..64) inputs each, on the device.
 * in: n_hashes x arity x 32 B canonical LE (< modulus), out: n_hashes x 32 B. */
int32_t zkmi_poseidon_hash_batch(zkmi_ctx* ctx, int32_t field, const uint8_t* in, uint64_t n_hashes, uint32_t arity,
                                 uint8_t* out);
int32_t zkmi_poseidon_hash_batch_dev(zkmi_ctx* ctx, int32_t field, const void* d_in, uint64_t n_hashes, uint32_t arity,
                                     void* d_out);
/* Binary Poseidon Merkle tree (node = hash_fix_len_array([left, right]), merkle_proof.rs:56):
 * d_nodes holds 2^(log_leaves+1) - 1 elements of 32 B; the caller fills the first 2^log_leaves
 * (the leaves); each level is appended behind the previous one, the root is the last element. */
int32_t zkmi_poseidon_merkle_tree_dev(zkmi_ctx* ctx, int32_t field, void* d_nodes, uint32_t log_leaves);
/* Merkle paths of n leaves out of that node array: out_shape = n x log_leaves selector bytes
 * (0: the sibling is the left input, merkle_proof.rs:53-55), out_paths = n x log_leaves x 32 B siblings
 * (host buffers) = MerkleProof::{path_shape, path} of zkmi_note_update. */
int32_t zkmi_poseidon_merkle_paths_dev(zkmi_ctx* ctx, const void* d_nodes, uint32_t log_leaves, const uint32_t* leaf_idx,
                                       uint32_t n, uint8_t* out_shape, uint8_t* out_paths);
/* n Merkle-path recomputations (the value CircuitMerkleProof::verify compares with the root):
 * d_leaves n x 32 B, d_shape n x depth bytes, d_paths n x depth x 32 B -> d_roots n x 32 B. */
int32_t zkmi_poseidon_merkle_roots_dev(zkmi_ctx* ctx, int32_t field, const void* d_leaves, const void* d_shape,
                                       const void* d_paths, uint32_t depth, uint64_t n, void* d_roots);

/* ---- the resident Poseidon note tree: batched appends, roots and paths in HBM ---- *
 * The relation's tree of merkle_proof.rs:38-61 (NOT the contract's SHA-256 tree above), append-only, at any height the
 * relation admits.  One rule: a tree of height h holding n leaves is the dense tree of
 * zkmi_poseidon_merkle_tree_dev(field, log_leaves = h) over those n leaves followed by 2^h - n zero leaves, byte for
 * byte: the root, every stored node, every path sibling.  The padding is never materialised: with Z_0 = 0 and
 * Z_{l+1} = hash_fix_len_array([Z_l, Z_l]), level l stores its filled prefix of ceil(n / 2^l) nodes, and a child or
 * sibling behind it is Z_l; the root of the empty tree is Z_h.  Shape bytes are those of
 * zkmi_poseidon_merkle_paths_dev (0: the sibling is the left input).
 * An append of m leaves hashes sum_l ((n+m-1 >> l) - (n >> l) + 1) nodes, not 2^h.
 * create allocates every level once (sum_l ceil(capacity / 2^l) nodes plus the Z table; nothing is reallocated later);
 * a failed allocation is ZKMI_ERR_HIP with *out NULL.  field: ZKMI_FIELD_*; height 1..ZKMI_MAX_TREE_HEIGHT; capacity
 * 1..2^height leaves.
 * ZKMI_ERR_BAD_ARG, with nothing changed: a NULL argument (the optional ones excepted), m = 0, a bad field, height or
 * capacity, n + m > capacity, a leaf_idx[i] >= n, a tree of another context or device, a device pointer of leaves,
 * roots or paths that is not 16-byte aligned.
 * ZKMI_ERR_NON_CANONICAL: a leaf >= the field's modulus.  The host entry checks on the host; _dev checks on the device
 * before any node is written (one flag, read back).
 * A refused append changes nothing: shape, root and every path are what they were, and the leaf count advances only
 * after the call has waited for its launches.  Every call waits for its result; one context means one thread. */
typedef struct zkmi_note_tree zkmi_note_tree;
int32_t zkmi_note_tree_create(zkmi_ctx* ctx, int32_t field, uint32_t height, uint64_t capacity, zkmi_note_tree** out);
int32_t zkmi_note_tree_free(zkmi_note_tree* tree);
/* out = height, capacity, n_leaves */
int32_t zkmi_note_tree_shape(const zkmi_note_tree* tree, uint64_t out[3]);
int32_t zkmi_note_tree_root(zkmi_ctx* ctx, const zkmi_note_tree* tree, uint8_t out_root[32]);
/* m leaves (32 B canonical LE each) appended at indices n .. n+m-1.  out_root (optional) = the new root; out_roots /
 * d_roots (optional) = m x 32 B, roots[j] = the root of the tree holding leaves 0 .. n+j: what the contract's add_leaf
 * logs per leaf (contract/merkle.rs:48-80).  roots[m-1] = out_root. */
int32_t zkmi_note_tree_append(zkmi_ctx* ctx, zkmi_note_tree* tree, const uint8_t* leaves, uint64_t m, uint8_t out_root[32],
                              uint8_t* out_roots);
int32_t zkmi_note_tree_append_dev(zkmi_ctx* ctx, zkmi_note_tree* tree, const void* d_leaves, uint64_t m, uint8_t out_root[32],
                                  void* d_roots);
/* Paths of k leaves against the current root: k x height shape bytes, k x height x 32 B siblings, leaf level first
 * (MerkleProof::{path_shape, path} of zkmi_note_update; the inputs of zkmi_poseidon_merkle_roots_dev).  leaf_idx is a
 * host array in both; indices may repeat and come in any order.  k = 0 writes nothing. */
int32_t zkmi_note_tree_paths(zkmi_ctx* ctx, const zkmi_note_tree* tree, const uint64_t* leaf_idx, uint32_t k, uint8_t* out_shape,
                             uint8_t* out_paths);
int32_t zkmi_note_tree_paths_dev(zkmi_ctx* ctx, const zkmi_note_tree* tree, const uint64_t* leaf_idx, uint32_t k, void* d_shape,
                                 void* d_paths);

/* ---- rows a1-a5 with real hashing: the update_note relation ---------------- *
 * update_note_circuit (shielder/relations/src/relations/update_note.rs:106-149) with
 * verify_note_circuit (:91-103), CircuitMerkleProof::verify (merkle_proof.rs:38-61)
 * and update_account_circuit (update_account.rs:68-95) over the concrete account the
 * mock defines (two (token, balance) slots, u128 balances; mocked_zk/src/account.rs),
 * arithmetised as R1CS with Poseidon-5 and padded with the multiplication chain to
 * constraints + publics = 2^log_n, variables = 2^log_n (log_n >= 13).
 * Public inputs, in the order update_note.rs:121,127 fixes:
 *   amount, token, user, new_note_hash, merkle_root, old_note.nullifier. */
#define ZKMI_OP_DEPOSIT 0
#define ZKMI_OP_WITHDRAW 1
#define ZKMI_MAX_TREE_HEIGHT 32
typedef struct {
  zkmi_fr amount, token, user;   /* op_pub                                          */
  zkmi_fr new_note[3];           /* zk_id, trapdoor, nullifier (account_hash derived) */
  zkmi_fr old_note[3];           /* zk_id, trapdoor, nullifier                      */
  /* TREE_HEIGHT is a const generic of the reference (merkle_proof.rs:11); here a run-time field:
   * the first tree_height entries of path_shape / path are used.  0 = ZKMI_MERKLE_TREE_DEPTH (10). */
  uint32_t tree_height;
  uint8_t path_shape[ZKMI_MAX_TREE_HEIGHT]; /* MerkleProof::path_shape              */
  zkmi_fr path[ZKMI_MAX_TREE_HEIGHT];       /* MerkleProof::path                    */
  zkmi_fr op_priv_user;          /* op_priv                                         */
  zkmi_fr account[4];            /* old account: token_0, balance_0, token_1, balance_1 */
} zkmi_note_update;
/* log_n >= 13 (the relation proper has ~5.7 k constraints at height 10); tree_height 1..32 */
int32_t zkmi_update_note_r1cs(uint32_t log_n, int32_t op_kind, zkmi_r1cs** out); /* height 10 */
int32_t zkmi_update_note_r1cs_h(uint32_t log_n, int32_t op_kind, uint32_t tree_height, zkmi_r1cs** out);
/* Full assignment (2^log_n x 32 B) from the semantic inputs; the note/account hashes, the
 * Merkle root and every S-box intermediate are computed here.  out_publics (optional)
 * receives the 6 public inputs.  Returns ZKMI_ERR_ACCOUNT_UPDATE / ZKMI_ERR_OPERATION_COMBINE
 * (the mock's ZkpError variants) when the update is impossible: the assignment is still
 * written but does not satisfy the relation. */
int32_t zkmi_update_note_witness(uint32_t log_n, int32_t op_kind, const zkmi_note_update* in, uint8_t* out_z,
                                 uint8_t* out_publics);

/* SURVEY.md 8f-1 "witness generation on device": n instances at once, one GPU thread per
 * instance walking the same statement sequence (value-only).  `in` = host array of n inputs,
 * d_z_out[i] = device buffer of 2^log_n x 32 B for instance i (ready for zkmi_groth16_prove_dev /
 * _prove_batch_dev), out_status[i] = ZKMI_OK or the mock's error code for that instance. */
int32_t zkmi_update_note_witness_batch_dev(zkmi_ctx* ctx, uint32_t log_n, int32_t op_kind, const zkmi_note_update* in,
                                           uint32_t n, void* const* d_z_out, int32_t* out_status);
/* zkmi_update_note_witness_batch_dev with tree_height / path_shape / path of every in[i] ignored and taken on the
 * device from the path of leaf_idx[i] (a host array) in `tree`, against its current root: no path travels through the
 * host.  BLS12-381 Fr trees only (a BN254 tree, a tree of another context, a leaf_idx[i] >= n_leaves:
 * ZKMI_ERR_BAD_ARG); the batch's height is the tree's.  The leaf at leaf_idx[i] is NOT compared with the instance's
 * old-note hash: the relation computes the root, so a mismatch gives a satisfying assignment for another root.
 * Statuses are those of zkmi_update_note_witness_batch_dev. */
int32_t zkmi_update_note_witness_batch_tree_dev(zkmi_ctx* ctx, uint32_t log_n, int32_t op_kind, const zkmi_note_update* in,
                                                const zkmi_note_tree* tree, const uint64_t* leaf_idx, uint32_t n,
                                                void* const* d_z_out, int32_t* out_status);
/* the same device code executed on the host for one instance (test hook: must equal
 * zkmi_update_note_witness byte for byte) */
int32_t zkmi_update_note_witness_values_host(uint32_t log_n, int32_t op_kind, const zkmi_note_update* in, uint8_t* out_z);

/* ---- rows a7, a10: Groth16 ------------------------------------------------ */
/* Trusted setup with explicit toxic waste tau|alpha|beta|gamma|delta
 * (5 x 32 B), heavy part (fixed-base multiplications) on the device.  The
 * proving key stays resident in HBM; vk_out receives
 *   alpha_g1 (96) | beta_g2 (192) | gamma_g2 (192) | delta_g2 (192) | n_pub x gamma_abc_g1 (96 each). */
int32_t zkmi_groth16_setup(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const uint8_t toxic[160], zkmi_pk** out_pk,
                           uint8_t* vk_out, uint64_t vk_cap);
/* Proofs of small domains travel through the batch prover in groups (one digit sort and one accumulation launch per
 * query for up to 64 proofs).  group = 0: the library's choice (about 2^20 constraints per group), 1: never group,
 * 2..64: at most that many (clamped to what the key's domain allows).  Applies to keys created on `ctx` AFTER the call. */
int32_t zkmi_ctx_set_group_size(zkmi_ctx* ctx, uint32_t group);
/* Load a proving key from host arrays in wire format (drop-in for a key
 * produced by another Groth16 implementation). */
int32_t zkmi_pk_load(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const uint8_t alpha_g1[96], const uint8_t beta_g1[96],
                     const uint8_t beta_g2[192], const uint8_t delta_g1[96], const uint8_t delta_g2[192],
                     const uint8_t* a_query, const uint8_t* b_g1_query, const uint8_t* b_g2_query,
                     const uint8_t* h_query, const uint8_t* l_query, zkmi_pk** out_pk);
int32_t zkmi_pk_free(zkmi_pk* pk);
int32_t zkmi_pk_shape(const zkmi_pk* pk, uint32_t* n_vars, uint32_t* n_pub, uint32_t* log_n);
int32_t zkmi_pk_export_g1_elems(const zkmi_pk* pk, uint8_t out_beta_g1[96], uint8_t out_delta_g1[96]);
/* What the prover learned from the last finished proof (group) of this key, and what it decided from it: out[0] = 1 while
 * the B1 MSM is folded into the reduction L and H share (taken over r z; only while the assignments fill at least 9 in 10
 * of their digits -- a witness of bits is cheaper through the sort of z), out[1] = non-zero digits the digit sort of that
 * proof's (group's) assignment(s) placed, out[2] = digits a completely dense assignment would have placed.  Diagnostic:
 * the proof bytes do not depend on it. */
int32_t zkmi_pk_schedule_state(const zkmi_pk* pk, uint64_t out[3]);
/* export one query of a resident key (0=a,1=b_g1,2=b_g2,3=h,4=l) in wire format */
int32_t zkmi_pk_export_query(zkmi_ctx* ctx, const zkmi_pk* pk, int32_t which, uint64_t first, uint64_t count, uint8_t* out);
/* witness -> proof.  z = full assignment (n_vars x 32 B, z[0] = 1); r, s =
 * prover randomness (32 B each, explicit so proofs are reproducible).
 * Replaces ark_groth16::prover::create_proof_with_assignment [not in tree]. */
int32_t zkmi_groth16_prove(zkmi_ctx* ctx, const zkmi_pk* pk, const uint8_t* z, const uint8_t r[32], const uint8_t s[32],
                           uint8_t out_proof[192]);
/* same with the witness already resident in HBM (n_vars x 32 B canonical LE) — the entry point bench.py
 * times.  Every prove entry point checks on the device that the elements are < r, that z[0] = 1 and that
 * the assignment satisfies the relation (ZKMI_ERR_NON_CANONICAL / ZKMI_ERR_UNSATISFIED). */
int32_t zkmi_groth16_prove_dev(zkmi_ctx* ctx, const zkmi_pk* pk, const void* d_z, const uint8_t r[32], const uint8_t s[32],
                               uint8_t out_proof[192]);
/* Batch of n_proofs independent proofs over one resident key (BASELINE config 2):
 * d_z[i] = device pointer to witness i, r/s = n_proofs x 32 B, out = n_proofs x 192 B.
 * Two proofs are kept in flight (GPU works on proof i+1 while the CPU finishes proof i). */
int32_t zkmi_groth16_prove_batch_dev(zkmi_ctx* ctx, const zkmi_pk* pk, uint32_t n_proofs, const void* const* d_z,
                                     const uint8_t* r, const uint8_t* s, uint8_t* out_proofs);
/* The same pipeline over HOST witnesses (z[i] = n_vars x 32 B): witness i+1 is uploaded on a copy stream
 * while earlier proofs compute.  Pin the buffers for a truly asynchronous copy.  Elements >= r are
 * detected on the device (ZKMI_ERR_NON_CANONICAL). */
int32_t zkmi_groth16_prove_batch(zkmi_ctx* ctx, const zkmi_pk* pk, uint32_t n_proofs, const uint8_t* const* z,
                                 const uint8_t* r, const uint8_t* s, uint8_t* out_proofs);
/* h-polynomial coefficients only (row a7), N x 32 B canonical LE */
int32_t zkmi_groth16_witness_map(zkmi_ctx* ctx, const zkmi_pk* pk, const uint8_t* z, uint8_t* out_h);
/* BASELINE config 2 inside ONE host process: a batch of independent proofs over n_dev GPUs,
 * proof i -> ctxs[i % n_dev]; pks[d] = the same key set up / loaded on ctxs[d] (replicas); one host thread per
 * device, no collective.  z[i]: host pointer (z_on_device = 0) or device pointer on ctxs[i % n_dev]'s GPU
 * (z_on_device = 1).  r, s: n_proofs x 32 B; out_proofs: n_proofs x 192 B in the caller's order.
 * This is what a Rust host calls where the reference's callers loop over actors and call
 * ZkProof::update_account one by one (shielder/drink_tests/mod.rs:133-207). */
int32_t zkmi_groth16_prove_batch_multi(zkmi_ctx* const* ctxs, const zkmi_pk* const* pks, uint32_t n_dev, uint32_t n_proofs,
                                       const void* const* z, int32_t z_on_device, const uint8_t* r, const uint8_t* s,
                                       uint8_t* out_proofs);

/* row a11: pairing check on the host CPU.  publics excludes the leading 1.
 * Validating, like arkworks' / zcash's deserialisation: proof points must be canonical compressed
 * encodings (one encoding of infinity) of points in the r-order subgroups, and so must the vk's points;
 * anything else returns ZKMI_ERR_NON_CANONICAL, a failed pairing equation ZKMI_ERR_VERIFICATION. */
int32_t zkmi_groth16_verify(const uint8_t* vk, uint32_t n_pub, const uint8_t* publics, const uint8_t proof[192]);

/* A verifying key validated ONCE (host only, no context): exactly the checks zkmi_groth16_verify makes on its vk
 * argument at every call -- canonical wire form, curve, subgroup of alpha, beta, gamma, delta and every gamma_abc.
 * ZKMI_ERR_NON_CANONICAL on a refused key (*out stays NULL). */
typedef struct zkmi_vk zkmi_vk;
int32_t zkmi_vk_prepare(const uint8_t* vk, uint32_t n_pub, zkmi_vk** out);
int32_t zkmi_vk_free(zkmi_vk* vk);

/* Batch verification of n proofs of ONE key: the points are decompressed and subgroup-checked on the device, and one
 * random linear combination of the n pairing equations is checked with n + 3 Miller loops on the device and ONE final
 * exponentiation,
 *   prod_i e(w_i A_i, B_i) * e(-(sum w_i) alpha, beta) * e(-sum_i w_i X_i, gamma) * e(-sum_i w_i C_i, delta) = 1,
 *   X_i = ic_0 + sum_j pub_ij ic_j.
 * proofs: n x 192 B (host); publics: n x (n_pub - 1) x 32 B (host).
 * weights: n x 16 B little-endian, each non-zero, drawn uniformly by the caller -- or NULL: the library draws them from
 * the OS (getrandom).  Explicit for the reason r and s are explicit in the prover: reproducible runs.
 * Accepts iff every proof would be accepted by zkmi_groth16_verify, up to a false accept with probability <= 2^-128
 * over the weights.  ZKMI_OK / ZKMI_ERR_NON_CANONICAL (some proof malformed) / ZKMI_ERR_VERIFICATION (all well formed,
 * some equation fails).  out_status (optional, n bytes): per proof; out_first_bad (optional): smallest failing index,
 * UINT64_MAX when none.  n = 0: ZKMI_OK.  A zero weight: ZKMI_ERR_BAD_ARG before anything is launched.
 * A malformed proof (status 1-4) is left out of the product, the others are still checked.  When the product over the
 * well-formed proofs is not 1 and out_status is given, the failing proofs are found by bisection: the per-proof Miller
 * values e(w_i A_i, B_i) are kept, a subset costs three scalar sums, three Miller loops and one final exponentiation.
 * Worst case (every proof bad): 2 n - 1 subsets, i.e. about 2 n final exponentiations -- as slow as the host loop;
 * k bad proofs cost at most about 2 k log2(n) subsets.  With neither out_status nor out_first_bad the call returns
 * after the first verdict (out_first_bad alone still needs the localisation to name the smallest failing index). */
#define ZKMI_PROOF_OK 0
#define ZKMI_PROOF_BAD_ENCODING 1     /* = ZKMI_PT_* of the first faulty point among A, B, C */
#define ZKMI_PROOF_NOT_ON_CURVE 2
#define ZKMI_PROOF_NOT_IN_SUBGROUP 3
#define ZKMI_PROOF_BAD_PUBLIC 4       /* a public input >= r */
#define ZKMI_PROOF_PAIRING 5          /* well formed, the equation does not hold */
int32_t zkmi_groth16_verify_batch(zkmi_ctx* ctx, const zkmi_vk* vk, uint64_t n, const uint8_t* publics,
                                  const uint8_t* proofs, const uint8_t* weights, uint8_t* out_status,
                                  uint64_t* out_first_bad);
/* Every proof of one key checked by ITS OWN equation e(A_i,B_i) e(-X_i,gamma) e(-C_i,delta) e(-alpha,beta) = 1 on the
 * device: no weights, no error term, and the same launches whatever the verdicts -- the call for proofs from outside,
 * where zkmi_groth16_verify_batch is the call for trusted or mostly good input: one exponentiation for all proofs, but a
 * bisection with one HOST exponentiation per range once something fails.  The points are read as there, X_i is summed
 * on the device from a window table of the key, ONE launch runs the 3 n + 1 Miller loops (the pair (-alpha, beta) once per
 * call), and one lane pair per proof multiplies its four values and raises the product to (p^12 - 1)/r: no pairing and
 * no final exponentiation runs on the host.  Arguments, statuses (ZKMI_PROOF_*), return codes and out_first_bad as
 * zkmi_groth16_verify_batch; out_status is required (NULL: ZKMI_ERR_BAD_ARG, as a NULL proofs or publics with n > 0,
 * before anything is launched).  A malformed proof keeps status 1-4.  n = 0: ZKMI_OK. */
int32_t zkmi_groth16_verify_each(zkmi_ctx* ctx, const zkmi_vk* vk, uint64_t n, const uint8_t* publics,
                                 const uint8_t* proofs, uint8_t* out_status, uint64_t* out_first_bad);

/* ---- keys in arkworks' CanonicalSerialize layout (drop-in for keys made by ark-groth16) -------- *
 * VerifyingKey = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | Vec<gamma_abc_g1>;
 * ProvingKey = vk | beta_g1 | delta_g1 | Vec a | Vec b_g1 | Vec b_g2 | Vec h | Vec l; Vec = u64 LE length + elements;
 * points in the zcash-style big-endian encoding, compressed (48 / 96 B) or not (96 / 192 B).
 * Layout restated from ark-groth16 0.4 / ark-serialize 0.4 / ark-bls12-381 0.4 [not in the reference tree;
 * oracle/README.md rows 8, 10].  A compressed Proof is this library's 192-byte proof as is. */
int32_t zkmi_ark_vk_read(const uint8_t* buf, uint64_t len, int32_t compressed, uint8_t* out_vk, uint64_t vk_cap,
                         uint32_t* out_n_pub, uint64_t* out_consumed);
/* out may be NULL to query the size; *out_len receives the bytes needed / written */
int32_t zkmi_ark_vk_write(const uint8_t* vk, uint32_t n_pub, int32_t compressed, uint8_t* out, uint64_t cap, uint64_t* out_len);
/* proving key for `r1cs` from arkworks bytes (shape must match: n_vars, n_pub, domain); out_vk optional.
 * The points are decompressed one by one on the host, and the queries are checked for curve membership only, never
 * for the prime-order subgroups: a key that did not come from your own setup belongs in zkmi_ark_pk_load_validated
 * below, which does both on the device. */
int32_t zkmi_ark_pk_load(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const uint8_t* buf, uint64_t len, int32_t compressed,
                         int32_t check_curve, zkmi_pk** out_pk, uint8_t* out_vk, uint64_t vk_cap);
int32_t zkmi_ark_pk_write(zkmi_ctx* ctx, const zkmi_pk* pk, const uint8_t* vk, int32_t compressed, uint8_t* out,
                          uint64_t cap, uint64_t* out_len);

/* ---- point arrays parsed, decompressed and checked on the device (key and SRS ingest) ---------- *
 * Three byte encodings of a BLS12-381 point, with exactly the acceptance rules of the host entry points
 * (zkmi_g1_decompress, zkmi_bases_g1_load, zkmi_ark_pk_load, ...):
 *   WIRE               this library's affine form: little-endian x | y (G2: x.c0 x.c1 y.c0 y.c1), 96 / 192 B,
 *                      all zero = infinity, every coordinate < p
 *   ZCASH_COMPRESSED   48 / 96 B big-endian, bit 7 set, infinity only as 0xC0 00.., bit 5 = y is the larger root
 *   ZCASH_UNCOMPRESSED 96 / 192 B big-endian, bit 7 clear, infinity only as 0x40 00.., bit 5 clear
 * checks: CURVE = y^2 = x^3 + b (a compressed point is on the curve or has no root: implied); SUBGROUP = [r]P = O,
 * what arkworks' Validate::Yes and the zcash format ask of every point (implies CURVE). */
#define ZKMI_ENC_WIRE 0
#define ZKMI_ENC_ZCASH_COMPRESSED 1
#define ZKMI_ENC_ZCASH_UNCOMPRESSED 2
#define ZKMI_CHECK_CURVE 1
#define ZKMI_CHECK_SUBGROUP 2
/* per-element status bytes; an element with several faults reports the smallest */
#define ZKMI_PT_OK 0
#define ZKMI_PT_BAD_ENCODING 1    /* flag bits, non-canonical infinity, coordinate >= p */
#define ZKMI_PT_NOT_ON_CURVE 2    /* no square root / curve equation fails */
#define ZKMI_PT_NOT_IN_SUBGROUP 3
/* n points in HBM (d_in 4-byte aligned) -> affine WIRE form in HBM (d_out_wire may be NULL: validate only);
 * d_status: NULL or n bytes in HBM; *out_first_bad (optional): smallest failing index, UINT64_MAX when none.
 * ZKMI_OK, or ZKMI_ERR_NON_CANONICAL when any element fails (d_out_wire is then unspecified at failing indices). */
int32_t zkmi_g1_points_read_dev(zkmi_ctx* ctx, const void* d_in, uint64_t n, int32_t encoding, int32_t checks,
                                void* d_out_wire, void* d_status, uint64_t* out_first_bad);
int32_t zkmi_g2_points_read_dev(zkmi_ctx* ctx, const void* d_in, uint64_t n, int32_t encoding, int32_t checks,
                                void* d_out_wire, void* d_status, uint64_t* out_first_bad);
/* host bytes in any of the encodings -> resident bases, parsed / decompressed / checked on the device; a refused
 * load returns ZKMI_ERR_NON_CANONICAL, leaves *out NULL and names the element in *out_first_bad (optional) */
int32_t zkmi_bases_g1_load_encoded(zkmi_ctx* ctx, const uint8_t* points, uint64_t n, int32_t encoding, int32_t checks,
                                   zkmi_bases_g1** out, uint64_t* out_first_bad);
int32_t zkmi_bases_g2_load_encoded(zkmi_ctx* ctx, const uint8_t* points, uint64_t n, int32_t encoding, int32_t checks,
                                   zkmi_bases_g2** out, uint64_t* out_first_bad);
/* zkmi_ark_pk_load with every query point parsed on the device under `checks`; the verifying-key part, beta_g1 and
 * delta_g1 are validated on the host (subgroup included).  out_where (optional): [0] = section of the refused point
 * (0..4 = a, b_g1, b_g2, h, l; 5 = vk / beta_g1 / delta_g1), [1] = its index there (UINT64_MAX in section 5);
 * UINT64_MAX twice when the refusal is not about a point.  A refused key returns ZKMI_ERR_NON_CANONICAL and leaves *out_pk NULL. */
int32_t zkmi_ark_pk_load_validated(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const uint8_t* buf, uint64_t len,
                                   int32_t compressed, int32_t checks, zkmi_pk** out_pk, uint8_t* out_vk,
                                   uint64_t vk_cap, uint64_t out_where[2]);
/* a key that is already resident (zkmi_pk_load, zkmi_groth16_setup): every query point on the device, the five single
 * elements (section 5: alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2) on the host.  checks must not be 0. */
int32_t zkmi_pk_check(zkmi_ctx* ctx, const zkmi_pk* pk, int32_t checks, uint64_t out_where[2]);

/* ---- phase-1 transcripts ("powers of tau" with alpha and beta) and transforms of point arrays ------------------- *
 * The first layers of a setup that never sees the toxic waste: a ceremony transcript -- the five point arrays
 * [tau^i]G1, [tau^i]G2, [alpha tau^i]G1, [beta tau^i]G1, [beta]G2 -- resident and checked on the device, and the
 * transform that turns powers of tau into the Lagrange basis [L_i(tau)]G "in the exponent"; then the circuit-specific
 * step: zkmi_groth16_setup_from_srs derives a relation's key from the transcript (the sums over the R1CS columns and the
 * h query, on the device) and zkmi_pk_contribute applies a phase-2 contribution to delta.  The checks a ceremony
 * verifier makes run here too: zkmi_srs_verify holds a transcript to the same-ratio equations, and
 * zkmi_pk_verify_contribution holds a contributed key to its predecessor (below). */
/* In-place transform of 2^log_n points in HBM, affine WIRE form (all zero = infinity), natural order in and out:
 * out[i] = sum_k w^(ik) in[k] (forward), out[i] = N^-1 sum_k w^(-ik) in[k] (inverse), w = the root zkmi_ntt_fr uses.
 * The points must be in the r-order subgroup (caller's duty, as for zkmi_pairing_product_dev); a coordinate >= p is
 * refused (ZKMI_ERR_NON_CANONICAL, nothing written).  log_n 0..26.  Waits for the result. */
int32_t zkmi_g1_points_ntt_dev(zkmi_ctx* ctx, void* d_points, uint32_t log_n, int32_t inverse);
int32_t zkmi_g2_points_ntt_dev(zkmi_ctx* ctx, void* d_points, uint32_t log_n, int32_t inverse);
typedef struct zkmi_srs zkmi_srs;
/* Phase-1 transcript from host bytes in any ZKMI_ENC_* encoding, parsed / decompressed / checked on the device
 * under `checks` (ZKMI_CHECK_*), exactly as zkmi_bases_g{1,2}_load_encoded does:
 *   tau_g1 n_tau_g1 points [tau^i]G1, tau_g2 n_tau_g2 points [tau^i]G2, alpha_tau_g1 / beta_tau_g1 n_ab points each,
 *   beta_g2 one point.  Also refused (ZKMI_ERR_NON_CANONICAL): tau_g1[0] != G1 generator, tau_g2[0] != G2 generator.
 * out_where (optional): [0] = section of the refused point (0 tau_g1, 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1,
 * 4 beta_g2), [1] = index; UINT64_MAX twice when no point was refused.  A refused transcript leaves *out NULL.
 * NOT checked by the load: that the arrays are consistent powers of ONE tau, alpha and beta -- the pairing "same ratio"
 * checks of a ceremony verifier.  A transcript that fails those yields a key that proves nothing: run zkmi_srs_verify
 * on the handle before a key is derived from it.  The handle remembers `checks`. */
int32_t zkmi_srs_load(zkmi_ctx* ctx, int32_t encoding, int32_t checks,
                      const uint8_t* tau_g1, uint64_t n_tau_g1, const uint8_t* tau_g2, uint64_t n_tau_g2,
                      const uint8_t* alpha_tau_g1, const uint8_t* beta_tau_g1, uint64_t n_ab,
                      const uint8_t* beta_g2, zkmi_srs** out, uint64_t out_where[2]);
/* The same transcript from explicit toxic waste tau|alpha|beta (3 x 32 B), for a domain of 2^log_n: 2^(log_n+1) - 1
 * powers in tau_g1, 2^log_n in the others; fixed-base multiplications on the device.  Tests and benches only,
 * like zkmi_groth16_setup.  log_n 0..26. */
int32_t zkmi_srs_generate(zkmi_ctx* ctx, const uint8_t toxic[96], uint32_t log_n, zkmi_srs** out);
int32_t zkmi_srs_shape(const zkmi_srs* s, uint64_t out[3]);          /* n_tau_g1, n_tau_g2, n_ab */
/* count points of a section (numbered as in out_where above) from `first`, affine WIRE form (96 / 192 B each) */
int32_t zkmi_srs_read(zkmi_ctx* ctx, const zkmi_srs* s, int32_t section, uint64_t first, uint64_t count, uint8_t* out_wire);
int32_t zkmi_srs_free(zkmi_srs* s);
/* A relation's Groth16 key from a phase-1 transcript, gamma = delta = 1 (the state before any phase-2 contribution).
 * Needs n_tau_g1 >= 2N - 1, n_tau_g2 >= N, n_ab >= N for N = 2^r1cs->log_n; a longer transcript gives the same key.
 * vk_out as zkmi_groth16_setup.  The transcript is not modified and may be freed afterwards.
 * ZKMI_ERR_BAD_ARG: a NULL argument, a short transcript, a short vk_cap, a transcript of another context or device;
 * *out_pk is NULL after every refusal.  The key equals that of zkmi_groth16_setup with the same tau, alpha, beta and gamma = delta = 1, byte for byte. */
int32_t zkmi_groth16_setup_from_srs(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const zkmi_srs* srs, zkmi_pk** out_pk,
                                    uint8_t* vk_out, uint64_t vk_cap);
/* One phase-2 contribution d (32 B canonical, 0 < d < r), in place on an idle resident key: delta <- d * delta in G1
 * and G2, h_query and the non-public l_query <- d^-1 * (.).  out_delta_g1 / out_delta_g2 receive the new elements
 * (the caller patches vk bytes 480..671 with out_delta_g2).  d >= r: ZKMI_ERR_NON_CANONICAL; d = 0 or a NULL argument:
 * ZKMI_ERR_BAD_ARG; a refused call leaves the key untouched.  Waits for everything queued on the context first. */
int32_t zkmi_pk_contribute(zkmi_ctx* ctx, zkmi_pk* pk, const uint8_t d[32], uint8_t out_delta_g1[96],
                           uint8_t out_delta_g2[192]);

/* ---- verifying a ceremony: random linear combinations with weights derived on the device ------------------------ *
 * The weight of index i in domain `dom` under a 32-byte seed is
 *   w(seed, dom, i) = the first 16 bytes of SHA-256(seed[32] | LE32(dom) | LE64(i)), read as a little-endian 128-bit integer
 * (one SHA-256 block per weight, one lane per index).  Domains: the section numbers of zkmi_srs_load in phase 1 (0 tau_g1,
 * 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1), 16 + the query number of zkmi_pk_export_query in phase 2 (19 h, 20 l, the
 * index counted as that export counts it).  Every equation below is a random linear combination of the per-index
 * equations under these weights: for a seed the prover of the data did not choose (NULL draws one from the OS), data
 * that breaks a relation passes the equation that names it with probability at most 2^-128.
 *
 * m points in HBM, affine WIRE form (4-byte aligned), in the r-order subgroup (caller's duty):
 *   out_lo = sum_{i=0}^{m-2} w(seed,dom,i) * P[i],   out_hi = sum_{i=0}^{m-2} w(seed,dom,i) * P[i+1]
 * m = 1: both infinity (all-zero wire form).  m = 0 or a NULL argument: ZKMI_ERR_BAD_ARG; a coordinate >= p:
 * ZKMI_ERR_NON_CANONICAL.  Two runs of the library's MSM over one conversion of the array.  Waits for the results. */
int32_t zkmi_g1_points_adjacent_sums_dev(zkmi_ctx* ctx, const void* d_points, uint64_t m, const uint8_t seed[32],
                                         uint32_t dom, uint8_t out_lo[96], uint8_t out_hi[96]);
int32_t zkmi_g2_points_adjacent_sums_dev(zkmi_ctx* ctx, const void* d_points, uint64_t m, const uint8_t seed[32],
                                         uint32_t dom, uint8_t out_lo[192], uint8_t out_hi[192]);
/* The same-ratio checks of a resident transcript, each its own two-pair product (lo / hi: the adjacent sums of a section): */
#define ZKMI_SRS_BAD_TAU_G1    1u   /* e(hi(tau_g1), G2)        != e(lo(tau_g1), tau_g2[1]) */
#define ZKMI_SRS_BAD_TAU_G2    2u   /* e(tau_g1[1], lo(tau_g2)) != e(G1, hi(tau_g2))   (i = 0 ties tau in G1 to tau in G2) */
#define ZKMI_SRS_BAD_ALPHA     4u   /* e(hi(alpha_tau_g1), G2)  != e(lo(alpha_tau_g1), tau_g2[1]) */
#define ZKMI_SRS_BAD_BETA      8u   /* the same for beta_tau_g1 */
#define ZKMI_SRS_BAD_BETA_G2  16u   /* e(beta_tau_g1[0], G2)    != e(G1, beta_g2) */
#define ZKMI_SRS_DEGENERATE   32u   /* tau_g1[1], tau_g2[1], alpha_tau_g1[0], beta_tau_g1[0] or beta_g2 is infinity,
                                       or n_tau_g1 < 2 or n_tau_g2 < 2 (no tau to compare against) */
/* ZKMI_OK with *out_failed = 0 for a consistent transcript; ZKMI_ERR_VERIFICATION with the mask of every failed check
 * otherwise; ZKMI_ERR_BAD_ARG for NULLs or a transcript of another context or device.  A chain of one point (n_ab = 1)
 * holds: both sums are infinity.  DEGENERATE is reported alone, the equations are not evaluated then; a transcript
 * with no power of tau at all (all three lengths 1, the domain of size 1) is not degenerate: there is nothing to
 * compare, and only the anchors and BETA_G2 are checked.
 * The sums are only sound over points of the r-order subgroup (a component of small order could cancel under the
 * pairing), so a transcript that was not loaded under ZKMI_CHECK_SUBGROUP is refused with ZKMI_ERR_BAD_ARG;
 * zkmi_srs_generate counts as fully checked.  seed NULL: drawn from the OS, as zkmi_groth16_verify_batch draws its
 * weights.  Waits for everything queued on the context first; the transcript is only read. */
int32_t zkmi_srs_verify(zkmi_ctx* ctx, const zkmi_srs* srs, const uint8_t seed[32], uint32_t* out_failed);
/* One phase-2 contribution, `after` against `before` (which may itself be the result of earlier contributions: a
 * verifier chains calls): */
#define ZKMI_PK2_FIXED_PART_DIFFERS 1u  /* alpha_g1, beta_g1, beta_g2, or any entry of the a, b_g1, b_g2 queries */
#define ZKMI_PK2_BAD_DELTA          2u  /* delta' infinity, or e(delta'_g1, G2) != e(G1, delta'_g2) */
#define ZKMI_PK2_BAD_H              4u  /* e(sum w_i h'_i, delta'_g2) != e(sum w_i h_i, delta_g2),  i < N - 1 */
#define ZKMI_PK2_BAD_L              8u  /* the same over l[n_pub .. n_vars) */
/* Both keys resident on ctx and idle; the call waits for everything queued on the context first and only reads them.
 * ZKMI_OK with *out_failed = 0, ZKMI_ERR_VERIFICATION with the mask of every failed check, ZKMI_ERR_BAD_ARG for NULLs,
 * keys of another context, or keys of different shape (n_vars, n_pub, log_n).  Precondition: the points of both keys
 * are in the r-order subgroup (zkmi_pk_check, zkmi_ark_pk_load_validated, or keys this library made).  The verifying
 * key's bytes are the caller's to compare, as they are the caller's to patch.  seed NULL: drawn from the OS. */
int32_t zkmi_pk_verify_contribution(zkmi_ctx* ctx, const zkmi_pk* before, const zkmi_pk* after, const uint8_t seed[32],
                                    uint32_t* out_failed);

/* ---- phase-1 contributions: every point of an array times a scalar of its own ---------------------------------- *
 * out[i] = k[i] * P[i].  P: n points in HBM, affine WIRE form; k: n x 32 B little-endian canonical (< r) in HBM; both
 * 4-byte aligned, as d_out is; d_out may equal d_points.  Infinity in, infinity out; k[i] = 0 gives infinity.  The points
 * must be in the r-order subgroup (caller's duty).  A NULL argument or n = 0: ZKMI_ERR_BAD_ARG; a coordinate >= p or a
 * scalar >= r: ZKMI_ERR_NON_CANONICAL, nothing written.  One lane per point, a fixed signed 4-bit window: every lane of a
 * wave runs the same sequence of group operations whatever its scalar.  Waits for the result. */
int32_t zkmi_g1_points_mul_each_dev(zkmi_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out);
int32_t zkmi_g2_points_mul_each_dev(zkmi_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, void* d_out);
/* P[i] <- (c * q^i) * P[i] in place, the scalars made on the device; c, q: 32 B canonical, < r (host memory).  Otherwise
 * as above.  The library overwrites its copies of c, q and of every power before it frees them. */
int32_t zkmi_g1_points_mul_powers_dev(zkmi_ctx* ctx, void* d_points, uint64_t n, const uint8_t c[32], const uint8_t q[32]);
int32_t zkmi_g2_points_mul_powers_dev(zkmi_ctx* ctx, void* d_points, uint64_t n, const uint8_t c[32], const uint8_t q[32]);
/* One phase-1 contribution sab = s | a | b (3 x 32 B canonical, each 0 < . < r), on an idle resident transcript:
 *   tau_g1[i] <- s^i tau_g1[i], tau_g2[i] <- s^i tau_g2[i], alpha_tau_g1[i] <- a s^i (.), beta_tau_g1[i] <- b s^i (.),
 *   beta_g2 <- b beta_g2.   out_step_g2 = [s]G2 | [a]G2 | [b]G2 (3 x 192 B wire): what a verifier needs.
 * Waits for everything queued on the context first.  The new arrays are written beside the old ones and swapped in at
 * the end: a refused or failed call leaves the transcript byte for byte as it was; `checks` is kept.  A zero scalar or a
 * NULL argument: ZKMI_ERR_BAD_ARG; a scalar >= r: ZKMI_ERR_NON_CANONICAL.
 * s, a and b are toxic waste: every host and device copy the call makes of them or of their powers is overwritten
 * with zeros before it is freed.  The caller's sab is the caller's to destroy. */
int32_t zkmi_srs_contribute(zkmi_ctx* ctx, zkmi_srs* srs, const uint8_t sab[96], uint8_t out_step_g2[576]);
/* `after` is `before` moved by one contribution whose step elements are step_g2 = [s]G2 | [a]G2 | [b]G2 (a verifier chains
 * calls).  *out_failed: the ZKMI_SRS_* mask of `after` in the low six bits, exactly as zkmi_srs_verify(after, seed) reports
 * it, and on top: */
#define ZKMI_SRS_STEP_BAD_TAU     256u  /* e(after.tau_g1[1], G2)       != e(before.tau_g1[1], step_s) */
#define ZKMI_SRS_STEP_BAD_ALPHA   512u  /* e(after.alpha_tau_g1[0], G2) != e(before.alpha_tau_g1[0], step_a) */
#define ZKMI_SRS_STEP_BAD_BETA   1024u  /* the same for beta_tau_g1[0] and step_b */
#define ZKMI_SRS_STEP_DEGENERATE 2048u  /* a step element, or an anchor of `before` that a step is compared on, is infinity */
/* The step equations share the Miller-loop and final-exponentiation launches of the consistency equations; each is its own
 * two-pair product.  STEP_DEGENERATE is reported without the step equations, ZKMI_SRS_DEGENERATE without the consistency
 * ones.  A transcript with no tau_g1[1] (the domain of size 1) has no tau step to compare: STEP_BAD_TAU is not raised.
 * The step elements are parsed and subgroup-checked on the host: a bad one is ZKMI_ERR_NON_CANONICAL.  ZKMI_ERR_BAD_ARG:
 * NULLs, different shapes, a transcript of another context or device, or one not loaded under ZKMI_CHECK_SUBGROUP.
 * ZKMI_OK with *out_failed = 0, or ZKMI_ERR_VERIFICATION with the mask.  seed NULL: drawn from the OS.
 * What this proves: given a `before` that verifies, `after` is `before` moved by the discrete logarithms of the step
 * elements.  What it does NOT prove: that anybody knows those logarithms.  Proofs of knowledge of s, a and b, and the
 * hash of the transcript they are bound to, are the coordinator's protocol and the caller's to check, as the verifying
 * key's bytes are the caller's to patch. */
int32_t zkmi_srs_verify_contribution(zkmi_ctx* ctx, const zkmi_srs* before, const zkmi_srs* after, const uint8_t step_g2[576],
                                     const uint8_t seed[32], uint32_t* out_failed);

/* ---- row a12: the reference's prove/verify surface ------------------------ */
#define ZKMI_MERKLE_TREE_DEPTH 10 /* shielder/mocked_zk/src/lib.rs:16 */
#define ZKMI_TOKENS_NUMBER 2      /* shielder/mocked_zk/src/lib.rs:17 */
typedef struct { uint8_t bytes[32]; } zkmi_scalar;                 /* scalar.rs:1-6 */
typedef struct { zkmi_scalar balances[ZKMI_TOKENS_NUMBER][2]; } zkmi_account; /* account.rs:10-14, (token, balance) */
typedef struct { uint32_t kind; /* 0 Deposit, 1 Withdraw */ uint8_t amount[16]; zkmi_scalar token; zkmi_scalar user; } zkmi_op_pub; /* ops.rs:4-25 */
typedef struct { zkmi_scalar user; } zkmi_op_priv;                 /* ops.rs:28-37 */
typedef struct {                                                   /* relations.rs:14-26 */
  zkmi_scalar id, trapdoor_new, trapdoor_old, nullifier_new;
  zkmi_account acc_old, acc_new;
  zkmi_op_priv op_priv;
  zkmi_scalar merkle_proof[ZKMI_MERKLE_TREE_DEPTH];
  uint32_t merkle_proof_leaf_id;
} zkmi_zkproof;
int32_t zkmi_scalar_from_u128(const uint8_t le16[16], zkmi_scalar* out);      /* scalar.rs:14-24 */
int32_t zkmi_scalar_to_u128(const zkmi_scalar* s, uint8_t out_le16[16]);      /* scalar.rs:26-30 */
int32_t zkmi_account_new(const zkmi_scalar tokens[ZKMI_TOKENS_NUMBER], zkmi_account* out); /* account.rs:27-34 */
int32_t zkmi_account_hash(const zkmi_account* a, zkmi_scalar* out);           /* account.rs:16-24 */
int32_t zkmi_account_update(const zkmi_account* a, const zkmi_op_pub* op_pub, const zkmi_op_priv* op_priv, zkmi_account* out); /* account.rs:36-79 */
int32_t zkmi_note_hash(const zkmi_scalar* id, const zkmi_scalar* trapdoor, const zkmi_scalar* nullifier,
                       const zkmi_scalar* account_hash, zkmi_scalar* out);    /* note.rs:25-40 */
int32_t zkmi_combine_merkle_hash(const zkmi_scalar* first, const zkmi_scalar* second, zkmi_scalar* out); /* lib.rs:24-28 */
int32_t zkmi_operation_combine(const zkmi_op_pub* op_pub, const zkmi_op_priv* op_priv);   /* ops.rs:47-63 */
int32_t zkmi_zkproof_new(const zkmi_scalar* id, const zkmi_scalar* trapdoor, const zkmi_scalar* nullifier,
                         const zkmi_op_priv* op_priv, const zkmi_account* acc, zkmi_zkproof* out); /* relations.rs:37-55 */
int32_t zkmi_zkproof_update_account(const zkmi_zkproof* self, const zkmi_op_pub* op_pub, const zkmi_op_priv* op_priv,
                                    const zkmi_scalar* trapdoor, const zkmi_scalar* nullifier,
                                    const zkmi_scalar merkle_proof[ZKMI_MERKLE_TREE_DEPTH], uint32_t leaf_id,
                                    zkmi_scalar* out_h_note_new, zkmi_zkproof* out_new);  /* relations.rs:79-98 */
int32_t zkmi_zkproof_verify_creation(const zkmi_zkproof* self, const zkmi_scalar* h_note_new,
                                     const zkmi_scalar tokens[ZKMI_TOKENS_NUMBER]);       /* relations.rs:127-136 */
int32_t zkmi_zkproof_verify_update(const zkmi_zkproof* self, const zkmi_op_pub* op_pub, const zkmi_scalar* h_note_new,
                                   const zkmi_scalar* merkle_root, const zkmi_scalar* nullifier_old); /* relations.rs:138-155 */


/* ---- the same surface with REAL proofs --------------------------------------- *
 * The mock's "proof" is the witness; these entry points produce / check a Groth16 proof of the
 * Poseidon relations instead.  Scalars are arbitrary 32-byte strings in the mock; the relations
 * work over Fr, so every Scalar enters as its value mod r (zkmi_fr_reduce) and `amount` as its
 * u128 value.  h_note_new / merkle_root are Poseidon outputs (canonical Fr) produced by the prover.
 *
 * Creation relation = what verify_creation stands for (relations.rs:127-136, contract/lib.rs:50-58):
 * verify_account_circuit (update_account.rs:52-65) on Account::new(tokens) (account.rs:27-34) +
 * verify_note_circuit (update_note.rs:91-103).  Publics: h_note_new, token_0, token_1. */
typedef struct {
  zkmi_fr tokens[ZKMI_TOKENS_NUMBER];
  zkmi_fr note[3]; /* zk_id, trapdoor, nullifier */
} zkmi_note_create;
int32_t zkmi_create_note_r1cs(uint32_t log_n, zkmi_r1cs** out); /* log_n >= 11 */
int32_t zkmi_create_note_witness(uint32_t log_n, const zkmi_note_create* in, uint8_t* out_z, uint8_t* out_publics /* 3 x 32 B */);
/* ZkProof::new (relations.rs:37-55) + a proof that verify_creation's statement holds */
int32_t zkmi_shielder_prove_creation(zkmi_ctx* ctx, const zkmi_pk* pk_create, const zkmi_zkproof* knowledge,
                                     const zkmi_scalar tokens[ZKMI_TOKENS_NUMBER], const uint8_t r[32], const uint8_t s[32],
                                     zkmi_scalar* out_h_note_new, uint8_t out_proof[192]);
/* verify_creation (relations.rs:127-136): ZKMI_OK or ZKMI_ERR_VERIFICATION */
int32_t zkmi_shielder_verify_creation(const uint8_t* vk_create, const zkmi_scalar* h_note_new,
                                      const zkmi_scalar tokens[ZKMI_TOKENS_NUMBER], const uint8_t proof[192]);
/* ZkProof::update_account (relations.rs:79-98): same arguments (merkle_proof = tree_height siblings,
 * leaf first; leaf_id), same error codes (ZKMI_ERR_OPERATION_COMBINE / ZKMI_ERR_ACCOUNT_UPDATE), returns
 * (h_note_new, new ZkProof) plus the recomputed Merkle root and the 192-byte proof.  The key is picked by
 * op_pub->kind (one circuit per operation kind: deposit adds, withdraw subtracts). */
int32_t zkmi_shielder_prove_update(zkmi_ctx* ctx, const zkmi_pk* pk_deposit, const zkmi_pk* pk_withdraw,
                                   const zkmi_zkproof* self, const zkmi_op_pub* op_pub, const zkmi_op_priv* op_priv,
                                   const zkmi_scalar* trapdoor, const zkmi_scalar* nullifier,
                                   const zkmi_scalar* merkle_proof, uint32_t tree_height, uint32_t leaf_id,
                                   const uint8_t r[32], const uint8_t s[32], zkmi_scalar* out_h_note_new,
                                   zkmi_scalar* out_merkle_root, zkmi_zkproof* out_new, uint8_t out_proof[192]);
/* verify_update (relations.rs:138-155, called at contract/lib.rs:74): OpPub -> publics
 * (amount, token, user | h_note_new | merkle_root | nullifier_old: ops.rs:6-25, update_note.rs:121,127) */
int32_t zkmi_shielder_verify_update(const uint8_t* vk_deposit, const uint8_t* vk_withdraw, const zkmi_op_pub* op_pub,
                                    const zkmi_scalar* h_note_new, const zkmi_scalar* merkle_root,
                                    const zkmi_scalar* nullifier_old, const uint8_t proof[192]);

#ifdef __cplusplus
}
#endif
#endif /* ZKMI_H */
