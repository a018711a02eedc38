/* libfhecore -- MI355X-native (gfx950) FHE polynomial-arithmetic core: C ABI.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (Kelly-Zhe/GPU-FHE @ 2025-02-12) is a Python/numpy module whose whole operator surface is
 *     vec_add(a, b, MOD)   /root/reference/arithmetic.py:3-5
 *     vec_sub(a, b, MOD)   /root/reference/arithmetic.py:7-9
 *     vec_mul(a, b, MOD)   /root/reference/arithmetic.py:11-13   (= poly_mul_pointwise)
 *     NTT(x), iNTT(x)      /root/reference/arithmetic.py:15-19   (identity stubs there)
 *     poly_add(a, b, MOD)  /root/reference/ polynomial.py:3-5
 * Each entry point below names the reference function it replaces; the Python shim in
 * gpu-fhe_amd/arithmetic.py and gpu-fhe_amd/polynomial.py binds them by ctypes under the
 * reference's own names.  Components the north star names but the
 * reference lacks (Shoup/Barrett modmul, RNS base conversion, key-switch, HomMult) follow
 * the build-defined spec of SURVEY.md §8a'.
 *
 * Conventions
 *  - Return 0 on success, a negative FHE_E* code on error; fhe_last_error() (thread-local)
 *    describes the last failure.  No entry point aborts or throws.
 *  - Every data pointer is DEVICE memory owned by the caller.  Residues are uint64 in
 *    layout [poly][limb][N] (limb-major, each limb's N coefficients contiguous).  The only
 *    other element type is the double: the complex slots of fhe_encode / fhe_decode,
 *    [count][N/2][2] interleaved (re, im), and the host table of fhe_encode_roots.
 *  - `stream` is a hipStream_t (NULL = the legacy default stream).  Launches are
 *    asynchronous and capture-safe (no allocation or synchronisation inside) unless noted.
 *  - A context is immutable after creation: calls on different streams may share it.  Passing
 *    workspace == NULL uses the context's internal workspace: a call on a different stream
 *    than the previous such call first waits for the device (hipDeviceSynchronize), so calls
 *    issued one after another never overlap on it; host threads calling concurrently must each
 *    pass their own workspace.
 *  - limb0 / nlimbs select a contiguous window of the context's Q-limbs (RNS-limb sharding).
 */
#ifndef FHECORE_H
#define FHECORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_OK 0
#define FHE_EINVAL (-1)
#define FHE_ENOMEM (-2)
#define FHE_EDEVICE (-3)
#define FHE_EUNSUPPORTED (-4)

typedef struct fhe_ctx fhe_ctx;
typedef void* fhe_stream_t; /* hipStream_t */

/* Thread-local description of the last error ("" if none). */
const char* fhe_last_error(void);
/* Library version string. */
const char* fhe_version(void);

/* ---- parameters (host only) -------------------------------------------------------- */
/* The `count` largest primes q < 2^bits with q = 1 (mod 2^(log_n+1)), descending, after skipping
 * `skip` (SURVEY.md §8a' modulus chain; special primes P continue the same list). */
int fhe_gen_moduli(uint32_t log_n, uint32_t count, uint32_t bits, uint32_t skip, uint64_t* out);

/* ---- context ------------------------------------------------------------------------ */
/* Creates a context on HIP device `device` for ring degree N = 2^log_n (10 <= log_n <= 17) with
 * Q-primes q[0..L) and special primes p[0..K) (K may be 0: no key-switch) and dnum gadget digits.
 * Every modulus must be a distinct prime < 2^63 with q = 1 (mod 2N).  Moduli below 2^61 take the
 * lazy-range NTTs and, with dnum <= 4, the fused key-switch kernels; a context with any modulus in
 * [2^61, 2^63) runs exact butterflies and the unfused key-switch (same results, slower).
 * Precomputes psi^brv twiddles (psi = g^((q-1)/2N), g the smallest primitive root), Shoup
 * companions, Barrett constants and key-switch base-conversion tables; uploads them.
 * Replaces: nothing in the reference (it passes MOD per call, arithmetic.py:3). */
int fhe_ctx_create(fhe_ctx** ctx, uint32_t log_n, const uint64_t* q, uint32_t L,
                   const uint64_t* p, uint32_t K, uint32_t dnum, int device);
int fhe_ctx_destroy(fhe_ctx* ctx);
/* Copies the L + K moduli (Q then P) and their psi roots to host arrays (either may be NULL). */
int fhe_ctx_moduli(const fhe_ctx* ctx, uint64_t* moduli, uint64_t* psi);
/* log_n, L, K, dnum, device. */
int fhe_ctx_shape(const fhe_ctx* ctx, uint32_t* log_n, uint32_t* L, uint32_t* K, uint32_t* dnum,
                  int* device);
/* Grows the context's internal workspace to >= bytes (allocates; not capture-safe). */
int fhe_ctx_reserve(fhe_ctx* ctx, size_t bytes);

/* ---- coefficient-wise ops on canonical residues ------------------------------------- */
/* out = (a op b) mod q_{limb0 + l} for every poly and limb l in [0, nlimbs); inputs in [0, q).
 * out may alias a or b.  Replaces vec_add / vec_sub / vec_mul (arithmetic.py:3-13) and
 * poly_add (' polynomial.py':3-5, with polys = 2). */
int fhe_vec_add(const fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b,
                uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t stream);
int fhe_vec_sub(const fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b,
                uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t stream);
int fhe_vec_mul(const fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b,
                uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t stream);

/* Generic form used by the reference-shaped Python API: a, b, out are rows x cols matrices;
 * row r uses modulus mods[r * mod_stride] (mod_stride 0 = one scalar MOD).  `mods` is a HOST
 * array; inputs may be any uint64 (signed_in = 1: any int64), moduli any value in [2, 2^64).
 * Result = Python's exact (a op b) % MOD.  op: 0 add, 1 sub, 2 mul.
 * Up to 32 distinct modulus records (a scalar MOD, or a column of <= 32 rows) travel in the
 * kernel arguments: no allocation or synchronisation, capture-safe.  Longer modulus columns
 * allocate a stream-ordered table and synchronise `stream`. */
int fhe_vec_op_mod(int op, uint64_t* out, const uint64_t* a, const uint64_t* b, uint64_t rows,
                   uint64_t cols, const uint64_t* mods, uint64_t mod_stride, int signed_in,
                   int device, fhe_stream_t stream);

/* ---- negacyclic NTT ------------------------------------------------------------------ */
/* In place on data [polys][nlimbs][N]; limb l uses q_{limb0 + l} (limb0 + nlimbs <= L + K, so
 * P-limbs are addressable too).  Forward: natural -> bit-reversed order,
 * NTT(a)[k] = sum_i a_i psi^((2 brv(k) + 1) i); inverse: exact inverse incl. N^-1.
 * Inputs canonical in [0, q); outputs canonical.  Replaces NTT / iNTT (arithmetic.py:15-19). */
int fhe_ntt_fwd(const fhe_ctx* ctx, uint64_t* data, uint32_t polys, uint32_t limb0,
                uint32_t nlimbs, fhe_stream_t stream);
int fhe_ntt_inv(const fhe_ctx* ctx, uint64_t* data, uint32_t polys, uint32_t limb0,
                uint32_t nlimbs, fhe_stream_t stream);
/* Out of place: dst = NTT(src) / INTT(src), both [polys][nlimbs][N]; src is left untouched (the
 * first pass reads src and writes dst, the second runs in place on dst -- no copy).  dst == src is
 * the in-place call; other overlaps are undefined. */
int fhe_ntt_fwd_to(const fhe_ctx* ctx, uint64_t* dst, const uint64_t* src, uint32_t polys,
                   uint32_t limb0, uint32_t nlimbs, fhe_stream_t stream);
int fhe_ntt_inv_to(const fhe_ctx* ctx, uint64_t* dst, const uint64_t* src, uint32_t polys,
                   uint32_t limb0, uint32_t nlimbs, fhe_stream_t stream);

/* ---- ct x ct homomorphic multiplication (tensor) ----------------------------------------
 * a, b: [batch][2][nlimbs][N] coefficient form; d: [batch][3][nlimbs][N] coefficient form with
 * d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1 in Z_q[X]/(X^N + 1) (NTT -> pointwise -> INTT).
 * workspace: >= fhe_hommult_workspace(ctx, batch, nlimbs) bytes of device memory, or NULL.
 * Replaces the caller-composed NTT -> vec_mul/vec_add -> iNTT chain (SURVEY.md §3 stack 4). */
size_t fhe_hommult_workspace(const fhe_ctx* ctx, uint32_t batch, uint32_t nlimbs);
int fhe_hommult(const fhe_ctx* ctx, uint64_t* d, const uint64_t* a, const uint64_t* b,
                uint32_t batch, uint32_t limb0, uint32_t nlimbs, void* workspace,
                fhe_stream_t stream);

/* ---- RNS base conversion ---------------------------------------------------------------
 * Fast basis extension (no correction) from ctx limbs [s0, s0+S) to [t0, t0+T) (disjoint),
 * coefficient domain: in [S][N] -> out [T][N].  S <= 16.  The conversion tables of a
 * (s0, S) source range are built and uploaded on its first use and cached on the context (that
 * first call synchronises `stream`); later calls neither allocate nor synchronise. */
int fhe_baseconv(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t s0, uint32_t S,
                 uint32_t t0, uint32_t T, fhe_stream_t stream);

/* ---- hybrid key-switch (relinearisation) -------------------------------------------------
 * `batch` ciphertexts share one key.  Single-device form: d2 [batch][L][N] NTT form over Q;
 * evk_b, evk_a [dnum][L + K][N] NTT form over Q u P; ks0, ks1 [batch][L][N] NTT form:
 * ks0 + ks1 s = d2 s'' + small (SURVEY.md §8a').  The key is read once per batch.
 * Sharded form (one rank of G): c_all [batch][L][N] = INTT(d2) all-gathered (coefficient form),
 * d2_own [batch][nlimbs][N] NTT form of Q-limbs [limb0, limb0 + nlimbs), evk slices
 * [dnum][nlimbs + K][N] (own Q-limbs then all K P-limbs); outputs [batch][nlimbs][N].  The
 * sharded outputs of G ranks concatenate to the single-device result bit for bit.
 * fhe_keyswitch (and fhe_mul_relin, fhe_rotate) run the batch in passes of at most 256 MiB of
 * d2 (the Infinity Cache), so the internal workspace is sized for one pass; a caller's workspace
 * of the documented *_workspace(ctx, ..., batch) bytes is always large enough.
 * Aliasing (every key-switch entry point, incl. the _shard, _dist and _loopback forms): ks0 and
 * ks1 may each be d2 (d2_own) itself -- the in-place call, same start pointer -- or must not
 * overlap it at all; ks0 and ks1 must not overlap each other.  Any other overlap returns
 * FHE_EINVAL before anything is launched.  c_all / c_gathered, the keys and the workspace must
 * not overlap the outputs (not checked). */
size_t fhe_keyswitch_workspace(const fhe_ctx* ctx, uint32_t nlimbs, uint32_t batch);
/* The pass size of fhe_keyswitch / fhe_rotate / fhe_mul_relin for `batch` ciphertexts:
 * min(batch, the ciphertexts whose L limbs fit 256 MiB), at least 1 (0 for batch 0).  A workspace
 * of fhe_keyswitch_workspace(ctx, L, pass) (fhe_rotate_workspace(ctx, pass),
 * fhe_mul_relin_workspace(ctx, pass)) bytes is enough for any batch those calls split into passes
 * of that size. */
uint32_t fhe_keyswitch_pass_batch(const fhe_ctx* ctx, uint32_t batch);
int fhe_keyswitch(const fhe_ctx* ctx, uint64_t* ks0, uint64_t* ks1, const uint64_t* d2,
                  const uint64_t* evk_b, const uint64_t* evk_a, uint32_t batch, void* workspace,
                  fhe_stream_t stream);
int fhe_keyswitch_shard(const fhe_ctx* ctx, uint64_t* ks0, uint64_t* ks1, const uint64_t* c_all,
                        const uint64_t* d2_own, const uint64_t* evk_b, const uint64_t* evk_a,
                        uint32_t limb0, uint32_t nlimbs, uint32_t batch, void* workspace,
                        fhe_stream_t stream);

/* ---- levels below the top: key-switch, multiply-relinearise and rotation over l <= L limbs ----
 * `level` = l is the number of live Q-limbs, 1 <= l <= L: ciphertexts are [batch][2][l][N], d2 /
 * ks0 / ks1 [batch][l][N] (the rescaled product [batch][2][l-1][N]), NTT form.  The keys are the
 * caller's top-level keys [dnum][L + K][N], read in place: the same key serves every level.  The
 * level-l key-switch keeps the top-level digit width alpha = ceil(L / dnum): digits
 * D_j = [j alpha, min(l, (j + 1) alpha)) for j < ceil(l / alpha), key rows {0 .. l-1} u
 * {L .. L+K-1} of those digits (the last digit may be partial; its conversion constants are
 * precomputed per level at context creation).  level == L is bit-identical to fhe_keyswitch /
 * fhe_mul_relin / fhe_rotate, which are these calls with level = L.
 * Errors: level == 0, level > L, or rescale with level < 2 return FHE_EINVAL before any launch;
 * the aliasing rules are those of the top-level forms with l in place of L.
 * Workspace: fhe_keyswitch_workspace(ctx, L, pass), fhe_mul_relin_workspace(ctx, pass) and
 * fhe_rotate_workspace(ctx, pass) bytes are sufficient at every level (a level's regions are never
 * larger than the top level's); fhe_keyswitch_pass_batch governs the passes at every level.
 * Capture-safe like the top-level forms.
 * The hoisted rotations, the rotation sums and the linear transform have _level forms too (below,
 * after their top-level forms), and the plaintext arithmetic (linear combination with scalars,
 * plaintext multiply, level drop) is fhe_lincomb_level / fhe_mul_plain_level further
 * down. Top-level only (their current errors for fewer limbs): the multi-GPU (_shard, _dist,
 * _loopback) forms. */
int fhe_keyswitch_level(const fhe_ctx* ctx, uint64_t* ks0, uint64_t* ks1, const uint64_t* d2,
                        const uint64_t* evk_b, const uint64_t* evk_a, uint32_t level,
                        uint32_t batch, void* workspace, fhe_stream_t stream);
int fhe_mul_relin_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b,
                        const uint64_t* evk_b, const uint64_t* evk_a, uint32_t level,
                        uint32_t batch, int rescale, void* workspace, fhe_stream_t stream);
int fhe_rotate_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t galois_elt,
                     const uint64_t* rot_b, const uint64_t* rot_a, uint32_t level, uint32_t batch,
                     void* workspace, fhe_stream_t stream);

/* ---- multi-GPU: the limb-sharded key-switch over RCCL ---------------------
 * One process per GPU.  Rank r of G owns Q-limbs [r c, min((r + 1) c, L)), c = ceil(L / G)
 * (fhe_comm_shard), plus the K special limbs of the key.  A communicator is created from a
 * unique id that rank 0 makes (fhe_comm_get_unique_id) and the caller distributes out of band
 * (e.g. a torch.distributed broadcast), one fhe_comm_create per rank on its device.
 * fhe_keyswitch_dist: d2_own [batch][nlimbs][N] NTT form of the rank's limbs, evk_b / evk_a
 * [dnum][nlimbs + K][N] (own Q-limbs then all K P-limbs) -> ks0, ks1 [batch][nlimbs][N] NTT
 * form.  INTT of the own limbs, one all-gather of the coefficient-form d2 per chunk of the batch
 * (`chunks` pieces, 0 = default 4; each chunk's transfer runs on the communicator's stream and
 * overlaps the previous chunk's key-switch), then the local key-switch: the G ranks' outputs
 * concatenate to fhe_keyswitch's bit for bit.  Every rank must call it with the same batch and
 * chunks; one call at a time per communicator.
 * fhe_keyswitch_shard_ranked: the local step alone, on an all-gather output already in the
 * rank-major layout [ranks][batch][c][N] (blocks of the last ranks padded to c limbs). */
#define FHE_COMM_ID_BYTES 128
typedef struct fhe_comm_s* fhe_comm_t;
int fhe_comm_get_unique_id(uint8_t* id);
int fhe_comm_create(fhe_comm_t* comm, const uint8_t* id, int nranks, int rank, int device);
int fhe_comm_destroy(fhe_comm_t comm);
int fhe_comm_shard(const fhe_ctx* ctx, fhe_comm_t comm, uint32_t* limb0, uint32_t* nlimbs);
size_t fhe_keyswitch_dist_workspace(const fhe_ctx* ctx, fhe_comm_t comm, uint32_t batch,
                                    uint32_t chunks);
int fhe_keyswitch_dist(const fhe_ctx* ctx, fhe_comm_t comm, uint64_t* ks0, uint64_t* ks1,
                       const uint64_t* d2_own, const uint64_t* evk_b, const uint64_t* evk_a,
                       uint32_t batch, uint32_t chunks, void* workspace, fhe_stream_t stream);
int fhe_keyswitch_shard_ranked(const fhe_ctx* ctx, uint64_t* ks0, uint64_t* ks1,
                               const uint64_t* c_gathered, uint32_t ranks, const uint64_t* d2_own,
                               const uint64_t* evk_b, const uint64_t* evk_a, uint32_t limb0,
                               uint32_t nlimbs, uint32_t batch, void* workspace,
                               fhe_stream_t stream);
/* Per-chunk all-gather durations (ms, HIP events on the communicator's stream) of the last
 * fhe_keyswitch_dist call on `comm`: waits for that call's gathers; *count = its chunk count. */
int fhe_comm_gather_ms(fhe_comm_t comm, float* ms, uint32_t cap, uint32_t* count);

/* The placement plan fhe_keyswitch_dist follows (host only: no device access, callable without a
 * GPU).  Rank `rank` of `ranks` owns Q-limbs [limb0, limb0 + nlimbs); the batch is cut into
 * `chunks` chunks of `chunk_batch` ciphertexts (the last one possibly shorter, none empty); per
 * chunk every rank contributes one block of chunk_batch x width x N words (width = ceil(L / ranks),
 * padded on ranks owning fewer limbs), and the all-gather leaves the blocks rank-major in a region
 * of gather_words words: [chunks][ranks][chunk_batch][width][N].
 * fhe_dist_plan_chunk: the chunk's first ciphertext and length.
 * fhe_dist_plan_send_word: word offset in the gather region where this rank writes row (ciphertext
 * b, own limb j); fhe_dist_plan_read_word: where the key-switch reads row (b, Q-limb l) -- the
 * addressing its kernels use.  UINT64_MAX for an out-of-range argument. */
typedef struct fhe_dist_plan {
  uint32_t L, log_n, ranks, rank, batch;
  uint32_t limb0, nlimbs, width;
  uint32_t chunks, chunk_batch;
  uint64_t block_words, gather_words;
} fhe_dist_plan;
int fhe_dist_plan_make(fhe_dist_plan* plan, uint32_t L, uint32_t log_n, uint32_t ranks,
                       uint32_t rank, uint32_t batch, uint32_t chunks);
int fhe_dist_plan_chunk(const fhe_dist_plan* plan, uint32_t k, uint32_t* b0, uint32_t* bn);
uint64_t fhe_dist_plan_send_word(const fhe_dist_plan* plan, uint32_t b, uint32_t j);
uint64_t fhe_dist_plan_read_word(const fhe_dist_plan* plan, uint32_t b, uint32_t l);

/* fhe_keyswitch_dist for `ranks` ranks run one after another on this context's device (a
 * loopback communicator: the ranks' INTTs write one shared gather region, which is exactly what
 * the all-gather would leave on every rank).  Executes the G-rank plan, offsets and chunking of
 * fhe_keyswitch_dist on one GPU; per-rank arguments are host arrays of `ranks` device pointers
 * (ranks owning no limb may pass NULL), laid out as fhe_keyswitch_dist's. */
size_t fhe_keyswitch_dist_loopback_workspace(const fhe_ctx* ctx, uint32_t ranks, uint32_t batch,
                                             uint32_t chunks);
int fhe_keyswitch_dist_loopback(const fhe_ctx* ctx, uint32_t ranks, uint64_t* const* ks0,
                                uint64_t* const* ks1, const uint64_t* const* d2_own,
                                const uint64_t* const* evk_b, const uint64_t* const* evk_a,
                                uint32_t batch, uint32_t chunks, void* workspace,
                                fhe_stream_t stream);

/* Hybrid partition of a key-switch batch over `ranks` GPUs: `groups` ciphertext groups of
 * g = ranks / groups limb shards each (groups | ranks).  Rank r is limb shard r % g of group r / g;
 * group k takes the job's ciphertexts [batch0, batch0 + batch) (contiguous, ceil(job batch /
 * groups) per group, the last ones possibly shorter or empty) and runs the limb-sharded
 * key-switch above among its own g ranks: `plan` is fhe_dist_plan_make(L, log_n, g, r % g, batch,
 * chunks), the all-gather stays inside the group (the caller creates one communicator per group,
 * g ranks, with fhe_comm_create), and per-rank work is ~ batch (L / g + K) instead of the
 * limb-only job batch (L / ranks + K).  groups = 1 is the limb-only partition (the default);
 * groups = ranks replicates nothing but the key: each GPU key-switches whole ciphertexts, no
 * collective.  Host only, callable without a GPU. */
typedef struct fhe_dist_hybrid {
  uint32_t ranks, groups, g;
  uint32_t group, shard;   /* rank / g, rank % g */
  uint32_t batch0, batch;  /* the group's ciphertexts within the job's batch */
  fhe_dist_plan plan;      /* the group's limb plan for this rank */
} fhe_dist_hybrid;
int fhe_dist_hybrid_make(fhe_dist_hybrid* h, uint32_t L, uint32_t log_n, uint32_t ranks,
                         uint32_t groups, uint32_t rank, uint32_t batch, uint32_t chunks);
/* The hybrid partition's ranks run one after another on this device (per group: the loopback
 * above over its g ranks and its ciphertexts).  Per-rank host arrays of device pointers, rank r's
 * d2_own / ks0 / ks1 being [group batch][nlimbs_r][N] of its group's ciphertexts and its limbs;
 * `batch` is the job's.  The per-rank outputs equal fhe_keyswitch's rows (group k's ciphertexts,
 * shard s's limbs) bit for bit. */
size_t fhe_keyswitch_dist_hybrid_loopback_workspace(const fhe_ctx* ctx, uint32_t ranks,
                                                    uint32_t groups, uint32_t batch,
                                                    uint32_t chunks);
int fhe_keyswitch_dist_hybrid_loopback(const fhe_ctx* ctx, uint32_t ranks, uint32_t groups,
                                       uint64_t* const* ks0, uint64_t* const* ks1,
                                       const uint64_t* const* d2_own,
                                       const uint64_t* const* evk_b,
                                       const uint64_t* const* evk_a, uint32_t batch,
                                       uint32_t chunks, void* workspace, fhe_stream_t stream);

/* ---- rescale and rotation (not in the reference) ---------------------
 * Standard RNS-CKKS operations on this library's layout, restated by oracle/pyoracle.py
 * (rescale_coeff / rescale_ntt, automorphism_*, rotate).
 * fhe_rescale: divide-and-round by the last modulus.  in [polys][nlimbs][N] over Q-limbs
 * 0 .. nlimbs-1 (2 <= nlimbs <= L) -> out [polys][nlimbs-1][N], out_i = floor((X + q_l/2) / q_l)
 * mod q_i for the CRT value X; ntt_form selects NTT or coefficient form for both (the NTT form
 * needs a workspace of fhe_rescale_workspace bytes; NULL = internal). */
size_t fhe_rescale_workspace(const fhe_ctx* ctx, uint32_t polys, uint32_t nlimbs);
int fhe_rescale(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t polys,
                uint32_t nlimbs, int ntt_form, void* workspace, fhe_stream_t stream);
/* fhe_automorphism: sigma_k(a)(X) = a(X^k) for an odd Galois element k < 2N, on
 * [polys][nlimbs][N] rows over limbs [limb0, limb0 + nlimbs), NTT or coefficient form (a slot
 * permutation, resp. a signed coefficient permutation).  out must not alias in.  Rotating the
 * slots by r uses k = 5^r mod 2N, conjugation k = 2N - 1. */
int fhe_automorphism(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t polys,
                     uint32_t limb0, uint32_t nlimbs, uint32_t galois_elt, int ntt_form,
                     fhe_stream_t stream);
/* fhe_rotate: in, out [batch][2][L][N] NTT form over Q (out must not overlap in at all:
 * FHE_EINVAL -- the finish reads c0 through sigma while other workgroups write out);
 * out = (sigma_k c0 + KS0(sigma_k c1), KS1(sigma_k c1)) with rot_b, rot_a [dnum][L + K][N] the
 * key-switch key from sigma_k(s) to s (NTT form, as for fhe_keyswitch). */
size_t fhe_rotate_workspace(const fhe_ctx* ctx, uint32_t batch);
int fhe_rotate(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t galois_elt,
               const uint64_t* rot_b, const uint64_t* rot_a, uint32_t batch, void* workspace,
               fhe_stream_t stream);

/* fhe_rotate_hoisted: `count` rotations of the same ciphertexts sharing one ModUp (hoisting:
 * the INTT, base conversion and NTT of c1's digits run once; each rotation reads them through
 * its automorphism inside the inner product).  in [batch][2][L][N] NTT form over Q; out
 * [count][batch][2][L][N] (must not overlap in); galois_elts[r] with its key rot_b[r], rot_a[r]
 * ([dnum][L + K][N] device pointers in host arrays, as for fhe_rotate).  Each output decrypts to
 * sigma_k(m) like fhe_rotate's, but is not bit-identical to it (ModUp of sigma(c1) differs from
 * sigma of ModUp(c1) by multiples of the digit moduli); restated by oracle/pyoracle.py
 * rotate_hoisted. */
size_t fhe_rotate_hoisted_workspace(const fhe_ctx* ctx, uint32_t batch);
int fhe_rotate_hoisted(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in,
                       const uint32_t* galois_elts, const uint64_t* const* rot_b,
                       const uint64_t* const* rot_a, uint32_t count, uint32_t batch,
                       void* workspace, fhe_stream_t stream);

/* fhe_rotate_sum_hoisted: out = sum_r pt[r] * rot_{galois_elts[r]}(in) over `count` (1..16)
 * terms -- the inner loop of a baby-step / giant-step linear transform (CKKS bootstrapping's
 * CoeffToSlot / SlotToCoeff) -- with one ModUp of c1 and ONE ModDown per output polynomial
 * (double hoisting: each rotation's key-switch accumulators are multiplied by pt[r] and summed in
 * the extended basis Q u P before ModDown).  in, out [batch][2][L][N] NTT form over Q (out must
 * not overlap in); pt[r] [L + K][N] NTT form over Q u P (the diagonal, encoded over the extended
 * basis); galois_elts[r] == 1 is the unrotated term and takes no key (rot_b[r] / rot_a[r] may be
 * null there).  Decrypts to sum_r pt_r sigma_r(m) up to one ModDown's rounding; not bit-identical
 * to summing fhe_rotate_hoisted outputs.  Restated by oracle/pyoracle.py rotate_sum_hoisted.
 * Contexts with dnum <= 8. */
size_t fhe_rotate_sum_hoisted_workspace(const fhe_ctx* ctx, uint32_t batch);
int fhe_rotate_sum_hoisted(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in,
                           const uint32_t* galois_elts, const uint64_t* const* rot_b,
                           const uint64_t* const* rot_a, const uint64_t* const* pt,
                           uint32_t count, uint32_t batch, void* workspace, fhe_stream_t stream);

/* fhe_rotate_sum_multi: out = sum_r rot_{galois_elts[r]}(cts[r]) over `count` (1..16) DIFFERENT
 * ciphertexts (each [batch][2][L][N] NTT form over Q) with ONE ModDown: a ModUp of each rotated
 * term's own c1 (the workspace holds every term's digits), then one pass forming all the gathered
 * inner products in Q u P (the giant-step sum of a baby-step / giant-step linear transform).  galois_elts[r] == 1 adds cts[r] unrotated (no key; rot_b[r] /
 * rot_a[r] may be null).  out must not overlap any cts[r].  Decrypts to sum_r sigma_r(m_r) up to one
 * ModDown's rounding.  Restated by oracle/pyoracle.py rotate_sum_multi.  Contexts with dnum <= 8. */
size_t fhe_rotate_sum_multi_workspace(const fhe_ctx* ctx, uint32_t count, uint32_t batch);
int fhe_rotate_sum_multi(const fhe_ctx* ctx, uint64_t* out, const uint64_t* const* cts,
                         const uint32_t* galois_elts, const uint64_t* const* rot_b,
                         const uint64_t* const* rot_a, uint32_t count, uint32_t batch,
                         void* workspace, fhe_stream_t stream);

/* fhe_linear_transform: the baby-step / giant-step plaintext-matrix product of CKKS bootstrapping
 * (CoeffToSlot / SlotToCoeff) with both hoistings:
 *   out = sum_{g < n2} rot_{giant_elts[g]}( sum_{b < n1} pt[g n1 + b] * rot_{baby_elts[b]}(in) ),
 * n1, n2 in 1..16; pt[g n1 + b] [L + K][N] NTT form over Q u P (the diagonals, pre-rotated by the
 * caller as BSGS requires); element 1 in either list is an unrotated step (its keys may be null).
 * ONE ModUp of in's c1 serves every baby step; each giant step's inner sum is exactly
 * fhe_rotate_sum_hoisted(in, baby_elts, baby keys, pt[g n1 ..]) and the outer sum exactly
 * fhe_rotate_sum_multi of those.  in, out [batch][2][L][N] NTT form; out must not overlap in.
 * Restated by oracle/pyoracle.py linear_transform. */
size_t fhe_linear_transform_workspace(const fhe_ctx* ctx, uint32_t n2, uint32_t batch);
int fhe_linear_transform(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t n1,
                         uint32_t n2, const uint32_t* baby_elts, const uint64_t* const* baby_b,
                         const uint64_t* const* baby_a, const uint32_t* giant_elts,
                         const uint64_t* const* giant_b, const uint64_t* const* giant_a,
                         const uint64_t* const* pt, uint32_t batch, void* workspace,
                         fhe_stream_t stream);

/* ---- hoisted rotations, rotation sums and the linear transform over l <= L limbs -------------
 * The four calls above with `level` = l live Q-limbs (1 <= l <= L), under the rule of the _level
 * block further up: ciphertexts are [batch][2][l][N] (fhe_rotate_hoisted_level's out
 * [count][batch][2][l][N]), the digits are D_j = [j alpha, min(l, (j + 1) alpha)) for
 * j < ceil(l / alpha), and the rows run over {0 .. l-1} u {L .. L+K-1}.  The keys stay the
 * caller's top-level keys [dnum][L + K][N] and the plaintext diagonals stay [L + K][N]; both are
 * read in place at those rows (a diagonal is an integer polynomial whose residues do not depend
 * on the level, so one encoding over Q u P serves every level, like a key).  Everything else is
 * the top-level definition (oracle/pyoracle.py rotate_hoisted, rotate_sum_hoisted,
 * rotate_sum_multi, linear_transform, which take the level as level=).
 * level == L is bit-identical to the top-level forms, which are these calls with level = L.
 * Errors: level == 0 or level > L returns FHE_EINVAL before any launch; every other error and
 * aliasing rule is the top-level one with l in place of L.
 * Workspace: fhe_rotate_hoisted_workspace(ctx, batch), fhe_rotate_sum_hoisted_workspace(ctx,
 * batch), fhe_rotate_sum_multi_workspace(ctx, count, batch) and fhe_linear_transform_workspace(ctx,
 * n2, batch) bytes, sized for L, are sufficient at every level (a level's regions are never
 * larger than the top level's).  Capture-safe like the top-level forms: no allocation and no
 * synchronisation with an explicit workspace. */
int fhe_rotate_hoisted_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in,
                             const uint32_t* galois_elts, const uint64_t* const* rot_b,
                             const uint64_t* const* rot_a, uint32_t level, uint32_t count,
                             uint32_t batch, void* workspace, fhe_stream_t stream);
int fhe_rotate_sum_hoisted_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in,
                                 const uint32_t* galois_elts, const uint64_t* const* rot_b,
                                 const uint64_t* const* rot_a, const uint64_t* const* pt,
                                 uint32_t level, uint32_t count, uint32_t batch, void* workspace,
                                 fhe_stream_t stream);
int fhe_rotate_sum_multi_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* const* cts,
                               const uint32_t* galois_elts, const uint64_t* const* rot_b,
                               const uint64_t* const* rot_a, uint32_t level, uint32_t count,
                               uint32_t batch, void* workspace, fhe_stream_t stream);
int fhe_linear_transform_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t n1,
                               uint32_t n2, const uint32_t* baby_elts,
                               const uint64_t* const* baby_b, const uint64_t* const* baby_a,
                               const uint32_t* giant_elts, const uint64_t* const* giant_b,
                               const uint64_t* const* giant_a, const uint64_t* const* pt,
                               uint32_t level, uint32_t batch, void* workspace,
                               fhe_stream_t stream);

/* ---- wire format (not in the reference) ------------------------------
 * A self-describing little-endian blob for any [polys][nlimbs][N] residue tensor over context
 * limbs [limb0, limb0 + nlimbs) -- ciphertexts, keys, plaintexts: "FHEC", version 1, flags (bit 0
 * NTT form), log_n, polys, limb0, nlimbs, the nlimbs moduli, the residues, an FNV-1a-64 checksum
 * (layout in gpu-fhe_amd/csrc/serialize.cpp).  fhe_serialize copies device -> host and
 * synchronises `stream`.  fhe_deserialize validates the blob against the context (N, moduli,
 * checksum, every residue below its modulus) before copying host -> device; with dev == NULL it
 * only validates and reports the shape, so a caller can size the device buffer (dev_words). */
size_t fhe_serialized_size(const fhe_ctx* ctx, uint32_t polys, uint32_t nlimbs);
int fhe_serialize(const fhe_ctx* ctx, const uint64_t* dev, uint32_t polys, uint32_t limb0,
                  uint32_t nlimbs, int ntt_form, void* host_buf, size_t buf_size,
                  fhe_stream_t stream);
int fhe_deserialize(const fhe_ctx* ctx, const void* host_buf, size_t size, uint64_t* dev,
                    size_t dev_words, uint32_t* polys, uint32_t* limb0, uint32_t* nlimbs,
                    int* ntt_form, fhe_stream_t stream);

/* ---- sampling, keys, encryption (not in the reference) ---------------
 * Counter-based Philox4x32-10 randomness: every sample is a function of (seed, tag, poly, limb,
 * coefficient), restated bit for bit by oracle/pyoracle.py.  kind: 0 uniform mod q, 1 ternary
 * {-1, 0, 1}, 2 centred binomial eta = 21 (small kinds: one integer per coefficient on every limb).
 * Keys are NTT form: sk [L + K][N] (all context limbs); pk [2][L][N] = (-a s + e, a);
 * switch key [2][dnum][L + K][N] = (b part, a part) from s_from ([L + K][N], NTT form: s^2 for
 * relinearisation, sigma_k(s) for rotation by Galois element k) to s -- the layout fhe_keyswitch,
 * fhe_rotate and fhe_mul_relin take as (evk_b, evk_a).  Ciphertexts [2][L][N] NTT form;
 * plaintexts [L][N] NTT form.  fhe_decrypt: pt = c0 + c1 s over the first nlimbs Q-limbs of
 * `batch` ciphertexts [batch][2][nlimbs][N].
 * SECURITY: the seed is the whole nonce.  Encryption randomness (u, e0, e1, and a for fhe_encrypt_sk)
 * and a switch key's a_j are pure functions of (seed, fixed tag), so two encryptions under one key
 * with the same seed have identical masks (their difference reveals pt1 - pt2), and two switch keys
 * generated from one seed share a_j.  Never repeat a seed per secret key: draw it from a CSPRNG or
 * a per-key monotonically increasing counter.  The explicit seed exists so tests are reproducible.
 * For the batched calls below (fhe_encrypt_level, fhe_encrypt_sk_level, fhe_encrypt_slots) the
 * nonce is the pair (seed, j), j = index0 + i the ciphertext's index in the Philox counter's poly
 * field: one seed serves a stream of up to 2^32 ciphertexts, and a (seed, j) pair must never
 * repeat under one key.  fhe_encrypt / fhe_encrypt_sk are the pair (seed, 0). */
int fhe_sample(const fhe_ctx* ctx, uint64_t* out, uint32_t polys, uint32_t limb0,
               uint32_t nlimbs, int kind, uint64_t seed, uint32_t tag, fhe_stream_t stream);
int fhe_keygen_secret(const fhe_ctx* ctx, uint64_t* sk, uint64_t seed, fhe_stream_t stream);
/* fhe_keygen_secret_sparse: a secret of fixed Hamming weight h (CKKS bootstrapping: ModRaise's
 * integer polynomial obeys |I| <= (h + 2) / 2), sk [L + K][N] NTT form as fhe_keygen_secret.
 * Coefficient c draws r = philox4x32_10({c, 0xffffffff, 0, tag 4}, seed) and carries the 64-bit key
 * (r.x << 32) | c (distinct by construction); the h coefficients with the smallest keys are
 * nonzero, +1 if (r.y & 1) == 0, else -1, the same integer on every limb.  The definition does not
 * depend on the order of evaluation (one workgroup selects the h-th smallest key by a radix select
 * that regenerates the draws: no workspace).  FHE_EINVAL before any launch: a null context or
 * pointer, h == 0 or h > N. */
int fhe_keygen_secret_sparse(const fhe_ctx* ctx, uint64_t* sk, uint32_t h, uint64_t seed,
                             fhe_stream_t stream);
int fhe_keygen_public(const fhe_ctx* ctx, uint64_t* pk, const uint64_t* sk, uint64_t seed,
                      fhe_stream_t stream);
int fhe_keygen_switch(const fhe_ctx* ctx, uint64_t* key, const uint64_t* sk,
                      const uint64_t* s_from, uint64_t seed, fhe_stream_t stream);
int fhe_encrypt(const fhe_ctx* ctx, uint64_t* ct, const uint64_t* pt, const uint64_t* pk,
                uint64_t seed, void* workspace, fhe_stream_t stream);
int fhe_encrypt_sk(const fhe_ctx* ctx, uint64_t* ct, const uint64_t* pt, const uint64_t* sk,
                   uint64_t seed, fhe_stream_t stream);
int fhe_decrypt(const fhe_ctx* ctx, uint64_t* pt, const uint64_t* ct, const uint64_t* sk,
                uint32_t batch, uint32_t nlimbs, fhe_stream_t stream);

/* ---- batched encryption at any level, from plaintexts or slots --------------------------------
 * Everything in NTT form, canonical residues.  ct [batch][2][level][N], 1 <= level <= L.  For
 * i < batch let j = index0 + i: the poly field of the Philox counter (oracle/pyoracle.py
 * sample(kind, seed, tag, poly = j, ...)).
 *   public key   pk the top-level [2][L][N], read in place at rows l < level.
 *                u, e0, e1 = sample(ternary / error / error, seed, tags 32 / 33 / 34, poly j)
 *                ct[i][0][l] = NTT_l(e0) + pk[0][l] NTT_l(u) + pt_i[l]
 *                ct[i][1][l] = NTT_l(e1) + pk[1][l] NTT_l(u)
 *   secret key   sk [L + K][N], read at rows l < level.
 *                a[l] = sample(uniform, tag 35, poly j, limb l), drawn directly in NTT form
 *                e    = sample(error, tag 36, poly j)
 *                ct[i][1][l] = a[l],   ct[i][0][l] = NTT_l(e) - a[l] s[l] + pt_i[l]
 *   plaintext    pt [pt_batch][pt_rows][N], pt_rows >= level, rows 0 .. level-1 read in place (a
 *                top-level plaintext serves every level, as in fhe_mul_plain_level); pt_batch is 1
 *                (one plaintext for the whole batch) or batch; pt == NULL encrypts zero.
 *   slots        fhe_encrypt_slots is fhe_encode_sparse(slots [batch][2^log_slots][2], delta,
 *                log_slots, level, special = 0) followed by the matching call above, bit for bit
 *                (log_slots = log_n - 1: full packing); secret_key != 0 chooses the secret-key
 *                form and says that `key` is sk, else pk.  The message's coefficients join e0 / e
 *                before the transform: no plaintext is formed.
 * Hence: element 0 of a call with index0 = 0 at level L is fhe_encrypt / fhe_encrypt_sk's result;
 * level l gives rows 0 .. l-1 of the level-L result (small draws are limb-free, uniform draws
 * keyed by the limb's own index); element i of a call with index0 = k is element 0 of a call with
 * index0 = k + i, so one seed serves a stream of batches (SECURITY note above: never repeat a
 * (seed, j) pair under one key).
 * FHE_EINVAL before any launch: a null context, ct or key; null slots (fhe_encrypt_slots); level 0
 * or above L; pt_rows < level with a non-null pt; pt_batch not 1 or batch; index0 + batch > 2^32; a
 * delta that is not finite and positive; log_slots > log_n - 1; ct overlapping pt, slots, the key
 * or the workspace passed; workspace == NULL while the stream is capturing.  batch == 0 is a
 * no-op.  Workspace: fhe_encrypt_workspace(ctx, level, batch) bytes serve all three calls
 * ((4 + level) N words per ciphertext of a pass; a batch runs in passes of at most 256 MiB of
 * ciphertext); with an explicit workspace the calls are capture-safe (nothing is allocated, copied
 * or synchronised).  Restated by tests/encrypt_ref.py. */
size_t fhe_encrypt_workspace(const fhe_ctx* ctx, uint32_t level, uint32_t batch);
int fhe_encrypt_level(const fhe_ctx* ctx, uint64_t* ct, const uint64_t* pt, uint32_t pt_rows,
                      uint32_t pt_batch, const uint64_t* pk, uint32_t level, uint32_t batch,
                      uint64_t seed, uint32_t index0, void* workspace, fhe_stream_t stream);
int fhe_encrypt_sk_level(const fhe_ctx* ctx, uint64_t* ct, const uint64_t* pt, uint32_t pt_rows,
                         uint32_t pt_batch, const uint64_t* sk, uint32_t level, uint32_t batch,
                         uint64_t seed, uint32_t index0, void* workspace, fhe_stream_t stream);
int fhe_encrypt_slots(const fhe_ctx* ctx, uint64_t* ct, const double* slots, double delta,
                      uint32_t log_slots, const uint64_t* key, int secret_key, uint32_t level,
                      uint32_t batch, uint64_t seed, uint32_t index0, void* workspace,
                      fhe_stream_t stream);

/* ---- fused multiply -> relinearise -> rescale ------------------------
 * a, b [batch][2][L][N] NTT form; evk_b, evk_a [dnum][L + K][N] the relinearisation key (NTT
 * form, as for fhe_keyswitch).  out = Relin(a x b) [batch][2][L][N], or with rescale != 0 its
 * divide-and-round by q_{L-1}, [batch][2][L-1][N]; NTT form.  Restated by oracle mul_relin. */
size_t fhe_mul_relin_workspace(const fhe_ctx* ctx, uint32_t batch);
int fhe_mul_relin(const fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b,
                  const uint64_t* evk_b, const uint64_t* evk_a, uint32_t batch, int rescale,
                  void* workspace, fhe_stream_t stream);

/* ---- sum of ciphertext products with one relinearisation (lazy relinearisation) ---------------
 * Everything in NTT form, canonical residues in and out, l = level live Q-limbs:
 *   D_k = sum_{i < count} d_k(a[i]|_l, b[i]|_l) mod q_j   (k = 0, 1, 2),
 *   d   = (a0 b0, a0 b1 + a1 b0, a1 b1),
 *   out = (D_0 + KS0(D_2), D_1 + KS1(D_2)),
 * KS = fhe_keyswitch_level at `level` with the caller's top-level key read in place; with
 * rescale != 0, out then goes through fhe_rescale(nlimbs = level, ntt_form = 1).  One key-switch
 * and one rescale rounding whatever the count.  The canonical result does not depend on the order
 * of the terms; count == 1 with a_levels[0] == b_levels[0] == level is bit-identical to
 * fhe_mul_relin_level.
 * count in 1..16.  a / b and a_levels / b_levels are host arrays of `count` entries: a[i]
 * [batch][2][a_levels[i]][N], b[i] [batch][2][b_levels[i]][N] with level <= each <= L, every term
 * read through its own stride (the level-drop rule of fhe_lincomb_level).  The inputs may alias
 * each other in any way (squares a[i] == b[i], an operand shared by several terms).  out
 * [batch][2][level][N], or [batch][2][level - 1][N] with rescale.
 * Errors (FHE_EINVAL before any launch): K == 0; a null pointer, also inside a / b; count 0 or
 * above 16; level 0 or above L; an input level below `level` or above L; rescale with level < 2;
 * any overlap of out with any input; workspace == NULL while the stream is capturing.  batch == 0
 * is a no-op.
 * Workspace: fhe_mul_relin_workspace(ctx, fhe_keyswitch_pass_batch(ctx, batch)) bytes are
 * sufficient at every level and count (NULL: the internal workspace).  With an explicit workspace
 * the call is capture-safe: the pointers and strides travel in the kernel arguments, nothing is
 * allocated, copied or synchronised.  A large batch runs in passes like fhe_mul_relin. */
int fhe_mul_sum_relin_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* const* a,
                            const uint32_t* a_levels, const uint64_t* const* b,
                            const uint32_t* b_levels, const uint64_t* evk_b, const uint64_t* evk_a,
                            uint32_t level, uint32_t count, uint32_t batch, int rescale,
                            void* workspace, fhe_stream_t stream);

/* ---- plaintext arithmetic over l <= L limbs: scalars, constants, plaintexts, level drop --------
 * The leaves of a polynomial evaluation (CKKS bootstrapping's EvalMod) in one pass each, under the
 * rule of the _level block further up: `level` = l live Q-limbs, 1 <= l <= L, NTT form, canonical
 * residues in and out.
 * fhe_lincomb_level:
 *   out = [rescale]( sum_{i < count} k_i * cts[i]|_l  (+ k_count on every slot of c0) ),
 * count in 1..16.  cts[i] is [batch][2][in_levels[i]][N] with l <= in_levels[i] <= L (cts and
 * in_levels are host arrays); only its limbs 0 .. l-1 are read, through its own stride: dropping
 * RNS limbs IS the level drop, so one term with k = 1 is the strided copy [batch][2][l_in][N] ->
 * [batch][2][l][N], and ciphertexts of different levels add at the lowest one.  `scalars` is a
 * DEVICE table [count + 1][scalar_stride] of canonical residues, row i column j = k_i mod q_j
 * (columns j < l are read; scalar_stride >= l, so one table encoded over all L limbs serves every
 * level, like a key).  Row `count` is the additive constant, read only when has_const != 0: a
 * constant polynomial has the same value at every NTT slot, so it is added to every element of c0
 * and to nothing of c1.  out is [batch][2][l][N]; with rescale != 0 (l >= 2) it is
 * [batch][2][l-1][N], defined as -- and bit-identical to -- the canonical sum followed by
 * fhe_rescale(..., nlimbs = l, ntt_form = 1).
 * fhe_mul_plain_level: out = [rescale]( ct * pt ) for ct [batch][2][l][N] and a plaintext pt
 * [pt_batch][pt_rows][N], NTT form, pt_rows >= l, rows 0 .. l-1 read in place (a top-level [L][N]
 * plaintext or a BSGS diagonal [L + K][N] serves every level; an [l][N] one is accepted too);
 * pt_batch is 1 (one plaintext for the whole batch) or batch.  Bit-identical to fhe_vec_mul on both
 * components followed, with rescale, by fhe_rescale(ntt_form = 1).
 * Errors (FHE_EINVAL before any launch): level == 0 or level > L; in_levels[i] < level or > L;
 * count == 0 or count > 16; scalar_stride < level; pt_rows < level; pt_batch not 1 or batch; a null
 * pointer (also inside cts); rescale with level < 2.
 * Aliasing: without rescale, out may be an input ciphertext itself (same start pointer, and for
 * fhe_lincomb_level in_levels[i] == level); any other overlap of out with an input ciphertext or
 * the plaintext, and any overlap at all with rescale, is FHE_EINVAL.  The scalar table and the
 * workspace must not overlap out (not checked).
 * Workspace: only the rescaling forms take one, fhe_lincomb_workspace(ctx, batch) bytes for both
 * calls, sized for L and sufficient at every level; NULL = internal (FHE_EINVAL while the stream is
 * capturing).  Capture-safe: no scalar travels in the kernel arguments, nothing is allocated or
 * synchronised with an explicit workspace. */
size_t fhe_lincomb_workspace(const fhe_ctx* ctx, uint32_t batch);
int fhe_lincomb_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* const* cts,
                      const uint32_t* in_levels, const uint64_t* scalars, uint32_t scalar_stride,
                      int has_const, uint32_t level, uint32_t count, uint32_t batch, int rescale,
                      void* workspace, fhe_stream_t stream);
int fhe_mul_plain_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* ct, const uint64_t* pt,
                        uint32_t pt_rows, uint32_t pt_batch, uint32_t level, uint32_t batch,
                        int rescale, void* workspace, fhe_stream_t stream);

/* ---- real / imaginary split and merge of the slots (CKKS bootstrapping) -----------------------
 * X^(N/2) multiplies every slot by i: slot j sits at the root exp(i pi 5^j / N) and 5^j = 1 mod 4.
 * In NTT layout it is the constant w_j = psi_j^(N/2) at elements k < N/2 of limb j and q_j - w_j at
 * k >= N/2, so the product is exact and costs no level.  All operands are [batch][2][l][N], NTT
 * form, `level` = l live Q-limbs, canonical residues in and out.
 * fhe_conj_split_level: ct a ciphertext and cc its conjugate (fhe_rotate_level with Galois element
 * 2N - 1);  re = ct + cc,  im = -X^(N/2) (ct - cc):  the slots of re / im are 2 Re z / 2 Im z.
 * fhe_conj_merge_level: out = a + X^(N/2) b  (slots a_j + i b_j).
 * One pass each: two ciphertexts read, two (split) or one (merge) written; the composed forms
 * (fhe_lincomb_level twice and fhe_mul_plain_level by a plaintext of +-w; fhe_mul_plain_level and
 * fhe_lincomb_level) take four and two.
 * FHE_EINVAL before any launch: a null context or pointer; level == 0 or level > L.
 * Aliasing: an output may be an input itself (same start pointer: the operation is elementwise);
 * any other overlap of an output with an input, or of re with im, is FHE_EINVAL.
 * No workspace; capture-safe: nothing is allocated or synchronised. */
int fhe_conj_split_level(const fhe_ctx* ctx, uint64_t* re, uint64_t* im, const uint64_t* ct,
                         const uint64_t* cc, uint32_t level, uint32_t batch, fhe_stream_t stream);
int fhe_conj_merge_level(const fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b,
                         uint32_t level, uint32_t batch, fhe_stream_t stream);

/* ---- ModRaise: from the bottom of the modulus chain back up (CKKS bootstrapping) ------------
 * in is [batch][2][in_level][N], NTT form, canonical residues; only limb 0 of each polynomial is
 * read, through its own stride (a ciphertext at any level is raised without a copy).  out is
 * [batch][2][out_level][N], 1 <= out_level <= L, and for every polynomial p and limb l < out_level
 *   x = INTT_0(in[p][0])                        coefficient form, 0 <= x < q_0
 *   c = x if x <= (q_0 - 1) / 2, else x - q_0   the centred representative
 *   out[p][l] = NTT_l(c mod q_l)                canonical residues
 * so out[p][0] equals in[p][0] bit for bit, and the raised ciphertext decrypts to m + q_0 I for a
 * small integer polynomial I (|I| <= (||s||_1 + 2) / 2), which EvalMod (fhecore.polyeval.eval_mod)
 * removes.  q_l may be smaller or larger than q_0 and of another bit size.
 * FHE_EINVAL before any launch: a null context or pointer; in_level or out_level of 0 or above L;
 * any overlap of out with in; workspace == NULL while the stream is capturing.  batch == 0 is a
 * no-op.  Workspace: fhe_mod_raise_workspace(ctx, batch) bytes (2 batch N words); NULL = internal.
 * Capture-safe with an explicit workspace: nothing is allocated or synchronised. */
size_t fhe_mod_raise_workspace(const fhe_ctx* ctx, uint32_t batch);
int fhe_mod_raise(const fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t in_level,
                  uint32_t out_level, uint32_t batch, void* workspace, fhe_stream_t stream);

/* ---- CKKS encode / decode on the device ------------------------------------------------------
 * The canonical embedding over the rotation group (slot j at the root exp(i pi 5^j / N), as
 * fhecore.ckks.Encoder) by the HEAAN / Lattigo special FFT in float64.  n = N/2, M = 2N,
 * rot[j] = 5^j mod M, W[k] = (cos, sin)(pi k / N) computed as M_PI * (double)k / (double)N, every
 * entry straight from libm (fhe_encode_roots returns the table the context uploads; it needs no
 * device).  A complex product (dr, di)(wr, wi) is the four rounded products dr wr, di wi, dr wi,
 * di wr and the two rounded sums p1 - p2, p3 + p4: no fused multiply-add, no reassociation.
 * tests/encode_ref.py restates both directions; the results equal it bit for bit.
 *
 * fhe_encode: slots is device memory [count][N/2][2] doubles, interleaved (re, im).
 *   v = z;  for len = n, n/2 .. 2 (lh = len/2, lq = 4 len), every block start i, j < lh:
 *       w = W[(lq - rot[j] % lq) (M/lq)];  (v[i+j], v[i+j+lh]) = (a + b, (a - b) w)
 *   v = v[bitrev_n];  s = delta / n;  c[k] = rint(Re v[k] s),  c[k + n] = rint(Im v[k] s)
 *   (ties to even), and row r of out [count][level (+ K)][N] is NTT(c mod q_limb(r)), canonical
 *   residues; the rows are the Q-limbs 0 .. level-1, then with special != 0 the P-limbs.
 *   level = L with special is the [L + K][N] diagonal fhe_linear_transform / rotate_sum_hoisted
 *   read in place at every level; special == 0 is the [level][N] plaintext of fhe_mul_plain_level
 *   and fhe_encrypt.  Precondition (not checked): |c| < 2^62; for NaN, infinite or larger values
 *   the residues are unspecified but canonical, and nothing faults.
 * fhe_decode: pt is [count][pt_rows][N], NTT form; limb 0 is read, and limb 1 when level >= 2,
 *   through the row stride pt_rows.  x_i = INTT_i(limb i); level 1: V = x_0 centred over q_0;
 *   level >= 2: t = ((x_1 - x_0) q_0^-1) mod q_1, V = x_0 + q_0 t centred over q_0 q_1;
 *   x = (double)V with one round-to-nearest-even;  v[k] = (x[k], x[k + n]);  v = v[bitrev_n];
 *   for len = 2, 4 .. n:  w = W[(rot[j] % lq) (M/lq)];  b = v[i+j+lh] w;
 *       (v[i+j], v[i+j+lh]) = (a + b, a - b);   slots = v / delta (IEEE division).
 *   Precondition: the plaintext's true centred value is below q_0 q_1 / 2 (q_0 / 2 at level 1)
 *   in magnitude, which holds for every plaintext whose scaled message fits two primes.
 * FHE_EINVAL before any launch: a delta that is not finite and positive; a null context or
 * pointer; level 0 or above L; special on a context with K = 0; pt_rows < min(level, 2); any
 * overlap of out with slots (of slots with pt); workspace == NULL while the stream is capturing.
 * count == 0 is a no-op.  Workspace: fhe_encode_workspace / fhe_decode_workspace(ctx, count) bytes
 * (2 / 3 count N words); NULL = internal.  Capture-safe with an explicit workspace: nothing is
 * allocated or synchronised.  FHECORE_ENCODE_UNFUSED=1 makes fhe_encode take the form of contexts
 * with a modulus >= 2^61 (a separate lift, then whole NTTs) on any context: the same bits. */
int fhe_encode_roots(uint32_t log_n, double* out /* [2N][2] = (cos, sin)(pi k / N) */);
size_t fhe_encode_workspace(const fhe_ctx* ctx, uint32_t count);
int fhe_encode(const fhe_ctx* ctx, uint64_t* out, const double* slots, double delta,
               uint32_t level, int special, uint32_t count, void* workspace, fhe_stream_t stream);
size_t fhe_decode_workspace(const fhe_ctx* ctx, uint32_t count);
int fhe_decode(const fhe_ctx* ctx, double* slots, const uint64_t* pt, double delta,
               uint32_t pt_rows, uint32_t level, uint32_t count, void* workspace,
               fhe_stream_t stream);

/* ---- Sparse packing: n_s = 2^log_slots slots, 0 <= log_slots <= log_n - 1 --------------------
 * With gap = N / (2 n_s) and Y = X^gap the message lives in the subring Z[Y]/(Y^(2 n_s) + 1): a
 * sparse plaintext is an ordinary plaintext whose slot vector is n_s-periodic, and every other
 * call (encrypt, rotate, multiply, the linear transform) takes it as it is.  The subring's tables
 * are slices of the context's own: W_s[k] = W[k gap], 5^j mod 4 n_s = rot[j] mod 4 n_s.
 *
 * fhe_encode_sparse: slots is [count][n_s][2] doubles; out is fhe_encode's [count][level (+ K)][N].
 *   v = z;  for len = n_s, n_s/2 .. 2 (lh = len/2, lq = 4 len):
 *       w = W[(lq - rot[j] % lq) (M/lq)];  (a, b) -> (a + b, (a - b) w)       (M = 2N, as above)
 *   v = v[bitrev over log_slots bits];  s = delta / n_s;
 *   c[k gap] = rint(Re v[k] s),  c[(k + n_s) gap] = rint(Im v[k] s),  every other coefficient 0;
 *   the rows are fhe_encode's.  The result equals fhe_encode of the vector tiled gap times bit for
 *   bit: the first log2(gap) stages of the tiled transform only double, and delta / n against
 *   delta / n_s is a power of two.
 * fhe_decode_sparse: INTT and centring as fhe_decode, of the coefficients k gap only (the
 *   projection onto the subring: what a ciphertext's noise leaves between them is not read);
 *   x'[k] = x[k gap], k < 2 n_s;  v[k] = (x'[k], x'[k + n_s]);  v = v[bitrev];  the stages
 *   len = 2 .. n_s with w = W[(rot[j] % lq) (M/lq)];  slots [count][n_s][2] = v / delta.
 * log_slots = log_n - 1 is fhe_encode / fhe_decode (the same launches); log_slots = 0 is one slot
 * with no stage, c[0] and c[N/2].  Every refusal of the full calls carries over, the overlap
 * checks with the sparse slot extent; log_slots > log_n - 1 is FHE_EINVAL before any launch.
 * Workspace: fhe_encode_workspace / fhe_decode_workspace(ctx, count) bytes; capture-safe with an
 * explicit one.  FHECORE_ENCODE_UNFUSED=1 is honoured. */
int fhe_encode_sparse(const fhe_ctx* ctx, uint64_t* out, const double* slots, double delta,
                      uint32_t log_slots, uint32_t level, int special, uint32_t count,
                      void* workspace, fhe_stream_t stream);
int fhe_decode_sparse(const fhe_ctx* ctx, double* slots, const uint64_t* pt, double delta,
                      uint32_t log_slots, uint32_t pt_rows, uint32_t level, uint32_t count,
                      void* workspace, fhe_stream_t stream);

/* ---- Decrypt straight to slots: fhe_encrypt_slots' way back -------------------------------------
 * ct [batch][2][level][N], NTT form, canonical residues, 1 <= level <= L; sk [L + K][N], of which
 * only the rows l < min(level, 2) are read; slots [batch][2^log_slots][2] doubles,
 * 0 <= log_slots <= log_n - 1 (log_n - 1: full packing).  The result is, bit for bit, that of
 *   fhe_decrypt(pt, ct, sk, batch, level)   ("sampling, keys, encryption" above), then
 *   fhe_decode_sparse(slots, pt, delta, log_slots, pt_rows = level, level, batch)
 * ("Sparse packing" above; with log_slots = log_n - 1 that is fhe_decode): nothing new is defined.
 * Only limb 0 of both components is read, and limb 1 when level >= 2, through the ciphertext's own
 * strides; no [level][N] plaintext is formed (c0 + c1 s is computed by the inverse transform's
 * first pass as it loads).
 * FHE_EINVAL before any launch: a null context, slots, ct or sk; level 0 or above L;
 * log_slots > log_n - 1; a delta that is not finite and positive; slots overlapping ct, sk (its
 * first two rows) or the workspace passed; workspace == NULL while the stream is capturing.
 * batch == 0 is a no-op.  Workspace: fhe_decode_workspace(ctx, batch) bytes; NULL = internal.
 * Capture-safe with an explicit workspace: nothing is allocated, copied or synchronised.
 * FHECORE_DECRYPT_UNFUSED=1 makes the call take the form of contexts with a modulus >= 2^61 (the
 * product written out over the limbs read, then the whole inverse transform) on any context: the
 * same bits. */
int fhe_decrypt_slots(const fhe_ctx* ctx, double* slots, const uint64_t* ct, const uint64_t* sk,
                      double delta, uint32_t log_slots, uint32_t level, uint32_t batch,
                      void* workspace, fhe_stream_t stream);

/* ---- HIP graphs: capture a sequence of libfhecore calls on `stream` and replay it -----------
 * Between fhe_graph_begin and fhe_graph_end every call that takes a workspace must be given an
 * explicit one: with workspace == NULL a call returns FHE_EINVAL while the stream is capturing
 * (the context's internal workspace may be reallocated later, which would leave the graph
 * pointing at freed memory).  Replays reuse the captured pointers, so every buffer a captured
 * call touches must outlive the graph. */
typedef struct fhe_graph_s* fhe_graph_t;
int fhe_graph_begin(fhe_stream_t stream);
int fhe_graph_end(fhe_stream_t stream, fhe_graph_t* graph);
int fhe_graph_launch(fhe_graph_t graph, fhe_stream_t stream);
int fhe_graph_destroy(fhe_graph_t graph);

/* ---- timing marks (measurement support, not part of the reference surface) ------------------
 * fhe_prof_begin records a HIP event on `stream`, then every kernel this host thread launches
 * through libfhecore records one more event after itself (up to max_marks).  fhe_prof_end waits
 * for the last event and returns the per-launch elapsed times (ms) and the kernel names,
 * newline-separated, in launch order. */
int fhe_prof_begin(uint32_t max_marks, fhe_stream_t stream);
int fhe_prof_end(float* elapsed_ms, uint32_t cap, uint32_t* count, char* names, size_t names_cap);

#ifdef __cplusplus
}
#endif

#endif /* FHECORE_H */
