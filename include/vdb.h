/*
 * vdb.h — C ABI of the MI355X-native proving hot path for halo2-vectordb circuits.
 *
 * This is the drop-in boundary.  The reference (Rust) has no FFI of its own: the seam
 * is the set of upstream Rust functions its prover reaches through
 *   /root/reference/src/scaffold/mod.rs:296  gen_snark_shplonk -> create_proof   (MSM, NTT)
 *   /root/reference/src/scaffold/mod.rs:273  create_pk                            (MSM, NTT, keygen)
 *   /root/reference/src/scaffold/mod.rs:378-396  closure + RangeCircuitBuilder::prover (witness, layout)
 * A patched halo2-axiom / halo2-base (Cargo `[patch]`) forwards those calls here; INTEGRATION.md shows
 * the Rust `extern "C"` stubs.  Each entry point below names the interface it replaces.
 *
 * Conventions
 *  - vdb_fr  : BN254 scalar, 4 x u64 little-endian limbs, MONTGOMERY form (R = 2^256) — the in-memory
 *              layout of halo2curves::bn256::Fr, so `&[Fr]` crosses zero-copy.
 *  - vdb_g1  : affine point {x, y}, each a Montgomery Fq; identity = (0, 0) as halo2curves.
 *  - Every function returns 0 on success or a negative VDB_ERR_*; nothing aborts or throws across
 *    the ABI.  vdb_last_error() returns a thread-local message for the last failure.
 *  - Host pointers unless the name ends in _dev (then: device pointers in HBM of the bound GPU).
 *  - A process binds one GPU (vdb_init(device): one process per GPU) or several (vdb_init_devices(n): one context per
 *    device, the calling thread's device chosen with vdb_set_device).  Calls are not re-entrant per device context,
 *    matching the reference's single prover thread.  Entry points with host outputs block until the result is there;
 *    _dev entry points only queue work on the library's stream (in order), and the vdb_msm_batch_*_begin /
 *    vdb_msm_batch_end pair is explicitly asynchronous (see there).  vdb_sync() waits for everything queued.
 */
#ifndef VDB_H
#define VDB_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } vdb_fr;
typedef struct { uint64_t l[4]; } vdb_fq;
typedef struct { vdb_fq x, y; } vdb_g1;
/* G2 point on the twist y^2 = x^3 + 3 / (9 + u) over Fq2 = Fq[u] / (u^2 + 1), affine: x = x[0] + x[1] u, y = y[0] + y[1] u, each
 * coordinate a Montgomery Fq like vdb_g1's (so a halo2curves G2Affine {x: Fq2 {c0, c1}, y: Fq2 {c0, c1}} crosses as is); the
 * identity is all zero. */
typedef struct { vdb_fq x[2], y[2]; } vdb_g2;
typedef struct vdb_srs vdb_srs;

enum {
  VDB_OK = 0,
  VDB_ERR_NOT_INIT = -1,
  VDB_ERR_HIP = -2,       /* HIP runtime failure (message has the hipError string) */
  VDB_ERR_ARG = -3,       /* bad argument (size mismatch, null pointer, unsupported parameter) */
  VDB_ERR_OOM = -4,
  VDB_ERR_DOMAIN = -5,    /* data-dependent failure the reference turns into a panic (div by zero, K >= N) */
  VDB_ERR_NO_DEVICE = -6
};

/* ---- b0 lifecycle -------------------------------------------------------------------------- */
/* Binds this process to HIP device `device` and creates streams/workspaces (whatever was bound before is released).
 * Fails loudly with VDB_ERR_NO_DEVICE when no GPU is visible: there is NO CPU fallback in this library. */
int vdb_init(int device);
/* binds devices 0 .. n_devices-1 in ONE process, each with its own context (streams, workspaces, twiddle and
 * gadget tables).  A host thread works on the device it selected with vdb_set_device (thread-local; device 0 until then);
 * device pointers, vdb_srs handles and deferred MSMs belong to the device they were created on.  The path shards by
 * column with no exchange between devices: the *_multi entry points below cut a batch of columns into one
 * block per device and return every device's results D2H; no RCCL communicator is needed for that.  The other supported
 * arrangement is one process per GPU (vdb_init(local_rank), torch.distributed / RCCL all_gather of the commitments:
 * bench.py). */
int vdb_init_devices(int n_devices);
int vdb_devices_bound(void);      /* number of bound devices */
int vdb_set_device(int device);   /* the calling thread works on this (bound) device from now on */
int vdb_current_device(void);     /* -1 when nothing is bound */
void vdb_shutdown(void);          /* releases every bound device */
const char *vdb_last_error(void);
int vdb_device_count(void);
const char *vdb_version(void);

/* device memory helpers for HBM-resident pipelines */
int vdb_malloc(void **dptr, size_t bytes);
int vdb_free(void *dptr);
int vdb_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int vdb_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
/* Frees the library's cached work buffers (MSM buckets and sort records — up to half of the free HBM —, NTT staging); they
 * are re-created on demand.  For callers that need the memory between two phases.  Waits for queued work. */
int vdb_scratch_release(void);
/* Bytes the cached work buffers hold at the moment (what vdb_scratch_release would give back). */
int vdb_scratch_held(size_t *bytes);
/* Wall time, bytes and number of the device allocations this process made through the library (vdb_malloc, the work buffers, keygen's
 * sort records) since start or the last reset: what a setup / keygen time consists of when HBM has to be mapped or cleared first. */
int vdb_alloc_stats(double *seconds, uint64_t *bytes, uint64_t *calls, int reset);
/* Upper bound for the MSM's work space from now on (0 = the default: half of the free HBM, between 8 and 96 GiB — one batch for
 * the whole k = 16 job).  A keygen that commits the fixed columns while the card is still empty sets a bound first: mapping 96 GiB
 * of fresh HBM for a two-second MSM and handing it back costs more than the MSM (keygen). */
int vdb_msm_set_scratch_cap(size_t bytes);
int vdb_mem_info(size_t *free_bytes, size_t *total_bytes); /* HBM of the calling thread's device (hipMemGetInfo) */
int vdb_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes); /* asynchronous on the library stream */
int vdb_memset_dev(void *dst_dev, int value, size_t bytes);
int vdb_sync(void);
/* HIP-event timing on the library's own stream (bench.py: torch.cuda.Event does not see it) */
int vdb_timer_start(void);
int vdb_timer_stop(float *ms_out);
/* per-kernel HIP-event timing: between begin and end every kernel launch of the library is bracketed by
 * events on its stream (serialising them); end returns {"kernel": {"ms": total, "launches": n}, ...} */
int vdb_profile_begin(void);
/* the same without serialising: events are recorded on the stream each launch goes to and read in vdb_profile_end, so
 * the kernels run (and overlap) exactly as they do untimed — what bench.py uses inside its timed region */
int vdb_profile_begin_deferred(void);
int vdb_profile_end(char *json_out, size_t cap);

/* ---- field helpers (tests / staging) -------------------------------------------------------- */
/* acc <- acc x + values[i], i = 0 .. n - 1, on the host (Montgomery in and out; needs no GPU): combining the evaluations of a
 * multi-open with powers of a challenge (halo2 poly/kzg/multiopen) */
int vdb_fr_horner(const vdb_fr *values, size_t n, const vdb_fr *x, vdb_fr *acc);
/* out[i] = (64 little-endian bytes wide[64 i ..]) mod r, Montgomery: Fr::random / Fr::from_u512 of halo2curves — how the
 * prover's blinding scalars are drawn from OS entropy (halo2 create_proof: Blind(Scalar::random(rng)), reached from
 * src/scaffold/mod.rs:296).  Device pointers; asynchronous on the library stream. */
int vdb_fr_from_wide_dev(const uint8_t *wide_dev, size_t n, vdb_fr *out_dev);
int vdb_fr_from_canonical(const vdb_fr *in, vdb_fr *out, size_t n);
int vdb_fr_to_canonical(const vdb_fr *in, vdb_fr *out, size_t n);
int vdb_fr_mul(const vdb_fr *a, const vdb_fr *b, vdb_fr *out, size_t n);
int vdb_fr_add(const vdb_fr *a, const vdb_fr *b, vdb_fr *out, size_t n);
int vdb_fr_sub(const vdb_fr *a, const vdb_fr *b, vdb_fr *out, size_t n);
/* replaces halo2 `BatchInvert` over `Assigned::Rational` denominators (poly::batch_invert_assigned);
 * 0 maps to 0 */
int vdb_fr_batch_invert(const vdb_fr *in, vdb_fr *out, size_t n);
/* micro-benchmark: `iters` dependent Montgomery multiplications in each of `threads` GPU threads;
 * reports Fr multiplications per second (kernel time only) */
int vdb_bench_fr_mul(size_t threads, size_t iters, double *mul_per_sec);

/* ---- a2/a3/a18 fixed-point staging: replaces FixedPointChip::{quantization, dequantization} and
 *      FixedPointVectorInstructions::{quantize_vector, dequantize_vector}
 *      (src/gadget/fixed_point.rs:104-136, src/gadget/fixed_point_vec.rs:29-51).  Host side, exact. ---- */
int vdb_fp_quantize(uint32_t precision_bits, const double *x, vdb_fr *out, size_t n);
int vdb_fp_dequantize(uint32_t precision_bits, const vdb_fr *x, double *out, size_t n);

/* ---- b5 witness streams.  Each call emits exactly the cells the Rust gadget pushes into
 *      halo2-base `Context.advice` (stream_out) and `cells_to_lookup` (lookup_out), in order, for
 *      already-assigned quantized inputs; sizes come from the matching *_size call.
 *      metric: 0 euclidean, 1 cosine, 2 manhattan, 3 hamming (DistanceChip, src/gadget/distance.rs:97-195; hamming = one minus the
 *      share of equal elements, its two load_witness cells unconstrained as in the reference, :165-169).
 *      selector_out (optional, 1 flag byte per advice cell): bit 0 marks gate starts — the keygen-side information
 *      from which vdb_layout_plan derives the break points that the reference pins in configs/<name>.json
 *      (src/scaffold/mod.rs:272, 285-287); bit 1 marks cells that hold a data-independent QuantumCell::Constant
 *      of the gate templates (used by vdb_msm_batch_masked_dev).  VDB_ERR_DOMAIN replaces the reference's panics. ---------- */
int vdb_wit_distance_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t n_pairs, size_t dim, uint64_t *cells, uint64_t *lookups);
/* DistanceChip::{euclidean,cosine,manhattan,hamming}_distance for n_pairs independent (a_i, b_i) */
int vdb_wit_distance(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *a, const vdb_fr *b, size_t n_pairs, size_t dim,
                     vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out, vdb_fr *result_out);
/* the same with inputs and outputs resident in HBM (the distances circuit of examples/distances.rs / examples/euclid.rs inside the hot
 * path: pipeline.DistancesHotPath); honours vdb_wit_set_window */
int vdb_wit_distance_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *a_dev, const vdb_fr *b_dev, size_t n_pairs, size_t dim,
                         vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, vdb_fr *result_dev);
/* FixedPointInstructions, one call per instance (src/gadget/fixed_point.rs:213-460 — what the chips above are composed of, for circuits
 * that apply an operation to many values): n independent calls op(a_i [, b_i]); instance i's cells are cells/n consecutive cells of the
 * stream (its lookup cells likewise), in the order the gadget pushes them.  op: 0 qadd, 1 qsub, 2 qmul, 3 qdiv, 4 neg, 5 qabs, 6 is_neg,
 * 7 qmin, 8 qsqrt, 9 qlog2, 10 qexp2, 11 qlog, 12 qexp, 13 qpow, 14 bit_xor, 15 cond_neg (b: the flag), 16 signed_div_scale (result:
 * the quotient), 17 qmax, 18 sign (the field elements 1 / -1), 19 clip, 20 qmod (b positive), 21 qsin, 22 qcos, 23 qtan, 24 qsinh,
 * 25 qcosh, 26 qtanh.  b may be null for the unary ones.  VDB_ERR_DOMAIN where the reference panics (a division by zero).  The _dev
 * form honours vdb_wit_set_window. */
int vdb_wit_fp_op_size(int op, uint32_t precision_bits, uint32_t lookup_bits, size_t n, uint64_t *cells, uint64_t *lookups);
int vdb_wit_fp_op(int op, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *a, const vdb_fr *b, size_t n, vdb_fr *stream_out,
                  vdb_fr *lookup_out, uint8_t *selector_out, vdb_fr *result_out);
int vdb_wit_fp_op_dev(int op, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *a_dev, const vdb_fr *b_dev, size_t n, vdb_fr *stream_dev,
                      vdb_fr *lookup_dev, uint8_t *selector_dev, vdb_fr *result_dev);
/* VectorDBChip::nearest_vector (src/gadget/vectordb.rs:122-163): indicator_out n raw 0/1 field bits.  vdb_wit_nearest_batch with one
 * query, and so within its limits of one call: n and dim at most 2^24, the cells at most 2^34.  No call that could run is refused by
 * them: 2^34 cells are 512 GiB of stream, more than the card holds. */
int vdb_wit_nearest_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t n, size_t dim, uint64_t *cells, uint64_t *lookups);
int vdb_wit_nearest(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *query, const vdb_fr *vectors, size_t n, size_t dim,
                    vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out, vdb_fr *indicator_out, vdb_fr *result_out);
/* the same on device-resident buffers (query_dev: dim, vectors_dev: n x dim; outputs stay in HBM); honours vdb_wit_set_window:
 * a rank stores the cells of its own columns, every rank computes every value (the n distances, the short minimum chain) */
int vdb_wit_nearest_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *query_dev, const vdb_fr *vectors_dev, size_t n, size_t dim,
                        vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, vdb_fr *indicator_dev, vdb_fr *result_dev);
/* nearest_vector for a batch of queries over ONE database (src/gadget/vectordb.rs:122-163 called once per query, query after query, as a
 * closure over the reference's chips would): the stream holds n_queries blocks of vdb_wit_nearest's cells end to end, the lookup stream
 * their lookup runs in query order; queries n_queries x dim, indicators_out n_queries x n raw 0/1 bits, results_out n_queries x dim.
 * Bit-identical to n_queries calls of vdb_wit_nearest at the matching offsets, with a number of kernel launches that does not depend on
 * n_queries.  The _dev form honours vdb_wit_set_window like vdb_wit_nearest_dev.
 * Limits of one call (VDB_ERR_ARG beyond them, as for n_queries == 0): n_queries * n and n_queries * dim at most
 * VDB_NEAREST_BATCH_MAX_INSTANCES (32-bit instance numbers; 164 B of work space per (query, vector)), n_queries * cells of one
 * nearest_vector at most VDB_NEAREST_BATCH_MAX_CELLS: vdb_wit_nearest_topk's limits at topk == 1, which refuse exactly these calls (the
 * constants are the TOPK ones).  The deferred-inversion list holds 16 M entries whatever the batch: beyond them
 * inverse cells are computed in line — slower, the same stream.  VDB_ERR_OOM when the work space cannot be allocated. */
#define VDB_NEAREST_BATCH_MAX_INSTANCES ((size_t)1 << 24)
#define VDB_NEAREST_BATCH_MAX_CELLS ((uint64_t)1 << 34)
int vdb_wit_nearest_batch_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t n_queries, size_t n, size_t dim, uint64_t *cells,
                               uint64_t *lookups);
int vdb_wit_nearest_batch(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *queries, const vdb_fr *vectors, size_t n_queries,
                          size_t n, size_t dim, vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out, vdb_fr *indicators_out,
                          vdb_fr *results_out);
int vdb_wit_nearest_batch_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *queries_dev, const vdb_fr *vectors_dev,
                              size_t n_queries, size_t n, size_t dim, vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev,
                              vdb_fr *indicators_dev, vdb_fr *results_dev);
/* The topk nearest vectors of every query over ONE database (top-k query).  The reference has no such gadget; the cells are those of the
 * closure a user of its chips writes.  Per query, in query order: the n distance blocks of vdb_wit_nearest, then for round
 * r = 0 .. topk - 1 over the entries cur (cur = the distances for r = 0):
 *   min_r   = qmin folded over cur_0 .. cur_{n-1}                (n - 1 qmin blocks, with their lookup cells)
 *   ind_r,i = gate.is_equal(min_r, cur_i)                        (12 cells each)
 *   res_r,j = gate.select_by_indicator(v_.,j, ind_r,.)           (1 + 3 n cells each)
 *   cur_i   = gate.select(Constant(M), cur_i, ind_r,i)           (8 cells each; not emitted after the last round)
 * with M = 2^(2 precision_bits) - 1, the largest value of the chip's range.  Lookup stream: per query the n distance runs, then per round
 * the n - 1 qmin runs.  indicators_out n_queries x topk x n raw 0/1 bits, results_out n_queries x topk x dim, nearest first.
 * topk == 1 is vdb_wit_nearest_batch, which forwards here.  Ties behave as in nearest_vector: every entry that equals the round's minimum gets
 * its indicator set, the round's result is the LAST of them, and all of them are masked in that round; once fewer distinct distances than
 * rounds remain, a round runs on an all-M array, sets every indicator and returns the last vector.
 * The number of kernel launches depends on neither n_queries nor topk.  The _dev form honours vdb_wit_set_window like
 * vdb_wit_nearest_batch_dev.  Work space: 32 B per (query, round, vector) for the round's prefix minima, and per (query, vector) 128 B
 * for the distances plus 4 B for the round that masked the entry: 164 B per (query, vector) at topk == 1.
 * Limits of one call (VDB_ERR_ARG beyond them, as for topk == 0, topk > n and n_queries == 0, before anything is launched):
 * n_queries * topk * n and n_queries * topk * dim at most VDB_NEAREST_TOPK_MAX_INSTANCES (32-bit lane numbers), all cells at most
 * VDB_NEAREST_TOPK_MAX_CELLS.  VDB_ERR_OOM when the work space cannot be allocated. */
#define VDB_NEAREST_TOPK_MAX_INSTANCES ((size_t)1 << 24)
#define VDB_NEAREST_TOPK_MAX_CELLS ((uint64_t)1 << 34)
int vdb_wit_nearest_topk_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t n_queries, size_t n, size_t dim, size_t topk,
                              uint64_t *cells, uint64_t *lookups);
int vdb_wit_nearest_topk(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *queries, const vdb_fr *vectors, size_t n_queries,
                         size_t n, size_t dim, size_t topk, vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out, vdb_fr *indicators_out,
                         vdb_fr *results_out);
int vdb_wit_nearest_topk_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *queries_dev, const vdb_fr *vectors_dev,
                             size_t n_queries, size_t n, size_t dim, size_t topk, vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev,
                             vdb_fr *indicators_dev, vdb_fr *results_dev);
/* nearest_vector's answer as VALUES alone: for every query q the minimum over i of the circuit's fixed-point
 * distance(vector_i, query_q) (src/gadget/vectordb.rs:138's argument order), bit for bit what vdb_wit_nearest_batch's qmin chain ends
 * in, and the LAST i at that minimum, the index of nearest_vector's last set indicator.  No stream is written or attached: the distance
 * generators run on their value-only path (those of a rank whose window holds no cell), then one wavefront per query takes the
 * minimum in qmin's order, the signed fixed-point one.  Routing for a circuit that proves the choice (which cluster a written vector
 * belongs to) has to use this arithmetic: a near-tie that f64 resolves differently is a different answer.
 * idx_out n_queries x uint32; dist_out n_queries values, may be NULL.  The number of kernel launches depends on neither n_queries nor
 * n.  Work space: 128 B per (query, vector).  vdb_wit_set_window does not apply.  VDB_ERR_ARG before anything is launched: n_queries,
 * n or dim == 0, and vdb_wit_nearest_topk's limits at topk == 1; VDB_ERR_DOMAIN as for the witness call (cosine of a zero vector). */
int vdb_nearest_values_dev(uint32_t precision_bits, uint32_t lookup_bits, int metric, const vdb_fr *queries_dev, const vdb_fr *vectors_dev,
                           size_t n_queries, size_t n, size_t dim, uint32_t *idx_out_dev, vdb_fr *dist_out_dev);
int vdb_nearest_values(uint32_t precision_bits, uint32_t lookup_bits, int metric, const vdb_fr *queries, const vdb_fr *vectors, size_t n_queries,
                       size_t n, size_t dim, uint32_t *idx_out, vdb_fr *dist_out);
/* VectorDBChip::kmeans::<K, I> (src/gadget/vectordb.rs:225-362): centroids K x dim, indicators n x K
 * (quantized 1.0 / 0).  zero_cached: Context::load_zero already called earlier in this context. */
int vdb_wit_kmeans_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t n, size_t dim, size_t K, size_t I, int zero_cached,
                        uint64_t *cells, uint64_t *lookups);
int vdb_wit_kmeans(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *vectors, size_t n, size_t dim, size_t K, size_t I,
                   int zero_cached, vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out, vdb_fr *centroids_out, vdb_fr *indicators_out);
/* Multi-GPU: restricts what the following *_dev witness calls STORE to the advice cells [adv_lo, adv_hi) and lookup
 * cells [lookup_lo, lookup_hi) (coordinates of the stream / lookup pointers passed to the call): a rank that commits a
 * block of columns only needs those cells; all values (distances, centroids, ...) are still computed everywhere.
 * Pass (0, UINT64_MAX, 0, UINT64_MAX) to restore the full range. */
int vdb_wit_set_window(uint64_t adv_lo, uint64_t adv_hi, uint64_t lookup_lo, uint64_t lookup_hi);
int vdb_wit_kmeans_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *vectors_dev, size_t n, size_t dim, size_t K, size_t I,
                       int zero_cached, vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, vdb_fr *centroids_dev, vdb_fr *indicators_dev);
/* VectorDBChip::merkle_commitment with PoseidonChip<F,3,2>(R_F=8, R_P=57) (src/gadget/vectordb.rs:165-223):
 * the permutation trace cells; no lookups.  n at most 2^30 (a tree of at most 30 levels), like vdb_merkle_tree_build_dev:
 * VDB_ERR_ARG above */
int vdb_wit_merkle_size(size_t n, size_t dim, int zero_cached, uint64_t *cells);
int vdb_wit_merkle(const vdb_fr *vectors, size_t n, size_t dim, int zero_cached, vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *root_out);
int vdb_wit_merkle_dev(const vdb_fr *vectors_dev, size_t n, size_t dim, int zero_cached, vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *root_dev);
/* The tree of merkle_commitment (src/gadget/vectordb.rs:165-223) kept on the device, values only: levels_dev receives the digests of every
 * level one after the other — the lp = next_power_of_two(n) leaf digests (the padding leaves 0), then lp / 2 nodes, ..., the root at
 * entry 2 lp - 2; 2 lp entries are written (the last is 0).  A service keeps this buffer between batches of updates and never rehashes
 * the database. */
int vdb_merkle_tree_build_dev(const vdb_fr *vectors_dev, size_t n, size_t dim, vdb_fr *levels_dev);
/* Inserts and replacements proved against the committed root: a batch of m Merkle path updates (indices[j], new vector j), applied in
 * order.  The reference has no such gadget; the cells are those of the closure a user of its chips writes.  depth = log2(lp) >= 1.
 * Stream, from cell 0: the assigned witnesses — the m new vectors (m x dim), m old leaves, per update the depth index bits (least
 * significant first), per update the depth siblings (leaf level first): input_cells of them — then per update j
 *   new_leaf = poseidon.clear(); update(new_vector_j); squeeze()               (the leaf hash of merkle_commitment)
 *   per level l: gate.assert_bit(b_l); lo = select(sib_l, cur_old, b_l); ro = select(cur_old, sib_l, b_l); cur_old = H(lo, ro);
 *                ln = select(sib_l, cur_new, b_l); rn = select(cur_new, sib_l, b_l); cur_new = H(ln, rn)      (9,048 cells a level)
 *   idx = gate.inner_product(bits, Constant(2^l))                              (1 + 3 (depth - 1) cells)
 * with H the node hash of merkle_commitment.  The circuit ties cur_old at the top of update j to cur_new at the top of update j - 1
 * (a copy constraint, no cells).  public 3 m + 2 values: [old root | idx_j, old_leaf_j, new_leaf_j per update | new root].
 * An insert is an update of a padding slot (old leaf 0).  Updates of one batch see each other (repeated slots, sibling slots); the
 * result is that of applying them one after the other.  levels (vdb_merkle_tree_build_dev's layout) is read and left in the state
 * after the batch.  indices is a HOST array in both forms (it is checked before anything is launched).
 * The number of kernel launches depends on depth, not on m.  The _dev form honours vdb_wit_set_window like vdb_wit_merkle_dev.
 * Work space: 32 B x m x (3 (dim / 2 + 1) + 4 depth + 3) plus 5 B per (update, level).
 * Limits of one call (VDB_ERR_ARG beyond them, as for m == 0, depth == 0 (n == 1) and an index >= lp, before anything is launched):
 * m at most VDB_MERKLE_UPDATE_MAX_UPDATES (the batch's indices are scanned in LDS), depth at most 30, all cells at most
 * VDB_MERKLE_UPDATE_MAX_CELLS.  These three calls are the vdb_wit_merkle_update_ops calls below with every update a write and the
 * tree not grown (kinds == NULL, grow == 0): one kernel family.  A read is vdb_wit_merkle_open. */
#define VDB_MERKLE_UPDATE_MAX_UPDATES ((size_t)4096)
#define VDB_MERKLE_UPDATE_MAX_CELLS ((uint64_t)1 << 34)
int vdb_wit_merkle_update_size(size_t n, size_t dim, size_t m, uint64_t *cells, uint64_t *input_cells);
int vdb_wit_merkle_update(vdb_fr *levels, size_t n, size_t dim, const vdb_fr *new_vectors, const uint64_t *indices, size_t m, vdb_fr *stream_out,
                          uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_merkle_update_dev(vdb_fr *levels_dev, size_t n, size_t dim, const vdb_fr *new_vectors_dev, const uint64_t *indices, size_t m,
                              vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *public_dev);
/* Growing the resident tree: the tree `levels_dev` over n vectors (lp padded leaves, depth d) laid out again with lp << grow leaves, the
 * new slots empty, into grown_dev: 2 (lp << grow) entries in the same layout.  Level l < d keeps its digests and continues with Z_l,
 * level d + i holds R_i at entry 0 and Z_{d+i} behind it, the last entry is 0; Z_0 = 0, Z_{l+1} = H(Z_l, Z_l) (the digest of an empty
 * subtree of height l: data independent, hashed once per device and kept there), R_0 the old root, R_{i+1} = H(R_i, Z_{d+i}).
 * levels_dev is only read.  d + grow at most 30 (VDB_ERR_ARG above); 1 + grow launches. */
int vdb_merkle_tree_grow_dev(const vdb_fr *levels_dev, size_t n, unsigned grow, vdb_fr *grown_dev);
/* Writes, deletes and growth proved against the committed root: the update circuit above with, per update, kinds[j] (0: a write, 1: a
 * delete; a HOST array of m bytes, NULL: all writes) and the padded leaf count doubled `grow` times before the first update.
 * d = log2(lp), depth = d + grow >= 1 (d == 0 is allowed when grow >= 1), w = the number of writes.  Stream: the assigned witnesses
 * [new vectors w x dim (the writes, in update order) | old leaves m | bits m x depth | siblings m x depth], when grow >= 1 followed by
 * R_0, the root before the growth (input_cells counts it); then, when grow >= 1, the growth block
 *   Z_0 = ctx.load_constant(0); Z_{l+1} = H(Z_l, Z_l), l = 0 .. depth - 2; R_{i+1} = H(R_i, Z_{d+i}), i = 0 .. grow - 1
 * ((depth - 1 + grow) x 4,506 + 1 cells; no digest is a constant of the circuit); then per update its block as above, a delete
 * emitting the one cell ctx.load_constant(0) in place of the leaf sponge: that cell is its new_leaf.  cur_old at the top of update 0
 * is tied to R_grow.  public, 3 m + 2 values as above: the old root is R_0, a delete shows new_leaf 0; grow and kinds are circuit shape
 * (the verifying key's).  Deleting an empty slot is legal.  `levels` is the tree at depth d + grow (vdb_merkle_tree_grow_dev's when
 * grow >= 1) and is left in the state after the batch; new_vectors holds the w rows of the writes (may be NULL when w == 0).
 * The number of launches depends on depth and on grow > 0, never on m, w or the kinds.  The _dev form honours vdb_wit_set_window.
 * VDB_ERR_ARG before anything is launched: a kind other than 0 or 1, d + grow > 30, d + grow == 0, an index >= lp << grow, and the
 * limits on m and on the cell count above. */
int vdb_wit_merkle_update_ops_size(size_t n, size_t dim, size_t m, const uint8_t *kinds, unsigned grow, uint64_t *cells, uint64_t *input_cells);
int vdb_wit_merkle_update_ops(vdb_fr *levels, size_t n, size_t dim, unsigned grow, const vdb_fr *new_vectors, const uint64_t *indices,
                              const uint8_t *kinds, size_t m, vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_merkle_update_ops_dev(vdb_fr *levels_dev, size_t n, size_t dim, unsigned grow, const vdb_fr *new_vectors_dev, const uint64_t *indices,
                                  const uint8_t *kinds, size_t m, vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *public_dev);
/* Reads proved against the committed root: m openings of slots indices[j] of the tree `levels` (vdb_merkle_tree_build_dev's layout, or
 * what a batch of updates left), "slot i of the database with this root holds vector v" or "slot i is empty".  The reference has no such
 * gadget; the cells are those of the closure a user of its chips writes.  depth = log2(lp) >= 1.  Repeats are allowed; reads do not
 * see each other; levels is only read.
 * Vector mode (vectors: the m vectors read, m x dim).  Stream, from cell 0: the assigned witnesses — the m vectors, per read the depth
 * index bits (least significant first), per read the depth siblings (leaf level first): input_cells of them — then per read j
 *   leaf = poseidon.clear(); update(vector_j); squeeze()                       (the leaf hash of merkle_commitment)
 *   cur = leaf; per level l: gate.assert_bit(b_l); lo = select(sib_l, cur, b_l); ro = select(cur, sib_l, b_l); cur = H(lo, ro)
 *                                                                              (4 + 8 + 8 + 4,506 = 4,526 cells a level)
 *   idx = gate.inner_product(bits, Constant(2^l))                              (1 + 3 (depth - 1) cells)
 * with H the node hash of merkle_commitment.  The circuit ties the top of read j >= 1 to the top of read 0 (a copy constraint, no
 * cells).  public 1 + 2 m + m dim values: [root | idx_j, leaf_j per read | vector_0 ... vector_{m-1}, dim words each].  A slot >= n
 * holds no vector and is refused.
 * Leaf mode (vectors NULL): the leaf digest is itself an assigned witness and public; stream [leaves m | bits | siblings], then per read
 * the levels and the index, no leaf sponge.  public 1 + 2 m values: [root | idx_j, leaf_j per read].  Any slot < lp may be opened; a
 * padding slot shows leaf 0: "this slot is empty".
 * Every digest of a path and every sibling is read from levels; nothing compares the vectors with the tree.  If a vector is not the one
 * committed at its slot, or levels is stale, the call still writes a stream, and that stream breaks a copy constraint (the sponge's
 * squeeze cell, or a node hash's output, differs from the `cur` cells that copy it): the Mock stage reports it and no proof verifies.
 * indices is a HOST array in both forms.  The number of kernel launches depends on neither m nor depth (five in vector mode, three in
 * leaf mode).  The _dev form honours vdb_wit_set_window like vdb_wit_merkle_dev.
 * Work space: vector mode 32 B x m x (3 (dim / 2 + 1) + 1) plus 4 B per read; leaf mode 4 B per read.
 * VDB_ERR_ARG, before anything is launched and before any buffer is touched: m == 0, depth == 0 (n == 1), n == 0 or dim == 0, n > 2^30
 * or dim > 2^20, an index >= lp, an index >= n in vector mode, m x depth >= 2^31, more than VDB_MERKLE_OPEN_MAX_CELLS cells.  There is
 * no cap on m itself: nothing is scanned in LDS. */
#define VDB_MERKLE_OPEN_MAX_CELLS ((uint64_t)1 << 34)
int vdb_wit_merkle_open_size(size_t n, size_t dim, size_t m, int with_vectors, uint64_t *cells, uint64_t *input_cells);
int vdb_wit_merkle_open(const vdb_fr *levels, size_t n, size_t dim, const vdb_fr *vectors /* m x dim, NULL: leaf mode */, const uint64_t *indices,
                        size_t m, vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_merkle_open_dev(const vdb_fr *levels_dev, size_t n, size_t dim, const vdb_fr *vectors_dev /* m x dim, NULL: leaf mode */,
                            const uint64_t *indices /* host */, size_t m, vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *public_dev);

/* The index of approximate-nearest-neighbour queries and the circuit of one query.  The reference's demo (tests/demo/mod.rs:38-91) finds
 * the nearest centroid, then the nearest vector of that centroid's cluster, in two circuits whose roots it compares outside any proof;
 * this is the closure that does both in one circuit, bound to one public index root.
 * members(c): the database vectors whose cluster id is c, in database order (select_cluster).  The index commitment:
 *   centroids_root = merkle_commitment(centroids);  cluster_root_c = merkle_commitment(members(c))
 *   index_root     = poseidon.clear(); update([centroids_root, cluster_root_0 .. cluster_root_{K-1}]); squeeze()
 * i.e. the leaf hash merkle_commitment computes for one vector of K + 1 words.
 * vdb_ann_index_build_dev (values only, everything left on the device): grouped_dev n x dim: the rows grouped by cluster, stable in
 * database order; slots_dev n x uint32: the database slot of every grouped row; offsets_dev (K + 1) x uint64: cluster c's rows are
 * [offsets[c], offsets[c + 1]) of the grouped rows; forest_dev: K + 1 segments, segment s at digest segment_offsets[s] holding the
 * 2 lp_s digests of a tree in vdb_merkle_tree_build_dev's layout (leaves, zero padding, root at 2 lp_s - 2), lp_s the power of two >=
 * the segment's leaf count — segment c < K is cluster c's tree, a valid levels_dev of vdb_wit_merkle_open_dev and
 * vdb_wit_merkle_update_dev over |members(c)| vectors, segment K the centroids' tree; roots_dev K + 2 digests:
 * [centroids_root | cluster_root_0 .. cluster_root_{K-1} | index_root].  vdb_ann_index_forest_size gives the digests of the forest and
 * (segment_offsets, K + 2 entries, may be NULL) where its segments start.  cluster_ids is a HOST array in both calls.
 * Launches: one grouping kernel (offsets and ranks for all clusters at once), one gather, two leaf launches (rows, centroids), one
 * segmented level launch per level of the deepest tree over all K + 1 trees, one for the roots and one for the sponge: 6 + max depth,
 * whatever K.  VDB_ERR_ARG before anything is launched: K == 0, n == 0, an id >= K, an empty cluster, n > VDB_ANN_MAX_VECTORS (32-bit
 * forest offsets and row numbers), K > VDB_ANN_MAX_CLUSTERS (the grouping kernel counts the clusters in 16 KiB of LDS).
 * Cost: the grouping kernel is a single wavefront that walks the n rows 64 at a time (a 64-step shuffle loop and two barriers a tile)
 * and writes every row's place itself: n / 64 serial tiles on one compute unit, 262,144 of them at n = VDB_ANN_MAX_VECTORS.
 *
 * vdb_wit_ann_query_size, vdb_wit_ann_query and vdb_wit_ann_query_dev are vdb_wit_ann_probe_size, vdb_wit_ann_probe and
 * vdb_wit_ann_probe_dev (below) at p == t == 1, the cluster searched the one entry of their lists: they forward there.  Its stream at
 * these values: assigned, from cell 0: the query (dim), the centroids (K x dim), the members of the cluster searched (n_c x dim), the K
 * cluster roots: input_cells of them.  Then
 *   ind_c, _  = nearest_vector(query, centroids)            croot = merkle_commitment(centroids)
 *   _, result = nearest_vector(query, members)              mroot = merkle_commitment(members)
 *   sel       = gate.select_by_indicator(cluster_roots, ind_c)                  (1 + 3 K cells)
 *   index_root = the sponge over [croot, cluster_roots ..]
 * and the circuit ties sel to mroot (a copy constraint, no cell): the cluster searched is the one whose centroid won.  Lookup cells:
 * the two nearest blocks', in block order.  public dim + 1 values: the result words, then index_root; the query, the winning cluster
 * and its size stay private.  The shape depends on (K, n_c, dim, metric): one proving key per cluster size.  Ties are nearest_vector's.
 * Members of another cluster than the winner's still give a stream; it breaks the sel = mroot copy.
 * centroid_levels_dev / member_levels_dev: the two trees where they are resident (forest segments K and c), only read — then the launch
 * count depends on neither K nor n_c; both NULL: the digests are computed by the call, a launch per level; one of them alone:
 * VDB_ERR_ARG.  The caller answers for member_levels_dev being the tree of members_dev (and centroid_levels_dev that of
 * centroids_dev): nothing checks it, and a stale tree gives a stream that fails only at Mock or verify time.  The _dev form honours
 * vdb_wit_set_window.  VDB_ERR_ARG before anything is launched: K == 0, n_c == 0, dim == 0, the limits above, dim > 2^20, more than
 * 2^34 cells, and the limits of vdb_wit_nearest_topk for each of the two searches. */
#define VDB_ANN_MAX_VECTORS ((size_t)1 << 24)
#define VDB_ANN_MAX_CLUSTERS 4096
int vdb_ann_index_forest_size(const uint32_t *cluster_ids /* host */, size_t n, size_t K, uint64_t *digests, uint64_t *segment_offsets);
int vdb_ann_index_build_dev(const vdb_fr *vectors_dev, const uint32_t *cluster_ids /* host */, const vdb_fr *centroids_dev, size_t n, size_t K,
                            size_t dim, vdb_fr *grouped_dev, uint32_t *slots_dev, uint64_t *offsets_dev, vdb_fr *forest_dev, vdb_fr *roots_dev);
int vdb_wit_ann_query_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t K, size_t n_c, size_t dim, uint64_t *cells,
                           uint64_t *lookups, uint64_t *input_cells);
int vdb_wit_ann_query(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *query, const vdb_fr *centroids, const vdb_fr *members,
                      const vdb_fr *cluster_roots, size_t K, size_t n_c, size_t dim, vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out,
                      vdb_fr *centroid_indicator_out, vdb_fr *member_indicator_out, vdb_fr *public_out);
int vdb_wit_ann_query_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *query_dev, const vdb_fr *centroids_dev,
                          const vdb_fr *members_dev, const vdb_fr *cluster_roots_dev, const vdb_fr *centroid_levels_dev, const vdb_fr *member_levels_dev,
                          size_t K, size_t n_c, size_t dim, vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev,
                          vdb_fr *centroid_indicator_dev, vdb_fr *member_indicator_dev, vdb_fr *public_dev);

/* The query over the p nearest clusters that returns the t nearest candidates, in one circuit bound to one index root: the two knobs of
 * an IVF-style index.  The reference's demo (tests/demo/mod.rs:47-90) searches one cluster for one vector, in two circuits; this is the
 * closure a user of its chips writes for p probes and t neighbours, every block one of the gadgets above.  n_c[r]: the size of the
 * cluster that round r of the centroid search states, N = sum n_c[r].  Assigned, from cell 0: the query (dim), the centroids (K x dim),
 * the candidates (N x dim: the members of the p probed clusters end to end in round order), the K cluster roots: input_cells of them.
 *   ind_c (p x K), _      = nearest_topk(query, centroids, p)        croot   = merkle_commitment(centroids)
 *   ind_m (t x N), result = nearest_topk(query, candidates, t)       mroot_r = merkle_commitment(candidates[o_r, o_r + n_c[r]))  r < p
 *   sel_r = gate.select_by_indicator(cluster_roots, ind_c[r])        (1 + 3 K cells each, the p of them end to end)
 *   index_root = the sponge over [croot, cluster_roots ..]
 * and the circuit ties sel_r to mroot_r for every r (copies, no cell): the candidates are exactly the members committed under the roots
 * of the centroids the p rounds state.  Context::load_zero caches its cell: among the trees [centroids, members_0 .. members_{p-1}] the
 * first padded one emits the zero cell, every later padded one copies it.  Lookup cells: the two searches', in block order.  public
 * t x dim + 1 values: the t results nearest first, then index_root; the query, the clusters probed and their sizes stay private (the
 * sizes shape the verifying key).  NOT stated: that no vector outside the probed clusters is nearer — the answer is approximate.
 * Ties are vdb_wit_nearest_topk's: centroids at equal distance leave in the same round, which states the LAST of them — two centroids
 * tied nearest cost one probe and the earlier one is never searched; a round with nothing left unmasked states centroid K - 1 again.
 * The entry points take whatever cluster list they are given: candidates of other clusters still give a stream, which breaks a
 * sel_r = mroot_r copy.  At p == t == 1 this is vdb_wit_ann_query: its entry points are these with lists of one.
 * vdb_wit_ann_probe: candidates is one flat N x dim host array; the call hashes the trees itself.  vdb_wit_ann_probe_dev: members_dev is a
 * HOST array of p device pointers to the clusters' rows, member_levels_dev a HOST array of p device pointers to their trees (forest
 * segments) or NULL, centroid_levels_dev the centroids' tree or NULL: the p + 1 resident trees come all together or not at all
 * (VDB_ERR_ARG otherwise), and the caller answers for their being the trees of these rows, as above.  With them the launch count depends
 * on p (one tree trace per probed cluster) and on neither K, any n_c[r] nor t.  One gather pass writes the candidates' assigned cells and
 * the contiguous buffer the second search reads.  centroid_indicators p x K, candidate_indicators t x N raw 0/1 bits.  The _dev form
 * honours vdb_wit_set_window.  VDB_ERR_ARG before anything is launched: K == 0, dim == 0, dim > 2^20, K > VDB_ANN_MAX_CLUSTERS, p == 0,
 * p > K, p > VDB_ANN_PROBE_MAX, an empty cluster, N > VDB_ANN_MAX_VECTORS, t == 0, t > N, the limits of vdb_wit_nearest_topk for each of
 * the two searches, more than 2^34 cells. */
#define VDB_ANN_PROBE_MAX 16
int vdb_wit_ann_probe_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t K, size_t dim, size_t p, const size_t *n_c, size_t t,
                           uint64_t *cells, uint64_t *lookups, uint64_t *input_cells);
int vdb_wit_ann_probe(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *query, const vdb_fr *centroids, const vdb_fr *candidates,
                      const vdb_fr *cluster_roots, size_t K, size_t dim, size_t p, const size_t *n_c, size_t t, vdb_fr *stream_out, vdb_fr *lookup_out,
                      uint8_t *selector_out, vdb_fr *centroid_indicators_out, vdb_fr *candidate_indicators_out, vdb_fr *public_out);
int vdb_wit_ann_probe_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *query_dev, const vdb_fr *centroids_dev,
                          const vdb_fr *const *members_dev /* host array */, const vdb_fr *cluster_roots_dev, const vdb_fr *centroid_levels_dev,
                          const vdb_fr *const *member_levels_dev /* host array or NULL */, size_t K, size_t dim, size_t p, const size_t *n_c, size_t t,
                          vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, vdb_fr *centroid_indicators_dev,
                          vdb_fr *candidate_indicators_dev, vdb_fr *public_dev);
/* The winners of p rounds of top-k as VALUES alone (vdb_nearest_values at p rounds): for every query q and round r < p the minimum of
 * the entries the earlier rounds left and the LAST i at it — the index vdb_wit_nearest_topk's select_by_indicator states for that round,
 * ties and exhausted rounds as there.  idx_out n_queries x p uint32, dist_out n_queries x p values or NULL.  The launch count depends on
 * neither n_queries, n nor p.  Work space: vdb_wit_nearest_topk's.  VDB_ERR_ARG before anything is launched: n_queries, n or dim == 0 and
 * vdb_wit_nearest_topk's limits at topk == p; VDB_ERR_DOMAIN as for the witness call. */
int vdb_nearest_topk_values_dev(uint32_t precision_bits, uint32_t lookup_bits, int metric, const vdb_fr *queries_dev, const vdb_fr *vectors_dev,
                                size_t n_queries, size_t n, size_t dim, size_t p, uint32_t *idx_out_dev, vdb_fr *dist_out_dev);
int vdb_nearest_topk_values(uint32_t precision_bits, uint32_t lookup_bits, int metric, const vdb_fr *queries, const vdb_fr *vectors, size_t n_queries,
                            size_t n, size_t dim, size_t p, uint32_t *idx_out, vdb_fr *dist_out);

/* Inserts and replacements proved against the committed index root: m writes into ONE cluster c of an index of K clusters move
 * index_root_old to index_root_new in one circuit.  The reference has no such gadget; the cells are those of the closure a user of its
 * chips writes.  n_c = |members(c)| before the batch, lp the power of two >= n_c, depth = log2(lp) + grow >= 1; the cluster's tree may
 * be doubled `grow` times before the first write, as in vdb_wit_merkle_update_ops.  Stream, from cell 0:
 *   A  [c | centroids_root | cluster_root_0 .. cluster_root_{K-1}] assigned                      (K + 2 cells: input_cells)
 *   B  ind = gate.idx_to_indicator(c, K): ind_0 = is_zero(c) (8 cells), ind_j = is_equal(c, Constant(j)) (12 cells), j >= 1
 *   C  picked = gate.select_by_indicator(cluster roots, ind)                                     (1 + 3 K cells)
 *   D  index_root_old = poseidon.clear(); update([centroids_root, cluster roots ..]); squeeze()  (the sponge of vdb_wit_ann_query)
 *   E  the whole stream of vdb_wit_merkle_update_ops(levels, n_c, dim, grow, new_vectors, indices, kinds = NULL), its assigned
 *      witnesses included, from cell update_base on
 *   F  out_j = gate.select(new cluster root, cluster_root_j, ind_j), j = 0 .. K - 1              (8 K cells)
 *   G  index_root_new = the sponge over [centroids_root, out_0 .. out_{K-1}]
 * Copies (no cell): every idx operand of B is c; C's operands are the header's roots and B's outputs; D's words are the header's; picked
 * is tied to the old root block E exposes (R_0 when grow >= 1, else cur_old at the top of update 0); F's a is E's final root, its b and
 * sel the header's roots and B's outputs; G's words are centroids_root and F's outputs.
 * public, 3 m + 3 values: [index_root_old | c | idx_j, old_leaf_j, new_leaf_j per write | index_root_new].  E's own old and new roots
 * stay private.  K, m, grow and the depth are circuit shape; c is not: one proving key serves every cluster of the same depth.
 * Writes only, and the members stay dense: the query circuit hashes merkle_commitment(members(c)) over n_c dense rows, so a hole would
 * make the cluster unqueryable.  Write j is accepted when indices[j] is below the fill at its turn (a replacement) or equal to it (an
 * append: the fill rises by one); the fill starts at n_c; writes of a batch see each other.  Deletes are a batch of their own:
 * vdb_wit_ann_delete below (chain the two calls to mix them).
 * Cluster assignment is NOT proved: nothing in the circuit shows that c is the cluster whose centroid is nearest to a new vector (the
 * index build does not prove its cluster ids either).  The caller chooses c; nearest_vector over the centroids is its tool.
 * roots: the K + 1 digests [centroids_root | cluster roots] (the head of vdb_ann_index_build_dev's roots_dev).  levels: cluster c's tree
 * at depth d + grow (forest segment c, copied, and grown by vdb_merkle_tree_grow_dev when grow >= 1), left in the state after the batch.
 * indices is a HOST array.  If levels is not the tree whose root is cluster_root_c the call still writes a stream; it breaks the picked
 * copy.  The number of launches depends on the depth and on grow > 0, never on K, m, c or n_c.  The _dev form honours
 * vdb_wit_set_window.  VDB_ERR_ARG before anything is launched: K == 0, K > VDB_ANN_MAX_CLUSTERS, c >= K, an index above the fill at
 * its turn or >= lp << grow, and every limit of vdb_wit_merkle_update_ops (m, depth, cells).
 *
 * vdb_ann_index_apply_dev (values only, functional): the index after the batch into caller-provided buffers, from the old index's
 * buffers (only read: the old index stays valid), updated_levels_dev (the 2 (lp_c << grow) digests the witness call left), the batch
 * and db_slots (HOST, one database slot per append, in append order: n, n + 1, ... keeps "members in database order").  cluster_sizes:
 * HOST, the K sizes before the batch.  Rows of clusters <= c stay, the appended rows follow cluster c's, later rows move by the number
 * of appends; the last write of the batch to a slot wins; the forest is moved segment by segment (segment c from the updated tree); the
 * K + 1 roots are copied, root c replaced, and the index root hashed again: four launches whatever the shape.  The result equals,
 * entry for entry, vdb_ann_index_build_dev over the updated database and ids — so `grow` must be the smallest number of doublings
 * that fits the appends (lp_c << grow == the power of two >= n_c + appends), VDB_ERR_ARG otherwise, as for the refusals above.
 * vdb_ann_index_apply_size: the number of appends, the digests of the new forest and its K + 2 segment offsets (each may be NULL).
 * Output sizes: grouped (n + appends) x dim, slots n + appends, offsets K + 1, forest `digests`, roots K + 2. */
int vdb_wit_ann_update_size(size_t K, size_t n_c, size_t dim, size_t m, unsigned grow, uint64_t *cells, uint64_t *input_cells,
                            uint64_t *update_base);
int vdb_wit_ann_update(vdb_fr *levels, const vdb_fr *roots, size_t K, size_t cluster, size_t n_c, size_t dim, unsigned grow,
                       const vdb_fr *new_vectors, const uint64_t *indices, size_t m, vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_ann_update_dev(vdb_fr *levels_dev, const vdb_fr *roots_dev, size_t K, size_t cluster, size_t n_c, size_t dim, unsigned grow,
                           const vdb_fr *new_vectors_dev, const uint64_t *indices /* host */, size_t m, vdb_fr *stream_dev, uint8_t *selector_dev,
                           vdb_fr *public_dev);
int vdb_ann_index_apply_size(const uint64_t *cluster_sizes /* host */, size_t K, size_t cluster, unsigned grow, const uint64_t *indices /* host */,
                             size_t m, uint64_t *appends, uint64_t *digests, uint64_t *segment_offsets);
int vdb_ann_index_apply_dev(const vdb_fr *grouped_dev, const uint32_t *slots_dev, const vdb_fr *forest_dev, const vdb_fr *roots_dev,
                            const uint64_t *cluster_sizes /* host */, size_t K, size_t dim, size_t cluster, unsigned grow,
                            const vdb_fr *updated_levels_dev, const vdb_fr *new_vectors_dev, const uint64_t *indices /* host */,
                            const uint32_t *db_slots /* host */, size_t m, vdb_fr *grouped_out_dev, uint32_t *slots_out_dev,
                            uint64_t *offsets_out_dev, vdb_fr *forest_out_dev, vdb_fr *roots_out_dev);

/* Deletes against the index root: m deletes from ONE cluster c move index_root_old to index_root_new in one circuit.  The members stay
 * dense by swap-with-last: delete j of slot_j moves the member at last_j = fill - 1 (the fill at its turn: n_c - j) into slot_j and
 * empties slot last_j.  slot_j == last_j is legal (the leaf is carried onto itself, then deleted) and so are repeats: deleting slot 0
 * twice removes the vector the first delete moved there.  n_c - m >= 1: an emptied cluster is refused, as the build refuses one.
 * With lp the power of two >= n_c, d = log2(lp) and s the number of halvings with lp >> s == the power of two >= n_c - m (computed
 * by the call, returned by _size; nothing has to be prepared for a shrink), the stream is, from cell 0:
 *   A - D  exactly those of vdb_wit_ann_update
 *   E'     the update block of vdb_wit_merkle_update_ops (grow = 0) over 2 m path updates, from cell update_base on: update 2 j at
 *          slot_j, whose new leaf is CARRIED — one ctx.load_witness(digest) cell where a delete has its load_constant(0), the digest being
 *          the leaf at last_j at that turn — and update 2 j + 1 at last_j, a delete.  (The carried kind is internal to this call:
 *          vdb_wit_merkle_update_ops keeps refusing a kind above 1.)
 *   S      only when s >= 1, from cell shrink_base on: S_0 assigned, Z_0 = load_constant(0), Z_{l+1} = H(Z_l, Z_l) for l = 0 .. d - 2,
 *          S_{i+1} = H(S_i, Z_{d-s+i}) for i = 0 .. s - 1: 2 + (d - 1 + s) * 4506 cells
 *   F, G   those of vdb_wit_ann_update; F's a copies the new cluster root: S_0 when s >= 1, else E''s final root
 * Copies (no cell), beyond those of vdb_wit_ann_update: picked <-> cur_old at the top of update 0; the carried-leaf cell of update 2 j
 * <-> the assigned old-leaf cell of update 2 j + 1 (what left the last slot is what arrived); S_s <-> E''s final root, so the removed
 * half is PROVED empty: were it not, the hashes would disagree with the tree and the copy would break.
 * public, 4 m + 3 values: [index_root_old | c | slot_j, removed_leaf_j, last_j, moved_leaf_j per delete | index_root_new].  The fill is
 * not committed (nothing in vdb_wit_ann_update commits it either): a verifier who tracks n_c checks last_j == n_c - 1 - j on the public
 * values.  The shape depends on (K, d, m, s, dim) only, never on which slots are deleted; the launches depend on d and on s > 0.
 * levels: cluster c's tree over its n_c members (forest segment c, copied), left in the state after the batch AT ITS OLD SIZE:
 * vdb_ann_index_remove_dev cuts it.  slots is a HOST array.  The _dev form honours vdb_wit_set_window.
 * VDB_ERR_ARG before anything is launched: m == 0, 2 m > VDB_MERKLE_UPDATE_MAX_UPDATES, m >= n_c, a slot >= the fill at its turn,
 * c >= K, K == 0, K > VDB_ANN_MAX_CLUSTERS, the cell limit.  _size takes no slots; each of its outputs may be NULL.
 *
 * vdb_ann_index_remove_dev (values only, functional; the old buffers are only read): the index after the batch.  Cluster c's
 * surviving position p < n_c - m holds the original member origin[p] the batch leaves there, rows of later clusters move down by m,
 * forest segment c is the updated tree cut to lp >> s leaves, later segments move, root c is replaced and the index root hashed again:
 * four launches whatever the shape.  A REMOVAL COMPACTS THE DATABASE: database slots are renumbered so that the result equals, entry
 * for entry (grouped rows, slots 0 .. n - m - 1, offsets, forest, roots), vdb_ann_index_build_dev over the database whose rows are the
 * result's own grouped rows in order, with nondecreasing cluster ids.  A caller that keeps outside references to database slots maps
 * them through the old slots array before the call.  vdb_ann_index_remove_size: s, the digests of the new forest and its K + 2 segment
 * offsets (each may be NULL).  Output sizes: grouped (n - m) x dim, slots n - m, offsets K + 1, forest `digests`, roots K + 2. */
int vdb_wit_ann_delete_size(size_t K, size_t n_c, size_t dim, size_t m, uint64_t *cells, uint64_t *input_cells, uint64_t *update_base,
                            uint64_t *shrink_base, unsigned *shrink);
int vdb_wit_ann_delete(vdb_fr *levels, const vdb_fr *roots, size_t K, size_t cluster, size_t n_c, size_t dim, const uint64_t *slots, size_t m,
                       vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_ann_delete_dev(vdb_fr *levels_dev, const vdb_fr *roots_dev, size_t K, size_t cluster, size_t n_c, size_t dim,
                           const uint64_t *slots /* host */, size_t m, vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *public_dev);
int vdb_ann_index_remove_size(const uint64_t *cluster_sizes /* host */, size_t K, size_t cluster, const uint64_t *slots /* host */, size_t m,
                              unsigned *shrink, uint64_t *digests, uint64_t *segment_offsets);
int vdb_ann_index_remove_dev(const vdb_fr *grouped_dev, const vdb_fr *forest_dev, const vdb_fr *roots_dev,
                             const uint64_t *cluster_sizes /* host */, size_t K, size_t dim, size_t cluster, const vdb_fr *updated_levels_dev,
                             const uint64_t *slots /* host */, size_t m, vdb_fr *grouped_out_dev, uint32_t *slots_out_dev,
                             uint64_t *offsets_out_dev, vdb_fr *forest_out_dev, vdb_fr *roots_out_dev);

/* Moves against the index root: m members pass from cluster a = src to cluster b = dst (a != b) in one circuit, index_root_old to
 * index_root_new.  The database, its slots and its database_root are untouched: no vector enters the circuit, a leaf travels as one
 * witness cell.  Move j is delete j of a as vdb_wit_ann_delete has it (swap-with-last; repeats and slot_j == last_j are legal) and an
 * append to b at dest_j = n_b + j whose new leaf is the removed leaf.  s: a's halvings as in vdb_wit_ann_delete; g: the smallest number
 * of doublings after which b's tree holds n_b + m leaves (both returned by _size).  Stream, from cell 0:
 *   A      [a | b | centroids_root | cluster_root_0 .. cluster_root_{K-1}] assigned, K + 3 cells (input_cells)
 *   B_a, C_a  idx_to_indicator(a, K), select_by_indicator(cluster roots, .) -> picked_a            (blocks B, C of vdb_wit_ann_update)
 *   D      the sponge over [centroids_root | cluster roots] -> index_root_old
 *   E'     the delete's update block on a's tree, from cell delete_base on: 2 m path updates, 2 j at slot_j with a carried leaf, 2 j + 1 at
 *          last_j a delete; S from shrink_base on when s >= 1
 *   F_a    mid_j = select(a's new root, cluster_root_j, ind_a_j), 8 K cells
 *   B_b, C_b  idx_to_indicator(b, K), select_by_indicator(mid_0 .. mid_{K-1}, .) -> picked_b: over the roots AFTER the removal
 *   E_b    the update block of vdb_wit_merkle_update_ops on b's tree with grow = g, from cell append_base on: m appends at dest_j, each
 *          new leaf CARRIED: one ctx.load_witness(digest) cell where a write has its leaf sponge
 *   F_b    out_j = select(b's new root, mid_j, ind_b_j)
 *   G      the sponge over [centroids_root | out_0 ..] -> index_root_new
 * Copies (no cell), beyond those of the blocks themselves: picked_a <-> the old root E' exposes; picked_b <-> the old root E_b exposes
 * (R_0 when g >= 1, else cur_old at the top of its update 0); THE MOVE: the carried-leaf cell of E_b's update j <-> the assigned old-leaf
 * cell of E''s update 2 j, the removed leaf; F_a's a <-> S_0 (E''s final root when s == 0); F_b's a <-> E_b's final root.  Because b's
 * root is selected from mid, the circuit is sound whatever a and b are and holds no a != b gate; the library refuses a == b because the
 * resident operation is not defined for it.
 * public, 6 m + 4 values: [index_root_old | a | b | slot_j, leaf_j, last_j, moved_leaf_j, dest_j, dest_old_leaf_j per move |
 * index_root_new].  The fills are not committed: a verifier who tracks n_a and n_b checks last_j == n_a - 1 - j, dest_j == n_b + j and
 * dest_old_leaf_j == 0.  The shape depends on (K, d_a, s, d_b, g, m) only; no input row, no lookup cell; the launches depend on d_a, d_b,
 * s > 0 and g > 0.
 * levels_src: a's tree over its n_a members, left in the state after the batch at its old size; levels_dst: b's tree AFTER
 * vdb_merkle_tree_grow_dev when g > 0, left in the state after the batch.  slots is a HOST array.  The _dev form honours
 * vdb_wit_set_window.  VDB_ERR_ARG before anything is launched: m == 0, 2 m > VDB_MERKLE_UPDATE_MAX_UPDATES, m >= n_a, a slot >= a's
 * fill at its turn, a == b, a >= K, b >= K, K < 2, K > VDB_ANN_MAX_CLUSTERS, n_b == 0, a grow that is not the smallest that fits, the cell
 * limit.  _size takes no slots; each of its outputs may be NULL.
 *
 * vdb_ann_index_move_dev (values only, functional; the old buffers are only read): the index after the batch.  a's surviving position p
 * holds its original member origin[p], the moved rows follow b's rows in move order, the rows between the two clusters shift by m; THE
 * SLOTS ENTRIES TRAVEL WITH THEIR ROWS: the database is not renumbered.  Forest segment a is its updated tree cut to lp_a >> s, segment
 * b the grown, updated tree; two roots are replaced and the index root is hashed once: four launches whatever the shape.
 * vdb_ann_index_move_size: s, g, the digests of the new forest and its K + 2 segment offsets (each may be NULL).  Output sizes: grouped
 * n x dim, slots n, offsets K + 1, forest `digests`, roots K + 2. */
int vdb_wit_ann_move_size(size_t K, size_t n_a, size_t n_b, size_t m, uint64_t *cells, uint64_t *input_cells, uint64_t *delete_base,
                          uint64_t *shrink_base, uint64_t *append_base, unsigned *shrink, unsigned *grow);
int vdb_wit_ann_move(vdb_fr *levels_src, vdb_fr *levels_dst, const vdb_fr *roots, size_t K, size_t src, size_t dst, size_t n_a, size_t n_b,
                     unsigned grow, const uint64_t *slots, size_t m, vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_ann_move_dev(vdb_fr *levels_src_dev, vdb_fr *levels_dst_dev, const vdb_fr *roots_dev, size_t K, size_t src, size_t dst, size_t n_a,
                         size_t n_b, unsigned grow, const uint64_t *slots /* host */, size_t m, vdb_fr *stream_dev, uint8_t *selector_dev,
                         vdb_fr *public_dev);
int vdb_ann_index_move_size(const uint64_t *cluster_sizes /* host */, size_t K, size_t src, size_t dst, const uint64_t *slots /* host */, size_t m,
                            unsigned *shrink, unsigned *grow, uint64_t *digests, uint64_t *segment_offsets);
int vdb_ann_index_move_dev(const vdb_fr *grouped_dev, const uint32_t *slots_dev, const vdb_fr *forest_dev, const vdb_fr *roots_dev,
                           const uint64_t *cluster_sizes /* host */, size_t K, size_t dim, size_t src, size_t dst, unsigned grow,
                           const vdb_fr *updated_src_dev, const vdb_fr *updated_dst_dev, const uint64_t *slots /* host */, size_t m,
                           vdb_fr *grouped_out_dev, uint32_t *slots_out_dev, uint64_t *offsets_out_dev, vdb_fr *forest_out_dev,
                           vdb_fr *roots_out_dev);

/* Linked writes: m inserts or replacements into ONE cluster c of the index and the same m leaf changes in the database tree, in one
 * circuit: (database_root_old, index_root_old) to (database_root_new, index_root_new).  Every vector is hashed once.  Blocks A - D, E, F
 * and G are vdb_wit_ann_update's, cell for cell (E from cell update_base on, grow = g_c); one block E_db lies between E and F, from cell
 * update_db_base on: the update block of vdb_wit_merkle_update_ops on the database tree (n_db leaves, dim 1, grow = g_db) with m updates
 * at the database slots db_idx_j, each new leaf CARRIED: one ctx.load_witness(digest) cell where a write has its leaf sponge.  A slot of
 * E_db may be occupied (a replacement) or empty (an append: its old leaf is 0, the padding of the grown tree).
 * Copies (no cell), beyond those of vdb_wit_ann_update: the carried-leaf cell of E_db's update j <-> the new-leaf digest cell of E's
 * update j (the squeeze of its leaf sponge); the assigned old-leaf cell of E_db's update j <-> the assigned old-leaf cell of E's update j;
 * the public database_root_old / database_root_new <-> the old root E_db exposes (R_0 when g_db >= 1, else cur_old at the top of its
 * update 0) and its final root.
 * public, 4 m + 5 values: [database_root_old | index_root_old | c | idx_j, db_idx_j, old_leaf_j, new_leaf_j per write |
 * database_root_new | index_root_new].  The fills are not committed: a verifier who tracks n_c and n_db checks for an append idx_j ==
 * the cluster's fill, db_idx_j == the database's fill and old_leaf_j == 0.  db_idx_j need not be "the" slot of the member: both trees
 * lose the same digest and gain the same digest, and equal digests are interchangeable in a multiset.
 * The shape depends on (K, d_c, g_c, d_db, g_db, m, dim) only; no input row, no lookup cell.
 * levels_c: cluster c's tree AFTER vdb_merkle_tree_grow_dev when g_c > 0; levels_db: the database tree (vdb_ann_index_db_tree_dev's) AFTER
 * vdb_merkle_tree_grow_dev when g_db > 0; both are left in the state after the batch.  indices and db_indices are HOST arrays.  The _dev
 * form honours vdb_wit_set_window.  VDB_ERR_ARG before anything is launched: vdb_wit_ann_update's refusals; n_db == 0; n_c > n_db; a
 * db_indices entry the batch does not yield (an append's is n_db + the appends so far, a write to a member this batch appended has that
 * member's, a replacement's lies below n_db + the appends so far); a grow_db that is not the smallest that fits; the cell limit.
 * vdb_ann_write_db_indices (values only, host arrays, no device call): db_indices from the cluster's n_c recorded database slots (what the
 * index's slots hold for cluster c) and the batch's indices, with the appends and g_db (each may be NULL); VDB_ERR_ARG on a write above
 * the fill, n_db == 0, n_c > n_db or a recorded slot >= n_db.
 * _size takes the number of appends in place of the indices (the shape of every batch with as many) and returns the g_c and g_db it
 * would pick; each of its outputs may be NULL.
 *
 * vdb_ann_index_write_dev (values only, functional; the old buffers are only read): both resident objects after the batch.  The index
 * is vdb_ann_index_apply_dev's (its four launches), the appends at database slots n, n + 1, ... in append order; db_tree_out (2 * the
 * grown padded leaf count digests, db_digests of _size) is updated_db_levels copied device to device: the new index's database tree, no
 * vector or node hashed again.  Its refusals are vdb_ann_index_apply_dev's (n_db is the sum of the sizes) and a grow_db that is not the
 * smallest that fits.  vdb_ann_index_write_size: the appends, g_c, g_db, the digests of the new forest, its K + 2 segment offsets and
 * the digests of the database tree (each may be NULL). */
int vdb_wit_ann_write_size(size_t K, size_t n_c, size_t n_db, size_t dim, size_t m, size_t appends, uint64_t *cells, uint64_t *input_cells,
                           uint64_t *update_base, uint64_t *update_db_base, unsigned *grow_c, unsigned *grow_db);
int vdb_ann_write_db_indices(const uint64_t *cluster_slots /* host */, size_t n_c, size_t n_db, const uint64_t *indices /* host */, size_t m,
                             uint64_t *db_indices /* host, m */, uint64_t *appends, unsigned *grow_db);
int vdb_wit_ann_write(vdb_fr *levels_c, vdb_fr *levels_db, const vdb_fr *roots, size_t K, size_t cluster, size_t n_c, size_t n_db, size_t dim,
                      unsigned grow_c, unsigned grow_db, const vdb_fr *new_vectors, const uint64_t *indices, const uint64_t *db_indices, size_t m,
                      vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_ann_write_dev(vdb_fr *levels_c_dev, vdb_fr *levels_db_dev, const vdb_fr *roots_dev, size_t K, size_t cluster, size_t n_c, size_t n_db,
                          size_t dim, unsigned grow_c, unsigned grow_db, const vdb_fr *new_vectors_dev, const uint64_t *indices /* host */,
                          const uint64_t *db_indices /* host */, size_t m, vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *public_dev);
int vdb_ann_index_write_size(const uint64_t *cluster_sizes /* host */, size_t K, size_t cluster, const uint64_t *indices /* host */, size_t m,
                             uint64_t *appends, unsigned *grow_c, unsigned *grow_db, uint64_t *digests, uint64_t *segment_offsets,
                             uint64_t *db_digests);
int vdb_ann_index_write_dev(const vdb_fr *grouped_dev, const uint32_t *slots_dev, const vdb_fr *forest_dev, const vdb_fr *roots_dev,
                            const uint64_t *cluster_sizes /* host */, size_t K, size_t dim, size_t cluster, unsigned grow_c, unsigned grow_db,
                            const vdb_fr *updated_levels_dev, const vdb_fr *updated_db_levels_dev, const vdb_fr *new_vectors_dev,
                            const uint64_t *indices /* host */, size_t m, vdb_fr *grouped_out_dev, uint32_t *slots_out_dev,
                            uint64_t *offsets_out_dev, vdb_fr *forest_out_dev, vdb_fr *roots_out_dev, vdb_fr *db_tree_out_dev);

/* The audit of one cluster's routing: in the index with root index_root, every member committed under cluster_root_c is at least as
 * close to centroid c as to any other committed centroid, in the circuit's fixed-point distance for `metric`.  It covers the build's
 * cluster ids and the writes after them alike (audit cluster c of the index a batch into c leaves); K such proofs cover an index.  It
 * does not prove that centroids are means (vdb_wit_ann_mean below does, per cluster and by a proof of its own) or that the database is
 * complete.  The reference has no such gadget; the cells are those of
 * the closure a user of its chips writes.  Stream, from cell 0:
 *   A - D  exactly those of vdb_wit_ann_update: the header [c | centroids_root | cluster roots] (K + 2 cells: input_cells),
 *          ind = idx_to_indicator(c, K), picked = select_by_indicator(cluster roots, ind), index_root = the sponge over the roots
 *   I      [centroids K x dim | members n_c x dim] assigned
 *   R      per member i, at R + i * per_member: d_ij = distance(centroid_j, member_i), j = 0 .. K - 1 (the centroid in the vector role,
 *          the member in the query role: nearest_vector's argument order, so the values are vdb_nearest_values' bit for bit); the
 *          K - 1 qmin of the chain -> m_i; own_i = gate.select_by_indicator([d_i0 .. d_i,K-1], ind)      (1 + 3 K cells)
 *   MC     croot = merkle_commitment(centroids)
 *   MM     mroot = merkle_commitment(members), its padding copying MC's zero cell where MC's padding has loaded one
 * Copies (no cell): R's distance operands copy I and its ind cells B's outputs; own_i is tied to m_i (to d_i0 at K == 1, where there
 * is no chain); croot is tied to the header's centroids_root and mroot to picked.  Lookup cells are R's alone, member i's from
 * i * per_member_l on: the distance runs, then the qmin runs.  public, 2 values: [index_root | c].
 * Ties: the statement is "centroid c attains the minimum", not nearest_vector's indicator is_equal(min, d_j), whose select_by_indicator
 * is only satisfiable when it is one-hot: a member equidistant from two centroids is accepted under either, so an honest index with a
 * tie stays provable.  Without ties this is vdb_nearest_values' rule (the last index at the minimum).
 * A misrouted member still gives a stream: the call succeeds, routed[i] = 0 for that member (1 for every member whose own centroid
 * attains the minimum) and only its own_i = m_i copy fails at Mock or verify time.  The shape depends on (K, n_c, dim, metric): one
 * proving key per cluster size; c is a witness.
 * roots: the K + 1 digests [centroids_root | cluster roots].  centroid_levels_dev / member_levels_dev: the two trees where they are
 * resident (forest segments K and c), only read — then the launch count depends on neither K nor n_c; both NULL: the digests are
 * computed by the call, a launch per level; one alone: VDB_ERR_ARG.  The caller answers for the trees being those of the rows given,
 * as in vdb_wit_ann_query.  Launches: the head's four emitters and its sponge, one assignment kernel, the distance generators over
 * n_c * K instances, one kernel for the prefix minima, one for the qmin chains (launched at K == 1 too, where it has no lane), one for the
 * picks, the two trees' traces and the inverse fix-up: 20 with resident trees under Euclidean, whatever K, c and n_c.  A member EQUAL to
 * a centroid has distance 0, where the reference's qsqrt(0) violates its own asserted constants (Euclidean): such a stream fails Mock.
 * The _dev form honours vdb_wit_set_window.  VDB_ERR_ARG before anything is launched: K == 0,
 * K > VDB_ANN_MAX_CLUSTERS, cluster >= K, n_c > VDB_ANN_MAX_VECTORS, n_c == 0, dim == 0, dim > 2^20, n_c * K or n_c * dim above
 * VDB_NEAREST_TOPK_MAX_INSTANCES, more than 2^34 cells.  _size takes no cluster; each of its outputs may be NULL. */
int vdb_wit_ann_audit_size(int metric, uint32_t precision_bits, uint32_t lookup_bits, size_t K, size_t n_c, size_t dim, uint64_t *cells,
                           uint64_t *lookups, uint64_t *input_cells);
int vdb_wit_ann_audit(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *centroids, const vdb_fr *members,
                      const vdb_fr *roots, size_t K, size_t cluster, size_t n_c, size_t dim, vdb_fr *stream_out, vdb_fr *lookup_out,
                      uint8_t *selector_out, uint8_t *routed_out, vdb_fr *public_out);
int vdb_wit_ann_audit_dev(int metric, uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *centroids_dev, const vdb_fr *members_dev,
                          const vdb_fr *roots_dev, const vdb_fr *centroid_levels_dev, const vdb_fr *member_levels_dev, size_t K, size_t cluster,
                          size_t n_c, size_t dim, vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, uint8_t *routed_dev,
                          vdb_fr *public_dev);

/* The mean audit of one cluster: in the index with root index_root, word for word, centroid c equals
 * qdiv(sum of the members committed under cluster_root_c, quantization(n_c)) in the circuit's fixed-point arithmetic.  K such proofs and
 * K routing audits (vdb_wit_ann_audit) together state that the index is a fixed point of one Lloyd step over the committed members.  Not
 * proved: that the database is complete, that a recentred index (new centroids, new root) descends from its predecessor.  The reference
 * leaves this gadget commented out (src/gadget/vectordb.rs, mean_merkle: a qadd chain over the vectors, qdiv by
 * load_constant(quantization(len)), bound to a Merkle root); the cells are those of that closure.  Stream, from cell 0:
 *   A - D  exactly those of vdb_wit_ann_update: the header [c | centroids_root | cluster roots] (K + 2 cells: input_cells),
 *          ind = idx_to_indicator(c, K), picked = select_by_indicator(cluster roots, ind), index_root = the sponge over the roots
 *   I      [centroids K x dim | members n_c x dim] assigned
 *   S      own_j = gate.select_by_indicator([centroid_0[j] .. centroid_K-1[j]], ind), j = 0 .. dim - 1          (1 + 3 K cells each)
 *   M      len = load_constant(quantization(n_c)) (one cell, constant flag); for members i = 1 .. n_c - 1 and words j the qadd
 *          [member_i[j], s_i-1,j, 1, s_ij] at M + 1 + 4 ((i - 1) dim + j), s_0j = member_0[j] (kmeans' argument order); then per word
 *          mean_j = qdiv(s_n_c-1,j, len)                                                                        (qdiv's cells each)
 *   MC     croot = merkle_commitment(centroids)
 *   MM     mroot = merkle_commitment(members), its padding copying MC's zero cell where MC's padding has loaded one
 * Copies (no cell): the chain's operands copy I (at n_c == 1 there is no chain and qdiv's first operand copies the member's cell), every
 * qdiv divisor copies len, S's indicator cells copy B's outputs; mean_j is tied to own_j; croot is tied to the header's centroids_root and
 * mroot to picked.  Lookup cells are the qdiv blocks' alone, word j's from j * (qdiv's lookup cells) on.  public, 2 values:
 * [index_root | c].
 * A centroid that is not the mean still gives a stream: the call succeeds, mean_ok[j] = 0 for the words that differ (1 for the others)
 * and only their mean_j = own_j copies fail at Mock or verify time.  The shape depends on (K, n_c, dim): n_c enters as a constant, so there
 * is one proving key per cluster size; c is a witness.
 * Known cost: MC hashes all K centroids to bind one.  A Merkle opening of slot c of the centroids' tree, its index tied to c, would cost
 * about one leaf and depth levels instead.
 * roots, centroid_levels_dev / member_levels_dev: as in vdb_wit_ann_audit (both resident: the launch count depends on neither K nor n_c;
 * both NULL: the digests are computed by the call; one alone: VDB_ERR_ARG).  Launches: the head's four emitters and its sponge, one
 * assignment kernel, one selection, one constant, one kernel for the chains (launched at n_c == 1 too, where it emits nothing), one for
 * the quotients, the two trees' traces and the inverse fix-up.  The _dev form honours vdb_wit_set_window; mean_ok and public are whole
 * in every window.  VDB_ERR_ARG before anything is launched: K == 0, K > VDB_ANN_MAX_CLUSTERS, cluster >= K,
 * n_c > VDB_ANN_MAX_VECTORS, n_c == 0, dim == 0, dim > 2^20, K * dim or n_c * dim above VDB_NEAREST_TOPK_MAX_INSTANCES,
 * n_c >= 2^precision_bits (qdiv asserts its divisor below 2^(2 precision_bits), and quantization(n_c) = n_c 2^precision_bits; with
 * precision_bits >= 32 and VDB_ANN_MAX_VECTORS = 2^24 the two limits before it already imply this one), more than 2^34 cells.  _size takes no cluster; each of its outputs may be NULL. */
int vdb_wit_ann_mean_size(uint32_t precision_bits, uint32_t lookup_bits, size_t K, size_t n_c, size_t dim, uint64_t *cells, uint64_t *lookups,
                          uint64_t *input_cells);
int vdb_wit_ann_mean(uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *centroids, const vdb_fr *members, const vdb_fr *roots, size_t K,
                     size_t cluster, size_t n_c, size_t dim, vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out, uint8_t *mean_ok_out,
                     vdb_fr *public_out);
int vdb_wit_ann_mean_dev(uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *centroids_dev, const vdb_fr *members_dev,
                         const vdb_fr *roots_dev, const vdb_fr *centroid_levels_dev, const vdb_fr *member_levels_dev, size_t K, size_t cluster,
                         size_t n_c, size_t dim, vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, uint8_t *mean_ok_dev,
                         vdb_fr *public_dev);

/* The recentre of ONE cluster c, proved from the old index root to the new one (pipeline.AnnRecentreHotPath): the index under
 * index_root_new has the K cluster roots of the index under index_root_old, and its centroids' tree is the old one with leaf c replaced
 * by the leaf of the vector qdiv(sum of the members committed under cluster_root_c, quantization(n_c)), word for word the quotient
 * vdb_wit_ann_mean accepts.  K such proofs, c = 0 .. K - 1, recentre an index: the memberships do not change between them, so the chain
 * ends on the root of the index built on vdb_ann_cluster_means.  The old centroid c is never assigned: it is the opaque old leaf of
 * the path.  Blocks in stream order:
 *   A - D  the head of vdb_wit_ann_update: header [c | centroids_root | cluster roots], indicators, picked, sponge -> index_root_old
 *   I      assigned members n_c x dim
 *   M      vdb_wit_ann_mean's block M cell for cell: len = load_constant(quantization(n_c)), the qadd chains, one qdiv per word -> mean_j
 *   MM     mroot = merkle_commitment(members) (its padding loads the zero cell: nothing before it has)
 *   U      vdb_wit_merkle_update_ops' block at its base over the centroids' tree (n = K, depth = ceil(log2 K)): one write, no growth
 *   G      the sponge over [U's new root | the header's cluster roots] -> index_root_new
 * Copies (no cell): U's old root copies the header's centroids_root, U's idx copies c, U's assigned new-vector word j copies mean_j
 * (the last cell of quotient j), mroot copies picked, G's word 0 copies U's new root and its words 1 .. K the header's cluster roots.
 * Lookup cells are the qdiv blocks' alone, word j's from j * (qdiv's lookup cells) on.  public, 3 values:
 * [index_root_old | c | index_root_new].  The shape depends on (K, n_c, dim): n_c enters as a constant; c is a witness.
 * centroid_levels: the centroids' tree, 2 lp_K digests (vdb_merkle_tree_build_dev's layout, forest segment K), a copy the caller owns:
 * the call leaves it in the state after the write.  roots: [centroids_root | K cluster roots].  member_levels_dev: cluster c's tree where
 * it is resident (then the launch list does not depend on n_c, and on K only through one kernel per level of U), or NULL.
 * new_centroid: dim words out.  The _dev form honours vdb_wit_set_window; new_centroid, centroid_levels and public are whole in every
 * window.  VDB_ERR_ARG before anything is launched: K == 1 (a centroids' tree of one leaf has no path), K == 0,
 * K > VDB_ANN_MAX_CLUSTERS, cluster >= K, n_c > VDB_ANN_MAX_VECTORS, n_c == 0, dim == 0, dim > 2^20, n_c * dim above
 * VDB_NEAREST_TOPK_MAX_INSTANCES, n_c >= 2^precision_bits, more than 2^34 cells.  _size takes no cluster; each of its outputs may be
 * NULL (update_base: the first cell of U). */
int vdb_wit_ann_recentre_size(uint32_t precision_bits, uint32_t lookup_bits, size_t K, size_t n_c, size_t dim, uint64_t *cells, uint64_t *lookups,
                              uint64_t *input_cells, uint64_t *update_base);
int vdb_wit_ann_recentre(uint32_t precision_bits, uint32_t lookup_bits, vdb_fr *centroid_levels, const vdb_fr *members, const vdb_fr *roots, size_t K,
                         size_t cluster, size_t n_c, size_t dim, vdb_fr *stream_out, vdb_fr *lookup_out, uint8_t *selector_out,
                         vdb_fr *new_centroid_out, vdb_fr *public_out);
int vdb_wit_ann_recentre_dev(uint32_t precision_bits, uint32_t lookup_bits, vdb_fr *centroid_levels_dev, const vdb_fr *members_dev,
                             const vdb_fr *roots_dev, const vdb_fr *member_levels_dev, size_t K, size_t cluster, size_t n_c, size_t dim,
                             vdb_fr *stream_dev, vdb_fr *lookup_dev, uint8_t *selector_dev, vdb_fr *new_centroid_dev, vdb_fr *public_dev);
/* The index after that proof (values only, functional; the old buffers are only read), on buffers of its own and with no rebuild: the
 * grouped rows, slots, offsets and forest segments 0 .. K - 1 are copied device to device, forest segment K is updated_levels_dev (what
 * the witness call left in centroid_levels_dev), row c of the centroids is new_centroid_dev, the K + 2 roots are rewritten and the index
 * root is hashed by one sponge launch.  cluster_sizes: K x uint64, a HOST array.  The result equals vdb_ann_index_build_dev over the
 * same rows with row c of the centroids replaced, buffer for buffer.  VDB_ERR_ARG: K < 2, K > VDB_ANN_MAX_CLUSTERS, cluster >= K, dim
 * outside [1, 2^20], an empty cluster, n above VDB_ANN_MAX_VECTORS. */
int vdb_ann_index_recentre_dev(const vdb_fr *grouped_dev, const uint32_t *slots_dev, const uint64_t *offsets_dev, const vdb_fr *forest_dev,
                               const vdb_fr *roots_dev, const vdb_fr *centroids_dev, const uint64_t *cluster_sizes, size_t K, size_t dim,
                               size_t cluster, const vdb_fr *updated_levels_dev, const vdb_fr *new_centroid_dev, vdb_fr *grouped_out_dev,
                               uint32_t *slots_out_dev, uint64_t *offsets_out_dev, vdb_fr *forest_out_dev, vdb_fr *roots_out_dev,
                               vdb_fr *centroids_out_dev);

/* The cover of the database by the index (pipeline.AnnCoverHotPath): the index under index_root holds exactly the vectors under
 * database_root, with their multiplicities.  The verifying key is fixed by n, K and the cluster sizes n_0 .. n_{K-1} (they sum to n, and
 * are public with it).  Statement: database_root is the root of a merkle_commitment tree over n leaves, index_root is the sponge over
 * [centroids_root | cluster_root_0 .. cluster_root_{K-1}], cluster_root_c is the root of a merkle_commitment tree over n_c leaves, both
 * kinds padded with the zero cell, and the multiset of the n database leaf digests is the union of the multisets of the clusters' leaf
 * digests.  Both commitments use one leaf hash (the sponge of a vector), so the statement is made on leaf digests: no vector is hashed.
 * The multisets are compared by prod (gamma - a_i) = prod (gamma - b_j) at gamma = sponge([database_root, index_root]), a challenge the
 * circuit derives itself (a random-oracle argument: DESIGN 4n).  Blocks in stream order:
 *   A   assigned header [centroids_root | cluster_root_0 .. K-1]                                              K + 1 cells
 *   I   assigned leaf digests a_0 .. a_{n-1} (database slot order), then b_0 .. b_{n-1} (grouped order)      2 n
 *   Z   load_zero, once, where the database tree or a cluster tree is padded                                   0 or 1
 *   TD  the database tree's nodes over a (level-major) -> droot                                                (lp - 1) NODE
 *   TC  the K cluster trees' nodes over their stretches of b, c = 0 .. K - 1 -> root_c (n_c = 1: the leaf)     sum (lp_c - 1) NODE
 *   D   the sponge over the header -> index_root
 *   G   the sponge over [droot, index_root] -> gamma (two words: the cells of a node)
 *   SA  g_sub(gamma, a_i) at SA + 4 i;  MA  g_mul(acc_{i-1}, t_i) at MA + 4 (i - 1), acc_0 = t_0             4 n + 4 (n - 1)
 *   SB, MB  the same over b                                                                                    4 n + 4 (n - 1)
 * NODE = 4,506 cells.  Copies (no cell): the trees' level-0 inputs copy I (padding copies Z), root_c copies the header's cluster_root_c,
 * D's words copy A, G's words copy droot and D's digest, every gamma cell copies G's digest, the a_i / b_j cells of SA / SB copy I, the
 * last accumulator of MA copies the last of MB.  No lookup cell.  public, 2 values: [database_root | index_root].
 * db_leaves / cluster_leaves: n digests each; cluster_sizes: K x uint64, a HOST array; centroids_root: one digest.  The host-array form
 * hashes the K + 1 trees itself (a launch per level and tree).  The _dev form takes the resident trees instead — db_tree_dev
 * (vdb_ann_index_db_tree_dev, 2 lp digests) and forest_dev (vdb_ann_index_build_dev's), both or neither (one alone: VDB_ERR_ARG) — reads
 * every digest where it lies (the two leaf arrays may then be NULL), and its launch list depends on neither K nor n.  It honours
 * vdb_wit_set_window; public is whole in every window.  VDB_ERR_ARG before anything is launched: K == 0, K > VDB_ANN_MAX_CLUSTERS, an
 * empty cluster, n > VDB_ANN_MAX_VECTORS, sizes that do not sum to n, more than 2^34 cells.  Each output of _size may be NULL. */
int vdb_wit_ann_cover_size(const uint64_t *cluster_sizes, size_t K, size_t n, uint64_t *cells, uint64_t *input_cells);
int vdb_wit_ann_cover(const vdb_fr *db_leaves, const vdb_fr *cluster_leaves, const vdb_fr *centroids_root, const uint64_t *cluster_sizes, size_t K,
                      size_t n, vdb_fr *stream_out, uint8_t *selector_out, vdb_fr *public_out);
int vdb_wit_ann_cover_dev(const vdb_fr *db_leaves_dev, const vdb_fr *cluster_leaves_dev, const vdb_fr *centroids_root_dev,
                          const uint64_t *cluster_sizes, size_t K, size_t n, const vdb_fr *db_tree_dev, const vdb_fr *forest_dev,
                          vdb_fr *stream_dev, uint8_t *selector_dev, vdb_fr *public_dev);
/* The database tree of an index, values only: levels_out (2 lp digests, vdb_merkle_tree_build_dev's layout) is the tree over the n
 * vectors in database slot order, bit for bit vdb_merkle_tree_build_dev over the same rows, without hashing a vector: grouped row g's
 * leaf digest is copied from level 0 of its cluster's forest segment to slot slots[g], then the levels are hashed.  cluster_sizes:
 * K x uint64, a HOST array; slots_dev: vdb_ann_index_build_dev's.  VDB_ERR_ARG before anything is launched: K == 0,
 * K > VDB_ANN_MAX_CLUSTERS, n == 0, n > VDB_ANN_MAX_VECTORS, an empty cluster, sizes that do not sum to n; and after the call's one flag
 * read: slots that are no permutation of 0 .. n - 1 (a database with slots no cluster holds; levels_out is then undefined). */
int vdb_ann_index_db_tree_dev(const vdb_fr *forest_dev, const uint64_t *cluster_sizes, const uint32_t *slots_dev, size_t K, size_t n,
                              vdb_fr *levels_out_dev);

/* The means of all K clusters of an index as vdb_ann_index_build_dev leaves it, values only: means[k][j] =
 * qdiv(sum_i member_i[j], quantization(n_k)) over the rows [offsets[k], offsets[k + 1]) of the grouped rows, bit for bit what
 * vdb_wit_ann_mean constrains (the sum is exact in the field, so its order does not matter; the quotient is qdiv's value).  A server
 * recomputes centroids that have drifted after writes and deletes with it, without proving a k-means.  grouped: n x dim; offsets:
 * K + 1 x uint64; means: K x dim.  One launch whatever K and the cluster sizes; the _dev form reads the K + 1 offsets back first and
 * checks them on the host.  VDB_ERR_ARG before anything is launched: K == 0, K > VDB_ANN_MAX_CLUSTERS, dim == 0, dim > 2^20,
 * n > VDB_ANN_MAX_VECTORS, offsets that do not rise from 0 to n, an empty cluster.  VDB_ERR_DOMAIN: a quotient qdiv's value form flags. */
int vdb_ann_cluster_means_dev(uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *grouped_dev, const uint64_t *offsets_dev, size_t n,
                              size_t K, size_t dim, vdb_fr *means_dev);
int vdb_ann_cluster_means(uint32_t precision_bits, uint32_t lookup_bits, const vdb_fr *grouped, const uint64_t *offsets, size_t n, size_t K,
                          size_t dim, vdb_fr *means_out);

/* ---- b4 stream -> columns: replaces halo2-base GateThreadBuilder::assign_all (break points, keygen)
 *      and assign_threads_in (prover) as driven by RangeCircuitBuilder::prover(builder, break_points)
 *      (src/scaffold/mod.rs:393-396).  Columns are 2^k rows; the cell on a break row is duplicated at
 *      row 0 of the next column.  Lookup cells fill dedicated columns of 2^k - minimum_rows cells. ---- */
int vdb_layout_plan(const uint8_t *selector, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t *break_points_out, uint64_t cap,
                    uint64_t *n_break_points);
int vdb_layout_plan_dev(const uint8_t *selector_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t *break_points_out, uint64_t cap,
                        uint64_t *n_break_points);
/* advice_cols_out: (n_bp + 1) x 2^k; lookup_cols_out: n_lookup_cols x 2^k (may be NULL) */
int vdb_layout_columns(const vdb_fr *stream, uint64_t n_cells, const uint64_t *break_points, uint64_t n_bp, const vdb_fr *lookup, uint64_t n_lookup,
                       uint32_t k, uint32_t minimum_rows, vdb_fr *advice_cols_out, vdb_fr *lookup_cols_out, uint64_t n_lookup_cols);
/* device variants; blind_dev (optional): n_cols x n_blind scalars written to the last n_blind rows
 * (the prover's blinding rows) */
int vdb_layout_columns_dev(const vdb_fr *stream_dev, uint64_t n_cells, const uint64_t *break_points, uint64_t n_bp, uint32_t k, vdb_fr *cols_dev,
                           const vdb_fr *blind_dev, uint32_t n_blind);
int vdb_layout_lookup_dev(const vdb_fr *lookup_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, vdb_fr *cols_dev, uint64_t n_cols,
                          const vdb_fr *blind_dev, uint32_t n_blind);
/* Columns without the copy.  A vdb_colsrc describes one column that still lies in a witness stream: rows [0, len) are the
 * contiguous cells src[0 .. len), the last n_blind rows come from `blind` (may be NULL), every other row is zero — exactly
 * what vdb_layout_columns[_range]_dev / vdb_layout_lookup[_range]_dev would have written.  The commitment MSM
 * (vdb_msm_batch_src_dev_begin) and the first pass of lagrange_to_coeff (vdb_lagrange_to_coeff_src_dev, which writes the
 * coefficient columns) read through it, so the 64 B / cell of the layout copy disappear from the prover's step.  The
 * descriptors are data independent: build them once per circuit.  out_dev: (col_hi - col_lo) descriptors in device memory.
 * The cells and the blinding rows of a column do not overlap: both readers take a row below len from the stream before they look
 * at the blinding rows, so with blind_dev given the builders refuse a column with len + n_blind > 2^k (VDB_ERR_ARG, nothing is
 * written) — a layout planned with minimum_rows >= n_blind never has one.  Without blind_dev a column may be 2^k cells long.
 * A caller that writes descriptors itself keeps len + n_blind <= n where blind is set. */
typedef struct {
  const vdb_fr *src;
  uint64_t len;
  const vdb_fr *blind;
} vdb_colsrc;
int vdb_colsrc_build_dev(const vdb_fr *stream_dev, uint64_t n_cells, const uint64_t *break_points, uint64_t n_bp, uint32_t k, uint64_t col_lo,
                         uint64_t col_hi, const vdb_fr *blind_dev, uint32_t n_blind, vdb_colsrc *out_dev);
int vdb_colsrc_build_lookup_dev(const vdb_fr *lookup_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t col_lo, uint64_t col_hi,
                                const vdb_fr *blind_dev, uint32_t n_blind, vdb_colsrc *out_dev);
/* same, restricted to columns [col_lo, col_hi) (multi-GPU column shards); cols_dev holds just that range; blind_dev is
 * still indexed by absolute column */
int vdb_layout_columns_range_dev(const vdb_fr *stream_dev, uint64_t n_cells, const uint64_t *break_points, uint64_t n_bp, uint32_t k, uint64_t col_lo,
                                 uint64_t col_hi, vdb_fr *cols_dev, const vdb_fr *blind_dev, uint32_t n_blind);
int vdb_layout_lookup_range_dev(const vdb_fr *lookup_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t col_lo, uint64_t col_hi,
                                vdb_fr *cols_dev, const vdb_fr *blind_dev, uint32_t n_blind);
/* keygen side: column-layout image ((n_bp + 1) x 2^k bytes) of the constant-cell flags (bit 1 of the flag bytes) */
int vdb_layout_const_mask_dev(const uint8_t *flags_dev, uint64_t n_cells, const uint64_t *break_points, uint64_t n_bp, uint32_t k, uint8_t *mask_dev);
/* out = mask ? in : 0 (keep_const = 1) or mask ? 0 : in (keep_const = 0), elementwise over n field elements */
int vdb_mask_select_dev(const vdb_fr *in_dev, const uint8_t *mask_dev, uint64_t n, int keep_const, vdb_fr *out_dev);

/* ---- b1 SRS: replaces halo2 ParamsKZG::{get_g, g_lagrange} as consumed by commit / commit_lagrange;
 *      the reference obtains the params with gen_srs(k) (src/scaffold/mod.rs:260) ------------------ */
/* Uploads the bases (caller keeps ownership of the host arrays; either may be NULL) and precomputes
 * the fixed-base window tables 2^(c*j) * G_i in HBM. */
int vdb_srs_load(uint32_t k, const vdb_g1 *g, const vdb_g1 *g_lagrange, vdb_srs **out);
/* the same with an explicit Pippenger window (2..14 bits; 0 = the default, 11 bits for k > 8, tuned for witness columns whose
 * scalars are mostly short).  Columns of full-width scalars (Poseidon traces, the product columns of the permutation and
 * lookup arguments, quotient and opening polynomials) commit ~15 % faster with 14 bits: 19 windows instead of 24. */
int vdb_srs_load_window(uint32_t k, const vdb_g1 *g, const vdb_g1 *g_lagrange, uint32_t window_bits, vdb_srs **out);
/* "unsafe" trusted setup with a caller-supplied tau, the construction ParamsKZG::setup performs behind
 * gen_srs(k) (src/scaffold/mod.rs:260-261: "unsafe" message); tau is a Montgomery Fr.  Test/bench SRS. */
int vdb_srs_setup_unsafe(uint32_t k, const vdb_fr *tau, vdb_g1 *g_out, vdb_g1 *g_lagrange_out);
/* A params file instead of a known tau: what halo2-base's gen_srs(k) reads from params/kzg_bn254_{k}.srs when the file exists
 * (src/scaffold/mod.rs:260), typically one ceremony file cut down with ParamsKZG::downsize(k).
 * vdb_g1_check_dev replaces the point checks of halo2's SerdeFormat::RawBytes reader (ParamsKZG::read): both coordinates below q
 * (as the raw Montgomery words) and y^2 = x^3 + 3, (0, 0) accepted as the identity.  *n_bad: the number of points that fail;
 * *first_bad: the lowest index among them (n when none fails).  Blocks until done. */
int vdb_g1_check_dev(const vdb_g1 *pts_dev, size_t n, uint64_t *n_bad, uint64_t *first_bad);
/* Replaces halo2's g_to_lagrange (ParamsKZG::downsize: best_fft over G1 with omega^-1, times n^-1, batch_normalize):
 * g_lagrange[i] = n^-1 sum_j omega^(-ij) g[j] for n = 2^k arbitrary affine points (identity allowed), omega =
 * vdb_fr_root_of_unity(k); canonical affine out, identity (0, 0).  k = 1 .. 26; the two buffers may be the same.  Blocks until
 * done (its work buffers, 2 x 128 B per point, are released before it returns). */
int vdb_g1_lagrange_from_monomial_dev(uint32_t k, const vdb_g1 *g_dev, vdb_g1 *g_lagrange_dev);
/* ParamsKZG::downsize(k) for a host caller: g_host holds at least 2^k monomial points (the first 2^k of a longer g are used),
 * g_lagrange_out receives the 2^k Lagrange points.  g itself is the prefix of the longer one. */
int vdb_srs_downsize(uint32_t k, const vdb_g1 *g_host, vdb_g1 *g_lagrange_out);
void vdb_srs_free(vdb_srs *srs);
/* out[c] = parts[0][c] + ... + parts[m-1][c] in G1 (host arrays, m x n and n affine points; the identity is (0, 0)): the
 * combine step of a point-sharded MSM — each GPU commits its slice of the rows of every column against the matching slice of
 * the bases, the partial commitments are all-gathered and added.  RCCL has no curve reduction operator. */
int vdb_g1_sum(const vdb_g1 *parts, size_t m, size_t n, vdb_g1 *out);
int vdb_srs_device(const vdb_srs *srs, int *device); /* the device whose HBM holds the handle's tables */
int vdb_srs_info(const vdb_srs *srs, uint32_t *k, uint32_t *window_bits, uint32_t *windows);

/* ---- b2 MSM: replaces halo2 arithmetic::best_multiexp(&[Fr], &[G1Affine]) -> G1 and
 *      ParamsKZG::commit_lagrange / commit (reached from src/scaffold/mod.rs:296, :273).
 *      basis: 0 = monomial (g), 1 = lagrange (g_lagrange).  Result: exact group element as canonical
 *      affine, identity = (0,0).  n <= 2^k scalars use the first n bases. ------------------------- */
int vdb_msm(const vdb_srs *srs, int basis, const vdb_fr *scalars, size_t n, vdb_g1 *out);
int vdb_msm_batch(const vdb_srs *srs, int basis, const vdb_fr *const *cols, size_t n_cols, size_t n, vdb_g1 *out);
/* The same over every device bound by vdb_init_devices (columns are independent, the bases are replicated):
 * vdb_srs_load_all builds one handle per bound device (out[i] belongs to the i-th bound device, n_out = vdb_devices_bound());
 * vdb_msm_batch_multi gives device i the i-th contiguous block of the columns, one host thread per device, results D2H into
 * out[] in column order.  With one bound device they reduce to the calls above. */
int vdb_srs_load_all(uint32_t k, const vdb_g1 *g, const vdb_g1 *g_lagrange, uint32_t window_bits, vdb_srs **out, int n_out);
int vdb_msm_batch_multi(vdb_srs *const *srs, int n_srs, int basis, const vdb_fr *const *cols, size_t n_cols, size_t n, vdb_g1 *out);
/* scalars_dev: contiguous n_cols x n in HBM; out_host: n_cols points */
int vdb_msm_batch_dev(const vdb_srs *srs, int basis, const vdb_fr *scalars_dev, size_t n_cols, size_t n, vdb_g1 *out_host);
/* Deferred form of vdb_msm_batch[_masked]_dev (mask and constant points may both be NULL): _begin queues the whole MSM and
 * returns without waiting; the bucket folding of its last batch — short, latency-bound launches — runs on a second
 * stream, so work queued next (vdb_lagrange_to_coeff_dev / vdb_coeff_to_extended_dev on the same columns: the scalars
 * are no longer read) overlaps it.  _end waits FOR THE MSM ONLY and copies the n_cols commitments out: what was queued on the
 * library's stream after _begin may still be running when it returns (the caller feeds the commitments to its transcript
 * while the transforms run; vdb_sync() or any blocking call joins).  One deferred MSM at a time: while one is open every other
 * MSM (a second _begin, vdb_msm_batch[_masked]_dev) returns VDB_ERR_ARG and leaves the open one as it is; _end(NULL, 0) drops it. */
int vdb_msm_batch_masked_dev_begin(const vdb_srs *srs, int basis, const vdb_fr *scalars_dev, size_t n_cols, size_t n, const uint8_t *skip_mask_dev,
                                   const vdb_g1 *const_points_dev);
/* same for columns described by vdb_colsrc (n rows each, the last n_blind of them blinding rows) */
int vdb_msm_batch_src_dev_begin(const vdb_srs *srs, int basis, const vdb_colsrc *src_dev, size_t n_cols, size_t n, uint32_t n_blind,
                                const uint8_t *skip_mask_dev, const vdb_g1 *const_points_dev);
int vdb_msm_batch_end(vdb_g1 *out_host, size_t n_cols);
/* per column: the number of (scalar, window) entries vdb_msm_batch[_masked]_dev would sort and accumulate for it (non-zero
 * signed digits of the cells not flagged in skip_mask_dev, which may be NULL).  A keygen-time statistic used to balance
 * column shards across GPUs.  counts_out: host, n_cols values. */
int vdb_msm_count_entries_dev(const vdb_srs *srs, const vdb_fr *scalars_dev, size_t n_cols, size_t n, const uint8_t *skip_mask_dev,
                              uint64_t *counts_out);
/* Prover-side commit with the constant cells factored out: cells flagged in skip_mask_dev (n_cols x n bytes, from
 * vdb_layout_const_mask_dev) are skipped and const_points_dev[col] — the keygen-time MSM of exactly those cells
 * (vdb_mask_select_dev(keep_const = 1) + vdb_msm_batch_dev) — is added.  Same group element as vdb_msm_batch_dev. */
int vdb_msm_batch_masked_dev(const vdb_srs *srs, int basis, const vdb_fr *scalars_dev, size_t n_cols, size_t n, const uint8_t *skip_mask_dev,
                             const vdb_g1 *const_points_dev, vdb_g1 *out_host);

/* ---- b3 NTT: replaces halo2 arithmetic::best_fft / EvaluationDomain::{lagrange_to_coeff,
 *      coeff_to_extended} (reached from src/scaffold/mod.rs:296) ------------------------------ */
#define VDB_NTT_INVERSE_SCALE 1 /* multiply the result by n^{-1} (EvaluationDomain::ifft) */
/* In place on each column; natural order in, natural order out; X[i] = sum_j a[j] omega^(ij). */
int vdb_ntt_batch(vdb_fr *const *cols, size_t n_cols, uint32_t log_n, const vdb_fr *omega, int flags);
/* the same with the columns cut into one contiguous block per bound device (vdb_init_devices), one host thread each */
int vdb_ntt_batch_multi(vdb_fr *const *cols, size_t n_cols, uint32_t log_n, const vdb_fr *omega, int flags);
/* contiguous device buffer of n_cols columns of 2^log_n elements */
int vdb_ntt_batch_dev(vdb_fr *cols_dev, size_t n_cols, uint32_t log_n, const vdb_fr *omega, int flags);
/* lagrange_to_coeff for the 2^k domain (omega = ROOT_OF_UNITY^(2^(28-k))) */
int vdb_lagrange_to_coeff(vdb_fr *const *cols, size_t n_cols, uint32_t k);
int vdb_lagrange_to_coeff_dev(vdb_fr *cols_dev, size_t n_cols, uint32_t k);
/* lagrange_to_coeff of columns described by vdb_colsrc: reads the witness stream, writes n_cols coefficient columns of
 * 2^k elements to coeff_dev (k > 10) */
int vdb_lagrange_to_coeff_src_dev(const vdb_colsrc *src_dev, vdb_fr *coeff_dev, size_t n_cols, uint32_t k, uint32_t n_blind);
/* Batched grand product of the permutation / lookup arguments (the first prover-round primitive after
 * commit + NTT): per column of n entries z[0] = 1, z[i + 1] = z[i] * num[i] / den[i] (i < n - 1).  A zero denominator
 * inverts to zero like halo2's batch_invert, i.e. z is zero from that row on.  One field inversion per column.
 * num_dev, den_dev, z_dev: n_cols x n, column-major contiguous, device memory. */
int vdb_grand_product_dev(const vdb_fr *num_dev, const vdb_fr *den_dev, size_t n_cols, size_t n, vdb_fr *z_dev);
/* out[c] = sum_i coeff[c][i] * x^i for n_cols coefficient-form polynomials of n coefficients (halo2 eval_polynomial, the
 * opening evaluations of the advice polynomials).  coeff_dev: device; x: one field element on the host; out_host: host. */
int vdb_eval_polys_dev(const vdb_fr *coeff_dev, size_t n_cols, size_t n, const vdb_fr *x, vdb_fr *out_host);
/* the same queued only: the n_cols values go to out_dev, nothing is waited for (the caller reads them with vdb_memcpy_d2h, which is
 * ordered behind the kernel, and may queue the next evaluation before it turns to the host side of the previous one) */
int vdb_eval_polys_dev_out(const vdb_fr *coeff_dev, size_t n_cols, size_t n, const vdb_fr *x, vdb_fr *out_dev);
/* Lookup argument, permuted columns (halo2 plonk/lookup/prover.rs permute_expression_pair) for range-table lookups: per
 * input column, over rows [0, usable_rows): permuted_input = the input values in ascending canonical order;
 * permuted_table = at the first row of every run of equal values that value, elsewhere the table's left-over values in
 * ascending order assigned from the last repeated row backwards; rows >= usable_rows are zeroed (the caller adds the
 * blinding rows).  All values must be canonical integers below 2^max_bits (max_bits <= 20: a counting sort) and every
 * input value must occur in the table, otherwise VDB_ERR_DOMAIN (the reference panics).
 * input_dev, permuted_*_dev: n_cols x n; table_dev: one column of n. */
int vdb_lookup_permute_dev(const vdb_fr *input_dev, const vdb_fr *table_dev, size_t n_cols, size_t n, size_t usable_rows, uint32_t max_bits,
                           vdb_fr *permuted_input_dev, vdb_fr *permuted_table_dev);
/* Lookup argument, running product (halo2 plonk/lookup/prover.rs commit_product): per input column z[0] = 1,
 * z[i + 1] = z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)) for i < usable_rows, rows above usable_rows zero
 * (the caller blinds them).  A, A', S': n_cols x n; S (the table): one column of n.  z[usable_rows] is one exactly when
 * (A', S') is a valid permutation pair of (A, S). */
int vdb_lookup_product_dev(const vdb_fr *input_dev, const vdb_fr *table_dev, const vdb_fr *perm_input_dev, const vdb_fr *perm_table_dev, size_t n_cols, size_t n,
                           size_t usable_rows, const vdb_fr *beta, const vdb_fr *gamma, vdb_fr *z_dev);
/* Permutation argument.  halo2curves' Fr::DELTA = 7^(2^28). */
int vdb_fr_delta(vdb_fr *out);
/* keygen side (halo2 plonk/permutation/keygen.rs build_pk: the sigma columns in Lagrange form): sigma[c][row] =
 * delta^c' omega^row' for the cell (c', row') that the copy-constraint permutation sends (c, row) to;
 * mapping_dev: n_cols x 2^k words c' << 32 | row' (the identity where a cell is unconstrained). */
int vdb_permutation_sigma_dev(const uint64_t *mapping_dev, size_t n_cols, uint32_t k, const vdb_fr *delta, vdb_fr *sigma_dev);
/* The mapping kept with the proving key in 32 bits per cell (c' << k | row'; VDB_ERR_ARG when column and row do not fit), and the
 * sigma columns of a block of columns in Lagrange form straight from it: halo2's ProvingKey holds the permutation polynomials in
 * Lagrange, coefficient and coset form (plonk/permutation.rs ProvingKey: permutations, polys, cosets); here the coefficient form
 * is held, the cosets are made per block in the quotient, and the Lagrange form the product round reads costs one product per
 * cell from these 4 bytes instead of a forward transform per column.  packed_block_dev: the block's n_block_cols x 2^k words. */
int vdb_permutation_mapping_pack_dev(const uint64_t *mapping_dev, size_t n_cols, uint32_t k, uint32_t *packed_dev);
int vdb_permutation_sigma_packed_dev(const uint32_t *packed_block_dev, size_t n_block_cols, size_t n_cols_total, uint32_t k, const vdb_fr *delta,
                                     vdb_fr *sigma_block_dev);
/* prover side (plonk/permutation/prover.rs commit): the columns are taken in chunks of chunk_len (= constraint degree - 2);
 * per chunk one product column z with z[i + 1] = z[i] prod_c (v_c[i] + beta delta^c omega^i + gamma) / (v_c[i] + beta
 * sigma_c[i] + gamma) over the chunk's columns c, i < usable_rows; chunk j starts from the value chunk j - 1 ended on
 * (z_0[0] = 1); rows above usable_rows are zero (the caller blinds them).  The last chunk's z[usable_rows] is one
 * exactly when every cell equals the cell the permutation sends it to (up to the soundness error in beta, gamma).
 * cols_dev, sigma_dev: n_cols x 2^k; z_dev: ceil(n_cols / chunk_len) x 2^k. */
int vdb_permutation_product_dev(const vdb_fr *cols_dev, const vdb_fr *sigma_dev, size_t n_cols, uint32_t k, size_t usable_rows, size_t chunk_len,
                                const vdb_fr *beta, const vdb_fr *gamma, const vdb_fr *delta, vdb_fr *z_dev);
/* Permutation and lookup parts of the quotient numerator on the extended coset of 2^(k+ext_k) points (halo2
 * plonk/evaluation.rs evaluate_h), folded into acc_dev term by term as acc = acc * y + term, after the gates
 * (vdb_gate_eval_dev).  All *_ext_dev arrays are vdb_coeff_to_extended_dev images: the advice, sigma and product columns;
 * l0 (Lagrange basis of row 0), l_last (row usable_rows), l_active = 1 - (l_last + sum of the rows above usable_rows).
 * Permutation terms: l0 (1 - z_0); l_last (z_last^2 - z_last); l0 (z_i - z_{i-1}(w^-(n-usable_rows) X)) for i >= 1; per chunk
 * l_active (z_i(wX) prod (v + beta sigma + gamma) - z_i(X) prod (v + delta^c beta X + gamma)).
 * Lookup terms per input column: l0 (1 - z); l_last (z^2 - z); l_active (z(wX)(A' + beta)(S' + gamma) - z (A + beta)(S + gamma));
 * l0 (A' - S'); l_active (A' - S')(A' - A'(w^-1 X)). */
int vdb_permutation_eval_dev(const vdb_fr *adv_ext_dev, const vdb_fr *sigma_ext_dev, const vdb_fr *z_ext_dev, size_t n_cols, size_t chunk_len, uint32_t k,
                             uint32_t ext_k, size_t usable_rows, const vdb_fr *l0_ext_dev, const vdb_fr *l_last_ext_dev, const vdb_fr *l_active_ext_dev,
                             const vdb_fr *beta, const vdb_fr *gamma, const vdb_fr *delta, const vdb_fr *y, vdb_fr *acc_dev);
/* the same for the sets [set_lo, set_hi) only (the terms that involve nothing but the product columns come with set_lo == 0):
 * sigma_ext_block_dev holds the cosets of columns set_lo * chunk_len onwards, so that the sigma cosets can be produced block
 * by block from their coefficients instead of being kept resident; calls must be made in ascending order of the sets. */
int vdb_permutation_eval_range_dev(const vdb_fr *adv_ext_dev, const vdb_fr *sigma_ext_block_dev, const vdb_fr *z_ext_dev, size_t n_cols, size_t chunk_len,
                                   uint32_t k, uint32_t ext_k, size_t usable_rows, const vdb_fr *l0_ext_dev, const vdb_fr *l_last_ext_dev,
                                   const vdb_fr *l_active_ext_dev, const vdb_fr *beta, const vdb_fr *gamma, const vdb_fr *delta, const vdb_fr *y, vdb_fr *acc_dev,
                                   size_t set_lo, size_t set_hi);
/* Streaming forms for circuits whose columns do not all fit HBM at once (the rounds then work on blocks of columns):
 * vdb_permutation_product_range_dev: the running products of the chunks of ONE block of columns (cols_block / sigma_block hold
 * columns col0 .. col0 + n_block_cols, col0 a multiple of chunk_len), each starting from one; vdb_permutation_chain_dev then
 * puts all chunks of all blocks on one chain (z_c starts where z_{c-1} ended), as vdb_permutation_product_dev does in one go.
 * vdb_permutation_eval_parts_dev: the permutation part of the quotient numerator with block buffers — adv_ext_block holds the
 * cosets of columns adv_col0 .., z_ext_block those of product sets z_set0 .., z_first / z_last the cosets of the first and last
 * set; `head` bit 0: fold in l0 (1 - z_0) and l_last (z_last^2 - z_last); bit 1: sigma_ext_block holds the cosets of beta sigma(X)
 * (vdb_coeff_to_extended_scaled_dev) and the kernel skips its product by beta; [chain_lo, chain_hi): fold in l0 (z_i - z_{i-1}(..)) for these
 * sets (reads sets chain_lo - 1 .. chain_hi - 1); [set_lo, set_hi): fold in the product terms of these sets (reads their columns,
 * sigma_ext_block starting at column set_lo * chunk_len).  Terms must be folded in the order head, chain 1 .. n_sets - 1, products
 * 0 .. n_sets - 1 to agree with the resident form. */
int vdb_permutation_product_range_dev(const vdb_fr *cols_block_dev, const vdb_fr *sigma_block_dev, size_t n_block_cols, size_t col0, uint32_t k,
                                      size_t usable_rows, size_t chunk_len, const vdb_fr *beta, const vdb_fr *gamma, const vdb_fr *delta, vdb_fr *z_block_dev);
int vdb_permutation_chain_dev(vdb_fr *z_dev, size_t n_chunks, uint32_t k, size_t usable_rows);
int vdb_permutation_eval_parts_dev(const vdb_fr *adv_ext_block_dev, size_t adv_col0, const vdb_fr *sigma_ext_block_dev, const vdb_fr *z_ext_block_dev, size_t z_set0,
                                   const vdb_fr *z_first_ext_dev, const vdb_fr *z_last_ext_dev, size_t n_cols, size_t chunk_len, uint32_t k, uint32_t ext_k,
                                   size_t usable_rows, const vdb_fr *l0_ext_dev, const vdb_fr *l_last_ext_dev, const vdb_fr *l_active_ext_dev, const vdb_fr *beta,
                                   const vdb_fr *gamma, const vdb_fr *delta, const vdb_fr *y, vdb_fr *acc_dev, int head, size_t chain_lo, size_t chain_hi,
                                   size_t set_lo, size_t set_hi);
int vdb_lookup_eval_dev(const vdb_fr *input_ext_dev, const vdb_fr *table_ext_dev, const vdb_fr *perm_input_ext_dev, const vdb_fr *perm_table_ext_dev,
                        const vdb_fr *z_ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k, const vdb_fr *l0_ext_dev, const vdb_fr *l_last_ext_dev,
                        const vdb_fr *l_active_ext_dev, const vdb_fr *beta, const vdb_fr *gamma, const vdb_fr *y, vdb_fr *acc_dev);
/* rows [from_row, n) of each of the n_cols columns <- src_dev (n_cols x (n - from_row) values): the blinding rows of the
 * columns the prover derives (permuted columns, product columns) */
int vdb_fill_rows_dev(vdb_fr *cols_dev, size_t n_cols, size_t n, size_t from_row, const vdb_fr *src_dev);
/* Opening proofs (halo2 poly/kzg/multiopen: both GWC and SHPLONK are built from these two steps and a commit).
 * vdb_poly_lincomb_dev: acc <- Horner over the n_cols polynomials, acc = acc * v + p_c, coefficient by coefficient (acc_dev:
 * n coefficients, read and written; zero it first).
 * vdb_kate_div_dev (arithmetic::kate_division): per polynomial of n coefficients q(X) = (p(X) - p(x)) / (X - x), n coefficients
 * written (the top one zero); rem_host (may be NULL) receives p(x).  Dividing by a product of linear factors — the vanishing
 * polynomial of a SHPLONK rotation set — is this call once per point. */
/* acc <- acc + a * x over n coefficients (SHPLONK's linearisation polynomial is a sum of polynomials with unrelated scalars) */
int vdb_poly_axpy_dev(vdb_fr *acc_dev, const vdb_fr *a, const vdb_fr *x_dev, size_t n);
/* x <- a * x over n elements.  The sharded prover rounds use it for what a rank does not hold: a fold acc <- acc y + term that
 * skips g terms of other ranks is acc <- y^g acc, and a rank's running products start from the product of all earlier ranks'. */
int vdb_poly_scale_dev(vdb_fr *x_dev, const vdb_fr *a, size_t n);
int vdb_poly_lincomb_dev(const vdb_fr *polys_dev, size_t n_cols, size_t n, const vdb_fr *v, vdb_fr *acc_dev);
int vdb_kate_div_dev(const vdb_fr *coeff_dev, size_t n_cols, size_t n, const vdb_fr *x, vdb_fr *quot_dev, vdb_fr *rem_host);
/* coeff_to_extended: zeta-coset scaling [1, ZETA, ZETA^2] cyclic, zero-extend to 2^(k+ext_k), forward NTT */
int vdb_coeff_to_extended(const vdb_fr *const *coeff_cols, vdb_fr *const *ext_cols, size_t n_cols, uint32_t k, uint32_t ext_k);
int vdb_coeff_to_extended_dev(const vdb_fr *coeff_dev, vdb_fr *ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k);
/* the coset image of scale * p(X): the scalar rides on the coset factors of the transform's first pass (a third of a product per
 * coefficient) — how the quotient takes beta sigma(X) instead of multiplying every point of every sigma coset by beta */
int vdb_coeff_to_extended_scaled_dev(const vdb_fr *coeff_dev, vdb_fr *ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k, const vdb_fr *scale);
/* EvaluationDomain::extended_to_coeff without the final truncation (the way back for h(X)): in place, per
 * column of 2^(k+ext_k) evaluations on the extended coset -> the 2^(k+ext_k) coefficients. */
int vdb_extended_to_coeff_dev(vdb_fr *ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k);
/* Gate part of the quotient numerator for halo2-base's vertical gate q * (a + b * c - d) with a, b, c, d in
 * four consecutive rows of one advice column: acc[j] <- Horner over the n_cols columns of (acc * y + q_c[j] * gate_c[j]) on
 * the extended coset of 2^(k+ext_k) points.  adv_ext_dev, sel_ext_dev: n_cols x 2^(k+ext_k) (vdb_coeff_to_extended_dev of
 * the advice and selector polynomials); acc_dev: 2^(k+ext_k), read and written (zero it before the first call). */
int vdb_gate_eval_dev(const vdb_fr *adv_ext_dev, const vdb_fr *sel_ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k, const vdb_fr *y, vdb_fr *acc_dev);
/* The same on a sub-coset: the gate has degree 3, so its share of the quotient, (sum of the gate terms) / (X^n - 1), has degree
 * below 2 n and is determined by the coset of 2^(k+ext_k) points that lies inside the 2^(k+adv_ext_k) points the advice cosets were
 * made for (every 2^(adv_ext_k-ext_k)-th point: halo2's extended domain is sized for the highest-degree term, here the
 * permutation's, and evaluates every term on all of it).  adv_ext_dev: n_cols x 2^(k+adv_ext_k); sel_ext_dev: n_cols x
 * 2^(k+ext_k) (vdb_coeff_to_extended_dev with ext_k: half the transform); acc_dev: 2^(k+ext_k).  The caller divides by the
 * vanishing polynomial on the small coset, returns to coefficients there and adds them to the quotient's. */
int vdb_gate_eval_sub_dev(const vdb_fr *adv_ext_dev, uint32_t adv_ext_k, const vdb_fr *sel_ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k,
                          const vdb_fr *y, vdb_fr *acc_dev);
/* EvaluationDomain::divide_by_vanishing_poly: h[j] /= (X^n - 1) at the j-th point of the extended coset, in place. */
int vdb_divide_by_vanishing_dev(vdb_fr *h_ext_dev, uint32_t k, uint32_t ext_k);
/* ---- The extended domain coset by coset (round 3).  halo2 evaluates the quotient's numerator on all 2^(k+2) points of the extended
 *      domain (EvaluationDomain::coeff_to_extended, reached from src/scaffold/mod.rs:296) although the quotient of the reference's
 *      circuits has degree below 3 n (constraint degree 4: three pieces) and the gates' share degree below 2 n: three of the four
 *      cosets g_t H of the 2^k-th roots of unity H determine it, two the gates' share.  "Slot" t of a polynomial is its image on
 *      g_t H, g_t = zeta w_{4n}^(bitrev2(t)): slot t, row r is point 4 r + bitrev2(t) of vdb_coeff_to_extended_dev's output, slots
 *      0 and 1 together the coset of 2 n points.  Arrays are [column][slot][row]; a rotation by one row is one step inside a slot.
 *      The quotient that comes out is the same polynomial, coefficient for coefficient.
 * vdb_coeff_to_cosets_dev: n_slots (1..4) cosets of each of n_cols polynomials of 2^k coefficients, times *scale_or_null if given
 *      (the scalar rides on the transform's input factors); one 2^k-point transform per slot instead of a 2^(k+2)-point one.
 * vdb_cosets_to_coeff_dev: the way back for ONE polynomial and the division by the vanishing polynomial in one: cosets_dev
 *      ([n_slots][2^k], overwritten) holds numerator values; coeff_dev receives the n_slots pieces of 2^k coefficients of
 *      numerator / (X^n - 1), which the caller asserts to have degree below n_slots 2^k (residues modulo X^n - g_t^n, then the
 *      Vandermonde system in g_t^n).
 * vdb_gate_eval_cosets_dev / vdb_lookup_eval_cosets_dev / vdb_permutation_eval_parts_cosets_dev: vdb_gate_eval_sub_dev /
 *      vdb_lookup_eval_dev / vdb_permutation_eval_parts_dev on such arrays — n_slots where those take ext_k; the advice cosets of the
 *      gate call may hold more slots per column (adv_slots) than the selectors' and the accumulator's n_slots. */
int vdb_coeff_to_cosets_dev(const vdb_fr *coeff_dev, vdb_fr *cosets_dev, size_t n_cols, uint32_t k, uint32_t n_slots, const vdb_fr *scale_or_null);
int vdb_cosets_to_coeff_dev(vdb_fr *cosets_dev, vdb_fr *coeff_dev, uint32_t k, uint32_t n_slots);
int vdb_gate_eval_cosets_dev(const vdb_fr *adv_cosets_dev, uint32_t adv_slots, const vdb_fr *sel_cosets_dev, size_t n_cols, uint32_t k, uint32_t n_slots,
                             const vdb_fr *y, vdb_fr *acc_dev);
int vdb_lookup_eval_cosets_dev(const vdb_fr *input_dev, const vdb_fr *table_dev, const vdb_fr *perm_input_dev, const vdb_fr *perm_table_dev, const vdb_fr *z_dev,
                               size_t n_cols, uint32_t k, uint32_t n_slots, const vdb_fr *l0_dev, const vdb_fr *l_last_dev, const vdb_fr *l_active_dev,
                               const vdb_fr *beta, const vdb_fr *gamma, const vdb_fr *y, vdb_fr *acc_dev);
int vdb_permutation_eval_parts_cosets_dev(const vdb_fr *adv_block_dev, size_t adv_col0, const vdb_fr *sigma_block_dev, const vdb_fr *z_block_dev, size_t z_set0,
                                          const vdb_fr *z_first_dev, const vdb_fr *z_last_dev, size_t n_cols, size_t chunk_len, uint32_t k, uint32_t n_slots,
                                          size_t usable_rows, const vdb_fr *l0_dev, const vdb_fr *l_last_dev, const vdb_fr *l_active_dev, const vdb_fr *beta,
                                          const vdb_fr *gamma, const vdb_fr *delta, const vdb_fr *y, vdb_fr *acc_dev, int head, size_t chain_lo, size_t chain_hi,
                                          size_t set_lo, size_t set_hi);
/* column-layout image of the gate selectors as field elements (keygen side; flags as for vdb_layout_const_mask_dev, bit 0):
 * q_dev: (n_bp + 1) x 2^k, one where a gate starts. */
int vdb_layout_selectors_dev(const uint8_t *flags_dev, uint64_t n_cells, const uint64_t *break_points, uint64_t n_bp, uint32_t k, vdb_fr *q_dev);
int vdb_fr_root_of_unity(uint32_t k, vdb_fr *out);

/* ---- f2 Fiat–Shamir transcript + proof byte stream: stands in for snark_verifier's PoseidonTranscript<NativeLoader, _>
 *      (src/scaffold/mod.rs:309-310) and the proof writer behind gen_snark_shplonk (src/scaffold/mod.rs:296).  Host code.
 *      Poseidon sponge of width t (the reference's transcript: t = 5, r_f = 8, r_p = 60 [UPSTREAM-RECALL]); values are
 *      buffered and absorbed at the next squeeze, which returns state[1]; `write_*` = `common_*` + append to the proof
 *      (points: 32 bytes, x little-endian, bit 6 of the last byte = y odd; scalars: 32 bytes little-endian canonical). */
typedef struct vdb_transcript vdb_transcript;
int vdb_transcript_new(uint32_t t, uint32_t r_f, uint32_t r_p, vdb_transcript **out);
/* where a compressed point carries "y is odd": bit 6 (default; halo2curves >= 0.4 as recalled) or bit 7 (halo2curves 0.3.x) of the
 * last byte — parity unpinned either way, the reference holds no proof bytes */
int vdb_transcript_set_sign_bit(vdb_transcript *tr, uint32_t bit);
void vdb_transcript_free(vdb_transcript *tr);
int vdb_transcript_common_scalar(vdb_transcript *tr, const vdb_fr *s);
int vdb_transcript_common_point(vdb_transcript *tr, const vdb_g1 *p);
int vdb_transcript_write_scalar(vdb_transcript *tr, const vdb_fr *s);
int vdb_transcript_write_point(vdb_transcript *tr, const vdb_g1 *p);
/* the same over arrays (one call per round instead of one per column) */
int vdb_transcript_write_points(vdb_transcript *tr, const vdb_g1 *p, size_t n);
int vdb_transcript_write_scalars(vdb_transcript *tr, const vdb_fr *s, size_t n);
int vdb_transcript_common_points(vdb_transcript *tr, const vdb_g1 *p, size_t n);
/* the public inputs of a proof: halo2's create_proof absorbs every instance value with common_scalar before anything else */
int vdb_transcript_common_scalars(vdb_transcript *tr, const vdb_fr *s, size_t n);
int vdb_transcript_squeeze(vdb_transcript *tr, vdb_fr *out);
/* absorbs the complete RATE-sized chunks written so far (same state as leaving them to the next squeeze): lets a caller run the
 * sponge's host work beside device work that is already queued */
int vdb_transcript_flush(vdb_transcript *tr);
int vdb_transcript_proof_len(const vdb_transcript *tr, size_t *len);
int vdb_transcript_proof_bytes(const vdb_transcript *tr, uint8_t *out, size_t cap);

/* ---- keygen: the permutation of the copy constraints, on the device.  Replaces the cycle construction of halo2's
 *      keygen_vk / keygen_pk (plonk/permutation/keygen.rs Assembly, reached from src/scaffold/mod.rs:273) for circuits of
 *      10^8 - 10^9 cells.  parent_dev[i], i < n_cells: the stream cell that advice cell i copies (an earlier cell, or i), or
 *      n_cells + r: row r of the constants' fixed column (QuantumCell::Constant, assert_is_const); OVERWRITTEN with the roots.
 *      break_points (host): rows per advice column as vdb_layout_plan gives them; lookup_src_dev[j]: the advice cell lookup cell
 *      j copies (lookup cell j sits at row j % lookup_rows of column n_adv + j / lookup_rows).  n_cols = advice + lookup
 *      columns; the fixed column is column n_cols, the INSTANCE column is column n_cols + 1: instance_cells_dev[i] is the
 *      stream cell the circuit makes public i-th (the closure's make_public vector, src/scaffold/mod.rs:378-400:
 *      RangeWithInstanceCircuitBuilder ties assigned_instances[i] to row i of its one instance column), n_instances <= 2^k.
 *      mapping_dev: (n_cols + 2) x 2^k words col << 32 | row, the input of vdb_permutation_sigma_dev.
 *      VDB_ERR_ARG (checked on the device, nothing is read out of bounds): an instance cell or a lookup source < 0 or >= n_cells,
 *      a copy map that holds a cycle. -------------------------------------------------------------------------------------- */
int vdb_permutation_mapping_dev(int64_t *parent_dev, uint64_t n_cells, uint64_t n_consts, const uint64_t *break_points, uint64_t n_bp, uint32_t k,
                                const int64_t *lookup_src_dev, uint64_t n_lookup, uint64_t lookup_rows, uint64_t n_cols,
                                const int64_t *instance_cells_dev, uint64_t n_instances, uint64_t *mapping_dev);
/* The same with device memory lent for the sort records (4 x 8 B per grid position of a copy class + the sort's histograms): a keygen
 * passes the buffer its sigma columns and selectors fill afterwards; null or too small: the call allocates its own, as above. */
int vdb_permutation_mapping_ws_dev(int64_t *parent_dev, uint64_t n_cells, uint64_t n_consts, const uint64_t *break_points, uint64_t n_bp, uint32_t k,
                                   const int64_t *lookup_src_dev, uint64_t n_lookup, uint64_t lookup_rows, uint64_t n_cols,
                                   const int64_t *instance_cells_dev, uint64_t n_instances, uint64_t *mapping_dev, void *work_dev, size_t work_bytes);
/* The constraint map itself built on the device.  halo2-base records one equality per `Existing` / `Constant` cell while the closure
 * runs (reached from src/scaffold/mod.rs:378-400); the gadgets' structure is data independent and repeats, so a caller that knows a
 * block's template (one distance, one assignment, one filter, one division: halo2_vectordb_amd/circuit_sym.py) places it at all its
 * stream offsets with one call instead of walking 10^9 cells on the host.  All pointers are device pointers.
 *   vdb_copymap_init_dev    copy_of[i] = i, const_idx[i] = -1, flags[i] = 0, lookup_src[j] = -1
 *   vdb_copymap_place_dev   m instances of a block of n_blk cells at stream offsets bases[m]: block cell c with code blk_src[c] >= 0
 *                           copies block cell blk_src[c] of the same instance, <= -10 copies the instance's external input number
 *                           -10 - blk_src[c] (ext[m][n_ext]: stream cells), anything else copies nothing; const_idx <- blk_cid[c]
 *                           (index of the fixed-column value, -1 none); flags <- blk_flags[c] (bit 0 gate start, bit 1 the tie is an
 *                           assert_is_const); the block's n_blk_lk lookup cells at lk_bases[m] get their source cells likewise
 *   vdb_copymap_finish_dev  parent_dev (may be NULL) <- the input of vdb_permutation_mapping_dev; counts cells tied to a constant that
 *                           also copy another cell (must be 0) and lookup cells without a source (must be 0) */
int vdb_copymap_init_dev(uint64_t n_cells, uint64_t n_lookup, int64_t *copy_of_dev, int64_t *const_idx_dev, uint8_t *flags_dev, int64_t *lookup_src_dev);
int vdb_copymap_place_dev(const int64_t *blk_src_dev, const int64_t *blk_cid_dev, const uint8_t *blk_flags_dev, uint64_t n_blk, const int64_t *blk_lk_dev,
                          uint64_t n_blk_lk, const int64_t *bases_dev, const int64_t *lk_bases_dev, const int64_t *ext_dev, uint64_t m, uint64_t n_ext,
                          uint64_t n_cells, uint64_t n_lookup, int64_t *copy_of_dev, int64_t *const_idx_dev, uint8_t *flags_dev, int64_t *lookup_src_dev);
int vdb_copymap_finish_dev(const int64_t *copy_of_dev, const int64_t *const_idx_dev, uint64_t n_cells, const int64_t *lookup_src_dev, uint64_t n_lookup,
                           int64_t *parent_dev, uint64_t *tied_not_root, uint64_t *lookups_without_source);
/* out_dev[i] = src_dev[idx_dev[i]]: the public cells read out of the witness stream in instance order (what
 * circuit.instances() returns, src/scaffold/mod.rs:265) without leaving HBM */
int vdb_gather_fr_dev(const vdb_fr *src_dev, const int64_t *idx_dev, size_t n, vdb_fr *out_dev);

/* ---- Mock stage: replaces MockProver::run(k, &circuit, instances).assert_satisfied() of the reference's Mock arm
 *      (src/scaffold/mod.rs:263-266): every gate row a + b c = d, every lookup cell against the range table, every copy
 *      constraint and every constant, checked on the witness where it lies in HBM (flat streams; device pointers).
 *      flags_dev: the flag byte per advice cell of a keygen-style run (bit 0 gate start, bit 1 constant cell);
 *      copy_of_dev[i] = the cell that cell i copies (i itself or negative: none); lookup_src_dev[j] = the advice cell
 *      lookup cell j copies; const_stream_dev: a stream of the same circuit whose constant cells hold the fixed values;
 *      const_idx_dev[i] = r >= 0: cell i is tied to entry r of const_table_dev (n_consts field elements) — Constant cells
 *      and assert_is_const alike.  Any of these may be null (that check is skipped; index and table go together).
 *      Counts and the first offending index per kind. ------ */
typedef struct {
  uint64_t gate_rows_violated, first_gate_row;
  uint64_t lookup_cells_out_of_table, first_lookup_cell;
  uint64_t copies_unequal, first_copy;
  uint64_t lookup_copies_unequal, first_lookup_copy;
  uint64_t constants_changed, first_constant;
  uint64_t instances_unequal, first_instance; /* filled by vdb_mock_check_instances_dev only */
} vdb_mock_report;
int vdb_mock_check_dev(const vdb_fr *stream_dev, uint64_t n_cells, const uint8_t *flags_dev, const vdb_fr *lookup_dev, uint64_t n_lookup,
                       uint32_t lookup_bits, const int64_t *copy_of_dev, const int64_t *lookup_src_dev, const vdb_fr *const_stream_dev,
                       const int64_t *const_idx_dev, const vdb_fr *const_table_dev, uint64_t n_consts, vdb_mock_report *out);
/* The `instances` argument of MockProver::run: stream cell instance_cells_dev[i] must hold instances_dev[i] (the copy between
 * the cell and row i of the instance column).  Sets out->instances_unequal / first_instance and leaves the other fields alone. */
int vdb_mock_check_instances_dev(const vdb_fr *stream_dev, uint64_t n_cells, const int64_t *instance_cells_dev, const vdb_fr *instances_dev,
                                 uint64_t n_instances, vdb_mock_report *out);

/* ---- b7 Verify: the Verify arm of the reference's scaffold (SnarkCmd::Verify, src/scaffold/mod.rs:298-320) — halo2's
 *      read_snark + verify_proof over a proof this library wrote (halo2_vectordb_amd/verifier.py drives them). -------------- */
/* Status byte per point of vdb_g1_decompress_dev. */
enum { VDB_G1_OK = 0, VDB_G1_NONCANONICAL = 1 /* x >= q, or the spare top bit that is not the sign is set */,
       VDB_G1_NOT_ON_CURVE = 2 /* x^3 + 3 has no square root */, VDB_G1_BAD_IDENTITY = 3 /* x = 0 with a flag bit set */ };
/* Replaces the point reads of halo2's TranscriptRead::read_point (G1Affine::from_bytes) for a whole proof at once: n 32-byte
 * compressed encodings (x little-endian; bit sign_bit of the last byte — 6 or 7, as vdb_transcript_set_sign_bit — says y is odd;
 * the identity is the all-zero encoding) -> n Montgomery affine points in out_dev (the identity and every rejected point as
 * (0, 0)) and one VDB_G1_* status per point in status_dev.  Device pointers; blocks until done. */
int vdb_g1_decompress_dev(const uint8_t *enc_dev, size_t n, uint32_t sign_bit, vdb_g1 *out_dev, uint8_t *status_dev);
/* Replaces the MSM of halo2's verify_proof (the verifier's MSMKZG::eval, best_multiexp over arbitrary bases):
 * out_host = sum_i scalars[i] points[i] for n arbitrary affine points (identity allowed) and Montgomery scalars below r, both in
 * HBM.  Variable-base Pippenger: no window tables are built, the bases are used once.  n = 0 gives the identity. */
int vdb_msm_points_dev(const vdb_g1 *points_dev, const vdb_fr *scalars_dev, size_t n, vdb_g1 *out_host);
/* Host arithmetic (no GPU needed, no vdb_init): replaces halo2's KZG verifier key side.
 * [s] G2 for the EIP-197 generator of G2 — the SRS's [tau]_2 (ParamsKZG::s_g2) from the key's scalar s (Montgomery Fr). */
int vdb_g2_mul_generator(const vdb_fr *s, vdb_g2 *out);
/* *ok = 1 when prod_i e(a[i], b[i]) = 1 in GT (the optimal ate pairing, one final exponentiation for the product), else 0 —
 * Bn256::multi_miller_loop(...).final_exponentiation() == Gt::identity() of halo2's KZG verification.  Identities contribute 1;
 * n = 0 accepts.  VDB_ERR_ARG when a coordinate is not below q or a point is not on its curve (G2's subgroup is not checked:
 * the verifier's G2 points are the generator and [tau]_2 from vdb_g2_mul_generator). */
int vdb_pairing_check(const vdb_g1 *a, const vdb_g2 *b, size_t n, int *ok);
/* *ok = 1 when each of the n points is a G2 element: coordinates below q, on the twist (the all-zero identity included) and
 * r P = O — what halo2's RawBytes reader checks of a params file's g2 and s_g2 (ParamsKZG::read), plus the subgroup.  Host
 * arithmetic, no GPU needed. */
int vdb_g2_check(const vdb_g2 *p, size_t n, int *ok);

/* ---- b6 Poseidon: replaces poseidon::PoseidonChip<F,3,2> value semantics (T=3, RATE=2, R_F=8,
 *      R_P=57 as examples/merkle.rs:15-18; call sites src/gadget/vectordb.rs:180-182, 213-215) --- */
int vdb_poseidon_hash_many(const vdb_fr *inputs, size_t n_msgs, size_t msg_len, vdb_fr *digests);
int vdb_poseidon_merkle_root(const vdb_fr *vectors, size_t n, size_t dim, vdb_fr *root);
int vdb_poseidon_permute(vdb_fr *states /* n x 3 */, size_t n);

#ifdef __cplusplus
}
#endif
#endif
