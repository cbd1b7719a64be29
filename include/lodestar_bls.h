/*
 * lodestar_bls.h — C ABI of the MI355X BLS12-381 signature-set verifier.
 *
 * This is the drop-in boundary for Lodestar's IBlsVerifier hot path
 * (SURVEY.md §8(b)).  Plain pointers and sizes only; no torch / HIP types.
 * Every entry point returns an lb_status code (0 = OK) and never throws.
 *
 * Reference interfaces each entry point replaces (paths under the reference repo):
 *   lb_verify_jobs / lb_batch_*   packages/beacon-node/src/chain/bls/multithread/worker.ts:32-108
 *                                 (verifyManySignatureSets: BlsWorkReq[] -> per-job results),
 *                                 packages/beacon-node/src/chain/bls/maybeBatch.ts:16-39
 *                                 (verifySignatureSetsMaybeBatch) and the blst calls it makes
 *                                 (Signature.fromBytes(sig, affine, true), verifyMultipleSignatures,
 *                                 Signature.verify).
 *   lb_aggregate_pubkeys          packages/beacon-node/src/chain/bls/utils.ts:5-16
 *                                 (getAggregatedPubkey) + PublicKey.toBytes(uncompressed),
 *                                 packages/beacon-node/src/chain/bls/multithread/index.ts:126,160.
 *   lb_batch_partial /
 *   lb_fp12_product_is_one        the multi-GPU split of blst Pairing.commit()+finalverify()
 *                                 (SURVEY.md §8(e)): per-GPU Fp12 partial products, one
 *                                 final exponentiation over their product.
 *
 * Data formats (all ZCash BLS12-381 encodings, big-endian):
 *   pubkey      96 B uncompressed affine G1 (x || y), as the reference's main thread
 *               serialises it (PointFormat.uncompressed); infinity = 0x40 || 0^95.
 *   signing root 32 B (ISignatureSet.signingRoot).
 *   signature   96 B compressed G2 (ISignatureSet.signature).
 *   Fp12 partial 576 B: 12 Fp coefficients, tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ...
 *
 * Job results (int32 per job): 1 = valid, 0 = invalid, -code = the job rejects with
 * error `code` (lb_error_name(code) gives the blst error string the reference throws).
 */
#ifndef LODESTAR_BLS_H
#define LODESTAR_BLS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status / error codes: blst BLST_ERROR values plus Lodestar's own errors */
#define LB_OK 0
#define LB_BAD_ENCODING 1
#define LB_POINT_NOT_ON_CURVE 2
#define LB_POINT_NOT_IN_GROUP 3
#define LB_AGGR_TYPE_MISMATCH 4
#define LB_VERIFY_FAIL 5
#define LB_PK_IS_INFINITY 6
#define LB_BAD_SCALAR 7
#define LB_INVALID_SIZE 10           /* "BLST_INVALID_SIZE" (multithread.test.ts:97) */
#define LB_EMPTY_AGGREGATE_ARRAY 11  /* bls.PublicKey.aggregate([]) */
#define LB_EMPTY_SIGNATURE_SET 12    /* "Empty signature set" (maybeBatch.ts:29-31) */
#define LB_ERR_ARGUMENT 100          /* bad C-ABI arguments (NULL, inconsistent offsets) */
#define LB_ERR_DEVICE 101            /* HIP runtime failure */
#define LB_ERR_NO_DEVICE 102         /* no usable gfx950 device */

typedef struct lb_engine lb_engine;
typedef struct lb_batch lb_batch;

/* Human-readable blst-style name for a status code ("BLST_INVALID_SIZE", ...). */
const char* lb_error_name(int32_t code);

/* ABI version (bumped on incompatible changes). */
int32_t lb_abi_version(void);

/*
 * The number of usable devices: ordinals 0 .. n-1 are gfx950 and lb_engine_create accepts each of
 * them (a pool that spreads over the host's GPUs creates its engines on these).  0 when there is
 * none or when the HIP runtime fails to enumerate; never an error.
 */
int32_t lb_device_count(void);

/*
 * One engine = one batch in flight on one GPU (own HIP streams and device workspaces); a process
 * may drive several engines per GPU concurrently (the reference runs one job package per worker
 * thread at a time, multithread/index.ts:290-381).  device < 0 = current.  Returns
 * LB_ERR_DEVICE once the per-device engine cap is reached (10, or LB_MAX_ENGINES_PER_DEVICE;
 * each engine's scratch for the largest private segment is reserved at creation, so an exhausted
 * pool fails here instead of aborting a queue later).
 */
int32_t lb_engine_create(int32_t device, lb_engine** out);
/*
 * The same with flags.  LB_ENGINE_LATENCY: the engine is the device's latency engine (the
 * reference's verifyOnMainThread path, multithread/index.ts:138-151): its streams run on a
 * reserved set of CUs (LB_LATENCY_CUS, default 8) and it always takes the small-batch latency
 * forms; engines created AFTER it on the device run on the remaining CUs, so a 1-set call does not
 * queue behind the pool's batches.  Create the latency engine first (engines created before it keep
 * every CU; a warning is printed).  The partition lasts while a latency engine exists: engines
 * created after the last one is destroyed get the whole device again.  CU-masked streams are
 * blocking streams (they synchronise with the legacy null stream).
 */
#define LB_ENGINE_LATENCY 1u
int32_t lb_engine_create_ex(int32_t device, uint32_t flags, lb_engine** out);
void lb_engine_destroy(lb_engine* e);
/* CUs the engine's streams may use: the device's count, the reserved CUs for a latency engine, or
 * the rest while a partition exists.  0 for NULL. */
int32_t lb_engine_cu_count(const lb_engine* e);

/*
 * Upload one batch of jobs into device memory (copies; the caller keeps its buffers).
 *   n_jobs        number of jobs (one job = one BlsWorkReq / one verifySignatureSets chunk)
 *   job_offsets   n_jobs+1 prefix sums over sets (job j = sets [job_offsets[j], job_offsets[j+1]))
 *   set_pk_offsets n_sets+1 prefix sums over pubkeys (set i aggregates pubkeys
 *                 [set_pk_offsets[i], set_pk_offsets[i+1]); a `single` set has exactly one)
 *   pubkeys       set_pk_offsets[n_sets] x 96 B
 *   signing_roots n_sets x 32 B
 *   signatures    n_sets x 96 B
 *   sig_sizes     optional n_sets original signature byte lengths (NULL = all 96); a set whose
 *                 length is not 96 makes its job reject with LB_INVALID_SIZE
 */
int32_t lb_batch_create(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                        const uint32_t* set_pk_offsets, const uint8_t* pubkeys,
                        const uint8_t* signing_roots, const uint8_t* signatures,
                        const uint32_t* sig_sizes, lb_batch** out);
void lb_batch_destroy(lb_batch* b);
uint32_t lb_batch_num_sets(const lb_batch* b);
uint32_t lb_batch_num_jobs(const lb_batch* b);

/*
 * Verify a resident batch: out_job[n_jobs] receives 1 / 0 / -code per job.
 * scalars: n_sets non-zero 64-bit blinding words, or NULL to draw them from the OS
 * CSPRNG (getrandom), as blst's verifyMultipleSignatures draws 8 random bytes per set.
 * A word w = hi:lo stands for the blinding value r = lo + hi * lambda mod q, lambda = -x^2
 * (the GLV eigenvalue; oracle/bls_oracle.py blinding_scalar).  Like blst's 64-bit integer,
 * a uniform word is a uniform draw from 2^64 - 1 distinct values, and it halves the blinding
 * scalar multiplications (lb_curve.h jac_mul_glv).
 * All valid jobs are checked with ONE final exponentiation; a failing batch is bisected
 * over a product tree of jobs down to the invalid ones.
 */
int32_t lb_batch_verify(lb_engine* e, lb_batch* b, const uint64_t* scalars, int32_t* out_job);

/*
 * Multi-GPU split.  lb_batch_partial runs the batch up to its root partial product
 *   f = prod_i ML(r_i PK_i, H(m_i)) * ML(-G1, sum_i r_i sig_i)        (576 B, see above)
 * and per-job error codes (out_job: -code for rejecting jobs, 1 otherwise).
 * lb_fp12_product_is_one multiplies n such partials and runs one final exponentiation;
 * *ok = 1 iff the product is 1 in GT (every valid job of every partial verifies).
 * On a 0 verdict, lb_batch_search_after_partial localises each shard's invalid jobs from the
 * state its lb_batch_partial left in the engine (the shard's own final exponentiation, then the
 * invalid-set search, with the same blinding): no second pipeline run.  It returns
 * LB_ERR_ARGUMENT if any other call ran on the engine in between (then call lb_batch_verify).
 * Replaces the reference's per-job re-verification of a failing chunk
 * (packages/beacon-node/src/chain/bls/multithread/worker.ts:76-98) for a sharded segment.
 */
int32_t lb_batch_partial(lb_engine* e, lb_batch* b, const uint64_t* scalars, uint8_t* out576,
                         int32_t* out_job);
int32_t lb_fp12_product_is_one(lb_engine* e, const uint8_t* partials576, uint32_t n, int32_t* ok);
int32_t lb_batch_search_after_partial(lb_engine* e, lb_batch* b, int32_t* out_job);

/*
 * Upload + verify in one call (the worker's verifyManySignatureSets, worker.ts:32-108): inputs go
 * into an engine-owned device workspace that is grown once and reused (no per-call device
 * allocation).  Inputs in pinned host memory (lb_host_alloc) are DMA'd directly; pageable inputs
 * are staged by the HIP runtime.
 */
int32_t lb_verify_jobs(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                       const uint32_t* set_pk_offsets, const uint8_t* pubkeys,
                       const uint8_t* signing_roots, const uint8_t* signatures,
                       const uint32_t* sig_sizes, const uint64_t* scalars, int32_t* out_job);
/* lb_verify_jobs over the resident pubkey table (pk_indices as in lb_batch_create_indexed) */
int32_t lb_verify_jobs_indexed(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                               const uint32_t* set_pk_offsets, const uint32_t* pk_indices,
                               const uint8_t* signing_roots, const uint8_t* signatures,
                               const uint32_t* sig_sizes, const uint64_t* scalars, int32_t* out_job);

/* Pinned (page-locked) host memory for request staging; NULL on failure. */
void* lb_host_alloc(size_t bytes);
void lb_host_free(void* p);

/*
 * G1 pubkey aggregation (getAggregatedPubkey + toBytes(uncompressed)):
 * out96[n_sets x 96] = ZCash uncompressed sum of each set's pubkeys; out_status[n_sets]
 * = LB_OK or the error (bad encoding / not on curve / LB_EMPTY_AGGREGATE_ARRAY).
 */
int32_t lb_aggregate_pubkeys(lb_engine* e, uint32_t n_sets, const uint32_t* set_pk_offsets,
                             const uint8_t* pubkeys, uint8_t* out96, int32_t* out_status);

/*
 * G2 signature aggregation, bls.Signature.aggregate(sigs).toBytes() as the op pools use it for
 * block production (beacon-node/src/chain/opPools/aggregatedAttestationPool.ts:321,
 * attestationPool.ts:184, syncContributionAndProofPool.ts:185).
 * Group g sums signatures [group_offsets[g], group_offsets[g+1]) of sigs96 (96 B compressed
 * each; sig_sizes as in lb_batch_create, NULL = all 96); validate != 0 adds the G2 subgroup
 * check of Signature.fromBytes(.., true).  out96[g] = compressed sum (infinity = 0xc0 || 0^95),
 * out_status[g] = LB_OK, the first bad signature's decode error, or LB_EMPTY_AGGREGATE_ARRAY.
 */
int32_t lb_aggregate_signatures(lb_engine* e, uint32_t n_groups, const uint32_t* group_offsets,
                                const uint8_t* sigs96, const uint32_t* sig_sizes, int32_t validate,
                                uint8_t* out96, int32_t* out_status);

/*
 * Batch G1 decompression (48 B compressed -> 96 B uncompressed), the pubkey cache's one-time
 * deserialisation (state-transition/src/cache/pubkeyCache.ts:56-77).  validate != 0 adds
 * PublicKey.keyValidate: infinity -> LB_PK_IS_INFINITY, not in G1 -> LB_POINT_NOT_IN_GROUP.
 */
int32_t lb_g1_decompress(lb_engine* e, uint32_t n, const uint8_t* in48, uint8_t* out96, int32_t* out_status,
                         int32_t validate);

/*
 * SSZ merkleization (the hashing of signing-root production: getBlockSignatureSets ->
 * computeSigningRoot, state-transition/src/signatureSets/index.ts:64-111, src/util/signingRoot.ts:7-13;
 * SURVEY.md §8(f) row 2).  Tree t hashes chunks [chunk_offsets[t], chunk_offsets[t+1]) of
 * chunks32 (32 B each) padded with zero chunks to 2^depths[t] leaves; mix_lengths[t] != UINT64_MAX
 * mixes in that length (SSZ lists / bitlists).  out_roots32[t] = the 32-byte root.
 */
int32_t lb_merkleize(lb_engine* e, uint32_t n_trees, const uint32_t* chunk_offsets, const uint8_t* chunks32,
                     const uint32_t* depths, const uint64_t* mix_lengths, uint8_t* out_roots32);

/*
 * A segment's block signature sets from the SignedBeaconBlocks' SSZ bytes, as range sync and gossip
 * deliver them (getBlockSignatureSets, state-transition/src/signatureSets/index.ts:26-72): every
 * set's signing root and signature, and a reference that says which keys the host supplies from
 * the state.  The device finds everything at offsets the bytes give (csrc/lb_ssz_walk.h) and hashes
 * it (csrc/lb_ssz_sets.h); the host never walks a block.  One upload, a launch sequence that depends
 * on nothing read back, one download, one stream synchronisation.
 *
 * Block b = ssz[byte_offsets[b], byte_offsets[b+1]) of ForkSeq forks[b] (0 phase0 .. 3 capella; a
 * later fork is LB_ERR_ARGUMENT).  domains32[b] = 2 x 6 domains of 32 B: [the state's previous = 0 /
 * current = 1 fork version][proposer, attester, randao, voluntary_exit, sync_committee,
 * bls_to_execution_change]; a set takes version 0 when its message's epoch is below fork_epochs[b],
 * as config.getDomain does.  The epoch is the block's (randao, proposer), the header's slot / 32
 * (proposer slashing), target.epoch (attestation, attester slashing), the exit's, (max(slot, 1) - 1)
 * / 32 (sync aggregate), state_slots[b] / 32 (BLS change).  flags & 1 leaves the proposer set out.
 *
 * out_status[b] = LB_OK; LB_BAD_ENCODING for bytes that are not a well-formed block of that fork
 * (every offset is checked before use and nothing outside the block is read; the other blocks are
 * unaffected); LB_VERIFY_FAIL for a sync aggregate without participants whose signature is not the
 * point at infinity.  out_n_sets[b] = its sets (0 unless LB_OK), rows [b * LB_BLOCK_MAX_SETS, +n) of
 * out_kind (LB_SET_*), out_roots32, out_sigs96 and out_ref (4 words a row), in the reference's order:
 * randao, proposer slashings (two sets each), attester slashings (two each), attestations, exits,
 * proposer, sync aggregate (none when no participant and the signature is infinity), BLS changes.
 * out_ref: {validator index, 0, 0, 0} (randao, proposer, exit; proposer slashing: header 1's
 * proposer for both sets); {data.slot, data.index, byte position of aggregation_bits in ssz, its
 * byte length} (attestation); {0, count, position of attesting_indices, byte length} (attester
 * slashing); {0, 0, position of the 64-byte bit vector, 64} (sync aggregate); {0, 0, position of
 * from_bls_pubkey, 48} (BLS change).
 *
 * LB_ERR_ARGUMENT, with nothing launched: a needed pointer that is NULL, byte_offsets[0] != 0,
 * decreasing offsets, a fork above 3, n_blocks > 64, more than 64 MiB in all.  n_blocks == 0 returns
 * LB_OK at once.  lb_block_sets_syncs: the stream synchronisations these calls made on the engine.
 */
#define LB_BLOCK_MAX_SETS 199 /* 1 + 32 + 4 + 128 + 16 + 1 + 1 + 16 */
enum { LB_SET_RANDAO, LB_SET_PROPOSER_SLASHING, LB_SET_ATTESTER_SLASHING, LB_SET_ATTESTATION,
       LB_SET_VOLUNTARY_EXIT, LB_SET_PROPOSER, LB_SET_SYNC_AGGREGATE, LB_SET_BLS_TO_EXECUTION_CHANGE };
int32_t lb_block_sets_from_ssz(lb_engine* e, uint32_t n_blocks, const uint32_t* byte_offsets, const uint8_t* ssz,
                               const uint32_t* forks, const uint8_t* domains32, const uint64_t* fork_epochs,
                               const uint64_t* state_slots, uint32_t flags, int32_t* out_status,
                               uint32_t* out_n_sets, uint32_t* out_kind, uint8_t* out_roots32, uint8_t* out_sigs96,
                               uint64_t* out_ref);
uint64_t lb_block_sets_syncs(const lb_engine* e);

/*
 * KZG (EIP-4844 blobs; the c-kzg calls behind packages/beacon-node/src/util/kzg.ts:15-65, SURVEY.md
 * §8(f) row 4).  Two levels: the group calls (lb_g1_lincomb, lb_kzg_verify_proof), for a host that
 * does the scalar-field work itself (lodestar_amd/kzg.py with field="host"), and the blob-level
 * calls further down (lb_kzg_blob_to_commitment ...), which take blobs and do the field work on the
 * GPU as well.
 *
 * lb_kzg_load_setup (ckzg.loadTrustedSetup, kzg.ts:54-67): the monomial-form setup as Lodestar's
 * trusted_setup.bin holds it -- n_g1 compressed [tau^i] G1 (48 B each) and at least two compressed
 * [tau^i] G2 (96 B each; [tau^0] G2 and [tau^1] G2 are kept, and with n_g2 >= 65 also [tau^64] G2,
 * which the cell calls below pair against; with fewer, everything but lb_kzg_verify_cell_proof_batch
 * works).  Every point is decoded and checked (curve, subgroup); out_status[i] per G1 point, and
 * LB_POINT_NOT_IN_GROUP is returned for a bad G2 point.  Replaces any previously loaded setup of
 * this engine.
 */
int32_t lb_kzg_load_setup(lb_engine* e, const uint8_t* g1_48, uint32_t n_g1, const uint8_t* g2_96, uint32_t n_g2,
                          int32_t* out_status);

/*
 * G1 linear combination out48 = compress(sum_i s_i P_i) (the spec's g1_lincomb): P_i = setup point i
 * (points48 == NULL; n <= the loaded setup size), or n compressed points (points48).  scalars32:
 * n little-endian 32-byte scalars below r.  Returns the decode error of the first bad point.
 */
int32_t lb_g1_lincomb(lb_engine* e, uint32_t n, const uint8_t* points48, const uint8_t* scalars32, uint8_t* out48);

/*
 * verify_kzg_proof_impl: *ok = 1 iff e(C - [y] G1, -G2) e(proof, [tau] G2 - [z] G2) == 1, else 0;
 * *ok = -code if C or proof fails to decode.  z32, y32: little-endian scalars below r.
 */
int32_t lb_kzg_verify_proof(lb_engine* e, const uint8_t* commitment48, const uint8_t* z32, const uint8_t* y32,
                            const uint8_t* proof48, int32_t* ok);

/*
 * Blob-level KZG: bytes in, commitment / proof / verdict out, the scalar-field work (inverse NTT of
 * the blob's evaluations, aggregation, evaluation, quotient: lb_kzg_field.h) and the group work both
 * on the GPU; only the Fiat-Shamir transcript is hashed on the host.  A blob is 4096 field
 * elements of 32 big-endian bytes (131 072 bytes), its polynomial's values at the bit-reversed
 * 4096th roots of unity.  Every call needs a loaded setup of exactly 4096 G1 points
 * (LB_ERR_ARGUMENT otherwise); a blob element >= r is LB_BAD_SCALAR.  The semantics are those of
 * lodestar_amd/kzg.py (the EIP-4844 spec of consensus-specs v1.3.0-alpha.2); byte parity with c-kzg
 * is unpinned, as for the group calls.
 *
 * lb_kzg_blob_to_commitment (ckzg.blobToKzgCommitment) for n_blobs blobs: out48[b], and
 * out_status[b] = LB_OK or LB_BAD_SCALAR (out48[b] is then zeroed); returns LB_OK when the call
 * itself ran.
 * lb_kzg_compute_proof: the proof that the blob's polynomial takes the value y at z (z32le, y32le:
 * little-endian, z below r else LB_BAD_SCALAR); z on the evaluation domain is allowed.
 * lb_kzg_compute_aggregate_proof (ckzg.computeAggregateKzgProof): commitments, challenges r and x
 * from the transcript, the proof of sum r^j poly_j at x.  Zero blobs: the point at infinity.
 * lb_kzg_verify_aggregate_proof (ckzg.verifyAggregateKzgProof): *ok = 1 / 0, or -code for a
 * commitment or proof that fails to decode or lies outside G1.  Zero blobs still decode the proof
 * (1 iff it is the point at infinity).
 * lb_kzg_blob_coefficients: the blob's polynomial in monomial form, 4096 little-endian 32-byte
 * coefficients (the scalars whose lb_g1_lincomb is the commitment).
 */
int32_t lb_kzg_blob_to_commitment(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, uint8_t* out48,
                                  int32_t* out_status);
int32_t lb_kzg_compute_proof(lb_engine* e, const uint8_t* blob, const uint8_t* z32le, uint8_t* out_proof48,
                             uint8_t* out_y32le);
int32_t lb_kzg_compute_aggregate_proof(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, uint8_t* out48);
int32_t lb_kzg_verify_aggregate_proof(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs,
                                      const uint8_t* commitments48, const uint8_t* proof48, int32_t* ok);
int32_t lb_kzg_blob_coefficients(lb_engine* e, const uint8_t* blob, uint8_t* out_coeffs32le /* 4096 x 32 */);

/*
 * lb_kzg_verify_aggregate_proof for many sidecars in one pass (a range-sync segment's blocks): every
 * stage runs once over all of them, with one stream synchronisation, and each sidecar gets its own
 * exact pairing check.  Sidecar k owns blobs blob_offsets[k] .. blob_offsets[k + 1] - 1 and their
 * commitments; a sidecar without blobs is allowed anywhere (1 iff its proof is the point at
 * infinity; the proof is still decoded and subgroup-checked).
 * out_ok[k] is what lb_kzg_verify_aggregate_proof reports for sidecar k alone: its *ok (1, 0, or
 * -code for a commitment or proof that fails to decode or lies outside G1), or -LB_BAD_SCALAR where
 * the single call returns LB_BAD_SCALAR.  Precedence as there: a blob element >= r, the first
 * failing commitment in order, the proof's decode error, the proof outside G1.  A sidecar that
 * rejects changes nothing for the others.
 * Returns LB_OK whenever the call ran (n_sidecars == 0: at once, nothing written); LB_ERR_ARGUMENT
 * for no 4096-point setup, a needed pointer that is NULL, blob_offsets[0] != 0, decreasing offsets,
 * more than 1024 sidecars or more than 1024 blobs in all.
 * lb_kzg_batch_hash_ns: the host time the engine's last batch call spent hashing transcripts.
 */
int32_t lb_kzg_verify_aggregate_proof_batch(lb_engine* e, uint32_t n_sidecars,
                                            const uint32_t* blob_offsets, /* n_sidecars + 1 prefix sums over blobs */
                                            const uint8_t* blobs,         /* blob_offsets[n] x 131072 B */
                                            const uint8_t* commitments48, /* blob_offsets[n] x 48 B, same order */
                                            const uint8_t* proofs48,      /* n_sidecars x 48 B */
                                            int32_t* out_ok);             /* n_sidecars */
uint64_t lb_kzg_batch_hash_ns(const lb_engine* e);

/*
 * One proof per blob: the form of EIP-4844 that shipped in Deneb (c-kzg computeBlobKzgProof,
 * verifyBlobKzgProof, verifyBlobKzgProofBatch).  Both calls need the 4096-point setup and take at
 * most 1024 blobs (and 1024 groups); LB_ERR_ARGUMENT otherwise, or for a needed pointer that is NULL.
 * The challenge of blob i is z_i = hash_to_bls_field(FS_DOMAIN || 4096 as 16 bytes BE || blob_i ||
 * C_i), hashed on up to LB_KZG_HASH_THREADS host threads (environment, default 8, at most 16).
 * Byte parity with c-kzg is not pinned, as for the calls above.
 *
 * lb_kzg_compute_blob_proofs: out_proofs48[b] = commit((p_b - p_b(z_b)) / (X - z_b)) for every blob
 * and its commitment (which must decode and lie in G1; infinity is allowed).  out_status[b] = LB_OK,
 * the commitment's decode / group error, or LB_BAD_SCALAR for a blob element >= r; the proof of a
 * rejected blob is zeroed.  Returns LB_OK whenever the call ran.
 *
 * lb_kzg_verify_blob_proof_batch: one group is one verifyBlobKzgProofBatch call (one block's
 * sidecars).  Group k owns blobs group_offsets[k] .. group_offsets[k + 1] - 1 with their commitments
 * and proofs, one proof per blob, and gets its own exact check with the spec's combiner
 *   r = hash_to_bls_field(RC_DOMAIN || 4096, n as 8 bytes BE each || per blob: C_i || z_i || y_i || proof_i):
 *   e(sum r^i C_i - [sum r^i y_i] G1 + sum [r^i z_i] proof_i, -G2) e(sum r^i proof_i, [tau] G2) == 1.
 * out_ok[k] = 1, 0, or -code: the lowest blob index with any error wins, and within a blob the
 * commitment's decode / group error, then -LB_BAD_SCALAR for a blob element >= r, then the proof's
 * error.  An empty group gives 1; a rejecting group changes nothing for the others; the verdicts
 * are deterministic (no random combination across groups).  Argument errors as for
 * lb_kzg_verify_aggregate_proof_batch.  lb_kzg_batch_hash_ns reports this call's hashing time too.
 */
int32_t lb_kzg_compute_blob_proofs(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, /* n_blobs x 131072 B */
                                   const uint8_t* commitments48, uint8_t* out_proofs48, int32_t* out_status);
int32_t lb_kzg_verify_blob_proof_batch(lb_engine* e, uint32_t n_groups,
                                       const uint32_t* group_offsets, /* n_groups + 1 prefix sums over blobs */
                                       const uint8_t* blobs,          /* group_offsets[n] x 131072 B */
                                       const uint8_t* commitments48,  /* group_offsets[n] x 48 B */
                                       const uint8_t* proofs48,       /* group_offsets[n] x 48 B */
                                       int32_t* out_ok);              /* n_groups */

/*
 * Cells (EIP-7594 data-availability sampling; c-kzg computeCells, verifyCellKzgProofBatch).  The
 * blob's polynomial is evaluated over the 8192-point domain of w = 7^((r - 1) / 8192), in 128 cells of
 * 64 field elements (2048 bytes, 32 big-endian bytes each): cell i holds the values at the bit-reversed
 * roots 64 i .. 64 i + 63, the coset h_i <w^128> with h_i = w^brp7(i).  Cells 0 .. 63 are the blob.
 * Every call needs the 4096-point setup; byte parity with c-kzg is not pinned, as above.
 *
 * lb_kzg_compute_cells (ckzg.computeCells) for n_blobs <= 1024 blobs: out_cells[b] = the 128 cells of
 * blob b; out_status[b] = LB_OK or LB_BAD_SCALAR for a blob element >= r (its cells are then zeroed).
 * Returns LB_OK whenever the call ran.
 *
 * lb_kzg_compute_cell_proofs: the proofs of n_cells <= 128 chosen cells of ONE blob by the spec's
 * direct route, proof_i = commit((p - I_i) / (X^64 - h_i^64)): the quotient on the device, then one
 * 4096-term multi-scalar multiplication PER CELL: the route to a few cells.  For all 128 proofs of
 * whole blobs use lb_kzg_compute_cells_and_proofs below, which gives the same bytes by FK20 at about
 * the price of a dozen such multiplications.  *out_status = LB_OK or LB_BAD_SCALAR (the proofs are then zeroed); a cell index >= 128
 * is LB_ERR_ARGUMENT.
 *
 * lb_kzg_verify_cell_proof_batch: one group is one verifyCellKzgProofBatch call (a data-column
 * sidecar).  Group g owns cells cell_offsets[g] .. cell_offsets[g + 1] - 1 of the flat per-cell arrays
 * and gets its own exact check with the spec's combiner: the group's commitments are deduplicated in
 * order of first appearance, r = hash_to_bls_field(CELL_DOMAIN || 4096 || 64 || #distinct || n || the
 * distinct commitments || per cell: commitment index || cell index || cell || proof), integers as 8
 * bytes BE, and with I_k the interpolation polynomial of cell k over its coset
 *   e(sum r^k proof_k, [tau^64] G2) e(sum r^k C_k - commit(sum r^k I_k) + sum [r^k h_k^64] proof_k, -G2) == 1.
 * r hashes nothing the device computes, so the whole pass has ONE stream synchronisation.
 * out_ok[g] = 1, 0, or -code in the spec's reading order: the first commitment (by position) that
 * fails to decode or lies outside G1, then -LB_BAD_SCALAR for the first cell with an element >= r,
 * then the first bad proof.  Infinity is a legal commitment and proof; an empty group gives 1; a
 * rejecting group changes nothing for the others.  Returns LB_OK whenever the call ran (n_groups == 0:
 * at once); LB_ERR_ARGUMENT for no 4096-point setup or one loaded with n_g2 < 65, a needed pointer that
 * is NULL, cell_offsets[0] != 0, decreasing offsets, a cell index >= 128, more than 1024 groups or
 * more than 16384 cells in all.  lb_kzg_batch_hash_ns reports this call's hashing time too.
 *
 * lb_kzg_compute_cells_and_proofs (ckzg.computeCellsAndKzgProofs) for n_blobs <= 128 blobs: out_cells[b]
 * = the 128 cells of blob b, exactly lb_kzg_compute_cells' bytes, and out_proofs48[b] = its 128 cell
 * proofs, proof i = commit((p - I_i) / (X^64 - h_i^64)): the bytes lb_kzg_compute_cell_proofs gives for
 * cell i (a compressed point is canonical), computed by FK20: one ladder pass over a resident 8192-point
 * transform of the setup, two 128-point transforms in G1 per blob.  That table is built on the first
 * call after lb_kzg_load_setup (once per setup; the call that builds it takes that much longer).
 * out_status[b] = LB_OK, or LB_BAD_SCALAR for a blob element >= r: that blob's cells and proofs are
 * zeroed, the other blobs are unaffected.  Returns LB_OK whenever the call ran (n_blobs == 0: at once,
 * nothing read); LB_ERR_ARGUMENT for no 4096-point setup, a needed pointer that is NULL or
 * n_blobs > 128.  It pairs against nothing: a setup loaded with two G2 points will do.
 *
 * lb_kzg_recover_cells_and_proofs (ckzg.recoverCellsAndKzgProofs) for n_blobs <= 128 blobs: blob b is
 * given by cells cell_offsets[b] .. cell_offsets[b + 1] - 1 of the flat arrays, any 64 .. 128 of its
 * 128 cells with their indices strictly ascending.  out_cells[b] = all 128 cells and out_proofs48[b] =
 * all 128 proofs, the bytes lb_kzg_compute_cells_and_proofs gives for the blob: the scalar-field
 * erasure decode runs as 64 independent decodes of size 128 per blob on the device, every output
 * cell is recomputed from the recovered coefficients (none is copied from the input), and the proofs
 * come from the same FK20 pass.  out_status[b] = LB_OK, LB_BAD_SCALAR for a cell element >= r, or
 * LB_VERIFY_FAIL when the given cells lie on no polynomial of degree < 4096 (possible only with more
 * than 64 cells; this is STRICTER than c-kzg, which returns cells of some other polynomial there);
 * LB_BAD_SCALAR comes first.  A rejected blob's cells and proofs are zeroed, the other blobs are
 * unaffected.  Returns LB_OK whenever the call ran (n_blobs == 0: at once, nothing read);
 * LB_ERR_ARGUMENT, with nothing launched, for no 4096-point setup, a needed pointer that is NULL,
 * n_blobs > 128, cell_offsets[0] != 0, decreasing offsets, a blob with fewer than 64 or more than 128
 * cells, an index >= 128 or indices of a blob that do not strictly ascend (the spec's sorted and
 * no-duplicates checks).  One stream synchronisation (after the FK20 table's first build); it pairs
 * against nothing: a setup loaded with two G2 points will do.
 */
int32_t lb_kzg_compute_cells(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, /* n_blobs x 131072 B */
                             uint8_t* out_cells,                                  /* n_blobs x 128 x 2048 B */
                             int32_t* out_status);                                /* n_blobs */
int32_t lb_kzg_compute_cell_proofs(lb_engine* e, const uint8_t* blob, uint32_t n_cells, const uint32_t* cell_indices,
                                   uint8_t* out_proofs48, /* n_cells x 48 B */
                                   int32_t* out_status);  /* one: the blob's */
int32_t lb_kzg_verify_cell_proof_batch(lb_engine* e, uint32_t n_groups,
                                       const uint32_t* cell_offsets,  /* n_groups + 1 prefix sums over cells */
                                       const uint8_t* commitments48,  /* one per cell: cell_offsets[n] x 48 B */
                                       const uint32_t* cell_indices,  /* one per cell, < 128 */
                                       const uint8_t* cells,          /* cell_offsets[n] x 2048 B */
                                       const uint8_t* proofs48,       /* cell_offsets[n] x 48 B */
                                       int32_t* out_ok);              /* n_groups */
int32_t lb_kzg_compute_cells_and_proofs(lb_engine* e, uint32_t n_blobs, const uint8_t* blobs, /* n x 131072 B */
                                        uint8_t* out_cells,    /* n x 128 x 2048 B */
                                        uint8_t* out_proofs48, /* n x 128 x 48 B   */
                                        int32_t* out_status);  /* n */
int32_t lb_kzg_recover_cells_and_proofs(lb_engine* e, uint32_t n_blobs,
                                        const uint32_t* cell_offsets, /* n_blobs + 1 prefix sums over the given cells */
                                        const uint32_t* cell_indices, /* one per given cell, < 128 */
                                        const uint8_t* cells,         /* cell_offsets[n] x 2048 B */
                                        uint8_t* out_cells,           /* n x 128 x 2048 B */
                                        uint8_t* out_proofs48,        /* n x 128 x 48 B   */
                                        int32_t* out_status);         /* n */

/*
 * Synthetic-data helpers for tests and the benchmark (not on the verification path):
 * SecretKey.toPublicKey and SecretKey.sign as used by the reference's own tests
 * (test/e2e/chain/bls/multithread.test.ts:28-31).  Secret keys are 32-byte big-endian < r.
 */
int32_t lb_sk_to_pk(lb_engine* e, uint32_t n, const uint8_t* sks32, uint8_t* out48, uint8_t* out96);
int32_t lb_sign(lb_engine* e, uint32_t n, const uint8_t* sks32, const uint8_t* msgs32, uint8_t* out96);

/*
 * GPU-resident pubkey table (the epoch cache's index2pubkey,
 * state-transition/src/cache/pubkeyCache.ts:56-77, epochContext.ts:704).  Keys are decoded once
 * (48-byte compressed or 96-byte uncompressed, key_size says which) into affine Montgomery form in
 * HBM; out_status[n] gets LB_OK or the decode error (validate != 0 adds the infinity + subgroup
 * checks of PublicKey.keyValidate).  Appending extends the table (new validators); the table
 * belongs to the engine.
 */
int32_t lb_pubkey_table_append(lb_engine* e, uint32_t n, const uint8_t* keys, uint32_t key_size, int32_t validate,
                               int32_t* out_status, uint32_t* out_first_index);
uint32_t lb_pubkey_table_size(const lb_engine* e);
/*
 * Keys of the table (its first lb_pubkey_comb_size) that also carry fixed-base window entries: 72
 * affine points, 6.75 KiB per key and engine, filled inside lb_pubkey_table_append.  A set over
 * exactly one such key takes r * PK from them without doublings; every other set takes the GLV
 * ladder.  Environment, read at engine creation: LB_PK_COMB_MB = the entries' budget per engine in
 * MiB (default 8192, a 2^20-key table in full; keys past it use the ladder), LB_PK_COMB=0 = none.
 */
uint32_t lb_pubkey_comb_size(const lb_engine* e);
/* Sets whose r * PK the engine has taken from those entries so far, over all its batches. */
uint64_t lb_pubkey_comb_sets(const lb_engine* e);

/*
 * The signatures' subgroup check once per batch.  A batch on the bucket MSM whose blinding scalars
 * the engine draws itself skips the per-signature test: 64 random 0/1 combinations of the MSM's
 * bucket sums take it instead.  If one of them fails, the same batch runs again with the
 * per-signature test, so every code is what that test gives.  Returns the pipeline runs that took
 * the per-batch test so far; *fallbacks (may be NULL) gets how many of them ran again.
 * Environment, read at engine creation: LB_SUBGROUP_BATCH=0 = the per-signature test always.
 */
uint64_t lb_subgroup_batch_runs(const lb_engine* e, uint64_t* fallbacks);

/*
 * Like lb_batch_create, but set i aggregates table entries pk_indices[set_pk_offsets[i] ..
 * set_pk_offsets[i+1]) instead of carrying pubkey bytes (4 bytes per key on the bus instead of 96).
 * An index beyond the table makes that set's job reject with LB_ERR_ARGUMENT.  pk_indices may be
 * NULL only when no set carries a key (set_pk_offsets[n_sets] == 0), else LB_ERR_ARGUMENT.
 */
int32_t lb_batch_create_indexed(lb_engine* e, uint32_t n_jobs, const uint32_t* job_offsets,
                                const uint32_t* set_pk_offsets, const uint32_t* pk_indices,
                                const uint8_t* signing_roots, const uint8_t* signatures,
                                const uint32_t* sig_sizes, lb_batch** out);

/*
 * Per-stage device timings of the last lb_batch_verify / lb_batch_partial on this engine,
 * measured with HIP events on the engine's stream.  names[i] / ms[i] for i < *n (max cap).
 */
int32_t lb_engine_set_profiling(lb_engine* e, int32_t enable);
int32_t lb_engine_last_profile(lb_engine* e, const char** names, float* ms, int32_t cap, int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* LODESTAR_BLS_H */
