// Type declarations for the MI355X IBlsVerifier drop-in (lodestar_amd/js/index.js).
// Mirrors packages/beacon-node/src/chain/bls/interface.ts:3-46 and
// packages/state-transition/src/util/signatureSets.ts:5-22.

/** @chainsafe/bls PointFormat */
export declare const PointFormat: {compressed: "compressed"; uncompressed: "uncompressed"};

/**
 * A registered handle, a @chainsafe/bls PublicKey (serialised with toBytes("uncompressed"); a
 * 48-byte result is decompressed on the GPU), or raw 96- / 48-byte encodings.
 */
export type PublicKeyLike = Uint8Array | GpuPublicKey | {toBytes(format?: "compressed" | "uncompressed"): Uint8Array};

export declare const SignatureSetType: {single: "single"; aggregate: "aggregate"};

export type ISignatureSet =
  | {type: "single"; pubkey: PublicKeyLike; signingRoot: Uint8Array; signature: Uint8Array}
  | {type: "aggregate"; pubkeys: PublicKeyLike[]; signingRoot: Uint8Array; signature: Uint8Array};

export type VerifySignatureOpts = {
  batchable?: boolean;
  verifyOnMainThread?: boolean;
};

export interface IBlsVerifier {
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  close(): Promise<void>;
}

/** beacon-node/src/util/queue/errors.ts:3-6 */
export declare const QueueErrorCode: {
  QUEUE_ABORTED: "QUEUE_ERROR_QUEUE_ABORTED";
  QUEUE_MAX_LENGTH: "QUEUE_ERROR_QUEUE_MAX_LENGTH";
};

/** LodestarError<{code}>: message = type.code */
export declare class QueueError extends Error {
  constructor(type: {code: string});
  type: {code: string};
  getMetadata(): {code: string};
}

/** A key registered in the GPU-resident table (the epoch cache's index2pubkey entry). */
export declare class GpuPublicKey {
  readonly index: number;
  toBytes(): Uint8Array;
}

export declare class BlsGpuVerifier implements IBlsVerifier {
  /** engines: batches in flight on the device (default 2), each with its own streams + workspace; the
   *  pool also creates one engine for verifyOnMainThread calls, so it takes engines + 1 of the
   *  per-device cap (LB_MAX_ENGINES_PER_DEVICE, default 16) */
  /** devices: the device ordinals the pool spreads over, one slot of `engines` pool engines each ("all":
   *  every usable device; a repeated ordinal is a second, independent slot on that device).  One latency
   *  engine serves the whole verifier, on devices[0].  A queue is cut over the slots with an idle engine
   *  at equal cost quantiles, into packages of at least minPackageSets sets.  Without `devices`: one slot
   *  on `device` (default 0), which takes every queue whole. */
  /** modules as BlsMultiThreadWorkerPool's: metrics.blsThreadPool.* / metrics.bls.* get the same updates;
   *  addon replaces the native addon for this instance (tests) */
  constructor(opts?: {device?: number; devices?: number[] | "all"; engines?: number; minPackageSets?: number;
                      blsVerifyAllMultiThread?: boolean; latencyPartition?: boolean},
              modules?: {logger?: {error(msg: string, ctx?: object, e?: Error): void}; metrics?: unknown; addon?: object});
  /** the slots' device ordinals, in slot order */
  readonly devices: number[];
  readonly minPackageSets: number;
  /** 48- or 96-byte keys -> handles carrying their table index (validate: keyValidate checks) */
  registerPubkeys(keys: Uint8Array[], validate?: boolean): GpuPublicKey[];
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  /** state-transition verifySignatureSet: synchronous, throws the blst error on malformed input */
  verifySignatureSet(set: ISignatureSet): boolean;
  /** bls.Signature.aggregate(signatures).toBytes() (op pools), 96-byte compressed */
  aggregateSignatures(signatures: Uint8Array[], validate?: boolean): Uint8Array;
  close(): Promise<void>;
  readonly stats: {batches: number; jobs: number; sets: number; batchRetries: number; batchSigsSuccess: number;
    jobsInvalid: number; jobsError: number; jobWaitMs: number; deviceMs: number; mainThreadMs: number;
    /** packages launched per slot; dispatch rounds that launched more than one package */
    packagesPerSlot: number[]; splits: number};
}

/** Device work of one job (distributed.py's SET_COST per set + KEY_COST per pubkey). */
export declare function jobCost(job: ISignatureSet[] | {sets: ISignatureSet[]}): number;
/** k contiguous [lo, hi) ranges of whole jobs at equal cost quantiles (distributed.shard_jobs_by_cost). */
export declare function splitByCost(jobs: (ISignatureSet[] | {sets: ISignatureSet[]})[], k: number): [number, number][];
export declare const SET_COST: number;
export declare const KEY_COST: number;
export declare const DEFAULT_MIN_PACKAGE_SETS: number;

/** light-client isValidBlsAggregate (validation.ts:154-184) with its stage-prefixed errors */
export declare function isValidBlsAggregate(verifier: BlsGpuVerifier, publicKeys: PublicKeyLike[],
                                            message: Uint8Array, signature: Uint8Array): boolean;

export declare function chunkifyMaximizeChunkSize<T>(arr: T[], minPerChunk: number): T[][];
export declare const MAX_SIGNATURE_SETS_PER_JOB: number;
export declare const MAX_BUFFERED_SIGS: number;
export declare const MAX_BUFFER_WAIT_MS: number;

/**
 * The c-kzg module surface of lodestar_amd/js/kzg.js (`require("@lodestar/bls-mi355x/kzg")`, the
 * calls of packages/beacon-node/src/util/kzg.ts:15-65).  field "host" (default): scalar-field work
 * in BigInt, group work on the GPU; "device": both on the GPU (lb_kzg_blob_to_commitment ...).
 */
export type KzgOptions = {field?: "host" | "device"};
export interface CKzg {
  loadTrustedSetup(filePath: string, device?: number, options?: KzgOptions): void;
  blobToKzgCommitment(blob: Uint8Array): Uint8Array;
  computeAggregateKzgProof(blobs: Uint8Array[]): Uint8Array;
  verifyAggregateKzgProof(blobs: Uint8Array[], expectedKzgCommitments: Uint8Array[], kzgAggregatedProof: Uint8Array): boolean;
  /**
   * verifyAggregateKzgProof for many sidecars (a range-sync segment's blocks) in one pass over the
   * GPU, in either field mode: true, false, or the Error the single call would throw, per sidecar.
   */
  verifyAggregateKzgProofBatch(sidecars: KzgSidecar[]): (boolean | Error)[];
  /** One proof per blob (Deneb), c-kzg's names and shapes; z and y are 32 big-endian bytes below r. */
  computeBlobKzgProof(blob: Uint8Array, commitment: Uint8Array): Uint8Array;
  verifyBlobKzgProof(blob: Uint8Array, commitment: Uint8Array, proof: Uint8Array): boolean;
  verifyBlobKzgProofBatch(blobs: Uint8Array[], commitments: Uint8Array[], proofs: Uint8Array[]): boolean;
  computeKzgProof(blob: Uint8Array, zBytes: Uint8Array): [Uint8Array, Uint8Array];
  verifyKzgProof(commitment: Uint8Array, zBytes: Uint8Array, yBytes: Uint8Array, proof: Uint8Array): boolean;
  /**
   * verifyBlobKzgProofBatch for many groups (one group = one block's sidecars) in one pass over the
   * GPU, in either field mode: true, false, or the Error the single call would throw, per group.
   */
  verifyBlobKzgProofBatchMany(groups: KzgBlobGroup[]): (boolean | Error)[];
  /** c-kzg computeCells (EIP-7594): the blob's 128 cells of 2048 bytes, computed on the GPU. */
  computeCells(blob: Uint8Array): Uint8Array[];
  /**
   * c-kzg computeCellsAndKzgProofs: [the blob's 128 cells, their 128 proofs of 48 bytes], all proofs in
   * one FK20 pass over the GPU.
   */
  computeCellsAndKzgProofs(blob: Uint8Array): [Uint8Array[], Uint8Array[]];
  /**
   * computeCellsAndKzgProofs for many blobs in one pass: [cells, proofs], or the Error the single call
   * would throw, per blob.
   */
  computeCellsAndKzgProofsMany(blobs: Uint8Array[]): ([Uint8Array[], Uint8Array[]] | Error)[];
  /**
   * c-kzg recoverCellsAndKzgProofs: [all 128 cells, all 128 proofs] of the blob that the given 64 .. 128
   * cells (with their strictly ascending indices) belong to, on the GPU.  Throws BLST_BAD_SCALAR for a
   * cell element >= r and BLST_VERIFY_FAIL where more than 64 cells lie on no one polynomial of degree
   * < 4096 (stricter than c-kzg).
   */
  recoverCellsAndKzgProofs(cellIndices: number[], cells: Uint8Array[]): [Uint8Array[], Uint8Array[]];
  /**
   * recoverCellsAndKzgProofs for many blobs in one pass: [cells, proofs], or the Error the single call
   * would throw, per blob.
   */
  recoverCellsAndKzgProofsMany(groups: KzgRecoverGroup[]): ([Uint8Array[], Uint8Array[]] | Error)[];
  /** c-kzg verifyCellKzgProofBatch: one commitment, cell index, cell and proof per cell; on the GPU. */
  verifyCellKzgProofBatch(commitments: Uint8Array[], cellIndices: number[], cells: Uint8Array[], proofs: Uint8Array[]): boolean;
  /**
   * verifyCellKzgProofBatch for many groups (data-column sidecars) in one pass over the GPU: true,
   * false, or the Error the single call would throw, per group.
   */
  verifyCellKzgProofBatchMany(groups: KzgCellGroup[]): (boolean | Error)[];
  readonly BYTES_PER_CELL: 2048;
  readonly CELLS_PER_EXT_BLOB: 128;
  readonly G1_INFINITY48: Uint8Array;
}
/** One verifyCellKzgProofBatch call: one entry of each array per cell. */
export type KzgCellGroup = {commitments: Uint8Array[]; cellIndices: number[]; cells: Uint8Array[]; proofs: Uint8Array[]};
/** One recoverCellsAndKzgProofs call: 64 .. 128 cells of one blob and their indices, ascending. */
export type KzgRecoverGroup = {cellIndices: number[]; cells: Uint8Array[]};
export type KzgSidecar = {blobs: Uint8Array[]; commitments: Uint8Array[]; proof: Uint8Array};
/** One verifyBlobKzgProofBatch call: one proof per blob. */
export type KzgBlobGroup = {blobs: Uint8Array[]; commitments: Uint8Array[]; proofs: Uint8Array[]};

// ---- block signature sets from SSZ bytes (js/signing_roots.js; addon.blockSetsFromSsz = lb_block_sets_from_ssz)
/** What getBlockSignatureSets reads from the cached state; only the keys are needed from it here. */
export type StateView = {
  genesisValidatorsRoot: Uint8Array; forkPreviousVersion: Uint8Array; forkCurrentVersion: Uint8Array;
  forkEpoch: number; slot?: number; pubkey: (index: number) => unknown;
  beaconCommittee: (slot: number, index: number) => number[]; syncCommittee: () => unknown[];
  keyFromBytes?: (bytes48: Uint8Array) => unknown; forkSeq?: (slot: number) => number;
};
export type BlockSignatureSet = {
  name: "randao" | "proposer_slashing" | "attester_slashing" | "attestation" | "voluntary_exit" | "proposer" |
    "sync_aggregate" | "bls_to_execution_change";
  type: "single" | "aggregate"; pubkey?: unknown; pubkeys?: unknown[]; signingRoot: Uint8Array; signature: Uint8Array;
};
/** rows [b * 199, b * 199 + nSets[b]) of kind / roots (32 B) / sigs (96 B) / ref (4 words) belong to block b */
export type BlockSetRows = {status: Int32Array; nSets: Uint32Array; kind: Uint32Array; roots: Uint8Array;
  sigs: Uint8Array; ref: BigUint64Array};
export interface SigningRootsAddon {
  blockSetsFromSsz(engine: unknown, byteOffsets: Uint32Array, ssz: Uint8Array, forks: Uint32Array, domains: Uint8Array,
    forkEpochs: BigUint64Array, stateSlots: BigUint64Array, flags: number): BlockSetRows;
}
/** require("lodestar_amd/js/signing_roots").getBlockSignatureSetsFromSsz: the sets of SignedBeaconBlocks handed
 * over as SSZ bytes (phase0 .. capella; at most 64 blocks and 64 MiB), or an Error per rejected block */
export declare function getBlockSignatureSetsFromSsz(blocks: Uint8Array[], states: StateView | StateView[],
  opts: {engine: unknown; skipProposerSignature?: boolean}): (BlockSignatureSet[] | Error)[];
