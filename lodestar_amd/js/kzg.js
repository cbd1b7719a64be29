"use strict";
/**
 * The `c-kzg` module surface Lodestar binds (packages/beacon-node/src/util/kzg.ts:15-65):
 *   loadTrustedSetup(filePath), blobToKzgCommitment(blob), computeAggregateKzgProof(blobs),
 *   verifyAggregateKzgProof(blobs, expectedKzgCommitments, kzgAggregatedProof)
 * so `ckzg = require("@lodestar/bls-mi355x/kzg")` replaces `await import("c-kzg")` (initCKZG).
 *
 * The scalar-field work runs here in BigInt (inverse NTT of the blob's evaluations to monomial
 * coefficients, the Fiat-Shamir transcript of the EIP-4844 spec's compute_challenges, Horner
 * evaluation, the quotient by synthetic division); the group work runs on the GPU through the
 * addon (kzgLoadSetup / g1Lincomb / kzgVerifyProof -> include/lodestar_bls.h lb_kzg_*), as in
 * lodestar_amd/kzg.py, which it mirrors line for line.  The setup file is the text format
 * kzg.ts writes (trustedSetupJsonToTxt: "4096", "65", then hex points) or Lodestar's
 * trusted_setup.bin.  Field elements are big-endian (blobsSidecar.ts:138-150).  Parity with
 * c-kzg's bytes is unpinned (DESIGN.md §5.1); calls are synchronous, as c-kzg's are.
 *
 * loadTrustedSetup(filePath, device, {field: "device"}) moves the scalar-field work to the GPU too:
 * the three calls then hand the blobs' bytes to the addon's blob-level calls (kzgBlobToCommitment /
 * kzgComputeAggregateProof / kzgVerifyAggregateProof -> lb_kzg_blob_to_commitment ...) and no BigInt
 * arithmetic runs.  The default, {field: "host"}, is the BigInt path above; both give the same bytes.
 *
 * verifyAggregateKzgProofBatch(sidecars) is not part of c-kzg: many sidecars (a range-sync segment's
 * blocks) in one pass over the GPU, one verdict per sidecar, in either field mode.
 *
 * The per-blob proof form that shipped in Deneb is here too, under c-kzg's names and shapes:
 * computeBlobKzgProof, verifyBlobKzgProof, verifyBlobKzgProofBatch, computeKzgProof, verifyKzgProof,
 * and verifyBlobKzgProofBatchMany(groups) for many blocks' sidecars in one pass (see below).
 */
const crypto = require("crypto");
const fs = require("fs");
const path = require("path");

const addon = require(path.join(__dirname, "..", "napi", "lodestar_bls.node"));

const R = 52435875175126190479447740508185965837690552500527637822603658699938581184513n;
const N = 4096;
const BYTES_PER_BLOB = 32 * N;
const DOMAIN = Buffer.from("FSBLOBVERIFY_V1_", "ascii");

function powmod(b, e) {
  let r = 1n;
  b %= R;
  while (e > 0n) {
    if (e & 1n) r = (r * b) % R;
    b = (b * b) % R;
    e >>= 1n;
  }
  return r;
}
const mod = (a) => ((a % R) + R) % R;

const BRP = (() => {
  const bits = Math.log2(N);
  const out = new Array(N);
  for (let i = 0; i < N; i++) {
    let r = 0;
    for (let b = 0; b < bits; b++) if (i & (1 << b)) r |= 1 << (bits - 1 - b);
    out[i] = r;
  }
  return out;
})();
const ROOTS = (() => {
  const w = powmod(7n, (R - 1n) / BigInt(N));
  const out = new Array(N);
  let x = 1n;
  for (let i = 0; i < N; i++) {
    out[i] = x;
    x = (x * w) % R;
  }
  return out;
})();

function ntt(a, roots) {
  const n = a.length;
  const v = new Array(n);
  for (let i = 0; i < n; i++) v[i] = a[BRP[i]];
  for (let m = 1; m < n; m *= 2) {
    const step = n / (2 * m);
    for (let s = 0; s < n; s += 2 * m) {
      for (let j = 0; j < m; j++) {
        const u = v[s + j];
        const t = (v[s + j + m] * roots[j * step]) % R;
        v[s + j] = (u + t) % R;
        v[s + j + m] = mod(u - t);
      }
    }
  }
  return v;
}

function bytesToBig(b) {
  return BigInt("0x" + (Buffer.from(b).toString("hex") || "0"));
}
function bigToBytes(x, n, little) {
  const hex = x.toString(16).padStart(2 * n, "0");
  const buf = Buffer.from(hex, "hex");
  return little ? Buffer.from(buf.reverse()) : buf;
}

function blobToPolynomial(blob) {
  if (!(blob instanceof Uint8Array) || blob.length !== BYTES_PER_BLOB) throw Error("blob length != 131072");
  const out = new Array(N);
  for (let i = 0; i < N; i++) {
    const v = bytesToBig(blob.subarray(32 * i, 32 * i + 32));
    if (v >= R) throw Error("blob field element >= BLS_MODULUS");
    out[i] = v;
  }
  return out;
}
function evaluationsToCoefficients(poly) {
  const nat = new Array(N);
  for (let i = 0; i < N; i++) nat[BRP[i]] = poly[i];
  const inv = new Array(N);
  for (let k = 0; k < N; k++) inv[k] = ROOTS[(N - k) % N];
  const invN = powmod(BigInt(N), R - 2n);
  return ntt(nat, inv).map((c) => (c * invN) % R);
}
function evaluate(coeffs, z) {
  let y = 0n;
  for (let k = coeffs.length - 1; k >= 0; k--) y = (y * z + coeffs[k]) % R;
  return y;
}
function quotient(coeffs, z) {
  const q = new Array(coeffs.length - 1);
  let acc = 0n;
  for (let k = coeffs.length - 1; k > 0; k--) {
    acc = (acc * z + coeffs[k]) % R;
    q[k - 1] = acc;
  }
  return q;
}
function hashToBlsField(data) {
  return bytesToBig(crypto.createHash("sha256").update(data).digest()) % R;
}
function computeChallenges(polys, commitments) {
  const parts = [DOMAIN, bigToBytes(BigInt(N), 8, false), bigToBytes(BigInt(polys.length), 8, false)];
  for (const p of polys) for (const v of p) parts.push(bigToBytes(v, 32, false));
  for (const c of commitments) parts.push(Buffer.from(c));
  const h = crypto.createHash("sha256").update(Buffer.concat(parts)).digest();
  const r = hashToBlsField(Buffer.concat([h, Buffer.from([0])]));
  const powers = [];
  let x = 1n;
  for (let i = 0; i < commitments.length; i++) {
    powers.push(x);
    x = (x * r) % R;
  }
  return {rPowers: powers, x: hashToBlsField(Buffer.concat([h, Buffer.from([1])]))};
}
function scalarsLE(vals) {
  const out = new Uint8Array(32 * vals.length);
  vals.forEach((v, i) => out.set(bigToBytes(v, 32, true), 32 * i));
  return out;
}

let engine = null;
function requireSetup() {
  if (!engine) throw Error("c-kzg library not loaded");
}

function parseSetup(filePath) {
  const raw = fs.readFileSync(filePath);
  let g1 = [];
  let g2 = [];
  if (raw.length === 8 + 4096 * 48 + 65 * 96) {
    for (let i = 0; i < 4096; i++) g1.push(raw.subarray(8 + 48 * i, 8 + 48 * (i + 1)));
    const base = 8 + 4096 * 48;
    for (let i = 0; i < 65; i++) g2.push(raw.subarray(base + 96 * i, base + 96 * (i + 1)));
  } else {
    const lines = raw.toString("utf8").split(/\s+/).filter((l) => l.length);
    const n1 = parseInt(lines[0], 10);
    const n2 = parseInt(lines[1], 10);
    g1 = lines.slice(2, 2 + n1).map((h) => Buffer.from(h, "hex"));
    g2 = lines.slice(2 + n1, 2 + n1 + n2).map((h) => Buffer.from(h, "hex"));
  }
  return {g1: Buffer.concat(g1), g2: Buffer.concat(g2)};
}

let field = "host";
function loadTrustedSetup(filePath, device = 0, options = {field: "host"}) {
  const f = (options && options.field) || "host";
  if (f !== "host" && f !== "device") throw Error('loadTrustedSetup: options.field must be "host" or "device"');
  const {g1, g2} = parseSetup(filePath);
  const e = engine || addon.createEngine(device);
  addon.kzgLoadSetup(e, new Uint8Array(g1), new Uint8Array(g2));
  engine = e;
  field = f;
}

function checkBlob(blob) {
  if (!(blob instanceof Uint8Array) || blob.length !== BYTES_PER_BLOB) throw Error("blob length != 131072");
}
function concatBlobs(blobs) {
  const out = new Uint8Array(BYTES_PER_BLOB * blobs.length);
  blobs.forEach((b, i) => {
    checkBlob(b);
    out.set(b, BYTES_PER_BLOB * i);
  });
  return out;
}

function commitCoefficients(coeffs) {
  return addon.g1Lincomb(engine, scalarsLE(coeffs));
}
function blobToKzgCommitment(blob) {
  requireSetup();
  if (field === "device") {
    checkBlob(blob);
    return addon.kzgBlobToCommitment(engine, blob);
  }
  return commitCoefficients(evaluationsToCoefficients(blobToPolynomial(blob)));
}
function aggregate(blobs, commitments) {
  const polys = blobs.map(blobToPolynomial);
  const {rPowers, x} = computeChallenges(polys, commitments);
  const agg = new Array(N);
  for (let i = 0; i < N; i++) {
    let s = 0n;
    for (let j = 0; j < polys.length; j++) s += rPowers[j] * polys[j][i];
    agg[i] = s % R;
  }
  return {agg, rPowers, x};
}
// compressed point at infinity: the proof of zero blobs (the zero polynomial)
const G1_INFINITY48 = Uint8Array.from([0xc0, ...new Array(47).fill(0)]);

function computeAggregateKzgProof(blobs) {
  requireSetup();
  // chain.ts:402 calls this for every produced block, blobless ones included
  if (!blobs.length) return G1_INFINITY48.slice();
  if (field === "device") return addon.kzgComputeAggregateProof(engine, concatBlobs(blobs));
  const commitments = blobs.map(blobToKzgCommitment);
  const {agg, x} = aggregate(blobs, commitments);
  return commitCoefficients(quotient(evaluationsToCoefficients(agg), x));
}
function verifyAggregateKzgProof(blobs, expectedKzgCommitments, kzgAggregatedProof) {
  requireSetup();
  if (blobs.length !== expectedKzgCommitments.length) throw Error("blobs / commitments length mismatch");
  if (field === "device") {
    const cm = new Uint8Array(48 * expectedKzgCommitments.length);
    expectedKzgCommitments.forEach((c, i) => {
      if (c.length !== 48) throw Error("commitment length != 48");
      cm.set(c, 48 * i);
    });
    return addon.kzgVerifyAggregateProof(engine, concatBlobs(blobs), cm, kzgAggregatedProof);
  }
  if (!blobs.length) {
    // aggregated commitment = infinity, y = 0: true iff the proof is infinity (still decoded)
    const {x} = computeChallenges([], []);
    return addon.kzgVerifyProof(engine, G1_INFINITY48, bigToBytes(x, 32, true), bigToBytes(0n, 32, true), kzgAggregatedProof);
  }
  const {agg, rPowers, x} = aggregate(blobs, expectedKzgCommitments);
  const pts = new Uint8Array(48 * expectedKzgCommitments.length);
  expectedKzgCommitments.forEach((c, i) => pts.set(c, 48 * i));
  const c = addon.g1Lincomb(engine, scalarsLE(rPowers), pts);
  const y = evaluate(evaluationsToCoefficients(agg), x);
  return addon.kzgVerifyProof(engine, c, bigToBytes(x, 32, true), bigToBytes(y, 32, true), kzgAggregatedProof);
}

// verifyAggregateKzgProof for many sidecars (a range-sync segment's blocks) in one pass over the GPU
// (kzgVerifyAggregateProofBatch -> lb_kzg_verify_aggregate_proof_batch), in either field mode.
// sidecars: {blobs, commitments, proof}[].  One entry per sidecar: true, false, or the Error the
// single call would throw -- returned, not thrown, so one bad sidecar does not hide the others.
// Malformed input throws before anything is sent.
function verifyAggregateKzgProofBatch(sidecars) {
  requireSetup();
  const offsets = new Uint32Array(sidecars.length + 1);
  const allBlobs = [];
  const allComms = [];
  sidecars.forEach((s, k) => {
    if (s.blobs.length !== s.commitments.length) throw Error("blobs / commitments length mismatch");
    s.commitments.forEach((c) => {
      if (c.length !== 48) throw Error("commitment length != 48");
      allComms.push(c);
    });
    if (s.proof.length !== 48) throw Error("proof length != 48");
    allBlobs.push(...s.blobs);
    offsets[k + 1] = allBlobs.length;
  });
  if (!sidecars.length) return [];
  const cm = new Uint8Array(48 * allComms.length);
  allComms.forEach((c, i) => cm.set(c, 48 * i));
  const pr = new Uint8Array(48 * sidecars.length);
  sidecars.forEach((s, k) => pr.set(s.proof, 48 * k));
  const ok = addon.kzgVerifyAggregateProofBatch(engine, concatBlobs(allBlobs), offsets, cm, pr);
  return Array.from(ok, (v) => (v < 0 ? Error(addon.errorName(-v)) : v === 1));
}

// ------------------------------------------------------------------ one proof per blob (Deneb)
// The c-kzg surface of the shipped form of EIP-4844: computeBlobKzgProof, verifyBlobKzgProof,
// verifyBlobKzgProofBatch, computeKzgProof, verifyKzgProof.  Every blob has its own transcript,
//   z = hash_to_bls_field(FS_DOMAIN || 4096 as 16 bytes BE || blob || commitment),
// and a batch its own combiner r (computeBatchR).  verifyBlobKzgProofBatch always runs on the GPU
// (kzgVerifyBlobProofBatch -> lb_kzg_verify_blob_proof_batch); computeBlobKzgProof and
// verifyBlobKzgProof honour the field mode and give the same bytes and verdicts in both.
const RC_DOMAIN = Buffer.from("RCKZGBATCH___V1_", "ascii");

function check48(p, what) {
  if (!(p instanceof Uint8Array) || p.length !== 48) throw Error(what + " length != 48");
}
function computeChallenge(blob, commitment) {
  checkBlob(blob);
  check48(commitment, "commitment");
  return hashToBlsField(Buffer.concat([DOMAIN, bigToBytes(BigInt(N), 16, false), Buffer.from(blob), Buffer.from(commitment)]));
}
function computeBatchR(commitments, zs, ys, proofs) {
  const parts = [RC_DOMAIN, bigToBytes(BigInt(N), 8, false), bigToBytes(BigInt(commitments.length), 8, false)];
  commitments.forEach((c, i) => {
    parts.push(Buffer.from(c), bigToBytes(zs[i], 32, false), bigToBytes(ys[i], 32, false), Buffer.from(proofs[i]));
  });
  return hashToBlsField(Buffer.concat(parts));
}
function fieldElement(b, what) {
  if (!(b instanceof Uint8Array) || b.length !== 32) throw Error(what + " length != 32");
  const v = bytesToBig(b);
  if (v >= R) throw Error("BLST_BAD_SCALAR");
  return v;
}
// decodes and subgroup-checks a point given by the caller (throws the blst-style name)
function validateG1(p) {
  addon.g1Lincomb(engine, scalarsLE([1n]), p);
}

function computeBlobKzgProof(blob, commitment) {
  requireSetup();
  checkBlob(blob);
  check48(commitment, "commitment");
  if (field === "device") return addon.kzgComputeBlobProofs(engine, blob, commitment);
  validateG1(commitment);
  const coeffs = evaluationsToCoefficients(blobToPolynomial(blob));
  return commitCoefficients(quotient(coeffs, computeChallenge(blob, commitment)));
}

// verifyBlobKzgProofBatch for many groups (one group = one block's sidecars) in one pass over the
// GPU, in either field mode.  groups: {blobs, commitments, proofs}[], one proof per blob.  One entry
// per group: true, false, or the Error the single call would throw -- returned, not thrown.
// Malformed input throws before anything is sent.
function verifyBlobKzgProofBatchMany(groups) {
  requireSetup();
  const offsets = new Uint32Array(groups.length + 1);
  const allBlobs = [];
  const allComms = [];
  const allProofs = [];
  groups.forEach((g, k) => {
    if (g.blobs.length !== g.commitments.length || g.blobs.length !== g.proofs.length) {
      throw Error("blobs / commitments / proofs length mismatch");
    }
    g.commitments.forEach((c) => check48(c, "commitment"));
    g.proofs.forEach((p) => check48(p, "proof"));
    allBlobs.push(...g.blobs);
    allComms.push(...g.commitments);
    allProofs.push(...g.proofs);
    offsets[k + 1] = allBlobs.length;
  });
  if (!groups.length) return [];
  const cm = new Uint8Array(48 * allComms.length);
  const pr = new Uint8Array(48 * allProofs.length);
  allComms.forEach((c, i) => cm.set(c, 48 * i));
  allProofs.forEach((p, i) => pr.set(p, 48 * i));
  const ok = addon.kzgVerifyBlobProofBatch(engine, concatBlobs(allBlobs), offsets, cm, pr);
  return Array.from(ok, (v) => (v < 0 ? Error(addon.errorName(-v)) : v === 1));
}
function verifyBlobKzgProofBatch(blobs, commitments, proofs) {
  const res = verifyBlobKzgProofBatchMany([{blobs, commitments, proofs}])[0];
  if (res instanceof Error) throw res;
  return res;
}
function verifyBlobKzgProof(blob, commitment, proof) {
  requireSetup();
  if (field === "device") return verifyBlobKzgProofBatch([blob], [commitment], [proof]);
  checkBlob(blob);
  check48(commitment, "commitment");
  check48(proof, "proof");
  validateG1(commitment); // the commitment's error comes before the blob's
  const z = computeChallenge(blob, commitment);
  const y = evaluate(evaluationsToCoefficients(blobToPolynomial(blob)), z);
  return addon.kzgVerifyProof(engine, commitment, bigToBytes(z, 32, true), bigToBytes(y, 32, true), proof);
}
// computeKzgProof(blob, zBytes) -> [proof, yBytes] and verifyKzgProof(commitment, zBytes, yBytes,
// proof): z and y as 32 big-endian bytes, each below r.  The field work of computeKzgProof is
// BigInt in either mode (the addon binds no single-point proof call); the commitment to the
// quotient and the pairing check run on the GPU.
function computeKzgProof(blob, zBytes) {
  requireSetup();
  const z = fieldElement(zBytes, "z");
  const coeffs = evaluationsToCoefficients(blobToPolynomial(blob));
  return [commitCoefficients(quotient(coeffs, z)), new Uint8Array(bigToBytes(evaluate(coeffs, z), 32, false))];
}
function verifyKzgProof(commitment, zBytes, yBytes, proof) {
  requireSetup();
  check48(commitment, "commitment");
  check48(proof, "proof");
  const z = fieldElement(zBytes, "z");
  const y = fieldElement(yBytes, "y");
  return addon.kzgVerifyProof(engine, commitment, bigToBytes(z, 32, true), bigToBytes(y, 32, true), proof);
}

// ------------------------------------------------------------------ cells (EIP-7594, PeerDAS)
// c-kzg computeCells, computeCellsAndKzgProofs, recoverCellsAndKzgProofs(cellIndices, cells) and
// verifyCellKzgProofBatch(commitments, cellIndices, cells, proofs), always on the GPU (kzgComputeCells ->
// lb_kzg_compute_cells, kzgComputeCellsAndProofs -> lb_kzg_compute_cells_and_proofs: FK20,
// kzgRecoverCellsAndProofs -> lb_kzg_recover_cells_and_proofs, kzgVerifyCellProofBatch ->
// lb_kzg_verify_cell_proof_batch), in either field mode.  The batch's combiner (computeCellBatchR:
// the commitments deduplicated in order of first appearance) hashes only the caller's bytes; like
// the other transcripts its byte parity with c-kzg is unpinned, and no verdict depends on it.
const BYTES_PER_CELL = 2048;
const CELLS_PER_EXT_BLOB = 128;
const CELL_DOMAIN = Buffer.from("RCKZGCBATCH__V1_", "ascii");

function checkCell(c) {
  if (!(c instanceof Uint8Array) || c.length !== BYTES_PER_CELL) throw Error("cell length != 2048");
}
function checkCellIndex(i) {
  if (!Number.isInteger(i) || i < 0 || i >= CELLS_PER_EXT_BLOB) throw Error("cell index not below 128");
}
function computeCellBatchR(commitments, cellIndices, cells, proofs) {
  const distinct = [];
  const indexOf = new Map();
  const ci = commitments.map((c) => {
    const key = Buffer.from(c).toString("hex");
    if (!indexOf.has(key)) {
      indexOf.set(key, distinct.length);
      distinct.push(Buffer.from(c));
    }
    return indexOf.get(key);
  });
  const u64 = (v) => bigToBytes(BigInt(v), 8, false);
  const parts = [CELL_DOMAIN, u64(N), u64(64), u64(distinct.length), u64(cells.length), ...distinct];
  cells.forEach((cell, k) => parts.push(u64(ci[k]), u64(cellIndices[k]), Buffer.from(cell), Buffer.from(proofs[k])));
  return hashToBlsField(Buffer.concat(parts));
}
function computeCells(blob) {
  requireSetup();
  checkBlob(blob);
  const all = addon.kzgComputeCells(engine, blob);
  return Array.from({length: CELLS_PER_EXT_BLOB}, (_, i) => all.slice(BYTES_PER_CELL * i, BYTES_PER_CELL * (i + 1)));
}
// One entry per blob: [cells, proofs] (128 of each) as c-kzg's computeCellsAndKzgProofs gives them, or
// the Error the single call would throw -- returned, not thrown.  A wrong blob length throws before
// anything is sent; more than 128 blobs go in passes.
const MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL = 128;
function computeCellsAndKzgProofsMany(blobs) {
  requireSetup();
  blobs.forEach(checkBlob);
  const res = [];
  for (let lo = 0; lo < blobs.length; lo += MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL) {
    const part = blobs.slice(lo, lo + MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL);
    const flat = new Uint8Array(BYTES_PER_BLOB * part.length);
    part.forEach((b, i) => flat.set(b, BYTES_PER_BLOB * i));
    const {cells, proofs, status} = addon.kzgComputeCellsAndProofs(engine, flat);
    part.forEach((_, b) => {
      if (status[b] !== 0) {
        res.push(Error(addon.errorName(status[b])));
        return;
      }
      const c0 = b * CELLS_PER_EXT_BLOB * BYTES_PER_CELL;
      const p0 = b * CELLS_PER_EXT_BLOB * 48;
      res.push([
        Array.from({length: CELLS_PER_EXT_BLOB}, (_x, i) => cells.slice(c0 + BYTES_PER_CELL * i, c0 + BYTES_PER_CELL * (i + 1))),
        Array.from({length: CELLS_PER_EXT_BLOB}, (_x, i) => proofs.slice(p0 + 48 * i, p0 + 48 * (i + 1))),
      ]);
    });
  }
  return res;
}
function computeCellsAndKzgProofs(blob) {
  const res = computeCellsAndKzgProofsMany([blob])[0];
  if (res instanceof Error) throw res;
  return res;
}
// groups: {cellIndices, cells}[], one blob each: any 64 .. 128 of its cells with their strictly ascending
// indices.  One entry per blob: [cells, proofs] (all 128 of each), or the Error the single call would
// throw -- returned, not thrown: BLST_BAD_SCALAR for a cell element >= r, BLST_VERIFY_FAIL where more
// than 64 cells lie on no one polynomial of degree < 4096 (stricter than c-kzg).  Malformed input
// throws before anything is sent; more than 128 blobs go in passes.
function checkRecoverGroup(g) {
  if (!g || !Array.isArray(g.cellIndices) || !Array.isArray(g.cells)) throw Error("cellIndices and cells: arrays");
  if (g.cellIndices.length !== g.cells.length) throw Error("cellIndices / cells length mismatch");
  if (g.cells.length < CELLS_PER_EXT_BLOB / 2 || g.cells.length > CELLS_PER_EXT_BLOB) throw Error("cell count not in 64 .. 128");
  g.cells.forEach(checkCell);
  g.cellIndices.forEach(checkCellIndex);
  for (let k = 1; k < g.cellIndices.length; k++) {
    if (g.cellIndices[k] <= g.cellIndices[k - 1]) throw Error("cell indices not strictly ascending");
  }
}
function recoverCellsAndKzgProofsMany(groups) {
  groups.forEach(checkRecoverGroup);
  requireSetup();
  const res = [];
  for (let lo = 0; lo < groups.length; lo += MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL) {
    const part = groups.slice(lo, lo + MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL);
    const offsets = new Uint32Array(part.length + 1);
    part.forEach((g, k) => (offsets[k + 1] = offsets[k] + g.cells.length));
    const idx = new Uint32Array(offsets[part.length]);
    const flat = new Uint8Array(BYTES_PER_CELL * offsets[part.length]);
    part.forEach((g, k) => {
      idx.set(g.cellIndices, offsets[k]);
      g.cells.forEach((c, i) => flat.set(c, BYTES_PER_CELL * (offsets[k] + i)));
    });
    const {cells, proofs, status} = addon.kzgRecoverCellsAndProofs(engine, offsets, idx, flat);
    part.forEach((_, b) => {
      if (status[b] !== 0) {
        res.push(Error(addon.errorName(status[b])));
        return;
      }
      const c0 = b * CELLS_PER_EXT_BLOB * BYTES_PER_CELL;
      const p0 = b * CELLS_PER_EXT_BLOB * 48;
      res.push([
        Array.from({length: CELLS_PER_EXT_BLOB}, (_x, i) => cells.slice(c0 + BYTES_PER_CELL * i, c0 + BYTES_PER_CELL * (i + 1))),
        Array.from({length: CELLS_PER_EXT_BLOB}, (_x, i) => proofs.slice(p0 + 48 * i, p0 + 48 * (i + 1))),
      ]);
    });
  }
  return res;
}
function recoverCellsAndKzgProofs(cellIndices, cells) {
  const res = recoverCellsAndKzgProofsMany([{cellIndices, cells}])[0];
  if (res instanceof Error) throw res;
  return res;
}
// groups: {commitments, cellIndices, cells, proofs}[], one of each per cell.  One entry per group:
// true, false, or the Error the single call would throw -- returned, not thrown.  Malformed input
// throws before anything is sent.
function verifyCellKzgProofBatchMany(groups) {
  requireSetup();
  const offsets = new Uint32Array(groups.length + 1);
  const comms = [];
  const idx = [];
  const cells = [];
  const proofs = [];
  groups.forEach((g, k) => {
    const n = g.cells.length;
    if (g.commitments.length !== n || g.cellIndices.length !== n || g.proofs.length !== n) {
      throw Error("commitments / cellIndices / cells / proofs length mismatch");
    }
    g.commitments.forEach((c) => check48(c, "commitment"));
    g.proofs.forEach((p) => check48(p, "proof"));
    g.cells.forEach(checkCell);
    g.cellIndices.forEach(checkCellIndex);
    comms.push(...g.commitments);
    idx.push(...g.cellIndices);
    cells.push(...g.cells);
    proofs.push(...g.proofs);
    offsets[k + 1] = cells.length;
  });
  if (!groups.length) return [];
  const cm = new Uint8Array(48 * comms.length);
  const pr = new Uint8Array(48 * proofs.length);
  const ce = new Uint8Array(BYTES_PER_CELL * cells.length);
  comms.forEach((c, i) => cm.set(c, 48 * i));
  proofs.forEach((p, i) => pr.set(p, 48 * i));
  cells.forEach((c, i) => ce.set(c, BYTES_PER_CELL * i));
  const ok = addon.kzgVerifyCellProofBatch(engine, offsets, cm, Uint32Array.from(idx), ce, pr);
  return Array.from(ok, (v) => (v < 0 ? Error(addon.errorName(-v)) : v === 1));
}
function verifyCellKzgProofBatch(commitments, cellIndices, cells, proofs) {
  const res = verifyCellKzgProofBatchMany([{commitments, cellIndices, cells, proofs}])[0];
  if (res instanceof Error) throw res;
  return res;
}

module.exports = {
  loadTrustedSetup,
  computeCells,
  computeCellsAndKzgProofs,
  computeCellsAndKzgProofsMany,
  recoverCellsAndKzgProofs,
  recoverCellsAndKzgProofsMany,
  verifyCellKzgProofBatch,
  verifyCellKzgProofBatchMany,
  BYTES_PER_CELL,
  CELLS_PER_EXT_BLOB,
  blobToKzgCommitment,
  computeAggregateKzgProof,
  verifyAggregateKzgProof,
  verifyAggregateKzgProofBatch,
  computeBlobKzgProof,
  verifyBlobKzgProof,
  verifyBlobKzgProofBatch,
  verifyBlobKzgProofBatchMany,
  computeKzgProof,
  verifyKzgProof,
  G1_INFINITY48,
  // host field work, exported for tests
  _internal: {evaluationsToCoefficients, evaluate, quotient, computeChallenges, computeChallenge, computeBatchR, computeCellBatchR, ROOTS, BRP, R},
};
