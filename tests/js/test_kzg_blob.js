"use strict";
// The per-blob (Deneb) c-kzg names of lodestar_amd/js/kzg.js: computeBlobKzgProof, verifyBlobKzgProof,
// verifyBlobKzgProofBatch(Many), computeKzgProof, verifyKzgProof.
//   node test_kzg_blob.js cpu            argument validation and the two transcripts (no GPU call);
//                                        prints z and r values for tests/test_js_kzg_blob.py to
//                                        compare with Python's
//   node test_kzg_blob.js gpu <file>     <file>: six blobs; groups of 0, 1, 2, 0 and 3 of them in
//                                        both field modes; prints the bytes and verdicts for the
//                                        Python surface to be compared with
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const kzg = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));
const SETUP = path.join(__dirname, "..", "..", "lodestar_amd", "trusted_setup.bin");
const mode = process.argv[2];
const hex = (b) => Buffer.from(b).toString("hex");
const show = (v) => (v instanceof Error ? "Error: " + v.message : v);

function sequentialBlob(off) {
  const b = new Uint8Array(4096 * 32);
  const dv = new DataView(b.buffer);
  for (let i = 0; i < 4096; i++) dv.setUint32(i * 32, (i + off) >>> 0);
  return b;
}

if (mode === "cpu") {
  const {computeChallenge, computeBatchR, R} = kzg._internal;
  for (const name of ["computeBlobKzgProof", "verifyBlobKzgProof", "verifyBlobKzgProofBatch", "verifyBlobKzgProofBatchMany",
                      "computeKzgProof", "verifyKzgProof"]) {
    assert.strictEqual(typeof kzg[name], "function", name);
  }
  const blob = sequentialBlob(3);
  const c = new Uint8Array(48).fill(0x11);
  const p = new Uint8Array(48).fill(0x22);
  // nothing runs before a setup is loaded
  assert.throws(() => kzg.computeBlobKzgProof(blob, c), /not loaded/);
  assert.throws(() => kzg.verifyBlobKzgProof(blob, c, p), /not loaded/);
  assert.throws(() => kzg.verifyBlobKzgProofBatch([blob], [c], [p]), /not loaded/);
  assert.throws(() => kzg.verifyBlobKzgProofBatchMany([]), /not loaded/);
  assert.throws(() => kzg.computeKzgProof(blob, new Uint8Array(32)), /not loaded/);
  assert.throws(() => kzg.verifyKzgProof(c, new Uint8Array(32), new Uint8Array(32), p), /not loaded/);
  // the transcript's own validation
  assert.throws(() => computeChallenge(blob.subarray(1), c), /blob length/);
  assert.throws(() => computeChallenge(blob, c.subarray(1)), /commitment length/);
  const z = computeChallenge(blob, c);
  const z0 = computeChallenge(new Uint8Array(4096 * 32), c);
  assert.ok(z < R && z0 < R && z !== z0);
  const zs = [z, 0n, R - 1n];
  const ys = [5n, R - 1n, 0n];
  const r = [0, 1, 3].map((n) => computeBatchR(new Array(n).fill(c), zs.slice(0, n), ys.slice(0, n), new Array(n).fill(p)));
  console.log(JSON.stringify({z: z.toString(), z0: z0.toString(), r: r.map(String)}));
  console.log("js kzg blob cpu ok");
} else if (mode === "gpu") {
  const raw = fs.readFileSync(process.argv[3]);
  assert.strictEqual(raw.length, 6 * 131072);
  const B = [0, 1, 2, 3, 4, 5].map((i) => new Uint8Array(raw.subarray(131072 * i, 131072 * (i + 1))));
  const SIZES = [0, 1, 2, 0, 3];
  const out = {};
  for (const field of ["device", "host"]) {
    kzg.loadTrustedSetup(SETUP, 0, {field});
    const C = B.map((b) => kzg.blobToKzgCommitment(b));
    const P = B.map((b, i) => kzg.computeBlobKzgProof(b, C[i]));
    const groupsOf = (blobs, comms, proofs) => {
      let at = 0;
      return SIZES.map((n) => {
        const g = {blobs: blobs.slice(at, at + n), commitments: comms.slice(at, at + n), proofs: proofs.slice(at, at + n)};
        at += n;
        return g;
      });
    };
    const sub = (a, j, v) => a.map((x, i) => (i === j ? v : x));
    const elemR = Uint8Array.from(B[2]);
    elemR.set(Buffer.from("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001", "hex"), 32 * 4095);
    const flagless = Uint8Array.from(C[4]);
    flagless[0] &= 0x7f; // compression flag cleared
    const res = {
      commitments: C.map(hex),
      proofs: P.map(hex),
      valid: kzg.verifyBlobKzgProofBatchMany(groupsOf(B, C, P)).map(show),
      tampered: kzg.verifyBlobKzgProofBatchMany(groupsOf(B, C, sub(P, 5, P[1]))).map(show),
      swapped: kzg.verifyBlobKzgProofBatchMany(groupsOf(B, C, sub(sub(P, 1, P[2]), 2, P[1]))).map(show),
      elemR: kzg.verifyBlobKzgProofBatchMany(groupsOf(sub(B, 2, elemR), C, P)).map(show),
      flagless: kzg.verifyBlobKzgProofBatchMany(groupsOf(B, sub(C, 4, flagless), P)).map(show),
      single: [kzg.verifyBlobKzgProof(B[1], C[1], P[1]), kzg.verifyBlobKzgProof(B[1], C[1], P[2])],
      batch: [kzg.verifyBlobKzgProofBatch(B.slice(3), C.slice(3), P.slice(3)), kzg.verifyBlobKzgProofBatch([], [], []),
              kzg.verifyBlobKzgProofBatch(B.slice(3), C.slice(3), [P[3], P[5], P[4]])],
    };
    assert.throws(() => kzg.verifyBlobKzgProofBatch([elemR], [C[2]], [P[2]]), /BLST_BAD_SCALAR/);
    assert.throws(() => kzg.verifyBlobKzgProof(B[1], flagless, P[1]), Error);
    const zBytes = new Uint8Array(32);
    zBytes[5] = 0x12;
    zBytes[31] = 5;
    const [proof, yBytes] = kzg.computeKzgProof(B[2], zBytes);
    assert.strictEqual(proof.length, 48);
    assert.strictEqual(yBytes.length, 32);
    res.point = [hex(proof), hex(yBytes)];
    res.pointOk = [kzg.verifyKzgProof(C[2], zBytes, yBytes, proof), kzg.verifyKzgProof(C[2], zBytes, new Uint8Array(32), proof)];
    const rBytes = Buffer.from("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001", "hex");
    assert.throws(() => kzg.verifyKzgProof(C[2], new Uint8Array(rBytes), yBytes, proof), /BLST_BAD_SCALAR/);
    assert.throws(() => kzg.verifyKzgProof(C[2], zBytes, new Uint8Array(rBytes), proof), /BLST_BAD_SCALAR/);
    assert.throws(() => kzg.computeKzgProof(B[2], new Uint8Array(rBytes)), /BLST_BAD_SCALAR/);
    // malformed input throws before anything is sent
    assert.deepStrictEqual(kzg.verifyBlobKzgProofBatchMany([]), []);
    assert.throws(() => kzg.verifyBlobKzgProofBatch([B[1]], [C[1]], []));
    assert.throws(() => kzg.verifyBlobKzgProofBatch([B[1].subarray(1)], [C[1]], [P[1]]));
    assert.throws(() => kzg.verifyBlobKzgProofBatch([B[1]], [C[1].subarray(1)], [P[1]]));
    assert.throws(() => kzg.computeBlobKzgProof(B[1], C[1].subarray(1)));
    out[field] = res;
  }
  assert.deepStrictEqual(out.host, out.device);
  console.log(JSON.stringify(out.device));
  console.log("js kzg blob gpu ok");
} else {
  throw Error("usage: test_kzg_blob.js cpu | gpu <blobs file>");
}
