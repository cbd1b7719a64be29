"use strict";
// verifyAggregateKzgProofBatch of the JS c-kzg surface (lodestar_amd/js/kzg.js): a mixed batch of
// sidecars with 0, 1, 2, 0 and 1 blobs, then the same batch with defects, in both field modes.
// Every expected verdict is the JS single call's (verifyAggregateKzgProof) for that sidecar alone.
const path = require("path");
const assert = require("assert");
const kzg = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));
const SETUP = path.join(__dirname, "..", "..", "lodestar_amd", "trusted_setup.bin");

function sequentialBlob(off) {
  const b = new Uint8Array(4096 * 32);
  const dv = new DataView(b.buffer);
  for (let i = 0; i < 4096; i++) dv.setUint32(i * 32, (i + off) >>> 0);
  return b;
}
const B = [sequentialBlob(0), sequentialBlob(7), sequentialBlob(1000)];

kzg.loadTrustedSetup(SETUP, 0, {field: "device"});
const C = B.map((b) => kzg.blobToKzgCommitment(b));
const sidecar = (idx) => ({
  blobs: idx.map((i) => B[i]),
  commitments: idx.map((i) => C[i]),
  proof: kzg.computeAggregateKzgProof(idx.map((i) => B[i])),
});
const valid = [[], [0], [1, 2], [], [2]].map(sidecar);
const over = Uint8Array.from(B[0]);
over.fill(0xff, 32, 64); // a field element >= r
const flagless = Uint8Array.from(valid[1].proof);
flagless[0] &= 0x7f; // compression flag cleared
const defects = [
  {blobs: [], commitments: [], proof: valid[1].proof}, // no blobs, a proof that is not infinity
  valid[1],
  {blobs: valid[2].blobs, commitments: valid[2].commitments.slice().reverse(), proof: valid[2].proof},
  {blobs: [over], commitments: [C[0]], proof: valid[1].proof},
  {blobs: valid[4].blobs, commitments: valid[4].commitments, proof: flagless},
  valid[4],
];

function single(s) {
  try {
    return kzg.verifyAggregateKzgProof(s.blobs, s.commitments, s.proof);
  } catch (e) {
    return e;
  }
}
const show = (v) => (v instanceof Error ? "Error: " + v.message : v);

const seen = {};
for (const field of ["device", "host"]) {
  kzg.loadTrustedSetup(SETUP, 0, {field});
  for (const [name, batch] of [["valid", valid], ["defects", defects]]) {
    const got = kzg.verifyAggregateKzgProofBatch(batch).map(show);
    const exp = batch.map(single).map(show);
    if (field === "device") assert.deepStrictEqual(got, exp, name);
    else {
      // the host field words its own range error; everything else is the addon's and agrees
      got.forEach((g, k) => {
        if (!(name === "defects" && k === 3)) assert.deepStrictEqual(g, exp[k], name + " " + k);
        else assert.ok(String(exp[k]).startsWith("Error"), String(exp[k]));
      });
    }
    seen[field + " " + name] = got;
  }
  assert.deepStrictEqual(kzg.verifyAggregateKzgProofBatch([]), []);
  assert.throws(() => kzg.verifyAggregateKzgProofBatch([{blobs: [B[0]], commitments: [], proof: valid[1].proof}]));
  assert.throws(() => kzg.verifyAggregateKzgProofBatch([{blobs: [B[0].subarray(1)], commitments: [C[0]], proof: valid[1].proof}]));
  assert.throws(() => kzg.verifyAggregateKzgProofBatch([{blobs: [B[0]], commitments: [C[0]], proof: valid[1].proof.subarray(1)}]));
}
assert.deepStrictEqual(seen["device valid"], [true, true, true, true, true]);
assert.deepStrictEqual(seen["host valid"], seen["device valid"]);
assert.deepStrictEqual(seen["host defects"], seen["device defects"]);
assert.deepStrictEqual(seen["device defects"].map((v) => v === true), [false, true, false, false, false, true]);
assert.strictEqual(seen["device defects"][3], "Error: BLST_BAD_SCALAR");

console.log(JSON.stringify(seen["device defects"]));
console.log("js kzg batch ok");
