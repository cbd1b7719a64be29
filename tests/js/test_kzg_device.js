"use strict";
// The JS c-kzg surface (lodestar_amd/js/kzg.js) with the scalar-field work on the GPU:
// loadTrustedSetup(file, 0, {field: "device"}) against {field: "host"} (the BigInt path) on
// kzg.test.ts's two blobs -- same commitments, same aggregate proof, each path's proof verified by
// the other, tampering rejected, zero blobs.  The bytes are printed for tests/test_kzg_device.py to
// compare with lodestar_amd/kzg.py.
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
const hex = (u) => Buffer.from(u).toString("hex");
const blobs = [sequentialBlob(0), sequentialBlob(7)];

function run(field) {
  kzg.loadTrustedSetup(SETUP, 0, {field});
  const comms = blobs.map((b) => kzg.blobToKzgCommitment(b));
  const proof = kzg.computeAggregateKzgProof(blobs);
  return {comms, proof};
}

const host = run("host");
// still on the host field: default options leave it there
kzg.loadTrustedSetup(SETUP);
assert.strictEqual(hex(kzg.blobToKzgCommitment(blobs[0])), hex(host.comms[0]));
const dev = run("device");
// the device path checks the host path's proof, then tampering
assert.strictEqual(kzg.verifyAggregateKzgProof(blobs, host.comms, host.proof), true);
const bad = Uint8Array.from(blobs[1]);
bad[31] ^= 1;
assert.strictEqual(kzg.verifyAggregateKzgProof([blobs[0], bad], dev.comms, dev.proof), false);
assert.strictEqual(kzg.verifyAggregateKzgProof(blobs, dev.comms.slice().reverse(), dev.proof), false);
const inf = kzg.computeAggregateKzgProof([]);
assert.strictEqual(hex(inf), "c0" + "00".repeat(47));
assert.strictEqual(kzg.verifyAggregateKzgProof([], [], inf), true);
assert.strictEqual(kzg.verifyAggregateKzgProof([], [], dev.proof), false);
assert.throws(() => kzg.verifyAggregateKzgProof(blobs, dev.comms.slice(0, 1), dev.proof));
// a field element >= r (all 0xff) is refused
const over = Uint8Array.from(blobs[0]);
over.fill(0xff, 0, 32);
assert.throws(() => kzg.blobToKzgCommitment(over), /BLST_BAD_SCALAR/);
assert.throws(() => kzg.loadTrustedSetup(SETUP, 0, {field: "gpu"}));
// ... and the host path checks the device path's proof
kzg.loadTrustedSetup(SETUP, 0, {field: "host"});
assert.strictEqual(kzg.verifyAggregateKzgProof(blobs, dev.comms, dev.proof), true);

const out = (r) => ({commitments: r.comms.map(hex), proof: hex(r.proof)});
console.log(JSON.stringify({host: out(host), device: out(dev)}));
console.log("js kzg device ok");
