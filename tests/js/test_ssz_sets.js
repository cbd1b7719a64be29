"use strict";
// getBlockSignatureSetsFromSsz (lodestar_amd/js/signing_roots.js) against the JSON walk of the same
// module with a Node crypto merkleizer.  Driven by tests/test_js_ssz_sets.py:
//   node tests/js/test_ssz_sets.js cases.json
// cases.json: {k3, cases: [{name, fork, ssz (hex), block (JSON) | null, error | null}]}; the blocks of all
// cases go through ONE call.  Prints "js ssz sets ok".
const assert = require("assert");
const crypto = require("crypto");
const fs = require("fs");
const path = require("path");
const SR = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "signing_roots.js"));
const addon = require(path.join(__dirname, "..", "..", "lodestar_amd", "napi", "lodestar_bls.node"));

const hexb = (h) => Uint8Array.from(Buffer.from(h.replace(/^0x/, ""), "hex"));
const hex = (b) => Buffer.from(b).toString("hex");
const ZH = [new Uint8Array(32)];
for (let i = 0; i < 64; i++) ZH.push(crypto.createHash("sha256").update(ZH[i]).update(ZH[i]).digest());

function cpuMerkleize(trees) {
  return trees.map((t) => {
    let layer = t.parts.map((p) => (p instanceof SR.Tree ? p.root : p));
    for (let d = 0; d < t.depth; d++) {
      if (layer.length % 2) layer.push(ZH[d]);
      const next = [];
      for (let i = 0; i < layer.length; i += 2) next.push(crypto.createHash("sha256").update(layer[i]).update(layer[i + 1]).digest());
      layer = next;
    }
    let r = layer.length ? layer[0] : ZH[t.depth];
    if (t.mix !== null && t.mix !== undefined) {
      const len = Buffer.alloc(32);
      len.writeBigUInt64LE(BigInt(t.mix));
      r = crypto.createHash("sha256").update(r).update(len).digest();
    }
    return Uint8Array.from(r);
  });
}

const input = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const k3 = input.k3;
const state = (fork) => ({
  genesisValidatorsRoot: hexb(k3.genesis_validators_root),
  forkPreviousVersion: hexb(k3.fork.previous_version), forkCurrentVersion: hexb(k3.fork.current_version),
  forkEpoch: k3.fork.epoch,
  pubkey: (i) => i, beaconCommittee: () => Array.from({length: 2048}, (_, j) => j),
  syncCommittee: () => Array.from({length: 512}, (_, j) => j), keyFromBytes: (b) => hex(b), forkSeq: () => fork,
});
const norm = (sets) => sets.map((s) => ({name: s.name, type: s.type, root: hex(s.signingRoot), sig: hex(s.signature),
  keys: s.type === "single" ? [s.pubkey] : s.pubkeys}));

const eng = addon.createEngine(0);
const states = input.cases.map((c) => state(c.fork));
const got = SR.getBlockSignatureSetsFromSsz(input.cases.map((c) => hexb(c.ssz)), states, {engine: eng});
assert.strictEqual(got.length, input.cases.length);
input.cases.forEach((c, k) => {
  if (c.error) {
    assert.ok(got[k] instanceof Error, c.name);
    assert.ok(got[k].message.includes(c.error), c.name + ": " + got[k].message);
    return;
  }
  const want = SR.resolve(SR.getBlockSignatureSets(state(c.fork), c.block), cpuMerkleize);
  assert.deepStrictEqual(norm(got[k]), norm(want), c.name);
});
// skip-proposer, one state for all blocks
const ops = input.cases.find((c) => c.name === "every_operation");
const skipped = SR.getBlockSignatureSetsFromSsz([hexb(ops.ssz)], state(3), {engine: eng, skipProposerSignature: true});
assert.deepStrictEqual(norm(skipped[0]),
  norm(SR.resolve(SR.getBlockSignatureSets(state(3), ops.block, {skipProposerSignature: true}), cpuMerkleize)));
assert.deepStrictEqual(SR.getBlockSignatureSetsFromSsz([], state(3), {engine: eng}), []);
assert.throws(() => addon.blockSetsFromSsz(eng, new Uint32Array([0, 4]), new Uint8Array(4), new Uint32Array([4]),
  new Uint8Array(384), new BigUint64Array(1), new BigUint64Array(1), 0));  // deneb: LB_ERR_ARGUMENT
addon.destroyEngine(eng);
console.log("js ssz sets ok");
