"use strict";
// computeCellsAndKzgProofs(Many) of lodestar_amd/js/kzg.js (lb_kzg_compute_cells_and_proofs: FK20).
//   node test_kzg_fk20.js cpu           the names and argument validation (no GPU call)
//   node test_kzg_fk20.js gpu <file>    <file>: JSON written by tests/test_kzg_fk20.py write_js_fixture
//                                       (the degree-70 blob, its cells and proofs from the Python
//                                       surface, all hex): the JS surface must give the same bytes
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const kzg = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));
const SETUP = path.join(__dirname, "..", "..", "lodestar_amd", "trusted_setup.bin");
const mode = process.argv[2];
const hex = (b) => Buffer.from(b).toString("hex");
const unhex = (h) => new Uint8Array(Buffer.from(h, "hex"));

if (mode === "cpu") {
  for (const name of ["computeCellsAndKzgProofs", "computeCellsAndKzgProofsMany"]) {
    assert.strictEqual(typeof kzg[name], "function", name);
  }
  // nothing runs before a setup is loaded
  assert.throws(() => kzg.computeCellsAndKzgProofs(new Uint8Array(131072)), /not loaded/);
  assert.throws(() => kzg.computeCellsAndKzgProofsMany([]), /not loaded/);
  console.log(JSON.stringify({}));
  console.log("js kzg fk20 cpu ok");
} else if (mode === "gpu") {
  const fx = JSON.parse(fs.readFileSync(process.argv[3], "utf8"));
  const blob = unhex(fx.blob);
  for (const field of ["device", "host"]) {
    kzg.loadTrustedSetup(SETUP, 0, {field});
    const res = kzg.computeCellsAndKzgProofs(blob);
    assert.ok(Array.isArray(res) && res.length === 2);
    const [cells, proofs] = res;
    assert.strictEqual(cells.length, 128);
    assert.strictEqual(proofs.length, 128);
    assert.ok(proofs.every((p) => p instanceof Uint8Array && p.length === 48));
    assert.deepStrictEqual(cells.map(hex), fx.cells);
    assert.deepStrictEqual(proofs.map(hex), fx.proofs);
    assert.deepStrictEqual(cells.map(hex), kzg.computeCells(blob).map(hex));
    // a blob element equal to r: thrown by the single call, returned by the Many form, the others unaffected
    const elemR = Uint8Array.from(blob);
    elemR.set(Buffer.from("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001", "hex"), 32 * 5);
    assert.throws(() => kzg.computeCellsAndKzgProofs(elemR), /BLST_BAD_SCALAR/);
    const many = kzg.computeCellsAndKzgProofsMany([blob, elemR, blob]);
    assert.strictEqual(many.length, 3);
    assert.ok(many[1] instanceof Error && /BLST_BAD_SCALAR/.test(many[1].message));
    for (const k of [0, 2]) {
      assert.deepStrictEqual(many[k][0].map(hex), fx.cells);
      assert.deepStrictEqual(many[k][1].map(hex), fx.proofs);
    }
    assert.deepStrictEqual(kzg.computeCellsAndKzgProofsMany([]), []);
    // a wrong blob length throws before anything is sent
    assert.throws(() => kzg.computeCellsAndKzgProofs(blob.subarray(1)), /blob length/);
    assert.throws(() => kzg.computeCellsAndKzgProofsMany([blob, new Uint8Array(0)]), /blob length/);
  }
  console.log(JSON.stringify({proofs: 128}));
  console.log("js kzg fk20 gpu ok");
} else {
  throw Error("usage: test_kzg_fk20.js cpu | gpu <fixture file>");
}
