"use strict";
// recoverCellsAndKzgProofs(Many) of lodestar_amd/js/kzg.js (lb_kzg_recover_cells_and_proofs).
//   node test_kzg_recover.js cpu           the names and argument validation (no GPU call)
//   node test_kzg_recover.js gpu <file>    <file>: JSON written by tests/test_kzg_recover.py write_js_fixture
//                                          (the degree-70 blob's cells by the Python transform and its
//                                          proofs by FK20 on the blob, all hex): recovery from cells
//                                          64 .. 127 must give those bytes
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const kzg = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));
const SETUP = path.join(__dirname, "..", "..", "lodestar_amd", "trusted_setup.bin");
const mode = process.argv[2];
const hex = (b) => Buffer.from(b).toString("hex");
const unhex = (h) => new Uint8Array(Buffer.from(h, "hex"));
const range = (lo, hi) => Array.from({length: hi - lo}, (_, i) => lo + i);
const cell = () => new Uint8Array(2048);

// malformed input throws before anything is sent, with or without a setup
function checkValidation() {
  const idx = range(0, 64);
  const cells = idx.map(cell);
  assert.throws(() => kzg.recoverCellsAndKzgProofs(idx, cells.slice(1)), /length mismatch/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs(range(0, 63), cells.slice(1)), /cell count/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs(range(0, 129), range(0, 129).map(cell)), /cell count/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs(idx, [new Uint8Array(2047), ...cells.slice(1)]), /cell length/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs([...range(0, 63), 128], cells), /cell index/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs([...range(0, 63), 63.5], cells), /cell index/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs([1, 0, ...range(2, 64)], cells), /ascending/);
  assert.throws(() => kzg.recoverCellsAndKzgProofs([...range(0, 63), 62], cells), /ascending/);
  assert.throws(() => kzg.recoverCellsAndKzgProofsMany([{cellIndices: idx, cells}, {cellIndices: idx}]), /arrays/);
}

if (mode === "cpu") {
  for (const name of ["recoverCellsAndKzgProofs", "recoverCellsAndKzgProofsMany"]) {
    assert.strictEqual(typeof kzg[name], "function", name);
  }
  checkValidation();
  // nothing runs before a setup is loaded
  assert.throws(() => kzg.recoverCellsAndKzgProofs(range(0, 64), range(0, 64).map(cell)), /not loaded/);
  assert.throws(() => kzg.recoverCellsAndKzgProofsMany([]), /not loaded/);
  console.log(JSON.stringify({}));
  console.log("js kzg recover cpu ok");
} else if (mode === "gpu") {
  const fx = JSON.parse(fs.readFileSync(process.argv[3], "utf8"));
  const all = fx.cells.map(unhex);
  const upper = range(64, 128);
  for (const field of ["device", "host"]) {
    kzg.loadTrustedSetup(SETUP, 0, {field});
    const res = kzg.recoverCellsAndKzgProofs(upper, upper.map((i) => all[i]));
    assert.ok(Array.isArray(res) && res.length === 2);
    const [cells, proofs] = res;
    assert.strictEqual(cells.length, 128);
    assert.strictEqual(proofs.length, 128);
    assert.ok(cells.every((c) => c instanceof Uint8Array && c.length === 2048));
    assert.ok(proofs.every((p) => p instanceof Uint8Array && p.length === 48));
    assert.deepStrictEqual(cells.map(hex), fx.cells);
    assert.deepStrictEqual(proofs.map(hex), fx.proofs);
    // 65 cells with one element changed lie on no polynomial of degree < 4096: thrown by the single
    // call, returned by the Many form, the others unaffected
    const idx65 = range(10, 75);
    const changed = idx65.map((i) => Uint8Array.from(all[i]));
    changed[7][32 * 9 + 31] ^= 1;
    assert.throws(() => kzg.recoverCellsAndKzgProofs(idx65, changed), /BLST_VERIFY_FAIL/);
    const many = kzg.recoverCellsAndKzgProofsMany([
      {cellIndices: range(0, 128), cells: all},
      {cellIndices: idx65, cells: changed},
      {cellIndices: idx65, cells: idx65.map((i) => all[i])},
    ]);
    assert.strictEqual(many.length, 3);
    assert.ok(many[1] instanceof Error && /BLST_VERIFY_FAIL/.test(many[1].message));
    for (const k of [0, 2]) {
      assert.deepStrictEqual(many[k][0].map(hex), fx.cells);
      assert.deepStrictEqual(many[k][1].map(hex), fx.proofs);
    }
    assert.deepStrictEqual(kzg.recoverCellsAndKzgProofsMany([]), []);
    checkValidation();
  }
  console.log(JSON.stringify({proofs: 128}));
  console.log("js kzg recover gpu ok");
} else {
  throw Error("usage: test_kzg_recover.js cpu | gpu <fixture file>");
}
