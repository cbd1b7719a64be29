"use strict";
// The cell names (EIP-7594) of lodestar_amd/js/kzg.js: computeCells, verifyCellKzgProofBatch(Many),
// BYTES_PER_CELL, CELLS_PER_EXT_BLOB.
//   node test_kzg_cells.js cpu           argument validation and the batch combiner (no GPU call);
//                                        prints r values for tests/test_js_kzg_cells.py to compare
//                                        with Python's
//   node test_kzg_cells.js gpu <file>    <file>: JSON written by tests/test_kzg_cells.py
//                                        write_js_fixture (a blob, its cells, one group of three
//                                        cells with commitments and proofs, all hex); checks the
//                                        cells and prints the verdicts for the Python surface to be
//                                        compared with
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const kzg = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));
const SETUP = path.join(__dirname, "..", "..", "lodestar_amd", "trusted_setup.bin");
const mode = process.argv[2];
const hex = (b) => Buffer.from(b).toString("hex");
const unhex = (h) => new Uint8Array(Buffer.from(h, "hex"));
const show = (v) => (v instanceof Error ? "Error: " + v.message : v);

if (mode === "cpu") {
  const {computeCellBatchR, R} = kzg._internal;
  for (const name of ["computeCells", "verifyCellKzgProofBatch", "verifyCellKzgProofBatchMany"]) {
    assert.strictEqual(typeof kzg[name], "function", name);
  }
  assert.strictEqual(kzg.BYTES_PER_CELL, 2048);
  assert.strictEqual(kzg.CELLS_PER_EXT_BLOB, 128);
  const cell = (v) => new Uint8Array(2048).fill(v);
  const a = new Uint8Array(48).fill(0x11);
  const b = new Uint8Array(48).fill(0x22);
  const p = new Uint8Array(48).fill(0x33);
  // nothing runs before a setup is loaded
  assert.throws(() => kzg.computeCells(new Uint8Array(131072)), /not loaded/);
  assert.throws(() => kzg.verifyCellKzgProofBatch([a], [0], [cell(1)], [p]), /not loaded/);
  assert.throws(() => kzg.verifyCellKzgProofBatchMany([]), /not loaded/);
  // n = 0, 1, 3 and a repeated commitment (b a b: first-appearance order)
  const r = [
    computeCellBatchR([], [], [], []),
    computeCellBatchR([a], [127], [cell(1)], [p]),
    computeCellBatchR([a, b, p], [0, 64, 127], [cell(1), cell(2), cell(3)], [p, p, a]),
    computeCellBatchR([b, a, b], [5, 5, 6], [cell(1), cell(2), cell(3)], [p, p, a]),
  ];
  assert.ok(r.every((v) => v < R));
  console.log(JSON.stringify({r: r.map(String)}));
  console.log("js kzg cells cpu ok");
} else if (mode === "gpu") {
  const fx = JSON.parse(fs.readFileSync(process.argv[3], "utf8"));
  const blob = unhex(fx.blob);
  const C = fx.commitments.map(unhex);
  const I = fx.cellIndices;
  const X = fx.groupCells.map(unhex);
  const P = fx.proofs.map(unhex);
  const out = {};
  for (const field of ["device", "host"]) {
    kzg.loadTrustedSetup(SETUP, 0, {field});
    const cells = kzg.computeCells(blob);
    assert.strictEqual(cells.length, 128);
    assert.deepStrictEqual(cells.map(hex), fx.cells);
    const sub = (a, j, v) => a.map((x, i) => (i === j ? v : x));
    const elemR = Uint8Array.from(X[0]);
    elemR.set(Buffer.from("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001", "hex"), 0);
    const flagless = Uint8Array.from(P[1]);
    flagless[0] &= 0x7f; // compression flag cleared
    const g = (c, i, x, p) => ({commitments: c, cellIndices: i, cells: x, proofs: p});
    const res = {
      many: kzg.verifyCellKzgProofBatchMany([g(C, I, X, P), g([], [], [], []), g(C, I, X, [P[1], P[0], P[2]]),
                                             g(C, I, sub(X, 0, elemR), P), g(C, I, X, sub(P, 1, flagless)),
                                             g(C.slice(1), I.slice(1), X.slice(1), P.slice(1))]).map(show),
      single: [kzg.verifyCellKzgProofBatch(C, I, X, P), kzg.verifyCellKzgProofBatch([], [], [], []),
               kzg.verifyCellKzgProofBatch(C, sub(I, 2, (I[2] + 1) % 128), X, P)],
    };
    assert.throws(() => kzg.verifyCellKzgProofBatch(C, I, sub(X, 0, elemR), P), /BLST_BAD_SCALAR/);
    // malformed input throws before anything is sent
    assert.deepStrictEqual(kzg.verifyCellKzgProofBatchMany([]), []);
    assert.throws(() => kzg.verifyCellKzgProofBatch(C, I, X, P.slice(1)), /length mismatch/);
    assert.throws(() => kzg.verifyCellKzgProofBatch(C, sub(I, 0, 128), X, P), /cell index/);
    assert.throws(() => kzg.verifyCellKzgProofBatch(C, I, sub(X, 0, X[0].subarray(1)), P), /cell length/);
    assert.throws(() => kzg.verifyCellKzgProofBatch(sub(C, 0, C[0].subarray(1)), I, X, P), /commitment length/);
    assert.throws(() => kzg.computeCells(blob.subarray(1)), /blob length/);
    out[field] = res;
  }
  assert.deepStrictEqual(out.host, out.device);
  console.log(JSON.stringify(out.device));
  console.log("js kzg cells gpu ok");
} else {
  throw Error("usage: test_kzg_cells.js cpu | gpu <fixture file>");
}
