"use strict";
// BlsGpuVerifier({devices}): the pool spread over several device slots (lodestar_amd/js/index.js).
//   node tests/js/test_multidevice.js cpu                 -> the dispatch against a mock addon (modules.addon)
//   node tests/js/test_multidevice.js split <lists.json>  -> splitByCost of the given job lists, k = 1..8
//   node tests/js/test_multidevice.js gpu <case> [file]   -> one GPU case: golden | split | keys | all | close
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "index.js"));

const golden = (name) => JSON.parse(fs.readFileSync(path.join(__dirname, "..", "golden", name), "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));
const tick = (ms) => new Promise((r) => setTimeout(r, ms || 5));

async function outcome(p) {
  try {
    return await p;
  } catch (e) {
    return e.message;
  }
}

// ---------------------------------------------------------------- the mock addon
// Records every call; engines are {device, flags, id}; verifyJobs returns a promise the test settles
// by hand (pending[i].settle() resolves it with the per-job codes derived from the marker byte of
// each job's first signature: 1 -> valid, 0 -> invalid, 2 -> -10 BLST_INVALID_SIZE).
function mockAddon(deviceCount) {
  const a = {calls: [], pending: [], tables: new Map(), destroyed: []};
  let nextId = 0;
  a.deviceCount = () => deviceCount;
  a.errorName = (code) => m.addon.errorName(code);
  a.createEngine = function (device, flags) {
    a.calls.push(["createEngine", ...arguments]);
    const e = {device, flags, id: nextId++};
    a.tables.set(e, 0);
    return e;
  };
  a.destroyEngine = (e) => {
    a.calls.push(["destroyEngine", e.id]);
    a.destroyed.push(e.id);
  };
  a.registerPubkeys = (e, flat, size) => {
    a.calls.push(["registerPubkeys", e.id, flat.length / size]);
    const first = a.tables.get(e);
    a.tables.set(e, first + flat.length / size);
    return {first, status: new Int32Array(flat.length / size)};
  };
  a.g1Decompress = (e, flat48) => {
    a.calls.push(["g1Decompress", e.id, flat48.length / 48]);
    return {out: new Uint8Array(2 * flat48.length).fill(9), status: new Int32Array(flat48.length / 48)};
  };
  a.verifyJobs = (engine, jobOff, pkOff, pks, roots, sigs) =>
    new Promise((resolve, reject) => {
      const codes = new Int32Array(jobOff.length - 1);
      const tags = [];
      for (let j = 0; j + 1 < jobOff.length; j++) {
        const marker = sigs[96 * jobOff[j]];
        codes[j] = marker === 1 ? 1 : marker === 0 ? 0 : -10;
        tags.push(roots[32 * jobOff[j]] | (roots[32 * jobOff[j] + 1] << 8));  // the job's serial number (below)
      }
      a.pending.push({engine, jobOff, pkOff, nSets: jobOff[jobOff.length - 1], nKeys: pkOff[pkOff.length - 1], tags,
        indexed: pks instanceof Uint32Array, settle: () => resolve(codes), fail: (e) => reject(e)});
    });
  return a;
}

// jobs carry a serial number in their first signing root, so a package shows which jobs it holds
let serial = 0;
function mkSets(nSets, keysOfLast, marker) {
  const tag = serial++;
  const sets = [];
  for (let i = 0; i < nSets; i++) {
    const root = new Uint8Array(32);
    root[0] = tag & 255;
    root[1] = tag >> 8;
    const signature = new Uint8Array(96);
    signature[0] = marker === undefined ? 1 : marker;
    sets.push(i === nSets - 1 && keysOfLast > 0
      ? {type: "aggregate", pubkeys: Array.from({length: keysOfLast}, () => new Uint8Array(96)), signingRoot: root, signature}
      : {type: "single", pubkey: new Uint8Array(96), signingRoot: root, signature});
  }
  return {tag, sets};
}
const ONE = () => mkSets(1, 0);         // a gossip attestation
const AGG = () => mkSets(3, 256);       // an aggregate-and-proof: two single sets and a 256-key aggregate
const BIG = () => mkSets(128, 0);       // one chunk of a block-sync call

// The mixed queue of 64 jobs.  A job heavier than a cost quantile leaves the quantiles it spans
// without a job's midpoint (those ranges launch nothing), and the 128-set job (378 880) is heavier
// than any eighth of 64 such jobs (at most 149 000), so it can take a whole eighth for itself only
// where the eighths before and after it each still hold another job's midpoint.  findMixedOrder()
// looks for such an order: most jobs aggregates, the big job second in the queue (the first eighth
// holds the job before it, the second the big job's midpoint, the third begins inside its tail).
function mixedQueue() {
  const jobs = [];
  for (let i = 0; i < 64; i++) jobs.push(MIXED_ORDER[i] === "B" ? BIG() : MIXED_ORDER[i] === "1" ? ONE() : AGG());
  return jobs;
}
let MIXED_ORDER = null;  // set by findMixedOrder()

/** the first order (big job's position, 1-set jobs spread evenly) whose 8-way cut has no empty range */
function findMixedOrder() {
  for (let nOne = 3; nOne <= 12; nOne++)
    for (let pos = 0; pos < 64; pos++) {
      const order = [];
      for (let i = 0; i < 64; i++) order.push(i === pos ? "B" : "A");
      // 1-set jobs at evenly spaced places other than the big job's
      for (let q = 0; q < nOne; q++) {
        const at = Math.floor(((q + 0.5) * 64) / nOne);
        if (order[at] === "A") order[at] = "1";
      }
      const jobs = order.map((c) => (c === "B" ? BIG() : c === "1" ? ONE() : AGG()).sets);
      if (m.splitByCost(jobs, 8).every(([lo, hi]) => hi > lo)) return order.join("");
    }
  throw Error("no order of the mixed queue fills all eight ranges");
}

function submitAll(pool, jobs, opts) {
  return jobs.map((j) => outcome(pool.verifySignatureSets(j.sets, opts)));
}

/** checks that `pkgs` (mock pending entries) hold contiguous ranges of `jobs` covering all of it, in some order */
function assertCover(pkgs, jobs) {
  const ranges = pkgs.map((p) => {
    const lo = jobs.findIndex((j) => j.tag === p.tags[0]);
    assert.ok(lo >= 0);
    p.tags.forEach((t, i) => assert.strictEqual(t, jobs[lo + i].tag, "a package is a contiguous range of the queue"));
    return [lo, lo + p.tags.length];
  }).sort((x, y) => x[0] - y[0]);
  let at = 0;
  for (const [lo, hi] of ranges) {
    assert.strictEqual(lo, at, "ranges cover the queue without gap or overlap");
    at = hi;
  }
  assert.strictEqual(at, jobs.length);
  return ranges;
}

const pkgCost = (p, jobs) => p.tags.reduce((c, t) => c + m.jobCost(jobs.find((j) => j.tag === t).sets), 0);

async function cpuTests() {
  MIXED_ORDER = findMixedOrder();
  assert.ok(MIXED_ORDER.includes("1") && MIXED_ORDER.includes("A") && MIXED_ORDER.split("B").length === 2);
  const eight = [0, 1, 2, 3, 4, 5, 6, 7];

  // 1. engine creation, 8 devices: the latency engine first on devices[0], then one pool engine per slot
  {
    const a = mockAddon(8);
    const pool = new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: 16}, {addon: a});
    const created = a.calls.filter((c) => c[0] === "createEngine");
    assert.strictEqual(created.length, 9);
    assert.deepStrictEqual(created[0], ["createEngine", 0, 1]);
    assert.deepStrictEqual(created.slice(1).map((c) => c[1]), eight);
    assert.strictEqual(pool.engines.length, 8);
    assert.deepStrictEqual(pool.devices, eight);
    const handles = pool.registerPubkeys([new Uint8Array(96), new Uint8Array(96).fill(1), new Uint8Array(96).fill(2)]);
    const reg = a.calls.filter((c) => c[0] === "registerPubkeys");
    assert.deepStrictEqual(reg.map((c) => c[1]).sort((x, y) => x - y), [0, 1, 2, 3, 4, 5, 6, 7, 8]);
    assert.deepStrictEqual(handles.map((h) => h.index), [0, 1, 2]);
    const more = pool.registerPubkeys([new Uint8Array(48)]);  // decompressed once, on the latency engine
    assert.deepStrictEqual(a.calls.filter((c) => c[0] === "g1Decompress"), [["g1Decompress", 0, 1]]);
    assert.strictEqual(more[0].index, 3);
    // a table out of step with the others is refused
    a.tables.set(pool.engines[5], 99);
    assert.throws(() => pool.registerPubkeys([new Uint8Array(96)]), /out of step/);
    await pool.close();
    assert.deepStrictEqual(a.destroyed.slice().sort((x, y) => x - y), [0, 1, 2, 3, 4, 5, 6, 7, 8]);
    // a failing createEngine destroys what was created and throws
    const b = mockAddon(8);
    const create = b.createEngine;
    b.createEngine = function (device) {
      if (device === 5) throw Error("LB_ERR_DEVICE");
      return create.apply(b, arguments);
    };
    assert.throws(() => new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: 16}, {addon: b}), /LB_ERR_DEVICE/);
    assert.deepStrictEqual(b.destroyed.slice().sort((x, y) => x - y), [0, 1, 2, 3, 4, 5]);
  }

  // 2. balanced split: one runJobs round cuts the mixed queue into 8 packages on 8 distinct devices
  {
    const a = mockAddon(8);
    const pool = new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: 16}, {addon: a});
    const jobs = mixedQueue();
    const results = submitAll(pool, jobs);
    await tick();
    assert.strictEqual(a.pending.length, 8);
    assert.deepStrictEqual(a.pending.map((p) => p.engine.device).sort((x, y) => x - y), eight);
    assertCover(a.pending, jobs);
    const costs = a.pending.map((p) => pkgCost(p, jobs));
    const largest = Math.max(...jobs.map((j) => m.jobCost(j.sets)));
    assert.strictEqual(largest, 128 * (m.SET_COST + m.KEY_COST));
    assert.ok(Math.max(...costs) - Math.min(...costs) <= largest, `package costs ${costs}`);
    assert.deepStrictEqual(pool.stats.packagesPerSlot, [1, 1, 1, 1, 1, 1, 1, 1]);
    assert.strictEqual(pool.stats.splits, 1);
    a.pending.forEach((p) => p.settle());
    assert.deepStrictEqual(await Promise.all(results), Array(64).fill(true));
    await pool.close();
  }

  // 2b. a job heavier than a quantile: the ranges it leaves empty launch nothing, the queue is still covered
  {
    const a = mockAddon(8);
    const pool = new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: 16}, {addon: a});
    const jobs = [BIG()];
    for (let i = 0; i < 40; i++) jobs.push(ONE());
    const results = submitAll(pool, jobs);
    await tick();
    assert.ok(a.pending.length >= 2 && a.pending.length < 8, `${a.pending.length} packages`);
    assert.strictEqual(new Set(a.pending.map((p) => p.engine.device)).size, a.pending.length);
    assertCover(a.pending, jobs);
    a.pending.forEach((p) => p.settle());
    assert.deepStrictEqual(await Promise.all(results), Array(41).fill(true));
    await pool.close();
  }

  // 3. no split below the threshold: the same queue is one package
  {
    const a = mockAddon(8);
    const jobs = mixedQueue();
    const nSets = jobs.reduce((n, j) => n + j.sets.length, 0);
    const pool = new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: nSets + 1}, {addon: a});
    const results = submitAll(pool, jobs);
    await tick();
    assert.strictEqual(a.pending.length, 1);
    assert.strictEqual(a.pending[0].nSets, nSets);
    assert.strictEqual(a.pending[0].engine.device, 0);  // no cost in flight anywhere: the lowest slot
    assert.strictEqual(pool.stats.splits, 0);
    // exactly at the threshold for two packages
    const pool2 = new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: Math.floor(nSets / 2)}, {addon: a});
    const results2 = submitAll(pool2, jobs);
    await tick();
    assert.strictEqual(a.pending.length, 3);
    a.pending.forEach((p) => p.settle());
    await Promise.all(results.concat(results2));
    await pool.close();
    await pool2.close();
  }

  // 4. busy slot: nothing more goes to a slot without an idle engine; slots with no cost in flight come first
  {
    const a = mockAddon(8);
    const pool = new m.BlsGpuVerifier({devices: eight, engines: 1, minPackageSets: 16}, {addon: a});
    const first = mixedQueue();
    const r1 = submitAll(pool, first);
    await tick();
    assert.strictEqual(a.pending.length, 8);
    const held = a.pending.find((p) => p.engine.device === 3);
    a.pending.filter((p) => p !== held).forEach((p) => p.settle());
    a.pending = [];
    await tick();
    const second = mixedQueue();
    const r2 = submitAll(pool, second);
    await tick();
    assert.strictEqual(a.pending.length, 7);
    assert.deepStrictEqual(a.pending.map((p) => p.engine.device).sort((x, y) => x - y), [0, 1, 2, 4, 5, 6, 7]);
    assertCover(a.pending, second);
    held.settle();
    a.pending.forEach((p) => p.settle());
    await Promise.all(r1.concat(r2));
    await pool.close();
    // two engines per slot: device 3 has an idle engine left, but its package in flight ranks it last
    const b = mockAddon(4);
    const pool2 = new m.BlsGpuVerifier({devices: [0, 1, 2, 3], engines: 2, minPackageSets: 16}, {addon: b});
    const q1 = [ONE(), ONE()];
    const s1 = submitAll(pool2, q1);  // 2 sets: one package, on slot 0
    await tick();
    assert.deepStrictEqual(b.pending.map((p) => p.engine.device), [0]);
    const q2 = Array.from({length: 48}, ONE);  // 48 sets: k = 3 -> the slots with nothing in flight: 1, 2, 3
    const s2 = submitAll(pool2, q2);
    await tick();
    assert.deepStrictEqual(b.pending.slice(1).map((p) => p.engine.device).sort(), [1, 2, 3]);
    const q3 = Array.from({length: 16}, ONE);  // k = 1, every slot has a package in flight: the least loaded, slot 0 (2 sets)
    const s3 = submitAll(pool2, q3);
    await tick();
    assert.strictEqual(b.pending.length, 5);
    assert.strictEqual(b.pending[4].engine.device, 0);
    assert.notStrictEqual(b.pending[4].engine.id, b.pending[0].engine.id);  // the slot's other engine
    assert.deepStrictEqual(pool2.stats.packagesPerSlot, [2, 1, 1, 1]);
    b.pending.forEach((p) => p.settle());
    await Promise.all(s1.concat(s2, s3));
    await pool2.close();
  }

  // 5. isolation: per-job codes within a package; a device failure rejects only its own package's jobs
  {
    const a = mockAddon(3);
    const logged = [];
    const pool = new m.BlsGpuVerifier({devices: [0, 1, 2], engines: 1, minPackageSets: 1},
      {addon: a, logger: {error: (msg) => logged.push(msg)}});
    const jobs = [mkSets(1, 0, 1), mkSets(1, 0, 0), mkSets(1, 0, 2), ONE(), ONE(), ONE(), ONE(), ONE(), ONE()];
    const results = submitAll(pool, jobs);
    await tick();
    assert.strictEqual(a.pending.length, 3);
    assertCover(a.pending, jobs);
    const [p0, p1, p2] = a.pending.slice().sort((x, y) => x.tags[0] - y.tags[0]);
    assert.strictEqual(p0.tags.length, 3);
    p0.settle();
    assert.deepStrictEqual(await Promise.all(results.slice(0, 3)), [true, false, "BLST_INVALID_SIZE"]);
    p1.fail(Error("LB_ERR_DEVICE"));
    assert.deepStrictEqual(await Promise.all(results.slice(3, 6)), Array(3).fill("LB_ERR_DEVICE"));
    assert.strictEqual(logged.length, 1);
    // nothing is requeued, and the third package is untouched
    await tick();
    assert.strictEqual(a.pending.length, 3);
    p2.settle();
    assert.deepStrictEqual(await Promise.all(results.slice(6)), [true, true, true]);
    assert.strictEqual(pool.stats.jobsInvalid, 1);
    assert.strictEqual(pool.stats.jobsError, 1);
    await pool.close();
  }

  // 6. close(): queued jobs abort, the package in flight is awaited, every engine is destroyed once
  {
    const a = mockAddon(2);
    const pool = new m.BlsGpuVerifier({devices: [0, 1], engines: 1, minPackageSets: 1000}, {addon: a});
    const flying = submitAll(pool, [ONE(), ONE()]);
    await tick();
    assert.strictEqual(a.pending.length, 1);
    const queued = submitAll(pool, [ONE()]);                       // in the queue, not yet dispatched
    const buffered = submitAll(pool, [ONE()], {batchable: true});  // in the buffer
    let closed = false;
    const closing = pool.close().then(() => { closed = true; });
    assert.deepStrictEqual(await Promise.all(queued.concat(buffered)), Array(2).fill("QUEUE_ERROR_QUEUE_ABORTED"));
    await tick(20);
    assert.strictEqual(closed, false, "close() waits for the package in flight");
    assert.strictEqual(a.destroyed.length, 0);
    a.pending[0].settle();
    await closing;
    assert.deepStrictEqual(await Promise.all(flying), [true, true]);
    assert.deepStrictEqual(a.destroyed.slice().sort((x, y) => x - y), [0, 1, 2]);
    await pool.close();
    assert.strictEqual(a.destroyed.length, 3);
    assert.strictEqual(a.pending.length, 1);  // nothing launched after close
    assert.strictEqual(await outcome(pool.verifySignatureSets(ONE().sets)), "QUEUE_ERROR_QUEUE_ABORTED");
  }

  // 7. no `devices`: today's engines and today's dispatch
  for (const [opts, d] of [[{}, 0], [{device: 5}, 5]]) {
    const a = mockAddon(8);
    const pool = new m.BlsGpuVerifier(opts, {addon: a});
    assert.deepStrictEqual(a.calls, [["createEngine", d, 1], ["createEngine", d], ["createEngine", d]]);
    const jobs = mixedQueue();
    const results = submitAll(pool, jobs);
    await tick();
    assert.strictEqual(a.pending.length, 1);
    assert.strictEqual(a.pending[0].tags.length, 64);
    assert.deepStrictEqual(pool.stats.packagesPerSlot, [1]);
    assert.strictEqual(pool.stats.splits, 0);
    a.pending[0].settle();
    await Promise.all(results);
    await pool.close();
  }
  // metrics: jobsWorkerTime's workerId is the engine's position in the flattened engine list
  {
    const a = mockAddon(2);
    const ids = [];
    const sink = {observe() {}, inc() {}, set() {}};
    const metrics = {bls: {aggregatedPubkeys: sink}, blsThreadPool: new Proxy({}, {get: (t, name) =>
      name === "jobsWorkerTime" ? {inc: (labels) => ids.push(labels.workerId)} : sink})};
    const pool = new m.BlsGpuVerifier({devices: [0, 1], engines: 2, minPackageSets: 1}, {addon: a, metrics});
    const results = submitAll(pool, [ONE(), ONE()]);
    await tick();
    const engineAt = a.pending.map((p) => pool.engines.indexOf(p.engine));
    a.pending.forEach((p) => p.settle());
    await Promise.all(results);
    assert.deepStrictEqual(ids.slice().sort(), engineAt.slice().sort());
    assert.ok(engineAt.some((i) => i >= 2));  // an engine of the second slot
    await pool.close();
  }

  // 8. devices: "all"
  assert.throws(() => new m.BlsGpuVerifier({devices: "all", minPackageSets: 16}, {addon: mockAddon(0)}), /^Error: LB_ERR_NO_DEVICE$/);
  {
    const a = mockAddon(3);
    const pool = new m.BlsGpuVerifier({devices: "all", engines: 1, minPackageSets: 16}, {addon: a});
    assert.deepStrictEqual(pool.devices, [0, 1, 2]);
    await pool.close();
  }
  assert.throws(() => new m.BlsGpuVerifier({devices: [], minPackageSets: 16}, {addon: mockAddon(1)}), /devices must be/);
  // the real addon: a count, never an error (0 on a machine without a GPU, where "all" then throws)
  const realCount = m.addon.deviceCount();
  assert.ok(Number.isInteger(realCount) && realCount >= 0);
  if (realCount === 0) assert.throws(() => new m.BlsGpuVerifier({devices: "all"}), /^Error: LB_ERR_NO_DEVICE$/);
  assert.ok(Number.isInteger(Math.log2(m.DEFAULT_MIN_PACKAGE_SETS)) && m.DEFAULT_MIN_PACKAGE_SETS >= 256);
  console.log("js multidevice cpu ok");
}

/** lists: per job the key count of each of its sets -> splitByCost ranges for k = 1..8 */
function splitMode(file) {
  const lists = JSON.parse(fs.readFileSync(file, "utf8"));
  const out = lists.map((list) => {
    const jobs = list.map((keyCounts) => keyCounts.map((n) => ({type: "aggregate", pubkeys: Array(n).fill(null)})));
    const perK = [];
    for (let k = 1; k <= 8; k++) perK.push(m.splitByCost(jobs, k));
    return perK;
  });
  console.log(JSON.stringify(out));
  console.log("js multidevice split ok");
}

// ---------------------------------------------------------------- GPU
function setsFromCase(c) {
  return c.sets.map((s) =>
    s.pubkeys.length === 1 && c.name.indexOf("aggregate") < 0
      ? {type: "single", pubkey: hex(s.pubkeys[0]), signingRoot: hex(s.signing_root), signature: hex(s.signature)}
      : {type: "aggregate", pubkeys: s.pubkeys.map(hex), signingRoot: hex(s.signing_root), signature: hex(s.signature)}
  );
}

/** the signed material tests/test_js_multidevice.py wrote: 8 keys, 16 roots, sigs[key][root] */
function loadSigned(file) {
  const w = JSON.parse(fs.readFileSync(file, "utf8"));
  return {keys: w.keys.map(hex), roots: w.roots.map(hex), sigs: w.sigs.map((row) => row.map(hex))};
}

/** 512 one-set jobs over the 8 keys and 16 roots; job 100 signs another root, job 300 carries 32 bytes */
function splitJobs(w, pubkeys) {
  const jobs = [];
  for (let j = 0; j < 512; j++) {
    const k = j % 8, r = (j >> 3) % 16;
    let signature = w.sigs[k][r];
    if (j === 100) signature = w.sigs[k][(r + 1) % 16];
    if (j === 300) signature = new Uint8Array(32);
    jobs.push([{type: "single", pubkey: pubkeys[k], signingRoot: w.roots[r], signature}]);
  }
  return jobs;
}

async function gpuTests(which, file) {
  const two = {devices: [0, 0], engines: 1, minPackageSets: 64};
  if (which === "golden") {
    // every golden case on two slots, all submitted at once, batchable and not
    const pool = new m.BlsGpuVerifier(two);
    const cases = golden("jobs.json").cases;
    for (const batchable of [false, true]) {
      const got = await Promise.all(cases.map((c) => outcome(pool.verifySignatureSets(setsFromCase(c), {batchable}))));
      cases.forEach((c, k) => assert.strictEqual(got[k], c.expected, `${c.name} batchable=${batchable}`));
    }
    await pool.close();
  } else if (which === "split") {
    const w = loadSigned(file);
    const run = async (opts) => {
      const pool = new m.BlsGpuVerifier(opts);
      const got = await Promise.all(splitJobs(w, w.keys).map((sets) => outcome(pool.verifySignatureSets(sets))));
      const stats = pool.stats;
      await pool.close();
      return {got, stats};
    };
    const split = await run(two);
    assert.ok(split.stats.packagesPerSlot.every((n) => n >= 1), `packagesPerSlot ${split.stats.packagesPerSlot}`);
    assert.ok(split.stats.splits >= 1);
    assert.strictEqual(split.got.filter((v) => v === true).length, 510);
    assert.strictEqual(split.got[100], false);
    assert.strictEqual(split.got[300], "BLST_INVALID_SIZE");
    const plain = await run({engines: 1});
    assert.deepStrictEqual(plain.stats.packagesPerSlot.length, 1);
    assert.deepStrictEqual(split.got, plain.got);
  } else if (which === "keys") {
    // registered handles verify on both slots: indexed packages go to each
    const w = loadSigned(file);
    const pool = new m.BlsGpuVerifier(two);
    const seen = [];
    const real = pool.addon;
    pool.addon = Object.create(real);  // the native addon, with verifyJobs observed
    Object.defineProperty(pool.addon, "verifyJobs", {value: (engine, jobOff, pkOff, pks, ...rest) => {
      seen.push({slot: pool.engines.indexOf(engine), indexed: pks instanceof Uint32Array});
      return real.verifyJobs(engine, jobOff, pkOff, pks, ...rest);
    }});
    const handles = pool.registerPubkeys(w.keys);
    assert.deepStrictEqual(handles.map((h) => h.index), [0, 1, 2, 3, 4, 5, 6, 7]);
    const got = await Promise.all(splitJobs(w, handles).map((sets) => outcome(pool.verifySignatureSets(sets))));
    assert.strictEqual(got.filter((v) => v === true).length, 510);
    assert.strictEqual(got[100], false);
    assert.strictEqual(got[300], "BLST_INVALID_SIZE");
    for (const slot of [0, 1]) assert.ok(seen.some((s) => s.slot === slot && s.indexed), `indexed package on slot ${slot}`);
    assert.ok(seen.every((s) => s.indexed));
    // the latency engine holds the table too
    assert.strictEqual(await pool.verifySignatureSets(splitJobs(w, handles)[0], {verifyOnMainThread: true}), true);
    await pool.close();
  } else if (which === "all") {
    assert.ok(m.addon.deviceCount() >= 1);
    const pool = new m.BlsGpuVerifier({devices: "all", engines: 1, minPackageSets: 64});
    assert.strictEqual(pool.devices.length, m.addon.deviceCount());
    const c = golden("jobs.json").cases.find((x) => x.name === "mixed_valid_with_aggregate");
    assert.strictEqual(await outcome(pool.verifySignatureSets(setsFromCase(c))), c.expected);
    await pool.close();
  } else if (which === "close") {
    // close() leaves no engine behind: [0, 0] with 2 engines per slot is 5 engines, and the engines
    // of three such verifiers together (15) would pass the per-device cap (10): a leaked engine
    // makes a later constructor throw LB_ERR_DEVICE
    const c = golden("jobs.json").cases.find((x) => x.name === "two_valid");
    for (let round = 0; round < 3; round++) {
      const pool = new m.BlsGpuVerifier({devices: [0, 0], engines: 2, minPackageSets: 64});
      assert.strictEqual(pool.engines.length, 4);
      assert.strictEqual(await outcome(pool.verifySignatureSets(setsFromCase(c))), c.expected);
      await pool.close();
      assert.strictEqual(pool.engines.length, 0);
    }
  } else {
    throw Error(`unknown gpu case ${which}`);
  }
  console.log(`js multidevice gpu ${which} ok`);
}

const mode = process.argv[2];
(mode === "gpu" ? gpuTests(process.argv[3], process.argv[4])
  : mode === "split" ? Promise.resolve(splitMode(process.argv[3])) : cpuTests()).catch((e) => {
  console.error(e);
  process.exit(1);
});
