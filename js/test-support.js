// What the js/test-*.js scripts share: the failing assert, a deterministic stream, the comparisons, and scalar vectors to and
// from the device through the facade.
"use strict";
const M = require("./montgomery-hip.js");

function assert(c, msg) { if (!c) { console.error("FAILED: " + msg); process.exit(1); } }

// deterministic 64-bit stream (xorshift64*), as BigInt
function stream(seed) {
  let s = BigInt(seed) | BigInt(1);
  const mask = (BigInt(1) << BigInt(64)) - BigInt(1);
  return () => {
    s ^= s >> BigInt(12); s = (s ^ (s << BigInt(25))) & mask; s ^= s >> BigInt(27);
    return (s * BigInt("2685821657736338717")) & mask;
  };
}

const ZERO = BigInt(0), ONE = BigInt(1);
const same = (a, b) => a.isZero === b.isZero && a.x === b.x && a.y === b.y;
const eq = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);

async function upload(curve, vals) {
  const raw = Buffer.concat(vals.map((v) => M.bigintToLeBytes(v, 32)));
  const sp = curve.Parallel.getScalarPointer(raw.length);
  await curve.Parallel.scalarsFromBytes(sp, raw, vals.length);
  return sp;
}

function read(curve, sp, n) {
  const raw = curve.Parallel.scalarsToBytes(sp, n);
  return Array.from({ length: n }, (_, i) => M.leBytesToBigint(raw.subarray(32 * i, 32 * i + 32)));
}

function throwsWith(fn, re, what) {
  let thrown = null;
  try { fn(); } catch (e) { thrown = e; }
  assert(thrown && re.test(thrown.message), `${what}: expected ${re}, got ${thrown && thrown.message}`);
}

module.exports = { assert, stream, ZERO, ONE, same, eq, upload, read, throwsWith };
