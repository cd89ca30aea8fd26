// Parallel.msmIndexed / msmIndexedNarrow against Parallel.msm over the dense equivalent (t[i] = sum of scalars[j] over
// indices[j] == i, mod q), on generated points.  Run on a GPU box: node js/test-indexed.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same } = require("./test-support.js");

const mod = (v, q) => ((v % q) + q) % q;

// msm over the dense equivalent of (indices, values): values are BigInts of either sign
async function dense(curve, pp, n, indices, vals, q) {
  const t = new Array(n).fill(BigInt(0));
  indices.forEach((i, j) => { t[i] = mod(t[i] + vals[j], q); });
  const raw = Buffer.concat(t.map((v) => M.bigintToLeBytes(v, 32)));
  const sp = curve.Parallel.getScalarPointer(raw.length);
  await curve.Parallel.scalarsFromBytes(sp, raw, n);
  const { result } = await curve.Parallel.msm(sp, pp, n);
  sp.free();
  return result;
}

// not the throwsWith of test-support.js: fn is async here and is awaited
async function throwsWith(fn, re, what) {
  let thrown = null;
  try { await fn(); } catch (e) { thrown = e; }
  assert(thrown && re.test(thrown.message), `${what}: expected ${re}, got ${thrown && thrown.message}`);
}

async function runCurve(curve, label) {
  const n = 700, m = 1000, q = curve.params.order, P = curve.Parallel;
  const pp = await P.randomPointsFast(n, { seed: 6 });
  const next = stream(41);
  const idx = Uint32Array.from({ length: m }, () => Number(next() % BigInt(n)));   // m > n: repeats
  idx[0] = 0; idx[1] = n - 1; idx[2] = n - 1;
  const vals = Array.from({ length: m }, () => ((next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next()) % q);
  vals[3] = q - vals[2];                                                            // cancels on the point n - 1
  const raw = Buffer.concat(vals.map((v) => M.bigintToLeBytes(v, 32)));
  const exp = await dense(curve, pp, n, Array.from(idx), vals, q);
  let cases = 0;
  const got = await P.msmIndexed(raw, idx, pp);
  assert(same(got.result, exp), `${label} msmIndexed`);
  assert(got.log.length > 0, "log");
  assert(same((await P.msmIndexed(raw, Array.from(idx), pp, { c: 9 })).result, exp), `${label} msmIndexed, plain array, c = 9`);
  assert(same((await P.msmIndexed(raw, idx, pp, { noGlv: true })).result, exp), `${label} msmIndexed noGlv`);
  const none = await P.msmIndexed(Buffer.alloc(0), new Uint32Array(0), pp);
  assert(same(none.result, await dense(curve, pp, n, [], [], q)), `${label} m = 0`);
  cases += 4;
  // narrow: signed 16-bit values with repeats, unsigned 64-bit with declared bits
  const i16 = Int16Array.from({ length: m }, () => Number(next() % BigInt(65536)) - 32768);
  i16[0] = -32768; i16[1] = 32767;
  assert(same((await P.msmIndexedNarrow(i16, idx, pp)).result, await dense(curve, pp, n, Array.from(idx), Array.from(i16, BigInt), q)), `${label} Int16Array`);
  const u40 = BigUint64Array.from({ length: m }, () => next() >> BigInt(24));
  assert(same((await P.msmIndexedNarrow(u40, idx, pp, { bits: 40, c: 11 })).result, await dense(curve, pp, n, Array.from(idx), Array.from(u40), q)), `${label} BigUint64Array bits 40`);
  cases += 2;
  // refusals: a bad index (the smallest bad position is named), a value outside the declared range, lengths that differ;
  // the context goes on working
  const bad = Uint32Array.from(idx);
  bad[600] = n; bad[123] = n + 5;
  await throwsWith(() => P.msmIndexed(raw, bad, pp), new RegExp(`msm error 1.*indices\\[123\\] = ${n + 5}`), `${label} bad index`);
  await throwsWith(() => P.msmIndexedNarrow(i16, bad, pp), new RegExp(`msm error 1.*indices\\[123\\] = ${n + 5}`), `${label} bad index, narrow`);
  await throwsWith(() => P.msmIndexedNarrow(u40, idx, pp, { bits: 39 }), /msm error 6/, `${label} out-of-range value`);
  await throwsWith(() => P.msmIndexed(raw, idx.subarray(1), pp), /need/, `${label} lengths`);
  await throwsWith(() => P.msmIndexed(raw.slice(0, 64), [0, -1], pp), /not an integer in/, `${label} negative index`);
  await throwsWith(() => P.msmIndexed(raw.slice(0, 64), [0, 1.5], pp), /not an integer in/, `${label} fractional index`);
  assert(same((await P.msmIndexed(raw, idx, pp)).result, exp), `${label} after the refusals`);
  cases += 7;
  pp.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 indexed ok:", await runCurve(bls, "bls12-377"), "cases");
  bls.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 indexed ok:", await runCurve(ed, "ed-on-bls12-377"), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
