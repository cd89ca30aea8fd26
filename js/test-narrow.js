// Parallel.msmNarrow / msmBatchNarrow / scalarBits against Parallel.msm over the same values written as 32-byte scalars
// (negatives as q - |v|), on generated points.  Run on a GPU box: node js/test-narrow.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same } = require("./test-support.js");

// n values of `bits` magnitude bits, the extremes among them
function values(n, bits, signed, seed) {
  const next = stream(seed), span = BigInt(1) << BigInt(bits), out = [];
  for (let i = 0; i < n; i++) {
    let v = ((next() << BigInt(64)) | next()) % span;
    if (signed && (next() & BigInt(1))) v = -v - BigInt(1);
    out.push(v);
  }
  out[1] = span - BigInt(1);
  out[2] = signed ? -span : BigInt(0);
  return out;
}

function widen(vals, q) {
  return Buffer.concat(vals.map((v) => M.bigintToLeBytes(v < BigInt(0) ? q + v : v, 32)));
}

async function wide(curve, pp, vals, q) {
  const raw = widen(vals, q);
  const sp = curve.Parallel.getScalarPointer(raw.length);
  await curve.Parallel.scalarsFromBytes(sp, raw, vals.length);
  const { result } = await curve.Parallel.msm(sp, pp, vals.length);
  sp.free();
  return result;
}

async function runCurve(curve, label) {
  const n = 1000, q = curve.params.order;
  const pp = await curve.Parallel.randomPointsFast(n, { seed: 5 });
  const typed = [
    [Uint8Array, 8, false, Number], [Uint16Array, 16, false, Number], [Uint32Array, 32, false, Number], [BigUint64Array, 64, false, (v) => v],
    [Int8Array, 7, true, Number], [Int16Array, 15, true, Number], [Int32Array, 31, true, Number], [BigInt64Array, 63, true, (v) => v],
  ];
  let cases = 0;
  for (const [T, bits, signed, conv] of typed) {
    const vals = values(n, bits, signed, 100 + bits);
    const arr = T.from(vals.map(conv));
    const exp = await wide(curve, pp, vals, q);
    const got = await curve.Parallel.msmNarrow(arr, pp, n);
    assert(same(got.result, exp), `${label} ${T.name}`);
    assert(got.log.length > 0, "log");
    const c13 = await curve.Parallel.msmNarrow(arr, pp, n, { c: 13 });
    assert(same(c13.result, exp), `${label} ${T.name} c = 13`);
    cases += 2;
  }
  // declared bits below the width, raw bytes with a width, and the 32-byte form
  const v20 = values(n, 20, true, 7);
  const exp20 = await wide(curve, pp, v20, q);
  assert(same((await curve.Parallel.msmNarrow(Int32Array.from(v20.map(Number)), pp, n, { bits: 20 })).result, exp20), `${label} bits 20`);
  assert(same((await curve.Parallel.msmNarrow(widen(v20, q), pp, n, { width: 32, bits: 20, signed: true })).result, exp20), `${label} width 32`);
  const v128 = values(n, 128, false, 9);
  const raw16 = Buffer.concat(v128.map((v) => M.bigintToLeBytes(v, 16)));
  assert(same((await curve.Parallel.msmNarrow(raw16, pp, n, { width: 16 })).result, await wide(curve, pp, v128, q)), `${label} width 16`);
  cases += 3;
  // a value outside the declared range is refused, and the context still works
  let thrown = null;
  try { await curve.Parallel.msmNarrow(Int32Array.from(v20.map(Number)), pp, n, { bits: 19 }); } catch (e) { thrown = e; }
  assert(thrown && /msm error 6/.test(thrown.message), `${label} out-of-range value must throw msm error 6, got ${thrown && thrown.message}`);
  assert(same((await curve.Parallel.msmNarrow(Int32Array.from(v20.map(Number)), pp, n, { bits: 20 })).result, exp20), `${label} after a refusal`);
  // scalarBits
  const sb = curve.Parallel.scalarBits(widen(v20, q));
  assert(sb.signed === 20 && sb.unsigned === 255, `${label} scalarBits ${JSON.stringify(sb)}`);
  const ub = curve.Parallel.scalarBits(widen(values(n, 40, false, 3), q));
  assert(ub.unsigned === 40 && ub.signed === 40, `${label} scalarBits ${JSON.stringify(ub)}`);
  // batch
  const els = [11, 12, 13, 14, 15].map((s) => values(n, 32, false, s));
  const batch = await curve.Parallel.msmBatchNarrow(els.map((v) => Uint32Array.from(v.map(Number))), pp, n);
  assert(batch.length === els.length, "one result per element");
  for (let b = 0; b < els.length; b++) assert(same(batch[b].result, await wide(curve, pp, els[b], q)), `${label} batch element ${b}`);
  cases += els.length;
  pp.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 narrow ok:", await runCurve(bls, "bls12-377"), "cases");
  bls.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 narrow ok:", await runCurve(ed, "ed-on-bls12-377"), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
