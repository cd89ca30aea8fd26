// Parallel.pointsLincomb / foldPoints / pointsetSize against Parallel.msm: an MSM with scalars t over the produced points equals
// the MSM with a * t || b * t over the points they were made from.  Run on a GPU box: node js/test-points-lincomb.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same, throwsWith } = require("./test-support.js");

async function msmOver(curve, pp, vals) {
  const raw = Buffer.concat(vals.map((v) => M.bigintToLeBytes(v, 32)));
  const sp = curve.Parallel.getScalarPointer(raw.length);
  await curve.Parallel.scalarsFromBytes(sp, raw, vals.length);
  const { result } = await curve.Parallel.msm(sp, pp, vals.length);
  sp.free();
  return result;
}

async function runCurve(curve, label) {
  const n = 642, h = n / 2, q = curve.params.order, P = curve.Parallel;
  const next = stream(43);
  const big = () => ((next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next()) % q;
  const pp = await P.randomPointsFast(n, { seed: 8 });
  const kept = P.getPointer(0);
  let cases = 0;
  // a copy, then the in-place fold of the original
  P.pointsLincomb(kept, 1, pp);
  assert(kept.n === n && P.pointsetSize(kept) === n, `${label} copy size`);
  const t = Array.from({ length: h }, big), tn = Array.from({ length: n }, big);
  assert(same(await msmOver(curve, kept, tn), await msmOver(curve, pp, tn)), `${label} copy`);
  const a = big(), b = big();
  P.foldPoints(pp, a, b);
  assert(pp.n === h && P.pointsetSize(pp) === h, `${label} fold size`);
  const want = await msmOver(curve, kept, t.map((v) => (a * v) % q).concat(t.map((v) => (b * v) % q)));
  assert(same(await msmOver(curve, pp, t), want), `${label} fold`);
  cases += 3;
  // the same fold into a third pointer, scalars as bytes; one term; the shortcuts
  const dst = P.getPointer(0);
  P.pointsLincomb(dst, M.bigintToLeBytes(a, 32), kept, M.bigintToLeBytes(b, 32), kept, { aLo: 0, bLo: h, count: h });
  assert(dst.n === h && same(await msmOver(curve, dst, t), want), `${label} fold into another set`);
  P.pointsLincomb(dst, a, kept, null, null, { aLo: 5, count: 65 });
  const t65 = t.slice(0, 65);
  assert(dst.n === 65 && P.pointsetSize(dst) === 65, `${label} one term size`);
  assert(same(await msmOver(curve, dst, t65), await msmOver(curve, kept, new Array(5).fill(BigInt(0)).concat(t65.map((v) => (a * v) % q)))), `${label} one term`);
  P.pointsLincomb(dst, q - BigInt(1), kept, 1, kept, { count: 65 });       // -P + P
  const zero = await msmOver(curve, dst, t65);
  assert(same(zero, await msmOver(curve, kept, new Array(65).fill(BigInt(0)))), `${label} -P + P is the identity`);
  P.pointsLincomb(dst, 0, kept, 0, kept, { count: 65 });
  assert(same(await msmOver(curve, dst, t65), zero), `${label} 0, 0`);
  cases += 4;
  // refusals; the context and the sets go on working
  throwsWith(() => P.pointsLincomb(dst, q, kept), /msm error 6/, `${label} scalar = q`);
  throwsWith(() => P.pointsLincomb(kept, a, kept, b, kept, { aLo: 1, bLo: h, count: h }), /msm error 1/, `${label} overlap`);
  throwsWith(() => P.pointsLincomb(dst, a, kept, null, null, { aLo: n - 1, count: 2 }), /msm error 4/, `${label} range beyond the set`);
  throwsWith(() => P.pointsLincomb(dst, BigInt(1) << BigInt(256), kept), /2\^256/, `${label} scalar too wide`);
  throwsWith(() => P.pointsLincomb(dst, a, kept, b, null), /come together/, `${label} b without its pointer`);
  throwsWith(() => P.foldPoints(dst, a, b), /odd/, `${label} odd fold`);
  assert(kept.n === n && P.pointsetSize(kept) === n && dst.n === 65 && P.pointsetSize(dst) === 65, `${label} sizes after the refusals`);
  assert(same(await msmOver(curve, kept, tn), await msmOver(curve, kept, tn)) && same(await msmOver(curve, dst, t65), zero), `${label} after the refusals`);
  cases += 7;
  pp.free(); kept.free(); dst.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 points lincomb ok:", await runCurve(bls, "bls12-377"), "cases");
  bls.close();
  const pallas = M.Weierstrass.create(M.pallasParams);
  console.log("pallas points lincomb ok:", await runCurve(pallas, "pallas"), "cases");
  pallas.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 points lincomb ok:", await runCurve(ed, "ed-on-bls12-377"), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
