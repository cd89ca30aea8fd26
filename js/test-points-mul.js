// Parallel.pointsMul / pointsMulBase against Parallel.msm and pointsLincomb: an MSM with scalars t over the produced points equals
// the MSM with s[i] * t[i] over the points they were made from; under equal scalars pointsMul writes what pointsLincomb writes;
// pointsMulBase over scalarsPowers is a commitment key.  Run on a GPU box: node js/test-points-mul.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same, throwsWith } = require("./test-support.js");

const bytesOf = (vals) => Buffer.concat(vals.map((v) => M.bigintToLeBytes(v, 32)));

async function scalarPtrOf(curve, vals) {
  const raw = bytesOf(vals);
  const sp = curve.Parallel.getScalarPointer(raw.length);
  await curve.Parallel.scalarsFromBytes(sp, raw, vals.length);
  return sp;
}

async function msmOver(curve, pp, vals) {
  const sp = await scalarPtrOf(curve, vals);
  const { result } = await curve.Parallel.msm(sp, pp, vals.length);
  sp.free();
  return result;
}

async function runCurve(curve, label) {
  const n = 321, q = curve.params.order, P = curve.Parallel;
  const next = stream(47);
  const big = () => ((next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next()) % q;
  const pp = await P.randomPointsFast(n + 3, { seed: 11 });
  const dst = P.getPointer(0), ref = P.getPointer(0);
  let cases = 0;
  const s = Array.from({ length: n }, big), t = Array.from({ length: n }, big);
  // host bytes, rows [3, 3 + n): the MSM over the result is the MSM over the source with the products
  P.pointsMul(dst, bytesOf(s), pp, { aLo: 3 });
  assert(dst.n === n && P.pointsetSize(dst) === n && pp.n === n + 3, `${label} sizes`);
  const zeros3 = new Array(3).fill(BigInt(0));
  const want = await msmOver(curve, pp, zeros3.concat(s.map((v, i) => (v * t[i]) % q)));
  assert(same(await msmOver(curve, dst, t), want), `${label} host scalars`);
  // the same scalars from a scalar pointer
  const sp = await scalarPtrOf(curve, s);
  P.pointsMul(dst, sp, pp, { aLo: 3 });
  assert(dst.n === n && same(await msmOver(curve, dst, t), want), `${label} device scalars`);
  // one scalar for all rows: what pointsLincomb writes
  const a = big();
  P.pointsMul(dst, bytesOf(new Array(65).fill(a)), pp, { count: 65 });
  P.pointsLincomb(ref, a, pp, null, null, { count: 65 });
  const t65 = t.slice(0, 65);
  assert(dst.n === 65 && same(await msmOver(curve, dst, t65), await msmOver(curve, ref, t65)), `${label} equals pointsLincomb`);
  // a window of a scalar pointer, in place on the rows [0, count)
  P.pointsMul(ref, sp, ref, { sLo: 7, count: 64 });
  assert(ref.n === 64, `${label} in place size`);
  assert(same(await msmOver(curve, ref, t.slice(0, 64)),
    await msmOver(curve, pp, s.slice(7, 71).map((v, i) => (((v * a) % q) * t[i]) % q))), `${label} in place`);
  cases += 4;
  // one base: the generator under the powers of tau is a commitment key; sum c_i [tau^i] G = [sum c_i tau^i] G
  const tau = big();
  const pw = P.scalarsPowers(tau, n);
  P.pointsMulBase(dst, pw);
  assert(dst.n === n, `${label} base size`);
  let acc = BigInt(0), p = BigInt(1);
  for (let i = 0; i < n; i++) { acc = (acc + t[i] * p) % q; p = (p * tau) % q; }
  P.pointsMulBase(ref, bytesOf([acc]));
  const one = [BigInt(1)];
  assert(same(await msmOver(curve, dst, t), await msmOver(curve, ref, one)), `${label} commitment key`);
  cases += 2;
  // refusals; the pointers go on working
  throwsWith(() => P.pointsMul(dst, bytesOf(s), pp, { aLo: 4 }), /msm error 4/, `${label} range beyond the set`);
  throwsWith(() => P.pointsMul(dst, sp, dst, { aLo: 1, count: 8 }), /msm error 1/, `${label} overlap`);
  throwsWith(() => P.pointsMul(dst, Buffer.alloc(33), pp), /multiple of 32/, `${label} ragged bytes`);
  throwsWith(() => P.pointsMul(dst, bytesOf(s), pp, { count: n + 1 }), /rows requested/, `${label} more rows than scalars`);
  throwsWith(() => P.pointsMul(dst, sp, pp, { sLo: 1, count: n }), /scalar pointer holds/, `${label} scalars beyond the pointer`);
  throwsWith(() => P.pointsMulBase(dst, sp, Buffer.alloc(5)), /bytes \(x \|\| y\)/, `${label} base size`);
  throwsWith(() => P.pointsMulBase(dst, sp, { x: BigInt(1), y: BigInt(1) }), /msm error 3/, `${label} base off the curve`);
  assert(dst.n === n && P.pointsetSize(dst) === n && same(await msmOver(curve, dst, t), await msmOver(curve, ref, one)), `${label} after the refusals`);
  cases += 8;
  sp.free(); pw.free(); pp.free(); dst.free(); ref.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 points mul ok:", await runCurve(bls, "bls12-377"), "cases");
  bls.close();
  const pallas = M.Weierstrass.create(M.pallasParams);
  console.log("pallas points mul ok:", await runCurve(pallas, "pallas"), "cases");
  pallas.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 points mul ok:", await runCurve(ed, "ed-on-bls12-377"), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
