// Parallel.scalarsLincomb / foldScalars / scalarsInner / scalarsPowers / scalarsMul against BigInt arithmetic mod the group order,
// and an msm over a folded vector against the msm over the products.  Run on a GPU box: node js/test-scalars.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same, eq, upload, read, throwsWith } = require("./test-support.js");

// kept here: the copies of powmod differ (this one takes the exponent as a plain number)
function powmod(x, e, q) {
  let r = BigInt(1), b = x % q;
  for (; e > 0; e >>= 1) { if (e & 1) r = (r * b) % q; b = (b * b) % q; }
  return r;
}

async function runCurve(curve, label) {
  const n = 321, q = curve.params.order, P = curve.Parallel;
  const next = stream(47);
  const raw256 = () => (next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next();
  const big = () => raw256() % q;
  const top = (BigInt(1) << BigInt(256)) - BigInt(1);
  // 2 n elements, some of them not canonical: they count as their residues
  const V = Array.from({ length: 2 * n }, (_, i) => (i % 7 === 3 ? [q, q + BigInt(1), top, BigInt(0)][(i >> 3) % 4] : big()));
  const W = Array.from({ length: n }, big);
  let cases = 0;
  // the in-place fold: the lower half is written, the pointer shrinks, the upper half keeps its bytes
  const v = await upload(curve, V);
  const a = big(), b = big();
  P.foldScalars(v, a, b);
  assert(v.n === n, `${label} fold size`);
  const folded = Array.from({ length: n }, (_, i) => (a * V[i] + b * V[n + i]) % q);
  assert(eq(read(curve, v, n), folded), `${label} fold`);
  v.n = 2 * n;
  assert(eq(read(curve, v, 2 * n).slice(n), V.slice(n)), `${label} fold leaves the upper half`);
  v.n = n;
  cases += 3;
  // inner products, with offsets; powers; the element-wise product
  const w = await upload(curve, W);
  const dot = (x, y) => x.reduce((acc, t, i) => (acc + t * y[i]) % q, BigInt(0));
  assert(P.scalarsInner(v, w, n) === dot(folded, W), `${label} inner`);
  assert(P.scalarsInner(v, w, 65, { aLo: 5, bLo: 7 }) === dot(folded.slice(5, 70), W.slice(7, 72)), `${label} inner with offsets`);
  assert(P.scalarsInner(v, w, 0) === BigInt(0), `${label} empty inner`);
  const z = big(), s = big();
  const pw = P.scalarsPowers(z, n, s);
  const expPw = Array.from({ length: n }, (_, i) => (s * powmod(z, i, q)) % q);
  assert(pw.n === n && eq(read(curve, pw, n), expPw), `${label} powers`);
  assert(P.scalarsInner(w, pw, n) === dot(W, expPw), `${label} a polynomial evaluation`);
  const prod = P.scalarsMul(P.getScalarPointer(0), v, w, n);
  assert(prod.n === n && eq(read(curve, prod, n), folded.map((t, i) => (t * W[i]) % q)), `${label} mul`);
  const lc = P.scalarsLincomb(P.getScalarPointer(0), a, w, null, null, { aLo: 1, count: 64 });
  assert(lc.n === 64 && eq(read(curve, lc, 64), W.slice(1, 65).map((t) => (a * t) % q)), `${label} one term`);
  cases += 7;
  // an msm over the folded vector equals the msm over the products computed here
  const pp = await P.randomPointsFast(n, { seed: 9 });
  const want = await upload(curve, folded);
  assert(same((await P.msm(v, pp, n)).result, (await P.msm(want, pp, n)).result), `${label} msm over the folded vector`);
  cases += 1;
  // refusals; the pointers go on working
  throwsWith(() => P.scalarsLincomb(lc, q, w), /msm error 6/, `${label} scalar = q`);
  throwsWith(() => P.scalarsLincomb(w, a, w, b, w, { aLo: 0, bLo: 0, dstLo: 1, count: 64 }), /msm error 1/, `${label} partial overlap`);
  throwsWith(() => P.scalarsInner(v, w, n + 1), /holds/, `${label} more than the pointer holds`);
  throwsWith(() => P.scalarsLincomb(lc, a, w, b, null), /come together/, `${label} y without its pointer`);
  throwsWith(() => P.foldScalars(w, a, b), /odd/, `${label} odd fold`);
  assert(eq(read(curve, w, n), W) && P.scalarsInner(v, w, n) === dot(folded, W), `${label} after the refusals`);
  cases += 6;
  for (const p of [v, w, pw, prod, lc, want]) p.free();
  pp.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 scalars ok:", await runCurve(bls, "bls12-377"), "cases");
  bls.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 scalars ok:", await runCurve(ed, "ed-on-bls12-377"), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
