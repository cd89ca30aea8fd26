// Parallel.scalarsScan / scalarsInverse / scalarsDivLinear against BigInt arithmetic at 257 and 65 537 elements: sums and products,
// inclusive and exclusive, with and without a start value, in place; the batch inverse with residues of 0; the division by X - z
// with its remainder; a grand product that closes at 1; an msm over the quotient a division left on the device.
// Run on a GPU box: node js/test-scans.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, ZERO, ONE, same, eq, upload, read, throwsWith } = require("./test-support.js");

// kept here: the copies of powmod differ (this one reduces a base that is never negative with %)
function powmod(x, e, q) {
  let r = ONE, b = x % q;
  for (e = BigInt(e); e > ZERO; e >>= ONE) { if (e & ONE) r = (r * b) % q; b = (b * b) % q; }
  return r;
}

function scanRef(vals, q, op, exclusive, init) {
  let acc = init;
  const out = [];
  for (const v of vals) {
    if (exclusive) out.push(acc);
    acc = op === "sum" ? (acc + v) % q : (acc * v) % q;
    if (!exclusive) out.push(acc);
  }
  return { out, total: acc };
}

function divRef(vals, q, z) {
  const out = vals.map(() => ZERO);
  let acc = ZERO;
  for (let j = vals.length - 1; j >= 0; j--) { out[j] = acc; acc = (acc * z + vals[j]) % q; }
  return { out, rem: acc };
}

async function runCurve(curve, label) {
  const q = curve.params.order, P = curve.Parallel;
  const next = stream(59);
  const raw256 = () => (next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next();
  const big = () => raw256() % q;
  const unit = () => (raw256() % (q - ONE)) + ONE;
  const top = (ONE << BigInt(256)) - ONE;
  let cases = 0;
  for (const n of [257, 65537]) {
    // some elements not canonical: they count as their residues
    const V = Array.from({ length: n }, (_, i) => (i % 7 === 3 ? [q, q + ONE, top, ZERO][(i >> 3) % 4] : big()));
    const U = Array.from({ length: n }, (_, i) => (i % 7 === 3 ? [q + ONE, top][(i >> 3) % 2] : unit()));
    const Vq = V.map((t) => t % q), Uq = U.map((t) => t % q);
    const v = await upload(curve, V), u = await upload(curve, U);
    const d = P.getScalarPointer(0);
    const init = big(), z = big();
    let ref = scanRef(Vq, q, "sum", false, ZERO);
    assert(P.scalarsScan(d, v, n) === ref.total && d.n === n && eq(read(curve, d, n), ref.out), `${label} ${n} sum`);
    ref = scanRef(Vq, q, "sum", true, init);
    assert(P.scalarsScan(d, v, n, { exclusive: true, init }) === ref.total && eq(read(curve, d, n), ref.out), `${label} ${n} exclusive sum`);
    ref = scanRef(Uq, q, "product", false, ONE);
    assert(P.scalarsScan(d, u, n, { op: "product" }) === ref.total && eq(read(curve, d, n), ref.out), `${label} ${n} product`);
    ref = scanRef(Uq, q, "product", true, init);
    assert(P.scalarsScan(d, u, n, { op: "product", exclusive: true, init }) === ref.total && eq(read(curve, d, n), ref.out),
      `${label} ${n} exclusive product`);
    assert(eq(read(curve, v, n), V) && eq(read(curve, u, n), U), `${label} ${n} the sources are as they were`);
    cases += 5;
    // the inverse: residues of 0 give 0 and are counted
    const zeros = Vq.filter((t) => t === ZERO).length;
    assert(P.scalarsInverse(d, v, n) === zeros, `${label} ${n} zero count`);
    const inv = read(curve, d, n);
    assert(inv.every((r, i) => r < q && (Vq[i] === ZERO ? r === ZERO : (r * Vq[i]) % q === ONE)), `${label} ${n} inverse`);
    assert(inv[0] === powmod(Vq[0], q - BigInt(2), q), `${label} ${n} inverse by Fermat`);
    cases += 2;
    // the grand product of a permutation argument: num a permutation of den, so prod num[i] / den[i] = 1
    const den = await upload(curve, Uq), num = await upload(curve, Uq.slice(1).concat(Uq.slice(0, 1)));
    assert(P.scalarsInverse(den, den, n) === 0, `${label} ${n} no zero among the denominators`);
    P.scalarsMul(num, num, den, n);
    assert(P.scalarsScan(num, num, n, { op: "product", exclusive: true }) === ONE, `${label} ${n} grand product closes at 1`);
    assert(read(curve, num, 1)[0] === ONE, `${label} ${n} grand product starts at 1`);
    cases += 3;
    // division by X - z, in place
    const dr = divRef(Vq, q, z);
    assert(P.scalarsDivLinear(v, v, n, z) === dr.rem && eq(read(curve, v, n), dr.out), `${label} ${n} division by X - z`);
    assert(P.scalarsDivLinear(d, u, n, ZERO) === Uq[0] && eq(read(curve, d, n), Uq.slice(1).concat([ZERO])), `${label} ${n} division by X`);
    cases += 2;
    if (n === 257) {
      // the witness of an opening: an msm over the quotient where it lies, against the msm over the quotient computed here
      const pp = await P.randomPointsFast(n, { seed: 13 });
      const want = await upload(curve, dr.out);
      assert(same((await P.msm(v, pp, n)).result, (await P.msm(want, pp, n)).result), `${label} msm over the quotient`);
      // refusals; the pointers go on working
      throwsWith(() => P.scalarsScan(d, u, n, { init: q }), /msm error 6/, `${label} init = q`);
      throwsWith(() => P.scalarsDivLinear(d, u, n, q), /msm error 6/, `${label} z = q`);
      throwsWith(() => P.scalarsScan(d, u, n, { op: "max" }), /op must be/, `${label} unknown op`);
      throwsWith(() => P.scalarsInverse(d, u, n + 1), /holds/, `${label} more than the pointer holds`);
      ref = scanRef(Uq, q, "product", false, ONE);
      assert(P.scalarsScan(d, u, n, { op: "product" }) === ref.total && eq(read(curve, d, n), ref.out), `${label} after the refusals`);
      cases += 6;
      pp.free();
      want.free();
    }
    for (const p of [v, u, d, den, num]) p.free();
  }
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 scans ok:", await runCurve(bls, "bls12-377"), "cases");
  bls.close();
  const bn = M.Weierstrass.create(M.bn254Params);
  console.log("bn254 scans ok:", await runCurve(bn, "bn254"), "cases");
  bn.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
