// Parallel.scalarsNtt / scalarsRootOfUnity against a BigInt transform: forward, inverse, coset, a caller's root, batches, in
// place, a polynomial product, and an msm over the coefficients an inverse transform left on the device.
// Run on a GPU box: node js/test-ntt.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same, eq, upload, read, throwsWith } = require("./test-support.js");

// kept here: the copies of powmod differ (this one spells its constants out and takes e as a number or a BigInt)
function powmod(x, e, q) {
  let r = BigInt(1), b = x % q;
  for (e = BigInt(e); e > BigInt(0); e >>= BigInt(1)) { if (e & BigInt(1)) r = (r * b) % q; b = (b * b) % q; }
  return r;
}

// out[k] = sum_j a[j] (shift omega^k)^j by Horner's rule, O(n^2): the definition
function evaluate(a, q, omega, shift) {
  return a.map((_, k) => {
    const x = (shift * powmod(omega, k, q)) % q;
    let acc = BigInt(0);
    for (let j = a.length - 1; j >= 0; j--) acc = (acc * x + a[j]) % q;
    return acc;
  });
}

async function runCurve(curve, label, nonResidue, adicity) {
  const q = curve.params.order, P = curve.Parallel, log2n = 6, n = 64;
  const next = stream(53);
  const raw256 = () => (next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next();
  const big = () => raw256() % q;
  const top = (BigInt(1) << BigInt(256)) - BigInt(1);
  let cases = 0;
  // the root formula
  const omega = P.scalarsRootOfUnity(log2n);
  assert(omega === powmod(BigInt(nonResidue), (q - BigInt(1)) >> BigInt(log2n), q), `${label} root of unity`);
  assert(powmod(omega, n / 2, q) === q - BigInt(1), `${label} root order`);
  throwsWith(() => P.scalarsRootOfUnity(adicity + 1), /factor/, `${label} no such root`);
  cases += 3;
  // three vectors back to back, some elements not canonical: they count as their residues
  const V = Array.from({ length: 3 * n }, (_, i) => (i % 7 === 3 ? [q, q + BigInt(1), top, BigInt(0)][(i >> 3) % 4] : big()));
  const Vq = V.map((t) => t % q);
  const v = await upload(curve, V);
  const shift = big() || BigInt(5), omega3 = powmod(omega, 3, q);
  const one = BigInt(1);
  const fwd = P.scalarsNtt(P.getScalarPointer(0), v, log2n);
  assert(fwd.n === n && eq(read(curve, fwd, n), evaluate(Vq.slice(0, n), q, omega, one)), `${label} forward`);
  const coset = P.scalarsNtt(P.getScalarPointer(0), v, log2n, { shift, omega: omega3, batch: 3 });
  const expCoset = [0, 1, 2].map((b) => evaluate(Vq.slice(b * n, (b + 1) * n), q, omega3, shift));
  assert(coset.n === 3 * n && eq(read(curve, coset, 3 * n), [].concat(...expCoset)), `${label} coset batch with a caller's root`);
  P.scalarsNtt(coset, coset, log2n, { shift, omega: omega3, batch: 3, inverse: true });
  assert(eq(read(curve, coset, 3 * n), Vq), `${label} inverse in place`);
  assert(eq(read(curve, v, 3 * n), V), `${label} the source is as it was`);
  cases += 4;
  // a polynomial product: two polynomials of degree < 32 at n = 64
  const A = Array.from({ length: 32 }, big), B = Array.from({ length: 32 }, big);
  const zeros = Array.from({ length: 32 }, () => BigInt(0));
  const pa = await upload(curve, A.concat(zeros)), pb = await upload(curve, B.concat(zeros));
  P.scalarsNtt(pa, pa, log2n);
  P.scalarsNtt(pb, pb, log2n);
  P.scalarsMul(pa, pa, pb, n);
  P.scalarsNtt(pa, pa, log2n, { inverse: true });
  const prod = Array.from({ length: n }, () => BigInt(0));
  A.forEach((x, i) => B.forEach((y, j) => { prod[i + j] = (prod[i + j] + x * y) % q; }));
  assert(eq(read(curve, pa, n), prod), `${label} polynomial product`);
  cases += 1;
  // evaluations -> coefficients -> msm, nothing leaves the device; against the msm over coefficients computed here
  const pp = await P.randomPointsFast(n, { seed: 11 });
  const coeffs = P.scalarsNtt(P.getScalarPointer(0), fwd, log2n, { inverse: true });
  const want = await upload(curve, Vq.slice(0, n));
  assert(same((await P.msm(coeffs, pp, n)).result, (await P.msm(want, pp, n)).result), `${label} msm over the inverse transform`);
  cases += 1;
  // refusals; the pointers go on working
  throwsWith(() => P.scalarsNtt(fwd, v, log2n, { omega: (omega * omega) % q }), /msm error 1.*order/, `${label} omega of order n / 2`);
  throwsWith(() => P.scalarsNtt(fwd, v, log2n, { omega: q }), /msm error 6/, `${label} omega = q`);
  throwsWith(() => P.scalarsNtt(fwd, v, log2n, { shift: 0 }), /msm error 1/, `${label} shift = 0`);
  throwsWith(() => P.scalarsNtt(fwd, v, log2n, { batch: 4 }), /holds/, `${label} more than the pointer holds`);
  throwsWith(() => P.scalarsNtt(fwd, v, 30), /msm error 1|holds/, `${label} log2n = 30`);
  P.scalarsNtt(fwd, v, log2n);
  assert(eq(read(curve, fwd, n), evaluate(Vq.slice(0, n), q, omega, one)), `${label} after the refusals`);
  cases += 6;
  for (const p of [v, fwd, coset, pa, pb, coeffs, want]) p.free();
  pp.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 ntt ok:", await runCurve(bls, "bls12-377", 11, 47), "cases");
  bls.close();
  const bn = M.Weierstrass.create(M.bn254Params);
  console.log("bn254 ntt ok:", await runCurve(bn, "bn254", 5, 28), "cases");
  bn.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
