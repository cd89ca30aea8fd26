// Parallel.pointsNtt against a BigInt transform: over points d[j] G made by pointsMulBase the result must be the points E[k] G,
// E = the transform of d -- compared through MSMs under random scalars with pointsMulBase(E); round trips in place and inside one
// set; and the use of it: the inverse transform of a monomial key [tau^j] G is the Lagrange key, on which an MSM over the
// EVALUATIONS of a polynomial gives the commitment an MSM over its coefficients gives on the monomial key (on a coset: the
// transpose inverse, 1 / n times the forward transform under omega^-1 and shift^-1).
// Run on a GPU box: node js/test-points-ntt.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same, throwsWith } = require("./test-support.js");

const bytesOf = (vals) => Buffer.concat(vals.map((v) => M.bigintToLeBytes(v, 32)));

// kept here: the copies of powmod differ (this one takes a BigInt exponent only)
function powMod(b, e, q) {
  let r = BigInt(1);
  b %= q;
  for (; e > BigInt(0); e >>= BigInt(1)) { if (e & BigInt(1)) r = (r * b) % q; b = (b * b) % q; }
  return r;
}
const invMod = (a, q) => powMod(a, q - BigInt(2), q);

// the documented map: forward D[k] = sum_j (shift omega^k)^j d[j]; inverse: its exact inverse
function transform(d, omega, shift, inverse, q) {
  const n = d.length, out = [];
  const w = inverse ? invMod(omega, q) : omega;
  const tab = [BigInt(1)];
  for (let e = 1; e < n; e++) tab.push((tab[e - 1] * w) % q);
  const a = inverse ? d : d.map((v, j) => (v * powMod(shift, BigInt(j), q)) % q);
  for (let k = 0; k < n; k++) {
    let acc = BigInt(0);
    for (let j = 0; j < n; j++) acc += a[j] * tab[(j * k) % n];
    out.push(acc % q);
  }
  if (!inverse) return out;
  const ni = invMod(BigInt(n), q), si = invMod(shift, q);
  return out.map((v, j) => (((v * ni) % q) * powMod(si, BigInt(j), q)) % q);
}

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

async function runCurve(curve, label, maxLog, keyLog) {
  const q = curve.params.order, P = curve.Parallel;
  const next = stream(53);
  const big = () => ((next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next()) % q;
  const src = P.getPointer(0), dst = P.getPointer(0), ref = P.getPointer(0);
  let cases = 0;
  // forward and inverse, the library's root and another, with and without a shift, from row 0 and from row 3
  for (let L = 0; L <= maxLog; L++) {
    const n = 2 ** L, aLo = L % 2 ? 3 : 0;
    const d = Array.from({ length: n + aLo }, big), t = Array.from({ length: n }, big), u = Array.from({ length: n }, big);
    P.pointsMulBase(src, bytesOf(d));
    const root = L ? P.scalarsRootOfUnity(L) : BigInt(1);
    for (const inverse of [false, true]) {
      for (const own of [false, true]) {
        const omega = own ? powMod(root, BigInt(3), q) : root;
        const shift = own === inverse ? big() | BigInt(2) : BigInt(1);
        const options = { aLo, inverse };
        if (own) options.omega = omega;
        if (shift !== BigInt(1)) options.shift = shift;
        P.pointsNtt(dst, src, L, options);
        assert(dst.n === n && P.pointsetSize(dst) === n && src.n === n + aLo, `${label} 2^${L} sizes`);
        P.pointsMulBase(ref, bytesOf(transform(d.slice(aLo), omega, shift, inverse, q)));
        for (const s of [t, u])
          assert(same(await msmOver(curve, dst, s), await msmOver(curve, ref, s)), `${label} 2^${L} inverse=${inverse} own root=${own}`);
        cases++;
      }
    }
  }
  // round trips: out of place inside one set (the rows [n, 2 n) -> the rows [0, n)), then back in place
  {
    const L = maxLog, n = 2 ** L;
    const d = Array.from({ length: 2 * n }, big), t = Array.from({ length: n }, big);
    const shift = big() | BigInt(2);
    for (const inverse of [false, true]) {
      P.pointsMulBase(src, bytesOf(d));
      P.pointsMulBase(ref, bytesOf(d.slice(n)));
      const want = await msmOver(curve, ref, t);
      P.pointsNtt(src, src, L, { aLo: n, shift, inverse });
      assert(src.n === n && P.pointsetSize(src) === n, `${label} truncated to n`);
      P.pointsNtt(src, src, L, { shift, inverse: !inverse });
      assert(src.n === n && same(await msmOver(curve, src, t), want), `${label} round trip, inverse first = ${inverse}`);
      cases++;
    }
    // refusals; the pointers go on working
    P.pointsMulBase(src, bytesOf(d));
    if (L >= 1) {
      throwsWith(() => P.pointsNtt(src, src, L, { aLo: 1 }), /msm error 1/, `${label} overlap`);
      throwsWith(() => P.pointsNtt(dst, src, L, { aLo: n + 1 }), /msm error 4/, `${label} range beyond the set`);
      throwsWith(() => P.pointsNtt(dst, src, L, { omega: BigInt(1) }), /msm error 1.*order/, `${label} omega of order 1`);
      throwsWith(() => P.pointsNtt(dst, src, L, { omega: q }), /msm error 6/, `${label} omega = q`);
    }
    throwsWith(() => P.pointsNtt(dst, src, L, { shift: 0 }), /msm error 1/, `${label} shift = 0`);
    throwsWith(() => P.pointsNtt(dst, src, 30), /msm error 1/, `${label} log2n = 30`);
    assert(src.n === 2 * n && P.pointsetSize(src) === 2 * n, `${label} after the refusals`);
    cases += 6;
  }
  // monomial key -> Lagrange key
  if (keyLog) {
    const L = keyLog, n = 2 ** L;
    const tau = big() | BigInt(2);
    const f = Array.from({ length: n }, big);
    const pw = P.scalarsPowers(tau, n);
    P.pointsMulBase(src, pw);
    const commitment = await msmOver(curve, src, f);
    const fp = await scalarPtrOf(curve, f);
    for (const shift of [null, big() | BigInt(2)]) {
      if (shift === null) {
        P.pointsNtt(dst, src, L, { inverse: true });
      } else {
        P.pointsNtt(dst, src, L, { omega: invMod(P.scalarsRootOfUnity(L), q), shift: invMod(shift, q) });
        P.pointsLincomb(dst, invMod(BigInt(n), q), dst, null, null, { count: n });
      }
      const ev = P.scalarsNtt(P.getScalarPointer(0), fp, L, { shift });
      const { result } = await P.msm(ev, dst, n);
      assert(same(result, commitment), `${label} Lagrange key, shift = ${shift}`);
      ev.free();
      cases++;
    }
    fp.free(); pw.free();
  }
  src.free(); dst.free(); ref.free();
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 points ntt ok:", await runCurve(bls, "bls12-377", 5, 8), "cases");
  bls.close();
  const pallas = M.Weierstrass.create(M.pallasParams);
  console.log("pallas points ntt ok:", await runCurve(pallas, "pallas", 5, 0), "cases");
  pallas.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 points ntt ok:", await runCurve(ed, "ed-on-bls12-377", 1, 0), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
