// Parallel.scalarsSumcheckRound / scalarsBind / scalarsEq against BigInt arithmetic: one whole sumcheck per curve family over
// tables of 2^8 scalars -- the product of two tables binding the top variable in place, eq(tau) times two tables binding
// variable 0 out of place, and the R1CS shape -- with s(0) + s(1) = claim in every round and, at the end, every bound scalar
// equal to <eq(point), table>; then the eq table itself and the refusals.
// Run on a GPU box: node js/test-sumcheck.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, ZERO, ONE, eq, upload, read, throwsWith } = require("./test-support.js");

const mod = (x, q) => ((x % q) + q) % q;

// kept here: the copies of powmod differ (this one takes a base of either sign through mod)
function powmod(x, e, q) {
  let r = ONE, b = mod(x, q);
  for (e = BigInt(e); e > ZERO; e >>= ONE) { if (e & ONE) r = (r * b) % q; b = (b * b) % q; }
  return r;
}

// element i = s prod_j (bit_j(i) ? r[j] : 1 - r[j])
function eqRef(r, s, q) {
  let tab = [mod(s, q)];
  for (const x of r) tab = tab.map((t) => mod(t * (ONE - x), q)).concat(tab.map((t) => mod(t * x, q)));
  return tab;
}

const gOf = (shape, f, q) => (shape === "r1cs" ? mod(f[0] * (f[1] * f[2] - f[3]), q) : f.reduce((p, x) => mod(p * x, q), ONE));

// the value at x of the polynomial through (t, evals[t])
function interpolate(evals, x, q) {
  let total = ZERO;
  evals.forEach((y, t) => {
    let num = ONE, den = ONE;
    evals.forEach((_, u) => { if (u !== t) { num = mod(num * (x - BigInt(u)), q); den = mod(den * BigInt(t - u), q); } });
    total = mod(total + y * num * powmod(den, q - BigInt(2), q), q);
  });
  return total;
}

async function protocol(curve, label, shape, m, withEq, order, next) {
  const q = curve.params.order, P = curve.Parallel, V = 8, N = 1 << V;
  const raw256 = () => (next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next();
  const top = (ONE << BigInt(256)) - ONE;
  // some elements not canonical: they count as their residues
  const tables = Array.from({ length: m }, () => Array.from({ length: N }, (_, i) => (i % 7 === 3 ? [q, q + ONE, top, ZERO][(i >> 3) % 4] : raw256() % q)));
  const tau = Array.from({ length: V }, () => raw256() % q);
  const ptrs = [];
  for (let j = 0; j < m; j++) {
    if (j === 0 && withEq) {
      tables[0] = eqRef(tau, ONE, q);
      ptrs.push(P.scalarsEq(tau));
      assert(eq(read(curve, ptrs[0], N), tables[0]), `${label} eq(tau)`);
    } else {
      ptrs.push(await upload(curve, tables[j]));
    }
  }
  const originals = [];
  for (let j = 0; j < m; j++) originals.push(await upload(curve, tables[j]));
  let claim = ZERO;
  for (let i = 0; i < N; i++) claim = mod(claim + gOf(shape, tables.map((t) => t[i]), q), q);
  if (shape === "prod" && m === 2) assert(P.scalarsInner(ptrs[0], ptrs[1], N) === claim, `${label} the claim is the inner product`);
  let cur = ptrs, spare = Array.from({ length: m }, () => P.getScalarPointer(0));
  const point = new Array(V);
  for (let k = 0; k < V; k++) {
    const log2n = V - k, variable = order === "top" ? log2n - 1 : 0;
    const evals = P.scalarsSumcheckRound(cur, log2n, variable, { shape });
    assert(evals.length === (shape === "r1cs" ? 4 : m + 1), `${label} round ${k}: ${evals.length} values`);
    assert(mod(evals[0] + evals[1], q) === claim, `${label} round ${k}: s(0) + s(1) is the claim`);
    const r = raw256() % q;
    claim = interpolate(evals, r, q);
    if (order === "top") {
      P.scalarsBind(cur, log2n, variable, r);
      assert(cur.every((p) => p.n === 2 ** (log2n - 1)), `${label} round ${k}: the pointers hold half`);
      point[V - 1 - k] = r;
    } else {
      const bound = P.scalarsBind(cur, log2n, variable, r, { dst: spare });
      spare = cur;
      cur = bound;
      point[k] = r;
    }
  }
  const finals = cur.map((p) => read(curve, p, 1)[0]);
  const eqPoint = P.scalarsEq(point);
  const eqVals = eqRef(point, ONE, q);
  for (let j = 0; j < m; j++) {
    assert(finals[j] === P.scalarsInner(eqPoint, originals[j], N), `${label} table ${j} bound = <eq(point), table> on the device`);
    assert(finals[j] === eqVals.reduce((a, e, i) => mod(a + e * tables[j][i], q), ZERO), `${label} table ${j} bound = <eq(point), table>`);
  }
  assert(gOf(shape, finals, q) === claim, `${label} g of the bound scalars is the last claim`);
  for (const p of ptrs.concat(spare, originals, [eqPoint])) p.free();
  return V;
}

async function runCurve(curve, label) {
  const q = curve.params.order, P = curve.Parallel;
  const next = stream(61);
  let rounds = 0;
  rounds += await protocol(curve, `${label} prod2/top`, "prod", 2, false, "top", next);
  rounds += await protocol(curve, `${label} eq*prod3/var0`, "prod", 3, true, "var0", next);
  rounds += await protocol(curve, `${label} r1cs/top`, "r1cs", 4, true, "top", next);
  rounds += await protocol(curve, `${label} r1cs/var0`, "r1cs", 4, true, "var0", next);
  // the eq table: a scale, a point of zeros and ones, no variables at all
  const r = [BigInt(3), q - ONE, ZERO, ONE, BigInt(5)], s = q - BigInt(2);
  let e = P.scalarsEq(r, s);
  assert(e.n === 32 && eq(read(curve, e, 32), eqRef(r, s, q)), `${label} eq with a scale`);
  e.free();
  e = P.scalarsEq([ONE, ZERO, ONE]);
  assert(eq(read(curve, e, 8), [0, 0, 0, 0, 0, 1, 0, 0].map(BigInt)), `${label} eq of a point of the cube`);
  e.free();
  e = P.scalarsEq([], BigInt(7));
  assert(e.n === 1 && read(curve, e, 1)[0] === BigInt(7), `${label} eq over no variables`);
  // refusals; the pointers go on working
  const a = await upload(curve, [ONE, BigInt(2), BigInt(3), BigInt(4)]);
  throwsWith(() => P.scalarsEq([q]), /msm error 6/, `${label} r = q`);
  throwsWith(() => P.scalarsBind([a], 2, 1, q), /msm error 6/, `${label} bind r = q`);
  throwsWith(() => P.scalarsBind([a], 2, 0, ONE), /in place/, `${label} in place below the top`);
  throwsWith(() => P.scalarsSumcheckRound([a], 2, 2), /msm error 1/, `${label} var = log2n`);
  throwsWith(() => P.scalarsSumcheckRound([a, a, a], 2, 0, { shape: "r1cs" }), /msm error 1/, `${label} r1cs with three tables`);
  throwsWith(() => P.scalarsSumcheckRound([a], 3, 0), /holds/, `${label} more than the pointer holds`);
  throwsWith(() => P.scalarsSumcheckRound([a], 2, 0, { shape: "sum" }), /shape must be/, `${label} unknown shape`);
  assert(eq(P.scalarsSumcheckRound([a], 2, 0), [BigInt(4), BigInt(6)]), `${label} the plain sum after the refusals`);
  assert(eq(P.scalarsSumcheckRound([a, a], 2, 1), [BigInt(5), BigInt(25), BigInt(61)]), `${label} squares after the refusals`);
  for (const p of [e, a]) p.free();
  return rounds;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 sumcheck ok:", await runCurve(bls, "bls12-377"), "rounds");
  bls.close();
  const bn = M.Weierstrass.create(M.bn254Params);
  console.log("bn254 sumcheck ok:", await runCurve(bn, "bn254"), "rounds");
  bn.close();
  const pallas = M.Weierstrass.create(M.pallasParams);
  console.log("pallas sumcheck ok:", await runCurve(pallas, "pallas"), "rounds");
  pallas.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 sumcheck ok:", await runCurve(ed, "ed-on-bls12-377"), "rounds");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
