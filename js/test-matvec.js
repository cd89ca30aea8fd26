// Parallel.matrixFromTriplets / matrixCreate / matrixInfo / scalarsMatvec against BigInt arithmetic: the ladder of row lengths
// 0, 4, 5, 63, 64, 65, 128, 129, 5 * 64 + 3 at the forced thresholds (4, 64) with alpha and accumulate, the all-ones gather, the
// transposition with the adjoint identity, and three refusals.
// Run on a GPU box: node js/test-matvec.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, ZERO, ONE, eq, upload, read, throwsWith } = require("./test-support.js");

const mod = (x, q) => ((x % q) + q) % q;

// triples -> the product as BigInts: out[r] = alpha sum val x[col] + old[r]
function productRef(rows, trip, x, q, alpha, old) {
  const out = new Array(rows).fill(ZERO);
  for (const [r, c, v] of trip) out[r] += (v === undefined ? ONE : v) * x[c];
  return out.map((s, r) => mod((alpha === undefined ? ONE : alpha) * s + (old ? old[r] : ZERO), q));
}

async function runCurve(curve, label) {
  const q = curve.params.order, P = curve.Parallel;
  const next = stream(67);
  const raw256 = () => (next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next();
  const top = (ONE << BigInt(256)) - ONE;
  const element = (i) => (i % 7 === 3 ? [q, q + ONE, top, ZERO][(i >> 3) % 4] : raw256() % q);   // some not canonical
  const small = (n) => Number(next() % BigInt(n));

  // the ladder at the forced thresholds (4, 64): triples given row by row from the last row up, so the sort has work to do
  const lens = [0, 4, 5, 63, 64, 65, 128, 129, 5 * 64 + 3], cols = 50;
  const trip = [];
  for (let r = lens.length - 1; r >= 0; r--) for (let k = 0; k < lens[r]; k++) trip.push([r, small(cols), element(trip.length)]);
  const x = Array.from({ length: cols }, (_, i) => element(i + 1));
  const xp = await upload(curve, x);
  const csr = P.matrixFromTriplets(lens.length, cols, trip);
  assert(eq(Array.from(csr.rowPtr), lens.reduce((a, n) => a.concat([a[a.length - 1] + n]), [0])), `${label} rowPtr of the ladder`);
  const id = P.matrixCreate(csr, { testGeometry: [4, 64] });
  const info = P.matrixInfo(id);
  assert(info.rows === lens.length && info.cols === cols && info.nnz === trip.length && info.bytes >= 36 * trip.length, `${label} matrixInfo`);
  const dst = P.getScalarPointer(0);
  P.scalarsMatvec(id, dst, xp);
  assert(dst.n === lens.length && eq(read(curve, dst, lens.length), productRef(lens.length, trip, x, q)), `${label} the ladder`);
  assert(eq(P.testLastMatvec(), [4, 64, 7, 16, 3]), `${label} the ladder's plan: ${P.testLastMatvec()}`);
  const old = lens.map((_, r) => element(7 * r + 3)), alpha = q - BigInt(2);
  const acc = await upload(curve, old);
  P.scalarsMatvec(id, acc, xp, { alpha, accumulate: true });
  assert(eq(read(curve, acc, lens.length), productRef(lens.length, trip, x, q, alpha, old)), `${label} the ladder with alpha and accumulate`);
  // the same matrix at the default thresholds gives the same elements
  const id2 = P.matrixCreate(csr);
  const dst2 = P.getScalarPointer(0);
  P.scalarsMatvec(id2, dst2, xp);
  assert(eq(read(curve, dst2, lens.length), read(curve, dst, lens.length)), `${label} the default thresholds`);

  // the all-ones gather: a permutation of 300 rows
  const n = 300, perm = Array.from({ length: n }, (_, i) => i);
  for (let i = n - 1; i > 0; i--) { const j = small(i + 1); [perm[i], perm[j]] = [perm[j], perm[i]]; }
  const t = Array.from({ length: n }, (_, i) => element(i + 2));
  const tp = await upload(curve, t);
  const gather = P.matrixFromTriplets(n, n, perm.map((p, i) => [i, p]));
  assert(gather.val === null, `${label} triples without values give the all-ones form`);
  const gid = P.matrixCreate(gather);
  assert(P.matrixInfo(gid).bytes < 36 * n, `${label} the all-ones form stores no coefficients`);
  const gp = P.getScalarPointer(0);
  P.scalarsMatvec(gid, gp, tp);
  assert(eq(read(curve, gp, n), perm.map((p) => mod(t[p], q))), `${label} the gather`);

  // transposition: by the library from the host CSR, by the helper from the triples; column 0 is hit by every row
  const R = 40, C = 23, tt = [];
  for (let r = 0; r < R; r++) { tt.push([r, 0, element(r)]); for (let k = small(4); k > 0; k--) tt.push([r, small(C), element(r + k)]); }
  const y = Array.from({ length: R }, (_, i) => element(i + 5)), z = Array.from({ length: C }, (_, i) => element(i + 6));
  const yp = await upload(curve, y), zp = await upload(curve, z);
  const m = P.matrixCreate(P.matrixFromTriplets(R, C, tt), { testGeometry: [4, 64] });
  const mt = P.matrixCreate(P.matrixFromTriplets(R, C, tt), { transpose: true, testGeometry: [4, 64] });
  const mt2 = P.matrixCreate(P.matrixFromTriplets(R, C, tt, true));
  const ti = P.matrixInfo(mt);
  assert(ti.rows === C && ti.cols === R && ti.nnz === tt.length, `${label} the transposed handle is cols x rows`);
  const want = productRef(C, tt.map(([r, c, v]) => [c, r, v]), y, q);
  const mty = P.getScalarPointer(0), mty2 = P.getScalarPointer(0), mz = P.getScalarPointer(0);
  P.scalarsMatvec(mt, mty, yp);
  assert(P.testLastMatvec()[2] >= 1, `${label} the column of every row is a long row`);
  P.scalarsMatvec(mt2, mty2, yp);
  P.scalarsMatvec(m, mz, zp);
  assert(eq(read(curve, mty, C), want) && eq(read(curve, mty2, C), want), `${label} the transposed product`);
  assert(P.scalarsInner(yp, mz, R) === P.scalarsInner(mty, zp, C), `${label} <y, M z> = <M^T y, z>`);

  // three refusals; the handles go on working
  throwsWith(() => P.matrixCreate({ rows: 2, cols: 3, rowPtr: [0, 1, 2], col: [0, 3], val: null }), /msm error 1.*col\[1\] = 3 but cols = 3/, `${label} a column index out of range`);
  throwsWith(() => P.scalarsMatvec(id, dst, xp, { alpha: q }), /msm error 6/, `${label} alpha = q`);
  throwsWith(() => P.scalarsMatvec(gid, tp, tp), /msm error 1.*overlaps/, `${label} dst = x`);
  P.matrixDestroy(id2);
  throwsWith(() => P.scalarsMatvec(id2, dst2, xp), /msm error 1.*no matrix/, `${label} a destroyed id`);
  P.scalarsMatvec(id, dst2, xp);
  assert(eq(read(curve, dst2, lens.length), productRef(lens.length, trip, x, q)), `${label} the ladder after the refusals`);
  for (const i of [id, gid, m, mt, mt2]) P.matrixDestroy(i);
  for (const p of [xp, dst, acc, dst2, tp, gp, yp, zp, mty, mty2, mz]) p.free();
  return trip.length + n + 3 * tt.length;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 matvec ok:", await runCurve(bls, "bls12-377"), "entries");
  bls.close();
  const bn = M.Weierstrass.create(M.bn254Params);
  console.log("bn254 matvec ok:", await runCurve(bn, "bn254"), "entries");
  bn.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 matvec ok:", await runCurve(ed, "ed-on-bls12-377"), "entries");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
