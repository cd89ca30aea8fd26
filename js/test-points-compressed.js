// pointsFromBytes with {compressed, validate} against the uncompressed load: the same msm, and a refused point throws with its
// index.  Run on a GPU box: node js/test-points-compressed.js DIR, where DIR holds <curve>.raw (n points, x || y) and
// <curve>.cmp (the same points compressed) for curve = bls377, bls381, ed377 (tests/test_napi_points.py writes them).
"use strict";
const fs = require("fs");
const path = require("path");
const M = require("./montgomery-hip.js");
const { assert } = require("./test-support.js");
const dir = process.argv[2];

async function runCurve(curve, label, file, coordBytes) {
  const raw = fs.readFileSync(path.join(dir, file + ".raw"));
  const enc = fs.readFileSync(path.join(dir, file + ".cmp"));
  const n = enc.length / coordBytes;
  assert(raw.length === n * 2 * coordBytes && n > 4321, `${label}: input sizes`);
  const sp = await curve.Parallel.randomScalars(n, { seed: 78 });
  const pu = curve.Parallel.getPointer(raw.length);
  await curve.Parallel.pointsFromBytes(pu, raw, n);
  const pc = curve.Parallel.getPointer(enc.length);
  await curve.Parallel.pointsFromBytes(pc, enc, n, { compressed: true, validate: "subgroup" });
  const a = (await curve.Parallel.msm(sp, pu, n)).result;
  const b = (await curve.Parallel.msm(sp, pc, n)).result;
  assert(a.isZero === b.isZero && a.x === b.x && a.y === b.y, `${label}: msm over compressed-loaded points`);
  // a coordinate >= p at index 4321 (all-ones bytes, flags included: >= p whatever the layout)
  const bad = Buffer.from(enc);
  bad.fill(0xff, 4321 * coordBytes, 4321 * coordBytes + coordBytes);
  if (label === "bls12-381") bad[4321 * coordBytes] = 0x9f;   // compressed, no infinity / sign flag, x >= p
  if (label === "bls12-377") bad[4321 * coordBytes + coordBytes - 1] = 0x01;   // no flags, bit 376 set: x >= p
  if (label === "ed-on-bls12-377") bad[4321 * coordBytes + coordBytes - 1] = 0x1f;   // no flags, y >= r
  let threw = null;
  try {
    await curve.Parallel.pointsFromBytes(pc, bad, n, { compressed: true, validate: "subgroup" });
  } catch (e) {
    threw = e;
  }
  assert(threw !== null, `${label}: a bad point must throw`);
  assert(/point 4321: coordinate >= p/.test(threw.message) && threw.badIndex === 4321, `${label}: ${threw.message}`);
  return a;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  await runCurve(bls, "bls12-377", "bls377", 48);
  console.log("bls12-377 compressed ok");
  bls.close();
  const b381 = M.Weierstrass.create(M.bls12381Params);
  await runCurve(b381, "bls12-381", "bls381", 48);
  console.log("bls12-381 compressed ok");
  b381.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  await runCurve(ed, "ed-on-bls12-377", "ed377", 32);
  console.log("ed-on-bls12-377 compressed ok");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
