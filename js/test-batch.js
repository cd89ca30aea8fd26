// Parallel.msmBatch against Parallel.msm, element by element, on the golden vectors (tests/golden/msm377.json,
// msm_ed377.json).  Run on a GPU box: node js/test-batch.js
"use strict";
const fs = require("fs");
const path = require("path");
const M = require("./montgomery-hip.js");
const { assert } = require("./test-support.js");

// the case's scalars, the same scalars rotated by one point, and all zeros
function variants(sc, n) {
  const rot = Buffer.alloc(sc.length);
  if (n > 0) { sc.copy(rot, 0, 32); sc.copy(rot, 32 * (n - 1), 0, 32); }
  return [sc, rot, Buffer.alloc(sc.length)];
}

async function runCurve(curve, goldFile, coordBytes) {
  const gold = JSON.parse(fs.readFileSync(path.join(__dirname, "..", "tests", "golden", goldFile), "utf8"));
  let cases = 0;
  for (const c of gold.cases) {
    if (c.n === 0) continue;
    let pts = Buffer.from(c.points, "hex");
    if (coordBytes !== 48 && pts.length === 96 * c.n) {   // (48-byte coordinates in the file: the low bytes of each)
      const parts = [];
      for (let i = 0; i < pts.length / 48; i++) parts.push(pts.subarray(48 * i, 48 * i + coordBytes));
      pts = Buffer.concat(parts);
    }
    const pp = curve.Parallel.getPointer(pts.length);
    await curve.Parallel.pointsFromBytes(pp, pts, c.n);
    const sps = [];
    for (const sc of variants(Buffer.from(c.scalars, "hex"), c.n)) {
      const sp = curve.Parallel.getScalarPointer(sc.length);
      await curve.Parallel.scalarsFromBytes(sp, sc, c.n);
      sps.push(sp);
    }
    const opts = { c: c.c || 0 };
    const batch = await curve.Parallel.msmBatch(sps, pp, c.n, true, opts);
    assert(batch.length === sps.length, "one result per scalar pointer");
    for (let b = 0; b < sps.length; b++) {
      const { result } = await curve.Parallel.msm(sps[b], pp, c.n, false, opts);
      const r = batch[b].result;
      assert(r.isZero === result.isZero && r.x === result.x && r.y === result.y, `${goldFile} ${c.name} element ${b}`);
      assert(batch[b].log.length > 0, "log");
    }
    cases++;
  }
  return cases;
}

async function main() {
  const bls = M.Weierstrass.create(M.bls12377Params);
  console.log("bls12-377 batch ok:", await runCurve(bls, "msm377.json", 48), "cases");
  bls.close();
  const ed = M.TwistedEdwards.create(M.edOnBls12377Params);
  console.log("ed-on-bls12-377 batch ok:", await runCurve(ed, "msm_ed377.json", 32), "cases");
  ed.close();
  console.log("ALL OK");
}

main().catch((e) => { console.error(e); process.exit(1); });
