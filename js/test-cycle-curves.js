// BN254 G1, Grumpkin and Vesta through the JS facade: 32-byte coordinates, Parallel.msm against the known discrete logs of
// the curve's generator (sum s_i (a_i G) = (sum s_i a_i) G, each a_i G from a one-point MSM over G), msmUnsafe == msm,
// msmBatch and msmNarrow == msm.  Run on a GPU box: node js/test-cycle-curves.js
"use strict";
const M = require("./montgomery-hip.js");
const { assert, stream, same } = require("./test-support.js");

const generators = {
  bn254: [BigInt(1), BigInt(2)],
  grumpkin: [BigInt(1), BigInt("0x2cf135e7506a45d632d270d45f1181294833fc48d823f272c")],
  vesta: [M.vestaParams.modulus - BigInt(1), BigInt(2)],
};

function scalars(n, q, seed) {
  const next = stream(seed), out = [];
  for (let i = 0; i < n; i++) out.push(((next() << BigInt(192)) | (next() << BigInt(128)) | (next() << BigInt(64)) | next()) % q);
  return out;
}

async function msmOf(curve, pointBytes, vals) {
  const n = vals.length;
  const pp = curve.Parallel.getPointer(pointBytes.length);
  const sp = curve.Parallel.getScalarPointer(32 * n);
  await curve.Parallel.pointsFromBytes(pp, pointBytes, n);
  await curve.Parallel.scalarsFromBytes(sp, Buffer.concat(vals.map((v) => M.bigintToLeBytes(v, 32))), n);
  const safe = (await curve.Parallel.msm(sp, pp, n)).result;
  const unsafe = (await curve.Parallel.msmUnsafe(sp, pp, n)).result;
  assert(same(safe, unsafe), "msmUnsafe == msm");
  return { result: safe, pp, sp };
}

async function runCurve(params) {
  const label = params.label, q = params.order, p = params.modulus;
  const curve = M.Weierstrass.create(params);
  const [gx, gy] = generators[label];
  assert((gy * gy - gx * gx * gx - (label === "bn254" ? BigInt(3) : label === "grumpkin" ? p - BigInt(17) : BigInt(5))) % p === BigInt(0), `${label} generator`);
  const G = Buffer.concat([M.bigintToLeBytes(gx, 32), M.bigintToLeBytes(gy, 32)]);
  // q G = O, (q - 1) G = -G, 1 G = G
  let r = await msmOf(curve, G, [BigInt(1)]);
  assert(!r.result.isZero && r.result.x === gx && r.result.y === gy, `${label} 1 G`);
  r.pp.free(); r.sp.free();
  r = await msmOf(curve, G, [q - BigInt(1)]);
  assert(r.result.x === gx && r.result.y === p - gy, `${label} (q - 1) G = -G`);
  r.pp.free(); r.sp.free();
  r = await msmOf(curve, Buffer.concat([G, G]), [q - BigInt(5), BigInt(5)]);
  assert(r.result.isZero, `${label} (q - 5) G + 5 G = O`);
  r.pp.free(); r.sp.free();
  // points a_i G, each from a one-point MSM
  const n = 64, a = scalars(n, q, 11), s = scalars(n, q, 12);
  const rows = [];
  for (let i = 0; i < n; i++) {
    const one = await msmOf(curve, G, [a[i]]);
    rows.push(Buffer.concat([M.bigintToLeBytes(one.result.x, 32), M.bigintToLeBytes(one.result.y, 32)]));
    one.pp.free(); one.sp.free();
  }
  const pts = Buffer.concat(rows);
  assert(pts.length === 64 * n, "32-byte coordinates");
  let k = BigInt(0);
  for (let i = 0; i < n; i++) k = (k + a[i] * s[i]) % q;
  const exp = await msmOf(curve, G, [k]);
  const got = await msmOf(curve, pts, s);
  assert(same(got.result, exp.result), `${label} sum s_i a_i G`);
  exp.pp.free(); exp.sp.free();
  // compute_msm, batch and narrow over the same points
  const cm = await M.compute_msm_on(curve, 32, pts, Buffer.concat(s.map((v) => M.bigintToLeBytes(v, 32))));
  assert(cm.x === got.result.x && cm.y === got.result.y, `${label} compute_msm`);
  const vecs = [21, 22, 23].map((seed) => scalars(n, q, seed));
  const sps = [];
  for (const v of vecs) {
    const sp = curve.Parallel.getScalarPointer(32 * n);
    await curve.Parallel.scalarsFromBytes(sp, Buffer.concat(v.map((x) => M.bigintToLeBytes(x, 32))), n);
    sps.push(sp);
  }
  const batch = await curve.Parallel.msmBatch(sps, got.pp, n);
  for (let b = 0; b < vecs.length; b++) {
    const single = (await curve.Parallel.msm(sps[b], got.pp, n)).result;
    assert(same(batch[b].result, single), `${label} batch element ${b}`);
    sps[b].free();
  }
  const small = scalars(n, BigInt(1) << BigInt(32), 31);
  const narrow = await curve.Parallel.msmNarrow(Uint32Array.from(small.map(Number)), got.pp, n);
  const wide = await msmOf(curve, pts, small);
  assert(same(narrow.result, wide.result), `${label} msmNarrow`);
  wide.pp.free(); wide.sp.free();
  got.pp.free(); got.sp.free();
  curve.close();
  console.log(`${label} ok`);
}

async function main() {
  for (const params of [M.bn254Params, M.grumpkinParams, M.vestaParams]) await runCurve(params);
  console.log("cycle curves ok");
}

main().catch((e) => { console.error(e); process.exit(1); });
