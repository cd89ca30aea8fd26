// JS facade over the N-API shim: the reference's curve-module surface for the MSM path.
//   Weierstraß.create(params) -> { params, Parallel }            src/parallel.ts:40-177
//   Parallel.{getPointer, getScalarPointer, pointsFromBytes, scalarsFromBytes, msm, msmUnsafe}, and Parallel.msmBatch (many MSMs
//   over one point set in one call)
//                                                                src/parallel.ts:135-145
//   compute_msm(points, scalars) -> {x: bigint, y: bigint}       scripts/zprize23/submission-bls377.ts:20-65
// Plain CommonJS without top-level await so the image's node 12 can load it (the reference's own
// sources need node >= 20).  In the reference "pointers" are offsets into wasm memory; here they are
// small handle objects, the data lives in buffers owned by libmsm_hip.so.
"use strict";
const path = require("path");
const hip = require(path.join(__dirname, "..", "montgomery_amd", "msm_hip.node"));

const bls12377Params = {
  label: "bls12-377",
  modulus: BigInt("0x01ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001"),
  order: BigInt("0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001"),
};
const bls12381Params = {
  label: "bls12-381",
  modulus: BigInt("0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab"),
  order: BigInt("0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001"),
};
const pallasParams = {
  label: "pallas",
  modulus: BigInt("0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001"),
  order: BigInt("0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001"),
};
// the two curve cycles of recursive provers (not in the reference): 32-byte coordinates like Pallas
const bn254Params = {
  label: "bn254",   // alt_bn128 G1 (EIP-196): y^2 = x^3 + 3, generator (1, 2)
  modulus: BigInt("0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47"),
  order: BigInt("0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001"),
};
const grumpkinParams = {
  label: "grumpkin",   // y^2 = x^3 - 17 over BN254's scalar field
  modulus: bn254Params.order,
  order: bn254Params.modulus,
};
const vestaParams = {
  label: "vesta",   // y^2 = x^3 + 5 over Pallas' scalar field, generator (-1, 2)
  modulus: pallasParams.order,
  order: pallasParams.modulus,
};
const edOnBls12377Params = {
  label: "ed-on-bls12-377",
  modulus: BigInt("0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001"),
  order: BigInt("0x4aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff"),
};

function leBytesToBigint(buf) {
  let x = BigInt(0);
  for (let i = buf.length - 1; i >= 0; i--) x = (x << BigInt(8)) | BigInt(buf[i]);
  return x;
}
function bigintToLeBytes(x, n) {
  const out = Buffer.alloc(n);
  for (let i = 0; i < n; i++) { out[i] = Number(x & BigInt(255)); x >>= BigInt(8); }
  return out;
}

function createCurve(params, curveId, coordBytes, device, wireBytes) {
  wireBytes = wireBytes || coordBytes;   // the reference's packed coordinate size = the C ABI's: 48, or 32 for the 255-bit fields
  const ctx = hip.createContext(curveId, device || 0);   // device: an index, or a list of indices (one context over several GPUs)
  const pointBytes = 2 * coordBytes;
  // `let [pointPtr] = await Parallel.randomPointsFast(N)` -- the reference hands back one pointer per point / scalar and its
  // callers keep the first (scripts/msm-weierstrass.ts:18,21,29); a handle here stands for the whole array, so it unpacks to itself
  const firstOf = (ptr) => { ptr[Symbol.iterator] = function* () { yield ptr; }; return ptr; };
  const Parallel = {
    // every point pointer is its own resident point set of the context, as every pointer of the reference is its own
    // allocation; msm() selects the set of the pointer it is given
    getPointer(size) { return { size, n: 0, set: hip.pointsetCreate(ctx), free() { hip.pointsetDestroy(ctx, this.set); } }; },
    // A scalar pointer owns ONE device buffer from scalarsFromBytes / randomScalars on: the reference's scalars live in the
    // memory its kernels compute in (src/parallel.ts:119-133), so msm() crosses no PCIe.  free() gives the buffer back at
    // once; a pointer that is simply dropped gives it back when it is collected (the addon registers a finalizer).
    getScalarPointer(size) { return newScalarPtr(size); },
    // options (optional): {compressed: the curve's compressed encoding (one coordinate and flag bits, INTEGRATION.md),
    // validate: "curve" | "subgroup" | undefined (none, as the reference)}; a refused point throws with its index
    async pointsFromBytes(pointPtr, input, n, options) {
      if (options && (options.compressed || options.validate)) {
        const levels = { none: hip.VALIDATE_NONE, curve: hip.VALIDATE_CURVE, subgroup: hip.VALIDATE_SUBGROUP };
        const validate = options.validate ? levels[options.validate] : hip.VALIDATE_NONE;
        if (validate === undefined) throw new RangeError(`pointsFromBytes: unknown validate level ${options.validate}`);
        const step = options.compressed ? coordBytes : pointBytes;
        hip.pointsetSelect(ctx, pointPtr.set);
        pointPtr.n = 0;
        pointPtr.n = hip.setPointsEx(ctx, Buffer.from(input.buffer, input.byteOffset, n * step),
          options.compressed ? hip.POINTS_COMPRESSED : hip.POINTS_UNCOMPRESSED, validate);
        return;
      }
      let b = Buffer.from(input.buffer, input.byteOffset, n * 2 * wireBytes);
      if (wireBytes !== coordBytes) {
        const padded = Buffer.alloc(n * pointBytes);
        for (let i = 0; i < 2 * n; i++) b.copy(padded, i * coordBytes, i * wireBytes, (i + 1) * wireBytes);
        b = padded;
      }
      hip.pointsetSelect(ctx, pointPtr.set);
      pointPtr.n = hip.setPoints(ctx, b, pointBytes, 0);
    },
    async scalarsFromBytes(scalarPtr, input, n) {   // src/parallel.ts:119-133: one upload, then resident
      scalarPtr.free();
      scalarPtr.dev = hip.deviceAlloc(ctx, Math.max(32 * n, 32));
      hip.deviceUpload(ctx, scalarPtr.dev, Buffer.from(input.buffer, input.byteOffset, n * 32));
      scalarPtr.n = n;
    },
    async randomPointsFast(n, options) {   // src/curve-random.ts:14-92; generated on the GPU, explicit seed
      const pointPtr = Parallel.getPointer(n * 2 * wireBytes);
      pointPtr.n = hip.generatePoints(ctx, n, (options && options.seed) || 1);
      return firstOf(pointPtr);
    },
    async randomScalars(n, options) {      // src/curve-random.ts:151-194: generated in HBM, nothing crosses PCIe
      const ptr = newScalarPtr(n * 32);
      const seed = (options && options.seed) || 1;
      ptr.dev = hip.deviceAlloc(ctx, Math.max(32 * n, 32));
      hip.generateScalars(ctx, n, seed, ptr.dev);
      ptr.n = n;
      ptr.toBytes = () => hip.generateScalars(ctx, n, seed);   // the same stream read back (tests)
      return firstOf(ptr);
    },
    async msm(scalarPtr, pointPtr, N, verboseTiming, options) {
      const c = (options && options.c) || 0;
      if (N > pointPtr.n) throw new Error(`msm: ${N} scalars but ${pointPtr.n} points behind this pointer`);
      if (!scalarPtr.dev || N > scalarPtr.n) throw new Error(`msm: ${N} scalars requested but the scalar pointer holds ${scalarPtr.dev ? scalarPtr.n : 0}`);
      hip.pointsetSelect(ctx, pointPtr.set);
      const unsafe = options && options.useSafeAdditions === false ? 1 : 0;
      const r = hip.msmDevice(ctx, scalarPtr.dev, N, c, options && options.noGlv ? 1 : 0, unsafe);
      const result = { x: leBytesToBigint(r.x), y: leBytesToBigint(r.y), isZero: r.isZero };
      return { result, log: verboseTiming ? buildLog(N, r) : [] };
    },
    // many MSMs over one point set in one call (msm_run_batch): [b].result equals (await msm(scalarPtrs[b], pointPtr, N)).result
    async msmBatch(scalarPtrs, pointPtr, N, verboseTiming, options) {
      const c = (options && options.c) || 0;
      if (N > pointPtr.n) throw new Error(`msmBatch: ${N} scalars but ${pointPtr.n} points behind this pointer`);
      for (const sp of scalarPtrs)
        if (!sp.dev || N > sp.n) throw new Error(`msmBatch: ${N} scalars requested but a scalar pointer holds ${sp.dev ? sp.n : 0}`);
      hip.pointsetSelect(ctx, pointPtr.set);
      const unsafe = options && options.useSafeAdditions === false ? 1 : 0;
      const rs = hip.msmBatchDevice(ctx, scalarPtrs.map((sp) => sp.dev), N, c, options && options.noGlv ? 1 : 0, unsafe);
      return rs.map((r) => ({
        result: { x: leBytesToBigint(r.x), y: leBytesToBigint(r.y), isZero: r.isZero },
        log: verboseTiming ? buildLog(N, r) : [],
      }));
    },
    // Narrow scalars (msm_run_narrow; the reference has no counterpart): `scalars` is a Uint8Array .. BigUint64Array (unsigned) or
    // Int8Array .. BigInt64Array (signed) -- width and signedness from the array type -- or a Buffer with options {width, signed};
    // options.bits: magnitude bits (default: all the width gives), options.c: window.  result equals msm over the same values
    // written as 32-byte scalars (negatives as q - |v|); a value outside the declared range throws (msm error 6).
    async msmNarrow(scalars, pointPtr, N, options) {
      const f = narrowFormat(scalars, N, options);
      if (N > pointPtr.n) throw new Error(`msmNarrow: ${N} scalars but ${pointPtr.n} points behind this pointer`);
      hip.pointsetSelect(ctx, pointPtr.set);
      const r = hip.msmNarrow(ctx, f.buf, f.width, f.bits, f.signed, (options && options.c) || 0);
      return { result: { x: leBytesToBigint(r.x), y: leBytesToBigint(r.y), isZero: r.isZero }, log: buildLog(N, r) };
    },
    // many narrow MSMs over one point set (msm_run_batch_narrow): one array per element, all of one type and length
    async msmBatchNarrow(scalarArrays, pointPtr, N, options) {
      if (!scalarArrays.length) throw new RangeError("msmBatchNarrow: empty batch");
      const fs = scalarArrays.map((s) => narrowFormat(s, N, options));
      for (const f of fs)
        if (f.width !== fs[0].width || f.signed !== fs[0].signed) throw new TypeError("msmBatchNarrow: the elements must share one format");
      if (N > pointPtr.n) throw new Error(`msmBatchNarrow: ${N} scalars but ${pointPtr.n} points behind this pointer`);
      hip.pointsetSelect(ctx, pointPtr.set);
      const rs = hip.msmBatchNarrow(ctx, fs.map((f) => f.buf), fs[0].width, fs[0].bits, fs[0].signed, (options && options.c) || 0);
      return rs.map((r) => ({ result: { x: leBytesToBigint(r.x), y: leBytesToBigint(r.y), isZero: r.isZero }, log: buildLog(N, r) }));
    },
    // Indexed (sparse) MSM (msm_run_indexed; the reference has no counterpart): sum_j scalars[j] * P[indices[j]] over the points
    // behind pointPtr.  scalars: a Buffer / Uint8Array of m x 32 bytes; indices: a Uint32Array, or an array of m non-negative
    // integers -- any order, repeats allowed.  options: {c, noGlv}.  result equals msm over the dense equivalent (the vector with
    // t[i] = sum of scalars[j] over indices[j] == i); an index >= the number of points throws (msm error 1) naming its position.
    async msmIndexed(scalars, indices, pointPtr, options) {
      const idx = indexBuffer(indices, "msmIndexed");
      if (!ArrayBuffer.isView(scalars) || scalars.byteLength !== 32 * idx.m)
        throw new RangeError(`msmIndexed: ${idx.m} indices need ${32 * idx.m} bytes of scalars`);
      hip.pointsetSelect(ctx, pointPtr.set);
      const r = hip.msmIndexed(ctx, Buffer.from(scalars.buffer, scalars.byteOffset, scalars.byteLength), idx.buf,
        (options && options.c) || 0, options && options.noGlv ? 1 : 0);
      return { result: { x: leBytesToBigint(r.x), y: leBytesToBigint(r.y), isZero: r.isZero }, log: buildLog(idx.m, r) };
    },
    // the same over narrow scalars (msm_run_indexed_narrow): scalars and options {bits, width, signed, c} as for msmNarrow
    async msmIndexedNarrow(scalars, indices, pointPtr, options) {
      const idx = indexBuffer(indices, "msmIndexedNarrow");
      const f = narrowFormat(scalars, idx.m, options);
      if (f.width * idx.m !== scalars.byteLength) throw new RangeError(`msmIndexedNarrow: ${idx.m} indices but ${scalars.byteLength / f.width} scalars`);
      hip.pointsetSelect(ctx, pointPtr.set);
      const r = hip.msmIndexedNarrow(ctx, f.buf, idx.buf, f.width, f.bits, f.signed, (options && options.c) || 0);
      return { result: { x: leBytesToBigint(r.x), y: leBytesToBigint(r.y), isZero: r.isZero }, log: buildLog(idx.m, r) };
    },
    // Point-set linear combinations (msm_points_lincomb; the reference has no counterpart): the points behind dstPtr become
    // dst[i] = a * A[aLo + i] + b * B[bLo + i], i < count.  a, b: BigInt / number or 32 little-endian bytes, < the group order
    // (a larger value throws msm error 6); b and ptrB null: one term.  options: {aLo, bLo, count} (count: default all of ptrA from
    // aLo on).  dstPtr may be ptrA or ptrB: a source range inside it is its rows [0, count) or starts at or above row count.
    pointsLincomb(dstPtr, a, ptrA, b, ptrB, options) {
      const o = options || {}, aLo = o.aLo || 0, bLo = o.bLo || 0;
      if ((b === null || b === undefined) !== (ptrB === null || ptrB === undefined)) throw new TypeError("pointsLincomb: b and ptrB come together");
      const count = o.count === undefined ? Math.max(ptrA.n - aLo, 0) : o.count;
      dstPtr.n = hip.pointsLincomb(ctx, ptrA.set, aLo, scalarBuffer(a, "a"), ptrB ? ptrB.set : -1, bLo, ptrB ? scalarBuffer(b, "b") : null, count, dstPtr.set);
      return dstPtr;
    },
    // points behind a pointer, as the library counts them (msm_pointset_size)
    pointsetSize(pointPtr) { return hip.pointsetSize(ctx, pointPtr.set); },
    // the in-place fold of an inner-product argument: P[i] <- a * P[i] + b * P[i + n/2], i < n/2; the pointer then holds n/2 points
    foldPoints(pointPtr, a, b) {
      const n = pointPtr.n;
      if (n % 2) throw new RangeError(`foldPoints: the pointer holds ${n} points, an odd number`);
      return Parallel.pointsLincomb(pointPtr, a, pointPtr, b, pointPtr, { aLo: 0, bLo: n / 2, count: n / 2 });
    },
    // Per-row scalar multiplication (msm_points_mul; the reference has no counterpart): the points behind dstPtr become
    // dst[i] = s[i] * A[aLo + i], i < count, every row under its own scalar.  scalars: a scalar pointer (the scalars stay on the
    // device: what scalarsPowers or scalarsInverse wrote) or count x 32 little-endian bytes; values at or above the group order
    // are reduced.  options: {aLo, sLo, count} (sLo: the first scalar of a scalar pointer; count: default all the scalars from sLo
    // on).  dstPtr may be ptrA with aLo = 0 or aLo >= count.
    pointsMul(dstPtr, scalars, ptrA, options) {
      const o = options || {}, v = scalarVector(scalars, o, "pointsMul");
      dstPtr.n = hip.pointsMul(ctx, ptrA.set, o.aLo || 0, v.arg, v.off, v.count, dstPtr.set);
      return dstPtr;
    },
    // the same for one base point (msm_points_mul_base): dst[i] = s[i] * base.  base: {x, y} of BigInts, x || y as bytes in the
    // wire format of pointsFromBytes, or null / undefined for the curve's generator.  options: {sLo, count}
    pointsMulBase(dstPtr, scalars, base, options) {
      const o = options || {}, v = scalarVector(scalars, o, "pointsMulBase");
      let b = null;
      if (base !== null && base !== undefined) {
        if (ArrayBuffer.isView(base)) {
          if (base.byteLength !== 2 * wireBytes) throw new RangeError(`pointsMulBase: the base must be ${2 * wireBytes} bytes (x || y)`);
          b = Buffer.alloc(pointBytes);
          for (let i = 0; i < 2; i++) Buffer.from(base.buffer, base.byteOffset, base.byteLength).copy(b, i * coordBytes, i * wireBytes, (i + 1) * wireBytes);
        } else {
          b = Buffer.concat([bigintToLeBytes(BigInt(base.x), coordBytes), bigintToLeBytes(BigInt(base.y), coordBytes)]);
        }
      }
      dstPtr.n = hip.pointsMulBase(ctx, b, v.arg, v.off, v.count, dstPtr.set);
      return dstPtr;
    },
    // The transform over points (msm_points_ntt; the reference has no counterpart): the points behind dstPtr become the transform
    // of the n = 2^log2n points [aLo, aLo + n) behind ptrA, natural order in and out.  forward: dst[k] = sum_j (shift omega^k)^j A[j];
    // inverse: the exact inverse map -- over a monomial key [tau^j] G and without a shift it gives the key in the Lagrange basis
    // of <omega>; the key of the coset shift <omega> is 1 / n times the FORWARD transform under omega^-1 and shift^-1.  options: {aLo, inverse, omega, shift} -- omega: a primitive n-th root of unity (default:
    // scalarsRootOfUnity(log2n)), shift: in [1, order) (default 1), both BigInt / number or 32 bytes.  dstPtr may be ptrA with
    // aLo = 0 or aLo >= n.
    pointsNtt(dstPtr, ptrA, log2n, options) {
      const o = options || {};
      const opt = (v, what) => (v === undefined || v === null ? null : scalarBuffer(v, what));
      dstPtr.n = hip.pointsNtt(ctx, ptrA.set, o.aLo || 0, log2n, opt(o.omega, "omega"), opt(o.shift, "shift"), !!o.inverse, dstPtr.set);
      return dstPtr;
    },
    // Resident scalar vectors (msm_scalars_*; the reference has no counterpart): arithmetic mod the group order over the scalars
    // behind scalar pointers, which stay on the device.  Host scalars x, y, s: BigInt / number or 32 bytes, below the group order
    // (a larger value throws msm error 6); elements of the vectors may be any 32-byte integers and are taken mod the order.
    // dstPtr[i] = x * ptrA[aLo + i] + y * ptrB[bLo + i], i < count; y and ptrB null: one term.  options: {aLo, bLo, dstLo, count}
    // (count: default all of ptrA from aLo on).  dstPtr may be ptrA or ptrB over the same elements; a pointer without a buffer
    // that large gets one.
    scalarsLincomb(dstPtr, x, ptrA, y, ptrB, options) {
      const o = options || {}, aLo = o.aLo || 0, bLo = o.bLo || 0, dstLo = o.dstLo || 0;
      if ((y === null || y === undefined) !== (ptrB === null || ptrB === undefined)) throw new TypeError("scalarsLincomb: y and ptrB come together");
      const count = o.count === undefined ? Math.max(ptrA.n - aLo, 0) : o.count;
      needScalars(ptrA, aLo + count, "scalarsLincomb");
      if (ptrB) needScalars(ptrB, bLo + count, "scalarsLincomb");
      roomFor(dstPtr, dstLo + count);
      hip.scalarsLincomb(ctx, dstPtr.dev, dstLo, scalarBuffer(x, "x"), ptrA.dev, aLo, ptrB ? scalarBuffer(y, "y") : null,
        ptrB ? ptrB.dev : null, bLo, count);
      return dstPtr;
    },
    // dstPtr[i] = ptrA[i] * ptrB[i], i < N
    scalarsMul(dstPtr, ptrA, ptrB, N) {
      needScalars(ptrA, N, "scalarsMul");
      needScalars(ptrB, N, "scalarsMul");
      roomFor(dstPtr, N);
      hip.scalarsMul(ctx, dstPtr.dev, 0, ptrA.dev, 0, ptrB.dev, 0, N);
      return dstPtr;
    },
    // sum_i ptrA[aLo + i] * ptrB[bLo + i], i < N, as a BigInt.  options: {aLo, bLo}
    scalarsInner(ptrA, ptrB, N, options) {
      const o = options || {}, aLo = o.aLo || 0, bLo = o.bLo || 0;
      needScalars(ptrA, aLo + N, "scalarsInner");
      needScalars(ptrB, bLo + N, "scalarsInner");
      return leBytesToBigint(hip.scalarsInner(ctx, ptrA.dev, aLo, ptrB.dev, bLo, N));
    },
    // a new scalar pointer holding (s, s x, s x^2, ..., s x^(N-1)); s: default 1
    scalarsPowers(x, N, s) {
      const ptr = newScalarPtr(32 * N);
      roomFor(ptr, N);
      hip.scalarsPowers(ctx, ptr.dev, 0, scalarBuffer(s === undefined || s === null ? 1 : s, "s"), scalarBuffer(x, "x"), N);
      return firstOf(ptr);
    },
    // The resident NTT (msm_scalars_ntt): dstPtr = the transform of the `batch` vectors of 2^log2n scalars at the start of ptr,
    // natural order in and out.  forward: dst[k] = sum_j a[j] (shift omega^k)^j; inverse: the exact inverse map.
    // options: {inverse, omega, shift, batch} -- omega: a primitive 2^log2n-th root of unity (default: scalarsRootOfUnity(log2n)),
    // shift: in [1, order) (default 1), both BigInt / number or 32 bytes.  dstPtr may be ptr.
    scalarsNtt(dstPtr, ptr, log2n, options) {
      const o = options || {}, batch = o.batch === undefined ? 1 : o.batch;
      const count = batch * 2 ** log2n;
      needScalars(ptr, count, "scalarsNtt");
      roomFor(dstPtr, count);
      const opt = (v, what) => (v === undefined || v === null ? null : scalarBuffer(v, what));
      hip.scalarsNtt(ctx, dstPtr.dev, 0, ptr.dev, 0, log2n, batch, opt(o.omega, "omega"), opt(o.shift, "shift"), !!o.inverse);
      return dstPtr;
    },
    // the library's primitive 2^log2n-th root of unity mod the group order, as a BigInt (msm_scalars_root_of_unity)
    scalarsRootOfUnity(log2n) { return leBytesToBigint(hip.scalarsRootOfUnity(ctx, log2n)); },
    // Resident scans (msm_scalars_scan): dstPtr = the running sum or product mod the group order of the first N scalars of ptr;
    // returns the total as a BigInt.  options: {op: "sum" | "product", exclusive, init} -- inclusive: dst[i] = init o a[0] o ... o a[i],
    // exclusive: dst[i] = init o a[0] o ... o a[i-1]; init: BigInt / number or 32 bytes below the order (default 0 / 1).
    // dstPtr may be ptr.
    scalarsScan(dstPtr, ptr, N, options) {
      const o = options || {}, op = o.op === undefined ? "sum" : o.op;
      if (op !== "sum" && op !== "product") throw new TypeError(`scalarsScan: op must be "sum" or "product", not ${op}`);
      needScalars(ptr, N, "scalarsScan");
      roomFor(dstPtr, N);
      const init = o.init === undefined || o.init === null ? null : scalarBuffer(o.init, "init");
      return leBytesToBigint(hip.scalarsScan(ctx, dstPtr.dev, 0, ptr.dev, 0, N, op === "product" ? 1 : 0, !!o.exclusive, init));
    },
    // dstPtr[i] = ptr[i]^-1 mod the group order, 0 where the residue is 0; returns how many of those there were
    // (msm_scalars_inverse).  dstPtr may be ptr.
    scalarsInverse(dstPtr, ptr, N) {
      needScalars(ptr, N, "scalarsInverse");
      roomFor(dstPtr, N);
      return hip.scalarsInverse(ctx, dstPtr.dev, 0, ptr.dev, 0, N);
    },
    // dstPtr = the quotient of the polynomial with the N coefficients of ptr (the constant term first) by X - z, dstPtr[N-1] = 0;
    // returns the remainder, the polynomial's value at z, as a BigInt (msm_scalars_div_linear).  dstPtr may be ptr.
    scalarsDivLinear(dstPtr, ptr, N, z) {
      needScalars(ptr, N, "scalarsDivLinear");
      roomFor(dstPtr, N);
      return leBytesToBigint(hip.scalarsDivLinear(ctx, dstPtr.dev, 0, ptr.dev, 0, N, scalarBuffer(z, "z")));
    },
    // The resident sumcheck (msm_scalars_sumcheck_round / _bind / _eq) over multilinear tables of 2^log2n scalars at the start of
    // scalar pointers.  Variable j is bit j of the index: variable 0 is the least significant bit (arkworks' order); a caller
    // with the most-significant-first convention reverses its point.
    // The round polynomial s(0), .., s(d) as BigInts: s(t) = sum over the pairs of g(f_0(t), ..), f_j(t) = lo + t (hi - lo).
    // options: {shape: "prod" | "r1cs"} -- "prod": the product of 1 .. 4 tables, d = their number; "r1cs": f0 (f1 f2 - f3),
    // d = 3.  s(0) + s(1) is the claim of the round.  A sum of products runs one call per product: s is linear in g.
    scalarsSumcheckRound(ptrs, log2n, variable, options) {
      const o = options || {}, shape = o.shape === undefined ? "prod" : o.shape;
      if (shape !== "prod" && shape !== "r1cs") throw new TypeError(`scalarsSumcheckRound: shape must be "prod" or "r1cs", not ${shape}`);
      for (const p of ptrs) needScalars(p, 2 ** log2n, "scalarsSumcheckRound");
      const raw = hip.scalarsSumcheckRound(ctx, ptrs.map((p) => p.dev), ptrs.map(() => 0), log2n, variable, shape === "r1cs" ? 1 : 0);
      const out = [];
      for (let t = 0; t < raw.length / 32; t++) out.push(leBytesToBigint(raw.subarray(32 * t, 32 * t + 32)));
      return out;
    },
    // Binds `variable` of the tables behind ptrs (1 .. 8 of them) to r: dst[i] = lo(i) + r (hi(i) - lo(i)), i < 2^(log2n - 1).
    // Without options the top variable is bound in place and every pointer then holds 2^(log2n - 1) scalars; options {dst: [...]}
    // names as many destination pointers, which may not be the sources.  Returns the pointers that hold the result.
    scalarsBind(ptrs, log2n, variable, r, options) {
      const o = options || {}, n = 2 ** log2n, h = n / 2, zeros = ptrs.map(() => 0);
      for (const p of ptrs) needScalars(p, n, "scalarsBind");
      const srcs = ptrs.map((p) => p.dev);
      if (!o.dst) {
        if (variable !== log2n - 1) throw new RangeError("scalarsBind: only the top variable is bound in place; name options.dst");
        hip.scalarsBind(ctx, srcs, zeros, srcs, zeros, log2n, variable, scalarBuffer(r, "r"));
        for (const p of ptrs) p.n = h;
        return ptrs;
      }
      for (const d of o.dst) roomFor(d, h);
      hip.scalarsBind(ctx, o.dst.map((d) => d.dev), o.dst.map(() => 0), srcs, zeros, log2n, variable, scalarBuffer(r, "r"));
      return o.dst;
    },
    // a new scalar pointer holding the table eq(r, .) scaled by s (default 1): element i = s prod_j (bit_j(i) ? r[j] : 1 - r[j])
    scalarsEq(r, s) {
      const N = 2 ** r.length;
      const ptr = newScalarPtr(32 * N);
      roomFor(ptr, N);
      const rb = Buffer.concat(r.map((x) => scalarBuffer(x, "an entry of r")), 32 * r.length);
      hip.scalarsEq(ctx, ptr.dev, 0, rb, s === undefined || s === null ? null : scalarBuffer(s, "s"));
      return firstOf(ptr);
    },
    // Resident sparse matrices (msm_matrix_*, msm_scalars_matvec; the reference has no counterpart): a CSR matrix lives on the
    // device under an id, and dstPtr = alpha M xPtr (+ dstPtr) mod the group order over scalar pointers -- A z of an R1CS, the
    // transposed product of Spartan's second phase, and with all coefficients 1 the gather dst[i] = x[idx[i]] and the row sum.
    // (row, col, value) triples -> {rows, cols, rowPtr, col, val}: a stable sort over the rows, duplicates kept (the product sums
    // them).  value: BigInt / number in [0, 2^256) or 32 bytes; triples without a value give the all-ones form (val null).
    // transpose: the CSR of the transposed matrix, cols x rows.
    matrixFromTriplets(rows, cols, triplets, transpose) {
      let trip = triplets.map((t) => (transpose ? [t[1], t[0], t[2]] : [t[0], t[1], t[2]]));
      if (transpose) [rows, cols] = [cols, rows];
      const ones = trip.every((t) => t[2] === undefined || t[2] === null);
      if (!ones && trip.some((t) => t[2] === undefined || t[2] === null)) throw new TypeError("matrixFromTriplets: every triple carries a value, or none does");
      trip.forEach((t, j) => {
        if (!Number.isInteger(t[0]) || !Number.isInteger(t[1]) || t[0] < 0 || t[0] >= rows || t[1] < 0 || t[1] >= cols)
          throw new RangeError(`matrixFromTriplets: triple ${j} lies outside the ${rows} x ${cols} matrix`);
      });
      const rowPtr = new Uint32Array(rows + 1);
      for (const t of trip) rowPtr[t[0] + 1]++;
      for (let r = 0; r < rows; r++) rowPtr[r + 1] += rowPtr[r];
      const cursor = Array.from(rowPtr.subarray(0, rows)), col = new Uint32Array(trip.length);
      const val = ones ? null : Buffer.alloc(32 * trip.length);
      for (const t of trip) {
        const d = cursor[t[0]]++;
        col[d] = t[1];
        if (val) scalarBuffer(t[2], "a value").copy(val, 32 * d);
      }
      return { rows, cols, rowPtr, col, val };
    },
    // matrix: what matrixFromTriplets returns (rowPtr and col: Uint32Arrays; val: nnz x 32 bytes or null).  options:
    // {transpose}: the id then names the transposed matrix.  A defect of the CSR throws (msm error 1) naming its position.
    matrixCreate(matrix, options) {
      const u32 = (a) => { const t = a instanceof Uint32Array ? a : Uint32Array.from(a); return Buffer.from(t.buffer, t.byteOffset, t.byteLength); };
      const v = matrix.val === null || matrix.val === undefined ? null : Buffer.from(matrix.val.buffer, matrix.val.byteOffset, matrix.val.byteLength);
      const g = options && options.testGeometry;   // debug surface: [shortMax, partLen] of this matrix (msm_test_set_matvec_geometry)
      if (g) hip.testSetMatvecGeometry(ctx, g[0], g[1]);
      try {
        return hip.matrixCreate(ctx, matrix.rows, matrix.cols, u32(matrix.rowPtr), u32(matrix.col), v, options && options.transpose ? 1 : 0);
      } finally {
        if (g) hip.testSetMatvecGeometry(ctx, 0, 0);
      }
    },
    // debug surface: [shortMax, partLen, long rows, parts, launches] of the last scalarsMatvec (msm_test_last_matvec)
    testLastMatvec() { return hip.testLastMatvec(ctx); },
    matrixDestroy(id) { hip.matrixDestroy(ctx, id); },
    // {rows, cols, nnz, bytes} of a matrix as it is held; bytes: the device memory it takes
    matrixInfo(id) { return hip.matrixInfo(ctx, id); },
    // dstPtr = alpha M xPtr, plus the old dstPtr with options.accumulate.  options: {alpha: BigInt / number or 32 bytes below the
    // group order (default 1), accumulate}.  dstPtr and xPtr must be different pointers; without accumulate a dstPtr that holds
    // fewer than `rows` scalars gets a buffer of that size.
    scalarsMatvec(id, dstPtr, xPtr, options) {
      const o = options || {}, info = hip.matrixInfo(ctx, id);
      if (info.nnz) needScalars(xPtr, info.cols, "scalarsMatvec");
      if (o.accumulate) needScalars(dstPtr, info.rows, "scalarsMatvec");
      else roomFor(dstPtr, info.rows);
      hip.scalarsMatvec(ctx, id, dstPtr.dev, 0, info.nnz ? xPtr.dev : null, 0,
        o.alpha === undefined || o.alpha === null ? null : scalarBuffer(o.alpha, "alpha"), o.accumulate ? 1 : 0);
      return dstPtr;
    },
    // the in-place fold of an inner-product argument: v[i] <- a * v[i] + b * v[i + n/2], i < n/2; the pointer then holds n/2 scalars
    foldScalars(scalarPtr, a, b) {
      const n = scalarPtr.n;
      if (n % 2) throw new RangeError(`foldScalars: the pointer holds ${n} scalars, an odd number`);
      Parallel.scalarsLincomb(scalarPtr, a, scalarPtr, b, scalarPtr, { aLo: 0, bLo: n / 2, count: n / 2 });
      scalarPtr.n = n / 2;
      return scalarPtr;
    },
    // the first N scalars behind a pointer, back on the host: a Buffer of N x 32 bytes (msm_device_download)
    scalarsToBytes(scalarPtr, N) {
      N = N === undefined ? scalarPtr.n : N;
      needScalars(scalarPtr, N, "scalarsToBytes");
      return N ? hip.deviceDownload(ctx, scalarPtr.dev, 0, 32 * N) : Buffer.alloc(0);
    },
    // {unsigned, signed}: the smallest `bits` msmNarrow accepts these n x 32-byte scalars under as a Buffer with width 32
    // (0: all zero; 255: a scalar needs more than 128 bits)
    scalarBits(scalars32) {
      return hip.scalarBits(ctx, Buffer.from(scalars32.buffer, scalars32.byteOffset, scalars32.byteLength));
    },
    msmProjective(scalarPtr, pointPtr, N, options) {
      // src/parallel.ts:69-87: signed windows of the whole scalar, no endomorphism split (same group element)
      return Parallel.msm(scalarPtr, pointPtr, N, false, Object.assign({}, options, { noGlv: true }));
    },
    msmUnsafe(scalarPtr, pointPtr, N, verboseTiming, options) {   // src/msm-batched-affine.ts:587-598
      return Parallel.msm(scalarPtr, pointPtr, N, verboseTiming, Object.assign({}, options, { useSafeAdditions: false }));
    },
  };
  // typed array -> {buf, width, signed, bits} of the first N scalars; a Buffer / Uint8Array with options.width is raw bytes
  function narrowFormat(scalars, N, options) {
    const types = [[Int8Array, 1, 1], [Int16Array, 2, 1], [Int32Array, 4, 1], [Uint16Array, 2, 0], [Uint32Array, 4, 0]];
    if (typeof BigInt64Array !== "undefined") types.push([BigInt64Array, 8, 1], [BigUint64Array, 8, 0]);
    let width = 0, signed = 0;
    if (options && options.width) { width = options.width; signed = options.signed ? 1 : 0; }
    else if (scalars instanceof Uint8Array) { width = 1; signed = 0; }   // (a Buffer is one too)
    else for (const [T, w, s] of types) if (scalars instanceof T) { width = w; signed = s; }
    if (![1, 2, 4, 8, 16, 32].includes(width) || !ArrayBuffer.isView(scalars))
      throw new TypeError("msmNarrow: expected an integer typed array, or a Buffer with options.width in {1, 2, 4, 8, 16, 32}");
    if (N * width > scalars.byteLength) throw new RangeError(`msmNarrow: ${N} scalars of ${width} bytes requested but the array holds ${scalars.byteLength} bytes`);
    return { buf: Buffer.from(scalars.buffer, scalars.byteOffset, N * width), width, signed, bits: (options && options.bits) || 0 };
  }
  // indices of an indexed call -> {buf: m x 4 bytes, uint32 little-endian, m}; a Uint32Array is taken as it is
  // one scalar of pointsLincomb as 32 little-endian bytes: a BigInt / non-negative integer below 2^256, or 32 bytes
  function scalarBuffer(v, what) {
    if (typeof v === "bigint" || typeof v === "number") {
      if (typeof v === "number" && !Number.isSafeInteger(v)) throw new RangeError(`pointsLincomb: ${what} is not an integer`);
      const big = BigInt(v);
      if (big < BigInt(0) || big >> BigInt(256)) throw new RangeError(`pointsLincomb: ${what} must lie in [0, 2^256)`);
      return bigintToLeBytes(big, 32);
    }
    if (ArrayBuffer.isView(v) && v.byteLength === 32) return Buffer.from(v.buffer, v.byteOffset, 32);
    throw new TypeError(`pointsLincomb: ${what} must be a BigInt or 32 bytes`);
  }
  function indexBuffer(indices, who) {
    let arr = indices;
    if (!(arr instanceof Uint32Array)) {
      if (!Array.isArray(arr) && !ArrayBuffer.isView(arr)) throw new TypeError(`${who}: indices must be a Uint32Array or an array of integers`);
      if (arr instanceof Float32Array || arr instanceof Float64Array) throw new TypeError(`${who}: indices must be integers`);
      const list = Array.from(arr, (v) => (typeof v === "bigint" ? Number(v) : v));
      for (const v of list)
        if (!Number.isInteger(v) || v < 0 || v > 0xFFFFFFFF) throw new RangeError(`${who}: index ${v} is not an integer in [0, 2^32)`);
      arr = Uint32Array.from(list);
    }
    return { buf: Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength), m: arr.length };
  }
  // the scalar vector of pointsMul / pointsMulBase -> {arg, off, count} of the addon: a scalar pointer or n x 32 bytes
  function scalarVector(scalars, o, who) {
    if (ArrayBuffer.isView(scalars)) {
      if (scalars.byteLength % 32) throw new RangeError(`${who}: ${scalars.byteLength} bytes of scalars are not a multiple of 32`);
      const n = scalars.byteLength / 32, count = o.count === undefined ? n : o.count;
      if (count > n) throw new RangeError(`${who}: ${count} rows requested but ${n} scalars given`);
      return { arg: Buffer.from(scalars.buffer, scalars.byteOffset, scalars.byteLength), off: 0, count };
    }
    if (!scalars || typeof scalars !== "object" || !("dev" in scalars)) throw new TypeError(`${who}: scalars must be a scalar pointer or bytes`);
    const off = o.sLo || 0, count = o.count === undefined ? Math.max(scalars.n - off, 0) : o.count;
    needScalars(scalars, off + count, who);
    if (!count) return { arg: Buffer.alloc(0), off: 0, count };
    return { arg: scalars.dev, off, count };
  }
  function needScalars(ptr, n, who) {
    if (n > ptr.n || (n && !ptr.dev)) throw new Error(`${who}: ${n} scalars requested but the scalar pointer holds ${ptr.dev ? ptr.n : 0}`);
  }
  // a destination of the scalar-vector calls: a pointer that holds fewer than n scalars gets a buffer of n
  function roomFor(ptr, n) {
    if (ptr.dev && ptr.n >= n) return;
    ptr.free();
    ptr.dev = hip.deviceAlloc(ctx, Math.max(32 * n, 32));
    ptr.n = n;
  }
  function newScalarPtr(size) {
    return { size, n: 0, dev: null, free() { if (this.dev) { const d = this.dev; this.dev = null; this.n = 0; hip.deviceFree(ctx, d); } } };
  }
  // `log` in the reference's shape (createLog, src/msm-common.ts:176-214; filled at src/msm-batched-affine.ts:79-338): one
  // entry with the parameters, then one "label... x.xms" line per phase, "msm total" last.  The phases are the library's
  // eight device timings (msm_result.phase_ms) under the reference's labels where a counterpart exists.
  function buildLog(N, r) {
    const t = r.phaseMs, line = (label, ms) => [`${label}... ${ms.toFixed(1)}ms`];
    return [
      [{ n: Math.ceil(Math.log2(Math.max(N, 1))), K: r.K, c: r.c }],   // log({ n, K, c }), src/msm-batched-affine.ts:93
      line("scalars to device", t[1]),
      line("slice scalars & count buckets", t[2]),
      line("sort points", t[3]),
      line("bucket accumulation (first round)", t[7]),
      line("bucket accumulation", t[4]),
      line("bucket reduction (local)", t[5]),
      line("final sum", t[6]),
      line("msm total", t[0]),
    ];
  }
  // What the reference's callers do with `result` (scripts/msm-weierstrass.ts:89-91):
  //     let sAffinePtr = Curve.Field.getPointer(Curve.Affine.size);
  //     Curve.Projective.toAffine(scratch, sAffinePtr, result);
  //     let s = Curve.Affine.toBigint(sAffinePtr);
  // There `result` points at a projective point in wasm memory; here the library has already normalised it, so the three
  // calls only hand the value through: pointers are small objects, toAffine stores, toBigint returns {x, y, isZero}.
  const newPtr = (size) => ({ size, value: null });
  // The fine operator table (the reference's wasm exports, src/field-msm.ts:86-123,190-243): element-wise over Buffers of
  // n field elements (coordBytes each, little-endian, MONTGOMERY form like the reference's field elements in wasm memory)
  // instead of pointers into wasm memory; every call is one kernel launch over all n elements.  fromBigints / toBigints are
  // fromPackedBytes + toMontgomery and their inverse (src/field-msm.ts:108-115).
  const fieldOp = (op) => (a, b) => hip.fieldOp(ctx, op, a, b);
  const Field = {
    getPointer: newPtr, getPointers(n, size) { return Array.from({ length: n }, () => newPtr(size)); },
    sizeInBytes: coordBytes,
    multiply: fieldOp(hip.OP_MUL), square: fieldOp(hip.OP_SQR), add: fieldOp(hip.OP_ADD), subtract: fieldOp(hip.OP_SUB),
    inverse: fieldOp(hip.OP_INV), toMontgomery: fieldOp(hip.OP_TO_MONT), fromMontgomery: fieldOp(hip.OP_FROM_MONT),
    batchInverse(xs, perLane) { return hip.batchInverse(ctx, xs, perLane || 64); },   // src/wasm/inverse.ts:220-271
    fromBigints(vals) { return hip.fieldOp(ctx, hip.OP_TO_MONT, Buffer.concat(vals.map((v) => bigintToLeBytes(BigInt(v), coordBytes)))); },
    toBigints(buf) {
      const plain = hip.fieldOp(ctx, hip.OP_FROM_MONT, buf), out = [];
      for (let i = 0; i < plain.length; i += coordBytes) out.push(leBytesToBigint(plain.slice(i, i + coordBytes)));
      return out;
    },
  };
  // Scalar.decompose (src/scalar-glv.ts:105-128, src/wasm/glv.ts:68-169): s = (-1)^neg0 s0 + (-1)^neg1 s1 lambda mod q
  const Scalar = {
    decompose(scalars) {
      const sb = Buffer.isBuffer(scalars) ? scalars : Buffer.concat(scalars.map((v) => bigintToLeBytes(BigInt(v), 32)));
      const raw = hip.glvDecompose(ctx, sb), out = [];
      for (let i = 0; i < raw.length; i += 40)
        out.push({ s0: leBytesToBigint(raw.slice(i, i + 16)), s1: leBytesToBigint(raw.slice(i + 16, i + 32)),
                   neg0: raw.readUInt32LE(i + 32) !== 0, neg1: raw.readUInt32LE(i + 36) !== 0 });
      return out;
    },
  };
  const toBigint = (ptr) => { const r = (ptr && ptr.value) || ptr; return { x: r.x, y: r.y, isZero: !!r.isZero }; };
  // Affine.batchAdd (batchAddNew, src/curve-affine.ts:376-522): n pairs of affine points {x, y} | null (identity) -> n sums,
  // all through one launch of the tree kernel with its shared inversions; every kind of pair (P + P, P - P, identities) is handled
  const encPoint = (P) => (P ? Buffer.concat([bigintToLeBytes(BigInt(P.x), coordBytes), bigintToLeBytes(BigInt(P.y), coordBytes)]) : Buffer.alloc(pointBytes));
  const batchAdd = (G, H) => {
    const out = hip.batchAdd(ctx, Buffer.concat(G.map(encPoint)), Buffer.concat(H.map(encPoint))), sums = [];
    for (let i = 0; i < out.length; i += pointBytes) {
      const x = leBytesToBigint(out.slice(i, i + coordBytes)), y = leBytesToBigint(out.slice(i + coordBytes, i + pointBytes));
      sums.push(x === BigInt(0) && y === BigInt(0) ? null : { x, y });
    }
    return sums;
  };
  const Affine = { size: 2 * wireBytes + 4, toBigint, batchAdd };                         // src/curve-affine.ts:77, 220-233, 376-522
  const Projective = { size: 3 * wireBytes + 4, toAffine(_scratch, affinePtr, result) { affinePtr.value = toBigint(result); } };   // src/curve-projective.ts:335-349
  // twisted Edwards callers: `Curve.Curve.toBigint(result)` -> extended bigint point, `Curve.Bigint.toAffine(P)` -> {x, y}
  // (scripts/msm-twisted-edwards.ts:87, scripts/zprize23/submission.ts:33-34)
  const P_MOD = params.modulus;
  const modInv = (a) => { let [r0, r1, s0, s1] = [((a % P_MOD) + P_MOD) % P_MOD, P_MOD, BigInt(1), BigInt(0)];
    while (r1 !== BigInt(0)) { const q = r0 / r1; [r0, r1] = [r1, r0 - q * r1]; [s0, s1] = [s1, s0 - q * s1]; }
    return ((s0 % P_MOD) + P_MOD) % P_MOD; };
  const Curve = { toBigint(result) { const r = toBigint(result); return { X: r.x, Y: r.y, Z: BigInt(1), T: (r.x * r.y) % P_MOD }; } };
  const Bigint = { toAffine(P) { const zi = modInv(P.Z); return { x: (P.X * zi) % P_MOD, y: (P.Y * zi) % P_MOD }; } };
  return { params, Parallel, Field, Scalar, Affine, Projective, Curve, Bigint, close() { hip.destroyContext(ctx); } };
}

const weierstrassIds = { "bls12-377": hip.CURVE_BLS12_377_G1, "bls12-381": hip.CURVE_BLS12_381_G1, "pallas": hip.CURVE_PALLAS,
                         "bn254": hip.CURVE_BN254_G1, "grumpkin": hip.CURVE_GRUMPKIN, "vesta": hip.CURVE_VESTA };
const coordBytesOf = (params) => (params.modulus >> BigInt(256)) === BigInt(0) ? 32 : 48;   // per field, as the C ABI sizes them
const Weierstrass = {
  create(params, device) {
    if (!(params.label in weierstrassIds)) throw new Error(`curve ${params.label} has no device constants`);
    return createCurve(params, weierstrassIds[params.label], coordBytesOf(params), device);
  },
};
const TwistedEdwards = { create(params, device) { return createCurve(params, hip.CURVE_ED_ON_BLS12_377, 32, device); } };

// The ZPrize entry with the reference's own signature -- compute_msm(points, scalars) -- is exported per curve by
// js/submission-bls377.js and js/submission.js (scripts/zprize23/submission-bls377.ts:20-23, submission.ts:19-22);
// this is the shared body.  points: {x, y, isZero}[] | Buffer, scalars: bigint[] | Buffer -> {x, y}
async function compute_msm_on(curve, coordBytes, inputPoints, inputScalars) {
  const pointBytes = 2 * coordBytes;
  let sbytes, pbytes;
  if (Buffer.isBuffer(inputScalars) || inputScalars instanceof Uint8Array) sbytes = Buffer.from(inputScalars);
  else sbytes = Buffer.concat(inputScalars.map((s) => bigintToLeBytes(BigInt(s), 32)));
  const n = sbytes.length / 32;
  if (Buffer.isBuffer(inputPoints) || inputPoints instanceof Uint8Array) pbytes = Buffer.from(inputPoints);
  else pbytes = Buffer.concat(inputPoints.map((P) => (P.isZero ? Buffer.alloc(pointBytes) : Buffer.concat([bigintToLeBytes(BigInt(P.x), coordBytes), bigintToLeBytes(BigInt(P.y), coordBytes)]))));
  const pp = curve.Parallel.getPointer(pbytes.length);
  const sp = curve.Parallel.getScalarPointer(sbytes.length);
  try {   // point set and scalar buffer are freed whatever the conversion or the MSM throws (bad point, HIP error): `curve` outlives the call
    await curve.Parallel.pointsFromBytes(pp, pbytes, n);
    await curve.Parallel.scalarsFromBytes(sp, sbytes, n);
    const same = n > 1 && pbytes.slice(0, pointBytes).equals(pbytes.slice(pointBytes, 2 * pointBytes));
    const { result } = same ? await curve.Parallel.msm(sp, pp, n) : await curve.Parallel.msmUnsafe(sp, pp, n);
    return { x: result.x, y: result.y, isZero: result.isZero };
  } finally {
    pp.free();
    sp.free();
  }
}

// `startThreads(n)` / `stopThreads()` of src/parallel.ts:291-320 -- the reference's callers bracket every MSM with them
// (scripts/msm-weierstrass.ts:14,50, src/msm.test.ts:23,33).  The worker pool they manage is replaced by the GPU grid, which
// needs no start-up: both resolve at once.  `n` is accepted and ignored (it sized the pool and the memory segmentation).
async function startThreads(_n) {}
async function stopThreads() {}

module.exports = { hip, startThreads, stopThreads, Weierstrass, Weierstraß: Weierstrass /* the reference's spelling, src/parallel.ts:40 */, TwistedEdwards, bls12377Params, bls12381Params, pallasParams, bn254Params, grumpkinParams, vestaParams, edOnBls12377Params, compute_msm_on, compute_msm: compute_msm_on, leBytesToBigint, bigintToLeBytes };
