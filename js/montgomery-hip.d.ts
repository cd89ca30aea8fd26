// Type declarations of js/montgomery-hip.js in the vocabulary of the reference's TypeScript sources
// (src/parallel.ts:135-160, 251-289; scripts/zprize23/submission-bls377.ts:20-23).
export type CurveParams = { label: string; modulus: bigint; order: bigint };

/** one resident point set of the context (its own allocation, like every pointer of the reference) */
export type PointPtr = { size: number; n: number; set: number; free(): void };
/** one device buffer of the context from scalarsFromBytes / randomScalars on (the reference's scalars live in wasm memory);
 * free() returns it at once, a dropped pointer returns it when collected */
export type ScalarPtr = { size: number; n: number; dev: unknown | null; free(): void; toBytes?: () => Buffer };

/** canonical affine result: what `Affine.toBigint(Projective.toAffine(result))` yields in the reference */
export type AffineResult = { x: bigint; y: bigint; isZero: boolean };
export type MsmOptions = { c?: number; useSafeAdditions?: boolean; noGlv?: boolean };
export type NarrowScalars = Uint8Array | Uint16Array | Uint32Array | BigUint64Array | Int8Array | Int16Array | Int32Array | BigInt64Array;
/** bits: magnitude bits, values in [0, 2^bits) or, signed, [-2^bits, 2^bits) (default: all the width gives); width / signed:
 * for raw bytes (a Buffer): 1, 2, 4, 8, 16 bytes per scalar, or 32 for field elements holding small values (then bits is required) */
export type NarrowOptions = { c?: number; bits?: number; width?: 1 | 2 | 4 | 8 | 16 | 32; signed?: boolean };
/** log: the reference's shape (src/msm-common.ts:176-214) -- [{n, K, c}], then ["label... x.xms"] per phase, "msm total" last */
export type MsmOutput = { result: AffineResult; log: unknown[][] };

/** a sparse matrix in CSR on the host: rowPtr holds rows + 1 entries, col the column indices, val 32 bytes per entry or null (all ones) */
export interface CsrMatrix {
  rows: number;
  cols: number;
  rowPtr: Uint32Array | number[];
  col: Uint32Array | number[];
  val: Uint8Array | null;
}

export interface Parallel {
  getPointer(size: number): PointPtr;
  getScalarPointer(size: number): ScalarPtr;
  /** src/parallel.ts:97-116 (Weierstrass: x || y, packed field size each) / :215-229 (twisted Edwards) */
  /** options.compressed: the curve's compressed encoding; options.validate: "curve" | "subgroup" (default: none) */
  pointsFromBytes(pointPtr: PointPtr, input: Uint8Array, n: number,
                  options?: { compressed?: boolean; validate?: "none" | "curve" | "subgroup" }): Promise<void>;
  /** src/parallel.ts:119-133: n x 32 bytes little-endian */
  scalarsFromBytes(scalarPtr: ScalarPtr, input: Uint8Array, n: number): Promise<void>;
  /** src/curve-random.ts:14-92, generated on the GPU (explicit seed; the reference is unseeded) */
  randomPointsFast(n: number, options?: { seed?: number }): Promise<PointPtr>;
  /** src/curve-random.ts:151-194 */
  randomScalars(n: number, options?: { seed?: number }): Promise<ScalarPtr>;
  /** src/msm-batched-affine.ts:69-340 */
  msm(scalarPtr: ScalarPtr, pointPtr: PointPtr, N: number, verboseTiming?: boolean, options?: MsmOptions): Promise<MsmOutput>;
  /** many MSMs over one point set in one call (msm_run_batch): [b].result equals (await msm(scalarPtrs[b], pointPtr, N)).result */
  msmBatch(scalarPtrs: ScalarPtr[], pointPtr: PointPtr, N: number, verboseTiming?: boolean, options?: MsmOptions): Promise<MsmOutput[]>;
  /** narrow scalars (msm_run_narrow; no counterpart in the reference): width and signedness from the typed array, or a Buffer
   * with options.width; result equals msm over the same values as 32-byte scalars; a value outside the declared range throws */
  msmNarrow(scalars: NarrowScalars, pointPtr: PointPtr, N: number, options?: NarrowOptions): Promise<MsmOutput>;
  /** many narrow MSMs over one point set (msm_run_batch_narrow): one array per element, all of one type */
  msmBatchNarrow(scalarArrays: NarrowScalars[], pointPtr: PointPtr, N: number, options?: NarrowOptions): Promise<MsmOutput[]>;
  /** indexed (sparse) MSM (msm_run_indexed): sum_j scalars[j] * P[indices[j]]; scalars m x 32 bytes, indices in any order, repeats
   *  allowed; equals msm over the dense equivalent.  An index >= the number of points throws (msm error 1, the position in the message) */
  msmIndexed(scalars: Uint8Array, indices: Uint32Array | number[], pointPtr: PointPtr, options?: { c?: number; noGlv?: boolean }): Promise<MsmOutput>;
  /** the same over narrow scalars (msm_run_indexed_narrow): scalars and options as for msmNarrow */
  msmIndexedNarrow(scalars: NarrowScalars, indices: Uint32Array | number[], pointPtr: PointPtr, options?: NarrowOptions): Promise<MsmOutput>;
  /** point-set linear combinations (msm_points_lincomb): dst[i] = a * A[aLo + i] + b * B[bLo + i], i < count; a, b below the group
   *  order (BigInt, number or 32 little-endian bytes), b and ptrB null for one term; dstPtr may be a source.  Returns dstPtr */
  pointsLincomb(dstPtr: PointPtr, a: bigint | number | Uint8Array, ptrA: PointPtr, b?: bigint | number | Uint8Array | null, ptrB?: PointPtr | null,
                options?: { aLo?: number; bLo?: number; count?: number }): PointPtr;
  /** points behind a pointer, as the library counts them (msm_pointset_size) */
  pointsetSize(pointPtr: PointPtr): number;
  /** in-place fold: P[i] <- a * P[i] + b * P[i + n/2], i < n/2 (n even); the pointer then holds n/2 points */
  foldPoints(pointPtr: PointPtr, a: bigint | number | Uint8Array, b: bigint | number | Uint8Array): PointPtr;
  /** per-row scalar multiplication (msm_points_mul): dst[i] = s[i] * A[aLo + i], i < count, every row under its own scalar; scalars: a
   *  scalar pointer (they stay on the device) or count x 32 little-endian bytes, values at or above the group order are reduced;
   *  dstPtr may be ptrA with aLo = 0 or aLo >= count.  Returns dstPtr */
  pointsMul(dstPtr: PointPtr, scalars: ScalarPtr | Uint8Array, ptrA: PointPtr, options?: { aLo?: number; sLo?: number; count?: number }): PointPtr;
  /** the same for one base point (msm_points_mul_base): dst[i] = s[i] * base; base: {x, y}, x || y as wire bytes, or null for the
   *  curve's generator.  Returns dstPtr */
  pointsMulBase(dstPtr: PointPtr, scalars: ScalarPtr | Uint8Array, base?: { x: bigint; y: bigint } | Uint8Array | null,
                options?: { sLo?: number; count?: number }): PointPtr;
  /** the transform over points (msm_points_ntt): dst = the transform of the n = 2^log2n points [aLo, aLo + n) behind ptrA, natural
   *  order; forward: dst[k] = sum_j (shift omega^k)^j A[j]; inverse: the exact inverse map (without a shift a monomial key becomes the
   *  Lagrange key of <omega>); omega: default scalarsRootOfUnity(log2n), shift: default 1; dstPtr may be ptrA with aLo = 0 or
   *  aLo >= n.  Returns dstPtr */
  pointsNtt(dstPtr: PointPtr, ptrA: PointPtr, log2n: number,
            options?: { aLo?: number; inverse?: boolean; omega?: bigint | number | Uint8Array | null; shift?: bigint | number | Uint8Array | null }): PointPtr;
  /** resident scalar vectors (msm_scalars_lincomb): dst[i] = x * A[aLo + i] + y * B[bLo + i] mod the group order, i < count, over
   *  scalars that stay on the device; x, y below the group order, y and ptrB null for one term; dstPtr may be a source.  Returns dstPtr */
  scalarsLincomb(dstPtr: ScalarPtr, x: bigint | number | Uint8Array, ptrA: ScalarPtr, y?: bigint | number | Uint8Array | null, ptrB?: ScalarPtr | null,
                 options?: { aLo?: number; bLo?: number; dstLo?: number; count?: number }): ScalarPtr;
  /** dst[i] = A[i] * B[i] mod the group order, i < N (msm_scalars_mul) */
  scalarsMul(dstPtr: ScalarPtr, ptrA: ScalarPtr, ptrB: ScalarPtr, N: number): ScalarPtr;
  /** sum_i A[aLo + i] * B[bLo + i] mod the group order, i < N (msm_scalars_inner) */
  scalarsInner(ptrA: ScalarPtr, ptrB: ScalarPtr, N: number, options?: { aLo?: number; bLo?: number }): bigint;
  /** a new scalar pointer holding s * x^i, i < N (msm_scalars_powers); s: default 1 */
  scalarsPowers(x: bigint | number | Uint8Array, N: number, s?: bigint | number | Uint8Array): ScalarPtr;
  /** dstPtr = the NTT of `batch` vectors of 2^log2n scalars at the start of ptr, natural order in and out (msm_scalars_ntt);
   *  forward: dst[k] = sum_j a[j] (shift omega^k)^j, inverse: the exact inverse map; dstPtr may be ptr */
  scalarsNtt(dstPtr: ScalarPtr, ptr: ScalarPtr, log2n: number, options?: { inverse?: boolean; omega?: bigint | number | Uint8Array;
    shift?: bigint | number | Uint8Array; batch?: number }): ScalarPtr;
  /** the library's primitive 2^log2n-th root of unity mod the group order (msm_scalars_root_of_unity) */
  scalarsRootOfUnity(log2n: number): bigint;
  /** dstPtr = the running sum or product mod the group order of the first N scalars of ptr (msm_scalars_scan); returns the total.
   *  inclusive: dst[i] = init o a[0] o ... o a[i], exclusive: dst[i] = init o a[0] o ... o a[i-1]; dstPtr may be ptr */
  scalarsScan(dstPtr: ScalarPtr, ptr: ScalarPtr, N: number, options?: { op?: "sum" | "product"; exclusive?: boolean;
    init?: bigint | number | Uint8Array }): bigint;
  /** dstPtr[i] = ptr[i]^-1 mod the group order, 0 where the residue is 0; returns how many of those there were (msm_scalars_inverse) */
  scalarsInverse(dstPtr: ScalarPtr, ptr: ScalarPtr, N: number): number;
  /** dstPtr = the quotient of the polynomial with the N coefficients of ptr by X - z, dstPtr[N-1] = 0; returns the remainder, its
   *  value at z (msm_scalars_div_linear); dstPtr may be ptr */
  scalarsDivLinear(dstPtr: ScalarPtr, ptr: ScalarPtr, N: number, z: bigint | number | Uint8Array): bigint;
  /** the round polynomial s(0), .., s(d) of a sumcheck over the multilinear tables of 2^log2n scalars behind ptrs
   *  (msm_scalars_sumcheck_round): variable j is bit j of the index; "prod": the product of 1 .. 4 tables, d = their number;
   *  "r1cs": f0 (f1 f2 - f3), d = 3.  s(0) + s(1) is the claim.  A sum of products: one call per product, s is linear in g */
  scalarsSumcheckRound(ptrs: ScalarPtr[], log2n: number, variable: number, options?: { shape?: "prod" | "r1cs" }): bigint[];
  /** binds `variable` of up to 8 tables to r: dst[i] = lo(i) + r (hi(i) - lo(i)) (msm_scalars_bind).  Without options.dst the top
   *  variable is bound in place and every pointer then holds 2^(log2n - 1) scalars; returns the pointers that hold the result */
  scalarsBind(ptrs: ScalarPtr[], log2n: number, variable: number, r: bigint | number | Uint8Array,
    options?: { dst?: ScalarPtr[] }): ScalarPtr[];
  /** a new scalar pointer holding eq(r, .) scaled by s (default 1), 2^r.length scalars: element i = s prod_j (bit_j(i) ? r[j] : 1 - r[j])
   *  (msm_scalars_eq) */
  scalarsEq(r: Array<bigint | number | Uint8Array>, s?: bigint | number | Uint8Array): ScalarPtr;
  /** (row, col, value) triples -> CSR by a stable sort over the rows, duplicates kept; triples without a value: the all-ones form
   *  (val null); transpose: the CSR of the transposed matrix */
  matrixFromTriplets(rows: number, cols: number, triplets: Array<[number, number, (bigint | number | Uint8Array)?]>,
    transpose?: boolean): CsrMatrix;
  /** a resident sparse matrix (msm_matrix_create); returns its id.  options.transpose: the id names the transposed matrix */
  matrixCreate(matrix: CsrMatrix, options?: { transpose?: boolean; testGeometry?: [number, number] }): number;
  /** debug surface: [shortMax, partLen, long rows, parts, launches] of the last scalarsMatvec */
  testLastMatvec(): number[];
  matrixDestroy(id: number): void;
  /** sizes of the matrix as held and the device bytes it takes (msm_matrix_info) */
  matrixInfo(id: number): { rows: number; cols: number; nnz: number; bytes: number };
  /** dstPtr = alpha M xPtr (+ dstPtr with accumulate) mod the group order (msm_scalars_matvec); dstPtr and xPtr are different
   *  pointers */
  scalarsMatvec(id: number, dstPtr: ScalarPtr, xPtr: ScalarPtr,
    options?: { alpha?: bigint | number | Uint8Array; accumulate?: boolean }): ScalarPtr;
  /** in-place fold: v[i] <- a * v[i] + b * v[i + n/2], i < n/2 (n even); the pointer then holds n/2 scalars */
  foldScalars(scalarPtr: ScalarPtr, a: bigint | number | Uint8Array, b: bigint | number | Uint8Array): ScalarPtr;
  /** the first N scalars behind a pointer (default: all) as N x 32 bytes on the host (msm_device_download) */
  scalarsToBytes(scalarPtr: ScalarPtr, N?: number): Buffer;
  /** smallest `bits` msmNarrow(width 32) accepts these n x 32-byte scalars under (0: all zero; 255: more than 128 bits needed) */
  scalarBits(scalars32: Uint8Array): { unsigned: number; signed: number };
  /** src/msm-batched-affine.ts:587-598: msm with useSafeAdditions = false (msm_opts.unsafe) */
  msmUnsafe(scalarPtr: ScalarPtr, pointPtr: PointPtr, N: number, verboseTiming?: boolean, options?: MsmOptions): Promise<MsmOutput>;
  /** src/parallel.ts:69-87: window structure of msmBasic, no endomorphism split */
  msmProjective(scalarPtr: ScalarPtr, pointPtr: PointPtr, N: number, options?: MsmOptions): Promise<MsmOutput>;
}

/** opaque stand-in for a wasm pointer of the reference (`Field.getPointer(size)`) */
export type ValuePtr = { size: number; value: AffineResult | null };
/** The fine operator table of the reference's wasm exports (src/field-msm.ts:86-123, 190-243) over Buffers of n field elements
 * (sizeInBytes each, little-endian, Montgomery form) instead of pointers into wasm memory: one kernel launch per call. */
export interface FieldOps {
  getPointer(size: number): ValuePtr;
  getPointers(n: number, size: number): ValuePtr[];
  sizeInBytes: number;
  multiply(a: Buffer, b: Buffer): Buffer;
  square(a: Buffer): Buffer;
  add(a: Buffer, b: Buffer): Buffer;
  subtract(a: Buffer, b: Buffer): Buffer;
  inverse(a: Buffer): Buffer;
  /** src/wasm/inverse.ts:220-271: Montgomery's trick, perLane elements per inversion */
  batchInverse(xs: Buffer, perLane?: number): Buffer;
  toMontgomery(a: Buffer): Buffer;
  fromMontgomery(a: Buffer): Buffer;
  fromBigints(vals: bigint[]): Buffer;
  toBigints(buf: Buffer): bigint[];
}
export interface Curve {
  params: CurveParams;
  Parallel: Parallel;
  /** the reference's way from `result` to bigints (scripts/msm-weierstrass.ts:89-91); values are already affine here */
  Field: FieldOps;
  /** src/scalar-glv.ts:105-128: s = (-1)^neg0 s0 + (-1)^neg1 s1 lambda mod q (Weierstrass curves with an endomorphism) */
  Scalar: { decompose(scalars: bigint[] | Buffer): { s0: bigint; s1: bigint; neg0: boolean; neg1: boolean }[] };
  Affine: {
    size: number;
    toBigint(ptr: ValuePtr | AffineResult): AffineResult;
    /** batchAddNew, src/curve-affine.ts:376-522: n pairs (null = identity) -> n sums through one launch of the tree kernel */
    batchAdd(G: ({ x: bigint; y: bigint } | null)[], H: ({ x: bigint; y: bigint } | null)[]): ({ x: bigint; y: bigint } | null)[];
  };
  Projective: { size: number; toAffine(scratch: unknown, affinePtr: ValuePtr, result: AffineResult): void };
  /** twisted Edwards call sites (scripts/msm-twisted-edwards.ts:87, scripts/zprize23/submission.ts:33-34) */
  Curve: { toBigint(result: AffineResult | ValuePtr): { X: bigint; Y: bigint; Z: bigint; T: bigint } };
  Bigint: { toAffine(P: { X: bigint; Y: bigint; Z: bigint }): { x: bigint; y: bigint } };
  close(): void;
}

/** device: a GPU index, or a list of indices: one curve object over several GPUs of the node (windows sharded inside the library) */
export const Weierstrass: { create(params: CurveParams, device?: number | number[]): Curve };
export const TwistedEdwards: { create(params: CurveParams, device?: number | number[]): Curve };
/** the reference's spelling (src/parallel.ts:40) */
export const Weierstraß: typeof Weierstrass;
export const bls12377Params: CurveParams;
export const bls12381Params: CurveParams;
export const pallasParams: CurveParams;
/** BN254 G1 (alt_bn128), Grumpkin and Vesta: 32-byte coordinates, like Pallas */
export const bn254Params: CurveParams;
export const grumpkinParams: CurveParams;
export const vestaParams: CurveParams;
export const edOnBls12377Params: CurveParams;

/** shared body of the per-curve entries js/submission-bls377.js and js/submission.js, which export the reference's exact
 * `compute_msm(inputPoints, inputScalars)` (scripts/zprize23/submission-bls377.ts:20-65, submission.ts:19-60) */
export function compute_msm_on(
  curve: Curve,
  coordBytes: number,
  inputPoints: { x: bigint; y: bigint; isZero?: boolean }[] | Uint8Array,
  inputScalars: bigint[] | Uint8Array
): Promise<{ x: bigint; y: bigint }>;
export function compute_msm(
  curve: Curve,
  coordBytes: number,
  inputPoints: { x: bigint; y: bigint; isZero?: boolean }[] | Uint8Array,
  inputScalars: bigint[] | Uint8Array
): Promise<{ x: bigint; y: bigint }>;
/** src/parallel.ts:291-320: no-ops here (the GPU grid is the worker pool); kept so that the reference's call sites run unchanged */
export function startThreads(n?: number): Promise<void>;
export function stopThreads(): Promise<void>;
export function leBytesToBigint(buf: Uint8Array): bigint;
export function bigintToLeBytes(x: bigint, n: number): Buffer;
