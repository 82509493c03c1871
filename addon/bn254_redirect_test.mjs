// bn254 G1 through the REDIRECT: the reference's own `bn254.G1.Point` (src/bn254.ts) registered with the shim as gpu.CURVE.BN254_G1
// and installed as the MSM backend of the reference's `pippenger` export (js_hooked/ of oracle/_ref/refjs.bundle, INTEGRATION.md).
//   - argument errors: the same class and message with the backend installed as from the reference's own loop;
//   - random sets above minPoints with ZERO, -P and points whose Z != 1: pippenger through the backend equals the reference's loop
//     (backend uninstalled), and gpu.STATS shows the GPU path was taken;
//   - gpu.multiplyUnsafeBatch against the reference's multiplyUnsafe, point by point.
//   node addon/bn254_redirect_test.mjs <unpacked js_hooked dir>
// TEST INFRASTRUCTURE (run by tests/test_gpu_bn254_node.py).
import assert from 'assert';
import path from 'path';
import { createRequire } from 'module';
import { pathToFileURL } from 'url';

const require = createRequire(import.meta.url);
const gpu = require('./noble_gpu.js');
const dir = path.resolve(process.argv[2] || '');
const load = (f) => import(pathToFileURL(path.join(dir, f)).href);

function rng(seed) {          // xorshift64: deterministic BigInt scalars
  let s = BigInt(seed);
  return () => {
    s ^= (s << 13n) & 0xFFFFFFFFFFFFFFFFn; s ^= s >> 7n; s ^= (s << 17n) & 0xFFFFFFFFFFFFFFFFn;
    return s;
  };
}
function errOf(f) {
  try { f(); } catch (e) { return [e.constructor.name, e.message]; }
  return null;
}

async function main() {
  await load('polyfill.mjs');
  const curveMod = await load('src/abstract/curve.mjs');
  const { pippenger } = curveMod;
  const { bn254 } = await load('src/bn254.mjs');
  const P = bn254.G1.Point;
  const r = P.Fn.ORDER;
  gpu.register(P, gpu.CURVE.BN254_G1);
  const next = rng(0x254);
  const rnd = () => ((next() << 192n) ^ (next() << 128n) ^ (next() << 64n) ^ next()) % r;

  // argument errors: the reference's, by class and message, whether or not the backend is installed
  const bad = [
    () => pippenger(P, [P.BASE], [r]),
    () => pippenger(P, [P.BASE, 5], [1n, 2n]),
    () => pippenger(P, [P.BASE], [1n, 2n]),
    () => pippenger(P, [P.BASE], [-1n]),
  ];
  const refErr = bad.map(errOf);
  gpu.install(curveMod, [P], { minPoints: 1 });
  const gpuErr = bad.map(errOf);
  assert.deepStrictEqual(gpuErr, refErr);
  refErr.forEach((e) => assert.ok(e !== null));
  assert.deepStrictEqual(errOf(() => gpu.pippenger(P, [P.BASE], [r])), refErr[0]);
  assert.strictEqual(pippenger(P, [], []), P.ZERO);
  gpu.init(0);                                             // the checks above run before the device is touched

  const minPoints = 64;
  for (const n of [65, 200, 700]) {
    const pts = [];
    for (let i = 0; i < n; i++) {
      const k = rnd() || 1n;
      let q = P.BASE.multiply(k);
      if (i % 5 === 1) q = q.add(P.BASE);                  // projective, Z != 1
      if (i % 7 === 3) q = pts[i - 1].negate();            // -P beside P
      if (i % 11 === 4) q = P.ZERO;
      pts.push(q);
    }
    const ks = pts.map((_, i) => (i % 13 === 0 ? 0n : i % 17 === 0 ? r - 1n : rnd()));
    gpu.install(curveMod, [P], { minPoints });
    const before = gpu.STATS.msmRedirected;
    const got = pippenger(P, pts, ks);
    assert.strictEqual(gpu.STATS.msmRedirected, before + 1, 'the call took the GPU path');
    gpu.uninstall(curveMod, [P]);
    const want = pippenger(P, pts, ks);
    assert.strictEqual(gpu.STATS.msmRedirected, before + 1, 'uninstalled: the reference loop');
    assert.ok(got.equals(want), 'pippenger n=' + n);
    if (n === 65) {
      const mul = gpu.multiplyUnsafeBatch(P, pts, ks);
      pts.forEach((p, i) => assert.ok(mul[i].equals(p.multiplyUnsafe(ks[i])), 'multiplyUnsafeBatch ' + i));
    }
  }
  console.log('bn254 redirect OK', JSON.stringify(gpu.STATS));
}

main().catch((e) => { console.error(e); process.exit(1); });
