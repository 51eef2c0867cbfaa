'use strict';
/*
 * Drop-in for snarkjs' `groth16.prove(zkeyFileName, witnessFileName, logger)`
 * (snarkjs@0.4.22, reference package-lock.json:3884-3896; callers
 * app/src/helpers/zkp.ts:94 via fullProve, dizkus-scripts/5_gen_proof.sh:8 via the CLI).
 *
 * Same arguments (a path or a fastfile memory descriptor {type:"mem", data}), same
 * Promise<{proof, publicSignals}> result with decimal strings and snarkjs' key order,
 * same Error messages (from the C ABI).  The zkey is loaded once per process and stays
 * resident in HBM (snarkjs re-reads it on every call): a path zkey is keyed by its path, a
 * memory zkey ({type:"mem"} / Buffer, the fullProve / fastfile path) by the SHA-256 of its
 * bytes, so repeated proofs with the same in-memory key reuse the resident handle.  The hash is
 * computed once per key buffer (a WeakMap on the underlying ArrayBuffer remembers it), not on
 * every call: a GB-scale key would otherwise block the event loop for ~1 s per proof.  There is
 * no CPU fallback: if the native addon or libzkp_amd.so is missing, require() throws.
 */
const crypto = require('crypto');
const fs = require('fs');
const path = require('path');
const addon = require(path.join(__dirname, 'build', 'zkp_napi.node'));

const provers = new Map();     // zkey path -> handle
const memProvers = new Map();  // sha256(zkey bytes) -> handle, most recently used last
const MEM_PROVERS_MAX = 2;     // each holds its key's base tables in HBM (~50 GB for Venmo)
const memKeyHash = new WeakMap();  // ArrayBuffer -> [{off, len, hash}] of key buffers already hashed

function readInput(x) {
  if (x && typeof x === 'object' && x.type === 'mem') return Buffer.from(x.data.buffer ? x.data : Buffer.from(x.data));
  if (Buffer.isBuffer(x)) return x;
  return fs.readFileSync(x);
}

function sampleHash(buf) {
  const h = crypto.createHash('sha256').update(buf.subarray(0, Math.min(4096, buf.length)));
  for (let k = 0; k < 32 && buf.length > 4096; ++k) {
    const at = Math.floor((buf.length - 256) * (k + 1) / 32);
    h.update(buf.subarray(at, at + 256));
  }
  return h.digest('hex');
}

function proverFor(zkey, devices) {
  if (typeof zkey === 'string') {
    let h = provers.get(zkey);
    if (!h) {
      h = addon.loadProver(zkey, devices);
      provers.set(zkey, h);
    }
    return h;
  }
  const src = zkey && typeof zkey === 'object' && zkey.type === 'mem' ? zkey.data : zkey;
  const buf = ArrayBuffer.isView(src) ? Buffer.from(src.buffer, src.byteOffset, src.byteLength) : readInput(zkey);
  // The full SHA-256 of a key buffer is computed once per (ArrayBuffer, offset, length).  Key
  // buffers are meant to be immutable; a buffer re-filled with another key (a file re-read into
  // it, a reused fastfile mem object) is caught by a sampled fingerprint (the first 4 KiB and 32
  // evenly spaced 256-byte windows) checked on every hit: a mismatch re-hashes the whole buffer.
  let seen = ArrayBuffer.isView(src) ? memKeyHash.get(src.buffer) : undefined;
  let hit = seen && seen.find((e) => e.off === src.byteOffset && e.len === src.byteLength);
  if (hit && hit.sample !== sampleHash(buf)) {
    seen.splice(seen.indexOf(hit), 1);
    hit = undefined;
  }
  if (!hit) {
    hit = { off: buf.byteOffset, len: buf.byteLength, hash: crypto.createHash('sha256').update(buf).digest('hex'),
            sample: sampleHash(buf) };
    if (ArrayBuffer.isView(src)) {
      if (!seen) memKeyHash.set(src.buffer, (seen = []));
      seen.push(hit);
    }
  }
  const key = hit.hash + ':' + JSON.stringify(devices || []);
  let h = memProvers.get(key);
  if (h) {
    memProvers.delete(key);  // refresh its LRU position
  } else {
    h = addon.loadProver(buf, devices);
    while (memProvers.size >= MEM_PROVERS_MAX) {  // evict the least recently used key; a proof
      const [k0, h0] = memProvers.entries().next().value;  // still running on it keeps it alive
      memProvers.delete(k0);                               // until it finishes (addon refcount)
      addon.freeProver(h0);
    }
  }
  memProvers.set(key, h);
  return h;
}

function toBuf32(v) {
  if (v === undefined || v === null) return undefined;
  if (Buffer.isBuffer(v)) return v;
  let x = BigInt(v);
  const b = Buffer.alloc(32);
  for (let i = 0; i < 32; ++i) { b[i] = Number(x & 0xffn); x >>= 8n; }
  return b;
}

/**
 * @param zkeyFileName  path | {type:"mem", data}
 * @param witnessFileName path | {type:"mem", data}
 * @param logger        optional snarkjs-style logger ({debug, info})
 * @param opts          {devices?: number[], r?: bigint|string, s?: bigint|string}  (r/s: tests only)
 */
async function prove(zkeyFileName, witnessFileName, logger, opts) {
  opts = opts || {};
  const h = proverFor(zkeyFileName, opts.devices);
  const wtns = readInput(witnessFileName);
  if (logger && logger.debug) logger.debug('zkp_amd: proving on MI355X');
  return toSnarkjs(await addon.prove(h, wtns, toBuf32(opts.r), toBuf32(opts.s)));
}

function toSnarkjs(r) {
  const proof = {
    pi_a: [r.piA[0], r.piA[1], '1'],
    pi_b: [[r.piB[0][0], r.piB[0][1]], [r.piB[1][0], r.piB[1][1]], ['1', '0']],
    pi_c: [r.piC[0], r.piC[1], '1'],
    protocol: 'groth16',
    curve: 'bn128',
  };
  return { proof, publicSignals: r.publicSignals };
}

/**
 * Many onramp proofs in one call (configs[3] batch): the witnesses are spread over the
 * prover's devices (opts.devices) by the native batch scheduler, each device overlapping the
 * next witness's upload with the current proof.  Resolves to one entry per witness:
 * {proof, publicSignals}, or an Error for a witness that failed (the others still prove).
 * @param witnesses  array of path | {type:"mem", data} | Buffer
 * @param opts       {devices?: number[], rs?: (bigint|string)[], ss?: (bigint|string)[]}  (rs/ss: tests only)
 */
async function proveBatch(zkeyFileName, witnesses, logger, opts) {
  opts = opts || {};
  const h = proverFor(zkeyFileName, opts.devices);
  const bufs = witnesses.map(readInput);
  if (logger && logger.debug) logger.debug(`zkp_amd: proving a batch of ${bufs.length} on MI355X`);
  const rs = opts.rs ? opts.rs.map(toBuf32) : undefined;
  const ss = opts.ss ? opts.ss.map(toBuf32) : undefined;
  const res = await addon.proveBatch(h, bufs, rs, ss);
  return res.map((r) => (r instanceof Error ? r : toSnarkjs(r)));
}

// `snarkjs zkey export soliditycalldata` text (snarkjs 0.4.22 groth16ExportSolidityCallData,
// called at reference circuit/scripts/generate_calldata.sh:3): 64-hex-digit "0x" words,
// G2 coordinates in the EIP-197 [c1, c0] order that Verifier.sol:184-188 / :366-369 expects.
function p256(n) {
  let s = BigInt(n).toString(16);
  while (s.length < 64) s = '0' + s;
  return `"0x${s}"`;
}

async function exportSolidityCallData(proof, publicSignals) {
  const inputs = publicSignals.map(p256).join(',');
  return `[${p256(proof.pi_a[0])}, ${p256(proof.pi_a[1])}],` +
    `[[${p256(proof.pi_b[0][1])}, ${p256(proof.pi_b[0][0])}],[${p256(proof.pi_b[1][1])}, ${p256(proof.pi_b[1][0])}]],` +
    `[${p256(proof.pi_c[0])}, ${p256(proof.pi_c[1])}],` +
    `[${inputs}]`;
}

// Argument list of Ramp.onRamp(uint256[2] _a, uint256[2][2] _b, uint256[2] _c, uint256[msgLen] _signals)
// exactly as the app builds it (reference app/src/components/SubmitOrderOnRampForm.tsx:36-55:
// pi_a / pi_c without the projective "1", each pi_b pair reversed to [c1, c0]).
function onRampArgs(proof, publicSignals) {
  return [
    proof.pi_a.slice(0, 2),
    proof.pi_b.slice(0, 2).map((g2point) => g2point.slice().reverse()),
    proof.pi_c.slice(0, 2),
    publicSignals,
  ];
}

/*
 * snarkjs' `zKey.newZKey(r1csName, ptauName, zkeyName, logger)` (the `zkey new` step,
 * reference dizkus-scripts/3_gen_chunk_zkey.sh:18): the phase-2 initial key (gamma = delta = 1)
 * built on the GPU.  r1cs / ptau are paths or {type:"mem"} descriptors; with a zkeyName the key
 * is written there, and the key bytes are returned either way.
 */
async function newZKey(r1csName, ptauName, zkeyName, logger, device) {
  const out = addon.zkeyNew(readInput(r1csName), readInput(ptauName), device || 0);
  if (typeof zkeyName === 'string') fs.writeFileSync(zkeyName, out);
  else if (zkeyName && typeof zkeyName === 'object' && zkeyName.type === 'mem') zkeyName.data = out;
  if (logger && logger.info) logger.info(`zkey new: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `powersOfTau.preparePhase2(oldPtauFilename, newPTauFilename, logger)` (the `powersoftau prepare
 * phase2` step, reference circuit/scripts/generate_keys_phase1.sh:20): the Lagrange sections 12-15 that
 * `zkey new` reads, every level a group inverse FFT on the GPU.  The input is a path or a {type:"mem"}
 * descriptor; with an output name the file is written there, and its bytes are returned either way.
 */
async function preparePhase2(oldPtauName, newPtauName, logger, device) {
  const out = addon.ptauPreparePhase2(readInput(oldPtauName), device || 0);
  if (typeof newPtauName === 'string') fs.writeFileSync(newPtauName, out);
  else if (newPtauName && typeof newPtauName === 'object' && newPtauName.type === 'mem') newPtauName.data = out;
  if (logger && logger.info) logger.info(`powersoftau prepare phase2: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `zKey.beacon(zkeyNameOld, zkeyNameNew, name, beaconHashStr, numIterationsExp, logger)`
 * (reference dizkus-scripts/3_gen_chunk_zkey.sh:36): delta -> k delta, L/H -> k^-1 on the GPU, with
 * k and the contribution record (section 10: proof of knowledge, transcript, beacon parameters,
 * name) derived from the beacon as snarkjs does (oracle/mpc.py restates it; parity unpinned).
 */
async function beacon(zkeyNameOld, zkeyNameNew, name, beaconHashStr, numIterationsExp, logger, device) {
  const hex = String(beaconHashStr);
  const bytes = /^([0-9a-fA-F]{2})+$/.test(hex) ? Buffer.from(hex, 'hex') : Buffer.alloc(0);
  if (bytes.length === 0) throw new Error('Invalid Beacon Hash. (It must be a valid hexadecimal sequence)');
  const e = Number(numIterationsExp);
  if (!Number.isInteger(e) || e < 10 || e > 63) throw new Error('Invalid numIterationsExp. (Must be between 10 and 63)');
  const out = addon.zkeyBeacon(readInput(zkeyNameOld), bytes, e, device || 0, name ? String(name) : undefined);
  if (typeof zkeyNameNew === 'string') fs.writeFileSync(zkeyNameNew, out);
  else if (zkeyNameNew && typeof zkeyNameNew === 'object' && zkeyNameNew.type === 'mem') zkeyNameNew.data = out;
  if (logger && logger.info) logger.info(`zkey beacon ${name || ''}: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `zKey.contribute(zkeyNameOld, zkeyNameNew, name, entropy, logger)` (reference
 * dizkus-scripts/3_gen_chunk_zkey.sh:27, `zkey contribute -e=... -n=...`): the secret and the
 * record drawn from ChaCha20 seeded with Blake2b(64 random bytes || entropy), the group arithmetic
 * on the GPU.
 */
async function contribute(zkeyNameOld, zkeyNameNew, name, entropy, logger, device) {
  if (!entropy) throw new Error('zkey contribute: entropy is required (-e=...)');
  const out = addon.zkeyContribute(readInput(zkeyNameOld), String(entropy), name ? String(name) : undefined,
                                   device || 0);
  if (typeof zkeyNameNew === 'string') fs.writeFileSync(zkeyNameNew, out);
  else if (zkeyNameNew && typeof zkeyNameNew === 'object' && zkeyNameNew.type === 'mem') zkeyNameNew.data = out;
  if (logger && logger.info) logger.info(`zkey contribute ${name || ''}: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `zKey.verifyFromR1cs(r1csName, ptauName, zkeyName, logger)` (the `zkey verify` gate of a
 * ceremony, reference circuit/scripts/generate_keys_phase2_groth16.sh:26): the initial key is rebuilt
 * on the GPU (`zkey new`) and the key checked against it (the transcript chain on the host, the L / H
 * sections as random linear combinations on the GPU).  Resolves to a boolean as snarkjs does; the
 * failing check goes to logger.error, "ZKey Ok!" to logger.info (strings recalled from snarkjs
 * 0.4.22, unpinned).  Malformed input rejects.
 */
function reportVerdict(res, logger) {
  if (logger) {
    if (res.valid && logger.info) logger.info('ZKey Ok!');
    if (!res.valid && logger.error) {
      logger.error(res.message);
      logger.error('Invalid zkey');
    }
  }
  return res.valid;
}
async function verifyFromR1cs(r1csName, ptauName, zkeyName, logger, device) {
  return reportVerdict(addon.zkeyVerifyFromR1cs(readInput(r1csName), readInput(ptauName), readInput(zkeyName),
                                                device || 0), logger);
}
/*
 * `zKey.verifyFromInit(initName, zkeyName, logger)`: the same against an initial key at hand.  snarkjs'
 * own shape (initName, ptauName, zkeyName, logger) is accepted too; the ptau is not needed, the H
 * section is compared against the initial key's.
 */
async function verifyFromInit(initName, zkeyName, logger, device, ...rest) {
  const isInput = (x) => typeof x === 'string' || (x && typeof x === 'object' && x.type === 'mem');
  if (isInput(logger)) return verifyFromInit(initName, logger, device, ...rest);
  return reportVerdict(addon.zkeyVerify(readInput(initName), readInput(zkeyName), device || 0), logger);
}

/*
 * `wtns.check(r1csFileName, wtnsFileName, logger)` of later snarkjs versions (the `wtns check` command;
 * recalled, unpinned: the reference's snarkjs 0.4.22 has neither): every constraint of the .r1cs evaluated
 * on the witness on the GPU.  Resolves to a boolean; "WITNESS IS CORRECT" goes to logger.info, the verdict
 * ("INVALID: constraint <i> is not satisfied (<k> of <n> fail)", ...) and "WITNESS IS NOT CORRECT" to
 * logger.error (the log words as recalled from later snarkjs, unpinned).  Malformed input rejects.
 * checkDetails resolves to the whole verdict {valid, message, nBad, firstBad, bad, nConstraints}.
 */
async function wtnsCheckDetails(r1csFileName, wtnsFileName, device) {
  return addon.wtnsCheck(readInput(r1csFileName), readInput(wtnsFileName), device || 0);
}
async function wtnsCheck(r1csFileName, wtnsFileName, logger, device) {
  const res = await wtnsCheckDetails(r1csFileName, wtnsFileName, device);
  if (logger) {
    if (res.valid && logger.info) logger.info('WITNESS IS CORRECT');
    if (!res.valid && logger.error) {
      logger.error(res.message);
      logger.error('WITNESS IS NOT CORRECT');
    }
  }
  return res.valid;
}

/*
 * snarkjs' `powersOfTau.verify(tauFilename, logger)` (the `powersoftau verify` step, reference
 * circuit/scripts/generate_keys_phase1.sh:16; skipped as too slow in generate_keys_phase2_groth16.sh:3): the
 * contribution chain on the host, every point section on the GPU.  Resolves to a boolean; the failing check
 * goes to logger.error, "Powers Of tau file OK!" to logger.info (strings recalled from snarkjs 0.4.22,
 * unpinned).  Malformed input rejects.
 */
async function verifyPtau(ptauName, logger, device) {
  const res = addon.ptauVerify(readInput(ptauName), device || 0);
  if (logger) {
    if (res.valid && logger.info) logger.info('Powers Of tau file OK!');
    if (!res.valid && logger.error) {
      logger.error(res.message);
      logger.error('Invalid ptau');
    }
  }
  return res.valid;
}

/*
 * snarkjs' `powersOfTau.newAccumulator(curve, power, fileName, logger)` (the `powersoftau new bn128 <power>`
 * step, reference circuit/scripts/generate_keys_phase1.sh:6): sections 1-7, every point a generator.  Only
 * bn128 exists here; any other curve name fails as snarkjs' getCurveFromName does.
 */
async function newAccumulator(curve, power, fileName, logger) {
  const name = String(curve && curve.name ? curve.name : curve);
  if (!['BN128', 'BN254', 'ALTBN128'].includes(name.toUpperCase().replace(/[^0-9A-Z]/g, ''))) {
    throw new Error(`Curve not supported: ${name}`);
  }
  const p = Number(power);
  if (!Number.isInteger(p) || p < 1 || p > 28) throw new Error('Invalid power. (Must be between 1 and 28)');
  const out = addon.ptauNew(p, 0);
  if (typeof fileName === 'string') fs.writeFileSync(fileName, out);
  else if (fileName && typeof fileName === 'object' && fileName.type === 'mem') fileName.data = out;
  if (logger && logger.info) logger.info(`powersoftau new: power ${p}, ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `powersOfTau.contribute(oldPtauFilename, newPTauFilename, name, entropy, logger)` (the `powersoftau
 * contribute` step, reference circuit/scripts/generate_keys_phase1.sh:8,10): the key drawn from ChaCha20 seeded
 * with Blake2b(64 random bytes || entropy), every point of sections 2-5 times its own scalar on the GPU, the
 * record appended to section 7.  snarkjs asks for the entropy when none is given; here it is then empty and
 * the 64 random bytes alone seed the draw.
 */
async function contributePtau(oldPtauName, newPtauName, name, entropy, logger, device) {
  const out = addon.ptauContribute(readInput(oldPtauName), entropy == null ? '' : String(entropy),
                                   name ? String(name) : undefined, device || 0);
  if (typeof newPtauName === 'string') fs.writeFileSync(newPtauName, out);
  else if (newPtauName && typeof newPtauName === 'object' && newPtauName.type === 'mem') newPtauName.data = out;
  if (logger && logger.info) logger.info(`powersoftau contribute ${name || ''}: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `powersOfTau.beacon(oldPtauFilename, newPTauFilename, name, beaconHashStr, numIterationsExp, logger)`
 * (the `powersoftau beacon` step, reference circuit/scripts/generate_keys_phase1.sh:18).
 */
async function beaconPtau(oldPtauName, newPtauName, name, beaconHashStr, numIterationsExp, logger, device) {
  const hex = String(beaconHashStr);
  const bytes = /^([0-9a-fA-F]{2})+$/.test(hex) ? Buffer.from(hex, 'hex') : Buffer.alloc(0);
  if (bytes.length === 0) throw new Error('Invalid Beacon Hash. (It must be a valid hexadecimal sequence)');
  if (bytes.length >= 256) throw new Error('Maximum length of beacon hash is 255 bytes');
  const e = Number(numIterationsExp);
  if (!Number.isInteger(e) || e < 10 || e > 63) throw new Error('Invalid numIterationsExp. (Must be between 10 and 63)');
  const out = addon.ptauBeacon(readInput(oldPtauName), bytes, e, device || 0, name ? String(name) : undefined);
  if (typeof newPtauName === 'string') fs.writeFileSync(newPtauName, out);
  else if (newPtauName && typeof newPtauName === 'object' && newPtauName.type === 'mem') newPtauName.data = out;
  if (logger && logger.info) logger.info(`powersoftau beacon ${name || ''}: ${out.length} bytes`);
  return out;
}

function writeOutput(target, out) {
  if (typeof target === 'string') fs.writeFileSync(target, out);
  else if (target && typeof target === 'object' && target.type === 'mem') target.data = out;
}

function requireBn128(curve) {
  const name = String(curve && curve.name ? curve.name : curve);
  if (!['BN128', 'BN254', 'ALTBN128'].includes(name.toUpperCase().replace(/[^0-9A-Z]/g, ''))) {
    throw new Error(`Curve not supported: ${name}`);
  }
}

/*
 * snarkjs' `powersOfTau.exportChallenge(pTauFilename, challengeFilename, logger)` (the `powersoftau export
 * challenge` step, reference circuit/scripts/generate_keys_phase1.sh:12): the last response hash and sections
 * 2-6 uncompressed, encoded on the GPU.  A file whose sections do not hash to its last challenge throws.
 */
async function exportChallenge(ptauName, challengeName, logger, device) {
  const out = addon.ptauExportChallenge(readInput(ptauName), device || 0);
  writeOutput(challengeName, out);
  if (logger && logger.info) logger.info(`powersoftau export challenge: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `powersOfTau.challengeContribute(curve, challengeFilename, responseFileName, entropy, logger)` (the
 * `powersoftau challenge contribute bn128` step, reference circuit/scripts/generate_keys_phase1.sh:13): one
 * contribution to a challenge file on the GPU, by a party that never holds the ptau.  Only bn128 exists here.
 */
async function challengeContribute(curve, challengeName, responseName, entropy, logger, device) {
  requireBn128(curve);
  const out = addon.ptauChallengeContribute(readInput(challengeName), entropy == null ? '' : String(entropy), device || 0);
  writeOutput(responseName, out);
  if (logger && logger.info) logger.info(`powersoftau challenge contribute: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `powersOfTau.importResponse(oldPtauFilename, contributionFilename, newPTauFilename, name, importPoints,
 * logger)` (the `powersoftau import response` step, reference circuit/scripts/generate_keys_phase1.sh:14): the
 * response's points decompressed on the GPU, a record appended to section 7.  The points are always imported
 * (snarkjs' --nopoints is not offered); the contribution itself is checked by powersOfTau.verify on the result.
 */
async function importResponse(oldPtauName, responseName, newPtauName, name, importPoints, logger, device) {
  if (importPoints === false) throw new Error('importResponse: importing without the points is not supported');
  const out = addon.ptauImportResponse(readInput(oldPtauName), readInput(responseName), name ? String(name) : undefined,
                                       device || 0);
  writeOutput(newPtauName, out);
  if (logger && logger.info) logger.info(`powersoftau import response ${name || ''}: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `zKey.exportBellman(zkeyName, mpcparamsName, logger)` (the `zkey export bellman` step): the key as an
 * MPCParams file, which an outside contributor (snarkjs' `zkey bellman contribute` or the Rust phase2 tools)
 * works on without holding the key.  Section 9 goes through a forward group FFT on the GPU.
 */
async function exportBellman(zkeyName, mpcparamsName, logger, device) {
  const out = addon.zkeyExportBellman(readInput(zkeyName), device || 0);
  writeOutput(mpcparamsName, out);
  if (logger && logger.info) logger.info(`zkey export bellman: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `zKey.bellmanContribute(curve, challengeName, responseName, entropy, logger)` (the `zkey bellman
 * contribute bn128` step): one contribution to an MPCParams file on the GPU.  Only bn128 exists here.  The
 * contribution hash goes to logger.info in snarkjs' four-word rows; resolves to it, as snarkjs does.
 */
async function bellmanContribute(curve, challengeName, responseName, entropy, logger, device) {
  requireBn128(curve);
  const res = addon.zkeyBellmanContribute(readInput(challengeName), entropy == null ? '' : String(entropy), device || 0);
  writeOutput(responseName, res.response);
  if (logger && logger.info) {
    const hex = res.hash.toString('hex');
    const rows = [0, 1, 2, 3].map((r) => '\t\t' + [0, 1, 2, 3].map((c) => hex.substr(32 * r + 8 * c, 8)).join(' '));
    logger.info('Contribution Hash: \n' + rows.join('\n'));
  }
  return res.hash;
}

/*
 * snarkjs' `zKey.importBellman(zkeyNameOld, mpcparamsName, zkeyNameNew, name, logger)` (the `zkey import bellman`
 * step): the key that follows the old one by the response's contribution.  Its section 9 differs from a direct
 * contribution's by a multiple that no prover sees and `zkey verify` accepts; the contribution itself is checked
 * by zKey.verifyFromR1cs on the result, not here.
 */
async function importBellman(zkeyNameOld, mpcparamsName, zkeyNameNew, name, logger, device) {
  const out = addon.zkeyImportBellman(readInput(zkeyNameOld), readInput(mpcparamsName), name ? String(name) : undefined,
                                      device || 0);
  writeOutput(zkeyNameNew, out);
  if (logger && logger.info) logger.info(`zkey import bellman ${name || ''}: ${out.length} bytes`);
  return out;
}

/*
 * snarkjs' `zKey.exportVerificationKey(zkeyName)` (the `zkey export verificationkey` step): the verification key
 * object of a key's sections 2 and 3, vk_alphabeta_12 by the host pairing.  Host only.
 */
async function exportVerificationKey(zkeyName, logger) {
  const vKey = JSON.parse(addon.zkeyExportVkey(readInput(zkeyName)));
  if (logger && logger.info) logger.info(`zkey export verificationkey: nPublic ${vKey.nPublic}`);
  return vKey;
}

function proofBytes(proof) {
  const b = Buffer.alloc(256);
  const put = (v, at) => toBuf32(v).copy(b, at);
  put(proof.pi_a[0], 0); put(proof.pi_a[1], 32);
  put(proof.pi_b[0][0], 64); put(proof.pi_b[0][1], 96); put(proof.pi_b[1][0], 128); put(proof.pi_b[1][1], 160);
  put(proof.pi_c[0], 192); put(proof.pi_c[1], 224);
  return b;
}

/*
 * `groth16.verifyBatch(vkey, [{publicSignals, proof}], logger)`: snarkjs' verification of many proofs under one
 * verification key in one call, the per-proof Miller loops on the GPU; resolves to one boolean per proof.  A value
 * that does not fit 256 bits or a publicSignals of another length than the key's nPublic rejects, as a caller error.
 */
async function verifyBatch(vkey, items, logger, device) {
  const vKey = typeof vkey === 'string' ? JSON.parse(vkey) : vkey;
  const nPublic = vKey.nPublic;
  for (const it of items) {
    if (it.publicSignals.length !== nPublic) throw new Error('Invalid number of public signals');
  }
  const proofs = Buffer.concat(items.map((it) => proofBytes(it.proof)));
  const pubs = Buffer.concat(items.map((it) => Buffer.concat(it.publicSignals.map((s) => toBuf32(s)))));
  const verdict = addon.groth16VerifyBatch(JSON.stringify(vKey), proofs, pubs, nPublic, device || 0);
  const res = Array.from(verdict, (x) => x !== 0);
  if (logger && logger.info) logger.info(`groth16 verify: ${res.filter((x) => x).length} of ${res.length} valid`);
  return res;
}

/*
 * snarkjs' `groth16.verify(vk_verifier, publicSignals, proof, logger)`: resolves to true and logs "OK!" (info), or
 * to false and logs "Invalid proof" (error) -- the words as recalled from snarkjs, unpinned.
 */
async function verify(vkey, publicSignals, proof, logger, device) {
  const [ok] = await verifyBatch(vkey, [{ publicSignals, proof }], undefined, device);
  if (logger) {
    if (ok && logger.info) logger.info('OK!');
    if (!ok && logger.error) logger.error('Invalid proof');
  }
  return ok;
}

function release() {
  for (const h of provers.values()) addon.freeProver(h);
  for (const h of memProvers.values()) addon.freeProver(h);
  provers.clear();
  memProvers.clear();
}

module.exports = {
  groth16: { prove, proveBatch, verify, verifyBatch },
  proveBatch,
  zKey: { exportVerificationKey, exportSolidityCallData, newZKey, beacon, contribute, verifyFromR1cs, verifyFromInit, exportBellman,
          bellmanContribute, importBellman },
  powersOfTau: { newAccumulator, contribute: contributePtau, beacon: beaconPtau, preparePhase2, verify: verifyPtau,
                 exportChallenge, challengeContribute, importResponse },
  wtns: { check: wtnsCheck, checkDetails: wtnsCheckDetails },
  preparePhase2,
  verifyFromR1cs,
  verifyFromInit,
  newZKey,
  beacon,
  contribute,
  prove,
  exportSolidityCallData,
  onRampArgs,
  release,
  version: addon.version,
};
