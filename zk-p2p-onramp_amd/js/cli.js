#!/usr/bin/env node
'use strict';
/*
 * CLI with snarkjs' argv shape (reference dizkus-scripts/5_gen_proof.sh:8, rapidsnark's
 * twin at 6_gen_proof_rapidsnark.sh:26):
 *   node cli.js groth16 prove <circuit.zkey> <witness.wtns> <proof.json> <public.json>
 * Output files are JSON.stringify(x, null, 1), byte-identical in layout to snarkjs.
 * and snarkjs' calldata export (reference circuit/scripts/generate_calldata.sh:3):
 *   node cli.js zkey export soliditycalldata <public.json> <proof.json>
 * and snarkjs' setup step (reference dizkus-scripts/3_gen_chunk_zkey.sh:18, `groth16 setup`):
 *   node cli.js groth16 setup|zkey new <circuit.r1cs> <pot.ptau> <circuit_0000.zkey> [-e=...]
 * a contribution and the final beacon (3_gen_chunk_zkey.sh:27,36; the record is appended to section 10):
 *   node cli.js zkey contribute <in.zkey> <out.zkey> -e=<entropy> [-n=name]
 *   node cli.js zkey beacon <in.zkey> <out.zkey> <beaconHashHex> <numIterationsExp> [-n=name]
 * and the gate of the ceremony (reference circuit/scripts/generate_keys_phase2_groth16.sh:26):
 *   node cli.js zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>
 *   node cli.js wtns check <circuit.r1cs> <witness.wtns> [-v]   (later snarkjs' command; recalled, unpinned)
 * and the last step of phase 1 (reference circuit/scripts/generate_keys_phase1.sh:20), whose output `zkey new` reads:
 *   node cli.js powersoftau prepare phase2 <pot_beacon.ptau> <pot_final.ptau> [-v]
 * and the check of a phase-1 file (reference circuit/scripts/generate_keys_phase1.sh:16; the step
 * generate_keys_phase2_groth16.sh:3 comments out as too slow):
 *   node cli.js powersoftau verify <pot.ptau> [-v]
 * and phase 1 from its start (reference circuit/scripts/generate_keys_phase1.sh:6,8,10,18):
 *   node cli.js powersoftau new bn128 <power> <out.ptau> [-v]
 *   node cli.js powersoftau contribute <in.ptau> <out.ptau> [--name=|-n=name] [-e=entropy] [-v]
 *   node cli.js powersoftau beacon <in.ptau> <out.ptau> <beaconHashHex> <numIterationsExp> [-n=name] [-v]
 * and the path of a contributor who never holds the ptau (reference circuit/scripts/generate_keys_phase1.sh:12-14):
 *   node cli.js powersoftau export challenge <in.ptau> <challenge> [-v]
 *   node cli.js powersoftau challenge contribute bn128 <challenge> <response> [-e=entropy] [-v]
 *   node cli.js powersoftau import response <old.ptau> <response> <new.ptau> [-n=|--name=name] [-v]
 * and the same path in phase 2, over an MPCParams file that the Rust phase2 tools also read:
 *   node cli.js zkey export bellman <circuit_xxxx.zkey> <circuit.mpcparams> [-v]
 *   node cli.js zkey bellman contribute bn128 <circuit.mpcparams> <circuit_response.mpcparams> [-e=entropy] [-v]
 *   node cli.js zkey import bellman <circuit_old.zkey> <circuit_response.mpcparams> <circuit_new.zkey> [-n=|--name=name] [-v]
 * and the two ends of the reference's key and proof scripts (dizkus-scripts/4_gen_vkey.sh:10, 5_gen_proof.sh:17,
 * circuit/scripts/verify_proof_groth16.sh:2):
 *   node cli.js zkey export verificationkey <circuit.zkey> [verification_key.json]
 *   node cli.js groth16 verify <verification_key.json> <public.json> <proof.json>
 */
const fs = require('fs');
const { groth16, zKey, exportSolidityCallData, newZKey, beacon, contribute, verifyFromR1cs, preparePhase2, powersOfTau, wtns: wtnsApi, release } = require('./groth16');

const USAGE = 'usage: cli.js groth16 prove <circuit.zkey> <witness.wtns> <proof.json> <public.json>\n' +
              '       cli.js groth16 verify <verification_key.json> <public.json> <proof.json>\n' +
              '       cli.js zkey export verificationkey <circuit.zkey> [verification_key.json]\n' +
              '       cli.js zkey export soliditycalldata <public.json> <proof.json>\n' +
              '       cli.js groth16 setup|zkey new <circuit.r1cs> <pot.ptau> <circuit_0000.zkey>\n' +
              '       cli.js zkey contribute <in.zkey> <out.zkey> -e=<entropy> [-n=name]\n' +
              '       cli.js zkey beacon <in.zkey> <out.zkey> <beaconHashHex> <numIterationsExp> [-n=name]\n' +
              '       cli.js zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>\n' +
              '       cli.js wtns check <circuit.r1cs> <witness.wtns> [-v]\n' +
              '       cli.js powersoftau prepare phase2 <in.ptau> <out.ptau> [-v]\n' +
              '       cli.js powersoftau verify <pot.ptau> [-v]\n' +
              '       cli.js powersoftau new bn128 <power> <out.ptau> [-v]\n' +
              '       cli.js powersoftau contribute <in.ptau> <out.ptau> [--name=|-n=name] [-e=entropy] [-v]\n' +
              '       cli.js powersoftau beacon <in.ptau> <out.ptau> <beaconHashHex> <numIterationsExp> [-n=name] [-v]\n' +
              '       cli.js powersoftau export challenge <in.ptau> <challenge> [-v]\n' +
              '       cli.js powersoftau challenge contribute bn128 <challenge> <response> [-e=entropy] [-v]\n' +
              '       cli.js powersoftau import response <old.ptau> <response> <new.ptau> [-n=|--name=name] [-v]\n' +
              '       cli.js zkey export bellman <circuit_xxxx.zkey> <circuit.mpcparams> [-v]\n' +
              '       cli.js zkey bellman contribute bn128 <circuit.mpcparams> <circuit_response.mpcparams> [-e=entropy] [-v]\n' +
              '       cli.js zkey import bellman <circuit_old.zkey> <circuit_response.mpcparams> <circuit_new.zkey> [-n=|--name=name] [-v]\n';

async function main(argv) {
  if (argv.length === 5 && argv[0] === 'zkey' && argv[1] === 'export' && argv[2] === 'soliditycalldata') {
    const pub = JSON.parse(fs.readFileSync(argv[3], 'utf-8'));
    const proof = JSON.parse(fs.readFileSync(argv[4], 'utf-8'));
    process.stdout.write(await exportSolidityCallData(proof, pub) + '\n');
    return 0;
  }
  if ((argv.length === 4 || argv.length === 5) && argv[0] === 'zkey' && argv[1] === 'export' && argv[2] === 'verificationkey') {
    const vKey = await zKey.exportVerificationKey(argv[3]);
    fs.writeFileSync(argv[4] || 'verification_key.json', JSON.stringify(vKey, null, 1), 'utf-8');
    return 0;
  }
  if (argv.length === 5 && argv[0] === 'groth16' && argv[1] === 'verify') {
    // snarkjs' log lines (recalled, unpinned): "[INFO]  snarkJS: OK!" and exit 0, else "[ERROR] snarkJS: Invalid
    // proof" and exit 1
    const logger = {
      info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`),
      error: (m) => process.stdout.write(`[ERROR] snarkJS: ${m}\n`),
    };
    const vKey = JSON.parse(fs.readFileSync(argv[2], 'utf-8'));
    const pub = JSON.parse(fs.readFileSync(argv[3], 'utf-8'));
    const proof = JSON.parse(fs.readFileSync(argv[4], 'utf-8'));
    return (await groth16.verify(vKey, pub, proof, logger)) ? 0 : 1;
  }
  const setupArgs = argv.filter((a) => !a.startsWith('-e='));  // entropy: unused by `groth16 setup`
  if (setupArgs.length === 5 && ((argv[0] === 'zkey' && argv[1] === 'new') || (argv[0] === 'groth16' && argv[1] === 'setup'))) {
    await newZKey(setupArgs[2], setupArgs[3], setupArgs[4]);
    return 0;
  }
  const named = argv.filter((a) => !/^(-n|--name)=/.test(a) && a !== '-v' && a !== '--verbose');
  if (named.length === 5 && argv[0] === 'powersoftau' && argv[1] === 'prepare' && argv[2] === 'phase2') {
    await preparePhase2(named[3], named[4]);
    return 0;
  }
  if (named.length === 3 && argv[0] === 'powersoftau' && argv[1] === 'verify') {
    // snarkjs' log lines (recalled from snarkjs 0.4.22, unpinned): "[INFO]  snarkJS: Powers Of tau file OK!" and
    // exit 0, else the reason and "[ERROR] snarkJS: Invalid ptau" and exit 1
    const logger = {
      info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`),
      error: (m) => process.stdout.write(`[ERROR] snarkJS: ${m}\n`),
    };
    return (await powersOfTau.verify(named[2], logger)) ? 0 : 1;
  }
  if (argv[0] === 'powersoftau' && ['export', 'challenge', 'import'].includes(argv[1])) {
    const verbose = argv.includes('-v') || argv.includes('--verbose');
    const logger = verbose ? { info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`) } : undefined;
    const pos = argv.filter((a) => !/^(-n|--name|-e|--entropy)=/.test(a) && a !== '-v' && a !== '--verbose');
    const opt = (re) => {
      const a = argv.find((x) => re.test(x));
      return a === undefined ? undefined : a.replace(/^[^=]*=/, '');
    };
    if (argv[1] === 'export' && pos[2] === 'challenge' && pos.length === 5) {
      await powersOfTau.exportChallenge(pos[3], pos[4], logger);
      return 0;
    }
    if (argv[1] === 'challenge' && pos[2] === 'contribute' && pos.length === 6) {
      try {
        await powersOfTau.challengeContribute(pos[3], pos[4], pos[5], opt(/^(-e|--entropy)=/), logger);
      } catch (e) {  // an unknown curve: snarkjs' error line, exit 1
        if (!/^Curve not supported/.test(e.message)) throw e;
        process.stdout.write(`[ERROR] snarkJS: Error: ${e.message}\n`);
        return 1;
      }
      return 0;
    }
    if (argv[1] === 'import' && pos[2] === 'response' && pos.length === 6) {
      await powersOfTau.importResponse(pos[3], pos[4], pos[5], opt(/^(-n|--name)=/), true, logger);
      return 0;
    }
    process.stderr.write(USAGE);
    return 1;
  }
  if (argv[0] === 'zkey' && (argv[1] === 'bellman' || (['export', 'import'].includes(argv[1]) && argv[2] === 'bellman'))) {
    const verbose = argv.includes('-v') || argv.includes('--verbose');
    const logger = verbose ? { info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`) } : undefined;
    const pos = argv.filter((a) => !/^(-n|--name|-e|--entropy)=/.test(a) && a !== '-v' && a !== '--verbose');
    const opt = (re) => {
      const a = argv.find((x) => re.test(x));
      return a === undefined ? undefined : a.replace(/^[^=]*=/, '');
    };
    if (argv[1] === 'export' && pos.length === 5) {
      await zKey.exportBellman(pos[3], pos[4], logger);
      return 0;
    }
    if (argv[1] === 'bellman' && pos[2] === 'contribute' && pos.length === 6) {
      try {
        await zKey.bellmanContribute(pos[3], pos[4], pos[5], opt(/^(-e|--entropy)=/), logger);
      } catch (e) {  // an unknown curve: snarkjs' error line, exit 1
        if (!/^Curve not supported/.test(e.message)) throw e;
        process.stdout.write(`[ERROR] snarkJS: Error: ${e.message}\n`);
        return 1;
      }
      return 0;
    }
    if (argv[1] === 'import' && pos.length === 6) {
      await zKey.importBellman(pos[3], pos[4], pos[5], opt(/^(-n|--name)=/), logger);
      return 0;
    }
    process.stderr.write(USAGE);
    return 1;
  }
  if (argv[0] === 'powersoftau' && ['new', 'contribute', 'beacon'].includes(argv[1])) {
    const verbose = argv.includes('-v') || argv.includes('--verbose');
    const logger = verbose ? { info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`) } : undefined;
    const pos = argv.filter((a) => !/^(-n|--name|-e|--entropy)=/.test(a) && a !== '-v' && a !== '--verbose');
    const opt = (re) => {
      const a = argv.find((x) => re.test(x));
      return a === undefined ? undefined : a.replace(/^[^=]*=/, '');
    };
    const name = opt(/^(-n|--name)=/);
    if (argv[1] === 'new' && pos.length === 5) {
      try {
        await powersOfTau.newAccumulator(pos[2], pos[3], pos[4], logger);
      } catch (e) {  // an unknown curve or power: snarkjs' error line, exit 1
        process.stdout.write(`[ERROR] snarkJS: Error: ${e.message}\n`);
        return 1;
      }
      return 0;
    }
    if (argv[1] === 'contribute' && pos.length === 4) {
      await powersOfTau.contribute(pos[2], pos[3], name, opt(/^(-e|--entropy)=/), logger);
      return 0;
    }
    if (argv[1] === 'beacon' && pos.length === 6) {
      await powersOfTau.beacon(pos[2], pos[3], name, pos[4], pos[5], logger);
      return 0;
    }
    process.stderr.write(USAGE);
    return 1;
  }
  if (named.length === 5 && argv[0] === 'zkey' && argv[1] === 'verify') {
    // snarkjs' log lines (recalled from snarkjs 0.4.22, unpinned): "[INFO]  snarkJS: ZKey Ok!" and exit 0,
    // else the reason and "[ERROR] snarkJS: Invalid zkey" and exit 1
    const logger = {
      info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`),
      error: (m) => process.stdout.write(`[ERROR] snarkJS: ${m}\n`),
    };
    return (await verifyFromR1cs(named[2], named[3], named[4], logger)) ? 0 : 1;
  }
  if (argv[0] === 'wtns' && argv[1] === 'check') {
    // exit 0 and "[INFO]  snarkJS: WITNESS IS CORRECT", else the verdict, "[ERROR] snarkJS: WITNESS IS NOT
    // CORRECT" and exit 1 (the log words of later snarkjs as recalled, unpinned); -v is accepted
    const pos = argv.filter((a) => !a.startsWith('-'));
    if (pos.length !== 4) {
      process.stderr.write(USAGE);
      return 1;
    }
    const logger = {
      info: (m) => process.stdout.write(`[INFO]  snarkJS: ${m}\n`),
      error: (m) => process.stdout.write(`[ERROR] snarkJS: ${m}\n`),
    };
    return (await wtnsApi.check(pos[2], pos[3], logger)) ? 0 : 1;
  }
  if (argv[0] === 'zkey' && argv[1] === 'contribute') {
    const pos = argv.filter((a) => !a.startsWith('-'));
    const ent = argv.find((a) => /^(-e|--entropy)=/.test(a));
    const nameArg = argv.find((a) => /^(-n|--name)=/.test(a));
    if (pos.length === 4 && ent) {
      await contribute(pos[2], pos[3], nameArg ? nameArg.replace(/^[^=]*=/, '') : '', ent.replace(/^[^=]*=/, ''));
      return 0;
    }
  }
  if (named.length === 6 && argv[0] === 'zkey' && argv[1] === 'beacon') {
    const nameArg = argv.find((a) => /^(-n|--name)=/.test(a));
    await beacon(named[2], named[3], nameArg ? nameArg.replace(/^[^=]*=/, '') : '', named[4], named[5]);
    return 0;
  }
  if (argv.length !== 6 || argv[0] !== 'groth16' || argv[1] !== 'prove') {
    process.stderr.write(USAGE);
    return 1;
  }
  const [, , zkey, wtns, proofOut, publicOut] = argv;
  const { proof, publicSignals } = await groth16.prove(zkey, wtns);
  fs.writeFileSync(proofOut, JSON.stringify(proof, null, 1), 'utf-8');
  fs.writeFileSync(publicOut, JSON.stringify(publicSignals, null, 1), 'utf-8');
  release();
  return 0;
}

main(process.argv.slice(2)).then((c) => process.exit(c), (e) => {
  process.stderr.write(String(e && e.stack || e) + '\n');
  process.exit(1);
});
