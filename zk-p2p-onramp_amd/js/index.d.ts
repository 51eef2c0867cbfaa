// Type declarations for the zkp_amd Node host layer (no tsc in the build image; this
// documents the contract a TypeScript caller such as app/src/helpers/zkp.ts sees).
export type Input = string | { type: 'mem'; data: Uint8Array };
export interface Proof {
  pi_a: [string, string, '1'];
  pi_b: [[string, string], [string, string], ['1', '0']];
  pi_c: [string, string, '1'];
  protocol: 'groth16';
  curve: 'bn128';
}
export interface ProveOptions { devices?: number[]; r?: bigint | string; s?: bigint | string }
export interface Logger { debug?(msg: string): void; info?(msg: string): void }
export interface BatchOptions { devices?: number[]; rs?: (bigint | string)[]; ss?: (bigint | string)[] }
export declare const groth16: {
  prove(zkeyFileName: Input, witnessFileName: Input, logger?: Logger, opts?: ProveOptions):
    Promise<{ proof: Proof; publicSignals: string[] }>;
  // one entry per witness: the proof, or an Error (code = zkp_status) for a witness that failed
  proveBatch(zkeyFileName: Input, witnesses: Input[], logger?: Logger, opts?: BatchOptions):
    Promise<({ proof: Proof; publicSignals: string[] } | Error)[]>;
  /** snarkjs' `groth16.verify(vKey, publicSignals, proof, logger)` from a verification key, the Miller loop on the
   *  GPU: logs "OK!" (info) or "Invalid proof" (error).  A malformed key rejects. */
  verify(vkey: VerificationKey | string, publicSignals: string[], proof: Proof, logger?: VerifyLogger,
         device?: number): Promise<boolean>;
  /** many proofs under one key in one call: one verdict per proof */
  verifyBatch(vkey: VerificationKey | string, items: { publicSignals: string[]; proof: Proof }[], logger?: Logger,
              device?: number): Promise<boolean[]>;
};
export declare function proveBatch(zkey: Input, witnesses: Input[], logger?: Logger, opts?: BatchOptions):
  Promise<({ proof: Proof; publicSignals: string[] } | Error)[]>;
export declare function prove(zkey: Input, wtns: Input, logger?: Logger, opts?: ProveOptions):
  Promise<{ proof: Proof; publicSignals: string[] }>;
export declare const zKey: {
  /** snarkjs' `zKey.exportVerificationKey(zkeyName)` (`zkey export verificationkey`); host only */
  exportVerificationKey(zkeyName: Input, logger?: Logger): Promise<VerificationKey>;
  exportSolidityCallData(proof: Proof, publicSignals: string[]): Promise<string>;
  /** `snarkjs zkey new` on the GPU; writes zkeyName when given, returns the key bytes */
  newZKey(r1csName: Input, ptauName: Input, zkeyName?: string | { type: "mem"; data?: Uint8Array }, logger?: Logger,
          device?: number): Promise<Buffer>;
  /** `snarkjs zkey beacon`'s group arithmetic on the GPU (no transcript record appended) */
  beacon(zkeyNameOld: Input, zkeyNameNew: string | { type: "mem"; data?: Uint8Array } | undefined, name: string,
         beaconHashStr: string, numIterationsExp: number, logger?: Logger, device?: number): Promise<Buffer>;
  /** `snarkjs zkey verify <r1cs> <ptau> <zkey>`: the initial key rebuilt on the GPU, the key checked against
   *  it (L / H on the GPU); the failing check goes to logger.error.  Malformed input rejects. */
  verifyFromR1cs(r1csName: Input, ptauName: Input, zkeyName: Input, logger?: VerifyLogger, device?: number):
    Promise<boolean>;
  /** the same against the initial key `zkey new` wrote */
  verifyFromInit(initName: Input, zkeyName: Input, logger?: VerifyLogger, device?: number): Promise<boolean>;
  /** `snarkjs zkey export bellman` on the GPU (zkp_zkey_export_bellman): the key as the MPCParams file an outside
   *  contributor works on */
  exportBellman(zkeyName: Input, mpcparamsName?: string | { type: "mem"; data?: Uint8Array }, logger?: Logger,
    device?: number): Promise<Uint8Array>;
  /** `snarkjs zkey bellman contribute bn128` on the GPU (zkp_zkey_bellman_contribute): the response file is written
   *  to responseName; resolves to the 64-byte contribution hash; any curve but bn128 throws */
  bellmanContribute(curve: string | { name: string }, challengeName: Input,
    responseName?: string | { type: "mem"; data?: Uint8Array }, entropy?: string, logger?: Logger, device?: number):
    Promise<Uint8Array>;
  /** `snarkjs zkey import bellman` on the GPU (zkp_zkey_import_bellman): the key that follows zkeyNameOld by the
   *  response's contribution.  The contribution is checked by verifyFromR1cs on the result, not here */
  importBellman(zkeyNameOld: Input, mpcparamsName: Input, zkeyNameNew?: string | { type: "mem"; data?: Uint8Array },
    name?: string, logger?: Logger, device?: number): Promise<Uint8Array>;
};
export declare const powersOfTau: {
  /** `snarkjs powersoftau new bn128 <power>`: a ceremony file of generators, no contribution; any curve but
   *  bn128 throws.  Writes fileName when given, returns the file's bytes */
  newAccumulator(curve: string | { name: string }, power: number, fileName?: string | { type: "mem"; data?: Uint8Array },
    logger?: Logger): Promise<Uint8Array>;
  /** `snarkjs powersoftau contribute` on the GPU (zkp_ptau_contribute): the record appended to section 7;
   *  sections 12-15 of the input are dropped */
  contribute(oldPtauName: Input, newPtauName?: string | { type: "mem"; data?: Uint8Array }, name?: string,
    entropy?: string, logger?: Logger, device?: number): Promise<Uint8Array>;
  /** `snarkjs powersoftau beacon` on the GPU (zkp_ptau_beacon); numIterationsExp within 10..63 */
  beacon(oldPtauName: Input, newPtauName: string | { type: "mem"; data?: Uint8Array } | undefined, name: string | undefined,
    beaconHashStr: string, numIterationsExp: number, logger?: Logger, device?: number): Promise<Uint8Array>;
  /** `snarkjs powersoftau prepare phase2` on the GPU: the ptau with its Lagrange sections 12-15 (what
   *  `zkey new` reads); writes newPtauName when given, returns the file's bytes */
  preparePhase2(oldPtauName: Input, newPtauName?: string | { type: "mem"; data?: Uint8Array }, logger?: Logger,
                device?: number): Promise<Buffer>;
  /** `snarkjs powersoftau verify` (zkp_ptau_verify): the contribution chain on the host, every point section
   *  on the GPU; resolves to the verdict, the failing check goes to logger.error */
  verify(ptauName: Input, logger?: VerifyLogger, device?: number): Promise<boolean>;
  /** `snarkjs powersoftau export challenge` on the GPU (zkp_ptau_export_challenge): the challenge file a third
   *  party contributes to; throws when the sections do not hash to the file's last challenge */
  exportChallenge(ptauName: Input, challengeName?: string | { type: "mem"; data?: Uint8Array }, logger?: Logger,
    device?: number): Promise<Uint8Array>;
  /** `snarkjs powersoftau challenge contribute bn128` on the GPU (zkp_ptau_challenge_contribute): the response
   *  file; any curve but bn128 throws */
  challengeContribute(curve: string | { name: string }, challengeName: Input,
    responseName?: string | { type: "mem"; data?: Uint8Array }, entropy?: string, logger?: Logger, device?: number):
    Promise<Uint8Array>;
  /** `snarkjs powersoftau import response` on the GPU (zkp_ptau_import_response): the response's points
   *  decompressed and a record appended; importPoints === false is not supported.  The contribution is checked
   *  by verify on the result, not here */
  importResponse(oldPtauName: Input, responseName: Input, newPtauName?: string | { type: "mem"; data?: Uint8Array },
    name?: string, importPoints?: boolean, logger?: Logger, device?: number): Promise<Uint8Array>;
};
export declare function preparePhase2(oldPtauName: Input, newPtauName?: string | { type: "mem"; data?: Uint8Array },
                                      logger?: Logger, device?: number): Promise<Buffer>;
export interface VerifyLogger extends Logger { error?(msg: string): void }
/** The verdict of `wtns check`: bad holds the lowest min(16, nBad) failing constraints in ascending order. */
export interface WitnessCheck {
  valid: boolean;
  message: string;
  nBad: number;
  firstBad: number;
  bad: number[];
  nConstraints: number;
}
export declare const wtns: {
  /** Later snarkjs' `wtns check <circuit.r1cs> <witness.wtns>` (recalled, unpinned): every constraint of the
   *  circuit on the witness, on the GPU.  Logs "WITNESS IS CORRECT" (info) or the verdict and "WITNESS IS NOT
   *  CORRECT" (error); malformed input rejects. */
  check(r1csFileName: Input, wtnsFileName: Input, logger?: VerifyLogger, device?: number): Promise<boolean>;
  checkDetails(r1csFileName: Input, wtnsFileName: Input, device?: number): Promise<WitnessCheck>;
};
export declare function verifyFromR1cs(r1csName: Input, ptauName: Input, zkeyName: Input, logger?: VerifyLogger,
                                       device?: number): Promise<boolean>;
export declare function verifyFromInit(initName: Input, zkeyName: Input, logger?: VerifyLogger, device?: number):
  Promise<boolean>;
export declare function exportSolidityCallData(proof: Proof, publicSignals: string[]): Promise<string>;
export declare function onRampArgs(proof: Proof, publicSignals: string[]):
  [[string, string], [[string, string], [string, string]], [string, string], string[]];
/** snarkjs' verification_key.json object (`zkey export verificationkey`). */
export interface VerificationKey {
  protocol: "groth16";
  curve: "bn128";
  nPublic: number;
  vk_alpha_1: string[];
  vk_beta_2: string[][];
  vk_gamma_2: string[][];
  vk_delta_2: string[][];
  vk_alphabeta_12?: string[][][];
  IC: string[][];
}
export declare function release(): void;
export declare function version(): string;
