/*
 * zkp_amd.h — C ABI of libzkp_amd.so, the MI355X-native Groth16 prover that is a
 * drop-in for the snarkjs `groth16.prove(zkey, wtns)` hot path of ZKP2P.
 *
 * Reference interface replaced (paths relative to the reference repo):
 *   - CLI  `snarkjs groth16 prove <zkey> <wtns> <proof.json> <public.json>`
 *          dizkus-scripts/5_gen_proof.sh:8, circuit/scripts/generate_proof_groth16.sh:11,
 *          and its rapidsnark twin dizkus-scripts/6_gen_proof_rapidsnark.sh:26,
 *          circuit/server-scripts/generate_proof.sh:5
 *   - JS   `snarkjs.groth16.fullProve(input, wasm, zkey)` -> groth16.prove(zkey, wtns)
 *          app/src/helpers/zkp.ts:94  (snarkjs@0.4.22, package-lock.json:3884-3896)
 * The N-API addon (zk-p2p-onramp_amd/js/) binds exactly these entry points; see
 * INTEGRATION.md for the binding a maintainer adds on the reference side.
 *
 * Conventions: plain pointers and sizes, no exceptions across the ABI, status codes
 * plus a thread-local message (zkp_last_error).  All field values cross the ABI as
 * 32-byte little-endian integers in STANDARD (non-Montgomery) form, exactly the
 * bytes snarkjs writes as decimal strings in proof.json / public.json.
 */
#ifndef ZKP_AMD_H
#define ZKP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum zkp_status {
  ZKP_OK = 0,
  ZKP_ERR_INVALID_ARG = 1,     /* null pointer / bad size                                   */
  ZKP_ERR_IO = 2,              /* file open/read/write failure                              */
  ZKP_ERR_FORMAT = 3,          /* bad magic, version or section layout (binfileutils)      */
  ZKP_ERR_PROTOCOL = 4,        /* zkey is not groth16   (snarkjs: "zkey file is not groth16") */
  ZKP_ERR_CURVE = 5,           /* field mismatch        (snarkjs: "Curve of the witness does not match the curve of the proving key") */
  ZKP_ERR_WITNESS_LENGTH = 6,  /* nWitness != nVars     (snarkjs: "Invalid witness length") */
  ZKP_ERR_DEVICE = 7,          /* HIP runtime error / no usable MI355X                     */
  ZKP_ERR_OUT_OF_MEMORY = 8,
  ZKP_ERR_INTERNAL = 9
} zkp_status;

/* Opaque prover handle: parsed + validated zkey whose point sections are resident in
 * HBM of every device in the list (uploaded once at load).  Immutable after load;
 * concurrent zkp_prove calls on one handle are safe.  Each device holds k proving
 * pipelines (environment ZKP_INFLIGHT = k, 1..4, default 1) that share one copy of its
 * base tables: up to k proofs run concurrently per device, each pipeline one at a time,
 * and each pipeline has two witness upload slots (a witness H2D overlaps the proof in
 * flight).  zkp_prove round-robins over the healthy pipelines; zkp_prove_batch runs two
 * workers per pipeline. */
typedef struct zkp_prover zkp_prover;

/* One Groth16 proof: affine coordinates, standard-form LE (the pi_a/pi_b/pi_c of
 * proof.json without the projective "1"/["1","0"] tails).  public_signals is a
 * caller-owned buffer of public_capacity * 32 bytes receiving w[1..nPublic]. */
typedef struct zkp_proof {
  uint8_t pi_a[2][32];    /* x, y                              */
  uint8_t pi_b[2][2][32]; /* [x.c0, x.c1], [y.c0, y.c1]        */
  uint8_t pi_c[2][32];    /* x, y                              */
  uint32_t n_public;      /* set by zkp_prove                  */
  uint32_t public_capacity;
  uint8_t* public_signals;
} zkp_proof;

/* MSM partial sums of one point range of one proof (the point-range split of a single
 * proof over several GPUs).  Affine standard-form LE, all-zero =
 * infinity.  392 bytes, no padding: ranks exchange these by an RCCL all-gather. */
typedef struct zkp_partial {
  uint8_t a[64], b1[64], c[64], h[64]; /* G1: sum over the slice of w_i A_i, w_i B1_i, w_i C_i, P_j H_j */
  uint8_t b2[128];                     /* G2: sum over the slice of w_i B2_i                          */
  uint32_t part, nparts;
} zkp_partial;

/* Load a .zkey (snarkjs groth16, version 1) from a path or a memory buffer.
 * devices: HIP device ordinals (NULL/0 -> device 0).  Every device gets a full
 * resident copy (batch mode: proofs are spread over devices by zkp_prove_batch). */
zkp_status zkp_prover_load_file(const char* zkey_path, const int* devices, int ndev, zkp_prover** out);
zkp_status zkp_prover_load_mem(const uint8_t* zkey, size_t len, const int* devices, int ndev, zkp_prover** out);

/* Chunked / compressed proving keys (the app's circuit.zkey{b..k}.gz: reference
 * app/src/helpers/zkp.ts:11-13,51-68).  zkp_prover_load_file and zkp_zkey_read accept a
 * path that exists (gzip detected by magic), else path.gz, else the chunks
 * path{a..z}[.gz] in suffix order.  Chunks are either a byte split of one binfile or
 * per-chunk "zkey" binfiles holding disjoint sections (told apart by content). */
zkp_status zkp_prover_load_chunks(const char* const* paths, int n, const int* devices, int ndev, zkp_prover** out);
/* Host only: the merged, decompressed zkey bytes (free with zkp_buffer_free). */
zkp_status zkp_zkey_read(const char* path, uint8_t** out, size_t* len);
zkp_status zkp_zkey_read_chunks(const char* const* paths, int n, uint8_t** out, size_t* len);
void zkp_buffer_free(uint8_t* p);

/* Setup acceleration, primitive: the group arithmetic of a phase-2 contribution with a given
 * secret k (32-byte LE, nonzero mod r) on `device`: delta1, delta2 x k (section 2), every
 * L (section 8) and H (section 9) point x k^-1.  Section 10 (the contribution record) is
 * copied unchanged, so the result does not pass `zkey verify`: the snarkjs commands are
 * zkp_zkey_contribute_entropy / zkp_zkey_beacon.  *out: the new zkey (zkp_buffer_free). */
zkp_status zkp_zkey_contribute(int device, const uint8_t* zkey, size_t len, const uint8_t* k32, uint8_t** out,
                               size_t* out_len);

/* Setup acceleration: `snarkjs zkey beacon <in.zkey> <out.zkey> <beaconHashHex> <numIterationsExp>
 * [-n=name]` (reference dizkus-scripts/3_gen_chunk_zkey.sh:36).  zkp_beacon_secret (host only)
 * derives the contribution scalar as snarkjs@0.4.22 / ffjavascript do: 2^e chained SHA-256 of the
 * beacon, a ChaCha20 stream seeded with the hash, Fr.fromRng; k32: 32-byte LE.  zkp_zkey_beacon
 * draws the rest of the contribution from the same stream (G1.fromRng, the transcript, hashToG2),
 * applies k on the GPU and appends the type-1 record (deltaAfter, proof of knowledge,
 * transcript, numIterationsExp, beacon hash, name) to section 10, so the key passes `zkey
 * verify` (zkp_zkey_verify; reference circuit/scripts/generate_keys_phase2_groth16.sh:26).  e <= 63; name may be
 * NULL (not recorded).  Record bytes restated (oracle/mpc.py), parity unpinned. */
zkp_status zkp_beacon_secret(const uint8_t* beacon, size_t len, uint32_t num_iterations_exp, uint8_t* k32);
zkp_status zkp_zkey_beacon(int device, const uint8_t* zkey, size_t len, const uint8_t* beacon, size_t beacon_len,
                           uint32_t num_iterations_exp, uint8_t** out, size_t* out_len);
zkp_status zkp_zkey_beacon_named(int device, const uint8_t* zkey, size_t len, const uint8_t* beacon, size_t beacon_len,
                                 uint32_t num_iterations_exp, const char* name, uint8_t** out, size_t* out_len);

/* Setup acceleration: `snarkjs zkey contribute <in.zkey> <out.zkey> -e=<entropy> [-n=name]`
 * (reference dizkus-scripts/3_gen_chunk_zkey.sh:27): the contribution's rng is ChaCha20 seeded with
 * Blake2b-512(64 random bytes || entropy) (snarkjs misc.getRandomRng); rand64: those 64 bytes
 * (NULL: /dev/urandom; non-NULL only for reproducible tests).  The secret and the type-0 record
 * are drawn as for the beacon; the group arithmetic runs on `device`. */
zkp_status zkp_zkey_contribute_entropy(int device, const uint8_t* zkey, size_t len, const uint8_t* rand64,
                                       const char* entropy, const char* name, uint8_t** out, size_t* out_len);

/* Host only: Blake2b-512 of a buffer (the hash of the MPC transcript and circuit hash; exported so
 * the CPU tests pin it against Python's hashlib). */
zkp_status zkp_blake2b512(const uint8_t* data, size_t len, uint8_t* out64);

/* Setup acceleration: `snarkjs zkey new <circuit.r1cs> <pot.ptau> <circuit_0000.zkey>`
 * (reference dizkus-scripts/3_gen_chunk_zkey.sh:18) on `device`: the phase-2 starting key
 * (gamma = delta = 1) of a circom .r1cs (v1) from a prepared .ptau (v1, Lagrange sections 12-15,
 * power >= log2(domain) + 1).  A/B1/B2/IC/L are sparse sums of ptau Lagrange points with the
 * circuit's coefficients, built on the GPU; H is copied from the odd points of the next level.
 * Section 10 holds no contributions and the circuit hash (csHash: Blake2b-512 over the key's
 * points and the ptau's tauG1 powers, host).  *out: the zkey (zkp_buffer_free). */
zkp_status zkp_zkey_new(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                        uint8_t** out, size_t* out_len);

/* Setup acceleration: `snarkjs powersoftau prepare phase2 <pot_beacon.ptau> <pot_final.ptau>` (reference
 * circuit/scripts/generate_keys_phase1.sh:20; the step circuit/scripts/generate_keys_phase2_groth16.sh:7
 * asks about) on `device`: the Lagrange sections 12-15 that zkp_zkey_new reads.  For every level
 * p = 0..power the first 2^p points of sections 2, 3, 4, 5 go through a group inverse FFT
 * (zkp_group_ifft); level p lands at point offset 2^p - 1 of lTauG1 (12), lTauG2 (13), lAlphaTauG1 (14),
 * lBetaTauG1 (15).  The input needs sections 1-7 of a bn128 ptau (v1) with the sizes its power gives;
 * every point of sections 2-5 must have canonical coordinates and be on its curve or all-zero, else
 * ZKP_ERR_FORMAT "ptau: section <id> point <i> is not on the curve" (the smallest such i; no subgroup
 * check: that is zkp_ptau_verify_sections).  The output holds sections 1-7 copied byte for byte in that
 * order, then 12, 13, 14, 15; sections 12-15 of the input are ignored and rebuilt, any other section id
 * is not copied.  A power whose working set does not fit in free HBM is ZKP_ERR_OUT_OF_MEMORY before
 * any launch.  Layout restated (oracle/binfile.py write_ptau), parity unpinned.
 * *out: the prepared ptau (zkp_buffer_free). */
zkp_status zkp_ptau_prepare_phase2(int device, const uint8_t* ptau, size_t len, uint8_t** out, size_t* out_len);
/* ms of the last zkp_ptau_prepare_phase2 on this thread: [0] total, [1] parse + point check, [2] upload
 * (host wall), [3] G1 iFFT (all levels, three vectors), [4] G2 iFFT, [5] affine conversion (the levels
 * above one workgroup; the small levels convert inside their one launch, counted in [3] / [4]),
 * [6] download (host wall; overlaps the next level), [7] kernel launches.  n = capacity of ms. */
zkp_status zkp_ptau_prepare_timings(double* ms, int n);

/* Setup acceleration: the point sections of `snarkjs powersoftau verify <ptau>` (reference
 * circuit/scripts/generate_keys_phase1.sh:16; commented out as too slow in generate_keys_phase2_groth16.sh:3
 * and generate_keys_phase2_plonk.sh:3) on `device`, of sections 2-6 and, if present, 12-15 (the project's
 * layout: 2^(power+1) - 1 points each, oracle/binfile.py write_ptau); section 7 is not read beyond its
 * presence.  In order, the first failing check gives the message:
 *  1. every point has canonical coordinates and is all-zero or on its curve ("section <id> point <i> is
 *     not on the curve": the smallest i of the smallest id); every G2 point (sections 3, 6, 13) is
 *     all-zero or in the subgroup of order r ("section <id> point <i> is not in the subgroup");
 *  2. tauG1[0], tauG2[0] are the generators ("First element of tau*G1 section must be the generator",
 *     "... tau*G2 ..."); tauG1[1], tauG2[1], alphaTauG1[0], betaTauG1[0], betaG2 are not infinity;
 *  3. powers: random linear combinations of adjacent points and one pairing check per section
 *     ("tauG1 section. Powers do not match", tauG2, alphaTauG1, betaTauG1; "betaG2 does not match
 *     betaTauG1");
 *  4. every Lagrange section against its tau section ("Lagrange section <id> does not match section
 *     <id'> at level <p>": the smallest failing level).
 * Status and verdict as zkp_zkey_verify: the status reports only a malformed file (bad magic or version,
 * n8 != 32, power outside 1..28, ceremonyPower < power, a section 2-7 missing or not the size its power
 * gives, sections 12-15 present in part or of another size: ZKP_ERR_FORMAT naming the section; another
 * prime: ZKP_ERR_CURVE), a working set beyond free HBM (ZKP_ERR_OUT_OF_MEMORY before any launch) or a
 * device error; a file that fails a check is ZKP_OK with *valid = 0.  seed32 and ZKP_VERIFY_CHUNK as
 * zkp_zkey_verify (PRODUCTION PASSES NULL).  Lagrange sections are checked up to power 27. */
zkp_status zkp_ptau_verify_sections(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32 /* NULL: OS CSPRNG */,
                                    int* valid, char* msg, size_t msg_cap);
/* `snarkjs powersoftau verify <ptau>` whole: the contribution chain of section 7 on the host, then the above.
 * Section 7 is a u32 count and that many records: tauG1, tauG2, alphaG1, betaG1, betaG2 (LEM points); the
 * public key's nine points (tau, alpha, beta: g1_s, g1_sx each, then the three g2_spx); partialHash (216
 * bytes, a Blake2b-512 state in progress: h[8], t, f, the 128-byte buffer, its fill, u64 LE each);
 * nextChallenge (64); type (u32: 0 contribute, 1 beacon); a u32 parameter length and the parameters as in
 * section 10 of a zkey.  Layout and hashes restated from snarkjs 0.4.22, parity unpinned; the model that
 * fixes them is tests/helpers/ptau_model.py.  A record cut short, a length that runs past the section's
 * end, a coordinate >= p, a malformed partialHash, a beacon without parameters or with numIterationsExp
 * > 63 are ZKP_ERR_FORMAT naming section 7.  Verdicts, in this order: no contribution ("This file has no
 * contribution! It cannot be used in production"); the last contribution against the one before it
 * (a beacon's key re-drawn: "BEACON key (tauG1_s) is not generated correctly" ...; "INVALID key (tau)" /
 * (alpha) / (beta); "INVALID tau*G1. contribution", tau*G2, alpha*G1, beta*G1, beta*G2); its five points
 * against the sections ("Second element of tau*G1 section does not match the one in the contribution
 * section" ...); the sections (above); if power = ceremonyPower, Blake2b(responseHash || sections 2-6
 * uncompressed) against the last nextChallenge ("Hash of the values does not match the next challenge of
 * the last contributor in the contributions section"); the earlier contributions, last but one first.
 * The first contribution is checked against the first challenge: a Blake2b over 384 * 2^ceremonyPower
 * bytes (about 100 GB at 28), hashed on a host thread beside the device work. */
zkp_status zkp_ptau_verify(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32 /* NULL: OS CSPRNG (production) */,
                           int* valid, char* msg, size_t msg_cap);
/* ms of the last zkp_ptau_verify / zkp_ptau_verify_sections on this thread: [0] total, [1] parse (host), [2] uploads (host
 * wall; they overlap the checks), [3] point check, [4] G2 subgroup check, [5] coefficients, [6] Lagrange
 * scalars (NTT + fold), [7] base conversion + plans, [8] accumulate + finish of the pair sums, [9] of the
 * Lagrange side (129-bit), [10] of the tau side (255-bit), [11] host folds, [12] host pairings,
 * [13] chunks; zkp_ptau_verify only (host): [14] the contributions' checks, [15] the first challenge hash
 * (its own thread), [16] the next-challenge hash.  n = capacity of ms. */
zkp_status zkp_ptau_verify_timings(double* ms, int n);

/* Setup acceleration: `snarkjs zkey verify`, the gate of every phase-2 ceremony (reference
 * circuit/scripts/generate_keys_phase2_groth16.sh:26, circuit/server-scripts/
 * generate_keys_phase2_groth16.sh:56, generate_chunked_keys_phase2_groth16.sh:68,
 * zk-email-verify-circuits/scripts/compile.js:109), against the initial key `zkey new` wrote for the same
 * circuit and ptau.  The checks of oracle/mpc.py zkey_verify in its order and words: the transcript
 * chain of every contribution (transcript hash, hashToG2, the two same-ratio pairings, the beacon's
 * re-draw), the header, delta1, delta2, the csHash, sections 3-7 byte for byte (host); then L and H
 * as random linear combinations of both keys' sections on `device`, one pairing check each.  Also,
 * with messages of their own: every point of sections 2 and 10 is on its curve (G2: in the subgroup)
 * and every L / H point is canonical and on the curve ("INVALID: L section point <i> is not on the
 * curve": the smallest such i).
 * The status reports only malformed input (ZKP_ERR_FORMAT, ...) or a device error.  A key that fails
 * a check is ZKP_OK with *valid = 0 and the failing check in msg ("OK" and *valid = 1 otherwise); msg
 * (may be NULL) receives at most msg_cap - 1 characters and a NUL.
 * The H check accepts a key written by zkp_zkey_import_bellman, as snarkjs does: such a key's section 9
 * differs from a direct contribution's by a multiple of (w^j)_j (n = 2^p the domain, w = Fr.w[p]), a direction
 * in which no prover's sum over H has a component.  Points 0..n-2 take the stream's coefficients r_j as before
 * (indices nL..nL+n-2) and point n - 1 takes r' = -w sum_(j<n-1) r_j w^j mod r, so that sum_j r_j w^j = 0 and the
 * combination does not see that direction; a wrong H section still passes with probability <= 2^-128 unless it
 * differs from the right one by such a multiple.  Every key accepted before is accepted, with the same messages.
 * seed32 seeds the linear combinations' coefficients (128-bit: a wrong section passes with
 * probability <= 2^-128 each).  PRODUCTION MUST PASS NULL (32 bytes from the OS CSPRNG): the
 * coefficients must be unpredictable to whoever wrote the key.  Non-NULL is for reproducible tests.
 * ZKP_VERIFY_CHUNK=<points> (default 4194304) sets the points per device chunk; a malformed value or
 * one below 1 is a ZKP_ERR_INVALID_ARG.  Messages restated (oracle/mpc.py), parity unpinned. */
zkp_status zkp_zkey_verify_frominit(int device, const uint8_t* init, size_t init_len, const uint8_t* key, size_t key_len,
                                    const uint8_t* seed32 /* NULL: OS CSPRNG (production) */, int* valid,
                                    char* msg, size_t msg_cap);
/* `snarkjs zkey verify <r1cs> <ptau> <zkey>`: zkp_zkey_new on `device`, then the above. */
zkp_status zkp_zkey_verify(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                           const uint8_t* key, size_t key_len, const uint8_t* seed32, int* valid, char* msg, size_t msg_cap);
/* ms of the last zkp_zkey_verify[_frominit] on this thread: [0] total, [1] host (parsing, transcript
 * chain, pairings), [2] the section compares, then the L and H linear combinations together:
 * [3] upload (host wall; overlaps the previous chunk's compute), [4] point check, [5] coefficient
 * generation, [6] base conversion + plan, [7] [8] accumulate + finish over the initial / the checked
 * key's points, [9] host folds, [10] their wall time, [11] chunks.  n = capacity of ms. */
zkp_status zkp_zkey_verify_timings(double* ms, int n);

/* Load only point slice `part` of `nparts` (contiguous ranges of the witness-indexed
 * sections 5-8 and of section 9) onto one device.  Such a prover computes partial sums
 * only (zkp_prove_partial); the quotient is computed in full on every part. */
zkp_status zkp_prover_load_part(const uint8_t* zkey, size_t len, int device, int part, int nparts,
                                zkp_prover** out);

zkp_status zkp_prover_info(const zkp_prover* p, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain_size);

/* Prove one witness (.wtns bytes, version <= 2).  r32 / s32: 32-byte LE blinding
 * scalars (< r); NULL -> drawn from the OS CSPRNG (production).  Non-NULL is for
 * bit-exact tests: A, B, C are then a deterministic function of (zkey, wtns, r, s). */
zkp_status zkp_prove(zkp_prover* p, const uint8_t* wtns, size_t len, const uint8_t* r32, const uint8_t* s32,
                     zkp_proof* out);

/* Prove n witnesses, spread over the prover's devices: a shared queue, two host workers per
 * device (the next witness's H2D overlaps the current proof), every proof attempted.
 * r32s / s32s may be NULL (all random) or arrays of n pointers.  Returns ZKP_OK if every
 * proof succeeded, else the first failing proof's status (message names its index). */
zkp_status zkp_prove_batch(zkp_prover* p, const uint8_t* const* wtns, const size_t* lens, int n,
                           const uint8_t* const* r32s, const uint8_t* const* s32s, zkp_proof* outs);
/* The same with a per-proof status array (n entries; proofs with ZKP_OK are valid).  A
 * device that fails (HIP error) is retired and its witness re-queued to the remaining
 * devices; an invalid witness fails alone. */
zkp_status zkp_prove_batch_status(zkp_prover* p, const uint8_t* const* wtns, const size_t* lens, int n,
                                  const uint8_t* const* r32s, const uint8_t* const* s32s, zkp_proof* outs,
                                  zkp_status* statuses);

/* Partial MSM sums of this prover's slice for one witness (any prover; a full one
 * reports part 0 of 1). */
zkp_status zkp_prove_partial(zkp_prover* p, const uint8_t* wtns, size_t len, zkp_partial* out);
/* Host only (no device): sum the nparts partials of one split, then blind (r32 / s32 as
 * in zkp_prove) and assemble the proof; public signals come from wtns.  The result is
 * bit-identical to zkp_prove on the full key. */
zkp_status zkp_proof_combine(const uint8_t* zkey, size_t len, const zkp_partial* parts, int nparts,
                             const uint8_t* wtns, size_t wlen, const uint8_t* r32, const uint8_t* s32,
                             zkp_proof* out);

/* CLI-equivalent: `groth16 prove <zkey> <wtns> <proof.json> <public.json>` on a
 * loaded prover; writes JSON byte-compatible with snarkjs (JSON.stringify(x,null,1)).
 * A regular witness file is memory-mapped for the transfer: it must not be truncated by another
 * writer during the call (other file kinds are read into a buffer first). */
zkp_status zkp_prove_files(zkp_prover* p, const char* wtns_path, const char* proof_json_path,
                           const char* public_json_path);

/* Format a proof as snarkjs proof.json / public.json text.  Returns the needed size
 * (including NUL) in *needed; writes when cap is large enough. */
zkp_status zkp_proof_json(const zkp_proof* proof, char* buf, size_t cap, size_t* needed);
zkp_status zkp_public_json(const zkp_proof* proof, char* buf, size_t cap, size_t* needed);

/* `snarkjs zkey export soliditycalldata` text of a proof + its public signals
 * (reference circuit/scripts/generate_calldata.sh:3): a, b (G2 pairs in EIP-197
 * [c1, c0] order, as Verifier.sol:184-188 expects), c, inputs as "0x" + 64 hex digits. */
zkp_status zkp_proof_calldata(const zkp_proof* proof, char* buf, size_t cap, size_t* needed);

/* Per-stage device timings (ms) of the last zkp_prove on this handle:
 * [0] wtns H2D, [1] buildABC, [2] NTT/quotient, [3] MSM G1 A,B1,C (own stream, overlaps
 * [1]-[2]), [4] MSM G2 B2 (own stream), [5] host assembly, [6] total wall, [7] MSM G1 H,
 * [8] verify-before-return (host; 0 when off), [9] the witness transfer's PCIe payload in MB
 * (compact encoding; 0 for staged proofs), [10] the witness-MSM configuration
 * the proof took (0: the default window bits, 1: the second, wider ones; zkp_prover_msm_config).
 * n = capacity of ms (entries beyond n are not written). */
zkp_status zkp_prover_timings(const zkp_prover* p, float* ms, int n);

void zkp_prover_free(zkp_prover* p);

/* Verify-before-return (the reference verifies every proof right after proving:
 * dizkus-scripts/5_gen_proof.sh:14-21 `snarkjs groth16 verify`).  A checked proof is verified on
 * the host (optimal-ate pairing, the Verifier.sol:340-358 equation) against the zkey's verification
 * key before it is returned; a proof that fails the check is never returned: the call (or that
 * proof's batch status) reports ZKP_ERR_INTERNAL ("proof failed verify-before-return ...").
 * on = 0: off; 1: every proof of zkp_prove / zkp_prove_batch[_status] / zkp_prove_staged /
 * zkp_prove_files; 2 (the DEFAULT): the proofs of zkp_prove_batch[_status] only -- there the check
 * runs on the worker thread while the next proof computes (no measured throughput cost), while on
 * a single proof it would add a few ms of one host core to the latency.  The environment
 * ZKP_VERIFY=0/1/2 at load overrides the default.  Any other nonzero `on` means 1. */
zkp_status zkp_prover_set_verify(zkp_prover* p, int on);
/* The current verify-before-return mode (0, 1 or 2 as above). */
zkp_status zkp_prover_get_verify(const zkp_prover* p, int* mode);

/* Host only (no device): `snarkjs groth16 verify` of one proof against a zkey's verification key
 * (sections 2 and 3).  *valid = 1 if the proof verifies (public signals from proof->public_signals,
 * each < r), else 0; the status reports only malformed input. */
zkp_status zkp_proof_verify(const uint8_t* zkey, size_t len, const zkp_proof* proof, int* valid);

/* Host only: the BN254 optimal-ate pairing e(P, Q) as snarkjs reports GT elements (ffjavascript's
 * final exponentiation), e.g. vk_alphabeta_12 = e(vk_alpha_1, vk_beta_2) of a verification key.
 * g1: x, y (64 bytes), g2: x.c0, x.c1, y.c0, y.c1 (128 bytes), standard-form LE, all-zero =
 * infinity.  out: 12 x 32 bytes, the Fq12 coefficients in snarkjs' JSON nesting order
 * [[c0.c0, c0.c1, c0.c2], [c1.c0, c1.c1, c1.c2]], each Fq2 as (c0, c1). */
zkp_status zkp_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* out384);

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* zkp_last_error(void);

/* Library / build identification, e.g. "zkp_amd 0.1 gfx950". */
const char* zkp_version(void);

/* ---- kernel-level entry points (tests and benchmarks; same kernels as zkp_prove) ----
 * points: zkey layout (affine, Montgomery 2^256 LE; infinity = zero bytes),
 * scalars: 32-byte LE standard form.  out: affine standard-form LE (64 / 128 bytes),
 * all-zero + *is_inf = 1 for the point at infinity. */
zkp_status zkp_msm_g1(int device, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out64,
                      int* is_inf);
zkp_status zkp_msm_g2(int device, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out128,
                      int* is_inf);
/* The same MSM with explicit Pippenger parameters (tests / tuning): window_bits c
 * (0 = automatic, else 8..24) and base-table depth T (0 = automatic = all windows in
 * one bucket set; 1 = no precomputed rows, one bucket group per window). */
zkp_status zkp_msm(int device, int g2, const uint8_t* points, const uint8_t* scalars, size_t n, int window_bits,
                   int table_depth, uint8_t* out, int* is_inf);
/* The device parts of zkp_zkey_verify, each on its own.
 * zkp_rlc_coeffs: coefficients first_index .. first_index + n - 1 of a verification, generated on the
 * device: coefficient i is the 128-bit LE integer of outputs 4i..4i+3 (lowest word first) of
 * ffjavascript's ChaCha word stream seeded with the 8 big-endian 32-bit words of seed32.  out: n x 16
 * bytes LE.  One stream serves a verification: L takes 0..nL-1, H takes nL..nL+nH-1.
 * zkp_points_check: *n_bad = the points (zkey layout; g2: 128 bytes each) that have a coordinate >= p
 * or are neither all-zero nor on the curve; *first_bad = the smallest such index (UINT64_MAX if none).
 * zkp_rlc_g1: sum_i coeff(first_index + i) * a_i and the same over b_i (G1, zkey layout) under one
 * MSM plan, after zkp_points_check of both (a bad point is a ZKP_ERR_INVALID_ARG). */
zkp_status zkp_rlc_coeffs(int device, const uint8_t* seed32, uint64_t first_index, size_t n, uint8_t* out);
/* The kernel of zkp_ptau_prepare_phase2 on one vector: out_c = n^-1 sum_j w^(-c j) P_j for the
 * n = 2^log_n points (zkey layout; g2: 128 bytes each; log_n <= 28) at `points`, w = Fr.w[log_n], natural
 * order in and out; out: n points.  For P_j = tau^j G this is L_c(tau) G.  Every exceptional addition
 * (infinity, equal and opposite operands) is computed, not assumed away. */
zkp_status zkp_group_ifft(int device, int g2, const uint8_t* points, int log_n, uint8_t* out);
/* The forward direction of the same kernels: out_c = sum_j w^(c j) P_j, no n^-1 (zkp_zkey_export_bellman takes
 * section 9 through it).  zkp_group_ifft(zkp_group_fft(x)) = x. */
zkp_status zkp_group_fft(int device, int g2, const uint8_t* points, int log_n, uint8_t* out);
zkp_status zkp_points_check(int device, int g2, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad);
zkp_status zkp_rlc_g1(int device, const uint8_t* seed32, uint64_t first_index, const uint8_t* points_a,
                      const uint8_t* points_b, size_t n, uint8_t* out_a64, int* inf_a, uint8_t* out_b64, int* inf_b);
/* The device parts of zkp_ptau_verify_sections, each on its own.
 * zkp_g2_subgroup_check: *n_bad = the G2 points (zkey layout, on the curve) that are neither all-zero nor
 * of order r; *first_bad = the smallest such index (UINT64_MAX if none).
 * zkp_rlc_pairs: A = sum_{i<n-1} r_i P_i and B = sum_{i<n-1} r_i P_(i+1) under one MSM plan, r_i =
 * coefficient first_index + i of zkp_rlc_coeffs; out_a / out_b: 64 bytes (g2: 128), affine standard-form
 * LE; n <= 1 gives two infinities; a point off its curve is a ZKP_ERR_INVALID_ARG. */
zkp_status zkp_g2_subgroup_check(int device, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad);
zkp_status zkp_rlc_pairs(int device, int g2, const uint8_t* seed32, uint64_t first_index, const uint8_t* points, size_t n,
                         uint8_t* out_a, int* inf_a, uint8_t* out_b, int* inf_b);
/* In-place Fr transforms on n = 2^k standard-form LE elements, natural order:
 * mode 0: forward (A_j = sum a_i w^ij), 1: inverse, 2: coset-extend (snarkjs
 * ifft -> batchApplyKey(1, Fr.w[k+1]) -> fft). */
zkp_status zkp_ntt_fr(int device, uint8_t* data, size_t n, int mode);
/* The H-MSM scalars P_j (standard form, n = domain) for (zkey, wtns): rows A4..A8. */
zkp_status zkp_quotient(zkp_prover* p, const uint8_t* wtns, size_t len, uint8_t* out);

/* ---- benchmarking / serving helpers ----
 * Keep a witness resident in HBM (dev_index: index into the `devices` list the prover was
 * loaded with, 0..ndev-1, whatever ZKP_INFLIGHT is; the witness goes to that device's first
 * pipeline; any slot number); zkp_prove_staged then runs the proof without the PCIe copy.
 * Calls for different dev_index values run concurrently; concurrent calls for the same
 * dev_index take that device's idle ZKP_INFLIGHT pipelines (which read the staged witness in
 * place) and queue on its first pipeline when none is idle. */
zkp_status zkp_witness_stage(zkp_prover* p, int dev_index, int slot, const uint8_t* wtns, size_t len);
zkp_status zkp_prove_staged(zkp_prover* p, int dev_index, int slot, const uint8_t* r32, const uint8_t* s32,
                            zkp_proof* out);
zkp_status zkp_prove_partial_staged(zkp_prover* p, int slot, zkp_partial* out);
/* Distributed quotient of a split proof: instead of every part
 * recomputing all three coset extensions, part v % nparts computes vector v (A, B, C) and
 * the parts exchange domain slices (zkp_amd.dist: RCCL send/recv over xGMI).
 * Stage 1: buildABC on the witness staged in `slot`, then the coset extension of the
 * vectors selected by mask (bit 0 A, 1 B, 2 C); vector v is copied whole (domain_size x
 * 32 bytes, opaque device layout) to dst[v], device memory on this prover's device
 * (entries of unselected vectors may be NULL).  Returns when the copies are complete. */
zkp_status zkp_quotient_part_staged(zkp_prover* p, int slot, int mask, void* const* dst);
/* Stage 2: the partial sums of this prover's slice with the H-MSM scalars joined from
 * abc[0..2] = device pointers to the stage-1 values of A, B, C at this part's domain
 * slice [part*n/nparts, (part+1)*n/nparts) (contiguous, complete before the call). */
zkp_status zkp_prove_partial_ext_staged(zkp_prover* p, int slot, const void* const* abc, zkp_partial* out);
/* Bracket every bucket-accumulate kernel launch with HIP events (on its stream).
 * zkp_prover_kernel_stats: [0] G1 accumulate ms (sum), [1] G1 launches, [2] G1 mixed
 * additions, [3] G1 tasks, [4..7] the same for G2.  Enabling resets the counters. */
zkp_status zkp_prover_instrument(zkp_prover* p, int on);
zkp_status zkp_prover_kernel_stats(const zkp_prover* p, double* out, int n);
/* Every instrumented bucket-accumulate launch since zkp_prover_instrument(p, 1), in order: record i =
 * out[4i .. 4i+3] = {kind, mixed additions, ms (HIP events on the launch's stream), workgroups of the
 * launch (to match the dispatch in a kernel trace)}, kind 0 / 1 / 2 =
 * the witness MSMs A / B1 / C (G1), 3 = the H MSM (G1), 4 = the witness MSM B2 (G2).  Writes at most
 * max_records records; *n_records = the number held (up to 65536 per pipeline). */
zkp_status zkp_prover_launch_stats(const zkp_prover* p, double* out, int max_records, int* n_records);
/* MSM configuration chosen at load (device 0): [0] witness-MSM window bits c, [1] its
 * base-table depth T, [2] its bucket groups ceil(W/T), [3..5] the same for the H MSM,
 * [6] bytes of precomputed base tables per device, [7..9] c, T and groups of the second witness-MSM
 * configuration (wider windows, taken by witnesses whose values are mostly >= 2^32; 0 when the
 * prover keeps only one).  n = capacity of out. */
zkp_status zkp_prover_msm_config(const zkp_prover* p, double* out, int n);
/* Device-resident kernel benchmarks.  MSM: stats[0] ms per MSM, [1] ms per
 * accumulate-kernel launch, [2] mixed additions per launch, [3] tasks per launch,
 * [4] window bits c, [5] windows.  out/is_inf receive the result (verification). */
zkp_status zkp_bench_msm(int device, int g2, const uint8_t* points, const uint8_t* scalars, size_t n, int warmup,
                         int iters, double* stats, uint8_t* out, int* is_inf);
/* The same with nstats = capacity of stats, and [6] ms to build the base tables (row 0 upload and
 * conversion + the derived rows 2^(c t) P, t < T: fixed bases, outside the timed MSMs, as the prover
 * builds them at zkey load), [7] the table depth T (rows per point). */
zkp_status zkp_bench_msm_ex(int device, int g2, const uint8_t* points, const uint8_t* scalars, size_t n, int warmup,
                            int iters, double* stats, int nstats, uint8_t* out, int* is_inf);
/* ms per MSM plan build (digits, bucket grouping, task offsets) of n scalars (32-byte LE):
 * window_bits 0 = automatic; dense != 0: every (window, point) digit an entry, grouped by the
 * hand-written LDS-staged bucket sort (the H MSM's plan), else the compacted witness plan */
zkp_status zkp_bench_plan(int device, const uint8_t* scalars, size_t n, int window_bits, int dense, int warmup,
                          int iters, double* ms);
/* ms per coset-extension (iNTT + coset key + NTT) of 2^log_n Fr elements */
zkp_status zkp_bench_ntt(int device, int log_n, int warmup, int iters, double* ms);
/* ms per batched coset-extension of count (1..3) vectors of 2^log_n Fr elements, every pass one
 * launch over all of them: what the prover runs on the quotient's A, B, C */
zkp_status zkp_bench_ntt_batch(int device, int log_n, int count, int warmup, int iters, double* ms);

/* ---- Phase 1 from its start: `snarkjs powersoftau new | contribute | beacon` (reference
 * circuit/scripts/generate_keys_phase1.sh:6,8,10,18).  With zkp_ptau_verify and zkp_ptau_prepare_phase2 the
 * script's commands run here end to end; `export challenge`, `challenge contribute` and `import response`
 * (script lines 12-14) follow below.  The
 * formats are restated from snarkjs 0.4.22 (parity unpinned); tests/helpers/ptau_model.py fixes them byte for
 * byte.  Buffers handed out are released with zkp_buffer_free.
 *
 * zkp_ptau_new: `powersoftau new bn128 <power>`; host only.  Sections 1-7, every point a generator, no
 * contribution.  power within 1..28, ceremony_power >= power (0: = power), else ZKP_ERR_INVALID_ARG.
 *
 * zkp_ptau_contribute: one contribution on the GPU.  The key comes from the rng that
 * zkp_zkey_contribute_entropy builds from rand64 (NULL: 64 bytes of the OS CSPRNG) and entropy; it answers the
 * last record's nextChallenge, or the first challenge of a file without contributions.  tauG1[i] and tauG2[i]
 * are multiplied by tau^i, alphaTauG1[i] by alpha tau^i, betaTauG1[i] by beta tau^i, betaG2 by beta
 * (5 * 2^power - 1 scalar multiplications, each point by its own scalar), and a record is appended to section
 * 7 (name: recorded unless NULL).  Input: sections 1-7 of a bn128 ptau v1 with the sizes its power gives, else
 * ZKP_ERR_FORMAT / ZKP_ERR_CURVE naming the section, before the device is touched; every point of sections 2-6
 * canonical and on its curve or all-zero, else ZKP_ERR_FORMAT "ptau: section <id> point <i> is not on the
 * curve" (checked on the device).  A truncated file (power < ceremonyPower) is refused with
 * ZKP_ERR_INVALID_ARG: the next challenge hashes the sections of the whole ceremony, which such a file no
 * longer holds.  Output: sections 1-7 in that order; sections 12-15 of the input are dropped (a contribution
 * invalidates them) and any other id is not copied.  ZKP_PTAU_CHUNK: points per chunk streamed through the
 * device (default 4194304; a malformed value or one below 1 is ZKP_ERR_INVALID_ARG).  ZKP_PTAU_WINDOW=1|2: the
 * window bits of the per-point ladder (default 2, the faster one; the bytes are the same).
 *
 * zkp_ptau_beacon: the same with the beacon's rng (zkp_zkey_beacon's), a type-1 record and its two
 * parameters; num_iterations_exp <= 63 and beacon_len <= 255, else ZKP_ERR_INVALID_ARG.
 *
 * zkp_ptau_contribute_timings: ms of the calling thread's last contribute / beacon: [0] total, [1] parse +
 * point check, [2] first / last challenge, [3] key draw, [4] upload, [5] G1 scaling, [6] G2 scaling,
 * [7] encoding, [8] download, [9] partial-hash thread, [10] next-challenge thread, [11] chunks.
 *
 * zkp_points_scale_powers (kernel-level): out_i = (first * ratio^i) * P_i, i < n; zkey layout in and out
 * (G1 64 bytes, G2 128; canonical and on the curve or all-zero, else ZKP_ERR_INVALID_ARG); first32 / ratio32
 * 32-byte LE, reduced mod r. */
zkp_status zkp_ptau_new(uint32_t power, uint32_t ceremony_power /* 0: = power */, uint8_t** out, size_t* out_len);
zkp_status zkp_ptau_contribute(int device, const uint8_t* ptau, size_t len, const uint8_t* rand64 /* NULL: OS CSPRNG */,
                               const char* entropy, const char* name, uint8_t** out, size_t* out_len);
zkp_status zkp_ptau_beacon(int device, const uint8_t* ptau, size_t len, const uint8_t* beacon, size_t beacon_len,
                           uint32_t num_iterations_exp, const char* name, uint8_t** out, size_t* out_len);
zkp_status zkp_ptau_contribute_timings(double* ms, int n);
zkp_status zkp_points_scale_powers(int device, int g2, const uint8_t* points, size_t n, const uint8_t* first32,
                                   const uint8_t* ratio32, uint8_t* out);

/* ---- The third-party path of phase 1: `snarkjs powersoftau export challenge | challenge contribute | import
 * response` (reference circuit/scripts/generate_keys_phase1.sh:12-14): a contributor works on a challenge file
 * and returns a response file, and never holds the ptau.  With these the reference's phase-1 script runs here
 * from its first line to its last.  Formats restated from snarkjs 0.4.22 (parity unpinned);
 * tests/helpers/ptau_challenge_model.py fixes them byte for byte.  N = 2^power.
 *   challenge file  384 N + 128 bytes: the last record's response hash (Blake2b-512 of "" for a file without
 *                   contributions), then tauG1 (2N - 1 points), tauG2 (N), alphaTauG1 (N), betaTauG1 (N), betaG2
 *                   (1), uncompressed (big-endian standard form, x then y, G2 c1 before c0; 0x40 then zeros:
 *                   infinity).  Blake2b-512 of the whole file is the challenge.
 *   response file   192 N + 864 bytes: the challenge hash, the five sections after the contribution compressed
 *                   (big-endian x; 0x80 in the first byte: y is the greater root), the contributor's public key
 *                   uncompressed (768 bytes).  Blake2b-512 of the whole file is the response hash.
 * Everything that can be refused is refused before the device is touched.  ZKP_PTAU_CHUNK as above.
 *
 * zkp_ptau_export_challenge: sections 1-7 are checked as by zkp_ptau_contribute (the header, the sizes, the
 * records of section 7); a truncated file (power < ceremonyPower) is ZKP_ERR_INVALID_ARG for the same reason.
 * The points are not checked one by one: the hash below vouches for them.  The file is hashed as it is written, and if the
 * hash is not the challenge that section 7 implies (the last record's nextChallenge, or the first challenge of
 * the ceremony) the call fails with ZKP_ERR_FORMAT "ptau: sections 2-6 do not hash to the last contribution's
 * nextChallenge" and returns no file.  snarkjs only logs this; here a challenge that is not the chain's would
 * yield a response that zkp_ptau_import_response refuses anyway.
 *
 * zkp_ptau_challenge_contribute: the power is read from the length ((len - 128) / 384 a power of two within
 * 2^1..2^28, else ZKP_ERR_FORMAT).  The key is drawn as by zkp_ptau_contribute (same rng, same order) and
 * answers the hash of the challenge file.  Every point must have its coordinates below p (infinity: 0x40 then
 * zeros) and be on its curve, else ZKP_ERR_FORMAT "challenge: section <id> point <i> is not on the curve"
 * (checked on the device; smallest id, then smallest i).  Output: the response file.
 *
 * zkp_ptau_import_response: the old file is checked as above (truncated: ZKP_ERR_INVALID_ARG).  The response
 * must have the length the old file's power gives (ZKP_ERR_FORMAT "response: size of the contribution is
 * invalid"), begin with the old file's last challenge (ZKP_ERR_FORMAT "response: this contribution is not based
 * on the previous hash") and hold a key of nine canonical points on their curves (ZKP_ERR_FORMAT "response: key
 * point <k> ..."), all checked on the host.  Every compressed point is then decompressed on the device (one
 * square root each, in Fq or Fq2): 0x40 with anything but zeros beside it, an x >= p or an x for which x^3 + b
 * is a non-residue is ZKP_ERR_FORMAT "response: section <id> point <i> is not a point of the curve".  A type-0
 * record is appended to section 7 (name: recorded unless NULL).  Output: sections 1-7; sections 12-15 are
 * dropped, as by zkp_ptau_contribute.  The same-ratio checks of the contribution are NOT run here:
 * zkp_ptau_verify does that on the result, as in snarkjs.  Through export, challenge contribute and import the
 * result equals zkp_ptau_contribute's with the same rand64, entropy and name byte for byte.
 *
 * zkp_ptau_challenge_timings: ms of the calling thread's last call of the three: [0] total, [1] parse + point
 * check, [2] the challenge hash (export / import: the first challenge of a file without contributions),
 * [3] key draw / key check, [4] upload, [5] decoding, [6] G1 decompression, [7] G2 decompression, [8] G1
 * scaling, [9] G2 scaling, [10] encoding, [11] download, [12] the hash threads, [13] chunks.
 *
 * Device parts, each on its own (kernel-level):
 * zkp_points_decompress: n compressed points (G1 32 bytes, G2 64) -> the zkey layout (out_lem: n x 64 / 128
 * bytes).  A refused point (as in import) is written as zeros; *n_bad counts them and *first_bad is the
 * smallest such index (all ones if none).  A G2 point on the twist but outside the subgroup is not refused.
 * zkp_points_from_uncompressed: n uncompressed points (G1 64 bytes, G2 128) -> the zkey layout with the same
 * two counts; refused: a coordinate >= p, 0x40 set and anything but zeros beside it.  Whether the point is on
 * its curve is zkp_points_check's question.
 * zkp_field_sqrt: n elements of Fq (fq2 = 0: 32 bytes LE, standard form) or Fq2 (64 bytes: c0 then c1); a
 * coordinate >= p is ZKP_ERR_INVALID_ARG.  out: a root of each in the same form (which of the two is
 * unspecified), or zeros; is_square: one byte per element. */
zkp_status zkp_ptau_export_challenge(int device, const uint8_t* ptau, size_t len, uint8_t** out, size_t* out_len);
zkp_status zkp_ptau_challenge_contribute(int device, const uint8_t* challenge, size_t len,
                                         const uint8_t* rand64 /* NULL: OS CSPRNG */, const char* entropy, uint8_t** out,
                                         size_t* out_len);
zkp_status zkp_ptau_import_response(int device, const uint8_t* ptau, size_t len, const uint8_t* response, size_t response_len,
                                    const char* name, uint8_t** out, size_t* out_len);
zkp_status zkp_ptau_challenge_timings(double* ms, int n);
zkp_status zkp_points_decompress(int device, int g2, const uint8_t* compressed, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                                 uint64_t* first_bad);
zkp_status zkp_points_from_uncompressed(int device, int g2, const uint8_t* bytes, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                                        uint64_t* first_bad);
zkp_status zkp_field_sqrt(int device, int fq2, const uint8_t* in, size_t n, uint8_t* out, uint8_t* is_square);

/* ---- The third-party path of phase 2: `snarkjs zkey export bellman | zkey bellman contribute | zkey import
 * bellman`: a contributor works on an MPCParams file, which the Rust phase2 tools also read, and never holds the
 * .zkey.  Formats restated from snarkjs 0.4.22 (parity unpinned); tests/helpers/bellman_model.py fixes them byte
 * for byte.  Every integer is a big-endian u32, every point uncompressed (big-endian standard form, x then y, G2
 * c1 before c0; 0x40 then zeros: infinity):
 *   alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2                    G1 G1 G2 G2 G1 G2
 *   u32 nPublic + 1 | IC        u32 n - 1 | B_0 .. B_(n-2)        u32 nVars - nPublic - 1 | L
 *   u32 nVars | A               u32 nVars | B1                     u32 nVars | B2 (G2)
 *   csHash (64)                 u32 nContributions | deltaAfter | g1_s | g1_sx | g2_spx | transcript (384 each)
 * Up to csHash this is the byte string whose Blake2b-512 zkp_zkey_new records as csHash.  B_i = delta^-1 tau^i
 * (tau^n - 1) G1, n = 2^p the key's domain.  With w = Fr.w[p], w2 = Fr.w[p + 1] and section 9 holding H_j, the
 * Lagrange points of the 2n-domain at its odd nodes,
 *   export:  B_i  = -2 w2^i sum_j w^(ij) H_j, i < n - 1      (zkp_group_fft, then point i times -2 w2^i)
 *   import:  H'_j = n^-1 sum_i w^(-ij) (-1/2 w2^-i) B_i       (B_(n-1) := infinity; scaling, zkp_group_ifft)
 * H' is NOT byte-equal to the section 9 a direct zkp_zkey_contribute_entropy writes: the two differ by a multiple
 * of (w^j)_j, which no prover notices and zkp_zkey_verify accepts (above).  Every per-point pass (decode, point
 * check, scaling, encode) streams through the device in chunks of ZKP_PTAU_CHUNK points.
 *
 * zkp_mpcparams_info: host only.  Parses the layout: the counts against the length, n - 1 = 2^p - 1 with
 * p <= 27, the counts of L, A, B1, B2 and IC against each other, no trailing bytes; ZKP_ERR_FORMAT
 * "mpcparams: ..." otherwise.
 *
 * zkp_zkey_export_bellman: the key is parsed, header and section 10 included, and anything malformed refused
 * with ZKP_ERR_FORMAT before the device is touched.
 *
 * zkp_zkey_bellman_contribute: the secret k and its proof of knowledge are drawn exactly as by
 * zkp_zkey_contribute_entropy (same rng, same order; the transcript over csHash and the earlier contributions).
 * delta1 and delta2 become k times their old values, every H and L point is multiplied by k^-1, every other
 * section is copied, the new 384-byte contribution is appended and its Blake2b-512 written to hash64 (may be
 * NULL).  Every point must be canonical and on its curve, else ZKP_ERR_FORMAT "mpcparams: <section name> point
 * <i> is not on the curve" (checked on the device; the smallest i of the first such section).
 *
 * zkp_zkey_import_bellman: the response must have the old key's counts and csHash, exactly one contribution
 * more than the old key, its earlier contributions, alpha1, beta1, beta2, gamma2, IC, A, B1 and B2 equal to the
 * old key's, delta1 equal to the new contribution's deltaAfter, and every point canonical and on its curve;
 * each failure is ZKP_ERR_FORMAT "mpcparams: ..." naming the section.  Output: the old key's sections 1 and
 * 3-7 unchanged, section 2 with the new deltas, section 8 the decoded L, section 9 = H', section 10 with a
 * type-0 record appended (name: recorded unless NULL; the old records keep theirs).  The contribution's
 * same-ratio checks are NOT run here: zkp_zkey_verify does that on the result, as in snarkjs.
 *
 * zkp_zkey_bellman_timings: ms of the calling thread's last call of the three: [0] total, [1] parse and other
 * host work, [2] upload, [3] decoding, [4] point check, [5] scaling by k^-1, [6] the forward / inverse
 * transform, [7] coset scaling, [8] encoding, [9] download, [10] chunks. */
zkp_status zkp_mpcparams_info(const uint8_t* buf, size_t len, uint32_t* n_public, uint32_t* domain_size, uint32_t* n_vars,
                              uint32_t* n_contributions);
zkp_status zkp_zkey_export_bellman(int device, const uint8_t* zkey, size_t len, uint8_t** out, size_t* out_len);
zkp_status zkp_zkey_bellman_contribute(int device, const uint8_t* challenge, size_t len,
                                       const uint8_t* rand64 /* NULL: OS CSPRNG */, const char* entropy, uint8_t** out,
                                       size_t* out_len, uint8_t* hash64 /* may be NULL */);
zkp_status zkp_zkey_import_bellman(int device, const uint8_t* old_zkey, size_t len, const uint8_t* response,
                                   size_t response_len, const char* name, uint8_t** out, size_t* out_len);
zkp_status zkp_zkey_bellman_timings(double* ms, int n);

/* `wtns check <circuit.r1cs> <witness.wtns>`: does the witness satisfy every constraint A.w * B.w = C.w of
 * the circuit, and if not, which ones fail.  Later snarkjs versions ship this command and circom_tester's
 * checkConstraints is the same test; both recalled, unpinned (the reference pins snarkjs 0.4.22, which has
 * neither), so the shape is restated and the words are ours.  The zkey holds A and B only: the .r1cs is
 * the one file with C.  On the device the check is one sparse matrix-vector product in Fr and a comparison
 * per constraint.
 *
 * A checker holds the circuit's matrices on `device` (loaded and converted once).  A malformed .r1cs
 * (bad magic or version, a truncated section, a wire index >= nWires, more than 2^32 - 1 terms:
 * ZKP_ERR_FORMAT; n8 != 32 or a prime other than bn128's r: ZKP_ERR_CURVE) fails before any device work.
 * One check at a time per checker (a mutex serialises concurrent callers).
 *
 * A check's status reports only a malformed witness file (ZKP_ERR_FORMAT / ZKP_ERR_CURVE as zkp_prove;
 * ZKP_ERR_WITNESS_LENGTH when its length is not the circuit's nWires) or a device error.  The verdict is
 * ZKP_OK with res->valid and a message (msg may be NULL; at most msg_cap - 1 characters and a NUL):
 *   "OK"                                                           valid = 1
 *   "INVALID: signal 0 is not 1"
 *   "INVALID: signal <i> is not reduced"                           the lowest i with a value >= r
 *   "INVALID: constraint <first_bad> is not satisfied (<n_bad> of <n> fail)"
 * in this order of precedence.  n_bad is the exact number of failing constraints, bad[] the lowest
 * n_listed = min(16, n_bad) of them in ascending order, first_bad = bad[0]; all zero unless the verdict is
 * the last one.  The result is a function of the input alone. */
typedef struct zkp_checker zkp_checker;
typedef struct zkp_check_result {
  int valid;
  uint64_t n_bad, first_bad, n_constraints;
  uint32_t n_listed;
  uint64_t bad[16];
} zkp_check_result;
zkp_status zkp_checker_load(int device, const uint8_t* r1cs, size_t len, zkp_checker** out);
/* any of the four may be NULL; n_vars = nWires, n_terms = the terms of A, B and C together */
zkp_status zkp_checker_info(const zkp_checker* c, uint32_t* n_vars, uint32_t* n_public, uint32_t* n_constraints,
                            uint64_t* n_terms);
zkp_status zkp_checker_check(zkp_checker* c, const uint8_t* wtns, size_t len, zkp_check_result* res, char* msg,
                             size_t msg_cap);
/* The witness zkp_witness_stage left in slot `slot` of p's device dev_index, read in place (no second
 * transfer): stage -> check -> zkp_prove_staged.  The checker must be on that device and the circuit's
 * nWires equal the key's nVars (else ZKP_ERR_INVALID_ARG, as an empty slot).  Holds the staging slots as
 * a staged proof does (a restage waits for it) and only reads the slot. */
zkp_status zkp_checker_check_staged(zkp_checker* c, zkp_prover* p, int dev_index, int slot, zkp_check_result* res,
                                    char* msg, size_t msg_cap);
void zkp_checker_free(zkp_checker* c);
/* load + check + free.  Both files are validated before any device work. */
zkp_status zkp_wtns_check(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* wtns, size_t wtns_len,
                          zkp_check_result* res, char* msg, size_t msg_cap);
/* ms of the calling thread's last zkp_wtns_check / zkp_checker_load / zkp_checker_check[_staged]:
 * [0] r1cs parse + CSR + row classification (host), [1] CSR upload + coefficient conversion, [2] witness
 * copy (HIP events), [3] the kernels and the result's copy back (HIP events), [4] host wall of the call.
 * A load fills [0] [1] [4] (the rest 0), a check [2] [3] [4], zkp_wtns_check all five.  n = capacity. */
zkp_status zkp_wtns_check_timings(double* ms, int n);
/* [0] constraints on the wavefront-per-constraint kernel, [1] the term count from which a constraint takes
 * it (ZKP_WTNS_CHECK_LONG at load overrides the default; 0: none does).  n = capacity. */
zkp_status zkp_checker_paths(const zkp_checker* c, uint64_t* out, int n);

/* ---- `zkey export verificationkey` and `groth16 verify` from a verification key ----
 * zkp_zkey_export_vkey (host only): snarkjs' verification_key.json of a key's sections 2 and 3, as
 * JSON.stringify(vKey, null, 1): keys protocol, curve, nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2,
 * vk_alphabeta_12, IC in this order, points as projective decimal strings with the "1" / ["1","0"] tails.  The
 * layout is restated from memory (format-unpinned).  Buffer contract of zkp_proof_json: buf may be NULL to query
 * *needed (terminator included); a buf that is too small is ZKP_ERR_INVALID_ARG with *needed set.
 *
 * A zkp_verifier holds a verification key and verifies batches of proofs with the per-proof Miller loops on the
 * GPU.  zkp_verifier_load_vkey_json parses a verification_key.json with a strict parser of its own: malformed
 * JSON, a missing or mistyped field, a coordinate >= p, a point off its curve or (G2) outside the subgroup of
 * order r, an IC whose length is not nPublic + 1, a vk_alphabeta_12 (optional) that is not e(vk_alpha_1, vk_beta_2)
 * are ZKP_ERR_FORMAT with a zkp_last_error naming the field; another protocol is ZKP_ERR_PROTOCOL, another curve
 * ZKP_ERR_CURVE.  zkp_verifier_load_zkey takes the same key from sections 2 and 3 of a .zkey under the same
 * point checks.  Verification uses alpha and beta, never vk_alphabeta_12.
 *
 * zkp_verifier_verify: valid[i] (n bytes) = 1 iff proof i verifies, the verdict zkp_proof_verify gives for that
 * proof under the same key; *n_valid (nullable) = their count.  Public signals come from proofs[i].public_signals;
 * a proofs[i].n_public other than the key's (or a capacity below it) is ZKP_ERR_INVALID_ARG for the whole call.  A
 * proof that merely fails -- a coordinate >= p, a point off its curve, a B outside the subgroup, a public signal
 * >= r, a false pairing equation -- is ZKP_OK with valid[i] = 0.  n = 0 is ZKP_OK with *n_valid = 0.  The batch is
 * checked by one randomised equation with 128-bit coefficients drawn from seed32 (zkp_rlc_coeffs' stream): an
 * invalid proof is accepted with probability about 2^-128 over the seed.  seed32 = NULL takes the seed from the OS
 * CSPRNG and is what a production call MUST pass; a caller-chosen seed is for tests only (whoever knows the seed
 * before choosing the proofs can forge a batch).  Batches are processed in device passes of ZKP_VERIFY_CHUNK
 * proofs (default 16384, 64..1048576; a malformed value is ZKP_ERR_INVALID_ARG), so n is unbounded.  Concurrent
 * calls on one handle are serialised.
 *
 * zkp_verifier_timings: ms of the calling thread's last zkp_verifier_verify: [0] upload, coefficients and the
 * per-proof gates, [1] the scalar multiplications r_i A_i, r_i C_i, [2] the Miller kernel, [3] the product kernel
 * and the copies back, [4] host: s-vector, point sums and the three fixed-Q Miller loops, [5] the final
 * exponentiation, [6] the tree search of a failing batch, [7] host wall of the call, [8] equations evaluated
 * (a count, not ms).  n = capacity. */
zkp_status zkp_zkey_export_vkey(const uint8_t* zkey, size_t len, char* buf, size_t cap, size_t* needed);
typedef struct zkp_verifier zkp_verifier;
zkp_status zkp_verifier_load_vkey_json(int device, const char* json, size_t len, zkp_verifier** out);
zkp_status zkp_verifier_load_zkey(int device, const uint8_t* zkey, size_t len, zkp_verifier** out);
zkp_status zkp_verifier_info(const zkp_verifier* v, uint32_t* n_public);
zkp_status zkp_verifier_verify(zkp_verifier* v, const zkp_proof* proofs, size_t n,
                               const uint8_t* seed32 /* NULL: OS CSPRNG (production) */, uint8_t* valid /* n bytes */,
                               size_t* n_valid);
zkp_status zkp_verifier_timings(double* ms, int n);
void zkp_verifier_free(zkp_verifier* v);

/* ---- kernel-level pairing entry points (tests and benchmarks) ----
 * zkp_miller_loop: n optimal-ate Miller loops on the device, one per lane.  g1: n x 64, g2: n x 128 bytes,
 * standard-form LE, all-zero = infinity (such a pair gives 1); the points are the caller's to validate (on their
 * curves, g2 of order r).  out: n x 384 bytes in zkp_pairing's coefficient order.  The device keeps T and P
 * projective and never inverts, so each value is the host's Miller value times a factor of Fq2 that the final
 * exponentiation removes: zkp_final_exponentiation(out_i) == zkp_pairing(g1_i, g2_i), and device Miller values
 * may be compared with anything only after it.
 * zkp_final_exponentiation (host): ffjavascript's final exponentiation of one Fq12 value.
 * zkp_fq12_product: the product of n Fq12 values (n x 384 bytes, coordinates < p) by the reduction kernel, the
 * last few factors multiplied on the host; n = 0 gives 1. */
zkp_status zkp_miller_loop(int device, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out);
zkp_status zkp_final_exponentiation(const uint8_t* in384, uint8_t* out384);
zkp_status zkp_fq12_product(int device, const uint8_t* in, size_t n, uint8_t* out384);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_AMD_H */
