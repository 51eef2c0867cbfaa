"""Python host binding of libzkp_amd.so — the MI355X-native Groth16 prover.

Mirrors the snarkjs interface this path replaces (snarkjs@0.4.22, reference
``package-lock.json:3884-3896``):

* ``groth16.prove(zkeyFileName, witnessFileName, logger=None)`` →
  ``{"proof": {...}, "publicSignals": [...]}`` — reference call sites
  ``app/src/helpers/zkp.ts:94`` (via fullProve) and
  ``dizkus-scripts/5_gen_proof.sh:8`` (CLI).  Inputs are a path or a fastfile
  memory descriptor ``{"type": "mem", "data": bytes}``.
* errors raise ``Error`` subclasses with snarkjs' messages ("zkey file is not
  groth16", "Invalid witness length...", ...).

The HIP library is REQUIRED: there is no CPU fallback.  Loading fails loudly
(``LibraryNotBuilt``) when ``lib/libzkp_amd.so`` is missing.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("ZKP_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libzkp_amd.so")  # override: A/B runs
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "zkp_amd.h")

ZKP_OK = 0
# BN254 scalar field order r (reference contracts/Verifier.sol:341)
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
STATUS_NAMES = {
    0: "ZKP_OK", 1: "ZKP_ERR_INVALID_ARG", 2: "ZKP_ERR_IO", 3: "ZKP_ERR_FORMAT", 4: "ZKP_ERR_PROTOCOL",
    5: "ZKP_ERR_CURVE", 6: "ZKP_ERR_WITNESS_LENGTH", 7: "ZKP_ERR_DEVICE", 8: "ZKP_ERR_OUT_OF_MEMORY",
    9: "ZKP_ERR_INTERNAL",
}


class LibraryNotBuilt(RuntimeError):
    pass


class ZkpError(Exception):
    def __init__(self, status: int, message: str):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))
        self.status = status
        self.message = message


class _Proof(ctypes.Structure):
    _fields_ = [
        ("pi_a", (ctypes.c_uint8 * 32) * 2),
        ("pi_b", ((ctypes.c_uint8 * 32) * 2) * 2),
        ("pi_c", (ctypes.c_uint8 * 32) * 2),
        ("n_public", ctypes.c_uint32),
        ("public_capacity", ctypes.c_uint32),
        ("public_signals", ctypes.POINTER(ctypes.c_uint8)),
    ]


class _CheckResult(ctypes.Structure):  # zkp_check_result
    _fields_ = [
        ("valid", ctypes.c_int),
        ("n_bad", ctypes.c_uint64),
        ("first_bad", ctypes.c_uint64),
        ("n_constraints", ctypes.c_uint64),
        ("n_listed", ctypes.c_uint32),
        ("bad", ctypes.c_uint64 * 16),
    ]


_lib = None
_lib_lock = threading.Lock()


def load_library(path: str = LIB_PATH):
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise LibraryNotBuilt("libzkp_amd.so not found at %s — run __graft_entry__.build() "
                                  "(make -C zk-p2p-onramp_amd)" % path)
        lib = ctypes.CDLL(path)
        P = ctypes.c_void_p
        u8p = ctypes.POINTER(ctypes.c_uint8)
        sz = ctypes.c_size_t
        lib.zkp_prover_load_mem.argtypes = [u8p, sz, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(P)]
        lib.zkp_prover_load_file.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                             ctypes.POINTER(P)]
        lib.zkp_prover_info.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                        ctypes.POINTER(ctypes.c_uint32)]
        lib.zkp_prove.argtypes = [P, u8p, sz, u8p, u8p, ctypes.POINTER(_Proof)]
        lib.zkp_prove_batch.argtypes = [P, ctypes.POINTER(u8p), ctypes.POINTER(sz), ctypes.c_int,
                                        ctypes.POINTER(u8p), ctypes.POINTER(u8p), ctypes.POINTER(_Proof)]
        lib.zkp_prove_batch_status.argtypes = [P, ctypes.POINTER(u8p), ctypes.POINTER(sz), ctypes.c_int,
                                               ctypes.POINTER(u8p), ctypes.POINTER(u8p), ctypes.POINTER(_Proof),
                                               ctypes.POINTER(ctypes.c_int)]
        lib.zkp_prove_files.argtypes = [P, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        lib.zkp_proof_json.argtypes = [ctypes.POINTER(_Proof), ctypes.c_char_p, sz, ctypes.POINTER(sz)]
        lib.zkp_public_json.argtypes = [ctypes.POINTER(_Proof), ctypes.c_char_p, sz, ctypes.POINTER(sz)]
        lib.zkp_prover_timings.argtypes = [P, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
        lib.zkp_prover_free.argtypes = [P]
        lib.zkp_prover_free.restype = None
        lib.zkp_last_error.restype = ctypes.c_char_p
        lib.zkp_version.restype = ctypes.c_char_p
        lib.zkp_msm_g1.argtypes = [ctypes.c_int, u8p, u8p, sz, u8p, ctypes.POINTER(ctypes.c_int)]
        lib.zkp_msm_g2.argtypes = [ctypes.c_int, u8p, u8p, sz, u8p, ctypes.POINTER(ctypes.c_int)]
        lib.zkp_ntt_fr.argtypes = [ctypes.c_int, u8p, sz, ctypes.c_int]
        lib.zkp_quotient.argtypes = [P, u8p, sz, u8p]
        lib.zkp_witness_stage.argtypes = [P, ctypes.c_int, ctypes.c_int, u8p, sz]
        lib.zkp_prove_staged.argtypes = [P, ctypes.c_int, ctypes.c_int, u8p, u8p, ctypes.POINTER(_Proof)]
        lib.zkp_prover_instrument.argtypes = [P, ctypes.c_int]
        lib.zkp_prover_kernel_stats.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        lib.zkp_prover_launch_stats.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int)]
        lib.zkp_bench_msm.argtypes = [ctypes.c_int, ctypes.c_int, u8p, u8p, sz, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_double), u8p, ctypes.POINTER(ctypes.c_int)]
        if hasattr(lib, "zkp_bench_msm_ex"):
            lib.zkp_bench_msm_ex.argtypes = [ctypes.c_int, ctypes.c_int, u8p, u8p, sz, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_double), ctypes.c_int, u8p,
                                             ctypes.POINTER(ctypes.c_int)]
        lib.zkp_bench_ntt.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_double)]
        lib.zkp_bench_ntt_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_double)]
        lib.zkp_bench_plan.argtypes = [ctypes.c_int, u8p, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        lib.zkp_msm.argtypes = [ctypes.c_int, ctypes.c_int, u8p, u8p, sz, ctypes.c_int, ctypes.c_int, u8p,
                                ctypes.POINTER(ctypes.c_int)]
        lib.zkp_prover_msm_config.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        lib.zkp_proof_calldata.argtypes = [ctypes.POINTER(_Proof), ctypes.c_char_p, sz, ctypes.POINTER(sz)]
        lib.zkp_prover_load_chunks.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(P)]
        lib.zkp_zkey_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
        lib.zkp_zkey_read_chunks.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.POINTER(u8p),
                                             ctypes.POINTER(sz)]
        lib.zkp_zkey_contribute.argtypes = [ctypes.c_int, u8p, sz, u8p, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
        lib.zkp_zkey_new.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
        lib.zkp_ptau_prepare_phase2.argtypes = [ctypes.c_int, u8p, sz, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
        lib.zkp_ptau_prepare_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        lib.zkp_group_ifft.argtypes = [ctypes.c_int, ctypes.c_int, u8p, ctypes.c_int, u8p]
        for name in ("zkp_ptau_prepare_phase2", "zkp_ptau_prepare_timings", "zkp_group_ifft"):
            getattr(lib, name).restype = ctypes.c_int
        lib.zkp_beacon_secret.argtypes = [u8p, sz, ctypes.c_uint32, u8p]
        lib.zkp_zkey_beacon.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_uint32, ctypes.POINTER(u8p),
                                        ctypes.POINTER(sz)]
        lib.zkp_buffer_free.argtypes = [u8p]
        lib.zkp_buffer_free.restype = None
        lib.zkp_prover_load_part.argtypes = [u8p, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
        lib.zkp_prove_partial.argtypes = [P, u8p, sz, ctypes.c_char_p]
        lib.zkp_prove_partial_staged.argtypes = [P, ctypes.c_int, ctypes.c_char_p]
        lib.zkp_proof_combine.argtypes = [u8p, sz, ctypes.c_char_p, ctypes.c_int, u8p, sz, u8p, u8p,
                                          ctypes.POINTER(_Proof)]
        lib.zkp_quotient_part_staged.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
        lib.zkp_prove_partial_ext_staged.argtypes = [P, ctypes.c_int, ctypes.POINTER(P), ctypes.c_char_p]
        lib.zkp_zkey_beacon_named.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_uint32, ctypes.c_char_p,
                                              ctypes.POINTER(u8p), ctypes.POINTER(sz)]
        lib.zkp_zkey_contribute_entropy.argtypes = [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, ctypes.c_char_p,
                                                    ctypes.POINTER(u8p), ctypes.POINTER(sz)]
        lib.zkp_blake2b512.argtypes = [u8p, sz, u8p]
        lib.zkp_prover_set_verify.argtypes = [P, ctypes.c_int]
        if hasattr(lib, "zkp_prover_get_verify"):  # round-5 entry points (an older library loads for A/B runs)
            lib.zkp_prover_get_verify.argtypes = [P, ctypes.POINTER(ctypes.c_int)]
        lib.zkp_proof_verify.argtypes = [u8p, sz, ctypes.POINTER(_Proof), ctypes.POINTER(ctypes.c_int)]
        lib.zkp_pairing.argtypes = [u8p, u8p, u8p]
        if hasattr(lib, "zkp_zkey_verify_frominit"):  # zkey verify (an older library loads for A/B runs)
            u64p = ctypes.POINTER(ctypes.c_uint64)
            ip = ctypes.POINTER(ctypes.c_int)
            lib.zkp_zkey_verify_frominit.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, u8p, ip, ctypes.c_char_p, sz]
            lib.zkp_zkey_verify.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, u8p, sz, u8p, ip, ctypes.c_char_p, sz]
            lib.zkp_zkey_verify_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            lib.zkp_rlc_coeffs.argtypes = [ctypes.c_int, u8p, ctypes.c_uint64, sz, u8p]
            lib.zkp_points_check.argtypes = [ctypes.c_int, ctypes.c_int, u8p, sz, u64p, u64p]
            lib.zkp_rlc_g1.argtypes = [ctypes.c_int, u8p, ctypes.c_uint64, u8p, u8p, sz, u8p, ip, u8p, ip]
        if hasattr(lib, "zkp_ptau_verify_sections"):  # powersoftau verify (an older library loads for A/B runs)
            u64p = ctypes.POINTER(ctypes.c_uint64)
            ip = ctypes.POINTER(ctypes.c_int)
            lib.zkp_ptau_verify_sections.argtypes = [ctypes.c_int, u8p, sz, u8p, ip, ctypes.c_char_p, sz]
            lib.zkp_ptau_verify.argtypes = [ctypes.c_int, u8p, sz, u8p, ip, ctypes.c_char_p, sz]
            lib.zkp_ptau_verify_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            lib.zkp_g2_subgroup_check.argtypes = [ctypes.c_int, u8p, sz, u64p, u64p]
            lib.zkp_rlc_pairs.argtypes = [ctypes.c_int, ctypes.c_int, u8p, ctypes.c_uint64, u8p, sz, u8p, ip, u8p, ip]
        if hasattr(lib, "zkp_ptau_contribute"):  # powersoftau new / contribute / beacon
            lib.zkp_ptau_new.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
            lib.zkp_ptau_contribute.argtypes = [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, ctypes.c_char_p,
                                                ctypes.POINTER(u8p), ctypes.POINTER(sz)]
            lib.zkp_ptau_beacon.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_uint32, ctypes.c_char_p,
                                            ctypes.POINTER(u8p), ctypes.POINTER(sz)]
            lib.zkp_ptau_contribute_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            lib.zkp_points_scale_powers.argtypes = [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u8p, u8p]
            for name in ("zkp_ptau_new", "zkp_ptau_contribute", "zkp_ptau_beacon", "zkp_ptau_contribute_timings",
                         "zkp_points_scale_powers"):
                getattr(lib, name).restype = ctypes.c_int
        if hasattr(lib, "zkp_ptau_import_response"):  # powersoftau export challenge / challenge contribute / import response
            u64p = ctypes.POINTER(ctypes.c_uint64)
            lib.zkp_ptau_export_challenge.argtypes = [ctypes.c_int, u8p, sz, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
            lib.zkp_ptau_challenge_contribute.argtypes = [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, ctypes.POINTER(u8p),
                                                          ctypes.POINTER(sz)]
            lib.zkp_ptau_import_response.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_char_p, ctypes.POINTER(u8p),
                                                     ctypes.POINTER(sz)]
            lib.zkp_ptau_challenge_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            lib.zkp_points_decompress.argtypes = [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u64p, u64p]
            lib.zkp_points_from_uncompressed.argtypes = [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u64p, u64p]
            lib.zkp_field_sqrt.argtypes = [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u8p]
            for name in ("zkp_ptau_export_challenge", "zkp_ptau_challenge_contribute", "zkp_ptau_import_response",
                         "zkp_ptau_challenge_timings", "zkp_points_decompress", "zkp_points_from_uncompressed",
                         "zkp_field_sqrt"):
                getattr(lib, name).restype = ctypes.c_int
        if hasattr(lib, "zkp_zkey_import_bellman"):  # zkey export bellman / bellman contribute / import bellman
            u32p = ctypes.POINTER(ctypes.c_uint32)
            lib.zkp_group_fft.argtypes = [ctypes.c_int, ctypes.c_int, u8p, ctypes.c_int, u8p]
            lib.zkp_mpcparams_info.argtypes = [u8p, sz, u32p, u32p, u32p, u32p]
            lib.zkp_zkey_export_bellman.argtypes = [ctypes.c_int, u8p, sz, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
            lib.zkp_zkey_bellman_contribute.argtypes = [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, ctypes.POINTER(u8p),
                                                        ctypes.POINTER(sz), u8p]
            lib.zkp_zkey_import_bellman.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_char_p, ctypes.POINTER(u8p),
                                                    ctypes.POINTER(sz)]
            lib.zkp_zkey_bellman_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            for name in ("zkp_group_fft", "zkp_mpcparams_info", "zkp_zkey_export_bellman", "zkp_zkey_bellman_contribute",
                         "zkp_zkey_import_bellman", "zkp_zkey_bellman_timings"):
                getattr(lib, name).restype = ctypes.c_int
        if hasattr(lib, "zkp_wtns_check"):  # wtns check
            rp = ctypes.POINTER(_CheckResult)
            u32p = ctypes.POINTER(ctypes.c_uint32)
            lib.zkp_checker_load.argtypes = [ctypes.c_int, u8p, sz, ctypes.POINTER(P)]
            lib.zkp_checker_info.argtypes = [P, u32p, u32p, u32p, ctypes.POINTER(ctypes.c_uint64)]
            lib.zkp_checker_paths.argtypes = [P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
            lib.zkp_checker_check.argtypes = [P, u8p, sz, rp, ctypes.c_char_p, sz]
            lib.zkp_checker_check_staged.argtypes = [P, P, ctypes.c_int, ctypes.c_int, rp, ctypes.c_char_p, sz]
            lib.zkp_checker_free.argtypes = [P]
            lib.zkp_checker_free.restype = None
            lib.zkp_wtns_check.argtypes = [ctypes.c_int, u8p, sz, u8p, sz, rp, ctypes.c_char_p, sz]
            lib.zkp_wtns_check_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            for name in ("zkp_checker_load", "zkp_checker_info", "zkp_checker_paths", "zkp_checker_check",
                         "zkp_checker_check_staged", "zkp_wtns_check", "zkp_wtns_check_timings"):
                getattr(lib, name).restype = ctypes.c_int
        for name in ("zkp_zkey_verify_frominit", "zkp_zkey_verify", "zkp_zkey_verify_timings", "zkp_rlc_coeffs",
                     "zkp_points_check", "zkp_rlc_g1", "zkp_ptau_verify", "zkp_ptau_verify_sections", "zkp_ptau_verify_timings",
                     "zkp_g2_subgroup_check", "zkp_rlc_pairs"):
            if hasattr(lib, name):
                getattr(lib, name).restype = ctypes.c_int
        for name in ("zkp_zkey_beacon_named", "zkp_zkey_contribute_entropy", "zkp_blake2b512", "zkp_prover_set_verify", "zkp_prover_get_verify", "zkp_proof_verify", "zkp_pairing", "zkp_prover_load_mem", "zkp_prover_load_file", "zkp_prover_info", "zkp_prove",
                     "zkp_prove_batch", "zkp_prove_batch_status", "zkp_prove_files", "zkp_proof_json", "zkp_public_json",
                     "zkp_prover_timings", "zkp_msm_g1", "zkp_msm_g2", "zkp_ntt_fr", "zkp_quotient",
                     "zkp_witness_stage", "zkp_prove_staged", "zkp_prover_instrument", "zkp_prover_kernel_stats",
                     "zkp_prover_launch_stats",
                     "zkp_bench_msm", "zkp_bench_msm_ex", "zkp_bench_ntt", "zkp_bench_ntt_batch", "zkp_bench_plan", "zkp_msm", "zkp_prover_msm_config",
                     "zkp_prover_load_part", "zkp_prove_partial", "zkp_proof_calldata",
                     "zkp_prover_load_chunks", "zkp_zkey_read", "zkp_zkey_read_chunks", "zkp_zkey_contribute", "zkp_zkey_new",
                     "zkp_beacon_secret", "zkp_zkey_beacon", "zkp_prove_partial_staged", "zkp_proof_combine",
                     "zkp_quotient_part_staged", "zkp_prove_partial_ext_staged"):
            if hasattr(lib, name):
                getattr(lib, name).restype = ctypes.c_int
        if hasattr(lib, "zkp_verifier_verify"):
            lib.zkp_zkey_export_vkey.argtypes = [u8p, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
            lib.zkp_verifier_load_vkey_json.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(P)]
            lib.zkp_verifier_load_zkey.argtypes = [ctypes.c_int, u8p, sz, ctypes.POINTER(P)]
            lib.zkp_verifier_info.argtypes = [P, ctypes.POINTER(ctypes.c_uint32)]
            lib.zkp_verifier_verify.argtypes = [P, ctypes.POINTER(_Proof), sz, u8p, u8p, ctypes.POINTER(sz)]
            lib.zkp_verifier_timings.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int]
            lib.zkp_verifier_free.argtypes = [P]
            lib.zkp_verifier_free.restype = None
            lib.zkp_miller_loop.argtypes = [ctypes.c_int, u8p, u8p, sz, u8p]
            lib.zkp_final_exponentiation.argtypes = [u8p, u8p]
            lib.zkp_fq12_product.argtypes = [ctypes.c_int, u8p, sz, u8p]
            for name in ("zkp_zkey_export_vkey", "zkp_verifier_load_vkey_json", "zkp_verifier_load_zkey",
                         "zkp_verifier_info", "zkp_verifier_verify", "zkp_verifier_timings", "zkp_miller_loop",
                         "zkp_final_exponentiation", "zkp_fq12_product"):
                getattr(lib, name).restype = ctypes.c_int
        _lib = lib
        return lib


def _check(st: int):
    if st != ZKP_OK:
        raise ZkpError(st, load_library().zkp_last_error().decode())


def _buf(data):
    """(ctypes uint8 pointer, keepalive) for a bytes-like object, without copying bytes /
    bytearray (witnesses are hundreds of MB; the C side only reads)."""
    if isinstance(data, bytes):
        return ctypes.cast(ctypes.c_char_p(data), ctypes.POINTER(ctypes.c_uint8)), data
    if isinstance(data, bytearray) and len(data):
        arr = (ctypes.c_uint8 * len(data)).from_buffer(data)
        return ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint8)), arr
    data = bytes(data)
    return ctypes.cast(ctypes.c_char_p(data), ctypes.POINTER(ctypes.c_uint8)), data


def _copy_out(ptr, n: int) -> bytes:
    """bytes of a library buffer (ctypes.string_at takes a C int size: > 2 GiB needs a view)."""
    if n < (1 << 31) - 1:
        return ctypes.string_at(ptr, n)
    addr = ctypes.cast(ptr, ctypes.c_void_p).value
    return bytes(memoryview((ctypes.c_uint8 * n).from_address(addr)))


def _le(b) -> int:
    return int.from_bytes(bytes(b), "little")


def version() -> str:
    return load_library().zkp_version().decode()


class Prover:
    """A zkey resident in HBM of one or more devices (loaded once, reused per proof)."""

    def __init__(self, zkey, devices=None, part=None, nparts=None):
        """part / nparts: hold only point slice `part` of `nparts` on devices[0] (the
        point-range split of one proof over several GPUs) -> prove_partial only."""
        lib = load_library()
        h = ctypes.c_void_p()
        devs = list(devices or [])
        darr = (ctypes.c_int * max(1, len(devs)))(*devs) if devs else None
        dptr = ctypes.cast(darr, ctypes.POINTER(ctypes.c_int)) if darr is not None else None
        self.part, self.nparts = (part or 0), (nparts or 1)
        if nparts is not None:
            if hasattr(zkey, "ptr") and hasattr(zkey, "len"):
                _check(lib.zkp_prover_load_part(ctypes.cast(zkey.ptr, ctypes.POINTER(ctypes.c_uint8)), zkey.len,
                                                devs[0] if devs else 0, self.part, self.nparts, ctypes.byref(h)))
            else:
                if not isinstance(zkey, (bytes, bytearray, memoryview)):
                    zkey = open(zkey, "rb").read()
                p, keep = _buf(bytes(zkey))
                _check(lib.zkp_prover_load_part(p, len(zkey), devs[0] if devs else 0, self.part, self.nparts,
                                                ctypes.byref(h)))
                del keep
        elif hasattr(zkey, "ptr") and hasattr(zkey, "len"):  # library-owned buffer (e.g. synth.ZkeyBuffer)
            _check(lib.zkp_prover_load_mem(ctypes.cast(zkey.ptr, ctypes.POINTER(ctypes.c_uint8)), zkey.len, dptr,
                                           len(devs), ctypes.byref(h)))
        elif isinstance(zkey, (bytes, bytearray, memoryview)):
            p, keep = _buf(bytes(zkey))
            _check(lib.zkp_prover_load_mem(p, len(zkey), dptr, len(devs), ctypes.byref(h)))
            del keep
        else:
            _check(lib.zkp_prover_load_file(os.fsencode(zkey), dptr, len(devs), ctypes.byref(h)))
        self._h = h
        nv, npub, dom = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib.zkp_prover_info(h, ctypes.byref(nv), ctypes.byref(npub), ctypes.byref(dom)))
        self.n_vars, self.n_public, self.domain_size = nv.value, npub.value, dom.value

    def close(self):
        if getattr(self, "_h", None):
            load_library().zkp_prover_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _new_proof(self):
        pub = (ctypes.c_uint8 * (32 * max(1, self.n_public)))()
        pr = _Proof()
        pr.public_capacity = self.n_public
        pr.public_signals = ctypes.cast(pub, ctypes.POINTER(ctypes.c_uint8))
        return pr, pub

    @staticmethod
    def _scalar(x):
        if x is None:
            return None, None
        return _buf(int(x).to_bytes(32, "little"))

    def prove_raw(self, wtns: bytes, r=None, s=None):
        """Returns ((ax, ay), ((bx0, bx1), (by0, by1)), (cx, cy)), [public ints]."""
        lib = load_library()
        wp, wk = _buf(wtns)
        rp, rk = self._scalar(r)
        sp, sk = self._scalar(s)
        pr, pub = self._new_proof()
        _check(lib.zkp_prove(self._h, wp, len(wtns), rp, sp, ctypes.byref(pr)))
        return _unpack_proof(pr, pub)

    def prove_batch_raw(self, wtns_list, rs=None, ss=None):
        """All proofs of a batch (raises ZkpError if any proof failed)."""
        res, st = self._batch(wtns_list, rs, ss, raise_first=True)
        return res

    def prove_batch_status_raw(self, wtns_list, rs=None, ss=None):
        """(results, statuses): results[i] is None where statuses[i] != 0 (zkp_prove_batch_status:
        every proof attempted, device failures re-queued to the remaining devices)."""
        return self._batch(wtns_list, rs, ss, raise_first=False)

    def _batch(self, wtns_list, rs, ss, raise_first):
        lib = load_library()
        n = len(wtns_list)
        keep = []
        wps = (ctypes.POINTER(ctypes.c_uint8) * max(1, n))()
        lens = (ctypes.c_size_t * max(1, n))()
        for i, w in enumerate(wtns_list):
            p, k = _buf(w)
            keep.append(k)
            wps[i] = p
            lens[i] = len(w)

        def arr(vals):
            if vals is None:
                return None
            a = (ctypes.POINTER(ctypes.c_uint8) * max(1, n))()
            for i, v in enumerate(vals):
                p, k = _buf(int(v).to_bytes(32, "little"))
                keep.append(k)
                a[i] = p
            return a

        ra, sa = arr(rs), arr(ss)
        proofs = (_Proof * max(1, n))()
        pubs = []
        for i in range(n):
            pub = (ctypes.c_uint8 * (32 * max(1, self.n_public)))()
            pubs.append(pub)
            proofs[i].public_capacity = self.n_public
            proofs[i].public_signals = ctypes.cast(pub, ctypes.POINTER(ctypes.c_uint8))
        st = (ctypes.c_int * max(1, n))()
        rc = lib.zkp_prove_batch_status(self._h, wps, lens, n, ra, sa, proofs, st)
        if rc != ZKP_OK and raise_first:
            _check(rc)
        statuses = [st[i] for i in range(n)]
        return [_unpack_proof(proofs[i], pubs[i]) if statuses[i] == ZKP_OK else None for i in range(n)], statuses

    def prove(self, wtns: bytes, r=None, s=None):
        """snarkjs-shaped result {"proof": {...}, "publicSignals": [...]} (decimal strings)."""
        (a, b, c), pub = self.prove_raw(wtns, r, s)
        return {"proof": proof_object(a, b, c), "publicSignals": [str(x) for x in pub]}

    def quotient(self, wtns: bytes):
        lib = load_library()
        wp, wk = _buf(wtns)
        out = (ctypes.c_uint8 * (32 * self.domain_size))()
        _check(lib.zkp_quotient(self._h, wp, len(wtns), ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
        raw = bytes(out)
        return [_le(raw[32 * i:32 * i + 32]) for i in range(self.domain_size)]

    def timings(self):
        lib = load_library()
        ms = (ctypes.c_float * 11)()
        _check(lib.zkp_prover_timings(self._h, ms, 11))
        keys = ["wtns_h2d", "build_abc", "ntt_quotient", "msm_g1_abc", "msm_g2", "host_assembly", "total_wall",
                "msm_g1_h", "verify", "wtns_pcie_mb", "witness_config"]
        return dict(zip(keys, list(ms)))

    VERIFY_OFF, VERIFY_ALL, VERIFY_BATCH = 0, 1, 2

    def set_verify(self, on=True):
        """Verify-before-return (zkp_prover_set_verify): a checked proof is verified by the host pairing
        against the zkey's verification key; a failing proof raises ZkpError (ZKP_ERR_INTERNAL), or has
        that status in a batch.  True / 1: every proof; False / 0: none; 2 (the default at load): the
        proofs of prove_batch* only."""
        mode = on if isinstance(on, int) and not isinstance(on, bool) else (1 if on else 0)
        _check(load_library().zkp_prover_set_verify(self._h, mode))

    def verify_mode(self) -> int:
        m = ctypes.c_int(-1)
        _check(load_library().zkp_prover_get_verify(self._h, ctypes.byref(m)))
        return m.value

    def stage(self, wtns: bytes, slot: int, dev_index: int = 0):
        wp, wk = _buf(wtns)
        _check(load_library().zkp_witness_stage(self._h, dev_index, slot, wp, len(wtns)))

    def prove_staged_raw(self, slot: int, r=None, s=None, dev_index: int = 0):
        rp, rk = self._scalar(r)
        sp, sk = self._scalar(s)
        pr, pub = self._new_proof()
        _check(load_library().zkp_prove_staged(self._h, dev_index, slot, rp, sp, ctypes.byref(pr)))
        return _unpack_proof(pr, pub)

    def instrument(self, on: bool = True):
        _check(load_library().zkp_prover_instrument(self._h, 1 if on else 0))

    def prove_partial(self, wtns: bytes) -> bytes:
        """This prover's slice of the five MSMs for one witness: a 392-byte zkp_partial."""
        wp, wk = _buf(wtns)
        out = ctypes.create_string_buffer(PARTIAL_BYTES)
        _check(load_library().zkp_prove_partial(self._h, wp, len(wtns), out))
        return out.raw

    def prove_partial_staged(self, slot: int) -> bytes:
        out = ctypes.create_string_buffer(PARTIAL_BYTES)
        _check(load_library().zkp_prove_partial_staged(self._h, slot, out))
        return out.raw

    def quotient_part_staged(self, slot: int, mask: int, dst_ptrs):
        """Distributed quotient, stage 1 (zkp_quotient_part_staged): coset extensions of the
        vectors in mask (bit 0 A, 1 B, 2 C) of the witness staged in `slot`, each copied to
        the device pointer dst_ptrs[v] (domain_size x 32 bytes; None for unselected)."""
        arr = (ctypes.c_void_p * 3)(*[p or None for p in dst_ptrs])
        _check(load_library().zkp_quotient_part_staged(self._h, slot, mask, arr))

    def prove_partial_ext_staged(self, slot: int, abc_ptrs) -> bytes:
        """Distributed quotient, stage 2 (zkp_prove_partial_ext_staged): this slice's
        partial sums with the H scalars joined from device pointers abc_ptrs[0..2] (A, B, C
        at this part's domain slice)."""
        arr = (ctypes.c_void_p * 3)(*abc_ptrs)
        out = ctypes.create_string_buffer(PARTIAL_BYTES)
        _check(load_library().zkp_prove_partial_ext_staged(self._h, slot, arr, out))
        return out.raw

    def msm_config(self):
        out = (ctypes.c_double * 10)()
        _check(load_library().zkp_prover_msm_config(self._h, out, 10))
        v = list(out)
        return {"witness": {"c": int(v[0]), "depth": int(v[1]), "groups": int(v[2])},
                "h": {"c": int(v[3]), "depth": int(v[4]), "groups": int(v[5])},
                "table_bytes_per_device": int(v[6]),
                "witness_second": ({"c": int(v[7]), "depth": int(v[8]), "groups": int(v[9])} if v[7] else None)}

    def kernel_stats(self):
        out = (ctypes.c_double * 8)()
        _check(load_library().zkp_prover_kernel_stats(self._h, out, 8))
        v = list(out)
        return {"g1": {"accumulate_ms": v[0], "launches": int(v[1]), "mixed_adds": int(v[2]), "tasks": int(v[3])},
                "g2": {"accumulate_ms": v[4], "launches": int(v[5]), "mixed_adds": int(v[6]), "tasks": int(v[7])}}

    LAUNCH_KINDS = ("A", "B1", "C", "H", "B2")

    def launch_stats(self):
        """Every instrumented accumulate launch: [{"msm": "A"|"B1"|"C"|"H"|"B2", "adds": n, "ms": t,
        "blocks": workgroups}]."""
        lib = load_library()
        n = ctypes.c_int(0)
        _check(lib.zkp_prover_launch_stats(self._h, None, 0, ctypes.byref(n)))
        cap = n.value
        out = (ctypes.c_double * (4 * max(1, cap)))()
        _check(lib.zkp_prover_launch_stats(self._h, out, cap, ctypes.byref(n)))
        v = list(out)
        # a proof finishing between the two calls grows the record count: read only what fits
        return [{"msm": self.LAUNCH_KINDS[int(v[4 * i])], "adds": int(v[4 * i + 1]), "ms": v[4 * i + 2],
                 "blocks": int(v[4 * i + 3])} for i in range(min(n.value, cap))]

    def prove_files(self, wtns_path, proof_path, public_path):
        _check(load_library().zkp_prove_files(self._h, os.fsencode(wtns_path), os.fsencode(proof_path),
                                              os.fsencode(public_path)))


def _unpack_proof(pr, pub):
    a = (_le(pr.pi_a[0]), _le(pr.pi_a[1]))
    b = ((_le(pr.pi_b[0][0]), _le(pr.pi_b[0][1])), (_le(pr.pi_b[1][0]), _le(pr.pi_b[1][1])))
    c = (_le(pr.pi_c[0]), _le(pr.pi_c[1]))
    raw = bytes(pub)
    signals = [_le(raw[32 * i:32 * i + 32]) for i in range(pr.n_public)]
    return (a, b, c), signals


def proof_object(a, b, c) -> dict:
    """snarkjs proof object (groth16_prove: pi_a, pi_b, pi_c, protocol, curve)."""
    return {
        "pi_a": [str(a[0]), str(a[1]), "1"],
        "pi_b": [[str(b[0][0]), str(b[0][1])], [str(b[1][0]), str(b[1][1])], ["1", "0"]],
        "pi_c": [str(c[0]), str(c[1]), "1"],
        "protocol": "groth16",
        "curve": "bn128",
    }


# ---------------------------------------------------------------- snarkjs-style module API

def _read_input(x) -> bytes:
    if isinstance(x, dict) and x.get("type") == "mem":
        return bytes(x["data"])
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    with open(x, "rb") as f:
        return f.read()


class _Groth16:
    """``groth16.prove`` with a per-process cache of loaded (HBM-resident) zkeys."""

    def __init__(self):
        self._cache = {}
        self._lock = threading.Lock()

    def _prover(self, zkey):
        key = zkey if isinstance(zkey, str) else id(zkey)
        with self._lock:
            p = self._cache.get(key)
            if p is None:
                p = Prover(zkey if isinstance(zkey, str) else _read_input(zkey))
                self._cache[key] = p
            return p

    def prove(self, zkeyFileName, witnessFileName, logger=None, r=None, s=None):
        p = self._prover(zkeyFileName)
        if logger is not None:
            logger.debug("zkp_amd: proving on device (nVars=%d, domain=%d)" % (p.n_vars, p.domain_size))
        return p.prove(_read_input(witnessFileName), r=r, s=s)


groth16 = _Groth16()

PARTIAL_BYTES = 392  # sizeof(zkp_partial)


def proof_combine_raw(zkey, partials, wtns: bytes, r=None, s=None):
    """Host-only: sum the partials (392-byte zkp_partial each, any order) of one split and
    assemble the proof -> same tuple as Prover.prove_raw."""
    lib = load_library()
    blob = b"".join(bytes(p) for p in partials)
    if len(blob) != PARTIAL_BYTES * len(partials):
        raise ValueError("each partial must be %d bytes" % PARTIAL_BYTES)
    if hasattr(zkey, "ptr") and hasattr(zkey, "len"):
        zp, zlen, zk = ctypes.cast(zkey.ptr, ctypes.POINTER(ctypes.c_uint8)), zkey.len, None
    else:
        if not isinstance(zkey, (bytes, bytearray, memoryview)):
            zkey = open(zkey, "rb").read()
        zp, zk = _buf(bytes(zkey))
        zlen = len(zkey)
    wp, wk = _buf(wtns)
    rp, rk = Prover._scalar(r)
    sp, sk = Prover._scalar(s)
    npub = 4096  # public-signal capacity (the Venmo circuit has 26)
    pub = (ctypes.c_uint8 * (32 * npub))()
    pr = _Proof()
    pr.public_capacity = npub
    pr.public_signals = ctypes.cast(pub, ctypes.POINTER(ctypes.c_uint8))
    _check(lib.zkp_proof_combine(zp, zlen, blob, len(partials), wp, len(wtns), rp, sp, ctypes.byref(pr)))
    if pr.n_public > npub:
        raise ZkpError(1, "more than %d public signals" % npub)
    return _unpack_proof(pr, pub)


def read_zkey(path_or_chunks) -> bytes:
    """Decompressed, merged zkey bytes (host only): a path (plain or gzip; else path.gz;
    else the chunks path{a..z}[.gz], the app's circuit.zkey{b..k}.gz) or a list of chunk paths."""
    lib = load_library()
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    if isinstance(path_or_chunks, (list, tuple)):
        arr = (ctypes.c_char_p * len(path_or_chunks))(*[os.fsencode(p) for p in path_or_chunks])
        _check(lib.zkp_zkey_read_chunks(arr, len(path_or_chunks), ctypes.byref(out), ctypes.byref(n)))
    else:
        _check(lib.zkp_zkey_read(os.fsencode(path_or_chunks), ctypes.byref(out), ctypes.byref(n)))
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def _in(buf):
    """(pointer, length, keepalive) of bytes or of a library-owned buffer (synth.ZkeyBuffer: .ptr / .len)."""
    if hasattr(buf, "ptr") and hasattr(buf, "len"):
        return ctypes.cast(buf.ptr, ctypes.POINTER(ctypes.c_uint8)), buf.len, buf
    p, k = _buf(bytes(buf) or b"\0")
    return p, len(buf), k


def zkey_contribute(zkey: bytes, k: int, device: int = 0) -> bytes:
    """Phase-2 contribution math on the GPU: delta -> k*delta (sections 2, 8, 9)."""
    lib = load_library()
    if hasattr(zkey, "ptr") and hasattr(zkey, "len"):  # library-owned buffer (synth.ZkeyBuffer)
        zp, zlen, zk = ctypes.cast(zkey.ptr, ctypes.POINTER(ctypes.c_uint8)), zkey.len, None
    else:
        zp, zk = _buf(zkey)
        zlen = len(zkey)
    kp, kk = _buf(int(k).to_bytes(32, "little"))
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_zkey_contribute(device, zp, zlen, kp, ctypes.byref(out), ctypes.byref(n)))
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def beacon_secret(beacon: bytes, num_iterations_exp: int) -> int:
    """The contribution scalar of `snarkjs zkey beacon <beacon hex> <num_iterations_exp>`
    (host only: chained SHA-256, ChaCha20 stream, Fr.fromRng)."""
    lib = load_library()
    bp, bk = _buf(bytes(beacon) or b"\0")
    k = (ctypes.c_uint8 * 32)()
    _check(lib.zkp_beacon_secret(bp, len(beacon), num_iterations_exp, ctypes.cast(k, ctypes.POINTER(ctypes.c_uint8))))
    return int.from_bytes(bytes(k), "little")


def zkey_beacon(zkey: bytes, beacon: bytes, num_iterations_exp: int, device: int = 0, name=None) -> bytes:
    """`snarkjs zkey beacon <in> <out> <hex> <e> [-n=name]` (zkp_zkey_beacon_named): delta -> k*delta
    with k the beacon's secret on the GPU, the type-1 contribution record appended to section 10."""
    lib = load_library()
    zp, zlen, zk = _in(zkey)
    bp, bk = _buf(bytes(beacon) or b"\0")
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_zkey_beacon_named(device, zp, zlen, bp, len(beacon), num_iterations_exp,
                                     name.encode() if name else None, ctypes.byref(out), ctypes.byref(n)))
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def zkey_contribute_entropy(zkey: bytes, entropy: str, rand64: bytes = None, name=None, device: int = 0) -> bytes:
    """`snarkjs zkey contribute <in> <out> -e=<entropy> [-n=name]` (zkp_zkey_contribute_entropy):
    rand64 = the 64 random bytes mixed with the entropy (None: /dev/urandom; tests pass fixed bytes)."""
    lib = load_library()
    zp, zlen, zk = _in(zkey)
    rp = None
    if rand64 is not None:
        if len(rand64) != 64:
            raise ValueError("rand64 must be 64 bytes")
        rp, rk = _buf(bytes(rand64))
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_zkey_contribute_entropy(device, zp, zlen, rp, entropy.encode(), name.encode() if name else None,
                                           ctypes.byref(out), ctypes.byref(n)))
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def blake2b512(data: bytes) -> bytes:
    """Host-only Blake2b-512 of the C++ MPC code (zkp_blake2b512)."""
    dp, dk = _buf(bytes(data) or b"\0")
    out = (ctypes.c_uint8 * 64)()
    _check(load_library().zkp_blake2b512(dp, len(data), ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    return bytes(out)


def zkey_new(r1cs: bytes, ptau: bytes, device: int = 0) -> bytes:
    """`snarkjs zkey new`: the phase-2 starting key of a circom .r1cs from a prepared .ptau,
    point sections built on the GPU (zkp_zkey_new)."""
    lib = load_library()
    rp, rlen, rk = _in(r1cs)
    pp, plen, pk = _in(ptau)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_zkey_new(device, rp, rlen, pp, plen, ctypes.byref(out), ctypes.byref(n)))
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def ptau_prepare_phase2(ptau: bytes, device: int = 0) -> bytes:
    """`snarkjs powersoftau prepare phase2 <in.ptau> <out.ptau>` (zkp_ptau_prepare_phase2): the ptau with
    its Lagrange sections 12-15, which zkey_new reads; every level is a group inverse FFT on the GPU.
    Sections 1-7 are copied, 12-15 of the input ignored and rebuilt, other ids dropped."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_prepare_phase2(device, pp, plen, ctypes.byref(out), ctypes.byref(n)))
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def ptau_prepare_timings() -> dict:
    """ms of the calling thread's last ptau_prepare_phase2 (zkp_ptau_prepare_timings)."""
    out = (ctypes.c_double * 8)()
    _check(load_library().zkp_ptau_prepare_timings(out, 8))
    keys = ["total", "parse_point_check", "upload", "g1_ifft", "g2_ifft", "affine", "download", "launches"]
    return dict(zip(keys, list(out)))


def group_ifft(points: bytes, log_n: int, g2: bool = False, device: int = 0) -> bytes:
    """Kernel-level (zkp_group_ifft): out_c = n^-1 sum_j w^(-c j) P_j over the n = 2^log_n zkey-layout
    points (w = Fr.w[log_n]), natural order in and out."""
    pb = 128 if g2 else 64
    if log_n < 0 or len(points) != pb << log_n:
        raise ValueError("group_ifft: points must hold 2^log_n points of %d bytes" % pb)
    pp, pk = _buf(points)
    out = (ctypes.c_uint8 * len(points))()
    _check(load_library().zkp_group_ifft(device, 1 if g2 else 0, pp, log_n,
                                         ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    return bytes(out)


def group_fft(points: bytes, log_n: int, g2: bool = False, device: int = 0) -> bytes:
    """Kernel-level (zkp_group_fft): out_c = sum_j w^(c j) P_j over the n = 2^log_n zkey-layout points
    (w = Fr.w[log_n]), natural order in and out, no n^-1: group_ifft(group_fft(x)) == x."""
    pb = 128 if g2 else 64
    if log_n < 0 or len(points) != pb << log_n:
        raise ValueError("group_fft: points must hold 2^log_n points of %d bytes" % pb)
    pp, pk = _buf(points)
    out = (ctypes.c_uint8 * len(points))()
    _check(load_library().zkp_group_fft(device, 1 if g2 else 0, pp, log_n,
                                        ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    return bytes(out)


def _seed(seed):
    if seed is None:
        return None, None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    return _buf(seed)


VERIFY_MSG_CAP = 256


def zkey_verify_frominit(init: bytes, key: bytes, seed: bytes = None, device: int = 0):
    """`snarkjs zkey verify` of `key` against `init`, the key `zkey new` wrote for the same circuit and
    ptau (zkp_zkey_verify_frominit) -> (valid, message): (True, "OK") or (False, the failing check).
    The L / H sections are checked on the GPU.  seed (32 bytes) fixes the coefficients of their linear
    combinations for reproducible tests; production passes None (the OS CSPRNG): the coefficients must
    be unpredictable to whoever wrote the key.  Malformed input raises ZkpError."""
    lib = load_library()
    ip, ilen, ik = _in(init)
    kp, klen, kk = _in(key)
    sp, sk = _seed(seed)
    ok = ctypes.c_int()
    msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
    _check(lib.zkp_zkey_verify_frominit(device, ip, ilen, kp, klen, sp, ctypes.byref(ok), msg, VERIFY_MSG_CAP))
    return bool(ok.value), msg.value.decode()


def zkey_verify(r1cs: bytes, ptau: bytes, key: bytes, seed: bytes = None, device: int = 0):
    """`snarkjs zkey verify <circuit.r1cs> <pot.ptau> <circuit.zkey>` (zkp_zkey_verify): zkey_new on the
    GPU, then zkey_verify_frominit -> (valid, message)."""
    lib = load_library()
    rp, rlen, rk = _in(r1cs)
    pp, plen, pk = _in(ptau)
    kp, klen, kk = _in(key)
    sp, sk = _seed(seed)
    ok = ctypes.c_int()
    msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
    _check(lib.zkp_zkey_verify(device, rp, rlen, pp, plen, kp, klen, sp, ctypes.byref(ok), msg, VERIFY_MSG_CAP))
    return bool(ok.value), msg.value.decode()


def zkey_verify_timings() -> dict:
    """ms of the calling thread's last zkey_verify / zkey_verify_frominit (zkp_zkey_verify_timings)."""
    out = (ctypes.c_double * 12)()
    _check(load_library().zkp_zkey_verify_timings(out, 12))
    keys = ["total", "host_transcript_pairings", "section_compares", "upload", "point_check", "coeff_gen", "plan",
            "accumulate_init", "accumulate_key", "host_fold", "lincomb_wall", "chunks"]
    return dict(zip(keys, list(out)))


class CheckResult:
    """The verdict of a witness check: valid, message ("OK" or "INVALID: ..."), n_bad (the exact number of
    failing constraints), first_bad (the lowest; None if none), bad (the lowest min(16, n_bad), ascending),
    n_constraints.  Truthy when the witness satisfies the circuit."""

    def __init__(self, res: _CheckResult, message: str):
        self.valid = bool(res.valid)
        self.message = message
        self.n_bad = int(res.n_bad)
        self.bad = [int(res.bad[k]) for k in range(min(int(res.n_listed), 16))]
        self.first_bad = int(res.first_bad) if self.n_bad else None
        self.n_constraints = int(res.n_constraints)

    def __bool__(self):
        return self.valid

    def __repr__(self):
        return "CheckResult(valid=%r, message=%r, n_bad=%d, bad=%r)" % (self.valid, self.message, self.n_bad, self.bad)


class WitnessChecker:
    """A circuit's A, B and C matrices (a circom .r1cs) resident on one device: `wtns check` of any number
    of witnesses against it.  A malformed r1cs raises ZkpError before any device work."""

    def __init__(self, r1cs, device: int = 0):
        lib = load_library()
        if not isinstance(r1cs, (bytes, bytearray, memoryview)) and not hasattr(r1cs, "ptr"):
            r1cs = open(r1cs, "rb").read()
        rp, rlen, rk = _in(r1cs)
        h = ctypes.c_void_p()
        _check(lib.zkp_checker_load(device, rp, rlen, ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            load_library().zkp_checker_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        nv, npub, nc = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        nt = ctypes.c_uint64()
        lib = load_library()
        _check(lib.zkp_checker_info(self._h, ctypes.byref(nv), ctypes.byref(npub), ctypes.byref(nc), ctypes.byref(nt)))
        paths = (ctypes.c_uint64 * 2)()
        _check(lib.zkp_checker_paths(self._h, paths, 2))
        return {"n_vars": nv.value, "n_public": npub.value, "n_constraints": nc.value, "n_terms": nt.value,
                "n_long": int(paths[0]), "long_terms": int(paths[1])}

    def check(self, wtns) -> CheckResult:
        """A .wtns file's bytes against the circuit.  A malformed file or one of another length raises
        ZkpError; a witness that fails is a verdict, not an error."""
        wp, wlen, wk = _in(wtns)
        res = _CheckResult()
        msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
        _check(load_library().zkp_checker_check(self._h, wp, wlen, ctypes.byref(res), msg, VERIFY_MSG_CAP))
        return CheckResult(res, msg.value.decode())

    def check_staged(self, prover: "Prover", slot: int, dev_index: int = 0) -> CheckResult:
        """The witness prover.stage() left in `slot`, read in place: stage -> check -> prove_staged."""
        res = _CheckResult()
        msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
        _check(load_library().zkp_checker_check_staged(self._h, prover._h, dev_index, slot, ctypes.byref(res), msg,
                                                       VERIFY_MSG_CAP))
        return CheckResult(res, msg.value.decode())


def wtns_check(r1cs, wtns, device: int = 0) -> CheckResult:
    """`wtns check <circuit.r1cs> <witness.wtns>` in one call (zkp_wtns_check: load, check, free)."""
    rp, rlen, rk = _in(r1cs)
    wp, wlen, wk = _in(wtns)
    res = _CheckResult()
    msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
    _check(load_library().zkp_wtns_check(device, rp, rlen, wp, wlen, ctypes.byref(res), msg, VERIFY_MSG_CAP))
    return CheckResult(res, msg.value.decode())


def wtns_check_timings() -> dict:
    """ms of the calling thread's last wtns_check / WitnessChecker call (zkp_wtns_check_timings)."""
    out = (ctypes.c_double * 5)()
    _check(load_library().zkp_wtns_check_timings(out, 5))
    return dict(zip(["parse_csr", "upload_convert", "witness_copy", "kernels", "total"], list(out)))


def rlc_coeffs(seed: bytes, first_index: int, n: int, device: int = 0):
    """Kernel-level: coefficients first_index .. first_index + n - 1 of a verification seeded with `seed`
    (32 bytes), generated on the GPU (zkp_rlc_coeffs) -> n ints below 2^128."""
    sp, sk = _seed(seed)
    out = (ctypes.c_uint8 * (16 * max(1, n)))()
    _check(load_library().zkp_rlc_coeffs(device, sp, first_index, n, ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    raw = bytes(out)
    return [_le(raw[16 * i:16 * i + 16]) for i in range(n)]


def points_check(points_lem: bytes, g2: bool = False, device: int = 0):
    """Kernel-level: (bad, first_bad) over zkey-layout points (zkp_points_check): how many have a
    coordinate >= p or are neither all-zero nor on the curve, and the smallest such index (None if 0)."""
    pp, pk = _buf(bytes(points_lem) or b"\0")
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    n = len(points_lem) // (128 if g2 else 64)
    _check(load_library().zkp_points_check(device, 1 if g2 else 0, pp, n, ctypes.byref(bad), ctypes.byref(first)))
    return bad.value, (first.value if bad.value else None)


def rlc_g1(seed: bytes, first_index: int, points_a: bytes, points_b: bytes, device: int = 0):
    """Kernel-level: the two linear combinations sum_i coeff(first_index + i) * P_i over two G1 point
    sets of one size under one MSM plan (zkp_rlc_g1) -> ((x, y) or None, (x, y) or None)."""
    if len(points_a) != len(points_b):
        raise ValueError("the two point sets must have one size")
    sp, sk = _seed(seed)
    ap, ak = _buf(bytes(points_a) or b"\0")
    bp, bk = _buf(bytes(points_b) or b"\0")
    oa, ob = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    ia, ib = ctypes.c_int(), ctypes.c_int()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    _check(load_library().zkp_rlc_g1(device, sp, first_index, ap, bp, len(points_a) // 64, ctypes.cast(oa, u8p),
                                     ctypes.byref(ia), ctypes.cast(ob, u8p), ctypes.byref(ib)))

    def pt(raw, inf):
        raw = bytes(raw)
        return None if inf.value else (_le(raw[:32]), _le(raw[32:]))
    return pt(oa, ia), pt(ob, ib)


def ptau_verify_sections(ptau: bytes, seed: bytes = None, device: int = 0):
    """The point sections of `snarkjs powersoftau verify <ptau>` on the GPU (zkp_ptau_verify_sections):
    every point of sections 2-6 and 12-15 on its curve, every G2 point in the subgroup, the singular
    points, the powers and the Lagrange sections -> (valid, message): (True, "OK") or (False, the first
    failing check).  seed as zkey_verify_frominit (production: None).  A malformed file raises ZkpError."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    sp, sk = _seed(seed)
    ok = ctypes.c_int()
    msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
    _check(lib.zkp_ptau_verify_sections(device, pp, plen, sp, ctypes.byref(ok), msg, VERIFY_MSG_CAP))
    return bool(ok.value), msg.value.decode()


def ptau_verify(ptau: bytes, seed: bytes = None, device: int = 0):
    """`snarkjs powersoftau verify <ptau>` (zkp_ptau_verify): the contribution chain of section 7 on the host
    and ptau_verify_sections on the GPU -> (valid, message)."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    sp, sk = _seed(seed)
    ok = ctypes.c_int()
    msg = ctypes.create_string_buffer(VERIFY_MSG_CAP)
    _check(lib.zkp_ptau_verify(device, pp, plen, sp, ctypes.byref(ok), msg, VERIFY_MSG_CAP))
    return bool(ok.value), msg.value.decode()


def ptau_verify_timings() -> dict:
    """ms of the calling thread's last ptau_verify / ptau_verify_sections (zkp_ptau_verify_timings)."""
    out = (ctypes.c_double * 17)()
    _check(load_library().zkp_ptau_verify_timings(out, 17))
    keys = ["total", "parse", "upload", "point_check", "subgroup_check", "coeff_gen", "ntt_scalar_fold", "plan",
            "accumulate_pairs", "accumulate_lagrange", "accumulate_tau", "host_fold", "host_pairings", "chunks",
            "contributions", "first_challenge", "next_challenge"]
    return dict(zip(keys, list(out)))


def _take(lib, out, n) -> bytes:
    try:
        return _copy_out(out, n.value)
    finally:
        lib.zkp_buffer_free(out)


def ptau_new(power: int, ceremony_power: int = 0) -> bytes:
    """`snarkjs powersoftau new bn128 <power>` (zkp_ptau_new; host only): sections 1-7, every point a
    generator, no contribution.  ceremony_power 0: = power."""
    lib = load_library()
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_new(power, ceremony_power, ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def ptau_contribute(ptau: bytes, entropy: str, rand64: bytes = None, name=None, device: int = 0) -> bytes:
    """`snarkjs powersoftau contribute <in> <out> -e=<entropy> [--name=]` (zkp_ptau_contribute): every point of
    sections 2-5 times its own scalar on the GPU, the record appended to section 7.  rand64 = the 64 random
    bytes mixed with the entropy (None: the OS CSPRNG; tests pass fixed bytes).  Sections 12-15 are dropped."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    rp = None
    if rand64 is not None:
        if len(rand64) != 64:
            raise ValueError("rand64 must be 64 bytes")
        rp, rk = _buf(bytes(rand64))
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_contribute(device, pp, plen, rp, entropy.encode(), None if name is None else name.encode(),
                                   ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def ptau_beacon(ptau: bytes, beacon: bytes, num_iterations_exp: int, name=None, device: int = 0) -> bytes:
    """`snarkjs powersoftau beacon <in> <out> <beaconHashHex> <numIterationsExp> [-n=]` (zkp_ptau_beacon)."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    bp, bk = _buf(bytes(beacon) or b"\0")
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_beacon(device, pp, plen, bp, len(beacon), num_iterations_exp,
                               None if name is None else name.encode(), ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def ptau_contribute_timings() -> dict:
    """ms of the calling thread's last ptau_contribute / ptau_beacon (zkp_ptau_contribute_timings)."""
    out = (ctypes.c_double * 12)()
    _check(load_library().zkp_ptau_contribute_timings(out, 12))
    keys = ["total", "parse_point_check", "challenge", "key_draw", "upload", "g1_scale", "g2_scale", "encode", "download",
            "partial_hash", "next_challenge", "chunks"]
    return dict(zip(keys, list(out)))


def points_scale_powers(points_lem: bytes, first: int, ratio: int, g2: bool = False, device: int = 0) -> bytes:
    """Kernel-level (zkp_points_scale_powers): out_i = (first * ratio^i) * P_i over zkey-layout points."""
    pb = 128 if g2 else 64
    if len(points_lem) % pb:
        raise ValueError("points_scale_powers: points of %d bytes each" % pb)
    pp, pk = _buf(bytes(points_lem) or b"\0")
    fp, fk = _buf(int(first).to_bytes(32, "little"))
    rp, rk = _buf(int(ratio).to_bytes(32, "little"))
    out = (ctypes.c_uint8 * max(1, len(points_lem)))()
    _check(load_library().zkp_points_scale_powers(device, 1 if g2 else 0, pp, len(points_lem) // pb, fp, rp,
                                                  ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    return bytes(out)[:len(points_lem)]


def ptau_export_challenge(ptau: bytes, device: int = 0) -> bytes:
    """`snarkjs powersoftau export challenge <in.ptau> <challenge>` (zkp_ptau_export_challenge): the last response
    hash and sections 2-6 uncompressed, 384 * 2^power + 128 bytes.  Its Blake2b-512 is the challenge; a file whose
    sections do not hash to the challenge its section 7 implies raises ZkpError."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_export_challenge(device, pp, plen, ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def ptau_challenge_contribute(challenge: bytes, entropy: str, rand64: bytes = None, device: int = 0) -> bytes:
    """`snarkjs powersoftau challenge contribute bn128 <challenge> <response> -e=<entropy>`
    (zkp_ptau_challenge_contribute): one contribution to a challenge file on the GPU -> the response file (the
    challenge hash, the new sections compressed, the key), 192 * 2^power + 864 bytes.  rand64 as ptau_contribute."""
    lib = load_library()
    cp, clen, ck = _in(challenge)
    rp = None
    if rand64 is not None:
        if len(rand64) != 64:
            raise ValueError("rand64 must be 64 bytes")
        rp, rk = _buf(bytes(rand64))
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_challenge_contribute(device, cp, clen, rp, entropy.encode(), ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def ptau_import_response(ptau: bytes, response: bytes, name=None, device: int = 0) -> bytes:
    """`snarkjs powersoftau import response <old.ptau> <response> <new.ptau> [-n=]` (zkp_ptau_import_response):
    the response's points decompressed on the GPU, a type-0 record appended.  The contribution itself is checked
    by ptau_verify on the result, not here."""
    lib = load_library()
    pp, plen, pk = _in(ptau)
    rp, rlen, rk = _in(response)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_ptau_import_response(device, pp, plen, rp, rlen, None if name is None else name.encode(),
                                        ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def ptau_challenge_timings() -> dict:
    """ms of the calling thread's last export / challenge contribute / import (zkp_ptau_challenge_timings)."""
    out = (ctypes.c_double * 14)()
    _check(load_library().zkp_ptau_challenge_timings(out, 14))
    keys = ["total", "parse_point_check", "challenge_hash", "key", "upload", "decode", "g1_decompress", "g2_decompress",
            "g1_scale", "g2_scale", "encode", "download", "hash_threads", "chunks"]
    return dict(zip(keys, list(out)))


def mpcparams_info(data: bytes) -> dict:
    """Host only (zkp_mpcparams_info): the counts of an MPCParams file, its layout validated (ZkpError
    ZKP_ERR_FORMAT "mpcparams: ..." otherwise)."""
    dp, dlen, dk = _in(data)
    v = [ctypes.c_uint32() for _ in range(4)]
    _check(load_library().zkp_mpcparams_info(dp, dlen, *[ctypes.byref(x) for x in v]))
    return dict(zip(["n_public", "domain_size", "n_vars", "n_contributions"], [x.value for x in v]))


def zkey_export_bellman(zkey: bytes, device: int = 0) -> bytes:
    """`snarkjs zkey export bellman <circuit.zkey> <circuit.mpcparams>` (zkp_zkey_export_bellman): the key as an
    MPCParams file; section 9 goes through the forward group FFT and a coset scaling into the n - 1 points
    delta^-1 tau^i (tau^n - 1) G1."""
    lib = load_library()
    zp, zlen, zk = _in(zkey)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_zkey_export_bellman(device, zp, zlen, ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def zkey_bellman_contribute(challenge: bytes, entropy: str, rand64: bytes = None, device: int = 0, with_hash: bool = False):
    """`snarkjs zkey bellman contribute bn128 <circuit.mpcparams> <response.mpcparams> -e=<entropy>`
    (zkp_zkey_bellman_contribute): one contribution to an MPCParams file on the GPU, drawn as
    zkey_contribute_entropy draws it -> the response file; with_hash: (response, the 64-byte contribution hash)."""
    lib = load_library()
    cp, clen, ck = _in(challenge)
    rp = None
    if rand64 is not None:
        if len(rand64) != 64:
            raise ValueError("rand64 must be 64 bytes")
        rp, rk = _buf(bytes(rand64))
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    h = (ctypes.c_uint8 * 64)()
    _check(lib.zkp_zkey_bellman_contribute(device, cp, clen, rp, entropy.encode(), ctypes.byref(out), ctypes.byref(n),
                                           ctypes.cast(h, ctypes.POINTER(ctypes.c_uint8))))
    res = _take(lib, out, n)
    return (res, bytes(h)) if with_hash else res


def zkey_import_bellman(old_zkey: bytes, response: bytes, name=None, device: int = 0) -> bytes:
    """`snarkjs zkey import bellman <old.zkey> <response.mpcparams> <new.zkey> [-n=]` (zkp_zkey_import_bellman): the
    key that follows old_zkey by the response's contribution.  Its section 9 differs from a direct contribution's
    by a multiple of (w^j)_j, which zkey_verify accepts; the contribution itself is checked by zkey_verify on the
    result, not here."""
    lib = load_library()
    zp, zlen, zk = _in(old_zkey)
    rp, rlen, rk = _in(response)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    _check(lib.zkp_zkey_import_bellman(device, zp, zlen, rp, rlen, None if name is None else name.encode(),
                                       ctypes.byref(out), ctypes.byref(n)))
    return _take(lib, out, n)


def zkey_bellman_timings() -> dict:
    """ms of the calling thread's last export / bellman contribute / import (zkp_zkey_bellman_timings)."""
    out = (ctypes.c_double * 11)()
    _check(load_library().zkp_zkey_bellman_timings(out, 11))
    keys = ["total", "parse", "upload", "decode", "point_check", "scale", "transform", "coset_scale", "encode", "download",
            "chunks"]
    return dict(zip(keys, list(out)))


def _points_to_lem(fn, data: bytes, in_pb: int, out_pb: int, device: int):
    if len(data) % in_pb:
        raise ValueError("points of %d bytes each" % in_pb)
    n = len(data) // in_pb
    pp, pk = _buf(bytes(data) or b"\0")
    out = (ctypes.c_uint8 * max(1, n * out_pb))()
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    _check(fn(device, 1 if out_pb == 128 else 0, pp, n, ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(bad),
              ctypes.byref(first)))
    return bytes(out)[:n * out_pb], bad.value, (first.value if bad.value else None)


def points_decompress(compressed: bytes, g2: bool = False, device: int = 0):
    """Kernel-level (zkp_points_decompress): compressed points -> (zkey-layout bytes, bad, first_bad); a refused
    point (flag misuse, x >= p, x^3 + b a non-residue) is written as zeros."""
    return _points_to_lem(load_library().zkp_points_decompress, compressed, 64 if g2 else 32, 128 if g2 else 64, device)


def points_from_uncompressed(data: bytes, g2: bool = False, device: int = 0):
    """Kernel-level (zkp_points_from_uncompressed): uncompressed points -> (zkey-layout bytes, bad, first_bad);
    refused: a coordinate >= p, 0x40 with anything but zeros beside it.  The curve equation is points_check's."""
    return _points_to_lem(load_library().zkp_points_from_uncompressed, data, 128 if g2 else 64, 128 if g2 else 64, device)


def field_sqrt(elements: bytes, fq2: bool = False, device: int = 0):
    """Kernel-level (zkp_field_sqrt): elements of Fq (32 bytes LE) or Fq2 (c0 then c1) -> (roots in the same form
    or zeros, is_square bytes)."""
    eb = 64 if fq2 else 32
    if len(elements) % eb:
        raise ValueError("elements of %d bytes each" % eb)
    n = len(elements) // eb
    pp, pk = _buf(bytes(elements) or b"\0")
    out = (ctypes.c_uint8 * max(1, n * eb))()
    sq = (ctypes.c_uint8 * max(1, n))()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    _check(load_library().zkp_field_sqrt(device, 1 if fq2 else 0, pp, n, ctypes.cast(out, u8p), ctypes.cast(sq, u8p)))
    return bytes(out)[:n * eb], bytes(sq)[:n]


def g2_subgroup_check(points_lem: bytes, device: int = 0):
    """Kernel-level: (bad, first_bad) over zkey-layout G2 points on the curve (zkp_g2_subgroup_check): how
    many are neither all-zero nor of order r, and the smallest such index (None if 0)."""
    pp, pk = _buf(bytes(points_lem) or b"\0")
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    _check(load_library().zkp_g2_subgroup_check(device, pp, len(points_lem) // 128, ctypes.byref(bad),
                                                ctypes.byref(first)))
    return bad.value, (first.value if bad.value else None)


def rlc_pairs(seed: bytes, first_index: int, points: bytes, g2: bool = False, device: int = 0):
    """Kernel-level: A = sum_{i<n-1} r_i P_i and B = sum_{i<n-1} r_i P_(i+1) over n zkey-layout points
    under one MSM plan, r_i = coefficient first_index + i (zkp_rlc_pairs) -> (A, B), each a point
    ((x, y); G2: ((x0, x1), (y0, y1))) or None for infinity."""
    pb = 128 if g2 else 64
    sp, sk = _seed(seed)
    pp, pk = _buf(bytes(points) or b"\0")
    oa, ob = (ctypes.c_uint8 * pb)(), (ctypes.c_uint8 * pb)()
    ia, ib = ctypes.c_int(), ctypes.c_int()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    _check(load_library().zkp_rlc_pairs(device, 1 if g2 else 0, sp, first_index, pp, len(points) // pb,
                                        ctypes.cast(oa, u8p), ctypes.byref(ia), ctypes.cast(ob, u8p), ctypes.byref(ib)))

    def pt(raw, inf):
        v = [_le(bytes(raw)[32 * i:32 * i + 32]) for i in range(pb // 32)]
        if inf.value:
            return None
        return ((v[0], v[1]), (v[2], v[3])) if g2 else (v[0], v[1])
    return pt(oa, ia), pt(ob, ib)


def _proof_struct(proof, public_signals):
    (a, b, c) = proof
    pr = _Proof()
    for i in range(2):
        pr.pi_a[i][:] = int(a[i]).to_bytes(32, "little")
        pr.pi_c[i][:] = int(c[i]).to_bytes(32, "little")
        for j in range(2):
            pr.pi_b[i][j][:] = int(b[i][j]).to_bytes(32, "little")
    pub = b"".join(int(x).to_bytes(32, "little") for x in public_signals) or bytes(32)
    pbuf = (ctypes.c_uint8 * len(pub)).from_buffer_copy(pub)
    pr.n_public = pr.public_capacity = len(public_signals)
    pr.public_signals = ctypes.cast(pbuf, ctypes.POINTER(ctypes.c_uint8))
    return pr, pbuf


def proof_verify(zkey, proof, public_signals) -> bool:
    """Host-only `snarkjs groth16 verify` (zkp_proof_verify) of a proof tuple
    ((ax, ay), ((bx0, bx1), (by0, by1)), (cx, cy)) against a zkey's verification key."""
    if hasattr(zkey, "ptr") and hasattr(zkey, "len"):
        zp, zlen, zk = ctypes.cast(zkey.ptr, ctypes.POINTER(ctypes.c_uint8)), zkey.len, None
    else:
        zp, zk = _buf(bytes(zkey))
        zlen = len(zkey)
    pr, keep = _proof_struct(proof, public_signals)
    ok = ctypes.c_int()
    _check(load_library().zkp_proof_verify(zp, zlen, ctypes.byref(pr), ctypes.byref(ok)))
    return bool(ok.value)


def pairing(g1, g2):
    """Host-only BN254 pairing e(P, Q) in snarkjs' GT convention (zkp_pairing): P = (x, y),
    Q = ((x.c0, x.c1), (y.c0, y.c1)), None = infinity -> 6 x (c0, c1) ints in snarkjs' nesting."""
    gb = bytes(64) if g1 is None else b"".join(int(v).to_bytes(32, "little") for v in g1)
    qb = bytes(128) if g2 is None else b"".join(int(v).to_bytes(32, "little")
                                               for v in (g2[0][0], g2[0][1], g2[1][0], g2[1][1]))
    gp, gk = _buf(gb)
    qp, qk = _buf(qb)
    out = (ctypes.c_uint8 * 384)()
    _check(load_library().zkp_pairing(gp, qp, ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    raw = bytes(out)
    v = [_le(raw[32 * i:32 * i + 32]) for i in range(12)]
    return [[(v[6 * h + 2 * k], v[6 * h + 2 * k + 1]) for k in range(3)] for h in range(2)]


def _f12_nested(raw: bytes):
    v = [_le(raw[32 * i:32 * i + 32]) for i in range(12)]
    return [[(v[6 * h + 2 * k], v[6 * h + 2 * k + 1]) for k in range(3)] for h in range(2)]


def _f12_bytes(f) -> bytes:
    return b"".join(int(c).to_bytes(32, "little") for h in f for k in h for c in k)


def _g1_bytes(p) -> bytes:
    return bytes(64) if p is None else b"".join(int(v).to_bytes(32, "little") for v in p)


def _g2_bytes(q) -> bytes:
    return bytes(128) if q is None else b"".join(int(v).to_bytes(32, "little")
                                                 for v in (q[0][0], q[0][1], q[1][0], q[1][1]))


def miller_loop(pairs, device: int = 0):
    """The device Miller loop (zkp_miller_loop) of every (P, Q) of `pairs`, points as `pairing` takes them.
    Each value equals the host's Miller value only up to a factor that the final exponentiation removes:
    final_exponentiation(miller_loop([(P, Q)])[0]) == pairing(P, Q)."""
    pairs = list(pairs)
    n = len(pairs)
    gp, gk = _buf(b"".join(_g1_bytes(p) for p, _ in pairs) or bytes(1))
    qp, qk = _buf(b"".join(_g2_bytes(q) for _, q in pairs) or bytes(1))
    out = (ctypes.c_uint8 * max(384 * n, 1))()
    _check(load_library().zkp_miller_loop(device, gp, qp, n, ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    raw = bytes(out)
    return [_f12_nested(raw[384 * i:384 * i + 384]) for i in range(n)]


def final_exponentiation(f):
    """Host final exponentiation (zkp_final_exponentiation) of an Fq12 value in `pairing`'s nesting."""
    ip, ik = _buf(_f12_bytes(f))
    out = (ctypes.c_uint8 * 384)()
    _check(load_library().zkp_final_exponentiation(ip, ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    return _f12_nested(bytes(out))


def fq12_product(values, device: int = 0):
    """Product of Fq12 values by the device reduction kernel (zkp_fq12_product); [] gives 1."""
    values = list(values)
    ip, ik = _buf(b"".join(_f12_bytes(f) for f in values) or bytes(1))
    out = (ctypes.c_uint8 * 384)()
    _check(load_library().zkp_fq12_product(device, ip, len(values), ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))))
    return _f12_nested(bytes(out))


def export_verification_key_text(zkey) -> str:
    """`snarkjs zkey export verificationkey`: the JSON text (zkp_zkey_export_vkey)."""
    lib = load_library()
    zp, zk = _buf(zkey)
    need = ctypes.c_size_t()
    _check(lib.zkp_zkey_export_vkey(zp, len(zkey), None, 0, ctypes.byref(need)))
    buf = ctypes.create_string_buffer(need.value)
    _check(lib.zkp_zkey_export_vkey(zp, len(zkey), buf, need.value, ctypes.byref(need)))
    return buf.value.decode()


def export_verification_key(zkey) -> dict:
    """`snarkjs zkey export verificationkey` as the parsed object."""
    import json
    return json.loads(export_verification_key_text(zkey))


def _proof_tuple(proof):
    """snarkjs' proof object (pi_a / pi_b / pi_c decimal strings) or the ((ax, ay), ((bx0, bx1), (by0, by1)),
    (cx, cy)) tuple -> the tuple"""
    if isinstance(proof, dict):
        a, b, c = proof["pi_a"], proof["pi_b"], proof["pi_c"]
        return ((int(a[0]), int(a[1])), ((int(b[0][0]), int(b[0][1])), (int(b[1][0]), int(b[1][1]))),
                (int(c[0]), int(c[1])))
    return proof


class Verifier:
    """`snarkjs groth16 verify` from a verification key, batched, with the per-proof Miller loops on the GPU
    (zkp_verifier_*).  vkey_or_zkey: the verification key as a dict, its JSON text (str), or the bytes of a
    .zkey (the key of its sections 2 and 3)."""

    def __init__(self, vkey_or_zkey, device: int = 0):
        import json
        lib = load_library()
        self._lib = lib
        self._h = ctypes.c_void_p()
        if isinstance(vkey_or_zkey, dict):
            vkey_or_zkey = json.dumps(vkey_or_zkey)
        if isinstance(vkey_or_zkey, str):
            text = vkey_or_zkey.encode()
            _check(lib.zkp_verifier_load_vkey_json(device, text, len(text), ctypes.byref(self._h)))
        else:
            zp, zk = _buf(vkey_or_zkey)
            _check(lib.zkp_verifier_load_zkey(device, zp, len(vkey_or_zkey), ctypes.byref(self._h)))
        n = ctypes.c_uint32()
        _check(lib.zkp_verifier_info(self._h, ctypes.byref(n)))
        self.n_public = n.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.zkp_verifier_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify_batch(self, items, seed=None):
        """items: (proof, public_signals) pairs -> one bool each.  seed: 32 bytes for tests; None (what a
        production call passes) draws it from the OS CSPRNG."""
        items = list(items)
        n = len(items)
        arr = (_Proof * max(n, 1))()
        keep = []
        for i, (proof, pub) in enumerate(items):
            pr, pbuf = _proof_struct(_proof_tuple(proof), [int(x) for x in pub])
            keep.append(pbuf)
            ctypes.memmove(ctypes.byref(arr, i * ctypes.sizeof(_Proof)), ctypes.byref(pr), ctypes.sizeof(_Proof))
        valid = (ctypes.c_uint8 * max(n, 1))()
        n_valid = ctypes.c_size_t()
        sp = None
        if seed is not None:
            if len(seed) != 32:
                raise ValueError("seed: 32 bytes")
            sp, sk = _buf(bytes(seed))
        _check(self._lib.zkp_verifier_verify(self._h, arr, n, sp, ctypes.cast(valid, ctypes.POINTER(ctypes.c_uint8)),
                                             ctypes.byref(n_valid)))
        out = [bool(valid[i]) for i in range(n)]
        assert n_valid.value == sum(out)
        return out

    def verify(self, proof, public_signals) -> bool:
        return self.verify_batch([(proof, public_signals)])[0]

    def timings(self) -> dict:
        ms = (ctypes.c_double * 9)()
        _check(self._lib.zkp_verifier_timings(ms, 9))
        keys = ("gates_ms", "scalar_ms", "miller_ms", "product_ms", "host_miller_ms", "final_exp_ms", "search_ms",
                "total_ms", "node_checks")
        return dict(zip(keys, list(ms)))


def solidity_calldata(proof, public_signals) -> str:
    """`snarkjs zkey export soliditycalldata` text via the C ABI (zkp_proof_calldata).
    proof: ((ax, ay), ((bx0, bx1), (by0, by1)), (cx, cy)) as from Prover.prove_raw."""
    (a, b, c) = proof
    pr = _Proof()
    for i in range(2):
        pr.pi_a[i][:] = int(a[i]).to_bytes(32, "little")
        pr.pi_c[i][:] = int(c[i]).to_bytes(32, "little")
        for j in range(2):
            pr.pi_b[i][j][:] = int(b[i][j]).to_bytes(32, "little")
    pub = b"".join(int(x).to_bytes(32, "little") for x in public_signals) or bytes(32)
    pbuf = (ctypes.c_uint8 * len(pub)).from_buffer_copy(pub)
    pr.n_public = pr.public_capacity = len(public_signals)
    pr.public_signals = ctypes.cast(pbuf, ctypes.POINTER(ctypes.c_uint8))
    need = ctypes.c_size_t()
    lib = load_library()
    _check(lib.zkp_proof_calldata(ctypes.byref(pr), None, 0, ctypes.byref(need)))
    out = ctypes.create_string_buffer(need.value)
    _check(lib.zkp_proof_calldata(ctypes.byref(pr), out, need.value, ctypes.byref(need)))
    return out.value.decode()


def partial_from_points(a, b1, c, h, b2, part: int, nparts: int) -> bytes:
    """Encode affine partial sums (oracle tuples, None = infinity) as a zkp_partial."""
    def g1(p):
        return bytes(64) if p is None else int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little")

    def g2(p):
        if p is None:
            return bytes(128)
        return b"".join(int(v).to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))
    return g1(a) + g1(b1) + g1(c) + g1(h) + g2(b2) + int(part).to_bytes(4, "little") + int(nparts).to_bytes(4, "little")


def _msm(points_lem, scalars_le, g2, device, window_bits, table_depth):
    lib = load_library()
    n = len(scalars_le) // 32
    pp, pk = _buf(points_lem)
    sp, sk = _buf(scalars_le)
    out = (ctypes.c_uint8 * 128)()
    inf = ctypes.c_int()
    o = ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))
    if window_bits or table_depth:
        _check(lib.zkp_msm(device, 1 if g2 else 0, pp, sp, n, window_bits, table_depth, o, ctypes.byref(inf)))
    elif g2:
        _check(lib.zkp_msm_g2(device, pp, sp, n, o, ctypes.byref(inf)))
    else:
        _check(lib.zkp_msm_g1(device, pp, sp, n, o, ctypes.byref(inf)))
    if inf.value:
        return None
    raw = bytes(out)
    v = [_le(raw[32 * i:32 * i + 32]) for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3])) if g2 else (v[0], v[1])


def msm_g1(points_lem: bytes, scalars_le: bytes, device: int = 0, window_bits: int = 0, table_depth: int = 0):
    """Kernel-level G1 MSM: zkey-layout points, 32-byte LE scalars -> affine (x, y) or None.
    window_bits / table_depth: Pippenger parameters (0 = automatic, as the prover)."""
    return _msm(points_lem, scalars_le, False, device, window_bits, table_depth)


def msm_g2(points_lem: bytes, scalars_le: bytes, device: int = 0, window_bits: int = 0, table_depth: int = 0):
    """Kernel-level G2 MSM -> ((x.c0, x.c1), (y.c0, y.c1)) or None."""
    return _msm(points_lem, scalars_le, True, device, window_bits, table_depth)


def ntt_fr(values, mode: int, device: int = 0):
    """mode 0 forward, 1 inverse, 2 coset-extend (snarkjs ifft -> applyKey -> fft)."""
    lib = load_library()
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    arr = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
    _check(lib.zkp_ntt_fr(device, ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint8)), len(values), mode))
    out = bytes(arr)
    return [_le(out[32 * i:32 * i + 32]) for i in range(len(values))]


def ntt_fr_bytes(raw, mode: int, device: int = 0) -> bytes:
    """As ntt_fr on len(raw) // 32 standard-form LE values (< r) given as bytes; returns bytes of the same
    layout (no per-element Python integers: the 2^20 / 2^23 parity tests)."""
    lib = load_library()
    arr = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
    _check(lib.zkp_ntt_fr(device, ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint8)), len(raw) // 32, mode))
    return bytes(arr)


def bench_msm(points_lem: bytes, scalars_le: bytes, g2: bool = False, warmup: int = 2, iters: int = 10,
              device: int = 0):
    """Device-resident MSM timing (HIP events on the engine stream).  Returns (stats dict, result)."""
    lib = load_library()
    n = len(scalars_le) // 32
    pp, pk = _buf(points_lem)
    sp, sk = _buf(scalars_le)
    st = (ctypes.c_double * 8)()
    out = (ctypes.c_uint8 * 128)()
    inf = ctypes.c_int()
    ext = hasattr(lib, "zkp_bench_msm_ex")  # an older library (A/B runs) has the 6-stat form only
    if ext:
        _check(lib.zkp_bench_msm_ex(device, 1 if g2 else 0, pp, sp, n, warmup, iters, st, 8,
                                    ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(inf)))
    else:
        _check(lib.zkp_bench_msm(device, 1 if g2 else 0, pp, sp, n, warmup, iters, st,
                                 ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(inf)))
    raw = bytes(out)
    if inf.value:
        res = None
    elif g2:
        v = [_le(raw[32 * i:32 * i + 32]) for i in range(4)]
        res = ((v[0], v[1]), (v[2], v[3]))
    else:
        res = (_le(raw[:32]), _le(raw[32:64]))
    stats = {"ms_per_msm": st[0], "ms_accumulate": st[1], "mixed_adds": int(st[2]), "tasks": int(st[3]),
             "c": int(st[4]), "windows": int(st[5]), "table_build_ms": st[6] if ext else None,
             "table_depth": int(st[7]) if ext else None}
    return stats, res


def bench_plan(scalars_le: bytes, window_bits: int = 0, dense: bool = True, warmup: int = 2, iters: int = 10,
               device: int = 0) -> float:
    """ms per MSM plan build (digits + bucket grouping + task offsets), device-resident scalars."""
    ms = ctypes.c_double()
    sp, sk = _buf(scalars_le)
    _check(load_library().zkp_bench_plan(device, sp, len(scalars_le) // 32, window_bits, 1 if dense else 0, warmup,
                                         iters, ctypes.byref(ms)))
    return ms.value


def bench_ntt(log_n: int, warmup: int = 2, iters: int = 10, device: int = 0, count: int = 1) -> float:
    """ms per coset extension of `count` (1..3) vectors of 2^log_n elements, every pass one launch
    over all of them (count 3 is the prover's A, B, C)."""
    ms = ctypes.c_double()
    if count == 1:
        _check(load_library().zkp_bench_ntt(device, log_n, warmup, iters, ctypes.byref(ms)))
    else:
        _check(load_library().zkp_bench_ntt_batch(device, log_n, count, warmup, iters, ctypes.byref(ms)))
    return ms.value
