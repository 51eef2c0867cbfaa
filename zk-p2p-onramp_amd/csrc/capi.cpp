// C ABI of libzkp_amd.so (include/zkp_amd.h).  Every entry point catches all C++
// exceptions and turns them into a zkp_status plus a thread-local message.
#include <stdexcept>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/zkp_amd.h"
#include "beacon.hpp"
#include "device_pipeline.hpp"
#include "groth16_verify.hpp"
#include "hip_check.hpp"
#include "host_ec.hpp"
#include "host_pairing.hpp"
#include "mpc.hpp"
#include "prover.hpp"
#include "ptau_challenge.hpp"
#include "ptau_contribute.hpp"
#include "ptau_verify.hpp"
#include "wtns_check.hpp"
#include "zkey_bellman.hpp"
#include "zkey_io.hpp"
#include "zkey_verify.hpp"

static_assert(sizeof(zkp_partial) == 392, "zkp_partial is exchanged as 392 raw bytes");

struct zkp_prover {
  zkp::Prover* impl;
};

struct zkp_verifier {
  std::unique_ptr<zkp::Verifier> impl;
};

namespace {

thread_local std::string g_err;

zkp_status fail(zkp_status s, const std::string& m) {
  g_err = m;
  return s;
}

template <class Fn>
zkp_status guard(Fn&& fn) {
  try {
    g_err.clear();
    fn();
    return ZKP_OK;
  } catch (const zkp::ZkpError& e) {
    return fail(e.status, e.what());
  } catch (const zkp::HipError& e) {
    if (e.code == hipErrorOutOfMemory) return fail(ZKP_ERR_OUT_OF_MEMORY, e.what());
    return fail(ZKP_ERR_DEVICE, e.what());
  } catch (const std::bad_alloc&) {
    return fail(ZKP_ERR_OUT_OF_MEMORY, "host out of memory");
  } catch (const std::invalid_argument& e) {
    return fail(ZKP_ERR_INVALID_ARG, e.what());
  } catch (const std::exception& e) {
    return fail(ZKP_ERR_INTERNAL, e.what());
  } catch (...) {
    return fail(ZKP_ERR_INTERNAL, "unknown error");
  }
}

std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw zkp::ZkpError(ZKP_ERR_IO, std::string("cannot open ") + path);
  const std::streamsize n = f.tellg();
  f.seekg(0);
  std::vector<uint8_t> buf((size_t)n);
  if (n && !f.read(reinterpret_cast<char*>(buf.data()), n))
    throw zkp::ZkpError(ZKP_ERR_IO, std::string("cannot read ") + path);
  return buf;
}

// A witness file mapped read-only: the prover's transfer threads read the page cache directly (the
// page faults spread over them) instead of one thread copying 205 MB into a zero-filled buffer
// first.  Regular files only; anything else (a pipe, a device, a procfs node) and a file that cannot
// be mapped is read into a buffer (read_file).  A mapped file must not be truncated by another writer
// while the call runs (the read of a page past the new end would raise SIGBUS): include/zkp_amd.h
// states this for zkp_prove_files.
class MappedFile {
 public:
  explicit MappedFile(const char* path) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) throw zkp::ZkpError(ZKP_ERR_IO, std::string("cannot open ") + path);
    struct stat st {};
    if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
      void* m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) {
        map_ = m;
        len_ = (size_t)st.st_size;
      }
    }
    ::close(fd);
    if (!map_) copy_ = read_file(path);
  }
  ~MappedFile() {
    if (map_) ::munmap(map_, len_);
  }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
  const uint8_t* data() const { return map_ ? static_cast<const uint8_t*>(map_) : copy_.data(); }
  size_t size() const { return map_ ? len_ : copy_.size(); }

 private:
  void* map_ = nullptr;
  size_t len_ = 0;
  std::vector<uint8_t> copy_;
};

std::string dec(const uint8_t* le32) { return zkp::host::u256_to_dec(zkp::host::u256_from_le(le32)); }

// JSON.stringify(obj, null, 1) of snarkjs' proof object (key order pi_a, pi_b, pi_c, protocol, curve)
std::string proof_json(const zkp_proof* p) {
  std::string s = "{\n \"pi_a\": [\n  \"" + dec(p->pi_a[0]) + "\",\n  \"" + dec(p->pi_a[1]) + "\",\n  \"1\"\n ],\n";
  s += " \"pi_b\": [\n  [\n   \"" + dec(p->pi_b[0][0]) + "\",\n   \"" + dec(p->pi_b[0][1]) + "\"\n  ],\n  [\n   \"" +
       dec(p->pi_b[1][0]) + "\",\n   \"" + dec(p->pi_b[1][1]) + "\"\n  ],\n  [\n   \"1\",\n   \"0\"\n  ]\n ],\n";
  s += " \"pi_c\": [\n  \"" + dec(p->pi_c[0]) + "\",\n  \"" + dec(p->pi_c[1]) + "\",\n  \"1\"\n ],\n";
  s += " \"protocol\": \"groth16\",\n \"curve\": \"bn128\"\n}";
  return s;
}

std::string public_json(const zkp_proof* p) {
  const uint32_t n = std::min(p->n_public, p->public_capacity);
  if (n == 0 || !p->public_signals) return "[]";
  std::string s = "[\n";
  for (uint32_t i = 0; i < n; ++i) {
    s += " \"" + dec(p->public_signals + 32 * i) + "\"";
    s += (i + 1 < n) ? ",\n" : "\n";
  }
  s += "]";
  return s;
}

// "0x" + 64 hex digits of a 32-byte LE integer, quoted (snarkjs p256)
std::string p256(const uint8_t* le32) {
  static const char* hx = "0123456789abcdef";
  std::string s = "\"0x";
  for (int i = 31; i >= 0; --i) {
    s += hx[le32[i] >> 4];
    s += hx[le32[i] & 15];
  }
  return s + "\"";
}

// snarkjs 0.4.22 `zkey export soliditycalldata` (G2 pairs in EIP-197 [c1, c0] order)
std::string calldata(const zkp_proof* p) {
  std::string s = "[" + p256(p->pi_a[0]) + ", " + p256(p->pi_a[1]) + "],";
  s += "[[" + p256(p->pi_b[0][1]) + ", " + p256(p->pi_b[0][0]) + "],[" + p256(p->pi_b[1][1]) + ", " +
       p256(p->pi_b[1][0]) + "]],";
  s += "[" + p256(p->pi_c[0]) + ", " + p256(p->pi_c[1]) + "],[";
  const uint32_t n = std::min(p->n_public, p->public_capacity);
  for (uint32_t i = 0; i < n && p->public_signals; ++i) {
    if (i) s += ",";
    s += p256(p->public_signals + 32 * i);
  }
  return s + "]";
}

zkp_status emit(const std::string& s, char* buf, size_t cap, size_t* needed) {
  if (needed) *needed = s.size() + 1;
  if (buf && cap >= s.size() + 1) {
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return ZKP_OK;
  }
  if (buf) return fail(ZKP_ERR_INVALID_ARG, "buffer too small");
  return ZKP_OK;
}

void write_file(const char* path, const std::string& s) {
  std::ofstream f(path, std::ios::binary);
  if (!f || !f.write(s.data(), (std::streamsize)s.size())) throw zkp::ZkpError(ZKP_ERR_IO, std::string("cannot write ") + path);
}

std::vector<int> dev_list(const int* devices, int ndev) {
  std::vector<int> v;
  if (devices)
    for (int i = 0; i < ndev; ++i) v.push_back(devices[i]);
  return v;
}

}  // namespace

extern "C" {

zkp_status zkp_prover_load_mem(const uint8_t* zkey, size_t len, const int* devices, int ndev, zkp_prover** out) {
  if (!zkey || !out || ndev < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  return guard([&] {
    auto* h = new zkp_prover{nullptr};
    try {
      h->impl = new zkp::Prover(zkey, len, dev_list(devices, ndev));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

zkp_status zkp_prover_load_file(const char* path, const int* devices, int ndev, zkp_prover** out) {
  if (!path || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::read_zkey_source(path); });
  if (s != ZKP_OK) return s;
  return zkp_prover_load_mem(buf.data(), buf.size(), devices, ndev, out);
}

zkp_status zkp_prover_load_chunks(const char* const* paths, int n, const int* devices, int ndev, zkp_prover** out) {
  if (!paths || n < 1 || !out) return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::read_zkey_chunks(std::vector<std::string>(paths, paths + n)); });
  if (s != ZKP_OK) return s;
  return zkp_prover_load_mem(buf.data(), buf.size(), devices, ndev, out);
}

static zkp_status hand_out(std::vector<uint8_t>&& v, uint8_t** out, size_t* len) {
  *out = static_cast<uint8_t*>(std::malloc(std::max<size_t>(v.size(), 1)));
  if (!*out) return fail(ZKP_ERR_OUT_OF_MEMORY, "host out of memory");
  std::memcpy(*out, v.data(), v.size());
  *len = v.size();
  return ZKP_OK;
}

zkp_status zkp_zkey_read(const char* path, uint8_t** out, size_t* len) {
  if (!path || !out || !len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::read_zkey_source(path); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, len);
}

zkp_status zkp_zkey_read_chunks(const char* const* paths, int n, uint8_t** out, size_t* len) {
  if (!paths || n < 1 || !out || !len) return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::read_zkey_chunks(std::vector<std::string>(paths, paths + n)); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, len);
}

void zkp_buffer_free(uint8_t* p) { std::free(p); }

zkp_status zkp_zkey_contribute(int device, const uint8_t* zkey, size_t len, const uint8_t* k32, uint8_t** out,
                               size_t* out_len) {
  if (!zkey || !k32 || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::zkey_apply_delta(device, zkey, len, k32); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_beacon_secret(const uint8_t* beacon, size_t len, uint32_t num_iterations_exp, uint8_t* k32) {
  if ((!beacon && len) || !k32) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::beacon_secret(beacon, len, num_iterations_exp, k32); });
}

}  // extern "C"

namespace {
// snarkjs misc.getRandomRng seeded as `contribute -e=<entropy>` seeds it: Blake2b(64 random bytes || entropy)
zkp::ChaChaRng entropy_rng(const uint8_t* rand64, const char* entropy) {
  uint8_t rnd[64];
  if (rand64)
    std::memcpy(rnd, rand64, 64);
  else
    zkp::os_random(rnd, 64);
  zkp::Blake2b hh;
  hh.update(rnd, 64);
  hh.update(entropy, std::strlen(entropy));
  uint8_t d[64];
  hh.final(d);
  uint32_t seed[8];
  zkp::seed_from_hash(d, seed);
  return zkp::ChaChaRng(seed);
}

// one phase-2 contribution drawn from rng: the record appended to section 10 (mpc.cpp), then the
// group arithmetic on the GPU (delta -> k delta, L and H -> k^-1) and the new section 10
std::vector<uint8_t> contribute_mpc(int device, const uint8_t* zkey, size_t len, zkp::ChaChaRng& rng, uint32_t type,
                                    const char* name, const uint8_t* beacon, size_t beacon_len, uint32_t e) {
  const zkp::ZkeyParsed z = zkp::parse_zkey(zkey, len, false);
  const zkp::Section& s10 = z.bf.sec[10];
  if (!s10.ptr) throw zkp::ZkpError(ZKP_ERR_FORMAT, "zkey: missing section 10 (MPC parameters)");
  zkp::MpcParams m = zkp::read_mpc(s10.ptr, s10.len);
  uint8_t k[32];
  zkp::mpc_contribute(m, rng, z.hdr.delta1, type, name ? std::string(name) : std::string(), beacon, beacon_len, e, k);
  std::vector<uint8_t> buf = zkp::zkey_apply_delta(device, zkey, len, k);
  zkp::binfile_replace_section(buf, 10, zkp::write_mpc(m));
  return buf;
}
}  // namespace
extern "C" {

zkp_status zkp_zkey_beacon_named(int device, const uint8_t* zkey, size_t len, const uint8_t* beacon, size_t beacon_len,
                                 uint32_t num_iterations_exp, const char* name, uint8_t** out, size_t* out_len) {
  if (!zkey || (!beacon && beacon_len) || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] {
    uint8_t h[32];
    zkp::beacon_hash(beacon, beacon_len, num_iterations_exp, h);
    uint32_t seed[8];
    zkp::seed_from_hash(h, seed);
    zkp::ChaChaRng rng(seed);
    buf = contribute_mpc(device, zkey, len, rng, 1, name, beacon, beacon_len, num_iterations_exp);
  });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_zkey_beacon(int device, const uint8_t* zkey, size_t len, const uint8_t* beacon, size_t beacon_len,
                           uint32_t num_iterations_exp, uint8_t** out, size_t* out_len) {
  return zkp_zkey_beacon_named(device, zkey, len, beacon, beacon_len, num_iterations_exp, nullptr, out, out_len);
}

zkp_status zkp_zkey_contribute_entropy(int device, const uint8_t* zkey, size_t len, const uint8_t* rand64,
                                       const char* entropy, const char* name, uint8_t** out, size_t* out_len) {
  if (!zkey || !entropy || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] {
    zkp::ChaChaRng rng = entropy_rng(rand64, entropy);
    buf = contribute_mpc(device, zkey, len, rng, 0, name, nullptr, 0, 0);
  });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_blake2b512(const uint8_t* data, size_t len, uint8_t* out64) {
  if ((!data && len) || !out64) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    zkp::Blake2b h;
    h.update(data, len);
    h.final(out64);
  });
}

zkp_status zkp_zkey_new(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                        uint8_t** out, size_t* out_len) {
  if (!r1cs || !ptau || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::zkey_new(device, r1cs, r1cs_len, ptau, ptau_len); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

}  // extern "C"

namespace {
thread_local zkp::VerifyTimings g_verify_timings;

// the verdict's message into the caller's buffer (truncated to msg_cap - 1 characters)
void put_msg(const std::string& m, char* msg, size_t msg_cap) {
  if (!msg || !msg_cap) return;
  const size_t n = std::min(m.size(), msg_cap - 1);
  std::memcpy(msg, m.data(), n);
  msg[n] = 0;
}
}  // namespace
extern "C" {

zkp_status zkp_zkey_verify_frominit(int device, const uint8_t* init, size_t init_len, const uint8_t* key,
                                    size_t key_len, const uint8_t* seed32, int* valid, char* msg, size_t msg_cap) {
  if (!init || !init_len || !key || !key_len || !valid) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  *valid = 0;
  put_msg("", msg, msg_cap);
  return guard([&] {
    std::string m;
    *valid = zkp::zkey_verify_frominit(device, init, init_len, key, key_len, seed32, m, &g_verify_timings) ? 1 : 0;
    put_msg(m, msg, msg_cap);
  });
}

zkp_status zkp_zkey_verify(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                           const uint8_t* key, size_t key_len, const uint8_t* seed32, int* valid, char* msg,
                           size_t msg_cap) {
  if (!r1cs || !r1cs_len || !ptau || !ptau_len || !key || !key_len || !valid)
    return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  *valid = 0;
  put_msg("", msg, msg_cap);
  return guard([&] {
    {  // a malformed key fails before the initial key is built on the device
      const zkp::ZkeyParsed z = zkp::parse_zkey(key, key_len, false);
      if (!z.bf.sec[10].ptr) throw zkp::ZkpError(ZKP_ERR_FORMAT, "zkey: missing section 10 (MPC parameters)");
      (void)zkp::read_mpc(z.bf.sec[10].ptr, z.bf.sec[10].len);
    }
    const std::vector<uint8_t> init = zkp::zkey_new(device, r1cs, r1cs_len, ptau, ptau_len);
    std::string m;
    *valid = zkp::zkey_verify_frominit(device, init.data(), init.size(), key, key_len, seed32, m, &g_verify_timings) ? 1 : 0;
    put_msg(m, msg, msg_cap);
  });
}

zkp_status zkp_zkey_verify_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::VerifyTimings& t = g_verify_timings;
  const double v[12] = {t.total_ms,      t.host_ms,         t.compare_ms,      t.rlc.upload_ms,
                        t.rlc.check_ms,  t.rlc.coeffs_ms,   t.rlc.plan_ms,     t.rlc.acc_ms[0],
                        t.rlc.acc_ms[1], t.rlc.fold_ms,     t.rlc.total_ms,    (double)t.rlc.chunks};
  for (int i = 0; i < n && i < 12; ++i) ms[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_ptau_prepare_phase2(int device, const uint8_t* ptau, size_t len, uint8_t** out, size_t* out_len) {
  if (!ptau || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::ptau_prepare_phase2(device, ptau, len); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_prepare_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::PrepareTimings t = zkp::ptau_prepare_timings();
  const double v[8] = {t.total_ms, t.parse_check_ms, t.upload_ms, t.g1_ms, t.g2_ms, t.affine_ms, t.download_ms, t.launches};
  for (int i = 0; i < n && i < 8; ++i) ms[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_group_ifft(int device, int g2, const uint8_t* points, int log_n, uint8_t* out) {
  if (!points || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::group_ifft(device, g2 != 0, points, log_n, out); });
}

zkp_status zkp_group_fft(int device, int g2, const uint8_t* points, int log_n, uint8_t* out) {
  if (!points || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::group_fft(device, g2 != 0, points, log_n, out); });
}

zkp_status zkp_mpcparams_info(const uint8_t* buf, size_t len, uint32_t* n_public, uint32_t* domain_size, uint32_t* n_vars,
                              uint32_t* n_contributions) {
  if (!buf || !n_public || !domain_size || !n_vars || !n_contributions) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    const zkp::MpcParamsFile f = zkp::mpcparams_parse(buf, len);
    *n_public = f.n_public, *domain_size = f.domain_size, *n_vars = f.n_vars, *n_contributions = f.n_contributions;
  });
}

zkp_status zkp_zkey_export_bellman(int device, const uint8_t* zkey, size_t len, uint8_t** out, size_t* out_len) {
  if (!zkey || !len || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::zkey_export_bellman(device, zkey, len); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_zkey_bellman_contribute(int device, const uint8_t* challenge, size_t len, const uint8_t* rand64,
                                       const char* entropy, uint8_t** out, size_t* out_len, uint8_t* hash64) {
  if (!challenge || !len || !entropy || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] {
    (void)zkp::mpcparams_parse(challenge, len);  // a malformed file is refused before the OS is asked for randomness
    zkp::ChaChaRng rng = entropy_rng(rand64, entropy);
    buf = zkp::zkey_bellman_contribute(device, challenge, len, rng, hash64);
  });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_zkey_import_bellman(int device, const uint8_t* old_zkey, size_t len, const uint8_t* response,
                                   size_t response_len, const char* name, uint8_t** out, size_t* out_len) {
  if (!old_zkey || !len || !response || !response_len || !out || !out_len)
    return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::zkey_import_bellman(device, old_zkey, len, response, response_len, name); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_zkey_bellman_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::BellmanTimings t = zkp::zkey_bellman_timings();
  const double v[11] = {t.total_ms,     t.parse_ms, t.upload_ms, t.decode_ms,   t.check_ms,        t.scale_ms,
                        t.transform_ms, t.coset_ms, t.encode_ms, t.download_ms, (double)t.chunks};
  for (int i = 0; i < n && i < 11; ++i) ms[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_rlc_coeffs(int device, const uint8_t* seed32, uint64_t first_index, size_t n, uint8_t* out) {
  if (!seed32 || (n && !out)) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::rlc_coeffs(device, seed32, first_index, n, out); });
}

zkp_status zkp_points_check(int device, int g2, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad) {
  if ((n && !points) || !n_bad || !first_bad) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::points_check(device, g2 != 0, points, n, n_bad, first_bad); });
}

zkp_status zkp_rlc_g1(int device, const uint8_t* seed32, uint64_t first_index, const uint8_t* points_a,
                      const uint8_t* points_b, size_t n, uint8_t* out_a64, int* inf_a, uint8_t* out_b64, int* inf_b) {
  if (!seed32 || (n && (!points_a || !points_b)) || !out_a64 || !inf_a || !out_b64 || !inf_b)
    return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    const zkp::RlcResult r = zkp::rlc_g1(device, seed32, first_index, points_a, points_b, n);
    if (r.first_bad_a != zkp::RLC_NO_BAD || r.first_bad_b != zkp::RLC_NO_BAD)
      throw zkp::ZkpError(ZKP_ERR_INVALID_ARG,
                          std::string("rlc: point ") +
                              std::to_string(r.first_bad_a != zkp::RLC_NO_BAD ? r.first_bad_a : r.first_bad_b) +
                              (r.first_bad_a != zkp::RLC_NO_BAD ? " of set a" : " of set b") + " is not on the curve");
    *inf_a = zkp::jac_to_bytes_g1(r.sum_a, out_a64) ? 0 : 1;
    *inf_b = zkp::jac_to_bytes_g1(r.sum_b, out_b64) ? 0 : 1;
  });
}

zkp_status zkp_ptau_verify_sections(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32, int* valid, char* msg,
                                    size_t msg_cap) {
  if (!ptau || !len || !valid) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  *valid = 0;
  put_msg("", msg, msg_cap);
  return guard([&] {
    std::string m;
    *valid = zkp::ptau_verify_sections(device, ptau, len, seed32, m) ? 1 : 0;
    put_msg(m, msg, msg_cap);
  });
}

zkp_status zkp_ptau_verify(int device, const uint8_t* ptau, size_t len, const uint8_t* seed32, int* valid, char* msg,
                           size_t msg_cap) {
  if (!ptau || !len || !valid) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  *valid = 0;
  put_msg("", msg, msg_cap);
  return guard([&] {
    std::string m;
    *valid = zkp::ptau_verify(device, ptau, len, seed32, m) ? 1 : 0;
    put_msg(m, msg, msg_cap);
  });
}

zkp_status zkp_ptau_verify_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::PtauVerifyTimings t = zkp::ptau_verify_timings();
  const double v[17] = {t.total_ms,   t.parse_ms,        t.upload_ms,          t.check_ms,          t.subgroup_ms,
                        t.coeffs_ms,  t.ntt_ms,          t.plan_ms,            t.acc_pairs_ms,      t.acc_lag_ms,
                        t.acc_tau_ms, t.fold_ms,         t.pairing_ms,         (double)t.chunks,    t.contributions_ms,
                        t.first_challenge_ms, t.next_challenge_ms};
  for (int i = 0; i < n && i < 17; ++i) ms[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_ptau_new(uint32_t power, uint32_t ceremony_power, uint8_t** out, size_t* out_len) {
  if (!out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::ptau_new(power, ceremony_power); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_contribute(int device, const uint8_t* ptau, size_t len, const uint8_t* rand64, const char* entropy,
                               const char* name, uint8_t** out, size_t* out_len) {
  if (!ptau || !len || !entropy || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] {
    zkp::ChaChaRng rng = entropy_rng(rand64, entropy);
    buf = zkp::ptau_contribute(device, ptau, len, rng, 0, name, nullptr, 0, 0);
  });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_beacon(int device, const uint8_t* ptau, size_t len, const uint8_t* beacon, size_t beacon_len,
                           uint32_t num_iterations_exp, const char* name, uint8_t** out, size_t* out_len) {
  if (!ptau || !len || (!beacon && beacon_len) || !out || !out_len)
    return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  if (num_iterations_exp > 63) return fail(ZKP_ERR_INVALID_ARG, "beacon: numIterationsExp must be <= 63");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] {
    uint8_t h[32];
    zkp::beacon_hash(beacon, beacon_len, num_iterations_exp, h);
    uint32_t seed[8];
    zkp::seed_from_hash(h, seed);
    zkp::ChaChaRng rng(seed);
    buf = zkp::ptau_contribute(device, ptau, len, rng, 1, name, beacon, beacon_len, num_iterations_exp);
  });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_contribute_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::PtauContributeTimings t = zkp::ptau_contribute_timings();
  const double v[12] = {t.total_ms, t.parse_check_ms, t.challenge_ms,  t.key_ms,          t.upload_ms,         t.g1_ms,
                        t.g2_ms,    t.encode_ms,      t.download_ms,   t.partial_hash_ms, t.next_challenge_ms, (double)t.chunks};
  for (int i = 0; i < n && i < 12; ++i) ms[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_points_scale_powers(int device, int g2, const uint8_t* points, size_t n, const uint8_t* first32,
                                   const uint8_t* ratio32, uint8_t* out) {
  if ((n && (!points || !out)) || !first32 || !ratio32) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::points_scale_powers(device, g2 != 0, points, n, first32, ratio32, out); });
}

zkp_status zkp_ptau_export_challenge(int device, const uint8_t* ptau, size_t len, uint8_t** out, size_t* out_len) {
  if (!ptau || !len || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::ptau_export_challenge(device, ptau, len); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_challenge_contribute(int device, const uint8_t* challenge, size_t len, const uint8_t* rand64,
                                         const char* entropy, uint8_t** out, size_t* out_len) {
  if (!challenge || !len || !entropy || !out || !out_len) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] {
    zkp::ChaChaRng rng = entropy_rng(rand64, entropy);
    buf = zkp::ptau_challenge_contribute(device, challenge, len, rng);
  });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_import_response(int device, const uint8_t* ptau, size_t len, const uint8_t* response, size_t response_len,
                                    const char* name, uint8_t** out, size_t* out_len) {
  if (!ptau || !len || !response || !response_len || !out || !out_len)
    return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  std::vector<uint8_t> buf;
  zkp_status s = guard([&] { buf = zkp::ptau_import_response(device, ptau, len, response, response_len, name); });
  return s != ZKP_OK ? s : hand_out(std::move(buf), out, out_len);
}

zkp_status zkp_ptau_challenge_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::PtauChallengeTimings t = zkp::ptau_challenge_timings();
  const double v[14] = {t.total_ms,     t.parse_check_ms, t.challenge_ms, t.key_ms,    t.upload_ms,
                        t.decode_ms,    t.decomp_g1_ms,   t.decomp_g2_ms, t.g1_ms,     t.g2_ms,
                        t.encode_ms,    t.download_ms,    t.partial_hash_ms + t.next_challenge_ms, (double)t.chunks};
  for (int i = 0; i < n && i < 14; ++i) ms[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_points_decompress(int device, int g2, const uint8_t* compressed, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                                 uint64_t* first_bad) {
  if ((n && (!compressed || !out_lem)) || !n_bad || !first_bad) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::points_decompress(device, g2 != 0, compressed, n, out_lem, n_bad, first_bad); });
}

zkp_status zkp_points_from_uncompressed(int device, int g2, const uint8_t* bytes, size_t n, uint8_t* out_lem, uint64_t* n_bad,
                                        uint64_t* first_bad) {
  if ((n && (!bytes || !out_lem)) || !n_bad || !first_bad) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::points_from_uncompressed(device, g2 != 0, bytes, n, out_lem, n_bad, first_bad); });
}

zkp_status zkp_field_sqrt(int device, int fq2, const uint8_t* in, size_t n, uint8_t* out, uint8_t* is_square) {
  if (n && (!in || !out || !is_square)) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::field_sqrt(device, fq2 != 0, in, n, out, is_square); });
}

zkp_status zkp_g2_subgroup_check(int device, const uint8_t* points, size_t n, uint64_t* n_bad, uint64_t* first_bad) {
  if ((n && !points) || !n_bad || !first_bad) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::g2_subgroup_check(device, points, n, n_bad, first_bad); });
}

zkp_status zkp_rlc_pairs(int device, int g2, const uint8_t* seed32, uint64_t first_index, const uint8_t* points, size_t n,
                         uint8_t* out_a, int* inf_a, uint8_t* out_b, int* inf_b) {
  if (!seed32 || (n && !points) || !out_a || !inf_a || !out_b || !inf_b) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    const zkp::PairSums r = zkp::rlc_pairs(device, g2 != 0, seed32, first_index, points, n);
    if (g2) {
      *inf_a = zkp::jac_to_bytes_g2(r.a2, out_a) ? 0 : 1;
      *inf_b = zkp::jac_to_bytes_g2(r.b2, out_b) ? 0 : 1;
    } else {
      *inf_a = zkp::jac_to_bytes_g1(r.a1, out_a) ? 0 : 1;
      *inf_b = zkp::jac_to_bytes_g1(r.b1, out_b) ? 0 : 1;
    }
  });
}

zkp_status zkp_prover_load_part(const uint8_t* zkey, size_t len, int device, int part, int nparts,
                                zkp_prover** out) {
  if (!zkey || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  return guard([&] {
    auto* h = new zkp_prover{nullptr};
    try {
      h->impl = new zkp::Prover(zkey, len, std::vector<int>{device}, part, nparts);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

zkp_status zkp_prove_partial(zkp_prover* p, const uint8_t* wtns, size_t len, zkp_partial* out) {
  if (!p || !wtns || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->prove_partial(wtns, len, out); });
}

zkp_status zkp_prove_partial_staged(zkp_prover* p, int slot, zkp_partial* out) {
  if (!p || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->prove_partial_staged(slot, out); });
}

zkp_status zkp_quotient_part_staged(zkp_prover* p, int slot, int mask, void* const* dst) {
  if (!p || !dst) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->quotient_part_staged(slot, mask, dst); });
}

zkp_status zkp_prove_partial_ext_staged(zkp_prover* p, int slot, const void* const* abc, zkp_partial* out) {
  if (!p || !abc || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->prove_partial_ext_staged(slot, abc, out); });
}

zkp_status zkp_proof_combine(const uint8_t* zkey, size_t len, const zkp_partial* parts, int nparts,
                             const uint8_t* wtns, size_t wlen, const uint8_t* r32, const uint8_t* s32,
                             zkp_proof* out) {
  if (!zkey || !parts || !wtns || !out || nparts < 1) return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  return guard([&] { zkp::proof_combine(zkey, len, parts, nparts, wtns, wlen, r32, s32, out); });
}

zkp_status zkp_prover_info(const zkp_prover* p, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain_size) {
  if (!p) return fail(ZKP_ERR_INVALID_ARG, "null prover");
  const auto& h = p->impl->header();
  if (n_vars) *n_vars = h.n_vars;
  if (n_public) *n_public = h.n_public;
  if (domain_size) *domain_size = h.domain_size;
  return ZKP_OK;
}

zkp_status zkp_prove(zkp_prover* p, const uint8_t* wtns, size_t len, const uint8_t* r32, const uint8_t* s32,
                     zkp_proof* out) {
  if (!p || !wtns || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->prove(wtns, len, r32, s32, out); });
}

zkp_status zkp_prove_batch(zkp_prover* p, const uint8_t* const* wtns, const size_t* lens, int n,
                           const uint8_t* const* r32s, const uint8_t* const* s32s, zkp_proof* outs) {
  return zkp_prove_batch_status(p, wtns, lens, n, r32s, s32s, outs, nullptr);
}

zkp_status zkp_prove_batch_status(zkp_prover* p, const uint8_t* const* wtns, const size_t* lens, int n,
                                  const uint8_t* const* r32s, const uint8_t* const* s32s, zkp_proof* outs,
                                  zkp_status* statuses) {
  if (!p || (n > 0 && (!wtns || !lens || !outs)) || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  zkp_status first = ZKP_OK;
  std::string msg;
  zkp_status s = guard([&] { first = p->impl->prove_batch(wtns, lens, n, r32s, s32s, outs, statuses, &msg); });
  if (s != ZKP_OK) return s;
  return first == ZKP_OK ? ZKP_OK : fail(first, msg);
}

zkp_status zkp_prove_files(zkp_prover* p, const char* wtns_path, const char* proof_path, const char* public_path) {
  if (!p || !wtns_path || !proof_path || !public_path) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    const MappedFile w(wtns_path);
    const uint32_t npub = p->impl->header().n_public;
    std::vector<uint8_t> pub((size_t)npub * 32 + 32);
    zkp_proof pr{};
    pr.public_capacity = npub;
    pr.public_signals = pub.data();
    p->impl->prove(w.data(), w.size(), nullptr, nullptr, &pr);
    write_file(proof_path, proof_json(&pr));
    write_file(public_path, public_json(&pr));
  });
}

zkp_status zkp_proof_json(const zkp_proof* proof, char* buf, size_t cap, size_t* needed) {
  if (!proof) return fail(ZKP_ERR_INVALID_ARG, "null proof");
  return emit(proof_json(proof), buf, cap, needed);
}

zkp_status zkp_public_json(const zkp_proof* proof, char* buf, size_t cap, size_t* needed) {
  if (!proof) return fail(ZKP_ERR_INVALID_ARG, "null proof");
  return emit(public_json(proof), buf, cap, needed);
}

zkp_status zkp_proof_calldata(const zkp_proof* proof, char* buf, size_t cap, size_t* needed) {
  if (!proof) return fail(ZKP_ERR_INVALID_ARG, "null proof");
  return emit(calldata(proof), buf, cap, needed);
}

zkp_status zkp_prover_timings(const zkp_prover* p, float* ms, int n) {
  if (!p || !ms) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  p->impl->timings(ms, n);
  return ZKP_OK;
}

void zkp_prover_free(zkp_prover* p) {
  if (!p) return;
  delete p->impl;
  delete p;
}

zkp_status zkp_prover_set_verify(zkp_prover* p, int on) {
  if (!p || !p->impl) return fail(ZKP_ERR_INVALID_ARG, "null prover");
  return guard([&] { p->impl->set_verify(on == 0 ? 0 : (on == 2 ? 2 : 1)); });
}

zkp_status zkp_prover_get_verify(const zkp_prover* p, int* mode) {
  if (!p || !p->impl || !mode) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  *mode = p->impl->verify_mode();
  return ZKP_OK;
}

}  // extern "C"

namespace {
using zkp::host::Affine;
using HFq = zkp::host::Fq;
using HFq2 = zkp::host::Fq2;
HFq fq_std(const uint8_t* b) {
  const zkp::host::U256 v = zkp::host::u256_from_le(b);
  if (zkp::host::u256_geq(v, zkp::host::FQ_DESC.mod)) throw zkp::ZkpError(ZKP_ERR_INVALID_ARG, "coordinate >= p");
  return HFq::from_std(v);
}
bool all_zero(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (b[i]) return false;
  return true;
}
Affine<HFq> g1_std(const uint8_t* b) {
  if (all_zero(b, 64)) return Affine<HFq>{HFq::zero(), HFq::zero(), true};
  return Affine<HFq>{fq_std(b), fq_std(b + 32), false};
}
Affine<HFq2> g2_std(const uint8_t* b) {
  if (all_zero(b, 128)) return Affine<HFq2>{HFq2::zero(), HFq2::zero(), true};
  return Affine<HFq2>{HFq2{fq_std(b), fq_std(b + 32)}, HFq2{fq_std(b + 64), fq_std(b + 96)}, false};
}
}  // namespace
extern "C" {

zkp_status zkp_proof_verify(const uint8_t* zkey, size_t len, const zkp_proof* proof, int* valid) {
  if (!zkey || !proof || !valid) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    *valid = 0;
    const zkp::ZkeyParsed z = zkp::parse_zkey(zkey, len, false);
    const zkp::ZkeyHeader& h = z.hdr;
    if (h.ic.size() != (size_t)h.n_public + 1) throw zkp::ZkpError(ZKP_ERR_FORMAT, "zkey: no IC section");
    if (proof->n_public != h.n_public || proof->public_capacity < h.n_public || (h.n_public && !proof->public_signals))
      throw zkp::ZkpError(ZKP_ERR_INVALID_ARG, "proof: public signals do not match the key's nPublic");
    zkp::host::VerifyingKey vk;
    vk.alpha1 = h.alpha1, vk.beta2 = h.beta2, vk.gamma2 = h.gamma2, vk.delta2 = h.delta2;
    vk.ic = h.ic.data();
    vk.n_public = (int)h.n_public;
    std::vector<zkp::host::U256> pub(h.n_public);
    for (uint32_t i = 0; i < h.n_public; ++i) pub[i] = zkp::host::u256_from_le(proof->public_signals + 32 * (size_t)i);
    const Affine<HFq> a = g1_std(proof->pi_a[0]), c = g1_std(proof->pi_c[0]);
    const Affine<HFq2> b = g2_std(proof->pi_b[0][0]);
    *valid = zkp::host::groth16_verify(vk, pub.data(), a, b, c) ? 1 : 0;
  });
}

zkp_status zkp_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* out384) {
  if (!g1 || !g2 || !out384) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    const Affine<HFq> p = g1_std(g1);
    const Affine<HFq2> q = g2_std(g2);
    if (!zkp::host::g1_on_curve(p) || !zkp::host::g2_on_curve(q))
      throw zkp::ZkpError(ZKP_ERR_INVALID_ARG, "pairing: point not on the curve");
    const zkp::host::Fq12 f = zkp::host::pairing(p, q);
    const HFq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
    for (int i = 0; i < 6; ++i) {
      zkp::host::u256_to_le(c[i]->c0.to_std(), out384 + 64 * i);
      zkp::host::u256_to_le(c[i]->c1.to_std(), out384 + 64 * i + 32);
    }
  });
}

zkp_status zkp_final_exponentiation(const uint8_t* in384, uint8_t* out384) {
  if (!in384 || !out384) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    HFq2 c[6];
    for (int i = 0; i < 6; ++i) c[i] = HFq2{fq_std(in384 + 64 * i), fq_std(in384 + 64 * i + 32)};
    const zkp::host::Fq12 f =
        zkp::host::final_exponentiation(zkp::host::Fq12{{c[0], c[1], c[2]}, {c[3], c[4], c[5]}});
    const HFq2* o[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
    for (int i = 0; i < 6; ++i) {
      zkp::host::u256_to_le(o[i]->c0.to_std(), out384 + 64 * i);
      zkp::host::u256_to_le(o[i]->c1.to_std(), out384 + 64 * i + 32);
    }
  });
}

zkp_status zkp_miller_loop(int device, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out) {
  if (n && (!g1 || !g2 || !out)) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::miller_loop_points(device, g1, g2, n, out); });
}

zkp_status zkp_fq12_product(int device, const uint8_t* in, size_t n, uint8_t* out384) {
  if ((n && !in) || !out384) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    for (size_t i = 0; i < n * 12; ++i)
      if (zkp::host::u256_geq(zkp::host::u256_from_le(in + 32 * i), zkp::host::FQ_DESC.mod))
        throw zkp::ZkpError(ZKP_ERR_INVALID_ARG, "fq12_product: coordinate >= p");
    zkp::fq12_product(device, in, n, out384);
  });
}

zkp_status zkp_zkey_export_vkey(const uint8_t* zkey, size_t len, char* buf, size_t cap, size_t* needed) {
  if (!zkey) return fail(ZKP_ERR_INVALID_ARG, "null zkey");
  std::string s;
  const zkp_status st = guard([&] { s = zkp::vkey_json(zkp::vkey_from_zkey(zkey, len)); });
  if (st != ZKP_OK) return st;
  return emit(s, buf, cap, needed);
}

zkp_status zkp_verifier_load_vkey_json(int device, const char* json, size_t len, zkp_verifier** out) {
  if (!json || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  return guard([&] {
    auto v = std::make_unique<zkp_verifier>();
    v->impl = std::make_unique<zkp::Verifier>(device, zkp::parse_vkey_json(json, len));
    *out = v.release();
  });
}

zkp_status zkp_verifier_load_zkey(int device, const uint8_t* zkey, size_t len, zkp_verifier** out) {
  if (!zkey || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  return guard([&] {
    auto v = std::make_unique<zkp_verifier>();
    v->impl = std::make_unique<zkp::Verifier>(device, zkp::vkey_from_zkey(zkey, len));
    *out = v.release();
  });
}

zkp_status zkp_verifier_info(const zkp_verifier* v, uint32_t* n_public) {
  if (!v || !v->impl) return fail(ZKP_ERR_INVALID_ARG, "null verifier");
  if (n_public) *n_public = v->impl->n_public();
  return ZKP_OK;
}

zkp_status zkp_verifier_verify(zkp_verifier* v, const zkp_proof* proofs, size_t n, const uint8_t* seed32, uint8_t* valid,
                               size_t* n_valid) {
  if (!v || !v->impl || (n && (!proofs || !valid))) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  if (n_valid) *n_valid = 0;
  return guard([&] { v->impl->verify(proofs, n, seed32, valid, n_valid); });
}

zkp_status zkp_verifier_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::Groth16VerifyTimings& t = zkp::verify_timings();
  const double v[9] = {t.gates_ms,     t.scalar_ms, t.miller_ms, t.product_ms, t.host_miller_ms,
                       t.final_exp_ms, t.search_ms, t.total_ms,  t.node_checks};
  for (int i = 0; i < n && i < 9; ++i) ms[i] = v[i];
  return ZKP_OK;
}

void zkp_verifier_free(zkp_verifier* v) { delete v; }

const char* zkp_last_error(void) { return g_err.c_str(); }

const char* zkp_version(void) { return "zkp_amd 0.1 gfx950"; }

zkp_status zkp_msm_g1(int device, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out64,
                      int* is_inf) {
  if ((n && (!points || !scalars)) || !out64 || !is_inf) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::msm_points(device, zkp::Curve::G1, points, scalars, n, out64, is_inf); });
}

zkp_status zkp_msm_g2(int device, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out128,
                      int* is_inf) {
  if ((n && (!points || !scalars)) || !out128 || !is_inf) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { zkp::msm_points(device, zkp::Curve::G2, points, scalars, n, out128, is_inf); });
}

zkp_status zkp_msm(int device, int g2, const uint8_t* points, const uint8_t* scalars, size_t n, int window_bits,
                   int table_depth, uint8_t* out, int* is_inf) {
  if ((n && (!points || !scalars)) || !out || !is_inf) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  if (window_bits < 0 || (window_bits > 0 && window_bits < 8) || window_bits > 24 || table_depth < 0)
    return fail(ZKP_ERR_INVALID_ARG, "MSM window bits must be 0 (automatic) or within 8..24, table_depth >= 0");
  return guard([&] {
    zkp::msm_points(device, g2 ? zkp::Curve::G2 : zkp::Curve::G1, points, scalars, n, out, is_inf, window_bits,
                    table_depth);
  });
}

zkp_status zkp_prover_msm_config(const zkp_prover* p, double* out, int n) {
  if (!p || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->msm_config(out, n); });
}

zkp_status zkp_ntt_fr(int device, uint8_t* data, size_t n, int mode) {
  if (!data || mode < 0 || mode > 2) return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  return guard([&] { zkp::ntt_fr(device, data, n, mode); });
}

zkp_status zkp_quotient(zkp_prover* p, const uint8_t* wtns, size_t len, uint8_t* out) {
  if (!p || !wtns || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->quotient(wtns, len, out); });
}

zkp_status zkp_witness_stage(zkp_prover* p, int dev_index, int slot, const uint8_t* wtns, size_t len) {
  if (!p || !wtns) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->stage(dev_index, slot, wtns, len); });
}

zkp_status zkp_prove_staged(zkp_prover* p, int dev_index, int slot, const uint8_t* r32, const uint8_t* s32,
                            zkp_proof* out) {
  if (!p || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->prove_staged(dev_index, slot, r32, s32, out); });
}

zkp_status zkp_prover_instrument(zkp_prover* p, int on) {
  if (!p) return fail(ZKP_ERR_INVALID_ARG, "null prover");
  return guard([&] { p->impl->set_instrument(on != 0); });
}

zkp_status zkp_prover_kernel_stats(const zkp_prover* p, double* out, int n) {
  if (!p || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { p->impl->kernel_stats(out, n); });
}

zkp_status zkp_prover_launch_stats(const zkp_prover* p, double* out, int max_records, int* n_records) {
  if (!p || !n_records || (max_records > 0 && !out)) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] { *n_records = p->impl->launch_records(out, max_records); });
}

zkp_status zkp_bench_msm_ex(int device, int g2, const uint8_t* points, const uint8_t* scalars, size_t n, int warmup,
                            int iters, double* stats, int nstats, uint8_t* out, int* is_inf) {
  if (!points || !scalars || !stats || nstats < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  return guard([&] {
    zkp::MsmBench b = zkp::bench_msm(device, g2 ? zkp::Curve::G2 : zkp::Curve::G1, points, scalars, n, warmup,
                                     iters, out, is_inf);
    const double v[8] = {b.ms_per_msm, b.ms_accumulate, (double)b.mixed_adds, (double)b.tasks,
                         (double)b.c, (double)b.windows, (double)b.table_ms, (double)b.depth};
    for (int i = 0; i < nstats && i < 8; ++i) stats[i] = v[i];
  });
}

zkp_status zkp_bench_msm(int device, int g2, const uint8_t* points, const uint8_t* scalars, size_t n, int warmup,
                         int iters, double* stats, uint8_t* out, int* is_inf) {
  return zkp_bench_msm_ex(device, g2, points, scalars, n, warmup, iters, stats, 6, out, is_inf);
}

zkp_status zkp_bench_plan(int device, const uint8_t* scalars, size_t n, int window_bits, int dense, int warmup,
                          int iters, double* ms) {
  if (!scalars || !ms || window_bits < 0 || window_bits == 1 || window_bits > 24)
    return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  return guard([&] { *ms = zkp::bench_plan(device, scalars, n, window_bits, dense, warmup, iters); });
}

zkp_status zkp_bench_ntt(int device, int log_n, int warmup, int iters, double* ms) {
  if (!ms || log_n < 1 || log_n > 27) return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  return guard([&] { *ms = zkp::bench_ntt(device, log_n, 1, warmup, iters); });
}

zkp_status zkp_bench_ntt_batch(int device, int log_n, int count, int warmup, int iters, double* ms) {
  if (!ms || log_n < 1 || log_n > 27 || count < 1 || count > 3) return fail(ZKP_ERR_INVALID_ARG, "bad argument");
  return guard([&] { *ms = zkp::bench_ntt(device, log_n, count, warmup, iters); });
}

}  // extern "C"

// ---------------------------------------------------------------- wtns check (wtns_check.hpp)

struct zkp_checker {
  zkp::WitnessChecker* impl;
};

namespace {
void clear_result(zkp_check_result* res, char* msg, size_t msg_cap) {
  std::memset(res, 0, sizeof(*res));
  put_msg("", msg, msg_cap);
}
}  // namespace

extern "C" {

zkp_status zkp_checker_load(int device, const uint8_t* r1cs, size_t len, zkp_checker** out) {
  if (!r1cs || !len || !out) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  *out = nullptr;
  return guard([&] {
    double parse_ms = 0;
    zkp::R1csCsr csr = zkp::parse_r1cs_or_throw(r1cs, len, &parse_ms);
    std::unique_ptr<zkp::WitnessChecker> w(new zkp::WitnessChecker(device, std::move(csr), parse_ms));
    *out = new zkp_checker{w.get()};
    w.release();
  });
}

zkp_status zkp_checker_info(const zkp_checker* c, uint32_t* n_vars, uint32_t* n_public, uint32_t* n_constraints,
                            uint64_t* n_terms) {
  if (!c) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  if (n_vars) *n_vars = c->impl->n_wires();
  if (n_public) *n_public = c->impl->n_public();
  if (n_constraints) *n_constraints = c->impl->n_constraints();
  if (n_terms) *n_terms = c->impl->n_terms();
  return ZKP_OK;
}

zkp_status zkp_checker_paths(const zkp_checker* c, uint64_t* out, int n) {
  if (!c || !out || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const uint64_t v[2] = {c->impl->n_long(), c->impl->long_terms()};
  for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
  return ZKP_OK;
}

zkp_status zkp_checker_check(zkp_checker* c, const uint8_t* wtns, size_t len, zkp_check_result* res, char* msg,
                             size_t msg_cap) {
  if (!c || !wtns || !len || !res) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  clear_result(res, msg, msg_cap);
  return guard([&] {
    std::string m;
    c->impl->check(wtns, len, res, m);
    put_msg(m, msg, msg_cap);
  });
}

zkp_status zkp_checker_check_staged(zkp_checker* c, zkp_prover* p, int dev_index, int slot, zkp_check_result* res,
                                    char* msg, size_t msg_cap) {
  if (!c || !p || !res) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  clear_result(res, msg, msg_cap);
  return guard([&] {
    std::string m;
    c->impl->check_staged(*p->impl, dev_index, slot, res, m);
    put_msg(m, msg, msg_cap);
  });
}

void zkp_checker_free(zkp_checker* c) {
  if (!c) return;
  delete c->impl;
  delete c;
}

zkp_status zkp_wtns_check(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* wtns, size_t wtns_len,
                          zkp_check_result* res, char* msg, size_t msg_cap) {
  if (!r1cs || !r1cs_len || !wtns || !wtns_len || !res) return fail(ZKP_ERR_INVALID_ARG, "null argument or zero length");
  clear_result(res, msg, msg_cap);
  return guard([&] {
    const auto t0 = std::chrono::steady_clock::now();
    double parse_ms = 0;
    zkp::R1csCsr csr = zkp::parse_r1cs_or_throw(r1cs, r1cs_len, &parse_ms);
    zkp::check_wtns_header(csr, wtns, wtns_len);  // both files are sound before the device is touched
    zkp::WitnessChecker w(device, std::move(csr), parse_ms);
    const zkp::CheckTimings load = zkp::check_timings();
    std::string m;
    w.check(wtns, wtns_len, res, m);
    put_msg(m, msg, msg_cap);
    zkp::CheckTimings& t = zkp::check_timings();
    t.parse_ms = load.parse_ms;
    t.upload_ms = load.upload_ms;
    t.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
}

zkp_status zkp_wtns_check_timings(double* ms, int n) {
  if (!ms || n < 0) return fail(ZKP_ERR_INVALID_ARG, "null argument");
  const zkp::CheckTimings& t = zkp::check_timings();
  const double v[5] = {t.parse_ms, t.upload_ms, t.copy_ms, t.kernel_ms, t.total_ms};
  for (int i = 0; i < n && i < 5; ++i) ms[i] = v[i];
  return ZKP_OK;
}

}  // extern "C"
