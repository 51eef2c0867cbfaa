// CPU replay of `powersoftau contribute`'s per-lane bodies (ptau_scale_kernels.hpp: the power table, the
// lane's scalar, the ladder, the affine conversion and the three encodings), as one launch of
// k_scale_powers over a chunk, for checking them without a GPU.
// usage: ptau_scale_emu <g1|g2> <file of n zkey-layout points> <n> <first hex> <ratio hex> <chunk start>
//   first, ratio: standard form below r, big-endian hex; point j of the file is point <chunk start> + j of
//   its section, so its scalar is first * ratio^(chunk start + j)
//   -> one line per point: the zkey-layout, the uncompressed and the compressed bytes in hex
//   --reencode: the same three streams a second time through encode_lem (k_encode_points' body) from the
//   zkey-layout bytes of the first; the program fails if they differ
// Every zkey-layout result is also compared with host_ec (jac_mul by first * ratio^(chunk start + j) computed
// with host::Fr); a difference fails the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zk-p2p-onramp_amd/csrc/host_ec.hpp"
#include "../../zk-p2p-onramp_amd/csrc/ptau_scale_kernels.hpp"
using namespace zkp;

static host::U256 u256_of(const uint32_t (&w)[8]) {
  host::U256 v;
  for (int i = 0; i < 4; ++i) v.w[i] = (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32;
  return v;
}
static host::Fq fq_at(const uint32_t* w) {
  host::U256 v;
  std::memcpy(v.w, w, 32);
  return host::Fq::raw(v);
}
static bool zero_words(const uint32_t* w, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (w[i]) return false;
  return true;
}
// point j of a zkey-layout array times k by host_ec, back in the zkey layout
static void host_mul(const uint32_t* in, bool g2, size_t j, const host::U256& k, uint32_t* out) {
  const size_t pw = g2 ? 32 : 16;
  const uint32_t* p = in + j * pw;
  std::memset(out, 0, pw * 4);
  if (zero_words(p, pw)) return;
  if (!g2) {
    const auto r = host::jac_to_aff(host::jac_mul(host::jac_from_aff(host::Affine<host::Fq>{fq_at(p), fq_at(p + 8), false}), k));
    if (r.inf) return;
    std::memcpy(out, r.x.v.w, 32), std::memcpy(out + 8, r.y.v.w, 32);
  } else {
    const host::Affine<host::Fq2> a{host::Fq2{fq_at(p), fq_at(p + 8)}, host::Fq2{fq_at(p + 16), fq_at(p + 24)}, false};
    const auto r = host::jac_to_aff(host::jac_mul(host::jac_from_aff(a), k));
    if (r.inf) return;
    std::memcpy(out, r.x.c0.v.w, 32), std::memcpy(out + 8, r.x.c1.v.w, 32);
    std::memcpy(out + 16, r.y.c0.v.w, 32), std::memcpy(out + 24, r.y.c1.v.w, 32);
  }
}

static bool hex_words(const char* h, uint32_t (&w)[8]) {
  std::string s(h);
  if (s.empty() || s.size() > 64) return false;
  s = std::string(64 - s.size(), '0') + s;
  for (int i = 0; i < 8; ++i) {
    char* stop = nullptr;
    const std::string part = s.substr(64 - 8 * (i + 1), 8);
    w[i] = (uint32_t)strtoul(part.c_str(), &stop, 16);
    if (*stop) return false;
  }
  return true;
}

static void print_hex(const uint32_t* w, size_t words) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(w);
  for (size_t i = 0; i < words * 4; ++i) printf("%02x", b[i]);
}

template <class F>
static int run(const std::vector<uint32_t>& in, size_t n, const pscale::Powers& pw, bool reencode, const uint32_t (&first)[8],
               const uint32_t (&ratio)[8], uint64_t start) {
  constexpr int W = FWords<F>::W;
  std::vector<uint32_t> lem(n * 2 * W), u(n * 2 * W), c(n * W);
  for (size_t j = 0; j < n; ++j)
    pscale::encode_xyzz<F>(pscale::scale_lane<F, 2>(in.data(), pw, j), pw.to_zkey, lem.data(), u.data(), c.data(), j);
  {
    const host::Fr r = host::Fr::from_std(u256_of(ratio));
    host::Fr s = host::Fr::from_std(u256_of(first)) * r.pow(host::U256{{start, 0, 0, 0}});
    std::vector<uint32_t> want(2 * W);
    for (size_t j = 0; j < n; ++j, s = s * r) {
      host_mul(in.data(), W == 16, j, s.to_std(), want.data());
      if (std::memcmp(want.data(), lem.data() + j * 2 * W, 8 * W) != 0) {
        fprintf(stderr, "point %zu differs from host_ec\n", j);
        return 4;
      }
    }
  }
  if (reencode) {
    std::vector<uint32_t> lem2(lem.size()), u2(u.size()), c2(c.size());
    for (size_t j = 0; j < n; ++j) pscale::encode_lem<F>(lem.data(), pw.to_zkey, lem2.data(), u2.data(), c2.data(), j);
    if (lem2 != lem || u2 != u || c2 != c) {
      fprintf(stderr, "encode_lem differs from encode_xyzz\n");
      return 3;
    }
  }
  for (size_t j = 0; j < n; ++j) {
    print_hex(lem.data() + j * 2 * W, 2 * W);
    printf(" ");
    print_hex(u.data() + j * 2 * W, 2 * W);
    printf(" ");
    print_hex(c.data() + j * W, W);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  std::vector<const char*> pos;
  bool reencode = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--reencode")) reencode = true;
    else pos.push_back(argv[i]);
  }
  uint32_t first[8], ratio[8];
  if (pos.size() != 6 || !hex_words(pos[3], first) || !hex_words(pos[4], ratio)) {
    fprintf(stderr, "usage: ptau_scale_emu <g1|g2> <file> <n> <first hex> <ratio hex> <chunk start> [--reencode]\n");
    return 2;
  }
  const bool g2 = std::string(pos[0]) == "g2";
  const size_t n = strtoull(pos[2], nullptr, 10), pw_words = g2 ? 32 : 16;
  const uint64_t start = strtoull(pos[5], nullptr, 10);
  if (n < 1 || n > (1u << 16)) return 2;
  std::vector<uint32_t> in(n * pw_words);
  FILE* f = fopen(pos[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) return 1;
  fclose(f);
  pscale::Powers pw;
  pscale::fill_powers(pw, first, ratio, start);
  return g2 ? run<Fq2>(in, n, pw, reencode, first, ratio, start) : run<Fq>(in, n, pw, reencode, first, ratio, start);
}
