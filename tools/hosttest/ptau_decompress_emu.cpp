// CPU replay of the per-lane bodies of `powersoftau challenge contribute` / `import response`
// (ptau_decompress_kernels.hpp: the square roots in Fq and Fq2, point decompression, the decoding of
// uncompressed points), one launch of k_field_sqrt / k_decompress_points / k_decode_points over a file, for
// checking them without a GPU.
// usage: ptau_decompress_emu sqrt <fq|fq2> <file of n elements, 32 bytes LE standard form each coordinate> <n>
//          -> one line per element: the root (same form, or zeros) in hex, then 1 or 0
//        ptau_decompress_emu decompress <g1|g2> <file of n compressed points> <n>
//          -> one line per point: 1 if refused else 0, the zkey-layout and the uncompressed bytes in hex
//        ptau_decompress_emu decode <g1|g2> <file of n uncompressed points> <n>
//          -> one line per point: 1 if refused else 0, the zkey-layout bytes in hex
// Every verdict is also checked with host_ec's field: a root by squaring it, a "no root" by Euler's criterion
// (Fq2: on the norm), a decompressed point by the curve equation; a difference fails the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zk-p2p-onramp_amd/csrc/host_ec.hpp"
#include "../../zk-p2p-onramp_amd/csrc/ptau_decompress_kernels.hpp"
using namespace zkp;

static host::Fq fq_std(const uint32_t* w) {  // 8 LE words, standard form
  host::U256 v;
  std::memcpy(v.w, w, 32);
  return host::Fq::from_std(v);
}
static host::Fq fq_lem(const uint32_t* w) {  // 8 LE words, the zkey's Montgomery form
  host::U256 v;
  std::memcpy(v.w, w, 32);
  return host::Fq::raw(v);
}
static bool is_residue(const host::Fq& a) {  // a^((p - 1) / 2) != -1
  host::U256 e = host::FQ_DESC.mod;
  for (int i = 0; i < 4; ++i) e.w[i] = (e.w[i] >> 1) | (i < 3 ? e.w[i + 1] << 63 : 0);
  return !(a.pow(e) == host::Fq::one().neg());
}
static void print_hex(const void* p, size_t bytes) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
  for (size_t i = 0; i < bytes; ++i) printf("%02x", b[i]);
}

template <class F>
static int run_sqrt(const std::vector<uint32_t>& in, size_t n) {
  constexpr int W = FWords<F>::W;
  pdec::Consts k;
  pdec::fill_consts(k, false);
  std::vector<uint32_t> out(n * W);
  std::vector<uint8_t> sq(n);
  for (size_t j = 0; j < n; ++j) pdec::sqrt_lane<F>(in.data(), k, out.data(), sq.data(), j);
  for (size_t j = 0; j < n; ++j) {
    const uint32_t *a = in.data() + j * W, *r = out.data() + j * W;
    bool ok;
    if (W == 8) {
      ok = sq[j] ? fq_std(r).sqr() == fq_std(a) : !is_residue(fq_std(a));
    } else {
      const host::Fq2 x{fq_std(a), fq_std(a + 8)}, y{fq_std(r), fq_std(r + 8)};
      ok = sq[j] ? y.sqr() == x : !is_residue(x.c0.sqr() + x.c1.sqr());
    }
    if (!ok) {
      fprintf(stderr, "element %zu: the verdict %d disagrees with host_ec\n", j, (int)sq[j]);
      return 4;
    }
    print_hex(r, 4 * W);
    printf(" %d\n", (int)sq[j]);
  }
  return 0;
}

// y^2 = x^3 + b on a zkey-layout point (not all-zero)
static bool on_curve(const uint32_t* p, bool g2) {
  const host::Fq three = host::Fq::from_std(host::U256{{3, 0, 0, 0}});
  if (!g2) {
    const host::Fq x = fq_lem(p), y = fq_lem(p + 8);
    return y.sqr() == x.sqr() * x + three;
  }
  const host::Fq2 x{fq_lem(p), fq_lem(p + 8)}, y{fq_lem(p + 16), fq_lem(p + 24)};
  const host::Fq2 b2 = host::Fq2{three, host::Fq::zero()} *
                       host::Fq2{host::Fq::from_std(host::U256{{9, 0, 0, 0}}), host::Fq::one()}.inv();
  return y.sqr() == x.sqr() * x + b2;
}

template <class F>
static int run_points(bool decompress, const std::vector<uint32_t>& in, size_t n) {
  constexpr int W = FWords<F>::W;
  pdec::Consts k;
  pdec::fill_consts(k, W == 16);
  std::vector<uint32_t> lem(n * 2 * W), u(n * 2 * W);
  for (size_t j = 0; j < n; ++j) {
    const bool bad = decompress ? pdec::decompress_lane<F>(in.data(), k, lem.data(), u.data(), j)
                                : pdec::decode_lane<F>(in.data(), k.to_zkey, lem.data(), j);
    const uint32_t* p = lem.data() + j * 2 * W;
    bool zero = true;
    for (int i = 0; i < 2 * W; ++i) zero = zero && !p[i];
    if (bad && !zero) {
      fprintf(stderr, "point %zu: refused but not written as zeros\n", j);
      return 3;
    }
    if (decompress && !bad && !zero && !on_curve(p, W == 16)) {
      fprintf(stderr, "point %zu: decompressed off the curve\n", j);
      return 4;
    }
    printf("%d ", bad ? 1 : 0);
    print_hex(p, 8 * W);
    if (decompress) {
      printf(" ");
      print_hex(u.data() + j * 2 * W, 8 * W);
    }
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: ptau_decompress_emu <sqrt|decompress|decode> <fq|fq2|g1|g2> <file> <n>\n");
    return 2;
  }
  const std::string mode = argv[1], what = argv[2];
  const bool wide = what == "fq2" || what == "g2";
  const size_t n = strtoull(argv[4], nullptr, 10);
  size_t words;  // per element of the input
  if (mode == "sqrt") words = wide ? 16 : 8;
  else if (mode == "decompress") words = wide ? 16 : 8;
  else if (mode == "decode") words = wide ? 32 : 16;
  else return 2;
  if (n < 1 || n > (1u << 16)) return 2;
  std::vector<uint32_t> in(n * words);
  FILE* f = fopen(argv[3], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) return 1;
  fclose(f);
  if (mode == "sqrt") return wide ? run_sqrt<Fq2>(in, n) : run_sqrt<Fq>(in, n);
  return wide ? run_points<Fq2>(mode == "decompress", in, n) : run_points<Fq>(mode == "decompress", in, n);
}
