// CPU run of the G2 subgroup check's per-thread body (csrc/g2_subgroup_kernels.hpp, the body of
// ptau_verify.hip k_g2_subgroup) beside the host's own test (host::g2_in_subgroup), without a GPU.
// usage: g2_subgroup_emu <file of zkey-layout G2 points, 128 bytes each> [--events]
//   -> one line per point: `<kernel> <host>`, 1 = all-zero or in the subgroup of order r
//   --events: then `event <dbl> <cancel> <acc_inf> <q_inf>`: how often the ladders' additions took an
//     exceptional branch (curve.hpp ZKP_XYZZ_EVENT)
#include <cstdio>
#include <cstring>
#include <vector>

static unsigned long long g_events[4];
static inline void emu_event(int kind) { ++g_events[kind]; }
#define ZKP_XYZZ_EVENT(kind) ::emu_event((int)(kind))
#include "../../zk-p2p-onramp_amd/csrc/g2_subgroup_kernels.hpp"
#include "../../zk-p2p-onramp_amd/csrc/host_pairing.hpp"
using namespace zkp;

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: g2_subgroup_emu <file> [--events]\n");
    return 2;
  }
  const bool events = argc > 2 && !strcmp(argv[2], "--events");
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  std::vector<uint32_t> in;
  uint32_t buf[32];
  while (fread(buf, 4, 32, f) == 32) in.insert(in.end(), buf, buf + 32);
  fclose(f);
  const size_t n = in.size() / 32;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(in.data() + i * 32);
    bool inf = true;
    for (int j = 0; j < 128; ++j) inf &= p[j] == 0;
    auto fq = [&](int k) { return host::Fq::raw(host::u256_from_le(p + 32 * k)); };
    const host::Affine<host::Fq2> a{host::Fq2{fq(0), fq(1)}, host::Fq2{fq(2), fq(3)}, inf};
    printf("%d %d\n", g2sub::in_subgroup(in.data(), i) ? 1 : 0, host::g2_in_subgroup(a) ? 1 : 0);
  }
  if (events) printf("event %llu %llu %llu %llu\n", g_events[0], g_events[1], g_events[2], g_events[3]);
  return 0;
}
