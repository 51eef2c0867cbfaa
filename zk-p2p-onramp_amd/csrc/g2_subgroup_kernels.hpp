// Per-thread body of the G2 subgroup check (ptau_verify.hip k_g2_subgroup): __host__ __device__ so that
// tools/hosttest/g2_subgroup_emu.cpp can run it on the CPU against host::g2_in_subgroup.
//
// A point of the twist E'(Fq2): y^2 = x^3 + 3 / (9 + u) is in G2 iff [r]P = infinity: #E' = r (2p - r) and
// gcd(r, 2p - r) = 1.  The ladder is gfft::scale<2> with the scalar r (254 bits: 127 two-bit digits, 80 of
// them nonzero: 253 doublings and 80 additions, the table {P, 2P, 3P} included).  r is the same in
// every lane, so the digit branches are wave-uniform.  The additions are the complete xyzz_add and
// xyzz_dbl: [r]P reaches infinity in the last step of every good point, and a point of small order
// (the cofactor 2p - r has the factors 10069 and 5864401) meets equal and opposite operands inside
// the ladder.
#pragma once
#include "gfft_kernels.hpp"

namespace zkp {
namespace g2sub {

// point i of a zkey-layout G2 array (as uploaded; on the curve, k_check_points ran): all-zero, or [r]P = inf
ZDEV bool in_subgroup(const uint32_t* pts, size_t i) {
  const Xyzz<Fq2> p = gfft::load_point<Fq2>(pts, i);
  if (xyzz_is_inf(p)) return true;
  uint32_t r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = FrCfg::MOD_W[k];
  return xyzz_is_inf(gfft::scale<2>(p, r));
}

}  // namespace g2sub
}  // namespace zkp
