// ec_locate_plan.h -- host plan of the scrub locate step (include/tfs_ec.h,
// tfs_ec_locate).  Header-only, no device.
//
// The encode matrix is Cauchy, m[p][j] = 1 / (p ^ (pn + j)) (ec_math.h).  Let S_p
// be stored parity p XOR the code of the data members as given.  When data
// member j alone is wrong in a unit by e, S_p = m[p][j] e for every p, so
//   S_o = (m[o][j] / m[0][j]) S_0   for o = 1 .. pn - 1,   e = (1 / m[0][j]) S_0.
// For a fixed o the ratios are pairwise distinct over j (checked below), so with
// pn >= 2 at most one j satisfies the first relation for a non-zero S_0.
//
// A GF(2^8) element acts on a unit through its 8 x 8 bit matrix (ec_math.h's
// rule: column x = e * 2^x, bit l of column x at row l): output packet r is the
// XOR of the input packets c whose bit [r][c] is set.  The matrices are expanded
// to 0 / ~0 words as upload_plan expands the coder's, for scalar loads.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ec_math.h"

namespace tfsec {

// e's bit matrix, row-major [r][c] (0/1): encode_bitmatrix's rule for one element.
inline void gf_bitmatrix(const Gf256& gf, int e, uint8_t (&bm)[kW][kW]) {
  for (int x = 0; x < kW; ++x) {
    for (int l = 0; l < kW; ++l) bm[l][x] = uint8_t((e >> l) & 1);
    e = gf.mul(e, 2);
  }
}

struct LocatePlan {
  int dn = 0, pn = 0;
  std::vector<uint8_t> ratio_e;  // [(pn - 1)][dn]: the element m[o][j] / m[0][j], o = 1 .. pn - 1
  std::vector<uint8_t> inv0_e;   // [dn]: the element 1 / m[0][j]
  std::vector<uint32_t> ratio;   // [(pn - 1)][dn][8][8] mask words
  std::vector<uint32_t> inv0;    // [dn][8][8] mask words
};

// 0 ok; -1 (dn, pn) outside pn >= 2, dn >= 1, dn + pn <= kMaxMembers; -2 two data members share a
// ratio for some o (the caller answers TFS_EXIT_MATRIX_INVALID: the kernel's uniqueness rests on it).
inline int make_locate_plan(int dn, int pn, LocatePlan* plan) {
  static const Gf256 gf;
  if (dn <= 0 || pn < 2 || dn + pn > kMaxMembers) return -1;
  plan->dn = dn;
  plan->pn = pn;
  plan->ratio_e.assign(size_t(pn - 1) * dn, 0);
  plan->inv0_e.assign(size_t(dn), 0);
  plan->ratio.assign(size_t(pn - 1) * dn * kW * kW, 0u);
  plan->inv0.assign(size_t(dn) * kW * kW, 0u);
  auto expand = [](int e, uint32_t* w) {
    uint8_t bm[kW][kW];
    gf_bitmatrix(gf, e, bm);
    for (int r = 0; r < kW; ++r)
      for (int c = 0; c < kW; ++c) w[r * kW + c] = bm[r][c] ? 0xFFFFFFFFu : 0u;
  };
  for (int j = 0; j < dn; ++j) {
    const int m0 = gf.div(1, 0 ^ (pn + j));
    const int inv = gf.div(1, m0);
    plan->inv0_e[size_t(j)] = uint8_t(inv);
    expand(inv, &plan->inv0[size_t(j) * kW * kW]);
    for (int o = 1; o < pn; ++o) {
      const int q = gf.div(gf.div(1, o ^ (pn + j)), m0);
      plan->ratio_e[size_t(o - 1) * dn + j] = uint8_t(q);
      expand(q, &plan->ratio[(size_t(o - 1) * dn + j) * kW * kW]);
    }
  }
  for (int o = 1; o < pn; ++o)
    for (int j = 0; j < dn; ++j)
      for (int i = 0; i < j; ++i)
        if (plan->ratio_e[size_t(o - 1) * dn + i] == plan->ratio_e[size_t(o - 1) * dn + j]) return -2;
  return 0;
}

}  // namespace tfsec
