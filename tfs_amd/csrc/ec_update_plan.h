// ec_update_plan.h -- host side of the parity update (include/tfs_ec.h,
// tfs_ec_update): where the 64 mask words of (parity member p,
// data member j) lie in the coder's encode plan, and the checks of a unit list.
// Header-only, no device; the kernel uses the same offset function.
//
// The encode plan is upload_plan's [pn][8][dn][8] array of 0 / ~0 words: word
// ((p * 8 + r) * dn + j) * 8 + c is bit [r][c] of the 8 x 8 bit matrix of
// m[p][j].  Parity member p of a family that is zero except for data member j
// is that matrix applied to member j, so a change d of member j moves parity p
// by it: packet r of the parity unit ^= XOR of the packets c of d whose word is
// set.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tfsec {

constexpr uint32_t kUpdateInline = 16;  // units of a list that travel in the launch arguments

// The first of the 8 words of row r of block (p, member) in the [pn][8][dn][8] plan.
#ifdef __HIP__
__attribute__((host)) __attribute__((device))
#endif
inline uint32_t update_mask_offset(uint32_t p, uint32_t r, uint32_t dn, uint32_t member) {
  return ((p * 8u + r) * dn + member) * 8u;
}

// The list checks of tfs_ec_update(_device), in the header's order: 0 fine; 1 a unit at or
// past `have` (without a list: n > have); 2 a unit named twice.  The list may be unsorted.
inline int update_list_check(const uint32_t* units, uint32_t n, uint32_t have) {
  if (!units) return n > have ? 1 : 0;
  for (uint32_t k = 0; k < n; ++k)
    if (units[k] >= have) return 1;
  if (n <= kUpdateInline) {  // the common call names one or two units: no allocation
    for (uint32_t k = 1; k < n; ++k)
      for (uint32_t i = 0; i < k; ++i)
        if (units[i] == units[k]) return 2;
    return 0;
  }
  std::vector<uint32_t> s(units, units + n);
  std::sort(s.begin(), s.end());
  return std::adjacent_find(s.begin(), s.end()) != s.end() ? 2 : 0;
}

}  // namespace tfsec
