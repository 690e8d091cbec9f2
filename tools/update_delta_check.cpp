// update_delta_check.cpp -- stand-alone check of the host-only pieces of the parity update
// (tfs_amd/ds/parity_update.h, tfs_amd/csrc/ec_update_plan.h), meant to be
// built with the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/update_delta_check.cpp -o /tmp/update_delta_check && /tmp/update_delta_check
//
// The covering units and delta slots of a changed range (inside one unit, ending on a unit
// boundary, straddling one, spanning several, empty), the list checks on sorted and unsorted
// lists on both sides of the in-arguments limit, and the offset of block (p, member) in the
// encode plan, against the coder's own encode bitmatrix: the 64 words at that offset, applied to
// a delta symbol by symbol, give the GF(2^8) product m[p][member] * delta.
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "../tfs_amd/csrc/ec_math.h"
#include "../tfs_amd/csrc/ec_update_plan.h"
#include "../tfs_amd/ds/parity_update.h"

using namespace tfsec;
using tfs::dataserver::make_parity_delta;
using tfs::dataserver::ParityDelta;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static int ranges = 0;

// One range against a byte-by-byte restatement over a whole image.
static void check_range(int64_t offset, int64_t len, std::vector<uint32_t> want_units) {
  const int64_t image = 8 * 1024;
  std::vector<char> before(8 * 1024), after;
  for (int64_t i = 0; i < image; ++i) before[size_t(i)] = char(i * 131 + 7);
  after = before;
  std::vector<char> fresh(size_t(len) ? size_t(len) : 1);
  for (int64_t i = 0; i < len; ++i) after[size_t(offset + i)] = fresh[size_t(i)] = char(i * 29 + 3);
  ParityDelta d;
  CHECK(make_parity_delta(offset, before.data() + offset, fresh.data(), len, &d) == TFS_SUCCESS);
  CHECK(d.units == want_units);
  CHECK(d.delta.size() == want_units.size() * 1024);
  // listed units carry before ^ after; every unit that is not listed did not change
  std::vector<char> seen(size_t(image / 1024), 0);
  for (size_t k = 0; k < d.units.size(); ++k) {
    CHECK(k == 0 || d.units[k] > d.units[k - 1]);
    seen[d.units[k]] = 1;
    for (int i = 0; i < 1024; ++i) {
      const size_t at = size_t(d.units[k]) * 1024 + size_t(i);
      CHECK(d.delta[k * 1024 + size_t(i)] == char(before[at] ^ after[at]));
    }
  }
  for (int64_t i = 0; i < image; ++i) CHECK(seen[size_t(i / 1024)] || before[size_t(i)] == after[size_t(i)]);
  ++ranges;
}

int main() {
  // the covering units and deltas
  check_range(100, 36, {0});                 // a FileInfo inside one unit
  check_range(1024 - 36, 36, {0});           // ends on a unit boundary: unit 1 is not touched
  check_range(1024, 36, {1});                // starts on one
  check_range(1024 - 20, 36, {0, 1});        // straddles: 20 bytes in unit 0, 16 in unit 1
  check_range(2 * 1024 - 1, 2, {1, 2});      // one byte on each side
  check_range(3 * 1024, 1024, {3});          // exactly one unit
  check_range(1000, 3000, {0, 1, 2, 3});     // a record over several units
  check_range(8 * 1024 - 1, 1, {7});         // the image's last byte
  check_range(500, 0, {});                   // nothing changes
  ParityDelta d;
  const char z[4] = {0, 0, 0, 0};
  CHECK(make_parity_delta(-1, z, z, 4, &d) == TFS_EXIT_PARAMETER_ERROR);
  CHECK(make_parity_delta(0, z, z, -1, &d) == TFS_EXIT_PARAMETER_ERROR);
  CHECK(make_parity_delta(0, nullptr, z, 4, &d) == TFS_EXIT_PARAMETER_ERROR);
  CHECK(make_parity_delta(0, z, nullptr, 4, &d) == TFS_EXIT_PARAMETER_ERROR);
  CHECK(make_parity_delta(int64_t(INT32_MAX) - 2, z, z, 4, &d) == TFS_EXIT_PARAMETER_ERROR);
  CHECK(make_parity_delta(0, z, z, 4, nullptr) == TFS_EXIT_PARAMETER_ERROR);
  CHECK(make_parity_delta(7, nullptr, nullptr, 0, &d) == TFS_SUCCESS && d.units.empty() && d.delta.empty());

  // the list checks: bounds before duplicates, sorted or not, both sides of the in-arguments limit
  int lists = 0;
  for (uint32_t n : {1u, 2u, 3u, 15u, 16u, 17u, 18u, 64u, 1000u}) {
    const uint32_t have = 2048;
    std::vector<uint32_t> u(n);
    std::iota(u.begin(), u.end(), 5u);
    for (uint32_t k = 0; k < n; ++k) std::swap(u[k], u[(k * 7 + 3) % n]);  // unsorted
    CHECK(update_list_check(u.data(), n, have) == 0);
    CHECK(update_list_check(u.data(), n, 5 + n) == 0);       // the last unit of the member is named
    CHECK(update_list_check(u.data(), n, 5 + n - 1) == 1);   // one unit too short
    if (n >= 2) {
      std::vector<uint32_t> dup = u;
      dup[n - 1] = dup[0];                                   // the first and the last entry
      CHECK(update_list_check(dup.data(), n, have) == 2);
      dup = u;
      dup[n / 2] = dup[n / 2 - 1];                           // neighbours
      CHECK(update_list_check(dup.data(), n, have) == 2);
      dup[0] = have;                                         // out of range and twice: the bounds come first
      CHECK(update_list_check(dup.data(), n, have) == 1);
    }
    ++lists;
  }
  CHECK(update_list_check(nullptr, 0, 0) == 0 && update_list_check(nullptr, 32, 32) == 0);
  CHECK(update_list_check(nullptr, 33, 32) == 1);
  const uint32_t top[2] = {0xFFFFFFFFu, 0u};
  CHECK(update_list_check(top, 2, 0x200000u) == 1);

  // the (p, member) mask offset, against the coder's encode bitmatrix and GF(2^8)
  const Gf256 gf;
  int coders = 0;
  for (int pn = 1; pn < kMaxMembers; ++pn)
    for (int dn = 1; dn + pn <= kMaxMembers; ++dn) {
      const BitMat enc = encode_bitmatrix(dn, pn);
      const int cols = dn * kW;
      // upload_plan's expansion of the whole plan: [pn][8][dn][8] words
      std::vector<uint32_t> plan(size_t(pn) * 8 * dn * 8);
      for (int o = 0; o < pn; ++o)
        for (int r = 0; r < 8; ++r)
          for (int s = 0; s < dn; ++s)
            for (int c = 0; c < 8; ++c)
              plan[((size_t(o) * 8 + r) * dn + s) * 8 + c] = enc[size_t(o * kW + r) * cols + s * kW + c] ? 0xFFFFFFFFu : 0u;
      for (int p = 0; p < pn; ++p)
        for (int j = 0; j < dn; ++j) {
          const int e = gf.div(1, p ^ (pn + j));  // the Cauchy element m[p][j]
          for (int sym = 1; sym < 256; sym += 23) {
            int out = 0;
            for (int r = 0; r < 8; ++r) {
              const uint32_t at = update_mask_offset(uint32_t(p), uint32_t(r), uint32_t(dn), uint32_t(j));
              CHECK(size_t(at) + 8 <= plan.size());
              int v = 0;
              for (int c = 0; c < 8; ++c) {
                CHECK(plan[at + c] == 0u || plan[at + c] == 0xFFFFFFFFu);
                v ^= int(plan[at + c] & 1u) & ((sym >> c) & 1);
              }
              out |= v << r;
            }
            CHECK(out == gf.mul(e, sym));
          }
        }
      ++coders;
    }
  printf("update delta ok: %d ranges, %d lists, %d coders\n", ranges, lists, coders);
  return 0;
}
