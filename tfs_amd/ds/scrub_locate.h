// scrub_locate.h -- after a scrub: the data member behind a unit that every parity member
// flags, and that member's right bytes (include/tfs_ec.h, tfs_ec_locate).
// The verdict part -- which units to ask about, and the report over the answers -- is pure
// host code over the C headers, like scrub_classify.h; locate_family and scrub_and_locate
// (ds_harness.cpp) run it over a family.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tfs_ec.h"
#include "scrub_classify.h"

namespace tfs {
namespace dataserver {

struct Family;

// The right bytes of one 1 KiB unit of one data member.  bytes past the member's own length
// are what the code yields -- zero for a true single-member fault -- and the caller writes
// only up to the member's length.  confirmed: the family has three or more parity members,
// so no two wrong data members can look like this one (include/tfs_ec.h); an unconfirmed
// patch is a proposal, to be written only when the records over the unit verify afterwards.
struct UnitPatch {
  int member = -1;
  uint32_t unit = 0;
  uint16_t diff_bytes = 0;  // bytes of the unit that the patch changes
  bool confirmed = false;
  std::array<char, 1024> bytes{};
};

struct LocateReport {
  std::vector<uint32_t> located_units;  // [dn]: units in which data member i alone is wrong
  uint32_t unlocated_units = 0;         // flagged in every parity member, result NONE: more than one member wrong
  uint32_t examined_units = 0;          // units flagged in every parity member
  std::vector<UnitPatch> patches;       // one per DATA result, ascending (member, unit)
};

// The units of a scrub session's tile map (pn rows of ceil(total / 4096) bytes) that every
// parity member flags, ascending: classify_scrub's "F all of them".
inline std::vector<uint32_t> units_flagged_everywhere(int pn, int32_t total, const std::vector<uint8_t>& tile_map) {
  std::vector<uint32_t> out;
  const int64_t units = total / TFS_EC_UNIT;
  const size_t ntiles = size_t((int64_t(total) + 4095) / 4096);
  for (int64_t u = 0; u < units; ++u) {
    int flagged = 0;
    for (int p = 0; p < pn; ++p) flagged += (tile_map[size_t(p) * ntiles + size_t(u >> 2)] >> (u & 3)) & 1;
    if (flagged == pn) out.push_back(uint32_t(u));
  }
  return out;
}

// The report over tfs_ec_locate's answers for `units` (entry k is unit units[k]; fixed holds
// 1,024 bytes per entry).  A PARITY or CLEAN answer for a unit the map flagged everywhere
// means the members changed since the scrub; it is counted nowhere but in examined_units.
inline void fill_locate_report(int dn, const std::vector<uint32_t>& units, const std::vector<tfs_ec_locate_result>& res,
                               const std::vector<char>& fixed, LocateReport* r) {
  r->located_units.assign(size_t(dn), 0);
  r->unlocated_units = 0;
  r->examined_units = uint32_t(units.size());
  r->patches.clear();
  for (size_t k = 0; k < units.size(); ++k) {
    if (res[k].kind == TFS_EC_LOCATE_NONE) ++r->unlocated_units;
    if (res[k].kind != TFS_EC_LOCATE_DATA || res[k].member < 0 || res[k].member >= dn) continue;
    ++r->located_units[size_t(res[k].member)];
    UnitPatch p;
    p.member = res[k].member;
    p.unit = units[k];
    p.diff_bytes = res[k].diff_bytes;
    p.confirmed = (res[k].flags & TFS_EC_LOCATE_CONFIRMED) != 0;
    memcpy(p.bytes.data(), fixed.data() + k * TFS_EC_UNIT, TFS_EC_UNIT);
    r->patches.push_back(p);
  }
  std::stable_sort(r->patches.begin(), r->patches.end(), [](const UnitPatch& a, const UnitPatch& b) {
    return a.member != b.member ? a.member < b.member : a.unit < b.unit;
  });
}

// For a family that was scrubbed (total and tile_map as scrub_family's session gave them, every
// member present): the units flagged in every parity member are gathered from the members,
// short data members zero-extended, and asked about in one tfs_ec_locate call.  pn < 2
// returns TFS_SUCCESS with examined_units = 0: nothing can be located.  Otherwise returns the
// number of NONE units, or a negative status.  Nothing is written: applying the patches is
// the dataserver's.
int locate_family(tfs_crc_ctx* ctx, const Family& family, int32_t total, const std::vector<uint8_t>& tile_map,
                  LocateReport* report);

// scrub_family, then locate_family over its tile map.  *scrub is exactly scrub_family's report.
// Returns locate_family's value, or the scrub's negative status.
int scrub_and_locate(tfs_crc_ctx* ctx, const Family& family, const std::vector<std::vector<tfs_raw_meta>>& indexes,
                     int32_t chunk_len, int32_t* total, ScrubReport* scrub, LocateReport* located);

}  // namespace dataserver
}  // namespace tfs
