// scrub_classify.h -- the verdict over a scrub session's results (include/tfs_ec.h,
// tfs_ec_scrub_finish): which member a flagged unit points at.
// Pure host code over the C headers, no device and no library: tools/scrub_classify_check.cpp
// builds it alone under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tfs_ec.h"

namespace tfs {
namespace dataserver {

// What a scrub of one family found (scrub_family, classify_scrub).
struct ScrubReport {
  std::vector<int32_t> status;              // one entry per index entry, member 0's first (tfs_ec_scrub_finish)
  uint32_t bad_records = 0;                 // entries of status that are not TFS_SUCCESS
  uint32_t flagged_units = 0;               // 1 KiB units in which at least one parity member differs
  std::vector<uint32_t> failed_records;     // [dn]: records of data member i that failed FILE_INFO, SYNC_FILE or CHECK_CRC
  std::vector<uint32_t> data_units;         // [dn]: units flagged in every parity member that a failed record of i meets
  std::vector<uint32_t> parity_only_units;  // [pn]: units flagged in parity member p and not in all of them
  uint32_t unattributed_units = 0;          // units flagged in every parity member that no failed record meets
  std::vector<uint8_t> suspect;             // [dn + pn]: a failed record or a non-zero counter
  int findings() const { return int(bad_records + flagged_units); }
};

// The verdict over a scrub session's results; pure host code, no device.  status holds one
// entry per index entry (member 0's first), tile_map pn rows of ceil(total / 4096) bytes
// (tfs_ec_scrub_finish).  For each 1 KiB unit, let F be the parity members flagged there:
//   F empty: nothing.
//   pn >= 2 and F a proper subset: parity_only_units[p]++ for p in F -- the data and the
//     other parity members agree, so parity p is wrong or stale there.
//   F all of them (pn == 1 included): data_units[i]++ for every data member i that has a
//     record that failed (TFS_EXIT_FILE_INFO_ERROR, TFS_EXIT_SYNC_FILE_ERROR or
//     TFS_EXIT_CHECK_CRC_ERROR) and whose [offset, offset + size) meets the unit; if there
//     is none, unattributed_units++: a gap, a deleted record, or with pn == 1 the parity
//     itself.
// The ground: every coefficient of the Cauchy matrix is non-zero, so its 8 x 8 bit matrix
// is invertible, and a wrong data byte changes every parity member in the same unit; a
// unit that only some parity members disagree on therefore has its data intact.  Locating
// the data member of an unattributed unit from the syndromes is not done here.
// A member is suspect when it has a failed record or a non-zero counter.
inline ScrubReport classify_scrub(int dn, int pn, int32_t total, const std::vector<std::vector<tfs_raw_meta>>& indexes,
                                  const std::vector<int32_t>& status, const std::vector<uint8_t>& tile_map) {
  ScrubReport r;
  r.status = status;
  r.failed_records.assign(size_t(dn), 0);
  r.data_units.assign(size_t(dn), 0);
  r.parity_only_units.assign(size_t(pn), 0);
  r.suspect.assign(size_t(dn + pn), 0);
  const int64_t units = total / TFS_EC_UNIT;
  const size_t ntiles = size_t((int64_t(total) + 4095) / 4096);
  // hit[i][U]: a failed record of data member i meets unit U (only members with a failed record have a row)
  std::vector<std::vector<uint8_t>> hit(static_cast<size_t>(dn));
  size_t at = 0;
  for (int i = 0; i < dn; ++i) {
    for (const tfs_raw_meta& m : indexes[size_t(i)]) {
      const int32_t st = at < status.size() ? status[at] : TFS_SUCCESS;
      ++at;
      if (st != TFS_SUCCESS) ++r.bad_records;
      if (st != TFS_EXIT_FILE_INFO_ERROR && st != TFS_EXIT_SYNC_FILE_ERROR && st != TFS_EXIT_CHECK_CRC_ERROR) continue;
      ++r.failed_records[size_t(i)];
      // a record that failed took part in the pass: 0 <= offset, size > 36, offset + size <= block_len <= total
      const int64_t lo = int64_t(m.offset) / TFS_EC_UNIT, hi = (int64_t(m.offset) + m.size - 1) / TFS_EC_UNIT;
      if (hit[size_t(i)].empty()) hit[size_t(i)].assign(size_t(units), 0);
      for (int64_t u = std::max<int64_t>(lo, 0); u <= hi && u < units; ++u) hit[size_t(i)][size_t(u)] = 1;
    }
  }
  for (int64_t u = 0; u < units; ++u) {
    int flagged = 0;
    for (int p = 0; p < pn; ++p) flagged += (tile_map[size_t(p) * ntiles + size_t(u >> 2)] >> (u & 3)) & 1;
    if (!flagged) continue;
    ++r.flagged_units;
    if (flagged < pn) {
      for (int p = 0; p < pn; ++p)
        if ((tile_map[size_t(p) * ntiles + size_t(u >> 2)] >> (u & 3)) & 1) ++r.parity_only_units[size_t(p)];
      continue;
    }
    bool named = false;
    for (int i = 0; i < dn; ++i)
      if (!hit[size_t(i)].empty() && hit[size_t(i)][size_t(u)]) {
        ++r.data_units[size_t(i)];
        named = true;
      }
    if (!named) ++r.unattributed_units;
  }
  for (int i = 0; i < dn; ++i) r.suspect[size_t(i)] = r.failed_records[size_t(i)] || r.data_units[size_t(i)];
  for (int p = 0; p < pn; ++p) r.suspect[size_t(dn + p)] = r.parity_only_units[size_t(p)] != 0;
  return r;
}

}  // namespace dataserver
}  // namespace tfs
