// parity_update.h -- a change made in place to one data member of a family, as the
// parity members need it (include/tfs_ec.h, tfs_ec_update): the 1 KiB
// units the changed range covers and the delta old ^ new of each, zero outside the range.
// Pure host code over the C headers, like scrub_classify.h: tools/update_delta_check.cpp
// builds it alone under the host sanitizers.  write_member_range and unlink_file_family
// (ds_harness.cpp) run it over a family.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tfs_ec.h"

namespace tfs {
namespace dataserver {

struct Family;

// What a parity server needs of one change: units ascending, delta[k] the 1,024 bytes of unit
// units[k].  This is what travels with the request that reaches the parity servers.
struct ParityDelta {
  std::vector<uint32_t> units;
  std::vector<char> delta;  // units.size() * 1024 bytes
};

// The delta of `len` bytes at `offset` of a data member that change from old_bytes to
// new_bytes.  A range that ends on a unit boundary does not reach into the next unit; a
// 36-byte FileInfo that straddles one gives two units.  len == 0 gives no unit.  Returns
// TFS_SUCCESS, or TFS_EXIT_PARAMETER_ERROR for a negative offset or length, a range that
// passes 2^31 or missing bytes.
inline int make_parity_delta(int64_t offset, const char* old_bytes, const char* new_bytes, int64_t len, ParityDelta* out) {
  if (!out || offset < 0 || len < 0 || offset > INT32_MAX - len || (len && (!old_bytes || !new_bytes)))
    return TFS_EXIT_PARAMETER_ERROR;
  out->units.clear();
  out->delta.clear();
  if (len == 0) return TFS_SUCCESS;
  const int64_t u0 = offset / TFS_EC_UNIT, u1 = (offset + len - 1) / TFS_EC_UNIT;
  for (int64_t u = u0; u <= u1; ++u) out->units.push_back(uint32_t(u));
  out->delta.assign(size_t(u1 - u0 + 1) * TFS_EC_UNIT, 0);
  char* d = out->delta.data() + (offset - u0 * TFS_EC_UNIT);
  for (int64_t i = 0; i < len; ++i) d[i] = char(old_bytes[i] ^ new_bytes[i]);
  return TFS_SUCCESS;
}

// images[i] is the writable view of family.members[i]: the data member's image and every parity
// member this server holds (NULL for a parity member it does not hold; other data members are
// not looked at).  The `len` bytes at `offset` of data member `member` (inside its size) are
// replaced by `bytes`, and the change is carried into every parity member held, through one
// tfs_ec_update call with the delta alone; the parity is updated first, and on a failure the
// data member is left as it was.  Parity members are at least the family's encode length (the
// longest data member rolled up to 1,024).  Returns the number of units updated, or a negative
// status (no parity member held: TFS_EXIT_DATA_INVALID, tfs_ec_update's).
int write_member_range(tfs_crc_ctx* ctx, const Family& family, char* const* images, int member, int64_t offset,
                       const char* bytes, int64_t len);

// Step 5 of LogicBlock::unlink_file (logic_block.cpp:649-656) on a block that belongs to a
// family: the FileInfo of file_id, at its offset in `index` (block block_id's index), is
// rewritten with modify_time_ = modify_time (the reference takes time(NULL)) through
// write_member_range, so the parity follows -- which the reference's unlink_file_parity
// (:539-577) leaves out.  The flag lives in the index (RawMeta::set_unlink_flag, :646) and
// stays the caller's.  A block that is not a data member of the family is
// EXIT_BLOCK_NOT_PRESENT, a missing id EXIT_META_NOT_FOUND_ERROR.  Returns the number of
// units updated (1, or 2 for a FileInfo that straddles a unit boundary), or a negative status.
int unlink_file_family(tfs_crc_ctx* ctx, const Family& family, char* const* images, const std::vector<tfs_raw_meta>& index,
                       uint32_t block_id, uint64_t file_id, int32_t modify_time);

}  // namespace dataserver
}  // namespace tfs
