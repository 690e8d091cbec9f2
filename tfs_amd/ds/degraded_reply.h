// degraded_reply.h -- DataService::read_data_degrade (dataservice.cpp:1713-1796) over a
// Family and the lost block's parity index, with the reply made in one pass (include/
// tfs_ec_read.h): a batch of read requests of one LOST block becomes one
// tfs_ec_read_reply call, which rebuilds each file's bytes from the survivors, checks
// them against the rebuilt FileInfo and leaves the sealed RESP_READ_DATA_MESSAGE(_V2/_V3)
// frame ready to send -- the alloc_data / read_data_degrade / reply triple as one call
// that writes into the connection's output buffer.
//
// A file that is not in the index (EXIT_META_NOT_FOUND_ERROR) never reaches the job
// list: its set_length(status) frame is sealed by PacketEncoder with the others of the
// batch, as reply_reads does.  The flag lives in the lost block, so it is the kernel
// that refuses a first fragment: refuse_flags is deleted | invalid | concealed, and
// invalid alone with `force` (EXIT_FILE_INFO_ERROR, a sealed error frame).  A job that
// ends in TFS_EXIT_CHECK_CRC_ERROR -- a corrupt survivor -- is counted in
// BlockCrcChecker under the lost block's id.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/tfs_ec_read.h"
#include "read_reply.h"

namespace tfs {
namespace dataserver {

struct Family;
class BlockCrcChecker;

// Returns the number of requests whose status is not TFS_SUCCESS, or a negative code
// when the call itself failed: the family's (EXIT_NO_ENOUGH_DATA, EXIT_BLOCK_NOT_PRESENT,
// as read_data_degrade), parameters, device.  `index` is the lost block's RawMeta list
// as a parity block keeps it.  Each frame is placed so that frame + 28 is congruent mod
// 16 to the slice's first byte in the lost member (offset + 36 + read_offset).
int reply_reads_degrade(tfs_crc_ctx* ctx, const Family& family, uint32_t block_id,
                        const std::vector<tfs_raw_meta>& index, const std::vector<ReadRequest>& requests,
                        ReadReplies* out, BlockCrcChecker* checker);

}  // namespace dataserver
}  // namespace tfs
