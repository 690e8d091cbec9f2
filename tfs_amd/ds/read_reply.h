// read_reply.h -- DataService::read_data / read_data_extra over a LogicBlockImage
// (dataservice.cpp:1466-1700) with the reply made in one pass (include/tfs_read.h,
// DESIGN.md §3.17): a batch of read requests of one block becomes one
// tfs_read_reply call, which checks each file against FileInfo.crc_ and leaves the
// sealed RESP_READ_DATA_MESSAGE(_V2/_V3) frame ready to send.
//
// A request that LogicBlock::read_file rejects before it reads (logic_block.cpp:
// 374-435) never reaches the job list: a file that is not in the index
// (EXIT_META_NOT_FOUND_ERROR) and, on the first fragment, one that is deleted,
// invalid or concealed -- only invalid with `force` (EXIT_FILE_INFO_ERROR).  Its
// set_length(status) frame is sealed by PacketEncoder with the others of the batch.
// A job that ends in TFS_EXIT_CHECK_CRC_ERROR is counted in BlockCrcChecker, as
// read_file_verified does.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/tfs_read.h"

namespace tfs {
namespace dataserver {

class LogicBlockImage;
class BlockCrcChecker;

struct ReadRequest {     // 32 bytes
  uint64_t file_id;
  uint64_t packet_id;    // header id of the reply
  int32_t read_offset;   // into the file's data
  int32_t read_len;
  int16_t pcode;         // TFS_RESP_READ_DATA_MESSAGE, _V2 or _V3
  int16_t version;       // the request's
  int32_t force;         // READ_DATA_OPTION_FLAG_FORCE: serve deleted and concealed files
};

struct ReadReply {       // 24 bytes
  int32_t status;        // TFS_SUCCESS, tfs_read_reply's codes, or read_file's for a request rejected before reading
  uint32_t frame_len;    // bytes to send
  uint32_t file_crc;     // Func::crc(0, payload) when the whole file was read
  uint32_t frame_crc;    // the header's crc
  int64_t frame_offset;  // of the frame in ReadReplies::frames
};

struct ReadReplies {
  std::vector<char> frames;        // every request's frame, in request order, each at its frame_offset
  std::vector<ReadReply> replies;  // one per request
};

// Returns the number of requests whose status is not TFS_SUCCESS, or a negative
// code when the call itself failed (parameters, device).  Each frame starts where
// its data lands on the source's address mod 16 (the whole-line store path).
int reply_reads(tfs_crc_ctx* ctx, const LogicBlockImage& block, const std::vector<ReadRequest>& requests,
                ReadReplies* out, BlockCrcChecker* checker);

}  // namespace dataserver
}  // namespace tfs
