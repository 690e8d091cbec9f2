// ec_frames.h -- the erasure-code tasks with their posts: MarshallingTask::
// do_marshalling's data loop (task.cpp:1210-1291) and ReinstateTask::do_reinstate's
// (task.cpp:1420-1529) over the frame-emitting chunk calls of the sessions
// (include/tfs_ec_frames.h).  They are do_marshalling / do_reinstate
// of ds_harness.h -- the same members, lengths, zero-filling and record verdicts --
// with one difference: where those copy each parity or rebuilt piece into the
// caller's buffer, these hand every finished WriteRawDataMessage frame of every
// output member to a sink, in the place of Task::write_raw_data's post (task.cpp:
// 86-113): PARITY_DATA on a parity member's first frame (:1272-1281, :1505-1519),
// NORMAL_DATA on a rebuilt data member's (:1484-1498).  The coded bytes are made,
// framed and checksummed in one pass on the GPU; the host never touches them.
//
// Pieces of chunk_len bytes (a multiple of frame_len) are read into chunk buffers
// reused piece after piece; after each piece the sink is called for member after
// member, frame after frame.  A sink that does not return TFS_SUCCESS ends the task
// with its code.  The reaction to records that did not verify is the caller's, as
// in do_marshalling / do_reinstate: the return value counts them.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/tfs_ec_frames.h"
#include "ds_harness.h"

namespace tfs {
namespace dataserver {

struct EcFramesOptions {
  int32_t frame_len = TFS_MAX_READ_SIZE;  // MAX_READ_SIZE; a multiple of 4096
  int32_t chunk_len = TFS_MAX_READ_SIZE;  // bytes of every member per piece; a multiple of frame_len
  int16_t version = 2;
  std::vector<uint64_t> packet_id;        // by member index: frame k of member i carries packet_id[i] + k (empty: 0)
};

// (member index, frame index in the member, frame, bytes) -> TFS_SUCCESS, or the code the task ends with.
using EcFrameSink = std::function<int(int, uint32_t, const char*, uint32_t)>;

// do_marshalling with a sink per (parity member, frame); the frames carry the members' block ids.
int do_marshalling_frames(tfs_crc_ctx* ctx, const Family& family, const std::vector<std::vector<tfs_raw_meta>>& indexes,
                          const EcFramesOptions& opt, const EcFrameSink& sink, int32_t* total,
                          std::vector<int32_t>* status);

// do_reinstate with a sink per (dead member, frame).  Nothing dead: TFS_SUCCESS, *total = 0, no frame.
int do_reinstate_frames(tfs_crc_ctx* ctx, const Family& family, const std::vector<std::vector<tfs_raw_meta>>& indexes,
                        const EcFramesOptions& opt, const EcFrameSink& sink, int32_t* total,
                        std::vector<int32_t>* status);

}  // namespace dataserver
}  // namespace tfs
