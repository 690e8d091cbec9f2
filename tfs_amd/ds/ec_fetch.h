// ec_fetch.h -- the erasure-code tasks with their fetches and their posts:
// MarshallingTask::do_marshalling's data loop (task.cpp:1210-1291) and
// ReinstateTask::do_reinstate's (task.cpp:1420-1529) over the task chunk calls of the
// sessions (include/tfs_ec_fetch.h).  They are do_marshalling_frames /
// do_reinstate_frames of ec_frames.h -- the same members, lengths, frames and record
// verdicts -- with one difference: where those read each source piece from local
// bytes, these call a fetch per (member, frame) in the place of Task::read_raw_data
// (task.cpp:115-169, bound at :1235 and :1448) and pass the RespReadRawDataMessage
// frame it hands back to the session unopened.  The frame is checked, its data coded
// and the outputs' frames sealed in one pass on the GPU; the host copies no data
// byte out of a frame and zero-fills nothing.
//
// A frame whose member ends at or before its offset is not fetched (:1233).  A fetch
// that does not return TFS_SUCCESS ends the task with its code, as :1254-1257 does;
// so does a frame that is the source's error reply (its negative length), half a
// frame (TFS_ERROR) and a frame that fails the session's check (TFS_ERROR or
// TFS_EXIT_CHECK_CRC_ERROR) -- in each case before anything of that chunk reaches
// the sink.  Only the members' block ids and sizes are read from the family: a
// member with size > 0 is present, its bytes live with the server the fetch asks.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/tfs_ec_fetch.h"
#include "ec_frames.h"

namespace tfs {
namespace dataserver {

// (member index, frame index in the member, member offset, bytes asked for, frame buffer, its capacity -- 32 +
// the bytes asked for --, *bytes written) -> TFS_SUCCESS, or the code the task ends with.
using EcFrameFetch = std::function<int(int, uint32_t, int32_t, int32_t, char*, uint32_t, uint32_t*)>;

// do_marshalling_frames with a fetch per (data member, frame).
int do_marshalling_task(tfs_crc_ctx* ctx, const Family& family, const std::vector<std::vector<tfs_raw_meta>>& indexes,
                        const EcFramesOptions& opt, const EcFrameFetch& fetch, const EcFrameSink& sink, int32_t* total,
                        std::vector<int32_t>* status);

// do_reinstate_frames with a fetch per (survivor, frame).  Nothing dead: TFS_SUCCESS, *total = 0, no fetch, no frame.
int do_reinstate_task(tfs_crc_ctx* ctx, const Family& family, const std::vector<std::vector<tfs_raw_meta>>& indexes,
                      const EcFramesOptions& opt, const EcFrameFetch& fetch, const EcFrameSink& sink, int32_t* total,
                      std::vector<int32_t>* status);

}  // namespace dataserver
}  // namespace tfs
