// replicate.h -- ReplicateTask::do_replicate over a LogicBlockImage (task.cpp:
// 1025-1090; the same loop moves a block during balancing) through a replicate
// session (include/tfs_replicate.h): the data file is read in
// calls of frames_per_call frames, every finished WriteRawDataMessage frame goes to
// the sink in order (the place of Task::write_raw_data's post, task.cpp:86-113),
// and after the last one every record has been checked against its own
// FileInfo.crc_ from the same single read.  The commit callback -- the place of
// batch_write_index -- is called only when no record failed; otherwise the block
// was sent but is not committed, the first failing record's status is returned with
// the full verdict list, and each TFS_EXIT_CHECK_CRC_ERROR is counted in
// BlockCrcChecker, as read_file_verified does.  Records flagged FI_DELETED or
// FI_INVALID travel like any gap, as verify_block leaves them out.  Building the
// WriteInfoBatchMessage is the caller's.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/tfs_replicate.h"
#include "ds_harness.h"

namespace tfs {
namespace dataserver {

struct ReplicateOptions {
  uint32_t dest_block_id = 0;             // WriteDataInfo.block_id_
  uint64_t packet_id = 0;                 // frame k carries packet_id + k
  int32_t frame_len = TFS_MAX_READ_SIZE;  // MAX_READ_SIZE
  int32_t frames_per_call = 8;
  int16_t new_block = TFS_RAW_NORMAL_DATA;
  int16_t version = 2;
};

struct ReplicateResult {
  std::vector<tfs_raw_meta> metas;  // the records that were checked, in offset order
  std::vector<int32_t> status;      // one per meta
  std::vector<uint32_t> crc;
  std::vector<uint32_t> frame_crc;  // one per frame of the block
  uint32_t n_bad = 0;
  uint32_t frames_sent = 0;
  bool committed = false;
};

// (frame index, frame, bytes) -> TFS_SUCCESS, or the code the replication ends with.
using ReplicateSink = std::function<int(uint32_t, const char*, uint32_t)>;
using ReplicateCommit = std::function<int(const ReplicateResult&)>;

inline int replicate_block(tfs_crc_ctx* ctx, const LogicBlockImage& block, const ReplicateOptions& opt,
                           const ReplicateSink& sink, const ReplicateCommit& commit, ReplicateResult* res,
                           BlockCrcChecker* checker) {
  if (!ctx || !res || !sink || opt.frames_per_call <= 0) return TFS_EXIT_PARAMETER_ERROR;
  *res = ReplicateResult();
  for (const tfs_raw_meta& m : block.sorted_metas())
    if (!(block.flag_of(m.file_id) & (TFS_FI_DELETED | TFS_FI_INVALID))) res->metas.push_back(m);
  tfs_replicate_cfg cfg{};
  cfg.packet_id = opt.packet_id, cfg.block_id = opt.dest_block_id;
  cfg.total = int32_t(block.data_size()), cfg.frame_len = opt.frame_len;
  cfg.new_block = opt.new_block, cfg.version = opt.version;
  tfs_replicate* s = nullptr;
  int rc = tfs_replicate_begin(ctx, &cfg, res->metas.data(), uint32_t(res->metas.size()), &s);
  if (rc != TFS_SUCCESS) return rc;
  const int64_t total = cfg.total, fl = cfg.frame_len, stride = fl + TFS_RAW_FRAME_OVERHEAD;
  const int64_t step = fl * opt.frames_per_call;
  std::vector<char> out(size_t(std::min<int64_t>(opt.frames_per_call, tfs_replicate_frame_count(&cfg)) * stride));
  const char* image = block.data().data();
  int64_t off = 0;
  do {  // (runs once for an empty data file, task.cpp:1050-1076)
    const int64_t len = std::min(step, total - off);
    rc = tfs_replicate_frames(s, len ? image + off : nullptr, int(off), int(len), out.data(), out.size());
    if (rc != TFS_SUCCESS) break;
    const int64_t nf = std::max<int64_t>(1, (len + fl - 1) / fl);
    for (int64_t j = 0; j < nf && rc == TFS_SUCCESS; ++j) {
      const int64_t dlen = std::min(fl, len - j * fl);
      rc = sink(uint32_t(off / fl + j), out.data() + j * stride, uint32_t(TFS_RAW_FRAME_OVERHEAD + dlen));
      if (rc == TFS_SUCCESS) ++res->frames_sent;
    }
    off += len;
  } while (rc == TFS_SUCCESS && off < total);
  if (rc == TFS_SUCCESS) {
    res->status.assign(res->metas.size(), 0);
    res->crc.assign(res->metas.size(), 0);
    res->frame_crc.assign(tfs_replicate_frame_count(&cfg), 0);
    rc = tfs_replicate_finish(s, res->crc.data(), res->status.data(), &res->n_bad, res->frame_crc.data());
  }
  tfs_replicate_free(s);
  if (rc != TFS_SUCCESS) return rc;
  int first = TFS_SUCCESS;
  for (size_t i = 0; i < res->metas.size(); ++i) {
    if (res->status[i] == TFS_EXIT_CHECK_CRC_ERROR && checker)
      checker->add_crc_error(block.block_id(), res->metas[i].file_id);
    if (first == TFS_SUCCESS) first = res->status[i];
  }
  if (first != TFS_SUCCESS) return first;
  if (commit) rc = commit(*res);
  res->committed = rc == TFS_SUCCESS;
  return rc;
}

}  // namespace dataserver
}  // namespace tfs
