// receive.h -- the handler pair DataService::write_raw_data / batch_write_info
// (dataservice.cpp:2487-2566) over a new LogicBlockImage through a receive session
// (include/tfs_receive.h).  The source yields reads: a buffer and
// the WriteRawDataMessage frames in it.  Every read is parsed with
// tfs_receive_parse and landed through the session; the first frame whose status
// is not TFS_SUCCESS ends the receive with that status (the place of
// reply_error_packet), and so does a flag_ other than 0 on a frame at offset > 0 or
// other than TFS_RAW_NORMAL_DATA / TFS_RAW_PARITY_DATA on the frame at 0
// (TFS_EXIT_PARAMETER_ERROR).  After the last read the caller's metas -- the
// WriteInfoBatchMessage's RawMetaVec -- go to finish.  The commit callback, the
// place of LogicBlock::batch_write_meta (logic_block.cpp:817-858), runs only when no
// record failed; otherwise the first failing record's status is returned with the
// full verdict list and each TFS_EXIT_CHECK_CRC_ERROR is counted in BlockCrcChecker,
// as replicate_block does.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/tfs_receive.h"
#include "../../include/tfs_replicate.h"
#include "ds_harness.h"

namespace tfs {
namespace dataserver {

struct ReceiveOptions {
  uint32_t block_id = 0;                   // WriteDataInfo.block_id_ every frame must carry
  int32_t image_cap = 64 * 1024 * 1024;    // bytes the new block can hold
  std::vector<tfs_raw_meta> metas;         // the RawMetaVec, any order
};

struct ReceiveRead {
  const char* buf = nullptr;         // host memory
  uint64_t len = 0;
  std::vector<uint64_t> frame_offs;  // the frames in it, in order
};

struct ReceiveResult {
  ByteImage image;                      // the landed bytes (filled when every frame succeeded)
  std::vector<tfs_receive_part> parts;  // one per frame landed
  std::vector<int32_t> status;          // one per meta, the caller's order
  std::vector<uint32_t> crc;
  uint32_t n_bad = 0;
  int32_t total = 0;
  int32_t new_block = 0;                // flag_ of the frame at offset 0
  bool committed = false;
};

// Fills *read with the next read; false when the sender is done.
using ReceiveSource = std::function<bool(ReceiveRead*)>;
using ReceiveCommit = std::function<int(ReceiveResult&)>;

inline int receive_block(tfs_crc_ctx* ctx, const ReceiveOptions& opt, const ReceiveSource& source,
                         const ReceiveCommit& commit, ReceiveResult* res, BlockCrcChecker* checker) {
  if (!ctx || !res || !source) return TFS_EXIT_PARAMETER_ERROR;
  *res = ReceiveResult();
  void* d_image = nullptr;
  int rc = opt.image_cap > 0 ? tfs_crc32_dev_malloc(ctx, uint64_t(opt.image_cap), &d_image) : TFS_SUCCESS;
  if (rc != TFS_SUCCESS) return rc;
  tfs_receive_cfg cfg{};
  cfg.block_id = opt.block_id, cfg.image_cap = opt.image_cap;
  tfs_receive* s = nullptr;
  rc = tfs_receive_begin(ctx, &cfg, d_image, &s);
  ReceiveRead rd;
  std::vector<tfs_receive_desc> descs;
  while (rc == TFS_SUCCESS && source(&rd)) {
    descs.resize(rd.frame_offs.size());
    for (size_t j = 0; j < descs.size() && rc == TFS_SUCCESS; ++j) {
      const uint64_t off = rd.frame_offs[j];
      if (!rd.buf || off > rd.len) rc = TFS_EXIT_PARAMETER_ERROR;
      else if (tfs_receive_parse(rd.buf + off, uint32_t(std::min<uint64_t>(rd.len - off, UINT32_MAX)), off, &descs[j]))
        rc = TFS_ERROR;  // a frame cut short: the streamer would still be waiting for it
    }
    if (rc != TFS_SUCCESS || descs.empty()) continue;
    const size_t at = res->parts.size();
    res->parts.resize(at + descs.size());
    uint32_t bad = 0;
    rc = tfs_receive_frames(s, rd.buf, rd.len, descs.data(), uint32_t(descs.size()), res->parts.data() + at, &bad);
    if (rc != TFS_SUCCESS) {
      res->parts.resize(at);
      break;
    }
    for (size_t j = 0; j < descs.size() && rc == TFS_SUCCESS; ++j) {
      const tfs_receive_part& p = res->parts[at + j];
      if (p.status != TFS_SUCCESS) rc = p.status;
      else if (at + j == 0) {  // the frame at offset 0
        if (p.flag != TFS_RAW_NORMAL_DATA && p.flag != TFS_RAW_PARITY_DATA) rc = TFS_EXIT_PARAMETER_ERROR;
        res->new_block = p.flag;
      } else if (p.flag != 0) {
        rc = TFS_EXIT_PARAMETER_ERROR;
      }
      if (rc != TFS_SUCCESS) res->parts.resize(at + j + 1);  // the receive ends at this frame
    }
  }
  if (rc == TFS_SUCCESS && s) {
    const uint32_t n = uint32_t(opt.metas.size());
    res->status.assign(n, 0);
    res->crc.assign(n, 0);
    rc = tfs_receive_finish(s, opt.metas.data(), n, res->crc.data(), res->status.data(), &res->n_bad, &res->total);
    if (rc == TFS_SUCCESS && res->total > 0) {
      res->image.resize(size_t(res->total));
      rc = tfs_crc32_memcpy(ctx, res->image.data(), d_image, uint64_t(res->total), nullptr);
    }
  }
  if (s) tfs_receive_free(s);
  if (d_image) tfs_crc32_dev_free(ctx, d_image);
  if (rc != TFS_SUCCESS) return rc;
  int first = TFS_SUCCESS;
  for (size_t i = 0; i < res->status.size(); ++i) {
    if (res->status[i] == TFS_EXIT_CHECK_CRC_ERROR && checker) checker->add_crc_error(opt.block_id, opt.metas[i].file_id);
    if (first == TFS_SUCCESS) first = res->status[i];
  }
  if (first != TFS_SUCCESS) return first;
  if (commit) rc = commit(*res);
  res->committed = rc == TFS_SUCCESS;
  return rc;
}

}  // namespace dataserver
}  // namespace tfs
