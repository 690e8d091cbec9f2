// mirror_sync.h -- TfsMirrorBackup::copy_file over a LogicBlockImage
// (sync_backup.cpp:315-472) through one mirror sync call (include/tfs_mirror.h,
// DESIGN.md §3.21): a batch from the sync queue -- file ids of one block, each with
// the destination's file_number, ds list and packet id -- is read once; every file is
// checked against its own FileInfo.crc_ and its sealed WriteDataMessage frames are
// left ready to send in the same pass.
//
// A file id that is not in the index is "need not sync" (file_not_exist,
// sync_backup.cpp:452-455): it counts as success and nothing is sent.  The first
// read is READ_DATA_OPTION_FLAG_FORCE, so only FI_INVALID refuses a file
// (logic_block.cpp:416-424), as the `force` case of read_reply.h does.  For a file
// that passes, its frames go to the sink in order and then close(file, file_crc) is
// called: the place of CloseFileMessage.set_crc, with the CRC of the bytes that were
// sent.  For a file that fails neither callback is called; its status is recorded,
// and a TFS_EXIT_CHECK_CRC_ERROR is counted in BlockCrcChecker, as
// read_file_verified does.  The reference sends first and compares last (:429), and
// closes the destination file anyway (:438-439).
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

#include "../../include/tfs_mirror.h"
#include "ds_harness.h"

namespace tfs {
namespace dataserver {

struct MirrorFile {
  uint64_t file_id = 0;
  uint64_t file_number = 0;  // from the destination's create-file reply
  uint64_t packet_id = 0;    // frame k of the file carries packet_id + k
  std::vector<uint64_t> ds;  // ds_ of its WriteDataMessages, the lease entries appended by the caller
};

struct MirrorOptions {
  uint32_t dest_block_id = 0;                // WriteDataInfo.block_id_
  int32_t first_len = TFS_MAX_READ_SIZE - TFS_FILEINFO_SIZE;
  int32_t frame_len = TFS_MAX_READ_SIZE;
  int32_t is_server = 0;
  int16_t version = 2;
};

struct MirrorFileResult {
  int32_t status = TFS_SUCCESS;
  uint32_t n_frames = 0;   // frames sent
  uint32_t file_crc = 0;   // Func::crc(0, payload) as recomputed
  int32_t skipped = 0;     // 1: not in the index, need not sync
};

struct MirrorResult {
  std::vector<MirrorFileResult> files;  // one per MirrorFile
  uint32_t n_bad = 0;
  uint32_t frames_sent = 0;
  uint32_t closed = 0;
};

// (index into files, frame of the file, frame, bytes) -> TFS_SUCCESS, or the code the batch ends with.
using MirrorSink = std::function<int(size_t, uint32_t, const char*, uint32_t)>;
// (index into files, file CRC) -> TFS_SUCCESS, or the code the batch ends with.
using MirrorClose = std::function<int(size_t, uint32_t)>;

// Returns the number of files that did not succeed, or a negative code when the call
// itself or a callback failed.
inline int mirror_copy_files(tfs_crc_ctx* ctx, const LogicBlockImage& block, const std::vector<MirrorFile>& files,
                             const MirrorOptions& opt, const MirrorSink& sink, const MirrorClose& close,
                             MirrorResult* res, BlockCrcChecker* checker) {
  if (!ctx || !res || !sink || !close) return TFS_EXIT_PARAMETER_ERROR;
  *res = MirrorResult();
  res->files.assign(files.size(), MirrorFileResult());
  std::map<uint64_t, tfs_raw_meta> index;
  for (const tfs_raw_meta& m : block.sorted_metas()) index[m.file_id] = m;
  tfs_mirror_cfg cfg{};
  cfg.first_len = opt.first_len, cfg.frame_len = opt.frame_len;
  cfg.is_server = opt.is_server, cfg.version = opt.version;
  const char* image = block.data().data();
  std::vector<tfs_mirror_job> jobs;
  std::vector<size_t> job_file;
  std::vector<uint64_t> ds;
  uint64_t at = 0;
  for (size_t i = 0; i < files.size(); ++i) {
    const MirrorFile& f = files[i];
    const auto it = index.find(f.file_id);
    if (it == index.end()) {
      res->files[i].skipped = 1;
      continue;
    }
    if (block.flag_of(f.file_id) & TFS_FI_INVALID) {
      res->files[i].status = TFS_EXIT_FILE_INFO_ERROR;
      ++res->n_bad;
      continue;
    }
    tfs_mirror_job j{};
    j.src_offset = uint64_t(int64_t(it->second.offset));
    j.file_id = f.file_id, j.file_number = f.file_number, j.packet_id = f.packet_id;
    j.block_id = opt.dest_block_id;
    j.size = it->second.size;
    j.ds_first = uint32_t(ds.size()), j.ds_count = uint32_t(f.ds.size());
    ds.insert(ds.end(), f.ds.begin(), f.ds.end());
    // the first frame's data lands on the source's address mod 16
    const uint64_t head = uint64_t(TFS_MIRROR_FRAME_HEAD) + 8u * f.ds.size();
    const uintptr_t want = reinterpret_cast<uintptr_t>(image) + j.src_offset + uint64_t(TFS_FILEINFO_SIZE);
    at += (want - (at + head)) & 15u;
    j.frame_offset = at;
    at += tfs_mirror_span(&cfg, &j);
    jobs.push_back(j);
    job_file.push_back(i);
  }
  if (jobs.empty()) return int(res->n_bad);
  std::vector<char> out(size_t(at) + 1);
  std::vector<tfs_mirror_result> r(jobs.size());
  uint32_t nbad = 0;
  const int rc = tfs_mirror_frames(ctx, &cfg, image, uint64_t(block.data_size()), jobs.data(), uint32_t(jobs.size()),
                                   ds.empty() ? nullptr : ds.data(), uint32_t(ds.size()), out.data(), at, r.data(), &nbad);
  if (rc != TFS_SUCCESS && rc != TFS_EXIT_CHECK_CRC_ERROR) return rc;
  res->n_bad += nbad;
  for (size_t k = 0; k < jobs.size(); ++k) {
    const size_t i = job_file[k];
    MirrorFileResult& fr = res->files[i];
    fr.status = r[k].status, fr.file_crc = r[k].file_crc;
    if (r[k].status != TFS_SUCCESS) {
      if (r[k].status == TFS_EXIT_CHECK_CRC_ERROR && checker) checker->add_crc_error(block.block_id(), jobs[k].file_id);
      continue;
    }
    const char* p = out.data() + jobs[k].frame_offset;
    for (uint32_t q = 0; q < r[k].n_frames; ++q) {
      uint32_t body = 0;
      memcpy(&body, p + 4, 4);  // (little-endian hosts, as everywhere in this harness)
      const uint32_t bytes = uint32_t(TFS_PACKET_HEADER_V1_SIZE) + body;
      if (const int s = sink(i, q, p, bytes)) return s < 0 ? s : TFS_EXIT_PARAMETER_ERROR;
      ++fr.n_frames, ++res->frames_sent;
      p += bytes;
    }
    if (const int s = close(i, r[k].file_crc)) return s < 0 ? s : TFS_EXIT_PARAMETER_ERROR;
    ++res->closed;
  }
  return int(res->n_bad);
}

}  // namespace dataserver
}  // namespace tfs
