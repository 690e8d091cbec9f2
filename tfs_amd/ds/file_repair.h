// file_repair.h -- BlockChecker::do_repair_crc over a batch of CrcCheckFiles
// (block_checker.cpp:131-182, file_repair.cpp:81-197) through one file repair call
// (include/tfs_repair.h).  Every entry is one file from
// BlockCrcChecker::repair_queue(): its CrcCheckFile (block id, file id, crc), what
// fstat on the good replica said (size, crc), the reply frames of its fetch as the
// streamer received them, and the update's file_number, packet id and ds list.  The
// fetched bytes are read once: every reply frame is checked, the file's CRC is held
// against fstat's and the CrcCheckFile's, and the update's sealed WriteDataMessage
// frames are left ready to send in the same pass.
//
// A block whose checker already asks for a whole-block repair is not repaired file
// by file (block_checker.cpp:150-157): its entries are skipped.  A source error
// reply (a negative length, file_repair.cpp:128) becomes the file's status without
// a job.  For a file that passes, its frames go to the sink in order and then
// close(file, file_crc) is called: the place of CloseFileMessage.set_crc, with the
// CRC of the bytes that were sent.  For a file that fails neither callback is
// called and its status is recorded: a fetched copy that is wrong never leaves as
// an update.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/tfs_repair.h"
#include "ds_harness.h"

namespace tfs {
namespace dataserver {

struct RepairFrame {
  uint64_t off = 0;    // of the reply frame in the receive buffer
  uint32_t avail = 0;  // its bytes
};

struct RepairEntry {
  uint32_t block_id = 0;   // CrcCheckFile.block_id_
  uint64_t file_id = 0;    // CrcCheckFile.file_id_
  uint32_t check_crc = 0;  // CrcCheckFile.crc_
  int64_t stat_size = 0;   // TfsFileStat.size_
  uint32_t stat_crc = 0;   // TfsFileStat.crc_
  int32_t pcode = TFS_REPAIR_RESP_READ;  // of the replies the fetch asked for
  std::vector<RepairFrame> frames;       // in payload order
  uint64_t file_number = 0;  // from the update's create-file reply
  uint64_t packet_id = 0;    // frame k of the update carries packet_id + k
  std::vector<uint64_t> ds;  // ds_ of its WriteDataMessages
};

struct RepairOptions {
  const char* recv = nullptr;  // the receive buffer the frames lie in
  uint64_t recv_len = 0;
  int32_t frame_len = TFS_MAX_READ_SIZE;
  int32_t is_server = 0;
  int16_t version = 2;
};

struct RepairFileResult {
  int32_t status = TFS_SUCCESS;
  uint32_t n_frames = 0;  // frames sent
  uint32_t file_crc = 0;  // Func::crc(0, payload) as computed
  uint32_t bad_in = TFS_REPAIR_NO_FRAME;
  uint32_t flags = 0;
  int32_t skipped = 0;    // 1: the block is marked for a whole-block repair
};

struct RepairResult {
  std::vector<RepairFileResult> files;  // one per RepairEntry
  uint32_t n_bad = 0;
  uint32_t frames_sent = 0;
  uint32_t closed = 0;
};

// (index into entries, frame of the file, frame, bytes) -> TFS_SUCCESS, or the code the batch ends with.
using RepairSink = std::function<int(size_t, uint32_t, const char*, uint32_t)>;
// (index into entries, file CRC) -> TFS_SUCCESS, or the code the batch ends with.
using RepairClose = std::function<int(size_t, uint32_t)>;

// Returns the number of files that did not succeed, or a negative code when the call
// itself or a callback failed.
inline int repair_files(tfs_crc_ctx* ctx, const std::vector<RepairEntry>& entries, const RepairOptions& opt,
                        const RepairSink& sink, const RepairClose& close, RepairResult* res,
                        const BlockCrcChecker* checker) {
  if (!ctx || !res || !sink || !close || (opt.recv_len && !opt.recv)) return TFS_EXIT_PARAMETER_ERROR;
  *res = RepairResult();
  res->files.assign(entries.size(), RepairFileResult());
  tfs_repair_cfg cfg{};
  cfg.frame_len = opt.frame_len, cfg.is_server = opt.is_server, cfg.version = opt.version;
  std::vector<tfs_repair_in> ins;
  std::vector<tfs_repair_job> jobs;
  std::vector<size_t> job_file;
  std::vector<uint64_t> ds;
  uint64_t at = 0;
  for (size_t i = 0; i < entries.size(); ++i) {
    const RepairEntry& e = entries[i];
    if (checker && checker->needs_repair(e.block_id)) {
      res->files[i].skipped = 1;
      continue;
    }
    tfs_repair_job j{};
    j.in_first = uint32_t(ins.size());
    int32_t early = TFS_SUCCESS;
    for (size_t k = 0; k < e.frames.size() && early == TFS_SUCCESS; ++k) {
      const RepairFrame& f = e.frames[k];
      if (f.off > opt.recv_len || f.avail > opt.recv_len - f.off) {
        early = TFS_EXIT_PARAMETER_ERROR;
        break;
      }
      tfs_repair_in d{};
      const int rc = tfs_repair_parse(opt.recv + f.off, f.avail, f.off, e.pcode, k == 0, &d);
      if (rc < 0) early = rc;                           // the source's error reply, or a refused argument
      else if (rc != 0) early = TFS_EXIT_PARAMETER_ERROR;  // a frame cut short
      else ins.push_back(d);
    }
    if (early != TFS_SUCCESS) {
      ins.resize(j.in_first);
      res->files[i].status = early;
      ++res->n_bad;
      continue;
    }
    j.in_count = uint32_t(ins.size()) - j.in_first;
    j.file_id = e.file_id, j.file_number = e.file_number, j.packet_id = e.packet_id;
    j.block_id = e.block_id;
    j.stat_size = e.stat_size, j.stat_crc = e.stat_crc, j.check_crc = e.check_crc;
    j.ds_first = uint32_t(ds.size()), j.ds_count = uint32_t(e.ds.size());
    ds.insert(ds.end(), e.ds.begin(), e.ds.end());
    at = (at + 15u) & ~uint64_t(15);
    j.frame_offset = at;
    at += tfs_repair_span(&cfg, &j);
    jobs.push_back(j);
    job_file.push_back(i);
  }
  if (jobs.empty()) return int(res->n_bad);
  std::vector<char> out(size_t(at) + 1);
  std::vector<tfs_repair_result> r(jobs.size());
  uint32_t nbad = 0;
  const int rc = tfs_repair_frames(ctx, &cfg, opt.recv, opt.recv_len, ins.empty() ? nullptr : ins.data(),
                                   uint32_t(ins.size()), jobs.data(), uint32_t(jobs.size()),
                                   ds.empty() ? nullptr : ds.data(), uint32_t(ds.size()), out.data(), at, r.data(), &nbad);
  if (rc != TFS_SUCCESS && rc != TFS_EXIT_CHECK_CRC_ERROR) return rc;
  res->n_bad += nbad;
  for (size_t k = 0; k < jobs.size(); ++k) {
    const size_t i = job_file[k];
    RepairFileResult& fr = res->files[i];
    fr.status = r[k].status, fr.file_crc = r[k].file_crc, fr.bad_in = r[k].bad_in, fr.flags = r[k].flags;
    if (r[k].status != TFS_SUCCESS) continue;
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
