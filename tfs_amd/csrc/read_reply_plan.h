// read_reply_plan.h -- host arithmetic of the read replies (include/tfs_read.h,
// DESIGN.md §3.17): what a job serves (n), how long its body and its span are,
// the status decided before anything is read, the header-CRC seed pre-shifted
// over the data, and the call-level span checks.  Header-only, no device; the
// kernel reads the ReadUnit this makes.
//
// The frame CRC is Func::crc(FLAG, L || D || T), L = le32(n).  The host knows L
// and n = |D| before the launch, so pre = shift(crc(FLAG, L), n) is host
// arithmetic per job and the wave that computes c = crc(0, D) gets
// crc(FLAG, L || D) = pre ^ c without touching L or D again.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tfs_read.h"
#include "crc_math.h"

namespace tfscrc {

constexpr uint32_t kReadHead = 28;       // the 24-byte V1 header and le32(n) before the data
constexpr uint32_t kReadInfo = 36;       // sizeof(FileInfo)
constexpr uint32_t kReadFlag = 0x4e534654u;  // TFS_PACKET_FLAG_V1, also the frame CRC's seed
constexpr int kReadPcodeV1 = TFS_RESP_READ_DATA_MESSAGE;  // the reply without a trailer
using ReadResult = tfs_read_result;
constexpr int32_t kReadParameterError = -1016, kReadSizeError = -8034;

// One job as the kernel takes it.  64 bytes.
struct ReadUnit {
  uint64_t soff, doff, fid, pid;  // FileInfo in the source, frame in out, expected id_, header id
  int32_t size;                   // RawMeta.size
  uint32_t roff, n;               // the data: payload bytes [roff, roff + n)
  uint32_t pre_seed;              // shift(crc(FLAG, le32(n)), n)
  int32_t pre;                    // TFS_SUCCESS, or the status decided before reading
  uint32_t type_ver;              // header bytes 8..11: pcode | version << 16
  uint32_t whole;                 // 1: the data is the whole payload (checked against crc_)
  uint32_t tlen;                  // trailer bytes after the data: 0, 4 or 40
};
static_assert(sizeof(ReadUnit) == 64, "read unit layout");

inline bool read_pcode_ok(int16_t pcode) {
  return pcode == TFS_RESP_READ_DATA_MESSAGE || pcode == TFS_RESP_READ_DATA_MESSAGE_V2 ||
         pcode == TFS_RESP_READ_DATA_MESSAGE_V3;
}

// The job's own fields are sound (everything of check 1 that needs no buffer length).
inline bool read_fields_ok(const tfs_read_job& j) {
  if (!read_pcode_ok(j.pcode) || j.read_offset < 0 || j.read_len < 0) return false;
  const int64_t payload = std::max<int64_t>(int64_t(j.size) - kReadInfo, 0);
  return int64_t(j.read_offset) <= payload;
}

// Data bytes served: min(read_len, size - 36 - read_offset); 0 for an unsound or short job.
inline uint32_t read_n(const tfs_read_job& j) {
  if (!read_fields_ok(j) || j.size < int32_t(kReadInfo)) return 0u;
  const int64_t left = int64_t(j.size) - kReadInfo - j.read_offset;
  return uint32_t(std::min<int64_t>(j.read_len, left));
}

// Trailer bytes of RespReadDataMessageV2::serialize after the data.
inline uint32_t read_trailer_len(const tfs_read_job& j) {
  if (j.pcode == TFS_RESP_READ_DATA_MESSAGE) return 0u;
  return j.read_offset == 0 ? 4u + kReadInfo : 4u;
}

inline uint32_t read_body_len(const tfs_read_job& j) { return 4u + read_n(j) + read_trailer_len(j); }

// The span a job may write from frame_offset.  The failure frame (28 / 32 bytes) always fits.
inline uint32_t read_frame_cap(const tfs_read_job& j) {
  if (!read_pcode_ok(j.pcode)) return 0u;
  return 24u + read_body_len(j);
}

// Length of the set_length(status) frame.
inline uint32_t read_fail_len(int16_t pcode) { return pcode == TFS_RESP_READ_DATA_MESSAGE ? 28u : 32u; }

// Func::crc (func.cpp:426-435), bit by bit: only ever run over the 4 length bytes.
inline uint32_t read_crc_bytes(uint32_t c, const uint8_t* p, uint32_t len) {
  for (uint32_t i = 0; i < len; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : (c >> 1);
  }
  return c;
}

// shift(crc(FLAG, le32(n)), n): XOR crc(0, D) into it for crc(FLAG, le32(n) || D).
inline uint32_t read_pre_seed(uint32_t n) {
  const uint8_t l[4] = {uint8_t(n), uint8_t(n >> 8), uint8_t(n >> 16), uint8_t(n >> 24)};
  return shift_bytes_pow(read_crc_bytes(kReadFlag, l, 4), n);
}

// The status a job has before anything is read (checks 1 and 2 of tfs_read.h).
inline int32_t read_pre_status(const tfs_read_job& j, uint64_t src_len, uint64_t out_cap) {
  if (!read_fields_ok(j)) return kReadParameterError;
  const uint64_t rec = uint64_t(uint32_t(std::max<int32_t>(j.size, 0)));
  if (j.src_offset > src_len || rec > src_len - j.src_offset) return kReadParameterError;
  const uint64_t cap = read_frame_cap(j);
  if (j.frame_offset > out_cap || cap > out_cap - j.frame_offset) return kReadParameterError;
  return j.size < int32_t(kReadInfo) ? kReadSizeError : 0;
}

// The seed of the last length asked for: the reads of one batch mostly share a few lengths.
struct ReadSeedMemo {
  uint32_t n = 0, seed = 0;
  bool valid = false;
  uint32_t get(uint32_t len) {
    if (!valid || len != n) n = len, seed = read_pre_seed(len), valid = true;
    return seed;
  }
};

inline ReadUnit read_make_unit(const tfs_read_job& j, uint64_t src_len, uint64_t out_cap, ReadSeedMemo* memo = nullptr) {
  ReadUnit u{};
  u.soff = j.src_offset, u.doff = j.frame_offset, u.fid = j.file_id, u.pid = j.packet_id;
  u.size = j.size;
  u.pre = read_pre_status(j, src_len, out_cap);
  u.type_ver = uint32_t(uint16_t(j.pcode)) | uint32_t(uint16_t(j.version)) << 16;
  if (u.pre == 0) {
    u.roff = uint32_t(j.read_offset);
    u.n = read_n(j);
    u.pre_seed = memo ? memo->get(u.n) : read_pre_seed(u.n);
    u.whole = j.read_offset == 0 && u.n == uint32_t(j.size) - kReadInfo ? 1u : 0u;
    u.tlen = read_trailer_len(j);
  }
  return u;
}

// True when the spans [frame_offset, frame_offset + cap) of two jobs that may write
// (every job but those refused with TFS_EXIT_PARAMETER_ERROR) share a byte.
inline bool read_spans_overlap(const tfs_read_job* jobs, uint32_t n, uint64_t src_len, uint64_t out_cap) {
  {  // frames laid out in job order, the usual case: one pass, no allocation
    uint64_t end = 0;
    uint32_t i = 0;
    for (; i < n; ++i) {
      if (read_pre_status(jobs[i], src_len, out_cap) == kReadParameterError) continue;
      const uint64_t cap = read_frame_cap(jobs[i]);
      if (!cap) continue;
      if (jobs[i].frame_offset < end) break;
      end = jobs[i].frame_offset + cap;
    }
    if (i == n) return false;
  }
  std::vector<std::pair<uint64_t, uint64_t>> s;
  s.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (read_pre_status(jobs[i], src_len, out_cap) == kReadParameterError) continue;
    const uint64_t cap = read_frame_cap(jobs[i]);
    if (cap) s.emplace_back(jobs[i].frame_offset, jobs[i].frame_offset + cap);  // inside out_cap: no wrap
  }
  std::sort(s.begin(), s.end());
  for (size_t i = 1; i < s.size(); ++i)
    if (s[i].first < s[i - 1].second) return true;
  return false;
}

}  // namespace tfscrc
