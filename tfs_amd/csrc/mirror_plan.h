// mirror_plan.h -- host arithmetic of the mirror sync call (include/tfs_mirror.h,
// DESIGN.md §3.21): the per-job checks made before anything is read, the frames of
// every file, the units that cut each frame's data for the waves, the multipliers
// that join the units' CRCs, each frame's header-CRC seed and the bytes that precede
// its data.  Header-only, no device; the kernels read the MirJob / MirFrame / MirUnit
// this makes.
//
// A unit is the intersection of one job's payload with one frame, cut further every
// kMirSeg bytes from the frame's first data byte.  With c(u) = crc(0, u) and
// shift(c, d) = c * x^(8d) mod P (replicate_plan.h):
//   file CRC  = XOR over the job's units of    mr * c(u)   d = bytes from the unit's end to the payload's
//   frame CRC = seed ^ XOR over its units of   mf * c(u)   d = bytes from the unit's end to the body's
// with seed = crc(FLAG, H || V || 0^length) = shift(crc(FLAG, H || V), length): the
// body with its data zeroed, H and V known before the launch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/tfs_mirror.h"
#include "replicate_plan.h"

namespace tfscrc {

constexpr uint32_t kMirHead = TFS_MIRROR_FRAME_HEAD;  // V1 header (24), WriteDataInfo (32) and the ds count (4)
constexpr uint32_t kMirInfo = 36;                     // sizeof(FileInfo)
constexpr uint32_t kMirSeg = kRepSeg;                 // no wave streams more than this alone
constexpr uint32_t kMirStart = 0x80000000u;           // MirUnit.job: the unit starts its job (its wave loads the FileInfo)
constexpr uint32_t kMirMaxItems = 0x7fffffffu;        // units / frames of one launch
constexpr int32_t kMirParameterError = -1016, kMirSizeError = -8034;
using MirResult = tfs_mirror_result;

// One unit as the kernel takes it.  32 bytes.
struct MirUnit {
  uint64_t soff;  // its first payload byte in the source
  uint64_t doff;  // where that byte goes in out
  uint32_t plen;  // payload bytes, 1..kMirSeg
  uint32_t job;   // its job in the launch; | kMirStart on the job's first unit
  uint32_t mf;    // x^(8d), d = bytes from the end of the unit to the end of the frame's body
  uint32_t mr;    // x^(8d), d = bytes from the end of the unit to the end of the payload
};
static_assert(sizeof(MirUnit) == 32, "mirror unit layout");

// One frame as the fold takes it.  32 bytes.
struct MirFrame {
  uint64_t doff;     // the frame's first byte in out
  uint32_t seed;     // crc(FLAG, H || V || 0^length)
  uint32_t pre_off;  // its prefix in the plan's prefix bytes
  uint32_t pre_len;  // 60 + 8 * count
  uint32_t job;
  uint32_t u0, nu;   // its units
};
static_assert(sizeof(MirFrame) == 32, "mirror frame layout");

// One job as the fold takes it.  40 bytes.
struct MirJob {
  uint64_t file_id;
  int32_t size;
  int32_t pre;       // TFS_SUCCESS, or the status decided before reading
  uint32_t f0, nf;   // its frames
  uint32_t u0, nu;   // its units
  uint32_t span_len;
  uint32_t version_crc;  // 1: the header CRC is written (version >= 1)
};
static_assert(sizeof(MirJob) == 40, "mirror job layout");

struct MirPlan {
  std::vector<MirJob> jobs;
  std::vector<MirFrame> frames;
  std::vector<MirUnit> units;
  std::vector<uint8_t> prefix;  // every frame's header, H and V, the header's crc field zero
};

inline bool mir_cfg_ok(const tfs_mirror_cfg& c) { return c.first_len > 0 && c.frame_len > 0 && c.reserved == 0; }

inline uint32_t mir_frame_count(const tfs_mirror_cfg& c, int32_t size) {
  if (c.first_len <= 0 || c.frame_len <= 0 || size <= int32_t(kMirInfo)) return 0u;
  const int64_t n = int64_t(size) - kMirInfo;
  if (n <= c.first_len) return 1u;
  return uint32_t(1 + (n - c.first_len + c.frame_len - 1) / c.frame_len);
}

// Payload bytes [*off, *off + *len) of frame k.
inline void mir_frame_range(const tfs_mirror_cfg& c, int64_t n, uint32_t k, int64_t* off, int64_t* len) {
  *off = k == 0 ? 0 : int64_t(c.first_len) + int64_t(k - 1) * c.frame_len;
  const int64_t end = std::min<int64_t>(n, int64_t(c.first_len) + int64_t(k) * c.frame_len);
  *len = end - *off;
}

inline uint64_t mir_span(const tfs_mirror_cfg& c, const tfs_mirror_job& j) {
  if (j.ds_count > uint32_t(TFS_MIRROR_MAX_DS)) return 0u;
  const uint64_t nf = mir_frame_count(c, j.size);
  if (!nf) return 0u;
  return nf * (uint64_t(kMirHead) + 8u * j.ds_count) + uint64_t(j.size - int32_t(kMirInfo));
}

// The status a job has before anything is read (include/tfs_mirror.h, the first two rows).
inline int32_t mir_pre_status(const tfs_mirror_cfg& c, const tfs_mirror_job& j, uint32_t ds_n, uint64_t src_len,
                              uint64_t out_cap) {
  if (j.ds_count > uint32_t(TFS_MIRROR_MAX_DS)) return kMirParameterError;
  if (uint64_t(j.ds_first) + j.ds_count > ds_n) return kMirParameterError;
  const uint64_t rec = uint64_t(uint32_t(std::max<int32_t>(j.size, 0)));
  if (j.src_offset > src_len || rec > src_len - j.src_offset) return kMirParameterError;
  const uint64_t span = mir_span(c, j);
  if (span && (j.frame_offset > out_cap || span > out_cap - j.frame_offset || span > 0xffffffffu))
    return kMirParameterError;
  if (j.reserved != 0) return kMirParameterError;
  return j.size <= int32_t(kMirInfo) ? kMirSizeError : 0;
}

// True when the spans of two jobs that may write (pre[i] == 0) share a byte.
inline bool mir_spans_overlap(const tfs_mirror_cfg& c, const tfs_mirror_job* jobs, const int32_t* pre, uint32_t n) {
  {  // frames laid out in job order, the usual case: one pass, no allocation
    uint64_t end = 0;
    uint32_t i = 0;
    for (; i < n; ++i) {
      if (pre[i] != 0) continue;
      if (jobs[i].frame_offset < end) break;
      end = jobs[i].frame_offset + mir_span(c, jobs[i]);
    }
    if (i == n) return false;
  }
  std::vector<std::pair<uint64_t, uint64_t>> s;
  s.reserve(n);
  for (uint32_t i = 0; i < n; ++i)
    if (pre[i] == 0) s.emplace_back(jobs[i].frame_offset, jobs[i].frame_offset + mir_span(c, jobs[i]));
  std::sort(s.begin(), s.end());
  for (size_t i = 1; i < s.size(); ++i)
    if (s[i].first < s[i - 1].second) return true;
  return false;
}

// Func::crc over H and V, a byte a step: a call seals a frame per file or more, and the
// plan is host time the device waits for.
inline uint32_t mir_crc_bytes(uint32_t c, const uint8_t* p, uint32_t len) {
  struct Tab {
    uint32_t t[256];
    Tab() { make_byte_table(t); }
  };
  static const Tab tb;
  for (uint32_t i = 0; i < len; ++i) c = (c >> 8) ^ tb.t[(c ^ p[i]) & 0xffu];
  return c;
}

inline void mir_le64(uint8_t* p, uint64_t v) {
  rep_le32(p, uint32_t(v));
  rep_le32(p + 4, uint32_t(v >> 32));
}

// The bytes of frame k of job j before its data: the V1 header with a zero crc
// field, H and V.  `p` holds 60 + 8 * ds_count bytes.
inline void mir_prefix_bytes(const tfs_mirror_cfg& c, const tfs_mirror_job& j, const uint64_t* ds, uint32_t k,
                             uint32_t offset, uint32_t length, uint8_t* p) {
  const uint32_t cnt = j.ds_count;
  rep_le32(p, kRepFlag);
  rep_le32(p + 4, kMirInfo + 8u * cnt + length);
  rep_le32(p + 8, uint32_t(TFS_WRITE_DATA_MESSAGE) | uint32_t(uint16_t(c.version)) << 16);
  mir_le64(p + 12, j.packet_id + k);
  rep_le32(p + 20, 0u);
  uint8_t* h = p + 24;
  rep_le32(h, j.block_id);
  mir_le64(h + 4, j.file_id);
  rep_le32(h + 12, offset);
  rep_le32(h + 16, length);
  rep_le32(h + 20, uint32_t(c.is_server));
  mir_le64(h + 24, j.file_number);
  rep_le32(p + 56, cnt);
  for (uint32_t i = 0; i < cnt; ++i) mir_le64(p + kMirHead + 8u * i, ds[j.ds_first + i]);
}

// The plan of a launch over jobs [0, n) with the statuses `pre` already decided
// (mir_pre_status against the caller's buffers; the offsets in `jobs` may since
// have been moved into staging).  False when the launch holds too many units.
inline bool make_mirror_plan(const tfs_mirror_cfg& c, const tfs_mirror_job* jobs, const int32_t* pre, uint32_t n,
                             const uint64_t* ds, MirPlan* p) {
  p->jobs.clear(), p->frames.clear(), p->units.clear(), p->prefix.clear();
  p->jobs.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    const tfs_mirror_job& j = jobs[i];
    MirJob mj{};
    mj.file_id = j.file_id, mj.size = j.size, mj.pre = pre[i];
    mj.f0 = uint32_t(p->frames.size()), mj.u0 = uint32_t(p->units.size());
    mj.version_crc = c.version >= 1 ? 1u : 0u;
    if (pre[i] == 0) {
      const int64_t npay = int64_t(j.size) - kMirInfo;
      const uint32_t nf = mir_frame_count(c, j.size);
      const uint32_t plen = kMirHead + 8u * j.ds_count;
      if (uint64_t(p->frames.size()) + nf > kMirMaxItems) return false;
      uint64_t fdoff = j.frame_offset;
      for (uint32_t k = 0; k < nf; ++k) {
        int64_t off, len;
        mir_frame_range(c, npay, k, &off, &len);
        if (uint64_t(p->units.size()) + uint64_t((len + kMirSeg - 1) / kMirSeg) > kMirMaxItems) return false;
        MirFrame fr{};
        fr.doff = fdoff;
        fr.pre_off = uint32_t(p->prefix.size()), fr.pre_len = plen;
        if (uint64_t(p->prefix.size()) + plen > 0xffffffffu) return false;
        fr.job = i;
        fr.u0 = uint32_t(p->units.size());
        p->prefix.resize(p->prefix.size() + plen);
        uint8_t* pb = p->prefix.data() + fr.pre_off;
        mir_prefix_bytes(c, j, ds, k, uint32_t(off), uint32_t(len), pb);
        fr.seed = multmodp(rep_pow(uint64_t(len)), mir_crc_bytes(kRepFlag, pb + 24, plen - 24u));
        for (int64_t at = 0; at < len; at += kMirSeg) {
          const uint32_t ul = uint32_t(std::min<int64_t>(kMirSeg, len - at));
          MirUnit u{};
          u.soff = j.src_offset + kMirInfo + uint64_t(off + at);
          u.doff = fdoff + plen + uint64_t(at);
          u.plen = ul;
          u.job = i | (off + at == 0 ? kMirStart : 0u);
          u.mf = uint32_t(len - (at + ul));            // (the distances; the pass below turns them into the multipliers)
          u.mr = uint32_t(npay - (off + at + ul));
          p->units.push_back(u);
        }
        fr.nu = uint32_t(p->units.size()) - fr.u0;
        p->frames.push_back(fr);
        fdoff += plen + uint64_t(len);
      }
      mj.nf = nf;
      mj.nu = uint32_t(p->units.size()) - mj.u0;
      mj.span_len = uint32_t(fdoff - j.frame_offset);
      RepPowWalk fw, rw;  // last unit to first: the pieces of one frame lie kMirSeg apart
      for (uint32_t k = mj.u0 + mj.nu; k-- > mj.u0;) {
        MirUnit& u = p->units[k];
        u.mf = fw.at(u.mf);
        u.mr = rw.at(u.mr);
      }
    }
    p->jobs.push_back(mj);
  }
  return true;
}

}  // namespace tfscrc
