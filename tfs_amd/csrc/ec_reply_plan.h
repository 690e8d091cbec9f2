// ec_reply_plan.h -- host arithmetic of the degraded read replies (include/
// tfs_ec_read.h): the unit the kernel takes for a job, the job's
// covering set, the call-level span check, and the host form's plan -- which
// units of the source members travel, packed and joined as ec_read_plan.h does,
// and where each frame lies in the staged output.  The job arithmetic (n, the
// frame lengths, the statuses decided before anything is read, the pre-shifted
// header-CRC seed) is read_reply_plan.h's.  No device code; the kernel reads the
// ReplyUnit and calls reply_cover.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tfs_ec_read.h"
#include "read_reply_plan.h"

namespace tfsec {

// One job as the kernel takes it.  64 bytes.  hpos and dpos are byte addresses in
// the source images: the target member's own for the device form, the packed
// image's for the host form.
struct ReplyUnit {
  uint64_t doff, fid, pid;  // frame in out, expected id_, header id
  uint32_t hpos, dpos;      // the FileInfo's first byte; the slice's first byte (H + 36 + read_offset)
  int32_t size;             // RawMeta.size
  uint32_t n;               // data bytes served
  uint32_t pre_seed;        // shift(crc(FLAG, le32(n)), n)
  int32_t pre;              // TFS_SUCCESS, or the status decided before reading
  uint32_t type_ver;        // header bytes 8..11: pcode | version << 16
  uint32_t whole;           // 1: the data is the whole payload (checked against crc_)
  uint32_t tlen;            // trailer bytes after the data: 0, 4 or 40
  uint32_t refuse;          // FileInfo.flag_ bits that refuse the job (0 unless read_offset == 0)
};
static_assert(sizeof(ReplyUnit) == 64, "reply unit layout");

// The covering set of a job as the kernel walks it: tile 0 is [hA, e0); tile t >= 1
// is 4 KiB from tb1 + 4096 t, cut at e1 (tb1 may lie below 0 mod 2^32: only tb1 +
// 4096 t with t >= 1 is ever formed).  When the slice's units touch or overlap the
// FileInfo's, both are one range from hA (tb1 = hA, e0 = e1); when they are
// disjoint, or there is no slice, tile 0 is the FileInfo's units alone and the
// slice's tiles count from its first unit.
struct ReplyCover {
  uint32_t hA, e0, tb1, e1, nt;
};
#ifdef __HIP__
__attribute__((host)) __attribute__((device))
#endif
inline ReplyCover reply_cover(uint32_t hpos, uint32_t dpos, uint32_t n) {
  ReplyCover c;
  c.hA = hpos & ~1023u;
  const uint32_t hE = (hpos + 36u + 1023u) & ~1023u;
  const uint32_t sA = dpos & ~1023u, sE = (dpos + n + 1023u) & ~1023u;
  if (n != 0u && sA <= hE) {
    c.e0 = c.e1 = sE, c.tb1 = c.hA;
    c.nt = (sE - c.hA + 4095u) >> 12;
  } else if (n != 0u) {
    c.e0 = hE, c.e1 = sE, c.tb1 = sA - 4096u;
    c.nt = 1u + ((sE - sA + 4095u) >> 12);
  } else {
    c.e0 = c.e1 = hE, c.tb1 = c.hA;
    c.nt = 1u;
  }
  return c;
}

// The status a job has before anything is read: the checks of tfs_read.h with src_len = the member's
// size, and the covering set against the member.  The covering set lies inside the record's own units,
// so it passes `size` only when the record does; the check stands on its own all the same (nothing may
// be read past a member).
inline int32_t reply_pre_status(const tfs_ec_reply_job& job, int32_t member_size, uint64_t out_cap) {
  const tfs_read_job& j = job.read;
  const uint64_t msize = uint64_t(uint32_t(std::max<int32_t>(member_size, 0)));
  const int32_t pre = tfscrc::read_pre_status(j, msize, out_cap);
  if (pre != 0) return pre;
  const uint32_t H = uint32_t(j.src_offset);  // <= member_size < 2^31
  const ReplyCover c = reply_cover(H, H + tfscrc::kReadInfo + uint32_t(j.read_offset), tfscrc::read_n(j));
  return uint64_t(c.e0) > msize || uint64_t(c.e1) > msize ? tfscrc::kReadParameterError : 0;
}

// The unit of a job over a member of member_size bytes (a multiple of 1024).
inline ReplyUnit reply_make_unit(const tfs_ec_reply_job& job, int32_t member_size, uint64_t out_cap,
                                 tfscrc::ReadSeedMemo* memo = nullptr) {
  const tfs_read_job& j = job.read;
  ReplyUnit u{};
  u.doff = j.frame_offset, u.fid = j.file_id, u.pid = j.packet_id;
  u.size = j.size;
  u.pre = reply_pre_status(job, member_size, out_cap);
  u.type_ver = uint32_t(uint16_t(j.pcode)) | uint32_t(uint16_t(j.version)) << 16;
  if (u.pre == tfscrc::kReadParameterError) return u;
  u.hpos = uint32_t(j.src_offset);
  u.dpos = u.hpos + tfscrc::kReadInfo;
  if (u.pre == 0) {
    u.n = tfscrc::read_n(j);
    u.dpos += uint32_t(j.read_offset);
    u.pre_seed = memo ? memo->get(u.n) : tfscrc::read_pre_seed(u.n);
    u.whole = j.read_offset == 0 && u.n == uint32_t(j.size) - tfscrc::kReadInfo ? 1u : 0u;
    u.tlen = tfscrc::read_trailer_len(j);
    u.refuse = j.read_offset == 0 ? job.refuse_flags : 0u;
  }
  return u;
}

// True when the spans [frame_offset, frame_offset + cap) of two jobs that may write
// (every job but those refused with TFS_EXIT_PARAMETER_ERROR) share a byte.
inline bool reply_spans_overlap(const tfs_ec_reply_job* jobs, uint32_t n, int32_t member_size, uint64_t out_cap) {
  {  // frames laid out in job order, the usual case: one pass, no allocation
    uint64_t end = 0;
    uint32_t i = 0;
    for (; i < n; ++i) {
      const uint64_t cap = tfscrc::read_frame_cap(jobs[i].read);
      if (!cap || reply_pre_status(jobs[i], member_size, out_cap) == tfscrc::kReadParameterError) continue;
      if (jobs[i].read.frame_offset < end) break;
      end = jobs[i].read.frame_offset + cap;  // inside out_cap: no wrap
    }
    if (i == n) return false;
  }
  std::vector<std::pair<uint64_t, uint64_t>> s;
  s.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t cap = tfscrc::read_frame_cap(jobs[i].read);
    if (!cap || reply_pre_status(jobs[i], member_size, out_cap) == tfscrc::kReadParameterError) continue;
    s.emplace_back(jobs[i].read.frame_offset, jobs[i].read.frame_offset + cap);
  }
  std::sort(s.begin(), s.end());
  for (size_t i = 1; i < s.size(); ++i)
    if (s[i].first < s[i - 1].second) return true;
  return false;
}

// ---- host form ---------------------------------------------------------------
struct ReplySpan {  // [start, end) of every source member -> [cbase, cbase + end - start) of its staging buffer
  uint32_t start, end;
  uint64_t cbase;
};
struct ReplyPlan {
  std::vector<ReplySpan> spans;   // the union of the covering sets, in address order, touching ranges joined
  std::vector<ReplyUnit> units;   // every job, restated against the packed images (and the staged output)
  std::vector<uint64_t> opos;     // staged output: where job i's frame lies (unset for a job that writes nothing)
  uint64_t up = 0;                // bytes of one source member that go up (a multiple of 1024)
  uint64_t down = 0;              // bytes of the staged output, placement padding included
};

// stage_out: the frames are packed into a staging buffer, each placed at the first
// address at or past the previous frame's end whose data byte 0 (frame + 28) is
// congruent mod 16 to the slice's first byte in the packed image -- under 16 bytes
// of padding a frame, and every piece leaves as a whole 8-byte store.  Otherwise
// the frames stay at the caller's frame_offset.
inline void make_reply_plan(const tfs_ec_reply_job* jobs, uint32_t n, int32_t member_size, uint64_t out_cap,
                            bool stage_out, ReplyPlan* p) {
  *p = ReplyPlan();
  p->units.resize(n);
  p->opos.assign(n, 0);
  tfscrc::ReadSeedMemo memo;
  std::vector<ReplySpan> cover;
  for (uint32_t i = 0; i < n; ++i) {
    const ReplyUnit u = p->units[i] = reply_make_unit(jobs[i], member_size, out_cap, &memo);
    if (u.pre != 0) continue;
    const ReplyCover c = reply_cover(u.hpos, u.dpos, u.n);
    cover.push_back(ReplySpan{c.hA, c.e0, 0});
    if (c.e1 != c.e0) cover.push_back(ReplySpan{c.tb1 + 4096u, c.e1, 0});
  }
  std::sort(cover.begin(), cover.end(), [](const ReplySpan& x, const ReplySpan& y) { return x.start < y.start; });
  for (const ReplySpan& c : cover) {
    if (!p->spans.empty() && c.start <= p->spans.back().end) {
      if (c.end > p->spans.back().end) p->spans.back().end = c.end;
    } else {
      p->spans.push_back(c);
    }
  }
  for (ReplySpan& s : p->spans) {
    s.cbase = p->up;
    p->up += uint64_t(s.end - s.start);
  }
  auto packed = [&](uint32_t addr) {  // the packed image's address of a covered member byte
    auto it = std::upper_bound(p->spans.begin(), p->spans.end(), addr,
                               [](uint32_t v, const ReplySpan& s) { return v < s.start; });
    const ReplySpan& s = *(it - 1);
    return uint32_t(s.cbase + uint64_t(addr - s.start));
  };
  for (uint32_t i = 0; i < n; ++i) {
    ReplyUnit& u = p->units[i];
    if (u.pre == 0) {
      const uint32_t h = u.hpos, d = u.dpos;
      u.hpos = packed(h);
      u.dpos = u.n ? packed(d) : u.hpos + tfscrc::kReadInfo;
    }
    if (!stage_out || u.pre == tfscrc::kReadParameterError) continue;
    const uint64_t cap = tfscrc::read_frame_cap(jobs[i].read);
    if (!cap) continue;
    const uint64_t op = p->down + ((uint64_t(u.dpos) - tfscrc::kReadHead - p->down) & 15u);
    p->opos[i] = u.doff = op;
    p->down = op + cap;
  }
}

}  // namespace tfsec
