// repair_plan.h -- host arithmetic of the file repair call (include/tfs_repair.h,
// DESIGN.md §3.22): the per-job checks made before anything is read, the outgoing
// frames of every file, the units that cut its payload for the waves, the
// multipliers that join the units' CRCs three ways, each incoming frame's and each
// outgoing frame's seed, and the bytes that precede an outgoing frame's data.
// Header-only, no device; the kernels read the RprJob / RprIn / MirFrame / RprUnit
// this makes.
//
// A unit is the intersection of one incoming frame's data with one outgoing
// frame's data, cut further every kRepSeg bytes from the incoming frame's first
// data byte.  With c(u) = crc(0, u) and shift(c, d) = c * x^(8d) mod P:
//   incoming frame  crc(FLAG, L || D) = iseed ^ XOR over its units of  mi * c(u)
//                   with iseed = shift(crc(FLAG, L), n_k), then the trailer's
//                   bytes one by one
//   file            crc(0, payload)   =         XOR over its units of  mr * c(u)
//   outgoing frame  crc(FLAG, body)   = seed  ^ XOR over its units of  mf * c(u)
//                   with seed = shift(crc(FLAG, H || V), length)
// d being the bytes from the unit's end to the end of the incoming frame's data,
// of the payload and of the outgoing body.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/tfs_repair.h"
#include "mirror_plan.h"

namespace tfscrc {

constexpr uint32_t kRprInHead = TFS_REPAIR_IN_HEAD;  // V1 header (24) and the body's le32 length
constexpr uint32_t kRprNoFrame = TFS_REPAIR_NO_FRAME;
constexpr uint32_t kRprMaxItems = 0x7fffffffu;       // units / frames of one launch
constexpr int32_t kRprParameterError = -1016, kRprSizeError = -8034, kRprSyncError = -8038;
using RprResult = tfs_repair_result;

// One unit as the kernel takes it.  40 bytes.
struct RprUnit {
  uint64_t soff;  // its first payload byte in the source
  uint64_t doff;  // where that byte goes in out
  uint32_t plen;  // payload bytes, 1..kRepSeg
  uint32_t job;   // its job in the launch
  uint32_t mi;    // x^(8d), d = bytes from the end of the unit to the end of the incoming frame's data
  uint32_t mf;    // ... to the end of the outgoing frame's body
  uint32_t mr;    // ... to the end of the payload
  uint32_t pad;
};
static_assert(sizeof(RprUnit) == 40, "repair unit layout");

// One incoming frame as the fold takes it.  40 bytes.
struct RprIn {
  uint64_t soff;      // the frame's first byte in the source
  uint32_t data_len;  // declared n_k
  uint32_t seed;      // shift(crc(FLAG, le32(n_k)), n_k)
  uint32_t u0, nu;    // its units
  uint32_t job;
  uint32_t idx;       // its place among the job's frames
  uint32_t pcode;     // declared
  uint32_t trailer;   // 0, 4 or 40
};
static_assert(sizeof(RprIn) == 40, "repair incoming frame layout");

// One job as the folds take it.  48 bytes.
struct RprJob {
  int32_t pre;       // TFS_SUCCESS, or the status decided before reading
  uint32_t i0, ni;   // its incoming frames
  uint32_t f0, nf;   // its outgoing frames
  uint32_t u0, nu;   // its units
  uint32_t span_len;
  uint32_t stat_crc, check_crc;
  uint32_t version_crc;  // 1: the outgoing header CRC is written (version >= 1)
  uint32_t pad;
};
static_assert(sizeof(RprJob) == 48, "repair job layout");

struct RprPlan {
  std::vector<RprJob> jobs;
  std::vector<RprIn> ins;
  std::vector<MirFrame> frames;  // the outgoing frames: the mirror call's record, job = the repair job
  std::vector<RprUnit> units;
  std::vector<uint8_t> prefix;   // every outgoing frame's header, H and V, the header's crc field zero
};

inline bool rpr_cfg_ok(const tfs_repair_cfg& c) { return c.frame_len > 0 && c.reserved == 0; }

inline uint32_t rpr_frame_count(const tfs_repair_cfg& c, int64_t stat_size) {
  if (c.frame_len <= 0 || stat_size <= 0) return 0u;
  const int64_t nf = (stat_size - 1) / c.frame_len + 1;
  return nf > int64_t(0xffffffffu) ? 0u : uint32_t(nf);
}

inline uint64_t rpr_span(const tfs_repair_cfg& c, const tfs_repair_job& j) {
  if (j.ds_count > uint32_t(TFS_WRITE_MAX_DS)) return 0u;
  const uint64_t nf = rpr_frame_count(c, j.stat_size);
  if (!nf) return 0u;
  return nf * (uint64_t(kMirHead) + 8u * j.ds_count) + uint64_t(j.stat_size);
}

inline bool rpr_trailer_ok(int32_t pcode, int32_t trailer) {
  if (pcode == TFS_REPAIR_RESP_READ) return trailer == 0;
  if (pcode == TFS_REPAIR_RESP_READ_V2 || pcode == TFS_REPAIR_RESP_READ_V3) return trailer == 4 || trailer == 40;
  return false;
}

// tfs_repair_parse.
inline int rpr_parse(const void* frame, uint32_t avail, uint64_t frame_off, int32_t pcode, int32_t first,
                     tfs_repair_in* out) {
  if (!frame || !out) return kRprParameterError;
  if (pcode != TFS_REPAIR_RESP_READ && pcode != TFS_REPAIR_RESP_READ_V2 && pcode != TFS_REPAIR_RESP_READ_V3)
    return kRprParameterError;
  if (avail < kRprInHead) return TFS_PACKET_INCOMPLETE;
  const uint8_t* b = static_cast<const uint8_t*>(frame);
  auto le32 = [](const uint8_t* p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
  };
  const int32_t n = int32_t(le32(b + TFS_PACKET_HEADER_V1_SIZE));
  if (n < 0) return n;  // the source's error reply
  out->frame_off = frame_off;
  out->avail = avail;
  out->data_len = n;
  out->pcode = int16_t(pcode);
  out->trailer = int16_t(pcode == TFS_REPAIR_RESP_READ ? 0 : (first ? 40 : 4));
  out->reserved = 0u;
  return 0;
}

// The status a job has before anything is read (include/tfs_repair.h, the first three rows).
inline int32_t rpr_pre_status(const tfs_repair_cfg& c, const tfs_repair_job& j, const tfs_repair_in* ins, uint32_t n_in,
                              uint32_t ds_n, uint64_t src_len, uint64_t out_cap) {
  if (j.ds_count > uint32_t(TFS_WRITE_MAX_DS)) return kRprParameterError;
  if (uint64_t(j.ds_first) + j.ds_count > ds_n) return kRprParameterError;
  if (j.in_count == 0 || uint64_t(j.in_first) + j.in_count > n_in) return kRprParameterError;
  int64_t sum = 0;
  for (uint32_t k = 0; k < j.in_count; ++k) {
    const tfs_repair_in& f = ins[j.in_first + k];
    if (f.data_len < 0 || f.reserved != 0 || !rpr_trailer_ok(f.pcode, f.trailer)) return kRprParameterError;
    if (uint64_t(f.avail) < uint64_t(kRprInHead) + uint64_t(uint32_t(f.data_len)) + uint64_t(f.trailer))
      return kRprParameterError;
    if (f.frame_off > src_len || uint64_t(f.avail) > src_len - f.frame_off) return kRprParameterError;
    sum += f.data_len;
  }
  const uint64_t span = rpr_span(c, j);
  if (span && (j.frame_offset > out_cap || span > out_cap - j.frame_offset || span > 0xffffffffu))
    return kRprParameterError;
  if (j.stat_size > 0 && !span) return kRprParameterError;  // more than 2^32 frames
  if (j.reserved != 0) return kRprParameterError;
  if (j.stat_size <= 0) return kRprSizeError;
  return sum != j.stat_size ? kRprSyncError : 0;
}

// True when the spans of two jobs that may write (pre[i] == 0) share a byte.
inline bool rpr_spans_overlap(const tfs_repair_cfg& c, const tfs_repair_job* jobs, const int32_t* pre, uint32_t n) {
  std::vector<std::pair<uint64_t, uint64_t>> s;
  uint64_t end = 0;
  bool sorted = true;
  for (uint32_t i = 0; i < n; ++i) {
    if (pre[i] != 0) continue;
    const uint64_t a = jobs[i].frame_offset, b = a + rpr_span(c, jobs[i]);
    if (a < end) sorted = false;  // not laid out in job order: sort below
    end = std::max(end, b);
    s.emplace_back(a, b);
  }
  if (sorted) return false;
  std::sort(s.begin(), s.end());
  for (size_t i = 1; i < s.size(); ++i)
    if (s[i].first < s[i - 1].second) return true;
  return false;
}

// The plan of a launch over jobs [0, n) with the statuses `pre` already decided
// (rpr_pre_status against the caller's buffers; the offsets in `jobs` and `ins` may
// since have been moved into staging).  False when the launch holds too many items.
inline bool make_repair_plan(const tfs_repair_cfg& c, const tfs_repair_in* ins, const tfs_repair_job* jobs,
                             const int32_t* pre, uint32_t n, const uint64_t* ds, RprPlan* p) {
  p->jobs.clear(), p->ins.clear(), p->frames.clear(), p->units.clear(), p->prefix.clear();
  p->jobs.reserve(n);
  tfs_mirror_cfg mc{};
  mc.first_len = mc.frame_len = c.frame_len, mc.is_server = c.is_server, mc.version = c.version;
  for (uint32_t i = 0; i < n; ++i) {
    const tfs_repair_job& j = jobs[i];
    RprJob rj{};
    rj.pre = pre[i];
    rj.i0 = uint32_t(p->ins.size()), rj.f0 = uint32_t(p->frames.size()), rj.u0 = uint32_t(p->units.size());
    rj.stat_crc = j.stat_crc, rj.check_crc = j.check_crc;
    rj.version_crc = c.version >= 1 ? 1u : 0u;
    if (pre[i] == 0) {
      const int64_t npay = j.stat_size, flen = c.frame_len;
      const uint32_t nf = rpr_frame_count(c, npay);
      const uint32_t plen = kMirHead + 8u * j.ds_count;
      if (uint64_t(p->frames.size()) + nf > kRprMaxItems || uint64_t(p->ins.size()) + j.in_count > kRprMaxItems)
        return false;
      if (uint64_t(p->prefix.size()) + uint64_t(nf) * plen > 0xffffffffu) return false;
      tfs_mirror_job mj{};
      mj.file_id = j.file_id, mj.file_number = j.file_number, mj.packet_id = j.packet_id, mj.block_id = j.block_id;
      mj.ds_first = j.ds_first, mj.ds_count = j.ds_count;
      for (uint32_t k = 0; k < nf; ++k) {  // the outgoing frames; their units come with the walk below
        const int64_t off = int64_t(k) * flen, len = std::min<int64_t>(flen, npay - off);
        MirFrame fr{};
        fr.doff = j.frame_offset + uint64_t(k) * (uint64_t(plen) + uint64_t(flen));
        fr.pre_off = uint32_t(p->prefix.size()), fr.pre_len = plen;
        fr.job = i;
        p->prefix.resize(p->prefix.size() + plen);
        uint8_t* pb = p->prefix.data() + fr.pre_off;
        mir_prefix_bytes(mc, mj, ds, k, uint32_t(off), uint32_t(len), pb);
        fr.seed = multmodp(rep_pow(uint64_t(len)), mir_crc_bytes(kRepFlag, pb + 24, plen - 24u));
        p->frames.push_back(fr);
      }
      int64_t pos = 0;  // in the payload
      for (uint32_t k = 0; k < j.in_count; ++k) {
        const tfs_repair_in& f = ins[j.in_first + k];
        const int64_t nk = f.data_len;
        RprIn ri{};
        ri.soff = f.frame_off, ri.data_len = uint32_t(nk);
        uint8_t l4[4];
        rep_le32(l4, uint32_t(nk));
        ri.seed = multmodp(rep_pow(uint64_t(nk)), mir_crc_bytes(kRepFlag, l4, 4u));
        ri.u0 = uint32_t(p->units.size());
        ri.job = i, ri.idx = k;
        ri.pcode = uint32_t(uint16_t(f.pcode)), ri.trailer = uint32_t(f.trailer);
        for (int64_t t = 0; t < nk;) {
          const int64_t fk = (pos + t) / flen, fo = (pos + t) - fk * flen;  // the outgoing frame, the place in its data
          const int64_t fl = std::min<int64_t>(flen, npay - fk * flen);
          const int64_t e = std::min({nk, (t / int64_t(kRepSeg) + 1) * int64_t(kRepSeg), t + (fl - fo)});
          if (p->units.size() >= kRprMaxItems) return false;
          MirFrame& fr = p->frames[rj.f0 + size_t(fk)];
          if (fr.nu == 0) fr.u0 = uint32_t(p->units.size());
          ++fr.nu;
          RprUnit u{};
          u.soff = f.frame_off + kRprInHead + uint64_t(t);
          u.doff = fr.doff + plen + uint64_t(fo);
          u.plen = uint32_t(e - t);
          u.job = i;
          u.mi = uint32_t(nk - e);  // (the distances; the pass below turns them into the multipliers)
          u.mf = uint32_t(fl - (fo + (e - t)));
          u.mr = uint32_t(npay - (pos + e));
          p->units.push_back(u);
          t = e;
        }
        ri.nu = uint32_t(p->units.size()) - ri.u0;
        p->ins.push_back(ri);
        pos += nk;
      }
      rj.ni = j.in_count, rj.nf = nf;
      rj.nu = uint32_t(p->units.size()) - rj.u0;
      rj.span_len = uint32_t(rpr_span(c, j));
      RepPowWalk iw, fw, rw;  // last unit to first: the pieces of one frame mostly lie kRepSeg apart
      for (uint32_t k = rj.u0 + rj.nu; k-- > rj.u0;) {
        RprUnit& u = p->units[k];
        u.mi = iw.at(u.mi);
        u.mf = fw.at(u.mf);
        u.mr = rw.at(u.mr);
      }
    }
    p->jobs.push_back(rj);
  }
  return true;
}

}  // namespace tfscrc
