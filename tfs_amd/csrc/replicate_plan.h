// replicate_plan.h -- host arithmetic of a replicate session (include/
// tfs_replicate.h): the begin-time checks, the units that cut the
// data file two ways at once (frames every frame_len bytes, records wherever they
// lie), each frame's header-CRC seed, and the slice of both that one call uploads.
// Header-only, no device; the kernels read the RepUnit / RepFrame this makes.
//
// A unit is the intersection of one frame with one record or one gap, cut further
// where it is longer than kRepSeg: hlen FileInfo bytes of the record (bytes
// [hk, hk + hlen) of its 36), then plen payload or gap bytes.  No unit crosses a
// frame cut, a FileInfo start, a payload start or a record end.
//
// Func::crc's register is linear, so with c(u) = crc(0, u) and shift(c, d) =
// c * x^(8d) mod P, crc(0, u1 || .. || uk) = XOR_i shift(c(ui), bytes after ui).
// The host knows every distance, so each unit carries the multipliers x^(8d):
//   record CRC = XOR over its payload units of  mr  * c(payload part)
//   frame CRC  = seed ^ XOR over its units of   mfh * c(FileInfo part) ^ mfp * c(payload part)
// with seed = crc(FLAG, H || 0^|D| || F) = shift(crc(FLAG, H), |D| + 4) ^ crc(0, F):
// the body with its data zeroed, H and F known before the launch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tfs_replicate.h"
#include "crc_math.h"

namespace tfscrc {

constexpr uint32_t kRepHead = 56;        // V1 header (24) and WriteDataInfo (32) before the data
constexpr uint32_t kRepOverhead = TFS_RAW_FRAME_OVERHEAD;
constexpr uint32_t kRepInfo = 36;        // sizeof(FileInfo)
constexpr uint32_t kRepFlag = 0x4e534654u;  // TFS_PACKET_FLAG_V1, also the frame CRC's seed
// No wave streams more than this alone.  One wave moves 1 - 1.6 GB/s, so a call of a few
// hundred units lasts as long as its longest unit: 64 KiB units made every call 67 us on the
// device.
constexpr uint32_t kRepSeg = 16u << 10;
constexpr uint32_t kRepNoRec = 0xffffffffu;
constexpr int32_t kRepParameterError = -1016, kRepSizeError = -8034, kRepSizeInvalid = -16002;

// One unit as the kernel takes it.  48 bytes.
struct RepUnit {
  uint64_t soff;   // its first byte: in the plan its place in the data file, in a call's slice relative to src
  uint64_t doff;   // where that byte goes in out (a call's slice only)
  uint32_t hlen;   // FileInfo bytes leading the unit, 0..36
  uint32_t hk;     // ... which are bytes [hk, hk + hlen) of the record's FileInfo
  uint32_t plen;   // payload (or gap) bytes after them
  uint32_t rec;    // the record (in plan order), kRepNoRec for a gap
  uint32_t frame;  // its frame: of the block in the plan, of the call in a slice
  uint32_t mfh;    // x^(8d), d = bytes from the end of the FileInfo part to the end of the frame's body; 0: no such part
  uint32_t mfp;    // x^(8d), d = bytes from the end of the unit to the end of the frame's body
  uint32_t mr;     // x^(8d), d = bytes from the end of the unit to the end of the record
};
static_assert(sizeof(RepUnit) == 48, "replicate unit layout");

// One frame of a call as the fold takes it.  48 bytes.
struct RepFrame {
  uint64_t doff;      // the frame's first byte in out
  uint64_t pid;       // header id
  uint32_t seed;      // crc(FLAG, H || 0^length || F)
  uint32_t length;    // data bytes
  uint32_t offset;    // WriteDataInfo.offset_
  uint32_t flag;      // F
  uint32_t block_id;
  uint32_t type_ver;  // header bytes 8..11: pcode | version << 16
  uint32_t u0, nu;    // its units in the call's slice
};
static_assert(sizeof(RepFrame) == 48, "replicate frame layout");

struct RepRec {
  uint64_t file_id;
  int32_t offset, size;
};

struct RepPlan {
  int32_t total = 0, frame_len = 0;
  uint32_t nframes = 0;
  std::vector<RepUnit> units;        // in address order
  std::vector<uint32_t> frame_first;  // [nframes + 1]: frame f's units are units[frame_first[f] .. frame_first[f + 1])
  std::vector<RepRec> recs;           // the records that take part, ascending
  std::vector<uint32_t> index;        // [rec]: its position in the caller's order
  std::vector<int32_t> early;         // per caller record: the status given at begin (0: it takes part)
};

inline uint32_t rep_frame_count(int64_t total, int64_t frame_len) {
  if (total < 0 || frame_len <= 0) return 0u;
  return uint32_t(std::max<int64_t>(1, (total + frame_len - 1) / frame_len));
}

// x^(8d) mod P: shift(c, d) = multmodp(rep_pow(d), c).  A plan asks for three per
// unit, so the powers come from byte tables: x^(8 v 256^j) for every byte value v of
// d's low four bytes, at most three multiplications a power.
inline uint32_t rep_pow(uint64_t d) {
  struct Pow {
    uint32_t t[4][256];
    Pow() {
      for (int j = 0; j < 4; ++j) {
        t[j][0] = 1u << 31;  // x^0
        const uint32_t step = shift_bytes_pow(1u << 31, uint64_t(1) << (8 * j));
        for (int v = 1; v < 256; ++v) t[j][v] = multmodp(t[j][v - 1], step);
      }
    }
  };
  static const Pow pw;
  uint32_t p = pw.t[0][d & 255u];
  for (int j = 1; j < 4; ++j)
    if ((d >> (8 * j)) & 255u) p = multmodp(p, pw.t[j][(d >> (8 * j)) & 255u]);
  return d >> 32 ? multmodp(p, shift_bytes_pow(1u << 31, d >> 32 << 32)) : p;
}

// The powers of a walk over distances that mostly grow by kRepSeg (the pieces of one long
// record or gap, last to first): such a step is four table lookups, any other a rep_pow.
struct RepPowWalk {
  uint64_t d = 0;
  uint32_t m = 0;
  bool valid = false;
  uint32_t at(uint64_t nd) {
    struct Seg {
      uint32_t t[4][256];
      Seg() { make_shift_table(t, kRepSeg); }
    };
    static const Seg sg;
    if (valid && nd == d + kRepSeg)
      m = sg.t[0][m & 255u] ^ sg.t[1][(m >> 8) & 255u] ^ sg.t[2][(m >> 16) & 255u] ^ sg.t[3][m >> 24];
    else
      m = rep_pow(nd);
    d = nd, valid = true;
    return m;
  }
};

// Func::crc (func.cpp:426-435), bit by bit: only ever run over H and F.
inline uint32_t rep_crc_bytes(uint32_t c, const uint8_t* p, uint32_t len) {
  for (uint32_t i = 0; i < len; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : (c >> 1);
  }
  return c;
}

inline void rep_le32(uint8_t* p, uint32_t v) {
  p[0] = uint8_t(v), p[1] = uint8_t(v >> 8), p[2] = uint8_t(v >> 16), p[3] = uint8_t(v >> 24);
}

// WriteDataInfo of a frame (internal.cpp:635-667).
inline void rep_info_bytes(uint32_t block_id, uint32_t offset, uint32_t length, uint8_t h[32]) {
  std::fill(h, h + 32, uint8_t(0));
  rep_le32(h, block_id);
  rep_le32(h + 12, offset);
  rep_le32(h + 16, length);
}

// crc(FLAG, H || 0^length || F).
inline uint32_t rep_frame_seed(uint32_t block_id, uint32_t offset, uint32_t length, uint32_t flag) {
  uint8_t h[32], f[4];
  rep_info_bytes(block_id, offset, length, h);
  rep_le32(f, flag);
  return shift_bytes_pow(rep_crc_bytes(kRepFlag, h, 32), uint64_t(length) + 4u) ^ rep_crc_bytes(0u, f, 4);
}

// Call-level checks 2 and 3 of tfs_replicate_begin.
inline int rep_cfg_status(const tfs_replicate_cfg& c) {
  if (c.total < 0 || c.frame_len <= 0 || c.frame_len % 1024 != 0) return kRepSizeInvalid;
  if (c.frame_stride != 0 && uint64_t(c.frame_stride) < uint64_t(c.frame_len) + kRepOverhead) return kRepParameterError;
  if (c.new_block != TFS_RAW_NORMAL_DATA && c.new_block != TFS_RAW_PARITY_DATA) return kRepParameterError;
  if (c.reserved != 0) return kRepParameterError;
  return 0;
}

inline uint64_t rep_stride(const tfs_replicate_cfg& c) {
  return c.frame_stride ? uint64_t(c.frame_stride) : uint64_t(c.frame_len) + kRepOverhead;
}

// The plan of a block: checks 2-5 of tfs_replicate_begin and the per-record
// checks (make_marshal_plan's rule for a member of length total).  Returns the
// call's status; the plan is complete only on 0.
inline int make_replicate_plan(const tfs_replicate_cfg& c, const tfs_raw_meta* metas, uint32_t n, RepPlan* p) {
  *p = RepPlan();
  if (const int rc = rep_cfg_status(c)) return rc;
  if (n && !metas) return kRepParameterError;
  const int64_t total = c.total, fl = c.frame_len;
  p->total = c.total, p->frame_len = c.frame_len;
  p->nframes = rep_frame_count(total, fl);
  int64_t last_end = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const tfs_raw_meta& m = metas[i];
    if (m.offset < 0 || int64_t(m.offset) + int64_t(m.size) > total) {
      p->early.push_back(kRepParameterError);
      continue;
    }
    if (m.size <= int32_t(kRepInfo)) {
      p->early.push_back(kRepSizeError);
      continue;
    }
    if (int64_t(m.offset) < last_end) return kRepParameterError;  // unsorted or overlapping
    last_end = int64_t(m.offset) + int64_t(m.size);
    p->early.push_back(0);
    p->recs.push_back(RepRec{m.file_id, m.offset, m.size});
    p->index.push_back(i);
  }
  // The walk: gap, record, gap, ... cut at every frame and, for a long piece, at
  // the multiples of kRepSeg.
  auto piece_end = [&](int64_t pos, int64_t end) {  // where a payload / gap piece starting at pos stops
    const int64_t fend = std::min<int64_t>((pos / fl + 1) * fl, total);
    int64_t e = std::min(end, fend);
    if (e - pos > int64_t(kRepSeg)) e = (pos / int64_t(kRepSeg) + 1) * int64_t(kRepSeg);
    return e;
  };
  auto push = [&](int64_t pos, uint32_t hlen, uint32_t hk, uint32_t plen, uint32_t rec, int64_t rec_end) {
    const int64_t fend = std::min<int64_t>((pos / fl + 1) * fl, total);
    const int64_t uend = pos + hlen + plen;
    RepUnit u{};
    u.soff = uint64_t(pos);
    u.hlen = hlen, u.hk = hk, u.plen = plen, u.rec = rec;
    u.frame = uint32_t(pos / fl);
    // (the distances; the pass below turns them into the multipliers)
    u.mfh = hlen ? rep_pow(uint64_t(fend - (pos + hlen)) + 4u) : 0u;
    u.mfp = uint32_t(fend - uend) + 4u;
    u.mr = rec == kRepNoRec ? 0u : uint32_t(rec_end - uend);
    p->units.push_back(u);
  };
  auto gap = [&](int64_t pos, int64_t end) {
    while (pos < end) {
      const int64_t e = piece_end(pos, end);
      push(pos, 0u, 0u, uint32_t(e - pos), kRepNoRec, 0);
      pos = e;
    }
  };
  int64_t pos = 0;
  for (uint32_t r = 0; r < uint32_t(p->recs.size()); ++r) {
    const int64_t off = p->recs[r].offset, info_end = off + kRepInfo, end = off + p->recs[r].size;
    gap(pos, off);
    pos = off;
    while (pos < end) {
      const int64_t fend = std::min<int64_t>((pos / fl + 1) * fl, total);
      uint32_t hlen = 0, hk = 0, plen = 0;
      const int64_t start = pos;
      if (pos < info_end) {
        hk = uint32_t(pos - off);
        hlen = uint32_t(std::min(info_end, fend) - pos);
        pos += hlen;
      }
      if (pos >= info_end && pos < fend) {
        plen = uint32_t(piece_end(pos, end) - pos);
        pos += plen;
      }
      push(start, hlen, hk, plen, r, end);
    }
  }
  gap(pos, total);
  RepPowWalk fw, rw;  // last unit to first: the pieces of one record or gap lie kRepSeg apart
  for (size_t k = p->units.size(); k-- > 0;) {
    RepUnit& u = p->units[k];
    u.mfp = fw.at(u.mfp);
    if (u.rec != kRepNoRec) u.mr = rw.at(u.mr);
  }
  p->frame_first.assign(size_t(p->nframes) + 1, uint32_t(p->units.size()));
  for (uint32_t k = uint32_t(p->units.size()); k-- > 0;) p->frame_first[p->units[k].frame] = k;
  for (uint32_t f = p->nframes; f-- > 0;)  // a frame without units (the empty block's) starts where the next does
    p->frame_first[f] = std::min(p->frame_first[f], p->frame_first[f + 1]);
  return 0;
}

// A frames call over [offset, offset + len) with `next` bytes covered so far
// (`done`: the empty block's one call was made) is the one that may come now.
inline bool rep_call_ok(const RepPlan& p, int64_t next, bool done, int64_t offset, int64_t len) {
  if (offset != next || len < 0) return false;
  if (p.total == 0) return !done && offset == 0 && len == 0;
  if (len == 0 || offset + len > p.total) return false;
  return offset % p.frame_len == 0 && (len % p.frame_len == 0 || offset + len == p.total);
}

// Frames of a legal call, and the bytes of out it needs at `stride`.
inline uint32_t rep_call_frames(const RepPlan& p, int64_t len) {
  return uint32_t(std::max<int64_t>(1, (len + p.frame_len - 1) / p.frame_len));
}
inline uint64_t rep_call_need(const RepPlan& p, int64_t len, uint64_t stride) {
  const uint32_t nf = rep_call_frames(p, len);
  const uint64_t last = uint64_t(len) - uint64_t(nf - 1) * uint64_t(p.frame_len);
  return uint64_t(nf - 1) * stride + kRepOverhead + last;
}

inline uint32_t rep_slice_units(const RepPlan& p, uint32_t f0, uint32_t nf) {
  return p.frame_first[f0 + nf] - p.frame_first[f0];
}

// The slice of a call over frames [f0, f0 + nf): frame j at out + j * stride, the
// units' sources relative to the call's src.
inline void rep_make_slice(const RepPlan& p, const tfs_replicate_cfg& c, uint64_t stride, uint32_t f0, uint32_t nf,
                           RepFrame* frames, RepUnit* units) {
  const uint32_t ub = p.frame_first[f0];
  const uint64_t base = uint64_t(f0) * uint64_t(p.frame_len);
  for (uint32_t j = 0; j < nf; ++j) {
    const uint32_t f = f0 + j;
    const uint64_t off = uint64_t(f) * uint64_t(p.frame_len);
    RepFrame& fr = frames[j];
    fr.doff = uint64_t(j) * stride;
    fr.pid = c.packet_id + f;
    fr.length = uint32_t(std::min<uint64_t>(uint64_t(p.frame_len), uint64_t(p.total) - off));
    fr.offset = uint32_t(off);
    fr.flag = f == 0 ? uint32_t(int32_t(c.new_block)) : 0u;
    fr.block_id = c.block_id;
    fr.type_ver = uint32_t(TFS_WRITE_RAW_DATA_MESSAGE) | uint32_t(uint16_t(c.version)) << 16;
    fr.seed = rep_frame_seed(c.block_id, fr.offset, fr.length, fr.flag);
    fr.u0 = p.frame_first[f] - ub;
    fr.nu = p.frame_first[f + 1] - p.frame_first[f];
  }
  const uint32_t nu = rep_slice_units(p, f0, nf);
  for (uint32_t k = 0; k < nu; ++k) {
    RepUnit u = p.units[ub + k];
    const uint64_t pos = u.soff;
    const uint32_t j = u.frame - f0;
    u.soff = pos - base;
    u.doff = uint64_t(j) * stride + kRepHead + (pos - uint64_t(u.frame) * uint64_t(p.frame_len));
    u.frame = j;
    units[k] = u;
  }
}

}  // namespace tfscrc
