// receive_plan.h -- host arithmetic of a receive session (include/tfs_receive.h,
// DESIGN.md §3.20): the checks of a frames call, the frames of a call as the
// kernels take them, and at finish the per-record descriptor that cuts a payload
// into a head edge, whole granules and a tail edge.  Header-only, no device.
//
// The block's data file is cut into granules of G = TFS_RECEIVE_GRANULE bytes at
// block offsets 0, G, 2G, ...  The session keeps word[g] = crc(0, the bytes of
// granule g received so far || zeros up to the granule's end).  With shift(c, d) =
// c * x^(8d) mod P, a payload [a, b) is
//   crc = shift(crc(0, [a, he)), b - he)
//       ^ XOR over g in [g0, g0 + ng) of shift(word[g], b - (g + 1) G)
//       ^ crc(0, [tb, b))
// with he = min(b, ceil_G(a)), the whole granules between ceil_G(a) and floor_G(b),
// and tb = floor_G(b); a payload inside one granule is all head edge.
#pragma once
#include <cstdint>

#include "../../include/tfs_receive.h"
#include "crc_math.h"

namespace tfscrc {

constexpr uint32_t kRecvG = TFS_RECEIVE_GRANULE;
constexpr uint32_t kRecvHead = 56;       // V1 header (24) and WriteDataInfo (32) before the data
constexpr uint32_t kRecvOverhead = TFS_RECEIVE_FRAME_OVERHEAD;
constexpr uint32_t kRecvInfo = 36;       // sizeof(FileInfo)
constexpr uint32_t kRecvPowN = 32;       // x^(8 * 2^k), k < 32: the device's powers
constexpr int32_t kRecvParameterError = -1016, kRecvSizeError = -8034;
static_assert((kRecvG & (kRecvG - 1)) == 0 && kRecvG >= 64, "the granule is a power of two");
constexpr uint32_t recv_lg(uint32_t v) { return v <= 1u ? 0u : 1u + recv_lg(v >> 1); }
constexpr uint32_t kRecvLgG = recv_lg(kRecvG);  // x^(8 G) is the device's power kRecvLgG

// One frame of a call as the kernels take it.  32 bytes.
struct RecvFrame {
  uint64_t soff;     // the frame's first byte, relative to the call's base
  uint64_t src_end;  // soff + avail: no byte of base at or past it is read for this frame
  uint32_t off;      // declared data offset in the block
  uint32_t len;      // declared data bytes
  uint32_t u0, nu;   // its units among the call's: the data cut at the granule grid
};
static_assert(sizeof(RecvFrame) == 32, "receive frame layout");

// One record at finish.  48 bytes.
struct RecvRec {
  uint64_t file_id;
  int32_t offset, size;
  int32_t pre;      // 0, or the status given without reading
  uint32_t a, he;   // head edge [a, he)
  uint32_t g0, ng;  // whole granules [g0, g0 + ng)
  uint32_t tb, b;   // tail edge [tb, b)
  uint32_t pad;
};
static_assert(sizeof(RecvRec) == 48, "receive record layout");

// tfs_receive_parse: the declared offset and length from body bytes 12..19.
inline int recv_parse(const void* frame, uint32_t avail, uint64_t frame_off, tfs_receive_desc* out) {
  if (!frame || !out) return kRecvParameterError;
  if (avail < kRecvHead) return TFS_PACKET_INCOMPLETE;
  const uint8_t* b = static_cast<const uint8_t*>(frame) + TFS_PACKET_HEADER_V1_SIZE;
  auto le32 = [](const uint8_t* p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
  };
  out->frame_off = frame_off;
  out->avail = avail;
  out->data_offset = int32_t(le32(b + 12));
  out->data_len = int32_t(le32(b + 16));
  out->reserved = 0u;
  return 0;
}

// Units of a frame's data [off, off + len): one per granule it touches.
inline uint32_t recv_units(uint32_t off, uint32_t len) {
  return len ? (off + len - 1u) / kRecvG - off / kRecvG + 1u : 0u;
}

inline uint64_t recv_words(int64_t image_cap) { return uint64_t((image_cap + kRecvG - 1) / kRecvG); }

// The checks of a frames call that need no device; *end receives the cursor after it.
inline bool recv_call_ok(const tfs_receive_desc* d, uint32_t n, int64_t cursor, int64_t image_cap, int64_t* end) {
  for (uint32_t j = 0; j < n; ++j) {
    if (d[j].data_len < 0 || int64_t(d[j].data_offset) != cursor) return false;
    if (cursor + int64_t(d[j].data_len) > image_cap) return false;
    if (uint64_t(d[j].avail) < uint64_t(kRecvOverhead) + uint64_t(uint32_t(d[j].data_len))) return false;
    cursor += d[j].data_len;
  }
  *end = cursor;
  return true;
}

// The call's frames; returns its units.
inline uint32_t recv_make_frames(const tfs_receive_desc* d, uint32_t n, RecvFrame* out) {
  uint32_t u = 0;
  for (uint32_t j = 0; j < n; ++j) {
    RecvFrame& f = out[j];
    f.soff = d[j].frame_off;
    f.src_end = d[j].frame_off + d[j].avail;
    f.off = uint32_t(d[j].data_offset);
    f.len = uint32_t(d[j].data_len);
    f.u0 = u;
    f.nu = recv_units(f.off, f.len);
    u += f.nu;
  }
  return u;
}

// The record's descriptor against `total` received bytes (tfs_replicate.h's rules).
inline RecvRec recv_make_rec(const tfs_raw_meta& m, int64_t total) {
  RecvRec r{};
  r.file_id = m.file_id;
  r.offset = m.offset, r.size = m.size;
  if (m.offset < 0 || int64_t(m.offset) + int64_t(m.size) > total) {
    r.pre = kRecvParameterError;
    return r;
  }
  if (m.size <= int32_t(kRecvInfo)) {
    r.pre = kRecvSizeError;
    return r;
  }
  const uint32_t a = uint32_t(m.offset) + kRecvInfo, b = uint32_t(m.offset) + uint32_t(m.size);
  const uint64_t up = (uint64_t(a) + kRecvG - 1u) / kRecvG * kRecvG;  // ceil_G(a)
  const uint32_t down = b / kRecvG * kRecvG;                          // floor_G(b)
  r.a = a, r.b = b;
  if (up > uint64_t(down)) {  // inside one granule: all edge
    r.he = b, r.g0 = 0u, r.ng = 0u, r.tb = b;
  } else {
    r.he = uint32_t(up);
    r.g0 = uint32_t(up / kRecvG);
    r.ng = (down - uint32_t(up)) / kRecvG;
    r.tb = down;
  }
  return r;
}

// x^(8 * 2^k), k < kRecvPowN, made by the compiler: the device's table of powers.
struct RecvPowTab {
  uint32_t p[kRecvPowN];
};
constexpr uint32_t recv_cmul(uint32_t a, uint32_t b) {  // a * b mod P (reflected)
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32u; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  }
  return p;
}
constexpr RecvPowTab recv_pow_tab() {
  RecvPowTab t{};
  t.p[0] = 1u << 23;  // x^8
  for (uint32_t k = 1; k < kRecvPowN; ++k) t.p[k] = recv_cmul(t.p[k - 1], t.p[k - 1]);
  return t;
}

// Func::crc (func.cpp:426-435), bit by bit.
inline uint32_t recv_crc_bytes(uint32_t c, const uint8_t* p, uint64_t len) {
  for (uint64_t i = 0; i < len; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : (c >> 1);
  }
  return c;
}

// The fold the finish kernel makes, on the host: the reference of its arithmetic.
inline uint32_t recv_fold_host(const RecvRec& r, const uint8_t* image, const uint32_t* words) {
  uint32_t c = shift_bytes_pow(recv_crc_bytes(0u, image + r.a, r.he - r.a), r.b - r.he);
  for (uint32_t k = 0; k < r.ng; ++k)
    c ^= shift_bytes_pow(words[r.g0 + k], uint64_t(r.b) - uint64_t(r.g0 + k + 1u) * kRecvG);
  return c ^ recv_crc_bytes(0u, image + r.tb, r.b - r.tb);
}

}  // namespace tfscrc
