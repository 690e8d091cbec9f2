// ec_frames_plan.h -- host arithmetic of the frame-emitting chunk calls of the
// marshalling and reinstate sessions (include/tfs_ec_frames.h):
// the call checks that need no device, the bytes a member's out must hold, and
// each frame's constants -- H, F, crc(FLAG_V1, H) and the two shifts that join
// head, data and tail.  Header-only, no device.
//
// Func::crc has no inversions, so its register is linear in the message and
//   crc(FLAG_V1, H || D || F) = shift(crc(FLAG_V1, H), |D| + 4) ^ shift(crc(0, D), 4) ^ crc(0, F)
// with shift(c, d) = c * x^(8d) mod P.  The tile pass leaves crc(0, tile) per 4 KiB
// tile of D; chained they give crc(0, D), and the rest is known before the launch.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/tfs_ec_frames.h"
#include "crc_math.h"
#include "replicate_plan.h"

namespace tfsec {

constexpr uint32_t kEcfHead = tfscrc::kRepHead;          // 56: V1 header and WriteDataInfo before the data
constexpr uint32_t kEcfOverhead = TFS_RAW_FRAME_OVERHEAD;  // 60
constexpr int32_t kEcfParameterError = -1016, kEcfSizeInvalid = -16002, kEcfDataInvalid = -16001;

inline uint64_t ecf_stride(const tfs_ec_frames_cfg& c) {
  return c.frame_stride ? uint64_t(c.frame_stride) : uint64_t(c.frame_len) + 64u;
}

// Frames of a call of `len` bytes (len > 0), and the bytes of one member's out they need at the cfg's stride.
inline uint32_t ecf_call_frames(int64_t frame_len, int64_t len) { return uint32_t((len + frame_len - 1) / frame_len); }
inline uint64_t ecf_call_need(const tfs_ec_frames_cfg& c, int64_t len) {
  const uint32_t nf = ecf_call_frames(c.frame_len, len);
  const uint64_t last = uint64_t(len) - uint64_t(nf - 1) * uint64_t(c.frame_len);
  return uint64_t(nf - 1) * ecf_stride(c) + kEcfOverhead + last;
}

// Check 3, then the part of check 4 that reads cfg alone.
inline int ecf_cfg_status(const tfs_ec_frames_cfg& c) {
  if (c.frame_len <= 0 || c.frame_len % 4096 != 0) return kEcfSizeInvalid;
  if (c.frame_stride != 0 && (uint64_t(c.frame_stride) < uint64_t(c.frame_len) + kEcfOverhead || c.frame_stride % 8u != 0u))
    return kEcfParameterError;
  if (c.reserved != 0) return kEcfParameterError;
  return 0;
}

// Checks 2 to 5 of a frames call, in the header's order, for a chunk that passed the session's own rules.
// members / out are indexed by member; sources and outputs list the members the session reads and writes.
inline int ecf_call_status(const tfs_ec_frames_cfg* c, const void* const* members, const void* const* out,
                           uint64_t out_cap, int32_t total, int32_t offset, int32_t len, const int* sources, int n_sources,
                           const int* outputs, int n_outputs) {
  if (!c || !out) return kEcfParameterError;
  if (const int rc = ecf_cfg_status(*c)) return rc;
  if (offset % c->frame_len != 0) return kEcfParameterError;
  if (len % c->frame_len != 0 && int64_t(offset) + int64_t(len) != int64_t(total)) return kEcfParameterError;
  for (int k = 0; k < n_outputs; ++k)
    if ((reinterpret_cast<uintptr_t>(out[outputs[k]]) & 7u) != 0u) return kEcfParameterError;
  if (out_cap < ecf_call_need(*c, len)) return kEcfParameterError;
  if (!members) return kEcfDataInvalid;
  for (int k = 0; k < n_sources; ++k)
    if (!members[sources[k]]) return kEcfDataInvalid;
  for (int k = 0; k < n_outputs; ++k)
    if (!out[outputs[k]]) return kEcfDataInvalid;
  return 0;
}

// x^(8d) mod P.
inline uint32_t ecf_pow(uint64_t d) { return tfscrc::x2nmodp(d, 3); }

// What every frame of a call shares: the multipliers of the seal.
struct EcfCallConst {
  uint32_t pow_head_full;  // x^(8 (frame_len + 4)): crc(FLAG_V1, H) to the body's end, a full frame
  uint32_t pow_head_last;  // the same for the frame that ends at `total` (== pow_head_full when that frame is full)
  uint32_t last_len;       // data bytes of the frame that ends at `total`
  uint32_t last_frame;     // its number in the member
};
inline EcfCallConst ecf_call_const(int32_t frame_len, int32_t total) {
  EcfCallConst k;
  const uint32_t nf = std::max<uint32_t>(1u, ecf_call_frames(frame_len, total));
  k.last_frame = nf - 1u;
  k.last_len = uint32_t(total) - k.last_frame * uint32_t(frame_len);
  k.pow_head_full = ecf_pow(uint64_t(frame_len) + 4u);
  k.pow_head_last = ecf_pow(uint64_t(k.last_len) + 4u);
  return k;
}

// One frame's constants.
struct EcfFrameConst {
  uint8_t h[32];      // H
  uint32_t flag;      // F
  uint32_t offset, length;
  uint64_t pid;
  uint32_t head_crc;  // crc(FLAG_V1, H)
  uint32_t pow_head;  // x^(8 (length + 4))
  uint32_t tail_crc;  // crc(0, F)
};
inline EcfFrameConst ecf_frame_const(const tfs_ec_frames_cfg& c, int member, bool parity, int32_t total, uint32_t k) {
  EcfFrameConst f;
  f.offset = k * uint32_t(c.frame_len);
  f.length = std::min<uint32_t>(uint32_t(c.frame_len), uint32_t(total) - f.offset);
  f.flag = k == 0u ? uint32_t(parity ? TFS_RAW_PARITY_DATA : TFS_RAW_NORMAL_DATA) : 0u;
  f.pid = c.packet_id[member] + k;
  tfscrc::rep_info_bytes(c.block_id[member], f.offset, f.length, f.h);
  f.head_crc = tfscrc::rep_crc_bytes(tfscrc::kRepFlag, f.h, 32);
  f.pow_head = ecf_pow(uint64_t(f.length) + 4u);
  uint8_t fb[4];
  tfscrc::rep_le32(fb, f.flag);
  f.tail_crc = tfscrc::rep_crc_bytes(0u, fb, 4);
  return f;
}

// The header CRC from the frame's constants and crc(0, D); 0 for a version-0 header.
inline uint32_t ecf_seal(const EcfFrameConst& f, uint32_t data_crc, int16_t version) {
  if (version < 1) return 0u;
  return tfscrc::multmodp(f.pow_head, f.head_crc) ^ tfscrc::multmodp(ecf_pow(4), data_crc) ^ f.tail_crc;
}

// The 56 bytes before the data.
inline void ecf_head_bytes(const EcfFrameConst& f, int16_t version, uint32_t crc, uint8_t out[56]) {
  tfscrc::rep_le32(out, tfscrc::kRepFlag);
  tfscrc::rep_le32(out + 4, 36u + f.length);
  tfscrc::rep_le32(out + 8, uint32_t(TFS_WRITE_RAW_DATA_MESSAGE) | uint32_t(uint16_t(version)) << 16);
  tfscrc::rep_le32(out + 12, uint32_t(f.pid));
  tfscrc::rep_le32(out + 16, uint32_t(f.pid >> 32));
  tfscrc::rep_le32(out + 20, crc);
  std::copy(f.h, f.h + 32, out + 24);
}

}  // namespace tfsec
