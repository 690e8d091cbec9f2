// ec_fetch_plan.h -- host arithmetic of the task chunk calls of the marshalling and
// reinstate sessions (include/tfs_ec_fetch.h): the call checks
// that need no device, the n each incoming frame must carry, the bytes a member's
// in must hold, the frame constants, and a host restatement of the per-frame check.
// Header-only, no device.
//
// Func::crc has no inversions, so its register is linear in the message and
//   crc(FLAG_V1, le32 n || D || le32 dfs)
//     = shift(crc(FLAG_V1, le32 n), n + 4) ^ shift(crc(0, D), 4) ^ crc(0, le32 dfs)
// with shift(c, d) = c * x^(8d) mod P.  The tile pass leaves crc(0, the tile's data
// bytes) per 4 KiB tile of D -- the last one 1 .. 4096 bytes long; chained they give
// crc(0, D).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/tfs_ec_fetch.h"
#include "ec_frames_plan.h"

namespace tfsec {

constexpr uint32_t kEcxHead = TFS_EC_FETCH_HEAD;          // 28: the V1 header and le32(n) before the data
constexpr uint32_t kEcxOverhead = TFS_EC_FETCH_OVERHEAD;  // 32
constexpr int32_t kEcxPcode = TFS_RESP_READ_RAW_DATA_MESSAGE;
constexpr int32_t kEcxError = -1, kEcxCrcError = -1010;
static_assert(sizeof(tfs_ec_fetch_result) == 16 && sizeof(tfs_ec_fetch_cfg) == 8, "fetch result and cfg layout");

inline uint64_t ecx_stride(const tfs_ec_frames_cfg& c, const tfs_ec_fetch_cfg& f) {
  return f.in_stride ? uint64_t(f.in_stride) : uint64_t(c.frame_len) + kEcxOverhead;
}

// The part of check 4 that reads the fetch cfg alone (frames_cfg has passed ecf_cfg_status).
inline int ecx_cfg_status(const tfs_ec_frames_cfg& c, const tfs_ec_fetch_cfg& f) {
  if (f.in_stride != 0 && (uint64_t(f.in_stride) < uint64_t(c.frame_len) + kEcxOverhead || f.in_stride % 8u != 0u))
    return kEcfParameterError;
  if (f.reserved != 0) return kEcfParameterError;
  return 0;
}

// The n of the frame at member offset `offset` asked for `requested` bytes: clamp(block_len - offset, 0, requested).
inline int32_t ecx_expect(int64_t block_len, int64_t offset, int64_t requested) {
  return int32_t(std::max<int64_t>(0, std::min<int64_t>(block_len - offset, requested)));
}
inline int32_t ecx_block_len(const int* sizes, int dn, int total, int member) { return member < dn ? sizes[member] : total; }

// The data bytes frame j of a call of `len` bytes is asked for.
inline int32_t ecx_requested(int32_t frame_len, int32_t len, uint32_t j) {
  return int32_t(std::min<int64_t>(frame_len, int64_t(len) - int64_t(j) * frame_len));
}

// Whether a call [offset, offset + len) has a frame of a member of `block_len` bytes to read.
inline bool ecx_reads(int32_t block_len, int32_t offset) { return block_len > offset; }

// The bytes of one member's in a call of `len` bytes may touch, counted from in[i] (in[i] % 8 == 4).
inline uint64_t ecx_call_need(const tfs_ec_frames_cfg& c, const tfs_ec_fetch_cfg& f, int64_t len) {
  const uint32_t nf = ecf_call_frames(c.frame_len, len);
  const uint64_t last = uint64_t(len) - uint64_t(nf - 1) * uint64_t(c.frame_len);
  return uint64_t(nf - 1) * ecx_stride(c, f) + ((4u + kEcxOverhead + last + 7u) & ~uint64_t(7)) - 4u;
}

// Checks 2 to 5 of a task call, in the header's order, for a chunk that passed the session's own rules.
// in / out are indexed by member; sources and outputs list the members the session reads and writes;
// block_len[k] belongs to sources[k].  dev: the device form's alignment rule applies to in.
inline int ecx_call_status(const tfs_ec_frames_cfg* c, const tfs_ec_fetch_cfg* f, const void* const* in,
                           const void* const* out, uint64_t out_cap, const void* results, int32_t total, int32_t offset,
                           int32_t len, const int* sources, const int32_t* block_len, int n_sources, const int* outputs,
                           int n_outputs, bool dev) {
  if (!c || !out || !f || !in || !results) return kEcfParameterError;
  if (const int rc = ecf_cfg_status(*c)) return rc;
  if (offset % c->frame_len != 0) return kEcfParameterError;
  if (len % c->frame_len != 0 && int64_t(offset) + int64_t(len) != int64_t(total)) return kEcfParameterError;
  for (int k = 0; k < n_outputs; ++k)
    if ((reinterpret_cast<uintptr_t>(out[outputs[k]]) & 7u) != 0u) return kEcfParameterError;
  if (out_cap < ecf_call_need(*c, len)) return kEcfParameterError;
  if (const int rc = ecx_cfg_status(*c, *f)) return rc;
  if (dev)
    for (int k = 0; k < n_sources; ++k) {
      const void* p = in[sources[k]];
      if (p && ecx_reads(block_len[k], offset) && (reinterpret_cast<uintptr_t>(p) & 7u) != 4u) return kEcfParameterError;
    }
  for (int k = 0; k < n_sources; ++k)
    if (!in[sources[k]] && ecx_reads(block_len[k], offset)) return kEcfDataInvalid;
  for (int k = 0; k < n_outputs; ++k)
    if (!out[outputs[k]]) return kEcfDataInvalid;
  return 0;
}

inline uint32_t ecx_rd32(const uint8_t* p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// The 28 bytes before a frame's data.
inline void ecx_head_bytes(uint32_t n, int16_t version, uint64_t pid, uint32_t crc, uint8_t out[28]) {
  tfscrc::rep_le32(out, tfscrc::kRepFlag);
  tfscrc::rep_le32(out + 4, 8u + n);
  tfscrc::rep_le32(out + 8, uint32_t(kEcxPcode) | uint32_t(uint16_t(version)) << 16);
  tfscrc::rep_le32(out + 12, uint32_t(pid));
  tfscrc::rep_le32(out + 16, uint32_t(pid >> 32));
  tfscrc::rep_le32(out + 20, crc);
  tfscrc::rep_le32(out + 24, n);
}

// crc(FLAG_V1, body) from crc(0, D): the check kernel's join of head, data and tail.
inline uint32_t ecx_join(uint32_t n, uint32_t data_crc, uint32_t dfs) {
  uint8_t w[4];
  tfscrc::rep_le32(w, n);
  const uint32_t head = tfscrc::rep_crc_bytes(tfscrc::kRepFlag, w, 4);
  tfscrc::rep_le32(w, dfs);
  return tfscrc::multmodp(ecf_pow(uint64_t(n) + 4u), head) ^ tfscrc::multmodp(ecf_pow(4), data_crc) ^
         tfscrc::rep_crc_bytes(0u, w, 4);
}

// crc(0, D) chained from per-tile words the way the check kernel chains them: whole tiles 4096 apart, then the
// last tile's 1 .. 4096 bytes on.  words[t] = crc(0, the data bytes of tile t); n > 0.
inline uint32_t ecx_chain(const uint32_t* words, uint32_t n) {
  const uint32_t nc = (n - 1u) >> 12, lastb = n - (nc << 12);
  uint32_t c = 0;
  for (uint32_t t = 0; t < nc; ++t) c = tfscrc::multmodp(ecf_pow(4096), c) ^ words[t];
  return tfscrc::multmodp(ecf_pow(lastb), c) ^ words[nc];
}

// The per-frame check, restated on host-readable bytes: `frame` holds 32 + expect bytes (nothing is read when
// expect == 0).  The statuses and their order are the header's.
inline tfs_ec_fetch_result ecx_check(const uint8_t* frame, uint32_t expect) {
  tfs_ec_fetch_result r;
  memset(&r, 0, sizeof r);
  if (expect == 0u) return r;
  const uint32_t flag = ecx_rd32(frame), blen = ecx_rd32(frame + 4), tv = ecx_rd32(frame + 8), hcrc = ecx_rd32(frame + 20);
  r.n = ecx_rd32(frame + 24);
  r.data_file_size = int32_t(ecx_rd32(frame + kEcxHead + expect));
  uint32_t words[1];
  words[0] = tfscrc::rep_crc_bytes(0u, frame + kEcxHead, expect);  // one "tile" of any length: the chain of one
  r.crc = ecx_join(expect, words[0], uint32_t(r.data_file_size));
  if (flag != tfscrc::kRepFlag || blen != 8u + expect || (tv & 0xffffu) != uint32_t(kEcxPcode) || r.n != expect)
    r.status = kEcxError;
  else if (int16_t(uint16_t(tv >> 16)) >= 1 && hcrc != r.crc)
    r.status = kEcxCrcError;
  return r;
}

// tfs_ec_fetch_parse.
inline int ecx_parse(const void* frame, uint32_t avail, int32_t* out_n, int32_t* out_dfs) {
  if (!frame || !out_n || !out_dfs) return kEcfParameterError;
  if (avail < kEcxOverhead) return 1;  // TFS_PACKET_INCOMPLETE
  const uint8_t* p = static_cast<const uint8_t*>(frame);
  const int32_t n = int32_t(ecx_rd32(p + 24));
  if (n < 0) return n;
  if (uint64_t(avail) < uint64_t(kEcxOverhead) + uint64_t(n)) return 1;
  *out_n = n;
  *out_dfs = int32_t(ecx_rd32(p + kEcxHead + uint32_t(n)));
  return 0;
}

}  // namespace tfsec
