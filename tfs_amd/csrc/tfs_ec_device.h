// tfs_ec_device.h -- launch arguments shared by tfs_ec_kernels.hip and tfs_ec_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tfs_ec_fetch.h"
#include "ec_reply_plan.h"
#include "ec_update_plan.h"

namespace tfsec {

constexpr int kMaxMembersDev = 12;  // MAX_MARSHALLING_NUM
constexpr int kMaxOutGroup = 4;     // outputs accumulated in registers per launch

struct EcArgs {
  const uint8_t* src[kMaxMembersDev];
  uint8_t* dst[kMaxOutGroup];
  const uint32_t* masks;  // [OG][8][S][8] words (0 or 0xffffffff) for this launch's outputs
  uint32_t S;
  uint64_t units;         // size / 1024
};

hipError_t launch_ec_apply(const EcArgs& a, int og, int variant, hipStream_t stream);

// Degraded read: one workgroup per job rebuilds the covering units
// of one erased data member and, for a record job, checks the record's FileInfo
// and payload CRC on the rebuilt bytes while they are in registers.
// Same bytes as tfs_ec_read_job in include/tfs_ec.h.
struct ReadJob {
  uint64_t file_id;
  uint64_t out_offset;
  int32_t offset, size;
  uint32_t flags, reserved;
};
static_assert(sizeof(ReadJob) == 32, "read job layout");
constexpr uint32_t kReadRange = 1u;
constexpr int kReadWaves = 8;             // waves of the workgroup that shares one job's tiles (a power of two)
constexpr unsigned kReadMaxGrid = 4096;   // workgroups at most; they stride over the jobs beyond
// A lane's chain steps from one of its 8-byte pieces to the next: 128 bytes on
// inside a tile (a jump over 120 foreign bytes, then its own 8), and from packet
// 7 of a tile to packet 0 of its wave's next tile, kReadWaves tiles on.
constexpr uint32_t kReadStepPacket = 128, kReadStepTile = 4096u * kReadWaves - 896u;
// xpow[i] = x^(8 * (i - kReadPowBias)) mod P: one multiplication moves a lane's
// register from the end of its last piece to the end of the job's last tile (0 ..
// 3,192 bytes on, plus up to kReadWaves - 1 tiles) and takes off the zero padding
// behind the payload (0 .. 4,095 bytes back) at once.
constexpr int kReadPowBias = 4095;
constexpr int kReadPowN = kReadPowBias + 4096 * (kReadWaves - 1) + 3192 + 1;
struct ReadTables {
  uint32_t slice[4][256];       // slice-by-4, as Tables::slice
  uint32_t step_packet[4][256]; // byte tables of shift(c, 128)
  uint32_t step_tile[4][256];   // byte tables of shift(c, kReadStepTile)
  uint32_t xpow[kReadPowN];
};
// The checks made before a job reads anything, shared by the kernel and the host
// form (include/tfs_ec.h, "per job" 1 and 2).  *A and *E receive the covering
// range [offset rounded down, offset + size rounded up) when the job passes.
#ifdef __HIP__
__attribute__((host)) __attribute__((device))
#endif
inline int32_t read_job_check(const ReadJob& jb, int32_t member_size, uint64_t out_cap, uint32_t* A, uint32_t* E) {
  const int64_t cover_end = (int64_t(jb.offset) + int64_t(jb.size) + 1023) & ~int64_t(1023);
  if (jb.offset < 0 || jb.size < 0 || cover_end > int64_t(member_size)) return -1016;  // EXIT_PARAMETER_ERROR
  *A = uint32_t(jb.offset) & ~1023u;
  *E = uint32_t(cover_end);
  if ((jb.out_offset & 1023u) != 0u || jb.out_offset > out_cap || uint64_t(*E - *A) > out_cap - jb.out_offset)
    return -1016;
  if (!(jb.flags & kReadRange) && jb.size <= 36) return -8034;  // EXIT_READ_FILE_SIZE_ERROR
  return 0;
}

struct ReadArgs {
  const uint8_t* src[kMaxMembersDev];
  const uint32_t* masks;  // [8][S][8] words: the target's rows of the decode plan
  const ReadTables* tab;
  const ReadJob* jobs;
  uint8_t* out;
  uint64_t out_cap;
  uint32_t* out_crc;
  int32_t* out_status;
  uint32_t* n_bad;  // may be nullptr
  uint32_t n, S;
  int32_t size;     // bytes of every source member
};

hipError_t launch_ec_read(const ReadArgs& a, hipStream_t stream);

// Degraded read reply: the degraded read's workgroup per job, with
// the reply frame as the destination of the rebuilt slice and the frame's header CRC
// from the same chain.  The units are ec_reply_plan.h's; tab is the degraded read's.
struct ReplyArgs {
  const uint8_t* src[kMaxMembersDev];
  const uint32_t* masks;  // [8][S][8] words: the target's rows of the decode plan
  const ReadTables* tab;
  const ReplyUnit* units;
  uint8_t* out;
  uint64_t out_cap;
  tfs_read_result* results;
  uint32_t* n_bad;  // may be nullptr
  uint32_t n, S;
  int32_t size;     // bytes of every source member
};
hipError_t launch_ec_read_reply(const ReplyArgs& a, hipStream_t stream);

// Marshalling session: the encode of one chunk of the family,
// with the payload CRC of every record of the data members taken from the
// registers that feed the code.  A tile is 4 KiB of every member, counted from
// the members' first byte; `first`, `cont`, `tail`, `hdr` are the session's plan
// and partial results (ec_marshal_plan.h builds the plan).
struct MarshalRec {      // one accepted record of a data member, 16 bytes
  uint32_t H, P1;        // the FileInfo's first byte; the payload is [H + 36, P1)
  uint32_t id_lo, id_hi; // RawMeta.file_id
};
// xpow[i] = x^(8 * (i - kMarshalPowBias)) mod P.  The pass moves a lane's register
// by d_lane - pad, d_lane = 3192 - 1024 u - 8 (l & 15) in [0, 3192], pad in
// [0, 4095]; the fold moves a record's register by P1 - T_last in [1, 4096].
constexpr int kMarshalPowBias = 4095;
constexpr int kMarshalPowN = kMarshalPowBias + 4096 + 1;
constexpr uint32_t kMarshalHdrWords = 9;  // 36 bytes of FileInfo per record
struct MarshalTables {
  uint32_t slice[4][256];        // slice-by-4, as Tables::slice
  uint32_t step_packet[4][256];  // byte tables of shift(c, 128)
  uint32_t xpow[kMarshalPowN];
};
struct MarshalArgs {
  EcArgs ec;                       // the chunk's members; ec.units = len / 1024
  const MarshalTables* tab;
  const MarshalRec* recs;          // accepted records, member after member, ascending by H
  const uint32_t* first;           // [S][ntiles]: first record of member s whose P1 lies past the tile's start
  uint32_t* cont;                  // [S][ntiles]: crc(0, payload bytes up to the tile's end) of the record that runs on
  uint32_t* tail;                  // [rec]: crc(0, payload bytes of the record's last tile)
  uint32_t* hdr;                   // [rec][9]: the record's FileInfo as it passed by
  uint32_t mend[kMaxMembersDev];   // one past member s's last record
  uint32_t tile0;                  // the chunk's first tile (offset / 4096)
  uint32_t ntiles;                 // tiles of the whole member (total rounded up)
};
hipError_t launch_ec_marshal(const MarshalArgs& a, int og, hipStream_t stream);

struct MarshalFoldArgs {
  const MarshalTables* tab;
  const MarshalRec* recs;
  const uint32_t* rec_member;  // [rec]: the data member that holds it
  const uint32_t* cont;
  const uint32_t* tail;
  const uint32_t* hdr;
  const uint32_t* pow_tile;    // [ntiles]: x^(8 * 4096 * k) mod P
  uint32_t* out_crc;           // [rec]
  int32_t* out_status;         // [rec]
  uint32_t n, ntiles;
};
hipError_t launch_ec_marshal_fold(const MarshalFoldArgs& a, hipStream_t stream);

// Reinstate session: the decode of one chunk of the family, with
// the payload CRC of every record of the data members taken from the registers
// that feed the code (surviving data members among the sources) and from the
// registers that hold its output (rebuilt data members).  A slot is the data
// member's number 0 .. dn - 1: it selects the member's rows of `first` and `cont`
// and its entry of `mend`, whatever position the member has among the launch's
// sources or outputs.  Parity members have no records and no slot.
constexpr uint32_t kReinstateNoSlot = 0xFFFFFFFFu;
struct ReinstateArgs {
  MarshalArgs m;                          // as the marshalling pass; first, cont and mend are indexed by slot
  uint32_t src_slot[kMaxMembersDev];      // source s's slot (all kReinstateNoSlot after the first output group)
  uint32_t out_slot[kMaxOutGroup];        // output o's slot
};
hipError_t launch_ec_reinstate(const ReinstateArgs& a, int og, hipStream_t stream);

// Frame-emitting chunk calls (include/tfs_ec_frames.h): the marshalling / reinstate
// pass over one chunk with the outputs' WriteRawDataMessage frames as the destination.  Tile t of the
// call belongs to frame j = t / tpf of the call; output o's packet bytes go to out[o] + j * stride +
// 56 + (t - j * tpf) * 4096, and crc(0, the tile's bytes of output o) goes to tile_crc[(o0 + o) *
// ntiles + T] (T counts from the members' first byte): one writer per word.  The seal kernel, a wave
// per (output, frame), chains a frame's words, joins them with the head and tail and stores the 56
// leading bytes and F.
constexpr uint32_t kFramesHead = 56;    // the V1 header (24) and WriteDataInfo (32) before a frame's data
struct FramesArgs {
  ReinstateArgs r;                    // the pass; r.m.ec.dst[o] is output o's out (the frames of this call)
  uint32_t* tile_crc;                 // [outputs][ntiles]
  uint32_t o0;                        // the launch's first output
  uint32_t tpf;                       // tiles per frame (frame_len / 4096)
  uint32_t stride;                    // bytes between frame starts
  uint32_t len;                       // bytes of the chunk
};
// walk: the launch has a record walk to run (else the session's plan arrays are not read)
hipError_t launch_ec_frames(const FramesArgs& a, int og, bool walk, hipStream_t stream);

struct FramesSealArgs {
  uint8_t* out[kMaxMembersDev];       // by output, in the plan's order
  uint64_t pid[kMaxMembersDev];       // packet_id of the output's frame 0
  uint32_t block_id[kMaxMembersDev];
  uint32_t flag0[kMaxMembersDev];     // F of the frame at data offset 0
  const MarshalTables* tab;
  const uint32_t* tile_crc;           // [outputs][ntiles]
  uint32_t ntiles;                    // tiles of the whole member
  uint32_t n_out, nf;                 // outputs, frames of the call
  uint32_t frame0;                    // the call's first frame (offset / frame_len)
  uint32_t frame_len, stride, total;
  uint32_t type_ver;                  // header bytes 8..11: pcode | version << 16
  uint32_t pow_head_full, pow_head_last;  // ec_frames_plan.h's EcfCallConst
};
hipError_t launch_ec_frames_seal(const FramesSealArgs& a, hipStream_t stream);

// Task chunk calls (include/tfs_ec_fetch.h): the frames pass with the sources' chunks
// given as the RespReadRawDataMessage frames they arrived in.  f.r.m.ec.src[s] is source s's in: frame j
// of the call starts at src[s] + j * in_stride (4 modulo 8), its data 28 bytes on.  blen[s] is the
// source's block_len (`total` for a parity member): the frame at member offset x carries clamp(blen -
// x, 0, requested) data bytes and the pass reads no byte behind them.  src_crc[s * ntiles + T] receives
// crc(0, the data bytes of source s in tile T): one writer per word.
constexpr uint32_t kTaskHead = 28;      // the V1 header (24) and le32(n) before a frame's data
constexpr uint32_t kTaskPcode = 46;     // RESP_READ_RAW_DATA_MESSAGE
constexpr int32_t kTaskError = -1;      // TFS_ERROR
struct TaskArgs {
  FramesArgs f;
  uint32_t blen[kMaxMembersDev];      // by source, in the plan's order
  uint32_t* src_crc;                  // [S][ntiles]; nullptr in the launches of the later output groups
  uint32_t in_stride;                 // bytes between frame starts in a source's in
};
hipError_t launch_ec_task(const TaskArgs& a, int og, bool walk, hipStream_t stream);

// The source check, a wave per (source, frame of the call): results[s * nf + j].
struct TaskCheckArgs {
  const uint8_t* in[kMaxMembersDev];  // by source, in the plan's order
  uint32_t blen[kMaxMembersDev];
  const MarshalTables* tab;
  const uint32_t* src_crc;            // [S][ntiles]
  tfs_ec_fetch_result* results;
  uint32_t ntiles;                    // tiles of the whole member
  uint32_t S, nf;                     // sources, frames of the call
  uint32_t frame0;                    // the call's first frame (offset / frame_len)
  uint32_t frame_len, in_stride, total;
};
hipError_t launch_ec_fetch_check(const TaskCheckArgs& a, hipStream_t stream);

// The seal of a task call: the frames seal, with frame j of every output left unusable (a zero flag
// word) when a source's frame j failed its check.
struct TaskSealArgs {
  FramesSealArgs f;
  const tfs_ec_fetch_result* results;  // [S][f.nf]
  uint32_t S;
};
hipError_t launch_ec_task_seal(const TaskSealArgs& a, hipStream_t stream);

// Scrub session: the marshalling pass over one chunk of a family
// whose parity is stored already.  The code of the data members is compared in
// registers with the stored parity instead of being written; one word per parity
// member and tile receives the four units' verdicts.  No member byte is written.
struct ScrubArgs {
  MarshalArgs m;                       // as the marshalling pass; m.ec.dst is not used by the kernel
  const uint8_t* par[kMaxOutGroup];    // the launch's stored parity members, this chunk
  uint32_t* pbad;                      // [pn][ntiles]: bit u set when unit u of the tile differs
  uint32_t o0;                         // the launch's first parity member
};
// walk: the CRC side runs (the first output group of a session that has records)
hipError_t launch_ec_scrub(const ScrubArgs& a, int og, bool walk, hipStream_t stream);

struct ScrubCountArgs {
  const uint32_t* pbad;  // [pn][ntiles]
  uint32_t* units;       // [pn]: differing units of parity member p
  uint8_t* map;          // [pn][ntiles]: pbad's low four bits
  uint32_t ntiles;
};
hipError_t launch_ec_scrub_count(const ScrubCountArgs& a, int pn, hipStream_t stream);

// Scrub locate: for every listed 1 KiB unit of a family whose members are all
// present, the syndromes of every parity member, the one data member they name when there is
// one, and that member's unit repaired.  Entry k is unit units[k] of every member (units ==
// nullptr: unit k).  The plan's words are ec_locate_plan.h's.  No member byte is written.
struct LocateResult {  // same bytes as tfs_ec_locate_result in include/tfs_ec.h
  int8_t kind, member;
  uint16_t parity, diff_bytes;
  uint8_t flags, zero;
};
static_assert(sizeof(LocateResult) == 8, "locate result layout");
constexpr int kLocateClean = 0, kLocateParity = 1, kLocateData = 2, kLocateNone = 3;
constexpr uint32_t kLocateConfirmed = 1u;
struct LocateArgs {
  const uint8_t* mem[kMaxMembersDev];  // dn data members, then pn parity members
  const uint32_t* masks;               // the encode plan's [pn][8][dn][8] words
  const uint32_t* ratio;               // [(pn - 1)][dn][8][8] words
  const uint32_t* inv0;                // [dn][8][8] words
  const uint32_t* units;               // [n], or nullptr
  LocateResult* result;                // [n]
  uint8_t* fixed;                      // [n][1024], or nullptr
  uint32_t n, dn, pn;
};
hipError_t launch_ec_locate(const LocateArgs& a, hipStream_t stream);

// Parity update: the change of one data member carried into the stored parity.
// Entry k is slot k of the delta buffers (a ^ b, or a alone when b is nullptr) and unit
// list[k] of every bound parity member: the first n_inline entries of `inl` when n_inline != 0,
// else units[k], else (units == nullptr) unit k.  par[p] == nullptr: parity member p is not
// bound, and is neither read nor written.  masks is the encode plan, as LocateArgs::masks.
struct UpdateArgs {
  uint8_t* par[kMaxMembersDev];    // pn parity members
  const uint32_t* masks;           // the encode plan's [pn][8][dn][8] words
  const uint32_t* units;           // [n] in device memory, or nullptr
  const uint8_t* a;                // [n][1024]
  const uint8_t* b;                // [n][1024], or nullptr
  uint32_t inl[kUpdateInline];     // a short list, in the launch arguments (ec_update_plan.h)
  uint32_t n, n_inline, dn, pn, member;
};
hipError_t launch_ec_update(const UpdateArgs& a, hipStream_t stream);

}  // namespace tfsec
