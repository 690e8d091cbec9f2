/*
 * tfs_ec_fetch.h -- the erasure-code tasks' source pieces enter as the reply
 * frames they arrived in.
 *
 * MarshallingTask::do_marshalling (src/dataserver/task.cpp:1210-1291) and
 * ReinstateTask::do_reinstate (:1420-1529) fetch every source piece with
 * Task::read_raw_data (:115-169): one RespReadRawDataMessage frame per piece,
 * checksummed by BasePacket::decode, the data lifted out by memcpy (:141) and the
 * rest of the piece zero-filled where the member is shorter than the chunk
 * (:1225-1228, :1437-1440).
 *
 * The calls below are chunk calls of the marshalling and reinstate sessions of
 * include/tfs_ec.h.  One call takes each source member's chunk as those frames,
 * checks every frame against what the session expects of it, codes the chunk from
 * the frames' data bytes (zeros behind them), verifies the records exactly as
 * tfs_ec_marshal_encode / tfs_ec_reinstate_decode do, and leaves every output
 * member's frames sealed as tfs_ec_*_frames_device does (include/tfs_ec_frames.h).
 * The data bytes are read once: the pieces that feed the code feed the frame's
 * checksum from the same registers.
 *
 * Incoming frame (read_data_message.cpp:215-252,371-394, base_packet.h:244), byte
 * for byte: the 24-byte V1 header (flag TFSN, body length 8 + n, pcode 46, version,
 * id, crc), then the body le32(n) | n data bytes | le32(data_file_size).  The data
 * starts at + 28; the header crc is Func::crc(TFS_PACKET_FLAG_V1, body) for version
 * >= 1.  Frame j of the call of source member i lies at in[i] + j * in_stride.
 * Incoming and outgoing frames share one grid, the frame_len of the
 * tfs_ec_frames_cfg passed with the call: frame j of every output depends on
 * exactly frame j of every source.
 *
 * Expected length.  The n a frame must carry is host arithmetic from the session's
 * sizes[] (tfs_ec_fetch_expect); the device compares the frame's own bytes with
 * it.  A frame whose expected n is 0 is neither read nor checked -- the reference
 * does not fetch it past offset 0 (:1233) -- and gets status TFS_SUCCESS with
 * n = 0; in[i] may be NULL when every frame of the call is such.  The code and the
 * record walk are fed the frame's data bytes [0, n) and zeros after them: the
 * trailer, the gap to the next frame and anything else in `in` enter neither.
 *
 * Per-frame statuses, in this order:
 *   TFS_ERROR                 flag != TFSN; header body length != 8 + n;
 *                             pcode != 46; body le32 != the expected n
 *   TFS_EXIT_CHECK_CRC_ERROR  version >= 1 and header crc != Func::crc(FLAG, body)
 * data_file_size is reported, not judged: the caller holds it against what it
 * began with.  When source frame j fails, frame j of every output member of the
 * call is unusable the way include/tfs_mirror.h marks it: its four flag bytes are
 * zero, which base_packet_streamer.cpp:78-79 rejects; its data area may hold
 * anything inside the frame.  Other frames of the call are unaffected, no byte
 * outside the call's frames is written, and the record walk still runs over what
 * arrived -- its verdicts at finish are no substitute for the frame results.
 */
#ifndef TFS_EC_FETCH_H_
#define TFS_EC_FETCH_H_

#include "tfs_ec_frames.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFS_RESP_READ_RAW_DATA_MESSAGE 46 /* base_packet.h:244 */
#define TFS_EC_FETCH_HEAD 28              /* the V1 header and le32(n) before a frame's data */
#define TFS_EC_FETCH_OVERHEAD 32          /* ... and le32(data_file_size) behind it */

typedef struct tfs_ec_fetch_cfg {
  uint32_t in_stride; /* bytes between frame starts in one member's in; 0: frame_len + 32;
                         else >= frame_len + 32 and % 8 == 0 */
  uint32_t reserved;  /* 0 */
} tfs_ec_fetch_cfg;

/* One per (source member, frame of the call). */
typedef struct tfs_ec_fetch_result {
  int32_t  status;
  uint32_t n;              /* as the frame declares it (body bytes 0..3); 0 for a frame that is not read */
  int32_t  data_file_size; /* as the frame's trailer carries it */
  uint32_t crc;            /* the body CRC as computed; 0 for a frame that is not read */
} tfs_ec_fetch_result;

/* Host arithmetic: the bytes one member's in must hold for a call of `len` bytes,
 * counted from in[i]: (frames - 1) * in_stride + 36 + the last frame's length -- the
 * end of the aligned 8-byte word that holds the last frame's last byte (in[i] % 8 ==
 * 4).  0 for a NULL or refused cfg or len <= 0. */
uint64_t tfs_ec_fetch_cap(const tfs_ec_frames_cfg* frames_cfg, const tfs_ec_fetch_cfg* fetch_cfg, int len);

/* Host arithmetic: the n that the frame at member offset `offset`, asked for
 * `requested` bytes, must carry: clamp(block_len - offset, 0, requested).  block_len
 * is sizes[member] for a data member (member < dn) and `total` for a parity member.
 * -1 for NULL sizes, a member outside [0, TFS_EC_MAX_MEMBERS) or a negative
 * argument. */
int32_t tfs_ec_fetch_expect(const int* sizes, int dn, int total, int member, int offset, int requested);

/* Host arithmetic on host-readable bytes: declares the reply frame at `frame`
 * (avail bytes) from body bytes 0..3 and, when the frame is complete, its trailer.
 * TFS_EXIT_PARAMETER_ERROR for a NULL frame, out_n or out_data_file_size;
 * TFS_PACKET_INCOMPLETE with fewer than 32 bytes or fewer than 32 + n.  A negative
 * length field is the source's error reply (set_length(status),
 * dataservice.cpp:1822): that negative value is returned and the outputs are left
 * untouched.  Else 0.  Nothing is checksummed here. */
int tfs_ec_fetch_parse(const void* frame, uint32_t avail, int32_t* out_n, int32_t* out_data_file_size);

/* One chunk [offset, offset + len) of the session with frames in and frames out.
 * `d_in` and `d_out` are indexed by member (dn + pn entries): d_in[i] is read for
 * the session's source members only, d_out[i] for its output members only, the
 * other entries are ignored.  d_results receives one tfs_ec_fetch_result per
 * (source in the plan's order -- ascending member number --, frame of the call):
 * entry s * frames + j.  Alignment: d_in[i] % 8 == 4, so that with in_stride % 8 ==
 * 0 every frame's data is 8-byte aligned at + 28 and is read in whole aligned
 * 8-byte loads; the call may read up to the end of the aligned 8-byte word that
 * holds a frame's last byte (tfs_ec_fetch_cap includes it) and reads no other byte
 * outside the frames.  d_out, out_cap and the frames' layout: tfs_ec_frames.h.
 *
 * Checks, in this order (a refused call launches nothing and leaves the session,
 * d_out and d_results where they were):
 *   1. the session, stream and chunk rules of tfs_ec_marshal_encode_device
 *   2. frames_cfg, d_out, fetch_cfg, d_in or d_results NULL  TFS_EXIT_PARAMETER_ERROR
 *   3. frame_len <= 0 or frame_len % 4096                   TFS_EXIT_SIZE_INVALID
 *   4. check 4 of tfs_ec_marshal_frames_device, then
 *      0 < in_stride < frame_len + 32 or in_stride % 8, fetch_cfg->reserved != 0,
 *      a d_in[i] of a source member with a frame to read that is not NULL and not
 *      4 modulo 8                                           TFS_EXIT_PARAMETER_ERROR
 *   5. a NULL d_in[i] of a source member with a frame to read, a NULL d_out[i] of
 *      an output member                                     TFS_EXIT_DATA_INVALID
 * A session may mix these calls with plain chunks and with frames chunks; begin,
 * finish, free and the record verdicts are unchanged.  Asynchronous on `stream`:
 * the call returns TFS_SUCCESS once queued; results and frames are complete when
 * the call's work on the stream is done. */
int tfs_ec_marshal_task_device(tfs_ec_marshal* m, const tfs_ec_frames_cfg* frames_cfg, const tfs_ec_fetch_cfg* fetch_cfg,
                               const void* const* d_in, void* const* d_out, uint64_t out_cap,
                               tfs_ec_fetch_result* d_results, int offset, int len, void* stream);

/* Host form, synchronous, on the context's stream under the coder's mutex.  in[i]
 * may lie at any address: the library places the frames when it stages them up; a
 * page-locked in[i] that meets the device rule is read in place.  The outputs come
 * down as tfs_ec_marshal_frames brings them; `results` is host memory.  Returns
 * TFS_EXIT_CHECK_CRC_ERROR when any frame's status is not TFS_SUCCESS (the chunk
 * is consumed all the same: the session goes on at offset + len). */
int tfs_ec_marshal_task(tfs_ec_marshal* m, const tfs_ec_frames_cfg* frames_cfg, const tfs_ec_fetch_cfg* fetch_cfg,
                        const char* const* in, char* const* out, uint64_t out_cap, tfs_ec_fetch_result* results,
                        int offset, int len);

/* The same for a reinstate session: the sources are the decode plan's survivors,
 * data and parity members alike; the outputs are the dead members. */
int tfs_ec_reinstate_task_device(tfs_ec_reinstate* s, const tfs_ec_frames_cfg* frames_cfg,
                                 const tfs_ec_fetch_cfg* fetch_cfg, const void* const* d_in, void* const* d_out,
                                 uint64_t out_cap, tfs_ec_fetch_result* d_results, int offset, int len, void* stream);
int tfs_ec_reinstate_task(tfs_ec_reinstate* s, const tfs_ec_frames_cfg* frames_cfg, const tfs_ec_fetch_cfg* fetch_cfg,
                          const char* const* in, char* const* out, uint64_t out_cap, tfs_ec_fetch_result* results,
                          int offset, int len);

#ifdef __cplusplus
}
#endif
#endif /* TFS_EC_FETCH_H_ */
