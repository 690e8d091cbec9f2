/*
 * tfs_ec_frames.h -- the erasure-code tasks' pieces leave as sealed raw frames.
 *
 * MarshallingTask::do_marshalling (src/dataserver/task.cpp:1210-1291) posts each
 * parity piece with write_raw_data(..., PARITY_DATA) (:1272-1281), and
 * ReinstateTask::do_reinstate (:1420-1529) each rebuilt piece: NORMAL_DATA for a
 * dead data member (:1484-1498), PARITY_DATA for a dead parity member
 * (:1505-1519).  Each post is a WriteRawDataMessage frame whose body BasePacket
 * checksums (base_packet.cpp:72-75; Task::write_raw_data, task.cpp:86-113).
 *
 * The calls below are chunk calls of the marshalling and reinstate sessions of
 * include/tfs_ec.h.  One call encodes or decodes the chunk, verifies the records
 * exactly as tfs_ec_marshal_encode / tfs_ec_reinstate_decode do, and leaves, for
 * every output member, that chunk's frames complete and sealed in a buffer of its
 * own (each member goes to another server).  The coded bytes go from the
 * registers they are made in to the frames' data areas and are checksummed from
 * those registers; they are written nowhere else and are not read back.
 *
 * Frame layout: include/tfs_replicate.h's, byte for byte -- the 24-byte V1 header
 * (flag TFSN, body length 36 + length, pcode 35, version, id, crc), H (32 bytes:
 * le32 block_id | le64 0 | le32 offset | le32 length | le32 0 | le64 0), D (length
 * data bytes), F (le32 flag_).  Frame k = (offset + j * frame_len) / frame_len of
 * member i lies at out[i] + j * stride and carries id packet_id[i] + k,
 * block_id[i], data offset k * frame_len and length min(frame_len, total - k *
 * frame_len).  F of the frame at data offset 0 is TFS_RAW_PARITY_DATA for a parity
 * member and TFS_RAW_NORMAL_DATA for a rebuilt data member; on every later frame
 * it is 0.  A rebuilt data member's frames cover all of [0, total), zero padding
 * included, as the reference writes decode_len per chunk.
 */
#ifndef TFS_EC_FRAMES_H_
#define TFS_EC_FRAMES_H_

#include "tfs_ec.h"
#include "tfs_replicate.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfs_ec_frames_cfg {
  int32_t  frame_len;     /* data bytes per frame; > 0 and % 4096 == 0; the reference's is TFS_MAX_READ_SIZE */
  uint32_t frame_stride;  /* bytes between frame starts in one member's out; 0: frame_len + 64;
                             else >= frame_len + 60 and % 8 == 0 */
  int16_t  version;       /* header version; the CRC is written when >= 1, else 0 */
  int16_t  reserved;      /* 0 */
  uint32_t block_id[TFS_EC_MAX_MEMBERS];  /* by member index; read for output members only */
  uint64_t packet_id[TFS_EC_MAX_MEMBERS]; /* frame k of member i carries packet_id[i] + k */
} tfs_ec_frames_cfg;

/* Host arithmetic: the bytes one member's out must hold for a call of `len` bytes,
 * (frames - 1) * stride + 60 + the last frame's length; 0 for a NULL or refused cfg
 * or len <= 0. */
uint64_t tfs_ec_frames_cap(const tfs_ec_frames_cfg* cfg, int len);

/* One chunk [offset, offset + len) of the session, as tfs_ec_marshal_encode_device
 * takes it, with sealed frames as the outputs.  `d_members` and `d_out` are indexed
 * by member (dn + pn entries).  d_members[i] is read for the session's source
 * members only (the data members); d_out[i] for its output members only (the
 * parity members); the other entries are ignored.  out_cap applies to each
 * d_out[i].  Alignment: d_out[i] % 8 == 0; with stride % 8 == 0 every frame's data
 * starts at + 56, so the coded bytes leave as whole aligned 8-byte stores.
 *
 * Checks, in this order (a refused call launches nothing and leaves the session
 * where it was):
 *   1. the session, stream and chunk rules of tfs_ec_marshal_encode_device
 *   2. cfg or d_out NULL                                    TFS_EXIT_PARAMETER_ERROR
 *   3. frame_len <= 0 or frame_len % 4096                   TFS_EXIT_SIZE_INVALID
 *   4. 0 < frame_stride < frame_len + 60 or frame_stride % 8, reserved != 0,
 *      offset % frame_len, len % frame_len unless offset + len == total,
 *      a d_out[i] of an output member not 8-byte aligned,
 *      out_cap < tfs_ec_frames_cap(cfg, len)                TFS_EXIT_PARAMETER_ERROR
 *   5. d_members NULL, a NULL source member or a NULL d_out[i] of an output member
 *                                                           TFS_EXIT_DATA_INVALID
 * No byte of d_out[i] outside the call's frames is written, the gap between two
 * frames included.  A session may mix these calls with plain encode chunks; begin,
 * finish, free and the statuses are unchanged.  Asynchronous on `stream`: the
 * frames are complete, header CRC included, when the call's work on the stream is
 * done. */
int tfs_ec_marshal_frames_device(tfs_ec_marshal* m, const tfs_ec_frames_cfg* cfg, void* const* d_members,
                                 void* const* d_out, uint64_t out_cap, int offset, int len, void* stream);

/* Host form, synchronous, on the context's stream under the coder's mutex: the
 * sources are staged up as tfs_ec_marshal_encode stages them, each output's frames
 * are brought down; a page-locked out[i] is written in place. */
int tfs_ec_marshal_frames(tfs_ec_marshal* m, const tfs_ec_frames_cfg* cfg, char* const* members, char* const* out,
                          uint64_t out_cap, int offset, int len);

/* The same for a reinstate session: the sources are the decode plan's, the outputs
 * the dead members. */
int tfs_ec_reinstate_frames_device(tfs_ec_reinstate* s, const tfs_ec_frames_cfg* cfg, void* const* d_members,
                                   void* const* d_out, uint64_t out_cap, int offset, int len, void* stream);
int tfs_ec_reinstate_frames(tfs_ec_reinstate* s, const tfs_ec_frames_cfg* cfg, char* const* members, char* const* out,
                            uint64_t out_cap, int offset, int len);

#ifdef __cplusplus
}
#endif
#endif /* TFS_EC_FRAMES_H_ */
