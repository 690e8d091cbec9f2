/*
 * tfs_replicate.h -- block replication: verify every record and seal the raw
 * frames in one pass.
 *
 * ReplicateTask::do_replicate (src/dataserver/task.cpp:1025-1090; the same loop
 * moves a block during balancing) reads a block's data file in MAX_READ_SIZE
 * pieces with read_raw_data, wraps each piece in a WriteRawDataMessage
 * (Task::write_raw_data, task.cpp:86-113) and commits with batch_write_index.
 * BasePacket checksums every frame for the wire (base_packet.cpp:72-75), but no
 * byte is checked against the record it belongs to: a record that rotted on the
 * source is copied under a valid frame CRC.  A replicate session reads each
 * source byte once and gives both: the sealed frames of every chunk, ready to
 * send, and at the end every record's verdict against its own FileInfo.
 *
 * Frame k of the block carries data bytes [k * frame_len, min((k + 1) *
 * frame_len, total)) (length = their count; the one frame of an empty data file
 * has length 0).  It is the serialized 24-byte V1 header (flag TFSN, body length
 * 36 + length, pcode 35, version, id = packet_id + k, crc) followed by the body
 * H || D || F, 60 + length bytes in all:
 *   H  WriteDataInfo, 32 bytes (internal.cpp:635-667), little-endian:
 *      le32 block_id | le64 0 | le32 offset | le32 length | le32 0 | le64 0
 *   D  length data bytes (write_data_message.cpp:230-248)
 *   F  le32(flag_): new_block on the frame at offset 0, else 0 (task.cpp:97-100)
 * The header CRC is Func::crc(TFS_PACKET_FLAG_V1, body); the id is outside it,
 * so a sender may overwrite it.
 *
 * Per-record statuses.  Given at begin (the record takes no part in the record
 * pass; its bytes still travel in the frames like any gap):
 *   TFS_EXIT_PARAMETER_ERROR       offset < 0 or offset + size > total
 *   TFS_EXIT_READ_FILE_SIZE_ERROR  size <= 36
 * Given at finish, checked in this order, exactly as tfs_block_verify gives them
 * for the same image and metas:
 *   TFS_EXIT_FILE_INFO_ERROR       FileInfo.id_ != file_id
 *   TFS_EXIT_SYNC_FILE_ERROR       FileInfo.size_ != size
 *   TFS_EXIT_CHECK_CRC_ERROR       Func::crc(0, payload) != FileInfo.crc_
 */
#ifndef TFS_REPLICATE_H_
#define TFS_REPLICATE_H_

#include "tfs_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef TFS_EXIT_DATA_INVALID           /* (include/tfs_ec.h has the same two) */
#define TFS_EXIT_DATA_INVALID (-16001)   /* error_msg.h:217 */
#define TFS_EXIT_SIZE_INVALID (-16002)   /* error_msg.h:218 */
#endif

#define TFS_WRITE_RAW_DATA_MESSAGE 35   /* base_packet.h:233 */
#define TFS_RAW_NORMAL_DATA 1           /* RawDataType, internal.h:1023-1027 */
#define TFS_RAW_PARITY_DATA 2
#define TFS_RAW_FRAME_OVERHEAD 60       /* 24 header + 32 WriteDataInfo + 4 flag_ */
#define TFS_MAX_READ_SIZE 1048576       /* internal.h:130 */

typedef struct tfs_replicate_cfg {      /* 32 bytes */
  uint64_t packet_id;     /* frame k of the block carries packet_id + k */
  uint32_t block_id;      /* WriteDataInfo.block_id_ (the destination's block) */
  int32_t  total;         /* the data file's length, get_data_file_size(); any byte count >= 0 */
  int32_t  frame_len;     /* data bytes per frame; > 0 and % 1024 == 0; the reference's is TFS_MAX_READ_SIZE */
  uint32_t frame_stride;  /* bytes between frame starts in a call's out; 0: frame_len + 60; else >= frame_len + 60 */
  int16_t  new_block;     /* flag_ of the frame at offset 0: TFS_RAW_NORMAL_DATA or TFS_RAW_PARITY_DATA */
  int16_t  version;       /* header version; the CRC is written when >= 1, else 0 */
  uint32_t reserved;      /* 0 */
} tfs_replicate_cfg;

typedef struct tfs_replicate tfs_replicate;

/* Host arithmetic: the frames of the block, max(1, ceil(total / frame_len)); 0 for
 * a NULL cfg, total < 0 or frame_len <= 0. */
uint32_t tfs_replicate_frame_count(const tfs_replicate_cfg* cfg);

/* Opens a session over one block.  `metas` (host, n entries, may be reused on
 * return) name its records, ascending by offset and not overlapping; n == 0 is
 * legal: the session then only copies and seals (parity and rebuilt pieces sent
 * with TFS_RAW_PARITY_DATA).  Call-level checks, in this order:
 *   1. ctx, cfg or out NULL                                   TFS_EXIT_PARAMETER_ERROR
 *   2. total < 0, frame_len <= 0 or frame_len % 1024          TFS_EXIT_SIZE_INVALID
 *   3. 0 < frame_stride < frame_len + 60, new_block not 1 or 2,
 *      reserved != 0                                          TFS_EXIT_PARAMETER_ERROR
 *   4. n != 0 with metas NULL                                 TFS_EXIT_PARAMETER_ERROR
 *   5. the records that take part do not ascend, or overlap   TFS_EXIT_PARAMETER_ERROR
 * One session is used by one thread at a time, on one stream. */
int tfs_replicate_begin(tfs_crc_ctx* ctx, const tfs_replicate_cfg* cfg, const tfs_raw_meta* metas, uint32_t n,
                        tfs_replicate** out);

/* Bytes [offset, offset + len) of the data file are at d_src (which points at
 * byte `offset`, as read_raw_data delivers it).  Calls arrive in order: the first
 * at 0, each next where the last ended; offset % frame_len == 0, and len %
 * frame_len == 0 unless offset + len == total; len > 0 unless total == 0 (whose one
 * legal call is offset 0, len 0, src may be NULL: the reference's single empty
 * frame).  Frame j of the call is written at d_out + j * stride, 60 + its length
 * bytes; no other byte of d_out is touched, and out_cap must hold
 * (frames - 1) * stride + 60 + the last frame's length.  Anything else is
 * TFS_EXIT_PARAMETER_ERROR with nothing launched and the session unchanged; a NULL
 * src with len > 0 or a NULL out is TFS_EXIT_DATA_INVALID.  d_out may not overlap
 * d_src.  Asynchronous on `stream` (NULL: the context's; hipStreamPerThread is
 * refused, and so is a stream other than the session's first:
 * TFS_EXIT_PARAMETER_ERROR); the frames are complete, header CRC included, when the call's work on
 * the stream is done, and d_src / d_out may be reused then. */
int tfs_replicate_frames_device(tfs_replicate* s, const void* d_src, int offset, int len,
                                void* d_out, uint64_t out_cap, void* stream);

/* Host form, synchronous, on the context's stream.  A page-locked src is read in
 * place and a page-locked out is written in place; a pageable side is staged
 * through the context's buffers, in pieces of whole frames. */
int tfs_replicate_frames(tfs_replicate* s, const void* src, int offset, int len, void* out, uint64_t out_cap);

/* Needs [0, total) covered (else TFS_EXIT_PARAMETER_ERROR).  Folds on the
 * session's stream and synchronises.  out_crc[i] / out_status[i] (n entries each,
 * may be NULL) come in the caller's meta order: the payload CRC as recomputed (0
 * for a record rejected at begin) and the status above.  *n_bad (may be NULL) is
 * increased by the records that did not succeed; out_frame_crc (may be NULL)
 * receives the header CRC of every frame, tfs_replicate_frame_count entries.
 * Findings are reported, not returned: TFS_SUCCESS for a block full of bad
 * records. */
int tfs_replicate_finish(tfs_replicate* s, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad,
                         uint32_t* out_frame_crc);

int tfs_replicate_free(tfs_replicate* s);

#ifdef __cplusplus
}
#endif
#endif /* TFS_REPLICATE_H_ */
