/*
 * tfs_mirror.h -- mirror sync: verify each file and seal its write frames in one
 * pass.
 *
 * TfsMirrorBackup::copy_file (src/dataserver/sync_backup.cpp:315-472) ships a
 * file to the backup cluster: it reads FileInfo || payload in MAX_READ_SIZE
 * pieces, hands every piece to the client, which wraps it in a WriteDataMessage,
 * and closes the destination file with the client's CRC.  Each payload byte is
 * checksummed three times on the way (the running Func::crc at :383,412, the
 * client's own for the CloseFileMessage, the frame's for the wire), and the
 * comparison with FileInfo.crc_ comes at :429, after every write has gone out: a
 * file that rotted on the source lands in the mirror under CRCs that are all
 * valid.  One call here reads each payload byte once and leaves the sealed
 * frames, the close CRC and the verdict; a file that fails never leaves.
 *
 * Frames of one file.  With n = size - 36 payload bytes, frame 0 carries payload
 * bytes [0, min(first_len, n)) and frame k >= 1 carries [first_len + (k - 1) *
 * frame_len, min(first_len + k * frame_len, n)): 1 frame when n <= first_len, else
 * 1 + ceil((n - first_len) / frame_len).  Neither length has an alignment rule;
 * the reference's are TFS_MAX_READ_SIZE - 36 and TFS_MAX_READ_SIZE
 * (sync_backup.cpp:336,370,391-400).
 *
 * Frame k is the serialized 24-byte V1 header (flag TFSN, body length 36 + 8 *
 * count + length, pcode 9, version, id = packet_id + k, crc) followed by the body
 * H || V || D:
 *   H  WriteDataInfo, 32 bytes (internal.cpp:635-663), little-endian:
 *      le32 block_id | le64 file_id | le32 offset | le32 length | le32 is_server
 *      | le64 file_number; offset is the data's place in the payload
 *   V  le32 count | count x le64, Stream::set_vint64 (write_data_message.cpp:
 *      71-90); a caller that holds a lease appends its three entries itself
 *   D  length data bytes
 * The header crc is Func::crc(TFS_PACKET_FLAG_V1, body) when version >= 1, else 0.
 * A job's frames lie back to back from frame_offset, which may be any byte
 * offset; bytes of out outside every job's span are never touched.
 *
 * Per-job statuses, checked in this order:
 *   TFS_EXIT_PARAMETER_ERROR       ds_count > TFS_MIRROR_MAX_DS; ds_first +
 *                                  ds_count passes ds_n; the record passes
 *                                  src_len; the span passes out_cap; reserved
 *                                  != 0.  Nothing is read or written.
 *   TFS_EXIT_READ_FILE_SIZE_ERROR  size <= 36 (sync_backup.cpp:348).  Nothing
 *                                  is written.  (A job of size <= 36 has no span;
 *                                  its record is max(size, 0) bytes.)
 *   TFS_EXIT_FILE_INFO_ERROR       FileInfo.id_ != file_id
 *   TFS_EXIT_SYNC_FILE_ERROR       FileInfo.size_ != size
 *   TFS_EXIT_CHECK_CRC_ERROR       Func::crc(0, payload) != FileInfo.crc_
 * A job that fails one of the last three leaves no usable frame: n_frames =
 * span_len = 0, and the four flag bytes of each of its frames are zero after the
 * call, so the streamer rejects them (base_packet_streamer.cpp:78-79); the other
 * bytes of its span are unspecified.
 */
#ifndef TFS_MIRROR_H_
#define TFS_MIRROR_H_

#include "tfs_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef TFS_WRITE_DATA_MESSAGE          /* (include/tfs_write.h has the same two) */
#define TFS_WRITE_DATA_MESSAGE 9        /* base_packet.h:207 */
#define TFS_WRITE_MAX_DS 27
#endif
#ifndef TFS_MAX_READ_SIZE               /* (include/tfs_replicate.h has the same) */
#define TFS_MAX_READ_SIZE 1048576       /* internal.h:130 */
#endif

#define TFS_MIRROR_MAX_DS 27            /* == TFS_WRITE_MAX_DS: the receiver's frame check still yields the data CRC */
#define TFS_MIRROR_FRAME_HEAD 60        /* 24 header + 32 WriteDataInfo + 4 count, before the ds entries */

typedef struct tfs_mirror_cfg {         /* 16 bytes */
  int32_t first_len, frame_len;         /* > 0; the reference's: TFS_MAX_READ_SIZE - 36, TFS_MAX_READ_SIZE */
  int32_t is_server;                    /* WriteDataInfo.is_server_ */
  int16_t version, reserved;            /* reserved == 0 */
} tfs_mirror_cfg;

typedef struct tfs_mirror_job {         /* 64 bytes */
  uint64_t src_offset;                  /* of the record's FileInfo in the source */
  uint64_t frame_offset;                /* of its first frame in out */
  uint64_t file_id;                     /* RawMeta.file_id; also WriteDataInfo.file_id_ (FSName keeps both ids) */
  uint64_t file_number;                 /* from the destination's create-file reply */
  uint64_t packet_id;                   /* frame k carries packet_id + k */
  uint32_t block_id;                    /* WriteDataInfo.block_id_ */
  int32_t  size;                        /* RawMeta.size */
  uint32_t ds_first, ds_count;          /* V = ds[ds_first .. ds_first + ds_count) of the call's ds array */
  uint64_t reserved;                    /* 0 */
} tfs_mirror_job;

typedef struct tfs_mirror_result {      /* 16 bytes */
  int32_t  status;
  uint32_t n_frames;                    /* 0 unless status == TFS_SUCCESS */
  uint32_t span_len;                    /* bytes to send from frame_offset; 0 unless TFS_SUCCESS */
  uint32_t file_crc;                    /* Func::crc(0, payload) as recomputed: CloseFileMessage.crc_ */
} tfs_mirror_result;

/* Host arithmetic: the frames of a file of `size` record bytes; 0 for a NULL cfg,
 * first_len <= 0, frame_len <= 0 or size <= 36. */
uint32_t tfs_mirror_frame_count(const tfs_mirror_cfg* cfg, int32_t size);

/* Host arithmetic: the bytes the job may write from frame_offset, frames * (60 +
 * 8 * ds_count) + size - 36; 0 where tfs_mirror_frame_count is 0, for a NULL job
 * or ds_count > TFS_MIRROR_MAX_DS. */
uint64_t tfs_mirror_span(const tfs_mirror_cfg* cfg, const tfs_mirror_job* job);

/* Device-resident form: d_src (src_len bytes), d_out (out_cap bytes), d_results (n
 * entries) and d_n_bad (may be NULL; increased by the jobs that did not succeed)
 * are device addresses; `jobs` (n entries) and `ds` (ds_n entries) are host arrays
 * that may be reused on return.  Asynchronous on `stream` (NULL: the context's;
 * hipStreamPerThread is refused); the frames and results are complete when the
 * call's work on the stream is done.  d_out may not overlap d_src.  Call-level
 * checks, TFS_EXIT_PARAMETER_ERROR with nothing launched: a NULL ctx, cfg, out or
 * results; NULL jobs with n > 0; NULL ds with ds_n > 0; NULL src with src_len > 0;
 * first_len <= 0, frame_len <= 0 or cfg.reserved != 0; the spans of two jobs that
 * may write sharing a byte.  Returns TFS_SUCCESS once the work is queued (n == 0
 * queues nothing). */
int tfs_mirror_frames_device(tfs_crc_ctx* ctx, const tfs_mirror_cfg* cfg, const void* d_src, uint64_t src_len,
                             const tfs_mirror_job* jobs, uint32_t n, const uint64_t* ds, uint32_t ds_n, void* d_out,
                             uint64_t out_cap, tfs_mirror_result* d_results, uint32_t* d_n_bad, void* stream);

/* Host form, synchronous, on the context's stream.  A page-locked src is read in
 * place and a page-locked out is written in place; a pageable side is staged
 * through the context's buffers in pieces.  *n_bad (may be NULL) is increased by
 * the jobs that did not succeed.  Returns TFS_EXIT_CHECK_CRC_ERROR when any job
 * failed, as tfs_read_reply does. */
int tfs_mirror_frames(tfs_crc_ctx* ctx, const tfs_mirror_cfg* cfg, const void* src, uint64_t src_len,
                      const tfs_mirror_job* jobs, uint32_t n, const uint64_t* ds, uint32_t ds_n, void* out,
                      uint64_t out_cap, tfs_mirror_result* results, uint32_t* n_bad);

#ifdef __cplusplus
}
#endif
#endif /* TFS_MIRROR_H_ */
