/*
 * tfs_repair.h -- file repair: check the fetched reply frames, verify the file
 * and seal the update's write frames in one pass.
 *
 * BlockChecker::do_repair_crc answers a CrcCheckFile with FileRepair::fetch_file
 * and FileRepair::repair_file (src/dataserver/file_repair.cpp:81-197): the file
 * is read from a good replica in MAX_READ_SIZE pieces, each arriving as a
 * RespReadDataMessage(_V2/_V3) frame that BasePacket::decode checksums; the data
 * goes to a temporary file, Func::crc runs over it again (:142), and
 * save_file_update reads it back and writes it through the client, which
 * checksums it for the CloseFileMessage and once more per WriteDataMessage: four
 * checksums and two copies of every payload byte.  One call here reads each
 * payload byte once: it checks every incoming frame, computes the file CRC and
 * compares it with what fstat and the CrcCheckFile say, and leaves the sealed
 * WriteDataMessage frames of the update and the CRC for its close.  A file whose
 * fetched copy is wrong never leaves as an update.
 *
 * Incoming frames.  A job's payload arrives as in_count reply frames, in payload
 * order, each anywhere in the source at any byte offset: the 24-byte V1 header,
 * the body le32(n_k) || n_k data bytes || T, where the trailer T is nothing for
 * pcode 8 and le32(36) || FileInfo (40 bytes) or le32(0) (4 bytes) for pcodes 39
 * and 63 (include/tfs_read.h).  The host declares each frame (tfs_repair_parse)
 * and the device checks the frame's own bytes against the declaration.  The
 * trailer's FileInfo is covered by the frame check and otherwise not
 * interpreted: the reference trusts fstat.
 *
 * Outgoing frames are include/tfs_mirror.h's WriteDataMessage frames: the header
 * with pcode 9 and id packet_id + k, H (32-byte WriteDataInfo, offset the data's
 * place in the payload), V (le32 count | count x le64) and the data.  Frame k
 * carries payload [k * frame_len, min((k + 1) * frame_len, n)); the frames lie
 * back to back from frame_offset; the header crc is Func::crc(TFS_PACKET_FLAG_V1,
 * body) when version >= 1, else 0.
 *
 * Per-job statuses, decided in this order:
 *   TFS_EXIT_PARAMETER_ERROR       on the host, nothing read or written:
 *                                  ds_count > TFS_WRITE_MAX_DS or the ds range
 *                                  passing ds_n; the in range passing n_in;
 *                                  in_count == 0; a frame with data_len < 0, with
 *                                  avail < 28 + data_len + trailer, or passing
 *                                  src_len; a pcode that is none of 8, 39, 63 or a
 *                                  trailer that does not belong to it; the out
 *                                  span passing out_cap or 32 bits; reserved != 0
 *   TFS_EXIT_READ_FILE_SIZE_ERROR  stat_size <= 0 (file_repair.cpp:128); host
 *   TFS_EXIT_SYNC_FILE_ERROR       the data_len of the job's frames do not sum
 *                                  to stat_size (:154); host
 *   TFS_ERROR                      a frame's own bytes against its declaration:
 *                                  flag != TFS_PACKET_FLAG_V1; header body length
 *                                  != 4 + data_len + trailer; header pcode != the
 *                                  declared one; body le32 != data_len; the
 *                                  trailer's leading le32 != 36 (40-byte trailer)
 *                                  or != 0 (4-byte trailer).  bad_in is set.
 *   TFS_EXIT_CHECK_CRC_ERROR       a frame of version >= 1 whose header crc !=
 *                                  Func::crc(TFS_PACKET_FLAG_V1, body).  bad_in
 *                                  is set.
 *   TFS_EXIT_CHECK_CRC_ERROR       Func::crc(0, payload) != stat_crc, or !=
 *                                  check_crc; bad_in = TFS_REPAIR_NO_FRAME and
 *                                  flags say which.
 * bad_in is the lowest failing frame of the job.  A job that fails one of the
 * last three leaves no usable frame, as in tfs_mirror.h: n_frames = span_len = 0
 * and the four flag bytes of each of its outgoing frames are zero; file_crc is
 * still reported as computed.  Bytes of out outside every job's span are never
 * touched, and no byte of the source is written.
 */
#ifndef TFS_REPAIR_H_
#define TFS_REPAIR_H_

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

#define TFS_REPAIR_RESP_READ 8          /* RESP_READ_DATA_MESSAGE, base_packet.h */
#define TFS_REPAIR_RESP_READ_V2 39      /* RESP_READ_DATA_MESSAGE_V2 */
#define TFS_REPAIR_RESP_READ_V3 63      /* RESP_READ_DATA_MESSAGE_V3 */
#define TFS_REPAIR_IN_HEAD 28           /* 24 header + the body's le32 length, before the data */
#define TFS_REPAIR_NO_FRAME 0xffffffffu /* tfs_repair_result.bad_in: no incoming frame failed */
#define TFS_REPAIR_STAT_MISMATCH 1u     /* flags: file CRC != stat_crc */
#define TFS_REPAIR_CHECK_MISMATCH 2u    /* flags: file CRC != check_crc */

typedef struct tfs_repair_in {          /* 24 bytes: one incoming reply frame */
  uint64_t frame_off;                   /* of its header in the source */
  uint32_t avail;                       /* bytes of the source that belong to it */
  int32_t  data_len;                    /* declared n_k */
  int16_t  pcode;                       /* 8, 39 or 63 */
  int16_t  trailer;                     /* 0 (pcode 8); 4 or 40 (pcodes 39, 63) */
  uint32_t reserved;                    /* 0 */
} tfs_repair_in;

typedef struct tfs_repair_job {         /* 72 bytes: one file */
  uint64_t frame_offset;                /* of its first outgoing frame in out */
  uint64_t file_id;                     /* CrcCheckFile.file_id_; WriteDataInfo.file_id_ */
  uint64_t file_number;                 /* from the update's create-file reply */
  uint64_t packet_id;                   /* outgoing frame k carries packet_id + k */
  int64_t  stat_size;                   /* TfsFileStat.size_: payload bytes */
  uint32_t block_id;                    /* WriteDataInfo.block_id_ */
  uint32_t in_first, in_count;          /* its frames: ins[in_first .. in_first + in_count) */
  uint32_t ds_first, ds_count;          /* V = ds[ds_first .. ds_first + ds_count) */
  uint32_t stat_crc;                    /* TfsFileStat.crc_ */
  uint32_t check_crc;                   /* CrcCheckFile.crc_ */
  uint32_t reserved;                    /* 0 */
} tfs_repair_job;

typedef struct tfs_repair_cfg {         /* 12 bytes */
  int32_t frame_len;                    /* > 0; the reference's: TFS_MAX_READ_SIZE */
  int32_t is_server;                    /* WriteDataInfo.is_server_ */
  int16_t version, reserved;            /* of the outgoing frames; reserved == 0 */
} tfs_repair_cfg;

typedef struct tfs_repair_result {      /* 24 bytes */
  int32_t  status;
  uint32_t n_frames;                    /* 0 unless status == TFS_SUCCESS */
  uint32_t span_len;                    /* bytes to send from frame_offset; 0 unless TFS_SUCCESS */
  uint32_t file_crc;                    /* Func::crc(0, payload) as computed: CloseFileMessage.crc_ */
  uint32_t bad_in;                      /* the job's first incoming frame that failed, or TFS_REPAIR_NO_FRAME */
  uint32_t flags;                       /* TFS_REPAIR_STAT_MISMATCH | TFS_REPAIR_CHECK_MISMATCH */
} tfs_repair_result;

/* Host arithmetic: the outgoing frames of a file of stat_size payload bytes,
 * ceil(stat_size / frame_len); 0 for a NULL cfg, frame_len <= 0, stat_size <= 0
 * or a count that does not fit 32 bits. */
uint32_t tfs_repair_frame_count(const tfs_repair_cfg* cfg, int64_t stat_size);

/* Host arithmetic: the bytes the job may write from frame_offset, frames * (60 +
 * 8 * ds_count) + stat_size; 0 where tfs_repair_frame_count is 0, for a NULL job
 * or ds_count > TFS_WRITE_MAX_DS. */
uint64_t tfs_repair_span(const tfs_repair_cfg* cfg, const tfs_repair_job* job);

/* Host arithmetic on host-readable bytes: declares the reply frame at `frame`
 * (avail bytes, at frame_off of the source to be) from body bytes 0..3 (the
 * header's body length is the device's to compare); `pcode` is what the caller asked for, `first` non-zero for
 * the file's first reply (the one that carries the FileInfo under pcodes 39 and
 * 63).  TFS_EXIT_PARAMETER_ERROR for a NULL frame or out or a pcode that is none
 * of 8, 39, 63; TFS_PACKET_INCOMPLETE with fewer than 28 bytes.  A negative
 * length field is the source's error reply (set_length(status)): that negative
 * value is returned and *out is left untouched.  Else 0. */
int tfs_repair_parse(const void* frame, uint32_t avail, uint64_t frame_off, int32_t pcode, int32_t first,
                     tfs_repair_in* out);

/* Device-resident form: d_src (src_len bytes), d_out (out_cap bytes), d_results (n
 * entries) and d_n_bad (may be NULL; increased by the jobs that did not succeed)
 * are device addresses; `ins` (n_in entries), `jobs` (n entries) and `ds` (ds_n
 * entries) are host arrays that may be reused on return.  Asynchronous on `stream`
 * (NULL: the context's; hipStreamPerThread is refused); the frames and results are
 * complete when the call's work on the stream is done.  d_out may not overlap
 * d_src.  Call-level checks, TFS_EXIT_PARAMETER_ERROR with nothing launched: a
 * NULL ctx, cfg, out or results; NULL jobs with n > 0; NULL ins with n_in > 0; NULL
 * ds with ds_n > 0; NULL src with src_len > 0; frame_len <= 0 or cfg.reserved != 0;
 * the spans of two jobs that may write sharing a byte.  Returns TFS_SUCCESS once
 * the work is queued (n == 0 queues nothing). */
int tfs_repair_frames_device(tfs_crc_ctx* ctx, const tfs_repair_cfg* cfg, const void* d_src, uint64_t src_len,
                             const tfs_repair_in* ins, uint32_t n_in, const tfs_repair_job* jobs, uint32_t n,
                             const uint64_t* ds, uint32_t ds_n, void* d_out, uint64_t out_cap,
                             tfs_repair_result* d_results, uint32_t* d_n_bad, void* stream);

/* Host form, synchronous, on the context's stream.  A page-locked src is read in
 * place and a page-locked out is written in place; a pageable side is staged
 * through the context's buffers in pieces of whole jobs.  *n_bad (may be NULL) is
 * increased by the jobs that did not succeed.  Returns TFS_EXIT_CHECK_CRC_ERROR
 * when any job failed. */
int tfs_repair_frames(tfs_crc_ctx* ctx, const tfs_repair_cfg* cfg, const void* src, uint64_t src_len,
                      const tfs_repair_in* ins, uint32_t n_in, const tfs_repair_job* jobs, uint32_t n,
                      const uint64_t* ds, uint32_t ds_n, void* out, uint64_t out_cap, tfs_repair_result* results,
                      uint32_t* n_bad);

#ifdef __cplusplus
}
#endif
#endif /* TFS_REPAIR_H_ */
