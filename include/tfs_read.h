/*
 * tfs_read.h -- read replies: verify the file and seal the frame in one pass.
 *
 * On a read the reference touches every byte that leaves twice: verify-on-read
 * runs Func::crc(0, payload) against FileInfo.crc_, then BasePacket::reply runs
 * Func::crc(TFS_PACKET_FLAG_V1, body) over a body that is the same payload
 * behind a 4-byte length (base_packet.cpp:192-209, read_data_message.cpp:
 * 240-252,307-328, dataservice.cpp:1466-1597).  Func::crc's register is linear:
 * with L = the 4 little-endian bytes of the data length, D the data and T what
 * follows it in the body,
 *
 *   crc(FLAG, L || D)      = shift(crc(FLAG, L), |D|) ^ crc(0, D)
 *   crc(FLAG, L || D || T) = crc(seed = crc(FLAG, L || D), T),
 *
 * so one read of the payload feeds the check against crc_, the copy into the
 * reply frame and the frame's header CRC.  T is at most 40 bytes, made from the
 * FileInfo.
 *
 * Frame of a job (n = min(read_len, size - 36 - read_offset)): the serialized
 * 24-byte V1 header (flag TFSN, body length, pcode, version, packet_id, crc),
 * then the body: le32(n) | n data bytes for pcode 8; for pcodes 39 and 63 that,
 * followed by RespReadDataMessageV2::serialize's trailer -- le32(36) | FileInfo
 * (as stored, size_ less 36, dataservice.cpp:1556) when read_offset == 0,
 * le32(0) when read_offset > 0.
 *
 * Checks per job, in this order:
 *   TFS_EXIT_PARAMETER_ERROR       a pcode other than 8 / 39 / 63; read_offset or
 *                                  read_len < 0; read_offset past the payload
 *                                  (read_offset > max(size - 36, 0)); the record
 *                                  passes src_len; the job's span passes out_cap.
 *                                  Nothing is read or written; frame_len = 0.
 *   TFS_EXIT_READ_FILE_SIZE_ERROR  size < 36 (an empty file, size == 36, is served)
 *   TFS_EXIT_FILE_INFO_ERROR       FileInfo.id_ != file_id
 *   TFS_EXIT_SYNC_FILE_ERROR       FileInfo.size_ != size
 *   TFS_EXIT_CHECK_CRC_ERROR       the job covers the whole payload
 *                                  (read_offset == 0 && n == size - 36) and
 *                                  crc(0, payload) != crc_
 * A job that reads a part of the file gets the first four checks only.
 *
 * A job that fails any check but the first still yields a sealed frame, the
 * reference's set_length(ret) reply: body le32(status) for pcode 8 (28 bytes),
 * le32(status) | le32(0) for pcodes 39 and 63 (32 bytes) -- a corrupt file never
 * leaves under a valid frame CRC.  Bytes of a job's span past frame_len are
 * unspecified; bytes of out outside every job's [frame_offset, frame_offset +
 * tfs_read_frame_cap(job)) are not touched.  The spans of two jobs may not
 * overlap (TFS_EXIT_PARAMETER_ERROR for the call, nothing launched).
 */
#ifndef TFS_READ_H_
#define TFS_READ_H_

#include "tfs_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFS_RESP_READ_DATA_MESSAGE 8      /* base_packet.h pcodes */
#define TFS_RESP_READ_DATA_MESSAGE_V2 39
#define TFS_RESP_READ_DATA_MESSAGE_V3 63

typedef struct tfs_read_job {   /* 48 bytes */
  uint64_t src_offset;    /* of the record's FileInfo in the source (64-bit: many block images in one buffer) */
  uint64_t frame_offset;  /* where the reply frame starts in out; any byte offset */
  uint64_t file_id;       /* RawMeta.file_id */
  uint64_t packet_id;     /* header id of the reply (the request's id + 1, base_packet.cpp:195) */
  int32_t  size;          /* RawMeta.size: 36-byte FileInfo + payload */
  int32_t  read_offset;   /* into the payload, >= 0 */
  int32_t  read_len;      /* payload bytes asked for, >= 0; cut at the payload's end (logic_block.cpp:388-391) */
  int16_t  pcode;         /* 8 RESP_READ_DATA_MESSAGE; 39 / 63 RESP_READ_DATA_MESSAGE_V2 / _V3 */
  int16_t  version;       /* the request's; the header CRC is written when >= 1, else 0 */
} tfs_read_job;

typedef struct tfs_read_result { /* 16 bytes */
  int32_t  status;     /* TFS_SUCCESS or one of the codes above */
  uint32_t frame_len;  /* bytes of the frame to send, from frame_offset */
  uint32_t file_crc;   /* Func::crc(0, payload) when the whole payload was read, else 0 */
  uint32_t frame_crc;  /* the CRC stored in the header (0 when version < 1) */
} tfs_read_result;

/* Host arithmetic: the bytes from frame_offset a job may write (24 + 4 + n + the
 * trailer; 0 for a pcode that is none of the three). */
uint32_t tfs_read_frame_cap(const tfs_read_job* job);

/* Device-resident form, asynchronous on `stream` (NULL: the context's stream;
 * hipStreamPerThread is refused).  `jobs` is a host array (the requests arrive on
 * the host) and may be reused when the call returns; d_src, d_out, d_results and
 * d_n_bad are device addresses.  *d_n_bad is increased by the number of jobs
 * whose status is not TFS_SUCCESS (NULL: not counted).  Returns TFS_SUCCESS when
 * the launch was queued. */
int tfs_read_reply_device(tfs_crc_ctx* ctx, const void* d_src, uint64_t src_len, const tfs_read_job* jobs, uint32_t n,
                          void* d_out, uint64_t out_cap, tfs_read_result* d_results, uint32_t* d_n_bad, void* stream);

/* Host form, synchronous.  A page-locked src is read in place and a page-locked
 * out is written in place (only the named bytes cross PCIe); a pageable side is
 * staged: only the records go up and only the frames come down, in pieces when
 * they do not fit.  *n_bad (may be NULL) is increased by the number of failed
 * jobs.  Returns TFS_SUCCESS, or TFS_EXIT_CHECK_CRC_ERROR when any job failed, as
 * tfs_packet_verify does. */
int tfs_read_reply(tfs_crc_ctx* ctx, const void* src, uint64_t src_len, const tfs_read_job* jobs, uint32_t n,
                   void* out, uint64_t out_cap, tfs_read_result* results, uint32_t* n_bad);

#ifdef __cplusplus
}
#endif
#endif /* TFS_READ_H_ */
