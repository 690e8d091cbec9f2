/*
 * tfs_receive.h -- replica receive: check the raw frames, land them, verify every
 * record in one pass.
 *
 * DataService::write_raw_data (src/dataserver/dataservice.cpp:2487-2529) gets a
 * WriteRawDataMessage that BasePacket::decode has checksummed (base_packet.cpp:
 * 141); DataManagement::write_raw_data (data_management.cpp:861-885) and
 * LogicBlock::write_raw_data (logic_block.cpp:795-815) copy its bytes into the
 * new block at offset_.  After the last frame DataService::batch_write_info
 * (dataservice.cpp:2531-2566) hands the RawMetaVec to LogicBlock::batch_write_meta
 * (logic_block.cpp:817-858) and the replica is committed.  No byte of it is ever
 * compared with the FileInfo.crc_ of the record it belongs to.  A receive session
 * reads each frame byte once and gives all three: the frame's wire check, the
 * bytes landed in the block image, and at the end every record's verdict.
 *
 * The records are known only at the end (WriteInfoBatchMessage follows the data),
 * so the pass leaves one 32-bit word per granule of TFS_RECEIVE_GRANULE bytes of
 * the block, anchored at block offsets 0, G, 2G, ...:
 *   word = Func::crc(0, granule bytes received so far || zeros up to its end)
 * Func::crc's register is linear, so a record's payload CRC is folded at finish
 * from the words of the granules it covers whole and from its two edges, which
 * are re-read from the landed image: at most 2 (G - 1) + 36 bytes a record.
 *
 * A frame is the 24-byte V1 header followed by the body H || D || F (tfs_replicate.h
 * describes it), 60 + data_len bytes in all.
 *
 * Per-frame status, decided on the device from the frame's own bytes, in this order:
 *   TFS_ERROR                  flag != TFS_PACKET_FLAG_V1
 *   TFS_ERROR                  header body length != 36 + data_len
 *   TFS_ERROR                  pcode != TFS_WRITE_RAW_DATA_MESSAGE
 *   TFS_ERROR                  H.block_id_ != cfg.block_id
 *   TFS_ERROR                  H.offset_ / H.length_ differ from the declared values
 *   TFS_EXIT_CHECK_CRC_ERROR   version >= 1 and header crc != Func::crc(FLAG, body)
 * Per-record statuses at finish are those of tfs_replicate.h, with total = the
 * bytes received.
 */
#ifndef TFS_RECEIVE_H_
#define TFS_RECEIVE_H_

#include "tfs_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef TFS_EXIT_DATA_INVALID           /* (include/tfs_ec.h and tfs_replicate.h have the same two) */
#define TFS_EXIT_DATA_INVALID (-16001)   /* error_msg.h:217 */
#define TFS_EXIT_SIZE_INVALID (-16002)   /* error_msg.h:218 */
#endif

#define TFS_RECEIVE_GRANULE 4096        /* bytes of the block behind one session word */
#define TFS_RECEIVE_FRAME_OVERHEAD 60   /* 24 header + 32 WriteDataInfo + 4 flag_ */
#define TFS_RECEIVE_PCODE 35            /* WRITE_RAW_DATA_MESSAGE, base_packet.h:233 */

/* The granule the library was built with; callers and tests read it here. */
uint32_t tfs_receive_granule(void);

typedef struct tfs_receive_cfg {   /* 16 bytes */
  uint32_t block_id;    /* WriteDataInfo.block_id_ every frame must carry */
  int32_t  image_cap;   /* bytes the image can hold, >= 0 */
  uint32_t reserved[2]; /* 0 */
} tfs_receive_cfg;

typedef struct tfs_receive_desc {  /* 24 bytes: one frame of a call */
  uint64_t frame_off;   /* frame starts at base + frame_off */
  uint32_t avail;       /* bytes available there */
  int32_t  data_offset; /* declared WriteDataInfo.offset_ */
  int32_t  data_len;    /* declared WriteDataInfo.length_ */
  uint32_t reserved;
} tfs_receive_desc;

typedef struct tfs_receive_part {  /* 16 bytes: one frame's outcome */
  int32_t  status;      /* the list above */
  uint32_t crc;         /* Func::crc(FLAG, body) as computed; 0 for a version-0 frame */
  int32_t  flag;        /* le32(F): the frame's flag_ */
  uint32_t reserved;    /* 0 */
} tfs_receive_part;

typedef struct tfs_receive tfs_receive;

/* Host arithmetic on host-readable bytes, no context: fills out->frame_off and
 * out->avail from the arguments and data_offset / data_len from body bytes 12..19
 * (what the dataserver's own deserialize reads); reserved = 0.  TFS_PACKET_INCOMPLETE
 * when fewer than 56 bytes are available (out untouched), TFS_EXIT_PARAMETER_ERROR
 * for a NULL frame or out, else TFS_SUCCESS. */
int tfs_receive_parse(const void* frame, uint32_t avail, uint64_t frame_off, tfs_receive_desc* out);

/* Opens a session over one new block.  d_image is device memory, or the device
 * address of page-locked memory, of image_cap bytes; the session keeps the
 * pointer.  Call-level checks, in this order:
 *   1. ctx, cfg or out NULL                                  TFS_EXIT_PARAMETER_ERROR
 *   2. image_cap < 0                                         TFS_EXIT_SIZE_INVALID
 *   3. reserved != 0, or d_image NULL with image_cap > 0     TFS_EXIT_PARAMETER_ERROR
 * One session is used by one thread at a time, on one stream. */
int tfs_receive_begin(tfs_crc_ctx* ctx, const tfs_receive_cfg* cfg, void* d_image, tfs_receive** out);

/* n frames lie in device memory at d_base + descs[j].frame_off (descs: host memory,
 * may be reused on return).  Frames arrive in order: frame j's data_offset equals
 * the session's cursor (0 at the start, then the previous frame's end), across
 * calls and within one; data_len >= 0, data_offset + data_len <= image_cap, avail
 * >= 60 + data_len; any frame length is legal.  All of this is checked on the host
 * before anything is queued: a refused call (TFS_EXIT_PARAMETER_ERROR; also a NULL
 * session, d_base, descs or d_parts with n > 0, a call after finish) leaves image,
 * outputs and session untouched.  d_parts[j] (device) receives frame j's outcome and
 * *d_n_bad (device, may be NULL) is increased by the frames whose status is not
 * TFS_SUCCESS.  The declared range [data_offset, data_offset + data_len) of the image
 * is written whatever the status (the caller drops the block); no other byte of the
 * image and no byte of d_base is written.  Findings are reported, not returned.
 * Asynchronous on `stream` (NULL: the context's; hipStreamPerThread is refused, and
 * so is a stream other than the session's first: TFS_EXIT_PARAMETER_ERROR). */
int tfs_receive_frames_device(tfs_receive* s, const void* d_base, const tfs_receive_desc* descs, uint32_t n,
                              tfs_receive_part* d_parts, uint32_t* d_n_bad, void* stream);

/* Host form, synchronous, on the context's stream: base is host memory of base_len
 * bytes (every frame_off + avail <= base_len), parts and n_bad host memory.  A
 * page-locked base is read in place; a pageable base is staged in pieces of whole
 * frames.  The image is always the session's d_image. */
int tfs_receive_frames(tfs_receive* s, const void* base, uint64_t base_len, const tfs_receive_desc* descs,
                       uint32_t n, tfs_receive_part* parts, uint32_t* n_bad);

/* metas (host, n entries, any order, overlaps allowed: each record is independent)
 * is the RawMetaVec as batch_write_info gets it.  out_crc[i] / out_status[i] (may be
 * NULL) come in the caller's order: the payload CRC as folded (0 for a record out of
 * range or with size <= 36) and the status; the FileInfo is read from the landed
 * image, and finish reads from the image only FileInfos and edges.  *n_bad (may be
 * NULL) is increased by the records that did not succeed; *out_total (may be NULL)
 * receives the cursor.  n == 0 is legal (parity members, rebuilt pieces).  May be
 * called once (again: TFS_EXIT_PARAMETER_ERROR); synchronises. */
int tfs_receive_finish(tfs_receive* s, const tfs_raw_meta* metas, uint32_t n, uint32_t* out_crc,
                       int32_t* out_status, uint32_t* n_bad, int32_t* out_total);

int tfs_receive_free(tfs_receive* s);

#ifdef __cplusplus
}
#endif
#endif /* TFS_RECEIVE_H_ */
