/*
 * tfs_write.h -- the write path's second checksum without a second pass.
 *
 * On the reference's write path the same payload bytes are checksummed twice:
 * BasePacket::decode checks the WRITE_DATA frame, Func::crc(TFS_PACKET_FLAG_V1,
 * body) (base_packet.cpp:141), and DataFile::get_crc checks the file at close,
 * Func::crc(0, data) (data_file.cpp:168-194).  A WriteDataMessage body is
 * H || D: the 32-byte WriteDataInfo (internal.cpp:606-667; length_ i32 at body
 * bytes 16..19), the vint64 ds_ (serialization.h:298-322: count i32 at body
 * bytes 32..35, then count x 8 bytes) and length_ data bytes
 * (write_data_message.cpp:35-55,71-96).  Func::crc's register is linear, so
 *
 *   Func::crc(0, D) = Func::crc(FLAG, H || D) ^ shift(Func::crc(FLAG, H), |D|),
 *   shift(c, n) = c * x^(8n) mod P:
 *
 * the pass that verifies a write frame also yields the fragment's file CRC, and
 * a close whose fragments all arrived this way combines their CRCs on the host
 * (tfs_crc32_combine) with no GPU work and no second read of the payload.
 */
#ifndef TFS_WRITE_H_
#define TFS_WRITE_H_

#include "tfs_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFS_WRITE_DATA_MESSAGE 9      /* pcode WRITE_DATA_MESSAGE (base_packet.h:207) */
#define TFS_WRITE_MAX_DS 27           /* ds_ entries a frame may carry and still yield a data CRC */

/* One frame's data fragment.  data_off is relative to the body (the byte after
 * the 24-byte header); data_len = -1: the frame yields no data CRC (another
 * pcode, a version-0 frame, a malformed WriteDataInfo / ds_ prefix, or a status
 * other than TFS_SUCCESS) -- recompute at close.  16 bytes. */
typedef struct tfs_write_part {
  int32_t data_off, data_len;
  uint32_t data_crc, reserved;
} tfs_write_part;

/* tfs_packet_verify, and per frame the file CRC of its data: statuses, CRCs and
 * n_bad exactly as tfs_packet_verify; out_parts[i].data_crc = Func::crc(0, D)
 * for a WRITE_DATA frame that decoded with TFS_SUCCESS and whose prefix is
 * well-formed (0 <= count <= 27, length_ >= 0, 36 + 8 count + length_ == body
 * length), data_len = -1 otherwise.  out_parts must not be NULL. */
int tfs_packet_verify_write(tfs_crc_ctx* ctx, const tfs_packet_desc* d, uint32_t n, const void* base,
                            uint64_t base_len, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad,
                            tfs_write_part* out_parts);
/* Device-resident form (asynchronous on `stream`; d_n_bad accumulated into). */
int tfs_packet_verify_write_device(tfs_crc_ctx* ctx, const tfs_packet_desc* d_desc, uint32_t n, const void* d_base,
                                   uint32_t* d_out_crc, int32_t* d_out_status, uint32_t* d_n_bad,
                                   tfs_write_part* d_out_parts, void* stream);
/* CRC of A || B from crc_a = Func::crc(seed, A) (any seed), crc_b = Func::crc(0, B)
 * and len_b = |B|: shift(crc_a, len_b) ^ crc_b.  Host arithmetic on two register
 * values: no context, no GPU call, no payload byte touched. */
uint32_t tfs_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

#ifdef __cplusplus
}
#endif
#endif /* TFS_WRITE_H_ */
