/*
 * tfs_ec_read.h -- degraded read replies: rebuild, verify and seal the frame in
 * one pass.
 *
 * The read of a record of a LOST block (DataService::read_data_degrade,
 * dataservice.cpp:1713-1796) composed from tfs_ec_read_degraded (tfs_ec.h) and
 * tfs_read_reply (tfs_read.h) rebuilds the record's covering units into a
 * scratch buffer, verifies it there, and reads the scratch again to copy and
 * seal the reply.  Here the rebuilt bytes go from the registers that hold them
 * straight into the reply frame, and the same registers feed the check against
 * FileInfo.crc_ and the frame's header CRC: dn source reads and one frame
 * write, one launch, no scratch.
 *
 * The contract: with refuse_flags == 0, every frame byte, frame_len and
 * tfs_read_result equal what tfs_read_reply yields for the same tfs_read_job
 * over the intact member with src_len = size -- the frame layouts of pcodes
 * 8 / 39 / 63, the trailer, the order of the per-job checks and the sealed
 * 28- / 32-byte error frames are those of tfs_read.h.  A corrupt survivor
 * therefore leaves as a sealed TFS_EXIT_CHECK_CRC_ERROR frame, never as a wrong
 * file under a valid frame CRC.
 *
 * Additions to the per-job checks of tfs_read.h:
 *   TFS_EXIT_PARAMETER_ERROR   also: the job's covering set passes `size`.
 *                              Nothing is read or written for it.
 *   TFS_EXIT_FILE_INFO_ERROR   also: read_offset == 0 and (FileInfo.flag_ &
 *                              refuse_flags) != 0 -- checked after id_ and size_
 *                              and before crc_.  The reference makes this check
 *                              after the decode (data_management.cpp:495-497);
 *                              the flag lives in the lost block, so only the
 *                              kernel can see it.
 *
 * The covering set of a job: the 1 KiB units of the target member that cover the
 * FileInfo [H, H + 36), H = read.src_offset, and those that cover the slice
 * [H + 36 + read_offset, + n).  Each such unit of each of the decode plan's dn
 * source members is read exactly once, and no other unit: a ranged read far into
 * a long file rebuilds the FileInfo's one or two units and the slice's, not what
 * lies between; a read_len == 0 job (the degrade stat) rebuilds the FileInfo's
 * units alone.
 *
 * Two deviations from the reference: its degraded data reply does not subtract
 * 36 from the trailer's size_ although its normal read does (dataservice.cpp:
 * 1556) -- here both replies are identical; and its flag test has a precedence
 * slip (flag_ & (MASK != 0)) -- here the mask is the caller's.
 */
#ifndef TFS_EC_READ_H_
#define TFS_EC_READ_H_

#include "tfs_ec.h"
#include "tfs_read.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfs_ec_reply_job { /* 56 bytes */
  tfs_read_job read;     /* src_offset = RawMeta.offset of the record in the LOST member; rest as in tfs_read.h */
  uint32_t refuse_flags; /* FileInfo.flag_ bits that refuse a first fragment (read_offset == 0); 0: none */
  uint32_t reserved;     /* 0 */
} tfs_ec_reply_job;
typedef char tfs_ec_reply_job_is_56_bytes[sizeof(tfs_ec_reply_job) == 56 ? 1 : -1]; /* static assert, C and C++ */

/* Call-level checks and their order are those of tfs_ec_read_degraded: ec NULL ->
 * TFS_EXIT_PARAMETER_ERROR; no decoding matrix -> TFS_EXIT_MATRIX_INVALID; size < 0
 * or size % 1024 -> TFS_EXIT_SIZE_INVALID; target not a data member, or not erased
 * -> TFS_EXIT_PARAMETER_ERROR; a source member of the decode plan NULL or sizes[i]
 * < size -> TFS_EXIT_DATA_INVALID; device form: hipStreamPerThread ->
 * TFS_EXIT_PARAMETER_ERROR; then n == 0 returns TFS_SUCCESS; jobs, out or results
 * NULL -> TFS_EXIT_PARAMETER_ERROR; the spans [frame_offset, frame_offset +
 * tfs_read_frame_cap(&job.read)) of two jobs that may write overlap ->
 * TFS_EXIT_PARAMETER_ERROR, nothing launched.
 *
 * `jobs` is a host array in both forms and may be reused on return.
 * Device form: members, d_out, d_results and d_n_bad in device memory of ctx's
 * GPU (d_members a host array of pointers, sizes may be NULL), asynchronous on
 * `stream` (NULL: the context's); the plan is uploaded on that stream.  Nothing
 * outside a job's span is written.  Frames whose data starts at an address
 * congruent mod 8 to the slice's first byte in the member (frame + 28 == H + 36 +
 * read_offset mod 8) leave as whole 8-byte stores; any other placement is served
 * with unaligned stores.
 * Host form: synchronous, on the context's stream, under the coder's mutex.  Only
 * the covering sets of the dn source members go up, packed and joined, and only
 * frame_len bytes per frame come down (plus the placement padding between frames
 * that come down in one run, under 16 bytes a frame); a page-locked `out` is
 * written in place.  tfs_ec_read_traffic counts both directions.  Returns
 * TFS_SUCCESS, or TFS_EXIT_CHECK_CRC_ERROR when any job failed, as tfs_read_reply
 * does; *n_bad (may be NULL) is increased by the number of failed jobs. */
int tfs_ec_read_reply_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, int target,
                             const tfs_ec_reply_job* jobs, uint32_t n, void* d_out, uint64_t out_cap,
                             tfs_read_result* d_results, uint32_t* d_n_bad, void* stream);
int tfs_ec_read_reply(tfs_ec* ec, char* const* members, const int* sizes, int size, int target,
                      const tfs_ec_reply_job* jobs, uint32_t n, void* out, uint64_t out_cap,
                      tfs_read_result* results, uint32_t* n_bad);

#ifdef __cplusplus
}
#endif
#endif /* TFS_EC_READ_H_ */
