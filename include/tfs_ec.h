/*
 * tfs_ec.h -- C ABI of the MI355X erasure-code region kernels.
 *
 * Drop-in for tfs::dataserver::ErasureCode (src/dataserver/erasure_code.{h,cpp})
 * as MarshallingTask / ReinstateTask / DataManagement use it (task.cpp:1179-1290,
 * 1382-1480; data_management.cpp:293-400): a Cauchy Reed-Solomon code over
 * GF(2^8) (polynomial 0435) in jerasure's bitmatrix form, w = 8, packetsize =
 * 128, so every call works on whole 1 KiB units.  Output bytes are identical to
 * jerasure_bitmatrix_encode / _dotprod (jerasure.cpp:304-348,1345-1364); the
 * byte work runs on the GPU, the matrix setup on the host.
 *
 * Members: dn data + pn parity buffers ("disks"), dn + pn <= 12
 * (MAX_MARSHALLING_NUM, common/internal.h:170).  Status codes as error_msg.h.
 */
#ifndef TFS_EC_H_
#define TFS_EC_H_

#include <stdint.h>

#include "tfs_crc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFS_EXIT_NO_MEMORY (-16000)      /* error_msg.h:216 */
#define TFS_EXIT_DATA_INVALID (-16001)   /* error_msg.h:217 */
#define TFS_EXIT_SIZE_INVALID (-16002)   /* error_msg.h:218 */
#define TFS_EXIT_MATRIX_INVALID (-16003) /* error_msg.h:219 */
#define TFS_EXIT_NO_ENOUGH_DATA (-16004) /* error_msg.h:220 */
#define TFS_EC_WORD_SIZE 8               /* ErasureCode::ws_ */
#define TFS_EC_PACKET_SIZE 128           /* ErasureCode::ps_ */
#define TFS_EC_UNIT 1024                 /* ws_ * ps_: sizes must be multiples */
#define TFS_EC_MAX_MEMBERS 12

typedef struct tfs_ec tfs_ec;

/* ErasureCode::config(dn, pn, erased) (erasure_code.cpp:49-119).  erased ==
 * NULL configures encode only; otherwise erased[dn+pn] holds 0 alive, 1 dead,
 * -1 not used, and the decoding plan is built: TFS_EXIT_NO_ENOUGH_DATA when
 * fewer than dn members are alive, TFS_EXIT_MATRIX_INVALID when the surviving
 * rows are singular.  *out is set even on failure (the coder then refuses to
 * decode) and must be released with tfs_ec_free. */
int tfs_ec_config(tfs_crc_ctx* ctx, int dn, int pn, const int* erased, tfs_ec** out);
int tfs_ec_free(tfs_ec* ec);

/* ErasureCode::encode(size) (:141-175): parity members dn..dn+pn-1 get the
 * code of data members 0..dn-1 over [0, size).  Checks in the reference's
 * order: no matrix -> TFS_EXIT_MATRIX_INVALID; size % 1024 ->
 * TFS_EXIT_SIZE_INVALID; a NULL member or sizes[i] < size ->
 * TFS_EXIT_DATA_INVALID.  Device form: members are device pointers of ctx's
 * GPU (host array of dn+pn pointers), sizes may be NULL (all large enough);
 * asynchronous on `stream`.  Host form: host buffers, synchronous. */
int tfs_ec_encode_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, void* stream);
int tfs_ec_encode(tfs_ec* ec, char* const* members, const int* sizes, int size);

/* ErasureCode::decode(size) (:177-235): rebuild every erased data member
 * (erased != 0) and every dead parity member (erased == 1) from the first dn
 * alive members.  Same checks as encode (a coder configured without `erased`
 * has no decoding matrix -> TFS_EXIT_MATRIX_INVALID). */
int tfs_ec_decode_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, void* stream);
int tfs_ec_decode(tfs_ec* ec, char* const* members, const int* sizes, int size);

/* Degraded read (DataManagement::read_data_degrade, data_management.cpp:283-506):
 * the records, or any byte ranges, of ONE erased data member `target`, rebuilt
 * from the decode plan's dn source members in one pass.  No other erased member
 * is rebuilt and nothing outside the jobs' covering ranges is read.  A record
 * job names a record as the lost block's index does (RawMeta: file id, offset
 * of its FileInfo, size with the FileInfo) and is verified on the rebuilt bytes,
 * which the reference does not do (:476-501 look at the id and flags only): a
 * corrupt survivor shows as TFS_EXIT_CHECK_CRC_ERROR instead of a wrong file.
 *
 * The covering range of a job is [offset rounded down to 1024, offset + size
 * rounded up to 1024); its units are written whole at out + out_offset, so the
 * job's own bytes start at out_offset + offset % 1024 (the reference's
 * data_buffer / offset_in_buffer, :383-408).  Bytes of out outside every
 * covering range are not touched; the out ranges of two jobs may not overlap.
 * out_status[i], in this order:
 *   TFS_EXIT_PARAMETER_ERROR        offset < 0, the covering range passes `size`,
 *                                   out_offset % 1024, or the range passes out_cap
 *   TFS_EXIT_READ_FILE_SIZE_ERROR   record job with size <= 36
 *     (nothing is written in these two cases; the bytes are written in all others)
 *   TFS_EXIT_FILE_INFO_ERROR        FileInfo.id_ != file_id
 *   TFS_EXIT_SYNC_FILE_ERROR        FileInfo.size_ != size
 *   TFS_EXIT_CHECK_CRC_ERROR        Func::crc(0, payload, size - 36) != FileInfo.crc_
 *   TFS_SUCCESS
 * A TFS_EC_READ_RANGE job only has the first check.  out_crc[i] is the payload
 * CRC as recomputed (0 for range jobs and jobs rejected before reading);
 * *n_bad (may be NULL) is increased by the number of jobs that did not succeed. */
#define TFS_EC_READ_RANGE 1u /* flags bit 0: any byte range, rebuilt, not checked */
typedef struct tfs_ec_read_job { /* 32 bytes */
  uint64_t file_id;    /* RawMeta.file_id of the record (unused by RANGE) */
  uint64_t out_offset; /* multiple of 1024: where the first covering unit lands in out */
  int32_t offset;      /* RawMeta.offset: byte offset in the target member (RANGE: range start) */
  int32_t size;        /* RawMeta.size: 36-byte FileInfo + payload (RANGE: bytes) */
  uint32_t flags;
  uint32_t reserved;   /* 0 */
} tfs_ec_read_job;

/* Call-level checks, in this order: ec NULL -> TFS_EXIT_PARAMETER_ERROR; no
 * decoding matrix -> TFS_EXIT_MATRIX_INVALID; size < 0 or size % 1024 ->
 * TFS_EXIT_SIZE_INVALID; target not a data member, or not erased ->
 * TFS_EXIT_PARAMETER_ERROR; a source member of the decode plan NULL or
 * sizes[i] < size -> TFS_EXIT_DATA_INVALID.  Erased members and alive members
 * the plan does not read may be NULL.
 * Device form: everything in device memory of ctx's GPU (d_members a host array
 * of pointers, sizes may be NULL), asynchronous on `stream` (NULL: the
 * context's; hipStreamPerThread is refused).  Host form: host memory,
 * synchronous; only the covering ranges of the source members go to the GPU and
 * only the covering units come back. */
int tfs_ec_read_degraded_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, int target,
                                const tfs_ec_read_job* d_jobs, uint32_t n, void* d_out, uint64_t out_cap,
                                uint32_t* d_out_crc, int32_t* d_out_status, uint32_t* d_n_bad, void* stream);
int tfs_ec_read_degraded(tfs_ec* ec, char* const* members, const int* sizes, int size, int target,
                         const tfs_ec_read_job* jobs, uint32_t n, void* out, uint64_t out_cap,
                         uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad);

/* Marshalling session (MarshallingTask::do_marshalling, task.cpp:1173-1355): the
 * parity of a family, encoded chunk by chunk as the data blocks arrive, with
 * every record of the data members verified against its own FileInfo from the
 * bytes that feed the code -- one read of every data byte.  The reference
 * encodes whatever arrived; a record that was already corrupt is then sealed
 * into the parity.  The library reports it; what follows is the dataserver's.
 *
 * begin: metas[i] / n_metas[i] is the index of data member i (i < dn) as
 * read_raw_index yields it (metas or n_metas NULL: no records), sizes[i] that
 * member's block_len, total the reference's encode_total_len (the longest
 * member rounded up to 1024).  Checks, in this order: ec NULL ->
 * TFS_EXIT_PARAMETER_ERROR; no encoding matrix -> TFS_EXIT_MATRIX_INVALID;
 * total <= 0 or total % 1024 -> TFS_EXIT_SIZE_INVALID; sizes[i] < 0 or
 * sizes[i] > total -> TFS_EXIT_DATA_INVALID; a member's metas not ascending by
 * offset or overlapping, the individually rejected ones set aside ->
 * TFS_EXIT_PARAMETER_ERROR.  A record with offset < 0 or offset + size >
 * sizes[i] gets TFS_EXIT_PARAMETER_ERROR, one with size <= 36
 * TFS_EXIT_READ_FILE_SIZE_ERROR; such a record has its status from begin and
 * takes no part in the pass.
 *
 * encode: tfs_ec_encode(_device) for [offset, offset + len) of the members;
 * members[i] (dn + pn of them) points at that chunk of member i, the data
 * members zero-filled past their block_len as the reference's memset leaves
 * them.  Chunks arrive in order: the first at 0, each next one where the last
 * ended.  offset % 4096 == 0, len % 1024 == 0, and len % 4096 == 0 unless
 * offset + len == total; anything else, a skipped or repeated chunk included,
 * is TFS_EXIT_PARAMETER_ERROR with nothing launched; a NULL member is
 * TFS_EXIT_DATA_INVALID.  Device form: asynchronous on `stream` (NULL: the
 * context's; hipStreamPerThread is refused), and every call of a session uses
 * the same stream.  The chunk buffers may be reused once the call's work on the
 * stream is done.  Host form: synchronous, on the context's stream, staged
 * through the coder's device buffers (dn * len up, pn * len down).
 *
 * finish: TFS_EXIT_PARAMETER_ERROR unless [0, total) has been covered.  Folds
 * the partial CRCs on the session's stream, brings the results to the host and
 * synchronises.  The order is member 0's metas, then member 1's, and so on;
 * out_status[j] is TFS_EXIT_FILE_INFO_ERROR (FileInfo.id_ != file_id),
 * TFS_EXIT_SYNC_FILE_ERROR (FileInfo.size_ != size), TFS_EXIT_CHECK_CRC_ERROR
 * or TFS_SUCCESS, in this order, as tfs_block_verify; out_crc[j] is the payload
 * CRC as recomputed (0 for records rejected at begin); *n_bad (may be NULL) is
 * increased by the number of records that did not succeed.  A session is used
 * by one thread at a time and freed before its coder. */
typedef struct tfs_ec_marshal tfs_ec_marshal;

int tfs_ec_marshal_begin(tfs_ec* ec, const tfs_raw_meta* const* metas, const uint32_t* n_metas, const int* sizes,
                         int total, tfs_ec_marshal** out);
int tfs_ec_marshal_encode_device(tfs_ec_marshal* m, void* const* d_members, int offset, int len, void* stream);
int tfs_ec_marshal_encode(tfs_ec_marshal* m, char* const* members, int offset, int len);
int tfs_ec_marshal_finish(tfs_ec_marshal* m, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad);
int tfs_ec_marshal_free(tfs_ec_marshal* m);

/* Reinstate session (ReinstateTask::do_reinstate, task.cpp:1376-1641): the dead
 * members of a family, rebuilt chunk by chunk from the survivors, with every
 * record of every data member verified against its own FileInfo in the same
 * pass -- the surviving data members from the bytes that feed the code, the
 * rebuilt ones from the bytes the code yields, each read or made once.  The
 * reference writes the rebuilt pieces out unseen (:1478-1519): one corrupt
 * survivor, data or parity, becomes wrong files in every rebuilt block, for
 * good.  The library reports it; what follows is the dataserver's.
 *
 * begin: over a coder configured with `erased` (tfs_ec_config).  metas[i] /
 * n_metas[i] is the index of data member i (i < dn): for an alive member as
 * read_raw_index(READ_DATA_INDEX) yields it, for a dead one (erased == 1) the
 * index a surviving parity block keeps (READ_PARITY_INDEX, :1547-1559); an
 * unused member (erased == -1) has no records.  sizes[i] is the member's
 * block_len -- for a dead member the length its records are checked against,
 * `total` when the caller knows no better -- and total the reference's
 * decode_total_len (:1455-1465).  Checks, in this order: ec NULL ->
 * TFS_EXIT_PARAMETER_ERROR; no decoding matrix -> TFS_EXIT_MATRIX_INVALID; a
 * decode plan without outputs (nothing to reinstate), or n_metas[i] != 0 for an
 * unused member -> TFS_EXIT_PARAMETER_ERROR; then the checks of
 * tfs_ec_marshal_begin from `total` on, with the same per-record statuses
 * given at begin (offset < 0 or offset + size > sizes[i]:
 * TFS_EXIT_PARAMETER_ERROR; size <= 36: TFS_EXIT_READ_FILE_SIZE_ERROR).
 *
 * decode: tfs_ec_decode(_device) for [offset, offset + len) of the members;
 * members[i] (dn + pn of them) points at that chunk of member i, the alive
 * members zero-filled past their block_len (:1437-1440).  The decode plan's
 * sources (the first dn alive members) and outputs (every erased data member,
 * every dead parity member) must be bound: a NULL one is
 * TFS_EXIT_DATA_INVALID; alive members the plan does not read may be NULL.
 * The chunk rule, the stream rule and the buffer-reuse rule are the marshalling
 * session's: chunks in order from 0, offset % 4096 == 0, len % 1024 == 0, and
 * len % 4096 == 0 unless offset + len == total, anything else
 * TFS_EXIT_PARAMETER_ERROR with nothing launched; the device form is
 * asynchronous on `stream` (NULL: the context's; hipStreamPerThread is
 * refused), one stream per session; the chunk buffers may be reused once the
 * call's work on the stream is done.  Host form: synchronous, on the context's
 * stream, staged through the coder's device buffers (sources up, dn * len;
 * outputs down; nothing else travels).
 *
 * finish: as tfs_ec_marshal_finish.  TFS_EXIT_PARAMETER_ERROR unless [0, total)
 * has been covered; folds on the session's stream and synchronises.  The order
 * is member 0's metas, then member 1's, over all dn data members, alive and
 * rebuilt alike; out_status[j] is TFS_EXIT_FILE_INFO_ERROR,
 * TFS_EXIT_SYNC_FILE_ERROR, TFS_EXIT_CHECK_CRC_ERROR or TFS_SUCCESS, in this
 * order, as tfs_block_verify; out_crc[j] is the payload CRC as recomputed (0
 * for records rejected at begin); *n_bad (may be NULL) is increased by the
 * number of records that did not succeed.  Every alive data member is a source
 * of the plan, so one session verifies every record of the family.  A session
 * is used by one thread at a time and freed before its coder. */
typedef struct tfs_ec_reinstate tfs_ec_reinstate;

int tfs_ec_reinstate_begin(tfs_ec* ec, const tfs_raw_meta* const* metas, const uint32_t* n_metas, const int* sizes,
                           int total, tfs_ec_reinstate** out);
int tfs_ec_reinstate_decode_device(tfs_ec_reinstate* s, void* const* d_members, int offset, int len, void* stream);
int tfs_ec_reinstate_decode(tfs_ec_reinstate* s, char* const* members, int offset, int len);
int tfs_ec_reinstate_finish(tfs_ec_reinstate* s, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad);
int tfs_ec_reinstate_free(tfs_ec_reinstate* s);

/* Scrub session (beyond the reference, which never re-reads a family between
 * marshalling and the next loss): the stored parity of a family compared with
 * the code of its data members as they are read, chunk by chunk, and every
 * record of the data members verified against its own FileInfo in the same
 * pass -- one read of every byte of every member, no member byte written.  A
 * parity byte that went wrong or stale, and a data byte that rotted where no
 * record covers it, show while the family still has every member.  The library
 * reports; what follows is the dataserver's.
 *
 * begin: exactly tfs_ec_marshal_begin -- any coder with an encoding matrix;
 * metas, n_metas, sizes and total with the same meaning; the same checks in
 * the same order (ec NULL -> TFS_EXIT_PARAMETER_ERROR; no encoding matrix ->
 * TFS_EXIT_MATRIX_INVALID; total <= 0 or total % 1024 -> TFS_EXIT_SIZE_INVALID;
 * sizes[i] < 0 or sizes[i] > total -> TFS_EXIT_DATA_INVALID; metas not
 * ascending or overlapping -> TFS_EXIT_PARAMETER_ERROR) and the same
 * per-record statuses given at begin (offset < 0 or offset + size > sizes[i]:
 * TFS_EXIT_PARAMETER_ERROR; size <= 36: TFS_EXIT_READ_FILE_SIZE_ERROR).
 *
 * check: members[i] (dn + pn of them) points at [offset, offset + len) of
 * member i; the data members zero-filled past their block_len, as the
 * marshalling loop leaves them, the parity members as stored.  All dn + pn
 * must be bound: a NULL one is TFS_EXIT_DATA_INVALID.  The chunk rule, the
 * stream rule and the buffer-reuse rule are the marshalling session's: chunks
 * in order from 0, offset % 4096 == 0, len % 1024 == 0, and len % 4096 == 0
 * unless offset + len == total, anything else TFS_EXIT_PARAMETER_ERROR with
 * nothing launched; the device form is asynchronous on `stream` (NULL: the
 * context's; hipStreamPerThread is refused), one stream per session; the chunk
 * buffers may be reused once the call's work on the stream is done.  Nothing
 * is written to any member.  Host form: synchronous, on the context's stream,
 * staged through the coder's device buffers ((dn + pn) * len up, nothing down).
 *
 * finish: TFS_EXIT_PARAMETER_ERROR unless [0, total) has been covered.  Folds,
 * copies the results and synchronises, as tfs_ec_marshal_finish; out_crc,
 * out_status and *n_bad are exactly that call's, for every record of the dn
 * data members.  out_parity_units[p] (p < pn; may be NULL): the number of
 * 1 KiB units of parity member p whose stored bytes differ from the code of
 * the data bytes as read.  out_tile_map (may be NULL): pn rows of
 * ceil(total / 4096) bytes; bit u (0..3) of byte [p][T] is set when unit u of
 * tile T of parity member p differs; bits of units at or past total are 0.
 * Mismatches are reported, not returned: finish returns TFS_SUCCESS for a
 * family full of errors, and *n_bad counts records only.  A session is used by
 * one thread at a time and freed before its coder. */
typedef struct tfs_ec_scrub tfs_ec_scrub;

int tfs_ec_scrub_begin(tfs_ec* ec, const tfs_raw_meta* const* metas, const uint32_t* n_metas, const int* sizes,
                       int total, tfs_ec_scrub** out);
int tfs_ec_scrub_check_device(tfs_ec_scrub* s, const void* const* d_members, int offset, int len, void* stream);
int tfs_ec_scrub_check(tfs_ec_scrub* s, const char* const* members, int offset, int len);
int tfs_ec_scrub_finish(tfs_ec_scrub* s, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad,
                        uint32_t* out_parity_units, uint8_t* out_tile_map);
int tfs_ec_scrub_free(tfs_ec_scrub* s);

/* Scrub locate (beyond the reference): for 1 KiB units that a scrub session
 * flagged, which data member is wrong there, and that member's right bytes --
 * while every member is still present, without a decode and without declaring
 * a member dead.  A scrub names a data member only through a failed record; a
 * byte that rotted in a gap between records, in a deleted record or under a
 * FileInfo that is itself hit leaves an unattributed unit.  The encode matrix
 * is Cauchy, m[p][j] = 1 / (p ^ (pn + j)), and for every parity row o >= 1 the
 * ratios m[o][j] / m[0][j] are pairwise distinct over the data members j.  Let
 * S_p be stored parity p XOR the code of the data members as given (8 packets
 * per unit), and F the parity members with S_p != 0 anywhere in the unit:
 *   F empty                     TFS_EC_LOCATE_CLEAN
 *   F a proper subset           TFS_EC_LOCATE_PARITY: the data and the other
 *                               parity members agree (classify_scrub's ground)
 *   F all pn of them            the data members j with (m[o][j] / m[0][j]) S_0
 *                               == S_o over the whole unit for every o >= 1:
 *     exactly one               TFS_EC_LOCATE_DATA, member j; its error is
 *                               (1 / m[0][j]) S_0 and the repaired unit is
 *                               member j's unit XOR that
 *     otherwise                 TFS_EC_LOCATE_NONE: more than one member is
 *                               wrong there
 * result[k], 8 bytes: kind; member (the data member for DATA, else -1); parity
 * (bit p set when S_p != 0); diff_bytes (how many of the unit's 1,024 bytes the
 * repair changes, 0 unless DATA); flags.  TFS_EC_LOCATE_CONFIRMED is set in
 * every result of a coder with pn >= 3 and in none with pn == 2: with exactly
 * two parity members the code's distance is 3, and a unit in which two data
 * members are wrong in the same symbol can look like a third member; with
 * three or more it cannot.  A DATA result without CONFIRMED is a proposal, to
 * be written only when the records over the unit verify afterwards.
 *
 * ec is any coder with an encoding matrix; the locate plan is built by the
 * first call and freed with the coder.  members[i] (dn + pn of them) is the
 * whole member i over [0, size), the data members zero-filled past their
 * block_len as the scrub session takes them.  Entry k is unit units[k] of every
 * member (byte units[k] * 1024); units == NULL: entry k is unit k, a densely
 * gathered buffer.  units is always a host array, may be unsorted and may name
 * a unit twice.  fixed (may be NULL) holds n * 1024 bytes: slot k receives the
 * repaired unit of a DATA entry k; slots of other entries are not written.  No
 * member byte is written.
 * Checks, in this order, nothing launched on any failure: ec NULL ->
 * TFS_EXIT_PARAMETER_ERROR; no encoding matrix -> TFS_EXIT_MATRIX_INVALID;
 * pn < 2 -> TFS_EXIT_PARAMETER_ERROR; size <= 0 or size % 1024 ->
 * TFS_EXIT_SIZE_INVALID; any of the dn + pn members NULL ->
 * TFS_EXIT_DATA_INVALID; some units[k] * 1024 + 1024 > size, or without a list
 * n * 1024 > size -> TFS_EXIT_PARAMETER_ERROR; then n == 0 returns TFS_SUCCESS;
 * result NULL -> TFS_EXIT_PARAMETER_ERROR.  Findings are reported, not
 * returned: a list full of NONE returns TFS_SUCCESS.
 * Device form: members, d_result (n results, 8-byte aligned) and d_fixed
 * (n * 1024 bytes) in device memory of ctx's GPU, d_members a host array of
 * pointers; the list is copied before the call returns and uploaded on
 * `stream`; asynchronous on `stream` (NULL: the context's; hipStreamPerThread
 * is refused with TFS_EXIT_PARAMETER_ERROR).  Host form: host memory,
 * synchronous, on the context's stream: the listed units of every member are
 * gathered into the coder's staging buffers, in pieces when they do not fit in
 * one go, the dense form runs, and results and repaired units come down.  A
 * coder's locate calls are serialised. */
#define TFS_EC_LOCATE_CLEAN 0
#define TFS_EC_LOCATE_PARITY 1
#define TFS_EC_LOCATE_DATA 2
#define TFS_EC_LOCATE_NONE 3
#define TFS_EC_LOCATE_CONFIRMED 1u /* flags bit 0 */
typedef struct tfs_ec_locate_result { /* 8 bytes */
  int8_t kind;         /* TFS_EC_LOCATE_* */
  int8_t member;       /* DATA: the data member, else -1 */
  uint16_t parity;     /* bit p: parity member p disagrees with the data as given */
  uint16_t diff_bytes; /* DATA: bytes of the unit the repair changes */
  uint8_t flags;       /* TFS_EC_LOCATE_CONFIRMED */
  uint8_t reserved;    /* 0 */
} tfs_ec_locate_result;
typedef char tfs_ec_locate_result_is_8_bytes[sizeof(tfs_ec_locate_result) == 8 ? 1 : -1]; /* static assert, C and C++ */

int tfs_ec_locate_device(tfs_ec* ec, const void* const* d_members, int size, const uint32_t* units, uint32_t n,
                         void* d_result, void* d_fixed, void* stream);
int tfs_ec_locate(tfs_ec* ec, const char* const* members, int size, const uint32_t* units, uint32_t n,
                  tfs_ec_locate_result* result, char* fixed);

/* Parity update (beyond the reference): a change made in place to one data
 * member of a family that exists -- an unlink rewrites the record's FileInfo
 * (logic_block.cpp:649-656) -- carried into the stored parity, from the delta of
 * that member alone.  The reference's unlink_file_parity (logic_block.cpp:
 * 539-577) touches the parity block's index only, so after the first unlink
 * the parity is no longer the code of the data: a scrub flags the unit in every
 * parity member, and a reinstate of another member rebuilds wrong bytes there.
 * The code is linear: parity member p changes by B[p][member] (old ^ new), the
 * jerasure bitmatrix product of block (p, member) of the encoding matrix with
 * the delta.  Nothing else is needed -- no other data member, and of the parity
 * only the member(s) the caller holds.
 *
 * ec is any coder with an encoding matrix.  parity is a host array of pn
 * pointers: parity[p] is the whole of parity member p over [0, size), or NULL
 * when the caller does not hold that member (a parity server binds its one).
 * Entry k is slot k of the delta buffers (bytes [k * 1024, k * 1024 + 1024) of a
 * and of b) and unit units[k] of the parity members (byte units[k] * 1024);
 * units == NULL: entry k is unit k.  The delta of entry k is a[k] ^ b[k], the
 * old and the new bytes of data member `member` in that unit, in either order;
 * b == NULL: a is the delta itself.  units is always a host array and may be
 * unsorted, but names no unit twice.
 * Effect: for every bound p and every k, unit units[k] of parity[p] becomes
 * itself XOR tfs_ec_encode's parity p of a family that is zero except for data
 * member `member` = the delta.  When the parity was the code of the data before
 * the change, it is the code of the data after it.  Parity units that are not
 * listed, and members that are not bound, are neither read nor written; a
 * listed unit whose delta is zero may be rewritten with the bytes it had.
 * AN UPDATE IS NOT IDEMPOTENT: applied twice it is undone.  Delivering each
 * delta to each parity member exactly once is the dataserver's job.
 * Checks, in this order, nothing launched and nothing written on any failure:
 * ec NULL -> TFS_EXIT_PARAMETER_ERROR; no encoding matrix ->
 * TFS_EXIT_MATRIX_INVALID; member < 0 or member >= dn ->
 * TFS_EXIT_PARAMETER_ERROR; size <= 0 or size % 1024 -> TFS_EXIT_SIZE_INVALID;
 * parity NULL or every entry NULL -> TFS_EXIT_DATA_INVALID; some units[k] * 1024
 * + 1024 > size, or without a list n * 1024 > size -> TFS_EXIT_PARAMETER_ERROR;
 * a unit named twice -> TFS_EXIT_PARAMETER_ERROR (two waves would race on one
 * read-modify-write); device form: hipStreamPerThread ->
 * TFS_EXIT_PARAMETER_ERROR; then n == 0 returns TFS_SUCCESS; a NULL ->
 * TFS_EXIT_PARAMETER_ERROR.
 * Device form: the parity members, d_a and d_b in device memory of ctx's GPU;
 * asynchronous on `stream` (NULL: the context's).  A list of at most 16 units
 * travels in the launch arguments, a longer one is copied before the call
 * returns and uploaded on `stream`.  Updates of one parity unit take effect in
 * stream order; a coder's update calls are serialised.  d_a and d_b may not
 * overlap a parity member.  Host form: host memory, synchronous, on the
 * context's stream: a, b and the listed units of every bound parity member are
 * staged through the coder's buffers, in pieces when they do not fit in one go,
 * the dense device form runs, and the updated units are scattered back; no
 * other host byte is written. */
int tfs_ec_update_device(tfs_ec* ec, int member, void* const* d_parity, int size, const uint32_t* units, uint32_t n,
                         const void* d_a, const void* d_b, void* stream);
int tfs_ec_update(tfs_ec* ec, int member, char* const* parity, int size, const uint32_t* units, uint32_t n,
                  const char* a, const char* b);

#ifdef __cplusplus
}
#endif
#endif /* TFS_EC_H_ */
