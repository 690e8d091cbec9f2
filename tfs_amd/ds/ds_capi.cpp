// ds_capi.cpp -- C entry points over the dataserver-shaped harness, so tests
// can drive the write / close / verify / compact call sites the way the
// reference's gtest programs drive LogicBlock/DataFile directly
// (tests/dataserver/test_logic_block_and_compact.cpp).  Host C++ only.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ds_harness.h"
#include "ec_fetch.h"
#include "ec_frames.h"
#include "file_repair.h"
#include "mirror_sync.h"
#include "packet_codec.h"
#include "receive.h"
#include "replicate.h"

using namespace tfs::dataserver;

extern "C" {

void* tfs_ds_datafile_new(tfs_crc_ctx* ctx, uint64_t fn, const char* tmp_dir) {
  return new DataFile(fn, tmp_dir ? tmp_dir : "/tmp", ctx);
}
// The same with its buffer from a LeaseBufferPool (tfs_ds_lease_pool_new; the heap
// when the pool is exhausted or NULL).
void* tfs_ds_datafile_new2(tfs_crc_ctx* ctx, uint64_t fn, const char* tmp_dir, void* pool) {
  return new DataFile(fn, tmp_dir ? tmp_dir : "/tmp", ctx, static_cast<LeaseBufferPool*>(pool));
}
int tfs_ds_datafile_pooled(void* df) { return static_cast<DataFile*>(df)->pool() != nullptr; }
void tfs_ds_datafile_free(void* df) { delete static_cast<DataFile*>(df); }
int tfs_ds_datafile_set_data(void* df, const char* data, int32_t len, int32_t offset) {
  return static_cast<DataFile*>(df)->set_data(data, len, offset);
}
// A fragment whose file CRC came with its packet check (include/tfs_write.h).
int tfs_ds_datafile_set_data_crc(void* df, const char* data, int32_t len, int32_t offset, uint32_t frag_crc) {
  return static_cast<DataFile*>(df)->set_data(data, len, offset, frag_crc);
}
int32_t tfs_ds_datafile_length(void* df) { return static_cast<DataFile*>(df)->get_length(); }
uint32_t tfs_ds_datafile_get_crc(void* df, int* status) {
  DataFile* d = static_cast<DataFile*>(df);
  const uint32_t c = d->get_crc();
  if (status) *status = d->last_status();
  return c;
}

void* tfs_ds_block_new(uint32_t block_id, int64_t capacity) { return new LogicBlockImage(block_id, capacity); }
// Page-locked block buffers lent to LogicBlockImages (a dataserver's preallocated blocks).
void* tfs_ds_pool_new(tfs_crc_ctx* ctx, uint32_t count, uint64_t bytes) {
  return new BlockImagePool(ctx, count, size_t(bytes));
}
void tfs_ds_pool_free(void* pool) { delete static_cast<BlockImagePool*>(pool); }
uint32_t tfs_ds_pool_in_use(void* pool) { return uint32_t(static_cast<BlockImagePool*>(pool)->in_use()); }
uint32_t tfs_ds_pool_size(void* pool) { return uint32_t(static_cast<BlockImagePool*>(pool)->size()); }
void* tfs_ds_block_new_in(void* pool, uint32_t block_id, int64_t capacity) {
  return new LogicBlockImage(block_id, capacity, pool ? static_cast<BlockImagePool*>(pool)->take() : nullptr);
}
void tfs_ds_block_free(void* b) { delete static_cast<LogicBlockImage*>(b); }
int64_t tfs_ds_block_size(void* b) { return static_cast<LogicBlockImage*>(b)->data_size(); }
const char* tfs_ds_block_data(void* b) { return static_cast<LogicBlockImage*>(b)->data().data(); }
int tfs_ds_block_set_flag(void* b, uint64_t file_id, int32_t flag) {
  return static_cast<LogicBlockImage*>(b)->set_flag(file_id, flag);
}
int tfs_ds_block_corrupt(void* b, int64_t offset, uint8_t xor_mask) {
  auto& d = static_cast<LogicBlockImage*>(b)->data();
  if (offset < 0 || offset >= int64_t(d.size())) return TFS_EXIT_PARAMETER_ERROR;
  d[size_t(offset)] = char(uint8_t(d[size_t(offset)]) ^ xor_mask);
  return TFS_SUCCESS;
}
int tfs_ds_block_metas(void* b, tfs_raw_meta* out, int32_t* flags, uint32_t cap) {
  const auto m = static_cast<LogicBlockImage*>(b)->sorted_metas();
  const auto f = static_cast<LogicBlockImage*>(b)->sorted_flags();
  for (size_t i = 0; i < m.size() && i < cap; ++i) {
    out[i] = m[i];
    if (flags) flags[i] = f[i];
  }
  return int(m.size());
}

int tfs_ds_close_write_file(void* block, uint64_t file_id, uint32_t client_crc, void* df) {
  CloseFileInfo info;
  info.block_id_ = static_cast<LogicBlockImage*>(block)->block_id();
  info.file_id_ = file_id;
  info.crc_ = client_crc;
  return close_write_file(info, *static_cast<DataFile*>(df), *static_cast<LogicBlockImage*>(block));
}

void* tfs_ds_batcher_new(tfs_crc_ctx* ctx, uint32_t max_batch, int max_wait_us) {
  return new CloseBatcher(ctx, max_batch, max_wait_us);
}
// in_flight: batches in use at once (1..16; the constructor's default is 8).
void* tfs_ds_batcher_new2(tfs_crc_ctx* ctx, uint32_t max_batch, int max_wait_us, int in_flight) {
  return new CloseBatcher(ctx, max_batch, max_wait_us, in_flight);
}
// pool (a tfs_ds_lease_pool_new handle, may be NULL): closes of DataFiles made
// on it are checked where their payload is, with no gather copy.
void* tfs_ds_batcher_new3(tfs_crc_ctx* ctx, uint32_t max_batch, int max_wait_us, int in_flight, void* pool) {
  return new CloseBatcher(ctx, max_batch, max_wait_us, in_flight, static_cast<LeaseBufferPool*>(pool));
}
void* tfs_ds_batcher_pool(void* b) { return static_cast<CloseBatcher*>(b)->pool(); }

// Page-locked DataFile buffers (LeaseBufferPool); NULL when the allocation fails.
void* tfs_ds_lease_pool_new(tfs_crc_ctx* ctx, uint32_t nbuffers) {
  std::unique_ptr<LeaseBufferPool> p(new LeaseBufferPool(ctx, nbuffers));
  return p->ok() ? p.release() : nullptr;
}
void tfs_ds_lease_pool_free(void* p) { delete static_cast<LeaseBufferPool*>(p); }
uint32_t tfs_ds_lease_pool_in_use(void* p) { return static_cast<LeaseBufferPool*>(p)->in_use(); }
void tfs_ds_batcher_free(void* b) { delete static_cast<CloseBatcher*>(b); }
uint64_t tfs_ds_batcher_batches(void* b) { return static_cast<CloseBatcher*>(b)->batches(); }
int tfs_ds_batcher_close(void* batcher, void* block, uint64_t file_id, uint32_t client_crc, void* df) {
  CloseFileInfo info;
  info.block_id_ = static_cast<LogicBlockImage*>(block)->block_id();
  info.file_id_ = file_id;
  info.crc_ = client_crc;
  return static_cast<CloseBatcher*>(batcher)->close(info, *static_cast<DataFile*>(df),
                                                    *static_cast<LogicBlockImage*>(block));
}

void* tfs_ds_checker_new(int max_crc_error_nums) { return new BlockCrcChecker(max_crc_error_nums); }
void tfs_ds_checker_free(void* c) { delete static_cast<BlockCrcChecker*>(c); }
int tfs_ds_checker_errors(void* c, uint32_t block_id) { return static_cast<BlockCrcChecker*>(c)->crc_errors(block_id); }
int tfs_ds_checker_needs_repair(void* c, uint32_t block_id) {
  return static_cast<BlockCrcChecker*>(c)->needs_repair(block_id) ? 1 : 0;
}

// The checker's repair queue: up to cap (block id, file id) pairs in the order they were reported; returns how many
// there are.
uint32_t tfs_ds_checker_repair_queue(void* c, uint32_t* block_ids, uint64_t* file_ids, uint32_t cap) {
  const auto q = static_cast<BlockCrcChecker*>(c)->repair_queue();
  for (size_t i = 0; i < q.size() && i < cap; ++i) {
    if (block_ids) block_ids[i] = q[i].first;
    if (file_ids) file_ids[i] = q[i].second;
  }
  return uint32_t(q.size());
}

int tfs_ds_verify_block(tfs_crc_ctx* ctx, void* block, int32_t* status, uint32_t cap, void* checker) {
  std::vector<int32_t> st;
  const int r = verify_block(ctx, *static_cast<LogicBlockImage*>(block), &st, static_cast<BlockCrcChecker*>(checker));
  for (size_t i = 0; i < st.size() && i < cap; ++i) status[i] = st[i];
  return r;
}

int tfs_ds_recombine_block(tfs_crc_ctx* ctx, void* src, void* dest, int* skipped_crc) {
  return recombine_block(ctx, *static_cast<LogicBlockImage*>(src), *static_cast<LogicBlockImage*>(dest), skipped_crc);
}

// LogicBlock::read_file (logic_block.cpp:374-440) into buf; *nbytes in/out.
int tfs_ds_block_read_file(void* b, uint64_t file_id, char* buf, int32_t* nbytes, int32_t offset, int force) {
  return static_cast<LogicBlockImage*>(b)->read_file(file_id, buf, nbytes, offset, force != 0);
}

// DataManagement::read_data_degrade: the family as arrays of dn + pn block ids, member
// bytes (NULL: lost) and their lengths; *real_read_len in/out, buf holds that many bytes.
static Family make_family(int dn, int pn, const uint32_t* block_ids, const char* const* data, const int64_t* sizes) {
  Family f;
  f.dn = dn;
  f.pn = pn;
  for (int i = 0; i < dn + pn && dn > 0 && pn > 0; ++i)
    f.members.push_back(FamilyMember{block_ids[i], data[i], data[i] ? sizes[i] : 0});
  return f;
}

int tfs_ds_read_data_degrade(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                             const int64_t* sizes, uint32_t block_id, uint64_t file_id, int32_t read_offset, int flag,
                             int32_t* real_read_len, char* buf, const tfs_raw_meta* index, uint32_t n_index) {
  return read_data_degrade(ctx, make_family(dn, pn, block_ids, data, sizes), block_id, file_id, read_offset,
                           int8_t(flag), real_read_len, buf, std::vector<tfs_raw_meta>(index, index + n_index));
}

// The batched form: file i's FileInfo|payload lands at out + out_off[i] (out_len[i] bytes,
// 0 unless status[i] is TFS_SUCCESS), packed in the order of file_ids.
int tfs_ds_read_files_degrade(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                              const int64_t* sizes, uint32_t block_id, const uint64_t* file_ids, uint32_t n, int flag,
                              const tfs_raw_meta* index, uint32_t n_index, char* out, uint64_t out_cap,
                              uint64_t* out_off, int32_t* out_len, int32_t* status) {
  std::vector<std::vector<char>> files;
  std::vector<int32_t> st;
  const int rc = read_files_degrade(ctx, make_family(dn, pn, block_ids, data, sizes), block_id,
                                    std::vector<uint64_t>(file_ids, file_ids + n), int8_t(flag),
                                    std::vector<tfs_raw_meta>(index, index + n_index), &files, &st);
  if (rc < 0) return rc;
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    status[i] = st[i];
    out_off[i] = at;
    out_len[i] = 0;
    if (files[i].empty()) continue;
    if (at + files[i].size() > out_cap) return TFS_EXIT_PARAMETER_ERROR;
    memcpy(out + at, files[i].data(), files[i].size());
    out_len[i] = int32_t(files[i].size());
    at += files[i].size();
  }
  return rc;
}

// MarshallingTask::do_marshalling: data member i's index is indexes[i] (n_index[i] entries); the
// parity members' bytes (data[dn + i], sizes[dn + i] >= *total) are filled; status holds one entry
// per index entry, member 0's first.
int tfs_ds_do_marshalling(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, char* const* data,
                          const int64_t* sizes, const tfs_raw_meta* const* indexes, const uint32_t* n_index,
                          int32_t chunk_len, int32_t* total, int32_t* status, uint32_t status_cap) {
  if (dn <= 0 || pn <= 0 || !data || !sizes || !indexes || !n_index || !total) return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  for (int i = 0; i < dn; ++i)
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
  std::vector<std::vector<char>> parity;
  std::vector<int32_t> st;
  const int rc = do_marshalling(ctx, make_family(dn, pn, block_ids, data, sizes), idx, chunk_len, &parity, total, &st);
  if (rc < 0) return rc;
  if (st.size() > status_cap) return TFS_EXIT_PARAMETER_ERROR;
  for (int i = 0; i < pn; ++i) {
    if (!data[dn + i] || sizes[dn + i] < int64_t(*total)) return TFS_EXIT_PARAMETER_ERROR;
    memcpy(data[dn + i], parity[size_t(i)].data(), parity[size_t(i)].size());
  }
  for (size_t i = 0; i < st.size(); ++i) status[i] = st[i];
  return rc;
}

// ReinstateTask::do_reinstate: data member i's index is indexes[i] (n_index[i] entries; a lost
// member's as a parity block keeps it); rebuilt[i] (rebuilt_cap[i] >= *total bytes) receives lost
// member i; status holds one entry per index entry, member 0's first.
int tfs_ds_do_reinstate(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                        const int64_t* sizes, const tfs_raw_meta* const* indexes, const uint32_t* n_index,
                        int32_t chunk_len, char* const* rebuilt, const int64_t* rebuilt_cap, int32_t* total,
                        int32_t* status, uint32_t status_cap) {
  if (dn <= 0 || pn <= 0 || !data || !sizes || !indexes || !n_index || !rebuilt || !rebuilt_cap || !total)
    return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  uint32_t records = 0;
  for (int i = 0; i < dn; ++i) {
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
    records += n_index[i];
  }
  if (records > status_cap) return TFS_EXIT_PARAMETER_ERROR;
  std::vector<int32_t> st;
  const int rc = do_reinstate(ctx, make_family(dn, pn, block_ids, data, sizes), idx, chunk_len,
                              std::vector<char*>(rebuilt, rebuilt + dn + pn),
                              std::vector<int64_t>(rebuilt_cap, rebuilt_cap + dn + pn), total, &st);
  if (rc < 0) return rc;
  for (size_t i = 0; i < st.size(); ++i) status[i] = st[i];
  return rc;
}

// do_marshalling_frames / do_reinstate_frames (ec_frames.h; reinstate != 0: the latter).  The sink appends every
// frame to buf (cap bytes; *len = the bytes needed) and notes its member, index, place in buf and length in
// frame_member / frame_k / frame_off / frame_bytes (frame_cap entries; *n_frames = the frames handed over).
// opt: {frame_len, chunk_len, version}; packet_ids by member index.  status: one entry per index entry.
int tfs_ds_ec_task_frames(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                          const int64_t* sizes, const tfs_raw_meta* const* indexes, const uint32_t* n_index,
                          int reinstate, const int32_t* opt, const uint64_t* packet_ids, char* buf, int64_t cap,
                          int64_t* len, int32_t* frame_member, uint32_t* frame_k, uint64_t* frame_off,
                          uint32_t* frame_bytes, uint32_t frame_cap, uint32_t* n_frames, int32_t* total, int32_t* status,
                          uint32_t status_cap) {
  if (dn <= 0 || pn <= 0 || !block_ids || !data || !sizes || !indexes || !n_index || !opt || !len || !n_frames || !total)
    return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  uint32_t records = 0;
  for (int i = 0; i < dn; ++i) {
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
    records += n_index[i];
  }
  if (records > status_cap) return TFS_EXIT_PARAMETER_ERROR;
  EcFramesOptions o;
  o.frame_len = opt[0], o.chunk_len = opt[1], o.version = int16_t(opt[2]);
  if (packet_ids) o.packet_id.assign(packet_ids, packet_ids + dn + pn);
  int64_t at = 0;
  uint32_t nf = 0;
  const EcFrameSink sink = [&](int member, uint32_t k, const char* frame, uint32_t bytes) {
    if (buf && at + int64_t(bytes) <= cap) memcpy(buf + at, frame, bytes);
    if (nf < frame_cap) {
      if (frame_member) frame_member[nf] = member;
      if (frame_k) frame_k[nf] = k;
      if (frame_off) frame_off[nf] = uint64_t(at);
      if (frame_bytes) frame_bytes[nf] = bytes;
    }
    at += bytes, ++nf;
    return TFS_SUCCESS;
  };
  std::vector<int32_t> st;
  const Family fam = make_family(dn, pn, block_ids, data, sizes);
  const int rc = reinstate ? do_reinstate_frames(ctx, fam, idx, o, sink, total, &st)
                           : do_marshalling_frames(ctx, fam, idx, o, sink, total, &st);
  *len = at, *n_frames = nf;
  if (rc < 0) return rc;
  for (size_t i = 0; i < st.size(); ++i) status[i] = st[i];
  return rc;
}

// do_marshalling_task / do_reinstate_task (ec_fetch.h; reinstate != 0: the latter): tfs_ds_ec_task_frames with a
// fetch callback per (member, frame) in the place of the members' bytes -- data[i] only marks member i present.
// fetch(user, member, k, offset, length, frame, cap, *bytes) returns TFS_SUCCESS or the code the task ends with.
typedef int (*tfs_ds_fetch_fn)(void* user, int member, uint32_t k, int32_t offset, int32_t length, char* frame, uint32_t cap,
                               uint32_t* bytes);
int tfs_ds_ec_task_fetch(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                         const int64_t* sizes, const tfs_raw_meta* const* indexes, const uint32_t* n_index, int reinstate,
                         const int32_t* opt, const uint64_t* packet_ids, tfs_ds_fetch_fn fetch, void* user, char* buf,
                         int64_t cap, int64_t* len, int32_t* frame_member, uint32_t* frame_k, uint64_t* frame_off,
                         uint32_t* frame_bytes, uint32_t frame_cap, uint32_t* n_frames, int32_t* total, int32_t* status,
                         uint32_t status_cap) {
  if (dn <= 0 || pn <= 0 || !block_ids || !data || !sizes || !indexes || !n_index || !opt || !len || !n_frames || !total ||
      !fetch)
    return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  uint32_t records = 0;
  for (int i = 0; i < dn; ++i) {
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
    records += n_index[i];
  }
  if (records > status_cap) return TFS_EXIT_PARAMETER_ERROR;
  EcFramesOptions o;
  o.frame_len = opt[0], o.chunk_len = opt[1], o.version = int16_t(opt[2]);
  if (packet_ids) o.packet_id.assign(packet_ids, packet_ids + dn + pn);
  int64_t at = 0;
  uint32_t nf = 0;
  const EcFrameSink sink = [&](int member, uint32_t k, const char* frame, uint32_t bytes) {
    if (buf && at + int64_t(bytes) <= cap) memcpy(buf + at, frame, bytes);
    if (nf < frame_cap) {
      if (frame_member) frame_member[nf] = member;
      if (frame_k) frame_k[nf] = k;
      if (frame_off) frame_off[nf] = uint64_t(at);
      if (frame_bytes) frame_bytes[nf] = bytes;
    }
    at += bytes, ++nf;
    return TFS_SUCCESS;
  };
  const EcFrameFetch get = [&](int member, uint32_t k, int32_t offset, int32_t length, char* frame, uint32_t fcap,
                               uint32_t* bytes) { return fetch(user, member, k, offset, length, frame, fcap, bytes); };
  std::vector<int32_t> st;
  const Family fam = make_family(dn, pn, block_ids, data, sizes);
  const int rc = reinstate ? do_reinstate_task(ctx, fam, idx, o, get, sink, total, &st)
                           : do_marshalling_task(ctx, fam, idx, o, get, sink, total, &st);
  *len = at, *n_frames = nf;
  if (rc < 0) return rc;
  for (size_t i = 0; i < st.size(); ++i) status[i] = st[i];
  return rc;
}

static void scrub_report_out(const ScrubReport& r, uint32_t* data_units, uint32_t* parity_only_units,
                             uint32_t* unattributed_units, uint8_t* suspect) {
  for (size_t i = 0; data_units && i < r.data_units.size(); ++i) data_units[i] = r.data_units[i];
  for (size_t p = 0; parity_only_units && p < r.parity_only_units.size(); ++p) parity_only_units[p] = r.parity_only_units[p];
  if (unattributed_units) *unattributed_units = r.unattributed_units;
  for (size_t i = 0; suspect && i < r.suspect.size(); ++i) suspect[i] = r.suspect[i];
}

// classify_scrub: status holds one entry per index entry (member 0's first), tile_map pn rows of
// ceil(total / 4096) bytes; data_units[dn], parity_only_units[pn], *unattributed_units and
// suspect[dn + pn] receive the verdict (each may be NULL).  Returns the number of findings.
int tfs_ds_scrub_classify(int dn, int pn, int32_t total, const tfs_raw_meta* const* indexes, const uint32_t* n_index,
                          const int32_t* status, const uint8_t* tile_map, uint32_t* data_units,
                          uint32_t* parity_only_units, uint32_t* unattributed_units, uint8_t* suspect) {
  if (dn <= 0 || pn <= 0 || dn + pn > TFS_EC_MAX_MEMBERS || total <= 0 || total % TFS_EC_UNIT != 0 || !indexes ||
      !n_index || !tile_map)
    return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  size_t records = 0;
  for (int i = 0; i < dn; ++i) {
    if (n_index[i] && !indexes[i]) return TFS_EXIT_PARAMETER_ERROR;
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
    records += n_index[i];
  }
  if (records && !status) return TFS_EXIT_PARAMETER_ERROR;
  const size_t ntiles = size_t((int64_t(total) + 4095) / 4096);
  const ScrubReport r = classify_scrub(dn, pn, total, idx, std::vector<int32_t>(status, status + records),
                                       std::vector<uint8_t>(tile_map, tile_map + size_t(pn) * ntiles));
  scrub_report_out(r, data_units, parity_only_units, unattributed_units, suspect);
  return r.findings();
}

// scrub_family: every member of the family present (data[i] != NULL, parity members of at least *total
// bytes); status holds one entry per index entry, member 0's first; the verdict as tfs_ds_scrub_classify.
int tfs_ds_scrub_family(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                        const int64_t* sizes, const tfs_raw_meta* const* indexes, const uint32_t* n_index,
                        int32_t chunk_len, int32_t* total, int32_t* status, uint32_t status_cap, uint32_t* data_units,
                        uint32_t* parity_only_units, uint32_t* unattributed_units, uint8_t* suspect) {
  if (dn <= 0 || pn <= 0 || !data || !sizes || !indexes || !n_index || !total) return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  uint32_t records = 0;
  for (int i = 0; i < dn; ++i) {
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
    records += n_index[i];
  }
  if (records > status_cap || (records && !status)) return TFS_EXIT_PARAMETER_ERROR;
  ScrubReport r;
  const int rc = scrub_family(ctx, make_family(dn, pn, block_ids, data, sizes), idx, chunk_len, total, &r);
  if (rc < 0) return rc;
  for (size_t i = 0; i < r.status.size(); ++i) status[i] = r.status[i];
  scrub_report_out(r, data_units, parity_only_units, unattributed_units, suspect);
  return rc;
}

// scrub_and_locate: the scrub's outputs as tfs_ds_scrub_family's, with *scrub_findings what that call returns;
// located_units[dn], *unlocated_units and *examined_units as LocateReport's; the patches, ascending (member,
// unit), into patch_member / patch_unit / patch_diff / patch_confirmed [patch_cap] and patch_bytes
// [patch_cap][1024], *n_patches of them (more than patch_cap: TFS_EXIT_PARAMETER_ERROR).  Returns the number of
// units that could not be located, or a negative status.
int tfs_ds_scrub_locate_family(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                               const int64_t* sizes, const tfs_raw_meta* const* indexes, const uint32_t* n_index,
                               int32_t chunk_len, int32_t* total, int32_t* status, uint32_t status_cap,
                               uint32_t* data_units, uint32_t* parity_only_units, uint32_t* unattributed_units,
                               uint8_t* suspect, int32_t* scrub_findings, uint32_t* located_units,
                               uint32_t* unlocated_units, uint32_t* examined_units, uint32_t patch_cap,
                               uint32_t* n_patches, int32_t* patch_member, uint32_t* patch_unit, uint16_t* patch_diff,
                               uint8_t* patch_confirmed, char* patch_bytes) {
  if (dn <= 0 || pn <= 0 || !data || !sizes || !indexes || !n_index || !total || !n_patches)
    return TFS_EXIT_PARAMETER_ERROR;
  if (patch_cap && (!patch_member || !patch_unit || !patch_diff || !patch_confirmed || !patch_bytes))
    return TFS_EXIT_PARAMETER_ERROR;
  std::vector<std::vector<tfs_raw_meta>> idx(static_cast<size_t>(dn));
  uint32_t records = 0;
  for (int i = 0; i < dn; ++i) {
    if (n_index[i]) idx[size_t(i)].assign(indexes[i], indexes[i] + n_index[i]);
    records += n_index[i];
  }
  if (records > status_cap || (records && !status)) return TFS_EXIT_PARAMETER_ERROR;
  ScrubReport r;
  LocateReport l;
  const int rc = scrub_and_locate(ctx, make_family(dn, pn, block_ids, data, sizes), idx, chunk_len, total, &r, &l);
  if (rc < 0) return rc;
  for (size_t i = 0; i < r.status.size(); ++i) status[i] = r.status[i];
  scrub_report_out(r, data_units, parity_only_units, unattributed_units, suspect);
  if (scrub_findings) *scrub_findings = r.findings();
  for (size_t i = 0; located_units && i < l.located_units.size(); ++i) located_units[i] = l.located_units[i];
  if (unlocated_units) *unlocated_units = l.unlocated_units;
  if (examined_units) *examined_units = l.examined_units;
  *n_patches = uint32_t(l.patches.size());
  if (l.patches.size() > patch_cap) return TFS_EXIT_PARAMETER_ERROR;
  for (size_t k = 0; k < l.patches.size(); ++k) {
    const UnitPatch& p = l.patches[k];
    patch_member[k] = p.member;
    patch_unit[k] = p.unit;
    patch_diff[k] = p.diff_bytes;
    patch_confirmed[k] = p.confirmed ? 1 : 0;
    memcpy(patch_bytes + k * TFS_EC_UNIT, p.bytes.data(), TFS_EC_UNIT);
  }
  return rc;
}

// write_member_range: data[member] and the parity members held (data[dn + p], NULL when not held) are written in
// place.  Returns the number of units updated, or a negative status.
int tfs_ds_write_member_range(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, char* const* data,
                              const int64_t* sizes, int member, int64_t offset, const char* bytes, int64_t len) {
  if (dn <= 0 || pn <= 0 || !block_ids || !data || !sizes) return TFS_EXIT_PARAMETER_ERROR;
  return write_member_range(ctx, make_family(dn, pn, block_ids, data, sizes), data, member, offset, bytes, len);
}

// unlink_file_family: index is block block_id's (n_index entries); the block's image and the parity members held
// are written in place.  Returns the number of units updated, or a negative status.
int tfs_ds_unlink_file_family(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, char* const* data,
                              const int64_t* sizes, const tfs_raw_meta* index, uint32_t n_index, uint32_t block_id,
                              uint64_t file_id, int32_t modify_time) {
  if (dn <= 0 || pn <= 0 || !block_ids || !data || !sizes || (n_index && !index)) return TFS_EXIT_PARAMETER_ERROR;
  return unlink_file_family(ctx, make_family(dn, pn, block_ids, data, sizes), data,
                            std::vector<tfs_raw_meta>(index, index + n_index), block_id, file_id, modify_time);
}

// read_data of a whole file + the GPU verify-on-read hook; FileInfo|payload into buf (cap bytes).
int tfs_ds_read_file_verified(tfs_crc_ctx* ctx, void* block, uint64_t file_id, char* buf, int32_t cap, int32_t* len,
                              void* checker) {
  std::vector<char> out;
  const int rc = read_file_verified(ctx, *static_cast<LogicBlockImage*>(block), file_id, &out,
                                    static_cast<BlockCrcChecker*>(checker));
  *len = int32_t(out.size());
  if (buf && !out.empty()) memcpy(buf, out.data(), std::min(out.size(), size_t(cap > 0 ? cap : 0)));
  return rc;
}

// reply_reads (read_reply.h): n requests of one block; the frames go into buf (cap bytes; *len = the bytes
// needed, TFS_EXIT_PARAMETER_ERROR when they do not fit) and one ReadReply per request into replies.
int tfs_ds_reply_reads(tfs_crc_ctx* ctx, void* block, const ReadRequest* requests, uint32_t n, char* buf, int64_t cap,
                       int64_t* len, ReadReply* replies, void* checker) {
  if (!block || (n && (!requests || !replies)) || !len) return TFS_EXIT_PARAMETER_ERROR;
  ReadReplies out;
  const int rc = reply_reads(ctx, *static_cast<LogicBlockImage*>(block),
                             std::vector<ReadRequest>(requests, requests + n), &out,
                             static_cast<BlockCrcChecker*>(checker));
  if (rc < 0) return rc;
  *len = int64_t(out.frames.size());
  if (*len > cap || (*len && !buf)) return TFS_EXIT_PARAMETER_ERROR;
  if (*len) memcpy(buf, out.frames.data(), out.frames.size());
  for (uint32_t i = 0; i < n; ++i) replies[i] = out.replies[i];
  return rc;
}

// reply_reads_degrade (degraded_reply.h): n requests of one lost block of the family (as tfs_ds_read_data_degrade
// takes it) over the block's parity index; frames, *len and replies as tfs_ds_reply_reads.
int tfs_ds_reply_reads_degrade(tfs_crc_ctx* ctx, int dn, int pn, const uint32_t* block_ids, const char* const* data,
                               const int64_t* sizes, uint32_t block_id, const tfs_raw_meta* index, uint32_t n_index,
                               const ReadRequest* requests, uint32_t n, char* buf, int64_t cap, int64_t* len,
                               ReadReply* replies, void* checker) {
  if (!block_ids || !data || !sizes || (n_index && !index) || (n && (!requests || !replies)) || !len)
    return TFS_EXIT_PARAMETER_ERROR;
  ReadReplies out;
  const int rc = reply_reads_degrade(ctx, make_family(dn, pn, block_ids, data, sizes), block_id,
                                     std::vector<tfs_raw_meta>(index, index + n_index),
                                     std::vector<ReadRequest>(requests, requests + n), &out,
                                     static_cast<BlockCrcChecker*>(checker));
  if (rc < 0) return rc;
  *len = int64_t(out.frames.size());
  if (*len > cap || (*len && !buf)) return TFS_EXIT_PARAMETER_ERROR;
  if (*len) memcpy(buf, out.frames.data(), out.frames.size());
  for (uint32_t i = 0; i < n; ++i) replies[i] = out.replies[i];
  return rc;
}

// replicate_block (replicate.h): the sink appends every frame to buf (cap bytes; *len = the bytes needed) and
// notes its index and length in frame_k / frame_bytes (frame_cap entries; *n_frames = the frames sent); the
// commit callback counts in *commits.  status / crc take one entry per checked record (rec_cap; *n_recs).
// opt: {dest_block_id, frame_len, frames_per_call, new_block, version}.
int tfs_ds_replicate_block(tfs_crc_ctx* ctx, void* block, const int32_t* opt, uint64_t packet_id, char* buf, int64_t cap,
                           int64_t* len, uint32_t* frame_k, uint32_t* frame_bytes, uint32_t frame_cap,
                           uint32_t* n_frames, int32_t* status, uint32_t* crc, uint64_t* file_ids, uint32_t rec_cap,
                           uint32_t* n_recs, int32_t* commits, void* checker) {
  if (!block || !opt || !len || !n_frames || !n_recs || !commits) return TFS_EXIT_PARAMETER_ERROR;
  ReplicateOptions o;
  o.dest_block_id = uint32_t(opt[0]), o.frame_len = opt[1], o.frames_per_call = opt[2];
  o.new_block = int16_t(opt[3]), o.version = int16_t(opt[4]);
  o.packet_id = packet_id;
  int64_t at = 0;
  uint32_t nf = 0;
  auto sink = [&](uint32_t k, const char* frame, uint32_t bytes) {
    if (buf && at + int64_t(bytes) <= cap) memcpy(buf + at, frame, bytes);
    if (nf < frame_cap && frame_k && frame_bytes) frame_k[nf] = k, frame_bytes[nf] = bytes;
    at += bytes;
    ++nf;
    return TFS_SUCCESS;
  };
  auto commit = [&](const ReplicateResult&) {
    ++*commits;
    return TFS_SUCCESS;
  };
  ReplicateResult res;
  const int rc = replicate_block(ctx, *static_cast<LogicBlockImage*>(block), o, sink, commit, &res,
                                 static_cast<BlockCrcChecker*>(checker));
  *len = at, *n_frames = nf, *n_recs = uint32_t(res.status.size());
  for (size_t i = 0; i < res.status.size() && i < rec_cap; ++i) {
    if (status) status[i] = res.status[i];
    if (crc) crc[i] = res.crc[i];
    if (file_ids) file_ids[i] = res.metas[i].file_id;
  }
  return rc;
}

// mirror_copy_files (mirror_sync.h): n files of one block, file i = {file_id, file_number, packet_id, ds_first |
// ds_count << 32} with its ds entries in ds.  opt: {dest_block_id, first_len, frame_len, is_server, version}.  The sink
// appends every frame to buf (cap bytes; *len = the bytes needed) and notes its file, its index in the file and its
// length in frame_file / frame_k / frame_bytes (frame_cap entries; *n_frames = the frames sent).  Each close is noted
// in closed_file / closed_crc / closed_at (the frames sent before it; n entries at most; *n_closed).  files_out takes
// {status, n_frames, file_crc, skipped} per file.
int tfs_ds_mirror_copy_files(tfs_crc_ctx* ctx, void* block, const int32_t* opt, const uint64_t* files, uint32_t n,
                             const uint64_t* ds, uint32_t ds_n, char* buf, int64_t cap, int64_t* len,
                             uint32_t* frame_file, uint32_t* frame_k, uint32_t* frame_bytes, uint32_t frame_cap,
                             uint32_t* n_frames, uint32_t* closed_file, uint32_t* closed_crc, uint32_t* closed_at,
                             uint32_t* n_closed, MirrorFileResult* files_out, void* checker) {
  if (!block || !opt || (n && (!files || !files_out)) || (ds_n && !ds) || !len || !n_frames || !n_closed)
    return TFS_EXIT_PARAMETER_ERROR;
  MirrorOptions o;
  o.dest_block_id = uint32_t(opt[0]), o.first_len = opt[1], o.frame_len = opt[2], o.is_server = opt[3];
  o.version = int16_t(opt[4]);
  std::vector<MirrorFile> fs(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t* f = files + 4u * size_t(i);
    const uint64_t first = f[3] & 0xffffffffu, count = f[3] >> 32;
    if (first + count > ds_n) return TFS_EXIT_PARAMETER_ERROR;
    fs[i].file_id = f[0], fs[i].file_number = f[1], fs[i].packet_id = f[2];
    fs[i].ds.assign(ds + first, ds + first + count);
  }
  int64_t at = 0;
  uint32_t nf = 0, nc = 0;
  auto sink = [&](size_t file, uint32_t k, const char* frame, uint32_t bytes) {
    if (buf && at + int64_t(bytes) <= cap) memcpy(buf + at, frame, bytes);
    if (nf < frame_cap && frame_file && frame_k && frame_bytes)
      frame_file[nf] = uint32_t(file), frame_k[nf] = k, frame_bytes[nf] = bytes;
    at += bytes;
    ++nf;
    return TFS_SUCCESS;
  };
  auto close = [&](size_t file, uint32_t crc) {
    if (nc < n && closed_file && closed_crc && closed_at) closed_file[nc] = uint32_t(file), closed_crc[nc] = crc, closed_at[nc] = nf;
    ++nc;
    return TFS_SUCCESS;
  };
  MirrorResult res;
  const int rc = mirror_copy_files(ctx, *static_cast<LogicBlockImage*>(block), fs, o, sink, close, &res,
                                   static_cast<BlockCrcChecker*>(checker));
  *len = at, *n_frames = nf, *n_closed = nc;
  for (size_t i = 0; i < res.files.size() && i < n; ++i) files_out[i] = res.files[i];
  return rc;
}

// repair_files (file_repair.h): n entries, entry i = {block_id | check_crc << 32, file_id, stat_size, stat_crc |
// pcode << 32, frame_first | frame_count << 32, file_number, packet_id, ds_first | ds_count << 32}; its reply frames
// are frames[2 * k] = offset and frames[2 * k + 1] = bytes in recv (recv_len bytes), its ds entries in ds.  opt:
// {frame_len, is_server, version}.  The sink, the closes and the outputs are those of tfs_ds_mirror_copy_files;
// files_out takes {status, n_frames, file_crc, bad_in, flags, skipped} per entry.
int tfs_ds_repair_files(tfs_crc_ctx* ctx, const int32_t* opt, const char* recv, uint64_t recv_len,
                        const uint64_t* entries, uint32_t n, const uint64_t* frames, uint32_t frames_n,
                        const uint64_t* ds, uint32_t ds_n, char* buf, int64_t cap, int64_t* len, uint32_t* frame_file,
                        uint32_t* frame_k, uint32_t* frame_bytes, uint32_t frame_cap, uint32_t* n_frames,
                        uint32_t* closed_file, uint32_t* closed_crc, uint32_t* closed_at, uint32_t* n_closed,
                        RepairFileResult* files_out, void* checker) {
  if (!opt || (n && (!entries || !files_out)) || (frames_n && !frames) || (ds_n && !ds) || !len || !n_frames ||
      !n_closed)
    return TFS_EXIT_PARAMETER_ERROR;
  RepairOptions o;
  o.recv = recv, o.recv_len = recv_len;
  o.frame_len = opt[0], o.is_server = opt[1], o.version = int16_t(opt[2]);
  std::vector<RepairEntry> es(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t* e = entries + 8u * size_t(i);
    const uint64_t f0 = e[4] & 0xffffffffu, fc = e[4] >> 32, d0 = e[7] & 0xffffffffu, dc = e[7] >> 32;
    if (f0 + fc > frames_n || d0 + dc > ds_n) return TFS_EXIT_PARAMETER_ERROR;
    es[i].block_id = uint32_t(e[0]), es[i].check_crc = uint32_t(e[0] >> 32);
    es[i].file_id = e[1], es[i].stat_size = int64_t(e[2]);
    es[i].stat_crc = uint32_t(e[3]), es[i].pcode = int32_t(e[3] >> 32);
    for (uint64_t k = f0; k < f0 + fc; ++k) {
      RepairFrame f;
      f.off = frames[2 * k], f.avail = uint32_t(std::min<uint64_t>(frames[2 * k + 1], UINT32_MAX));
      es[i].frames.push_back(f);
    }
    es[i].file_number = e[5], es[i].packet_id = e[6];
    es[i].ds.assign(ds + d0, ds + d0 + dc);
  }
  int64_t at = 0;
  uint32_t nf = 0, nc = 0;
  auto sink = [&](size_t file, uint32_t k, const char* frame, uint32_t bytes) {
    if (buf && at + int64_t(bytes) <= cap) memcpy(buf + at, frame, bytes);
    if (nf < frame_cap && frame_file && frame_k && frame_bytes)
      frame_file[nf] = uint32_t(file), frame_k[nf] = k, frame_bytes[nf] = bytes;
    at += bytes;
    ++nf;
    return TFS_SUCCESS;
  };
  auto close = [&](size_t file, uint32_t crc) {
    if (nc < n && closed_file && closed_crc && closed_at) closed_file[nc] = uint32_t(file), closed_crc[nc] = crc, closed_at[nc] = nf;
    ++nc;
    return TFS_SUCCESS;
  };
  RepairResult res;
  const int rc = repair_files(ctx, es, o, sink, close, &res, static_cast<const BlockCrcChecker*>(checker));
  *len = at, *n_frames = nf, *n_closed = nc;
  for (size_t i = 0; i < res.files.size() && i < n; ++i) files_out[i] = res.files[i];
  return rc;
}

// receive_block (receive.h): the frames lie in buf at frame_offs, in order; read r of n_reads holds the next
// read_frames[r] of them (each read hands the whole of buf with its own frames).  parts takes one entry per frame
// landed (parts_cap; *n_parts), status / crc one per meta.  The commit callback hands the landed bytes and the metas
// to `block` (LogicBlockImage::replace) and counts in *commits; out = {total, new_block}.
int tfs_ds_receive_block(tfs_crc_ctx* ctx, void* block, uint32_t block_id, int32_t image_cap, const char* buf,
                         int64_t len, const uint64_t* frame_offs, const uint32_t* read_frames, uint32_t n_reads,
                         const tfs_raw_meta* metas, uint32_t n_metas, tfs_receive_part* parts, uint32_t parts_cap,
                         uint32_t* n_parts, int32_t* status, uint32_t* crc, int32_t* commits, int32_t* out,
                         void* checker) {
  if (!block || len < 0 || (n_reads && (!frame_offs || !read_frames)) || (n_metas && !metas) || !n_parts || !commits)
    return TFS_EXIT_PARAMETER_ERROR;
  ReceiveOptions o;
  o.block_id = block_id, o.image_cap = image_cap;
  o.metas.assign(metas, metas + n_metas);
  uint32_t r = 0;
  size_t at = 0;
  auto source = [&](ReceiveRead* rd) {
    if (r >= n_reads) return false;
    rd->buf = buf, rd->len = uint64_t(len);
    rd->frame_offs.assign(frame_offs + at, frame_offs + at + read_frames[r]);
    at += read_frames[r++];
    return true;
  };
  LogicBlockImage* dest = static_cast<LogicBlockImage*>(block);
  auto commit = [&](ReceiveResult& res) {
    ++*commits;
    dest->replace(std::move(res.image), o.metas, std::vector<int32_t>());
    return TFS_SUCCESS;
  };
  ReceiveResult res;
  const int rc = receive_block(ctx, o, source, commit, &res, static_cast<BlockCrcChecker*>(checker));
  *n_parts = uint32_t(res.parts.size());
  for (size_t i = 0; i < res.parts.size() && i < parts_cap && parts; ++i) parts[i] = res.parts[i];
  for (size_t i = 0; i < res.status.size(); ++i) {
    if (status) status[i] = res.status[i];
    if (crc) crc[i] = res.crc[i];
  }
  if (out) out[0] = res.total, out[1] = res.new_block;
  return rc;
}

int tfs_ds_compact_block(tfs_crc_ctx* ctx, void* src, void* dest, uint8_t* crc_ok, uint32_t cap) {
  std::vector<uint8_t> ok;
  const int r = compact_block(ctx, *static_cast<LogicBlockImage*>(src), *static_cast<LogicBlockImage*>(dest), &ok);
  for (size_t i = 0; i < ok.size() && i < cap; ++i) crc_ok[i] = ok[i];
  return r;
}

// BASELINE.json configs[0] through the dataserver-shaped code: n payloads of
// `len` bytes written into `block` by `nthreads` worker threads (DataService's
// PacketQueueThreads, base_service.cpp:187-192).  Per file: DataFile::set_data
// (the staging memcpy, data_file.cpp:104), then close through the CloseBatcher
// (one GPU verify of every pending lease's client CRC, data_management.cpp:
// 196-198, then FileInfo|payload appended, logic_block.cpp:171-178).  Then
// verify-on-read of the whole block (sync_backup.cpp:383-429).  Returns the
// number of files that failed either check, or a negative status.
int tfs_ds_loopback_block_with(tfs_crc_ctx* ctx, void* batcher, const char* payloads, uint32_t n, int32_t len,
                               const uint32_t* client_crc, int nthreads, void* block);
int tfs_ds_loopback_block(tfs_crc_ctx* ctx, const char* payloads, uint32_t n, int32_t len, const uint32_t* client_crc,
                          int nthreads, void* block) {
  return tfs_ds_loopback_block_with(ctx, nullptr, payloads, n, len, client_crc, nthreads, block);
}

// The same with a long-lived CloseBatcher (DataService creates it once, at
// initialize); NULL = one for this call.
int tfs_ds_loopback_block_with(tfs_crc_ctx* ctx, void* batcher, const char* payloads, uint32_t n, int32_t len,
                               const uint32_t* client_crc, int nthreads, void* block) {
  if (!ctx || !block || len < 0 || (n && (!payloads || !client_crc))) return TFS_EXIT_PARAMETER_ERROR;
  LogicBlockImage& blk = *static_cast<LogicBlockImage*>(block);
  if (nthreads < 1) nthreads = 1;
  blk.reserve(blk.data_size() + int64_t(n) * (int64_t(len) + TFS_FILEINFO_SIZE));
  std::atomic<int> bad{0}, err{0};
  // TFS_DS_TRACE=1: per-phase thread-time totals on stderr (diagnostics only)
  const bool trace = getenv("TFS_DS_TRACE") != nullptr;
  std::atomic<int64_t> t_new{0}, t_set{0}, t_close{0}, t_free{0};
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto us = [](auto a, auto b) { return int64_t(std::chrono::duration_cast<std::chrono::microseconds>(b - a).count()); };
  const auto t_begin = now();
  {
    std::unique_ptr<CloseBatcher> own;
    if (!batcher) own.reset(new CloseBatcher(ctx, CloseBatcher::batch_for(size_t(nthreads)), 100));
    CloseBatcher& bat = batcher ? *static_cast<CloseBatcher*>(batcher) : *own;
    std::vector<std::thread> workers;
    for (int t = 0; t < nthreads; ++t)
      workers.emplace_back([&, t] {
        for (uint32_t i = uint32_t(t); i < n; i += uint32_t(nthreads)) {
          const auto t0 = now();
          std::unique_ptr<DataFile> df(new DataFile(i + 1, "/tmp", ctx, bat.pool()));
          const auto t1 = now();
          if (df->set_data(payloads + size_t(i) * size_t(len), len, 0) < 0) {
            err = TFS_EXIT_PARAMETER_ERROR;
            continue;
          }
          const auto t2 = now();
          CloseFileInfo info;
          info.block_id_ = blk.block_id();
          info.file_id_ = i + 1;
          info.crc_ = client_crc[i];
          const int rc = bat.close(info, *df, blk);
          const auto t3 = now();
          df.reset();
          if (trace) {
            t_new += us(t0, t1);
            t_set += us(t1, t2);
            t_close += us(t2, t3);
            t_free += us(t3, now());
          }
          if (rc == TFS_EXIT_DATA_FILE_ERROR) ++bad;
          else if (rc != TFS_SUCCESS) err = rc;
        }
      });
    for (auto& w : workers) w.join();
  }
  if (err.load() != 0) return err.load();
  const auto t_writes = now();
  const int nb = verify_block(ctx, blk, nullptr, nullptr);
  if (trace)
    fprintf(stderr, "loopback trace: writes %lld us wall, verify %lld us; thread-us new %lld set %lld close %lld free %lld\n",
            (long long)us(t_begin, t_writes), (long long)us(t_writes, now()), (long long)t_new.load(),
            (long long)t_set.load(), (long long)t_close.load(), (long long)t_free.load());
  return nb < 0 ? nb : bad.load() + nb;
}

// The write path with WRITE and CLOSE as separate queued items, as DataService's
// workers see them (dataservice.cpp:1038,1041): n leases of `frags` sealed
// WRITE_DATA frames each (frame k of lease i at frames + frame_off[i * frags + k],
// frame_len bytes) make one queue -- a lease's writes in order, then its close
// `gap` items of other leases later -- that `nthreads` workers pop.  WRITE: the
// frame's packet check (PacketDecoder::decode), then DataFile::set_data at the
// WriteDataInfo's offset_.  CLOSE: CloseBatcher::close, after the lease's writes
// are all in (one may still be in another worker).  mode 0: today's path, the
// file CRC computed at close.  mode 1: the packet check also yields each
// fragment's data CRC (tfs_packet_verify_write), set_data records it and the
// batcher runs with use_fragment_crc.  Then verify-on-read of the whole block.
// lease_status (may be NULL): per lease, the first failing write's status or the
// close's.  close_us (may be NULL): per lease, the close call's microseconds (-1:
// not closed).  Returns the number of files that failed a check, or the first
// status that is neither success nor a CRC verdict.
int tfs_ds_loopback_queue(tfs_crc_ctx* ctx, const char* frames, const uint64_t* frame_off, const uint32_t* frame_len,
                          uint32_t n, uint32_t frags, const uint32_t* client_crc, int nthreads, uint32_t gap, int mode,
                          void* block, int32_t* lease_status, double* close_us) {
  if (!ctx || !block || !frags || (mode != 0 && mode != 1) || (n && (!frames || !frame_off || !frame_len || !client_crc)))
    return TFS_EXIT_PARAMETER_ERROR;
  LogicBlockImage& blk = *static_cast<LogicBlockImage*>(block);
  if (nthreads < 1) nthreads = 1;
  {  // as tfs_ds_loopback_block: the block is sized up front (the frames bound the payloads)
    int64_t bytes = 0;
    for (size_t f = 0; f < size_t(n) * frags; ++f) bytes += frame_len[f];
    blk.reserve(blk.data_size() + bytes + int64_t(n) * TFS_FILEINFO_SIZE);
  }
  struct Item {
    uint32_t lease, frag;  // frag == frags: the lease's close
  };
  std::vector<Item> items;
  items.reserve(size_t(n) * (frags + 1u));
  {
    std::vector<std::pair<uint32_t, size_t>> pending;  // closes waiting: lease, the item count that releases it
    size_t head = 0;
    auto release = [&](bool all) {
      while (head < pending.size() && (all || items.size() >= pending[head].second))
        items.push_back(Item{pending[head++].first, frags});
    };
    for (uint32_t i = 0; i < n; ++i) {
      for (uint32_t k = 0; k < frags; ++k) {
        items.push_back(Item{i, k});
        if (k + 1 < frags) release(false);
      }
      pending.emplace_back(i, items.size() + gap);
      release(false);
    }
    release(true);
  }
  std::vector<std::unique_ptr<DataFile>> files(n);
  for (uint32_t i = 0; i < n; ++i) files[i].reset(new DataFile(i + 1, "/tmp", ctx));
  // A lease's writes may be in several workers at once; DataFile is not thread-safe
  // (neither is the reference's), so a lease's set_data calls take the lease's lock.
  std::unique_ptr<std::mutex[]> lease_mu(new std::mutex[n]);
  std::unique_ptr<std::atomic<uint32_t>[]> ready(new std::atomic<uint32_t>[n]);
  std::unique_ptr<std::atomic<int32_t>[]> wstatus(new std::atomic<int32_t>[n]);
  for (uint32_t i = 0; i < n; ++i) ready[i] = 0, wstatus[i] = TFS_SUCCESS;
  if (close_us)
    for (uint32_t i = 0; i < n; ++i) close_us[i] = -1.0;
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0}, err{0};
  {
    CloseBatcher bat(ctx, CloseBatcher::batch_for(size_t(nthreads)), 100, CloseBatcher::kBatches, nullptr, mode == 1);
    std::vector<std::thread> workers;
    for (int t = 0; t < nthreads; ++t)
      workers.emplace_back([&] {
        tfs::common::PacketDecoder dec(ctx);
        std::vector<tfs::common::PacketDecoder::Frame> fr;
        std::vector<tfs_write_part> parts;
        for (size_t q; (q = next.fetch_add(1)) < items.size();) {
          const Item it = items[q];
          if (it.frag < frags) {  // WRITE
            const size_t f = size_t(it.lease) * frags + it.frag;
            const char* p = frames + frame_off[f];
            const int64_t flen = frame_len[f];
            int64_t used = 0;
            int st = dec.decode(p, flen, &fr, &used, mode == 1 ? &parts : nullptr);
            if (st == TFS_SUCCESS && (fr.size() != 1 || used != flen || flen < TFS_PACKET_HEADER_V1_SIZE + 36))
              st = TFS_ERROR;
            if (st == TFS_SUCCESS) {
              // WriteDataMessage::deserialize (write_data_message.cpp:35-55): offset_
              // at body bytes 12..15, length_ at 16..19, ds_'s count at 32..35
              const char* body = p + TFS_PACKET_HEADER_V1_SIZE;
              int32_t off, dlen, cnt;
              memcpy(&off, body + 12, 4), memcpy(&dlen, body + 16, 4), memcpy(&cnt, body + 32, 4);
              int rc;
              std::lock_guard<std::mutex> lg(lease_mu[it.lease]);
              if (mode == 1 && parts[0].data_len >= 0) {
                rc = files[it.lease]->set_data(body + parts[0].data_off, parts[0].data_len, off, parts[0].data_crc);
              } else if (cnt < 0 || dlen < 0 || 36 + 8 * int64_t(cnt) + dlen > flen - TFS_PACKET_HEADER_V1_SIZE) {
                rc = TFS_ERROR;
              } else {
                rc = files[it.lease]->set_data(body + 36 + 8 * cnt, dlen, off);
              }
              if (rc < 0) st = rc;
            }
            if (st != TFS_SUCCESS) {
              int32_t none = TFS_SUCCESS;
              wstatus[it.lease].compare_exchange_strong(none, st);
            }
            ready[it.lease].fetch_add(1, std::memory_order_release);
            continue;
          }
          // CLOSE: the lease's writes are all popped; wait for the ones still in flight
          while (ready[it.lease].load(std::memory_order_acquire) != frags) std::this_thread::yield();
          int rc = wstatus[it.lease].load();
          if (rc == TFS_SUCCESS) {
            CloseFileInfo info;
            info.block_id_ = blk.block_id();
            info.file_id_ = it.lease + 1;
            info.crc_ = client_crc[it.lease];
            const auto t0 = std::chrono::steady_clock::now();
            rc = bat.close(info, *files[it.lease], blk);
            if (close_us)
              close_us[it.lease] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
          }
          files[it.lease].reset();
          if (lease_status) lease_status[it.lease] = rc;
          if (rc == TFS_EXIT_DATA_FILE_ERROR || rc == TFS_EXIT_CHECK_CRC_ERROR) ++bad;
          else if (rc != TFS_SUCCESS) err = rc;
        }
      });
    for (auto& w : workers) w.join();
  }
  if (err.load() != 0) return err.load();
  const int nb = verify_block(ctx, blk, nullptr, nullptr);
  return nb < 0 ? nb : bad.load() + nb;
}

// ---- write-path latency (SURVEY §7 "Batching vs. latency") ------------------

// Per-close latency of DataManagement::close_write_file through the CloseBatcher:
// `nleases` worker threads (concurrent leases) each close `iters` files of `len`
// bytes; a close is timed from the call to its return (GPU check of the client
// CRC + FileInfo|payload append).  out_us receives nleases*iters microseconds.
// out_phase (may be NULL): kClosePhases doubles per close, in out_us's order --
// CloseTiming's claim, copy, wait, append, lead_wait, verify (us), leader,
// batch_n, relaunches, ring_full.
constexpr int kClosePhases = 10;
int tfs_ds_close_latency_phases(tfs_crc_ctx* ctx, int nleases, int iters, int32_t len, double* out_us,
                                double* out_phase) {
  if (!ctx || nleases < 1 || iters < 1 || len < 0 || !out_us) return TFS_EXIT_PARAMETER_ERROR;
  std::vector<char> payload(size_t(len) + 1);
  for (int32_t i = 0; i < len; ++i) payload[size_t(i)] = char((i * 2654435761u) >> 11);
  uint32_t client = 0;
  int rc = tfs_datafile_get_crc(ctx, payload.data(), len, &client);  // the client's Func::crc
  if (rc != TFS_SUCCESS) return rc;
  LogicBlockImage blk(1, int64_t(INT32_MAX));
  constexpr int kWarm = 8;  // untimed closes per lease first: steady state, not first-use allocations
  const int64_t total = int64_t(nleases) * (iters + kWarm) * (int64_t(len) + TFS_FILEINFO_SIZE);
  if (total > int64_t(INT32_MAX)) return TFS_EXIT_PARAMETER_ERROR;
  blk.reserve(total);
  std::atomic<int> err{0};
  {
    CloseBatcher batcher(ctx, CloseBatcher::batch_for(size_t(nleases)), 100);
    std::vector<std::thread> workers;
    for (int t = 0; t < nleases; ++t)
      workers.emplace_back([&, t] {
        for (int k = -kWarm; k < iters; ++k) {
          const uint64_t fid = uint64_t(t) * uint64_t(iters + kWarm) + uint64_t(k + kWarm) + 1;
          DataFile df(fid, "/tmp", ctx);
          df.set_data(payload.data(), len, 0);
          CloseFileInfo info;
          info.block_id_ = 1;
          info.file_id_ = fid;
          info.crc_ = client;
          CloseTiming ph;
          const auto t0 = std::chrono::steady_clock::now();
          const int r = batcher.close(info, df, blk, out_phase ? &ph : nullptr);
          const auto t1 = std::chrono::steady_clock::now();
          const size_t at = size_t(t) * size_t(iters) + size_t(k);
          if (k >= 0) out_us[at] = std::chrono::duration<double, std::micro>(t1 - t0).count();
          if (k >= 0 && out_phase) {
            double* o = out_phase + at * kClosePhases;
            o[0] = ph.claim_us, o[1] = ph.copy_us, o[2] = ph.wait_us, o[3] = ph.append_us;
            o[4] = ph.lead_wait_us, o[5] = ph.verify_us, o[6] = ph.leader, o[7] = ph.batch_n;
            o[8] = ph.relaunches, o[9] = ph.ring_full;
          }
          if (r != TFS_SUCCESS) err = r;
        }
      });
    for (auto& w : workers) w.join();
  }
  return err.load();
}

int tfs_ds_close_latency(tfs_crc_ctx* ctx, int nleases, int iters, int32_t len, double* out_us) {
  return tfs_ds_close_latency_phases(ctx, nleases, iters, len, out_us, nullptr);
}

// A stream of closes (DataManagement::close_write_file, data_management.cpp:
// 173-236) from `nleases` worker threads through one CloseBatcher, running until
// *stop is set: the dataserver's packet workers closing 64 KiB writes while a
// throughput launch (a compaction on the task thread, dataservice.cpp:2915-2918,
// or a block verify) runs on the same GPU.  Each thread appends to a block of its
// own, replaced when full.  Latencies of up to `cap` closes (in completion order
// per thread, threads interleaved by slot) go to out_us; *count = closes done.
int tfs_ds_close_stream(tfs_crc_ctx* ctx, int nleases, int32_t len, const volatile int* stop, double* out_us,
                        uint64_t cap, uint64_t* count) {
  if (!ctx || nleases < 1 || len < 0 || !stop || !count) return TFS_EXIT_PARAMETER_ERROR;
  std::vector<char> payload(size_t(len) + 1);
  for (int32_t i = 0; i < len; ++i) payload[size_t(i)] = char((i * 2654435761u) >> 13);
  uint32_t client = 0;
  int rc = tfs_datafile_get_crc(ctx, payload.data(), len, &client);
  if (rc != TFS_SUCCESS) return rc;
  constexpr int64_t kBlockBytes = 64ll << 20;
  const int64_t per_block = std::max<int64_t>(1, kBlockBytes / (int64_t(len) + TFS_FILEINFO_SIZE));
  std::atomic<int> err{0};
  std::atomic<uint64_t> done{0};
  {
    CloseBatcher batcher(ctx, CloseBatcher::batch_for(size_t(nleases)), 100);
    std::vector<std::thread> workers;
    for (int t = 0; t < nleases; ++t)
      workers.emplace_back([&, t] {
        std::unique_ptr<LogicBlockImage> blk;
        int64_t in_blk = per_block;
        for (uint64_t k = 0; !*stop && err.load() == TFS_SUCCESS; ++k) {
          if (in_blk == per_block) {
            blk.reset(new LogicBlockImage(uint32_t(t + 1), kBlockBytes));
            blk->reserve(kBlockBytes);
            in_blk = 0;
          }
          ++in_blk;
          const uint64_t fid = k + 1;
          DataFile df(fid, "/tmp", ctx);
          df.set_data(payload.data(), len, 0);
          CloseFileInfo info;
          info.block_id_ = uint32_t(t + 1);
          info.file_id_ = fid;
          info.crc_ = client;
          const auto t0 = std::chrono::steady_clock::now();
          const int r = batcher.close(info, df, *blk);
          const auto t1 = std::chrono::steady_clock::now();
          const uint64_t slot = k * uint64_t(nleases) + uint64_t(t);
          if (out_us && slot < cap) out_us[slot] = std::chrono::duration<double, std::micro>(t1 - t0).count();
          if (r != TFS_SUCCESS) err = r;
          done.fetch_add(1);
        }
      });
    for (auto& w : workers) w.join();
  }
  *count = done.load();
  return err.load();
}

// The scalar drop-in: tfs_crc32(0, data, len) on a pageable buffer, timed per call.
int tfs_ds_scalar_latency(int iters, int32_t len, double* out_us) {
  if (iters < 1 || len < 0 || !out_us) return TFS_EXIT_PARAMETER_ERROR;
  std::vector<char> payload(size_t(len) + 1);
  for (int32_t i = 0; i < len; ++i) payload[size_t(i)] = char((i * 40503u) >> 5);
  int err = TFS_SUCCESS;
  for (int k = 0; k < 8 && err == TFS_SUCCESS; ++k) (void)tfs_crc32_e(0, payload.data(), len, &err);  // untimed
  for (int k = 0; k < iters; ++k) {
    const auto t0 = std::chrono::steady_clock::now();
    (void)tfs_crc32_e(0, payload.data(), len, &err);
    const auto t1 = std::chrono::steady_clock::now();
    out_us[k] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    if (err != TFS_SUCCESS) return err;
  }
  return TFS_SUCCESS;
}

// ---- multi-GPU service (CrcService over a tfs_crc_group) --------------------

void* tfs_ds_service_new(tfs_crc_group* group, uint32_t max_batch, int max_wait_us) {
  return group ? new CrcService(group, max_batch, max_wait_us) : nullptr;
}
void tfs_ds_service_free(void* s) { delete static_cast<CrcService*>(s); }
tfs_crc_ctx* tfs_ds_service_ctx_for_block(void* s, uint32_t block_id) {
  return static_cast<CrcService*>(s)->ctx_for_block(block_id);
}
int tfs_ds_service_close(void* s, void* block, uint64_t file_id, uint32_t client_crc, void* df) {
  CloseFileInfo info;
  info.block_id_ = static_cast<LogicBlockImage*>(block)->block_id();
  info.file_id_ = file_id;
  info.crc_ = client_crc;
  return static_cast<CrcService*>(s)->close_write_file(info, *static_cast<DataFile*>(df),
                                                       *static_cast<LogicBlockImage*>(block));
}
int tfs_ds_service_verify_blocks(void* s, void** blocks, uint32_t n, uint32_t* nbad) {
  std::vector<const LogicBlockImage*> b(n);
  for (uint32_t i = 0; i < n; ++i) b[i] = static_cast<const LogicBlockImage*>(blocks[i]);
  std::vector<uint32_t> nb;
  const int rc = static_cast<CrcService*>(s)->verify_blocks(b, &nb);
  for (uint32_t i = 0; nbad && i < n; ++i) nbad[i] = nb[i];
  return rc;
}

// BASELINE configs[0]'s loop over several blocks on a multi-GPU node: worker
// threads write file k of block b (block ids blocks[b]->block_id()) through a
// DataFile on that block's GPU and close it through the service (routed by
// block id), then every block is verified on its GPU, members concurrently.
// Returns the number of files that failed either check, or a negative status.
int tfs_ds_service_loopback(void* service, const char* payloads, uint32_t nblocks, uint32_t files_per_block,
                            int32_t len, const uint32_t* client_crc, int nthreads, void** blocks) {
  auto* svc = static_cast<CrcService*>(service);
  if (!svc || !blocks || len < 0) return TFS_EXIT_PARAMETER_ERROR;
  if (nthreads < 1) nthreads = 1;
  const uint32_t n = nblocks * files_per_block;
  for (uint32_t b = 0; b < nblocks; ++b) {
    auto* blk = static_cast<LogicBlockImage*>(blocks[b]);
    blk->reserve(blk->data_size() + int64_t(files_per_block) * (int64_t(len) + TFS_FILEINFO_SIZE));
  }
  std::atomic<int> bad{0}, err{0};
  std::vector<std::thread> workers;
  for (int t = 0; t < nthreads; ++t)
    workers.emplace_back([&, t] {
      for (uint32_t i = uint32_t(t); i < n; i += uint32_t(nthreads)) {
        auto* blk = static_cast<LogicBlockImage*>(blocks[i % nblocks]);
        DataFile df(i + 1, "/tmp", svc->ctx_for_block(blk->block_id()));
        if (df.set_data(payloads + size_t(i) * size_t(len), len, 0) < 0) {
          err = TFS_EXIT_PARAMETER_ERROR;
          continue;
        }
        CloseFileInfo info;
        info.block_id_ = blk->block_id();
        info.file_id_ = i + 1;
        info.crc_ = client_crc[i];
        const int rc = svc->close_write_file(info, df, *blk);
        if (rc == TFS_EXIT_DATA_FILE_ERROR) ++bad;
        else if (rc != TFS_SUCCESS) err = rc;
      }
    });
  for (auto& w : workers) w.join();
  if (err.load() != 0) return err.load();
  std::vector<const LogicBlockImage*> all(nblocks);
  for (uint32_t b = 0; b < nblocks; ++b) all[b] = static_cast<const LogicBlockImage*>(blocks[b]);
  std::vector<uint32_t> nb;
  const int rc = svc->verify_blocks(all, &nb);
  if (rc != TFS_SUCCESS && rc != TFS_EXIT_CHECK_CRC_ERROR) return rc;
  int total = bad.load();
  for (uint32_t x : nb) total += int(x);
  return total;
}

}  // extern "C"

// ---- packet codec (packet_codec.h) ----------------------------------------
#include "packet_codec.h"

extern "C" {

void* tfs_ds_encoder_new(tfs_crc_ctx* ctx) { return new tfs::common::PacketEncoder(ctx); }
void tfs_ds_encoder_free(void* e) { delete static_cast<tfs::common::PacketEncoder*>(e); }
void tfs_ds_encoder_add(void* e, int16_t pcode, int16_t version, uint64_t id, const char* body, int32_t len) {
  static_cast<tfs::common::PacketEncoder*>(e)->add(pcode, version, id, body, len);
}
int tfs_ds_encoder_flush(void* e) { return static_cast<tfs::common::PacketEncoder*>(e)->flush(); }
int64_t tfs_ds_encoder_size(void* e) { return int64_t(static_cast<tfs::common::PacketEncoder*>(e)->output().size()); }
const char* tfs_ds_encoder_data(void* e) { return static_cast<tfs::common::PacketEncoder*>(e)->output().data(); }

// Decode a received buffer: per frame offset/status/crc (cap entries), *nframes, *consumed.
int tfs_ds_decode(tfs_crc_ctx* ctx, const char* data, int64_t len, int64_t* offsets, int32_t* status, uint32_t* crc,
                  uint32_t cap, uint32_t* nframes, int64_t* consumed) {
  tfs::common::PacketDecoder dec(ctx);
  std::vector<tfs::common::PacketDecoder::Frame> fr;
  const int rc = dec.decode(data, len, &fr, consumed);
  *nframes = uint32_t(fr.size());
  for (size_t i = 0; i < fr.size() && i < cap; ++i) {
    if (offsets) offsets[i] = fr[i].offset;
    if (status) status[i] = fr[i].status;
    if (crc) crc[i] = fr[i].crc;
  }
  return rc;
}

// The same through tfs_packet_verify_write: parts[i] = frame i's data fragment.
int tfs_ds_decode_write(tfs_crc_ctx* ctx, const char* data, int64_t len, int64_t* offsets, int32_t* status,
                        uint32_t* crc, tfs_write_part* parts, uint32_t cap, uint32_t* nframes, int64_t* consumed) {
  tfs::common::PacketDecoder dec(ctx);
  std::vector<tfs::common::PacketDecoder::Frame> fr;
  std::vector<tfs_write_part> wp;
  const int rc = dec.decode(data, len, &fr, consumed, &wp);
  *nframes = uint32_t(fr.size());
  for (size_t i = 0; i < fr.size() && i < cap; ++i) {
    if (offsets) offsets[i] = fr[i].offset;
    if (status) status[i] = fr[i].status;
    if (crc) crc[i] = fr[i].crc;
    if (parts && i < wp.size()) parts[i] = wp[i];
  }
  return rc;
}

}  // extern "C"

// ---- on-disk blocks (block_store.h) ----------------------------------------
#include "block_store.h"

extern "C" {

static tfs::dataserver::BlockStore make_store(const char* mount, int32_t main_size, int32_t ext_size) {
  tfs::dataserver::BlockStore st;
  st.mount = mount;
  st.main_block_size = main_size;
  st.ext_block_size = ext_size;
  return st;
}

int tfs_ds_block_write_files(void* block, const char* mount, int32_t main_size, int32_t ext_size, uint32_t main_id,
                             uint32_t first_ext_id, int32_t bucket_size, uint32_t* ext_ids, uint32_t cap,
                             uint32_t* n_ext) {
  std::vector<uint32_t> ids;
  const int rc = tfs::dataserver::write_logic_block(make_store(mount, main_size, ext_size), main_id, first_ext_id,
                                                    *static_cast<LogicBlockImage*>(block), bucket_size, &ids);
  if (n_ext) *n_ext = uint32_t(ids.size());
  for (size_t i = 0; ext_ids && i < ids.size() && i < cap; ++i) ext_ids[i] = ids[i];
  return rc;
}

int tfs_ds_block_append(void* b, uint64_t file_id, const char* payload, int32_t len, uint32_t crc) {
  return static_cast<LogicBlockImage*>(b)->append_record(file_id, payload, len, crc);
}

void* tfs_ds_loaded_new(tfs_crc_ctx* ctx) { return new tfs::dataserver::LoadedBlock(ctx); }
void tfs_ds_loaded_free(void* b) { delete static_cast<tfs::dataserver::LoadedBlock*>(b); }
int tfs_ds_loaded_load(void* b, const char* mount, int32_t main_size, int32_t ext_size, uint32_t main_id) {
  return static_cast<tfs::dataserver::LoadedBlock*>(b)->load(make_store(mount, main_size, ext_size), main_id);
}
int64_t tfs_ds_loaded_size(void* b) { return static_cast<tfs::dataserver::LoadedBlock*>(b)->size(); }
const char* tfs_ds_loaded_data(void* b) { return static_cast<tfs::dataserver::LoadedBlock*>(b)->data(); }
uint32_t tfs_ds_loaded_logic_id(void* b) { return static_cast<tfs::dataserver::LoadedBlock*>(b)->logic_block_id; }
// Copy metas/flags (cap entries) and the chain (chain_cap); returns the meta count.
uint32_t tfs_ds_loaded_metas(void* b, tfs_raw_meta* metas, int32_t* flags, uint32_t cap, uint32_t* chain,
                             uint32_t chain_cap, uint32_t* chain_len, void* header48) {
  auto* lb = static_cast<tfs::dataserver::LoadedBlock*>(b);
  for (size_t i = 0; i < lb->metas.size() && i < cap; ++i) {
    if (metas) metas[i] = lb->metas[i];
    if (flags) flags[i] = lb->flags[i];
  }
  if (chain_len) *chain_len = uint32_t(lb->chain.size());
  for (size_t i = 0; chain && i < lb->chain.size() && i < chain_cap; ++i) chain[i] = lb->chain[i];
  if (header48) memcpy(header48, &lb->header, sizeof lb->header);
  return uint32_t(lb->metas.size());
}

namespace {
int export_compact_result(int rc, const tfs::dataserver::CompactFilesResult& r, tfs_raw_meta* dest_metas,
                          int32_t* status, uint32_t cap, uint32_t* ext_ids, uint32_t ext_cap, uint32_t* n_ext,
                          int64_t* counters) {
  for (size_t i = 0; i < r.dest_metas.size() && i < cap; ++i) {
    if (dest_metas) dest_metas[i] = r.dest_metas[i];
    if (status) status[i] = r.status[i];
  }
  if (n_ext) *n_ext = uint32_t(r.ext_ids.size());
  for (size_t i = 0; ext_ids && i < r.ext_ids.size() && i < ext_cap; ++i) ext_ids[i] = r.ext_ids[i];
  if (counters) {
    counters[0] = int64_t(r.dest_metas.size());
    counters[1] = r.dest_size;
    counters[2] = r.windows;
    counters[3] = r.launches;
    counters[4] = r.big_files;
    counters[5] = r.n_bad;
    counters[6] = int64_t(r.dropped.size());
  }
  return rc;
}
}  // namespace

// compact_block_files: the new block's metas / statuses (cap entries), ext ids
// (ext_cap), and counters[7] = {n_live, dest_size, windows, launches, big_files, n_bad, n_dropped}.
int tfs_ds_compact_block_files(tfs_crc_ctx* ctx, const char* src_mount, const char* dst_mount, int32_t main_size,
                               int32_t ext_size, uint32_t src_main_id, uint32_t dst_main_id, uint32_t first_ext_id,
                               int32_t bucket_size, int windows_per_launch, tfs_raw_meta* dest_metas,
                               int32_t* status, uint32_t cap, uint32_t* ext_ids, uint32_t ext_cap, uint32_t* n_ext,
                               int64_t* counters) {
  tfs::dataserver::CompactFilesResult r;
  const int rc = tfs::dataserver::compact_block_files(ctx, make_store(src_mount, main_size, ext_size), src_main_id,
                                                      make_store(dst_mount, main_size, ext_size), dst_main_id,
                                                      first_ext_id, bucket_size, windows_per_launch, &r);
  return export_compact_result(rc, r, dest_metas, status, cap, ext_ids, ext_cap, n_ext, counters);
}

// A BlockFileCompactor kept across blocks (window buffers and streams allocated once).
void* tfs_ds_compactor_new(tfs_crc_ctx* ctx, int windows_per_launch) {
  return ctx ? new tfs::dataserver::BlockFileCompactor(ctx, windows_per_launch) : nullptr;
}
void tfs_ds_compactor_free(void* h) { delete static_cast<tfs::dataserver::BlockFileCompactor*>(h); }
int tfs_ds_compactor_compact(void* h, const char* src_mount, const char* dst_mount, int32_t main_size,
                             int32_t ext_size, uint32_t src_main_id, uint32_t dst_main_id, uint32_t first_ext_id,
                             int32_t bucket_size, tfs_raw_meta* dest_metas, int32_t* status, uint32_t cap,
                             uint32_t* ext_ids, uint32_t ext_cap, uint32_t* n_ext, int64_t* counters) {
  if (!h) return TFS_EXIT_PARAMETER_ERROR;
  tfs::dataserver::CompactFilesResult r;
  const int rc = static_cast<tfs::dataserver::BlockFileCompactor*>(h)->compact(
      make_store(src_mount, main_size, ext_size), src_main_id, make_store(dst_mount, main_size, ext_size), dst_main_id,
      first_ext_id, bucket_size, &r);
  return export_compact_result(rc, r, dest_metas, status, cap, ext_ids, ext_cap, n_ext, counters);
}

int tfs_ds_verify_block_files(tfs_crc_ctx* ctx, const char* mount, int32_t main_size, int32_t ext_size,
                              uint32_t main_id, int32_t* status, uint32_t cap, uint32_t* n_live, void* checker) {
  std::vector<int32_t> st;
  const int rc = tfs::dataserver::verify_block_files(ctx, make_store(mount, main_size, ext_size), main_id, &st,
                                                     static_cast<BlockCrcChecker*>(checker));
  if (n_live) *n_live = uint32_t(st.size());
  for (size_t i = 0; status && i < st.size() && i < cap; ++i) status[i] = st[i];
  return rc;
}

}  // extern "C"
