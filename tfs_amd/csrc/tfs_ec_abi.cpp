// tfs_ec_abi.cpp -- host side of include/tfs_ec.h: ErasureCode's setup on the
// host (ec_math.h), the region work on the GPU (tfs_ec_kernels.hip).  No CPU
// fallback: without a device every call fails with the ctx's error.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/tfs_ec.h"
#include "../../include/tfs_ec_fetch.h"
#include "../../include/tfs_ec_frames.h"
#include "../../include/tfs_ec_read.h"
#include "crc_math.h"
#include "ec_math.h"

#include "ec_fetch_plan.h"
#include "ec_frames_plan.h"
#include "ec_locate_plan.h"
#include "ec_marshal_plan.h"
#include "ec_read_plan.h"
#include "ec_reply_plan.h"
#include "pin_registry.h"
#include "tfs_ec_device.h"

extern "C" int tfs_crc32_dev_malloc(tfs_crc_ctx* ctx, uint64_t bytes, void** d_ptr);
extern "C" int tfs_crc32_dev_free(tfs_crc_ctx* ctx, void* d_ptr);
extern "C" void* tfs_crc32_stream(tfs_crc_ctx* ctx);

using namespace tfsec;

namespace {
// One launch plan: sources, outputs, expanded masks [O][8][S][8] (device).
struct Plan {
  std::vector<int> sources, outputs;
  uint32_t* d_masks = nullptr;
  bool valid = false;
};
}  // namespace

struct tfs_ec {
  tfs_crc_ctx* ctx = nullptr;
  int dn = 0, pn = 0;
  Plan enc, dec;
  int config_rc = TFS_SUCCESS;
  std::mutex mu;
  std::vector<void*> staging;  // host-form device buffers, one per member (sized at config), grown on demand
  std::vector<uint64_t> staging_cap;
  int variant = 0;  // kernel form (TFS_EC_VARIANT at creation, measurement knob; 0 = product)
  tfsec::ReadTables* d_read_tab = nullptr;  // degraded read: set with the decode plan
  void* read_buf = nullptr;                 // host form: compact output, jobs and results
  uint64_t read_cap = 0;
  uint64_t read_up = 0, read_down = 0;      // member / output bytes the last host-form read moved
  tfsec::MarshalTables* d_marshal_tab = nullptr;  // marshalling / reinstate sessions: set by the first begin
  std::vector<int> erased;                        // config's erased[] (empty: encode only)
  // scrub locate: the plan, built by the first call, and the buffers of the list and the host form
  uint32_t* d_locate = nullptr;   // ratio words | inv0 words
  size_t locate_ratio_words = 0;
  int locate_rc = TFS_SUCCESS;    // a plan that was refused stays refused
  void* loc_list = nullptr;       // device: the list of the latest device-form call
  uint64_t loc_list_cap = 0;
  uint32_t* loc_pin = nullptr;    // page-locked: the list on its way up
  uint64_t loc_pin_cap = 0;
  hipEvent_t loc_copied = nullptr, loc_done = nullptr;  // the latest list's upload / the latest kernel
  hipStream_t loc_stream = nullptr;
  bool loc_busy = false;
  void* loc_out = nullptr;        // host form: results | repaired units of one piece
  uint64_t loc_out_cap = 0;
  uint32_t loc_piece = 4096;      // host form: units per piece (4 MiB of every member)
  // parity update: a list past kUpdateInline units goes up through the locate list's buffers
  void* upd_buf = nullptr;        // host form: the delta buffers a | b of one piece
  uint64_t upd_buf_cap = 0;
  uint32_t upd_piece = 4096;      // host form: units per piece
  // degraded read reply: the plans of the latest launches, each in page-locked memory with its
  // device copy, and the host form's staged frames and results
  struct ReplySlot {
    void* h = nullptr;   // page-locked: the units on their way up
    void* d = nullptr;
    uint64_t cap = 0;
    hipEvent_t done = nullptr;  // behind the launch that read d
    std::mutex mu;              // one call at a time fills and launches from the slot
  };
  ReplySlot reply_slots[4];
  uint32_t reply_next = 0;
  std::mutex reply_mu;            // deals the slots out: device-form calls come from any thread
  void* reply_out = nullptr;      // host form, device: frames as placed by the plan | results
  uint64_t reply_out_cap = 0;
  void* reply_host = nullptr;     // host form, page-locked: the same on their way down
  uint64_t reply_host_cap = 0;
};

// One marshalling session, and the base of every session: the
// plan and the partial results in one device allocation, and how far the chunks
// have come.
struct tfs_ec_marshal {
  tfs_ec* ec = nullptr;
  std::vector<int> up, down;  // the members a chunk call binds: read by the pass / written by it (host form: staged up / down)
  tfsec::MarshalPlan plan;
  int total = 0, next = 0;   // [0, next) has been encoded
  void* d_buf = nullptr;     // recs | first | rec_member | pow_tile | cont | tail | hdr | crc | status
  tfsec::MarshalRec* d_recs = nullptr;
  uint32_t *d_first = nullptr, *d_member = nullptr, *d_pow = nullptr, *d_cont = nullptr, *d_tail = nullptr,
           *d_hdr = nullptr, *d_crc = nullptr;
  int32_t* d_status = nullptr;
  hipStream_t stream = nullptr;
  bool stream_set = false;
  uint32_t* d_tile_crc = nullptr;  // frame calls: [outputs][ntiles] words, made by the first one
  // task calls: the data members' block_len as begin got them, and, made by the first task
  // call in one allocation, the sources' tile words [sources][ntiles] and the host form's results behind them
  std::vector<int> sizes;
  uint32_t* d_src_crc = nullptr;
  tfs_ec_fetch_result* d_task_res = nullptr;
};

// One reinstate session: a marshalling session's plan, partial
// results and chunk bookkeeping, run over the coder's decode plan.
struct tfs_ec_reinstate : tfs_ec_marshal {};

// One scrub session: a marshalling session's plan, partial results
// and chunk bookkeeping over the encode plan, and the compare's words behind them.
struct tfs_ec_scrub : tfs_ec_marshal {
  uint32_t* d_units = nullptr;  // behind the session's statuses: units [pn] words | map [pn][ntiles] bytes | pbad
  uint8_t* d_map = nullptr;
  uint32_t* d_pbad = nullptr;   // [pn][ntiles] words
};

namespace {

int upload_plan(tfs_ec* ec, Plan* p, const std::vector<int>& sources, const std::vector<int>& outputs,
                const BitMat& rows) {
  const int S = int(sources.size()), O = int(outputs.size());
  const int cols = S * kW;
  std::vector<uint32_t> m(size_t(O) * 8 * S * 8);
  for (int o = 0; o < O; ++o)
    for (int r = 0; r < 8; ++r)
      for (int s = 0; s < S; ++s)
        for (int c = 0; c < 8; ++c)
          m[((size_t(o) * 8 + r) * S + s) * 8 + c] = rows[size_t(o * kW + r) * cols + s * kW + c] ? 0xFFFFFFFFu : 0u;
  void* d = nullptr;
  int rc = tfs_crc32_dev_malloc(ec->ctx, m.size() * 4 + 4, &d);
  if (rc) return rc;
  if (hipMemcpy(d, m.data(), m.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    tfs_crc32_dev_free(ec->ctx, d);
    return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  p->sources = sources;
  p->outputs = outputs;
  p->d_masks = static_cast<uint32_t*>(d);
  p->valid = true;
  return TFS_SUCCESS;
}

// Checks of ErasureCode::encode/decode (erasure_code.cpp:145-172, 181-201).
int check_call(tfs_ec* ec, const Plan& p, void* const* members, const int* sizes, int size) {
  if (!p.valid) return TFS_EXIT_MATRIX_INVALID;
  if (size < 0 || size % kUnit != 0) return TFS_EXIT_SIZE_INVALID;
  if (!members) return TFS_EXIT_DATA_INVALID;
  for (int i = 0; i < ec->dn + ec->pn; ++i)
    if (!members[i] || (sizes && sizes[i] < size)) return TFS_EXIT_DATA_INVALID;
  return TFS_SUCCESS;
}

// The members, masks and length of one launch: outputs [o0, o0 + og) of the plan over `len` bytes.
void fill_ec_args(EcArgs& a, const Plan& p, void* const* members, size_t o0, int og, int len) {
  const size_t S = p.sources.size();
  for (size_t s = 0; s < S; ++s) a.src[s] = static_cast<const uint8_t*>(members[p.sources[s]]);
  for (int o = 0; o < og; ++o) a.dst[o] = static_cast<uint8_t*>(members[p.outputs[o0 + o]]);
  a.masks = p.d_masks + o0 * 8 * S * 8;
  a.S = uint32_t(S);
  a.units = uint64_t(len) / kUnit;
}

int run_plan(tfs_ec* ec, const Plan& p, void* const* members, int size, hipStream_t st) {
  if (uint64_t(size) / kUnit == 0) return TFS_SUCCESS;
  for (size_t o0 = 0; o0 < p.outputs.size(); o0 += kMaxOutGroup) {
    const int og = int(std::min<size_t>(kMaxOutGroup, p.outputs.size() - o0));
    EcArgs a;
    memset(&a, 0, sizeof a);
    fill_ec_args(a, p, members, o0, og, size);
    if (launch_ec_apply(a, og, ec->variant, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return TFS_SUCCESS;
}

// A device buffer of the coder that holds at least `bytes`, kept while it is large enough.
int grow(tfs_ec* ec, void** buf, uint64_t* cap, uint64_t bytes) {
  if (*cap >= bytes && *buf) return TFS_SUCCESS;
  if (*buf) tfs_crc32_dev_free(ec->ctx, *buf);
  *buf = nullptr;
  *cap = 0;
  const int r = tfs_crc32_dev_malloc(ec->ctx, bytes + 64, buf);
  if (r) return r;
  *cap = bytes;
  return TFS_SUCCESS;
}

// Host form: members staged through device buffers; sources up, outputs down.
int run_host(tfs_ec* ec, const Plan& p, char* const* members, const int* sizes, int size) {
  std::lock_guard<std::mutex> g(ec->mu);
  void* const* mv = reinterpret_cast<void* const*>(members);
  int rc = check_call(ec, p, mv, sizes, size);
  if (rc) return rc;
  const int n = ec->dn + ec->pn;
  hipStream_t st = static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  std::vector<void*> dm(n, nullptr);
  for (int s : p.sources) {
    if ((rc = grow(ec, &ec->staging[s], &ec->staging_cap[s], uint64_t(size)))) return rc;
    dm[s] = ec->staging[s];
    if (hipMemcpyAsync(dm[s], members[s], size_t(size), hipMemcpyHostToDevice, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  for (int o : p.outputs) {
    if ((rc = grow(ec, &ec->staging[o], &ec->staging_cap[o], uint64_t(size)))) return rc;
    dm[o] = ec->staging[o];
  }
  for (int i = 0; i < n; ++i)
    if (!dm[i]) dm[i] = ec->staging[p.sources[0]];  // members the plan does not touch
  rc = run_plan(ec, p, dm.data(), size, st);
  if (rc) return rc;
  for (int o : p.outputs)
    if (hipMemcpyAsync(members[o], dm[o], size_t(size), hipMemcpyDeviceToHost, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
  return hipStreamSynchronize(st) == hipSuccess ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
}

// ---- degraded read ----------------------------------------

// The read kernel's constant tables, built once per process (crc_math.h).
const ReadTables& read_tables() {
  static const ReadTables* t = [] {
    ReadTables* r = new ReadTables();
    tfscrc::make_slice_tables(r->slice, 4);
    tfscrc::make_shift_table(r->step_packet, kReadStepPacket);
    tfscrc::make_shift_table(r->step_tile, kReadStepTile);
    // x has an order dividing 2^32 - 1 mod P, so x^(-8) = x^(2^32 - 1 - 8)
    const uint32_t g = tfscrc::x2nmodp(8, 0), gi = tfscrc::x2nmodp(0xFFFFFFFFull - 8, 0);
    r->xpow[kReadPowBias] = 1u << 31;  // x^0
    for (int i = kReadPowBias + 1; i < kReadPowN; ++i) r->xpow[i] = tfscrc::multmodp(g, r->xpow[i - 1]);
    for (int i = kReadPowBias - 1; i >= 0; --i) r->xpow[i] = tfscrc::multmodp(gi, r->xpow[i + 1]);
    return r;
  }();
  return *t;
}

int upload_read_tables(tfs_ec* ec) {
  void* d = nullptr;
  const int rc = tfs_crc32_dev_malloc(ec->ctx, sizeof(ReadTables), &d);
  if (rc) return rc;
  if (hipMemcpy(d, &read_tables(), sizeof(ReadTables), hipMemcpyHostToDevice) != hipSuccess) {
    tfs_crc32_dev_free(ec->ctx, d);
    return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  ec->d_read_tab = static_cast<ReadTables*>(d);
  return TFS_SUCCESS;
}

// Call-level checks of the degraded read, in the header's order.  *row receives
// the target's position among the decode plan's outputs.
int check_read(tfs_ec* ec, void* const* members, const int* sizes, int size, int target, int* row) {
  const Plan& p = ec->dec;
  if (!p.valid || !ec->d_read_tab) return TFS_EXIT_MATRIX_INVALID;
  if (size < 0 || size % kUnit != 0) return TFS_EXIT_SIZE_INVALID;
  if (target < 0 || target >= ec->dn) return TFS_EXIT_PARAMETER_ERROR;
  *row = -1;
  for (size_t o = 0; o < p.outputs.size(); ++o)
    if (p.outputs[o] == target) *row = int(o);
  if (*row < 0) return TFS_EXIT_PARAMETER_ERROR;  // the target is alive
  if (!members) return TFS_EXIT_DATA_INVALID;
  for (int s : p.sources)
    if (!members[s] || (sizes && sizes[s] < size)) return TFS_EXIT_DATA_INVALID;
  return TFS_SUCCESS;
}

int launch_read(tfs_ec* ec, void* const* members, int size, int row, const void* d_jobs, uint32_t n, void* d_out,
                uint64_t out_cap, uint32_t* d_out_crc, int32_t* d_out_status, uint32_t* d_n_bad, hipStream_t st) {
  const Plan& p = ec->dec;
  const int S = int(p.sources.size());
  ReadArgs a;
  memset(&a, 0, sizeof a);
  for (int s = 0; s < S; ++s) a.src[s] = static_cast<const uint8_t*>(members[p.sources[s]]);
  a.masks = p.d_masks + size_t(row) * 8 * size_t(S) * 8;
  a.tab = ec->d_read_tab;
  a.jobs = static_cast<const ReadJob*>(d_jobs);
  a.out = static_cast<uint8_t*>(d_out);
  a.out_cap = out_cap;
  a.out_crc = d_out_crc;
  a.out_status = d_out_status;
  a.n_bad = d_n_bad;
  a.n = n;
  a.S = uint32_t(S);
  a.size = size;
  return launch_ec_read(a, st) == hipSuccess ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
}

// ---- degraded read reply -----------------------------------

// Make the n units of a launch (`fill` writes them straight into the slot's page-locked
// memory), upload them on `st` and launch the reply kernel there.  The plan goes through
// the next slot of the ring: its previous launch (normally long finished) is waited for,
// so the caller's job array and the plan memory are free on return.
template <typename Fill>
int reply_enqueue(tfs_ec* ec, hipStream_t st, void* const* members, int size, int row, uint32_t n, Fill fill,
                  void* d_out, uint64_t out_cap, tfs_read_result* d_results, uint32_t* d_n_bad) {
  // the ring's mutex only deals the slots out; a slot's own mutex covers the wait for its last launch and the
  // allocations, so a call whose slot is still in flight on a slow stream holds up no call on another slot
  tfs_ec::ReplySlot* slot;
  {
    std::lock_guard<std::mutex> g(ec->reply_mu);
    slot = &ec->reply_slots[ec->reply_next++ % 4u];
  }
  tfs_ec::ReplySlot& sl = *slot;
  std::lock_guard<std::mutex> g(sl.mu);
  if (sl.done && hipEventSynchronize(sl.done) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  const uint64_t bytes = uint64_t(n) * sizeof(ReplyUnit);
  if (sl.cap < bytes) {
    if (sl.h) (void)hipHostFree(sl.h);
    if (sl.d) tfs_crc32_dev_free(ec->ctx, sl.d);
    sl.h = sl.d = nullptr;
    sl.cap = 0;
    const uint64_t want = (std::max<uint64_t>(bytes, 4096) + 0xFFFFu) & ~uint64_t(0xFFFF);
    if (hipHostMalloc(&sl.h, want, hipHostMallocDefault) != hipSuccess) {
      sl.h = nullptr;
      return TFS_EXIT_NO_MEMORY;
    }
    if (const int rc = tfs_crc32_dev_malloc(ec->ctx, want, &sl.d)) return rc;
    sl.cap = want;
  }
  fill(static_cast<ReplyUnit*>(sl.h));
  if (hipMemcpyAsync(sl.d, sl.h, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  // from here on the copy may be in flight: the slot gets its event behind it, or the stream is waited for
  const Plan& p = ec->dec;
  const int S = int(p.sources.size());
  ReplyArgs a;
  memset(&a, 0, sizeof a);
  for (int s = 0; s < S; ++s) a.src[s] = static_cast<const uint8_t*>(members[p.sources[s]]);
  a.masks = p.d_masks + size_t(row) * 8 * size_t(S) * 8;
  a.tab = ec->d_read_tab;
  a.units = static_cast<const ReplyUnit*>(sl.d);
  a.out = static_cast<uint8_t*>(d_out);
  a.out_cap = out_cap;
  a.results = d_results;
  a.n_bad = d_n_bad;
  a.n = n;
  a.S = uint32_t(S);
  a.size = size;
  const bool launched = launch_ec_read_reply(a, st) == hipSuccess;
  if (!sl.done && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) sl.done = nullptr;
  if (!sl.done || hipEventRecord(sl.done, st) != hipSuccess) {  // no event behind the copy: the slot is free only
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;  // once the stream has drained
    if (sl.done) (void)hipEventDestroy(sl.done);
    sl.done = nullptr;
  }
  return launched ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
}

// The device-visible address of page-locked host memory: the library's own allocations
// from the registry, anything else from the runtime.  false: pageable.
bool reply_pinned(const void* p, void** dev) {
  if (tfscrc::pin_lookup(p, dev)) return true;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost &&
      hipHostGetDevicePointer(dev, const_cast<void*>(p), 0) == hipSuccess)
    return true;
  (void)hipGetLastError();
  *dev = nullptr;
  return false;
}

// ---- marshalling session ----------------------------------

const MarshalTables& marshal_tables() {
  static const MarshalTables* t = [] {
    MarshalTables* r = new MarshalTables();
    tfscrc::make_slice_tables(r->slice, 4);
    tfscrc::make_shift_table(r->step_packet, kReadStepPacket);
    const uint32_t g = tfscrc::x2nmodp(8, 0), gi = tfscrc::x2nmodp(0xFFFFFFFFull - 8, 0);
    r->xpow[kMarshalPowBias] = 1u << 31;  // x^0
    for (int i = kMarshalPowBias + 1; i < kMarshalPowN; ++i) r->xpow[i] = tfscrc::multmodp(g, r->xpow[i - 1]);
    for (int i = kMarshalPowBias - 1; i >= 0; --i) r->xpow[i] = tfscrc::multmodp(gi, r->xpow[i + 1]);
    return r;
  }();
  return *t;
}

// The session's stream rule and chunk rule (include/tfs_ec.h); *st receives the stream.
int chunk_check(tfs_ec_marshal* m, int offset, int len, hipStream_t want, hipStream_t* st) {
  if (!m || !m->ec) return TFS_EXIT_PARAMETER_ERROR;
  if (want == hipStreamPerThread) return TFS_EXIT_PARAMETER_ERROR;
  *st = want ? want : static_cast<hipStream_t>(tfs_crc32_stream(m->ec->ctx));
  if (m->stream_set && *st != m->stream) return TFS_EXIT_PARAMETER_ERROR;
  if (offset != m->next || len <= 0 || offset % 4096 != 0 || len % kUnit != 0 || len > m->total - offset)
    return TFS_EXIT_PARAMETER_ERROR;
  if (len % 4096 != 0 && offset + len != m->total) return TFS_EXIT_PARAMETER_ERROR;
  return TFS_SUCCESS;
}

// The session's plan and partial results for a launch that walks records; mend is indexed by data member.
void fill_session_args(MarshalArgs& a, const tfs_ec_marshal& m, int offset) {
  a.tab = m.ec->d_marshal_tab;
  a.recs = m.d_recs;
  a.first = m.d_first;
  a.cont = m.d_cont;
  a.tail = m.d_tail;
  a.hdr = m.d_hdr;
  for (int i = 0; i < m.ec->dn; ++i) a.mend[i] = m.plan.mbegin[size_t(i) + 1];
  a.tile0 = uint32_t(offset) >> 12;
  a.ntiles = m.plan.ntiles;
}

int marshal_launch(tfs_ec_marshal* m, void* const* members, int offset, int len, hipStream_t st) {
  tfs_ec* ec = m->ec;
  const Plan& p = ec->enc;
  if (m->plan.recs.empty()) return run_plan(ec, p, members, len, st);  // no records: the plain encode
  for (size_t o0 = 0; o0 < p.outputs.size(); o0 += kMaxOutGroup) {
    const int og = int(std::min<size_t>(kMaxOutGroup, p.outputs.size() - o0));
    MarshalArgs a;
    memset(&a, 0, sizeof a);
    fill_ec_args(a.ec, p, members, o0, og, len);
    if (o0) {  // the CRC side runs with the first output group only
      if (launch_ec_apply(a.ec, og, 0, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
      continue;
    }
    fill_session_args(a, *m, offset);
    if (launch_ec_marshal(a, og, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return TFS_SUCCESS;
}

// ---- reinstate session -------------------------------------

int reinstate_launch(tfs_ec_reinstate* m, void* const* members, int offset, int len, hipStream_t st) {
  tfs_ec* ec = m->ec;
  const Plan& p = ec->dec;
  if (m->plan.recs.empty()) return run_plan(ec, p, members, len, st);  // no records: the plain decode
  const int S = int(p.sources.size()), dn = ec->dn;
  for (size_t o0 = 0; o0 < p.outputs.size(); o0 += kMaxOutGroup) {
    const int og = int(std::min<size_t>(kMaxOutGroup, p.outputs.size() - o0));
    ReinstateArgs a;
    memset(&a, 0, sizeof a);
    fill_ec_args(a.m.ec, p, members, o0, og, len);
    // the source walk runs with the first output group only; the output walk with every group that rebuilds data
    bool walk = o0 == 0;
    for (int s = 0; s < kMaxMembersDev; ++s)
      a.src_slot[s] = (o0 == 0 && s < S && p.sources[s] < dn) ? uint32_t(p.sources[s]) : kReinstateNoSlot;
    for (int o = 0; o < kMaxOutGroup; ++o) {
      a.out_slot[o] = (o < og && p.outputs[o0 + o] < dn) ? uint32_t(p.outputs[o0 + o]) : kReinstateNoSlot;
      walk = walk || a.out_slot[o] != kReinstateNoSlot;
    }
    if (!walk) {  // a later group of parity members only
      if (launch_ec_apply(a.m.ec, og, 0, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
      continue;
    }
    fill_session_args(a.m, *m, offset);
    if (launch_ec_reinstate(a, og, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return TFS_SUCCESS;
}

// One chunk of a session, for every chunk entry point: the checks in the header's order (the session, the
// stream rule, the chunk rule, `members`, then each member the session binds), the launch, the bookkeeping.
// The host form stages the session's `up` members to the coder's device buffers under its mutex, launches over
// those, brings the `down` members back and synchronises; the device form launches over `members` as they are.
template <typename Session>
int session_chunk(Session* s, int (*launch)(Session*, void* const*, int, int, hipStream_t), void* const* members,
                  int offset, int len, void* stream, bool host) {
  tfs_ec_marshal* m = s;
  hipStream_t st = nullptr;
  int rc = chunk_check(m, offset, len, static_cast<hipStream_t>(stream), &st);
  if (rc) return rc;
  if (!members) return TFS_EXIT_DATA_INVALID;
  for (const std::vector<int>* v : {&m->up, &m->down})
    for (int i : *v)
      if (!members[i]) return TFS_EXIT_DATA_INVALID;
  if (!host) {
    if ((rc = launch(s, members, offset, len, st))) return rc;
  } else {
    tfs_ec* ec = m->ec;
    std::lock_guard<std::mutex> g(ec->mu);
    std::vector<void*> dm(ec->staging.size(), nullptr);
    for (const std::vector<int>* v : {&m->up, &m->down})
      for (int i : *v) {
        if ((rc = grow(ec, &ec->staging[i], &ec->staging_cap[i], uint64_t(len)))) return rc;
        dm[size_t(i)] = ec->staging[i];
      }
    for (int i : m->up)
      if (hipMemcpyAsync(dm[size_t(i)], members[i], size_t(len), hipMemcpyHostToDevice, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    if ((rc = launch(s, dm.data(), offset, len, st))) return rc;
    for (int i : m->down)
      if (hipMemcpyAsync(members[i], dm[size_t(i)], size_t(len), hipMemcpyDeviceToHost, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  m->next += len;
  m->stream = st;
  m->stream_set = true;
  return TFS_SUCCESS;
}

// ---- frame-emitting chunk calls (include/tfs_ec_frames.h) ----

// The tables of the tile CRC and the seal: a session without records never uploaded them at begin.
int ensure_marshal_tab(tfs_ec* ec) {
  std::lock_guard<std::mutex> g(ec->mu);
  if (ec->d_marshal_tab) return TFS_SUCCESS;
  void* d = nullptr;
  int rc = tfs_crc32_dev_malloc(ec->ctx, sizeof(MarshalTables), &d);
  if (rc) return rc;
  if (hipMemcpy(d, &marshal_tables(), sizeof(MarshalTables), hipMemcpyHostToDevice) != hipSuccess) {
    tfs_crc32_dev_free(ec->ctx, d);
    return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  ec->d_marshal_tab = static_cast<MarshalTables*>(d);
  return TFS_SUCCESS;
}

// The launches of one frames call: the tile pass of every output group, then one seal over every (output,
// frame).  `members` and `out` are device addresses by member; frame j of output member i goes to out[i] +
// j * stride.  A slot is given to a source or output that is a data member while the session has records:
// the marshalling session's sources all have one, its outputs none.
// A task call gives `task`: `members` then holds each source's incoming frames, the tile pass
// is ec_task_kernel, the source check runs before the seal and the seal is the one that reads its results.
struct TaskCall {
  uint32_t in_stride;
  tfs_ec_fetch_result* d_results;  // [sources][frames of the call]
};
int frames_launch(tfs_ec_marshal* m, const Plan& p, const tfs_ec_frames_cfg& cfg, void* const* members, void* const* out,
                  uint32_t stride, int offset, int len, hipStream_t st, const TaskCall* task = nullptr) {
  tfs_ec* ec = m->ec;
  const int S = int(p.sources.size()), dn = ec->dn;
  const bool recs = !m->plan.recs.empty();
  std::vector<void*> bound(size_t(ec->dn + ec->pn), nullptr);  // the sources' chunks and the outputs' frames
  for (int s : p.sources) bound[size_t(s)] = members[s];
  for (int o : p.outputs) bound[size_t(o)] = out[o];
  for (size_t o0 = 0; o0 < p.outputs.size(); o0 += kMaxOutGroup) {
    const int og = int(std::min<size_t>(kMaxOutGroup, p.outputs.size() - o0));
    FramesArgs a;
    memset(&a, 0, sizeof a);
    fill_ec_args(a.r.m.ec, p, bound.data(), o0, og, len);
    // the source walk runs with the first output group only; the output walk with every group that rebuilds data
    bool walk = false;
    for (int s = 0; s < kMaxMembersDev; ++s) {
      a.r.src_slot[s] = (recs && o0 == 0 && s < S && p.sources[s] < dn) ? uint32_t(p.sources[s]) : kReinstateNoSlot;
      walk = walk || a.r.src_slot[s] != kReinstateNoSlot;
    }
    for (int o = 0; o < kMaxOutGroup; ++o) {
      a.r.out_slot[o] = (recs && o < og && p.outputs[o0 + o] < dn) ? uint32_t(p.outputs[o0 + o]) : kReinstateNoSlot;
      walk = walk || a.r.out_slot[o] != kReinstateNoSlot;
    }
    fill_session_args(a.r.m, *m, offset);  // without records: the tables, tile0 and ntiles; no plan array is read
    a.tile_crc = m->d_tile_crc;
    a.o0 = uint32_t(o0);
    a.tpf = uint32_t(cfg.frame_len) >> 12;
    a.stride = stride;
    a.len = uint32_t(len);
    if (task) {
      TaskArgs t;
      memset(&t, 0, sizeof t);
      t.f = a;
      for (int s = 0; s < S; ++s) t.blen[s] = uint32_t(ecx_block_len(m->sizes.data(), dn, m->total, p.sources[s]));
      t.src_crc = o0 == 0 ? m->d_src_crc : nullptr;
      t.in_stride = task->in_stride;
      if (launch_ec_task(t, og, walk, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
      continue;
    }
    if (launch_ec_frames(a, og, walk, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  if (task) {
    TaskCheckArgs c;
    memset(&c, 0, sizeof c);
    for (int s = 0; s < S; ++s) {
      c.in[s] = static_cast<const uint8_t*>(members[p.sources[s]]);
      c.blen[s] = uint32_t(ecx_block_len(m->sizes.data(), dn, m->total, p.sources[s]));
    }
    c.tab = ec->d_marshal_tab;
    c.src_crc = m->d_src_crc;
    c.results = task->d_results;
    c.ntiles = m->plan.ntiles;
    c.S = uint32_t(S);
    c.nf = ecf_call_frames(cfg.frame_len, len);
    c.frame0 = uint32_t(offset / cfg.frame_len);
    c.frame_len = uint32_t(cfg.frame_len);
    c.in_stride = task->in_stride;
    c.total = uint32_t(m->total);
    if (launch_ec_fetch_check(c, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  FramesSealArgs f;
  memset(&f, 0, sizeof f);
  for (size_t k = 0; k < p.outputs.size(); ++k) {
    const int i = p.outputs[k];
    f.out[k] = static_cast<uint8_t*>(out[i]);
    f.pid[k] = cfg.packet_id[i];
    f.block_id[k] = cfg.block_id[i];
    f.flag0[k] = i >= dn ? uint32_t(TFS_RAW_PARITY_DATA) : uint32_t(TFS_RAW_NORMAL_DATA);
  }
  const EcfCallConst kc = ecf_call_const(cfg.frame_len, m->total);
  f.tab = ec->d_marshal_tab;
  f.tile_crc = m->d_tile_crc;
  f.ntiles = m->plan.ntiles;
  f.n_out = uint32_t(p.outputs.size());
  f.nf = ecf_call_frames(cfg.frame_len, len);
  f.frame0 = uint32_t(offset / cfg.frame_len);
  f.frame_len = uint32_t(cfg.frame_len);
  f.stride = stride;
  f.total = uint32_t(m->total);
  f.type_ver = uint32_t(TFS_WRITE_RAW_DATA_MESSAGE) | uint32_t(uint16_t(cfg.version)) << 16;
  f.pow_head_full = kc.pow_head_full;
  f.pow_head_last = kc.pow_head_last;
  if (task) {
    TaskSealArgs t;
    memset(&t, 0, sizeof t);
    t.f = f;
    t.results = task->d_results;
    t.S = uint32_t(S);
    return launch_ec_task_seal(t, st) == hipSuccess ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return launch_ec_frames_seal(f, st) == hipSuccess ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
}

// The host form's way down: every output's frames from the coder's device buffers (sstride apart) to their
// places in the caller's out (stride apart); no byte between two frames is written.
int frames_down(tfs_ec_marshal* m, const tfs_ec_frames_cfg& cfg, void* const* out, void* const* dout, uint32_t stride,
                uint32_t sstride, uint32_t nf, uint64_t last, hipStream_t st) {
  for (int i : m->down) {
    char* const h = static_cast<char*>(out[i]);
    const char* const d = static_cast<const char*>(dout[size_t(i)]);
    if (nf > 1 && hipMemcpy2DAsync(h, stride, d, sstride, size_t(cfg.frame_len) + kEcfOverhead, nf - 1,
                                   hipMemcpyDeviceToHost, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
    if (hipMemcpyAsync(h + uint64_t(nf - 1) * stride, d + uint64_t(nf - 1) * sstride, size_t(last),
                       hipMemcpyDeviceToHost, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return TFS_SUCCESS;
}

// One frames chunk of a session, for the four entry points: the checks in the header's order, the launches,
// the bookkeeping.  Host form, under the coder's mutex: the sources are staged up as session_chunk stages
// them; when every output's `out` is page-locked the frames are written in place at the caller's stride,
// otherwise they are made in the coder's device buffers, frame_len + 64 apart, and each frame is brought down
// to its place (no byte between two frames is written).
int session_frames(tfs_ec_marshal* m, const Plan* plan, const tfs_ec_frames_cfg* cfg, void* const* members,
                   void* const* out, uint64_t out_cap, int offset, int len, void* stream, bool host) {
  hipStream_t st = nullptr;
  int rc = chunk_check(m, offset, len, static_cast<hipStream_t>(stream), &st);
  if (rc) return rc;
  const Plan& p = *plan;
  rc = ecf_call_status(cfg, members, out, out_cap, m->total, offset, len, m->up.data(), int(m->up.size()), m->down.data(),
                       int(m->down.size()));
  if (rc) return rc;
  tfs_ec* ec = m->ec;
  if ((rc = ensure_marshal_tab(ec))) return rc;
  if (!m->d_tile_crc) {
    void* d = nullptr;
    if ((rc = tfs_crc32_dev_malloc(ec->ctx, 4 * p.outputs.size() * size_t(m->plan.ntiles) + 64, &d))) return rc;
    m->d_tile_crc = static_cast<uint32_t*>(d);
  }
  const uint32_t stride = uint32_t(ecf_stride(*cfg));
  if (!host) {
    if ((rc = frames_launch(m, p, *cfg, members, out, stride, offset, len, st))) return rc;
  } else {
    std::lock_guard<std::mutex> g(ec->mu);
    std::vector<void*> dm(ec->staging.size(), nullptr), dout(ec->staging.size(), nullptr);
    bool in_place = true;
    for (int i : m->down) in_place = reply_pinned(out[i], &dout[size_t(i)]) && in_place;
    const uint32_t sstride = in_place ? stride : uint32_t(cfg->frame_len) + 64u;
    const uint32_t nf = ecf_call_frames(cfg->frame_len, len);
    const uint64_t last = uint64_t(len) - uint64_t(nf - 1) * uint64_t(cfg->frame_len) + kEcfOverhead;
    for (int i : m->up) {
      if ((rc = grow(ec, &ec->staging[i], &ec->staging_cap[i], uint64_t(len)))) return rc;
      dm[size_t(i)] = ec->staging[i];
      if (hipMemcpyAsync(dm[size_t(i)], members[i], size_t(len), hipMemcpyHostToDevice, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    }
    if (!in_place)
      for (int i : m->down) {
        if ((rc = grow(ec, &ec->staging[i], &ec->staging_cap[i], uint64_t(nf - 1) * sstride + last))) return rc;
        dout[size_t(i)] = ec->staging[i];
      }
    if ((rc = frames_launch(m, p, *cfg, dm.data(), dout.data(), sstride, offset, len, st))) return rc;
    if (!in_place && (rc = frames_down(m, *cfg, out, dout.data(), stride, sstride, nf, last, st))) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  m->next += len;
  m->stream = st;
  m->stream_set = true;
  return TFS_SUCCESS;
}

// ---- task chunk calls (include/tfs_ec_fetch.h) ----

// One task chunk of a session, for the four entry points: the checks in the header's order, the launches, the
// bookkeeping.  Host form, under the coder's mutex: when every source with a frame to read has a page-locked
// `in` at 4 modulo 8 the frames are read in place at the caller's stride; otherwise each source's frames are
// staged to the coder's device buffers at that alignment, frame_len + 32 apart -- 32 + n bytes of a frame, and
// no frame whose expected n is 0.  The outputs come down as session_frames brings them, the results behind them.
int session_task(tfs_ec_marshal* m, const Plan* plan, const tfs_ec_frames_cfg* cfg, const tfs_ec_fetch_cfg* fcfg,
                 const void* const* in, void* const* out, uint64_t out_cap, tfs_ec_fetch_result* results, int offset,
                 int len, void* stream, bool host) {
  hipStream_t st = nullptr;
  int rc = chunk_check(m, offset, len, static_cast<hipStream_t>(stream), &st);
  if (rc) return rc;
  const Plan& p = *plan;
  tfs_ec* ec = m->ec;
  const int S = int(m->up.size());
  int32_t blen[kMaxMembersDev];
  for (int k = 0; k < S; ++k) blen[k] = ecx_block_len(m->sizes.data(), ec->dn, m->total, m->up[size_t(k)]);
  rc = ecx_call_status(cfg, fcfg, in, out, out_cap, results, m->total, offset, len, m->up.data(), blen, S, m->down.data(),
                       int(m->down.size()), !host);
  if (rc) return rc;
  if ((rc = ensure_marshal_tab(ec))) return rc;
  const size_t nt = m->plan.ntiles;
  if (!m->d_tile_crc) {
    void* d = nullptr;
    if ((rc = tfs_crc32_dev_malloc(ec->ctx, 4 * p.outputs.size() * nt + 64, &d))) return rc;
    m->d_tile_crc = static_cast<uint32_t*>(d);
  }
  if (!m->d_src_crc) {  // the words, then a result per (source, frame) of the longest call at the shortest frame
    void* d = nullptr;
    const size_t words = (size_t(S) * nt + 3) & ~size_t(3);
    if ((rc = tfs_crc32_dev_malloc(ec->ctx, 4 * words + sizeof(tfs_ec_fetch_result) * size_t(S) * nt + 64, &d))) return rc;
    m->d_src_crc = static_cast<uint32_t*>(d);
    m->d_task_res = reinterpret_cast<tfs_ec_fetch_result*>(m->d_src_crc + words);
  }
  const uint32_t stride = uint32_t(ecf_stride(*cfg));
  const uint32_t in_stride = uint32_t(ecx_stride(*cfg, *fcfg));
  const uint32_t nf = ecf_call_frames(cfg->frame_len, len);
  int verdict = TFS_SUCCESS;
  if (!host) {
    const TaskCall t{in_stride, results};
    if ((rc = frames_launch(m, p, *cfg, const_cast<void* const*>(in), out, stride, offset, len, st, &t))) return rc;
  } else {
    std::lock_guard<std::mutex> g(ec->mu);
    std::vector<void*> din(ec->staging.size(), nullptr), dout(ec->staging.size(), nullptr);
    bool out_place = true, in_place = true;
    for (int i : m->down) out_place = reply_pinned(out[i], &dout[size_t(i)]) && out_place;
    for (int k = 0; k < S; ++k) {
      const int i = m->up[size_t(k)];
      if (!ecx_reads(blen[k], offset)) continue;
      in_place = reply_pinned(in[i], &din[size_t(i)]) && (reinterpret_cast<uintptr_t>(din[size_t(i)]) & 7u) == 4u && in_place;
    }
    const uint32_t sstride = out_place ? stride : uint32_t(cfg->frame_len) + 64u;
    const uint32_t sin = in_place ? in_stride : uint32_t(cfg->frame_len) + kEcxOverhead;
    const uint64_t last = uint64_t(len) - uint64_t(nf - 1) * uint64_t(cfg->frame_len) + kEcfOverhead;
    if (!in_place) {
      tfs_ec_fetch_cfg packed = *fcfg;
      packed.in_stride = 0;
      for (int k = 0; k < S; ++k) {
        const int i = m->up[size_t(k)];
        din[size_t(i)] = nullptr;
        if (!ecx_reads(blen[k], offset)) continue;
        if ((rc = grow(ec, &ec->staging[i], &ec->staging_cap[i], 8u + ecx_call_need(*cfg, packed, len)))) return rc;
        char* const d = static_cast<char*>(ec->staging[i]) + 4;  // 4 modulo 8: the data of every frame 8-byte aligned
        din[size_t(i)] = d;
        const char* const h = static_cast<const char*>(in[i]);
        uint32_t full = 0;  // the leading frames that carry frame_len bytes go up in one copy
        while (full < nf && ecx_expect(blen[k], int64_t(offset) + int64_t(full) * cfg->frame_len,
                                       ecx_requested(cfg->frame_len, len, full)) == cfg->frame_len)
          ++full;
        if (full && hipMemcpy2DAsync(d, sin, h, in_stride, size_t(cfg->frame_len) + kEcxOverhead, full,
                                     hipMemcpyHostToDevice, st) != hipSuccess)
          return TFS_CRC_EXIT_DEVICE_ERROR;
        for (uint32_t j = full; j < nf; ++j) {
          const int32_t n = ecx_expect(blen[k], int64_t(offset) + int64_t(j) * cfg->frame_len,
                                       ecx_requested(cfg->frame_len, len, j));
          if (n == 0) break;  // and every later frame
          if (hipMemcpyAsync(d + uint64_t(j) * sin, h + uint64_t(j) * in_stride, size_t(n) + kEcxOverhead,
                             hipMemcpyHostToDevice, st) != hipSuccess)
            return TFS_CRC_EXIT_DEVICE_ERROR;
        }
      }
    }
    if (!out_place)
      for (int i : m->down) {
        if ((rc = grow(ec, &ec->staging[i], &ec->staging_cap[i], uint64_t(nf - 1) * sstride + last))) return rc;
        dout[size_t(i)] = ec->staging[i];
      }
    const TaskCall t{sin, m->d_task_res};
    if ((rc = frames_launch(m, p, *cfg, din.data(), dout.data(), sstride, offset, len, st, &t))) return rc;
    if (!out_place && (rc = frames_down(m, *cfg, out, dout.data(), stride, sstride, nf, last, st))) return rc;
    const size_t nres = size_t(S) * nf;
    if (hipMemcpyAsync(results, m->d_task_res, nres * sizeof(tfs_ec_fetch_result), hipMemcpyDeviceToHost, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
    for (size_t k = 0; k < nres; ++k)
      if (results[k].status != TFS_SUCCESS) verdict = TFS_EXIT_CHECK_CRC_ERROR;
  }
  m->next += len;
  m->stream = st;
  m->stream_set = true;
  return verdict;
}

template <typename Session>
int session_free(Session* s) {
  if (!s) return TFS_EXIT_PARAMETER_ERROR;
  if (s->stream_set) (void)hipStreamSynchronize(s->stream);
  if (s->d_buf) tfs_crc32_dev_free(s->ec->ctx, s->d_buf);
  if (s->d_tile_crc) tfs_crc32_dev_free(s->ec->ctx, s->d_tile_crc);
  if (s->d_src_crc) tfs_crc32_dev_free(s->ec->ctx, s->d_src_crc);
  delete s;
  return TFS_SUCCESS;
}

// The plan of a session (make_marshal_plan) and its one device allocation: the plan's
// arrays uploaded, the partial results behind them.  On failure nothing is left allocated.
// extra(ntiles) words more are allocated right behind the statuses (*d_extra), so that they reach
// the host in the statuses' copy; a session without records then holds those words alone.
int session_begin(tfs_ec* ec, tfs_ec_marshal* m, const tfs_raw_meta* const* metas, const uint32_t* n_metas,
                  const int* sizes, int total, size_t (*extra)(const tfs_ec*, uint32_t) = nullptr,
                  uint32_t** d_extra = nullptr) {
  m->ec = ec;
  m->total = total;
  int rc = make_marshal_plan(reinterpret_cast<const MarshalMeta* const*>(metas), n_metas, sizes, ec->dn, total, &m->plan);
  if (rc == TFS_SUCCESS) m->sizes.assign(sizes, sizes + ec->dn);
  const MarshalPlan& p = m->plan;
  const size_t n = p.recs.size(), nt = p.ntiles, dn = size_t(ec->dn);
  const size_t w_extra = (rc == TFS_SUCCESS && extra) ? extra(ec, p.ntiles) : 0;
  if (rc == TFS_SUCCESS && !n && w_extra) {
    rc = tfs_crc32_dev_malloc(ec->ctx, 4 * w_extra + 64, &m->d_buf);
    if (rc == TFS_SUCCESS) *d_extra = static_cast<uint32_t*>(m->d_buf);
  }
  if (rc == TFS_SUCCESS && n) {
    {
      std::lock_guard<std::mutex> g(ec->mu);
      if (!ec->d_marshal_tab) {
        void* d = nullptr;
        rc = tfs_crc32_dev_malloc(ec->ctx, sizeof(MarshalTables), &d);
        if (rc == TFS_SUCCESS && hipMemcpy(d, &marshal_tables(), sizeof(MarshalTables), hipMemcpyHostToDevice) != hipSuccess) {
          tfs_crc32_dev_free(ec->ctx, d);
          rc = TFS_CRC_EXIT_DEVICE_ERROR;
        }
        if (rc == TFS_SUCCESS) ec->d_marshal_tab = static_cast<MarshalTables*>(d);
      }
    }
    // words of the plan (uploaded) and of the results behind it
    const size_t w_recs = 4 * n, w_first = dn * nt, w_up = w_recs + w_first + n + nt;
    const size_t w_all = w_up + dn * nt + n + kMarshalHdrWords * n + 2 * n + w_extra;
    if (rc == TFS_SUCCESS) rc = tfs_crc32_dev_malloc(ec->ctx, 4 * w_all + 64, &m->d_buf);
    if (rc == TFS_SUCCESS) {
      std::vector<uint32_t> up(w_up);
      memcpy(up.data(), p.recs.data(), 16 * n);
      memcpy(up.data() + w_recs, p.first.data(), 4 * w_first);
      memcpy(up.data() + w_recs + w_first, p.member.data(), 4 * n);
      uint32_t* pw = up.data() + w_recs + w_first + n;  // x^(8 * 4096 * k)
      const uint32_t x4k = tfscrc::x2nmodp(4096, 3);
      pw[0] = 1u << 31;
      for (size_t k = 1; k < nt; ++k) pw[k] = tfscrc::multmodp(x4k, pw[k - 1]);
      uint32_t* d = static_cast<uint32_t*>(m->d_buf);
      m->d_recs = reinterpret_cast<MarshalRec*>(d);
      m->d_first = d + w_recs;
      m->d_member = m->d_first + w_first;
      m->d_pow = m->d_member + n;
      m->d_cont = d + w_up;
      m->d_tail = m->d_cont + dn * nt;
      m->d_hdr = m->d_tail + n;
      m->d_crc = m->d_hdr + kMarshalHdrWords * n;
      m->d_status = reinterpret_cast<int32_t*>(m->d_crc + n);
      if (d_extra) *d_extra = m->d_crc + 2 * n;
      if (hipMemcpy(d, up.data(), 4 * w_up, hipMemcpyHostToDevice) != hipSuccess) rc = TFS_CRC_EXIT_DEVICE_ERROR;
    }
  }
  if (rc != TFS_SUCCESS && m->d_buf) {
    tfs_crc32_dev_free(ec->ctx, m->d_buf);
    m->d_buf = nullptr;
  }
  return rc;
}

// The end of every session: the fold on the session's stream, the results to the host in one
// copy, one synchronisation.  `more` bytes behind the statuses (session_begin's extra words; a
// scrub session's counts and map) travel with them to h_more.
int session_finish(tfs_ec_marshal* m, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad, void* h_more,
                   const void* d_more, size_t more) {
  if (!m || !m->ec || m->next != m->total) return TFS_EXIT_PARAMETER_ERROR;
  const MarshalPlan& p = m->plan;
  const size_t all = p.early.size(), n = p.recs.size();
  if (all && (!out_crc || !out_status)) return TFS_EXIT_PARAMETER_ERROR;
  uint32_t bad = 0;
  for (size_t j = 0; j < all; ++j) {
    out_crc[j] = 0;
    out_status[j] = p.early[j];
    if (p.early[j]) ++bad;
  }
  hipStream_t st = m->stream_set ? m->stream : static_cast<hipStream_t>(tfs_crc32_stream(m->ec->ctx));
  if (n) {
    MarshalFoldArgs a;
    memset(&a, 0, sizeof a);
    a.tab = m->ec->d_marshal_tab;
    a.recs = m->d_recs;
    a.rec_member = m->d_member;
    a.cont = m->d_cont;
    a.tail = m->d_tail;
    a.hdr = m->d_hdr;
    a.pow_tile = m->d_pow;
    a.out_crc = m->d_crc;
    a.out_status = m->d_status;
    a.n = uint32_t(n);
    a.ntiles = p.ntiles;
    if (launch_ec_marshal_fold(a, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  std::vector<uint32_t> res(2 * n + (more + 3) / 4);  // crc, status and the `more` bytes lie back to back
  const void* src = n ? static_cast<const void*>(m->d_crc) : d_more;
  const bool copied =
      res.empty() || hipMemcpyAsync(res.data(), src, 8 * n + more, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess || !copied) return TFS_CRC_EXIT_DEVICE_ERROR;
  for (size_t k = 0; k < n; ++k) {
    out_crc[p.index[k]] = res[k];
    out_status[p.index[k]] = int32_t(res[n + k]);
    if (res[n + k]) ++bad;
  }
  if (more) memcpy(h_more, res.data() + 2 * n, more);
  if (n_bad) *n_bad += bad;
  return TFS_SUCCESS;
}

// ---- scrub session ------------------------------------------

// A scrub session's words behind the statuses: units [pn], the map's bytes, pbad [pn][ntiles].
size_t scrub_words(const tfs_ec* ec, uint32_t ntiles) {
  const size_t pn = size_t(ec->pn), nt = ntiles;
  return pn + (pn * nt + 3) / 4 + pn * nt;
}

int scrub_launch(tfs_ec_scrub* c, void* const* members, int offset, int len, hipStream_t st) {
  const Plan& p = c->ec->enc;
  for (size_t o0 = 0; o0 < p.outputs.size(); o0 += kMaxOutGroup) {
    const int og = int(std::min<size_t>(kMaxOutGroup, p.outputs.size() - o0));
    ScrubArgs a;
    memset(&a, 0, sizeof a);
    fill_ec_args(a.m.ec, p, members, o0, og, len);
    for (int o = 0; o < og; ++o) a.par[o] = a.m.ec.dst[o];  // the plan's outputs are read here, never written
    fill_session_args(a.m, *c, offset);  // a session without records has no plan arrays, and no launch that reads them
    a.pbad = c->d_pbad;
    a.o0 = uint32_t(o0);
    const bool walk = !c->plan.recs.empty() && o0 == 0;  // the CRC side runs with the first output group only
    if (launch_ec_scrub(a, og, walk, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return TFS_SUCCESS;
}

// ---- scrub locate --------------------------------------------

// The checks of tfs_ec_locate(_device) up to the unit bounds, in the header's order.
int locate_check(tfs_ec* ec, const void* const* members, int size, const uint32_t* units, uint32_t n) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  if (!ec->enc.valid) return TFS_EXIT_MATRIX_INVALID;
  if (ec->pn < 2) return TFS_EXIT_PARAMETER_ERROR;
  if (size <= 0 || size % kUnit != 0) return TFS_EXIT_SIZE_INVALID;
  if (!members) return TFS_EXIT_DATA_INVALID;
  for (int i = 0; i < ec->dn + ec->pn; ++i)
    if (!members[i]) return TFS_EXIT_DATA_INVALID;
  const uint32_t have = uint32_t(size) / kUnit;
  if (units) {
    for (uint32_t k = 0; k < n; ++k)
      if (units[k] >= have) return TFS_EXIT_PARAMETER_ERROR;
  } else if (n > have) {
    return TFS_EXIT_PARAMETER_ERROR;
  }
  return TFS_SUCCESS;
}

// The locate plan of the coder, built and uploaded by the first call (ec->mu held).
int locate_plan(tfs_ec* ec) {
  if (ec->d_locate || ec->locate_rc != TFS_SUCCESS) return ec->locate_rc;
  LocatePlan p;
  const int r = make_locate_plan(ec->dn, ec->pn, &p);
  if (r) return ec->locate_rc = (r == -2 ? TFS_EXIT_MATRIX_INVALID : TFS_EXIT_PARAMETER_ERROR);
  std::vector<uint32_t> w(p.ratio);
  w.insert(w.end(), p.inv0.begin(), p.inv0.end());
  void* d = nullptr;
  int rc = tfs_crc32_dev_malloc(ec->ctx, 4 * w.size() + 64, &d);
  if (rc) return rc;  // out of memory now: the next call tries again
  if (hipMemcpy(d, w.data(), 4 * w.size(), hipMemcpyHostToDevice) != hipSuccess) {
    tfs_crc32_dev_free(ec->ctx, d);
    return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  ec->d_locate = static_cast<uint32_t*>(d);
  ec->locate_ratio_words = p.ratio.size();
  return TFS_SUCCESS;
}

// One launch over device members (ec->mu held): d_units is a device list or nullptr.
int locate_launch(tfs_ec* ec, const void* const* d_members, const uint32_t* d_units, uint32_t n, void* d_result,
                  void* d_fixed, hipStream_t st) {
  LocateArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < ec->dn + ec->pn; ++i) a.mem[i] = static_cast<const uint8_t*>(d_members[i]);
  a.masks = ec->enc.d_masks;
  a.ratio = ec->d_locate;
  a.inv0 = ec->d_locate + ec->locate_ratio_words;
  a.units = d_units;
  a.result = static_cast<LocateResult*>(d_result);
  a.fixed = static_cast<uint8_t*>(d_fixed);
  a.n = n;
  a.dn = uint32_t(ec->dn);
  a.pn = uint32_t(ec->pn);
  return launch_ec_locate(a, st) == hipSuccess ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
}

// The caller's list to the device on st (ec->mu held), for locate and update calls alike.  The page-locked
// copy is the coder's, so the caller's array is free when the call returns; it is written again only after
// its last upload has left it, and a call on another stream waits for the last kernel that read the device
// list (the caller records loc_done behind its kernel).
int locate_upload_list(tfs_ec* ec, const uint32_t* units, uint32_t n, hipStream_t st) {
  const uint64_t bytes = 4ull * n;
  if (!ec->loc_copied && hipEventCreateWithFlags(&ec->loc_copied, hipEventDisableTiming) != hipSuccess)
    return TFS_CRC_EXIT_DEVICE_ERROR;
  if (!ec->loc_done && hipEventCreateWithFlags(&ec->loc_done, hipEventDisableTiming) != hipSuccess)
    return TFS_CRC_EXIT_DEVICE_ERROR;
  if (ec->loc_busy) {
    if (hipEventSynchronize(ec->loc_copied) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
    if (st != ec->loc_stream && hipStreamWaitEvent(st, ec->loc_done, 0) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  if (ec->loc_pin_cap < bytes) {
    if (ec->loc_pin) (void)hipHostFree(ec->loc_pin);
    ec->loc_pin = nullptr;
    ec->loc_pin_cap = 0;
    void* h = nullptr;
    const uint64_t cap = bytes < 4096 ? 4096 : bytes;
    if (hipHostMalloc(&h, cap, hipHostMallocDefault) != hipSuccess) return TFS_EXIT_NO_MEMORY;
    ec->loc_pin = static_cast<uint32_t*>(h);
    ec->loc_pin_cap = cap;
  }
  const int rc = grow(ec, &ec->loc_list, &ec->loc_list_cap, bytes < 4096 ? 4096 : bytes);  // a free waits for the device
  if (rc) return rc;
  memcpy(ec->loc_pin, units, bytes);
  if (hipMemcpyAsync(ec->loc_list, ec->loc_pin, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipEventRecord(ec->loc_copied, st) != hipSuccess)
    return TFS_CRC_EXIT_DEVICE_ERROR;
  ec->loc_busy = true;  // from here on the events have been recorded at least once
  ec->loc_stream = st;
  return TFS_SUCCESS;
}

// ---- parity update --------------------------------------------

// The checks of tfs_ec_update(_device) up to the unit list, in the header's order.
int update_check(tfs_ec* ec, int member, const void* const* parity, int size, const uint32_t* units, uint32_t n) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  if (!ec->enc.valid) return TFS_EXIT_MATRIX_INVALID;
  if (member < 0 || member >= ec->dn) return TFS_EXIT_PARAMETER_ERROR;
  if (size <= 0 || size % kUnit != 0) return TFS_EXIT_SIZE_INVALID;
  bool bound = false;
  for (int p = 0; parity && p < ec->pn; ++p) bound = bound || parity[p];
  if (!bound) return TFS_EXIT_DATA_INVALID;
  return update_list_check(units, n, uint32_t(size) / kUnit) ? TFS_EXIT_PARAMETER_ERROR : TFS_SUCCESS;
}

// One launch over device buffers (ec->mu held).  inl: a host list of at most kUpdateInline units that
// travels in the launch arguments; d_units: a device list; neither: entry k is unit k.
int update_launch(tfs_ec* ec, int member, void* const* d_parity, const uint32_t* inl, const uint32_t* d_units, uint32_t n,
                  const void* d_a, const void* d_b, hipStream_t st) {
  UpdateArgs a;
  memset(&a, 0, sizeof a);
  for (int p = 0; p < ec->pn; ++p) a.par[p] = static_cast<uint8_t*>(d_parity[p]);
  a.masks = ec->enc.d_masks;
  a.units = d_units;
  a.a = static_cast<const uint8_t*>(d_a);
  a.b = static_cast<const uint8_t*>(d_b);
  if (inl) {
    memcpy(a.inl, inl, 4 * size_t(n));
    a.n_inline = n;
  }
  a.n = n;
  a.dn = uint32_t(ec->dn);
  a.pn = uint32_t(ec->pn);
  a.member = uint32_t(member);
  return launch_ec_update(a, st) == hipSuccess ? TFS_SUCCESS : TFS_CRC_EXIT_DEVICE_ERROR;
}

}  // namespace

extern "C" {

int tfs_ec_read_degraded_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, int target,
                                const tfs_ec_read_job* d_jobs, uint32_t n, void* d_out, uint64_t out_cap,
                                uint32_t* d_out_crc, int32_t* d_out_status, uint32_t* d_n_bad, void* stream) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  int row = -1;
  const int rc = check_read(ec, d_members, sizes, size, target, &row);
  if (rc) return rc;
  if (stream && static_cast<hipStream_t>(stream) == hipStreamPerThread) return TFS_EXIT_PARAMETER_ERROR;
  if (n == 0) return TFS_SUCCESS;
  if (!d_jobs || !d_out_crc || !d_out_status || (!d_out && out_cap)) return TFS_EXIT_PARAMETER_ERROR;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  return launch_read(ec, d_members, size, row, d_jobs, n, d_out, out_cap, d_out_crc, d_out_status, d_n_bad, st);
}

int tfs_ec_read_degraded(tfs_ec* ec, char* const* members, const int* sizes, int size, int target,
                         const tfs_ec_read_job* jobs, uint32_t n, void* out, uint64_t out_cap, uint32_t* out_crc,
                         int32_t* out_status, uint32_t* n_bad) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  int row = -1;
  int rc = check_read(ec, reinterpret_cast<void* const*>(members), sizes, size, target, &row);
  if (rc) return rc;
  ec->read_up = ec->read_down = 0;
  if (n == 0) return TFS_SUCCESS;
  if (!jobs || !out_crc || !out_status || (!out && out_cap)) return TFS_EXIT_PARAMETER_ERROR;
  static_assert(sizeof(tfs_ec_read_job) == sizeof(ReadJob), "read job layout");
  ReadPlan plan;
  make_read_plan(reinterpret_cast<const ReadJob*>(jobs), n, size, out_cap, &plan);
  uint32_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) {
    out_crc[i] = 0;
    out_status[i] = plan.early[i];
    if (plan.early[i]) ++bad;
  }
  const uint32_t m = uint32_t(plan.jobs.size());
  if (m) {
    const int nm = ec->dn + ec->pn;
    hipStream_t st = static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
    const uint64_t up = plan.up ? plan.up : uint64_t(kUnit);
    std::vector<void*> dm(nm, nullptr);
    for (int s : ec->dec.sources) {
      if ((rc = grow(ec, &ec->staging[s], &ec->staging_cap[s], up))) return rc;
      dm[s] = ec->staging[s];
      for (const ReadSpan& sp : plan.spans)
        if (hipMemcpyAsync(static_cast<char*>(dm[s]) + sp.cbase, members[s] + sp.start, size_t(sp.end - sp.start),
                           hipMemcpyHostToDevice, st) != hipSuccess)
          return TFS_CRC_EXIT_DEVICE_ERROR;
      ec->read_up += plan.up;
    }
    // one buffer behind the members: [compact out][jobs][crc][status][n_bad]
    const uint64_t o_jobs = (plan.down + 255) & ~uint64_t(255), o_crc = o_jobs + 32ull * m, o_st = o_crc + 4ull * m,
                   o_bad = o_st + 4ull * m;
    if ((rc = grow(ec, &ec->read_buf, &ec->read_cap, o_bad + 4))) return rc;
    char* rb = static_cast<char*>(ec->read_buf);
    if (hipMemcpyAsync(rb + o_jobs, plan.jobs.data(), 32ull * m, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(rb + o_bad, 0, 4, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
    rc = launch_read(ec, dm.data(), int(plan.up), row, rb + o_jobs, m, rb, plan.down,
                     reinterpret_cast<uint32_t*>(rb + o_crc), reinterpret_cast<int32_t*>(rb + o_st),
                     reinterpret_cast<uint32_t*>(rb + o_bad), st);
    if (rc) return rc;
    std::vector<uint32_t> res(2 * size_t(m) + 1);  // crc, status and n_bad lie back to back
    if (hipMemcpyAsync(res.data(), rb + o_crc, 8ull * m + 4, hipMemcpyDeviceToHost, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
    for (const ReadCopy& c : plan.copies)
      if (hipMemcpyAsync(static_cast<char*>(out) + c.dst, rb + c.src, size_t(c.len), hipMemcpyDeviceToHost, st) !=
          hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
    ec->read_down = plan.down;
    for (uint32_t k = 0; k < m; ++k) {
      out_crc[plan.index[k]] = res[k];
      out_status[plan.index[k]] = int32_t(res[m + k]);
    }
    bad += res[2 * size_t(m)];
  }
  if (n_bad) *n_bad += bad;
  return TFS_SUCCESS;
}

// ---- degraded read reply (include/tfs_ec_read.h) ------------------------------

int tfs_ec_read_reply_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, int target,
                             const tfs_ec_reply_job* jobs, uint32_t n, void* d_out, uint64_t out_cap,
                             tfs_read_result* d_results, uint32_t* d_n_bad, void* stream) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  int row = -1;
  const int rc = check_read(ec, d_members, sizes, size, target, &row);
  if (rc) return rc;
  if (stream && static_cast<hipStream_t>(stream) == hipStreamPerThread) return TFS_EXIT_PARAMETER_ERROR;
  if (n == 0) return TFS_SUCCESS;
  if (!jobs || !d_out || !d_results) return TFS_EXIT_PARAMETER_ERROR;
  if (reply_spans_overlap(jobs, n, size, out_cap)) return TFS_EXIT_PARAMETER_ERROR;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  auto fill = [&](ReplyUnit* units) {
    tfscrc::ReadSeedMemo memo;
    for (uint32_t i = 0; i < n; ++i) units[i] = reply_make_unit(jobs[i], size, out_cap, &memo);
  };
  return reply_enqueue(ec, st, d_members, size, row, n, fill, d_out, out_cap, d_results, d_n_bad);
}

int tfs_ec_read_reply(tfs_ec* ec, char* const* members, const int* sizes, int size, int target,
                      const tfs_ec_reply_job* jobs, uint32_t n, void* out, uint64_t out_cap, tfs_read_result* results,
                      uint32_t* n_bad) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  int row = -1;
  int rc = check_read(ec, reinterpret_cast<void* const*>(members), sizes, size, target, &row);
  if (rc) return rc;
  ec->read_up = ec->read_down = 0;
  if (n == 0) return TFS_SUCCESS;
  if (!jobs || !out || !results) return TFS_EXIT_PARAMETER_ERROR;
  if (reply_spans_overlap(jobs, n, size, out_cap)) return TFS_EXIT_PARAMETER_ERROR;
  void* zout = nullptr;
  const bool out_zc = reply_pinned(out, &zout);
  ReplyPlan plan;
  make_reply_plan(jobs, n, size, out_cap, !out_zc, &plan);
  const int nm = ec->dn + ec->pn;
  hipStream_t st = static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  std::vector<void*> dm(nm, nullptr);
  for (int s : ec->dec.sources) {
    if ((rc = grow(ec, &ec->staging[s], &ec->staging_cap[s], std::max<uint64_t>(plan.up, uint64_t(kUnit))))) return rc;
    dm[s] = ec->staging[s];
    for (const ReplySpan& sp : plan.spans)
      if (hipMemcpyAsync(static_cast<char*>(dm[s]) + sp.cbase, members[s] + sp.start, size_t(sp.end - sp.start),
                         hipMemcpyHostToDevice, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    ec->read_up += plan.up;
  }
  // one device buffer and its page-locked twin: [frames as the plan placed them][results]
  const uint64_t o_res = out_zc ? 0 : (plan.down + 255) & ~uint64_t(255), total = o_res + 16ull * n;
  if ((rc = grow(ec, &ec->reply_out, &ec->reply_out_cap, total))) return rc;
  if (ec->reply_host_cap < total) {
    if (ec->reply_host) (void)hipHostFree(ec->reply_host);
    ec->reply_host = nullptr;
    ec->reply_host_cap = 0;
    const uint64_t want = (total + 0xFFFFu) & ~uint64_t(0xFFFF);
    if (hipHostMalloc(&ec->reply_host, want, hipHostMallocDefault) != hipSuccess) {
      ec->reply_host = nullptr;
      return TFS_EXIT_NO_MEMORY;
    }
    ec->reply_host_cap = want;
  }
  char* rb = static_cast<char*>(ec->reply_out);
  char* hb = static_cast<char*>(ec->reply_host);
  auto fill = [&](ReplyUnit* units) { memcpy(units, plan.units.data(), size_t(n) * sizeof(ReplyUnit)); };
  rc = reply_enqueue(ec, st, dm.data(), int(plan.up), row, n, fill, out_zc ? zout : rb, out_zc ? out_cap : plan.down,
                     reinterpret_cast<tfs_read_result*>(rb + o_res), nullptr);
  if (rc) return rc;
  if (hipMemcpyAsync(hb + o_res, rb + o_res, 16ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return TFS_CRC_EXIT_DEVICE_ERROR;
  const tfs_read_result* hr = reinterpret_cast<const tfs_read_result*>(hb + o_res);
  uint32_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) {
    results[i] = hr[i];
    bad += hr[i].status != TFS_SUCCESS ? 1u : 0u;
  }
  if (!out_zc) {
    // frame_len bytes of every frame come down; frames that fill their spans and lie one behind the other
    // in the staged output travel as one run, the placement padding between them included
    uint64_t a0 = 0, a1 = 0;  // the open run [a0, a1)
    bool open = false;
    auto flush = [&]() -> bool {
      if (open && a1 > a0) {
        if (hipMemcpyAsync(hb + a0, rb + a0, size_t(a1 - a0), hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        ec->read_down += a1 - a0;
      }
      open = false;
      return true;
    };
    for (uint32_t i = 0; i < n; ++i) {
      if (!hr[i].frame_len) continue;
      const uint64_t op = plan.opos[i];
      if (!open || op - a1 >= 16u) {
        if (!flush()) return TFS_CRC_EXIT_DEVICE_ERROR;
        a0 = op, open = true;
      }
      a1 = op + hr[i].frame_len;
      if (hr[i].frame_len != tfscrc::read_frame_cap(jobs[i].read) && !flush()) return TFS_CRC_EXIT_DEVICE_ERROR;
    }
    if (!flush() || hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
    for (uint32_t i = 0; i < n; ++i)
      if (hr[i].frame_len)
        memcpy(static_cast<char*>(out) + jobs[i].read.frame_offset, hb + plan.opos[i], hr[i].frame_len);
  } else {
    for (uint32_t i = 0; i < n; ++i) ec->read_down += hr[i].frame_len;
  }
  if (n_bad) *n_bad += bad;
  return bad ? TFS_EXIT_CHECK_CRC_ERROR : TFS_SUCCESS;
}

int tfs_ec_marshal_begin(tfs_ec* ec, const tfs_raw_meta* const* metas, const uint32_t* n_metas, const int* sizes,
                         int total, tfs_ec_marshal** out) {
  if (!ec || !out) return TFS_EXIT_PARAMETER_ERROR;
  *out = nullptr;
  if (!ec->enc.valid) return TFS_EXIT_MATRIX_INVALID;
  static_assert(sizeof(tfs_raw_meta) == sizeof(MarshalMeta), "raw meta layout");
  tfs_ec_marshal* m = new tfs_ec_marshal();
  const int rc = session_begin(ec, m, metas, n_metas, sizes, total);
  if (rc != TFS_SUCCESS) {
    delete m;
    return rc;
  }
  m->up = ec->enc.sources;  // the data members up, the parity down
  m->down = ec->enc.outputs;
  *out = m;
  return TFS_SUCCESS;
}

int tfs_ec_marshal_encode_device(tfs_ec_marshal* m, void* const* d_members, int offset, int len, void* stream) {
  return session_chunk(m, marshal_launch, d_members, offset, len, stream, false);
}

int tfs_ec_marshal_encode(tfs_ec_marshal* m, char* const* members, int offset, int len) {
  return session_chunk(m, marshal_launch, reinterpret_cast<void* const*>(members), offset, len, nullptr, true);
}

int tfs_ec_marshal_finish(tfs_ec_marshal* m, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad) {
  return session_finish(m, out_crc, out_status, n_bad, nullptr, nullptr, 0);
}

int tfs_ec_marshal_free(tfs_ec_marshal* m) { return session_free(m); }

int tfs_ec_reinstate_begin(tfs_ec* ec, const tfs_raw_meta* const* metas, const uint32_t* n_metas, const int* sizes,
                           int total, tfs_ec_reinstate** out) {
  if (!ec || !out) return TFS_EXIT_PARAMETER_ERROR;
  *out = nullptr;
  if (!ec->dec.valid) return TFS_EXIT_MATRIX_INVALID;
  if (ec->dec.outputs.empty()) return TFS_EXIT_PARAMETER_ERROR;  // nothing to reinstate
  for (int i = 0; i < ec->dn && metas && n_metas; ++i)
    if (ec->erased[size_t(i)] == -1 && n_metas[i] != 0) return TFS_EXIT_PARAMETER_ERROR;  // an unused member has no records
  tfs_ec_reinstate* r = new tfs_ec_reinstate();
  const int rc = session_begin(ec, r, metas, n_metas, sizes, total);
  if (rc != TFS_SUCCESS) {
    delete r;
    return rc;
  }
  r->up = ec->dec.sources;  // the decode plan's sources up, its outputs down; no other member is bound
  r->down = ec->dec.outputs;
  *out = r;
  return TFS_SUCCESS;
}

int tfs_ec_reinstate_decode_device(tfs_ec_reinstate* r, void* const* d_members, int offset, int len, void* stream) {
  return session_chunk(r, reinstate_launch, d_members, offset, len, stream, false);
}

int tfs_ec_reinstate_decode(tfs_ec_reinstate* r, char* const* members, int offset, int len) {
  return session_chunk(r, reinstate_launch, reinterpret_cast<void* const*>(members), offset, len, nullptr, true);
}

int tfs_ec_reinstate_finish(tfs_ec_reinstate* r, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad) {
  return tfs_ec_marshal_finish(r, out_crc, out_status, n_bad);  // the same fold over the same arrays
}

int tfs_ec_reinstate_free(tfs_ec_reinstate* r) { return session_free(r); }

uint64_t tfs_ec_frames_cap(const tfs_ec_frames_cfg* cfg, int len) {
  if (!cfg || len <= 0 || ecf_cfg_status(*cfg) != 0) return 0;
  return ecf_call_need(*cfg, len);
}

int tfs_ec_marshal_frames_device(tfs_ec_marshal* m, const tfs_ec_frames_cfg* cfg, void* const* d_members,
                                 void* const* d_out, uint64_t out_cap, int offset, int len, void* stream) {
  return session_frames(m, m && m->ec ? &m->ec->enc : nullptr, cfg, d_members, d_out, out_cap, offset, len, stream, false);
}

int tfs_ec_marshal_frames(tfs_ec_marshal* m, const tfs_ec_frames_cfg* cfg, char* const* members, char* const* out,
                          uint64_t out_cap, int offset, int len) {
  return session_frames(m, m && m->ec ? &m->ec->enc : nullptr, cfg, reinterpret_cast<void* const*>(members),
                        reinterpret_cast<void* const*>(out), out_cap, offset, len, nullptr, true);
}

int tfs_ec_reinstate_frames_device(tfs_ec_reinstate* r, const tfs_ec_frames_cfg* cfg, void* const* d_members,
                                   void* const* d_out, uint64_t out_cap, int offset, int len, void* stream) {
  return session_frames(r, r && r->ec ? &r->ec->dec : nullptr, cfg, d_members, d_out, out_cap, offset, len, stream, false);
}

int tfs_ec_reinstate_frames(tfs_ec_reinstate* r, const tfs_ec_frames_cfg* cfg, char* const* members, char* const* out,
                            uint64_t out_cap, int offset, int len) {
  return session_frames(r, r && r->ec ? &r->ec->dec : nullptr, cfg, reinterpret_cast<void* const*>(members),
                        reinterpret_cast<void* const*>(out), out_cap, offset, len, nullptr, true);
}

uint64_t tfs_ec_fetch_cap(const tfs_ec_frames_cfg* cfg, const tfs_ec_fetch_cfg* fcfg, int len) {
  if (!cfg || !fcfg || len <= 0 || ecf_cfg_status(*cfg) != 0 || ecx_cfg_status(*cfg, *fcfg) != 0) return 0;
  return ecx_call_need(*cfg, *fcfg, len);
}

int32_t tfs_ec_fetch_expect(const int* sizes, int dn, int total, int member, int offset, int requested) {
  if (!sizes || member < 0 || member >= TFS_EC_MAX_MEMBERS || dn < 0 || total < 0 || offset < 0 || requested < 0) return -1;
  return ecx_expect(ecx_block_len(sizes, dn, total, member), offset, requested);
}

int tfs_ec_fetch_parse(const void* frame, uint32_t avail, int32_t* out_n, int32_t* out_data_file_size) {
  return ecx_parse(frame, avail, out_n, out_data_file_size);
}

int tfs_ec_marshal_task_device(tfs_ec_marshal* m, const tfs_ec_frames_cfg* cfg, const tfs_ec_fetch_cfg* fcfg,
                               const void* const* d_in, void* const* d_out, uint64_t out_cap,
                               tfs_ec_fetch_result* d_results, int offset, int len, void* stream) {
  return session_task(m, m && m->ec ? &m->ec->enc : nullptr, cfg, fcfg, d_in, d_out, out_cap, d_results, offset, len,
                      stream, false);
}

int tfs_ec_marshal_task(tfs_ec_marshal* m, const tfs_ec_frames_cfg* cfg, const tfs_ec_fetch_cfg* fcfg,
                        const char* const* in, char* const* out, uint64_t out_cap, tfs_ec_fetch_result* results,
                        int offset, int len) {
  return session_task(m, m && m->ec ? &m->ec->enc : nullptr, cfg, fcfg, reinterpret_cast<const void* const*>(in),
                      reinterpret_cast<void* const*>(out), out_cap, results, offset, len, nullptr, true);
}

int tfs_ec_reinstate_task_device(tfs_ec_reinstate* r, const tfs_ec_frames_cfg* cfg, const tfs_ec_fetch_cfg* fcfg,
                                 const void* const* d_in, void* const* d_out, uint64_t out_cap,
                                 tfs_ec_fetch_result* d_results, int offset, int len, void* stream) {
  return session_task(r, r && r->ec ? &r->ec->dec : nullptr, cfg, fcfg, d_in, d_out, out_cap, d_results, offset, len,
                      stream, false);
}

int tfs_ec_reinstate_task(tfs_ec_reinstate* r, const tfs_ec_frames_cfg* cfg, const tfs_ec_fetch_cfg* fcfg,
                          const char* const* in, char* const* out, uint64_t out_cap, tfs_ec_fetch_result* results,
                          int offset, int len) {
  return session_task(r, r && r->ec ? &r->ec->dec : nullptr, cfg, fcfg, reinterpret_cast<const void* const*>(in),
                      reinterpret_cast<void* const*>(out), out_cap, results, offset, len, nullptr, true);
}

int tfs_ec_scrub_begin(tfs_ec* ec, const tfs_raw_meta* const* metas, const uint32_t* n_metas, const int* sizes, int total,
                       tfs_ec_scrub** out) {
  if (!ec || !out) return TFS_EXIT_PARAMETER_ERROR;
  *out = nullptr;
  if (!ec->enc.valid) return TFS_EXIT_MATRIX_INVALID;
  tfs_ec_scrub* c = new tfs_ec_scrub();
  // every word of pbad has one writer before finish reads it (finish demands [0, total)): nothing to clear
  const int rc = session_begin(ec, c, metas, n_metas, sizes, total, scrub_words, &c->d_units);
  if (rc != TFS_SUCCESS) {
    delete c;
    return rc;
  }
  const size_t pn = size_t(ec->pn), nt = c->plan.ntiles;
  c->d_map = reinterpret_cast<uint8_t*>(c->d_units + pn);
  c->d_pbad = c->d_units + pn + (pn * nt + 3) / 4;
  c->up = ec->enc.sources;  // every member up, nothing down: the pass writes no member byte
  c->up.insert(c->up.end(), ec->enc.outputs.begin(), ec->enc.outputs.end());
  *out = c;
  return TFS_SUCCESS;
}

// the chunk driver and the launch arguments are shared with the sessions that write members, hence the cast
int tfs_ec_scrub_check_device(tfs_ec_scrub* c, const void* const* d_members, int offset, int len, void* stream) {
  return session_chunk(c, scrub_launch, const_cast<void* const*>(d_members), offset, len, stream, false);
}

int tfs_ec_scrub_check(tfs_ec_scrub* c, const char* const* members, int offset, int len) {
  return session_chunk(c, scrub_launch, reinterpret_cast<void* const*>(const_cast<char* const*>(members)), offset, len,
                       nullptr, true);
}

int tfs_ec_scrub_finish(tfs_ec_scrub* c, uint32_t* out_crc, int32_t* out_status, uint32_t* n_bad,
                        uint32_t* out_parity_units, uint8_t* out_tile_map) {
  if (!c || !c->ec || c->next != c->total) return TFS_EXIT_PARAMETER_ERROR;
  tfs_ec_marshal* m = c;
  const size_t pn = size_t(m->ec->pn), nt = m->plan.ntiles;
  const bool want = out_parity_units || out_tile_map;
  std::vector<uint8_t> res(want ? 4 * pn + pn * nt : 0);  // units and map lie back to back, behind the statuses
  if (want) {
    hipStream_t st = m->stream_set ? m->stream : static_cast<hipStream_t>(tfs_crc32_stream(m->ec->ctx));
    ScrubCountArgs a;
    a.pbad = c->d_pbad;
    a.units = c->d_units;
    a.map = c->d_map;
    a.ntiles = uint32_t(nt);
    if (launch_ec_scrub_count(a, int(pn), st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  const int rc = session_finish(m, out_crc, out_status, n_bad, res.data(), c->d_units, res.size());
  if (rc != TFS_SUCCESS) return rc;
  if (out_parity_units) memcpy(out_parity_units, res.data(), 4 * pn);
  if (out_tile_map) memcpy(out_tile_map, res.data() + 4 * pn, pn * nt);
  return TFS_SUCCESS;
}

int tfs_ec_scrub_free(tfs_ec_scrub* c) { return session_free(c); }

int tfs_ec_locate_device(tfs_ec* ec, const void* const* d_members, int size, const uint32_t* units, uint32_t n,
                         void* d_result, void* d_fixed, void* stream) {
  int rc = locate_check(ec, d_members, size, units, n);
  if (rc) return rc;
  if (stream && static_cast<hipStream_t>(stream) == hipStreamPerThread) return TFS_EXIT_PARAMETER_ERROR;
  if (n == 0) return TFS_SUCCESS;
  if (!d_result) return TFS_EXIT_PARAMETER_ERROR;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  std::lock_guard<std::mutex> g(ec->mu);
  if ((rc = locate_plan(ec))) return rc;
  if (units && (rc = locate_upload_list(ec, units, n, st))) return rc;
  rc = locate_launch(ec, d_members, units ? static_cast<const uint32_t*>(ec->loc_list) : nullptr, n, d_result, d_fixed, st);
  if (rc == TFS_SUCCESS && units && hipEventRecord(ec->loc_done, st) != hipSuccess) rc = TFS_CRC_EXIT_DEVICE_ERROR;
  return rc;
}

int tfs_ec_locate(tfs_ec* ec, const char* const* members, int size, const uint32_t* units, uint32_t n,
                  tfs_ec_locate_result* result, char* fixed) {
  static_assert(sizeof(tfs_ec_locate_result) == sizeof(LocateResult), "locate result layout");
  int rc = locate_check(ec, reinterpret_cast<const void* const*>(members), size, units, n);
  if (rc) return rc;
  if (n == 0) return TFS_SUCCESS;
  if (!result) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  if ((rc = locate_plan(ec))) return rc;
  const int nm = ec->dn + ec->pn;
  hipStream_t st = static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  const uint32_t piece = n < ec->loc_piece ? n : ec->loc_piece;
  const uint64_t pbytes = uint64_t(piece) * kUnit, o_fixed = (8ull * piece + 255) & ~uint64_t(255);
  for (int i = 0; i < nm; ++i)
    if ((rc = grow(ec, &ec->staging[i], &ec->staging_cap[i], pbytes))) return rc;
  if ((rc = grow(ec, &ec->loc_out, &ec->loc_out_cap, o_fixed + (fixed ? pbytes : 0)))) return rc;
  char* const d_out = static_cast<char*>(ec->loc_out);
  std::vector<char> gather(size_t(nm) * pbytes), down(fixed ? size_t(pbytes) : 0);
  for (uint32_t k0 = 0; k0 < n; k0 += piece) {
    const uint32_t cnt = n - k0 < piece ? n - k0 : piece;
    const size_t cbytes = size_t(cnt) * kUnit;
    for (int i = 0; i < nm; ++i) {  // the listed units of member i, side by side
      char* gm = gather.data() + size_t(i) * pbytes;
      if (units) {
        for (uint32_t k = 0; k < cnt; ++k) memcpy(gm + size_t(k) * kUnit, members[i] + size_t(units[k0 + k]) * kUnit, kUnit);
      } else {
        memcpy(gm, members[i] + size_t(k0) * kUnit, cbytes);
      }
      if (hipMemcpyAsync(ec->staging[i], gm, cbytes, hipMemcpyHostToDevice, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    }
    if ((rc = locate_launch(ec, ec->staging.data(), nullptr, cnt, d_out, fixed ? d_out + o_fixed : nullptr, st))) return rc;
    if (hipMemcpyAsync(result + k0, d_out, 8ull * cnt, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (fixed && hipMemcpyAsync(down.data(), d_out + o_fixed, cbytes, hipMemcpyDeviceToHost, st) != hipSuccess))
      return TFS_CRC_EXIT_DEVICE_ERROR;
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;  // the gather buffer is free again
    for (uint32_t k = 0; fixed && k < cnt; ++k)  // only the slots of DATA entries were written on the device
      if (result[k0 + k].kind == TFS_EC_LOCATE_DATA)
        memcpy(fixed + size_t(k0 + k) * kUnit, down.data() + size_t(k) * kUnit, kUnit);
  }
  return TFS_SUCCESS;
}

int tfs_ec_update_device(tfs_ec* ec, int member, void* const* d_parity, int size, const uint32_t* units, uint32_t n,
                         const void* d_a, const void* d_b, void* stream) {
  int rc = update_check(ec, member, d_parity, size, units, n);
  if (rc) return rc;
  if (stream && static_cast<hipStream_t>(stream) == hipStreamPerThread) return TFS_EXIT_PARAMETER_ERROR;
  if (n == 0) return TFS_SUCCESS;
  if (!d_a) return TFS_EXIT_PARAMETER_ERROR;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  std::lock_guard<std::mutex> g(ec->mu);
  if (!units || n <= kUpdateInline) return update_launch(ec, member, d_parity, units, nullptr, n, d_a, d_b, st);
  if ((rc = locate_upload_list(ec, units, n, st))) return rc;
  rc = update_launch(ec, member, d_parity, nullptr, static_cast<const uint32_t*>(ec->loc_list), n, d_a, d_b, st);
  if (rc == TFS_SUCCESS && hipEventRecord(ec->loc_done, st) != hipSuccess) rc = TFS_CRC_EXIT_DEVICE_ERROR;
  return rc;
}

int tfs_ec_update(tfs_ec* ec, int member, char* const* parity, int size, const uint32_t* units, uint32_t n, const char* a,
                  const char* b) {
  int rc = update_check(ec, member, reinterpret_cast<const void* const*>(parity), size, units, n);
  if (rc) return rc;
  if (n == 0) return TFS_SUCCESS;
  if (!a) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  const int dn = ec->dn, pn = ec->pn;
  hipStream_t st = static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  const uint32_t piece = n < ec->upd_piece ? n : ec->upd_piece;
  const uint64_t pbytes = uint64_t(piece) * kUnit;
  std::vector<void*> dpar(size_t(pn), nullptr);  // parity p's listed units, side by side, in its staging buffer
  for (int p = 0; p < pn; ++p) {
    if (!parity[p]) continue;
    if ((rc = grow(ec, &ec->staging[dn + p], &ec->staging_cap[dn + p], pbytes))) return rc;
    dpar[size_t(p)] = ec->staging[dn + p];
  }
  if ((rc = grow(ec, &ec->upd_buf, &ec->upd_buf_cap, 2 * pbytes))) return rc;
  char* const d_a = static_cast<char*>(ec->upd_buf);
  char* const d_b = b ? d_a + pbytes : nullptr;
  std::vector<char> gather(units ? size_t(pn) * pbytes : 0);  // up, and down again into the same rows
  for (uint32_t k0 = 0; k0 < n; k0 += piece) {
    const uint32_t cnt = n - k0 < piece ? n - k0 : piece;
    const size_t cbytes = size_t(cnt) * kUnit;
    if (hipMemcpyAsync(d_a, a + size_t(k0) * kUnit, cbytes, hipMemcpyHostToDevice, st) != hipSuccess ||
        (b && hipMemcpyAsync(d_b, b + size_t(k0) * kUnit, cbytes, hipMemcpyHostToDevice, st) != hipSuccess))
      return TFS_CRC_EXIT_DEVICE_ERROR;
    for (int p = 0; p < pn; ++p) {
      if (!parity[p]) continue;
      const char* up = parity[p] + size_t(k0) * kUnit;  // the dense form: the units lie side by side already
      if (units) {
        char* gm = gather.data() + size_t(p) * pbytes;
        for (uint32_t k = 0; k < cnt; ++k) memcpy(gm + size_t(k) * kUnit, parity[p] + size_t(units[k0 + k]) * kUnit, kUnit);
        up = gm;
      }
      if (hipMemcpyAsync(dpar[size_t(p)], up, cbytes, hipMemcpyHostToDevice, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    }
    if ((rc = update_launch(ec, member, dpar.data(), nullptr, nullptr, cnt, d_a, d_b, st))) return rc;
    for (int p = 0; p < pn; ++p) {
      if (!parity[p]) continue;
      char* down = units ? gather.data() + size_t(p) * pbytes : parity[p] + size_t(k0) * kUnit;
      if (hipMemcpyAsync(down, dpar[size_t(p)], cbytes, hipMemcpyDeviceToHost, st) != hipSuccess)
        return TFS_CRC_EXIT_DEVICE_ERROR;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;  // the gather buffer is free again
    for (int p = 0; units && p < pn; ++p) {
      if (!parity[p]) continue;
      const char* gm = gather.data() + size_t(p) * pbytes;
      for (uint32_t k = 0; k < cnt; ++k) memcpy(parity[p] + size_t(units[k0 + k]) * kUnit, gm + size_t(k) * kUnit, kUnit);
    }
  }
  return TFS_SUCCESS;
}

int tfs_ec_update_set_piece(tfs_ec* ec, uint32_t units) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  ec->upd_piece = units ? units : 4096u;
  return TFS_SUCCESS;
}

int tfs_ec_locate_set_piece(tfs_ec* ec, uint32_t units) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  ec->loc_piece = units ? units : 4096u;
  return TFS_SUCCESS;
}

int tfs_ec_read_traffic(tfs_ec* ec, uint64_t* up, uint64_t* down) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  std::lock_guard<std::mutex> g(ec->mu);
  if (up) *up = ec->read_up;
  if (down) *down = ec->read_down;
  return TFS_SUCCESS;
}

int tfs_ec_config(tfs_crc_ctx* ctx, int dn, int pn, const int* erased, tfs_ec** out) {
  if (!ctx || !out) return TFS_EXIT_PARAMETER_ERROR;
  *out = nullptr;
  if (dn <= 0 || pn <= 0 || dn + pn > kMaxMembers) return TFS_EXIT_PARAMETER_ERROR;
  tfs_ec* ec = new tfs_ec();
  ec->ctx = ctx;
  ec->dn = dn;
  ec->pn = pn;
  ec->staging.assign(size_t(dn + pn), nullptr);
  ec->staging_cap.assign(size_t(dn + pn), 0);
#ifdef TFS_CRC_MEASURE
  if (const char* v = getenv("TFS_EC_VARIANT")) ec->variant = atoi(v);
#endif
  *out = ec;
  std::vector<int> data(dn), parity(pn);
  for (int j = 0; j < dn; ++j) data[j] = j;
  for (int i = 0; i < pn; ++i) parity[i] = dn + i;
  int rc = upload_plan(ec, &ec->enc, data, parity, encode_bitmatrix(dn, pn));
  if (rc == TFS_SUCCESS && erased) {
    DecodePlan dp;
    ec->erased.assign(erased, erased + dn + pn);
    const int r = make_decode_plan(dn, pn, erased, &dp);
    if (r == -1) rc = TFS_EXIT_NO_ENOUGH_DATA;
    else if (r == -2) rc = TFS_EXIT_MATRIX_INVALID;
    else rc = upload_plan(ec, &ec->dec, dp.sources, dp.outputs, dp.rows);
    if (rc == TFS_SUCCESS) rc = upload_read_tables(ec);
  }
  ec->config_rc = rc;
  return rc;
}

int tfs_ec_free(tfs_ec* ec) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  (void)hipStreamSynchronize(static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx)));
  if (ec->enc.d_masks) tfs_crc32_dev_free(ec->ctx, ec->enc.d_masks);
  if (ec->dec.d_masks) tfs_crc32_dev_free(ec->ctx, ec->dec.d_masks);
  if (ec->d_read_tab) tfs_crc32_dev_free(ec->ctx, ec->d_read_tab);
  if (ec->read_buf) tfs_crc32_dev_free(ec->ctx, ec->read_buf);
  if (ec->d_marshal_tab) tfs_crc32_dev_free(ec->ctx, ec->d_marshal_tab);
  if (ec->loc_busy) (void)hipEventSynchronize(ec->loc_done);  // a locate call on a caller's stream
  if (ec->d_locate) tfs_crc32_dev_free(ec->ctx, ec->d_locate);
  if (ec->loc_list) tfs_crc32_dev_free(ec->ctx, ec->loc_list);
  if (ec->loc_out) tfs_crc32_dev_free(ec->ctx, ec->loc_out);
  if (ec->upd_buf) tfs_crc32_dev_free(ec->ctx, ec->upd_buf);
  for (tfs_ec::ReplySlot& sl : ec->reply_slots) {
    if (sl.done) {
      (void)hipEventSynchronize(sl.done);  // a reply call on a caller's stream
      (void)hipEventDestroy(sl.done);
    }
    if (sl.h) (void)hipHostFree(sl.h);
    if (sl.d) tfs_crc32_dev_free(ec->ctx, sl.d);
  }
  if (ec->reply_out) tfs_crc32_dev_free(ec->ctx, ec->reply_out);
  if (ec->reply_host) (void)hipHostFree(ec->reply_host);
  if (ec->loc_pin) (void)hipHostFree(ec->loc_pin);
  if (ec->loc_copied) (void)hipEventDestroy(ec->loc_copied);
  if (ec->loc_done) (void)hipEventDestroy(ec->loc_done);
  for (void* p : ec->staging)
    if (p) tfs_crc32_dev_free(ec->ctx, p);
  delete ec;
  return TFS_SUCCESS;
}

int tfs_ec_encode_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, void* stream) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  const int rc = check_call(ec, ec->enc, d_members, sizes, size);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  return run_plan(ec, ec->enc, d_members, size, st);
}

int tfs_ec_decode_device(tfs_ec* ec, void* const* d_members, const int* sizes, int size, void* stream) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  const int rc = check_call(ec, ec->dec, d_members, sizes, size);
  if (rc) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  return run_plan(ec, ec->dec, d_members, size, st);
}

int tfs_ec_encode(tfs_ec* ec, char* const* members, const int* sizes, int size) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  return run_host(ec, ec->enc, members, sizes, size);
}

int tfs_ec_decode(tfs_ec* ec, char* const* members, const int* sizes, int size) {
  if (!ec) return TFS_EXIT_PARAMETER_ERROR;
  return run_host(ec, ec->dec, members, sizes, size);
}

}  // extern "C"
