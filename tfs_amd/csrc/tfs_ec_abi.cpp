// tfs_ec_abi.cpp -- host side of include/tfs_ec.h: ErasureCode's setup on the
// host (ec_math.h), the region work on the GPU (tfs_ec_kernels.hip).  No CPU
// fallback: without a device every call fails with the ctx's error.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/tfs_ec.h"
#include "crc_math.h"
#include "ec_math.h"

#include "ec_read_plan.h"
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
  std::vector<void*> staging;  // host-form device buffers (dn+pn), grown on demand
  std::vector<uint64_t> staging_cap;
  int variant = 0;  // kernel form (TFS_EC_VARIANT at creation, measurement knob; 0 = product)
  tfsec::ReadTables* d_read_tab = nullptr;  // degraded read: set with the decode plan
  void* read_buf = nullptr;                 // host form: compact output, jobs and results
  uint64_t read_cap = 0;
  uint64_t read_up = 0, read_down = 0;      // member / output bytes the last host-form read moved
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

int run_plan(tfs_ec* ec, const Plan& p, void* const* members, int size, hipStream_t st) {
  const uint64_t units = uint64_t(size) / kUnit;
  if (units == 0 || p.outputs.empty()) return TFS_SUCCESS;
  const int S = int(p.sources.size());
  for (size_t o0 = 0; o0 < p.outputs.size(); o0 += 4) {
    const int og = int(std::min<size_t>(4, p.outputs.size() - o0));
    EcArgs a;
    memset(&a, 0, sizeof a);
    for (int s = 0; s < S; ++s) a.src[s] = static_cast<const uint8_t*>(members[p.sources[s]]);
    for (int o = 0; o < og; ++o) a.dst[o] = static_cast<uint8_t*>(members[p.outputs[o0 + o]]);
    a.masks = p.d_masks + o0 * 8 * size_t(S) * 8;
    a.S = uint32_t(S);
    a.units = units;
    if (launch_ec_apply(a, og, ec->variant, st) != hipSuccess) return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  return TFS_SUCCESS;
}

// Host form: members staged through device buffers; sources up, outputs down.
int run_host(tfs_ec* ec, const Plan& p, char* const* members, const int* sizes, int size) {
  std::lock_guard<std::mutex> g(ec->mu);
  void* const* mv = reinterpret_cast<void* const*>(members);
  int rc = check_call(ec, p, mv, sizes, size);
  if (rc) return rc;
  const int n = ec->dn + ec->pn;
  if (ec->staging.empty()) {
    ec->staging.assign(n, nullptr);
    ec->staging_cap.assign(n, 0);
  }
  hipStream_t st = static_cast<hipStream_t>(tfs_crc32_stream(ec->ctx));
  std::vector<void*> dm(n, nullptr);
  auto need = [&](int i) -> int {
    if (ec->staging_cap[i] < uint64_t(size)) {
      if (ec->staging[i]) tfs_crc32_dev_free(ec->ctx, ec->staging[i]);
      ec->staging[i] = nullptr;
      ec->staging_cap[i] = 0;
      const int r = tfs_crc32_dev_malloc(ec->ctx, uint64_t(size) + 64, &ec->staging[i]);
      if (r) return r;
      ec->staging_cap[i] = uint64_t(size);
    }
    dm[i] = ec->staging[i];
    return TFS_SUCCESS;
  };
  for (int s : p.sources) {
    if ((rc = need(s))) return rc;
    if (hipMemcpyAsync(dm[s], members[s], size_t(size), hipMemcpyHostToDevice, st) != hipSuccess)
      return TFS_CRC_EXIT_DEVICE_ERROR;
  }
  for (int o : p.outputs)
    if ((rc = need(o))) return rc;
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
    if (ec->staging.empty()) {
      ec->staging.assign(nm, nullptr);
      ec->staging_cap.assign(nm, 0);
    }
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
