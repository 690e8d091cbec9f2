// read_reply_plan_check.cpp -- stand-alone check of tfs_amd/csrc/read_reply_plan.h, the host
// arithmetic of the read replies (include/tfs_read.h): n, body length, span and
// pre-shifted seed against a byte-wise loop, the statuses decided before reading,
// the out_cap and span-overlap checks, and offsets past 4 GiB.  No device.  Built
// and run by tests/test_read_math.py under the host's address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tfs_amd/csrc/read_reply_plan.h"

using namespace tfscrc;

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

static uint32_t crc_loop(uint32_t c, const std::vector<uint8_t>& b) {  // func.cpp:429-433
  return b.empty() ? c : read_crc_bytes(c, b.data(), uint32_t(b.size()));
}

static tfs_read_job job(uint64_t so, uint64_t fo, int32_t size, int32_t ro, int32_t rl, int16_t pcode) {
  tfs_read_job j{};
  j.src_offset = so, j.frame_offset = fo, j.file_id = 7, j.packet_id = 9;
  j.size = size, j.read_offset = ro, j.read_len = rl, j.pcode = pcode, j.version = 2;
  return j;
}

int main() {
  uint32_t njobs = 0, nspans = 0;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&] {
    rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
    return rng;
  };
  const int16_t pcodes[3] = {8, 39, 63};
  const int32_t payloads[] = {0, 1, 3, 4, 31, 32, 1023, 1024, 1025, 65536, 70001};
  const uint64_t big = 1ull << 40;
  for (int32_t pl : payloads)
    for (int16_t pc : pcodes)
      for (int32_t ro : {0, 1, 36, pl}) {
        if (ro > pl) continue;
        for (int32_t rl : {0, 1, pl - ro, pl - ro + 5, pl + 100}) {
          if (rl < 0) continue;
          const tfs_read_job j = job(100, 200, pl + 36, ro, rl, pc);
          ++njobs;
          // n, body and span by the definition in tfs_read.h
          const int64_t left = int64_t(pl) - ro;
          const uint32_t n = uint32_t(rl < left ? rl : left);
          const uint32_t tl = pc == 8 ? 0u : (ro == 0 ? 40u : 4u);
          CHECK(read_n(j) == n);
          CHECK(read_body_len(j) == 4u + n + tl);
          CHECK(read_frame_cap(j) == 28u + n + tl);
          CHECK(read_frame_cap(j) >= read_fail_len(pc));
          CHECK(read_pre_status(j, big, big) == 0);
          const ReadUnit u = read_make_unit(j, big, big);
          CHECK(u.n == n && u.roff == uint32_t(ro) && u.tlen == tl && u.pre == 0);
          CHECK(u.whole == uint32_t(ro == 0 && n == uint32_t(pl)));
          CHECK(u.type_ver == (uint32_t(pc) | 2u << 16));
          // crc(FLAG, le32(n) || D) == pre_seed ^ crc(0, D), byte by byte
          std::vector<uint8_t> d(n), body;
          for (auto& b : d) b = uint8_t(next());
          for (int k = 0; k < 4; ++k) body.push_back(uint8_t(n >> (8 * k)));
          body.insert(body.end(), d.begin(), d.end());
          CHECK(crc_loop(kReadFlag, body) == (u.pre_seed ^ crc_loop(0u, d)));
        }
      }
  // statuses decided before reading, in the header's order
  CHECK(read_pre_status(job(0, 0, 100, 0, 10, 9), big, big) == kReadParameterError);   // pcode
  CHECK(read_frame_cap(job(0, 0, 100, 0, 10, 9)) == 0u);
  CHECK(read_pre_status(job(0, 0, 100, -1, 10, 8), big, big) == kReadParameterError);  // negative offset
  CHECK(read_pre_status(job(0, 0, 100, 0, -1, 8), big, big) == kReadParameterError);   // negative length
  CHECK(read_pre_status(job(0, 0, 100, 65, 1, 8), big, big) == kReadParameterError);   // past the payload
  CHECK(read_pre_status(job(0, 0, 100, 64, 1, 8), big, big) == 0);                     // at its end: n = 0
  CHECK(read_n(job(0, 0, 100, 64, 1, 8)) == 0u);
  CHECK(read_pre_status(job(0, 0, 35, 0, 1, 8), big, big) == kReadSizeError);
  CHECK(read_pre_status(job(0, 0, 35, 1, 1, 8), big, big) == kReadParameterError);
  CHECK(read_pre_status(job(0, 0, 36, 0, 1, 39), big, big) == 0);                      // an empty file is served
  CHECK(read_frame_cap(job(0, 0, 36, 0, 1, 39)) == 68u && read_frame_cap(job(0, 0, 35, 0, 1, 39)) == 68u);
  CHECK(read_pre_status(job(0, 0, -5, 0, 1, 8), big, big) == kReadSizeError);
  CHECK(read_pre_status(job(1, 0, 100, 0, 1, 8), 100, big) == kReadParameterError);    // the record passes src_len
  CHECK(read_pre_status(job(0, 0, 100, 0, 1, 8), 100, big) == 0);
  CHECK(read_pre_status(job(0, 1, 100, 0, 64, 8), big, 92) == kReadParameterError);    // the span passes out_cap
  CHECK(read_pre_status(job(0, 0, 100, 0, 64, 8), big, 92) == 0);
  CHECK(read_pre_status(job(~0ull, 0, 100, 0, 64, 8), big, big) == kReadParameterError);  // no wrap-around
  CHECK(read_pre_status(job(0, ~0ull - 3, 100, 0, 64, 8), big, ~0ull) == kReadParameterError);
  // the three wrapped ranges of the device tests: 2^64 - 200 with 300 and with 20,000 bytes (the sums are 100
  // and 19,800), 2^64 - 1 with 37; against a short length, one over 4 GiB and the largest
  for (uint64_t len : {uint64_t(4096), uint64_t((5ull << 30) + 4096 + 7), uint64_t(~0ull)}) {
    CHECK(read_pre_status(job(~0ull - 199, 0, 300, 0, 264, 8), len, big) == kReadParameterError);
    CHECK(read_pre_status(job(~0ull - 199, 0, 20000, 0, 19964, 39), len, big) == kReadParameterError);
    CHECK(read_pre_status(job(~0ull, 0, 37, 0, 1, 63), len, big) == kReadParameterError);
    CHECK(read_pre_status(job(0, ~0ull - 199, 300, 0, 264, 8), big, len) == kReadParameterError);
    CHECK(read_pre_status(job(0, ~0ull - 199, 20000, 0, 19964, 39), big, len) == kReadParameterError);
    CHECK(read_pre_status(job(0, ~0ull, 37, 0, 1, 63), big, len) == kReadParameterError);
  }
  // offsets past 4 GiB
  {
    const uint64_t so = (5ull << 30) + 3, fo = (6ull << 30) + 1;
    const tfs_read_job j = job(so, fo, 1036, 0, 1000, 63);
    CHECK(read_pre_status(j, so + 1036, fo + 1068) == 0);
    CHECK(read_pre_status(j, so + 1035, fo + 1068) == kReadParameterError);
    CHECK(read_pre_status(j, so + 1036, fo + 1067) == kReadParameterError);
    const ReadUnit u = read_make_unit(j, so + 1036, fo + 1068);
    CHECK(u.soff == so && u.doff == fo && u.n == 1000u && u.tlen == 40u && u.whole == 1u);
    ++njobs;
  }
  // span overlap: back to back is fine, one shared byte is not; refused jobs do not count
  {
    std::vector<tfs_read_job> v;
    uint64_t fo = (4ull << 30) - 50;  // straddles 4 GiB
    for (int k = 0; k < 40; ++k) {
      v.push_back(job(0, fo, 36 + k, 0, k, pcodes[k % 3]));
      fo += read_frame_cap(v.back());
    }
    std::vector<tfs_read_job> w(v.rbegin(), v.rend());  // any order
    CHECK(!read_spans_overlap(w.data(), uint32_t(w.size()), big, big));
    ++nspans;
    for (size_t k = 1; k < w.size(); k += 7) {
      std::vector<tfs_read_job> x = w;
      x[k].frame_offset -= 1;
      CHECK(read_spans_overlap(x.data(), uint32_t(x.size()), big, big));
      x[k].pcode = 5;  // refused: writes nothing, overlaps nothing
      CHECK(!read_spans_overlap(x.data(), uint32_t(x.size()), big, big));
      x[k].pcode = 8;
      x[k].frame_offset = big;  // its span passes out_cap: refused
      CHECK(!read_spans_overlap(x.data(), uint32_t(x.size()), big, big));
      nspans += 3;
    }
    std::vector<tfs_read_job> same = {job(0, 10, 36, 0, 0, 8), job(0, 10, 36, 0, 0, 8)};
    CHECK(read_spans_overlap(same.data(), 2, big, big));
    CHECK(!read_spans_overlap(same.data(), 1, big, big));
    CHECK(!read_spans_overlap(nullptr, 0, big, big));
    nspans += 3;
  }
  if (g_fail) return 1;
  std::printf("read plan ok: %u jobs, %u span lists\n", njobs, nspans);
  return 0;
}
