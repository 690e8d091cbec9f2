// replicate_plan_check.cpp -- stand-alone check of tfs_amd/csrc/replicate_plan.h
// (no device, no Python): built and run by tests/test_replicate_plan.py under the
// host's address and undefined-behaviour sanitizers.
//
// For a few hundred seeded layouts: the units partition [0, total); no unit
// crosses a frame, FileInfo-start, payload-start or record-end cut, nor is longer
// than kRepSeg allows; every record's payload units sum to size - 36; the slices
// of any legal sequence of calls are contiguous in the source and land where the
// frames lie; and the fold the device does -- seed ^ XOR of the units' CRCs times
// their multipliers -- gives Func::crc(FLAG, body) of every frame and
// Func::crc(0, payload) of every record, computed here byte by byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tfs_amd/csrc/replicate_plan.h"

using namespace tfscrc;

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      if (g_fail++ < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                             \
  } while (0)

static uint64_t g_rng = 1;
static uint32_t rnd() {
  g_rng += 0x9E3779B97F4A7C15ull;
  uint64_t z = g_rng;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return uint32_t((z ^ (z >> 31)) >> 16);
}
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }

static uint32_t g_tab[256];
static uint32_t crc_of(uint32_t c, const uint8_t* p, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) c = (c >> 8) ^ g_tab[(c ^ p[i]) & 0xffu];
  return c;
}

static tfs_replicate_cfg cfg_of(int32_t total, int32_t frame_len) {
  tfs_replicate_cfg c{};
  c.packet_id = 0x1122334455667700ull + rnd() % 7;
  c.block_id = rnd();
  c.total = total, c.frame_len = frame_len;
  c.new_block = rnd() & 1 ? TFS_RAW_NORMAL_DATA : TFS_RAW_PARITY_DATA;
  c.version = 2;
  return c;
}

static uint32_t g_units = 0, g_layouts = 0, g_calls = 0;

static void check_layout(uint32_t seed) {
  g_rng = 0xC0FFEEull * (seed + 1);
  static const int32_t kFrames[] = {1024, 1024, 2048, 4096, 65536, 1 << 20};
  const int32_t fl = kFrames[rnd() % 6];
  // records and gaps: tiny payloads, FileInfos across cuts, long records, rejected ones
  std::vector<tfs_raw_meta> metas;
  std::vector<int32_t> expect_early;
  int64_t pos = 0;
  const uint32_t nrec = rnd() % 24;
  const bool big = fl >= 65536 && (seed % 5 == 0);
  for (uint32_t i = 0; i < nrec; ++i) {
    const uint32_t kind = rnd() % 10;
    if (kind < 4) pos += rnd() % 3 == 0 ? rnd_in(1, 3 * uint32_t(fl) / 2) : rnd_in(1, 90);
    if (kind == 9 && pos > 100) {  // a record rejected at begin: too short, lying anywhere (overlap allowed)
      metas.push_back(tfs_raw_meta{rnd(), int32_t(rnd() % uint32_t(pos)), int32_t(rnd() % 37)});
      expect_early.push_back(kRepSizeError);
      continue;
    }
    uint32_t size = 36 + (rnd() % 3 == 0 ? 1 : rnd_in(1, 5000));
    if (rnd() % 6 == 0) size = 36 + rnd_in(1, 3 * uint32_t(fl) + 77);
    if (big && i == 3) size = 36 + 200000 + rnd() % 99;
    if (rnd() % 5 == 0) pos += (fl - (pos + rnd_in(0, 36)) % fl) % fl;  // FileInfo on or across a frame cut
    metas.push_back(tfs_raw_meta{uint64_t(rnd()) << 32 | rnd(), int32_t(pos), int32_t(size)});
    expect_early.push_back(0);
    pos += size;
    if (pos > (48 << 20)) break;
  }
  int64_t total = pos + (rnd() % 2 ? rnd_in(0, 2 * uint32_t(fl)) : 0);
  if (seed % 17 == 0) total = pos = 0, metas.clear(), expect_early.clear();
  if (seed % 13 == 0 && !metas.empty()) {  // one past the end
    metas.push_back(tfs_raw_meta{7, int32_t(total - 10), 100});
    expect_early.push_back(kRepParameterError);
  }
  const tfs_replicate_cfg c = cfg_of(int32_t(total), fl);
  RepPlan p;
  CHECK(make_replicate_plan(c, metas.data(), uint32_t(metas.size()), &p) == 0);
  CHECK(p.early == expect_early);
  CHECK(p.nframes == rep_frame_count(total, fl) && p.frame_first.size() == size_t(p.nframes) + 1);
  ++g_layouts;
  g_units += uint32_t(p.units.size());

  // partition, cuts, sums
  int64_t at = 0;
  std::vector<int64_t> paysum(p.recs.size(), 0);
  std::vector<uint64_t> infomask(p.recs.size(), 0);
  uint32_t k = 0;
  for (const RepUnit& u : p.units) {
    CHECK(int64_t(u.soff) == at);
    const int64_t b = at, e = at + u.hlen + u.plen;
    CHECK(e > b && u.hlen <= kRepInfo && u.plen <= kRepSeg);
    CHECK(b / fl == (e - 1) / fl && u.frame == uint32_t(b / fl));
    CHECK(p.frame_first[u.frame] <= k && k < p.frame_first[u.frame + 1]);
    if (u.rec == kRepNoRec) {
      CHECK(u.hlen == 0);
      for (const RepRec& r : p.recs) CHECK(e <= r.offset || b >= int64_t(r.offset) + r.size);
    } else {
      CHECK(u.rec < p.recs.size());
      const RepRec& r = p.recs[u.rec];
      CHECK(b >= r.offset && e <= int64_t(r.offset) + r.size);
      if (u.hlen) {
        CHECK(b == r.offset + int64_t(u.hk) && u.hk + u.hlen <= kRepInfo);
        CHECK(u.plen == 0 || u.hk + u.hlen == kRepInfo);
        for (uint32_t i = 0; i < u.hlen; ++i) infomask[u.rec] |= 1ull << (u.hk + i);
      } else {
        CHECK(b >= int64_t(r.offset) + kRepInfo);
      }
      paysum[u.rec] += u.plen;
    }
    at = e;
    ++k;
  }
  CHECK(at == total);
  for (size_t r = 0; r < p.recs.size(); ++r) {
    CHECK(paysum[r] == int64_t(p.recs[r].size) - kRepInfo);
    CHECK(infomask[r] == (1ull << 36) - 1);
  }

  // the image, and the fold as the device does it
  std::vector<uint8_t> img(size_t(total) + 1);
  for (auto& x : img) x = uint8_t(rnd());
  std::vector<uint32_t> racc(p.recs.size(), 0);
  // a random legal sequence of calls
  const uint64_t stride = rep_stride(c) + (rnd() % 2 ? 0 : rnd_in(0, 100));
  int64_t next = 0;
  bool done = false;
  std::vector<RepFrame> fr;
  std::vector<RepUnit> un;
  while (total == 0 ? !done : next < total) {
    CHECK(!rep_call_ok(p, next, done, next + fl, fl) && !rep_call_ok(p, next, done, next, -1));
    if (next > 0) CHECK(!rep_call_ok(p, next, done, next - fl, fl));
    if (total - next > 1) CHECK(!rep_call_ok(p, next, done, next, 1));
    CHECK(!rep_call_ok(p, next, done, next, total - next + 1));
    const int64_t left = total - next;
    const int64_t nfl = (left + fl - 1) / fl;
    int64_t len = int64_t(rnd_in(1, uint32_t(std::max<int64_t>(nfl, 1)))) * fl;
    if (len > left) len = left;
    CHECK(rep_call_ok(p, next, done, next, len));
    const uint32_t f0 = uint32_t(next / fl), nf = rep_call_frames(p, len), nu = rep_slice_units(p, f0, nf);
    fr.assign(nf, RepFrame{});
    un.assign(nu, RepUnit{});
    rep_make_slice(p, c, stride, f0, nf, fr.data(), un.data());
    ++g_calls;
    uint64_t sat = 0;
    for (uint32_t j = 0; j < nf; ++j) {
      const RepFrame& f = fr[j];
      CHECK(f.doff == j * stride && f.pid == c.packet_id + f0 + j && f.offset == uint32_t((f0 + j) * uint64_t(fl)));
      CHECK(f.flag == (f0 + j == 0 ? uint32_t(c.new_block) : 0u));
      CHECK(f.u0 == (j ? fr[j - 1].u0 + fr[j - 1].nu : 0u));
      uint32_t x = 0;
      uint64_t fat = 0;
      for (uint32_t q = f.u0; q < f.u0 + f.nu; ++q) {
        const RepUnit& u = un[q];
        CHECK(u.frame == j && u.soff == sat && u.doff == f.doff + kRepHead + fat);
        const uint8_t* s = img.data() + next + u.soff;
        const uint32_t ch = crc_of(0, s, u.hlen), cp = crc_of(0, s + u.hlen, u.plen);
        CHECK((u.mfh != 0) == (u.hlen != 0) && u.mfp != 0);  // (multmodp does not take a zero first factor)
        x ^= (u.hlen ? multmodp(u.mfh, ch) : 0u) ^ multmodp(u.mfp, cp);
        if (u.rec != kRepNoRec && u.plen) racc[u.rec] ^= multmodp(u.mr, cp);
        sat += u.hlen + u.plen;
        fat += u.hlen + u.plen;
      }
      CHECK(fat == f.length);
      std::vector<uint8_t> body(36 + size_t(f.length));
      rep_info_bytes(c.block_id, f.offset, f.length, body.data());
      if (f.length) memcpy(body.data() + 32, img.data() + f.offset, f.length);
      rep_le32(body.data() + 32 + f.length, f.flag);
      CHECK((f.seed ^ x) == crc_of(kRepFlag, body.data(), body.size()));
    }
    CHECK(sat == uint64_t(len));
    CHECK(rep_call_need(p, len, stride) == (nf - 1) * stride + 60 + (uint64_t(len) - uint64_t(nf - 1) * fl));
    next += len;
    done = true;
  }
  CHECK(!rep_call_ok(p, next, done, next, 0) || total != 0);
  for (size_t r = 0; r < p.recs.size(); ++r)
    CHECK(racc[r] == crc_of(0, img.data() + p.recs[r].offset + kRepInfo, uint64_t(p.recs[r].size) - kRepInfo));
}

static void check_begin_order() {
  RepPlan p;
  tfs_raw_meta m[3] = {{1, 0, 100}, {2, 50, 100}, {3, 300, 100}};
  tfs_replicate_cfg c = cfg_of(4096, 1024);
  CHECK(make_replicate_plan(c, m + 2, 1, &p) == 0);
  CHECK(make_replicate_plan(c, m, 2, &p) == kRepParameterError);       // overlap
  tfs_raw_meta sw[2] = {m[2], m[0]};
  CHECK(make_replicate_plan(c, sw, 2, &p) == kRepParameterError);      // not ascending
  CHECK(make_replicate_plan(c, nullptr, 1, &p) == kRepParameterError);
  CHECK(make_replicate_plan(c, nullptr, 0, &p) == 0 && p.units.size() == 4);
  tfs_replicate_cfg b = c;
  b.total = -1, b.new_block = 3;
  CHECK(make_replicate_plan(b, nullptr, 1, &p) == kRepSizeInvalid);    // size before parameter
  b = c, b.frame_len = 0, b.reserved = 1;
  CHECK(make_replicate_plan(b, nullptr, 0, &p) == kRepSizeInvalid);
  b = c, b.frame_len = 1000;
  CHECK(make_replicate_plan(b, nullptr, 0, &p) == kRepSizeInvalid);
  b = c, b.frame_stride = 1024 + 59;
  CHECK(make_replicate_plan(b, nullptr, 0, &p) == kRepParameterError);
  b.frame_stride = 1024 + 60;
  CHECK(make_replicate_plan(b, nullptr, 0, &p) == 0);
  b = c, b.new_block = 0;
  CHECK(make_replicate_plan(b, nullptr, 0, &p) == kRepParameterError);
  b = c, b.reserved = 5;
  CHECK(make_replicate_plan(b, nullptr, 0, &p) == kRepParameterError);
  // rejected records are set aside before the order check
  tfs_raw_meta mix[4] = {{1, 200, 100}, {9, 100, 36}, {8, 4090, 100}, {2, 300, 37}};
  CHECK(make_replicate_plan(c, mix, 4, &p) == 0);
  CHECK(p.early.size() == 4 && p.early[0] == 0 && p.early[1] == kRepSizeError && p.early[2] == kRepParameterError &&
        p.early[3] == 0);
  CHECK(p.index.size() == 2 && p.index[0] == 0 && p.index[1] == 3);
  CHECK(rep_frame_count(0, 1024) == 1 && rep_frame_count(1, 1024) == 1 && rep_frame_count(1023, 1024) == 1 &&
        rep_frame_count(1024, 1024) == 1 && rep_frame_count(1025, 1024) == 2 && rep_frame_count(-1, 1024) == 0);
}

int main() {
  make_byte_table(g_tab);
  check_begin_order();
  for (uint32_t s = 0; s < 300; ++s) check_layout(s);
  if (g_fail) {
    printf("replicate plan: %d checks failed\n", g_fail);
    return 1;
  }
  printf("replicate plan ok: %u layouts, %u units, %u calls\n", g_layouts, g_units, g_calls);
  return 0;
}
