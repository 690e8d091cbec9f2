// mirror_plan_check.cpp -- stand-alone check of tfs_amd/csrc/mirror_plan.h (no
// device, no Python): built and run by tests/test_mirror_plan.py under the host's
// address and undefined-behaviour sanitizers.
//
// For a few hundred seeded layouts of (first_len, frame_len, sizes, ds counts): the
// statuses decided before reading; the units of every job tile its payload exactly
// once, in order, in the source and in out; no unit crosses a frame cut or is longer
// than kMirSeg; the frames lie back to back from frame_offset and fill the span; the
// prefix bytes are the header, H and V the header file describes; and the fold the
// device does -- seed ^ XOR of the units' CRCs times their multipliers -- gives
// Func::crc(FLAG, body) of every frame and Func::crc(0, payload) of every file,
// computed here by the byte-table loop.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tfs_amd/csrc/mirror_plan.h"

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
static uint32_t rd32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | uint32_t(p[3]) << 24; }
static uint64_t rd64(const uint8_t* p) { return rd32(p) | uint64_t(rd32(p + 4)) << 32; }

static uint32_t g_units = 0, g_layouts = 0, g_frames = 0;

static void check_layout(uint32_t seed) {
  g_rng = 0xBADC0DEull * (seed + 1);
  tfs_mirror_cfg c{};
  switch (rnd() % 5) {
    case 0: c.first_len = 1024 - 36, c.frame_len = 1024; break;
    case 1: c.first_len = TFS_MAX_READ_SIZE - 36, c.frame_len = TFS_MAX_READ_SIZE; break;
    case 2: c.first_len = 40000, c.frame_len = 32768; break;
    case 3: c.first_len = int32_t(rnd_in(1, 70000)), c.frame_len = int32_t(rnd_in(1, 70000)); break;
    default: c.first_len = int32_t(rnd_in(1, 40)), c.frame_len = int32_t(rnd_in(1, 40)); break;
  }
  const bool tiny = c.frame_len <= 40;
  c.is_server = int32_t(rnd() % 3);
  c.version = int16_t(rnd() % 3);
  const uint32_t ds_n = rnd() % 40;
  std::vector<uint64_t> ds(ds_n);
  for (uint64_t& d : ds) d = uint64_t(rnd()) << 32 | rnd();

  // the source: records at any byte offset; the out: spans with gaps between them
  const uint32_t njobs = rnd_in(1, 12);
  std::vector<tfs_mirror_job> jobs;
  std::vector<int32_t> expect;
  uint64_t spos = rnd() % 17, opos = rnd() % 17;
  for (uint32_t i = 0; i < njobs; ++i) {
    tfs_mirror_job j{};
    const uint32_t kind = rnd() % 12;
    uint32_t n;  // payload bytes
    switch (rnd() % 6) {
      case 0: n = rnd_in(1, 40); break;
      case 1: n = uint32_t(c.first_len) + rnd_in(0, 2) - 1; break;
      case 2: n = uint32_t(c.first_len) + uint32_t(c.frame_len) * rnd_in(1, 3) + rnd_in(0, 2) - 1; break;
      case 3: n = rnd_in(1, tiny ? 400 : 200000); break;
      default: n = rnd_in(1, tiny ? 200 : 5000); break;
    }
    if (n == 0) n = 1;
    j.size = int32_t(n + 36);
    j.src_offset = spos;
    j.frame_offset = opos;
    j.file_id = uint64_t(rnd()) << 32 | rnd();
    j.file_number = uint64_t(rnd()) << 32 | rnd();
    j.packet_id = uint64_t(rnd()) << 32 | rnd();
    j.block_id = rnd();
    j.ds_count = ds_n ? std::min<uint32_t>(rnd() % 4 == 0 ? 27u : rnd() % 4, ds_n) : 0u;
    j.ds_first = ds_n - j.ds_count ? rnd() % (ds_n - j.ds_count + 1) : 0u;
    int32_t want = 0;
    if (kind == 0) j.size = int32_t(rnd() % 37), want = kMirSizeError;
    else if (kind == 1) j.ds_count = 28, want = kMirParameterError;
    else if (kind == 2) j.ds_first = ds_n + 1 - j.ds_count + rnd() % 3, want = kMirParameterError;
    else if (kind == 3) j.reserved = 1 + rnd(), want = kMirParameterError;
    jobs.push_back(j);
    expect.push_back(want);
    spos += uint32_t(j.size) + rnd() % 19;
    opos += mir_span(c, j) + rnd() % 23;
  }
  uint64_t src_len = spos + 8, out_cap = opos + 8;
  if (seed % 7 == 0) {  // the last sound job's record passes src_len / its span passes out_cap
    for (size_t i = jobs.size(); i-- > 0;)
      if (expect[i] == 0) {
        if (seed % 14 == 0) src_len = jobs[i].src_offset + uint32_t(jobs[i].size) - 1;
        else out_cap = jobs[i].frame_offset + mir_span(c, jobs[i]) - 1;
        for (size_t k = i; k < jobs.size(); ++k)
          if (expect[k] == 0 || (expect[k] == kMirSizeError && jobs[k].src_offset + uint32_t(jobs[k].size) > src_len))
            expect[k] = kMirParameterError;
        break;
      }
  }
  std::vector<int32_t> pre(jobs.size());
  for (size_t i = 0; i < jobs.size(); ++i) pre[i] = mir_pre_status(c, jobs[i], ds_n, src_len, out_cap);
  CHECK(pre == expect);
  CHECK(mir_cfg_ok(c));
  CHECK(!mir_spans_overlap(c, jobs.data(), pre.data(), uint32_t(jobs.size())));

  MirPlan p;
  CHECK(make_mirror_plan(c, jobs.data(), pre.data(), uint32_t(jobs.size()), ds.data(), &p));
  CHECK(p.jobs.size() == jobs.size());
  ++g_layouts;
  g_units += uint32_t(p.units.size());
  g_frames += uint32_t(p.frames.size());

  std::vector<uint8_t> src(src_len);
  for (uint8_t& b : src) b = uint8_t(rnd());
  uint32_t fi = 0, ui = 0;
  for (size_t i = 0; i < jobs.size(); ++i) {
    const tfs_mirror_job& j = jobs[i];
    const MirJob& mj = p.jobs[i];
    CHECK(mj.pre == pre[i] && mj.file_id == j.file_id && mj.size == j.size);
    CHECK(mj.f0 == fi && mj.u0 == ui);
    if (pre[i] != 0) {
      CHECK(mj.nf == 0 && mj.nu == 0 && mj.span_len == 0);
      continue;
    }
    const int64_t n = int64_t(j.size) - 36;
    const uint32_t nf = mir_frame_count(c, j.size);
    const int64_t want_nf = n <= c.first_len ? 1 : 1 + (n - c.first_len + c.frame_len - 1) / c.frame_len;
    CHECK(nf == want_nf && mj.nf == nf);
    CHECK(mj.span_len == mir_span(c, j) && mj.version_crc == (c.version >= 1 ? 1u : 0u));
    const uint8_t* pay = src.data() + j.src_offset + 36;
    const uint32_t plen = 60 + 8 * j.ds_count;
    int64_t covered = 0;
    uint64_t at = j.frame_offset;
    uint32_t file_crc = 0;
    for (uint32_t k = 0; k < nf; ++k, ++fi) {
      const MirFrame& fr = p.frames[fi];
      const int64_t off = covered;
      const int64_t len = std::min<int64_t>(n - off, k == 0 ? c.first_len : c.frame_len);
      CHECK(len > 0 && fr.doff == at && fr.job == i && fr.pre_len == plen && fr.u0 == ui);
      CHECK(size_t(fr.pre_off) + plen <= p.prefix.size());
      const uint8_t* pb = p.prefix.data() + fr.pre_off;
      CHECK(rd32(pb) == 0x4e534654u && rd32(pb + 4) == 36 + 8 * j.ds_count + uint32_t(len));
      CHECK(rd32(pb + 8) == (9u | uint32_t(uint16_t(c.version)) << 16) && rd64(pb + 12) == j.packet_id + k);
      CHECK(rd32(pb + 20) == 0);
      CHECK(rd32(pb + 24) == j.block_id && rd64(pb + 28) == j.file_id && rd32(pb + 36) == uint32_t(off));
      CHECK(rd32(pb + 40) == uint32_t(len) && rd32(pb + 44) == uint32_t(c.is_server) && rd64(pb + 48) == j.file_number);
      CHECK(rd32(pb + 56) == j.ds_count);
      for (uint32_t d = 0; d < j.ds_count; ++d) CHECK(rd64(pb + 60 + 8 * d) == ds[j.ds_first + d]);
      // the body as it will lie on the wire
      std::vector<uint8_t> body(pb + 24, pb + plen);
      body.insert(body.end(), pay + off, pay + off + len);
      const uint32_t want_crc = crc_of(0x4e534654u, body.data(), body.size());
      uint32_t x = fr.seed;
      int64_t fat = 0;
      for (uint32_t q = 0; q < fr.nu; ++q, ++ui) {
        const MirUnit& u = p.units[ui];
        CHECK(u.plen >= 1 && u.plen <= kMirSeg && fat + u.plen <= len);
        CHECK(u.soff == j.src_offset + 36 + uint64_t(off + fat));
        CHECK(u.doff == at + plen + uint64_t(fat));
        CHECK((u.job & ~kMirStart) == i && ((u.job & kMirStart) != 0) == (off + fat == 0));
        const uint32_t cu = crc_of(0u, src.data() + u.soff, u.plen);
        x ^= multmodp(u.mf, cu);
        file_crc ^= multmodp(u.mr, cu);
        fat += u.plen;
      }
      CHECK(fat == len);
      CHECK(x == want_crc);
      covered += len;
      at += plen + uint64_t(len);
    }
    CHECK(covered == n && at == j.frame_offset + mj.span_len && mj.nu == ui - mj.u0);
    CHECK(file_crc == crc_of(0u, pay, uint64_t(n)));
  }
  CHECK(fi == p.frames.size() && ui == p.units.size());
}

static void check_arithmetic() {
  tfs_mirror_cfg c{};
  c.first_len = 1000, c.frame_len = 300;
  CHECK(mir_frame_count(c, 36) == 0 && mir_frame_count(c, 20) == 0 && mir_frame_count(c, -5) == 0);
  CHECK(mir_frame_count(c, 37) == 1 && mir_frame_count(c, 36 + 999) == 1 && mir_frame_count(c, 36 + 1000) == 1);
  CHECK(mir_frame_count(c, 36 + 1001) == 2 && mir_frame_count(c, 36 + 1300) == 2 && mir_frame_count(c, 36 + 1301) == 3);
  c.first_len = 1, c.frame_len = 1;
  CHECK(mir_frame_count(c, 0x7fffffff) == uint32_t(0x7fffffff - 36));
  tfs_mirror_cfg bad = c;
  bad.first_len = 0;
  CHECK(!mir_cfg_ok(bad) && mir_frame_count(bad, 100) == 0);
  bad = c, bad.frame_len = -1;
  CHECK(!mir_cfg_ok(bad) && mir_frame_count(bad, 100) == 0);
  bad = c, bad.reserved = 1;
  CHECK(!mir_cfg_ok(bad));
  // overlap: two jobs one byte into each other, in either order
  c.first_len = 100, c.frame_len = 100;
  tfs_mirror_job a{}, b{};
  a.size = b.size = 36 + 250;
  a.frame_offset = 10;
  b.frame_offset = 10 + mir_span(c, a) - 1;
  const int32_t ok[2] = {0, 0}, one[2] = {0, kMirParameterError};
  tfs_mirror_job ab[2] = {a, b}, ba[2] = {b, a};
  CHECK(mir_span(c, a) == 3 * 60 + 250);
  CHECK(mir_spans_overlap(c, ab, ok, 2) && mir_spans_overlap(c, ba, ok, 2));
  CHECK(!mir_spans_overlap(c, ab, one, 2));  // a refused job writes nothing
  ab[1].frame_offset += 1, ba[0].frame_offset += 1;
  CHECK(!mir_spans_overlap(c, ab, ok, 2) && !mir_spans_overlap(c, ba, ok, 2));
  // ranges whose end passes 2^64 (the sum wraps to a small number): refused, in the source and in out, also
  // against lengths over 4 GiB; a range that ends exactly at such a length is served
  const uint64_t far = (5ull << 30) + 4096 + 7;
  tfs_mirror_job w{};
  w.size = 300, w.src_offset = ~0ull - 199;  // 2^64 - 200: the sum is 100
  CHECK(mir_pre_status(c, w, 0, 4096, far) == kMirParameterError && mir_pre_status(c, w, 0, far, far) == kMirParameterError);
  w.size = 20000;
  CHECK(mir_pre_status(c, w, 0, far, far) == kMirParameterError);
  w.size = 37, w.src_offset = ~0ull;  // 2^64 - 1
  CHECK(mir_pre_status(c, w, 0, far, far) == kMirParameterError && mir_pre_status(c, w, 0, ~0ull, far) == kMirParameterError);
  w.size = 300, w.src_offset = far - 300;
  CHECK(mir_pre_status(c, w, 0, far, far) == 0 && mir_pre_status(c, w, 0, far - 1, far) == kMirParameterError);
  w.frame_offset = ~0ull - 199;  // the span (3 * 60 + 264) passes 2^64
  CHECK(mir_pre_status(c, w, 0, far, far) == kMirParameterError && mir_pre_status(c, w, 0, far, ~0ull) == kMirParameterError);
  w.frame_offset = far - mir_span(c, w);
  CHECK(mir_pre_status(c, w, 0, far, far) == 0 && mir_pre_status(c, w, 0, far, far - 1) == kMirParameterError);
}

int main() {
  make_byte_table(g_tab);
  check_arithmetic();
  for (uint32_t s = 0; s < 320; ++s) check_layout(s);
  if (g_fail) {
    printf("mirror plan: %d checks failed\n", g_fail);
    return 1;
  }
  printf("mirror plan ok: %u layouts, %u frames, %u units\n", g_layouts, g_frames, g_units);
  return 0;
}
