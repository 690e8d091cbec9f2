// repair_plan_check.cpp -- stand-alone check of tfs_amd/csrc/repair_plan.h (no
// device, no Python): built and run by tests/test_repair_plan.py under the host's
// address and undefined-behaviour sanitizers.
//
// For a few hundred seeded layouts of (frame_len, payloads cut at random into reply
// frames of the three pcodes, ds counts): the statuses decided before reading; the
// units of every job tile its payload exactly once, in order, in the source and in
// out; no unit crosses an incoming frame, an outgoing frame or a kRepSeg cut; the
// outgoing frames lie back to back and fill the span, their prefix bytes those of a
// plain serializer written here; and the three folds the device does over the
// units' CRCs give Func::crc(FLAG, body) of every incoming frame, Func::crc(0,
// payload) of every file and Func::crc(FLAG, body) of every outgoing frame,
// computed here by the byte-table loop.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tfs_amd/csrc/repair_plan.h"

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
static void put32(std::vector<uint8_t>& v, uint32_t x) {
  for (int k = 0; k < 4; ++k) v.push_back(uint8_t(x >> (8 * k)));
}
static void put64(std::vector<uint8_t>& v, uint64_t x) { put32(v, uint32_t(x)), put32(v, uint32_t(x >> 32)); }

static uint32_t g_units = 0, g_layouts = 0, g_frames = 0, g_ins = 0;

static void check_layout(uint32_t seed) {
  g_rng = 0xFEEDull * (seed + 1);
  tfs_repair_cfg c{};
  switch (rnd() % 5) {
    case 0: c.frame_len = 1024; break;
    case 1: c.frame_len = TFS_MAX_READ_SIZE; break;
    case 2: c.frame_len = 16384; break;
    case 3: c.frame_len = int32_t(rnd_in(1, 70000)); break;
    default: c.frame_len = int32_t(rnd_in(1, 40)); break;
  }
  const bool tiny = c.frame_len <= 40;
  c.is_server = int32_t(rnd() % 3);
  c.version = int16_t(rnd() % 3);
  const uint32_t ds_n = rnd() % 40;
  std::vector<uint64_t> ds(ds_n);
  for (uint64_t& d : ds) d = uint64_t(rnd()) << 32 | rnd();

  // the source: reply frames at any byte offset; the out: spans with gaps between them
  const uint32_t njobs = rnd_in(1, 10);
  std::vector<tfs_repair_job> jobs;
  std::vector<tfs_repair_in> ins;
  std::vector<int32_t> expect;
  std::vector<uint8_t> src(rnd() % 17);
  uint64_t opos = rnd() % 17;
  for (uint32_t i = 0; i < njobs; ++i) {
    tfs_repair_job j{};
    const uint32_t kind = rnd() % 14;
    uint32_t n;  // payload bytes
    switch (rnd() % 6) {
      case 0: n = rnd_in(1, 40); break;
      case 1: n = uint32_t(c.frame_len) * rnd_in(1, 3) + rnd_in(0, 2) - 1; break;
      case 2: n = rnd_in(1, tiny ? 400 : 150000); break;
      default: n = rnd_in(1, tiny ? 200 : 5000); break;
    }
    if (n == 0) n = 1;
    const int16_t pcode = int16_t(rnd() % 3 == 0 ? 8 : rnd() % 2 ? 39 : 63);
    const uint32_t in_max = rnd() % 3 == 0 ? n : rnd() % 2 ? rnd_in(1, 20000) : uint32_t(c.frame_len);
    j.in_first = uint32_t(ins.size());
    for (uint32_t at = 0, k = 0; at < n; ++k) {  // the reply frames as a source would write them
      const uint32_t nk = rnd() % 9 == 0 ? 0u : std::min<uint32_t>(n - at, rnd() % 4 == 0 ? rnd_in(1, in_max) : in_max);
      tfs_repair_in f{};
      src.resize(src.size() + rnd() % 19);
      f.frame_off = src.size();
      f.data_len = int32_t(nk);
      f.pcode = pcode;
      f.trailer = int16_t(pcode == 8 ? 0 : (k == 0 ? 40 : 4));
      std::vector<uint8_t> body;
      put32(body, nk);
      for (uint32_t b = 0; b < nk; ++b) body.push_back(uint8_t(rnd()));
      if (f.trailer) put32(body, f.trailer == 40 ? 36u : 0u);
      for (int b = 4; b < f.trailer; ++b) body.push_back(uint8_t(rnd()));
      put32(src, 0x4e534654u), put32(src, uint32_t(body.size()));
      put32(src, uint32_t(pcode) | 2u << 16), put64(src, rnd());
      put32(src, crc_of(0x4e534654u, body.data(), body.size()));
      src.insert(src.end(), body.begin(), body.end());
      f.avail = uint32_t(src.size() - f.frame_off);
      ins.push_back(f);
      at += nk;
    }
    j.in_count = uint32_t(ins.size()) - j.in_first;
    j.stat_size = n;
    j.frame_offset = opos;
    j.file_id = uint64_t(rnd()) << 32 | rnd();
    j.file_number = uint64_t(rnd()) << 32 | rnd();
    j.packet_id = uint64_t(rnd()) << 32 | rnd();
    j.block_id = rnd();
    j.stat_crc = rnd(), j.check_crc = rnd();
    j.ds_count = ds_n ? std::min<uint32_t>(rnd() % 4 == 0 ? 27u : rnd() % 4, ds_n) : 0u;
    j.ds_first = ds_n - j.ds_count ? rnd() % (ds_n - j.ds_count + 1) : 0u;
    int32_t want = 0;
    if (kind == 0) j.stat_size = -int64_t(rnd() % 3), want = kRprSizeError;
    else if (kind == 1) j.ds_count = 28, want = kRprParameterError;
    else if (kind == 2) j.ds_first = ds_n + 1 - j.ds_count + rnd() % 3, want = kRprParameterError;
    else if (kind == 3) j.reserved = 1 + rnd() % 100, want = kRprParameterError;
    else if (kind == 4) j.stat_size += 1 + rnd() % 2, want = kRprSyncError;
    else if (kind == 5) j.in_count = 0, want = kRprParameterError;
    else if (kind == 6) ins[j.in_first + rnd() % j.in_count].avail -= 1, want = kRprParameterError;
    else if (kind == 7) ins[j.in_first + rnd() % j.in_count].pcode = 9, want = kRprParameterError;
    else if (kind == 8 && pcode == 8) ins[j.in_first].trailer = 4, ins[j.in_first].avail += 4, want = kRprParameterError;
    jobs.push_back(j);
    expect.push_back(want);
    opos += rpr_span(c, j) + rnd() % 23;
  }
  src.resize(src.size() + 8);
  const uint64_t src_len = src.size(), out_cap = opos + 8;
  const uint32_t n_in = uint32_t(ins.size());
  std::vector<int32_t> pre(jobs.size());
  for (size_t i = 0; i < jobs.size(); ++i)
    pre[i] = rpr_pre_status(c, jobs[i], ins.data(), n_in, ds_n, src_len, out_cap);
  CHECK(pre == expect);
  CHECK(rpr_cfg_ok(c));
  CHECK(!rpr_spans_overlap(c, jobs.data(), pre.data(), uint32_t(jobs.size())));

  RprPlan p;
  CHECK(make_repair_plan(c, ins.data(), jobs.data(), pre.data(), uint32_t(jobs.size()), ds.data(), &p));
  CHECK(p.jobs.size() == jobs.size());
  ++g_layouts;
  g_units += uint32_t(p.units.size());
  g_frames += uint32_t(p.frames.size());
  g_ins += uint32_t(p.ins.size());

  uint32_t ii = 0, fi = 0, ui = 0;
  for (size_t i = 0; i < jobs.size(); ++i) {
    const tfs_repair_job& j = jobs[i];
    const RprJob& rj = p.jobs[i];
    CHECK(rj.pre == pre[i] && rj.i0 == ii && rj.f0 == fi && rj.u0 == ui);
    CHECK(rj.stat_crc == j.stat_crc && rj.check_crc == j.check_crc);
    if (pre[i] != 0) {
      CHECK(rj.ni == 0 && rj.nf == 0 && rj.nu == 0 && rj.span_len == 0);
      continue;
    }
    const int64_t n = j.stat_size;
    const uint32_t nf = rpr_frame_count(c, n);
    CHECK(nf == uint32_t((n + c.frame_len - 1) / c.frame_len) && rj.nf == nf && rj.ni == j.in_count);
    CHECK(rj.span_len == rpr_span(c, j) && rj.version_crc == (c.version >= 1 ? 1u : 0u));
    // the payload, from the frames' data
    std::vector<uint8_t> pay;
    for (uint32_t k = 0; k < j.in_count; ++k) {
      const tfs_repair_in& f = ins[j.in_first + k];
      pay.insert(pay.end(), src.begin() + long(f.frame_off) + 28, src.begin() + long(f.frame_off) + 28 + f.data_len);
    }
    CHECK(int64_t(pay.size()) == n);
    std::vector<uint32_t> ucrc(rj.nu);
    // the units in order: each incoming frame's, tiling its data; together the payload
    int64_t pos = 0;
    uint32_t file_crc = 0;
    for (uint32_t k = 0; k < j.in_count; ++k, ++ii) {
      const tfs_repair_in& f = ins[j.in_first + k];
      const RprIn& ri = p.ins[ii];
      CHECK(ri.soff == f.frame_off && ri.data_len == uint32_t(f.data_len) && ri.u0 == ui && ri.job == i && ri.idx == k);
      CHECK(ri.pcode == uint32_t(f.pcode) && ri.trailer == uint32_t(f.trailer));
      uint32_t x = ri.seed;
      int64_t t = 0;
      for (uint32_t q = 0; q < ri.nu; ++q, ++ui) {
        const RprUnit& u = p.units[ui];
        CHECK(u.plen >= 1 && u.plen <= kRepSeg && t + u.plen <= f.data_len && u.job == i);
        CHECK(t / kRepSeg == (t + u.plen - 1) / kRepSeg);                          // no segment cut inside
        CHECK((pos + t) / c.frame_len == (pos + t + u.plen - 1) / c.frame_len);    // no outgoing cut inside
        CHECK(u.soff == f.frame_off + 28 + uint64_t(t));
        const int64_t fk = (pos + t) / c.frame_len, fo = (pos + t) % c.frame_len;
        CHECK(u.doff == j.frame_offset + uint64_t(fk) * (60 + 8 * j.ds_count + uint64_t(c.frame_len)) + 60 +
                            8 * j.ds_count + uint64_t(fo));
        const uint32_t cu = crc_of(0u, src.data() + u.soff, u.plen);
        CHECK(memcmp(src.data() + u.soff, pay.data() + pos + t, u.plen) == 0);
        ucrc[ui - rj.u0] = cu;
        x ^= multmodp(u.mi, cu);
        file_crc ^= multmodp(u.mr, cu);
        t += u.plen;
      }
      CHECK(t == f.data_len);
      const uint8_t* body = src.data() + f.frame_off + 24;
      CHECK(x == crc_of(0x4e534654u, body, 4 + uint64_t(f.data_len)));
      x = crc_of(x, body + 4 + f.data_len, uint64_t(f.trailer));
      uint32_t hdr_crc;
      memcpy(&hdr_crc, src.data() + f.frame_off + 20, 4);
      CHECK(x == hdr_crc);
      pos += f.data_len;
    }
    CHECK(pos == n && rj.nu == ui - rj.u0);
    CHECK(file_crc == crc_of(0u, pay.data(), uint64_t(n)));
    // the outgoing frames against a plain serializer
    uint64_t at = j.frame_offset;
    uint32_t useen = rj.u0;
    for (uint32_t k = 0; k < nf; ++k, ++fi) {
      const MirFrame& fr = p.frames[fi];
      const int64_t off = int64_t(k) * c.frame_len, len = std::min<int64_t>(c.frame_len, n - off);
      std::vector<uint8_t> w;
      put32(w, 0x4e534654u), put32(w, 36 + 8 * j.ds_count + uint32_t(len));
      put32(w, 9u | uint32_t(uint16_t(c.version)) << 16), put64(w, j.packet_id + k), put32(w, 0u);
      put32(w, j.block_id), put64(w, j.file_id), put32(w, uint32_t(off)), put32(w, uint32_t(len));
      put32(w, uint32_t(c.is_server)), put64(w, j.file_number), put32(w, j.ds_count);
      for (uint32_t d = 0; d < j.ds_count; ++d) put64(w, ds[j.ds_first + d]);
      CHECK(fr.doff == at && fr.job == i && fr.pre_len == w.size() && fr.u0 == useen && fr.nu >= 1);
      CHECK(size_t(fr.pre_off) + fr.pre_len <= p.prefix.size());
      CHECK(fr.pre_len == w.size() && memcmp(p.prefix.data() + fr.pre_off, w.data(), w.size()) == 0);
      std::vector<uint8_t> body(w.begin() + 24, w.end());
      body.insert(body.end(), pay.begin() + off, pay.begin() + off + len);
      uint32_t x = fr.seed;
      int64_t fat = 0;
      for (uint32_t q = 0; q < fr.nu; ++q) {
        const RprUnit& u = p.units[fr.u0 + q];
        CHECK(u.doff == at + w.size() + uint64_t(fat));
        x ^= multmodp(u.mf, ucrc[fr.u0 + q - rj.u0]);
        fat += u.plen;
      }
      CHECK(fat == len);
      CHECK(x == crc_of(0x4e534654u, body.data(), body.size()));
      useen += fr.nu;
      at += w.size() + uint64_t(len);
    }
    CHECK(useen == ui && at == j.frame_offset + rj.span_len);
  }
  CHECK(ii == p.ins.size() && fi == p.frames.size() && ui == p.units.size());
}

static void check_arithmetic() {
  tfs_repair_cfg c{};
  c.frame_len = 300;
  CHECK(rpr_frame_count(c, 0) == 0 && rpr_frame_count(c, -5) == 0);
  CHECK(rpr_frame_count(c, 1) == 1 && rpr_frame_count(c, 299) == 1 && rpr_frame_count(c, 300) == 1);
  CHECK(rpr_frame_count(c, 301) == 2 && rpr_frame_count(c, 600) == 2 && rpr_frame_count(c, 601) == 3);
  tfs_repair_cfg bad = c;
  bad.frame_len = 0;
  CHECK(!rpr_cfg_ok(bad) && rpr_frame_count(bad, 100) == 0);
  bad = c, bad.frame_len = -1;
  CHECK(!rpr_cfg_ok(bad) && rpr_frame_count(bad, 100) == 0);
  bad = c, bad.reserved = 1;
  CHECK(!rpr_cfg_ok(bad));
  c.frame_len = 1;
  CHECK(rpr_frame_count(c, int64_t(1) << 33) == 0);
  // overlap: two jobs one byte into each other, in either order
  c.frame_len = 100;
  tfs_repair_job a{}, b{};
  a.stat_size = b.stat_size = 250;
  a.frame_offset = 10;
  b.frame_offset = 10 + rpr_span(c, a) - 1;
  const int32_t ok[2] = {0, 0}, one[2] = {0, kRprParameterError};
  tfs_repair_job ab[2] = {a, b}, ba[2] = {b, a};
  CHECK(rpr_span(c, a) == 3 * 60 + 250);
  CHECK(rpr_spans_overlap(c, ab, ok, 2) && rpr_spans_overlap(c, ba, ok, 2));
  CHECK(!rpr_spans_overlap(c, ab, one, 2));  // a refused job writes nothing
  ab[1].frame_offset += 1, ba[0].frame_offset += 1;
  CHECK(!rpr_spans_overlap(c, ab, ok, 2) && !rpr_spans_overlap(c, ba, ok, 2));
  // ranges whose end passes 2^64: refused in the source and in out
  const uint64_t far = (5ull << 30) + 4096 + 7;
  tfs_repair_in f{};
  f.data_len = 250, f.avail = 278, f.pcode = 8;
  tfs_repair_job w{};
  w.stat_size = 250, w.in_count = 1;
  f.frame_off = ~0ull - 199;
  CHECK(rpr_pre_status(c, w, &f, 1, 0, 4096, far) == kRprParameterError);
  CHECK(rpr_pre_status(c, w, &f, 1, 0, far, far) == kRprParameterError);
  f.frame_off = far - 278;
  CHECK(rpr_pre_status(c, w, &f, 1, 0, far, far) == 0 && rpr_pre_status(c, w, &f, 1, 0, far - 1, far) == kRprParameterError);
  w.frame_offset = ~0ull - 199;
  CHECK(rpr_pre_status(c, w, &f, 1, 0, far, far) == kRprParameterError);
  CHECK(rpr_pre_status(c, w, &f, 1, 0, far, ~0ull) == kRprParameterError);
  w.frame_offset = far - rpr_span(c, w);
  CHECK(rpr_pre_status(c, w, &f, 1, 0, far, far) == 0 && rpr_pre_status(c, w, &f, 1, 0, far, far - 1) == kRprParameterError);
  f.data_len = -1;
  CHECK(rpr_pre_status(c, w, &f, 1, 0, far, far) == kRprParameterError);
  // parse: short, each pcode, first and later, an error reply
  uint8_t fr[28] = {0};
  tfs_repair_in d{};
  fr[24] = 7;
  CHECK(rpr_parse(fr, 27, 5, 8, 1, &d) == TFS_PACKET_INCOMPLETE && rpr_parse(fr, 28, 5, 9, 1, &d) == kRprParameterError);
  CHECK(rpr_parse(fr, 28, 5, 8, 1, &d) == 0 && d.frame_off == 5 && d.avail == 28 && d.data_len == 7 && d.trailer == 0);
  CHECK(rpr_parse(fr, 28, 5, 39, 1, &d) == 0 && d.trailer == 40 && d.pcode == 39);
  CHECK(rpr_parse(fr, 28, 5, 63, 0, &d) == 0 && d.trailer == 4 && d.pcode == 63);
  fr[24] = 0x76, fr[25] = 0xe0, fr[26] = fr[27] = 0xff;  // -8074
  d.data_len = 99;
  CHECK(rpr_parse(fr, 28, 5, 8, 1, &d) == -8074 && d.data_len == 99);
}

int main() {
  make_byte_table(g_tab);
  check_arithmetic();
  for (uint32_t s = 0; s < 320; ++s) check_layout(s);
  if (g_fail) {
    printf("repair plan: %d checks failed\n", g_fail);
    return 1;
  }
  printf("repair plan ok: %u layouts, %u incoming frames, %u outgoing frames, %u units\n", g_layouts, g_ins, g_frames,
         g_units);
  return 0;
}
