// receive_plan_check.cpp -- stand-alone check of tfs_amd/csrc/receive_plan.h (no
// device, no Python): built and run by tests/test_receive_plan.py under the host's
// address and undefined-behaviour sanitizers.
//
// For a few hundred seeded layouts: a block's bytes are cut into frames of any
// lengths; the call checks accept the frames in order and refuse every disorder;
// the units of every frame partition its data at the granule grid; the granule
// words gathered from the units, each moved to its granule's end, are Func::crc of
// the granule's bytes followed by zeros; the frame identity gives Func::crc(FLAG,
// body); and for records lying anywhere (inside one granule, on the grid, over
// many granules, overlapping) the descriptor's parts partition the payload and the
// fold over edges and words gives Func::crc(0, payload), computed here byte by byte.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tfs_amd/csrc/receive_plan.h"

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

static uint32_t g_layouts = 0, g_units = 0, g_records = 0;

static void check_layout(uint32_t seed) {
  g_rng = 0xFEEDull * (seed + 1);
  const uint32_t G = kRecvG;
  static const uint32_t kTotals[] = {0, 1, G - 1, G, G + 1, 3 * G, 5 * G + 333};
  const uint32_t total = seed % 4 == 0 ? kTotals[rnd() % 7] : rnd_in(0, seed % 7 == 0 ? 80 * G : 9 * G);
  const int64_t cap = int64_t(total) + rnd() % 3 * 17;
  std::vector<uint8_t> img(size_t(total) + 1);
  for (auto& b : img) b = uint8_t(rnd());
  // frames of any lengths, in a base with filler between them
  std::vector<tfs_receive_desc> descs;
  std::vector<uint8_t> base;
  const uint32_t block_id = rnd();
  uint32_t off = 0;
  do {
    uint32_t len = 0;
    switch (rnd() % 6) {
      case 0: len = rnd_in(0, 40); break;
      case 1: len = G; break;
      case 2: len = rnd_in(1, 3 * G); break;
      case 3: len = (off / G + 1) * G - off; break;  // up to the grid
      default: len = rnd_in(1, 20 * G); break;
    }
    len = std::min(len, total - off);
    const size_t at = base.size() + rnd() % 9;
    base.resize(at + kRecvOverhead + len, uint8_t(0xEE));
    uint8_t* f = base.data() + at;
    memset(f, 0, kRecvHead);
    const uint32_t flag = TFS_PACKET_FLAG_V1, body = kRecvInfo + len, tv = TFS_RECEIVE_PCODE | 2u << 16;
    memcpy(f, &flag, 4), memcpy(f + 4, &body, 4), memcpy(f + 8, &tv, 4);
    memcpy(f + 24, &block_id, 4), memcpy(f + 36, &off, 4), memcpy(f + 40, &len, 4);
    if (len) memcpy(f + kRecvHead, img.data() + off, len);
    const uint32_t fl = descs.empty() ? 1u : 0u;
    memcpy(f + kRecvHead + len, &fl, 4);
    tfs_receive_desc d{};
    CHECK(recv_parse(f, uint32_t(kRecvOverhead + len), at, &d) == 0);
    CHECK(d.data_offset == int32_t(off) && d.data_len == int32_t(len) && d.frame_off == at);
    descs.push_back(d);
    off += len;
  } while (off < total);
  const uint32_t n = uint32_t(descs.size());
  // the call checks: in order, in any grouping; every disorder is refused
  int64_t cursor = 0, end = 0;
  for (uint32_t j = 0; j < n;) {
    const uint32_t m = std::min(n - j, rnd_in(1, 4));
    CHECK(recv_call_ok(descs.data() + j, m, cursor, cap, &end));
    if (j + m < n && descs[j].data_len > 0) CHECK(!recv_call_ok(descs.data() + j + 1, m > 1 ? m - 1 : 1, cursor, cap, &end));
    int64_t e2 = 0;
    CHECK(recv_call_ok(descs.data() + j, m, cursor, cap, &e2));
    cursor = e2;
    j += m;
  }
  CHECK(cursor == int64_t(total));
  if (total > 0) {
    CHECK(!recv_call_ok(descs.data(), n, 0, int64_t(total) - 1, &end));  // past image_cap
    std::vector<tfs_receive_desc> d2(descs);
    d2[n - 1].avail -= 1;
    CHECK(!recv_call_ok(d2.data(), n, 0, cap, &end));
    d2 = descs;
    d2[0].data_len = -1;
    CHECK(!recv_call_ok(d2.data(), n, 0, cap, &end));
  }
  // the units, the words, the frame identity
  std::vector<RecvFrame> frames(n);
  const uint32_t nu = recv_make_frames(descs.data(), n, frames.data());
  g_units += nu;
  std::vector<uint32_t> words(recv_words(cap) + 1, 0u);
  uint32_t seen = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const RecvFrame& fr = frames[j];
    CHECK(fr.u0 == seen && fr.src_end == fr.soff + kRecvOverhead + fr.len);
    const uint8_t* f = base.data() + fr.soff;
    uint32_t cd = 0, covered = fr.off;
    for (uint32_t k = 0; k < fr.nu; ++k) {
      const uint64_t gs = uint64_t(fr.off / G + k) * G, fe = uint64_t(fr.off) + fr.len;
      const uint64_t s = std::max<uint64_t>(gs, fr.off), e = std::min<uint64_t>(gs + G, fe);
      CHECK(s == covered && e > s && e - s <= G);
      covered = uint32_t(e);
      const uint32_t c = crc_of(0, f + kRecvHead + (s - fr.off), e - s);
      cd ^= shift_bytes_pow(c, fe - e);
      words[gs / G] ^= shift_bytes_pow(c, gs + G - e);
    }
    CHECK(covered == fr.off + fr.len);
    seen += fr.nu;
    const uint32_t body = shift_bytes_pow(crc_of(TFS_PACKET_FLAG_V1, f + 24, 32), uint64_t(fr.len) + 4u) ^
                          shift_bytes_pow(cd, 4) ^ crc_of(0, f + kRecvHead + fr.len, 4);
    CHECK(body == crc_of(TFS_PACKET_FLAG_V1, f + 24, kRecvInfo + fr.len));
  }
  CHECK(seen == nu);
  for (uint64_t g = 0; g < recv_words(cap); ++g) {
    std::vector<uint8_t> z(G, 0);
    const uint64_t s = g * G;
    if (s < total) memcpy(z.data(), img.data() + s, std::min<uint64_t>(G, total - s));
    CHECK(words[g] == crc_of(0, z.data(), G));
  }
  // records lying anywhere
  const uint32_t nrec = 4 + rnd() % 12;
  for (uint32_t i = 0; i < nrec; ++i) {
    tfs_raw_meta m{};
    m.file_id = rnd();
    const uint32_t kind = rnd() % 8;
    int64_t o = total ? rnd() % total : 0, size = 0;
    if (kind == 0) o = int64_t(rnd() % (total / G + 1)) * G - 36;  // payload starts on the grid
    if (kind == 1) size = 37 + rnd() % 60;                           // (mostly) inside one granule
    else if (kind == 2) size = rnd() % 37;                           // too short
    else if (kind == 3) size = int64_t(total) - o + int64_t(rnd() % 3) - 1;  // up to the end, or just past it
    else size = 37 + rnd() % (20 * G);
    if (kind == 4 && o + size > G) size = (o + size) / G * G - o;    // payload ends on the grid
    if (kind == 5) o = -int64_t(rnd() % 5) - 1;
    m.offset = int32_t(o), m.size = int32_t(size);
    const RecvRec r = recv_make_rec(m, total);
    if (o < 0 || o + size > int64_t(total)) {
      CHECK(r.pre == kRecvParameterError);
      continue;
    }
    if (size <= 36) {
      CHECK(r.pre == kRecvSizeError);
      continue;
    }
    ++g_records;
    const uint32_t a = uint32_t(o) + 36u, b = uint32_t(o + size);
    CHECK(r.pre == 0 && r.a == a && r.b == b && r.file_id == m.file_id && r.offset == m.offset && r.size == m.size);
    CHECK(r.a <= r.he && r.he <= r.tb && r.tb <= r.b);
    CHECK(r.he - r.a < G && r.b - r.tb < G);  // edges only: at most 2 (G - 1) payload bytes are read again
    if (r.ng) {
      CHECK(r.he == r.g0 * G && r.tb == (r.g0 + r.ng) * G);
    } else {
      CHECK(r.he == r.tb || (r.he == r.b && r.tb == r.b));
      if (r.he != r.b) CHECK(r.he % G == 0);
    }
    if (a % G == 0 && b - a >= G) CHECK(r.he == a && r.g0 == a / G);
    if (b % G == 0) CHECK(r.tb == b);
    CHECK(recv_fold_host(r, img.data(), words.data()) == crc_of(0, img.data() + a, b - a));
  }
  ++g_layouts;
}

int main() {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : (c >> 1);
    g_tab[i] = c;
  }
  constexpr RecvPowTab pw = recv_pow_tab();
  for (uint32_t k = 0; k < kRecvPowN; ++k) CHECK(pw.p[k] == x2nmodp(uint64_t(1) << k, 3));
  CHECK(recv_units(0, 0) == 0 && recv_units(5, 0) == 0 && recv_units(0, 1) == 1 && recv_units(kRecvG - 1, 2) == 2 &&
        recv_units(kRecvG, kRecvG) == 1 && recv_units(1, 2 * kRecvG) == 3);
  for (uint32_t seed = 0; seed < 300; ++seed) check_layout(seed);
  if (g_fail) {
    printf("receive plan: %d checks failed\n", g_fail);
    return 1;
  }
  printf("receive plan ok: %u layouts, %u units, %u records\n", g_layouts, g_units, g_records);
  return 0;
}
