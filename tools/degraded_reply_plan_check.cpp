// degraded_reply_plan_check.cpp -- stand-alone check of tfs_amd/csrc/ec_reply_plan.h, the host
// arithmetic of the degraded read replies (include/tfs_ec_read.h): on random job lists, the
// kernel's tile walk (reply_cover) against a brute-force restatement of the covering set -- every
// unit exactly once, no other unit -- the statuses decided before reading, the span-overlap check,
// and the host form's plan: the packed images hold exactly the union of the covering sets, every
// restated unit finds its FileInfo and its slice in them, and the staged frames lie one behind the
// other with frame + 28 congruent to the slice's first byte mod 16 and under 16 bytes of padding.
// No device.  Built and run by tests/test_degraded_reply_plan.py under the host's address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../tfs_amd/csrc/ec_reply_plan.h"

using namespace tfsec;
using tfscrc::kReadParameterError;
using tfscrc::kReadSizeError;

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}
static uint32_t below(uint32_t n) { return n ? uint32_t(next() % n) : 0u; }

static tfs_ec_reply_job job(uint64_t so, uint64_t fo, int32_t size, int32_t ro, int32_t rl, int16_t pcode,
                            uint32_t refuse = 0) {
  tfs_ec_reply_job j{};
  j.read.src_offset = so, j.read.frame_offset = fo, j.read.file_id = 7, j.read.packet_id = 9;
  j.read.size = size, j.read.read_offset = ro, j.read.read_len = rl, j.read.pcode = pcode, j.read.version = 2;
  j.refuse_flags = refuse;
  return j;
}

// The covering set by its definition: the units that hold a byte of [H, H + 36) or of [D0, D0 + n).
static std::set<uint32_t> brute_cover(uint32_t H, uint32_t D0, uint32_t n) {
  std::set<uint32_t> s;
  for (uint32_t b = H; b < H + 36u; ++b) s.insert(b >> 10);
  for (uint32_t b = D0; b < D0 + n; b += 512u) s.insert(b >> 10);  // a unit that holds a slice byte holds one of these,
  if (n) s.insert((D0 + n - 1u) >> 10);                            // or the last
  return s;
}

// The units the kernel's waves load for a job, with how often: tile t, unit u of it.
static std::map<uint32_t, int> walk(const ReplyCover& c) {
  std::map<uint32_t, int> seen;
  for (uint32_t t = 0; t < c.nt; ++t)
    for (uint32_t u = 0; u < 4; ++u) {
      const uint32_t pu = (t == 0u ? c.hA : c.tb1 + 4096u * t) + 1024u * u;
      if (pu < (t == 0u ? c.e0 : c.e1)) ++seen[pu >> 10];
    }
  return seen;
}

int main() {
  uint32_t njobs = 0, nlists = 0, noverlap = 0;
  const int16_t pcodes[3] = {8, 39, 63};
  const int32_t member = 8 << 20;
  const uint64_t big = 1ull << 40;
  // 1. the tile walk against the definition, slices around every kind of edge
  const uint32_t edges[] = {8, 128, 1024, 4096, 32768};
  for (int rep = 0; rep < 4000; ++rep) {
    const uint32_t H = below(200000);
    const uint32_t pay = rep % 7 == 0 ? below(40) : below(300000);
    uint32_t ro = below(pay + 1), n = below(pay - ro + 1);
    if (rep % 3 == 0 && pay > 64) {  // start or end 0..8 bytes around an edge
      const uint32_t e = edges[below(5)];
      const uint32_t want = ((H + 36u + ro) / e + 1u) * e + below(17) - 8u;  // a D0 near an edge
      if (want >= H + 36u && want - (H + 36u) <= pay) ro = want - (H + 36u), n = below(pay - ro + 1);
      if (rep % 6 == 0 && n > 16) {
        const uint32_t d1 = ((H + 36u + ro + n) / e) * e + below(17) - 8u;
        if (d1 > H + 36u + ro && d1 <= H + 36u + pay) n = d1 - (H + 36u + ro);
      }
    }
    if (rep % 11 == 0) n = 0;
    const uint32_t D0 = H + 36u + ro;
    const ReplyCover c = reply_cover(H, D0, n);
    const std::set<uint32_t> want = brute_cover(H, D0, n);
    const std::map<uint32_t, int> got = walk(c);
    CHECK(got.size() == want.size());
    for (const auto& kv : got) CHECK(kv.second == 1 && want.count(kv.first));
    // the FileInfo lies in tile 0; the last tile's end is under 4 KiB past the slice's
    CHECK(c.hA <= H && H + 36u <= c.hA + 4096u && H + 36u <= c.e0);
    if (n) {
      const uint32_t pad = c.tb1 + 4096u * c.nt - (D0 + n);
      CHECK(pad < 4096u);
      // the slice's tiles hold the whole slice
      CHECK(c.e1 >= D0 + n && (c.tb1 == c.hA ? c.hA : c.tb1 + 4096u) <= D0);
    } else {
      CHECK(c.nt == 1u);
    }
    ++njobs;
  }
  // 2. the unit, and the statuses decided before reading, in tfs_read.h's order plus the covering set
  {
    const ReplyUnit u = reply_make_unit(job(5000, 77, 10036, 100, 500, 39, 7u), member, big);
    CHECK(u.pre == 0 && u.hpos == 5000u && u.dpos == 5136u && u.n == 500u && u.tlen == 4u && u.whole == 0u);
    CHECK(u.refuse == 0u && u.doff == 77u && u.fid == 7u && u.pid == 9u);  // a later fragment is never refused
    const ReplyUnit w = reply_make_unit(job(5000, 77, 10036, 0, 1 << 20, 63, 7u), member, big);
    CHECK(w.pre == 0 && w.n == 10000u && w.whole == 1u && w.tlen == 40u && w.refuse == 7u);
    CHECK(w.pre_seed == tfscrc::read_pre_seed(10000u));
    CHECK(reply_make_unit(job(5000, 0, 10036, 0, 5, 9), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(5000, 0, 10036, -1, 5, 8), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(5000, 0, 10036, 0, -5, 8), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(5000, 0, 10036, 10001, 5, 8), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(5000, 0, 10036, 10000, 5, 8), member, big).pre == 0);
    CHECK(reply_make_unit(job(5000, 0, 35, 0, 5, 8), member, big).pre == kReadSizeError);
    CHECK(reply_make_unit(job(5000, 0, -3, 0, 5, 8), member, big).pre == kReadSizeError);
    CHECK(reply_make_unit(job(uint64_t(member) - 100, 0, 101, 0, 5, 8), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(uint64_t(member) - 100, 0, 100, 0, 5, 8), member, big).pre == 0);
    CHECK(reply_make_unit(job(uint64_t(member) + 1, 0, 0, 0, 0, 8), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(~0ull, 0, 100, 0, 5, 8), member, big).pre == kReadParameterError);
    // ranges whose end passes 2^64 (the sums wrap to 100, 19,800 and 36): in the member and in out
    CHECK(reply_make_unit(job(~0ull - 199, 0, 300, 0, 264, 8), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(~0ull - 199, 0, 20000, 0, 19964, 39), member, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(~0ull, 0, 37, 0, 1, 63), member, big).pre == kReadParameterError);
    for (uint64_t cap : {uint64_t(4096), uint64_t((5ull << 30) + 4096 + 7), uint64_t(~0ull)}) {
      CHECK(reply_make_unit(job(5000, ~0ull - 199, 300, 0, 264, 8), member, cap).pre == kReadParameterError);
      CHECK(reply_make_unit(job(5000, ~0ull - 199, 20000, 0, 19964, 39), member, cap).pre == kReadParameterError);
      CHECK(reply_make_unit(job(5000, ~0ull, 37, 0, 1, 63), member, cap).pre == kReadParameterError);
    }
    CHECK(reply_make_unit(job(5000, 10, 136, 0, 100, 8), member, 137).pre == kReadParameterError);  // span past out_cap
    CHECK(reply_make_unit(job(5000, 10, 136, 0, 100, 8), member, 138).pre == 0);
    CHECK(reply_make_unit(job(5000, 10, 136, 0, 100, 8), 0, big).pre == kReadParameterError);
    CHECK(reply_make_unit(job(5000, 10, 136, 0, 100, 8), -1024, big).pre == kReadParameterError);
    njobs += 19;
  }
  // 3. random lists: the span check against every pair, the plan against the definition
  for (int rep = 0; rep < 300; ++rep) {
    const uint32_t n = 1u + below(40);
    std::vector<tfs_ec_reply_job> v;
    uint64_t fo = below(64);
    for (uint32_t i = 0; i < n; ++i) {
      const int32_t pay = int32_t(rep % 2 ? below(3000) : below(200000));
      const uint32_t H = below(uint32_t(member) - uint32_t(pay) - 36u);
      const int32_t ro = int32_t(below(uint32_t(pay) + 1u)), rl = int32_t(below(uint32_t(pay) + 50u));
      tfs_ec_reply_job j = job(H, fo, pay + 36, ro, rl, pcodes[below(3)]);
      const uint32_t dice = below(20);
      if (dice == 0) j.read.pcode = 5;
      if (dice == 1) j.read.size = int32_t(below(36));
      if (dice == 2) j.read.src_offset = uint64_t(member) - 10;
      if (dice == 3) j.read.read_len = 0;
      v.push_back(j);
      fo += tfscrc::read_frame_cap(j.read) + (below(4) == 0 ? below(40) : 0u);
    }
    const uint64_t out_cap = fo + (below(3) == 0 ? 0u : below(100));
    if (rep % 5 == 0 && n > 1) {  // any order
      for (uint32_t i = n - 1; i > 0; --i) std::swap(v[i], v[below(i + 1)]);
    }
    if (rep % 4 == 0 && n > 1) {  // move one frame a byte into the frame before it in address order
      uint32_t a = below(n), b = n;
      for (uint32_t i = 0; i < n; ++i)
        if (i != a && v[i].read.frame_offset < v[a].read.frame_offset &&
            (b == n || v[i].read.frame_offset > v[b].read.frame_offset))
          b = i;
      if (b != n && tfscrc::read_frame_cap(v[b].read)) {
        v[a].read.frame_offset = v[b].read.frame_offset + tfscrc::read_frame_cap(v[b].read) - 1;
      }
    }
    bool brute = false;  // every pair of jobs that may write
    std::vector<ReplyUnit> us;
    for (uint32_t i = 0; i < n; ++i) us.push_back(reply_make_unit(v[i], member, out_cap));
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t k = i + 1; k < n; ++k) {
        if (us[i].pre == kReadParameterError || us[k].pre == kReadParameterError) continue;
        const uint64_t a0 = v[i].read.frame_offset, a1 = a0 + tfscrc::read_frame_cap(v[i].read);
        const uint64_t b0 = v[k].read.frame_offset, b1 = b0 + tfscrc::read_frame_cap(v[k].read);
        if (a0 < b1 && b0 < a1) brute = true;
      }
    CHECK(reply_spans_overlap(v.data(), n, member, out_cap) == brute);
    noverlap += brute ? 1u : 0u;
    ++nlists;
    for (int stage = 0; stage < 2; ++stage) {
      ReplyPlan p;
      make_reply_plan(v.data(), n, member, out_cap, stage != 0, &p);
      CHECK(p.units.size() == n && p.opos.size() == n);
      // the packed images: exactly the union of the covering sets, ascending, touching ranges joined
      std::set<uint32_t> uni;
      for (uint32_t i = 0; i < n; ++i)
        if (us[i].pre == 0) {
          const std::set<uint32_t> c = brute_cover(us[i].hpos, us[i].dpos, us[i].n);
          uni.insert(c.begin(), c.end());
        }
      CHECK(p.up == 1024ull * uni.size());
      std::vector<uint32_t> image;  // image[k]: the member unit at packed unit k
      uint64_t at = 0;
      for (size_t s = 0; s < p.spans.size(); ++s) {
        CHECK(p.spans[s].start % 1024u == 0 && p.spans[s].end % 1024u == 0 && p.spans[s].start < p.spans[s].end);
        CHECK(p.spans[s].cbase == at);
        if (s) CHECK(p.spans[s].start > p.spans[s - 1].end);
        for (uint32_t a = p.spans[s].start; a < p.spans[s].end; a += 1024u) {
          CHECK(uni.count(a >> 10));
          image.push_back(a >> 10);
        }
        at += p.spans[s].end - p.spans[s].start;
      }
      CHECK(image.size() == uni.size());
      uint64_t down = 0;
      for (uint32_t i = 0; i < n; ++i) {
        const ReplyUnit& u = p.units[i];
        CHECK(u.pre == us[i].pre && u.n == us[i].n && u.fid == us[i].fid && u.whole == us[i].whole);
        if (u.pre == 0) {
          // the kernel's walk over the packed image reads this job's units, each once, and finds its bytes
          const ReplyCover c = reply_cover(u.hpos, u.dpos, u.n);
          CHECK(uint64_t(c.e0) <= p.up && uint64_t(c.e1) <= p.up);
          const std::map<uint32_t, int> got = walk(c);
          std::set<uint32_t> back;
          for (const auto& kv : got) {
            CHECK(kv.second == 1 && kv.first < image.size());
            if (kv.first < image.size()) back.insert(image[kv.first]);
          }
          CHECK(back == brute_cover(us[i].hpos, us[i].dpos, us[i].n));
          for (uint32_t b = 0; b < 36u; b += 35u)  // the FileInfo's first and last byte
            CHECK(image[(u.hpos + b) >> 10] == (us[i].hpos + b) >> 10 && ((u.hpos + b) & 1023u) == ((us[i].hpos + b) & 1023u));
          if (u.n) {
            for (uint32_t b : {0u, u.n - 1u})
              CHECK(image[(u.dpos + b) >> 10] == (us[i].dpos + b) >> 10 &&
                    ((u.dpos + b) & 1023u) == ((us[i].dpos + b) & 1023u));
          }
        }
        const uint64_t cap = tfscrc::read_frame_cap(v[i].read);
        if (stage && u.pre != kReadParameterError && cap) {
          CHECK(p.opos[i] == u.doff && u.doff >= down && u.doff - down < 16u);
          CHECK(((u.doff + 28u) & 15u) == (uint64_t(u.dpos) & 15u));
          down = u.doff + cap;
        } else {
          CHECK(u.doff == v[i].read.frame_offset);
        }
      }
      if (stage) CHECK(p.down == down);
      else CHECK(p.down == 0);
    }
  }
  CHECK(!reply_spans_overlap(nullptr, 0, member, big));
  CHECK(noverlap >= 20u && noverlap < nlists / 2u);  // both answers are reached
  if (g_fail) return 1;
  std::printf("degraded reply plan ok: %u jobs, %u lists, %u with overlapping spans\n", njobs, nlists, noverlap);
  return 0;
}
