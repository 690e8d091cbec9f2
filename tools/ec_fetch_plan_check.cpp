// ec_fetch_plan_check.cpp -- stand-alone check of the host arithmetic of the task
// chunk calls (tfs_amd/csrc/ec_fetch_plan.h), meant to be built with the host
// sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan \
//       tools/ec_fetch_plan_check.cpp -o /tmp/ec_fetch_plan_check && /tmp/ec_fetch_plan_check
//
// Every call check, alone and in the header's order of precedence; the expected n
// and the bytes a member's in must hold at the cuts; and, over seeded frames of
// every length the kernels take another path for (n = 1, 7, 8, 9, 1023, 4095, 4096,
// 4097, 8191 and the full frame, in frames of 4096 and 8192, versions 0, 1 and 2),
// the tile words restated lane by lane with the kernel's byte masks and negative
// powers, their chain, the join of head, data and tail against Func::crc restated
// bit by bit over the whole body, and the per-frame verdicts under damage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tfs_amd/csrc/ec_fetch_plan.h"

using namespace tfsec;
using tfscrc::multmodp;
using tfscrc::rep_crc_bytes;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static tfs_ec_frames_cfg cfg_of(int32_t frame_len, uint32_t stride = 0, int16_t version = 2) {
  tfs_ec_frames_cfg c;
  memset(&c, 0, sizeof c);
  c.frame_len = frame_len;
  c.frame_stride = stride;
  c.version = version;
  return c;
}

static void check_calls() {
  alignas(8) static char mem[16][64];
  const void* in[8];
  const void* out[8];
  for (int i = 0; i < 8; ++i) in[i] = mem[i] + 4, out[i] = mem[8 + i];
  const int src[5] = {0, 1, 2, 3, 4}, dst[3] = {5, 6, 7};
  const int32_t total = 5 * 4096 + 2048;
  const int32_t blen[5] = {total, 9000, 4096, 1, 0};
  char res[16];
  const tfs_ec_fetch_cfg f0 = {0, 0};
  auto call = [&](const tfs_ec_frames_cfg* c, const tfs_ec_fetch_cfg* f, const void* const* i, const void* const* o,
                  uint64_t cap, const void* r, int32_t off, int32_t len, bool dev = true) {
    return ecx_call_status(c, f, i, o, cap, r, total, off, len, src, blen, 5, dst, 3, dev);
  };
  tfs_ec_frames_cfg c = cfg_of(4096);
  const uint64_t big = 1u << 20;
  CHECK(call(&c, &f0, in, out, big, res, 0, 8192) == 0);
  CHECK(call(&c, &f0, in, out, big, res, 4096, total - 4096) == 0);
  // 2
  CHECK(call(nullptr, &f0, in, out, big, res, 0, 8192) == kEcfParameterError);
  CHECK(call(&c, nullptr, in, out, big, res, 0, 8192) == kEcfParameterError);
  CHECK(call(&c, &f0, nullptr, out, big, res, 0, 8192) == kEcfParameterError);
  CHECK(call(&c, &f0, in, nullptr, big, res, 0, 8192) == kEcfParameterError);
  CHECK(call(&c, &f0, in, out, big, nullptr, 0, 8192) == kEcfParameterError);
  // 3, and 2 before 3
  for (int32_t fl : {0, -4096, 1024, 6144}) {
    tfs_ec_frames_cfg b = cfg_of(fl);
    const tfs_ec_fetch_cfg fb = {8, 1};
    CHECK(call(&b, &fb, in, out, big, res, 0, 8192) == kEcfSizeInvalid);
    CHECK(call(&b, &fb, in, out, big, nullptr, 0, 8192) == kEcfParameterError);
  }
  // 4: the frames call's own checks come first
  {
    tfs_ec_frames_cfg b = cfg_of(4096, 4096 + 60);
    CHECK(call(&b, &f0, in, out, big, res, 0, 8192) == kEcfParameterError);
    CHECK(call(&c, &f0, in, out, ecf_call_need(c, 8192) - 1, res, 0, 8192) == kEcfParameterError);
    CHECK(call(&c, &f0, in, out, ecf_call_need(c, 8192), res, 0, 8192) == 0);
  }
  // 4: in_stride, reserved
  for (uint32_t st : {8u, 4096u, 4096u + 24u, 4096u + 28u, 4096u + 31u, 4096u + 36u}) {
    const tfs_ec_fetch_cfg f = {st, 0};
    CHECK(call(&c, &f, in, out, big, res, 0, 8192) == kEcfParameterError);
  }
  for (uint32_t st : {4096u + 32u, 4096u + 40u, 8192u, 1u << 20}) {
    const tfs_ec_fetch_cfg f = {st, 0};
    CHECK(call(&c, &f, in, out, big, res, 0, 8192) == 0);
  }
  {
    const tfs_ec_fetch_cfg f = {0, 1};
    CHECK(call(&c, &f, in, out, big, res, 0, 8192) == kEcfParameterError);
  }
  // 4: alignment of a source with a frame to read, device form only; 4 before 5
  for (int k = 0; k < 8; ++k) {
    if (k == 4) continue;
    const void* i2[8];
    memcpy(i2, in, sizeof i2);
    i2[1] = mem[1] + k;
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192) == kEcfParameterError);
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192, false) == 0);           // the host form places the frames itself
    CHECK(call(&c, &f0, i2, out, big, res, 12288, 4096) == 0);              // member 1 (9000 bytes) has nothing to read there
    i2[0] = nullptr;
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192) == kEcfParameterError);  // 4 before 5
    memcpy(i2, in, sizeof i2);
    i2[4] = mem[4] + k;  // block_len 0: never read
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192) == 0);
    i2[4] = in[4];
    i2[6] = mem[6] + k;  // not a source: ignored
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192) == 0);
  }
  // 5
  {
    const void* i2[8];
    memcpy(i2, in, sizeof i2);
    i2[4] = nullptr;  // block_len 0
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192) == 0);
    i2[3] = nullptr;  // block_len 1: a frame to read at offset 0 only
    CHECK(call(&c, &f0, i2, out, big, res, 0, 8192) == kEcfDataInvalid);
    CHECK(call(&c, &f0, i2, out, big, res, 4096, 4096) == 0);
    i2[2] = nullptr;  // block_len 4096
    CHECK(call(&c, &f0, i2, out, big, res, 4096, 4096) == 0);
    i2[1] = nullptr;  // block_len 9000
    CHECK(call(&c, &f0, i2, out, big, res, 8192, 4096) == kEcfDataInvalid);
    CHECK(call(&c, &f0, i2, out, big, res, 12288, 4096) == 0);
    const void* o2[8];
    memcpy(o2, out, sizeof o2);
    o2[7] = nullptr;
    CHECK(call(&c, &f0, in, o2, big, res, 0, 8192) == kEcfDataInvalid);
  }
  // the expected n and the capacity at the cuts
  CHECK(ecx_expect(9000, 0, 4096) == 4096 && ecx_expect(9000, 8192, 4096) == 808 && ecx_expect(9000, 12288, 4096) == 0);
  CHECK(ecx_expect(8192, 4096, 4096) == 4096 && ecx_expect(8192, 8192, 4096) == 0 && ecx_expect(1, 0, 4096) == 1);
  CHECK(ecx_expect(total, 5 * 4096, 2048) == 2048 && ecx_expect(0, 0, 4096) == 0);
  const int sizes[2] = {9000, 5};
  CHECK(ecx_block_len(sizes, 2, total, 1) == 5 && ecx_block_len(sizes, 2, total, 2) == total);
  CHECK(ecx_call_need(c, f0, 4096) == 36 + 4096 && ecx_call_need(c, f0, 1024) == 36 + 1024);
  CHECK(ecx_call_need(c, f0, 3 * 4096 + 2048) == 3 * (4096 + 32) + 36 + 2048);
  const tfs_ec_fetch_cfg fw = {8192, 0};
  CHECK(ecx_call_need(c, fw, 3 * 4096) == 2 * 8192 + 36 + 4096);
}

static uint32_t xorshift(uint32_t& s) {
  s ^= s << 13, s ^= s >> 17, s ^= s << 5;
  return s;
}

// x^(8 e) mod P for e of either sign (x has an order dividing 2^32 - 1).
static uint32_t xpow8(int32_t e) {
  return e >= 0 ? tfscrc::x2nmodp(uint64_t(e), 3) : tfscrc::x2nmodp(0xFFFFFFFFull - 8ull * uint64_t(-int64_t(e)), 0);
}

// ec_task_kernel's word of one tile, lane by lane: `tile` holds 4096 bytes as they lie in the incoming buffer
// (trailer and gap bytes behind the data included), nrem of them are data.
static uint32_t tile_word_by_lanes(const uint8_t* tile, int32_t nrem) {
  const int32_t pad = (nrem >= 4096 || nrem <= 0) ? 0 : 4096 - nrem;
  uint32_t word = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const uint32_t lo = 1024u * uint32_t(lane >> 4) + 8u * uint32_t(lane & 15);
    uint32_t crc = 0;
    for (int c = 0; c < 8; ++c) {
      const int32_t k = nrem - int32_t(lo + 128u * c);
      uint8_t piece[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int b = 0; b < 8 && b < k; ++b) piece[b] = tile[lo + 128u * c + uint32_t(b)];
      const uint32_t pc = rep_crc_bytes(0u, piece, 8);
      crc = c == 0 ? pc : multmodp(xpow8(128), crc) ^ pc;
    }
    word ^= multmodp(xpow8(3192 - int32_t(lo) - pad), crc);
  }
  return word;
}

static int check_frames() {
  int frames = 0;
  uint32_t seed = 2468;
  for (int32_t fl : {4096, 8192})
    for (uint32_t n : {1u, 7u, 8u, 9u, 1023u, 4095u, 4096u, 4097u, 8191u, 8192u})
      for (int16_t version : {int16_t(0), int16_t(1), int16_t(2)}) {
        if (n > uint32_t(fl)) continue;
        // the frame in a buffer with garbage behind the trailer, as a gap holds it
        std::vector<uint8_t> buf(kEcxOverhead + size_t(fl) + 64);
        for (auto& b : buf) b = uint8_t(xorshift(seed) | 1u);
        const uint32_t dfs = xorshift(seed);
        tfscrc::rep_le32(buf.data() + kEcxHead + n, dfs);
        uint8_t w[4];
        tfscrc::rep_le32(w, n);
        std::vector<uint8_t> body(w, w + 4);
        body.insert(body.end(), buf.begin() + kEcxHead, buf.begin() + kEcxHead + n + 4);
        const uint32_t want = rep_crc_bytes(tfscrc::kRepFlag, body.data(), uint32_t(body.size()));
        ecx_head_bytes(n, version, 0x1122334455667788ull + n, version >= 1 ? want : 0u, buf.data());
        // the tile words, lane by lane, and their chain
        std::vector<uint32_t> words;
        for (uint32_t t = 0; t * 4096u < uint32_t(fl); ++t) {
          const int32_t nrem = int32_t(n) - int32_t(t * 4096u);
          const uint32_t word = tile_word_by_lanes(buf.data() + kEcxHead + t * 4096u, nrem);
          const uint32_t len = nrem <= 0 ? 0u : uint32_t(nrem < 4096 ? nrem : 4096);
          CHECK(word == rep_crc_bytes(0u, buf.data() + kEcxHead + t * 4096u, len));
          words.push_back(word);
        }
        const uint32_t cd = ecx_chain(words.data(), n);
        CHECK(cd == rep_crc_bytes(0u, buf.data() + kEcxHead, n));
        CHECK(ecx_join(n, cd, dfs) == want);
        tfs_ec_fetch_result r = ecx_check(buf.data(), n);
        CHECK(r.status == 0 && r.n == n && uint32_t(r.data_file_size) == dfs && r.crc == want);
        int32_t pn = 0, pd = 0;
        CHECK(ecx_parse(buf.data(), kEcxOverhead + n, &pn, &pd) == 0 && uint32_t(pn) == n && uint32_t(pd) == dfs);
        CHECK(ecx_parse(buf.data(), kEcxOverhead + n - 1, &pn, &pd) == 1 && ecx_parse(buf.data(), 31, &pn, &pd) == 1);
        // damage: TFS_ERROR for the frame's own bytes first, then the CRC (version >= 1 only)
        const int32_t crc_err = version >= 1 ? kEcxCrcError : 0;
        auto hurt = [&](size_t at) {
          buf[at] ^= 0x10;
          const int32_t st = ecx_check(buf.data(), n).status;
          buf[at] ^= 0x10;
          return st;
        };
        CHECK(hurt(kEcxHead) == crc_err && hurt(kEcxHead + n - 1) == crc_err && hurt(kEcxHead + n + 3) == crc_err);
        CHECK(hurt(21) == crc_err);
        CHECK(hurt(0) == kEcxError && hurt(5) == kEcxError && hurt(8) == kEcxError && hurt(25) == kEcxError);
        CHECK(hurt(kEcxHead + n + 4) == 0);  // behind the trailer: not the frame's
        buf[kEcxHead] ^= 1;                  // a data flip and a wrong pcode: the lower-numbered check wins
        CHECK(hurt(9) == kEcxError);
        buf[kEcxHead] ^= 1;
        ++frames;
      }
  // an error reply: the negative length is returned, the outputs are untouched
  uint8_t err[32];
  ecx_head_bytes(uint32_t(-8016), 2, 1, 0, err);
  int32_t pn = 77, pd = 78;
  CHECK(ecx_parse(err, 32, &pn, &pd) == -8016 && pn == 77 && pd == 78);
  CHECK(ecx_parse(nullptr, 32, &pn, &pd) == kEcfParameterError && ecx_parse(err, 32, nullptr, &pd) == kEcfParameterError);
  CHECK(ecx_check(nullptr, 0).status == 0 && ecx_check(nullptr, 0).n == 0);
  return frames;
}

int main() {
  check_calls();
  const int frames = check_frames();
  printf("ec fetch plan ok: %d frames\n", frames);
  return 0;
}
