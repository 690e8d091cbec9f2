// ec_frames_plan_check.cpp -- stand-alone check of the host arithmetic of the
// frame-emitting chunk calls (tfs_amd/csrc/ec_frames_plan.h), meant to be built
// with the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan \
//       tools/ec_frames_plan_check.cpp -o /tmp/ec_frames_plan_check && /tmp/ec_frames_plan_check
//
// Every call check, alone and in the header's order of precedence; the bytes a
// member's out must hold; and, for frames of every shape the kernels meet (frame
// lengths 4096 and 8192, a last frame of 1 - 4 units, version 0 and 1, F on and
// off, parity and data), each frame's constants against Func::crc restated bit by
// bit over the whole body, with crc(0, D) chained from per-tile words the way the
// seal kernel chains them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tfs_amd/csrc/ec_frames_plan.h"

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
  for (int i = 0; i < TFS_EC_MAX_MEMBERS; ++i) {
    c.block_id[i] = 0x1000u + uint32_t(i) * 77u;
    c.packet_id[i] = 0xABCDEF0000000000ull + uint64_t(i) * 1000u;
  }
  return c;
}

static void check_calls() {
  static_assert(sizeof(tfs_ec_frames_cfg) == 160, "cfg layout");
  alignas(8) static char mem[16][64];
  const void* members[8];
  const void* out[8];
  for (int i = 0; i < 8; ++i) members[i] = mem[i], out[i] = mem[8 + i];
  const int src[5] = {0, 1, 2, 3, 4}, dst[3] = {5, 6, 7};
  const int32_t total = 5 * 4096 + 2048;
  auto call = [&](const tfs_ec_frames_cfg* c, const void* const* m, const void* const* o, uint64_t cap, int32_t off,
                  int32_t len) { return ecf_call_status(c, m, o, cap, total, off, len, src, 5, dst, 3); };
  tfs_ec_frames_cfg c = cfg_of(4096);
  const uint64_t big = 1u << 20;
  CHECK(call(&c, members, out, big, 0, 8192) == 0);
  CHECK(call(&c, members, out, big, 4096, total - 4096) == 0);  // a short last frame ends at total
  CHECK(call(&c, members, out, big, 0, total) == 0);
  // 2
  CHECK(call(nullptr, members, out, big, 0, 8192) == kEcfParameterError);
  CHECK(call(&c, members, nullptr, big, 0, 8192) == kEcfParameterError);
  // 3
  for (int32_t fl : {0, -4096, 1024, 4095, 4097, 6144}) {
    tfs_ec_frames_cfg b = cfg_of(fl);
    CHECK(call(&b, members, out, big, 0, 8192) == kEcfSizeInvalid);
    b.reserved = 1;  // 3 comes before 4
    b.frame_stride = 8;
    CHECK(call(&b, members, out, big, 0, 8192) == kEcfSizeInvalid);
    CHECK(call(&b, members, nullptr, big, 0, 8192) == kEcfParameterError);  // and 2 before 3
  }
  // 4: the stride
  for (uint32_t st : {8u, 4096u, 4096u + 56u, 4096u + 59u, 4096u + 60u, 4096u + 62u, 4096u + 68u}) {
    tfs_ec_frames_cfg b = cfg_of(4096, st);
    CHECK(call(&b, members, out, big, 0, 8192) == kEcfParameterError);
  }
  for (uint32_t st : {4096u + 64u, 4096u + 72u, 8192u, 1u << 20}) {
    tfs_ec_frames_cfg b = cfg_of(4096, st);
    CHECK(call(&b, members, out, 2u << 20, 0, 8192) == 0);
  }
  {
    tfs_ec_frames_cfg b = cfg_of(4096);
    b.reserved = 1;
    CHECK(call(&b, members, out, big, 0, 8192) == kEcfParameterError);
    b.reserved = -1;
    CHECK(call(&b, members, out, big, 0, 8192) == kEcfParameterError);
  }
  // 4: the frame rule
  {
    tfs_ec_frames_cfg b = cfg_of(8192);
    CHECK(call(&b, members, out, big, 4096, 8192) == kEcfParameterError);   // offset % frame_len
    CHECK(call(&b, members, out, big, 0, 4096) == kEcfParameterError);      // len % frame_len, not at the end
    CHECK(call(&b, members, out, big, 0, 12288) == kEcfParameterError);
    CHECK(call(&b, members, out, big, 16384, total - 16384) == 0);          // ... at the end
  }
  // 4: alignment of the outputs' out only
  for (int k = 1; k < 8; ++k) {
    const void* o2[8];
    memcpy(o2, out, sizeof o2);
    o2[6] = mem[14] + k;
    CHECK(call(&c, members, o2, big, 0, 8192) == kEcfParameterError);
    memcpy(o2, out, sizeof o2);
    o2[2] = mem[10] + k;  // not an output: ignored
    CHECK(call(&c, members, o2, big, 0, 8192) == 0);
  }
  // 4: out_cap
  {
    const uint64_t need = ecf_call_need(c, 8192);
    CHECK(need == (4096 + 64) + 60 + 4096);
    CHECK(call(&c, members, out, need, 0, 8192) == 0);
    CHECK(call(&c, members, out, need - 1, 0, 8192) == kEcfParameterError);
    CHECK(call(&c, members, out, 0, 0, 8192) == kEcfParameterError);
    tfs_ec_frames_cfg b = cfg_of(4096, 8192);
    CHECK(ecf_call_need(b, total) == 5 * 8192 + 60 + 2048);
    CHECK(ecf_call_need(b, 1024) == 60 + 1024);
    CHECK(ecf_call_need(b, 4096) == 60 + 4096);
    b = cfg_of(4096, 4096 + 60);
    CHECK(ecf_call_status(&b, members, out, big, total, 0, 8192, src, 5, dst, 3) == kEcfParameterError);  // % 8
  }
  // 5, and 4 before 5
  {
    CHECK(call(&c, nullptr, out, big, 0, 8192) == kEcfDataInvalid);
    const void* m2[8];
    memcpy(m2, members, sizeof m2);
    m2[3] = nullptr;
    CHECK(call(&c, m2, out, big, 0, 8192) == kEcfDataInvalid);
    CHECK(call(&c, m2, out, 10, 0, 8192) == kEcfParameterError);
    memcpy(m2, members, sizeof m2);
    m2[6] = nullptr;  // an output's entry of members: ignored
    CHECK(call(&c, m2, out, big, 0, 8192) == 0);
    const void* o2[8];
    memcpy(o2, out, sizeof o2);
    o2[7] = nullptr;
    CHECK(call(&c, members, o2, big, 0, 8192) == kEcfDataInvalid);
    CHECK(call(&c, members, o2, big, 0, 4096 + 1024) == kEcfParameterError);
    memcpy(o2, out, sizeof o2);
    o2[0] = nullptr;  // a source's entry of out: ignored
    CHECK(call(&c, members, o2, big, 0, 8192) == 0);
  }
}

static uint32_t xorshift(uint32_t& s) {
  s ^= s << 13, s ^= s >> 17, s ^= s << 5;
  return s;
}

static int check_frames() {
  int frames = 0;
  uint32_t seed = 12345;
  for (int32_t fl : {4096, 8192})
    for (int units = 1; units <= 4; ++units)
      for (int16_t version : {int16_t(0), int16_t(1), int16_t(2)})
        for (int parity = 0; parity < 2; ++parity) {
          const tfs_ec_frames_cfg c = cfg_of(fl, 0, version);
          const int32_t total = 2 * fl + 1024 * units;  // frames 0 and 1 whole, frame 2 of `units` units
          const EcfCallConst kc = ecf_call_const(fl, total);
          CHECK(kc.last_frame == 2u && kc.last_len == uint32_t(1024 * units));
          const int member = parity ? 7 : 1;
          for (uint32_t k = 0; k < 3; ++k) {
            const EcfFrameConst f = ecf_frame_const(c, member, parity != 0, total, k);
            CHECK(f.offset == k * uint32_t(fl));
            CHECK(f.length == (k < 2 ? uint32_t(fl) : uint32_t(1024 * units)));
            CHECK(f.flag == (k ? 0u : parity ? uint32_t(TFS_RAW_PARITY_DATA) : uint32_t(TFS_RAW_NORMAL_DATA)));
            CHECK(f.pid == c.packet_id[member] + k);
            CHECK(f.pow_head == (k == kc.last_frame ? kc.pow_head_last : kc.pow_head_full));
            std::vector<uint8_t> body(32 + f.length + 4);
            tfscrc::rep_info_bytes(c.block_id[member], f.offset, f.length, body.data());
            CHECK(memcmp(body.data(), f.h, 32) == 0);
            for (uint32_t i = 0; i < f.length; ++i) body[32 + i] = uint8_t(xorshift(seed));
            tfscrc::rep_le32(body.data() + 32 + f.length, f.flag);
            const uint32_t want = rep_crc_bytes(tfscrc::kRepFlag, body.data(), uint32_t(body.size()));
            // the seal's chain over per-tile words: whole tiles 4096 apart, then the last one's bytes on
            const uint32_t nc = (f.length - 1u) >> 12, lastb = f.length - (nc << 12);
            uint32_t cd = 0;
            for (uint32_t t = 0; t < nc; ++t)
              cd = multmodp(ecf_pow(4096), cd) ^ rep_crc_bytes(0u, body.data() + 32 + 4096u * t, 4096);
            cd = multmodp(ecf_pow(lastb), cd) ^ rep_crc_bytes(0u, body.data() + 32 + 4096u * nc, lastb);
            CHECK(cd == rep_crc_bytes(0u, body.data() + 32, f.length));
            CHECK(ecf_seal(f, cd, version) == (version >= 1 ? want : 0u));
            // a second witness for the head and tail: the replicate plan's seed
            CHECK((tfscrc::rep_frame_seed(c.block_id[member], f.offset, f.length, f.flag) ^ multmodp(ecf_pow(4), cd)) == want);
            uint8_t head[56];
            ecf_head_bytes(f, version, ecf_seal(f, cd, version), head);
            CHECK(head[0] == 'T' && head[1] == 'F' && head[2] == 'S' && head[3] == 'N');
            CHECK(head[4] == uint8_t(36u + f.length) && head[8] == TFS_WRITE_RAW_DATA_MESSAGE && head[9] == 0);
            CHECK(head[10] == uint8_t(version) && memcmp(head + 24, f.h, 32) == 0);
            ++frames;
          }
        }
  // a total shorter than one frame, and total == frame_len
  for (int32_t total : {1024, 3072, 4096, 8192}) {
    const EcfCallConst kc = ecf_call_const(8192, total);
    CHECK(kc.last_frame == 0u && kc.last_len == uint32_t(total));
    const tfs_ec_frames_cfg c = cfg_of(8192);
    CHECK(ecf_call_frames(8192, total) == 1u && ecf_call_need(c, total) == 60u + uint32_t(total));
  }
  return frames;
}

int main() {
  check_calls();
  const int frames = check_frames();
  printf("ec frames plan ok: %d frames\n", frames);
  return 0;
}
