// tfs_ec_kernels.hip -- gfx950 region kernel of TFS's erasure code.
//
// The reference (ErasureCode::encode/decode, src/dataserver/erasure_code.cpp:
// 141-235 over jerasure_bitmatrix_dotprod, jerasure.cpp:304-348) works on
// units of w * packetsize = 8 * 128 bytes per device: output packet r of an
// output device is the XOR of every source packet (s, c) whose bit is set in
// row r of that device's 8 x (k*8) bitmatrix block.  XOR is associative and
// exact, so any order gives the reference's bytes.
//
// Mapping: a wave takes 4 units (4 KiB of every device) per step; lane l owns
// 8 bytes at offset 8*(l & 15) of packet c of unit (l >> 4), for all 8 packets
// c -- every load instruction reads four whole 128-byte lines.  The bitmatrix
// is expanded to 0 / ~0 words in device memory; its addresses are wave-uniform
// (scalar loads), so each bit costs one v_bitop3 (acc ^ (in & mask)) per dword.
// OG (<= 4) outputs are accumulated in registers per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfs_crc_device.h"
#include "tfs_ec_device.h"

namespace tfsec {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u32x2* gu64p;
typedef __attribute__((address_space(1))) u32x2* gu64wp;

__device__ __forceinline__ u32x2 ld64nt(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<gu64p>(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ void st64nt(uint8_t* p, u32x2 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<gu64wp>(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ uint32_t xand(uint32_t acc, uint32_t in, uint32_t m) {
  // truth table indexed (src0 << 2) | (src1 << 1) | src2: acc ^ (in & m) = 0x78
  return __builtin_amdgcn_bitop3_b32(acc, in, m, 0x78);
}

template <int OG>
__device__ __forceinline__ void ec_apply_body(const EcArgs& a, const uint32_t* __restrict__ masks) {
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint64_t ntiles = (a.units + 3) / 4;
  // wave-uniform loop counters (so the mask addresses are scalar loads)
  const uint64_t wave = uint64_t(blockIdx.x) * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t nwaves = uint64_t(gridDim.x) * (blockDim.x / 64);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const uint64_t unit = t * 4 + u;
    const bool ok = unit < a.units;
    const uint64_t base = unit * 1024u + off;
    u32x2 acc[OG][8];
#pragma unroll
    for (int o = 0; o < OG; ++o)
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[o][r] = u32x2{0u, 0u};
    u32x2 in[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = ok ? ld64nt(a.src[0] + base + 128u * c) : u32x2{0u, 0u};
    for (uint32_t s = 0; s < a.S; ++s) {
      u32x2 nx[8];
      const bool more = s + 1 < a.S;
      const uint8_t* np = a.src[more ? s + 1 : s];
#pragma unroll
      for (int c = 0; c < 8; ++c) nx[c] = (ok && more) ? ld64nt(np + base + 128u * c) : u32x2{0u, 0u};
#pragma unroll
      for (int o = 0; o < OG; ++o)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t* m = masks + ((uint32_t(o) * 8u + uint32_t(r)) * a.S + s) * 8u;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint32_t mk = m[c];
            acc[o][r].x = xand(acc[o][r].x, in[c].x, mk);
            acc[o][r].y = xand(acc[o][r].y, in[c].y, mk);
          }
        }
#pragma unroll
      for (int c = 0; c < 8; ++c) in[c] = nx[c];
    }
    if (ok) {
#pragma unroll
      for (int o = 0; o < OG; ++o)
#pragma unroll
        for (int r = 0; r < 8; ++r) st64nt(a.dst[o] + base + 128u * r, acc[o][r]);
    }
  }
}

template <int OG>
__global__ void __launch_bounds__(256) ec_apply_kernel(EcArgs a, const uint32_t* __restrict__ masks) {
  ec_apply_body<OG>(a, masks);
}


// Chunked form (K > 1): a wave takes K consecutive tiles (4K KiB of every
// member) per step of its grid stride, and the next tile's first member is
// loaded while the current tile's last member is combined, so the loads never
// stop at a tile boundary inside a chunk.
template <int OG, int K>
__global__ void __launch_bounds__(256) ec_apply_chunk_kernel(EcArgs a, const uint32_t* __restrict__ masks) {
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint64_t ntiles = (a.units + 3) / 4;
  const uint64_t nchunks = (ntiles + K - 1) / K;
  const uint64_t wave = uint64_t(blockIdx.x) * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t nwaves = uint64_t(gridDim.x) * (blockDim.x / 64);
  for (uint64_t q = wave; q < nchunks; q += nwaves) {
    const uint64_t t0 = q * K;
    const uint64_t t1 = t0 + K < ntiles ? t0 + K : ntiles;
    u32x2 in[8];
    {
      const uint64_t unit = t0 * 4 + u;
      const bool ok = unit < a.units;
#pragma unroll
      for (int c = 0; c < 8; ++c) in[c] = ok ? ld64nt(a.src[0] + unit * 1024u + off + 128u * c) : u32x2{0u, 0u};
    }
    for (uint64_t t = t0; t < t1; ++t) {
      const uint64_t unit = t * 4 + u;
      const bool ok = unit < a.units;
      const uint64_t base = unit * 1024u + off;
      const uint64_t nunit = unit + 4u;  // the next tile's unit of this lane
      const bool nok = t + 1 < t1 && nunit < a.units;
      u32x2 acc[OG][8];
#pragma unroll
      for (int o = 0; o < OG; ++o)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[o][r] = u32x2{0u, 0u};
      for (uint32_t s = 0; s < a.S; ++s) {
        u32x2 nx[8];
        const bool more = s + 1 < a.S;
        const uint8_t* np = more ? a.src[s + 1] + base : a.src[0] + nunit * 1024u + off;
        const bool lok = more ? ok : nok;
#pragma unroll
        for (int c = 0; c < 8; ++c) nx[c] = lok ? ld64nt(np + 128u * c) : u32x2{0u, 0u};
#pragma unroll
        for (int o = 0; o < OG; ++o)
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const uint32_t* m = masks + ((uint32_t(o) * 8u + uint32_t(r)) * a.S + s) * 8u;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              const uint32_t mk = m[c];
              acc[o][r].x = xand(acc[o][r].x, in[c].x, mk);
              acc[o][r].y = xand(acc[o][r].y, in[c].y, mk);
            }
          }
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = nx[c];
      }
      if (ok) {
#pragma unroll
        for (int o = 0; o < OG; ++o)
#pragma unroll
          for (int r = 0; r < 8; ++r) st64nt(a.dst[o] + base + 128u * r, acc[o][r]);
      }
    }
  }
}

#ifdef TFS_CRC_MEASURE
// The ceiling of f4's memory shape: the product's tile walk,
// grid and non-temporal loads and stores over the same members, with the
// bitmatrix combine replaced by one XOR per dword -- every output is the XOR of
// the S sources' same packet.  Not an erasure code (measurement only):
// AHEAD = 1 loads one member ahead as the product does; AHEAD = 0 issues every
// member's loads of a tile before the first XOR (a plain streaming 5:3 copy).
constexpr uint32_t kEcMaxSrc = 5;  // AHEAD = 0: the k = 5 encode of the ec line (sources past 5 are not read)
template <int OG, bool AHEAD>
__global__ void __launch_bounds__(256) ec_copy_kernel(EcArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint64_t ntiles = (a.units + 3) / 4;
  const uint64_t wave = uint64_t(blockIdx.x) * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t nwaves = uint64_t(gridDim.x) * (blockDim.x / 64);
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const uint64_t unit = t * 4 + u;
    const bool ok = unit < a.units;
    const uint64_t base = unit * 1024u + off;
    u32x2 acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = u32x2{0u, 0u};
    if (AHEAD) {
      u32x2 in[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) in[c] = ok ? ld64nt(a.src[0] + base + 128u * c) : u32x2{0u, 0u};
      for (uint32_t s = 0; s < a.S; ++s) {
        u32x2 nx[8];
        const bool more = s + 1 < a.S;
        const uint8_t* np = a.src[more ? s + 1 : s];
#pragma unroll
        for (int c = 0; c < 8; ++c) nx[c] = (ok && more) ? ld64nt(np + base + 128u * c) : u32x2{0u, 0u};
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] ^= in[c];
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = nx[c];
      }
    } else {
      u32x2 in[kEcMaxSrc][8];
#pragma unroll
      for (uint32_t s = 0; s < kEcMaxSrc; ++s)
#pragma unroll
        for (int c = 0; c < 8; ++c) in[s][c] = (ok && s < a.S) ? ld64nt(a.src[s] + base + 128u * c) : u32x2{0u, 0u};
#pragma unroll
      for (uint32_t s = 0; s < kEcMaxSrc; ++s)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] ^= in[s][c];
    }
    if (ok) {
#pragma unroll
      for (int o = 0; o < OG; ++o)
#pragma unroll
        for (int r = 0; r < 8; ++r) st64nt(a.dst[o] + base + 128u * r, acc[r]);
    }
  }
}

template <bool AHEAD>
static void launch_copy(const EcArgs& a, int og, dim3 g, dim3 b, hipStream_t stream) {
  switch (og) {
    case 1: hipLaunchKernelGGL((ec_copy_kernel<1, AHEAD>), g, b, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((ec_copy_kernel<2, AHEAD>), g, b, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((ec_copy_kernel<3, AHEAD>), g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL((ec_copy_kernel<4, AHEAD>), g, b, 0, stream, a); break;
  }
}

template <int K>
static void launch_chunk(const EcArgs& a, int og, dim3 g, dim3 b, hipStream_t stream) {
  switch (og) {
    case 1: hipLaunchKernelGGL((ec_apply_chunk_kernel<1, K>), g, b, 0, stream, a, a.masks); break;
    case 2: hipLaunchKernelGGL((ec_apply_chunk_kernel<2, K>), g, b, 0, stream, a, a.masks); break;
    case 3: hipLaunchKernelGGL((ec_apply_chunk_kernel<3, K>), g, b, 0, stream, a, a.masks); break;
    default: hipLaunchKernelGGL((ec_apply_chunk_kernel<4, K>), g, b, 0, stream, a, a.masks); break;
  }
}

#endif  // TFS_CRC_MEASURE

// The product: the grid-stride tile kernel.  Measurement build (TFS_EC_VARIANT
// 1, 2, 3): the chunked form with K = 2, 4, 8 tiles per wave step; 4, 6: the
// product's kernel over 8,192 / 2,048 workgroups striding (the product launches
// one grid step per wave).
hipError_t launch_ec_apply(const EcArgs& a, int og, int variant, hipStream_t stream) {
  if (a.units == 0) return hipSuccess;
  const uint64_t ntiles = (a.units + 3) / 4;
#ifdef TFS_CRC_MEASURE
  if (variant >= 1 && variant <= 3) {
    const int K = 1 << variant;
    uint64_t blocks = ((ntiles + K - 1) / K + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    const dim3 g(static_cast<unsigned>(blocks)), b(256);
    if (K == 2) launch_chunk<2>(a, og, g, b, stream);
    else if (K == 4) launch_chunk<4>(a, og, g, b, stream);
    else launch_chunk<8>(a, og, g, b, stream);
    return hipGetLastError();
  }
#else
  (void)variant;
#endif
  // One grid step per wave: a workgroup per 4 tiles of 4, far more workgroups than
  // fit at once, each gone after one step (8.8 % faster than a grid of 2,048
  // striding over the members, the round-2 form).
  uint64_t blocks = (ntiles + 3) / 4;
  uint64_t cap = uint64_t(1) << 30;
#ifdef TFS_CRC_MEASURE
  if (variant == 4) cap = 8192;       // measurement: 8,192 workgroups striding
  else if (variant == 6) cap = 2048;  // measurement: the round-2 product (2,048 striding)
#endif
  if (blocks > cap) blocks = cap;
  const dim3 g(static_cast<unsigned>(blocks)), b(256);
#ifdef TFS_CRC_MEASURE
  if (variant == 20 || variant == 21) {  // measurement: the 5:3 copy ceiling (ec_copy_kernel)
    if (variant == 20) launch_copy<true>(a, og, g, b, stream);
    else launch_copy<false>(a, og, g, b, stream);
    return hipGetLastError();
  }
#endif
  switch (og) {
    case 1: hipLaunchKernelGGL(ec_apply_kernel<1>, g, b, 0, stream, a, a.masks); break;
    case 2: hipLaunchKernelGGL(ec_apply_kernel<2>, g, b, 0, stream, a, a.masks); break;
    case 3: hipLaunchKernelGGL(ec_apply_kernel<3>, g, b, 0, stream, a, a.masks); break;
    default: hipLaunchKernelGGL(ec_apply_kernel<4>, g, b, 0, stream, a, a.masks); break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Degraded read (DataManagement::read_data_degrade, data_management.cpp:283-506;
// DESIGN.md §3.11).  One workgroup of kReadWaves waves per job.  The job's
// covering units [A, E) of the target are rebuilt tile by tile in
// ec_apply_kernel's lane layout (tiles count from A, so the record's FileInfo
// always lies in tile 0); wave w takes tiles w, w + kReadWaves, ..., so a 64 KiB
// record is 2 tiles per wave, not 16 in a row behind one wave's load latency.
// Every unit is stored once; a record job also checksums its payload from the
// registers that hold the rebuilt bytes.  Lane l of wave w keeps one CRC chain
// over its own 8-byte pieces, in address order: c' = shift(c, step) ^
// crc(0, piece), step = 128 bytes between packets and 4096 kReadWaves - 896
// between its tiles, with every byte outside the payload masked to zero
// (leading zeros leave a zero register alone).  After its last tile tl a
// lane's register stands at the end of its last piece, d = 4096 (nt - 1 - tl) +
// 3192 - 1024 u - 8 (l & 15) bytes before the end E' of the job's last tile,
// and the payload ends pad = E' - end bytes before E'; one multiplication by
// x^(8 (d - pad)) (ReadTables::xpow, negative exponents as inverse powers)
// brings every lane's register to the payload's end, and the XOR over the
// lanes of all waves is Func::crc(0, payload).
__device__ __forceinline__ uint32_t rd_lut4(const uint32_t* t, uint32_t x) {
  return t[x & 255u] ^ t[256u + ((x >> 8) & 255u)] ^ t[512u + ((x >> 16) & 255u)] ^ t[768u + (x >> 24)];
}
// One slice-by-4 step: slice k is "byte then k zero bytes", so the low byte takes slice 3.
__device__ __forceinline__ uint32_t rd_slice4(const uint32_t* s, uint32_t x) {
  return s[768u + (x & 255u)] ^ s[512u + ((x >> 8) & 255u)] ^ s[256u + ((x >> 16) & 255u)] ^ s[x >> 24];
}
// a * b mod P, reflected (crc_math.h multmodp), branch-free.
__device__ __forceinline__ uint32_t rd_multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 31; i >= 0; --i) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}
__device__ __forceinline__ uint64_t rd_low_bytes(int64_t k) {  // 0xff in the k lowest bytes, k clamped to 0..8
  return k <= 0 ? 0ull : k >= 8 ? ~0ull : (1ull << (8 * k)) - 1ull;
}

__global__ void __launch_bounds__(64 * kReadWaves) ec_read_kernel(ReadArgs a) {
  __shared__ uint32_t lt[3 * 1024];             // slice, step_packet, step_tile
  __shared__ uint32_t hdr[12];                  // the job's rebuilt FileInfo (36 bytes), from wave 0's tile 0
  __shared__ uint32_t part[kReadWaves];         // the waves' CRC parts
  {
    const uint32_t* g = reinterpret_cast<const uint32_t*>(a.tab);
    for (uint32_t i = threadIdx.x; i < 3u * 1024u; i += 64u * kReadWaves) lt[i] = g[i];
  }
  __syncthreads();
  const uint32_t* sl = lt;
  const uint32_t* stp = lt + 1024;
  const uint32_t* stt = lt + 2048;
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* hdr8 = reinterpret_cast<uint8_t*>(hdr);
  uint32_t bad = 0;
  // every wave of the workgroup walks the same jobs, so the barriers below are uniform
  for (uint32_t j = blockIdx.x; j < a.n; j += gridDim.x) {
    const ReadJob jb = a.jobs[j];
    const bool range = (jb.flags & kReadRange) != 0u;
    uint32_t A = 0, E = 0;  // the covering range
    int32_t status = read_job_check(jb, a.size, a.out_cap, &A, &E);
    if (status != tfscrc::kSuccess) {  // rejected before reading: nothing written
      if (threadIdx.x == 0) {
        a.out_crc[j] = 0u;
        a.out_status[j] = status;
      }
      ++bad;
      continue;
    }
    const uint32_t nt = (E - A + 4095u) >> 12;
    const uint32_t H = uint32_t(jb.offset);                  // the FileInfo's first byte
    const uint32_t P0 = H + uint32_t(tfscrc::kFileInfoSize);  // payload [P0, P1)
    const uint32_t P1 = H + uint32_t(jb.size);
    uint8_t* const outp = a.out + jb.out_offset;
    uint32_t crc = 0;
    u32x2 in[8];
    {
      const uint32_t pu = A + 4096u * wv + 1024u * u;
      const bool ok = wv < nt && pu < E;
#pragma unroll
      for (int c = 0; c < 8; ++c) in[c] = ok ? ld64nt(a.src[0] + pu + off + 128u * c) : u32x2{0u, 0u};
    }
    for (uint32_t t = wv; t < nt; t += kReadWaves) {
      const uint32_t pu = A + 4096u * t + 1024u * u;  // < 2^31 + 4096
      const bool ok = pu < E;
      const uint32_t base = pu + off;
      const bool nok = t + kReadWaves < nt && pu + 4096u * kReadWaves < E;
      u32x2 acc[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = u32x2{0u, 0u};
      for (uint32_t s = 0; s < a.S; ++s) {
        // the next member's loads (after the last member, the next tile's first) go out before this one's XORs
        u32x2 nx[8];
        const bool more = s + 1 < a.S;
        const uint8_t* np = more ? a.src[s + 1] + base : a.src[0] + base + 4096u * kReadWaves;
        const bool lok = more ? ok : nok;
#pragma unroll
        for (int c = 0; c < 8; ++c) nx[c] = lok ? ld64nt(np + 128u * c) : u32x2{0u, 0u};
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t* m = a.masks + (uint32_t(r) * a.S + s) * 8u;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint32_t mk = m[c];
            acc[r].x = xand(acc[r].x, in[c].x, mk);
            acc[r].y = xand(acc[r].y, in[c].y, mk);
          }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = nx[c];
      }
      if (ok) {
#pragma unroll
        for (int r = 0; r < 8; ++r) st64nt(outp + (base - A) + 128u * r, acc[r]);
      }
      if (range) continue;
      if (t == 0) {  // the FileInfo lies in [H, H + 36), inside tile 0 (wave 0's): its bytes go to LDS
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint32_t q = base + 128u * c;
          if (q + 8u > H && q < P0) {
            const uint64_t v = uint64_t(acc[c].x) | (uint64_t(acc[c].y) << 32);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
              const uint32_t p = q + uint32_t(b) - H;  // wraps below H
              if (p < uint32_t(tfscrc::kFileInfoSize)) hdr8[p] = uint8_t(v >> (8 * b));
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t q = base + 128u * c;
        uint32_t lo = acc[c].x, hi = acc[c].y;
        const int64_t sk = int64_t(P0) - int64_t(q), ek = int64_t(P1) - int64_t(q);
        if (sk > 0 || ek < 8) {  // a piece that is not all payload
          const uint64_t mk = ek <= sk ? 0ull : rd_low_bytes(ek) & ~rd_low_bytes(sk);
          lo &= uint32_t(mk);
          hi &= uint32_t(mk >> 32);
        }
        const uint32_t piece = rd_slice4(sl, rd_slice4(sl, lo) ^ hi);  // crc(0, the piece's 8 bytes)
        crc = rd_lut4(c == 0 ? stt : stp, crc) ^ piece;
      }
    }
    if (range) {
      if (threadIdx.x == 0) {
        a.out_crc[j] = 0u;
        a.out_status[j] = tfscrc::kSuccess;
      }
      continue;
    }
    {
      const uint32_t tl = nt - 1u - ((nt - 1u - wv) & (kReadWaves - 1u));  // this wave's last tile (nt > wv)
      const int32_t dl = wv < nt ? int32_t(4096u * (nt - 1u - tl)) + 3192 - int32_t(1024u * u + off) : 0;
      const int32_t pad = int32_t(A + 4096u * nt - P1);
      crc = rd_multmodp(a.tab->xpow[kReadPowBias + dl - pad], crc);  // a wave without a tile holds 0
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
      if (lane == 0) part[wv] = crc;
    }
    __syncthreads();  // the parts and the header bytes are in LDS
    if (threadIdx.x == 0) {
      uint32_t v = 0;
#pragma unroll
      for (int w = 0; w < kReadWaves; ++w) v ^= part[w];
      const uint64_t id = uint64_t(hdr[0]) | (uint64_t(hdr[1]) << 32);
      const int32_t fsize = int32_t(hdr[3]);
      const uint32_t fcrc = hdr[8];
      if (id != jb.file_id) status = tfscrc::kExitFileInfoError;
      else if (fsize != jb.size) status = tfscrc::kExitSyncFileError;
      else if (fcrc != v) status = tfscrc::kExitCheckCrcError;
      a.out_crc[j] = v;
      a.out_status[j] = status;
      if (status != tfscrc::kSuccess) ++bad;
    }
    __syncthreads();  // before the next job's parts and header bytes
  }
  if (threadIdx.x == 0 && bad && a.n_bad) atomicAdd(a.n_bad, bad);
}

hipError_t launch_ec_read(const ReadArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = a.n < kReadMaxGrid ? a.n : kReadMaxGrid;
  hipLaunchKernelGGL(ec_read_kernel, dim3(blocks), dim3(64 * kReadWaves), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Degraded read reply (include/tfs_ec_read.h): ec_read_kernel's
// workgroup per job with the reply frame as its destination.  The covering set is
// the units of the FileInfo and the units of the slice [D0, D1) (reply_cover):
// tile 0 always holds the FileInfo, and when the slice's units are disjoint from
// it the slice's tiles count from the slice's first unit -- a wave's tiles are
// still kReadWaves tiles apart, so the chain's two steps are ec_read_kernel's.
// Bytes outside the slice are masked out of the chain, pad is taken from D1, and
// the XOR over lanes and waves is c = crc(0, slice).  The rebuilt bytes of a
// piece go from its two registers to frame + 28 + (q - D0): one 8-byte store for a
// piece inside the slice (non-temporal when frame + 28 and D0 agree mod 8, at any
// byte address otherwise -- the unaligned access mode serves it as one
// instruction), byte stores for the slice's bytes of the two edge pieces.  No
// covering unit is written anywhere.  After the waves' parts meet in LDS wave 0
// decides the status from the FileInfo in LDS before any header byte exists,
// carries pre ^ c over the trailer's dwords and stores the 28 leading bytes and
// the trailer.  A failed job's verdict goes to the other waves through LDS: every
// wave waits for its own stores, the workgroup meets once more, and only then
// wave 0 stores the sealed set_length(status) frame over the data bytes.
__device__ __forceinline__ void st64any(uint8_t* p, u32x2 v) {
  typedef u32x2 __attribute__((aligned(1))) u32x2u;
  *reinterpret_cast<__attribute__((address_space(1))) u32x2u*>(reinterpret_cast<uintptr_t>(p)) = v;
}

__global__ void __launch_bounds__(64 * kReadWaves) ec_read_reply_kernel(ReplyArgs a) {
  __shared__ uint32_t lt[3 * 1024];             // slice, step_packet, step_tile
  __shared__ uint32_t hdr[12];                  // the job's rebuilt FileInfo (36 bytes), from wave 0's tile 0
  __shared__ uint32_t part[kReadWaves];         // the waves' CRC parts
  __shared__ uint32_t failed;                   // wave 0's verdict, for the waves that wait on it
  {
    const uint32_t* g = reinterpret_cast<const uint32_t*>(a.tab);
    for (uint32_t i = threadIdx.x; i < 3u * 1024u; i += 64u * kReadWaves) lt[i] = g[i];
  }
  __syncthreads();
  const uint32_t* sl = lt;
  const uint32_t* stp = lt + 1024;
  const uint32_t* stt = lt + 2048;
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* hdr8 = reinterpret_cast<uint8_t*>(hdr);
  uint32_t bad = 0;
  // every wave of the workgroup walks the same jobs, so the barriers below are uniform
  for (uint32_t j = blockIdx.x; j < a.n; j += gridDim.x) {
    const ReplyUnit jb = a.units[j];
    int32_t status = jb.pre;
    const uint32_t pcode = jb.type_ver & 0xffffu;
    const bool v2 = pcode != uint32_t(TFS_RESP_READ_DATA_MESSAGE);
    const uint32_t cap = tfscrc::kReadHead + jb.n + jb.tlen;  // the span a served job may write
    const ReplyCover cv = reply_cover(jb.hpos, jb.dpos, jb.n);
    if (status != tfscrc::kExitParameterError) {  // the plan's bounds, held once more: nothing is read past a member
      const uint64_t span = status == tfscrc::kSuccess ? uint64_t(cap) : (v2 ? 32u : 28u);  // or written past out
      if (jb.doff > a.out_cap || span > a.out_cap - jb.doff) status = tfscrc::kExitParameterError;
      else if (status == tfscrc::kSuccess && (cv.e0 > uint32_t(a.size) || cv.e1 > uint32_t(a.size)))
        status = tfscrc::kExitParameterError;
    }
    if (status == tfscrc::kExitParameterError) {  // refused: only the result is written
      if (threadIdx.x == 0) a.results[j] = tfs_read_result{status, 0u, 0u, 0u};
      ++bad;
      continue;
    }
    uint8_t* const frame = a.out + jb.doff;
    uint32_t crc = 0;
    if (status == tfscrc::kSuccess) {
      const uint32_t nt = cv.nt;
      const uint32_t H = jb.hpos, P0 = H + uint32_t(tfscrc::kFileInfoSize);  // the FileInfo is [H, P0)
      const uint32_t D0 = jb.dpos, D1 = D0 + jb.n;                           // the slice
      uint8_t* const fb = frame + tfscrc::kReadHead - D0;  // member byte q of the slice lands at fb + q
      const bool al8 = (reinterpret_cast<uintptr_t>(fb) & 7u) == 0u;
      u32x2 in[8];
      {
        const uint32_t pu = (wv == 0u ? cv.hA : cv.tb1 + 4096u * wv) + 1024u * u;
        const bool ok = wv < nt && pu < (wv == 0u ? cv.e0 : cv.e1);
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = ok ? ld64nt(a.src[0] + pu + off + 128u * c) : u32x2{0u, 0u};
      }
      for (uint32_t t = wv; t < nt; t += kReadWaves) {
        const uint32_t pu = (t == 0u ? cv.hA : cv.tb1 + 4096u * t) + 1024u * u;  // < 2^31 + 4096
        const bool ok = pu < (t == 0u ? cv.e0 : cv.e1);
        const uint32_t base = pu + off;
        // this lane's unit of the wave's next tile, never tile 0
        const uint32_t nbase = cv.tb1 + 4096u * (t + kReadWaves) + 1024u * u + off;
        const bool nok = t + kReadWaves < nt && nbase - off < cv.e1;
        u32x2 acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = u32x2{0u, 0u};
        for (uint32_t s = 0; s < a.S; ++s) {
          // the next member's loads (after the last member, the next tile's first) go out before this one's XORs
          u32x2 nx[8];
          const bool more = s + 1 < a.S;
          const uint8_t* np = more ? a.src[s + 1] + base : a.src[0] + nbase;
          const bool lok = more ? ok : nok;
#pragma unroll
          for (int c = 0; c < 8; ++c) nx[c] = lok ? ld64nt(np + 128u * c) : u32x2{0u, 0u};
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const uint32_t* m = a.masks + (uint32_t(r) * a.S + s) * 8u;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              const uint32_t mk = m[c];
              acc[r].x = xand(acc[r].x, in[c].x, mk);
              acc[r].y = xand(acc[r].y, in[c].y, mk);
            }
          }
#pragma unroll
          for (int c = 0; c < 8; ++c) in[c] = nx[c];
        }
        if (t == 0 && ok) {  // the FileInfo lies in [H, H + 36), inside tile 0 (wave 0's): its bytes go to LDS
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint32_t q = base + 128u * c;
            if (q + 8u > H && q < P0) {
              const uint64_t v = uint64_t(acc[c].x) | (uint64_t(acc[c].y) << 32);
#pragma unroll
              for (int b = 0; b < 8; ++b) {
                const uint32_t p = q + uint32_t(b) - H;  // wraps below H
                if (p < uint32_t(tfscrc::kFileInfoSize)) hdr8[p] = uint8_t(v >> (8 * b));
              }
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint32_t q = base + 128u * c;
          uint32_t lo = acc[c].x, hi = acc[c].y;
          const int64_t sk = int64_t(D0) - int64_t(q), ek = int64_t(D1) - int64_t(q);
          if (sk <= 0 && ek >= 8) {  // a piece inside the slice: one store
            if (ok) {
              if (al8) st64nt(fb + q, acc[c]);
              else st64any(fb + q, acc[c]);
            }
          } else {  // an edge piece, or one outside the slice: its slice bytes one by one, the rest out of the chain
            const uint64_t mk = ek <= sk ? 0ull : rd_low_bytes(ek) & ~rd_low_bytes(sk);
            if (ok && mk) {
              const uint64_t v = uint64_t(lo) | (uint64_t(hi) << 32);
              for (int b = 0; b < 8; ++b)
                if ((mk >> (8 * b)) & 1ull) fb[q + uint32_t(b)] = uint8_t(v >> (8 * b));
            }
            lo &= uint32_t(mk);
            hi &= uint32_t(mk >> 32);
          }
          const uint32_t piece = rd_slice4(sl, rd_slice4(sl, lo) ^ hi);  // crc(0, the piece's 8 bytes)
          crc = rd_lut4(c == 0 ? stt : stp, crc) ^ piece;
        }
      }
      if (jb.n != 0u) {
        const uint32_t tl = nt - 1u - ((nt - 1u - wv) & (kReadWaves - 1u));  // this wave's last tile (nt > wv)
        const int32_t dl = wv < nt ? int32_t(4096u * (nt - 1u - tl)) + 3192 - int32_t(1024u * u + off) : 0;
        const int32_t pad = int32_t(cv.tb1 + 4096u * nt - D1);  // 0 .. 4095: the last tile's end less the slice's
        crc = rd_multmodp(a.tab->xpow[kReadPowBias + dl - pad], crc);  // a wave without a slice byte holds 0
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
      }
      if (lane == 0) part[wv] = crc;
    }
    __syncthreads();  // the parts and the header bytes are in LDS
    const ReplyUnit jv = a.units[j];  // read again: the walk above need not carry what only the verdict uses
    tfs_read_result res{status, 0u, 0u, 0u};
    // the 28 leading bytes: the V1 header and the body's first word, a byte per lane
    auto store_head = [&](uint32_t body_len, uint32_t fcrc, uint32_t word6) {
      if (uint32_t(lane) < tfscrc::kReadHead) {
        const uint32_t k = uint32_t(lane) >> 2;
        const uint32_t w = k == 0u   ? tfscrc::kPacketFlagV1
                           : k == 1u ? body_len
                           : k == 2u ? jv.type_ver
                           : k == 3u ? uint32_t(jv.pid)
                           : k == 4u ? uint32_t(jv.pid >> 32)
                           : k == 5u ? fcrc
                                     : word6;
        frame[lane] = uint8_t(w >> (8u * (uint32_t(lane) & 3u)));
      }
      if (lane == 0) {
        res.status = status;
        res.frame_len = 24u + body_len;
        res.frame_crc = fcrc;
        a.results[j] = res;
      }
    };
    const bool ver0 = int16_t(uint16_t(jv.type_ver >> 16)) < 1;  // a version-0 request: no header CRC
    if (wv == 0u) {  // the verdict, before any header byte
      uint32_t c = 0;
      if (status == tfscrc::kSuccess) {
#pragma unroll
        for (int w = 0; w < kReadWaves; ++w) c ^= part[w];
        const uint64_t id = uint64_t(hdr[0]) | (uint64_t(hdr[1]) << 32);
        if (id != jv.fid) status = tfscrc::kExitFileInfoError;
        else if (int32_t(hdr[3]) != jv.size) status = tfscrc::kExitSyncFileError;
        else if ((hdr[7] & jv.refuse) != 0u) status = tfscrc::kExitFileInfoError;
        else if (jv.whole && c != hdr[8]) status = tfscrc::kExitCheckCrcError;
        res.file_crc = jv.whole ? c : 0u;
      }
      if (lane == 0) failed = status != tfscrc::kSuccess ? 1u : 0u;
      if (status == tfscrc::kSuccess) {
        uint32_t fcrc = jv.pre_seed ^ c;  // crc(FLAG, le32(n) || data)
        if (jv.tlen) {                    // the trailer's dwords: le32(36) | FileInfo with size_ less 36, or le32(0)
          const bool info = jv.tlen > 4u;
          const uint32_t size_less = hdr[3] - uint32_t(tfscrc::kFileInfoSize);
          fcrc = rd_slice4(sl, fcrc ^ (info ? uint32_t(tfscrc::kFileInfoSize) : 0u));
          if (info) {
#pragma unroll
            for (uint32_t k = 0; k < 9u; ++k) fcrc = rd_slice4(sl, fcrc ^ (k == 3u ? size_less : hdr[k]));
          }
          if (uint32_t(lane) < jv.tlen) {  // lane l stores trailer byte l: the length word, then FileInfo byte l - 4
            const uint32_t l4 = uint32_t(lane) - 4u;
            const uint32_t b = lane < 4 ? (lane == 0 && info ? uint32_t(tfscrc::kFileInfoSize) : 0u)
                               : (l4 >> 2) == 3u ? size_less >> (8u * (l4 & 3u))
                                                 : uint32_t(hdr8[l4 < uint32_t(tfscrc::kFileInfoSize) ? l4 : 0u]);
            frame[tfscrc::kReadHead + jv.n + uint32_t(lane)] = uint8_t(b);
          }
        }
        store_head(4u + jv.n + jv.tlen, ver0 ? 0u : fcrc, jv.n);
      }
    }
    __syncthreads();  // before the next job's parts and header bytes; the verdict is known to every wave
    if (failed) {
      // set_length(status): le32(status), and le32(0) for the V2 / V3 replies.  The le32(0) lies over the first data
      // bytes, which another wave may have stored: every wave's stores are complete before wave 0 stores over them.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (wv == 0u) {
        __threadfence();
        uint32_t fcrc = rd_slice4(sl, tfscrc::kPacketFlagV1 ^ uint32_t(status));
        if (v2) {
          fcrc = rd_slice4(sl, fcrc);
          if (lane < 4) frame[tfscrc::kReadHead + uint32_t(lane)] = 0;
        }
        store_head(v2 ? 8u : 4u, ver0 ? 0u : fcrc, uint32_t(status));
        if (lane == 0) ++bad;
      }
    }
  }
  if (threadIdx.x == 0 && bad && a.n_bad) atomicAdd(a.n_bad, bad);
}

hipError_t launch_ec_read_reply(const ReplyArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = a.n < kReadMaxGrid ? a.n : kReadMaxGrid;
  hipLaunchKernelGGL(ec_read_reply_kernel, dim3(blocks), dim3(64 * kReadWaves), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The session passes: marshalling, reinstate and scrub
// are ec_apply_kernel's tile walk over one chunk of the family, one wave per
// 4 KiB tile and one grid step per wave, with the payload CRCs of the data
// members' records taken from the registers the code goes through.  What the
// three kernels share is written once here: the record walk, the tile's
// prologue, the combine of one member, and the launch.

// A load / store at a wave-uniform pointer plus a 32-bit lane offset (a chunk is shorter than 2^31 bytes): the
// address stays "scalar base + lane offset" for the instruction, so the lanes keep one offset register for every
// member and packet.
__device__ __forceinline__ u32x2 ld64nt_at(const uint8_t* p, uint32_t o) {
  typedef const __attribute__((address_space(1))) uint8_t* g8p;
  return __builtin_nontemporal_load(reinterpret_cast<gu64p>(reinterpret_cast<g8p>(reinterpret_cast<uintptr_t>(p)) + o));
}
__device__ __forceinline__ void st64nt_at(uint8_t* p, uint32_t o, u32x2 v) {
  typedef __attribute__((address_space(1))) uint8_t* g8wp;
  __builtin_nontemporal_store(v, reinterpret_cast<gu64wp>(reinterpret_cast<g8wp>(reinterpret_cast<uintptr_t>(p)) + o));
}

// The lane's eight pieces of one member's tile (packet c at base + 128 c), or zeros.  EACH == false: one branch
// around the eight loads, where a condition per load costs the wave eight changes of its execution mask.
// EACH == true: the condition per load; ec_reinstate_kernel's calls of 1 MiB are faster with it.
template <bool EACH>
__device__ __forceinline__ void load_pieces(u32x2 (&v)[8], const uint8_t* p, uint32_t base, bool on) {
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = (EACH && on) ? ld64nt_at(p, base + 128u * c) : u32x2{0u, 0u};
  if (!EACH && on) {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = ld64nt_at(p, base + 128u * c);
  }
}

// What a wave knows about its tile for the record walk.
struct RecordWalk {
  const uint32_t* sl;   // LDS: slice
  const uint32_t* stp;  // LDS: step_packet
  uint32_t T, tile_lo, tile_hi;  // the tile, counted from the members' first byte, and its bytes (<= 2^31)
  uint32_t q0;                   // this lane's piece of packet 0, as a member offset
  uint32_t ntiles;
  int32_t dl;                    // from the end of the lane's last piece to the tile's end
  int lane;
  uint32_t *cont, *tail;
  uint8_t* hdr8;
};

// The CRC side of one data member's tile: pc[] holds the lane's eight pieces of it (in[] while a source sits
// there, acc[o][*] for a rebuilt member), `slot` names the member's rows of first and cont, rend is one past its
// last record.  The wave walks the records from first[slot][T] while their FileInfo starts before the tile's
// end; every value below but the lanes' pieces is scalar.  The intersection of a payload [P0, P1) with the tile
// is a segment: every lane chains crc(0, piece) over its eight pieces with the 128-byte step (bytes outside the
// payload masked to zero), then one multiplication by x^(8 (d_lane - pad)) brings its register to the segment's
// end -- the tile's end (pad = 0) when the payload runs on, P1 otherwise -- and the XOR over the wave goes to
// cont[slot][T] or tail[rec].  One writer per word, no atomics; the FileInfo bytes that pass by are stored to
// hdr[rec] because the caller reuses the chunk buffers before the fold runs.
// QREC: the lane's piece offsets are derived from the record-dependent mask too, so that the eight of them are
// made where a record needs them and are not held across the member loop.
template <bool QREC>
__device__ __forceinline__ void record_walk(const u32x2 (&pc)[8], const RecordWalk& w, uint32_t slot, uint32_t rend,
                                            const MarshalTables* __restrict__ tab, const MarshalRec* __restrict__ recs,
                                            const uint32_t* __restrict__ first) {
  const uint32_t tile_lo = w.tile_lo, tile_hi = w.tile_hi;
  for (uint32_t r = __builtin_amdgcn_readfirstlane(first[size_t(slot) * w.ntiles + w.T]); r < rend; ++r) {
    const uint32_t H = __builtin_amdgcn_readfirstlane(recs[r].H);
    const uint32_t P1 = __builtin_amdgcn_readfirstlane(recs[r].P1);
    if (H >= tile_hi) break;
    const uint32_t P0 = H + uint32_t(tfscrc::kFileInfoSize);
    // One scalar mask that depends on the record keeps everything derived from the pieces inside this walk:
    // without it the compiler computes the byte fields and first table steps of every piece ahead of the walk,
    // for tiles that use none of them, and holds 250 registers.  first[] never names a record that ends at or
    // before the tile's start, so the mask is all ones.
    const uint32_t live = 0u - uint32_t(P1 > tile_lo);
    const uint32_t q0 = QREC ? w.q0 + ~live : w.q0;  // ~live is 0
    if (P0 > tile_lo) {  // FileInfo bytes in this tile
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t q = q0 + 128u * c;
        if (q + 8u > H && q < P0) {
          const uint64_t v = uint64_t(pc[c].x & live) | (uint64_t(pc[c].y & live) << 32);
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const uint32_t p = q + uint32_t(b) - H;  // wraps below H
            if (p < uint32_t(tfscrc::kFileInfoSize)) w.hdr8[size_t(r) * (4u * kMarshalHdrWords) + p] = uint8_t(v >> (8 * b));
          }
        }
      }
    }
    if (P0 >= tile_hi) continue;  // the payload starts in a later tile
    uint32_t crc = 0;
    if (P0 <= tile_lo && P1 >= tile_hi) {  // the tile lies inside the payload: no byte masks
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t piece = rd_slice4(w.sl, rd_slice4(w.sl, pc[c].x & live) ^ (pc[c].y & live));
        crc = c == 0 ? piece : rd_lut4(w.stp, crc) ^ piece;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t q = q0 + 128u * c;
        uint32_t lo = pc[c].x & live, hi = pc[c].y & live;
        const int64_t sk = int64_t(P0) - int64_t(q), ek = int64_t(P1) - int64_t(q);
        if (sk > 0 || ek < 8) {  // a piece that is not all payload
          const uint64_t mk = ek <= sk ? 0ull : rd_low_bytes(ek) & ~rd_low_bytes(sk);
          lo &= uint32_t(mk);
          hi &= uint32_t(mk >> 32);
        }
        const uint32_t piece = rd_slice4(w.sl, rd_slice4(w.sl, lo) ^ hi);
        crc = c == 0 ? piece : rd_lut4(w.stp, crc) ^ piece;
      }
    }
    const bool on = P1 > tile_hi;  // the payload runs past this tile
    const int32_t pad = P1 >= tile_hi ? 0 : int32_t(tile_hi - P1);
    crc = rd_multmodp(tab->xpow[kMarshalPowBias + w.dl - pad], crc);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
    if (w.lane == 0) {
      if (on) w.cont[size_t(slot) * w.ntiles + w.T] = crc;
      else w.tail[r] = crc;
    }
  }
}

// The prologue of a tile: whether this lane's unit lies inside the chunk (ok), its piece of packet 0 as a chunk
// offset (base), the first member's pieces (EACH: load_pieces' form) in in[] and the walk's context in w.
// The first member's loads go out before the tables are staged: a wave lives for one tile only.  TABLES ==
// false (a launch without a walk) stages nothing and leaves lt alone.  Returns false for a wave past the
// chunk's last tile: one grid step per wave.
template <bool TABLES, bool EACH>
__device__ __forceinline__ bool tile_begin(const MarshalArgs& m, const MarshalTables* __restrict__ tab, uint32_t* lt,
                                           u32x2 (&in)[8], bool& ok, uint32_t& base, RecordWalk& w) {
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint64_t ntl = (m.ec.units + 3) / 4;  // tiles of this chunk
  const uint64_t t = uint64_t(blockIdx.x) * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t unit = t * 4 + u;
  ok = t < ntl && unit < m.ec.units;
  base = uint32_t(unit) * 1024u + off;  // a chunk is shorter than 2^31 bytes
  load_pieces<EACH>(in, m.ec.src[0], base, ok);
  if (TABLES) {
    const uint32_t* g = reinterpret_cast<const uint32_t*>(tab);
    for (uint32_t i = threadIdx.x; i < 2u * 1024u; i += 256u) lt[i] = g[i];
    __syncthreads();
  }
  if (t >= ntl) return false;
  w.sl = lt;
  w.stp = lt + (TABLES ? 1024 : 0);
  w.T = m.tile0 + uint32_t(t);
  w.tile_lo = w.T << 12;
  w.tile_hi = w.tile_lo + 4096u;
  w.q0 = w.tile_lo + 1024u * u + off;
  w.ntiles = m.ntiles;
  w.dl = 3192 - int32_t(1024u * u + off);
  w.lane = lane;
  w.cont = m.cont;
  w.tail = m.tail;
  w.hdr8 = reinterpret_cast<uint8_t*>(m.hdr);
  return true;
}

// Member s's pieces into the launch's outputs.  The masks are a __restrict__ kernel parameter of their own, as
// are the walk's read-only arrays: the stores of the CRC side inside the member loop must not turn the masks'
// scalar loads into vector loads.
template <int OG>
__device__ __forceinline__ void combine(u32x2 (&acc)[OG][8], const u32x2 (&in)[8], const uint32_t* __restrict__ masks,
                                        uint32_t S, uint32_t s) {
#pragma unroll
  for (int o = 0; o < OG; ++o)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t* m = masks + ((uint32_t(o) * 8u + uint32_t(r)) * S + s) * 8u;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t mk = m[c];
        acc[o][r].x = xand(acc[o][r].x, in[c].x, mk);
        acc[o][r].y = xand(acc[o][r].y, in[c].y, mk);
      }
    }
}

// A wave per tile, four to the workgroup; k[og - 1] is the kernel for og outputs.
template <typename Args>
using SessionKernel = void (*)(Args, const uint32_t*, const MarshalTables*, const MarshalRec*, const uint32_t*);

template <typename Args>
static hipError_t launch_session(const SessionKernel<Args> (&k)[kMaxOutGroup], const Args& a, const MarshalArgs& m, int og,
                                 hipStream_t stream) {
  if (m.ec.units == 0) return hipSuccess;
  const uint64_t ntl = (m.ec.units + 3) / 4;
  hipLaunchKernelGGL(k[og - 1], dim3(static_cast<unsigned>((ntl + 3) / 4)), dim3(256), 0, stream, a, m.ec.masks, m.tab,
                     m.recs, m.first);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Marshalling (MarshallingTask::do_marshalling, task.cpp:1173-1355; DESIGN.md
// §3.12).  While member s's eight pieces sit in in[], the same registers feed
// the record walk of data member s.  The walk's QREC is off: with it the
// OG = 1, 2 and 4 forms gain a wave per SIMD in the build figures, but the
// probe's whole-member encode calls (OG = 3) are 3 to 7 % slower.
template <int OG>
__global__ void __launch_bounds__(256, OG <= 3 ? 4 : 3)  // waves per SIMD the register budget is held to (no spill)
    ec_marshal_kernel(MarshalArgs a, const uint32_t* __restrict__ masks, const MarshalTables* __restrict__ tab,
                      const MarshalRec* __restrict__ recs, const uint32_t* __restrict__ first) {
  __shared__ uint32_t lt[2 * 1024];  // slice, step_packet
  u32x2 in[8];
  bool ok;
  uint32_t base;
  RecordWalk w;
  if (!tile_begin<true, false>(a, tab, lt, in, ok, base, w)) return;
  const uint32_t S = a.ec.S;
  u32x2 acc[OG][8] = {};
  for (uint32_t s = 0; s < S; ++s) {
    u32x2 nx[8];
    const bool more = s + 1 < S;
    load_pieces<false>(nx, a.ec.src[more ? s + 1 : s], base, ok && more);
    combine<OG>(acc, in, masks, S, s);
    record_walk<false>(in, w, s, a.mend[s], tab, recs, first);
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = nx[c];
  }
  if (ok) {
#pragma unroll
    for (int o = 0; o < OG; ++o)
#pragma unroll
      for (int r = 0; r < 8; ++r) st64nt_at(a.ec.dst[o], base + 128u * r, acc[o][r]);
  }
}

hipError_t launch_ec_marshal(const MarshalArgs& a, int og, hipStream_t stream) {
  static constexpr SessionKernel<MarshalArgs> k[] = {ec_marshal_kernel<1>, ec_marshal_kernel<2>, ec_marshal_kernel<3>,
                                                     ec_marshal_kernel<4>};
  return launch_session(k, a, a, og, stream);
}

// The fold: a wave per record.  The tiles t0 .. tl - 1 that the payload runs
// through each left crc(0, its payload bytes of that tile) in cont; lane l chains a
// run of them (c' = shift(c, 4096) ^ cont[t]), one multiplication by
// pow_tile[tl - e] brings its register to the start of the last tile, and the XOR
// over the wave, moved on by P1 - T_last bytes, meets tail[rec].  Then the
// FileInfo checks of tfs_block_verify, on the bytes kept in hdr.  No payload byte
// is read.
__global__ void __launch_bounds__(256) ec_marshal_fold_kernel(MarshalFoldArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= a.n) return;
  const MarshalRec rc = a.recs[r];
  const uint32_t P0 = rc.H + uint32_t(tfscrc::kFileInfoSize), P1 = rc.P1;
  const uint32_t t0 = P0 >> 12, tl = (P1 - 1u) >> 12;  // a record that ends on a tile's end ends in that tile
  const uint32_t nc = tl - t0;
  uint32_t c = 0;
  if (nc) {
    const uint32_t* cont = a.cont + size_t(a.rec_member[r]) * a.ntiles;
    const uint32_t R = (nc + 63u) / 64u;
    const uint32_t b = min(t0 + lane * R, tl), e = min(b + R, tl);
    const uint32_t x4k = a.pow_tile[1];
    for (uint32_t t = b; t < e; ++t) c = rd_multmodp(x4k, c) ^ cont[t];
    c = rd_multmodp(a.pow_tile[tl - e], c);  // a lane without a tile holds 0
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c ^= __shfl_xor(c, m, 64);
  }
  if (lane == 0) {
    const uint32_t v = rd_multmodp(a.tab->xpow[kMarshalPowBias + int32_t(P1 - (tl << 12))], c) ^ a.tail[r];
    const uint32_t* h = a.hdr + size_t(r) * kMarshalHdrWords;
    const int32_t size = int32_t(P1 - rc.H);
    int32_t status = tfscrc::kSuccess;
    if (h[0] != rc.id_lo || h[1] != rc.id_hi) status = tfscrc::kExitFileInfoError;
    else if (int32_t(h[3]) != size) status = tfscrc::kExitSyncFileError;
    else if (h[8] != v) status = tfscrc::kExitCheckCrcError;
    a.out_crc[r] = v;
    a.out_status[r] = status;
  }
}

hipError_t launch_ec_marshal_fold(const MarshalFoldArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(ec_marshal_fold_kernel, dim3((a.n + 3u) / 4u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Reinstate (ReinstateTask::do_reinstate, task.cpp:1376-1641).
// ec_marshal_kernel's pass over the decode plan's rows, with the segment walk
// run from two places: over in[] while a source that is a data member sits
// there, and over acc[o][*] after the member loop for every output that is a
// data member -- packet r of the lane's unit of output o has the lane layout of
// in[r].  `slot` names the data member whose rows of first and cont a walk
// uses.  The fold is ec_marshal_fold_kernel.
template <int OG>
__global__ void __launch_bounds__(256, OG <= 2 ? 4 : 3)  // waves per SIMD the register budget is held to (no spill)
    ec_reinstate_kernel(ReinstateArgs a, const uint32_t* __restrict__ masks, const MarshalTables* __restrict__ tab,
                        const MarshalRec* __restrict__ recs, const uint32_t* __restrict__ first) {
  __shared__ uint32_t lt[2 * 1024];  // slice, step_packet
  u32x2 in[8];
  bool ok;
  uint32_t base;
  RecordWalk w;
  if (!tile_begin<true, true>(a.m, tab, lt, in, ok, base, w)) return;
  const uint32_t S = a.m.ec.S;
  u32x2 acc[OG][8] = {};
  for (uint32_t s = 0; s < S; ++s) {
    u32x2 nx[8];
    const bool more = s + 1 < S;
    load_pieces<true>(nx, a.m.ec.src[more ? s + 1 : s], base, ok && more);
    combine<OG>(acc, in, masks, S, s);
    // the source walk: source s is a data member (wave-uniform)
    const uint32_t slot = a.src_slot[s];
    if (slot != kReinstateNoSlot) record_walk<false>(in, w, slot, a.m.mend[slot], tab, recs, first);
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = nx[c];
  }
  // every output's stores go out, then the output walk runs over the registers they were issued from
  if (ok) {
#pragma unroll
    for (int o = 0; o < OG; ++o)
#pragma unroll
      for (int r = 0; r < 8; ++r) st64nt_at(a.m.ec.dst[o], base + 128u * r, acc[o][r]);
  }
#pragma unroll
  for (int o = 0; o < OG; ++o) {  // compile-time o: a runtime index into acc would go to scratch
    const uint32_t slot = a.out_slot[o];
    if (slot != kReinstateNoSlot) record_walk<false>(acc[o], w, slot, a.m.mend[slot], tab, recs, first);
  }
}

hipError_t launch_ec_reinstate(const ReinstateArgs& a, int og, hipStream_t stream) {
  static constexpr SessionKernel<ReinstateArgs> k[] = {ec_reinstate_kernel<1>, ec_reinstate_kernel<2>,
                                                       ec_reinstate_kernel<3>, ec_reinstate_kernel<4>};
  return launch_session(k, a, a.m, og, stream);
}

// ---------------------------------------------------------------------------
// Frame-emitting chunk calls (include/tfs_ec_frames.h): the
// marshalling / reinstate pass with another end of the tile.  One kernel serves
// both sessions -- a marshalling launch names every source's slot and no
// output's.  acc[o][r] goes to the data area of the tile's frame: frame_len is a
// multiple of 4096, so a tile lies in one frame, j = t / tpf of the call, and the
// destination is the wave-uniform out[o] + j * stride + 56 + (tile in frame) *
// 4096 plus the lane's offset in the tile -- 8-byte aligned, as out, stride and 56
// are.  After the stores crc(0, the tile's bytes of output o) is taken from the
// same registers by record_walk's no-mask arithmetic: eight pieces, the 128-byte
// step, one multiplication by xpow[dl - pad], the wave's XOR; lane 0 writes it to
// tile_crc[output][T].  pad brings the chunk's short last tile (1 - 3 units, whose
// other lanes hold zeros) to the frame's end, not the tile's.  One writer per
// word, no atomics.  WALK == false: a session without records, or a later output
// group that rebuilds no data member -- no plan array is read.
template <int OG, bool WALK>
__global__ void __launch_bounds__(256, OG <= 2 ? 4 : 3)  // ec_reinstate_kernel's budget (no spill)
    ec_frames_kernel(FramesArgs a, const uint32_t* __restrict__ masks, const MarshalTables* __restrict__ tab,
                     const MarshalRec* __restrict__ recs, const uint32_t* __restrict__ first) {
  __shared__ uint32_t lt[2 * 1024];  // slice, step_packet
  u32x2 in[8];
  bool ok;
  uint32_t base;
  RecordWalk w;
  if (!tile_begin<true, true>(a.r.m, tab, lt, in, ok, base, w)) return;
  const uint32_t S = a.r.m.ec.S;
  u32x2 acc[OG][8] = {};
  for (uint32_t s = 0; s < S; ++s) {
    u32x2 nx[8];
    const bool more = s + 1 < S;
    load_pieces<true>(nx, a.r.m.ec.src[more ? s + 1 : s], base, ok && more);
    combine<OG>(acc, in, masks, S, s);
    if (WALK) {  // the source walk: source s is a data member (wave-uniform)
      const uint32_t slot = a.r.src_slot[s];
      if (slot != kReinstateNoSlot) record_walk<false>(in, w, slot, a.r.m.mend[slot], tab, recs, first);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = nx[c];
  }
  const uint32_t t = w.T - a.r.m.tile0;  // the tile in the call
  const uint32_t j = t / a.tpf;          // its frame in the call
  const uint64_t fo = uint64_t(j) * a.stride + kFramesHead + uint64_t(t - j * a.tpf) * 4096u;
  const uint32_t lo = base - (t << 12);  // the lane's piece of packet 0 in the tile
  if (ok) {
#pragma unroll
    for (int o = 0; o < OG; ++o)
#pragma unroll
      for (int r = 0; r < 8; ++r) st64nt_at(a.r.m.ec.dst[o] + fo, lo + 128u * r, acc[o][r]);
  }
  const uint32_t left = a.len - (t << 12);  // the chunk's bytes from this tile on
  const int32_t pad = left >= 4096u ? 0 : int32_t(4096u - left);
#pragma unroll
  for (int o = 0; o < OG; ++o) {
    uint32_t crc = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint32_t piece = rd_slice4(w.sl, rd_slice4(w.sl, acc[o][c].x) ^ acc[o][c].y);
      crc = c == 0 ? piece : rd_lut4(w.stp, crc) ^ piece;
    }
    crc = rd_multmodp(tab->xpow[kMarshalPowBias + w.dl - pad], crc);  // a lane past the chunk holds 0
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
    if (w.lane == 0) a.tile_crc[size_t(a.o0 + uint32_t(o)) * w.ntiles + w.T] = crc;
  }
  if (WALK) {
#pragma unroll
    for (int o = 0; o < OG; ++o) {  // compile-time o: a runtime index into acc would go to scratch
      const uint32_t slot = a.r.out_slot[o];
      if (slot != kReinstateNoSlot) record_walk<false>(acc[o], w, slot, a.r.m.mend[slot], tab, recs, first);
    }
  }
}

hipError_t launch_ec_frames(const FramesArgs& a, int og, bool walk, hipStream_t stream) {
  static constexpr SessionKernel<FramesArgs> k[2][kMaxOutGroup] = {
      {ec_frames_kernel<1, false>, ec_frames_kernel<2, false>, ec_frames_kernel<3, false>, ec_frames_kernel<4, false>},
      {ec_frames_kernel<1, true>, ec_frames_kernel<2, true>, ec_frames_kernel<3, true>, ec_frames_kernel<4, true>}};
  return launch_session(k[walk], a, a.r.m, og, stream);
}

// x^k mod P by squaring (k: a count of tiles).
__device__ __forceinline__ uint32_t fr_powk(uint32_t x, uint32_t k) {
  uint32_t r = 1u << 31;  // x^0
  for (; k; k >>= 1) {
    if (k & 1u) r = rd_multmodp(r, x);
    x = rd_multmodp(x, x);
  }
  return r;
}

// The seal: a wave per (output, frame) of the call, after the tile pass.  The frame's tile words but the last
// are chained as ec_marshal_fold_kernel chains cont (lane l a run of them, c' = shift(c, 4096) ^ word, one
// multiplication to the end of the last whole tile, the wave's XOR); the last tile's word, 1024 .. 4096 bytes
// on, completes crc(0, D).  Func::crc has no inversions, so
//   crc(FLAG_V1, H || D || F) = shift(crc(FLAG_V1, H), |D| + 4) ^ shift(crc(0, D), 4) ^ crc(0, F):
// H's eight words and F go through the slice tables, the head's multiplier comes with the launch.  Lanes 0 ..
// 13 store the V1 header and H, lane 14 stores F: plain dword stores, nothing else of out is touched.
__global__ void __launch_bounds__(256) ec_frames_seal_kernel(FramesSealArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t id = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (id >= a.n_out * a.nf) return;
  const uint32_t o = id / a.nf, j = id - o * a.nf;
  const uint32_t k = a.frame0 + j;
  const uint32_t offset = k * a.frame_len;  // < total < 2^31
  const uint32_t length = min(a.frame_len, a.total - offset);
  const uint32_t nc = (length - 1u) >> 12;          // whole tiles before the last one
  const uint32_t lastb = length - (nc << 12);       // the last tile's bytes, 1024 .. 4096
  const uint32_t* wd = a.tile_crc + size_t(o) * a.ntiles + (offset >> 12);
  const uint32_t* sl = &a.tab->slice[0][0];
  uint32_t c = 0;
  if (nc) {
    const uint32_t R = (nc + 63u) / 64u;
    const uint32_t b = min(lane * R, nc), e = min(b + R, nc);
    const uint32_t x4k = a.tab->xpow[kMarshalPowBias + 4096];
    for (uint32_t t = b; t < e; ++t) c = rd_multmodp(x4k, c) ^ wd[t];
    c = rd_multmodp(fr_powk(x4k, nc - e), c);  // a lane without a tile holds 0
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c ^= __shfl_xor(c, m, 64);
  }
  c = rd_multmodp(a.tab->xpow[kMarshalPowBias + int32_t(lastb)], c) ^ wd[nc];  // crc(0, D)
  const uint32_t flag = k == 0u ? a.flag0[o] : 0u;
  const uint32_t bid = a.block_id[o];
  uint32_t hc = tfscrc::kPacketFlagV1;
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) hc = rd_slice4(sl, hc ^ (i == 0u ? bid : i == 3u ? offset : i == 4u ? length : 0u));
  const uint32_t pw = k * a.frame_len + length == a.total ? a.pow_head_last : a.pow_head_full;
  uint32_t fcrc = rd_multmodp(pw, hc) ^ rd_slice4(sl, c) ^ rd_slice4(sl, flag);
  if (int16_t(uint16_t(a.type_ver >> 16)) < 1) fcrc = 0u;  // a version-0 header: no CRC
  const uint64_t pid = a.pid[o] + k;
  uint8_t* const frame = a.out[o] + uint64_t(j) * a.stride;
  if (lane < 14u) {
    const uint32_t v = lane == 0u    ? tfscrc::kPacketFlagV1
                       : lane == 1u  ? 36u + length
                       : lane == 2u  ? a.type_ver
                       : lane == 3u  ? uint32_t(pid)
                       : lane == 4u  ? uint32_t(pid >> 32)
                       : lane == 5u  ? fcrc
                       : lane == 6u  ? bid
                       : lane == 9u  ? offset
                       : lane == 10u ? length
                                     : 0u;
    *reinterpret_cast<uint32_t*>(frame + 4u * lane) = v;
  } else if (lane == 14u) {
    *reinterpret_cast<uint32_t*>(frame + kFramesHead + length) = flag;
  }
}

hipError_t launch_ec_frames_seal(const FramesSealArgs& a, hipStream_t stream) {
  const uint32_t n = a.n_out * a.nf;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ec_frames_seal_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Task chunk calls (include/tfs_ec_fetch.h): ec_frames_kernel's
// pass with another beginning of the tile.  Source s's chunk is the
// RespReadRawDataMessage frames it arrived in: the tile's pieces are loaded from the
// wave-uniform in[s] + j * in_stride + 28 + (tile in frame) * 4096 plus the lane's
// offset -- 8-byte aligned, as in[s] + 28 and in_stride are.  The frame carries
// n = clamp(block_len - frame offset, 0, requested) data bytes, and both grids
// start on a tile, so the tile has nrem = block_len[s] - tile_lo of them (wave-
// uniform): a piece at or past nrem is not loaded and stays zero, the piece that
// straddles it is masked by bytes.  That is the reference's memset of the short
// member; the trailer and the gap behind it never reach a register that is used.
// While the pieces sit in in[] the wave takes crc(0, the tile's nrem data bytes)
// from them as record_walk takes a segment that ends inside the tile -- the chain
// over the eight pieces, one multiplication by xpow[dl - pad] with pad = 4096 -
// nrem, the wave's XOR -- and lane 0 writes it to src_crc[s][T]: one writer per
// word, 0 for a tile wholly past n.  The record walk, the combine, the output
// stores and the output words are ec_frames_kernel's.

// The lane's eight pieces of a source's tile: p is the tile's first data byte in the frame, lo the lane's piece of
// packet 0 in the tile, nrem the data bytes from the tile's start on (<= 0: none, nothing is loaded).
__device__ __forceinline__ void load_frame_pieces(u32x2 (&v)[8], const uint8_t* p, uint32_t lo, int32_t nrem) {
  if (nrem >= 4096) {  // wave-uniform: a whole tile of data
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = ld64nt_at(p, lo + 128u * c);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int32_t k = nrem - int32_t(lo + 128u * c);  // the piece's data bytes
      v[c] = k > 0 ? ld64nt_at(p, lo + 128u * c) : u32x2{0u, 0u};
      if (k < 8) {
        const uint64_t mk = rd_low_bytes(k);
        v[c].x &= uint32_t(mk);
        v[c].y &= uint32_t(mk >> 32);
      }
    }
  }
}

// crc(0, the tile's bytes) from the lane's eight pieces, every lane's register brought to `pad` bytes before the
// tile's end; bytes behind that point are zero in the pieces.  The whole wave calls it.
__device__ __forceinline__ uint32_t tile_word(const u32x2 (&pc)[8], const RecordWalk& w,
                                              const MarshalTables* __restrict__ tab, int32_t pad) {
  uint32_t crc = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint32_t piece = rd_slice4(w.sl, rd_slice4(w.sl, pc[c].x) ^ pc[c].y);
    crc = c == 0 ? piece : rd_lut4(w.stp, crc) ^ piece;
  }
  crc = rd_multmodp(tab->xpow[kMarshalPowBias + w.dl - pad], crc);  // a lane without a byte holds 0
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
  return crc;
}

template <int OG, bool WALK>
__global__ void __launch_bounds__(256, OG <= 2 ? 4 : 3)  // ec_reinstate_kernel's budget (no spill)
    ec_task_kernel(TaskArgs a, const uint32_t* __restrict__ masks, const MarshalTables* __restrict__ tab,
                   const MarshalRec* __restrict__ recs, const uint32_t* __restrict__ first) {
  __shared__ uint32_t lt[2 * 1024];  // slice, step_packet
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t lo = 1024u * u + 8u * uint32_t(lane & 15);  // the lane's piece of packet 0 in the tile
  const uint64_t ntl = (a.f.r.m.ec.units + 3) / 4;           // tiles of this chunk
  const uint64_t t64 = uint64_t(blockIdx.x) * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool live = t64 < ntl;
  const uint32_t t = uint32_t(t64);      // the tile in the call (a chunk is shorter than 2^31 bytes)
  const uint32_t j = t / a.f.tpf;        // its frame in the call
  const uint32_t ti = t - j * a.f.tpf;   // the tile in the frame
  const bool ok = live && t64 * 4 + u < a.f.r.m.ec.units;
  const uint32_t T = a.f.r.m.tile0 + t;
  const uint32_t tile_lo = T << 12;      // < total < 2^31
  const uint64_t fi = uint64_t(j) * a.in_stride + kTaskHead + uint64_t(ti) * 4096u;
  u32x2 in[8];
  // the first source's loads go out before the tables are staged: a wave lives for one tile only
  int32_t nrem = live ? int32_t(a.blen[0]) - int32_t(tile_lo) : 0;
  load_frame_pieces(in, a.f.r.m.ec.src[0] + fi, lo, nrem);
  {
    const uint32_t* g = reinterpret_cast<const uint32_t*>(tab);
    for (uint32_t i = threadIdx.x; i < 2u * 1024u; i += 256u) lt[i] = g[i];
    __syncthreads();
  }
  if (!live) return;  // one grid step per wave
  RecordWalk w;
  w.sl = lt;
  w.stp = lt + 1024;
  w.T = T;
  w.tile_lo = tile_lo;
  w.tile_hi = tile_lo + 4096u;
  w.q0 = tile_lo + lo;
  w.ntiles = a.f.r.m.ntiles;
  w.dl = 3192 - int32_t(lo);
  w.lane = lane;
  w.cont = a.f.r.m.cont;
  w.tail = a.f.r.m.tail;
  w.hdr8 = reinterpret_cast<uint8_t*>(a.f.r.m.hdr);
  const uint32_t S = a.f.r.m.ec.S;
  u32x2 acc[OG][8] = {};
  for (uint32_t s = 0; s < S; ++s) {
    u32x2 nx[8];
    const bool more = s + 1 < S;
    const int32_t nnext = more ? int32_t(a.blen[s + 1]) - int32_t(tile_lo) : 0;
    load_frame_pieces(nx, a.f.r.m.ec.src[more ? s + 1 : s] + fi, lo, nnext);
    combine<OG>(acc, in, masks, S, s);
    if (a.src_crc) {  // the first output group's launch: the source's tile word
      const int32_t pad = (nrem >= 4096 || nrem <= 0) ? 0 : 4096 - nrem;
      const uint32_t crc = tile_word(in, w, tab, pad);
      if (lane == 0) a.src_crc[size_t(s) * w.ntiles + T] = crc;
    }
    if (WALK) {  // the source walk: source s is a data member (wave-uniform)
      const uint32_t slot = a.f.r.src_slot[s];
      if (slot != kReinstateNoSlot) record_walk<false>(in, w, slot, a.f.r.m.mend[slot], tab, recs, first);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = nx[c];
    nrem = nnext;
  }
  const uint64_t fo = uint64_t(j) * a.f.stride + kFramesHead + uint64_t(ti) * 4096u;
  if (ok) {
#pragma unroll
    for (int o = 0; o < OG; ++o)
#pragma unroll
      for (int r = 0; r < 8; ++r) st64nt_at(a.f.r.m.ec.dst[o] + fo, lo + 128u * r, acc[o][r]);
  }
  const uint32_t left = a.f.len - (t << 12);  // the chunk's bytes from this tile on
  const int32_t opad = left >= 4096u ? 0 : int32_t(4096u - left);
#pragma unroll
  for (int o = 0; o < OG; ++o) {
    const uint32_t crc = tile_word(acc[o], w, tab, opad);  // a lane past the chunk holds 0
    if (lane == 0) a.f.tile_crc[size_t(a.f.o0 + uint32_t(o)) * w.ntiles + T] = crc;
  }
  if (WALK) {
#pragma unroll
    for (int o = 0; o < OG; ++o) {  // compile-time o: a runtime index into acc would go to scratch
      const uint32_t slot = a.f.r.out_slot[o];
      if (slot != kReinstateNoSlot) record_walk<false>(acc[o], w, slot, a.f.r.m.mend[slot], tab, recs, first);
    }
  }
}

hipError_t launch_ec_task(const TaskArgs& a, int og, bool walk, hipStream_t stream) {
  static constexpr SessionKernel<TaskArgs> k[2][kMaxOutGroup] = {
      {ec_task_kernel<1, false>, ec_task_kernel<2, false>, ec_task_kernel<3, false>, ec_task_kernel<4, false>},
      {ec_task_kernel<1, true>, ec_task_kernel<2, true>, ec_task_kernel<3, true>, ec_task_kernel<4, true>}};
  return launch_session(k[walk], a, a.f.r.m, og, stream);
}

// The source check: a wave per (source, frame) of the call, after the tile passes.  The frame's tile words are
// chained as the seal chains them (the last tile is 1 .. 4096 bytes long here); then
//   crc(FLAG_V1, le32 n || D || le32 dfs) = shift(crc(FLAG_V1, le32 n), n + 4) ^ shift(crc(0, D), 4) ^ crc(0, le32 dfs)
// with n the expected length, which is what the tile pass fed the code.  Lane 0 reads the 28 bytes before the
// data and the 4 behind it, compares in the header's order and writes the result.  A frame whose expected n is
// 0 is not read.
__global__ void __launch_bounds__(256) ec_fetch_check_kernel(TaskCheckArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t id = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (id >= a.S * a.nf) return;
  const uint32_t s = id / a.nf, j = id - s * a.nf;
  const uint32_t offset = (a.frame0 + j) * a.frame_len;  // < total < 2^31
  const uint32_t req = min(a.frame_len, a.total - offset);
  // signed, as the tile pass counts: an unsigned "bl > offset ? bl - offset : 0" becomes a saturating subtraction,
  // which this wave-uniform code gets as a plain scalar one -- a member that ends before the frame would then be read
  const int32_t have = int32_t(a.blen[s]) - int32_t(offset);  // both below 2^31
  const uint32_t n = have > 0 ? min(uint32_t(have), req) : 0u;
  if (n == 0u) {
    if (lane == 0u) a.results[id] = tfs_ec_fetch_result{tfscrc::kSuccess, 0u, 0, 0u};
    return;
  }
  const uint32_t nc = (n - 1u) >> 12;         // whole tiles before the last one
  const uint32_t lastb = n - (nc << 12);      // the last tile's data bytes, 1 .. 4096
  const uint32_t* wd = a.src_crc + size_t(s) * a.ntiles + (offset >> 12);
  const uint32_t* sl = &a.tab->slice[0][0];
  uint32_t c = 0;
  if (nc) {
    const uint32_t R = (nc + 63u) / 64u;
    const uint32_t b = min(lane * R, nc), e = min(b + R, nc);
    const uint32_t x4k = a.tab->xpow[kMarshalPowBias + 4096];
    for (uint32_t t = b; t < e; ++t) c = rd_multmodp(x4k, c) ^ wd[t];
    c = rd_multmodp(fr_powk(x4k, nc - e), c);  // a lane without a tile holds 0
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c ^= __shfl_xor(c, m, 64);
  }
  if (lane != 0u) return;
  c = rd_multmodp(a.tab->xpow[kMarshalPowBias + int32_t(lastb)], c) ^ wd[nc];  // crc(0, D)
  const uint8_t* const frame = a.in[s] + uint64_t(j) * a.in_stride;
  const uint32_t* const h = reinterpret_cast<const uint32_t*>(frame);  // 4 modulo 8
  const uint32_t flag = h[0], blen = h[1], tv = h[2], hcrc = h[5], dn = h[6];
  const uint8_t* const tp = frame + kTaskHead + n;  // the trailer, at any byte address
  const uint32_t dfs = uint32_t(tp[0]) | uint32_t(tp[1]) << 8 | uint32_t(tp[2]) << 16 | uint32_t(tp[3]) << 24;
  const uint32_t head = rd_slice4(sl, tfscrc::kPacketFlagV1 ^ n);  // crc(FLAG_V1, le32 n)
  const uint32_t x8 = a.tab->xpow[kMarshalPowBias + 1];
  const uint32_t crc = rd_multmodp(fr_powk(x8, n + 4u), head) ^ rd_slice4(sl, c) ^ rd_slice4(sl, dfs);
  int32_t status = tfscrc::kSuccess;
  if (flag != tfscrc::kPacketFlagV1 || blen != 8u + n || (tv & 0xffffu) != kTaskPcode || dn != n) status = kTaskError;
  else if (int16_t(uint16_t(tv >> 16)) >= 1 && hcrc != crc) status = tfscrc::kExitCheckCrcError;
  a.results[id] = tfs_ec_fetch_result{status, dn, int32_t(dfs), crc};
}

hipError_t launch_ec_fetch_check(const TaskCheckArgs& a, hipStream_t stream) {
  const uint32_t n = a.S * a.nf;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ec_fetch_check_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// The seal of a task call: ec_frames_seal_kernel's wave per (output, frame), after the source check on the same
// stream.  The wave first reads the sources' statuses of frame j; if any failed it stores four zero bytes on the
// frame's flag word and nothing else -- no header, no H, no F -- so that no streamer takes the frame.
__global__ void __launch_bounds__(256) ec_task_seal_kernel(TaskSealArgs ta) {
  const FramesSealArgs& a = ta.f;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t id = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (id >= a.n_out * a.nf) return;
  const uint32_t o = id / a.nf, j = id - o * a.nf;
  uint8_t* const frame = a.out[o] + uint64_t(j) * a.stride;
  bool failed = false;
  for (uint32_t s = 0; s < ta.S; ++s) failed = failed || ta.results[size_t(s) * a.nf + j].status != tfscrc::kSuccess;
  if (failed) {  // wave-uniform
    if (lane == 0u) *reinterpret_cast<uint32_t*>(frame) = 0u;
    return;
  }
  const uint32_t k = a.frame0 + j;
  const uint32_t offset = k * a.frame_len;  // < total < 2^31
  const uint32_t length = min(a.frame_len, a.total - offset);
  const uint32_t nc = (length - 1u) >> 12;          // whole tiles before the last one
  const uint32_t lastb = length - (nc << 12);       // the last tile's bytes, 1024 .. 4096
  const uint32_t* wd = a.tile_crc + size_t(o) * a.ntiles + (offset >> 12);
  const uint32_t* sl = &a.tab->slice[0][0];
  uint32_t c = 0;
  if (nc) {
    const uint32_t R = (nc + 63u) / 64u;
    const uint32_t b = min(lane * R, nc), e = min(b + R, nc);
    const uint32_t x4k = a.tab->xpow[kMarshalPowBias + 4096];
    for (uint32_t t = b; t < e; ++t) c = rd_multmodp(x4k, c) ^ wd[t];
    c = rd_multmodp(fr_powk(x4k, nc - e), c);  // a lane without a tile holds 0
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c ^= __shfl_xor(c, m, 64);
  }
  c = rd_multmodp(a.tab->xpow[kMarshalPowBias + int32_t(lastb)], c) ^ wd[nc];  // crc(0, D)
  const uint32_t flag = k == 0u ? a.flag0[o] : 0u;
  const uint32_t bid = a.block_id[o];
  uint32_t hc = tfscrc::kPacketFlagV1;
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) hc = rd_slice4(sl, hc ^ (i == 0u ? bid : i == 3u ? offset : i == 4u ? length : 0u));
  const uint32_t pw = k * a.frame_len + length == a.total ? a.pow_head_last : a.pow_head_full;
  uint32_t fcrc = rd_multmodp(pw, hc) ^ rd_slice4(sl, c) ^ rd_slice4(sl, flag);
  if (int16_t(uint16_t(a.type_ver >> 16)) < 1) fcrc = 0u;  // a version-0 header: no CRC
  const uint64_t pid = a.pid[o] + k;
  if (lane < 14u) {
    const uint32_t v = lane == 0u    ? tfscrc::kPacketFlagV1
                       : lane == 1u  ? 36u + length
                       : lane == 2u  ? a.type_ver
                       : lane == 3u  ? uint32_t(pid)
                       : lane == 4u  ? uint32_t(pid >> 32)
                       : lane == 5u  ? fcrc
                       : lane == 6u  ? bid
                       : lane == 9u  ? offset
                       : lane == 10u ? length
                                     : 0u;
    *reinterpret_cast<uint32_t*>(frame + 4u * lane) = v;
  } else if (lane == 14u) {
    *reinterpret_cast<uint32_t*>(frame + kFramesHead + length) = flag;
  }
}

hipError_t launch_ec_task_seal(const TaskSealArgs& a, hipStream_t stream) {
  const uint32_t n = a.f.n_out * a.f.nf;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ec_task_seal_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Scrub (beyond the reference, which never re-reads a family).
// ec_marshal_kernel's pass with another end of the tile: the stored parity is
// loaded into the registers the sources went through, one member at a time, and
// compared with acc[o][*] where the marshalling pass stores it.  Parity 0's
// loads go out under the last source's code; parity o + 1's under the compare of
// parity o.  Per lane the eight XORs are ORed; a ballot of the wave turns "any
// lane of unit lane >> 4 nonzero" into four bits, and lane 0 stores them to
// pbad[(o0 + o) * ntiles + T]: one writer per word across all launches of a
// session, no atomics, no read-back.  A lane whose unit lies past the chunk
// loads nothing, so its acc and its parity registers are zero alike.  WALK: the
// CRC side (record_walk over in[], slot = the source's number) runs; the later
// output groups of a family with more than four parity members, and a session
// without records, only compare and stage no tables.
template <int OG, bool WALK>
__global__ void __launch_bounds__(256, OG <= 3 ? 4 : 3)  // ec_marshal_kernel's budget
    ec_scrub_kernel(ScrubArgs a, const uint32_t* __restrict__ masks, const MarshalTables* __restrict__ tab,
                    const MarshalRec* __restrict__ recs, const uint32_t* __restrict__ first) {
  __shared__ uint32_t lt[WALK ? 2 * 1024 : 1];  // slice, step_packet
  const uint32_t S = a.m.ec.S;
  __builtin_assume(S != 0u);  // a coder has data members: no path on which in[] is not stored parity 0 below
  u32x2 in[8];
  bool ok;
  uint32_t base;
  RecordWalk w;
  if (!tile_begin<WALK, false>(a.m, tab, lt, in, ok, base, w)) return;
  const uint32_t T = w.T;
  u32x2 acc[OG][8] = {};
  for (uint32_t s = 0; s < S; ++s) {
    u32x2 nx[8];
    load_pieces<false>(nx, s + 1 < S ? a.m.ec.src[s + 1] : a.par[0], base, ok);  // after the last source: stored parity 0
    combine<OG>(acc, in, masks, S, s);
    if (WALK) record_walk<true>(in, w, s, a.m.mend[s], tab, recs, first);
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = nx[c];
  }
  // in[] holds stored parity 0 (packet r of the lane's unit in in[r], acc[o][r]'s layout)
#pragma unroll
  for (int o = 0; o < OG; ++o) {
    u32x2 nx[8];
    load_pieces<false>(nx, a.par[o + 1 < OG ? o + 1 : o], base, ok && o + 1 < OG);
    uint32_t d = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) d |= (acc[o][r].x ^ in[r].x) | (acc[o][r].y ^ in[r].y);
    const uint64_t b = __builtin_amdgcn_ballot_w64(d != 0u);  // the whole wave is here: t is wave-uniform
    const uint32_t bits = uint32_t((b & 0xFFFFull) != 0ull) | (uint32_t(((b >> 16) & 0xFFFFull) != 0ull) << 1) |
                          (uint32_t(((b >> 32) & 0xFFFFull) != 0ull) << 2) | (uint32_t((b >> 48) != 0ull) << 3);
    // the lane number is taken anew: kept from above it would be one more register live across the member loop
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u) a.pbad[size_t(a.o0 + uint32_t(o)) * a.m.ntiles + T] = bits;
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = nx[c];
  }
}

hipError_t launch_ec_scrub(const ScrubArgs& a, int og, bool walk, hipStream_t stream) {
  static constexpr SessionKernel<ScrubArgs> k[2][kMaxOutGroup] = {
      {ec_scrub_kernel<1, false>, ec_scrub_kernel<2, false>, ec_scrub_kernel<3, false>, ec_scrub_kernel<4, false>},
      {ec_scrub_kernel<1, true>, ec_scrub_kernel<2, true>, ec_scrub_kernel<3, true>, ec_scrub_kernel<4, true>}};
  return launch_session(k[walk], a, a.m, og, stream);
}

// pbad's words to the caller's form: a workgroup per parity member counts the set
// bits into units[p] and packs each word's four bits into one byte of the map.
__global__ void __launch_bounds__(1024) ec_scrub_count_kernel(ScrubCountArgs a) {
  __shared__ uint32_t part[16];
  const uint32_t p = blockIdx.x;
  const uint32_t* w = a.pbad + size_t(p) * a.ntiles;
  uint8_t* mp = a.map + size_t(p) * a.ntiles;
  uint32_t c = 0;
  for (uint32_t T0 = threadIdx.x; T0 < a.ntiles; T0 += 4096u) {
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = T0 + 1024u * k < a.ntiles ? w[T0 + 1024u * k] & 15u : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (T0 + 1024u * k < a.ntiles) {
        mp[T0 + 1024u * k] = uint8_t(v[k]);
        c += uint32_t(__popc(v[k]));
      }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += part[k];
    a.units[p] = v;
  }
}

hipError_t launch_ec_scrub_count(const ScrubCountArgs& a, int pn, hipStream_t stream) {
  if (pn <= 0 || a.ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(ec_scrub_count_kernel, dim3(unsigned(pn)), dim3(1024), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Scrub locate (beyond the reference).  ec_apply_kernel's
// mapping over a list: a wave takes four entries, lane l owns 8 bytes at
// 8 (l & 15) of each packet of entry l >> 4, and entry k is unit units[k] of
// every member (unit k without a list).  The syndromes S_p = stored parity p ^
// code of the data as given are made G (<= 4) parity members per read of the
// data; S_0 stays in registers, the others live for their group only, so the
// registers do not grow with pn.  "Non-zero anywhere in the unit" and "differs
// anywhere in the unit" are ballots over the entry's 16 lanes, as the scrub
// kernel's.  The candidate stage of parity o (is ratio[o][j] S_0 == S_o over the
// whole unit, for every data member j) runs only when some entry of the wave is
// flagged in parity 0 .. o, the repair of member j (e = inv0[j] S_0) only when an
// entry of the wave located j: a wave of clean or parity-only entries pays for
// neither.  A lane whose entry lies past n loads nothing and holds zero
// syndromes.  One lane of an entry writes its result, the 16 lanes of a DATA
// entry its repaired unit: one writer per word, no atomics, no member written.
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) {
  uint32_t t = v | (v >> 4);
  t |= t >> 2;
  t |= t >> 1;
  return uint32_t(__popc(t & 0x01010101u));
}

template <int G>
__global__ void __launch_bounds__(256)
    ec_locate_kernel(LocateArgs a, const uint32_t* __restrict__ masks, const uint32_t* __restrict__ ratio,
                     const uint32_t* __restrict__ inv0, const uint32_t* __restrict__ units) {
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t sh = 16u * u;  // the entry's lanes in a ballot
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint32_t dn = a.dn, pn = a.pn;
  const uint64_t t = uint64_t(blockIdx.x) * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t * 4u >= a.n) return;  // one grid step per wave; the whole wave leaves
  const uint64_t k = t * 4u + u;
  const bool ok = k < a.n;
  const uint32_t unit = ok ? (units ? units[k] : uint32_t(k)) : 0u;
  const uint32_t base = unit * 1024u + off;  // a member is shorter than 2^31 bytes
  u32x2 S0[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) S0[r] = u32x2{0u, 0u};
  uint32_t pb = 0;                    // bit p: S_p != 0 in this lane's entry
  uint32_t cand = (1u << dn) - 1u;    // bit j: data member j still fits every S_o seen
  for (uint32_t g0 = 0; g0 < pn; g0 += G) {
    u32x2 acc[G][8];
#pragma unroll
    for (int o = 0; o < G; ++o)
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[o][r] = u32x2{0u, 0u};
    u32x2 in[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = ok ? ld64nt_at(a.mem[0], base + 128u * c) : u32x2{0u, 0u};
    for (uint32_t s = 0; s < dn; ++s) {
      u32x2 nx[8];
      const uint8_t* np = a.mem[s + 1 < dn ? s + 1 : dn + g0];  // after the last data member: the group's first stored parity
#pragma unroll
      for (int c = 0; c < 8; ++c) nx[c] = ok ? ld64nt_at(np, base + 128u * c) : u32x2{0u, 0u};
#pragma unroll
      for (int o = 0; o < G; ++o) {
        const uint32_t p = g0 + o < pn ? g0 + o : pn - 1u;  // past the last parity member: its code again, not used
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t* m = masks + ((p * 8u + uint32_t(r)) * dn + s) * 8u;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint32_t mk = m[c];
            acc[o][r].x = xand(acc[o][r].x, in[c].x, mk);
            acc[o][r].y = xand(acc[o][r].y, in[c].y, mk);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) in[c] = nx[c];
    }
    // the code becomes the syndrome; in[] holds stored parity g0, loaded under the last data member's code
#pragma unroll
    for (int o = 0; o < G; ++o) {
      const uint32_t p = g0 + o < pn ? g0 + o : pn - 1u;
      const uint8_t* pp = a.mem[dn + p];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const u32x2 v = o == 0 ? in[r] : (ok ? ld64nt_at(pp, base + 128u * r) : u32x2{0u, 0u});
        acc[o][r].x ^= v.x;
        acc[o][r].y ^= v.y;
      }
    }
#pragma unroll
    for (int o = 0; o < G; ++o) {  // compile-time o: a runtime index into acc would go to scratch
      const uint32_t p = g0 + o;
      if (p >= pn) break;  // wave-uniform
      uint32_t d = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) d |= acc[o][r].x | acc[o][r].y;
      const uint64_t b = __builtin_amdgcn_ballot_w64(d != 0u);  // the whole wave is here
      pb |= uint32_t(((b >> sh) & 0xFFFFull) != 0ull) << p;
      if (o == 0 && g0 == 0u) {
#pragma unroll
        for (int r = 0; r < 8; ++r) S0[r] = acc[0][r];
        continue;
      }
      const uint32_t sofar = (2u << p) - 1u;
      if (__builtin_amdgcn_ballot_w64((pb & sofar) == sofar) == 0ull) continue;  // no entry flagged in 0 .. p
      for (uint32_t j = 0; j < dn; ++j) {
        const uint32_t* m = ratio + (size_t(p - 1u) * dn + j) * 64u;
        uint32_t x = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          u32x2 v = acc[o][r];
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const uint32_t mk = m[r * 8 + c];
            v.x = xand(v.x, S0[c].x, mk);
            v.y = xand(v.y, S0[c].y, mk);
          }
          x |= v.x | v.y;  // (ratio S_0 ^ S_o)'s packet r
        }
        const uint64_t mb = __builtin_amdgcn_ballot_w64(x != 0u);
        cand &= ~(uint32_t(((mb >> sh) & 0xFFFFull) != 0ull) << j);
      }
    }
  }
  const uint32_t all = (1u << pn) - 1u;
  uint32_t kind = kLocateClean, member = 0xFFu, diff = 0;
  if (pb == all) {
    if (__popc(cand) == 1) {
      kind = kLocateData;
      member = uint32_t(__ffs(int(cand)) - 1);
    } else {
      kind = kLocateNone;
    }
  } else if (pb != 0u) {
    kind = kLocateParity;
  }
  if (__builtin_amdgcn_ballot_w64(kind == uint32_t(kLocateData)) != 0ull) {
    for (uint32_t j = 0; j < dn; ++j) {
      const bool mine = member == j;
      if (__builtin_amdgcn_ballot_w64(mine) == 0ull) continue;  // no entry of the wave located j
      const uint32_t* m = inv0 + size_t(j) * 64u;
      u32x2 e[8];
      uint32_t cnt = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        e[r] = u32x2{0u, 0u};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint32_t mk = m[r * 8 + c];
          e[r].x = xand(e[r].x, S0[c].x, mk);
          e[r].y = xand(e[r].y, S0[c].y, mk);
        }
        cnt += nonzero_bytes(e[r].x) + nonzero_bytes(e[r].y);
      }
#pragma unroll
      for (int w = 8; w >= 1; w >>= 1) cnt += __shfl_xor(cnt, w, 64);  // over the entry's 16 lanes
      if (mine) {
        diff = cnt;
        if (a.fixed) {
          uint8_t* const out = a.fixed + k * 1024u + off;
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const u32x2 v = ld64nt_at(a.mem[j], base + 128u * r);
            st64nt(out + 128u * r, u32x2{v.x ^ e[r].x, v.y ^ e[r].y});
          }
        }
      }
    }
  }
  if (ok && (lane & 15) == 0) {
    const uint32_t lo = kind | (member << 8) | (pb << 16);
    const uint32_t hi = diff | ((pn >= 3u ? kLocateConfirmed : 0u) << 16);
    *reinterpret_cast<u32x2*>(a.result + k) = u32x2{lo, hi};
  }
}

hipError_t launch_ec_locate(const LocateArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const uint64_t ntl = (uint64_t(a.n) + 3) / 4;
  const dim3 g(static_cast<unsigned>((ntl + 3) / 4)), b(256);
  switch (a.pn < uint32_t(kMaxOutGroup) ? a.pn : uint32_t(kMaxOutGroup)) {
    case 2: hipLaunchKernelGGL(ec_locate_kernel<2>, g, b, 0, stream, a, a.masks, a.ratio, a.inv0, a.units); break;
    case 3: hipLaunchKernelGGL(ec_locate_kernel<3>, g, b, 0, stream, a, a.masks, a.ratio, a.inv0, a.units); break;
    default: hipLaunchKernelGGL(ec_locate_kernel<4>, g, b, 0, stream, a, a.masks, a.ratio, a.inv0, a.units); break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Parity update (beyond the reference, whose unlink_file_parity leaves the parity
// bytes as they were).  ec_locate_kernel's mapping over a list:
// a wave takes four entries, lane l owns 8 bytes at 8 (l & 15) of each packet of
// entry l >> 4.  Entry k is slot k of the delta buffers and unit list[k] of the
// parity members.  The delta d = a ^ b (a alone without b) of the one changed
// data member stays in registers while the wave goes through the bound parity
// members one after the other: load the unit, acc[r] ^= d[c] & mask[p][r][member][c],
// store it back -- block (p, member) of the encode plan, scalar loads.  A short
// list comes in the launch arguments: the wave's four units are one uniform read
// of `inl` and a select by l >> 4, so nothing is indexed per lane.  Every listed
// unit belongs to one wave of one launch (the host refuses a unit named twice),
// and updates of one unit by several launches are ordered by the stream.  A lane
// whose entry lies past n loads and stores nothing; a parity member that is not
// bound is skipped by the whole wave.

__global__ void __launch_bounds__(256)
    ec_update_kernel(UpdateArgs a, const uint32_t* __restrict__ masks, const uint32_t* __restrict__ units) {
  const int lane = threadIdx.x & 63;
  const uint32_t u = uint32_t(lane) >> 4;
  const uint32_t off = 8u * uint32_t(lane & 15);
  const uint32_t t = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (uint64_t(t) * 4u >= a.n) return;  // one grid step per wave; the whole wave leaves
  const uint32_t k = t * 4u + u;        // n * 1024 <= size < 2^31
  const bool ok = k < a.n;
  uint32_t unit = k;
  if (a.n_inline) {  // t < kUpdateInline / 4: the four words lie inside inl
    const uint32_t x0 = a.inl[t * 4u], x1 = a.inl[t * 4u + 1u], x2 = a.inl[t * 4u + 2u], x3 = a.inl[t * 4u + 3u];
    unit = u == 0u ? x0 : u == 1u ? x1 : u == 2u ? x2 : x3;
  } else if (units) {
    unit = ok ? units[k] : 0u;
  }
  const uint32_t base = unit * 1024u + off;  // a member is shorter than 2^31 bytes
  const uint32_t slot = k * 1024u + off;
  u32x2 d[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) d[c] = ok ? ld64nt_at(a.a, slot + 128u * c) : u32x2{0u, 0u};
  if (a.b) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const u32x2 v = ok ? ld64nt_at(a.b, slot + 128u * c) : u32x2{0u, 0u};
      d[c].x ^= v.x;
      d[c].y ^= v.y;
    }
  }
  for (uint32_t p = 0; p < a.pn; ++p) {
    uint8_t* const pp = a.par[p];
    if (!pp) continue;  // wave-uniform: the member is not bound
    u32x2 acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = ok ? ld64nt_at(pp, base + 128u * r) : u32x2{0u, 0u};
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t* m = masks + update_mask_offset(p, uint32_t(r), a.dn, a.member);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t mk = m[c];
        acc[r].x = xand(acc[r].x, d[c].x, mk);
        acc[r].y = xand(acc[r].y, d[c].y, mk);
      }
    }
    if (ok) {
#pragma unroll
      for (int r = 0; r < 8; ++r) st64nt_at(pp, base + 128u * r, acc[r]);
    }
  }
}

hipError_t launch_ec_update(const UpdateArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  if (a.n_inline && (a.n_inline != a.n || a.n > kUpdateInline)) return hipErrorInvalidValue;  // the kernel reads inl[0, 16)
  const uint64_t ntl = (uint64_t(a.n) + 3) / 4;
  hipLaunchKernelGGL(ec_update_kernel, dim3(static_cast<unsigned>((ntl + 3) / 4)), dim3(256), 0, stream, a, a.masks, a.units);
  return hipGetLastError();
}

}  // namespace tfsec
