// scrub_classify_check.cpp -- stand-alone check of classify_scrub
// (tfs_amd/ds/scrub_classify.h), meant to be built with the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan \
//       tools/scrub_classify_check.cpp -o /tmp/scrub_classify_check && /tmp/scrub_classify_check
//
// Random families, indexes, statuses and tile maps: every counter and verdict against a
// brute-force restatement that walks the members byte by byte.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../tfs_amd/ds/scrub_classify.h"

using namespace tfs::dataserver;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  std::mt19937_64 rng(14);
  const int32_t kinds[] = {TFS_SUCCESS,           TFS_SUCCESS,           TFS_EXIT_CHECK_CRC_ERROR, TFS_EXIT_FILE_INFO_ERROR,
                           TFS_EXIT_SYNC_FILE_ERROR, TFS_EXIT_PARAMETER_ERROR, TFS_EXIT_READ_FILE_SIZE_ERROR};
  uint64_t seen_parity_only = 0, seen_data = 0, seen_unattributed = 0, seen_short_tile = 0;
  for (int round = 0; round < 4000; ++round) {
    const int pn = 1 + int(rng() % 4), dn = 1 + int(rng() % (12 - pn));
    const int32_t total = 1024 * int32_t(1 + rng() % 23);
    const int64_t units = total / 1024;
    const size_t ntiles = size_t((total + 4095) / 4096);
    seen_short_tile += total % 4096 != 0;
    std::vector<std::vector<tfs_raw_meta>> indexes(static_cast<size_t>(dn));
    std::vector<int32_t> status;
    // per byte of every data member: covered by a record that failed
    std::vector<std::vector<uint8_t>> failed_byte(static_cast<size_t>(dn), std::vector<uint8_t>(size_t(total), 0));
    std::vector<uint32_t> failed_records(static_cast<size_t>(dn), 0);
    uint32_t bad = 0;
    for (int i = 0; i < dn; ++i) {
      int64_t pos = int64_t(rng() % 300);
      const int n = int(rng() % 8);
      for (int k = 0; k < n; ++k) {
        tfs_raw_meta m{rng(), 0, 0};
        int32_t st = kinds[rng() % 7];
        if (st == TFS_EXIT_PARAMETER_ERROR) {  // rejected at begin: anywhere, even outside the member
          m.offset = rng() % 2 ? -int32_t(1 + rng() % 5000) : int32_t(total - int32_t(rng() % 50));
          m.size = int32_t(51 + rng() % 5000);
        } else if (st == TFS_EXIT_READ_FILE_SIZE_ERROR) {
          m.offset = int32_t(rng() % uint64_t(total));
          m.size = int32_t(rng() % 37);
        } else {
          m.offset = int32_t(pos + (rng() % 2 ? int64_t(rng() % 2500) : 0));
          m.size = int32_t(37 + (rng() % 3 ? rng() % 200 : rng() % 6000));
          if (int64_t(m.offset) + m.size > total) break;
          pos = int64_t(m.offset) + m.size;
          if (st != TFS_SUCCESS) {
            ++failed_records[size_t(i)];
            for (int64_t b = m.offset; b < int64_t(m.offset) + m.size; ++b) failed_byte[size_t(i)][size_t(b)] = 1;
          }
        }
        bad += st != TFS_SUCCESS;
        indexes[size_t(i)].push_back(m);
        status.push_back(st);
      }
    }
    std::vector<uint8_t> tile_map(size_t(pn) * ntiles, 0);
    const int density = int(rng() % 4);  // 0: clean map
    for (int64_t u = 0; density && u < units; ++u) {
      const int what = int(rng() % (density == 1 ? 12 : 3));
      for (int p = 0; p < pn; ++p)
        if (what == 0 || (what == 1 && rng() % 2)) tile_map[size_t(p) * ntiles + size_t(u >> 2)] |= uint8_t(1u << (u & 3));
    }
    const ScrubReport r = classify_scrub(dn, pn, total, indexes, status, tile_map);
    // brute force, byte by byte
    std::vector<uint32_t> data_units(static_cast<size_t>(dn), 0), parity_only(static_cast<size_t>(pn), 0);
    uint32_t unattributed = 0, flagged_units = 0;
    for (int64_t u = 0; u < units; ++u) {
      std::vector<int> F;
      for (int p = 0; p < pn; ++p)
        if (tile_map[size_t(p) * ntiles + size_t(u / 4)] & (1u << (u % 4))) F.push_back(p);
      if (F.empty()) continue;
      ++flagged_units;
      if (int(F.size()) < pn) {
        for (int p : F) ++parity_only[size_t(p)];
        continue;
      }
      bool named = false;
      for (int i = 0; i < dn; ++i) {
        bool meets = false;
        for (int64_t b = u * 1024; b < u * 1024 + 1024; ++b) meets |= failed_byte[size_t(i)][size_t(b)] != 0;
        if (meets) {
          ++data_units[size_t(i)];
          named = true;
        }
      }
      if (!named) ++unattributed;
    }
    CHECK(r.status == status && r.bad_records == bad && r.flagged_units == flagged_units);
    CHECK(r.failed_records == failed_records && r.data_units == data_units && r.parity_only_units == parity_only);
    CHECK(r.unattributed_units == unattributed && r.findings() == int(bad + flagged_units));
    CHECK(r.suspect.size() == size_t(dn + pn));
    for (int i = 0; i < dn; ++i) CHECK(r.suspect[size_t(i)] == (failed_records[size_t(i)] || data_units[size_t(i)]));
    for (int p = 0; p < pn; ++p) CHECK(r.suspect[size_t(dn + p)] == (parity_only[size_t(p)] != 0));
    if (pn == 1) CHECK(parity_only[0] == 0);
    for (uint32_t v : parity_only) seen_parity_only += v;
    for (uint32_t v : data_units) seen_data += v;
    seen_unattributed += unattributed;
  }
  CHECK(seen_parity_only > 1000 && seen_data > 1000 && seen_unattributed > 1000 && seen_short_tile > 1000);
  printf("scrub classify ok (%llu parity-only, %llu data, %llu unattributed units)\n",
         static_cast<unsigned long long>(seen_parity_only), static_cast<unsigned long long>(seen_data),
         static_cast<unsigned long long>(seen_unattributed));
  return 0;
}
