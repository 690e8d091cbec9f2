// read_plan_check.cpp -- stand-alone check of the host form's range plan
// (tfs_amd/csrc/ec_read_plan.h), meant to be built with the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/read_plan_check.cpp -o /tmp/read_plan_check && /tmp/read_plan_check
//
// Random job lists (records, ranges, rejected jobs, jobs sharing units, empty
// ranges) against a byte-marking model: every byte a job's covering range needs
// is inside a span, spans are disjoint, sorted and packed, every restated job
// points at the same bytes, and the output copies tile the compact output.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../tfs_amd/csrc/ec_read_plan.h"

using namespace tfsec;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  std::mt19937_64 rng(5);
  for (int round = 0; round < 2000; ++round) {
    const int32_t member = int32_t(1024 * (1 + rng() % 64));
    const uint32_t n = uint32_t(rng() % 40);
    std::vector<ReadJob> jobs(n);
    uint64_t o = 0;
    for (ReadJob& j : jobs) {
      j = ReadJob{};
      j.file_id = rng();
      j.offset = int32_t(rng() % uint64_t(member + 2048)) - 512;
      j.size = int32_t(rng() % 5000) - (rng() % 16 == 0 ? 100 : 0);
      if (rng() % 3 == 0) j.flags = kReadRange;
      if (rng() % 8 == 0) j.size = 0;
      if (rng() % 8 == 0) j.offset &= ~1023;
      j.out_offset = o + (rng() % 16 == 0 ? 8 : 0);
      o += 1024 * (rng() % 8);
    }
    const uint64_t out_cap = o ? o - (rng() % 4 == 0 ? 1024 : 0) : 0;
    ReadPlan p;
    make_read_plan(jobs.data(), n, member, out_cap, &p);
    uint64_t at = 0;
    for (size_t k = 0; k < p.spans.size(); ++k) {
      CHECK(p.spans[k].start < p.spans[k].end && p.spans[k].end <= uint32_t(member));
      CHECK(p.spans[k].start % 1024 == 0 && p.spans[k].end % 1024 == 0 && p.spans[k].cbase == at);
      if (k) CHECK(p.spans[k - 1].end < p.spans[k].start);
      at += p.spans[k].end - p.spans[k].start;
    }
    CHECK(at == p.up && p.up <= uint64_t(member));
    CHECK(p.early.size() == n && p.jobs.size() == p.index.size());
    size_t k = 0;
    uint64_t down = 0, copied = 0;
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t A = 0, E = 0;
      const int32_t st = read_job_check(jobs[i], member, out_cap, &A, &E);
      CHECK(st == p.early[i]);
      if (st) continue;
      CHECK(k < p.jobs.size() && p.index[k] == i);
      const ReadJob& r = p.jobs[k++];
      CHECK(r.size == jobs[i].size && r.flags == jobs[i].flags && r.file_id == jobs[i].file_id);
      CHECK(r.out_offset == down);
      uint32_t A2 = 0, E2 = 0;
      CHECK(read_job_check(r, int32_t(p.up ? p.up : 1024), p.down, &A2, &E2) == 0 && E2 - A2 == E - A);
      if (E > A) {
        CHECK((r.offset & 1023) == (jobs[i].offset & 1023));
        bool found = false;
        for (const ReadSpan& s : p.spans)
          if (s.start <= A && E <= s.end) {
            found = true;
            CHECK(s.cbase + (A - s.start) == A2);
          }
        CHECK(found);
      }
      down += E - A;
    }
    CHECK(k == p.jobs.size() && down == p.down);
    for (const ReadCopy& c : p.copies) {
      CHECK(c.src == copied && c.len > 0 && c.dst + c.len <= out_cap);
      copied += c.len;
    }
    CHECK(copied == p.down);
  }
  printf("read plan ok\n");
  return 0;
}
