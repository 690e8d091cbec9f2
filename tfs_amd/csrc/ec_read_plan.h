// ec_read_plan.h -- host form of the degraded read (include/tfs_ec.h): which
// bytes of the members travel.  Only the covering ranges of the jobs go up and
// only the covering units come down, so the plan restates the jobs against a
// compact image: the union of the covering ranges, packed in address order, is
// what every source member contributes (`spans`), and every job that passes the
// early checks gets its own run of a compact output buffer.  Host-side only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "tfs_ec_device.h"

namespace tfsec {

struct ReadSpan {   // [start, end) of every source member -> [cbase, cbase + end - start) of its staging buffer
  uint32_t start, end;
  uint64_t cbase;
};
struct ReadCopy {   // compact output [src, src + len) -> the caller's out + dst
  uint64_t src, dst, len;
};
struct ReadPlan {
  std::vector<ReadSpan> spans;
  std::vector<ReadJob> jobs;        // the jobs that read, restated against the compact images
  std::vector<uint32_t> index;      // their positions in the caller's list
  std::vector<int32_t> early;       // per caller job: the early status (0: the job is in `jobs`)
  std::vector<ReadCopy> copies;     // adjacent output runs joined
  uint64_t up = 0;                  // bytes of one source member that go up (multiple of 1024)
  uint64_t down = 0;                // bytes of the compact output
};

inline void make_read_plan(const ReadJob* jobs, uint32_t n, int32_t member_size, uint64_t out_cap, ReadPlan* p) {
  *p = ReadPlan();
  p->early.assign(n, 0);
  std::vector<ReadSpan> cover;
  std::vector<uint32_t> a0(n, 0), e0(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    p->early[i] = read_job_check(jobs[i], member_size, out_cap, &a0[i], &e0[i]);
    if (p->early[i] == 0 && e0[i] > a0[i]) cover.push_back(ReadSpan{a0[i], e0[i], 0});
  }
  std::sort(cover.begin(), cover.end(), [](const ReadSpan& x, const ReadSpan& y) { return x.start < y.start; });
  for (const ReadSpan& c : cover) {
    if (!p->spans.empty() && c.start <= p->spans.back().end) {
      if (c.end > p->spans.back().end) p->spans.back().end = c.end;
    } else {
      p->spans.push_back(c);
    }
  }
  for (ReadSpan& s : p->spans) {
    s.cbase = p->up;
    p->up += uint64_t(s.end - s.start);
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (p->early[i] != 0) continue;
    ReadJob j = jobs[i];
    const uint64_t len = uint64_t(e0[i] - a0[i]);
    if (len) {
      // the span that holds [a0, e0): the last one starting at or before a0
      auto it = std::upper_bound(p->spans.begin(), p->spans.end(), a0[i],
                                 [](uint32_t v, const ReadSpan& s) { return v < s.start; });
      const ReadSpan& s = *(it - 1);
      j.offset = int32_t(s.cbase + uint64_t(a0[i] - s.start) + (uint32_t(jobs[i].offset) & 1023u));
      if (!p->copies.empty() && p->copies.back().src + p->copies.back().len == p->down &&
          p->copies.back().dst + p->copies.back().len == jobs[i].out_offset)
        p->copies.back().len += len;
      else
        p->copies.push_back(ReadCopy{p->down, jobs[i].out_offset, len});
    } else {
      j.offset = 0;  // an empty range at an aligned offset: nothing to read
    }
    j.out_offset = p->down;
    p->down += len;
    p->jobs.push_back(j);
    p->index.push_back(i);
  }
}

}  // namespace tfsec
