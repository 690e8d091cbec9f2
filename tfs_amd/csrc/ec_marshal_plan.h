// ec_marshal_plan.h -- the plan of a marshalling session (include/tfs_ec.h,
// tfs_ec_marshal_begin): which records of the data members take part in the
// pass, and, for every 4 KiB tile of every data member, the first record the
// tile's wave has to look at, so that the kernel does no search.  Host-side only.
#pragma once
#include <cstdint>
#include <vector>

#include "tfs_ec_device.h"

namespace tfsec {

struct MarshalMeta {  // same bytes as tfs_raw_meta
  uint64_t file_id;
  int32_t offset, size;
};
static_assert(sizeof(MarshalMeta) == 16, "raw meta layout");

struct MarshalPlan {
  uint32_t ntiles = 0;             // tiles of 4 KiB in [0, total), the last one may be short
  std::vector<MarshalRec> recs;    // accepted records, member after member, ascending by H
  std::vector<uint32_t> member;    // [rec]: its data member
  std::vector<uint32_t> index;     // [rec]: its position in the caller's order (member 0's metas, then member 1's ...)
  std::vector<uint32_t> mbegin;    // [dn + 1]: member s's records are recs[mbegin[s] .. mbegin[s + 1])
  std::vector<uint32_t> first;     // [dn][ntiles]
  std::vector<int32_t> early;      // per caller record: the status given at begin (0: the record takes part)
};

constexpr int kMarshalParameterError = -1016, kMarshalReadFileSizeError = -8034;
constexpr int kMarshalSizeInvalid = -16002, kMarshalDataInvalid = -16001;

// Call-level checks 3-5 of tfs_ec_marshal_begin and the per-record checks.
// Returns the call's status; the plan is complete only on 0.
inline int make_marshal_plan(const MarshalMeta* const* metas, const uint32_t* n_metas, const int* sizes, int dn,
                             int total, MarshalPlan* p) {
  *p = MarshalPlan();
  if (total <= 0 || total % 1024 != 0) return kMarshalSizeInvalid;
  if (!sizes) return kMarshalDataInvalid;
  for (int s = 0; s < dn; ++s)
    if (sizes[s] < 0 || sizes[s] > total) return kMarshalDataInvalid;
  p->ntiles = uint32_t((int64_t(total) + 4095) >> 12);
  p->mbegin.assign(size_t(dn) + 1, 0);
  p->first.assign(size_t(dn) * p->ntiles, 0);
  for (int s = 0; s < dn; ++s) {
    const uint32_t n = (metas && n_metas) ? n_metas[s] : 0u;
    if (n && !metas[s]) return kMarshalParameterError;
    p->mbegin[s] = uint32_t(p->recs.size());
    int64_t last_end = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const MarshalMeta& m = metas[s][i];
      const uint32_t pos = uint32_t(p->early.size());
      if (m.offset < 0 || int64_t(m.offset) + int64_t(m.size) > int64_t(sizes[s])) {
        p->early.push_back(kMarshalParameterError);
        continue;
      }
      if (m.size <= 36) {
        p->early.push_back(kMarshalReadFileSizeError);
        continue;
      }
      if (int64_t(m.offset) < last_end) return kMarshalParameterError;  // unsorted or overlapping
      last_end = int64_t(m.offset) + int64_t(m.size);
      p->early.push_back(0);
      p->recs.push_back(MarshalRec{uint32_t(m.offset), uint32_t(last_end), uint32_t(m.file_id),
                                   uint32_t(m.file_id >> 32)});
      p->member.push_back(uint32_t(s));
      p->index.push_back(pos);
    }
    // first[s][t]: the records' ends ascend, so one walk over the tiles serves
    const uint32_t rend = uint32_t(p->recs.size());
    uint32_t r = p->mbegin[s];
    for (uint32_t t = 0; t < p->ntiles; ++t) {
      const uint64_t lo = uint64_t(t) << 12;
      while (r < rend && uint64_t(p->recs[r].P1) <= lo) ++r;
      p->first[size_t(s) * p->ntiles + t] = r;
    }
  }
  p->mbegin[dn] = uint32_t(p->recs.size());
  return 0;
}

}  // namespace tfsec
