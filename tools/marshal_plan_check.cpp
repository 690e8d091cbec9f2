// marshal_plan_check.cpp -- stand-alone check of a marshalling session's plan
// (tfs_amd/csrc/ec_marshal_plan.h), meant to be built with the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include tools/marshal_plan_check.cpp -o /tmp/marshal_plan_check && /tmp/marshal_plan_check
//
// Random record lists with random sizes and total: first[s][t] against a brute-force
// search over every tile, the statuses of the records rejected one by one, and the
// refusal of lists that are unsorted or overlap once those are set aside.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../tfs_amd/csrc/ec_marshal_plan.h"

using namespace tfsec;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  std::mt19937_64 rng(12);
  int refused = 0, accepted = 0;
  for (int round = 0; round < 3000; ++round) {
    const int dn = 1 + int(rng() % 6);
    int total = 1024 * int(1 + rng() % 40);
    std::vector<int> sizes(dn);
    for (int& s : sizes) s = rng() % 5 == 0 ? total : int(rng() % uint64_t(total + 1));
    std::vector<std::vector<MarshalMeta>> metas(dn);
    bool broken = false;  // a member whose good records are unsorted or overlap
    for (int s = 0; s < dn; ++s) {
      int64_t pos = int64_t(rng() % 200);
      const int n = int(rng() % 30);
      for (int i = 0; i < n; ++i) {
        MarshalMeta m{rng(), 0, 0};
        const int kind = int(rng() % 12);
        if (kind == 0) {  // too short, anywhere inside the member (even on top of a neighbour)
          m.offset = int32_t(rng() % uint64_t(sizes[s] + 1));
          m.size = int32_t(rng() % 37);
          if (int64_t(m.offset) + m.size > sizes[s]) m.size = 0;
        } else if (kind == 1) {  // negative offset
          m.offset = -int32_t(1 + rng() % 500);
          m.size = int32_t(rng() % 500);
        } else if (kind == 2) {  // past the member's end
          m.size = int32_t(37 + rng() % 500);
          m.offset = int32_t(std::max<int64_t>(0, int64_t(sizes[s]) - m.size + 1 + int64_t(rng() % 3000)));
        } else {
          m.offset = int32_t(pos + (rng() % 3 == 0 ? int64_t(rng() % 300) : 0));
          m.size = int32_t(37 + (rng() % 4 == 0 ? rng() % 9000 : rng() % 200));
          if (int64_t(m.offset) + m.size > sizes[s]) break;
          pos = int64_t(m.offset) + m.size;
        }
        metas[s].push_back(m);
      }
    }
    if (rng() % 4 == 0) {  // break one member: swap two good records, or stretch one into the next
      const int s = int(rng() % dn);
      std::vector<size_t> good;
      for (size_t i = 0; i < metas[s].size(); ++i) {
        const MarshalMeta& m = metas[s][i];
        if (m.offset >= 0 && int64_t(m.offset) + m.size <= sizes[s] && m.size > 36) good.push_back(i);
      }
      if (good.size() >= 2) {
        const size_t k = size_t(rng() % (good.size() - 1));
        MarshalMeta& a = metas[s][good[k]];
        MarshalMeta& b = metas[s][good[k + 1]];
        if (rng() % 2) std::swap(a, b);           // the later record first
        else a.size = b.offset - a.offset + 1;    // one byte into the next good record
        broken = true;
      }
    }
    if (rng() % 50 == 0) total += 100;
    std::vector<const MarshalMeta*> mp(dn);
    std::vector<uint32_t> nm(dn);
    for (int s = 0; s < dn; ++s) {
      mp[s] = metas[s].data();
      nm[s] = uint32_t(metas[s].size());
    }
    MarshalPlan p;
    const int rc = make_marshal_plan(mp.data(), nm.data(), sizes.data(), dn, total, &p);
    if (total % 1024) {
      CHECK(rc == kMarshalSizeInvalid);
      continue;
    }
    bool too_long = false;
    for (int s : sizes) too_long |= s > total;
    CHECK(!too_long);
    if (broken) {
      CHECK(rc == kMarshalParameterError);
      ++refused;
      continue;
    }
    CHECK(rc == 0);
    ++accepted;
    CHECK(p.ntiles == uint32_t((total + 4095) / 4096));
    CHECK(p.first.size() == size_t(dn) * p.ntiles && p.mbegin.size() == size_t(dn) + 1);
    size_t j = 0, k = 0;
    for (int s = 0; s < dn; ++s) {
      CHECK(p.mbegin[s] == k);
      for (const MarshalMeta& m : metas[s]) {
        const int want = (m.offset < 0 || int64_t(m.offset) + m.size > sizes[s]) ? kMarshalParameterError
                         : m.size <= 36                                         ? kMarshalReadFileSizeError
                                                                                : 0;
        CHECK(j < p.early.size() && p.early[j] == want);
        if (want == 0) {
          CHECK(k < p.recs.size() && p.index[k] == j && p.member[k] == uint32_t(s));
          CHECK(p.recs[k].H == uint32_t(m.offset) && p.recs[k].P1 == uint32_t(m.offset + m.size));
          CHECK((uint64_t(p.recs[k].id_hi) << 32 | p.recs[k].id_lo) == m.file_id);
          if (k > p.mbegin[s]) CHECK(p.recs[k - 1].P1 <= p.recs[k].H);
          ++k;
        }
        ++j;
      }
      // brute force: the first record of the member whose payload end lies past the tile's start
      for (uint32_t t = 0; t < p.ntiles; ++t) {
        uint32_t want = uint32_t(k);
        for (uint32_t r = p.mbegin[s]; r < k; ++r)
          if (uint64_t(p.recs[r].P1) > uint64_t(t) * 4096) {
            want = r;
            break;
          }
        CHECK(p.first[size_t(s) * p.ntiles + t] == want);
      }
    }
    CHECK(j == p.early.size() && k == p.recs.size() && p.mbegin[dn] == k);
  }
  CHECK(refused > 100 && accepted > 1000);
  // call-level checks in the header's order
  MarshalPlan p;
  const int one = 2048, big = 4096, neg = -1;
  const MarshalMeta m{1, 0, 100};
  const MarshalMeta* mp = &m;
  const uint32_t n1 = 1;
  CHECK(make_marshal_plan(&mp, &n1, &one, 1, 0, &p) == kMarshalSizeInvalid);
  CHECK(make_marshal_plan(&mp, &n1, &big, 1, 2048 + 512, &p) == kMarshalSizeInvalid);
  CHECK(make_marshal_plan(&mp, &n1, &big, 1, 2048, &p) == kMarshalDataInvalid);
  CHECK(make_marshal_plan(&mp, &n1, &neg, 1, 2048, &p) == kMarshalDataInvalid);
  CHECK(make_marshal_plan(&mp, &n1, &one, 1, 2048, &p) == 0 && p.recs.size() == 1);
  CHECK(make_marshal_plan(nullptr, nullptr, &one, 1, 2048, &p) == 0 && p.recs.empty() && p.first.size() == 1);
  printf("marshal plan ok (%d lists accepted, %d refused)\n", accepted, refused);
  return 0;
}
