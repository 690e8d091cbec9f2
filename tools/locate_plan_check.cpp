// locate_plan_check.cpp -- stand-alone check of the scrub locate plan
// (tfs_amd/csrc/ec_locate_plan.h), meant to be built with the host sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan \
//       tools/locate_plan_check.cpp -o /tmp/locate_plan_check && /tmp/locate_plan_check
//
// For every allowed (dn, pn), against the coder's own encode bitmatrix and a per-symbol
// GF(2^8) restatement: each ratio matrix applied to the bit matrix of m[0][j] is the bit
// matrix of m[o][j]; inv0[j] times the bit matrix of m[0][j] is the identity; every
// matrix acts on all 256 symbols as the multiplication by its element; the ratios of one
// o are pairwise distinct; and a single-member error is solved back from its syndromes.
#include <cstdio>
#include <cstdlib>

#include "../tfs_amd/csrc/ec_locate_plan.h"

using namespace tfsec;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

typedef uint8_t Bits[8][8];

static void from_words(const uint32_t* w, Bits& b) {
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) {
      CHECK(w[r * 8 + c] == 0u || w[r * 8 + c] == 0xFFFFFFFFu);
      b[r][c] = w[r * 8 + c] ? 1 : 0;
    }
}
static void product(const Bits& a, const Bits& b, Bits& out) {
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) {
      int v = 0;
      for (int t = 0; t < 8; ++t) v ^= a[r][t] & b[t][c];
      out[r][c] = uint8_t(v);
    }
}
static int apply(const Bits& a, int s) {  // the matrix over the bits of one symbol
  int out = 0;
  for (int r = 0; r < 8; ++r) {
    int v = 0;
    for (int c = 0; c < 8; ++c) v ^= a[r][c] & ((s >> c) & 1);
    out |= v << r;
  }
  return out;
}
static bool same(const Bits& a, const Bits& b) {
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c)
      if (a[r][c] != b[r][c]) return false;
  return true;
}

int main() {
  const Gf256 gf;
  LocatePlan bad;
  CHECK(make_locate_plan(3, 1, &bad) == -1);
  CHECK(make_locate_plan(0, 2, &bad) == -1);
  CHECK(make_locate_plan(11, 2, &bad) == -1);
  int coders = 0;
  for (int pn = 2; pn < kMaxMembers; ++pn)
    for (int dn = 1; dn + pn <= kMaxMembers; ++dn) {
      LocatePlan p;
      CHECK(make_locate_plan(dn, pn, &p) == 0);
      CHECK(p.ratio.size() == size_t(pn - 1) * dn * 64 && p.inv0.size() == size_t(dn) * 64);
      const BitMat enc = encode_bitmatrix(dn, pn);
      const int cols = dn * kW;
      auto coeff = [&](int o, int j, Bits& b) {  // the coder's own bits of m[o][j]
        for (int r = 0; r < 8; ++r)
          for (int c = 0; c < 8; ++c) b[r][c] = enc[size_t(o * kW + r) * cols + j * kW + c];
      };
      for (int j = 0; j < dn; ++j) {
        Bits m0, inv, prod, id = {};
        for (int r = 0; r < 8; ++r) id[r][r] = 1;
        coeff(0, j, m0);
        from_words(&p.inv0[size_t(j) * 64], inv);
        product(inv, m0, prod);
        CHECK(same(prod, id));
        const int e0 = gf.div(1, pn + j);
        CHECK(gf.mul(p.inv0_e[size_t(j)], e0) == 1);
        for (int s = 0; s < 256; ++s) CHECK(apply(inv, s) == gf.mul(p.inv0_e[size_t(j)], s));
        for (int o = 1; o < pn; ++o) {
          Bits q, mo;
          from_words(&p.ratio[(size_t(o - 1) * dn + j) * 64], q);
          coeff(o, j, mo);
          product(q, m0, prod);
          CHECK(same(prod, mo));
          const int qe = p.ratio_e[size_t(o - 1) * dn + j];
          CHECK(gf.mul(qe, e0) == gf.div(1, o ^ (pn + j)));
          for (int s = 0; s < 256; ++s) CHECK(apply(q, s) == gf.mul(qe, s));
          for (int i = 0; i < j; ++i) CHECK(p.ratio_e[size_t(o - 1) * dn + i] != qe);
          // one wrong symbol e in member j: only j satisfies ratio * S_0 == S_o, and inv0 * S_0 gives e back
          for (int e = 1; e < 256; e += 37) {
            const int s0 = gf.mul(e0, e), so = gf.mul(gf.div(1, o ^ (pn + j)), e);
            for (int i = 0; i < dn; ++i) CHECK((gf.mul(p.ratio_e[size_t(o - 1) * dn + i], s0) == so) == (i == j));
            CHECK(apply(inv, s0) == e);
          }
        }
      }
      ++coders;
    }
  printf("locate plan ok: %d coders\n", coders);
  return 0;
}
