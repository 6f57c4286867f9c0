// The host path of sift_join_matches (sift-gpu_amd/csrc/join_rule.hpp) as a
// stand-alone program: built with the address and undefined-behaviour
// sanitizers and run on the CPU (tests/test_join.py::test_join_rule_program).
//
//   1. a hand-written case: duplicate keys in A at different and at equal
//      distances, a best row that is masked out, keys of -1, n_keys, INT_MIN and
//      INT_MAX, distances of -0.0, +inf, NaN and -1, duplicate keys in B, both key
//      sides; the joined rows are listed literally;
//   2. 2000 random rows per table against a quadratic search written here;
//   3. the degenerate inputs: no rows, no keys, every output NULL, NULL masks; each
//      output is allocated at exactly the size the rule may write.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sift-gpu_amd/csrc/join_rule.hpp"

static void fail(const char* what) {
  fprintf(stderr, "FAIL: %s\n", what);
  exit(1);
}

static sift_match rec(int query, int train, float distance) { return sift_match{query, train, distance, -123}; }

// The rule by exhaustive search: for B row i the A row it joins, or -1.
static int search(const std::vector<sift_match>& a, int a_side, const unsigned char* am, const sift_match& r, int b_side,
                  int n_keys) {
  const int key = b_side ? r.train : r.query;
  if (key < 0 || key >= n_keys) return -1;
  int best = -1;
  for (int i = 0; i < (int)a.size(); ++i) {
    if ((am && !am[i]) || (a_side ? a[i].train : a[i].query) != key || !(a[i].distance >= 0)) continue;
    if (best < 0 || a[i].distance < a[best].distance) best = i;  // equal distances: the earlier row stays
  }
  return best;
}

int main() {
  // ---- 1. the hand-written case: A's key is its train, B's its query; 8 keys ----
  const float inf = INFINITY;
  const std::vector<sift_match> a = {
      rec(0, 1, 2.5f),  rec(1, 1, 0.5f),  rec(2, 1, 1.5f),        // key 1: row 1
      rec(3, 2, 0.75f), rec(4, 2, 0.75f),                         // key 2: equal, row 3
      rec(5, 3, 0.25f), rec(6, 3, 1.0f),  rec(7, 3, 1.25f),       // key 3: row 5 masked out -> row 6
      rec(8, -1, 0.f),  rec(9, 8, 0.f),   rec(10, INT32_MIN, 0.f), rec(11, INT32_MAX, 0.f),  // no key
      rec(12, 4, 0.5f), rec(13, 4, -0.0f),                        // key 4: -0.0 counts as 0 -> row 13
      rec(14, 5, inf),                                            // key 5: +inf is a candidate
      rec(15, 6, NAN),  rec(16, 6, -1.f),                         // key 6: none
      rec(17, 7, 0.f),  rec(18, 7, -0.0f)};                       // key 7: equal ranks -> row 17
  std::vector<unsigned char> am(a.size(), 1);
  am[5] = 0;
  std::vector<double> xyz(3 * a.size());
  for (size_t i = 0; i < xyz.size(); ++i) xyz[i] = 100.0 + (double)i;
  const uint64_t payload = 0x7ff8000000abcdefull;  // a NaN whose bytes must survive
  memcpy(&xyz[3 * 13 + 1], &payload, 8);
  const std::vector<sift_match> b = {rec(1, 50, 9.f), rec(1, 51, NAN), rec(6, 52, 0.f), rec(2, 53, 0.f), rec(-1, 54, 0.f),
                                     rec(8, 55, 0.f), rec(3, 56, 0.f), rec(4, 57, 0.f), rec(5, 58, 0.f), rec(7, 59, 0.f),
                                     rec(0, 60, 0.f), rec(3, 61, 0.f)};
  std::vector<unsigned char> bm(b.size(), 1);
  bm[11] = 0;
  std::vector<float> bxy(2 * b.size());
  for (size_t i = 0; i < bxy.size(); ++i) bxy[i] = 0.5f * (float)i;
  const int want_a[] = {1, 1, 3, 6, 13, 14, 17}, want_b[] = {0, 1, 3, 6, 7, 8, 9};
  const int nb = (int)b.size();
  {
    std::vector<double> xo(3 * nb);
    std::vector<float> po(2 * nb);
    std::vector<int> ar(nb), br(nb);
    std::vector<unsigned char> bj(nb, 7);
    const int n = sift::join_matches(a.data(), (int)a.size(), SIFT_JOIN_TRAIN, am.data(), xyz.data(), b.data(), nb,
                                     SIFT_JOIN_QUERY, bm.data(), bxy.data(), 8, xo.data(), po.data(), ar.data(),
                                     br.data(), bj.data());
    if (n != 7) fail("the hand-written case joins 7 rows");
    for (int j = 0; j < n; ++j) {
      if (ar[j] != want_a[j] || br[j] != want_b[j]) fail("the hand-written case: a joined row");
      if (memcmp(&xo[3 * j], &xyz[3 * want_a[j]], 24) || memcmp(&po[2 * j], &bxy[2 * want_b[j]], 8))
        fail("the hand-written case: the gathered bytes");
    }
    for (int i = 0, j = 0; i < nb; ++i) {
      const bool in = j < n && want_b[j] == i;
      if (bj[i] != (in ? 1 : 0)) fail("the hand-written case: b_joined");
      j += in;
    }
    // the sides exchanged on tables with the indices exchanged: the same rows
    std::vector<sift_match> as = a, bs = b;
    for (auto& r : as) std::swap(r.query, r.train);
    for (auto& r : bs) std::swap(r.query, r.train);
    std::vector<int> ar2(nb), br2(nb);
    if (sift::join_matches(as.data(), (int)as.size(), SIFT_JOIN_QUERY, am.data(), nullptr, bs.data(), nb, SIFT_JOIN_TRAIN,
                           bm.data(), nullptr, 8, nullptr, nullptr, ar2.data(), br2.data(), nullptr) != 7 ||
        memcmp(ar2.data(), ar.data(), 28) || memcmp(br2.data(), br.data(), 28))
      fail("the sides exchanged");
    // no masks: row 5 wins key 3 and B row 11 joins
    if (sift::join_matches(a.data(), (int)a.size(), SIFT_JOIN_TRAIN, nullptr, nullptr, b.data(), nb, SIFT_JOIN_QUERY,
                           nullptr, nullptr, 8, nullptr, nullptr, ar.data(), br.data(), nullptr) != 8 ||
        ar[3] != 5 || ar[7] != 5 || br[7] != 11)
      fail("NULL masks");
  }

  // ---- 2. random tables against the exhaustive search ----
  unsigned lcg = 99u;
  auto next = [&](unsigned m) {
    lcg = lcg * 1664525u + 1013904223u;
    return (int)((lcg >> 8) % m);
  };
  for (int round = 0; round < 4; ++round) {
    const int na = 2000, nq = 2000, n_keys = 700, a_side = round & 1, b_side = round >> 1;
    std::vector<sift_match> ra(na), rb(nq);
    std::vector<unsigned char> ma(na), mb(nq);
    for (int i = 0; i < na; ++i) ra[i] = rec(next(n_keys + 4) - 2, next(n_keys + 4) - 2, 0.25f * (float)next(9) - 0.25f);
    for (int i = 0; i < nq; ++i) rb[i] = rec(next(n_keys + 4) - 2, next(n_keys + 4) - 2, 1.f);
    for (auto& m : ma) m = next(5) != 0;
    for (auto& m : mb) m = next(7) != 0;
    std::vector<int> ar(nq), br(nq);
    std::vector<unsigned char> bj(nq);
    const int n = sift::join_matches(ra.data(), na, a_side, ma.data(), nullptr, rb.data(), nq, b_side, mb.data(), nullptr,
                                     n_keys, nullptr, nullptr, ar.data(), br.data(), bj.data());
    int j = 0;
    for (int i = 0; i < nq; ++i) {
      const int w = mb[i] ? search(ra, a_side, ma.data(), rb[i], b_side, n_keys) : -1;
      if (bj[i] != (w >= 0)) fail("random tables: b_joined");
      if (w < 0) continue;
      if (j >= n || ar[j] != w || br[j] != i) fail("random tables: a joined row");
      ++j;
    }
    if (j != n || n < 500) fail("random tables: the count");
  }

  // ---- 3. the degenerate inputs ----
  unsigned char one = 9;
  if (sift::join_matches(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 5, nullptr, nullptr, nullptr,
                         nullptr, nullptr) != 0)
    fail("no rows");
  if (sift::join_matches(a.data(), (int)a.size(), 1, nullptr, nullptr, b.data(), 1, 0, nullptr, nullptr, 0, nullptr,
                         nullptr, nullptr, nullptr, &one) != 0 ||
      one != 0)
    fail("no keys");
  if (sift::join_matches(nullptr, 0, 1, nullptr, nullptr, b.data(), nb, 0, nullptr, nullptr, 8, nullptr, nullptr,
                         nullptr, nullptr, nullptr) != 0)
    fail("no A rows");
  if (sift::join_matches(a.data(), (int)a.size(), 1, am.data(), nullptr, b.data(), nb, 0, bm.data(), nullptr, 8, nullptr,
                         nullptr, nullptr, nullptr, nullptr) != 7)
    fail("every output NULL");
  printf("join rule ok\n");
  return 0;
}
