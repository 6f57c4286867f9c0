// layout_check.hpp -- the harness the *_layout.cpp programs share: run() carves
// a layout of sift-gpu_amd/csrc/scratch.hpp twice, without a GPU, and checks
// that each piece starts on a 256-byte boundary, that pieces are pairwise
// disjoint and lie inside the measured total, and that the measuring pass
// (null base) agrees with the pass on a real block.  The block is a heap
// allocation of exactly the measured size and every piece is written end to
// end, so an address sanitizer build also sees any piece that leaves it.
// CHECK and AT expect `what` (the case's name) in scope; AT also `a` (the
// carver) and `base`.
#pragma once

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#include "../../sift-gpu_amd/csrc/scratch.hpp"

using namespace sift;

static int failures = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      ++failures;                       \
      printf("FAIL %s: ", what);        \
      printf(__VA_ARGS__);              \
      printf(" [%s]\n", #cond);         \
    }                                   \
  } while (0)

// layout(a, base) carves and, on the real pass (base != null), checks the
// pointers it got against the carver's pieces.
static void run(const char* what, int n_expected, const std::function<void(Carver&, char*)>& layout) {
  Carver measure(nullptr);
  layout(measure, nullptr);
  const size_t total = measure.bytes();
  CHECK(n_expected <= Carver::kMaxPieces, "%d pieces are more than a carver records", n_expected);
  CHECK(measure.n_pieces == n_expected, "%d pieces, expected %d", measure.n_pieces, n_expected);
  CHECK(total % Carver::kAlign == 0, "total %zu", total);
  char* base = static_cast<char*>(aligned_alloc(Carver::kAlign, total ? total : Carver::kAlign));
  Carver real(base);
  layout(real, base);
  CHECK(real.bytes() == total && real.n_pieces == measure.n_pieces, "passes disagree: %zu vs %zu bytes", real.bytes(),
        total);
  for (int i = 0; i < real.n_pieces; ++i) {
    const Carver::Piece p = real.pieces[i], m = measure.pieces[i];
    CHECK(p.off == m.off && p.bytes == m.bytes, "piece %d differs between the passes", i);
    CHECK(p.off % Carver::kAlign == 0, "piece %d at %zu", i, p.off);
    CHECK(p.off + p.bytes <= total, "piece %d ends at %zu of %zu", i, p.off + p.bytes, total);
    for (int j = 0; j < i; ++j) {
      const Carver::Piece q = real.pieces[j];
      CHECK(p.off >= q.off + q.bytes || q.off >= p.off + p.bytes, "pieces %d and %d overlap", j, i);
    }
    if (p.off + p.bytes <= total) memset(base + p.off, 0xA5, p.bytes);
  }
  free(base);
}

// The pointer a layout returned is piece i of the carver (or null when measuring).
#define AT(ptr, i)                                                                                      \
  do {                                                                                                  \
    const int i_ = (i);                                                                                 \
    const char* p_ = reinterpret_cast<const char*>(ptr);                                                \
    CHECK(base ? p_ == base + a.pieces[i_].off : p_ == nullptr, "field %s is not piece %d", #ptr, i_);  \
  } while (0)
