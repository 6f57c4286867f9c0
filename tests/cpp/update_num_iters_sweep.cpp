// update_num_iters of homography_math.hpp, compiled for the host, over the
// sweep of tests/homography_edge_inputs.py (n = 5..512, good = 4..n): writes
// the results as raw int32 to stdout.  argv: confidence max_iters.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "homography_math.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const double confidence = strtod(argv[1], nullptr);
  const int max_iters = atoi(argv[2]);
  std::vector<int32_t> out;
  for (int n = 5; n <= 512; ++n)
    for (int good = 4; good <= n; ++good)
      out.push_back(sift::hmath::update_num_iters(confidence, (double)(n - good) / n, 4, max_iters));
  return fwrite(out.data(), sizeof(int32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
