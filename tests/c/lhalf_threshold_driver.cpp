// lhalf_threshold_driver.cpp -- the host side of csrc/spx_lhalf_threshold.hpp (__host__ __device__): reads sigma * lambda values
// as C99 hexadecimal doubles, one per line, and prints lhalf_threshold of each in the same spelling
// (tests/test_proxstep_lhalf_batch_abi.py compares them with glibc's pow).
#include "spx_lhalf_threshold.hpp"

#include <cstdio>
#include <cstdlib>

int main() {
  char line[128];
  while (std::fgets(line, sizeof line, stdin)) {
    const double nl = std::strtod(line, nullptr);
    std::printf("%a\n", lhalf_threshold(nl));
  }
  return 0;
}
