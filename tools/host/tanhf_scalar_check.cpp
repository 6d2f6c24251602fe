// tools/host/tanhf_scalar_check.cpp: csrc/tanhf_scalar.hpp (the text the DDP kernel runs on the device) compiled for the host,
// against the installed libm's tanhf.
//   tanhf_scalar_check [stride]   stride 1 (default): all 2^32 bit patterns; stride s: every s-th
// Prints the number of inputs whose results differ in any bit (NaN results compare equal to NaN); exit code 1 if any.
// g++ -O2 -ffp-contract=off -fopenmp tools/host/tanhf_scalar_check.cpp -o tanhf_scalar_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../autorally_amd/csrc/tanhf_scalar.hpp"

int main(int argc, char **argv)
{
  const long long stride = argc > 1 ? atoll(argv[1]) : 1;
  unsigned long long bad = 0, n = 0;
  const long long count = ((1LL << 32) + stride - 1) / stride;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
  for (long long i = 0; i < count; i++) {
    const uint32_t b = (uint32_t)(i * stride);
    float x;
    memcpy(&x, &b, 4);
    const float r = tanhf(x), s = mppi::tanhf_scalar(x);
    n++;
    if (memcmp(&r, &s, 4) != 0 && !(r != r && s != s)) {
      bad++;
      if (bad < 5) {
        uint32_t br, bs;
        memcpy(&br, &r, 4); memcpy(&bs, &s, 4);
        fprintf(stderr, "x=%08x (%g): libm %08x scalar %08x\n", b, x, br, bs);
      }
    }
  }
  printf("tanhf_scalar vs libm tanhf: %llu inputs, %llu differ\n", n, bad);
  return bad != 0;
}
