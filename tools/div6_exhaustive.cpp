// Exhaustive host check of the division helper in
// csrc/include/stencil_amd/device_util.hpp: for every one of the 2^32 float
// bit patterns, div6_fast(x) against the correctly rounded x / 6.0f.
// Reports the mismatches inside the guard (div6_fast_ok; must be 0) and
// outside it (where the device helper takes the true division).
//
//   hipcc -x hip --offload-arch=gfx950 -O2 -ffp-contract=off -Icsrc/include tools/div6_exhaustive.cpp \
//         -o build/div6_exhaustive -pthread && build/div6_exhaustive
//
// About half a minute on 16 threads. Exit status 1 if any guarded input
// differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "stencil_amd/device_util.hpp"

namespace {

struct Counts {
  uint64_t guarded = 0, badGuarded = 0, unguarded = 0, badUnguarded = 0;
  uint32_t firstBad = 0;
};

uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

void scan(uint64_t lo, uint64_t hi, Counts &c) {
  for (uint64_t b = lo; b < hi; ++b) {
    const uint32_t u = (uint32_t)b;
    float x;
    std::memcpy(&x, &u, 4);
    if (std::isnan(x)) continue; // NaN in, NaN out on both sides
    volatile float six = 6.0f;   // a true division, never a reciprocal
    const float want = x / six;
    const float got = stencil_amd::div6_fast(x);
    const bool same = bits_of(got) == bits_of(want);
    if (stencil_amd::div6_fast_ok(x)) {
      ++c.guarded;
      if (!same) {
        if (!c.badGuarded) c.firstBad = u;
        ++c.badGuarded;
      }
    } else {
      ++c.unguarded;
      if (!same) ++c.badUnguarded;
    }
  }
}

} // namespace

int main() {
  const int nThreads = 16;
  std::vector<Counts> counts(nThreads);
  std::vector<std::thread> threads;
  const uint64_t total = 1ull << 32, per = total / nThreads;
  for (int t = 0; t < nThreads; ++t)
    threads.emplace_back(scan, t * per, t == nThreads - 1 ? total : (t + 1) * per,
                         std::ref(counts[t]));
  for (std::thread &t : threads) t.join();
  Counts sum;
  for (const Counts &c : counts) {
    sum.guarded += c.guarded;
    sum.unguarded += c.unguarded;
    sum.badUnguarded += c.badUnguarded;
    if (c.badGuarded && !sum.badGuarded) sum.firstBad = c.firstBad;
    sum.badGuarded += c.badGuarded;
  }
  std::printf("div6: %llu inputs inside the guard, %llu mismatches; "
              "%llu outside the guard, %llu mismatches (true division taken there)\n",
              (unsigned long long)sum.guarded, (unsigned long long)sum.badGuarded,
              (unsigned long long)sum.unguarded, (unsigned long long)sum.badUnguarded);
  if (sum.badGuarded) std::printf("first guarded mismatch: 0x%08x\n", sum.firstBad);
  return sum.badGuarded ? 1 : 0;
}
