// The generator of idocp_rbd_perturb_torques (idocp_amd/csrc/rbd_sampler.hpp) as a stand-alone program, built with the address and
// undefined-behaviour sanitizers by tests/test_rbd_sample_host.py: Philox4x32-10 against the published known-answer vectors, the word-to-uniform
// conversion at its end points, and a table of words and uniforms that the Python referee (tests/rbd_sample.py) must match bit for bit.  The header
// is the very text the kernel compiles; no HIP runtime header, no device.
#define IDOCP_NO_HIP_RUNTIME
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rbd_sampler.hpp"

using namespace idocp_dev;

namespace {

int failures = 0;

void expectWords(const char* what, const unsigned c[4], const unsigned k[2], const unsigned want[4]) {
  unsigned got[4];
  philox4x32_10(c, k, got);
  if (std::memcmp(got, want, sizeof(got)) != 0) {
    std::printf("FAIL %s: got %08x %08x %08x %08x, want %08x %08x %08x %08x\n", what, got[0], got[1], got[2], got[3], want[0], want[1], want[2], want[3]);
    ++failures;
  }
}

void expectDouble(const char* what, double got, double want) {
  if (std::memcmp(&got, &want, sizeof(double)) != 0) { std::printf("FAIL %s: got %a, want %a\n", what, got, want); ++failures; }
}

uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, sizeof(b)); return b; }

}  // namespace

int main() {
  // the known-answer vectors of Random123 (kat_vectors: philox4x32 10)
  {
    const unsigned c[4] = {0, 0, 0, 0}, k[2] = {0, 0}, want[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
    expectWords("zero counter, zero key", c, k, want);
  }
  {
    const unsigned c[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, k[2] = {0xffffffffu, 0xffffffffu};
    const unsigned want[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
    expectWords("all-ones counter and key", c, k, want);
  }
  {
    const unsigned c[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k[2] = {0xa4093822u, 0x299f31d0u};
    const unsigned want[4] = {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u};
    expectWords("digits of pi", c, k, want);
  }
  // the conversion at its end points: u1 never 0 and never 1, u2 reaches 0 and stays below 1
  {
    const unsigned zero[4] = {0, 0, 0, 0}, ones[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    double u1, u2;
    samplerUniforms(zero, &u1, &u2);
    expectDouble("u1 of all-zero words", u1, 0x1p-53);
    expectDouble("u2 of all-zero words", u2, 0.0);
    samplerUniforms(ones, &u1, &u2);
    expectDouble("u1 of all-one words", u1, 1.0 - 0x1p-53);
    expectDouble("u2 of all-one words", u2, 1.0 - 0x1p-53);
    // the low 12 / 11 bits of a pair are dropped, not rounded
    const unsigned low[4] = {0xfffu, 0, 0x7ffu, 0};
    samplerUniforms(low, &u1, &u2);
    expectDouble("u1 of the dropped bits", u1, 0x1p-53);
    expectDouble("u2 of the dropped bits", u2, 0.0);
    const unsigned next[4] = {0x1000u, 0, 0x800u, 0};
    samplerUniforms(next, &u1, &u2);
    expectDouble("u1 one step up", u1, 1.5 * 0x1p-52);
    expectDouble("u2 one step up", u2, 0x1p-53);
  }
  // the counter layout (i, step, pair, draw) and the key (seed low, seed high)
  {
    const unsigned long long seed = 0x299f31d0a4093822ull;
    const unsigned c[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k[2] = {0xa4093822u, 0x299f31d0u};
    unsigned a[4], b[4];
    philox4x32_10(c, k, a);
    samplerWords(seed, /*draw*/ 0x03707344u, /*step*/ 0x85a308d3u, /*i*/ 0x243f6a88u, /*pair*/ 0x13198a2eu, b);
    if (std::memcmp(a, b, sizeof(a)) != 0) { std::printf("FAIL counter layout\n"); ++failures; }
  }
  // the table for the Python referee: seed draw step i pair | four words | the bits of u1 and u2
  const unsigned long long seeds[3] = {0ull, 20260101ull, 0xfedcba9876543210ull};
  for (unsigned long long seed : seeds)
    for (unsigned draw = 0; draw < 2; ++draw)
      for (unsigned step : {0u, 7u, 4000000000u})
        for (unsigned i : {1u, 2u, 65u, 122879u})
          for (unsigned pair = 0; pair < 3; ++pair) {
            unsigned r[4];
            double u1, u2;
            samplerWords(seed, draw, step, i, pair, r);
            samplerUniforms(r, &u1, &u2);
            std::printf("table %llu %u %u %u %u %08x %08x %08x %08x %016" PRIx64 " %016" PRIx64 "\n", seed, draw, step, i, pair, r[0], r[1], r[2], r[3],
                        bits(u1), bits(u2));
          }
  if (failures) return 1;
  std::printf("rbd sampler: ok\n");
  return 0;
}
