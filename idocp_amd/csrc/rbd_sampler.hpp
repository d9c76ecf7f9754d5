// The counter-based generator of idocp_rbd_perturb_torques (include/idocp_hip.h): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC11) and the conversion of its four output words into the two uniforms of a Box-Muller pair.  Host + device, integer
// arithmetic and exact double conversions only, so the kernel (rbd_sample_kernel.hip) and a CPU program hold the very same text: under
// IDOCP_NO_HIP_RUNTIME this is a plain C++17 header without the HIP runtime (tests/cpp/rbd_sampler_host.cpp checks the published known-answer
// vectors and the end points of the conversion).
#ifndef IDOCP_RBD_SAMPLER_HPP_
#define IDOCP_RBD_SAMPLER_HPP_

#ifdef IDOCP_NO_HIP_RUNTIME
#ifndef __host__
#define __host__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#else
#include <hip/hip_runtime.h>
#endif

namespace idocp_dev {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // the two round multipliers
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // the key increments (golden ratio, sqrt 3 - 1)

// ten rounds on the counter c[4] under the key k[2]; the key is bumped between rounds (nine times)
__host__ __device__ __forceinline__ void philox4x32_10(const unsigned c[4], const unsigned k[2], unsigned out[4]) {
  unsigned c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0, p1 = (unsigned long long)PHILOX_M1 * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// u1 = (((r0 | r1 << 32) >> 12) + 0.5) 2^-52 in (0, 1): 2^-53 .. 1 - 2^-53, never 0 (its logarithm is taken); u2 = ((r2 | r3 << 32) >> 11) 2^-53 in
// [0, 1): 0 .. 1 - 2^-53.  Both are exact in a double (53 significant bits at most).
__host__ __device__ __forceinline__ void samplerUniforms(const unsigned r[4], double* u1, double* u2) {
  const unsigned long long a = ((unsigned long long)r[1] << 32 | r[0]) >> 12, b = ((unsigned long long)r[3] << 32 | r[2]) >> 11;
  *u1 = ((double)a + 0.5) * 0x1p-52;
  *u2 = (double)b * 0x1p-53;
}

// the words of sample i at step `step`, torque pair `pair` = j / 2, iteration `draw`
__host__ __device__ __forceinline__ void samplerWords(unsigned long long seed, unsigned draw, unsigned step, unsigned i, unsigned pair, unsigned out[4]) {
  const unsigned c[4] = {i, step, pair, draw}, k[2] = {(unsigned)seed, (unsigned)(seed >> 32)};
  philox4x32_10(c, k, out);
}

}  // namespace idocp_dev
#endif  // IDOCP_RBD_SAMPLER_HPP_
