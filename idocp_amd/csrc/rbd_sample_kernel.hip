// Sampling around a torque sequence (idocp_rbd_perturb_torques, idocp_rbd_importance_weights, idocp_rbd_weighted_mean; include/idocp_hip.h): an
// ADDITION like the rollout and its score -- the reference has no counterpart.
//
// perturb   one thread per (step k, sample i, torque pair j / 2), the pair running fastest so that a wavefront writes consecutive doubles.  The
//           Philox words and their uniforms come from rbd_sampler.hpp (the text a CPU program holds to the known-answer vectors); Box-Muller with
//           sincospi, because u2 is already a fraction of a turn.  Sample 0 is the clamped nominal itself.
// weights   four small launches: the minimum of every chunk of IDOCP_RBD_REDUCE_CHUNK scores with its index and the count of finite scores; the fold of those;
//           the weights and the chunk partials of their sum and of the sum of their squares; the fold of those, in index order, into stats.
// mean      the hot path, x [rows][n][m] read once.  One workgroup per (row, chunk): the chunk's IDOCP_RBD_REDUCE_CHUNK * m doubles are contiguous, the lanes
//           stride over them by the largest multiple of m that fits the workgroup, so a lane keeps ONE column (lane % m) and a wavefront reads
//           consecutive doubles.  A lane adds its samples in index order, a fixed tree in LDS folds the lanes of a column, the partials go to the
//           handle's scratch; a second launch adds the chunks in index order and divides.  A sample of weight 0 is skipped (a select, not a
//           product), so what a diverged rollout left there does not matter.
// Every sum has ONE order whatever n, rows or the launch is, and there is no floating-point atomic: results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rbd_launch.hpp"
#include "rbd_sampler.hpp"

namespace idocp_dev {

namespace {

constexpr int TPB = RBD_SAMPLE_THREADS;
constexpr int CHUNK = IDOCP_RBD_REDUCE_CHUNK;
static_assert(CHUNK % TPB == 0, "a lane takes CHUNK / TPB samples of a chunk");
static_assert(IDOCP_RBD_MEAN_MAX_COLUMNS < RBD_PARTIAL_STRIDE && IDOCP_RBD_MEAN_MAX_COLUMNS <= TPB, "one lane group per column, the weight sum behind the columns");

// ---------------------------------------------------------------------------------------------------------------- perturb

__global__ __launch_bounds__(TPB) void rbd_perturb_kernel(RbdPerturbArgs a) {
  const unsigned npairs = (unsigned)(a.nu + 1) / 2;
  const unsigned long long t = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
  if (t >= (unsigned long long)a.n * npairs) return;
  unsigned i, pair;
  if ((t >> 32) == 0) { i = (unsigned)t / npairs; pair = (unsigned)t - i * npairs; }
  else { i = (unsigned)(t / npairs); pair = (unsigned)(t - (unsigned long long)i * npairs); }
  const int j0 = 2 * (int)pair;
  const bool two = j0 + 1 < a.nu;
  const double s0 = a.sigma[j0], s1 = two ? a.sigma[j0 + 1] : 0.0;
  for (int k = blockIdx.y; k < a.steps; k += gridDim.y) {
    double z0 = 0.0, z1 = 0.0;
    if (i != 0) {
      unsigned r[4];
      samplerWords(a.seed, a.draw, (unsigned)(a.first_step + k), i, pair, r);
      double u1, u2, s, c;
      samplerUniforms(r, &u1, &u2);
      const double rho = sqrt(-2.0 * log(u1));
      sincospi(2.0 * u2, &s, &c);
      z0 = rho * c; z1 = rho * s;
    }
    const double* __restrict__ nom = a.u_nominal + (size_t)k * a.nu;
    double* __restrict__ out = a.u_samples + ((size_t)k * a.n + i) * a.nu;
    double u = nom[j0] + s0 * z0;
    if (a.u_min) { const double lo = a.u_min[j0]; u = u < lo ? lo : u; }
    if (a.u_max) { const double hi = a.u_max[j0]; u = u > hi ? hi : u; }
    out[j0] = u;
    if (two) {
      u = nom[j0 + 1] + s1 * z1;
      if (a.u_min) { const double lo = a.u_min[j0 + 1]; u = u < lo ? lo : u; }
      if (a.u_max) { const double hi = a.u_max[j0 + 1]; u = u > hi ? hi : u; }
      out[j0 + 1] = u;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the fixed trees

// the sum of one value per lane of the workgroup: lane l takes lane l + h for h = TPB / 2, TPB / 4, ... 1
__device__ __forceinline__ double blockSum(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();                                        // (s may still be read from the tree before)
  s[t] = v;
  __syncthreads();
  for (int h = TPB / 2; h > 0; h >>= 1) {
    if (t < h) s[t] += s[t + h];
    __syncthreads();
  }
  return s[0];
}

// the sum of a chunk's weights: lane l adds samples l, l + TPB, ... of the chunk in that order, then the tree.  w: the chunk's weights in LDS, 0
// behind the last sample.  The very sum of idocp_rbd_importance_weights' W and of idocp_rbd_weighted_mean's divisor.
__device__ __forceinline__ double chunkSum(const double* w, double* s) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < CHUNK / TPB; ++j) acc += w[threadIdx.x + j * TPB];
  return blockSum(acc, s);
}

struct MinAt { double s; int at; };                       // at < 0: no finite score seen
__device__ __forceinline__ MinAt lower(MinAt a, MinAt b) {
  const bool take = b.at >= 0 && (a.at < 0 || b.s < a.s || (b.s == a.s && b.at < a.at));
  return take ? b : a;
}
// the lowest finite score of the workgroup's lanes with the lowest index at a tie (any order of folding gives this pair), and the sum of `count`
__device__ __forceinline__ MinAt blockMin(MinAt v, int* count, double* s_val, int* s_at, int* s_count) {
  const int t = threadIdx.x;
  s_val[t] = v.s; s_at[t] = v.at; s_count[t] = *count;
  __syncthreads();
  for (int h = TPB / 2; h > 0; h >>= 1) {
    if (t < h) {
      const MinAt m = lower(MinAt{s_val[t], s_at[t]}, MinAt{s_val[t + h], s_at[t + h]});
      s_val[t] = m.s; s_at[t] = m.at; s_count[t] += s_count[t + h];
    }
    __syncthreads();
  }
  *count = s_count[0];
  return MinAt{s_val[0], s_at[0]};
}

// ---------------------------------------------------------------------------------------------------------------- weights

// s_i = cost_i + penalty violation_i, the product rounded before the sum (no contraction into an fma: the number a caller computes on the host)
__device__ __forceinline__ double scoreOf(const RbdWeightArgs& a, long i) {
#pragma clang fp contract(off)
  const double c = a.cost[i];
  if (!a.violation) return c;
  const double p = a.penalty * a.violation[i];
  return c + p;
}

// scratch of the weights call, nchunks doubles each: the chunk minima, their indices, the counts of finite scores, sum w, sum w^2
__global__ __launch_bounds__(TPB) void rbd_weights_chunk_min_kernel(RbdWeightArgs a) {
  __shared__ double s_val[TPB];
  __shared__ int s_at[TPB], s_count[TPB];
  const int chunk = blockIdx.x;
  const long i0 = (long)chunk * CHUNK;
  MinAt m{0.0, -1};
  int count = 0;
#pragma unroll
  for (int j = 0; j < CHUNK / TPB; ++j) {
    const long i = i0 + threadIdx.x + j * TPB;
    if (i < a.n) {
      const double s = scoreOf(a, i);
      if (std::isfinite(s)) { ++count; m = lower(m, MinAt{s, (int)i}); }
    }
  }
  m = blockMin(m, &count, s_val, s_at, s_count);
  if (threadIdx.x == 0) {
    a.scratch[chunk] = m.s;
    a.scratch[a.nchunks + chunk] = (double)m.at;
    a.scratch[2 * (size_t)a.nchunks + chunk] = (double)count;
  }
}

// one workgroup: stats[0 .. 2] = {|F|, s_min, argmin} ({0, NaN, -1} when F is empty)
__global__ __launch_bounds__(TPB) void rbd_weights_fold_min_kernel(RbdWeightArgs a) {
  __shared__ double s_val[TPB];
  __shared__ int s_at[TPB], s_count[TPB];
  MinAt m{0.0, -1};
  double total = 0.0;
  for (int c = threadIdx.x; c < a.nchunks; c += TPB) {
    m = lower(m, MinAt{a.scratch[c], (int)a.scratch[a.nchunks + c]});
    total += a.scratch[2 * (size_t)a.nchunks + c];          // (integers below 2^53: exact in any order)
  }
  int none = 0;
  m = blockMin(m, &none, s_val, s_at, s_count);
  const double all = blockSum(total, s_val);
  if (threadIdx.x == 0) {
    a.stats[0] = all;
    a.stats[1] = m.at >= 0 ? m.s : __builtin_nan("");
    a.stats[2] = (double)m.at;
  }
}

// weights[i] and the chunk partials of sum w and sum w^2
__global__ __launch_bounds__(TPB) void rbd_weights_write_kernel(RbdWeightArgs a) {
  __shared__ double s_w[CHUNK], s_tree[TPB];
  const int chunk = blockIdx.x;
  const long i0 = (long)chunk * CHUNK;
  const double s_min = a.stats[1];                        // (NaN when F is empty: no score is finite then, and every weight is 0)
#pragma unroll
  for (int j = 0; j < CHUNK / TPB; ++j) {
    const int l = threadIdx.x + j * TPB;
    const long i = i0 + l;
    double w = 0.0;
    if (i < a.n) {
      const double s = scoreOf(a, i);
      if (std::isfinite(s)) w = exp(-(s - s_min) / a.temperature);
      a.weights[i] = w;
    }
    s_w[l] = w;
  }
  __syncthreads();
  const double sum = chunkSum(s_w, s_tree);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CHUNK / TPB; ++j) { const int l = threadIdx.x + j * TPB; s_w[l] = s_w[l] * s_w[l]; }
  __syncthreads();
  const double sum2 = chunkSum(s_w, s_tree);
  if (threadIdx.x == 0) {
    a.scratch[3 * (size_t)a.nchunks + chunk] = sum;
    a.scratch[4 * (size_t)a.nchunks + chunk] = sum2;
  }
}

// one lane: the chunks in index order; stats[3 .. 4] = {W, W^2 / sum w^2} ({0, 0} when F is empty)
__global__ void rbd_weights_fold_sum_kernel(RbdWeightArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double* __restrict__ p = a.scratch + 3 * (size_t)a.nchunks;
  const double* __restrict__ p2 = a.scratch + 4 * (size_t)a.nchunks;
  double W = 0.0, W2 = 0.0;
#pragma unroll 8
  for (int c = 0; c < a.nchunks; ++c) { W += p[c]; W2 += p2[c]; }
  a.stats[3] = W;
  a.stats[4] = W > 0.0 ? W * W / W2 : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- weighted mean

__global__ __launch_bounds__(TPB) void rbd_mean_chunk_kernel(RbdMeanArgs a) {
  __shared__ double s_w[CHUNK], s_tree[TPB];
  const int t = threadIdx.x, m = a.m;
  const int block = (int)blockIdx.x, row = block / a.nchunks, chunk = block - row * a.nchunks;
  const long i0 = (long)chunk * CHUNK;
  const int count = (int)(a.n - i0 < CHUNK ? a.n - i0 : CHUNK);      // samples of this chunk
#pragma unroll
  for (int j = 0; j < CHUNK / TPB; ++j) { const int l = t + j * TPB; s_w[l] = l < count ? a.weights[i0 + l] : 0.0; }
  __syncthreads();
  const int groups = TPB / m, stride = groups * m;        // lanes 0 .. stride - 1 work: lane = group * m + column
  const int group = t / m;
  const double* __restrict__ x = a.x + ((size_t)row * a.n + i0) * m;
  const int total = count * m;
  double acc = 0.0;
  if (t < stride) {
    int sample = group;
#pragma unroll 4
    for (int e = t; e < total; e += stride, sample += groups) {
      const double w = s_w[sample], xv = x[e];
      acc = w != 0.0 ? fma(w, xv, acc) : acc;
    }
  }
  const double wsum = chunkSum(s_w, s_tree);
  __syncthreads();
  s_tree[t] = acc;
  __syncthreads();
  int top = 1;
  while (top < groups) top <<= 1;
  for (int h = top >> 1; h > 0; h >>= 1) {                // the lanes of a column: group g takes group g + h
    if (t < stride && group < h && group + h < groups) s_tree[t] += s_tree[t + h * m];
    __syncthreads();
  }
  double* __restrict__ part = a.scratch + (size_t)blockIdx.x * RBD_PARTIAL_STRIDE;
  if (t < m) part[t] = s_tree[t];
  if (t == 0) part[RBD_PARTIAL_STRIDE - 1] = wsum;
}

// one lane per (row, column): the chunks in index order, then the division
__global__ __launch_bounds__(TPB) void rbd_mean_fold_kernel(RbdMeanArgs a) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= a.rows * a.m) return;
  const int row = e / a.m, col = e - row * a.m;
  const double* __restrict__ part = a.scratch + (size_t)row * a.nchunks * RBD_PARTIAL_STRIDE;
  double sum = 0.0, W = 0.0;
#pragma unroll 8
  for (int c = 0; c < a.nchunks; ++c) {
    sum += part[(size_t)c * RBD_PARTIAL_STRIDE + col];
    W += part[(size_t)c * RBD_PARTIAL_STRIDE + RBD_PARTIAL_STRIDE - 1];
  }
  a.mean[e] = sum / W;
}

}  // namespace

void rbdPerturb(const RbdPerturbArgs& a, hipStream_t st) {
  const unsigned long long threads = (unsigned long long)a.n * (unsigned)((a.nu + 1) / 2);
  const dim3 grid((unsigned)((threads + TPB - 1) / TPB), (unsigned)(a.steps < 65535 ? a.steps : 65535));
  hipLaunchKernelGGL(rbd_perturb_kernel, grid, dim3(TPB), 0, st, a);
}

void rbdWeights(const RbdWeightArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(rbd_weights_chunk_min_kernel, dim3((unsigned)a.nchunks), dim3(TPB), 0, st, a);
  hipLaunchKernelGGL(rbd_weights_fold_min_kernel, dim3(1), dim3(TPB), 0, st, a);
  hipLaunchKernelGGL(rbd_weights_write_kernel, dim3((unsigned)a.nchunks), dim3(TPB), 0, st, a);
  hipLaunchKernelGGL(rbd_weights_fold_sum_kernel, dim3(1), dim3(64), 0, st, a);
}

void rbdMean(const RbdMeanArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(rbd_mean_chunk_kernel, dim3((unsigned)a.rows * (unsigned)a.nchunks), dim3(TPB), 0, st, a);
  hipLaunchKernelGGL(rbd_mean_fold_kernel, dim3((unsigned)((a.rows * a.m + TPB - 1) / TPB)), dim3(TPB), 0, st, a);
}

}  // namespace idocp_dev
