// flowsim_es.h -- evolution strategies around a policy population (include/flowsim.h fs_es_*): what the reference's
// flow/benchmarks/rllib/es_runner.py and ars_runner.py hand to RLlib's ES / ARS trainers -- a few thousand whole-episode
// rollouts of perturbed policies, a ranking of their returns, one weighted sum of noise vectors -- as four small kernels
// next to fs_population_rollout_dev.  N antithetic pairs and E evaluation members: M = 2 N + E weight sets.
//
// THE NOISE: eps(p, e) = gauss<float>(noise_seed, replica = p, vehicle = 0x60000000 | generation, step = e, exact = true):
// the library's exact Box-Muller (flowsim_kernels.h bm_ln_exact / bm_cos_exact2; oracle/refsim.py gaussian_noise(exact=True)
// is its numpy twin, bit for bit).  Four consecutive e share one Philox block, so every kernel below works on blocks
// b = e / 4 with gauss4 (which evaluates gauss()'s expressions).  No [N, P] matrix exists: k_es_grad draws the noise again.
//
// SUMMATION ORDERS (each a function of the shapes alone; no float atomics anywhere):
//   k_es_fitness  a replica: ret += (double)rew[k][r], k ascending, up to and including its first done != 0.
//                 a member:  fit[m] = (((0 + ret[m g]) + ret[m g + 1]) + ... + ret[m g + g - 1]) / g, one lane, in double.
//   k_es_weights  statistics and the ARS mean / squared deviations: one lane, ascending index (ARS: kept directions in
//                 ascending p, F+ before F-), in double.  Ranks are counts: no sum.
//   k_es_grad     workgroup (x, y) owns the Philox blocks 256 x .. 256 x + 255 (a lane each: four elements e) and the
//                 directions ES_CHUNK y .. ES_CHUNK (y + 1) - 1: acc = (acc + u[p] * eps(p, e)) for those p ascending,
//                 starting from +0, product and sum each rounded to float32 (a direction with u[p] == 0 adds exactly
//                 nothing and is skipped).  The partial goes to work[y][e]; the workgroup that draws the LAST ticket of
//                 column x (an integer counter per x) adds the partials g = ((0 + work[0][e]) + work[1][e]) + ... in
//                 ascending y and writes the result.  gridDim.y = ceil(N / ES_CHUNK): N alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fs {
constexpr int ES_MAX_PAIRS = 2048;                     // (include/flowsim.h FS_ES_MAX_PAIRS)
constexpr int ES_CHUNK = 32;                           // directions per workgroup of k_es_grad
constexpr int ES_GRAD_THREADS = 256, ES_MAX_COLS = 16384;   // columns of 256 Philox blocks: P <= 2^24
constexpr int ES_W_THREADS = 1024;
constexpr uint32_t ES_NOISE_COLUMN = 0x60000000u;      // next to the vehicles' columns and the policies' (0x40000000 + agent)

__host__ __device__ constexpr int es_chunks(int N) { return (N + ES_CHUNK - 1) / ES_CHUNK; }
__host__ __device__ constexpr long long es_blocks(long long P) { return (P + 3) / 4; }
__host__ __device__ constexpr size_t es_work_floats(long long P, int N) { return size_t(es_chunks(N)) * size_t(P); }
}  // namespace fs

namespace fsim {
// (defined in the learn_f32 part: flowsim_part.hip with -DFS_PART_LEARN=1)
int launch_es_perturb(hipStream_t stream, long long P, int N, int E, long long stride, const float* theta, float sigma,
                      uint32_t seed_lo, uint32_t seed_hi, uint32_t generation, float* w);
int launch_es_fitness(hipStream_t stream, int K, int M, int group, const float* rew, const uint8_t* done, int accumulate,
                      double* ret, uint8_t* alive, double* fit);
int launch_es_weights(hipStream_t stream, int mode, int N, int E, int top, const double* fit, float* u, double* stats);
int launch_es_grad(hipStream_t stream, int mode, long long P, int N, const float* u, uint32_t seed_lo, uint32_t seed_hi,
                   uint32_t generation, float coef, float* theta, float* grad, float* work, unsigned* tickets);
}  // namespace fsim

#ifdef FS_PART_LEARN
namespace fs {

// row q < N: the pair (2 q, 2 q + 1) of direction q; row N + i: evaluation member 2 N + i (theta itself).  A lane = one
// Philox block of one row.
__global__ __launch_bounds__(256) void k_es_perturb(long long P, int N, int E, long long stride,
                                                    const float* __restrict__ theta, float sigma, uint32_t seed_lo,
                                                    uint32_t seed_hi, uint32_t column, float* __restrict__ w) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y;
  if (b >= es_blocks(P) || q >= N + E) return;
  if (q < N) {                                          // (uniform: blockIdx.y)
    float g[4];
    gauss4<float>(seed_lo, seed_hi, uint32_t(q), column, uint32_t(b), g, true);
    float* wp = w + size_t(2 * q) * size_t(stride);
    float* wm = wp + size_t(stride);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * b + j;
      if (e < P) {
        const float t = sigma * g[j];
        const float th = theta[e];
        wp[e] = th + t;
        wm[e] = th - t;
      }
    }
  } else {
    float* we = w + (size_t(2 * N) + size_t(q - N)) * size_t(stride);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * b + j;
      if (e < P) we[e] = theta[e];
    }
  }
}

// one workgroup (a wave) per member: lane t walks replicas m g + t, m g + t + 64, ...; then lane 0 adds the member's returns
__global__ __launch_bounds__(64) void k_es_fitness(int K, long long R, int group, const float* __restrict__ rew,
                                                   const uint8_t* __restrict__ done, int accumulate, double* ret,
                                                   uint8_t* __restrict__ alive, double* __restrict__ fit) {
  const int m = blockIdx.x, t = threadIdx.x;
  const long long r0 = (long long)m * group;
  for (int i = t; i < group; i += 64) {
    const long long r = r0 + i;
    double acc = accumulate ? ret[r] : 0.0;
    bool live = accumulate ? alive[r] != 0 : true;
    for (int k = 0; k < K; ++k) {
      const size_t at = size_t(k) * size_t(R) + size_t(r);
      const float rw = rew[at];
      const uint8_t dn = done[at];
      if (live) acc += double(rw);
      live = live && dn == 0;
    }
    ret[r] = acc;
    alive[r] = live ? 1 : 0;
  }
  __syncthreads();                                      // (the workgroup's own stores to ret: visible to its lane 0)
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < group; ++i) s += ret[r0 + i];
    fit[m] = s / double(group);
  }
}

// ONE workgroup.  LDS: the 2 N returns (32 KB at N = 2048), the kept flags, the ARS scale.
__global__ __launch_bounds__(ES_W_THREADS) void k_es_weights(int mode, int N, int E, int top, const double* __restrict__ fit,
                                                              float* __restrict__ u, double* __restrict__ stats) {
  __shared__ double f[2 * ES_MAX_PAIRS];
  __shared__ float c[2 * ES_MAX_PAIRS];                 // ES: the centered ranks; ARS: 1 = kept
  __shared__ double scale;
  const int t = threadIdx.x, n2 = 2 * N;
  for (int i = t; i < n2; i += ES_W_THREADS) f[i] = fit[i];
  __syncthreads();
  if (t == ES_W_THREADS - 1) {                          // the statistics: one lane, ascending index
    double s = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
    for (int i = 0; i < n2; ++i) {
      s += f[i];
      lo = fmin(lo, f[i]);
      hi = fmax(hi, f[i]);
    }
    double se = 0.0;
    for (int i = 0; i < E; ++i) se += fit[n2 + i];
    stats[0] = s / double(n2);
    stats[1] = lo;
    stats[2] = hi;
    stats[3] = E > 0 ? se / double(E) : __builtin_nan("");
  }
  if (mode == 0) {                                      // ES: centered ranks
    for (int i = t; i < n2; i += ES_W_THREADS) {
      const double fi = f[i];
      int rank = 0;
      for (int j = 0; j < n2; ++j) rank += (f[j] < fi || (f[j] == fi && j < i)) ? 1 : 0;
      c[i] = float(double(rank) / double(n2 - 1) - 0.5);
    }
    __syncthreads();
    const float nf = float(N);
    for (int p = t; p < N; p += ES_W_THREADS) u[p] = (c[2 * p] - c[2 * p + 1]) / nf;
    return;
  }
  // ARS: the top b directions by max(F+, F-), ties to the smaller p
  const int b = (top <= 0 || top > N) ? N : top;
  for (int p = t; p < N; p += ES_W_THREADS) {
    const double kp = fmax(f[2 * p], f[2 * p + 1]);
    int rank = 0;
    for (int q = 0; q < N; ++q) {
      const double kq = fmax(f[2 * q], f[2 * q + 1]);
      rank += (kq > kp || (kq == kp && q < p)) ? 1 : 0;
    }
    c[p] = rank < b ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (t == 0) {                                         // the population standard deviation of the 2 b kept returns
    double s = 0.0;
    for (int p = 0; p < N; ++p) {
      if (c[p] != 0.0f) {
        s += f[2 * p];
        s += f[2 * p + 1];
      }
    }
    const double mean = s / double(2 * b);
    double ss = 0.0;
    for (int p = 0; p < N; ++p) {
      if (c[p] != 0.0f) {
        const double da = f[2 * p] - mean, db = f[2 * p + 1] - mean;
        ss += da * da;
        ss += db * db;
      }
    }
    scale = double(b) * sqrt(ss / double(2 * b));
  }
  __syncthreads();
  const double bs = scale;
  for (int p = t; p < N; p += ES_W_THREADS)
    u[p] = (c[p] != 0.0f && bs != 0.0) ? float((f[2 * p] - f[2 * p + 1]) / bs) : 0.0f;
}

// grid (columns of 256 Philox blocks, chunks of ES_CHUNK directions); tickets[x]: zero between launches
__global__ __launch_bounds__(ES_GRAD_THREADS) void k_es_grad(int mode, long long P, int N, const float* __restrict__ u,
                                                             uint32_t seed_lo, uint32_t seed_hi, uint32_t column, float coef,
                                                             float* theta, float* __restrict__ grad, float* work,
                                                             unsigned* tickets) {
  __shared__ int is_last;
  const int t = threadIdx.x, y = blockIdx.y, G = gridDim.y;
  const long long b = (long long)blockIdx.x * ES_GRAD_THREADS + t;
  const bool in = b < es_blocks(P);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int p1 = (y + 1) * ES_CHUNK < N ? (y + 1) * ES_CHUNK : N;
  for (int p = y * ES_CHUNK; p < p1; ++p) {
    const float up = u[p];                              // (uniform)
    if (up == 0.0f) continue;
    float g[4];
    gauss4<float>(seed_lo, seed_hi, uint32_t(p), column, uint32_t(in ? b : 0), g, true);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = acc[j] + up * g[j];
  }
  if (in) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * b + j;
      if (e < P) work[size_t(y) * size_t(P) + size_t(e)] = acc[j];
    }
  }
  // every lane releases its partials to the device, the barrier follows, lane 0 draws the column's ticket; the workgroup
  // that draws the last of the column's G tickets acquires and combines
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (t == 0) {
    const unsigned drawn = __hip_atomic_fetch_add(tickets + blockIdx.x, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = drawn == unsigned(G - 1) ? 1 : 0;
  }
  __syncthreads();
  if (is_last == 0) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (in) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * b + j;
      if (e < P) {
        float g = 0.0f;
        for (int yy = 0; yy < G; ++yy)
          g = g + __hip_atomic_load(work + size_t(yy) * size_t(P) + size_t(e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mode == 0) grad[e] = -g + coef * theta[e];
        else theta[e] = theta[e] + coef * g;
      }
    }
  }
  if (t == 0) __hip_atomic_store(tickets + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace fs

namespace fsim {

int launch_es_perturb(hipStream_t stream, long long P, int N, int E, long long stride, const float* theta, float sigma,
                      uint32_t seed_lo, uint32_t seed_hi, uint32_t generation, float* w) {
  const unsigned cols = unsigned((fs::es_blocks(P) + 255) / 256);
  hipLaunchKernelGGL(fs::k_es_perturb, dim3(cols, unsigned(N + E)), dim3(256), 0, stream, P, N, E, stride, theta, sigma,
                     seed_lo, seed_hi, fs::ES_NOISE_COLUMN | (generation & 0x1FFFFFFFu), w);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_es_fitness(hipStream_t stream, int K, int M, int group, const float* rew, const uint8_t* done, int accumulate,
                      double* ret, uint8_t* alive, double* fit) {
  hipLaunchKernelGGL(fs::k_es_fitness, dim3(unsigned(M)), dim3(64), 0, stream, K, (long long)M * group, group, rew, done,
                     accumulate, ret, alive, fit);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_es_weights(hipStream_t stream, int mode, int N, int E, int top, const double* fit, float* u, double* stats) {
  hipLaunchKernelGGL(fs::k_es_weights, dim3(1), dim3(fs::ES_W_THREADS), 0, stream, mode, N, E, top, fit, u, stats);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_es_grad(hipStream_t stream, int mode, long long P, int N, const float* u, uint32_t seed_lo, uint32_t seed_hi,
                   uint32_t generation, float coef, float* theta, float* grad, float* work, unsigned* tickets) {
  const unsigned cols = unsigned((fs::es_blocks(P) + fs::ES_GRAD_THREADS - 1) / fs::ES_GRAD_THREADS);
  hipLaunchKernelGGL(fs::k_es_grad, dim3(cols, unsigned(fs::es_chunks(N))), dim3(fs::ES_GRAD_THREADS), 0, stream, mode, P, N, u,
                     seed_lo, seed_hi, fs::ES_NOISE_COLUMN | (generation & 0x1FFFFFFFu), coef, theta, grad, work, tickets);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

}  // namespace fsim
#endif  // FS_PART_LEARN
