// flowsim_learn.h -- the PPO update on the device: what examples/train_vec.py ppo_update does in torch between two
// rollouts, as kernels (fs_ppo_eval_dev, fs_gae_dev, fs_adv_stats_dev, fs_adv_finish_dev, fs_ppo_grad_dev / fs_ppo_grad_n_dev,
// fs_adam_dev: include/flowsim.h).
//
//   k_ppo_eval   forward only: logp [n] and val [n] of n samples (the no_grad pass; act == NULL: values alone)
//   k_gae        the reverse recurrence of train_vec.gae, one lane per replica, float32 bits of CPU torch
//   k_ppo_grad   forward, PPO loss and backward of both networks in ONE launch: one partial gradient per workgroup,
//   k_ppo_reduce ... summed over the workgroups in ascending order (no float atomics: the same inputs give the same bits)
//   k_adv_stats  the float64 advantage statistics {sum adv, sum adv^2, count} of the present rows and the float64 copy of adv
//   k_adv_finish {mean, std, n} of the three sums (one thread; the data-parallel all-reduce of the sums comes before it)
//   k_adam       torch's Adam on the packed buffers, its step count and the powers of the betas in device memory
//   k_ppo_grad<true, true>  ("k_ppo_grad_loss") the same launch with RLlib's PPO loss: the KL penalty KL(old || new), the
//                clipped value loss and the entropy bonus on top of the surrogate, four loss sums {pg, vfl, KL, H}
//   k_kl_adapt   RLlib's rule for the KL coefficient, one thread, in double: {coef, mean KL} live in device memory
//   k_ppo_grad<true, true, true>  ("k_ppo_minibatch") ONE minibatch step of a shuffled epoch in one launch: the rows are
//                gathered through a computed permutation, the last workgroup to finish reduces the partials, divides by
//                the minibatch's own count and applies Adam (MB_STEP), or leaves the raw sums for k_mb_finish (MB_PARTIAL)
//   k_mb_finish  the divide and Adam of the MB_PARTIAL chain (several shards or ranks), one workgroup like k_adam
//   NET_LS       one more flag of k_ppo_eval and of the three device-n forms of k_ppo_grad (fs_last_kernel's "k_ppo_eval_ls",
//                "k_ppo_grad_ls", "k_ppo_grad_loss_ls", "k_ppo_minibatch_ls"): the head of 2 A outputs, whose rows A .. 2A-1
//                are the log stds -- a function of the observation -- and no free log_std (PpoView::log_std == NULL)
//
// Model class (DevicePolicy's): 1..3 hidden layers of 32 tanh units on 1..160 inputs, a head of A <= 32 means with a free
// log_std [A] -- or (NET_LS) a head of 2 A rows, the A means and then the A log stds: RLlib's DiagGaussian order --; the
// value network is the same trunk with one output.  Packed weights per network: per layer W [out][in] row-major, then
// b [out] (fs_policy's layout).
//
// Mapping: a workgroup is ONE wave and a lane is ONE sample of a 64-sample tile; tile t belongs to workgroup t mod G and a
// workgroup takes its tiles in ascending order.  G depends on (n, D, A, layers) alone (ppo_groups), and so does the order
// of every sum.  A layer's 32 outputs are 32 registers of the lane; its inputs come from an LDS staging buffer [input][lane]
// (the lane's own column), its weights from the LDS copy of the network, transposed to [input][unit] so that one
// ds_read_b128 broadcasts four units' weights of an input to the wave.  The network is written ONCE (net_forward): both
// kernels call it for both networks.  A weight gradient dW[u][i] = sum_s dz[s][u] h[s][i] is NOT a cross-lane reduction
// here: the lanes re-map to (input i, half of the units), and each walks the tile's 64 samples in ascending order over the
// staged dz [sample][unit] and h [input][sample] -- 16 FMAs per five LDS reads, exact float32, fixed order.  (The
// FP32-input MFMA runs at the vector FMA rate on this chip, so it buys nothing here; at D = 3 the update is a GFLOP.)
// The workgroup's gradient lives in LDS in the packed layout and is written out once, at the end.
// Every fused multiply-add is an explicit fmaf (the library is compiled with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fs {

constexpr int PPO_MAX_OBS = 160, PPO_MAX_ACT = 32, PPO_TILE = 64;
constexpr int PPO_TS = 65;     // stride of the staging buffer S [input][sample]: conflict-free by rows and by columns
constexpr int PPO_TT = 36;     // stride of the staging buffer T [sample][unit]: rows stay 16-byte aligned
constexpr int PPO_LDS_BYTES = 160 * 1024;

struct PpoView {
  const float* pw;         // policy weights (packed)
  const float* log_std;    // [A]; NULL: the head has 2 A rows, the log stds come from rows A .. 2A-1 (NET_LS)
  const float* vw;         // value weights (packed)
  int D, A, L;
};

// packed parameter counts: a network with n_out outputs; the whole gradient [policy][log_std A][value], or with the head of
// 2 A rows (ls) [policy with its 2A-row head][value]: no log_std slot
__host__ __device__ constexpr int ppo_net_params(int D, int L, int n_out) { return 32 * D + 32 + (L - 1) * 1056 + 33 * n_out; }
__host__ __device__ constexpr int ppo_params(int D, int A, int L, bool ls = false) {
  return ls ? ppo_net_params(D, L, 2 * A) + ppo_net_params(D, L, 1) : ppo_net_params(D, L, A) + A + ppo_net_params(D, L, 1);
}
// the LDS copy of a network: [input][unit] per layer, the head padded to 32 units; the head of 2 A rows is TWO such blocks,
// rows 0 .. A-1 (means) and rows A .. 2A-1 (log stds), each padded with zeros: 1056 floats more in the policy network's copy
__host__ __device__ constexpr int ppo_net_lds(int D, int L) { return 32 * D + 32 + L * 1056; }
__host__ __device__ constexpr int ppo_nets_lds(int D, int L, bool ls) { return 2 * ppo_net_lds(D, L) + (ls ? 1056 : 0); }
__host__ __device__ constexpr int ppo_stage_floats() { return 32 * PPO_TS + PPO_TILE * PPO_TT; }
__host__ __device__ constexpr int round4(int x) { return (x + 3) & ~3; }
__host__ __device__ constexpr size_t ppo_eval_lds(int D, int L, bool ls = false) {
  return sizeof(float) * size_t(ppo_nets_lds(D, L, ls) + ppo_stage_floats());
}
__host__ __device__ constexpr size_t ppo_grad_lds(int D, int A, int L, bool ls = false) {
  return sizeof(float) * size_t(ppo_nets_lds(D, L, ls) + ppo_stage_floats() + round4(ppo_params(D, A, L, ls) + 2));
}
// workgroups of k_ppo_grad: one per tile up to what the chip holds at once (256 CUs, as many workgroups per CU as their LDS
// allows, four at the most) -- a function of (n, D, A, L) and the head's form alone
__host__ __device__ constexpr int ppo_groups(long long n, int D, int A, int L, bool ls = false) {
  const long long tiles = (n + PPO_TILE - 1) / PPO_TILE;
  const int per_cu = int(size_t(PPO_LDS_BYTES) / ppo_grad_lds(D, A, L, ls));
  const long long cap = 256LL * (per_cu > 4 ? 4 : per_cu < 1 ? 1 : per_cu);
  return int(tiles < cap ? (tiles < 1 ? 1 : tiles) : cap);
}
// floats of the partial-gradient workspace of one fs_ppo_grad_dev call
__host__ __device__ constexpr size_t ppo_work_floats(long long n, int D, int A, int L, bool ls = false) {
  return size_t(ppo_groups(n, D, A, L, ls)) * size_t(ppo_params(D, A, L, ls) + 2);
}

// the full-loss form (k_ppo_grad<true, true>): FOUR loss sums behind the gradient, in LDS and in a workgroup's row of the
// workspace.  The workgroups are ppo_groups' (the two extra floats do not move the count: the order of every sum is the
// plain form's).
constexpr int PPO_LOSS_SUMS = 4;
__host__ __device__ constexpr size_t ppo_grad_loss_lds(int D, int A, int L, bool ls = false) {
  return sizeof(float) * size_t(ppo_nets_lds(D, L, ls) + ppo_stage_floats() + round4(ppo_params(D, A, L, ls) + PPO_LOSS_SUMS));
}
static_assert(ppo_grad_loss_lds(PPO_MAX_OBS, PPO_MAX_ACT, 3) <= size_t(PPO_LDS_BYTES), "the largest model's gradient fits LDS");
static_assert(ppo_params(PPO_MAX_OBS, PPO_MAX_ACT, 3, true) == 16673 && ppo_grad_loss_lds(PPO_MAX_OBS, PPO_MAX_ACT, 3, true) == 155040 &&
              ppo_grad_loss_lds(PPO_MAX_OBS, PPO_MAX_ACT, 3, true) <= size_t(PPO_LDS_BYTES),
              "the largest model with the head of 2 A rows fits LDS");
__host__ __device__ constexpr size_t ppo_loss_work_floats(long long n, int D, int A, int L, bool ls = false) {
  return size_t(ppo_groups(n, D, A, L, ls)) * size_t(ppo_params(D, A, L, ls) + PPO_LOSS_SUMS);
}

// what the full-loss form reads on top of k_ppo_grad's arguments (all device pointers; a NULL pointer or a zero
// coefficient switches its term off for the whole launch)
struct PpoLossArgs {
  const float* mean_old;       // [n, A]  the policy's means at the time of the rollout      (KL)
                               // (NET_LS: [n, 2A], a row's A means and then its A log stds, as k_ppo_eval<true, true> writes it)
  const float* log_std_old;    // [A]     log_std at the time of the rollout                 (KL; NET_LS: not read)
  const float* val_old;        // [n]     the value network's output at the time of the rollout (value clipping)
  const double* kl_state;      // {coef, ..}: NULL = no KL term
  float vf_clip;               // <= 0: no value clipping
  float entropy_coef;          // 0: no entropy term
};

// ---- minibatches (k_ppo_minibatch, k_mb_finish).  An epoch is a shuffled pass: minibatch k of size B is rows
// perm[kB .. min((k + 1) B, n)) of the shard, and perm is COMPUTED, never stored: a balanced Feistel network of 4 rounds
// over the smallest even number of bits that holds n - 1 (at least 2), round function murmur3's fmix32 of (right half +
// round key), keys = fmix32 chains of (seed, epoch, round), cycle-walked -- re-applied until the value is < n.  The network
// is a bijection of its domain of at most 4 n values and the start is < n, so the walk comes back below n (it returns to
// its start at the latest); it takes under 4 passes on average.  32-bit integer operations only: the host (fs_ppo_perm_host),
// the kernel and numpy (flow_amd.utils.device_ppo.epoch_permutation) give the same values.
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

struct PermKey {
  uint32_t key[4];
  uint32_t n, half, mask;      // the domain is [0, 2^(2 half)), mask = 2^half - 1
};

__host__ __device__ inline PermKey perm_key(unsigned long long seed, unsigned long long epoch, uint32_t n) {
  PermKey k;
  uint32_t bits = 0;
  while (bits < 32 && (n - 1u) >> bits) ++bits;               // bits of n - 1 (n >= 1)
  k.half = bits < 2 ? 1u : (bits + 1u) / 2u;
  k.mask = (1u << k.half) - 1u;
  k.n = n;
  uint32_t b = fmix32(uint32_t(seed) + 0x9e3779b9u);
  b = fmix32(b ^ uint32_t(seed >> 32));
  b = fmix32(b + uint32_t(epoch));
  b = fmix32(b ^ uint32_t(epoch >> 32));
  for (uint32_t r = 0; r < 4; ++r) k.key[r] = fmix32(b + 0x9e3779b9u * (r + 1u));
  return k;
}

// perm[i], i < n
__host__ __device__ inline uint32_t perm_at(const PermKey& k, uint32_t i) {
  uint32_t x = i;
  do {
    uint32_t l = x >> k.half, r = x & k.mask;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q) {
      const uint32_t f = fmix32(r + k.key[q]) & k.mask;
      const uint32_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << k.half) | r;
  } while (x >= k.n);
  return x;
}

// workgroups of k_ppo_minibatch: ppo_groups of a batch of B samples -- a function of (B, D, A, L) alone, the short last
// minibatch of an epoch included (its spare workgroups write zero partials)
__host__ __device__ constexpr int ppo_mb_groups(long long B, int D, int A, int L, bool ls = false) {
  return ppo_groups(B, D, A, L, ls);
}
// 4-byte words of the workspace of one fs_ppo_minibatch_dev call: G partials [P + 4], then G integer counts
__host__ __device__ constexpr size_t ppo_mb_work_floats(long long B, int D, int A, int L, bool ls = false) {
  return size_t(ppo_mb_groups(B, D, A, L, ls)) * size_t(ppo_params(D, A, L, ls) + PPO_LOSS_SUMS + 1);
}

constexpr int MB_STEP = 0, MB_PARTIAL = 1;                           // the tail's modes
constexpr int MB_ACCUMULATE = 1, MB_FIRST = 2, MB_LAST = 4;          // flags

// what the minibatch form reads and writes on top of the full-loss form's arguments
struct PpoMbArgs {
  unsigned long long seed;
  unsigned long long* epoch;   // the learner's epoch counter (device)
  long long B, k;              // minibatch k of B rows
  int mode, flags;
  unsigned* ticket;            // the handle's (zero between launches)
  float* grad;                 // [P]
  float* loss_sums;            // [4]
  double* count;               // [1] (MB_PARTIAL)
  float *w, *m, *v;            // [P] the packed weights and Adam's moments (MB_STEP)
  double* state;               // Adam's {t, beta1^t, beta2^t}
  double lr, beta1, beta2, eps;
};

// k_adv_stats: workgroups (a function of n alone) and the handle's scratch [ticket][G x 3 partial sums]
constexpr int ADV_THREADS = 256, ADV_MAX_GROUPS = 512;
constexpr size_t ADV_SCRATCH_BYTES = sizeof(double) * (1 + 3 * ADV_MAX_GROUPS);      // [ticket][G x 3 partial sums]

__host__ __device__ constexpr int adv_groups(long long n) {
  const long long g = (n + 4 * ADV_THREADS - 1) / (4 * ADV_THREADS);                 // four rows per lane before G saturates
  return int(g < 1 ? 1 : g > ADV_MAX_GROUPS ? ADV_MAX_GROUPS : g);
}

// k_episode_stats: workgroups (a function of R alone) and the handle's scratch [ticket][G x EP_STATS partials]
constexpr int EP_THREADS = 256, EP_MAX_GROUPS = 512, EP_STATS = 8, EP_AHEAD = 8;
constexpr size_t EP_SCRATCH_BYTES = sizeof(double) * (1 + EP_STATS * EP_MAX_GROUPS);

__host__ __device__ constexpr int ep_groups(long long R) {
  const long long g = (R + EP_THREADS - 1) / EP_THREADS;                             // one replica per lane before G saturates
  return int(g < 1 ? 1 : g > EP_MAX_GROUPS ? EP_MAX_GROUPS : g);
}

}  // namespace fs

namespace fsim {
// the head of 2 A rows: a model with policy weights and no free log_std (fs_ppo_model's log_std_dev == NULL)
inline bool ppo_net_ls(const fs::PpoView& m) { return m.pw != nullptr && m.log_std == nullptr; }
// (defined in the learn_f32 part: flowsim_part.hip with -DFS_PART_LEARN=1)
int launch_ppo_eval(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act, float* logp,
                    float* val);
int launch_gae(hipStream_t stream, int K, long long R, const float* rew, const float* val, const float* last_val,
               const uint8_t* done, float g, float gl, float* adv, float* ret);
int launch_ppo_grad(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act,
                    const float* logp_old, const double* adv, const float* ret, const double* mean_std, float lo, float hi,
                    float vf_coef, float inv_n, int accumulate, float* grad, float* loss, float* work);
// (mean_std_n [3] = {mean, std, n}: the kernel takes inv_n = float(1.0 / n) from the device)
int launch_ppo_grad_n(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act,
                      const float* logp_old, const double* adv, const float* ret, const double* mean_std_n, float lo, float hi,
                      float vf_coef, int accumulate, float* grad, float* loss, float* work);
// (the full-loss form: loss [4] = {sum pg, sum vfl, sum KL, sum H}; work: ppo_loss_work_floats)
int launch_ppo_eval_dist(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act, float* logp,
                         float* val, float* mean_old);
int launch_ppo_grad_loss(hipStream_t stream, const fs::PpoView& m, const fs::PpoLossArgs& x, long long n, const float* obs,
                         const float* act, const float* logp_old, const double* adv, const float* ret, const double* mean_std_n,
                         float lo, float hi, float vf_coef, int accumulate, float* grad, float* loss, float* work);
int launch_kl_adapt(hipStream_t stream, const float* loss_sums, const double* mean_std_n, double* kl_state, double kl_target);
// (the minibatch form, fs_last_kernel's "k_ppo_minibatch", and the finish of the PARTIAL chain, "k_mb_finish")
int launch_ppo_minibatch(hipStream_t stream, const fs::PpoView& m, const fs::PpoLossArgs& x, const fs::PpoMbArgs& mb, long long n,
                         const float* obs, const float* act, const float* logp_old, const double* adv, const float* ret,
                         const double* mean_std_n, float lo, float hi, float vf_coef, float* work);
int launch_mb_finish(hipStream_t stream, int P, float* w, float* grad, float* m, float* v, double* state, const double* count,
                     unsigned long long* epoch, int flags, double lr, double beta1, double beta2, double eps);
// (scratch: fs::ADV_SCRATCH_BYTES of device memory, zero before its first use: the handle owns it)
int launch_adv_stats(hipStream_t stream, long long n, const float* adv, const float* act, int A, int accumulate, double* adv64,
                     double* stats, double* scratch);
int launch_adv_finish(hipStream_t stream, const double* stats, double* mean_std_n);
// (scratch: fs::EP_SCRATCH_BYTES of device memory, zero before its first use: the handle owns it)
int launch_episode_stats(hipStream_t stream, int K, long long R, const float* rew, const uint8_t* done, double* run_ret,
                         int32_t* run_len, double* stats, int accumulate, double* scratch);
int launch_adam(hipStream_t stream, int P, float* w, const float* g, float* m, float* v, double* state, double lr, double beta1,
                double beta2, double eps);
}  // namespace fsim

#ifdef FS_PART_LEARN
namespace fs {

__device__ __forceinline__ float ppo_tanh(float z) {                     // (flowsim_policy.h policy_tanh)
  const float e = __builtin_amdgcn_exp2f(z * 2.885390081777927f);       // exp(2 z)
  const float r = __builtin_amdgcn_rcpf(e + 1.0f);
  return __builtin_fmaf(-2.0f, r, 1.0f);                                // 1 - 2 / (exp(2 z) + 1)
}

// a packed network -> LDS (all 64 lanes; the caller ends with a barrier): layer l at lds + ppo_layer_off(l), Wt [in][32]
// then b [32]; the head's units >= n_out are zero
__device__ __forceinline__ int ppo_layer_off(int D, int l) { return l == 0 ? 0 : 32 * D + 32 + (l - 1) * 1056; }

// NET_LS: the head has 2 n_out rows and becomes two blocks, rows 0 .. n_out-1 at ppo_layer_off(D, L) and rows n_out ..
// 2 n_out-1 behind it (+ 1056), each Wt [32][32] then b [32] with the units >= n_out zero
template <bool NET_LS = false>
__device__ __forceinline__ void net_load(const float* w, int D, int L, int n_out, float* lds, int lane) {
  for (int e = lane; e < 32 * D; e += 64) lds[(e % D) * 32 + e / D] = w[e];
  if (lane < 32) lds[32 * D + lane] = w[32 * D + lane];
  w += 32 * D + 32;
  for (int l = 1; l <= L; ++l) {
    float* q = lds + ppo_layer_off(D, l);
    const int rows = l < L ? 32 : n_out;
    if constexpr (NET_LS) {
      if (l == L) {
        for (int blk = 0; blk < 2; ++blk, q += 1056) {
          const float* wb = w + blk * rows * 32;
          for (int e = lane; e < 1024; e += 64) q[(e & 31) * 32 + (e >> 5)] = (e >> 5) < rows ? wb[e] : 0.0f;
          if (lane < 32) q[1024 + lane] = lane < rows ? w[2 * rows * 32 + blk * rows + lane] : 0.0f;
        }
        break;
      }
    }
    for (int e = lane; e < 1024; e += 64) q[(e & 31) * 32 + (e >> 5)] = (e >> 5) < rows ? w[e] : 0.0f;
    if (lane < 32) q[1024 + lane] = lane < rows ? w[rows * 32 + lane] : 0.0f;
    w += rows * 33;
  }
}

// z[u] += sum_i Wt[i][u] S[i][lane], i ascending: the one place a layer's product is written
__device__ __forceinline__ void layer_acc(const float* wt, const float* S, int n_in, int lane, float (&z)[32]) {
  for (int i = 0; i < n_in; ++i) {
    const float x = S[i * PPO_TS + lane];
    const float4* w4 = reinterpret_cast<const float4*>(wt + i * 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 w = w4[q];
      z[4 * q + 0] = __builtin_fmaf(w.x, x, z[4 * q + 0]);
      z[4 * q + 1] = __builtin_fmaf(w.y, x, z[4 * q + 1]);
      z[4 * q + 2] = __builtin_fmaf(w.z, x, z[4 * q + 2]);
      z[4 * q + 3] = __builtin_fmaf(w.w, x, z[4 * q + 3]);
    }
  }
}

// inputs [c0, c0 + 32) of the tile's observations -> S [input][sample]: coalesced rows of 32 floats; a sample beyond n,
// or one that `keep` (a lane mask of the tile) leaves out, is staged as zeros.  GATHER (the minibatch form): sample s of the
// tile is row `row` of lane s -- the lanes hand their rows round with a ds_bpermute -- and a negative row is a lane beyond
// the minibatch's end
template <bool GATHER = false>
__device__ __forceinline__ void stage_obs(const float* obs, long long s0, long long n, int D, int c0, unsigned long long keep,
                                          float* S, int lane, int row = 0) {
  const int i = lane & 31, col = c0 + i;
#pragma unroll 4
  for (int r = 0; r < 32; ++r) {
    const int s = 2 * r + (lane >> 5);
    if constexpr (GATHER) {
      const int rs = __shfl(row, s, 64);
      const bool ok = rs >= 0 && col < D && ((keep >> s) & 1ull);
      S[i * PPO_TS + s] = ok ? obs[size_t(rs) * size_t(D) + size_t(col)] : 0.0f;
    } else {
      const bool ok = s0 + s < n && col < D && ((keep >> s) & 1ull);
      S[i * PPO_TS + s] = ok ? obs[size_t(s0 + s) * size_t(D) + size_t(col)] : 0.0f;
    }
  }
}

__device__ __forceinline__ void stage_units(const float (&h)[32], float* S, int lane) {
#pragma unroll
  for (int u = 0; u < 32; ++u) S[u * PPO_TS + lane] = h[u];
}

// THE forward pass of one network on one tile: h[l] = the lane's activations of hidden layer l (l < L), out = the head's 32
// padded outputs.  Ends without a barrier: S holds the lane's own column.
template <bool GATHER = false>
__device__ __forceinline__ void net_forward(const float* net, int D, int L, const float* obs, long long s0, long long n,
                                            unsigned long long keep, float* S, int lane, float (&h)[3][32], float (&out)[32],
                                            int row = 0) {
  float z[32];
#pragma unroll
  for (int u = 0; u < 32; ++u) z[u] = net[32 * D + u];
  for (int c0 = 0; c0 < D; c0 += 32) {
    __syncthreads();                                       // (the last readers of S are done)
    stage_obs<GATHER>(obs, s0, n, D, c0, keep, S, lane, row);
    __syncthreads();
    layer_acc(net + c0 * 32, S, D - c0 < 32 ? D - c0 : 32, lane, z);
  }
#pragma unroll
  for (int u = 0; u < 32; ++u) h[0][u] = ppo_tanh(z[u]);
#pragma unroll
  for (int l = 1; l < 3; ++l) {
    if (l < L) {
      const float* q = net + ppo_layer_off(D, l);
      stage_units(h[l - 1], S, lane);
#pragma unroll
      for (int u = 0; u < 32; ++u) z[u] = q[1024 + u];
      layer_acc(q, S, 32, lane, z);
#pragma unroll
      for (int u = 0; u < 32; ++u) h[l][u] = ppo_tanh(z[u]);
    }
  }
  const float* q = net + ppo_layer_off(D, L);
  if (L == 1) stage_units(h[0], S, lane);
  else if (L == 2) stage_units(h[1], S, lane);
  else stage_units(h[2], S, lane);
#pragma unroll
  for (int u = 0; u < 32; ++u) out[u] = q[1024 + u];
  layer_acc(q, S, 32, lane, out);
}

// the second block of the head of 2 A rows (NET_LS): ls = the lane's 32 padded log stds, one more layer_acc over the hidden
// column that net_forward left in S (the lane's own column: no barrier between the two)
__device__ __forceinline__ void head_log_std(const float* net, int D, int L, const float* S, int lane, float (&ls)[32]) {
  const float* q = net + ppo_layer_off(D, L) + 1056;
#pragma unroll
  for (int u = 0; u < 32; ++u) ls[u] = q[1024 + u];
  layer_acc(q, S, 32, lane, ls);
}

// log-probability of the lane's action row under the Gaussian head (train_vec.GaussianPolicy.logp_value): zc = the
// standardised actions, inv_std = exp(-log_std) is not used: the division is the reference's.  log_std [c]: the free
// parameter in memory, or (NET_LS) the lane's registers
template <typename LS>
__device__ __forceinline__ float ppo_logp(const float (&mu)[32], const float (&a)[32], const LS& log_std, int A,
                                          float (&zc)[32], float (&sd)[32]) {
  float logp = 0.0f;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    zc[c] = 0.0f;
    sd[c] = 1.0f;
    if (c < A) {
      const float ls = log_std[c];
      sd[c] = expf(ls);
      zc[c] = (a[c] - mu[c]) / sd[c];
      logp += (-0.5f * (zc[c] * zc[c]) - ls) - 0.9189385f;
    }
  }
  return logp;
}

// the lane's action row; returns false when it holds a NaN (an absent agent: the row is replaced by zeros)
__device__ __forceinline__ bool ppo_load_act(const float* act, long long s, bool valid, int A, float (&a)[32]) {
  bool present = true;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    a[c] = 0.0f;
    if (c < A && valid) a[c] = act[size_t(s) * size_t(A) + size_t(c)];
    present = present && a[c] == a[c];
  }
  if (!present) {
#pragma unroll
    for (int c = 0; c < 32; ++c) a[c] = 0.0f;
  }
  return present;
}

// DIST: the head's means go out as well, mean_out [n, A] (the old distribution of the KL penalty)
// NET_LS (act != NULL): the head of 2 A rows; DIST then writes mean_out [n, 2A], a row's A means and then its A log stds
template <bool DIST, bool NET_LS = false>
__global__ __launch_bounds__(64) void k_ppo_eval(PpoView m, long long n, const float* __restrict__ obs,
                                                 const float* __restrict__ act, float* __restrict__ logp_out,
                                                 float* __restrict__ val_out, float* __restrict__ mean_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pnet = reinterpret_cast<float*>(smem);
  float* vnet = pnet + ppo_net_lds(m.D, m.L) + (NET_LS ? 1056 : 0);
  float* S = vnet + ppo_net_lds(m.D, m.L);
  const int lane = threadIdx.x;
  if (act != nullptr) net_load<NET_LS>(m.pw, m.D, m.L, m.A, pnet, lane);
  net_load(m.vw, m.D, m.L, 1, vnet, lane);
  __syncthreads();
  const long long tiles = (n + PPO_TILE - 1) / PPO_TILE;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long s0 = t * PPO_TILE, s = s0 + lane;
    const bool valid = s < n;
    float h[3][32], out[32];
    if (act != nullptr) {
      float a[32], zc[32], sd[32];
      ppo_load_act(act, s, valid, m.A, a);
      net_forward(pnet, m.D, m.L, obs, s0, n, ~0ull, S, lane, h, out);
      if constexpr (NET_LS) {
        float ls[32];
        head_log_std(pnet, m.D, m.L, S, lane, ls);
        const float lp = ppo_logp(out, a, ls, m.A, zc, sd);
        if (valid) logp_out[s] = lp;
        if (DIST && valid) {
          float* row = mean_out + size_t(s) * size_t(2 * m.A);
#pragma unroll
          for (int c = 0; c < 32; ++c) {
            if (c < m.A) {
              row[c] = out[c];
              row[m.A + c] = ls[c];
            }
          }
        }
      } else {
        const float lp = ppo_logp(out, a, m.log_std, m.A, zc, sd);
        if (valid) logp_out[s] = lp;
        if (DIST && valid) {
#pragma unroll
          for (int c = 0; c < 32; ++c)
            if (c < m.A) mean_out[size_t(s) * size_t(m.A) + size_t(c)] = out[c];
        }
      }
    }
    net_forward(vnet, m.D, m.L, obs, s0, n, ~0ull, S, lane, h, out);
    if (valid) val_out[s] = out[0];
  }
}

// one lane per replica: adv, ret [K, R] of rew, val, done [K, R] and last_val [R].  The float32 operation sequence is the
// one CPU torch runs for train_vec.gae (no contraction: -ffp-contract=off), g = float32(gamma), gl = float32(gamma * lam)
__global__ __launch_bounds__(256) void k_gae(int K, long long R, const float* __restrict__ rew, const float* __restrict__ val,
                                             const float* __restrict__ last_val, const uint8_t* __restrict__ done, float g,
                                             float gl, float* __restrict__ adv, float* __restrict__ ret) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float run = 0.0f, nxt = last_val[r];
  for (int t = K - 1; t >= 0; --t) {
    const size_t e = size_t(t) * size_t(R) + size_t(r);
    const float live = done[e] == 0 ? 1.0f : 0.0f, v = val[e];
    const float delta = (rew[e] + (g * nxt) * live) - v;
    run = delta + ((gl * live) * run);
    adv[e] = run;
    ret[e] = run + v;
    nxt = v;
  }
}

// G[u][col0 + i] += sum_s T[s][u] S[i][s] for u < 32, i < n_in (rows u >= n_out and columns i >= n_in are not written): lane
// = (input i = lane mod 32, units 16 (lane / 32) ..+16), s ascending
__device__ __forceinline__ void grad_block(const float* T, const float* S, int n_in, int n_out, float* G, int ld, int col0,
                                           int lane) {
  const int i = lane & 31, u0 = (lane >> 5) * 16;
  float acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
  for (int s = 0; s < PPO_TILE; ++s) {
    const float x = S[i * PPO_TS + s];
    const float4* d4 = reinterpret_cast<const float4*>(T + s * PPO_TT + u0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 d = d4[q];
      acc[4 * q + 0] = __builtin_fmaf(d.x, x, acc[4 * q + 0]);
      acc[4 * q + 1] = __builtin_fmaf(d.y, x, acc[4 * q + 1]);
      acc[4 * q + 2] = __builtin_fmaf(d.z, x, acc[4 * q + 2]);
      acc[4 * q + 3] = __builtin_fmaf(d.w, x, acc[4 * q + 3]);
    }
  }
  if (i < n_in) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (u0 + k < n_out) G[(u0 + k) * ld + col0 + i] += acc[k];
  }
}

// G[u] += sum_s T[s][u], s ascending, u < n_out <= 32
__device__ __forceinline__ void col_sum(const float* T, int n_out, float* G, int lane) {
  if (lane < n_out) {
    float acc = 0.0f;
    for (int s = 0; s < PPO_TILE; ++s) acc += T[s * PPO_TT + lane];
    G[lane] += acc;
  }
}

__device__ __forceinline__ void stage_dz(const float (&dz)[32], float* T, int lane) {
  float4* t4 = reinterpret_cast<float4*>(T + lane * PPO_TT);
#pragma unroll
  for (int q = 0; q < 8; ++q) t4[q] = make_float4(dz[4 * q], dz[4 * q + 1], dz[4 * q + 2], dz[4 * q + 3]);
}

// sum_u Wt[i][u] dz[u] of one block of 32 units (q: the layer's LDS copy): four strided partial sums, (a0 + a1) + (a2 + a3)
__device__ __forceinline__ float back_dot(const float* q, int i, const float (&dz)[32]) {
  const float4* w4 = reinterpret_cast<const float4*>(q + i * 32);
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 w = w4[k];
    a0 = __builtin_fmaf(w.x, dz[4 * k + 0], a0);
    a1 = __builtin_fmaf(w.y, dz[4 * k + 1], a1);
    a2 = __builtin_fmaf(w.z, dz[4 * k + 2], a2);
    a3 = __builtin_fmaf(w.w, dz[4 * k + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// (NET_LS) what the backward pass takes on top of dz: the loss's gradient at the 32 padded log-std outputs of the head
struct PpoNoLs {};
template <bool NET_LS>
struct PpoLsOf { typedef PpoNoLs type; };
template <>
struct PpoLsOf<true> { typedef float type[32]; };

// one layer of the backward pass (LYR = 1 .. L; the head when LYR == L): its weight and bias gradients from dz and its input
// h[LYR-1], then dz of the layer below: (Wt dz) (1 - h^2), through the lane's own column of S.
// NET_LS, at the head (n_out = A rows per block): block 0 (rows 0 .. A-1 of the packed head, bias 2A 32 ..) from dz exactly
// as above, then block 1 (rows A .. 2A-1, bias 2A 32 + A ..) from dz1 over the same staged h; the gradient at the last hidden
// layer is (block 0's sum) + (block 1's sum), each sum in back_dot's order
template <int LYR, bool NET_LS = false>
__device__ __forceinline__ void back_layer(const float* net, int D, int L, int n_out, float* S, float* T, int lane,
                                           const float (&h)[3][32], float (&dz)[32], float* G,
                                           const typename PpoLsOf<NET_LS>::type& dz1) {
  const float* q = net + ppo_layer_off(D, LYR);
  const int rows = LYR < L ? 32 : n_out;
  const bool two = NET_LS && LYR == L;
  float* g = G + 32 * D + 32 + (LYR - 1) * 1056;
  stage_units(h[LYR - 1], S, lane);
  stage_dz(dz, T, lane);
  __syncthreads();
  grad_block(T, S, 32, rows, g, 32, 0, lane);
  col_sum(T, rows, g + (two ? 2 * rows : rows) * 32, lane);
  __syncthreads();
  if constexpr (NET_LS) {
    if (two) {
      stage_dz(dz1, T, lane);
      __syncthreads();
      grad_block(T, S, 32, rows, g + rows * 32, 32, 0, lane);
      col_sum(T, rows, g + 2 * rows * 32 + rows, lane);
      __syncthreads();
    }
  }
  for (int i = 0; i < 32; ++i) {
    float back = back_dot(q, i, dz);
    if constexpr (NET_LS) {
      if (two) back += back_dot(q + 1056, i, dz1);
    }
    S[i * PPO_TS + lane] = back;
  }
#pragma unroll
  for (int u = 0; u < 32; ++u) dz[u] = S[u * PPO_TS + lane] * __builtin_fmaf(-h[LYR - 1][u], h[LYR - 1][u], 1.0f);
}

// the backward pass of one network on one tile: dz = the loss's gradient at the head's 32 padded outputs (zero for the
// samples that do not count); G = the network's gradient in LDS (packed layout); NET_LS: dz1, back_layer's
template <bool GATHER = false, bool NET_LS = false>
__device__ __forceinline__ void net_backward(const float* net, int D, int L, int n_out, const float* obs, long long s0,
                                             long long n, unsigned long long keep, float* S, float* T, int lane,
                                             const float (&h)[3][32], float (&dz)[32], float* G,
                                             const typename PpoLsOf<NET_LS>::type& dz1, int row = 0) {
  if (L >= 3) back_layer<3, NET_LS>(net, D, L, n_out, S, T, lane, h, dz, G, dz1);
  if (L >= 2) back_layer<2, NET_LS>(net, D, L, n_out, S, T, lane, h, dz, G, dz1);
  back_layer<1, NET_LS>(net, D, L, n_out, S, T, lane, h, dz, G, dz1);
  // layer 0: the bias, then the weights by chunks of 32 inputs
  stage_dz(dz, T, lane);
  __syncthreads();
  col_sum(T, 32, G + 32 * D, lane);
  for (int c0 = 0; c0 < D; c0 += 32) {
    __syncthreads();
    stage_obs<GATHER>(obs, s0, n, D, c0, keep, S, lane, row);
    __syncthreads();
    grad_block(T, S, D - c0 < 32 ? D - c0 : 32, 32, G, D, c0, lane);
  }
  __syncthreads();
}

// N_DEV: mean_std is {mean, std, n} and the sample count of the whole update comes from it, inv_n = float(1.0 / n) -- the
// bits a host passes as inv_n for the same n -- so that nothing between the statistics and the gradient needs the host
// LOSS (with N_DEV; fs_last_kernel's "k_ppo_grad_loss"): RLlib's PPO loss per present sample,
//   -pg + kl_coef KL(old || new) + vf_coef max((v - ret)^2, (v_c - ret)^2) - entropy_coef H,   all over n
//   KL = sum_c ls - ls_o + (exp(2 ls_o) + (mu_o - mu)^2) / (2 exp(2 ls)) - 0.5,   H = sum_c ls + 0.5 log(2 pi e)
//   v_c = v_o + clamp(v - v_o, -vf_clip, +vf_clip)
// with kl_coef = float(x.kl_state[0]) read from the device.  Every new term is added where its quantities already sit in
// registers, each behind a wave-uniform branch on its argument (a term that is off is not computed: nothing is multiplied
// by zero), and the old means / old value of an absent row are never loaded.  The sums are four: {pg, vfl, KL, H}.
// MB (with LOSS; fs_last_kernel's "k_ppo_minibatch"): ONE minibatch step in one launch.  The tile's 64 rows are
//   perm(seed, epoch, k B + 64 t + lane)
// and every per-row read goes through them (a lane beyond the minibatch's end is a lane beyond n: staged zeros, zero seeds);
// the lane arithmetic runs with inv_n = 1 -- every term is linear in it -- and each workgroup counts its present rows as an
// integer.  A workgroup writes its partial [P + 4] and its count, then draws an integer ticket (k_adv_stats's pattern: an
// agent-scope release before the ticket, an acquire after it); the workgroup that draws the LAST ticket runs the tail
// (mb_tail), every other one exits: nobody ever waits for anybody.
struct PpoNoMb {};
template <bool MB>
struct PpoMbOf { typedef PpoNoMb type; };
template <>
struct PpoMbOf<true> { typedef PpoMbArgs type; };

__device__ __forceinline__ void mb_tail(const PpoMbArgs& mb, float* work, int G, int P, int lane);

// NET_LS (with N_DEV; fs_last_kernel's "..._ls" names): the head of 2 A rows.  The lane's log stds are 32 more registers
// (head_log_std), read where the free form reads m.log_std[c]; the old distribution x.mean_old is [n, 2A] and the old log
// stds are read like the old means, column by column and never for an absent row; the per-sample gradient at the log stds
// is not column-summed into a log_std slot but goes down the network as dz of the head's second block (back_layer).
template <bool N_DEV, bool LOSS = false, bool MB = false, bool NET_LS = false>
__global__ __launch_bounds__(64) void k_ppo_grad(PpoView m, long long n, const float* __restrict__ obs,
                                                 const float* __restrict__ act, const float* __restrict__ logp_old,
                                                 const double* __restrict__ adv, const float* __restrict__ ret,
                                                 const double* __restrict__ mean_std, float lo, float hi, float vf_coef,
                                                 float inv_n, float* __restrict__ work, PpoLossArgs x,
                                                 typename PpoMbOf<MB>::type mb) {
  static_assert(N_DEV || !LOSS, "the full loss reads its sample count from the device");
  static_assert(LOSS || !MB, "the minibatch form is a form of the full loss");
  static_assert(N_DEV || !NET_LS, "the head of 2 A rows is built for the device-n forms");
  constexpr int NS = LOSS ? PPO_LOSS_SUMS : 2;               // loss sums behind the gradient
  if constexpr (!MB) {
    if (N_DEV) inv_n = float(1.0 / mean_std[2]);
  }
  long long mb_begin = 0, mb_end = 0;                        // (MB) the minibatch's positions in the permutation
  [[maybe_unused]] PermKey pk;
  [[maybe_unused]] unsigned cnt = 0;                         // (MB) present rows of this workgroup's tiles
  if constexpr (MB) {
    inv_n = 1.0f;
    pk = perm_key(mb.seed, *mb.epoch, uint32_t(n));
    mb_begin = mb.k * mb.B;
    mb_end = mb_begin + mb.B < n ? mb_begin + mb.B : n;
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = m.D, A = m.A, L = m.L, P = ppo_params(D, A, L, NET_LS);
  float* pnet = reinterpret_cast<float*>(smem);
  float* vnet = pnet + ppo_net_lds(D, L) + (NET_LS ? 1056 : 0);
  float* S = vnet + ppo_net_lds(D, L);
  float* T = S + 32 * PPO_TS;
  float* G = T + PPO_TILE * PPO_TT;                          // [P + NS]: the gradient, then the loss sums
  const int lane = threadIdx.x;
  net_load<NET_LS>(m.pw, D, L, A, pnet, lane);
  net_load(m.vw, D, L, 1, vnet, lane);
  for (int e = lane; e < P + NS; e += 64) G[e] = 0.0f;
  __syncthreads();
  const int Pp = ppo_net_params(D, L, NET_LS ? 2 * A : A);   // the policy's part; the value network's follows (after log_std [A])
  const int Pv = NET_LS ? Pp : Pp + A;
  const double mean = mean_std[0], scale = mean_std[1] + 1e-8;
  const long long tiles = ((MB ? mb_end - mb_begin : n) + PPO_TILE - 1) / PPO_TILE;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    long long s0 = t * PPO_TILE, s = s0 + lane;
    bool valid = s < n;
    int row = 0;                                             // (MB) the lane's row, -1 beyond the minibatch's end
    if constexpr (MB) {
      const long long at = mb_begin + s;
      valid = at < mb_end;
      row = valid ? int(perm_at(pk, uint32_t(valid ? at : 0))) : -1;
      s = row;
    }
    float a[32], h[3][32], out[32], dz[32];
    const bool present = ppo_load_act(act, s, valid, A, a) && valid;
    const unsigned long long keep = __ballot(present);
    if constexpr (MB) cnt += unsigned(__popcll(keep));
    // ---- the policy: logp, the clipped surrogate, its gradient at the means and at log_std
    net_forward<MB>(pnet, D, L, obs, s0, n, keep, S, lane, h, out, row);
    float pg = 0.0f, vf = 0.0f;
    float kl = 0.0f, ent = 0.0f;                             // (LOSS)
    float gls[32];                                           // the loss's gradient at the log stds, per sample
    {
      float zc[32], sd[32];
      [[maybe_unused]] float lsr[32];                        // (NET_LS) the lane's log stds
      float logp;
      if constexpr (NET_LS) {
        head_log_std(pnet, D, L, S, lane, lsr);
        logp = ppo_logp(out, a, lsr, A, zc, sd);
      } else {
        logp = ppo_logp(out, a, m.log_std, A, zc, sd);
      }
      const float adv_n = present ? float((adv[s] - mean) / scale) : 0.0f;
      const float ratio = present ? expf(logp - logp_old[s]) : 1.0f;
      const float clamped = ratio < lo ? lo : ratio > hi ? hi : ratio;
      const float s1 = ratio * adv_n, s2 = clamped * adv_n;
      pg = s1 < s2 ? s1 : s2;
      // d(-pg / n_total) / d logp: the unclipped branch is live inside [lo, hi] (both branches are it) or where it is the smaller
      const bool live = present && ((ratio >= lo && ratio <= hi) || s1 < s2);
      const float g_logp = live ? (-inv_n * adv_n) * ratio : 0.0f;
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        dz[c] = c < A ? g_logp * (zc[c] / sd[c]) : 0.0f;
        gls[c] = c < A ? g_logp * __builtin_fmaf(zc[c], zc[c], -1.0f) : 0.0f;
      }
      if constexpr (LOSS) {
        if (x.kl_state != nullptr) {
          // d KL / d mu = (mu - mu_o) / exp(2 ls);  d KL / d ls = 1 - (exp(2 ls_o) + (mu_o - mu)^2) / exp(2 ls)
          const float w = inv_n * float(x.kl_state[0]);
#pragma unroll
          for (int c = 0; c < 32; ++c) {
            if (c < A) {
              float ls, lso, mo;
              if constexpr (NET_LS) {
                const float* old = x.mean_old + size_t(s) * size_t(2 * A);
                ls = lsr[c];
                lso = present ? old[A + c] : 0.0f;
                mo = present ? old[c] : 0.0f;
              } else {
                ls = m.log_std[c];
                lso = x.log_std_old[c];
                mo = present ? x.mean_old[size_t(s) * size_t(A) + size_t(c)] : 0.0f;
              }
              const float so = expf(lso);
              const float var = sd[c] * sd[c], d = mo - out[c];
              const float q = __builtin_fmaf(d, d, so * so) / var;
              kl += present ? ((ls - lso) + 0.5f * q) - 0.5f : 0.0f;
              dz[c] = present ? __builtin_fmaf(w, -d / var, dz[c]) : dz[c];
              gls[c] = present ? __builtin_fmaf(w, 1.0f - q, gls[c]) : gls[c];
            }
          }
        }
        const bool ent_on = x.entropy_coef != 0.0f;
        const float we = inv_n * x.entropy_coef;
#pragma unroll
        for (int c = 0; c < 32; ++c) {
          if (c < A) {
            float ls;
            if constexpr (NET_LS) ls = lsr[c];
            else ls = m.log_std[c];
            ent += present ? ls + 1.4189385f : 0.0f;                       // 0.5 log(2 pi e)
            if (ent_on) gls[c] = present ? gls[c] - we : gls[c];           // d (-entropy_coef H) / d ls = -entropy_coef
          }
        }
      }
      if constexpr (!NET_LS) {
        __syncthreads();
        stage_dz(gls, T, lane);
        __syncthreads();
        col_sum(T, A, G + Pp, lane);
        __syncthreads();
      }
    }
    if constexpr (NET_LS) net_backward<MB, true>(pnet, D, L, A, obs, s0, n, keep, S, T, lane, h, dz, G, gls, row);
    else net_backward<MB>(pnet, D, L, A, obs, s0, n, keep, S, T, lane, h, dz, G, PpoNoLs{}, row);
    // ---- the value network: (v - ret)^2
    net_forward<MB>(vnet, D, L, obs, s0, n, keep, S, lane, h, out, row);
    {
      const float err = present ? out[0] - ret[s] : 0.0f;
      vf = err * err;
#pragma unroll
      for (int c = 0; c < 32; ++c) dz[c] = 0.0f;
      dz[0] = (vf_coef * inv_n) * (2.0f * err);
      if constexpr (LOSS) {
        if (x.vf_clip > 0.0f) {
          // max((v - ret)^2, (v_c - ret)^2): where the clipped error is the larger one its gradient is the loss's, and that
          // is zero where the clamp cut (v_c does not move with v)
          const float vo = present ? x.val_old[s] : 0.0f;
          const float dv = out[0] - vo;
          const float cl = dv < -x.vf_clip ? -x.vf_clip : dv > x.vf_clip ? x.vf_clip : dv;
          const float err_c = present ? (vo + cl) - ret[s] : 0.0f;
          const float vf_c = err_c * err_c;
          const bool clipped = vf_c > vf;
          dz[0] = clipped ? (cl == dv ? (vf_coef * inv_n) * (2.0f * err_c) : 0.0f) : dz[0];
          vf = clipped ? vf_c : vf;
        }
      }
    }
    net_backward<MB>(vnet, D, L, 1, obs, s0, n, keep, S, T, lane, h, dz, G + Pv, PpoNoLs{}, row);
    // ---- the loss sums
    T[lane * PPO_TT + 0] = pg;
    T[lane * PPO_TT + 1] = vf;
    if constexpr (LOSS) {
      T[lane * PPO_TT + 2] = kl;
      T[lane * PPO_TT + 3] = ent;
    }
    __syncthreads();
    col_sum(T, NS, G + P, lane);
    __syncthreads();
  }
  float* w = work + size_t(blockIdx.x) * size_t(P + NS);
  for (int e = lane; e < P + NS; e += 64) w[e] = G[e];
  if constexpr (MB) {
    const int groups = gridDim.x;
    unsigned* counts = reinterpret_cast<unsigned*>(work + size_t(groups) * size_t(P + NS));
    if (lane == 0) counts[blockIdx.x] = cnt;
    // the wave's stores are out (release, agent scope) before lane 0 draws the ticket; the last workgroup to draw sees every
    // partial (acquire).  Nobody waits: a workgroup that is not last is done.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned drawn = 0;
    if (lane == 0) drawn = __hip_atomic_fetch_add(mb.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    drawn = unsigned(__builtin_amdgcn_readfirstlane(int(drawn)));
    if (drawn != unsigned(groups - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    mb_tail(mb, work, groups, P, lane);
  }
}

// the partial gradients of the G workgroups, summed in ascending order: grad [P], loss [NS] (accumulate: added to what is
// there); NS = 2 loss sums, PPO_LOSS_SUMS for the full-loss form
template <int NS>
__global__ __launch_bounds__(256) void k_ppo_reduce(const float* __restrict__ work, int G, int P, int accumulate,
                                                    float* __restrict__ grad, float* __restrict__ loss) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P + NS) return;
  float acc = work[p];
  for (int g = 1; g < G; ++g) acc += work[size_t(g) * size_t(P + NS) + size_t(p)];
  float* dst = p < P ? grad + p : loss + (p - P);
  *dst = accumulate ? *dst + acc : acc;
}

// ---- the advantage statistics.  G = adv_groups(n) workgroups of ADV_THREADS lanes; lane t of workgroup b adds its rows
// b ADV_THREADS + t + k G ADV_THREADS, k ascending, in double; a workgroup's lanes meet in a binary tree over LDS (lane t +=
// lane t + half, half = 128 .. 1) and lane 0 writes the workgroup's three partial sums to the handle's scratch.  The
// workgroup that arrives last (an integer ticket; agent-scope release before it, acquire after) adds the G partials -- lane
// t those of workgroups t and t + ADV_THREADS, then the same tree -- so the order of every sum depends on n alone, whichever
// workgroup that is, and resets the ticket for the next launch.  A row whose action row holds a NaN is absent: it is selected out of the three sums and its
// adv64 is 0, so nothing it holds reaches an output.
__global__ __launch_bounds__(ADV_THREADS) void k_adv_stats(long long n, const float* __restrict__ adv,
                                                           const float* __restrict__ act, int A, int accumulate,
                                                           double* __restrict__ adv64, double* __restrict__ stats,
                                                           double* scratch) {
  __shared__ double red[3][ADV_THREADS];
  const int t = threadIdx.x, G = gridDim.x;
  double s0 = 0.0, s1 = 0.0, cnt = 0.0;
  for (long long i = (long long)blockIdx.x * ADV_THREADS + t; i < n; i += (long long)G * ADV_THREADS) {
    bool present = true;
    if (act != nullptr) {
      const float* row = act + size_t(i) * size_t(A);
      for (int c = 0; c < A; ++c) present = present && row[c] == row[c];
    }
    const double a = present ? double(adv[i]) : 0.0;
    adv64[i] = a;
    s0 += a;
    s1 += a * a;
    cnt += present ? 1.0 : 0.0;
  }
  red[0][t] = s0;
  red[1][t] = s1;
  red[2][t] = cnt;
  __syncthreads();
  for (int half = ADV_THREADS / 2; half >= 1; half >>= 1) {
    if (t < half) {
      red[0][t] += red[0][t + half];
      red[1][t] += red[1][t + half];
      red[2][t] += red[2][t + half];
    }
    __syncthreads();
  }
  // lane 0 publishes the partial sums and draws a ticket; the workgroup that draws the last one adds all of them up
  unsigned* ticket = reinterpret_cast<unsigned*>(scratch);
  double* part = scratch + 1;
  if (t == 0) {
    for (int k = 0; k < 3; ++k) part[3 * blockIdx.x + k] = red[k][0];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == unsigned(G - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    red[0][1] = last ? 1.0 : 0.0;                            // ("I am last", through the array that is there)
  }
  __syncthreads();
  if (red[0][1] == 0.0) return;
  __syncthreads();                                           // (every lane has read the flag: red is free again)
  // lane t adds the partial sums of workgroups t, t + ADV_THREADS (G <= 2 ADV_THREADS), then the same tree
  s0 = s1 = cnt = 0.0;
  for (int g = t; g < G; g += ADV_THREADS) {
    s0 += part[3 * g + 0];
    s1 += part[3 * g + 1];
    cnt += part[3 * g + 2];
  }
  red[0][t] = s0;
  red[1][t] = s1;
  red[2][t] = cnt;
  __syncthreads();
  for (int half = ADV_THREADS / 2; half >= 1; half >>= 1) {
    if (t < half) {
      red[0][t] += red[0][t + half];
      red[1][t] += red[1][t + half];
      red[2][t] += red[2][t + half];
    }
    __syncthreads();
  }
  if (t < 3) stats[t] = accumulate ? stats[t] + red[t][0] : red[t][0];
  if (t == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the episode statistics {episodes, sum ret, sum ret^2, min ret, max ret, sum len, min len, max len} of a fragment's
// rew / done [K, R].  G = ep_groups(R) workgroups of EP_THREADS lanes; lane t of workgroup b walks replicas
// r = b EP_THREADS + t + j G EP_THREADS, j ascending, each over k = 0 .. K-1 with the replica's carries (run_ret += rew in
// double, run_len += 1; done != 0 emits the episode into the lane's partials -- sums added, min / max combined, in that
// (j, k) order -- and zeroes the carries), and writes the carries back.  Then k_adv_stats's scheme: the lanes of a workgroup meet
// in a binary tree over LDS (lane t (+)= lane t + half, half = 128 .. 1; (+) = add, fmin or fmax per statistic), lane 0
// writes the workgroup's partials and draws an integer ticket, the workgroup that draws the last one combines the G
// partials (lane t those of workgroups t and t + EP_THREADS, then the same tree) and resets the ticket.  The order of
// every sum depends on (K, R) alone.  A lane without an episode contributes {0, 0, 0, +inf, -inf, 0, +inf, -inf}.
__device__ __forceinline__ double ep_combine(int k, double a, double b) {
  return (k == 3 || k == 6) ? fmin(a, b) : (k == 4 || k == 7) ? fmax(a, b) : a + b;
}

__device__ __forceinline__ void ep_tree(double (*red)[EP_THREADS], int t) {
  for (int half = EP_THREADS / 2; half >= 1; half >>= 1) {
    if (t < half) {
#pragma unroll
      for (int k = 0; k < EP_STATS; ++k) red[k][t] = ep_combine(k, red[k][t], red[k][t + half]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(EP_THREADS) void k_episode_stats(int K, long long R, const float* __restrict__ rew,
                                                              const uint8_t* __restrict__ done,
                                                              double* __restrict__ run_ret, int32_t* __restrict__ run_len,
                                                              double* __restrict__ stats, int accumulate, double* scratch) {
  __shared__ double red[EP_STATS][EP_THREADS];
  __shared__ int is_last;
  const int t = threadIdx.x, G = gridDim.x;
  const double inf = __builtin_inf();
  double p[EP_STATS] = {0.0, 0.0, 0.0, inf, -inf, 0.0, inf, -inf};
  for (long long r = (long long)blockIdx.x * EP_THREADS + t; r < R; r += (long long)G * EP_THREADS) {
    double ret = run_ret[r];
    int32_t len = run_len[r];
    // (EP_AHEAD steps' loads in flight together -- the walk is a chain of dependent adds, not of dependent loads --; the
    // loads past K - 1 repeat the last step's address and are not used)
    for (int k0 = 0; k0 < K; k0 += EP_AHEAD) {
      float rw[EP_AHEAD];
      uint8_t dn[EP_AHEAD];
#pragma unroll
      for (int j = 0; j < EP_AHEAD; ++j) {
        const int k = k0 + j < K ? k0 + j : K - 1;
        const size_t i = size_t(k) * size_t(R) + size_t(r);
        rw[j] = rew[i];
        dn[j] = done[i];
      }
#pragma unroll
      for (int j = 0; j < EP_AHEAD; ++j) {
        if (k0 + j < K) {
          ret += double(rw[j]);
          len += 1;
          if (dn[j] != 0) {
            const double l = double(len);
            p[0] += 1.0;
            p[1] += ret;
            p[2] += ret * ret;
            p[3] = fmin(p[3], ret);
            p[4] = fmax(p[4], ret);
            p[5] += l;
            p[6] = fmin(p[6], l);
            p[7] = fmax(p[7], l);
            ret = 0.0;
            len = 0;
          }
        }
      }
    }
    run_ret[r] = ret;
    run_len[r] = len;
  }
#pragma unroll
  for (int k = 0; k < EP_STATS; ++k) red[k][t] = p[k];
  __syncthreads();
  ep_tree(red, t);
  unsigned* ticket = reinterpret_cast<unsigned*>(scratch);
  double* part = scratch + 1;
  if (t == 0) {
    for (int k = 0; k < EP_STATS; ++k) part[EP_STATS * blockIdx.x + k] = red[k][0];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == unsigned(G - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    is_last = last ? 1 : 0;
  }
  __syncthreads();
  if (is_last == 0) return;
  // lane t combines the partials of workgroups t, t + EP_THREADS (G <= 2 EP_THREADS), then the same tree
  double q[EP_STATS] = {0.0, 0.0, 0.0, inf, -inf, 0.0, inf, -inf};
  for (int g = t; g < G; g += EP_THREADS) {
#pragma unroll
    for (int k = 0; k < EP_STATS; ++k) q[k] = ep_combine(k, q[k], part[EP_STATS * g + k]);
  }
#pragma unroll
  for (int k = 0; k < EP_STATS; ++k) red[k][t] = q[k];
  __syncthreads();
  ep_tree(red, t);
  if (t < EP_STATS) stats[t] = accumulate ? ep_combine(t, stats[t], red[t][0]) : red[t][0];
  if (t == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ppo_update's formula, in double (division and square root are correctly rounded; nothing contracts): a NaN variance
// (n = 1) stays a NaN, as torch's clamp_min leaves it
__global__ __launch_bounds__(64) void k_adv_finish(const double* __restrict__ stats, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double s0 = stats[0], s1 = stats[1], n = stats[2];
  const double mean = s0 / n;
  const double var = (s1 - (n * mean) * mean) / (n - 1.0);
  out[0] = mean;
  out[1] = sqrt(var < 0.0 ? 0.0 : var);
  out[2] = n;
}

// RLlib's rule for the KL coefficient, once per update: one thread, in double, nothing contracted.  sums [4] are the loss
// sums of the last epoch's gradient pass (sums[2] = sum KL), mean_std_n[2] the sample count; state = {coef, mean KL of this
// update} lives on the device, so that a replayed graph advances it
__global__ __launch_bounds__(64) void k_kl_adapt(const float* __restrict__ sums, const double* __restrict__ mean_std_n,
                                                 double* state, double kl_target) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double mean_kl = double(sums[2]) / mean_std_n[2];
  double coef = state[0];
  if (mean_kl > 2.0 * kl_target) coef = coef * 1.5;
  else if (mean_kl < 0.5 * kl_target) coef = coef * 0.5;
  state[0] = coef;
  state[1] = mean_kl;
}

// ---- Adam (torch.optim.Adam without weight decay, amsgrad or maximize) on the packed buffers.  state = {t, beta1^t,
// beta2^t} in double, on the device, so that a graph replay advances it.  ONE workgroup: every lane reads the state, the
// barrier follows, then lane 0 alone writes it -- no lane of another workgroup exists that could read the new state for the
// old step.  P is at most ppo_params(160, 32, 3) = 15 649: sixteen elements per lane.
constexpr int ADAM_THREADS = 1024;

// (the operation sequence is written once: k_adam, k_mb_finish and the tail of k_ppo_minibatch run these two)
struct AdamCoef {
  float step, rs, c1, b2, c2, e;
};

// every lane of the ONE workgroup reads the state, the barrier follows, then lane 0 alone writes it
__device__ __forceinline__ AdamCoef adam_advance(double* state, double lr, double beta1, double beta2, double eps, int tid) {
  const double t = state[0] + 1.0, p1 = state[1] * beta1, p2 = state[2] * beta2;
  __syncthreads();
  if (tid == 0) {
    state[0] = t;
    state[1] = p1;
    state[2] = p2;
  }
  return AdamCoef{float(lr / (1.0 - p1)), float(sqrt(1.0 - p2)), float(1.0 - beta1), float(beta2), float(1.0 - beta2),
                  float(eps)};
}

__device__ __forceinline__ void adam_element(const AdamCoef& c, float* w, float gi, float* m, float* v, int i) {
  const float mi = m[i] + (gi - m[i]) * c.c1;
  const float vi = v[i] * c.b2 + (gi * gi) * c.c2;
  m[i] = mi;
  v[i] = vi;
  w[i] = w[i] - c.step * (mi / (sqrtf(vi) / c.rs + c.e));
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam(int P, float* __restrict__ w, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, double* state, double lr,
                                                        double beta1, double beta2, double eps) {
  const AdamCoef c = adam_advance(state, lr, beta1, beta2, eps, threadIdx.x);
  for (int i = threadIdx.x; i < P; i += ADAM_THREADS) adam_element(c, w, g[i], m, v, i);
}

// ---- the end of a minibatch step: the mean's gradient and one Adam step.  grad [P] holds the RAW sums of the step (all
// shards, all ranks), c the count of its present rows.  Exactly
//   g[p] = grad[p] * (float)(1.0 / (double)c);   grad[p] = g[p];   then k_adam's sequence with g
// and with c == 0 nothing at all: no step, Adam's t, m, v and the weights untouched, grad left as it is (exact zeros).
// MB_LAST: the epoch counter advances (whether or not a step was made).  ONE workgroup of NT lanes.
template <int NT>
__device__ __forceinline__ void mb_finish(int P, float* __restrict__ w, float* __restrict__ grad, float* __restrict__ m,
                                          float* __restrict__ v, double* state, double c,
                                          unsigned long long* epoch, int flags, double lr, double beta1, double beta2,
                                          double eps, int tid) {
  if (tid == 0 && (flags & MB_LAST)) *epoch = *epoch + 1ull;
  if (c == 0.0) return;
  const float scale = float(1.0 / c);
  const AdamCoef k = adam_advance(state, lr, beta1, beta2, eps, tid);
#pragma unroll 4
  for (int i = tid; i < P; i += NT) {
    const float g = grad[i] * scale;
    grad[i] = g;
    adam_element(k, w, g, m, v, i);
  }
}

__global__ __launch_bounds__(ADAM_THREADS) void k_mb_finish(int P, float* w, float* grad, float* m, float* v, double* state,
                                                             const double* count, unsigned long long* epoch, int flags,
                                                             double lr, double beta1, double beta2, double eps) {
  mb_finish<ADAM_THREADS>(P, w, grad, m, v, state, count[0], epoch, flags, lr, beta1, beta2, eps, threadIdx.x);
}

// the tail of k_ppo_minibatch: ONE wave, the workgroup that drew the last ticket.  The G partials are added in ascending
// workgroup order (k_ppo_reduce's order; lane l takes elements l, l + 64, ..), the G counts as integers.  The raw sums go to
// grad (MB_ACCUMULATE: are added to it) and to loss_sums (added unless this is the epoch's first minibatch of the first
// shard: MB_FIRST without MB_ACCUMULATE overwrites).  MB_PARTIAL ends there, with the count in count[0]; MB_STEP goes on to
// mb_finish -- each lane re-reads the elements it wrote itself.  Writing the weights here is safe: every other workgroup
// finished net_load (and read the epoch counter) long before it wrote its partial, and that came before its ticket.
__device__ __forceinline__ void mb_tail(const PpoMbArgs& mb, float* work, int G, int P, int lane) {
  constexpr int NS = PPO_LOSS_SUMS;
  const unsigned* counts = reinterpret_cast<const unsigned*>(work + size_t(G) * size_t(P + NS));
  unsigned c = 0;
  for (int g = 0; g < G; ++g) c += counts[g];
  const bool acc = (mb.flags & MB_ACCUMULATE) != 0, add_sums = acc || (mb.flags & MB_FIRST) == 0;
  // (one wave has to keep many loads in flight to get through G (P + 4) floats: a lane carries four elements and loads
  // eight workgroups' values of each before it adds them -- in ascending workgroup order, element by element)
  const int W = P + NS;
  for (int p0 = lane; p0 < W; p0 += 256) {
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = p0 + 64 * j < W ? work[p0 + 64 * j] : 0.0f;
    int g = 1;
    for (; g + 8 <= G; g += 8) {
      float x[8][4];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) x[u][j] = p0 + 64 * j < W ? work[size_t(g + u) * size_t(W) + size_t(p0 + 64 * j)] : 0.0f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += x[u][j];
    }
    for (; g < G; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += p0 + 64 * j < W ? work[size_t(g) * size_t(W) + size_t(p0 + 64 * j)] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + 64 * j;
      if (p < P) {
        mb.grad[p] = acc ? mb.grad[p] + a[j] : a[j];
      } else if (p < W) {
        float* dst = mb.loss_sums + (p - P);
        *dst = add_sums ? *dst + a[j] : a[j];
      }
    }
  }
  if (lane == 0) __hip_atomic_store(mb.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (mb.mode == MB_PARTIAL) {
    if (lane == 0) mb.count[0] = acc ? mb.count[0] + double(c) : double(c);
    return;
  }
  mb_finish<64>(P, mb.w, mb.grad, mb.m, mb.v, mb.state, double(c), mb.epoch, mb.flags, mb.lr, mb.beta1, mb.beta2, mb.eps, lane);
}

}  // namespace fs

namespace fsim {

// the kernels' dynamic LDS may exceed the default limit of a launch: raise it once per process and device
inline int ppo_lds_limit() {
  static thread_local int done_dev = -1;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (done_dev == dev) return FS_OK;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_eval<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_eval<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<true, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              fs::PPO_LDS_BYTES));
  // the head of 2 A rows (NET_LS)
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_eval<false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_eval<true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<true, false, false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<true, true, false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&fs::k_ppo_grad<true, true, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fs::PPO_LDS_BYTES));
  done_dev = dev;
  return FS_OK;
}

template <bool DIST>
static int launch_ppo_eval_any(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act,
                               float* logp, float* val, float* mean_old) {
  if (int rc = ppo_lds_limit()) return rc;
  const long long tiles = (n + fs::PPO_TILE - 1) / fs::PPO_TILE;
  const int grid = int(tiles < 1024 ? tiles : 1024);
  if (fsim::ppo_net_ls(m) && act != nullptr)                 // (values alone, act == NULL: the policy is not read)
    hipLaunchKernelGGL((fs::k_ppo_eval<DIST, true>), dim3(grid), dim3(64), fs::ppo_eval_lds(m.D, m.L, true), stream, m, n, obs,
                       act, logp, val, mean_old);
  else
    hipLaunchKernelGGL(fs::k_ppo_eval<DIST>, dim3(grid), dim3(64), fs::ppo_eval_lds(m.D, m.L), stream, m, n, obs, act, logp,
                       val, mean_old);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_ppo_eval(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act, float* logp,
                    float* val) {
  return launch_ppo_eval_any<false>(stream, m, n, obs, act, logp, val, nullptr);
}

int launch_ppo_eval_dist(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act, float* logp,
                         float* val, float* mean_old) {
  return launch_ppo_eval_any<true>(stream, m, n, obs, act, logp, val, mean_old);
}

int launch_gae(hipStream_t stream, int K, long long R, const float* rew, const float* val, const float* last_val,
               const uint8_t* done, float g, float gl, float* adv, float* ret) {
  hipLaunchKernelGGL(fs::k_gae, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, K, R, rew, val, last_val, done, g, gl,
                     adv, ret);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

// the two forms of the gradient launch: inv_n from the host, or n from the device (mean_std [3]); the head of 2 A rows
// (m.log_std == NULL) is built for the second alone
template <bool N_DEV>
static int launch_ppo_grad_any(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act,
                               const float* logp_old, const double* adv, const float* ret, const double* mean_std, float lo,
                               float hi, float vf_coef, float inv_n, int accumulate, float* grad, float* loss, float* work) {
  if (int rc = ppo_lds_limit()) return rc;
  const bool ls = N_DEV && fsim::ppo_net_ls(m);
  const int G = fs::ppo_groups(n, m.D, m.A, m.L, ls), P = fs::ppo_params(m.D, m.A, m.L, ls);
  if constexpr (N_DEV) {
    if (ls)
      hipLaunchKernelGGL((fs::k_ppo_grad<true, false, false, true>), dim3(G), dim3(64), fs::ppo_grad_lds(m.D, m.A, m.L, true),
                         stream, m, n, obs, act, logp_old, adv, ret, mean_std, lo, hi, vf_coef, inv_n, work, fs::PpoLossArgs{},
                         fs::PpoNoMb{});
  }
  if (!ls)
    hipLaunchKernelGGL(fs::k_ppo_grad<N_DEV>, dim3(G), dim3(64), fs::ppo_grad_lds(m.D, m.A, m.L), stream, m, n, obs, act,
                       logp_old, adv, ret, mean_std, lo, hi, vf_coef, inv_n, work, fs::PpoLossArgs{}, fs::PpoNoMb{});
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fs::k_ppo_reduce<2>, dim3((P + 2 + 255) / 256), dim3(256), 0, stream, work, G, P, accumulate, grad, loss);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

// the full-loss form: the workgroups of the plain form (ppo_groups), four loss sums
int launch_ppo_grad_loss(hipStream_t stream, const fs::PpoView& m, const fs::PpoLossArgs& x, long long n, const float* obs,
                         const float* act, const float* logp_old, const double* adv, const float* ret, const double* mean_std_n,
                         float lo, float hi, float vf_coef, int accumulate, float* grad, float* loss, float* work) {
  if (int rc = ppo_lds_limit()) return rc;
  constexpr int NS = fs::PPO_LOSS_SUMS;
  const bool ls = fsim::ppo_net_ls(m);
  const int G = fs::ppo_groups(n, m.D, m.A, m.L, ls), P = fs::ppo_params(m.D, m.A, m.L, ls);
  if (ls)
    hipLaunchKernelGGL((fs::k_ppo_grad<true, true, false, true>), dim3(G), dim3(64), fs::ppo_grad_loss_lds(m.D, m.A, m.L, true),
                       stream, m, n, obs, act, logp_old, adv, ret, mean_std_n, lo, hi, vf_coef, 0.0f, work, x, fs::PpoNoMb{});
  else
    hipLaunchKernelGGL((fs::k_ppo_grad<true, true>), dim3(G), dim3(64), fs::ppo_grad_loss_lds(m.D, m.A, m.L), stream, m, n, obs,
                       act, logp_old, adv, ret, mean_std_n, lo, hi, vf_coef, 0.0f, work, x, fs::PpoNoMb{});
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fs::k_ppo_reduce<NS>, dim3((P + NS + 255) / 256), dim3(256), 0, stream, work, G, P, accumulate, grad, loss);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

// one minibatch step: the full-loss form's arguments and mb (work: ppo_mb_work_floats(mb.B, ..) words).  The LDS is the
// full-loss form's, under its static_assert
int launch_ppo_minibatch(hipStream_t stream, const fs::PpoView& m, const fs::PpoLossArgs& x, const fs::PpoMbArgs& mb, long long n,
                         const float* obs, const float* act, const float* logp_old, const double* adv, const float* ret,
                         const double* mean_std_n, float lo, float hi, float vf_coef, float* work) {
  if (int rc = ppo_lds_limit()) return rc;
  const bool ls = fsim::ppo_net_ls(m);
  const int G = fs::ppo_mb_groups(mb.B, m.D, m.A, m.L, ls);
  if (ls)
    hipLaunchKernelGGL((fs::k_ppo_grad<true, true, true, true>), dim3(G), dim3(64), fs::ppo_grad_loss_lds(m.D, m.A, m.L, true),
                       stream, m, n, obs, act, logp_old, adv, ret, mean_std_n, lo, hi, vf_coef, 0.0f, work, x, mb);
  else
    hipLaunchKernelGGL((fs::k_ppo_grad<true, true, true>), dim3(G), dim3(64), fs::ppo_grad_loss_lds(m.D, m.A, m.L), stream, m, n,
                       obs, act, logp_old, adv, ret, mean_std_n, lo, hi, vf_coef, 0.0f, work, x, mb);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_mb_finish(hipStream_t stream, int P, float* w, float* grad, float* m, float* v, double* state, const double* count,
                     unsigned long long* epoch, int flags, double lr, double beta1, double beta2, double eps) {
  hipLaunchKernelGGL(fs::k_mb_finish, dim3(1), dim3(fs::ADAM_THREADS), 0, stream, P, w, grad, m, v, state, count, epoch, flags,
                     lr, beta1, beta2, eps);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_kl_adapt(hipStream_t stream, const float* loss_sums, const double* mean_std_n, double* kl_state, double kl_target) {
  hipLaunchKernelGGL(fs::k_kl_adapt, dim3(1), dim3(64), 0, stream, loss_sums, mean_std_n, kl_state, kl_target);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_ppo_grad(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act,
                    const float* logp_old, const double* adv, const float* ret, const double* mean_std, float lo, float hi,
                    float vf_coef, float inv_n, int accumulate, float* grad, float* loss, float* work) {
  return launch_ppo_grad_any<false>(stream, m, n, obs, act, logp_old, adv, ret, mean_std, lo, hi, vf_coef, inv_n, accumulate,
                                    grad, loss, work);
}

int launch_ppo_grad_n(hipStream_t stream, const fs::PpoView& m, long long n, const float* obs, const float* act,
                      const float* logp_old, const double* adv, const float* ret, const double* mean_std_n, float lo, float hi,
                      float vf_coef, int accumulate, float* grad, float* loss, float* work) {
  return launch_ppo_grad_any<true>(stream, m, n, obs, act, logp_old, adv, ret, mean_std_n, lo, hi, vf_coef, 0.0f, accumulate,
                                   grad, loss, work);
}

int launch_adv_stats(hipStream_t stream, long long n, const float* adv, const float* act, int A, int accumulate, double* adv64,
                     double* stats, double* scratch) {
  hipLaunchKernelGGL(fs::k_adv_stats, dim3(fs::adv_groups(n)), dim3(fs::ADV_THREADS), 0, stream, n, adv, act, A, accumulate,
                     adv64, stats, scratch);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_episode_stats(hipStream_t stream, int K, long long R, const float* rew, const uint8_t* done, double* run_ret,
                         int32_t* run_len, double* stats, int accumulate, double* scratch) {
  hipLaunchKernelGGL(fs::k_episode_stats, dim3(fs::ep_groups(R)), dim3(fs::EP_THREADS), 0, stream, K, R, rew, done, run_ret,
                     run_len, stats, accumulate, scratch);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_adv_finish(hipStream_t stream, const double* stats, double* mean_std_n) {
  hipLaunchKernelGGL(fs::k_adv_finish, dim3(1), dim3(64), 0, stream, stats, mean_std_n);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

int launch_adam(hipStream_t stream, int P, float* w, const float* g, float* m, float* v, double* state, double lr, double beta1,
                double beta2, double eps) {
  hipLaunchKernelGGL(fs::k_adam, dim3(1), dim3(fs::ADAM_THREADS), 0, stream, P, w, g, m, v, state, lr, beta1, beta2, eps);
  HIP_TRY(hipGetLastError());
  return FS_OK;
}

}  // namespace fsim
#endif  // FS_PART_LEARN
