// flowsim_policy.h -- the closed loop in ONE kernel: policy -> action -> Env.step, K times, for the reference's RL ring
// experiment (examples/train.py:110-212 is what it replaces: one Python call + socket round trips per step and
// environment; examples/exp_configs/rl/singleagent/singleagent_ring.py: 21 IDM + 1 RL vehicle, WaveAttenuationPOEnv).
//
// What a learner gets per fragment: obs [K+1, R, 3], actions [K, R, 1], log-probabilities [K, R], rewards, done flags --
// the rollout batch of a policy-gradient method -- with the state of a replica in registers for the whole fragment and the
// policy evaluated where the observation is produced.  The policy is the reference's default model class: a fully
// connected network of up to three hidden layers of 32 tanh units (examples/train.py:152 `fcnet_hiddens [32, 32, 32]`)
// with a diagonal Gaussian head -- either two outputs (mean, log std: RLlib's default) or one output and a free log std.
//
// Mapping: the simulator's (k_ring_pair, flowsim_ringrl.h): a row of 16 lanes = one replica, four replicas per wave.
// Lane j of a row holds hidden units j and j + 16; a layer's inputs are fetched from the row with DPP row broadcasts
// (folded into the FMAs), its weights are read from an LDS copy (16 b128 reads per lane and layer), the two outputs are
// reduced over the row with the xor-tree of seg_sum.  The sampled action uses the replica's own Philox stream (keyed by
// the policy's seed, the global replica index and a per-replica counter that a fragment continues where the last one
// stopped).
//
// The network is written ONCE: policy_layer is the 32-input layer, policy_trunk the layer sequence (narrow or WIDE first
// layer, then the hidden layers), policy_load_trunk its weights' way into LDS.  All twelve kernels that evaluate a policy
// call that trunk -- the eager k_policy_act, k_policy_act_vec, k_policy_act_wide and k_policy_act_row (fs_policy_act_dev;
// the third with a first layer of more than 32 inputs, policy_wide_layer1, which is policy_layer over chunks), the fused
// k_ring_policy, k_loop_policy, k_loop_policy_vec, k_merge_queue<POLICY>, k_merge_policy and k_merge_wide_policy
// (flowsim_queue.h), and the two-policy pair k_policy_pair_act / k_loop_policy_pair (fs_policy_pair_*: two networks on one
// RL vehicle) -- through policy_eval (the trunk and the two-output Gaussian head), policy_vec_act (the trunk and the
// action-vector head, a wave per replica), policy_row_vec_act (that head with a row of 16 lanes per replica) or
// policy_wide_act (the same head behind a first layer of more than 32 inputs), so a fragment is bit-identical to
// eager stepping by construction (tests/test_policy_gpu.py and its siblings).  Every operation is an explicit fma /
// hardware exp2 / rcp: the arithmetic is defined by this file (a torch module with the same weights agrees to ~1e-6, not
// bit for bit) and its float32 bits are pinned by tests/test_policy_bits_gpu.py.
#pragma once
#include "flowsim_ringrl.h"

namespace fs {

struct PolicyView {
  const float* w;          // device: per layer W [out][in] row-major, then b [out]
  const float* log_std;    // device [1], or NULL: the network's second output is the log std
  uint32_t* ctr;           // device [R]: actions sampled so far per replica (the draw counter of the policy's stream)
  int in_dim, num_hidden, n_out;
  uint32_t seed_lo, seed_hi;
  int greedy;              // fs_policy.greedy: policy_sample applies the mean (the draw is still made: the streams advance)
  // fs_population (0, 0: one weight set): the workgroup whose first replica is r0 loads the set at w + (r0 / pop_group) *
  // pop_stride.  Read once, by policy_load_trunk, before the first barrier of the launch; nothing behind the load sees it.
  long long pop_stride = 0;
  int pop_group = 0;
};

struct alignas(16) PolicyLds {
  // hidden layers 2 and 3: [layer][quad q][lane j][4] = (W[j][2q], W[j+16][2q], W[j][2q+1], W[j+16][2q+1]) -- a packed FMA per
  // input, and the 16 lanes of a row read 256 consecutive bytes per quad (a per-lane row of 256 B would put all of them on
  // the same LDS banks: a 16-way conflict on every read, measured 1.4 -> 0.9 G)
  float w_hid[2][16][16][4];
  float w_in[32][4];       // layer 1: [unit][input (3, padded)]
  // layer 1 of a WIDE observation (in_dim <= 32, e.g. AccelEnv's speeds and positions; half = ceil(in_dim / 2)): input
  // i < half is the first value of lane i, input half + i < in_dim its second value -- the layout and the summation order
  // of a hidden layer (an odd in_dim leaves the second value of lane half - 1 at zero)
  float w_wide[16][16][4];
  float b[3][32];
  float w_out[2][32];
  float b_out[2];
  float obs[4][4][4];      // [wave of the block][row][value]: the observation of a replica, handed from its RL lane to the row
};

// THE layout of a WIDE observation (in_dim > 4): lane j < half of a row holds inputs j and half + j (the latter if
// < in_dim, else zero), every other lane zeros.  policy_wide_inputs reads it from a row of in_dim values in memory; the
// fused kernels that hold the values in registers gather them into the same places.
__host__ __device__ constexpr int policy_half(int in_dim) { return (in_dim + 1) >> 1; }

__device__ __forceinline__ void policy_wide_inputs(const float* o, int in_dim, int j, float& ia, float& ib) {
  const int half = policy_half(in_dim);
  ia = j < half ? o[j < half ? j : 0] : 0.0f;               // (the loads unconditional, at a valid index)
  ib = (j < half && half + j < in_dim) ? o[half + j < in_dim ? half + j : 0] : 0.0f;
}

// weights -> LDS (once per launch); layout of pv.w: [W1 32 x in_dim][b1 32][W2 32x32][b2][W3 32x32][b3][Wout n_out x 32][bout].
// policy_load_trunk: layers 1 .. num_hidden and their biases; returns where the output layer starts.  No barrier: the
// caller loads its output layer and ends with ONE __syncthreads.
// The weight set of THIS workgroup (fs_population): every kernel that takes a population -- k_policy_act, k_ring_policy,
// k_loop_policy -- gives a row of 16 lanes to a replica, so a workgroup's first replica is blockIdx.x * (blockDim.x / 16)
// and its replicas are one member's (Sim::launch_population: pop_group is a multiple of the 16 replicas of a workgroup).
__device__ __forceinline__ const float* policy_member_weights(const PolicyView& pv) {
  if (pv.pop_stride == 0) return pv.w;                       // (uniform: one set, or all members share set 0)
  const unsigned r0 = blockIdx.x * (blockDim.x >> 4);
  return pv.w + size_t(r0 / unsigned(pv.pop_group)) * size_t(pv.pop_stride);
}

__device__ __forceinline__ const float* policy_load_trunk(const PolicyView& pv, PolicyLds* L, int tid, int nthreads) {
  const float* p = policy_member_weights(pv);
  const bool wide = pv.in_dim > 4;
  for (int e = tid; e < 32 * 4; e += nthreads) L->w_in[e / 4][e % 4] = (!wide && (e % 4) < pv.in_dim) ? p[(e / 4) * pv.in_dim + (e % 4)] : 0.0f;
  {
    const int half = policy_half(pv.in_dim);
    for (int e = tid; e < 32 * 32; e += nthreads) {
      const int u = e / 32, ip = e % 32;                       // ip: place of the input in the hidden-layer order
      const int i = ip < 16 ? ip : half + (ip - 16);           // ... and its index in the observation
      const bool used = wide && (ip & 15) < half && i < pv.in_dim;
      L->w_wide[ip >> 1][u & 15][(ip & 1) * 2 + (u >> 4)] = used ? p[u * pv.in_dim + i] : 0.0f;
    }
  }
  p += 32 * pv.in_dim;
  for (int e = tid; e < 32; e += nthreads) L->b[0][e] = p[e];
  p += 32;
  for (int l = 0; l < 2; ++l) {
    const bool have = l + 1 < pv.num_hidden;
    for (int e = tid; e < 32 * 32; e += nthreads) {
      const int u = e / 32, i = e % 32;
      L->w_hid[l][i >> 1][u & 15][(i & 1) * 2 + (u >> 4)] = have ? p[e] : 0.0f;
    }
    if (have) p += 32 * 32;
    for (int e = tid; e < 32; e += nthreads) L->b[l + 1][e] = have ? p[e] : 0.0f;
    if (have) p += 32;
  }
  return p;
}

// the trunk and the Gaussian head of n_out <= 2 rows (mean [, log std])
__device__ __forceinline__ void policy_load(const PolicyView& pv, PolicyLds* L, int tid, int nthreads) {
  const float* p = policy_load_trunk(pv, L, tid, nthreads);
  for (int e = tid; e < 2 * 32; e += nthreads) L->w_out[e / 32][e % 32] = (e / 32) < pv.n_out ? p[e] : 0.0f;
  p += pv.n_out * 32;
  if (tid < 2) L->b_out[tid] = tid < pv.n_out ? p[tid] : 0.0f;
  __syncthreads();
}

// (a, b, c) of lanes (k, k + D1, k + D2) mod 16 of every 16-lane row -> all lanes of the row (k wave-uniform): three DPP
// row broadcasts behind ONE jump on k, where three ds_bpermute would be an LDS round trip the wave waits out (nothing
// else to issue: the policy's first layer needs the three values).  <1, 2>: a lane and its two neighbours; <0, 0>: the
// same lane three times.
template <int D1, int D2>
__device__ __forceinline__ void row_bcast(int k, float a, float b, float c, float& oa, float& ob, float& oc) {
#define FS_RB(K_) case K_: oa = dpp<DPP_ROW_NEWBCAST0 + K_>(a); ob = dpp<DPP_ROW_NEWBCAST0 + ((K_ + D1) & 15)>(b); \
                          oc = dpp<DPP_ROW_NEWBCAST0 + ((K_ + D2) & 15)>(c); break;
  switch (k & 15) {
    FS_RB(0) FS_RB(1) FS_RB(2) FS_RB(3) FS_RB(4) FS_RB(5) FS_RB(6) FS_RB(7)
    FS_RB(8) FS_RB(9) FS_RB(10) FS_RB(11) FS_RB(12) FS_RB(13) FS_RB(14) FS_RB(15)
  }
#undef FS_RB
}

__device__ __forceinline__ float policy_tanh(float z) {
  const float e = __builtin_amdgcn_exp2f(z * 2.885390081777927f);       // exp(2 z)
  const float r = __builtin_amdgcn_rcpf(e + 1.0f);
  return __builtin_fmaf(-2.0f, r, 1.0f);                                // 1 - 2 / (exp(2 z) + 1)
}

// ONE layer on 32 inputs, the only place it is written: z[u] = b[u] + sum_i W[u][i] in[i] for this lane's units u = j and
// j + 16 (bias b_j, b_j16).  Input i < 16 is `a` of lane i, input i >= 16 `b` of lane i - 16: row broadcasts, folded into
// the packed FMAs.  ww[i / 2] = the weights of inputs i, i + 1 -- all sixteen quads read by the caller first (the LDS
// reads in flight together) --, then four independent accumulators (inputs i with the same i mod 4 share one; the chain
// of dependent packed FMAs is 8 long instead of 32), combined as ((b + z0) + z1) + (z2 + z3).
__device__ __forceinline__ f2 policy_layer(const float4 (&ww)[16], float b_j, float b_j16, float a, float b) {
  f2 z0 = {b_j, b_j16}, z1 = {0.0f, 0.0f}, z2 = {0.0f, 0.0f}, z3 = {0.0f, 0.0f};
  static_for<4>([&](auto q_c) {                    // inputs 4q .. 4q + 3 (`a` of lanes 4q ..) and 16 + 4q .. (`b`)
    constexpr int q = decltype(q_c)::value;
    const float a0 = dpp<DPP_ROW_NEWBCAST0 + 4 * q>(a), a1 = dpp<DPP_ROW_NEWBCAST0 + 4 * q + 1>(a);
    const float a2 = dpp<DPP_ROW_NEWBCAST0 + 4 * q + 2>(a), a3 = dpp<DPP_ROW_NEWBCAST0 + 4 * q + 3>(a);
    const float b0 = dpp<DPP_ROW_NEWBCAST0 + 4 * q>(b), b1 = dpp<DPP_ROW_NEWBCAST0 + 4 * q + 1>(b);
    const float b2 = dpp<DPP_ROW_NEWBCAST0 + 4 * q + 2>(b), b3 = dpp<DPP_ROW_NEWBCAST0 + 4 * q + 3>(b);
    z0 = fma2(f2{ww[2 * q].x, ww[2 * q].y}, splat(a0), z0);
    z1 = fma2(f2{ww[2 * q].z, ww[2 * q].w}, splat(a1), z1);
    z2 = fma2(f2{ww[2 * q + 1].x, ww[2 * q + 1].y}, splat(a2), z2);
    z3 = fma2(f2{ww[2 * q + 1].z, ww[2 * q + 1].w}, splat(a3), z3);
    z0 = fma2(f2{ww[8 + 2 * q].x, ww[8 + 2 * q].y}, splat(b0), z0);
    z1 = fma2(f2{ww[8 + 2 * q].z, ww[8 + 2 * q].w}, splat(b1), z1);
    z2 = fma2(f2{ww[8 + 2 * q + 1].x, ww[8 + 2 * q + 1].y}, splat(b2), z2);
    z3 = fma2(f2{ww[8 + 2 * q + 1].z, ww[8 + 2 * q + 1].w}, splat(b3), z3);
  });
  return pk_add(pk_add(z0, z1), pk_add(z2, z3));
}

// THE trunk, the only place the layer sequence is written: the last hidden layer's units j and j + 16 (ha, hb) for the
// observation of THIS row's replica; j = lane within the row.  Narrow first layer: (o0, o1, o2), the same three values
// in every lane of the row.  WIDE: two values per lane in policy_wide_inputs' layout (o0: input j, o1: input half + j of
// THIS lane; o2 unused) -- a hidden layer's form and summation order.
// PRE (the first layer of MORE than 32 inputs, policy_wide_layer1 below): o0 / o1 are this lane's two first-layer sums,
// bias included; the trunk starts at their tanh.
template <bool WIDE, bool PRE = false>
__device__ __forceinline__ void policy_trunk(const PolicyView& pv, const PolicyLds* L, int j, float o0, float o1, float o2,
                                             float& ha, float& hb) {
  // The first two weight quads of a hidden layer are read one layer AHEAD (before the previous layer's tanh): the layer's
  // FMAs start on them while its other fourteen reads are in flight, instead of waiting out an LDS round trip at the top
  // of every layer.  (All sixteen ahead was measured slower: the 64 registers stay live through tanh and the kernel spills.)
  float4 wa0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), wa1 = wa0;
  auto load_ahead = [&](int l) {
    wa0 = *reinterpret_cast<const float4*>(L->w_hid[l][0][j]);
    wa1 = *reinterpret_cast<const float4*>(L->w_hid[l][1][j]);
  };
  if (pv.num_hidden > 1) load_ahead(0);
  // layer 1
  if constexpr (PRE) {
    ha = policy_tanh(o0);
    hb = policy_tanh(o1);
  } else if constexpr (WIDE) {
    float4 ww[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) ww[q] = *reinterpret_cast<const float4*>(L->w_wide[q][j]);
    const f2 z = policy_layer(ww, L->b[0][j], L->b[0][j + 16], o0, o1);
    ha = policy_tanh(z.x);
    hb = policy_tanh(z.y);
  } else {
    const float4 wa = *reinterpret_cast<const float4*>(L->w_in[j]), wb = *reinterpret_cast<const float4*>(L->w_in[j + 16]);
    float za = L->b[0][j], zb = L->b[0][j + 16];
    za = __builtin_fmaf(wa.x, o0, za); zb = __builtin_fmaf(wb.x, o0, zb);
    za = __builtin_fmaf(wa.y, o1, za); zb = __builtin_fmaf(wb.y, o1, zb);
    za = __builtin_fmaf(wa.z, o2, za); zb = __builtin_fmaf(wb.z, o2, zb);
    ha = policy_tanh(za);
    hb = policy_tanh(zb);
  }
  // hidden layers 2 .. num_hidden: input i < 16 sits in `ha` of lane i, input i >= 16 in `hb` of lane i - 16
#pragma unroll 1
  for (int l = 0; l + 1 < pv.num_hidden; ++l) {
    float4 ww[16];
    ww[0] = wa0;
    ww[1] = wa1;
#pragma unroll
    for (int q = 2; q < 16; ++q) ww[q] = *reinterpret_cast<const float4*>(L->w_hid[l][q][j]);
    const f2 z = policy_layer(ww, L->b[l + 1][j], L->b[l + 1][j + 16], ha, hb);
    if (l + 2 < pv.num_hidden) load_ahead(l + 1);  // (wave-uniform)
    ha = policy_tanh(z.x);
    hb = policy_tanh(z.y);
  }
}

// mean and log std of the action distribution for the observation of THIS row's replica: policy_trunk and the Gaussian
// head of two outputs
template <int ROW, bool WIDE = false>
__device__ __forceinline__ void policy_eval(const PolicyView& pv, const PolicyLds* L, int j, float o0, float o1, float o2,
                                            float& mu, float& log_std) {
  static_assert(ROW == 16, "policy_eval: a row of 16 lanes holds the 32 units of a layer");
  float ha, hb;      // units j and j + 16
  policy_trunk<WIDE>(pv, L, j, o0, o1, o2, ha, hb);
  // head: two outputs, each the row's tree sum of the lanes' two products
  float p0 = L->w_out[0][j] * ha, p1 = L->w_out[1][j] * ha;
  p0 = __builtin_fmaf(L->w_out[0][j + 16], hb, p0);
  p1 = __builtin_fmaf(L->w_out[1][j + 16], hb, p1);
  mu = seg_sum<ROW>(p0) + L->b_out[0];
  const float o1_ = seg_sum<ROW>(p1) + L->b_out[1];
  log_std = pv.log_std != nullptr ? pv.log_std[0] : o1_;
}

// the action: mean + std * g, g the replica's next standard normal draw (Philox block of four per counter / 4, column
// 0x40000000 + agent: a stream of its own next to the vehicles' noise -- agent 0 is the single-agent stream); log-probability
// of a 1-d diagonal Gaussian.  pv.greedy (wave-uniform): the mean itself -- a select, fma(sd, 0, mu) would be NaN where sd
// overflows -- and the density at the mean, the same expression with g = 0; the draw, the counters and the control flow
// around this call are the sampling path's, so greedy and sampling calls interleave on one stream.
// GREEDY: -1 reads pv.greedy at run time -- every kernel but the k_loop_policy family.  There the flag is a template
// parameter (0 / 1) and the launch picks the instantiation from fs_policy.greedy: with one more run-time scalar
// k_loop_policy<0, false, false> was one register over its recorded total (tests/test_codegen.py), so its sampling
// instantiations stay the code they were and the greedy ones are kernels of their own (k_greedy_loop_policy).
template <int GREEDY = -1>
__device__ __forceinline__ void policy_sample(const PolicyView& pv, uint32_t replica, uint32_t ctr, float mu, float log_std,
                                              float& action, float& logp, NoiseBlock<float>* nzb = nullptr,
                                              uint32_t agent = 0u) {
  // (a fragment keeps the four draws of a block over four steps: NoiseBlock::draw is gauss() bit for bit)
  const uint32_t col = 0x40000000u + agent;
  const float g = nzb ? nzb->draw(pv.seed_lo, pv.seed_hi, replica, col, ctr)
                      : gauss<float>(pv.seed_lo, pv.seed_hi, replica, col, ctr);
  const float sd = __builtin_amdgcn_exp2f(log_std * 1.4426950408889634f);
  const float a_s = __builtin_fmaf(sd, g, mu);
  const float lp_s = __builtin_fmaf(-0.5f * g, g, -log_std);
  if constexpr (GREEDY == 0) {
    action = a_s;
    logp = lp_s - 0.9189385332046727f;
  } else {
    const bool greedy = GREEDY == 1 || pv.greedy != 0;
    action = greedy ? mu : a_s;
    logp = (greedy ? -log_std : lp_s) - 0.9189385332046727f;
  }
}

// a fused kernel's draw for agent c of a shared policy: agents 0 and 1 keep their Philox block over four steps (one
// NoiseBlock each, six registers), agents from 2 on draw with gauss() -- the same bits either way (NoiseBlock::draw is
// gauss()); a block per agent for every agent would be an array indexed by the run-time agent: scratch memory
template <int GREEDY = -1>
__device__ __forceinline__ void policy_sample_agent(const PolicyView& pv, uint32_t replica, uint32_t ctr, int c, float mu,
                                                    float log_std, float& action, float& logp, NoiseBlock<float>& nzb0,
                                                    NoiseBlock<float>& nzb1) {
  if (c == 0) policy_sample<GREEDY>(pv, replica, ctr, mu, log_std, action, logp, &nzb0, 0u);          // (wave-uniform)
  else if (c == 1) policy_sample<GREEDY>(pv, replica, ctr, mu, log_std, action, logp, &nzb1, 1u);
  else policy_sample<GREEDY>(pv, replica, ctr, mu, log_std, action, logp, nullptr, uint32_t(c));
}

// an agent without a vehicle (FS_ENV_MERGE_MA: its column's RL slot is empty): no command (fs_step_dev reads NaN as
// "no action for this vehicle"), log-probability 0
__device__ __forceinline__ float policy_no_action() { return __builtin_nanf(""); }

// the agents present in the replica's state (FS_ENV_MERGE_MA: agent c is present when the RL slot of column c holds a
// vehicle), as a mask over the columns; every agent of the other heads (slot_lane == NULL).  The 16 lanes of row j test
// slots j, j + 16, ...
template <int ROW>
__device__ __forceinline__ unsigned long long policy_present(const int* slot_lane, const int* slot_ctrl,
                                                             const int* slot_rl, int N, int rr, int j) {
  if (slot_lane == nullptr) return ~0ull;
  unsigned lo = 0u, hi = 0u;
  for (int i = j; i < N; i += ROW) {
    if (slot_ctrl[i] != FS_CTRL_RL || slot_lane[size_t(rr) * N + i] < 0) continue;
    const int c = slot_rl[i] & 63;
    lo |= c < 32 ? 1u << c : 0u;
    hi |= c >= 32 ? 1u << (c - 32) : 0u;
  }
  return (static_cast<unsigned long long>(seg_or<ROW>(hi)) << 32) | seg_or<ROW>(lo);
}

// eager form: actions and log-probabilities for the observations obs [R, n_ag * in_dim] of n_ag agents sharing the policy
// (n_ag = 1: one RL vehicle); act / logp [R, n_ag].  A row of 16 lanes is one replica and evaluates its agents in turn:
// agent c draws from column 0x40000000 + c at the replica's counter, which advances by ONE per call.  (One row per
// (replica, agent) would let a replica's agents straddle two waves, and the row that advances the counter could run
// before a row that still has to read it.)  slot_lane / slot_ctrl / slot_rl (FS_ENV_MERGE_MA, else NULL): the handle's
// current routes [R, N] and its slots' controllers and columns, which say which agents are present (policy_present);
// an absent agent gets policy_no_action() and log-probability 0.
template <int ROW>     // (a template so that every object of the library may include this header)
__global__ __launch_bounds__(256) void k_policy_act(PolicyView pv, int R, int n_ag, uint32_t rep0,
                                                    const float* __restrict__ obs, float* __restrict__ act,
                                                    float* __restrict__ logp, const int* __restrict__ slot_lane,
                                                    const int* __restrict__ slot_ctrl, const int* __restrict__ slot_rl,
                                                    int N) {
  __shared__ PolicyLds L;
  policy_load(pv, &L, threadIdx.x, blockDim.x);
  const int lane = threadIdx.x & 63, j = lane & 15;
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int rr = r < R ? r : R - 1;
  const uint32_t c0 = pv.ctr[rr];
  const unsigned long long present = policy_present<ROW>(slot_lane, slot_ctrl, slot_rl, N, rr, j);
#pragma unroll 1
  for (int c = 0; c < n_ag; ++c) {
    const float* o = obs + (size_t(rr) * n_ag + c) * pv.in_dim;
    float mu, ls;
    if (pv.in_dim > 4) {                                   // (wave-uniform)
      float ia, ib;
      policy_wide_inputs(o, pv.in_dim, j, ia, ib);
      policy_eval<ROW, true>(pv, &L, j, ia, ib, 0.0f, mu, ls);
    } else {
      policy_eval<ROW>(pv, &L, j, o[0], pv.in_dim > 1 ? o[1] : 0.0f, pv.in_dim > 2 ? o[2] : 0.0f, mu, ls);
    }
    float a, lp;
    policy_sample(pv, rep0 + uint32_t(rr), c0, mu, ls, a, lp, nullptr, uint32_t(c));
    if (r < R && j == 0) {
      const bool here = ((present >> (c & 63)) & 1ull) != 0ull;
      act[size_t(r) * n_ag + c] = here ? a : policy_no_action();
      logp[size_t(r) * n_ag + c] = here ? lp : 0.0f;
    }
  }
  if (r < R && j == 0) pv.ctr[r] = c0 + 1u;
}

// ---- the ACTION-VECTOR head (FS_ENV_MERGE_PO: MergePOEnv) ---------------------------------------------------------
// ONE network maps the whole observation (in_dim = 5 A <= 32 values, A = num_rl) to A actions: policy_trunk<WIDE> (the
// trunk every policy kernel runs), then an output layer of n_out = 2 A rows (rows 0 .. A-1 the means, rows A .. 2A-1 the
// log stds: RLlib's DiagGaussian order) or of A rows next to A free log stds.  A WAVE is one replica: its four 16-lane rows run the trunk
// alike (a row holds the 32 units of a layer), every output is the row's tree sum, lane c of a row then samples column c
// (Philox column 0x40000000 + c at the replica's counter: agent c's stream of the shared-policy heads) and the wave
// adds the columns' log-probabilities in ascending order.  policy_vec_act is the head's one definition: k_policy_act_vec
// (eager) and k_merge_policy (fused, flowsim_queue.h) both call it, and it calls the shared trunk, so they agree bit for
// bit by construction.
constexpr int FS_POLICY_VEC_MAX = 6;                      // 5 A <= 32: the WIDE first layer

struct alignas(16) PolicyVecLds {
  float w_out[2 * FS_POLICY_VEC_MAX][32];                  // [output][unit]
  float b_out[2 * FS_POLICY_VEC_MAX];
  float log_std[FS_POLICY_VEC_MAX];                        // the free log stds (pv.log_std != NULL)
  float lp[16];                                            // the columns' log-probabilities of a step
};

// weights -> LDS, once per launch: policy_load_trunk, then the output layer of n_out = A or 2 A rows and the free log stds;
// one barrier
__device__ __forceinline__ void policy_vec_load(const PolicyView& pv, int A, PolicyLds* L, PolicyVecLds* V, int tid,
                                                int nthreads) {
  const float* p = policy_load_trunk(pv, L, tid, nthreads);
  const int n_out = pv.n_out;
  for (int e = tid; e < 2 * FS_POLICY_VEC_MAX * 32; e += nthreads) V->w_out[e / 32][e % 32] = (e / 32) < n_out ? p[e] : 0.0f;
  for (int e = tid; e < 2 * FS_POLICY_VEC_MAX; e += nthreads) V->b_out[e] = e < n_out ? p[n_out * 32 + e] : 0.0f;
  for (int e = tid; e < FS_POLICY_VEC_MAX; e += nthreads) V->log_std[e] = (pv.log_std != nullptr && e < A) ? pv.log_std[e] : 0.0f;
  __syncthreads();
}

// The A actions and the joint log-probability of ONE replica, computed by its wave (lane = 0 .. 63).  `o`: the replica's
// observation, 5 A floats (LDS or global); act_row [>= 16 floats of LDS]: columns 0 .. A-1 receive the samples (the rest
// of its first 16 entries zero).  Returns the joint log-probability: the columns' values added in ascending order.
// nzb (a fragment): this lane's Philox block kept over four steps (NoiseBlock::draw is gauss() bit for bit).
__device__ __forceinline__ float policy_vec_act(const PolicyView& pv, int A, const PolicyLds* L, PolicyVecLds* V,
                                                uint32_t replica, uint32_t ctr, int lane, const float* o, float* act_row,
                                                NoiseBlock<float>* nzb = nullptr) {
  const int j = lane & 15;
  float ia, ib, ha, hb;
  policy_wide_inputs(o, pv.in_dim, j, ia, ib);
  policy_trunk<true>(pv, L, j, ia, ib, 0.0f, ha, hb);
  // the outputs: each the row's tree sum of the lanes' two products (policy_eval's head); lane c keeps column c's
  const bool free_ls = pv.log_std != nullptr;
  float mu = 0.0f, ls = 0.0f;
#pragma unroll 1
  for (int c = 0; c < A; ++c) {
    float p0 = V->w_out[c][j] * ha;
    p0 = __builtin_fmaf(V->w_out[c][j + 16], hb, p0);
    const float m = seg_sum<16>(p0) + V->b_out[c];
    float l = V->log_std[c];
    if (!free_ls) {                                        // (wave-uniform)
      float p1 = V->w_out[A + c][j] * ha;
      p1 = __builtin_fmaf(V->w_out[A + c][j + 16], hb, p1);
      l = seg_sum<16>(p1) + V->b_out[A + c];
    }
    mu = j == c ? m : mu;
    ls = j == c ? l : ls;
  }
  // every lane samples its column (lanes beyond the A columns: values nobody reads)
  float a, lp;
  policy_sample(pv, replica, ctr, mu, ls, a, lp, nzb, uint32_t(j));
  if (lane < 16) {
    act_row[lane] = lane < A ? a : 0.0f;
    V->lp[lane] = lane < A ? lp : 0.0f;
  }
  asm volatile("" ::: "memory");                           // (one wave: the hardware keeps its DS instructions in order)
  float logp = V->lp[0];
#pragma unroll 1
  for (int c = 1; c < A; ++c) logp = logp + V->lp[c];
  asm volatile("" ::: "memory");
  return logp;
}

// eager form of the action-vector head: obs [R, 5 A] -> act [R, A], logp [R]; one wave per replica; the replica's counter
// advances by ONE per call
template <int ROW>     // (a template so that every object of the library may include this header)
__global__ __launch_bounds__(64) void k_policy_act_vec(PolicyView pv, int R, int A, uint32_t rep0,
                                                       const float* __restrict__ obs, float* __restrict__ act,
                                                       float* __restrict__ logp) {
  static_assert(ROW == 16, "k_policy_act_vec: a row of 16 lanes holds the 32 units of a layer");
  __shared__ PolicyLds L;
  __shared__ PolicyVecLds V;
  __shared__ float act_row[16];
  const int lane = threadIdx.x, r = blockIdx.x;            // (grid = R)
  policy_vec_load(pv, A, &L, &V, lane, 64);
  const uint32_t c0 = pv.ctr[r];
  const float lp = policy_vec_act(pv, A, &L, &V, rep0 + uint32_t(r), c0, lane, obs + size_t(r) * pv.in_dim, act_row);
  if (lane < A) act[size_t(r) * A + lane] = act_row[lane];
  if (lane == 0) {
    logp[r] = lp;
    pv.ctr[r] = c0 + 1u;
  }
}

// ---- the WIDE action-vector head (FS_ENV_BOTTLENECK_DV: BottleneckDesiredVelocityEnv, 141 -> 20; FS_ENV_MERGE_PO with 7 ..
// 32 places: 35 .. 160 -> num_rl, eagerly here and fused in k_merge_wide_policy, flowsim_queue.h) --------------------------
// ONE network maps the whole observation (in_dim = 4 cells + 1 values, 33 .. 513) to A = num_rl <= 64 action columns.  A
// WAVE is one replica, as in policy_vec_act; nothing below depends on R, the grid, or the place of the wave in its
// workgroup, so a fused kernel that gives a replica's wave to policy_wide_act computes the same bits (k_merge_wide_policy
// does).
//
// THE FIRST LAYER (policy_wide_layer1), its summation order:
//   * the observation is cut into CHUNKS of 32 inputs, chunk n = inputs 32 n .. 32 n + 31 (inputs from in_dim on: zero,
//     and so are their weights);
//   * row w (lanes 16 w .. 16 w + 15) of the wave takes chunks w, w + 4, w + 8, ... in ascending order and runs each
//     through policy_layer -- THE 32-input layer, with its four accumulators and its ((b + z0) + z1) + (z2 + z3) --
//     with the row's running sum in the bias' place: P_w = layer(chunk w + 4 m, layer(..., layer(chunk w, b_w))),
//     b_0 = the unit's bias, b_1 = b_2 = b_3 = 0; every row makes ceil(chunks / 4) passes, a pass beyond the last
//     chunk adds zeros;
//   * the unit's sum is (P_0 + P_1) + (P_2 + P_3): v_permlane16_swap, then v_permlane32_swap (a + b is commutative,
//     so the four rows hold the same bits).
// Lane j of every row ends with the sums of units j and j + 16: what policy_trunk<., PRE> takes.
// Weights: a first-layer weight is used ONCE per replica, so it is not staged in LDS (32 x 513 floats would not fit the
// 64 KB of static LDS either, and a workgroup would write as many bytes to LDS as it then reads).  Lane j reads the 32
// floats of rows j and j + 16 of W1 at its chunk as eight 16-byte loads each, straight from the packed buffer (W1 is
// row-major and in_dim is odd: the loads are 4-byte aligned, which global memory takes); the four rows of the wave read
// four consecutive 128-byte pieces of the same 32 weight rows, and every replica reads the same 18 .. 66 KB, which stay
// in L2.  A 16-byte load of the last chunk may run past the end of a weight row into the next one, and past W1 into b1
// and the layers behind it (at most 31 floats: inside the buffer); those values are replaced by zero before use.
__device__ __forceinline__ f2 policy_wide_layer1(const PolicyView& pv, const PolicyLds* L, int lane, const float* o) {
  const int j = lane & 15, row = lane >> 4;
  const int in_dim = pv.in_dim, nch = (in_dim + 31) >> 5;
  const float* wa = pv.w + size_t(j) * in_dim;
  const float* wb = pv.w + size_t(j + 16) * in_dim;
  f2 z = {row == 0 ? L->b[0][j] : 0.0f, row == 0 ? L->b[0][j + 16] : 0.0f};
#pragma unroll 1
  for (int n0 = 0; n0 < nch; n0 += 4) {
    const int n = n0 + row;
    const int base = 32 * (n < nch ? n : nch - 1);         // (a pass beyond the last chunk: a valid address, nothing used)
    const int left = in_dim - 32 * n;                      // inputs of this chunk that exist (<= 0: none)
    const int ia = base + j, ib = base + 16 + j;
    const float a = j < left ? o[ia < in_dim ? ia : 0] : 0.0f;
    const float b = 16 + j < left ? o[ib < in_dim ? ib : 0] : 0.0f;
    float4 ww[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {                          // inputs 4 t .. 4 t + 3 of the chunk: rows j and j + 16 of W1
      float4 ra, rb;
      __builtin_memcpy(&ra, wa + base + 4 * t, 16);
      __builtin_memcpy(&rb, wb + base + 4 * t, 16);
      const bool k0 = 4 * t < left, k1 = 4 * t + 1 < left, k2 = 4 * t + 2 < left, k3 = 4 * t + 3 < left;
      ww[2 * t] = make_float4(k0 ? ra.x : 0.0f, k0 ? rb.x : 0.0f, k1 ? ra.y : 0.0f, k1 ? rb.y : 0.0f);
      ww[2 * t + 1] = make_float4(k2 ? ra.z : 0.0f, k2 ? rb.z : 0.0f, k3 ? ra.w : 0.0f, k3 ? rb.w : 0.0f);
    }
    z = policy_layer(ww, z.x, z.y, a, b);
  }
  z.x = add_swap32(add_swap16(z.x));
  z.y = add_swap32(add_swap16(z.y));
  return z;
}

struct alignas(16) PolicyWideLds {
  float lp[4][64];                                         // [wave of the block][column]: the log-probabilities of a step
};

// The A actions and the joint log-probability of ONE replica, computed by its wave (lane = 0 .. 63): policy_wide_layer1,
// policy_trunk's hidden layers, then the output rows -- each the row's tree sum of the lanes' two products, as in
// policy_vec_act; row w of the wave works out columns 16 w .. 16 w + 15 and lane c keeps column c's.  w_out: where the
// output layer starts in pv.w (policy_load_trunk's return value; each of its weights is used once per replica: read from
// global memory, 64 consecutive bytes per row and half).  Lane c < A samples column c (Philox column 0x40000000 + c at
// the replica's counter) and returns the action in `action` (other lanes: 0); lp_row: 64 floats of LDS of THIS wave.
// Returns the joint log-probability: the columns' values added in ascending order, float32, the same in every lane.
// AHEAD: WHEN the output rows are loaded, which changes no value.  true (the eager kernel): first, so that they land
// while the first layer runs.  false (a fused kernel, whose wave holds a replica's simulator state in registers as well):
// behind the trunk, FS_WIDE_OUT_GROUP columns at a time, each group in front of the columns that use it -- 96 more
// registers live through the first layer, or 96 at once behind it, is what the fused kernel does not have (with all
// sixteen columns loaded together k_merge_wide_policy spilled to scratch memory).
constexpr int FS_WIDE_OUT_GROUP = 4;
template <bool AHEAD = true>
__device__ __forceinline__ float policy_wide_act(const PolicyView& pv, int A, const PolicyLds* L, const float* w_out,
                                                 float* lp_row, uint32_t replica, uint32_t ctr, int lane, const float* o,
                                                 float& action, NoiseBlock<float>* nzb = nullptr) {
  const int j = lane & 15, row = lane >> 4;
  // the output rows of this row's columns 16 row .. 16 row + 15 (a column >= A: row A - 1 again, its value is not kept)
  const bool free_ls = pv.log_std != nullptr;
  const float* b_out = w_out + size_t(pv.n_out) * 32;
  const int cols = A < 16 ? A : 16;                         // (wave-uniform)
  float wm_a[16], wm_b[16], wl_a[16], wl_b[16], bm[16], bl[16];
  auto load_out = [&](auto t0_c) {                          // columns t0 .. of this row: all sixteen, or one group
    constexpr int t0 = decltype(t0_c)::value;
#pragma unroll
    for (int t = t0; t < t0 + (AHEAD ? 16 : FS_WIDE_OUT_GROUP); ++t) {
      const int c = 16 * row + t, cc = c < A ? c : A - 1;
      wm_a[t] = wm_b[t] = wl_a[t] = wl_b[t] = bm[t] = bl[t] = 0.0f;
      if (t < cols) {                                      // (wave-uniform)
        wm_a[t] = w_out[size_t(cc) * 32 + j];
        wm_b[t] = w_out[size_t(cc) * 32 + j + 16];
        bm[t] = b_out[cc];
        if (!free_ls) {
          wl_a[t] = w_out[size_t(A + cc) * 32 + j];
          wl_b[t] = w_out[size_t(A + cc) * 32 + j + 16];
          bl[t] = b_out[A + cc];
        }
      }
    }
  };
  if constexpr (AHEAD) load_out(std::integral_constant<int, 0>{});
  const f2 z = policy_wide_layer1(pv, L, lane, o);
  float ha, hb;
  policy_trunk<true, true>(pv, L, j, z.x, z.y, 0.0f, ha, hb);
  float mu = 0.0f, ls = 0.0f;
  static_for<16>([&](auto t_c) {
    constexpr int t = decltype(t_c)::value;
    if constexpr (!AHEAD && t % FS_WIDE_OUT_GROUP == 0) load_out(t_c);
    if (t < cols) {                                        // (wave-uniform)
      float p0 = wm_a[t] * ha;
      p0 = __builtin_fmaf(wm_b[t], hb, p0);
      const float m = seg_sum<16>(p0) + bm[t];
      float l = 0.0f;
      if (!free_ls) {                                      // (wave-uniform)
        float p1 = wl_a[t] * ha;
        p1 = __builtin_fmaf(wl_b[t], hb, p1);
        l = seg_sum<16>(p1) + bl[t];
      }
      mu = j == t ? m : mu;
      ls = j == t ? l : ls;
    }
  });
  if (free_ls) ls = pv.log_std[lane < A ? lane : A - 1];
  float a, lp;
  policy_sample(pv, replica, ctr, mu, ls, a, lp, nzb, uint32_t(lane));
  action = lane < A ? a : 0.0f;
  lp_row[lane] = lane < A ? lp : 0.0f;
  asm volatile("" ::: "memory");                           // (one wave: the hardware keeps its DS instructions in order)
  float logp = lp_row[0];
#pragma unroll 1
  for (int c = 1; c < A; ++c) logp = logp + lp_row[c];
  asm volatile("" ::: "memory");
  return logp;
}

// eager form of the wide action-vector head: obs [R, in_dim] -> act [R, A], logp [R]; one wave per replica, four replicas
// per workgroup (they share the LDS copy of the hidden layers); the replica's counter advances by ONE per call
template <int ROW>     // (a template so that every object of the library may include this header)
__global__ __launch_bounds__(256) void k_policy_act_wide(PolicyView pv, int R, int A, uint32_t rep0,
                                                         const float* __restrict__ obs, float* __restrict__ act,
                                                         float* __restrict__ logp) {
  static_assert(ROW == 16, "k_policy_act_wide: a row of 16 lanes holds the 32 units of a layer");
  __shared__ PolicyLds L;
  __shared__ PolicyWideLds W;
  const float* w_out = policy_load_trunk(pv, &L, threadIdx.x, blockDim.x);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;                     // (grid = ceil(R / 4))
  if (r >= R) return;                                      // (wave-uniform, after the only barrier)
  const uint32_t c0 = pv.ctr[r];
  float a;
  const float lp = policy_wide_act(pv, A, &L, w_out, W.lp[wave], rep0 + uint32_t(r), c0, lane, obs + size_t(r) * pv.in_dim, a);
  if (lane < A) act[size_t(r) * A + lane] = a;
  if (lane == 0) {
    logp[r] = lp;
    pv.ctr[r] = c0 + 1u;
  }
}

// ---- the ROW-per-replica action-vector head (FS_ENV_ACCEL with num_rl = 2 .. 16 on a segment-table loop: the reference's
// flow/benchmarks/figureeight1.py, 28 -> 7, and figureeight2.py, 28 -> 14) -------------------------------------------
// ONE network maps the whole observation (in_dim <= 32 values in policy_wide_inputs' layout) to A = num_rl action
// columns, with a ROW of 16 lanes per replica -- k_loop_policy's mapping, where a lane already holds the vehicle a column
// belongs to -- instead of policy_vec_act's wave.  policy_trunk<true>, then an output layer of n_out = 2 A rows (rows
// 0 .. A-1 the means, A .. 2A-1 the log stds: RLlib's DiagGaussian order) or of A rows next to A free log stds; output
// row c is policy_vec_act's expression, the row's tree sum of the lanes' two products plus the bias.  Every lane is
// told which column it samples (`col`, -1: none): the eager k_policy_act_row gives column j to lane j, the fused
// k_loop_policy_vec gives column rl_index to the lane of that RL vehicle; a column's mean and log std are computed alike
// whichever lane keeps them, its draw is Philox column 0x40000000 + c at the replica's counter (agent c's stream of the
// shared-policy heads), and the joint log-probability is the columns' values added in ascending column order, so the
// two kernels agree bit for bit by construction (tests/test_policy_loop_vec_gpu.py).
constexpr int FS_POLICY_ROW_VEC_MAX = 16;                  // one column per lane of a row

struct alignas(16) PolicyRowVecLds {
  // the output rows in groups of four columns: [group g][half][lane j][t] = W[4 g + t][j + 16 half] -- a lane reads its two
  // weights of four columns with two b128 reads, the 16 lanes of a row 256 consecutive bytes (w_hid's reason).  w_ls: rows
  // A + 4 g + t (the 2 A head; zero next to free log stds).  Columns from A on: zero.
  float w_mu[4][2][16][4];
  float w_ls[4][2][16][4];
  float b_mu[16];
  float b_ls[16];                                          // the bias of row A + c, or the free log std of column c
  float lp[16][16];                                        // [row of the workgroup][column]: the log-probabilities of a step
};

// weights -> LDS, once per launch: policy_load_trunk, then the output layer and the free log stds; one barrier
__device__ __forceinline__ void policy_row_vec_load(const PolicyView& pv, int A, PolicyLds* L, PolicyRowVecLds* V, int tid,
                                                    int nthreads) {
  const float* p = policy_load_trunk(pv, L, tid, nthreads);
  const bool free_ls = pv.log_std != nullptr;
  const float* b = p + size_t(pv.n_out) * 32;
  for (int e = tid; e < 16 * 32; e += nthreads) {
    const int c = e / 32, u = e % 32;
    V->w_mu[c >> 2][u >> 4][u & 15][c & 3] = c < A ? p[c * 32 + u] : 0.0f;
    V->w_ls[c >> 2][u >> 4][u & 15][c & 3] = (c < A && !free_ls) ? p[(A + c) * 32 + u] : 0.0f;
  }
  for (int c = tid; c < 16; c += nthreads) {
    V->b_mu[c] = c < A ? b[c] : 0.0f;
    V->b_ls[c] = c < A ? (free_ls ? pv.log_std[c] : b[A + c]) : 0.0f;
  }
  __syncthreads();
}

// The action of THIS lane's column `col` (-1: none, action 0) and the joint log-probability of the row's replica (the
// return value, the same in every lane of the row).  j: the lane within its row; (ia, ib): its two inputs in
// policy_wide_inputs' layout; lp_row: 16 floats of LDS of THIS row (PolicyRowVecLds::lp).  Every column 0 .. A-1 must be
// some lane's.  nzb (a fragment): this lane's Philox block kept over four steps (NoiseBlock::draw is gauss() bit for bit).
// pv.greedy is read at run time (policy_sample<-1>).
__device__ __forceinline__ float policy_row_vec_act(const PolicyView& pv, int A, const PolicyLds* L,
                                                    const PolicyRowVecLds* V, float* lp_row, uint32_t replica, uint32_t ctr,
                                                    int j, float ia, float ib, int col, float& action,
                                                    NoiseBlock<float>* nzb = nullptr) {
  float ha, hb;
  policy_trunk<true>(pv, L, j, ia, ib, 0.0f, ha, hb);
  const bool free_ls = pv.log_std != nullptr;
  float mu = 0.0f, ls = 0.0f;
#pragma unroll 1
  for (int g = 0; 4 * g < A; ++g) {                        // four columns at a time (a column >= A: zeros, kept by no lane)
    const float4 wa = *reinterpret_cast<const float4*>(V->w_mu[g][0][j]), wb = *reinterpret_cast<const float4*>(V->w_mu[g][1][j]);
    const float4 bm = *reinterpret_cast<const float4*>(&V->b_mu[4 * g]), bl = *reinterpret_cast<const float4*>(&V->b_ls[4 * g]);
    const float was[4] = {wa.x, wa.y, wa.z, wa.w}, wbs[4] = {wb.x, wb.y, wb.z, wb.w};
    const float bms[4] = {bm.x, bm.y, bm.z, bm.w}, bls[4] = {bl.x, bl.y, bl.z, bl.w};
    float m[4], l[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float p0 = was[t] * ha;
      p0 = __builtin_fmaf(wbs[t], hb, p0);
      m[t] = seg_sum<16>(p0) + bms[t];
      l[t] = bls[t];
    }
    if (!free_ls) {                                        // (wave-uniform)
      const float4 la = *reinterpret_cast<const float4*>(V->w_ls[g][0][j]), lb = *reinterpret_cast<const float4*>(V->w_ls[g][1][j]);
      const float las[4] = {la.x, la.y, la.z, la.w}, lbs[4] = {lb.x, lb.y, lb.z, lb.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float p1 = las[t] * ha;
        p1 = __builtin_fmaf(lbs[t], hb, p1);
        l[t] = seg_sum<16>(p1) + bls[t];
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      mu = col == 4 * g + t ? m[t] : mu;
      ls = col == 4 * g + t ? l[t] : ls;
    }
  }
  float a, lp;
  policy_sample(pv, replica, ctr, mu, ls, a, lp, nzb, uint32_t(col < 0 ? 0 : col));
  action = col >= 0 ? a : 0.0f;
  if (col >= 0) lp_row[col & 15] = lp;
  asm volatile("" ::: "memory");                           // (one wave: the hardware keeps its DS instructions in order)
  float4 q[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) q[t] = *reinterpret_cast<const float4*>(lp_row + 4 * t);
  asm volatile("" ::: "memory");
  const float lps[16] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w,
                         q[2].x, q[2].y, q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w};
  float logp = lps[0];
#pragma unroll
  for (int c = 1; c < 16; ++c) logp = c < A ? logp + lps[c] : logp;      // ((lp0 + lp1) + lp2) + ...
  return logp;
}

// eager form of the row-per-replica action-vector head: obs [R, in_dim] -> act [R, A], logp [R]; a row of 16 lanes per
// replica and 256 threads per workgroup, as in k_policy_act; lane j samples column j; the replica's counter advances by
// ONE per call
template <int ROW>     // (a template so that every object of the library may include this header)
__global__ __launch_bounds__(256) void k_policy_act_row(PolicyView pv, int R, int A, uint32_t rep0,
                                                        const float* __restrict__ obs, float* __restrict__ act,
                                                        float* __restrict__ logp) {
  static_assert(ROW == 16, "k_policy_act_row: a row of 16 lanes holds the 32 units of a layer");
  __shared__ PolicyLds L;
  __shared__ PolicyRowVecLds V;
  policy_row_vec_load(pv, A, &L, &V, threadIdx.x, blockDim.x);
  const int j = threadIdx.x & 15;
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int rr = r < R ? r : R - 1;
  const uint32_t c0 = pv.ctr[rr];
  float ia, ib, a;
  policy_wide_inputs(obs + size_t(rr) * pv.in_dim, pv.in_dim, j, ia, ib);
  const float lp = policy_row_vec_act(pv, A, &L, &V, V.lp[threadIdx.x >> 4], rep0 + uint32_t(rr), c0, j, ia, ib,
                                      j < A ? j : -1, a);
  if (r < R && j < A) act[size_t(r) * A + j] = a;
  if (r < R && j == 0) {
    logp[r] = lp;
    pv.ctr[r] = c0 + 1u;
  }
}

// K x (policy -> action -> Env.step [-> reset of a finished episode]) for rings of IDM vehicles and RL vehicles.
// HEAD 1: WaveAttenuationPOEnv, ONE RL vehicle: obs [K+1, R, 3] (obs[0]: the observation of the state the fragment starts
// from), act [K, R], logp [K, R], rew [K, R], done [K, R].
// HEAD 2: MultiAgentWaveAttenuationPOEnv (float32), n_ag = num_rl agents sharing the policy: agent c is the RL vehicle of
// column c, obs [K+1, R, 3 n_ag] (block c: its three values), act / logp [K, R, n_ag], rew [K, R] (the shared reward); a
// collision ends nothing (multiagent/base.py:188-190).  Per step the row evaluates the agents in turn (the observation of
// agent c, the network, the draw of column 0x40000000 + c); each lane keeps the actions of its own slots' columns and of
// its places in the reward's sum by selects.
// HEAD 4: MultiWaveAttenuationPOEnv (float32; a row is ONE ring of MultiRingNetwork, one agent): HEAD 1 with the
// bumper-to-bumper headway as third value, the on-edge desired-velocity reward (multi_ring_terms / multi_ring_reward,
// flowsim_ringrl.h) and no crash; the shapes are HEAD 1's.
// The simulator part is RingPairCore (flowsim_ringrl.h): the ONE definition of the ring step, which k_ring_pair runs too.
template <typename T, int HEAD, bool NOISE, bool FAST>
__global__ __launch_bounds__(256) void k_ring_policy(DevView<T> s, PolicyView pv, int num_steps, int reset_done,
                                                     int warmup_steps, float* __restrict__ obs, float* __restrict__ act,
                                                     float* __restrict__ logp, float* __restrict__ rew,
                                                     uint8_t* __restrict__ done) {
  constexpr int ROW = 16;
  constexpr bool MIXED = sizeof(T) == 8;
  constexpr bool MA = HEAD == 2;
  constexpr bool MR = HEAD == 4;
  static_assert(HEAD == 1 || HEAD == 2 || HEAD == 4, "k_ring_policy: the PO heads");
  static_assert(!((MA || MR) && MIXED), "the multi-agent heads exist in float32 only");
  __shared__ PolicyLds PL;
  policy_load(pv, &PL, threadIdx.x, blockDim.x);
  RingPairCore<T, ROW, NOISE, FAST> core(s);
  const int lane = core.lane, k = core.k, N = core.N, LP = core.LP, rr = core.rr, iA = core.iA, iB = core.iB;
  const bool rvalid = core.rvalid, valid = core.valid, last = core.last, rlA = core.rlA, rlB = core.rlB;
  uint32_t pctr = pv.ctr[rr];
  core.set_length(s.ring_len[rr] + T(4) * s.jlen);
  core.load_state(s.pos, s.vel);
  core.snapshot();
  const f2 &v = core.v, &vl = core.vl, &h = core.h, &dgap = core.dgap;                  // (the core's state, by its names)
  MultiRingGeom mrg = {0.0f, 0.0f, 0.0f};
  if constexpr (MR) {
    mrg.quarter = float(s.ring_len[rr]) / 4.0f;
    mrg.qj = mrg.quarter + float(s.jlen);
    mrg.target = float(s.target_velocity);
  }

  // WaveAttenuationPOEnv.get_state of the current snapshot (k_ring_pair's write_obs): computed by the RL vehicle's
  // lane, handed to the row through LDS (the policy's input), stored by that lane
  const bool poA = valid && rlA, poB = valid && rlB;
  const double rc15 = 1.0 / 15.0, pml64 = double(s.po_max_length), rc_pml64 = 1.0 / pml64;
  float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
  // THE PO observation of a row of 16, float32 -- [v / 15, (v_lead - v) / 15, third / max_length] of the RL vehicle in
  // lane k_rl of the row (selB: its vehicle B, else A), stored at orow[0 .. 2] and handed to the row as the policy's
  // input.  The three quotients are exact divisions through float64 (five instructions each, issued for one lane): the
  // RL vehicle's lane hands its second and third numerator to its two neighbours (row rotations) and the three lanes
  // divide one value each -- one division sequence per step instead of three -- and three row broadcasts return them.
  auto observe_po = [&](int k_rl, bool selB, float third, float* orow) {
    const float v_me = selB ? v.y : v.x, v_ld = selB ? vl.y : vl.x;
    const float n1 = dpp<0x120 + 1>(v_ld - v_me), n2 = dpp<0x120 + 2>(third);     // row_ror: lane i <- lane i - 1 / i - 2
    const int pc = (k - k_rl) & (ROW - 1);                                        // 0: the RL vehicle's lane, 1 / 2: its helpers
    const float n = pc == 0 ? v_me : (pc == 1 ? n1 : n2);
    const float q = div_via_f64(n, pc == 2 ? pml64 : 15.0, pc == 2 ? rc_pml64 : rc15);
    if (rvalid && pc < 3) orow[pc] = q;
    row_bcast<1, 2>(k_rl, q, q, q, o0, o1, o2);
  };
  // the single-agent head: the third value is the RL vehicle's distance to its leader
  const unsigned long long po_m = __ballot(poA || poB);
  const int k_po = po_m ? (__builtin_ctzll(po_m) & (ROW - 1)) : 0;
  const int src0 = (lane - k) + k_po;
  auto observe = [&](float* orow) {
    if constexpr (!MIXED && ROW == 16) {
      // (MR: the third value is the bumper-to-bumper headway, k_ring_pair<MultiRing>'s write_obs)
      observe_po(k_po, poB, MR ? (poB ? h.y : h.x) : (poB ? dgap.y : dgap.x), orow);
    } else {
      // (hand-off to the row through the LDS crossbar, ds_bpermute: one round trip and no memory, where the first version
      // wrote the three values to LDS and read them back between two wave barriers)
      float q0, q1, q2;
      if (MIXED) {
        const double vdn = next_a<ROW>(core.vdA, last, lane);
        const double v_me = poB ? core.vdB : core.vdA, v_ld = poB ? vdn : core.vdB, d_me = poB ? core.dgB : core.dgA;
        q0 = float(v_me * rc15);
        q1 = float((v_ld - v_me) * rc15);
        q2 = float(d_me * rc_pml64);
      } else {
        const float v_me = poB ? v.y : v.x, v_ld = poB ? vl.y : vl.x, d_me = poB ? dgap.y : dgap.x;
        q0 = div_via_f64(v_me, 15.0, rc15);
        q1 = div_via_f64(v_ld - v_me, 15.0, rc15);
        q2 = div_via_f64(d_me, pml64, rc_pml64);
      }
      if (poA || poB) {
        orow[0] = q0;
        orow[1] = q1;
        orow[2] = q2;
      }
      o0 = __shfl(q0, src0, 64);
      o1 = __shfl(q1, src0, 64);
      o2 = __shfl(q2, src0, 64);
    }
  };

  // MultiAgentWaveAttenuationPOEnv.get_state of agent c (k_ring_pair<POMA>'s write_obs: the third value is the
  // bumper-to-bumper headway), block c of the row.  The lane of column c's RL slot -- and whether it is A or B -- is a slot
  // role, the same in every row of the wave.
  const int n_ag = MA ? s.num_rl : 1;
  const int colA = rlA ? s.rl_index[iA] : -1, colB = rlB ? s.rl_index[iB] : -1;
  const bool redA = MA && valid && iA < s.num_rl, redB = MA && valid && iB < s.num_rl;    // (finish()'s places)
  const int obs_dim = MA ? 3 * n_ag : 3;
  auto observe_agent = [&](int c, float* orow) {
    const unsigned long long m = __ballot(k < LP && (colA == c || colB == c));
    const int k_c = m ? (__builtin_ctzll(m) & (ROW - 1)) : 0;
    observe_po(k_c, colB == c, colB == c ? h.y : h.x, orow + 3 * c);
  };

  const size_t R = size_t(s.R);
  NoiseBlock<float> act_draws, act_draws1;
  act_draws.init();
  act_draws1.init();
  if constexpr (!MA) observe(obs + size_t(rr) * 3);
  for (int step = 0; step < num_steps; ++step) {
    // ---- policy -> action --------------------------------------------------------------------------------------
    float a, aA, aB, arA = 0.0f, arB = 0.0f;            // arA / arB: the columns summed at the lane's places (MA)
    if constexpr (MA) {
      aA = 0.0f;
      aB = 0.0f;
      a = 0.0f;
      float* orow = obs + (size_t(step) * R + rr) * obs_dim;
#pragma unroll 1
      for (int c = 0; c < n_ag; ++c) {
        observe_agent(c, orow);
        float mu, ls, ac, lp;
        policy_eval<ROW>(pv, &PL, k, o0, o1, o2, mu, ls);
        policy_sample_agent(pv, s.rep0 + uint32_t(rr), pctr, c, mu, ls, ac, lp, act_draws, act_draws1);
        if (rvalid && k == 0) {
          act[(size_t(step) * R + rr) * n_ag + c] = ac;
          logp[(size_t(step) * R + rr) * n_ag + c] = lp;
        }
        aA = colA == c ? ac : aA;
        aB = colB == c ? ac : aB;
        arA = iA == c ? ac : arA;
        arB = iB == c ? ac : arB;
      }
    } else {
      float mu, ls, lp;
      policy_eval<ROW>(pv, &PL, k, o0, o1, o2, mu, ls);
      policy_sample(pv, s.rep0 + uint32_t(rr), pctr, mu, ls, a, lp, &act_draws);
      if (rvalid && k == 0) {
        act[size_t(step) * R + rr] = a;
        logp[size_t(step) * R + rr] = lp;
      }
      aA = a;
      aB = a;
    }
    pctr += 1u;
    // ---- Env.step ------------------------------------------------------------------------------------------------
    core.template advance<false>(true, true, aA, aB);
    unsigned fl_step;
    float mr_t0 = 0.0f, mr_t1 = 0.0f;
    if constexpr (MR) multi_ring_terms(mrg, valid, core.x, v, fl_step, mr_t0, mr_t1);
    else fl_step = core.step_flags();
    const unsigned fany = seg_or<ROW>(fl_step);
    const bool crashed = !MA && !MR && (fany & 1u) != 0u;   // (multiagent/base.py:188-190: crash = 0)
    const bool bad = (fany & 2u) != 0u || crashed;
    const float sv = seg_sum<ROW>(MR ? mr_t0 : (valid ? v.x + v.y : 0.0f));
    float mean_a;
    if constexpr (MR) {                                     // k_ring_pair<MultiRing>'s terms / finish
      mean_a = seg_sum<ROW>(mr_t1);                         // (the number of on-edge vehicles)
    } else if constexpr (MA) {                              // k_ring_pair's terms / finish: column i summed where slot i stands
      const float caA = tabs(core.clip(arA)), caB = tabs(core.clip(arB));
      const float sa = seg_sum<ROW>((redA ? caA : 0.0f) + (redB ? caB : 0.0f));
      mean_a = div_via_f64(sa, double(s.num_rl), 1.0 / double(s.num_rl));
    } else {
      mean_a = tabs(core.clip(a));                              // (one column: the sum is the value, / 1)
    }
    float reward;
    if constexpr (MR) reward = multi_ring_reward(reinterpret_cast<const float*>(s.max_cost_tab), sv, mean_a, bad);
    else reward = wave_reward(sv, N, mean_a, bad);
    const uint8_t dflag = done_flag(core.tcount >= s.step_limit, crashed);
    if (rvalid && k == 0) {
      rew[size_t(step) * R + rr] = reward;
      done[size_t(step) * R + rr] = dflag;
    }
    // ---- Env.reset of a finished episode (what VecFlowEnv.capture(reset_done=True) does with a masked fs_reset_dev):
    // placement, the pending ring length, warm-up steps with rl_actions = None; the other replicas of the wave wait
    const bool fin = reset_done && dflag != 0;
    if (__ballot(fin) != 0ull) {
      if (fin) {
        core.load_state(s.init_pos, s.init_vel);
        core.set_length(s.init_ring_len[rr] + T(4) * s.jlen);
        core.tcount = 0;
        if constexpr (MR) {
          mrg.quarter = float(s.init_ring_len[rr]) / 4.0f;
          mrg.qj = mrg.quarter + float(s.jlen);
        }
      }
      core.snapshot();
#pragma unroll 1
      for (int w = 0; w < warmup_steps; ++w) core.template advance<false>(fin, false, 0.0f, 0.0f);
      if (fin && valid && core.kk == 0) const_cast<T*>(s.ring_len)[rr] = s.init_ring_len[rr];
    }
    // (MA: the agents' observations are made at the top of the next step, where the policy takes them)
    if constexpr (!MA) observe(obs + (size_t(step + 1) * R + rr) * 3);
  }
  if constexpr (MA) {
#pragma unroll 1
    for (int c = 0; c < n_ag; ++c) observe_agent(c, obs + (size_t(num_steps) * R + rr) * obs_dim);
  }

  if (valid) {
    core.store_state();
    if (core.kk == 0) pv.ctr[rr] = pctr;
  }
}


// K x (policy -> action -> Env.step [-> reset of a finished episode]) on a segment-table loop (the figure eight: BASELINE's
// C3, examples/exp_configs/rl/singleagent/singleagent_figure_eight.py) with ONE RL vehicle.  HEAD 1: WaveAttenuationPOEnv
// (observation 3: BASELINE's pairing), HEAD 0: AccelEnv (observation 2 N: the reference's own pairing -- every lane feeds its
// vehicle's speed and position into the first layer, policy_eval<., WIDE>).  The simulator part is k_rollout_loop's step
// (flowsim_fig8.h), statement by statement: the same model functions, crossing rule, segment cursor, flag word, observation
// quotients and reward expressions, so a fragment equals eager stepping (fs_policy_act_dev, fs_step_dev -- which runs
// k_rollout_loop --, masked fs_reset_dev) bit for bit (tests/test_policy_gpu.py).  Resets inside the fragment: placement only
// (warmup_steps = 0: Sim::launch_policy refuses anything else).
// HEAD 2: MultiAgentAccelPOEnv (examples/exp_configs/rl/multiagent/multiagent_figure_eight.py), n_ag = num_rl agents sharing
// the policy: obs [K+1, R, 6 n_ag], act / logp [K, R, n_ag], the shared desired-velocity reward, no crash
// (tests/test_policy_ma_gpu.py).  Agent c's six values sit on two lanes -- its RL vehicle's (four) and its follower's (two,
// k_rollout_loop's flush_obs) -- and are gathered from registers into policy_wide_inputs' layout for in_dim = 6.
//
// VEC (HEAD 0 with num_rl = 2 .. 16 RL vehicles: the reference's figureeight1 / figureeight2 benchmarks): ONE network, the
// 2 N observations in, num_rl action columns out -- policy_row_vec_act above; the lane of the RL vehicle with rl_index c
// samples and applies column c; act [K, R, num_rl], logp [K, R] (FS_ENV_MERGE_PO's layouts).  Observation, step, reward,
// done and reset are HEAD 0's statements (the desired-velocity reward does not read the action).
//
// The body is written ONCE, loop_policy_body: k_loop_policy calls it with PAIR = false, k_loop_policy_pair (below) with
// HEAD 0 and PAIR = true.  PAIR (two policies, one RL vehicle: AdversarialAccelEnv on the figure eight) adds, all of it
// under `if constexpr (PAIR)`: the adversary's PolicyView pv2 with its LDS copy PL2 and the weight pw; its evaluation on
// the same o0, o1 registers; its draw from Philox column 0x40000000 + 1 (act_draws1) at the replica's counter, keyed by
// ITS seed; the RL lane's command a = fmaf(pw, a_adv, a_av); the stores into the planes of act / logp [2, K, R] (plane 0
// the av, plane 1 the adversary).  The reward of HEAD 0 does not read the action: rew is the av's, the adversary's its
// negation.  The views are taken by value and the LDS is declared in the body, as the kernel had them: with references
// and the tables handed in as pointers k_loop_policy<0, true, true> came out one AGPR larger (tests/test_codegen.py).
template <bool PAIR>
struct PairLds {           // the adversary's LDS copy (PAIR), or nothing
  PolicyLds L;
};
template <>
struct PairLds<false> {};
template <bool VEC>
struct RowVecLds {         // the action-vector head's output rows (VEC), or nothing
  PolicyRowVecLds V;
};
template <>
struct RowVecLds<false> {};

template <int HEAD, bool DELTA4, bool FASTC, bool PAIR, int GREEDY, bool VEC = false>
__device__ __forceinline__ void loop_policy_body(const DevView<float> s, const PolicyView pv, const PolicyView pv2,
                                                 float pw, int num_steps, int reset_done, float* __restrict__ obs,
                                                 float* __restrict__ act, float* __restrict__ logp,
                                                 float* __restrict__ rew, uint8_t* __restrict__ done) {
  typedef float T;
  typedef float X;
  constexpr int SEG = 16, RPW = 4;
  static_assert(!PAIR || HEAD == 0, "loop_policy_body: two policies drive the AccelEnv head's one RL vehicle");
  static_assert(!VEC || (HEAD == 0 && !PAIR && GREEDY == -1), "loop_policy_body: the action-vector head is AccelEnv's, one policy");
  // (the LDS of the kernel this body is inlined into: every instantiation has ONE caller)
  __shared__ X tab_start[FS_MAX_SEGMENTS + 2], tab_fs[FS_MAX_SEGMENTS + 2], tab_sl[FS_MAX_SEGMENTS + 2];
  __shared__ PolicyLds PL;
  __shared__ PairLds<PAIR> PL2;
  __shared__ RowVecLds<VEC> PV;
  if constexpr (VEC) policy_row_vec_load(pv, s.num_rl, &PL, &PV.V, threadIdx.x, blockDim.x);
  else policy_load(pv, &PL, threadIdx.x, blockDim.x);
  if constexpr (PAIR) policy_load(pv2, &PL2.L, threadIdx.x, blockDim.x);
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int seg = lane / SEG;
  const int i = lane % SEG;
  const int r = wave * RPW + seg;
  const int N = s.N;
  const bool rvalid = r < s.R;
  const bool valid = rvalid && i < N;
  const int rr = rvalid ? r : s.R - 1;
  const int ii = i < N ? i : N - 1;
  const size_t idx = size_t(rr) * N + ii;
  const bool wrap_lead = (i + 1 >= N);
  constexpr bool has = true;                          // N > 1 (host-checked)
  const int flags = s.flags;

  if (threadIdx.x < FS_MAX_SEGMENTS + 2) {
    const int q = threadIdx.x, qq = q < FS_MAX_SEGMENTS ? q : 0;
    tab_start[q] = q < s.nseg ? s.seg_start[qq] : X(3.0e38);
    tab_fs[q] = q < s.nseg ? s.seg_flow_start[qq] : X(0);
    tab_sl[q] = q < s.nseg ? s.seg_flow_slope[qq] : X(0);
  }
  __syncthreads();

  Slot<T> sl;
  sl.ctrl = s.ctrl[ii];
  sl.failsafe = 0;
  sl.speed_mode = s.speed_mode[ii];
  sl.rl_index = s.rl_index[ii];
  sl.pis_index = -1;
#pragma unroll
  for (int k = 0; k < FS_MAX_CTRL_PARAMS; ++k) sl.p[k] = T(s.p[k * N + ii]);
  sl.noise = T(s.noise[ii]);
  sl.delay = T(0);
  sl.max_accel = T(s.max_accel[ii]);
  sl.max_decel = T(s.max_decel[ii]);
  sl.length = T(s.length[ii]);
  sl.sumo_tau = T(s.sumo_tau[ii]);
  sl.sumo_min_gap = T(s.sumo_min_gap[ii]);
  sl.sumo_max_speed = T(s.sumo_max_speed[ii]);
  const X len_me = s.length[ii];
  const X len_lead = lead16(len_me, wrap_lead);

  const X L = s.ring_len[rr] + X(4) * s.jlen;
  int tcount = s.time[rr];
  const bool any_noise = (flags & FLAG_HAS_NOISE) != 0;
  uint32_t nctr = any_noise ? s.noise_ctr[rr] : 0u;
  uint32_t pctr = pv.ctr[rr];
  const bool noisy = any_noise && sl.noise > T(0) && sl.ctrl != FS_CTRL_RL && sl.ctrl != FS_CTRL_SIM;

  X x = s.pos[idx];
  X v = s.vel[idx];
  int k = 0;
  X c_st, c_next, c_fs, c_sl;
  auto cursor = [&]() {                                    // the segment of x and its table row
    k = 0;
    for (int q = 1; q < s.nseg; ++q) k = (x >= tab_start[q]) ? q : k;
    c_st = tab_start[k]; c_next = tab_start[k + 1]; c_fs = tab_fs[k]; c_sl = tab_sl[k];
  };
  cursor();
  X xl, vl, d;
  T h;
  const X Lv = in_vgpr(L);
  auto snapshot = [&]() {
    xl = lead16(x, wrap_lead);
    vl = lead16(v, wrap_lead);
    d = wrap_up(xl - x, Lv);
    h = has ? T(d - len_lead) : T(1000);
  };
  snapshot();

  const X dt = in_vgpr(X(s.dt)), ramp = in_vgpr(X(s.ramp));
  const T crash_gap = in_vgpr(T(s.crash_gap)), target_v = in_vgpr(T(s.target_velocity));
  const X ja_in = in_vgpr(X(s.ja_in)), ja_out = in_vgpr(X(s.ja_out)), jb_in = in_vgpr(X(s.jb_in)), jb_out = in_vgpr(X(s.jb_out));
  const X look = in_vgpr(X(s.j_lookahead)), tgap = in_vgpr(X(s.j_time_gap));
  const X za_lo = in_vgpr(X(s.za_lo)), za_hi = in_vgpr(X(s.za_hi)), zb_lo = in_vgpr(X(s.zb_lo)), zb_hi = in_vgpr(X(s.zb_hi));
  const T max_cost = in_vgpr(T(s.max_cost));
  const DivC d_ms = make_divc(T(s.max_speed)), d_L = make_divc(T(L)), d_15 = make_divc(15.0f), d_po = make_divc(T(s.po_max_length));
  // the reward's quotients (k_rollout_loop divides in float32 once per block of four steps; here every step does, so the
  // constant divisors take the float64 route: the correctly rounded quotient either way, half the instructions)
  const DivC d_N = make_divc(T(s.N)), d_nrl = make_divc(T(s.num_rl > 0 ? s.num_rl : 1)), d_20 = make_divc(20.0f),
             d_mc = make_divc(T(s.max_cost) + T(1.1920928955078125e-07));
  IdmC ic;
  ic.p1 = sl.p[1]; ic.p2 = sl.p[2]; ic.p4 = sl.p[4]; ic.p5 = sl.p[5];
  ic.v0 = make_divc(sl.p[0]);
  ic.two_sqrt = make_divc(T(2) * tsqrt(sl.p[2] * sl.p[3]));
  SumoC sc;
  sc.min_gap = sl.sumo_min_gap; sc.tau = sl.sumo_tau; sc.max_accel = sl.max_accel;
  sc.two_sqrt = make_divc(T(2) * tsqrt(sl.max_accel * sl.max_decel));
  sc.max_speed = make_divc(sl.sumo_max_speed);
  const unsigned seg_internal = s.seg_internal;
  const bool junction_on = s.junction_on != 0, need_sumo = (flags & FLAG_NEED_SUMO) != 0;
  const bool gated = s.junction_mode && sl.ctrl != FS_CTRL_RL && sl.ctrl != FS_CTRL_SIM;
  const T clip_lo = in_vgpr(s.clip_actions != 0 ? T(s.act_lo) : T(-3.0e38)), clip_hi = in_vgpr(s.clip_actions != 0 ? T(s.act_hi) : T(3.0e38));
  const bool rl_lane = sl.ctrl == FS_CTRL_RL, sim_lane = sl.ctrl == FS_CTRL_SIM;
  const int num_rl = s.num_rl;
  const bool obs_lane = HEAD == 1 ? (valid && rl_lane && sl.rl_index == 0) : valid;
  const unsigned valid_bits = valid ? 0x3Fu : 0u;
  const unsigned gate_u = gated ? 1u : 0u, cmd_rl = rl_lane ? 1u : 0u, cmd_other = (!rl_lane && !sim_lane) ? 1u : 0u,
                 sm1_u = unsigned(sl.speed_mode) & 1u;
  const bool sm1_lane = (sl.speed_mode & 1) != 0;
  const X adt_c = (sl.speed_mode & 2) ? X(s.max_accel[ii]) * dt : X(3.0e38), ddt_c = (sl.speed_mode & 4) ? X(s.max_decel[ii]) * dt : X(3.0e38);
  T g4[4] = {T(0), T(0), T(0), T(0)};
  if (any_noise && (nctr & 3u) != 0u && noisy) {
    gauss4<T>(s.seed_lo, s.seed_hi, s.rep0 + uint32_t(rr), uint32_t(ii), nctr >> 2, g4, s.noise_exact != 0);
    for (uint32_t q = 0; q < (nctr & 3u); ++q) { g4[0] = g4[1]; g4[1] = g4[2]; g4[2] = g4[3]; }
  }
  X prev_v = v;
  T last_acc = T(0);
  auto junction_flags = [&](X xx, X vv) -> unsigned {
    const unsigned busy_a = sm_in(xx, ja_in - tgap * vv, ja_out + len_me);
    const unsigned in_b = sm_in(xx, jb_in, jb_out + len_me);
    return (busy_a >> 31) | ((in_b >> 31) << 1);
  };
  unsigned jf = junction_on ? seg_or<SEG>(junction_flags(x, v) & valid_bits) : 0u;

  // the observation of the current state: stored, and handed to the row as the policy's input.  PO head: the RL vehicle's
  // three values reach every lane of its row; AccelEnv head: every lane keeps its own two (inputs ii and N + ii)
  const int obs_dim = HEAD == 1 ? 3 : (HEAD == 2 ? 6 * num_rl : 2 * N);
  const unsigned long long rl_m = __ballot(valid && rl_lane);
  const int k_rl = rl_m ? (__builtin_ctzll(rl_m) & (SEG - 1)) : 0;
  const int src_rl = (lane - i) + k_rl;
  float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
  // HEAD 2 (k_rollout_loop<AccelMA>'s observation): a lane's four values of its own block and the two of its leader's
  // (lead_col: the leader's column, -1 if the leader is no RL vehicle); kept for the agents' gather (m3l: the leader's m3)
  const int own_col = sl.rl_index < 0 ? 0 : sl.rl_index;
  const int lead_col = HEAD == 2 ? __builtin_bit_cast(int, lead16(__builtin_bit_cast(float, rl_lane ? own_col : -1), wrap_lead)) : -1;
  const bool fw_lane = HEAD == 2 && valid && lead_col >= 0;
  float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3l = 0.0f, m5 = 0.0f;
  auto observe = [&](float* orow) {
    if (HEAD == 2) {
      const T xo = c_fs + c_sl * (x - c_st);
      const T xol = lead16(xo, wrap_lead);
      m0 = divc(xo, d_L);                                                          // multiagent/ring/accel.py:163-208
      m1 = divc(v, d_ms);
      m2 = divc(vl - v, d_ms);
      const float m3 = divc((xol - xo) - len_me, d_L);
      m5 = divc(h, d_L);
      if (valid && rl_lane) { float* o = orow + 6 * own_col; o[0] = m0; o[1] = m1; o[2] = m2; o[3] = m3; }
      if (fw_lane) { float* o = orow + 6 * lead_col; o[4] = m2; o[5] = m5; }
      m3l = lead16(m3, wrap_lead);                     // the follower of an RL vehicle holds that vehicle's fourth value
    } else if (HEAD == 1) {
      const float po0 = divc(v, d_15), po1 = divc(vl - v, d_15), po2 = divc(d, d_po);      // wave_attenuation.py:248-269
      if (obs_lane) { orow[0] = po0; orow[1] = po1; orow[2] = po2; }
      row_bcast<0, 0>(k_rl, po0, po1, po2, o0, o1, o2);
    } else {
      const X xo = c_fs + c_sl * (x - c_st);
      const float po0 = divc(v, d_ms), po1 = divc(xo, d_L);                                   // accel.py:116-123
      if (obs_lane) { orow[ii] = po0; orow[N + ii] = po1; }
      o0 = valid ? po0 : 0.0f;
      o1 = valid ? po1 : 0.0f;
    }
  };

  const size_t R = size_t(s.R);
  const int n_ag = HEAD == 2 ? num_rl : 1;
  NoiseBlock<float> act_draws, act_draws1;
  act_draws.init();
  act_draws1.init();
  // VEC: the column this lane samples and applies -- its RL vehicle's rl_index
  const int vec_col = (VEC && valid && rl_lane) ? sl.rl_index : -1;
  observe(obs + size_t(rr) * obs_dim);
  for (int step = 0; step < num_steps; ++step) {
    // ---- policy -> action --------------------------------------------------------------------------------------
    float mu, ls, a, lp;
    if constexpr (HEAD == 2) {
      // agent c: its RL vehicle's lane i_c and the follower's f_c (slot roles: the same in every row) hand their values
      // to the row, lanes 0..2 keep theirs; the lane of an RL vehicle keeps its own column's action
      a = 0.0f;
#pragma unroll 1
      for (int c = 0; c < n_ag; ++c) {
        const unsigned long long m = __ballot(i < N && rl_lane && sl.rl_index == c);
        const int i_c = m ? (__builtin_ctzll(m) & (SEG - 1)) : 0;
        const int f_c = i_c == 0 ? N - 1 : i_c - 1;
        float a0, a1, a2, b0, b1, b2;
        row_bcast<0, 0>(i_c, m0, m1, m2, a0, a1, a2);
        row_bcast<0, 0>(f_c, m3l, m2, m5, b0, b1, b2);
        const float ia = i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : 0.0f));
        const float ib = i == 0 ? b0 : (i == 1 ? b1 : (i == 2 ? b2 : 0.0f));
        float ac;
        policy_eval<SEG, true>(pv, &PL, i, ia, ib, 0.0f, mu, ls);
        policy_sample_agent<GREEDY>(pv, s.rep0 + uint32_t(rr), pctr, c, mu, ls, ac, lp, act_draws, act_draws1);
        if (rvalid && i == 0) {
          act[(size_t(step) * R + rr) * n_ag + c] = ac;
          logp[(size_t(step) * R + rr) * n_ag + c] = lp;
        }
        a = (rl_lane && own_col == c) ? ac : a;
      }
    } else if constexpr (VEC) {
      // ONE evaluation, num_rl columns (policy_row_vec_act: what k_policy_act_row runs); act [K, R, A], logp [K, R]
      lp = policy_row_vec_act(pv, num_rl, &PL, &PV.V, PV.V.lp[threadIdx.x >> 4], s.rep0 + uint32_t(rr), pctr, i, o0, o1,
                              vec_col, a, &act_draws);
      if (rvalid && vec_col >= 0) act[(size_t(step) * R + rr) * num_rl + vec_col] = a;
      if (rvalid && i == 0) logp[size_t(step) * R + rr] = lp;
    } else {
      if (HEAD == 1) policy_eval<SEG>(pv, &PL, i, o0, o1, o2, mu, ls);
      else policy_eval<SEG, true>(pv, &PL, i, o0, o1, 0.0f, mu, ls);
      policy_sample<GREEDY>(pv, s.rep0 + uint32_t(rr), pctr, mu, ls, a, lp, &act_draws);
      if (rvalid && i == 0) {
        act[size_t(step) * R + rr] = a;
        logp[size_t(step) * R + rr] = lp;
      }
      if constexpr (PAIR) {                              // the adversary: the same observation, its own network and stream
        float mu2, ls2, a2, lp2;
        policy_eval<SEG, true>(pv2, &PL2.L, i, o0, o1, 0.0f, mu2, ls2);
        policy_sample<GREEDY>(pv2, s.rep0 + uint32_t(rr), pctr, mu2, ls2, a2, lp2, &act_draws1, 1u);
        if (rvalid && i == 0) {
          act[(size_t(num_steps) + step) * R + rr] = a2;
          logp[(size_t(num_steps) + step) * R + rr] = lp2;
        }
        a = __builtin_fmaf(pw, a2, a);                   // (k_policy_pair_act's cmd: THE combination)
      }
    }
    pctr += 1u;
    // ---- Env.step: k_rollout_loop's step ---------------------------------------------------------------------------
    bool on_a = false, on_b = false, on_any = false, on_both = false;
    if (junction_on) {
      const unsigned on_b_m = sm_in(x, jb_in - look, jb_in) & (jf << 31);
      const unsigned on_a_m = sm_in(x, ja_in - look, ja_in) & (jf << 30);
      on_b = sm_true(on_b_m);
      on_a = sm_true(on_a_m);
      on_any = sm_true(on_a_m | on_b_m);
      on_both = sm_true(on_a_m & on_b_m);
    }
    const unsigned on_edge_u = 1u ^ (gate_u & (seg_internal >> k));
    const unsigned commanded_u = (on_edge_u & cmd_other) | cmd_rl;
    const bool commanded = commanded_u != 0u;
    T acc;
    {
      if (any_noise) {
        if (__ballot(noisy && (nctr & 3u) == 0u) != 0ull) {
          if (noisy && (nctr & 3u) == 0u)
            gauss4<T>(s.seed_lo, s.seed_hi, s.rep0 + uint32_t(rr), uint32_t(ii), nctr >> 2, g4, s.noise_exact != 0);
        }
      }
      T ai = idm_fast<DELTA4, FASTC>(T(v), T(vl), h, has, ic);
      if (any_noise) {
        const T an = ai + sl.noise * g4[0];
        ai = noisy ? an : ai;
        g4[0] = g4[1]; g4[1] = g4[2]; g4[2] = g4[3];
      }
      const T arl = hmin(hmax(T(a), clip_lo), clip_hi);
      acc = rl_lane ? arl : (sim_lane ? T(0) : ai);
    }
    X next_vel = xmax(v + X(acc) * dt, X(0));
    X vc = v + (next_vel - v) * ramp;
    X v_new = vc;
    if (need_sumo) {
      X v_sumo = sumo_fast<FASTC>(v, vl, h, has, dt, sc);
      vc = xmin(vc, sm1_lane ? v_sumo : X(3.0e38));
      vc = xmin(vc, v + adt_c);
      vc = xmax(vc, v - ddt_c);
      v_new = commanded ? vc : v_sumo;
    }
    if (junction_on) {
      if (__ballot(on_any) != 0ull) {
        const X line = on_b ? jb_in - x : ja_in - x;
        X cap = sumo_fast<FASTC>(v, X(0), T(line), true, dt, sc);
        cap = on_any ? cap : X(3.0e38);
        if (__ballot(on_both) != 0ull) {
          const X cap_a = sumo_fast<FASTC>(v, X(0), T(ja_in - x), true, dt, sc);
          cap = xmin(cap, on_both ? cap_a : X(3.0e38));
        }
        const bool cap_applies = (sm1_u | (commanded_u ^ 1u)) != 0u;
        v_new = xmin(v_new, cap_applies ? cap : X(3.0e38));
      }
    }
    X x_new = x + v_new * dt;
    x_new = wrap_down(x_new, Lv);
    prev_v = v;
    last_acc = acc;
    x = x_new;
    v = v_new;
    tcount += 1;
    nctr += 1u;
    // the segment cursor (k_rollout_loop advances it by compares; the position decides the segment either way)
    if (__ballot((x < c_st) || (x >= c_next)) != 0ull) cursor();
    snapshot();
    unsigned f2_ = sm_lt(h, crash_gap) >> 31;
    if (junction_on) {
      f2_ |= (sm_in(x, za_lo, za_hi) >> 31) << 1;
      f2_ |= (sm_in(x, zb_lo, zb_hi) >> 31) << 2;
    }
    f2_ |= (sm_lt(v, X(-100)) >> 31) << 3;
    if (junction_on) f2_ |= junction_flags(x, v) << 4;
    f2_ &= valid_bits;
    f2_ = seg_or<SEG>(f2_);
    jf = (f2_ >> 4) & 3u;
    // (the multi-agent head sees no crash: multiagent/base.py:188-190)
    const bool crashed = HEAD != 2 && ((f2_ | ((f2_ >> 1) & (f2_ >> 2))) & 1u) != 0u;
    const bool bad = (((f2_ >> 3) & 1u) != 0u) || crashed;
    // ---- reward (the block form's transposed_sum is seg_sum's tree) --------------------------------------------------
    T reward;
    if (HEAD == 1) {                                               // wave_attenuation.py:113-139
      const T racc = seg_sum<SEG>(valid ? T(v) : T(0));
      // (k_rollout_loop sums |clip(a)| over the lanes of the RL columns: one column, one non-zero term -- the term itself)
      const T racc2 = tabs(hmin(hmax(T(a), clip_lo), clip_hi));
      const T mean_v = divc(racc, d_N);
      const T mean_a = divc(racc2, d_nrl);
      reward = divc(T(4.0) * mean_v, d_20);
      if (mean_a > T(0)) reward = reward + T(4) * (T(0) - mean_a);
      reward = bad ? T(0) : reward;
    } else {                                                       // rewards.py:6-59 (AccelEnv, MultiAgentAccelPOEnv)
      const T dv = valid ? T(v) - target_v : T(0);
      const T cost = tsqrt(seg_sum<SEG>(dv * dv));
      reward = divc(tmax(max_cost - cost, T(0)), d_mc);
      reward = bad ? T(0) : reward;
    }
    const uint8_t dflag = done_flag(tcount >= s.step_limit, crashed);
    if (rvalid && i == 0) {
      rew[size_t(step) * R + rr] = reward;
      done[size_t(step) * R + rr] = dflag;
    }
    // ---- Env.reset of a finished episode (masked fs_reset_dev: the placement; the noise stream runs on) ---------------
    const bool fin = reset_done && dflag != 0;
    if (__ballot(fin) != 0ull) {
      if (fin) {
        x = s.init_pos[idx];
        v = s.init_vel[idx];
        tcount = 0;
      }
      cursor();
      snapshot();
      jf = junction_on ? seg_or<SEG>(junction_flags(x, v) & valid_bits) : 0u;
    }
    observe(obs + (size_t(step + 1) * R + rr) * obs_dim);
  }

  if (valid) {
    s.pos[idx] = x;
    s.vel[idx] = v;
    if (s.track_aux && num_steps > 0) {
      s.prev_vel[idx] = prev_v;
      s.accel[idx] = last_acc;
    }
    if (ii == 0) {
      s.time[rr] = tcount;
      pv.ctr[rr] = pctr;
      if (any_noise) s.noise_ctr[rr] = nctr;
    }
  }
}

template <int HEAD, bool DELTA4, bool FASTC>
__global__ __launch_bounds__(256) void k_loop_policy(DevView<float> s, PolicyView pv, int num_steps, int reset_done,
                                                     float* __restrict__ obs, float* __restrict__ act,
                                                     float* __restrict__ logp, float* __restrict__ rew,
                                                     uint8_t* __restrict__ done) {
  loop_policy_body<HEAD, DELTA4, FASTC, false, 0>(s, pv, pv, 0.0f, num_steps, reset_done, obs, act, logp, rew, done);
}

// fs_policy.greedy on this family: the same body with policy_sample<1> (the mean action), a kernel of its own so that the
// sampling instantiations above keep their names and their code
template <int HEAD, bool DELTA4, bool FASTC>
__global__ __launch_bounds__(256) void k_greedy_loop_policy(DevView<float> s, PolicyView pv, int num_steps, int reset_done,
                                                            float* __restrict__ obs, float* __restrict__ act,
                                                            float* __restrict__ logp, float* __restrict__ rew,
                                                            uint8_t* __restrict__ done) {
  loop_policy_body<HEAD, DELTA4, FASTC, false, 1>(s, pv, pv, 0.0f, num_steps, reset_done, obs, act, logp, rew, done);
}

// ---- TWO policies on one RL vehicle (AdversarialAccelEnv on the figure eight: the reference's adversarial_figure_eight.py
// maps the agents 'av' and 'adversary' to a policy each) ---------------------------------------------------------------
// Both networks read the replica's observation; the av draws from the single-agent stream (column 0x40000000, its seed),
// the adversary from column 0x40000000 + 1 keyed by ITS seed (equal seeds still give independent draws), both at the
// replica's counter -- the handle's, shared by the two policies (pv.ctr == pv2.ctr), advancing by ONE per step.  The
// vehicle receives cmd = fmaf(perturb_weight, a_adv, a_av): the one float32 expression that defines the combination
// (flow/envs/multiagent/adversarial_accel.py: av_action + perturb_weight * adv_action); clipping stays where fs_step_dev
// does it.

// eager form: obs [R, in_dim] -> act / logp [2, R] (plane 0 the av, plane 1 the adversary), cmd [R]; a row of 16 lanes is
// one replica, as in k_policy_act
template <int ROW>     // (a template so that every object of the library may include this header)
__global__ __launch_bounds__(256) void k_policy_pair_act(PolicyView pv, PolicyView pv2, float pw, int R, uint32_t rep0,
                                                         const float* __restrict__ obs, float* __restrict__ act,
                                                         float* __restrict__ logp, float* __restrict__ cmd) {
  __shared__ PolicyLds L, L2;
  policy_load(pv, &L, threadIdx.x, blockDim.x);
  policy_load(pv2, &L2, threadIdx.x, blockDim.x);
  const int lane = threadIdx.x & 63, j = lane & 15;
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int rr = r < R ? r : R - 1;
  const uint32_t c0 = pv.ctr[rr];
  float ia, ib;
  policy_wide_inputs(obs + size_t(rr) * pv.in_dim, pv.in_dim, j, ia, ib);
  float mu, ls, a, lp, mu2, ls2, a2, lp2;
  policy_eval<ROW, true>(pv, &L, j, ia, ib, 0.0f, mu, ls);
  policy_eval<ROW, true>(pv2, &L2, j, ia, ib, 0.0f, mu2, ls2);
  policy_sample(pv, rep0 + uint32_t(rr), c0, mu, ls, a, lp, nullptr, 0u);
  policy_sample(pv2, rep0 + uint32_t(rr), c0, mu2, ls2, a2, lp2, nullptr, 1u);
  if (r < R && j == 0) {
    act[r] = a;
    act[size_t(R) + r] = a2;
    logp[r] = lp;
    logp[size_t(R) + r] = lp2;
    cmd[r] = __builtin_fmaf(pw, a2, a);
    pv.ctr[r] = c0 + 1u;
  }
}

// fused form: K x (pair act -> Env.step(cmd) [-> reset of a finished episode]) on a segment-table loop, AccelEnv head:
// loop_policy_body<0, ., ., PAIR>; the mapping is k_loop_policy's (a row of 16 lanes per replica, four replicas per wave,
// 16 per workgroup).  obs [K+1, R, 2 N], act / logp [2, K, R], rew / done [K, R].  LDS: two PolicyLds and the segment
// tables, about 28 KB per workgroup.
template <bool DELTA4, bool FASTC>
__global__ __launch_bounds__(256) void k_loop_policy_pair(DevView<float> s, PolicyView pv, PolicyView pv2, float pw,
                                                          int num_steps, int reset_done, float* __restrict__ obs,
                                                          float* __restrict__ act, float* __restrict__ logp,
                                                          float* __restrict__ rew, uint8_t* __restrict__ done) {
  // (the flag per policy, read at run time: the pair kernels keep their registers with it, tests/test_policy_pair_codegen.py)
  loop_policy_body<0, DELTA4, FASTC, true, -1>(s, pv, pv2, pw, num_steps, reset_done, obs, act, logp, rew, done);
}

// the action-vector AccelEnv head in the loop (fs_last_kernel "k_loop_policy<AccelVec>"): loop_policy_body<0, ., ., ., ., VEC>;
// obs [K+1, R, 2 N], act [K, R, num_rl], logp / rew / done [K, R].  fs_policy.greedy is read at run time.
template <bool DELTA4, bool FASTC>
__global__ __launch_bounds__(256) void k_loop_policy_vec(DevView<float> s, PolicyView pv, int num_steps, int reset_done,
                                                         float* __restrict__ obs, float* __restrict__ act,
                                                         float* __restrict__ logp, float* __restrict__ rew,
                                                         uint8_t* __restrict__ done) {
  loop_policy_body<0, DELTA4, FASTC, false, -1, true>(s, pv, pv, 0.0f, num_steps, reset_done, obs, act, logp, rew, done);
}

}  // namespace fs
