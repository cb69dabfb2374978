// flowsim_sim.h -- host side of libflowsim.so shared by its translation units: the handle (SimBase / Sim<T>),
// allocation, table upload, kernel choice (Sim<T>::launch_steps).  The library is compiled as several objects
// (flow_amd/build.py): flowsim.hip holds the C ABI, validation and everything but the kernel launches; flowsim_part.hip
// is compiled once per (precision, lanes-per-replica) pair and holds the Sim<T>::launch_* of that width with the step
// kernels they instantiate (defined in flowsim_launch.h, which only the parts include).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "flowsim.h"
#include "flowsim_kernels.h"
#include "flowsim_open.h"
#include "flowsim_pair.h"
#include "flowsim_fig8.h"
#include "flowsim_ringrl.h"
#include "flowsim_policy.h"
#include "flowsim_wide.h"
#include "flowsim_queue_consts.h"
#include "flowsim_snap.h"


namespace fsim {

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(FS_ERR_HIP, std::string(#expr) + " failed: " + hipGetErrorString(e_));   \
  } while (0)

// the arguments of one step launch, as every launch_* takes them
struct StepArgs {
  int num_steps;
  const uint8_t* mask;
  const float* actions;
  size_t act_stride;
  float* obs;
  float* rew;
  uint8_t* done;
  int obs_every_step;
};

template <int N>
using Int = std::integral_constant<int, N>;

// a run-time switch as a template argument: f(std::true_type()) if b, else f(std::false_type())
template <typename F>
auto pick(bool b, F&& f) {
  return b ? f(std::true_type()) : f(std::false_type());
}

struct SimBase {
  virtual ~SimBase() {}
  fs_config cfg{};
  std::vector<fs_vehicle_spec> veh;
  std::vector<fs_segment> segs;
  std::vector<fs_inflow> inflows;
  std::vector<fs_cell> obs_cells, act_cells;
  std::vector<int32_t> obs_perm;
  std::vector<uint8_t> init_alive;
  int obs_dim = 0;
  int act_dim = 0;
  int seg = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // host-API staging buffers (device)
  float* d_actions = nullptr;
  float* d_obs = nullptr;
  float* d_rew = nullptr;
  uint8_t* d_done = nullptr;
  uint8_t* d_mask = nullptr;
  float* d_dump = nullptr;      // scratch words the idle lanes of k_rollout_idm store to
  std::vector<void*> allocs;
  int after_reset = 0;          // open networks: the next zero-step launch follows a reset (update(reset=True))
  bool force_generic = false;   // FLOWSIM_FORCE_GENERIC=1: never take the specialised kernels (tests)
  bool no_fastdiv = false;      // FLOWSIM_NO_FASTDIV=1: keep the IEEE division sequence in k_rollout_idm
  bool f16s = false;            // FS_F16S: the state between launches is kept as halves (DevView::st16)
  bool mixed = false;           // FS_MIXED: float64 state, float32 controller arithmetic (k_rollout_pair<double>)
  bool no_pair = false;         // FLOWSIM_NO_PAIR=1: keep k_rollout_idm (one vehicle per lane) for the float rollout
  bool pair_generic_n = false;  // FLOWSIM_PAIR_GENERIC_N=1: keep k_rollout_pair where k_rollout_pair_n would run (A/B, tests)
  bool pair_n_always = false;   // FLOWSIM_PAIR_N_ALWAYS=1: k_rollout_pair_n also for launches shorter than PAIR_N_MIN_STEPS (tests)
  static constexpr int PAIR_N_MIN_STEPS = 512;
  bool kernel_detail = false;   // FLOWSIM_KERNEL_DETAIL=1: fs_last_kernel names the vehicle-count-specialised entry ("[n11]")
  bool no_loop_kernel = false;  // FLOWSIM_NO_LOOP_KERNEL=1: keep the generic k_steps for segment-table loops (tests)
  bool no_loop_full = false;    // FLOWSIM_NO_LOOP_FULL=1: keep the run-time-flag instantiation of k_rollout_loop (tests)
  bool no_ring_rl = false;      // FLOWSIM_NO_RING_RL=1: keep the generic k_steps for IDM + RL rings (tests)
  bool no_mask_skip = false;    // FLOWSIM_NO_MASK_SKIP=1: a masked k_steps_open / k_steps_wide launch steps every wave (A/B, tests)
  bool no_queue = false;        // FLOWSIM_NO_QUEUE=1: keep k_steps_open / k_steps_wide for the open networks (tests)
  bool snap_copies = false;     // FLOWSIM_SNAPSHOT_COPIES=1: an unmasked fs_snapshot_dev / fs_restore_dev is one hipMemcpyAsync per field (A/B)
  double* d_ep_scratch = nullptr;   // k_episode_stats: ticket and partials (flowsim_learn.h), allocated by its first launch
  double* d_adv_scratch = nullptr;  // k_adv_stats: ticket and partial sums (flowsim_learn.h), allocated by its first launch
  unsigned* d_mb_ticket = nullptr;  // k_ppo_minibatch: the ticket its workgroups draw (zero between launches), allocated by its first launch
  int* d_qflag = nullptr;       // k_drop_queue: bit 0 = a path held more than its 64 lanes (the launch's results are invalid)
  bool qflag_armed = false;     // a queue-order launch ran since the flag was last read
  // after a stream synchronisation: did a queue-order launch overflow a path?  (sticky: the handle is unusable then)
  int check_qflag() {
    if (!qflag_armed || !d_qflag) return FS_OK;
    int f = 0;
    HIP_TRY(hipMemcpy(&f, d_qflag, sizeof(int), hipMemcpyDeviceToHost));
    if (f != 0)
      return fail(FS_ERR_UNSUPPORTED, "k_drop_queue: a path of the lane-drop network held more than 64 vehicles (or more than 8 "
                                      "arrived in one sub-step): the results of this handle are invalid -- create it "
                                      "with FLOWSIM_NO_QUEUE=1 (slot-order kernels)");
    qflag_armed = false;
    return FS_OK;
  }
  bool has_user_ctrl = false;   // a FS_CTRL_USER slot: only a library built with the user's controller may launch it
  const char* last_kernel = "";  // family of the step kernel the last launch_steps call chose (fs_last_kernel)
  // after a kernel launch: its launch error, if any
  int launched() {
    HIP_TRY(hipGetLastError());
    return FS_OK;
  }

  virtual int launch_steps(int num_steps, const uint8_t* mask, const float* actions, size_t act_stride,
                           float* obs, float* rew, uint8_t* done, int obs_every_step) = 0;
  virtual int launch_reset(const uint8_t* mask) = 0;
  // policy in the loop (flowsim_policy.h): obs == nullptr selects the eager form (act only)
  virtual int launch_policy(const fs_policy* pol, int num_steps, int reset_done, const float* obs_in, float* obs,
                            float* act, float* logp, float* rew, uint8_t* done) = 0;
  // two policies on one RL vehicle (fs_policy_pair_*): obs == nullptr selects the eager form (act, logp, cmd)
  virtual int launch_policy_pair(const fs_policy* av, const fs_policy* adv, float pw, int num_steps, int reset_done,
                                 const float* obs_in, float* obs, float* act, float* logp, float* cmd, float* rew,
                                 uint8_t* done) = 0;
  // policy populations (fs_population_*): `probe` != 0 runs the checks alone (fs_population_granule: nothing launches)
  virtual int launch_population(const fs_policy* pol, const fs_population* pop, int probe, int num_steps, int reset_done,
                                const float* obs_in, float* obs, float* act, float* logp, float* rew, uint8_t* done) = 0;
  std::string last_kernel_pop;     // (the storage of a population launch's fs_last_kernel name)
  unsigned* d_es_ticket = nullptr; // k_es_grad: the tickets its workgroups draw (zero between launches), allocated by its first launch
  uint32_t* d_pol_ctr = nullptr;   // [R] actions sampled so far per replica (the policy's draw counters)
  // ---- snapshots (flowsim_snap.h; include/flowsim.h fs_snapshot_info): the table Sim<T>::init builds once
  fs::SnapTable snap{};
  size_t snap_bytes = 0;           // the device blob
  uint64_t snap_layout = 0;        // fingerprint of everything the blob's layout depends on
  uint64_t snap_nonce = 0;         // this handle's: fs_restore_dev takes blobs of this handle only (snap_mirrors_out says why)
  // The host mirrors of device state (h_ring_len behind the divisor proofs, neg_speed_possible, init_vel_negative) must
  // cover whatever a restore brings back.  fs_snapshot_dev notes them (out), fs_restore_dev widens the handle's by what
  // was noted (in): host work only, no HIP call.  A blob of ANOTHER handle has no note here, hence the nonce; fs_restore
  // (host blob) rebuilds the mirrors from the blob's contents instead (blob).
  virtual void snap_mirrors_out() = 0;
  virtual void snap_mirrors_in() = 0;
  virtual void snap_mirrors_blob(const char* dev_part) = 0;
  virtual int get_state(int field, void* dst, size_t bytes) = 0;
  virtual int set_state(int field, const void* src, size_t bytes) = 0;
  virtual int add_vehicle(int replica, int slot, int route, double x, double speed) = 0;
};

template <typename T>
struct Sim : SimBase {
  fs::DevView<T> dv{};
  fs::OpenView<T> ov{};        // open networks (FS_NET_MERGE) only
  fs::QueueConsts qc{};        // the queue-order kernels' view of the network (flowsim_queue.h)
  bool open_net = false;
  std::vector<T> h_len;        // vehicle lengths (host copy, for FS_FIELD_HEADWAY)
  std::vector<T> h_ring_len;   // ring lengths (host copy, for the divisor verification)

  template <typename U>
  int dev_alloc(U** out, size_t count) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, (count ? count : 1) * sizeof(U)));
    allocs.push_back(p);
    *out = static_cast<U*>(p);
    return FS_OK;
  }

  template <typename U>
  int upload(const U** out, const std::vector<U>& host) {
    U* p = nullptr;
    int rc = dev_alloc(&p, host.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(p, host.data(), host.size() * sizeof(U), hipMemcpyHostToDevice));
    *out = p;
    return FS_OK;
  }

  int init() {
    const int R = cfg.num_replicas, N = cfg.num_vehicles;
    const size_t RN = size_t(R) * N;
    int rc;
    if ((rc = dev_alloc(&dv.pos, RN))) return rc;
    if ((rc = dev_alloc(&dv.vel, RN))) return rc;
    if ((rc = dev_alloc(&dv.prev_vel, RN))) return rc;
    if ((rc = dev_alloc(&dv.accel, RN))) return rc;
    if ((rc = dev_alloc(&dv.ctrl_state, RN))) return rc;
    if ((rc = dev_alloc(&dv.lane, RN))) return rc;
    if ((rc = dev_alloc(&dv.last_lc, RN))) return rc;
    {
      std::vector<int32_t> il(RN, 0);
      if (cfg.init_lane)
        for (size_t e = 0; e < RN; ++e) il[e] = cfg.init_lane[e];
      if ((rc = upload(&dv.init_lane, il))) return rc;
    }
    if ((rc = dev_alloc(&dv.time, size_t(R)))) return rc;
    if ((rc = dev_alloc(&dv.sort_key, RN))) return rc;
    dv.sort_vehicles = cfg.sort_vehicles;
    dv.obs_perm = nullptr;
    if (!obs_perm.empty()) {
      if ((rc = upload(&dv.obs_perm, obs_perm))) return rc;
    }
    if ((rc = dev_alloc(&dv.noise_ctr, size_t(R)))) return rc;
    HIP_TRY(hipMemset(dv.noise_ctr, 0, size_t(R) * sizeof(uint32_t)));
    HIP_TRY(hipMemset(dv.time, 0, size_t(R) * sizeof(int32_t)));

    std::vector<T> ipos(RN), ivel(RN), rlen(R);
    for (size_t e = 0; e < RN; ++e) {
      ipos[e] = T(cfg.init_pos[e]);
      ivel[e] = cfg.init_vel ? T(cfg.init_vel[e]) : T(veh[e % N].initial_speed);
    }
    for (int r = 0; r < R; ++r) rlen[r] = cfg.ring_length ? T(cfg.ring_length[r]) : T(0);
    for (T vv : ivel) init_vel_negative = init_vel_negative || !(vv >= T(-100));
    neg_speed_possible = init_vel_negative;
    if ((rc = upload(&dv.init_pos, ipos))) return rc;
    if ((rc = upload(&dv.init_vel, ivel))) return rc;
    if ((rc = upload(&dv.ring_len, rlen))) return rc;
    if ((rc = upload(&dv.init_ring_len, rlen))) return rc;
    dv.st16 = nullptr;
    if (f16s && (rc = dev_alloc(&dv.st16, 3 * RN))) return rc;
    h_ring_len = rlen;

    std::vector<int32_t> ctrl(N), fsafe(N), smode(N), rli(N), pisi(N, -1);
    int n_pis = 0;
    std::vector<T> p(size_t(FS_MAX_CTRL_PARAMS) * N), noise(N), delay(N), maxa(N), maxd(N), len(N), stau(N),
        sgap(N), smax(N);
    int flags = 0;
    bool all_idm = true, idm_set = true;
    for (int i = 0; i < N; ++i) {
      const fs_vehicle_spec& v = veh[i];
      ctrl[i] = v.controller;
      fsafe[i] = v.fail_safe;
      smode[i] = v.speed_mode;
      rli[i] = v.rl_index;
      for (int k = 0; k < FS_MAX_CTRL_PARAMS; ++k) p[size_t(k) * N + i] = T(v.p[k]);
      noise[i] = T(v.noise);
      delay[i] = T(v.delay);
      maxa[i] = T(v.max_accel);
      maxd[i] = T(v.max_decel);
      len[i] = T(v.length);
      stau[i] = T(v.sumo_tau);
      sgap[i] = T(v.sumo_min_gap);
      smax[i] = T(v.sumo_max_speed);
      if (v.controller == FS_CTRL_BCM || v.controller == FS_CTRL_USER) flags |= fs::FLAG_NEED_FOLLOWER;
      if (v.controller == FS_CTRL_USER) has_user_ctrl = true;
      if (v.controller == FS_CTRL_NONLOCAL_FOLLOWER_STOPPER) flags |= fs::FLAG_NEED_MEAN;
      if (v.controller == FS_CTRL_LAC) flags |= fs::FLAG_HAS_LAC;
      if (v.controller == FS_CTRL_PISATURATION) {
        flags |= fs::FLAG_HAS_LAC;
        pisi[i] = n_pis++;
      }
      if (v.noise > 0 && v.controller != FS_CTRL_SIM && v.controller != FS_CTRL_RL) flags |= fs::FLAG_HAS_NOISE;
      if (v.fail_safe != FS_FAILSAFE_NONE) flags |= fs::FLAG_HAS_FAILSAFE;
      if (v.controller == FS_CTRL_SIM || v.controller == FS_CTRL_RL || (v.speed_mode & 1) || cfg.junction_mode)
        flags |= fs::FLAG_NEED_SUMO;
      if (v.speed_mode & 6) flags |= fs::FLAG_NEED_SUMO;
      if (v.controller == FS_CTRL_SIM || v.controller == FS_CTRL_RL || cfg.junction_mode) sumo_beyond_speed_mode = true;
      if (v.speed_mode & 7) speed_mode_any = true;
      if (v.controller == FS_CTRL_SIM) any_sim = true;
      if (v.controller != FS_CTRL_IDM) all_idm = false;
      if (v.controller != FS_CTRL_IDM && v.controller != FS_CTRL_RL && v.controller != FS_CTRL_SIM) idm_set = false;
    }
    loop_div_ok = true;      // premises of div_core in k_rollout_loop: s0 and minGap keep the dividends out of the tiny range
    for (int i = 0; i < N; ++i)
      loop_div_ok = loop_div_ok && float(veh[i].sumo_min_gap) >= 1e-3f && float(veh[i].sumo_min_gap) <= 1e6f &&
                    (veh[i].controller != FS_CTRL_IDM || (float(veh[i].p[5]) >= 1e-3f && float(veh[i].p[5]) <= 1e6f));
    loop_delta4 = true;
    for (int i = 0; i < N; ++i) loop_delta4 = loop_delta4 && (veh[i].controller != FS_CTRL_IDM || veh[i].p[4] == 4.0);
    if (loop_delta4) flags |= fs::FLAG_DELTA4;
    // premises of the open-network kernels' div_core forms (flowsim_kernels.h idm_fd / sumo_speed_fd)
    open_div_ok = loop_div_ok && (cfg.speed_limit <= 0 ||        // (0: no limit)
                                  (float(cfg.speed_limit) >= 9.5367431640625e-07f && float(cfg.speed_limit) <= 1048576.0f));
    for (int i = 0; i < N; ++i) {
      auto in_range = [](float c) { return c >= 9.5367431640625e-07f && c <= 1048576.0f; };      // [2^-20, 2^20]
      open_div_ok = open_div_ok && in_range(float(veh[i].sumo_max_speed)) &&
                    in_range(2.0f * std::sqrt(float(veh[i].max_accel) * float(veh[i].max_decel))) &&
                    (veh[i].controller != FS_CTRL_IDM ||
                     (in_range(float(veh[i].p[0])) && in_range(2.0f * std::sqrt(float(veh[i].p[2]) * float(veh[i].p[3])))));
    }
    {
      bool no_ctrl = true;
      for (int i = 0; i < N; ++i) no_ctrl = no_ctrl && (veh[i].controller == FS_CTRL_SIM || veh[i].controller == FS_CTRL_RL);
      if (no_ctrl) flags |= fs::FLAG_NO_FLOW_CTRL;
    }
    if (all_idm) flags |= fs::FLAG_ALL_IDM;
    if (idm_set) flags |= fs::FLAG_IDM_SET;
    delta4 = all_idm;
    for (int i = 0; i < N; ++i) delta4 = delta4 && (veh[i].p[4] == 4.0);
    h_len = len;
    if ((rc = upload(&dv.ctrl, ctrl))) return rc;
    if ((rc = upload(&dv.failsafe, fsafe))) return rc;
    if ((rc = upload(&dv.speed_mode, smode))) return rc;
    if ((rc = upload(&dv.rl_index, rli))) return rc;
    if ((rc = upload(&dv.pis_index, pisi))) return rc;
    dv.n_pis = n_pis;
    dv.pis_H = int(38.0 / cfg.sim_step) - 1;          // velocity_controllers.py:221
    if (dv.pis_H < 1) dv.pis_H = 1;
    if ((rc = dev_alloc(&dv.pis_hist, size_t(R) * (n_pis ? n_pis : 1) * (n_pis ? dv.pis_H : 1)))) return rc;
    if ((rc = dev_alloc(&dv.pis_n, size_t(R) * (n_pis ? n_pis : 1)))) return rc;
    HIP_TRY(hipMemset(dv.pis_n, 0, size_t(R) * (n_pis ? n_pis : 1) * sizeof(int32_t)));
    if ((rc = upload(&dv.p, p))) return rc;
    if ((rc = upload(&dv.noise, noise))) return rc;
    if ((rc = upload(&dv.delay, delay))) return rc;
    if ((rc = upload(&dv.max_accel, maxa))) return rc;
    if ((rc = upload(&dv.max_decel, maxd))) return rc;
    if ((rc = upload(&dv.length, len))) return rc;
    if ((rc = upload(&dv.sumo_tau, stau))) return rc;
    if ((rc = upload(&dv.sumo_min_gap, sgap))) return rc;
    if ((rc = upload(&dv.sumo_max_speed, smax))) return rc;

    dv.R = R;
    dv.N = N;
    dv.num_rl = cfg.num_rl;
    dv.env = cfg.env;
    dv.integrator = cfg.integrator;
    dv.sims_per_step = cfg.sims_per_step;
    dv.junction_mode = cfg.junction_mode;
    dv.clip_actions = cfg.clip_actions;
    dv.evaluate = cfg.evaluate;
    dv.track_aux = cfg.track_aux;
    dv.num_lanes = cfg.num_lanes < 1 ? 1 : cfg.num_lanes;
    dv.lane_change_mode = cfg.lane_change_mode;
    dv.last_lc_quirk = cfg.last_lc_quirk;
    dv.noise_exact = cfg.noise_exact != 0 ? 1 : 0;
    dv.lc_duration = T(cfg.lane_change_duration);
    {  // ML7: autonomous lane changing of the non-RL vehicles on a multi-lane ring
      std::vector<int32_t> lca(N, 0);
      int any_lc = 0;
      for (int i = 0; i < N; ++i) {
        lca[i] = (veh[i].lane_change_mode & 0x55) != 0 && veh[i].controller != FS_CTRL_RL;
        any_lc |= lca[i];
      }
      if ((rc = upload(&dv.lc_auto, lca))) return rc;
      dv.lc_enabled = (cfg.network == FS_NET_RING && cfg.num_lanes > 1 && any_lc) ? 1 : 0;
      dv.lc_cooldown = cfg.lane_change_cooldown_steps > 0 ? cfg.lane_change_cooldown_steps : 1;
      dv.lc_min_gain = T(cfg.lane_change_min_gain);
    }
    dv.nseg = cfg.num_segments;
    dv.seg_internal = 0u;
    for (int k = 0; k < FS_MAX_SEGMENTS; ++k) {
      const bool in = k < cfg.num_segments;
      dv.seg_start[k] = in ? T(segs[k].start) : T(0);
      dv.seg_flow_start[k] = in ? T(segs[k].flow_start) : T(0);
      dv.seg_flow_slope[k] = in ? T(segs[k].flow_slope) : T(0);
      if (in && segs[k].internal) dv.seg_internal |= (1u << k);
    }
    dv.junction_on = cfg.junction.enabled;
    dv.ja_in = T(cfg.junction.a_in);
    dv.ja_out = T(cfg.junction.a_out);
    dv.jb_in = T(cfg.junction.b_in);
    dv.jb_out = T(cfg.junction.b_out);
    dv.j_lookahead = T(cfg.junction.lookahead);
    dv.j_time_gap = T(cfg.junction.time_gap);
    dv.za_lo = T(cfg.junction.za_lo);
    dv.za_hi = T(cfg.junction.za_hi);
    dv.zb_lo = T(cfg.junction.zb_lo);
    dv.zb_hi = T(cfg.junction.zb_hi);
    if (cfg.horizon < 0) {
      dv.step_limit = INT_MAX;
    } else {
      long long lim = (long long)cfg.sims_per_step * ((long long)cfg.warmup_steps + cfg.horizon);
      dv.step_limit = lim > INT_MAX ? INT_MAX : int(lim);
    }
    dv.flags = flags;
    dv.seed_lo = uint32_t(cfg.seed & 0xFFFFFFFFull);
    dv.seed_hi = uint32_t(cfg.seed >> 32);
    dv.rep0 = uint32_t(cfg.replica_offset);
    dv.dt = T(cfg.sim_step);
    dv.ramp = T(cfg.slowdown_ramp);
    dv.jlen = T(cfg.junction_length);
    dv.crash_gap = T(cfg.crash_gap);
    dv.max_speed = T(cfg.max_speed);
    dv.target_velocity = T(cfg.target_velocity);
    {  // np.linalg.norm([target_velocity] * N) evaluated in double (rewards.py:50-51)
      double ss = 0.0;
      for (int i = 0; i < N; ++i) ss += cfg.target_velocity * cfg.target_velocity;
      dv.max_cost = T(std::sqrt(ss));
    }
    dv.max_cost_tab = nullptr;
    if (cfg.env == FS_ENV_MULTI_WAVE_ATTENUATION_PO) {
      // the reward's vehicle count changes from step to step: np.linalg.norm([target_velocity] * n) for n = 0 .. N
      std::vector<T> tab(size_t(N) + 1);
      double ss = 0.0;
      for (int n = 0; n <= N; ++n) {
        tab[n] = T(std::sqrt(ss));
        ss += cfg.target_velocity * cfg.target_velocity;
      }
      if ((rc = upload(&dv.max_cost_tab, tab))) return rc;
    }
    dv.act_lo = T(cfg.action_low);
    dv.act_hi = T(cfg.action_high);
    dv.po_max_length = T(cfg.po_max_length);

    open_net = (cfg.network == FS_NET_MERGE || cfg.network == FS_NET_BOTTLENECK);
    if (open_net && (rc = init_open())) return rc;

    // host-API staging
    if ((rc = dev_alloc(&d_actions, size_t(R) * (act_dim > 0 ? act_dim : 1)))) return rc;
    if ((rc = dev_alloc(&d_obs, size_t(R) * obs_dim))) return rc;
    if ((rc = dev_alloc(&d_rew, size_t(R)))) return rc;
    if ((rc = dev_alloc(&d_done, size_t(R)))) return rc;
    if ((rc = dev_alloc(&d_mask, size_t(R)))) return rc;
    if ((rc = dev_alloc(&d_dump, size_t(256)))) return rc;
    if ((rc = launch_reset(nullptr))) return rc;
    if (open_net) HIP_TRY(hipMemsetAsync(ov.episode, 0xFF, size_t(R) * sizeof(int32_t), stream));
    if ((rc = policy_counters())) return rc;      // (allocated here, not by the first policy launch: the table holds its address)
    return build_snapshot_table();
  }

  // ---- snapshots: every device array a kernel or an fs_* call writes after fs_create (DESIGN.md 4.3 lists what is in,
  // what is out and why); [R][row] each, in the blob at multiples of 16 bytes
  int build_snapshot_table() {
    const size_t R = size_t(dv.R), N = size_t(dv.N), t = sizeof(T), F = FS_MAX_INFLOWS;
    snap.n = 0;
    snap.R = dv.R;
    size_t off = 0;
    bool fits = true;
    auto add = [&](unsigned tag, const void* p, size_t row) {
      if (!p || row == 0) return;
      if (snap.n >= fs::SNAP_MAX_FIELDS || row > 0xFFFFFFFFull) { fits = false; return; }
      snap.e[snap.n++] = fs::SnapEntry{static_cast<char*>(const_cast<void*>(p)), (unsigned long long)off, unsigned(row), tag};
      off = (off + R * row + 15) & ~size_t(15);
    };
    add(fs::SNAP_POS, dv.pos, N * t);
    add(fs::SNAP_VEL, dv.vel, N * t);
    add(fs::SNAP_PREV_VEL, dv.prev_vel, N * t);
    add(fs::SNAP_ACCEL, dv.accel, N * t);
    add(fs::SNAP_CTRL_STATE, dv.ctrl_state, N * t);
    add(fs::SNAP_LANE, dv.lane, N * 4);
    add(fs::SNAP_LAST_LC, dv.last_lc, N * 4);
    add(fs::SNAP_TIME, dv.time, 4);
    add(fs::SNAP_SORT_KEY, dv.sort_key, N * t);
    add(fs::SNAP_NOISE_CTR, dv.noise_ctr, 4);
    add(fs::SNAP_RING_LEN, dv.ring_len, t);
    add(fs::SNAP_INIT_RING_LEN, dv.init_ring_len, t);
    if (dv.st16) {                                   // FS_F16S: three planes [R,N] of halves
      add(fs::SNAP_ST16_HI, dv.st16, N * 2);
      add(fs::SNAP_ST16_LO, dv.st16 + R * N, N * 2);
      add(fs::SNAP_ST16_VEL, dv.st16 + 2 * R * N, N * 2);
    }
    if (dv.n_pis > 0) {
      add(fs::SNAP_PIS_HIST, dv.pis_hist, size_t(dv.n_pis) * dv.pis_H * t);
      add(fs::SNAP_PIS_N, dv.pis_n, size_t(dv.n_pis) * 4);
    }
    add(fs::SNAP_INIT_POS, dv.init_pos, N * t);
    add(fs::SNAP_INIT_VEL, dv.init_vel, N * t);
    add(fs::SNAP_INIT_LANE, dv.init_lane, N * 4);
    if (open_net) {
      add(fs::SNAP_SEQ, ov.seq, N * 4);
      add(fs::SNAP_ORIGIN, ov.origin, N * 4);
      add(fs::SNAP_FOLL, ov.foll, N * 4);
      add(fs::SNAP_FOLL_H, ov.foll_h, N * t);
      add(fs::SNAP_CTL_SEQ, ov.ctl_seq, N * 4);
      add(fs::SNAP_LEAD, ov.lead, N * 4);
      add(fs::SNAP_HEADWAY, ov.headway, N * t);
      add(fs::SNAP_VMAX, ov.vmax, N * t);
      add(fs::SNAP_ARRIVED_RL, ov.arrived_rl, N * 4);
      add(fs::SNAP_ARR_HIST, ov.arr_hist, 20 * 4);
      add(fs::SNAP_COUNTERS, ov.counters, 8 * 4);
      add(fs::SNAP_EMITTED, ov.emitted, F * 4);
      add(fs::SNAP_GENERATED, ov.generated, F * 4);
      add(fs::SNAP_FLOW_PER, ov.flow_per(dv.R), F * 8);
      add(fs::SNAP_INIT_FLOW_PER, ov.init_flow_per(dv.R), F * 8);
      add(fs::SNAP_EPISODE, ov.episode, 4);
    }
    add(fs::SNAP_POL_CTR, d_pol_ctr, 4);
    add(fs::SNAP_OBS, d_obs, size_t(obs_dim) * 4);
    if (!fits) return fail(FS_ERR_UNSUPPORTED, "fs_create: the snapshot table does not hold this handle's fields");
    snap_bytes = off;
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint64_t v : {uint64_t(FS_ABI_VERSION), uint64_t(cfg.precision), uint64_t(dv.R), uint64_t(dv.N), uint64_t(cfg.network),
                       uint64_t(cfg.env), uint64_t(obs_dim), uint64_t(act_dim), uint64_t(snap.n)})
      h = fs::snap_hash(h, v);
    for (int k = 0; k < snap.n; ++k) h = fs::snap_hash(fs::snap_hash(h, snap.e[k].tag), snap.e[k].row);
    snap_layout = h;
    static std::mutex mu;
    static uint64_t serial = 0;
    {
      std::lock_guard<std::mutex> lock(mu);
      ++serial;
      uint64_t z = serial * 0x9E3779B97F4A7C15ull + uint64_t(reinterpret_cast<uintptr_t>(this));     // splitmix64
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      snap_nonce = (z ^ (z >> 31)) | 1ull;           // never 0
    }
    return FS_OK;
  }

  std::vector<T> snap_ring_len;       // the distinct ring lengths (current and pending) of every snapshot taken so far
  bool snap_out_stale = true;         // h_ring_len changed since snap_ring_len last took it in
  bool snap_in_stale = false;         // snap_ring_len may hold a length h_ring_len lacks
  bool snap_neg = false, snap_init_neg = false;
  static void sorted_union(std::vector<T>& into, const std::vector<T>& more) {
    into.insert(into.end(), more.begin(), more.end());
    std::sort(into.begin(), into.end());
    into.erase(std::unique(into.begin(), into.end()), into.end());
  }
  void ring_mirror_changed() {
    fastdiv_state = -1;
    ringrl_fast_state = -1;
    snap_out_stale = true;
    snap_in_stale = true;
  }
  void snap_mirrors_out() override {
    if (snap_out_stale) {
      sorted_union(snap_ring_len, h_ring_len);
      snap_out_stale = false;
    }
    snap_neg = snap_neg || neg_speed_possible;
    snap_init_neg = snap_init_neg || init_vel_negative;
  }
  void snap_mirrors_in() override {
    if (snap_in_stale) {
      std::vector<T> have = h_ring_len;
      sorted_union(have, {});
      std::vector<T> all = have;
      sorted_union(all, snap_ring_len);
      if (all.size() != have.size()) {             // a snapshot holds a length set_state has since replaced
        h_ring_len = all;
        fastdiv_state = -1;
        ringrl_fast_state = -1;
        snap_out_stale = true;
      }
      snap_in_stale = false;
    }
    neg_speed_possible = neg_speed_possible || snap_neg;
    init_vel_negative = init_vel_negative || snap_init_neg;
  }
  // fs_restore: the device part of a host blob of this layout, whatever handle it came from
  void snap_mirrors_blob(const char* dev_part) override {
    const size_t R = size_t(dv.R);
    for (int k = 0; k < snap.n; ++k) {
      const fs::SnapEntry& en = snap.e[k];
      const T* vals = reinterpret_cast<const T*>(dev_part + en.off);
      const size_t count = R * en.row / sizeof(T);
      if (en.tag == fs::SNAP_RING_LEN || en.tag == fs::SNAP_INIT_RING_LEN) {
        sorted_union(h_ring_len, std::vector<T>(vals, vals + count));
        ring_mirror_changed();
      } else if (en.tag == fs::SNAP_VEL || en.tag == fs::SNAP_INIT_VEL) {
        bool neg = false;
        for (size_t e = 0; e < count; ++e) neg = neg || !(vals[e] >= T(-100));
        neg_speed_possible = neg_speed_possible || neg;
        if (en.tag == fs::SNAP_INIT_VEL) init_vel_negative = init_vel_negative || neg;
      }
    }
  }

  // ---- open networks: per-slot bookkeeping arrays, route tables, inflow table ------------------
  int init_open() {
    const int R = cfg.num_replicas, N = cfg.num_vehicles;
    const size_t RN = size_t(R) * N;
    int rc;
    if ((rc = dev_alloc(&ov.seq, RN))) return rc;
    if ((rc = dev_alloc(&ov.origin, RN))) return rc;
    if ((rc = dev_alloc(&ov.foll, RN))) return rc;
    if ((rc = dev_alloc(&ov.ctl_seq, RN))) return rc;
    if ((rc = dev_alloc(&ov.lead, RN))) return rc;
    if ((rc = dev_alloc(&ov.arrived_rl, RN))) return rc;
    if ((rc = dev_alloc(&ov.foll_h, RN))) return rc;
    if ((rc = dev_alloc(&ov.headway, RN))) return rc;
    if ((rc = dev_alloc(&ov.vmax, RN))) return rc;
    if ((rc = dev_alloc(&ov.arr_hist, size_t(R) * 20))) return rc;
    if ((rc = dev_alloc(&ov.counters, size_t(R) * 8))) return rc;
    // one allocation: emitted, generated (int32 each), then the current and the pending periods (float64 each; 8-byte
    // aligned behind 64 R bytes of counters) -- OpenView::flow_per() says why the periods have no pointers of their own
    if ((rc = dev_alloc(&ov.emitted, size_t(R) * FS_MAX_INFLOWS * 6))) return rc;
    ov.generated = ov.emitted + size_t(R) * FS_MAX_INFLOWS;
    if ((rc = dev_alloc(&ov.episode, size_t(R)))) return rc;
    if ((rc = dev_alloc(&d_qflag, size_t(1)))) return rc;
    HIP_TRY(hipMemset(d_qflag, 0, sizeof(int)));
    HIP_TRY(hipMemset(ov.episode, 0xFF, size_t(R) * sizeof(int32_t)));     // -1: fs_create's own reset below is not an episode
    HIP_TRY(hipMemset(ov.ctl_seq, 0xFF, RN * sizeof(int32_t)));            // rl_veh starts empty (a reset keeps it, O2)
    HIP_TRY(hipMemset(ov.origin, 0xFF, RN * sizeof(int32_t)));
    HIP_TRY(hipMemset(ov.counters, 0, size_t(R) * 8 * sizeof(int32_t)));
    if ((rc = upload(&ov.init_alive, init_alive))) return rc;
    std::vector<int32_t> st(N);
    int n_rl_slots = 0;
    for (int i = 0; i < N; ++i) {
      st[i] = veh[i].type;
      if (veh[i].controller == FS_CTRL_RL) ++n_rl_slots;
    }
    if ((rc = upload(&ov.slot_type, st))) return rc;
    std::vector<T> tab(size_t(fs::TAB_ROWS) * 64, T(0));
    for (int n = 0; n <= 64; ++n) {               // np.linalg.norm([target] * n) in double (rewards.py:50-51)
      double ss = 0.0;
      for (int i = 0; i < n; ++i) ss += cfg.target_velocity * cfg.target_velocity;
      if (n < 64) tab[size_t(fs::TAB_MAX_COST) * 64 + n] = T(std::sqrt(ss));
      else ov.max_cost_full = T(std::sqrt(ss));
    }
    ov.n_inflows = cfg.num_inflows;
    ov.ma_apply_actions = cfg.ma_apply_actions;
    ov.n_rl_slots = n_rl_slots;
    std::vector<double> ftd(3 * 64, 0.0);
    std::vector<int32_t> fti(3 * 64, 0);
    ov.n_prob = 0;
    for (int f = 0; f < cfg.num_inflows; ++f) {
      ftd[f] = inflows[f].period;
      if (inflows[f].probability >= 0.0) {
        // a probabilistic inflow keeps, in the place of its period, -(threshold + 1): a vehicle is generated in a
        // sub-step when the sub-step's 32-bit Philox draw is below threshold = floor(p * sim_step * 2^32)
        double thr = std::floor(inflows[f].probability * cfg.sim_step * 4294967296.0);
        if (thr > 4294967295.0) thr = 4294967295.0;
        ftd[f] = -(thr + 1.0);
        ov.n_prob += 1;
      }
      ftd[64 + f] = inflows[f].begin;
      ftd[128 + f] = inflows[f].end;
      fti[f] = inflows[f].type;
      fti[64 + f] = inflows[f].route;
      fti[128 + f] = inflows[f].number;
      int first = 0;                               // the type's parameters: those of its first slot
      for (int i = N - 1; i >= 0; --i)
        if (veh[i].type == inflows[f].type) first = i;
      // same operations, in T, as oracle/opennet.py _insert
      // (the lane-drop network has ONE route table: its "routes" are entry lanes, -1 = a random one)
      const int rs = (cfg.network == FS_NET_MERGE && inflows[f].route == 1) ? 1 : 0;
      tab[size_t(fs::TAB_FL_XDEP) * 64 + f] = T(cfg.route_start[rs]) + T(inflows[f].depart_pos);
      tab[size_t(fs::TAB_FL_VDEP) * 64 + f] = T(inflows[f].depart_speed);
      tab[size_t(fs::TAB_FL_MINGAP) * 64 + f] = T(veh[first].sumo_min_gap);
      tab[size_t(fs::TAB_FL_TAU) * 64 + f] = T(veh[first].sumo_tau);
      tab[size_t(fs::TAB_FL_TWOSQRT) * 64 + f] = T(2) * std::sqrt(T(veh[first].max_accel) * T(veh[first].max_decel));
    }
    ov.dt_d = cfg.sim_step;
    for (int r = 0; r < 2; ++r) {
      ov.nseg[r] = 0;
      ov.seg_internal[r] = 0u;
    }
    for (const fs_segment& sg : segs) {
      const int r = sg.route, k = ov.nseg[r]++;
      tab[size_t(fs::TAB_SEG_START) * 64 + r * 16 + k] = T(sg.start);
      tab[size_t(fs::TAB_SEG_FLOW) * 64 + r * 16 + k] = T(sg.flow_start);
      tab[size_t(fs::TAB_SEG_SLOPE) * 64 + r * 16 + k] = T(sg.flow_slope);
      if (sg.internal) ov.seg_internal[r] |= (1u << k);
    }
    if ((rc = upload(&ov.lane_tab, tab))) return rc;
    if ((rc = upload(&ov.flow_tab_d, ftd))) return rc;
    {   // every replica starts on the handle's schedule, and returns to it at a reset until told otherwise
      std::vector<double> per(size_t(R) * FS_MAX_INFLOWS, 0.0);
      for (int r = 0; r < R; ++r)
        for (int f = 0; f < cfg.num_inflows; ++f) per[size_t(r) * FS_MAX_INFLOWS + f] = ftd[f];
      HIP_TRY(hipMemcpy(ov.flow_per(R), per.data(), per.size() * sizeof(double), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(ov.init_flow_per(R), per.data(), per.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = upload(&ov.flow_tab_i, fti))) return rc;
    {   // lane drops + bottleneck heads
      const bool bn = cfg.network == FS_NET_BOTTLENECK;
      ov.m1 = T(bn ? cfg.merge1_x : cfg.merge_x);
      ov.m2 = T(bn ? cfg.merge2_x : cfg.merge_x);
      ov.zip_d = T(bn ? cfg.zipper_distance : 0.0);
      ov.speed_limit = cfg.speed_limit > 0 ? T(cfg.speed_limit) : T(3.0e38);
      ov.n_obs_cells = int(obs_cells.size());
      ov.n_act_cells = int(act_cells.size());
      ov.obs_window = cfg.obs_outflow_window;
      ov.rew_window = cfg.reward_outflow_window;
      ov.out_norm = T(cfg.outflow_norm > 0 ? cfg.outflow_norm : 2000.0);
      ov.obs_dim = obs_dim;
      std::vector<T> ct(6 * 64, T(0));
      std::vector<int32_t> cti(3 * 64, 0);
      // consecutive cells that differ only in the lane (lane l, l+1, ...) form one group
      auto group = [&](const std::vector<fs_cell>& cells, int row_start, int row_lo, int row_hi, int row_i) {
        int g = 0;
        for (size_t c = 0; c < cells.size();) {
          size_t e = c + 1;
          while (e < cells.size() && cells[e].edge_start == cells[c].edge_start && cells[e].lo == cells[c].lo &&
                 cells[e].hi == cells[c].hi && cells[e].last_segment == cells[c].last_segment &&
                 cells[e].lane == cells[c].lane + int(e - c))
            ++e;
          ct[size_t(row_start) * 64 + g] = T(cells[c].edge_start);
          ct[size_t(row_lo) * 64 + g] = T(cells[c].lo);
          ct[size_t(row_hi) * 64 + g] = T(cells[c].hi);
          cti[size_t(row_i) * 64 + g] = int(c) | (int(e - c) << 8) | (cells[c].lane << 16) |
                                         ((cells[c].last_segment ? 1 : 0) << 24);
          ++g;
          c = e;
        }
        return g;
      };
      ov.n_obs_groups = group(obs_cells, fs::CELL_OBS_START, fs::CELL_OBS_LO, fs::CELL_OBS_HI, 0);
      ov.n_act_groups = group(act_cells, fs::CELL_ACT_START, fs::CELL_ACT_LO, fs::CELL_ACT_HI, 1);
      // row 2: the groups that lie on route segment k (an edge and its groups share the start coordinate), so that a
      // vehicle only tries the lane-segments of its own edge
      ov.obs_span = ov.act_span = 0;
      auto ranges = [&](int n_groups, int row_start, int shift) {
        int span = 0;
        for (size_t k = 0; k < segs.size() && k < 64; ++k) {
          int first = -1, cnt = 0;
          for (int g = 0; g < n_groups; ++g)
            if (double(ct[size_t(row_start) * 64 + g]) == double(T(segs[k].start)) && !segs[k].internal) {
              if (first < 0) first = g;
              ++cnt;
            }
          if (first >= 0) cti[size_t(2) * 64 + k] |= (first | (cnt << 8)) << shift;
          span = cnt > span ? cnt : span;
        }
        return span;
      };
      ov.obs_span = ranges(ov.n_obs_groups, fs::CELL_OBS_START, 0);
      ov.act_span = ranges(ov.n_act_groups, fs::CELL_ACT_START, 16);
      ov.track_followers = cfg.track_followers;
      ov.mask_skip = no_mask_skip ? 0 : 1;
      std::vector<int32_t> lca(N, 0);
      int any_lc = 0;
      for (int i = 0; i < N; ++i) {
        lca[i] = (veh[i].lane_change_mode & 0x55) != 0;
        any_lc |= lca[i];
      }
      if ((rc = upload(&ov.lc_auto, lca))) return rc;
      ov.lc_enabled = bn && any_lc;
      ov.lc_cooldown = cfg.lane_change_cooldown_steps;
      ov.lc_min_gain = T(cfg.lane_change_min_gain);
      if ((rc = upload(&ov.cell_tab, ct))) return rc;
      if ((rc = upload(&ov.cell_tab_i, cti))) return rc;
    }
    {   // flowsim_queue.h: the junction-internal stretches of each route as intervals, the one vehicle length
      qc.ok = (cfg.network == FS_NET_MERGE) ? 1 : 0;
      for (int r = 0; r < 2; ++r)
        for (int j = 0; j < 2; ++j) qc.in_lo[r][j] = qc.in_hi[r][j] = 3.0e38f;
      int n_int[2] = {0, 0}, k_of[2] = {0, 0};
      for (int r = 0; r < 2; ++r)
        for (int q = 0; q < 6; ++q) { qc.seg_start[r][q] = 3.0e38f; qc.seg_flow[r][q] = 0.0f; qc.seg_slope[r][q] = 0.0f; }
      for (size_t i = 0; i < segs.size() && qc.ok; ++i) {
        const int r = segs[i].route;
        if (r < 0 || r > 1) { qc.ok = 0; break; }
        const int k = k_of[r]++;
        if (k >= 6) { qc.ok = 0; break; }
        qc.seg_start[r][k] = float(segs[i].start);
        qc.seg_flow[r][k] = float(segs[i].flow_start);
        qc.seg_slope[r][k] = float(segs[i].flow_slope);
        if (!segs[i].internal) continue;
        if (n_int[r] >= 2) { qc.ok = 0; break; }
        float hi = 3.0e38f;                              // the next segment of the same route starts where this one ends
        for (size_t j = i + 1; j < segs.size(); ++j)
          if (segs[j].route == r) { hi = float(segs[j].start); break; }
        qc.in_lo[r][n_int[r]] = k == 0 ? -3.0e38f : float(segs[i].start);
        qc.in_hi[r][n_int[r]] = hi;
        n_int[r] += 1;
      }
      qc.veh_len = N > 0 ? float(veh[0].length) : 5.0f;          // (k_drop_queue checks the lengths itself: dropq_ok)
      for (int i = 0; i < N; ++i)
        if (float(veh[i].length) != qc.veh_len) qc.ok = 0;
    }
    ov.merge_x = T(cfg.merge_x);
    ov.box_in = T(cfg.box_in);
    ov.end_x = T(cfg.end_x);
    ov.net_length = T(cfg.net_length);
    dv.nseg = 0;                                   // the closed-loop segment table is not used
    return FS_OK;
  }

  // ---- exact division by launch constants (flowsim_kernels.h div_const) --------------------
  // The 3-operation reciprocal sequence is enabled only if, for every divisor the rollout kernel
  // will use (v0 and 2*sqrt(a*b) of every slot, the loop length of every replica), it
  // reproduces x / c for ALL 2^23 float mantissas of x.  Checked lazily, once per handle state;
  // set_state of the ring lengths invalidates it.  Only the float kernels use it.
  // rewards.py:46 ("any speed < -100 -> reward 0") can only fire on speeds put there from outside (see
  // k_rollout_idm): true while the initial speeds or an upload since the last full reset held such a value
  bool neg_speed_possible = false;
  bool init_vel_negative = false;
  int fastdiv_state = -1;       // -1 unknown, 0 no, 1 yes
  static bool fastdiv_exact_for(float c) {
    if (!(c > 0.0f) || !std::isfinite(c)) return false;
    // process-wide memo: the answer depends on the divisor only
    static std::mutex mu;
    static std::map<uint32_t, bool> memo;
    uint32_t key;
    std::memcpy(&key, &c, 4);
    {
      std::lock_guard<std::mutex> lock(mu);
      auto it = memo.find(key);
      if (it != memo.end()) return it->second;
    }
    const bool ok = fastdiv_exact_uncached(c);
    std::lock_guard<std::mutex> lock(mu);
    memo[key] = ok;
    return ok;
  }
  static bool fastdiv_exact_uncached(float c) {
    const float rc = 1.0f / c;
    for (uint32_t m = 0; m < (1u << 23); ++m) {
      const uint32_t bits = 0x3F800000u | m;
      float x;
      std::memcpy(&x, &bits, 4);
      const float q0 = x * rc;
      const float r = std::fmaf(-q0, c, x);
      if (std::fmaf(r, rc, q0) != x / c) return false;
    }
    return true;
  }
  // The divisor proofs share this routine: collect(cs) checks the kernel's premises (false: one fails) and gathers its
  // distinct divisors.  The answer is cached in `state`.
  template <typename Collect>
  bool prove_divisors(int& state, Collect collect) {
    if (state >= 0) return state == 1;
    state = 0;
    std::vector<float> cs;
    if (!collect(cs)) return false;
    for (float c : cs)
      if (!fastdiv_exact_for(c)) return false;
    state = 1;
    return true;
  }
  static void add_divisor(std::vector<float>& cs, float c) {
    if (std::find(cs.begin(), cs.end(), c) == cs.end()) cs.push_back(c);
  }
  void add_idm_divisors(std::vector<float>& cs, int i) const {     // v0 and 2 sqrt(a b) of slot i's IDM
    add_divisor(cs, float(veh[i].p[0]));
    add_divisor(cs, 2.0f * std::sqrt(float(veh[i].p[2]) * float(veh[i].p[3])));
  }
  void add_sumo_divisors(std::vector<float>& cs, int i) const {    // SUMO's max speed and 2 sqrt(a b) of slot i
    add_divisor(cs, float(veh[i].sumo_max_speed));
    add_divisor(cs, 2.0f * std::sqrt(float(veh[i].max_accel) * float(veh[i].max_decel)));
  }
  // the loop length of every replica; more than `limit` distinct divisors are too many to verify cheaply
  bool add_ring_divisors(std::vector<float>& cs, size_t limit) const {
    for (T b : h_ring_len) {                    // host copy: no HIP call on the launch path
      const float L = float(b) + 4.0f * float(dv.jlen);
      if (!(L >= 1.0f)) return false;        // keeps x = 0 or x >= ulp(L)/2 out of the tiny range
      add_divisor(cs, L);
      if (cs.size() > limit) return false;
    }
    return true;
  }
  static bool gap_in(double g, float lo) { return float(g) >= lo && float(g) <= 1e6f; }    // the s0 / minGap premises

  bool fastdiv_ok() {
    if ((!std::is_same<T, float>::value && !mixed) || force_generic || no_fastdiv) return false;
    return prove_divisors(fastdiv_state, [&](std::vector<float>& cs) {
      for (int i = 0; i < dv.N; ++i) {            // per-slot IDM divisors and the s0 >= 1e-3 premise
        add_idm_divisors(cs, i);
        if (!gap_in(veh[i].p[5], 1e-3f)) return false;
        if (speed_mode_any) {                     // sumo_acc_pair's divisors and its minGap >= 1e-3 premise
          add_sumo_divisors(cs, i);
          if (!gap_in(veh[i].sumo_min_gap, 1e-3f)) return false;
        }
      }
      return add_ring_divisors(cs, 80);
    });
  }

  // k_rollout_loop<..., FULL>: its controller divisions by launch constants are div_const -- every divisor proven
  int loop_fastc_state = -1;
  bool loop_fastc_ok() {
    if (!(std::is_same<T, float>::value || mixed) || no_fastdiv) return false;
    return prove_divisors(loop_fastc_state, [&](std::vector<float>& cs) {
      if (!loop_div_ok) return false;               // s0 / minGap in [1e-3, 1e6]: tiny dividends cannot matter
      for (int i = 0; i < dv.N; ++i) {
        if (veh[i].controller == FS_CTRL_IDM) add_idm_divisors(cs, i);
        add_sumo_divisors(cs, i);
      }
      return true;
    });
  }

  // k_ring_pair<..., FAST> (flowsim_ringrl.h): exponent 4 and the exact reciprocal divisions -- every divisor proven.
  // The premises on s0 / minGap are weaker than fastdiv_ok()'s (>= 0 instead of >= 1e-3): s* = s0 + max(0, dyn) below
  // 2^-60 makes q = s* / h < 2^-50, whose square vanishes against every non-zero 1 - (v/v0)^4 (>= 2^-24) and, where that
  // term is exactly zero, gives an acceleration too small to move a speed near v0 -- so an inexact quotient there
  // cannot change a result; from 2^-60 up div_core's operands are inside its proven range (|h| in [1e-3, L]).
  int ringrl_fast_state = -1;
  bool ringrl_fast_ok() {
    if (no_fastdiv || force_generic) return false;
    return prove_divisors(ringrl_fast_state, [&](std::vector<float>& cs) {
      for (int i = 0; i < dv.N; ++i) {
        if (veh[i].controller == FS_CTRL_IDM) {
          if (veh[i].p[4] != 4.0 || !gap_in(veh[i].p[5], 0.0f)) return false;
          add_idm_divisors(cs, i);
        }
        add_sumo_divisors(cs, i);
        if (!gap_in(veh[i].sumo_min_gap, 0.0f)) return false;
      }
      return add_ring_divisors(cs, 96);
    });
  }

  // the specialisations for the headline configuration (see flowsim_kernels.h)
  bool delta4 = false;
  bool loop_div_ok = false, loop_delta4 = false, open_div_ok = false;
  bool sumo_beyond_speed_mode = false;   // FLAG_NEED_SUMO for more than speed-mode bits (Sim / RL slots, junction mode)
  bool speed_mode_any = false;           // some slot carries a speed-mode clamp (bits 0-2)
  bool any_sim = false;                  // some slot is a SimCarFollowingController

  // ---- the conditions of launch_steps' kernels (each is asked only after those before it in launch_steps failed) ----
  // allow_speed_mode: the caller's kernel evaluates the speed-mode clamps itself (k_rollout_pair<..., SM = true>)
  bool fast_ok(const StepArgs& a, bool allow_speed_mode = false, bool allow_noise = false) const {
    const int f = dv.flags;
    const bool sumo_free = !(f & fs::FLAG_NEED_SUMO) || (allow_speed_mode && !sumo_beyond_speed_mode);
    const bool noise_free = !(f & fs::FLAG_HAS_NOISE) || allow_noise;
    return (f & fs::FLAG_ALL_IDM) && !(f & fs::FLAG_HAS_FAILSAFE) && noise_free && sumo_free &&
           dv.env == FS_ENV_ACCEL && !dv.evaluate && dv.sims_per_step == 1 && dv.integrator == FS_EULER &&
           !dv.junction_mode && !dv.track_aux && a.mask == nullptr && a.num_steps > 0 && !force_generic &&
           dv.nseg == 0 && !dv.junction_on && !dv.sort_vehicles && dv.obs_perm == nullptr;
  }

  // the merge network in queue order (flowsim_queue.h): float32, IDM / RL / Sim slots, either merge head (MergePOEnv,
  // MultiAgentMergePOEnv), scheduled inflows, every replica stepping
  bool queue_ok(const StepArgs& a) const {
    if (!std::is_same<T, float>::value || !open_net || cfg.network != FS_NET_MERGE || no_queue || force_generic) return false;
    if ((dv.env != FS_ENV_MERGE_MA && dv.env != FS_ENV_MERGE_PO) || !(dv.flags & fs::FLAG_IDM_SET) || !open_div_ok || ov.n_prob > 0) return false;
    if (!(dv.flags & fs::FLAG_DELTA4) || (dv.flags & fs::FLAG_HAS_FAILSAFE) || dv.integrator != FS_EULER || !qc.ok) return false;
    if (a.mask != nullptr || a.num_steps < 1 || dv.N > 64) return false;
    for (const fs_inflow& f : inflows)
      if (f.route < 0 || f.route > 1) return false;
    return true;
  }
  // the lane-drop network in queue order (flowsim_dropq.h): one wave per entry lane, every vehicle on SUMO's model
  bool dropq_ok(const StepArgs& a) const {
    if (!std::is_same<T, float>::value || !open_net || cfg.network != FS_NET_BOTTLENECK || no_queue || force_generic) return false;
    if (cfg.num_paths != 4 || ov.lc_enabled || ov.track_followers || ov.n_prob > 0 || !open_div_ok) return false;
    if (!(dv.flags & fs::FLAG_NO_FLOW_CTRL) || dv.integrator != FS_EULER) return false;
    if (dv.env != FS_ENV_BOTTLENECK_DV && dv.env != FS_ENV_BOTTLENECK) return false;
    if (dv.env == FS_ENV_BOTTLENECK && dv.num_rl > 0 && ov.ma_apply_actions) return false;   // per-vehicle RL accelerations (BottleneckAccelEnv)
    if (a.mask != nullptr || a.num_steps < 1 || dv.N > 256 || ov.nseg[0] > 16 || ov.obs_span > 3 || ov.act_span > 2) return false;
    for (int i = 0; i < dv.N; ++i)
      if (float(veh[i].length) != float(veh[0].length) || veh[i].type < 0 || veh[i].type > 7) return false;
    for (const fs_inflow& f : inflows)
      if (f.route > 3) return false;
    return true;
  }
  // several lanes, or a lane-changing head (flowsim_kernels.h k_steps_ml)
  bool ml_ok() const {
    return dv.num_lanes > 1 || dv.env == FS_ENV_LANE_CHANGE_ACCEL || dv.env == FS_ENV_LANE_CHANGE_ACCEL_PO;
  }
  // closed loops with a segment table (figure eight) in rows of 16 lanes: the rollout kernel of flowsim_fig8.h
  // (FS_MIXED handles: its float64-state instantiation; whatever that does not cover -- resets, masks, warm-up, single
  // vehicles -- steps on the generic float64 kernel, which is the reference's arithmetic)
  bool loop_ok(const StepArgs& a) const {
    const int f = dv.flags;
    const bool ma_loop = std::is_same<T, float>::value && dv.env == FS_ENV_ACCEL_PO_MA;   // MultiAgentAccelPOEnv (multiagent_figure_eight.py)
    const bool head_ok = (dv.env == FS_ENV_ACCEL && !dv.evaluate) || dv.env == FS_ENV_WAVE_ATTENUATION_PO || ma_loop;
    return seg == 16 && (std::is_same<T, float>::value || mixed) && dv.nseg > 0 && (f & fs::FLAG_IDM_SET) &&
           !(f & fs::FLAG_HAS_FAILSAFE) && head_ok && dv.integrator == FS_EULER && dv.sims_per_step == 1 &&
           a.mask == nullptr && !dv.sort_vehicles && dv.obs_perm == nullptr && a.num_steps > 0 &&
           (a.obs_every_step || a.num_steps == 1) && dv.N > 1 && loop_div_ok && !force_generic && !no_loop_kernel;
  }
  // single-lane rings of IDM and RL vehicles, float32 (noise included) or FS_MIXED (flowsim_ringrl.h): the RL
  // experiments' populations and heads, masked and zero-step launches included; the all-IDM AccelEnv rollout keeps
  // k_rollout_pair (pair_ok)
  bool ring_rl_ok(const StepArgs& a) const {
    const int f = dv.flags;
    const bool ma_head = dv.env == FS_ENV_WAVE_ATTENUATION_PO_MA || dv.env == FS_ENV_ACCEL_PO_MA ||
                         dv.env == FS_ENV_MULTI_WAVE_ATTENUATION_PO;                                 // float32 only
    return (std::is_same<T, float>::value || mixed) && dv.nseg == 0 && !dv.junction_on && (f & fs::FLAG_IDM_SET) &&
           !any_sim && !(f & fs::FLAG_HAS_FAILSAFE) && dv.sims_per_step == 1 && dv.integrator == FS_EULER &&
           !dv.junction_mode && !dv.track_aux && !dv.sort_vehicles && dv.obs_perm == nullptr && !dv.evaluate &&
           (dv.env == FS_ENV_ACCEL || dv.env == FS_ENV_WAVE_ATTENUATION_PO || (ma_head && !mixed)) && dv.N >= 2 &&
           (dv.N % 2) == 0 && !force_generic && !no_ring_rl && !pair_ok(a);
  }
  // two vehicles per lane (flowsim_pair.h): float32 (the noisy form too) or FS_MIXED, even N
  bool pair_ok(const StepArgs& a) const {
    return (std::is_same<T, float>::value || mixed) && fast_ok(a, true, std::is_same<T, float>::value) &&
           (a.obs_every_step || a.num_steps == 1) && dv.N >= 2 && (dv.N % 2) == 0 && a.actions == nullptr && !no_pair &&
           size_t(dv.R) * 2 * dv.N * sizeof(float) * 16 < (size_t(1) << 32);   // 32-bit offsets in a block
  }
  // one vehicle per lane (flowsim_kernels.h k_rollout_idm)
  bool rollout_idm_ok(const StepArgs& a) const {
    return fast_ok(a) && a.obs_every_step && dv.N > 1 && a.actions == nullptr &&
           size_t(dv.R) * 2 * dv.N * sizeof(float) < (size_t(1) << 32);   // 32-bit byte offsets inside one step's block
  }

  // ---- the launches, one per kernel family: flowsim_launch.h, compiled into the parts (flowsim_part.hip) ----
  int launch_queue(const StepArgs& a);       // float32 (the queue part)
  int launch_policy_queue(const fs::PolicyView& pv, int num_steps, int reset_done, float* obs, float* act, float* logp,
                          float* rew, uint8_t* done);    // float32 (the queue part): the merge heads' fused policies
  int launch_policy_act_vec(const fs::PolicyView& pv, const float* obs_in, float* act, float* logp);   // (the queue part)
  int launch_policy_act_wide(const fs::PolicyView& pv, const float* obs_in, float* act, float* logp);  // (the queue part)
  int launch_dropq(const StepArgs& a);       // float32 (the queue part)
  template <int W>
  int launch_wide(const StepArgs& a);        // one workgroup of W waves per replica
  // one wave carries 64 / SEG replicas
  template <int SEG>
  int launch_open(const StepArgs& a);
  template <int SEG>
  int launch_ml(const StepArgs& a);
  int launch_loop(const StepArgs& a);        // SEG = 16
  template <int SEG>
  int launch_ring(const StepArgs& a);
  int launch_obs_mixed(const StepArgs& a);   // FS_MIXED
  template <int SEG>
  int launch_pair(const StepArgs& a);
  template <int SEG>
  int launch_idm(const StepArgs& a);
  template <int SEG>
  int launch_k_steps(const StepArgs& a);
  // f(Int<SEG>()): a family's instantiation for this handle's lanes per replica
  template <typename F>
  int per_seg(F&& f) {
    switch (seg) {
      case 8: return f(Int<8>());
      case 16: return f(Int<16>());
      case 32: return f(Int<32>());
      default: return f(Int<64>());
    }
  }

  // The step kernel of a launch, in order of preference.
  int launch_steps(int num_steps, const uint8_t* mask, const float* actions, size_t act_stride, float* obs,
                   float* rew, uint8_t* done, int obs_every_step) override {
    const StepArgs a{num_steps, mask, actions, act_stride, obs, rew, done, obs_every_step};
    if (has_user_ctrl && !fs::kHasUserController)
      return fail(FS_ERR_UNSUPPORTED, "FS_CTRL_USER: this library was built without a user controller "
                                      "(flow_amd.build.build_user / flow_amd.controllers.CompiledController)");
    // a user head (FS_ENV_USER; fs_create has refused it on a library without one) lives in k_steps alone: none of the
    // conditions below admits it, and this line keeps that true when one of them changes
    if (dv.env == FS_ENV_USER) return per_seg([&](auto S) { return launch_k_steps<S>(a); });
    if constexpr (std::is_same<T, float>::value) {
      if (queue_ok(a)) return launch_queue(a);
      if (dropq_ok(a)) return launch_dropq(a);
    }
    if (seg == 128) return launch_wide<2>(a);            // more than 64 slots per replica (lane-drop network)
    if (seg == 256) return launch_wide<4>(a);
    if (open_net) return per_seg([&](auto S) { return launch_open<S>(a); });
    if (ml_ok()) return per_seg([&](auto S) { return launch_ml<S>(a); });
    if (loop_ok(a)) return launch_loop(a);
    if (ring_rl_ok(a)) return per_seg([&](auto S) { return launch_ring<S>(a); });
    if (mixed && num_steps == 0 && dv.nseg == 0) return launch_obs_mixed(a);   // observation of the current state (Env.reset)
    if (mixed && !pair_ok(a) && dv.nseg == 0)
      return fail(FS_ERR_UNSUPPORTED, "FS_MIXED: this launch fits neither mixed kernel (k_rollout_pair / k_ring_pair: "
                                      "single-lane ring, even number of IDM / RL vehicles, AccelEnv or "
                                      "WaveAttenuationPOEnv, track_aux = 0)");
    if (pair_ok(a)) return per_seg([&](auto S) { return launch_pair<S>(a); });
    if (rollout_idm_ok(a)) return per_seg([&](auto S) { return launch_idm<S>(a); });
    return per_seg([&](auto S) { return launch_k_steps<S>(a); });        // k_steps: FAST / CSET / generic
  }

  // policy in the loop (flowsim_policy.h; flowsim_launch.h): the eager policy, the fused policy + step kernels of rings
  // (rows of 16 lanes: 18..32 vehicles) and of segment-table loops (the figure eight: up to 16 vehicles); n_ag agents
  // share the policy on the multi-agent heads (MultiAgentWaveAttenuationPOEnv on rings, MultiAgentAccelPOEnv on loops,
  // MultiAgentMergePOEnv with its actions applied on the merge's queue kernel: k_merge_queue<POLICY>); MergePOEnv's ONE
  // network with num_rl action columns: k_policy_act_vec (eager) and k_merge_policy (fused) up to 6 places, k_policy_act_wide
  // and k_merge_wide_policy with 7 .. 32; BottleneckDesiredVelocityEnv's (more than 32 inputs, up to 64 columns):
  // k_policy_act_wide, eager only; AccelEnv's on a segment-table loop with 2 .. 16 RL vehicles (the figure-eight
  // benchmarks: 2 N inputs, num_rl columns, a row of 16 lanes per replica): k_policy_act_row and k_loop_policy_vec
  int launch_policy_act(const fs::PolicyView& pv, int n_ag, const float* obs_in, float* act, float* logp);
  int launch_policy_row16(const fs::PolicyView& pv, int num_steps, int reset_done, float* obs, float* act, float* logp,
                          float* rew, uint8_t* done);
  int launch_policy_loop16(const fs::PolicyView& pv, int num_steps, int reset_done, float* obs, float* act, float* logp,
                           float* rew, uint8_t* done);
  int launch_policy_act_row16(const fs::PolicyView& pv, const float* obs_in, float* act, float* logp);
  // ---- launch_policy's checks and set-up that fs_policy_pair shares (launch_policy_pair below) ----
  // the model class every policy kernel evaluates
  const char* policy_model_why(const fs_policy* pol) const {
    if (pol->num_hidden < 1 || pol->num_hidden > 3 || pol->hidden_width != 32 || pol->activation != 0)
      return "fs_policy model (1..3 hidden layers of 32 tanh units)";
    if (!pol->weights_dev) return "fs_policy.weights_dev (NULL)";
    return nullptr;
  }
  // AccelEnv with several RL vehicles on a segment-table loop: the handles of the row-per-replica action-vector head
  bool accel_vec() const { return dv.nseg > 0 && dv.env == FS_ENV_ACCEL && dv.num_rl > 1; }
  // ONE RL vehicle on a segment-table loop (k_loop_policy): why this handle / policy is not built, or nullptr.  po_ok:
  // the WaveAttenuationPOEnv head counts (not for two policies); fragment_resets: a fused launch that resets in place;
  // vec_ok: an accel_vec() handle counts too -- ONE network with num_rl = 2 .. 16 action columns (k_policy_act_row,
  // k_loop_policy_vec; not for two policies).  Every refusal of such a handle names FS_ENV_ACCEL and num_rl
  const char* policy_loop_why(const fs_policy* pol, bool po_ok, bool fragment_resets, bool vec_ok = false) const {
    const bool po = po_ok && dv.env == FS_ENV_WAVE_ATTENUATION_PO, accel = dv.env == FS_ENV_ACCEL && !dv.evaluate;
    const bool vec = accel_vec();
    if (vec && (!std::is_same<T, float>::value || mixed))
      return "precision (FS_ENV_ACCEL with num_rl > 1 is FS_F32 only: FS_MIXED / FS_F64 handles are not built)";
    if (!std::is_same<T, float>::value || mixed) return "precision (f32 on segment-table loops)";
    if (seg != 16 || dv.N < 2) return "num_vehicles (9..16: a row of 16 lanes per replica; up to 8 vehicles a replica is laid out in 8 lanes)";
    if (vec && !vec_ok)
      return "env (FS_ENV_ACCEL with num_rl > 1 takes ONE policy with num_rl action columns, fs_policy_act_dev / "
             "fs_policy_rollout_dev: two policies drive AccelEnv with one RL vehicle)";
    if (dv.env == FS_ENV_WAVE_ATTENUATION_PO && dv.num_rl > 1)
      return "env (WaveAttenuationPOEnv with num_rl > 1: the PO head observes one RL vehicle; the action-vector head is "
             "FS_ENV_ACCEL's, num_rl = 2..16)";
    const bool vec_head = vec && accel && dv.num_rl <= fs::FS_POLICY_ROW_VEC_MAX;      // (the action-vector head)
    if (!vec_head && (!(po || accel) || dv.num_rl != 1))
      return po_ok ? "env (WaveAttenuationPOEnv or AccelEnv with one RL vehicle)" : "env (AccelEnv with one RL vehicle)";
    if (pol->obs_dim != (po ? 3 : 2 * dv.N)) return "fs_policy.obs_dim (the environment's observation)";
    if (!(dv.flags & fs::FLAG_IDM_SET) || (dv.flags & fs::FLAG_HAS_FAILSAFE) || dv.sims_per_step != 1 ||
        dv.integrator != FS_EULER || dv.track_aux || dv.sort_vehicles || dv.obs_perm != nullptr || !loop_div_ok ||
        (fragment_resets && cfg.warmup_steps != 0))
      return "configuration (what k_rollout_loop steps: IDM / RL / Sim vehicles, Euler, track_aux = 0; resets inside a "
             "fragment: warmup_steps = 0)";
    return nullptr;
  }
  // the draw counters [R]: allocated (zero) by the first policy launch of the handle
  int policy_counters() {
    if (d_pol_ctr) return FS_OK;
    int rc = dev_alloc(&d_pol_ctr, size_t(dv.R));
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_pol_ctr, 0, size_t(dv.R) * sizeof(uint32_t), stream));
    return FS_OK;
  }
  // the kernels' view of a policy with ONE action column (the action-vector heads scale n_out)
  fs::PolicyView policy_view(const fs_policy* pol) const {
    fs::PolicyView pv;
    pv.w = pol->weights_dev;
    pv.log_std = pol->log_std_dev;
    pv.ctr = d_pol_ctr;
    pv.in_dim = pol->obs_dim;
    pv.num_hidden = pol->num_hidden;
    pv.n_out = pol->log_std_dev ? 1 : 2;
    pv.seed_lo = uint32_t(pol->seed & 0xFFFFFFFFull);
    pv.seed_hi = uint32_t(pol->seed >> 32);
    pv.greedy = pol->greedy != 0 ? 1 : 0;
    pv.pop_stride = pop_stride;
    pv.pop_group = pop_group;
    return pv;
  }
  int launch_policy(const fs_policy* pol, int num_steps, int reset_done, const float* obs_in, float* obs, float* act,
                    float* logp, float* rew, uint8_t* done) override {
    if (!pol || pol->struct_size != sizeof(fs_policy)) return fail(FS_ERR_INVALID, "fs_policy: struct_size mismatch");
    const bool f32_or_mixed = mixed || std::is_same<T, float>::value;
    const bool loop = dv.nseg > 0;                       // a segment-table loop (figure eight) or a ring
    const bool ma = dv.env == FS_ENV_WAVE_ATTENUATION_PO_MA || dv.env == FS_ENV_ACCEL_PO_MA || dv.env == FS_ENV_MERGE_MA;
    const char* why = policy_model_why(pol);
    if (why) {}                                          // (the model class: every head's first check)
    else if (dv.env == FS_ENV_USER) {                    // a user head: the eager k_policy_act only
      const bool shared = fs::kUserObsRlOnly;            // num_rl agents share the policy, one block each
      if (obs != nullptr)
        why = "fs_policy_rollout_dev (FS_ENV_USER: the policy is not fused into a user head's step; the eager "
              "fs_policy_act_dev is built (k_policy_act) -- capture it around the step: VecFlowEnv.capture with a "
              "DevicePolicy)";
      else if (!std::is_same<T, float>::value || mixed)
        why = "precision (FS_ENV_USER: the policy kernels serve float32 handles; FS_F64 handles are not built)";
      else if (dv.num_rl < 1) why = "num_rl (FS_ENV_USER: an RL vehicle)";
      else if (!shared && dv.num_rl != 1)
        why = "num_rl (FS_ENV_USER with OBSERVE = \"all\": one RL vehicle; several RL vehicles share a policy with "
              "OBSERVE = \"rl\")";
      else if (shared && pol->obs_dim != fs::kUserObsPerVehicle)
        why = "fs_policy.obs_dim (FS_ENV_USER with OBSERVE = \"rl\": one agent's block, OBS_PER_VEHICLE)";
      else if (!shared && (pol->obs_dim != obs_dim || obs_dim > 32))
        why = "fs_policy.obs_dim (FS_ENV_USER with OBSERVE = \"all\": the whole observation, fs_obs_dim <= 32)";
    }
    else if (dv.env == FS_ENV_MERGE_PO) {              // ONE network: the whole observation -> num_rl action columns
      if (!std::is_same<T, float>::value || mixed)
        why = "precision (FS_ENV_MERGE_PO is FS_F32 / FS_F16S only: FS_MIXED / FS_F64 handles are not built)";
      else if (dv.num_rl < 1 || dv.num_rl > 32)
        why = "num_rl (FS_ENV_MERGE_PO: 1..32 places; num_rl <= 6 runs k_policy_act_vec / k_merge_policy<PO>, 7..32 "
              "k_policy_act_wide / k_merge_policy<PO,WIDE>)";
      else if (pol->obs_dim != obs_dim && dv.num_rl > fs::FS_POLICY_VEC_MAX)
        why = "fs_policy.obs_dim (FS_ENV_MERGE_PO: a first layer of at most 32 inputs is the num_rl <= 6 head's; this "
              "handle has more places and needs the whole observation, obs_dim = fs_obs_dim = 5 num_rl, with num_rl "
              "output rows next to num_rl free log stds, or 2 num_rl; any other policy can run in torch around the "
              "step, e.g. VecFlowEnv.capture)";
      else if (pol->obs_dim != obs_dim)
        why = "fs_policy.obs_dim (FS_ENV_MERGE_PO: the whole observation, fs_obs_dim = 5 num_rl; the output layer has "
              "num_rl rows next to num_rl free log stds, or 2 num_rl)";
      else if (!queue_ok(StepArgs{num_steps > 0 ? num_steps : 1, nullptr, nullptr, 0, obs, rew, done, 1}))
        why = "configuration (FS_ENV_MERGE_PO: what k_merge_queue steps, Sim::queue_ok: IDM / RL / Sim slots without "
              "fail-safes, one vehicle length, Euler, scheduled inflows only, FLOWSIM_NO_QUEUE unset)";
      else if (obs != nullptr && reset_done && cfg.warmup_steps != 0)
        why = "configuration (FS_ENV_MERGE_PO: resets inside a fragment: warmup_steps = 0)";
    }
    else if (dv.env == FS_ENV_BOTTLENECK_DV) {           // ONE network: the whole observation (33 .. 513) -> num_rl columns
      if (!std::is_same<T, float>::value || mixed)
        why = "precision (FS_ENV_BOTTLENECK_DV is FS_F32 only: k_policy_act_wide is a float32 kernel)";
      else if (obs != nullptr)
        why = "fs_policy_rollout_dev (FS_ENV_BOTTLENECK_DV: the policy is not fused into k_drop_queue; the eager "
              "fs_policy_act_dev is built (k_policy_act_wide) -- capture it around the step: VecFlowEnv.capture with a "
              "DevicePolicy)";
      else if (dv.num_rl < 1 || dv.num_rl > 64)
        why = "num_rl (FS_ENV_BOTTLENECK_DV: 1..64 action cells, one column per lane of a wave)";
      else if (pol->obs_dim != obs_dim)
        why = "fs_policy.obs_dim (FS_ENV_BOTTLENECK_DV: the whole observation, fs_obs_dim = 4 cells + 1; the output "
              "layer has num_rl rows next to num_rl free log stds, or 2 num_rl)";
    }
    else if (dv.env == FS_ENV_MERGE_MA) {                // agent c: the RL slot of column c, present while it holds a vehicle
      if (!ov.ma_apply_actions)
        why = "env (FS_ENV_MERGE_MA with ma_apply_actions = 0: the shipped MultiAgentMergePOEnv never applies an action, "
              "so actions never reach the simulator; roll out open loop instead)";
      else if (!std::is_same<T, float>::value || mixed)
        why = "precision (the multi-agent merge is FS_F32 / FS_F16S only: FS_MIXED / FS_F64 handles are not built)";
      else if (dv.num_rl < 1 || pol->obs_dim * dv.num_rl != obs_dim)
        why = "fs_policy.obs_dim (one agent's block: fs_obs_dim / num_rl)";
      else if (!queue_ok(StepArgs{num_steps > 0 ? num_steps : 1, nullptr, nullptr, 0, obs, rew, done, 1}))
        why = "configuration (what k_merge_queue steps, Sim::queue_ok: IDM / RL / Sim slots without fail-safes, one "
              "vehicle length, Euler, scheduled inflows only, FLOWSIM_NO_QUEUE unset)";
      else if (obs != nullptr && reset_done && cfg.warmup_steps != 0)
        why = "configuration (resets inside a fragment: warmup_steps = 0)";
    }
    else if (ma) {                                       // one policy shared by the num_rl agents of a replica
      if (!std::is_same<T, float>::value || mixed)
        why = "precision (the multi-agent heads are float32 only: FS_MIXED / FS_F64 handles are not built)";
      else if (!loop && dv.env != FS_ENV_WAVE_ATTENUATION_PO_MA)
        why = "env (FS_ENV_ACCEL_PO_MA on a ring: rings take MultiAgentWaveAttenuationPOEnv)";
      else if (loop && dv.env != FS_ENV_ACCEL_PO_MA)
        why = "env (FS_ENV_WAVE_ATTENUATION_PO_MA on a segment-table loop: loops take MultiAgentAccelPOEnv)";
      else if (dv.num_rl < 1 || pol->obs_dim * dv.num_rl != obs_dim)
        why = "fs_policy.obs_dim (one agent's block: fs_obs_dim / num_rl)";
      else if (loop && (seg != 16 || dv.N < 2)) why = "num_vehicles (9..16: a row of 16 lanes per replica; up to 8 vehicles a replica is laid out in 8 lanes)";
      else if (loop && (!(dv.flags & fs::FLAG_IDM_SET) || (dv.flags & fs::FLAG_HAS_FAILSAFE) || dv.sims_per_step != 1 ||
                        dv.integrator != FS_EULER || dv.track_aux || dv.sort_vehicles || dv.obs_perm != nullptr ||
                        !loop_div_ok || (obs != nullptr && reset_done && cfg.warmup_steps != 0)))
        why = "configuration (what k_rollout_loop steps: IDM / RL / Sim vehicles, Euler, track_aux = 0; resets inside a "
              "fragment: warmup_steps = 0)";
      else if (!loop && seg != 32) why = "num_vehicles (18..32: a row of 16 lanes per replica)";
      else if (!loop && (dv.junction_on || dv.num_lanes > 1 || !(dv.flags & fs::FLAG_IDM_SET) || any_sim ||
                         (dv.flags & fs::FLAG_HAS_FAILSAFE) || dv.sims_per_step != 1 || dv.integrator != FS_EULER ||
                         dv.junction_mode || dv.track_aux || dv.sort_vehicles || dv.obs_perm != nullptr || dv.evaluate ||
                         (dv.N % 2) != 0))
        why = "configuration (what k_ring_pair steps: single-lane ring of IDM / RL vehicles, Euler, track_aux = 0)";
    }
    else if (loop) why = policy_loop_why(pol, true, obs != nullptr && reset_done, true);
    else if (!f32_or_mixed) why = "precision (f32 or mixed)";
    else if (seg != 32) why = "num_vehicles (18..32: a row of 16 lanes per replica)";
    else if (dv.env == FS_ENV_MULTI_WAVE_ATTENUATION_PO && (!std::is_same<T, float>::value || mixed))
      why = "precision (FS_ENV_MULTI_WAVE_ATTENUATION_PO: the policy kernels are float32 only)";
    else if ((dv.env != FS_ENV_WAVE_ATTENUATION_PO && dv.env != FS_ENV_MULTI_WAVE_ATTENUATION_PO) || dv.num_rl != 1)
      why = "env (WaveAttenuationPOEnv or MultiWaveAttenuationPOEnv with one RL vehicle)";
    else if (pol->obs_dim != 3) why = "fs_policy.obs_dim (3)";
    else if (dv.nseg != 0 || dv.junction_on || dv.num_lanes > 1 || !(dv.flags & fs::FLAG_IDM_SET) || any_sim ||
             (dv.flags & fs::FLAG_HAS_FAILSAFE) || dv.sims_per_step != 1 || dv.integrator != FS_EULER || dv.junction_mode ||
             dv.track_aux || dv.sort_vehicles || dv.obs_perm != nullptr || dv.evaluate || (dv.N % 2) != 0)
      why = "configuration (what k_ring_pair steps: single-lane ring of IDM / RL vehicles, Euler, track_aux = 0)";
    if (why) {
      std::string msg = std::string("fs_policy: not built for this handle: ") + why;
      if (dv.env == FS_ENV_BOTTLENECK_DV && msg.find("FS_ENV_BOTTLENECK_DV") == std::string::npos)
        msg += " (FS_ENV_BOTTLENECK_DV)";                // (the checks shared by every head: model class, weights)
      return fail(FS_ERR_UNSUPPORTED, msg);
    }
    if (pop_probe) return FS_OK;                         // (fs_population_granule: the checks alone)
    if (int rc = policy_counters()) return rc;
    fs::PolicyView pv = policy_view(pol);
    if (dv.env == FS_ENV_MERGE_PO || dv.env == FS_ENV_BOTTLENECK_DV || accel_vec()) pv.n_out *= dv.num_rl;  // the action-vector heads: num_rl means [and num_rl log stds]
    if constexpr (std::is_same<T, float>::value) {
      const bool po_wide = dv.env == FS_ENV_MERGE_PO && dv.num_rl > fs::FS_POLICY_VEC_MAX;   // 35 .. 160 inputs
      if (dv.env == FS_ENV_MERGE_PO && obs == nullptr && !po_wide) return launch_policy_act_vec(pv, obs_in, act, logp);
      if (dv.env == FS_ENV_BOTTLENECK_DV || (po_wide && obs == nullptr)) return launch_policy_act_wide(pv, obs_in, act, logp);
      if (dv.env == FS_ENV_MERGE_MA || dv.env == FS_ENV_MERGE_PO) {
        if (obs != nullptr) return launch_policy_queue(pv, num_steps, reset_done, obs, act, logp, rew, done);
      }
    }
    if (obs == nullptr && accel_vec()) return launch_policy_act_row16(pv, obs_in, act, logp);     // (launch_policy_loop16 takes the fused form)
    const bool user_shared = dv.env == FS_ENV_USER && fs::kUserObsRlOnly;
    if (obs == nullptr) return launch_policy_act(pv, (ma || user_shared) ? dv.num_rl : 1, obs_in, act, logp);   // eager: the policy alone
    if (loop) return launch_policy_loop16(pv, num_steps, reset_done, obs, act, logp, rew, done);
    return launch_policy_row16(pv, num_steps, reset_done, obs, act, logp, rew, done);
  }

  // ---- policy populations (include/flowsim.h fs_population): launch_policy with a stride and a group in the PolicyView.
  // The kernels that take one -- k_policy_act, k_ring_policy, k_loop_policy -- give a workgroup of 256 lanes to 16 replicas.
  static constexpr int POP_GRANULE = 16;
  long long pop_stride = 0;        // (what policy_view hands the kernels: set for the duration of launch_population)
  int pop_group = 0;
  bool pop_probe = false;
  static long long policy_floats(const fs_policy* pol) {
    const long long n_out = pol->log_std_dev ? 1 : 2;
    return 32ll * pol->obs_dim + 32 + (pol->num_hidden - 1) * (32ll * 32 + 32) + n_out * 32 + n_out;
  }
  int launch_population(const fs_policy* pol, const fs_population* pop, int probe, int num_steps, int reset_done,
                        const float* obs_in, float* obs, float* act, float* logp, float* rew, uint8_t* done) override {
    if (!pol || pol->struct_size != sizeof(fs_policy)) return fail(FS_ERR_INVALID, "fs_population: fs_policy struct_size mismatch");
    if (!probe && (!pop || pop->struct_size != sizeof(fs_population)))
      return fail(FS_ERR_INVALID, "fs_population: struct_size mismatch");
    if (dv.env == FS_ENV_USER)
      return fail(FS_ERR_UNSUPPORTED, "fs_population: not built for FS_ENV_USER (a user head takes one policy through the eager "
                                      "fs_policy_act_dev)");
    if (dv.env == FS_ENV_MERGE_PO || dv.env == FS_ENV_BOTTLENECK_DV)
      return fail(FS_ERR_UNSUPPORTED, "fs_population: not built for the action-vector heads (FS_ENV_MERGE_PO, "
                                      "FS_ENV_BOTTLENECK_DV): their kernels give a wave to a replica and read weights past "
                                      "the workgroup's LDS copy");
    if (dv.env == FS_ENV_MERGE_MA)
      return fail(FS_ERR_UNSUPPORTED, "fs_population: not built for FS_ENV_MERGE_MA (k_merge_queue<POLICY> gives a wave to a replica)");
    if (accel_vec())
      return fail(FS_ERR_UNSUPPORTED, "fs_population: not built for FS_ENV_ACCEL with num_rl > 1 (the action-vector head of "
                                      "k_policy_act_row / k_loop_policy<AccelVec>: policy_floats and the members' stride "
                                      "count one action column)");
    if (!probe) {
      if (pop->members < 1 || pop->group < 1 || pop->reserved != 0)
        return fail(FS_ERR_INVALID, "fs_population: members and group must be at least 1, reserved 0");
      if (pop->group % POP_GRANULE != 0)
        return fail(FS_ERR_INVALID, "fs_population: group is not a multiple of the granule (fs_population_granule: 16 replicas "
                                    "share a workgroup's copy of the weights)");
      if ((long long)pop->members * pop->group != (long long)dv.R)
        return fail(FS_ERR_INVALID, "fs_population: members * group != num_replicas");
    }
    // (what fs_policy_rollout_dev refuses on this handle, with its message, before the stride can be judged: the model class)
    static float probe_buf;        // (fs_population_granule asks about the fused form; launch_policy only tests obs for NULL)
    pop_probe = true;
    int rc = launch_policy(pol, num_steps, reset_done, obs_in, probe ? &probe_buf : obs, act, logp, rew, done);
    pop_probe = false;
    if (rc || probe) return rc;
    if (pop->stride < 0 || (pop->stride != 0 && pop->stride < policy_floats(pol)))
      return fail(FS_ERR_INVALID, "fs_population: stride is smaller than the policy's own size (" +
                                  std::to_string(policy_floats(pol)) + " floats; 0: all members share set 0)");
    pop_stride = pop->stride;
    pop_group = pop->group;
    rc = launch_policy(pol, num_steps, reset_done, obs_in, obs, act, logp, rew, done);
    pop_stride = 0;
    pop_group = 0;
    if (rc) return rc;
    // fs_last_kernel: the family's name with Population among its tags
    std::string name = last_kernel;
    if (!name.empty() && name.back() == '>') name = name.substr(0, name.size() - 1) + ",Population>";
    else name += "<Population>";
    last_kernel_pop = name;
    last_kernel = last_kernel_pop.c_str();
    return FS_OK;
  }

  // two policies, one RL vehicle (fs_policy_pair_act_dev / fs_policy_pair_rollout_dev; flowsim_policy.h k_policy_pair_act,
  // k_loop_policy_pair): what launch_policy's loop branch takes for the AccelEnv head, for BOTH policies; obs == nullptr
  // selects the eager form (act, logp, cmd)
  int launch_policy_pair16(const fs::PolicyView& pv, const fs::PolicyView& pv2, float pw, int num_steps, int reset_done,
                           const float* obs_in, float* obs, float* act, float* logp, float* cmd, float* rew, uint8_t* done);
  int launch_policy_pair(const fs_policy* av, const fs_policy* adv, float pw, int num_steps, int reset_done,
                         const float* obs_in, float* obs, float* act, float* logp, float* cmd, float* rew,
                         uint8_t* done) override {
    if (!av || !adv || av->struct_size != sizeof(fs_policy) || adv->struct_size != sizeof(fs_policy))
      return fail(FS_ERR_INVALID, "fs_policy_pair: fs_policy struct_size mismatch");
    if (!std::isfinite(pw)) return fail(FS_ERR_INVALID, "fs_policy_pair: perturb_weight is not finite");
    const bool resets = obs != nullptr && reset_done;
    const char *why = nullptr, *who = "";
    if (dv.env == FS_ENV_USER) why = "env (FS_ENV_USER: two policies on a user head are not built)";
    else if (dv.nseg == 0) why ="network (a segment-table loop: the figure eight; rings and the open networks take one policy)";
    for (const fs_policy* pol : {av, adv}) {
      if (why) break;
      who = pol == av ? "av: " : "adversary: ";
      if ((why = policy_model_why(pol)) == nullptr) why = policy_loop_why(pol, false, resets);
    }
    if (why) return fail(FS_ERR_UNSUPPORTED, std::string("fs_policy_pair: not built for this handle: ") + who + why);
    if (int rc = policy_counters()) return rc;
    return launch_policy_pair16(policy_view(av), policy_view(adv), pw, num_steps, reset_done, obs_in, obs, act, logp, cmd,
                                rew, done);
  }

  int launch_reset(const uint8_t* mask) override {
    if (mask == nullptr) neg_speed_possible = init_vel_negative;     // every replica back at its initial speeds
    if (open_net) {
      const size_t n_open = size_t(dv.R) * dv.N;
      int blocks_open = int((n_open + 255) / 256);
      if (blocks_open > 2048) blocks_open = 2048;
      hipLaunchKernelGGL((fs::k_reset_open<T>), dim3(blocks_open), dim3(256), 0, stream, dv, ov, mask);
      if (dv.st16) hipLaunchKernelGGL((fs::k_state16_pack<T>), dim3(blocks_open), dim3(256), 0, stream, dv, mask);
      HIP_TRY(hipGetLastError());
      return FS_OK;
    }
    const size_t n = size_t(dv.R) * dv.N;
    int blocks = int((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL((fs::k_reset<T>), dim3(blocks), dim3(256), 0, stream, dv, mask);
    HIP_TRY(hipGetLastError());
    return FS_OK;
  }

  T* field_ptr(int field, size_t* count, bool* writable) {
    const size_t RN = size_t(dv.R) * dv.N;
    *writable = true;
    switch (field) {
      case FS_FIELD_POS: *count = RN; return dv.pos;
      case FS_FIELD_VEL: *count = RN; return dv.vel;
      case FS_FIELD_PREV_VEL: *count = RN; return dv.prev_vel;
      case FS_FIELD_ACCEL: *count = RN; return dv.accel;
      case FS_FIELD_CTRL_STATE: *count = RN; return dv.ctrl_state;
      case FS_FIELD_MAX_SPEED: *count = open_net ? RN : 0; return open_net ? ov.vmax : nullptr;
      case FS_FIELD_RING_LENGTH: *count = size_t(dv.R); return const_cast<T*>(dv.ring_len);
      case FS_FIELD_INIT_RING_LENGTH: *count = size_t(dv.R); return const_cast<T*>(dv.init_ring_len);
      case FS_FIELD_SORT_KEY: *count = RN; return dv.sort_key;
      case FS_FIELD_INIT_POS: *count = RN; return const_cast<T*>(dv.init_pos);
      case FS_FIELD_INIT_VEL: *count = RN; return const_cast<T*>(dv.init_vel);
      default: *count = 0; return nullptr;
    }
  }

  // FS_FIELD_INFLOW_PERIOD / FS_FIELD_INIT_INFLOW_PERIOD: float64 [R, FS_MAX_INFLOWS] whatever the handle's precision
  int inflow_period_check(int field, size_t bytes, const char** name) {
    *name = field == FS_FIELD_INFLOW_PERIOD ? "FS_FIELD_INFLOW_PERIOD" : "FS_FIELD_INIT_INFLOW_PERIOD";
    const std::string n(*name);
    if (!open_net || cfg.num_inflows == 0)
      return fail(FS_ERR_INVALID, (n + ": exists for open networks with inflows only").c_str());
    if (ov.n_prob > 0)
      return fail(FS_ERR_UNSUPPORTED, (n + ": per-replica rates are built for scheduled inflows; this handle has a "
                                           "probabilistic one").c_str());
    if (bytes != size_t(dv.R) * FS_MAX_INFLOWS * sizeof(double))
      return fail(FS_ERR_INVALID, (n + ": wrong byte count (float64 [R, FS_MAX_INFLOWS])").c_str());
    return FS_OK;
  }

  int get_state(int field, void* dst, size_t bytes) override {
    if (field == FS_FIELD_INFLOW_PERIOD || field == FS_FIELD_INIT_INFLOW_PERIOD) {
      const char* name;
      if (int rc = inflow_period_check(field, bytes, &name)) return rc;
      HIP_TRY(hipStreamSynchronize(stream));
      if (int qrc = check_qflag()) return qrc;
      HIP_TRY(hipMemcpy(dst, field == FS_FIELD_INFLOW_PERIOD ? ov.flow_per(dv.R) : ov.init_flow_per(dv.R), bytes, hipMemcpyDeviceToHost));
      return FS_OK;                                   // (columns >= num_inflows were created 0 and are never written)
    }
    if (dv.st16 && (field == FS_FIELD_POS || field == FS_FIELD_VEL)) {     // the halves -> the float32 staging arrays
      hipLaunchKernelGGL((fs::k_state16_unpack<T>), dim3(256), dim3(256), 0, stream, dv);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (int qrc = check_qflag()) return qrc;
    if (field == FS_FIELD_TIME) {
      if (bytes != size_t(dv.R) * sizeof(int32_t)) return fail(FS_ERR_INVALID, "FS_FIELD_TIME: wrong byte count");
      HIP_TRY(hipMemcpy(dst, dv.time, bytes, hipMemcpyDeviceToHost));
      return FS_OK;
    }
    if (field == FS_FIELD_LANE || field == FS_FIELD_LAST_LC || field == FS_FIELD_INIT_LANE) {
      const size_t RN = size_t(dv.R) * dv.N;
      if (bytes != RN * sizeof(int32_t)) return fail(FS_ERR_INVALID, "fs_get_state: wrong byte count");
      const int32_t* p = field == FS_FIELD_LANE ? dv.lane : (field == FS_FIELD_LAST_LC ? dv.last_lc : dv.init_lane);
      HIP_TRY(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
      return FS_OK;
    }
    if (field >= FS_FIELD_ROUTE && field <= FS_FIELD_ARRIVED_RL) {
      if (!open_net) return fail(FS_ERR_INVALID, "fs_get_state: field exists for open networks only");
      const size_t RN = size_t(dv.R) * dv.N;
      const int32_t* p = nullptr;
      size_t count = RN;
      switch (field) {
        case FS_FIELD_ROUTE: p = dv.lane; break;
        case FS_FIELD_SEQ: p = ov.seq; break;
        case FS_FIELD_ORIGIN: p = ov.origin; break;
        case FS_FIELD_FOLLOWER: p = ov.foll; break;
        case FS_FIELD_CTL_SEQ: p = ov.ctl_seq; break;
        case FS_FIELD_COUNTERS: p = ov.counters; count = size_t(dv.R) * 8; break;
        default: p = ov.arrived_rl; break;
      }
      if (bytes != count * sizeof(int32_t)) return fail(FS_ERR_INVALID, "fs_get_state: wrong byte count");
      HIP_TRY(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
      return FS_OK;
    }
    if (open_net && (field == FS_FIELD_HEADWAY || field == FS_FIELD_LEADER)) {
      // open networks keep the snapshot of the last update on the device (vehicle/traci.py:219-250)
      const size_t RN = size_t(dv.R) * dv.N;
      const size_t want = RN * (field == FS_FIELD_HEADWAY ? sizeof(T) : sizeof(int32_t));
      if (bytes != want) return fail(FS_ERR_INVALID, "fs_get_state: wrong byte count");
      HIP_TRY(hipMemcpy(dst, field == FS_FIELD_HEADWAY ? static_cast<const void*>(ov.headway)
                                                        : static_cast<const void*>(ov.lead),
                        bytes, hipMemcpyDeviceToHost));
      return FS_OK;
    }
    if (field == FS_FIELD_HEADWAY || field == FS_FIELD_LEADER) {
      // the kernels' neighbour rule, evaluated on the host from the positions (and lanes):
      // headway = (x_lead - x) mod L - len_lead (vehicle/traci.py:219-250); leader = own-lane nearest ahead
      const int R = dv.R, N = dv.N;
      const size_t RN = size_t(R) * N;
      const size_t want = RN * (field == FS_FIELD_HEADWAY ? sizeof(T) : sizeof(int32_t));
      if (bytes != want) return fail(FS_ERR_INVALID, "fs_get_state: wrong byte count");
      std::vector<T> x(RN), rl(R);
      std::vector<int32_t> ln(RN, 0);
      HIP_TRY(hipMemcpy(x.data(), dv.pos, RN * sizeof(T), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(rl.data(), dv.ring_len, size_t(R) * sizeof(T), hipMemcpyDeviceToHost));
      if (dv.num_lanes > 1) HIP_TRY(hipMemcpy(ln.data(), dv.lane, RN * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int r = 0; r < R; ++r) {
        const T L = rl[r] + T(4) * dv.jlen;
        for (int i = 0; i < N; ++i) {
          int lead = -1;
          T best = T(0);
          if (dv.num_lanes > 1) {
            for (int j = 0; j < N; ++j) {
              if (j == i || ln[size_t(r) * N + j] != ln[size_t(r) * N + i]) continue;
              T d = x[size_t(r) * N + j] - x[size_t(r) * N + i];
              if (d < T(0) || (d == T(0) && j < i)) d = d + L;
              if (lead < 0 || d < best) { best = d; lead = j; }
            }
          } else if (N > 1) {
            lead = (i + 1 >= N) ? 0 : i + 1;
            best = x[size_t(r) * N + lead] - x[size_t(r) * N + i];
            if (best < T(0)) best = best + L;
          }
          if (field == FS_FIELD_LEADER) static_cast<int32_t*>(dst)[size_t(r) * N + i] = lead;
          else static_cast<T*>(dst)[size_t(r) * N + i] = lead < 0 ? T(1000) : best - h_len[lead];
        }
      }
      return FS_OK;
    }
    size_t count;
    bool writable;
    T* p = field_ptr(field, &count, &writable);
    if (!p) return fail(FS_ERR_INVALID, "fs_get_state: unknown field");
    if (bytes != count * sizeof(T)) return fail(FS_ERR_INVALID, "fs_get_state: wrong byte count");
    HIP_TRY(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return FS_OK;
  }

  // k.vehicle.add (vehicle/traci.py:1089-1122) for a vehicle that has a slot of its own and is not in the network (an
  // initial vehicle that arrived: BottleneckAccelEnv.additional_command re-inserts its RL vehicles, bottleneck.py:733-757):
  // the slot's vehicle is back at coordinate x of entry lane / route `route` with the given speed, last in the id list
  int add_vehicle(int replica, int slot, int route, double x, double speed) override {
    HIP_TRY(hipStreamSynchronize(stream));
    if (!open_net) return fail(FS_ERR_UNSUPPORTED, "fs_add_vehicle: open networks only (a closed loop keeps its vehicles)");
    const int paths = cfg.network == FS_NET_MERGE ? 2 : (cfg.num_paths ? cfg.num_paths : 4);
    if (replica < 0 || replica >= dv.R || slot < 0 || slot >= dv.N || route < 0 || route >= paths)
      return fail(FS_ERR_INVALID, "fs_add_vehicle: replica / slot / route out of range");
    if (!(speed >= 0.0) || !(x >= 0.0) || !(x < double(ov.end_x)))
      return fail(FS_ERR_INVALID, "fs_add_vehicle: need speed >= 0 and 0 <= x < the end of the route");
    const size_t e = size_t(replica) * dv.N + slot;
    int32_t cur = 0, cnt[8];
    HIP_TRY(hipMemcpy(&cur, dv.lane + e, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (cur >= 0) return fail(FS_ERR_INVALID, "fs_add_vehicle: the slot's vehicle is in the network");
    HIP_TRY(hipMemcpy(cnt, ov.counters + size_t(replica) * 8, sizeof(cnt), hipMemcpyDeviceToHost));
    const T xv = T(x), vv = T(speed), zero = T(0), big = T(3.0e38), vm = T(veh[slot].sumo_max_speed);
    const int32_t rt = route, sq = cnt[fs::CNT_SEQ], minus1 = -1, org = -1 - slot, never = -(1 << 30);
    cnt[fs::CNT_SEQ] += 1;
    HIP_TRY(hipMemcpy(dv.pos + e, &xv, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv.vel + e, &vv, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv.prev_vel + e, &zero, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv.accel + e, &zero, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(const_cast<int32_t*>(dv.lane) + e, &rt, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(const_cast<int32_t*>(dv.last_lc) + e, &never, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.seq + e, &sq, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.origin + e, &org, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.foll + e, &minus1, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.ctl_seq + e, &minus1, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.foll_h + e, &big, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.vmax + e, &vm, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ov.counters + size_t(replica) * 8, cnt, sizeof(cnt), hipMemcpyHostToDevice));
    return launch_steps(0, nullptr, nullptr, 0, d_obs, d_rew, d_done, 0);      // the neighbour fields of the new arrangement
  }

  int set_state(int field, const void* src, size_t bytes) override {
    HIP_TRY(hipStreamSynchronize(stream));
    if (field == FS_FIELD_INFLOW_PERIOD || field == FS_FIELD_INIT_INFLOW_PERIOD) {
      const char* name;
      if (int rc = inflow_period_check(field, bytes, &name)) return rc;
      std::vector<double> per(size_t(dv.R) * FS_MAX_INFLOWS, 0.0);
      const double* vals = static_cast<const double*>(src);
      for (int r = 0; r < dv.R; ++r)
        for (int f = 0; f < cfg.num_inflows; ++f) {
          const double p = vals[size_t(r) * FS_MAX_INFLOWS + f];
          if (!std::isfinite(p) || !(p > 0.0))
            return fail(FS_ERR_INVALID, (std::string(name) + ": a period must be finite and > 0 (replica " +
                                         std::to_string(r) + ", inflow " + std::to_string(f) + ")").c_str());
          per[size_t(r) * FS_MAX_INFLOWS + f] = p;
        }
      HIP_TRY(hipMemcpy(ov.init_flow_per(dv.R), per.data(), bytes, hipMemcpyHostToDevice));
      if (field == FS_FIELD_INFLOW_PERIOD)            // the running episode too (as FS_FIELD_RING_LENGTH sets both)
        HIP_TRY(hipMemcpy(ov.flow_per(dv.R), per.data(), bytes, hipMemcpyHostToDevice));
      return FS_OK;
    }
    if (field == FS_FIELD_TIME) {
      if (bytes != size_t(dv.R) * sizeof(int32_t)) return fail(FS_ERR_INVALID, "FS_FIELD_TIME: wrong byte count");
      HIP_TRY(hipMemcpy(dv.time, src, bytes, hipMemcpyHostToDevice));
      return FS_OK;
    }
    if (field == FS_FIELD_HEADWAY || field == FS_FIELD_LEADER)
      return fail(FS_ERR_INVALID, "headway / leader are derived from positions and lanes");
    if (field >= FS_FIELD_SEQ && field <= FS_FIELD_ARRIVED_RL)
      return fail(FS_ERR_INVALID, "fs_set_state: read-only field");
    if (field == FS_FIELD_MAX_SPEED && !open_net)
      return fail(FS_ERR_INVALID, "fs_set_state: FS_FIELD_MAX_SPEED exists for open networks only");
    if (field == FS_FIELD_ROUTE) field = FS_FIELD_LANE;
    if (field == FS_FIELD_LANE || field == FS_FIELD_LAST_LC || field == FS_FIELD_INIT_LANE) {
      const size_t RN = size_t(dv.R) * dv.N;
      if (bytes != RN * sizeof(int32_t)) return fail(FS_ERR_INVALID, "fs_set_state: wrong byte count");
      const int32_t* p = field == FS_FIELD_LANE ? dv.lane : (field == FS_FIELD_LAST_LC ? dv.last_lc : dv.init_lane);
      HIP_TRY(hipMemcpy(const_cast<int32_t*>(p), src, bytes, hipMemcpyHostToDevice));
      if (open_net && field == FS_FIELD_LANE) return launch_steps(0, nullptr, nullptr, 0, d_obs, d_rew, d_done, 0);
      return FS_OK;
    }
    size_t count;
    bool writable;
    T* p = field_ptr(field, &count, &writable);
    if (!p) return fail(FS_ERR_INVALID, "fs_set_state: unknown field");
    if (bytes != count * sizeof(T)) return fail(FS_ERR_INVALID, "fs_set_state: wrong byte count");
    HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    if (field == FS_FIELD_VEL || field == FS_FIELD_INIT_VEL) {
      bool neg = false;
      const T* vals = static_cast<const T*>(src);
      for (size_t e = 0; e < count; ++e) neg = neg || !(vals[e] >= T(-100));
      if (field == FS_FIELD_INIT_VEL) init_vel_negative = neg;
      neg_speed_possible = neg_speed_possible || neg;
    }
    if (dv.st16 && (field == FS_FIELD_POS || field == FS_FIELD_VEL)) {
      // one of the two staging arrays was just overwritten: bring the OTHER one up to date from the halves first, then
      // pack both (a float32 value that is no half is rounded here, as every launch boundary does)
      std::vector<T> keep(count);
      HIP_TRY(hipMemcpy(keep.data(), p, bytes, hipMemcpyDeviceToHost));
      hipLaunchKernelGGL((fs::k_state16_unpack<T>), dim3(256), dim3(256), 0, stream, dv);
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipMemcpy(p, keep.data(), bytes, hipMemcpyHostToDevice));
      hipLaunchKernelGGL((fs::k_state16_pack<T>), dim3(256), dim3(256), 0, stream, dv, static_cast<const uint8_t*>(nullptr));
      HIP_TRY(hipGetLastError());
    }
    if (open_net && (field == FS_FIELD_POS || field == FS_FIELD_VEL))   // refresh the leader / headway snapshot
      return launch_steps(0, nullptr, nullptr, 0, d_obs, d_rew, d_done, 0);
    if (field == FS_FIELD_RING_LENGTH) {            // sets the pending lengths too
      HIP_TRY(hipMemcpy(const_cast<T*>(dv.init_ring_len), src, bytes, hipMemcpyHostToDevice));
      h_ring_len.assign(static_cast<const T*>(src), static_cast<const T*>(src) + count);
      ring_mirror_changed();
    }
    if (field == FS_FIELD_INIT_RING_LENGTH) {
      // the host copy the divisor proofs walk holds every length a replica may be running on: the current ones and,
      // appended, the pending ones (a masked reset on the device swaps them in without the host knowing which)
      const T* vals = static_cast<const T*>(src);
      h_ring_len.insert(h_ring_len.end(), vals, vals + count);
      std::sort(h_ring_len.begin(), h_ring_len.end());             // the distinct lengths only: the proofs walk this list
      h_ring_len.erase(std::unique(h_ring_len.begin(), h_ring_len.end()), h_ring_len.end());
      ring_mirror_changed();
    }
    return FS_OK;
  }
};

}  // namespace fsim
