/*
 * flowsim.h -- C ABI of libflowsim.so, the MI355X-native batched traffic
 * micro-simulation step loop.
 *
 * The reference (parthjaggi/flow) has no native boundary on this path: its
 * "FFI" is the TraCI TCP protocol between flow.envs.Env and a SUMO subprocess.
 * Each entry point below replaces the group of reference calls cited next to
 * it (paths relative to the reference root).  Plain pointers and sizes only;
 * no torch / numpy types.  All functions return FS_OK (0) or a negative
 * FS_ERR_* code; fs_last_error() returns the message of the last failure on
 * the calling thread.
 *
 * Threading: a handle is not thread-safe; use one handle per (process, GPU)
 * (reference: one Env + one SUMO process per rollout worker,
 * examples/train.py:149).  All device work of a handle is enqueued on one HIP
 * stream (fs_set_stream) and is asynchronous with respect to the host unless
 * the call copies results to host memory.
 *
 * Ownership: the library owns the simulator state in HBM; the caller owns
 * every buffer it passes in.  "_dev" entry points take device pointers
 * (hipMalloc / torch-ROCm storage); the others take host pointers and copy.
 */
#ifndef FLOWSIM_H
#define FLOWSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 8

/* ---- error codes -------------------------------------------------------- */
#define FS_OK 0
#define FS_ERR_INVALID -1       /* bad argument / config (Python: ValueError / KeyError)   */
#define FS_ERR_UNSUPPORTED -2   /* valid in the reference, not built yet (NotImplementedError) */
#define FS_ERR_HIP -3           /* HIP runtime failure (FatalFlowError)                    */
#define FS_ERR_NOSPACE -4       /* vehicles do not fit (network/base.py:603-605)            */

/* ---- enums -------------------------------------------------------------- */
/* FS_F32 / FS_F64: arithmetic and state in that type (FS_F64 = the reference's Python-float arithmetic).
 * FS_MIXED: positions and speeds kept and integrated in float64, the acceleration controller evaluated in
 * float32 on their rounded images -- within 1e-4 of the float64 trajectories over a 1500-step episode at
 * float32 cost.  Built for single-lane rings of IDM and RL vehicles (AccelEnv and WaveAttenuationPOEnv heads, warm-up
 * steps, masked resets, acceleration noise), for the figure eight (rollouts of up to 16 vehicles; what that kernel
 * does not cover steps in float64) and for the open networks up to 64 vehicle slots (the float64 kernel with float32
 * car-following models; beyond 64 slots: plain float64); fs_create names the field of a configuration that does not
 * fit.  State fields are float64 as for FS_F64. */
enum fs_precision { FS_F32 = 0, FS_F64 = 1, FS_MIXED = 2,
                    FS_F16S = 3    /* "fp16 state, fp32 integrator" (BASELINE configs[4]): the positions and speeds a handle
                                      keeps in HBM BETWEEN launches are IEEE half values -- a speed is one half, a position
                                      two (x = hi + lo, 22 significant bits: a single half has a 0.5 m ulp at 700 m) -- and a
                                      launch loads them into float32 registers, steps in float32 exactly as FS_F32 does, and
                                      stores halves again.  6 bytes of state per vehicle instead of 8; every launch boundary
                                      rounds the speeds to 11 bits (<= 0.008 m/s below 32 m/s).  Built for FS_NET_MERGE
                                      (the configuration BASELINE names); fs_get_state / fs_set_state speak float32.
                                      NOTE: a trajectory therefore depends on where the launches are cut -- K fs_step calls
                                      round K times, one fs_rollout_dev of K steps once; runs are reproducible for a fixed
                                      launch pattern only (tests/test_f16s_gpu.py measures the drift between the two). */
};

/* acceleration controllers, flow/controllers/__init__.py */
enum fs_controller {
  FS_CTRL_SIM = 0,              /* SimCarFollowingController: never commanded          car_following_models.py:485-497 */
  FS_CTRL_RL = 1,               /* RLController: commanded by the action vector        rlcontroller.py:6-39 */
  FS_CTRL_IDM = 2,              /* p = {v0, T, a, b, delta, s0}                         car_following_models.py:400-482 */
  FS_CTRL_CFM = 3,              /* p = {k_d, k_v, k_c, d_des, v_des}                    :17-88 */
  FS_CTRL_BCM = 4,              /* p = {k_d, k_v, k_c, d_des, v_des}                    :91-176 */
  FS_CTRL_LAC = 5,              /* p = {k_1, k_2, h, tau}; stateful a                   :179-245 */
  FS_CTRL_OVM = 6,              /* p = {alpha, beta, h_st, h_go, v_max}                 :248-328 */
  FS_CTRL_LINEAR_OVM = 7,       /* p = {v_max, adaptation, h_st}                        :331-397 */
  FS_CTRL_GIPPS = 8,            /* p = {v0, acc, b, b_l, s0, tau}                       :500-582 */
  FS_CTRL_FOLLOWER_STOPPER = 9, /* p = {v_des}                                          velocity_controllers.py:7-116 */
  FS_CTRL_NONLOCAL_FOLLOWER_STOPPER = 10, /* v_des = replica mean speed                 velocity_controllers.py:119-164 */
  FS_CTRL_PISATURATION = 11,    /* no parameters; keeps int(38/sim_step)-1 past speeds  velocity_controllers.py:167-240 */
  FS_CTRL_USER = 12             /* a controller of the USER's (the reference lets user code subclass BaseController and write
                                   get_accel in Python, base_controller.py:42-118): its get_accel is a device function compiled
                                   INTO a copy of this library -- `python -m flow_amd.build` with
                                   -DFS_USER_CONTROLLER_HEADER, see flow_amd.controllers.CompiledController and
                                   flow_amd.build.build_user; p = its (up to 8) parameters.  The stock library refuses a
                                   launch with such a slot (FS_ERR_UNSUPPORTED) */
};

/* BaseController fail-safes, flow/controllers/base_controller.py:113-116 */
enum fs_failsafe { FS_FAILSAFE_NONE = 0, FS_FAILSAFE_INSTANTANEOUS = 1, FS_FAILSAFE_SAFE_VELOCITY = 2 };

/* environments (observation + reward heads) */
enum fs_env {
  FS_ENV_ACCEL = 0,                 /* AccelEnv                 flow/envs/ring/accel.py:25-183 */
  FS_ENV_WAVE_ATTENUATION = 1,      /* WaveAttenuationEnv       flow/envs/ring/wave_attenuation.py:50-210 */
  FS_ENV_WAVE_ATTENUATION_PO = 2,   /* WaveAttenuationPOEnv     flow/envs/ring/wave_attenuation.py:213-276 */
  FS_ENV_LANE_CHANGE_ACCEL = 3,     /* LaneChangeAccelEnv       flow/envs/ring/lane_change_accel.py:28-154;
                                       actions are [acc_0, dir_0, acc_1, dir_1, ...] (2 per RL vehicle) */
  FS_ENV_MERGE_PO = 4,              /* MergePOEnv               flow/envs/merge.py:28-231: num_rl controlled vehicles
                                       (rl_queue / rl_veh slotting), obs 5*num_rl, action column = place in rl_veh */
  FS_ENV_MERGE_MA = 5,              /* MultiAgentMergePOEnv     flow/envs/multiagent/merge.py:19-190: one 5-vector and
                                       one action column per RL slot (column = rl_index), shared reward, no crash */
  FS_ENV_BOTTLENECK_DV = 6,         /* BottleneckDesiredVelocityEnv  flow/envs/bottleneck.py:760-1085: 4 values per
                                       observed lane-segment + outflow; one action per controlled lane-segment (num_rl =
                                       num_act_cells) shifting the maxSpeed of the RL vehicles inside it.  The mean
                                       speed of a lane-segment: FS_F32 handles with more than 64 vehicle slots, and the
                                       queue-order kernel k_drop_queue, add the speeds as integers of 2^-16 m/s (exact,
                                       order-free; oracle/opennet.py cell_sum = 'fixed'); FS_F64 and <= 64 slots add
                                       them as floats in slot order */
  FS_ENV_BOTTLENECK = 7,            /* BottleneckEnv            flow/envs/bottleneck.py:83-483: observation [1], outflow reward */
  FS_ENV_WAVE_ATTENUATION_PO_MA = 8,/* MultiAgentWaveAttenuationPOEnv  flow/envs/multiagent/ring/wave_attenuation.py:128-252:
                                       per RL vehicle (column = rl_index) [v / 15, (v_lead - v) / 15, headway / max_length],
                                       obs 3 * num_rl; WaveAttenuationEnv's reward shared by the agents; crash = 0 */
  FS_ENV_LANE_CHANGE_ACCEL_PO = 10, /* LaneChangeAccelPOEnv     flow/envs/ring/lane_change_accel.py:163-262: LaneChangeAccelEnv's
                                       actions and reward; per RL vehicle (column c = rl_index) and lane q its nearest
                                       leader / follower of that lane as flow/core/kernel/vehicle/traci.py:776-867 finds them:
                                       obs[4 * lanes * c + {0, 1, 2, 3} * lanes + q] = gap to the leader [m], gap to the follower
                                       [m], leader speed / v_max, follower speed / v_max (1000, 1000, 0, 0 for an empty lane; a
                                       vehicle alone in its lane is its own leader and follower, one lap away), then
                                       obs[4 * lanes * num_rl + c] = own speed [m/s]; obs 4 * lanes * num_rl + num_rl */
  FS_ENV_ACCEL_PO_MA = 9,           /* MultiAgentAccelPOEnv     flow/envs/multiagent/ring/accel.py:84-227: per RL vehicle
                                       [x / L, v / v_max, (v_lead - v) / v_max, (x_lead - x - len_ego) / L,
                                       (v - v_follow) / v_max, headway(follower) / L], obs 6 * num_rl; desired_velocity
                                       reward shared by the agents; crash = 0 (multiagent/base.py:188-190) */
  FS_ENV_MULTI_WAVE_ATTENUATION_PO = 11, /* MultiWaveAttenuationPOEnv flow/envs/multiagent/ring/wave_attenuation.py:34-140
                                       on MultiRingNetwork: a replica ROW is ONE ring with one RL vehicle (num_rl = 1); obs 3 =
                                       [v / 15, (v_lead - v) / 15, headway / max_length] (bumper to bumper); the reward is a
                                       desired-velocity norm over the n vehicles whose front is on one of the ring's four
                                       edges (not inside a junction): max(max_cost[n] - cost, 0) / max_cost[n] with
                                       max_cost[n] = ||[target] * n|| and NO epsilon (n = 0: NaN, as numpy's 0 / 0), 0 if one
                                       of those speeds is below -100, 0 without actions (warm-up); crash = 0.  FS_F32 (every
                                       ring kernel) and FS_F64 (the generic kernel); FS_MIXED is refused */
  FS_ENV_USER = 12                  /* an observation / reward head of the USER's (the reference lets user code subclass Env
                                       and write get_state / compute_reward, flow/envs/base.py): three device functions
                                       compiled INTO a copy of this library with -DFS_USER_ENV_HEADER, see
                                       flow_amd.envs.CompiledEnv and flow_amd.build.build_user.  The header also fixes the
                                       shapes: kUserObsPerVehicle (1..8), kUserObsRlOnly, kUserRewardTerms (0..4).  Contract:
                                       - per vehicle, fs_user_obs writes o[0 .. kUserObsPerVehicle-1]; the lane stores float(o[k]).
                                         kUserObsRlOnly: only an RL vehicle's lane writes, at kUserObsPerVehicle * rl_index + k,
                                         fs_obs_dim = kUserObsPerVehicle * num_rl; else obs[k * N + i] with i the vehicle's
                                         place in get_ids() (AccelEnv's index without sort_vehicles: obs_perm or the slot),
                                         fs_obs_dim = kUserObsPerVehicle * N;
                                       - per vehicle, fs_user_terms writes t[0 .. kUserRewardTerms-1]; sum[m] is the replica's
                                         sum of (valid ? t[m] : 0) over its lanes in the built-in heads' tree order
                                         (seg_sum; oracle.rewards.tree_sum);
                                       - per replica, fs_user_reward(sum, fail, ...) returns the reward; fail = a collision in
                                         this step or a speed below -100 (the built-in heads' condition); the replica's first
                                         vehicle stores it;
                                       - actions are accelerations of the RL vehicles in rl_index order, clipped as
                                         clip_actions says (FS_ENV_ACCEL's); `action` is the vehicle's clipped command of the
                                         step just taken (0 for a non-RL vehicle or a step without actions);
                                       - done is the built-in flag byte (horizon, collision);
                                       - p[0..7] = fs_config.user_env_p in the handle's precision.
                                       Single-lane rings and segment-table loops, at most 64 vehicles, FS_F32 / FS_F64, no
                                       sort_vehicles; always on k_steps.  The stock library refuses such a handle at fs_create
                                       (FS_ERR_UNSUPPORTED); fs_policy_rollout_dev, fs_policy_pair_* and fs_population_* refuse
                                       it by name, fs_policy_act_dev takes it (see there) */
};

enum fs_network {
  FS_NET_RING = 0,          /* RingNetwork, flow/networks/ring.py (any number of lanes) */
  FS_NET_FIGURE_EIGHT = 1,  /* FigureEightNetwork, flow/networks/figure_eight.py: a closed one-lane loop that
                               crosses itself; described by fs_config.segments + fs_config.junction */
  FS_NET_MERGE = 2,         /* MergeNetwork, flow/networks/merge.py: an OPEN one-lane network, two routes (0 = highway,
                               1 = on-ramp) converging at a priority junction; vehicles enter through fs_config.inflows
                               and leave at end_x.  num_vehicles is the slot CAPACITY of a replica. */
  FS_NET_BOTTLENECK = 3     /* BottleneckNetwork, flow/networks/bottleneck.py (scaling 1 or 2): an OPEN network of
                               num_paths = 4 * scaling entry lanes that join pairwise at two zipper junctions
                               (4 -> 2 -> 1, or 8 -> 4 -> 2); a vehicle's "route" is the entry lane it continues,
                               0..num_paths-1 (the simplified lane changing of M11 moves it to a neighbouring one) */
};

enum fs_integrator { FS_EULER = 0, FS_BALLISTIC = 1 /* SumoParams.use_ballistic, core/params.py:578-602 */ };

/* fields of fs_get_state / fs_set_state (the read accessors of
 * flow/core/kernel/vehicle/base.py:327-672 and the test back-doors of
 * flow/core/kernel/vehicle/traci.py:411-425) */
enum fs_field {
  FS_FIELD_POS = 0,        /* real[R,N]  absolute position along the loop (get_x_by_id) */
  FS_FIELD_VEL = 1,        /* real[R,N]  get_speed                                       */
  FS_FIELD_HEADWAY = 2,    /* real[R,N]  get_headway (derived; read-only)                */
  FS_FIELD_PREV_VEL = 3,   /* real[R,N]  get_previous_speed                              */
  FS_FIELD_ACCEL = 4,      /* real[R,N]  last commanded acceleration (0 if uncommanded)  */
  FS_FIELD_TIME = 5,       /* int32[R]   Env.time_counter                                */
  FS_FIELD_RING_LENGTH = 6,/* real[R]    per-replica ring length (edges only)            */
  FS_FIELD_INIT_POS = 7,   /* real[R,N]  Env.initial_state positions                     */
  FS_FIELD_INIT_VEL = 8,   /* real[R,N]  Env.initial_state speeds                        */
  FS_FIELD_CTRL_STATE = 9, /* real[R,N]  controller state (LAC: self.a)                  */
  FS_FIELD_LANE = 10,      /* int32[R,N] get_lane                                        */
  FS_FIELD_LAST_LC = 11,   /* int32[R,N] time_counter of the last lane change (vehicle/traci.py:205-209) */
  FS_FIELD_LEADER = 12,    /* int32[R,N] slot of the own-lane leader, -1 if none (get_leader; read-only) */
  FS_FIELD_INIT_LANE = 13, /* int32[R,N] Env.initial_state lanes (open networks: routes)  */
  /* open networks only (read-only except ROUTE) */
  FS_FIELD_ROUTE = 14,     /* int32[R,N] route of the vehicle in the slot, -1 = free slot (alias of LANE) */
  FS_FIELD_SEQ = 15,       /* int32[R,N] place in the id list = departure order (vehicle/traci.py:279-280)  */
  FS_FIELD_ORIGIN = 16,    /* int32[R,N] inflow * 2^20 + running number ("flow_<f>.<k>"), or -1-i for initial vehicle i */
  FS_FIELD_FOLLOWER = 17,  /* int32[R,N] get_follower: the sticky follower of vehicle/traci.py:243-250, -1 if none */
  FS_FIELD_CTL_SEQ = 18,   /* int32[R,N] >= 0: the vehicle is in MergePOEnv.rl_veh, value = order of joining */
  FS_FIELD_COUNTERS = 19,  /* int32[R,8] {steps since simulator start, vehicles ever departed (id counter), rl_veh
                              join counter, arrived last sub-step, departed last sub-step, arrived total,
                              departed total, random-lane vehicles dropped at insertion}  (get_num_arrived /
                              get_outflow_rate inputs, vehicle/traci.py:493-533) */
  FS_FIELD_ARRIVED_RL = 20,/* int32[R,N] 1: the RL vehicle of this slot arrived in the last sub-step (get_arrived_rl_ids) */
  FS_FIELD_MAX_SPEED = 21, /* real[R,N]  get_max_speed / set_max_speed: maxSpeed of the SUMO car-following model */
  FS_FIELD_SORT_KEY = 23,  /* real[R,N] AccelEnv.absolute_position as of the last additional_command (sort_vehicles only,
                              flow/envs/ring/accel.py:150-169): the key the kernel ranks observations and actions by */
  FS_FIELD_INIT_RING_LENGTH = 22,/* real[R] the ring length a replica takes at its NEXT reset (WaveAttenuationEnv.reset
                              draws a new length per episode, flow/envs/ring/wave_attenuation.py:157-210): fs_reset[_dev]
                              copies it into FS_FIELD_RING_LENGTH for the replicas it resets, so a reset inside a
                              captured graph can change the length without touching replicas that are mid-episode.
                              Writing FS_FIELD_RING_LENGTH sets both. */
  FS_FIELD_INFLOW_PERIOD = 24, /* float64[R,FS_MAX_INFLOWS] (whatever the handle's precision) the period [s] of inflow f
                              in replica r: vehicle k of the flow is due at begin + k * period, k the vehicles the replica
                              has emitted (begin, end and number stay the handle's).  fs_create fills it from
                              fs_inflow.period.  Columns >= num_inflows read as 0 and are ignored on write.  A period
                              written mid-episode moves the due time of the replica's next vehicle.  Refused, with the
                              field's name: closed networks and open ones without inflows (FS_ERR_INVALID), a handle
                              with a probabilistic inflow (FS_ERR_UNSUPPORTED), a period that is not finite or not > 0
                              (FS_ERR_INVALID; nothing is written).  Writing it sets FS_FIELD_INIT_INFLOW_PERIOD too. */
  FS_FIELD_INIT_INFLOW_PERIOD = 25 /* float64[R,FS_MAX_INFLOWS] the period a replica takes at its NEXT reset (the twin of
                              FS_FIELD_INIT_RING_LENGTH; BottleneckDesiredVelocityEnv.reset draws a new inflow per
                              episode, flow/envs/bottleneck.py:988-1085): fs_reset[_dev] and the resets inside a
                              policy rollout copy it into FS_FIELD_INFLOW_PERIOD for the replicas they reset; writing
                              it leaves the running episodes alone. */
};

#define FS_MAX_CTRL_PARAMS 8
#define FS_MAX_SEGMENTS 16
#define FS_MAX_INFLOWS 8
#define FS_MAX_SLOTS_WIDE 256   /* vehicle slots per replica on FS_NET_BOTTLENECK (64 everywhere else) */

/* One edge of a closed loop in route order (non-ring networks).  `start` is the loop coordinate of the
 * edge's first metre; Flow's own coordinate of a point `x` on it (get_x_by_id, vehicle/traci.py:1011-1017
 * with the network's edge-start table) is flow_start + flow_slope * (x - start); internal edges without
 * a table entry have slope 0 (network/traci.py:280-287). */
typedef struct fs_segment {
  double start;
  double flow_start;
  double flow_slope;
  int32_t internal;                   /* 1: junction-internal edge (':...'): no Flow command with junction_mode */
  int32_t route;                      /* FS_NET_MERGE: the route this row belongs to (rows of a route are contiguous,
                                         starts increasing); 0 otherwise (FS_NET_BOTTLENECK: one table for all lanes) */
} fs_segment;

/* One InFlows.add entry (flow/core/params.py:1080-1213) of an open network. */
typedef struct fs_inflow {
  int32_t type;                       /* vehicle type = fs_vehicle_spec.type of the slots it may occupy */
  int32_t route;                      /* route of its edge (0 highway, 1 on-ramp); FS_NET_BOTTLENECK: entry lane, or -1 for
                                         departLane = "random" (drawn per vehicle from the Philox stream) */
  int32_t number;                     /* total vehicles to create, < 0 = unlimited */
  int32_t reserved;
  double period;                      /* seconds between vehicles: 3600 / vehs_per_hour, or `period` */
  double begin, end;                  /* first departure time / end of the departure interval [s] */
  double depart_speed;                /* departSpeed [m/s] */
  double depart_pos;                  /* front position on the first edge at insertion (SUMO "base": the vehicle length) */
  double probability;                 /* < 0: equally spaced vehicles (`period`).  In [0, 1]: InFlows.add(probability=p),
                                         params.py:1103-1105 -- in every simulation sub-step between begin and end a
                                         vehicle is generated with probability p * sim_step (at most `number` of them);
                                         generated vehicles wait their turn like due ones (M2b, Philox-drawn) */
} fs_inflow;

/* The self-crossing of the figure eight (docs/HISTORY.md S-J; SUMO's junction logic restated, unpinned).
 * Stream a (bottom->top, priority 78) crosses stream b (right->left, priority 46),
 * flow/networks/figure_eight.py:126-154. */
typedef struct fs_junction {
  int32_t enabled;
  int32_t reserved;
  double a_in, a_out;                 /* loop coordinates of the internal edge of stream a */
  double b_in, b_out;                 /* ... of stream b */
  double lookahead;                   /* a vehicle this close to its entry line may have to yield */
  double time_gap;                    /* stream a blocks the box when it reaches a_in within time_gap */
  double za_lo, za_hi, zb_lo, zb_hi;  /* front positions at which a body covers the crossing point */
} fs_junction;

/* One lane-segment of the bottleneck environments (bottleneck.py:796-812): the vehicles on `lane` whose position
 * on the edge lies in (lo, hi]  (np.searchsorted(slices, pos) - 1). */
typedef struct fs_cell {
  double edge_start;                  /* coordinate of the first metre of the edge */
  double lo, hi;                      /* segment boundaries, relative to the edge start */
  int32_t lane;                       /* lane index on that edge */
  int32_t last_segment;               /* 1: last segment of its edge (takes a vehicle standing exactly at pos 0) */
} fs_cell;

/* One vehicle slot; identical for every replica (VehicleParams.add,
 * flow/core/params.py:236-351, expanded per vehicle). */
typedef struct fs_vehicle_spec {
  int32_t controller;                 /* enum fs_controller */
  int32_t fail_safe;                  /* enum fs_failsafe */
  int32_t speed_mode;                 /* SUMO speed-mode bitmask, core/params.py:12-18 */
  int32_t rl_index;                   /* column of the action vector, -1 if not RL */
  int32_t type;                       /* open networks: index of the vehicle type (VehicleParams.add order) */
  int32_t lane_change_mode;           /* SumoLaneChangeParams.lane_change_mode of the type; FS_NET_BOTTLENECK: a strategic /
                                         cooperative / speed-gain / keep-right bit (mode & 0x55) switches the simplified
                                         lane-change model on for this vehicle (docs/HISTORY.md M11) */
  double p[FS_MAX_CTRL_PARAMS];       /* controller parameters, see enum fs_controller */
  double noise;                       /* sigma of the Gaussian acceleration noise */
  double delay;                       /* delay used by the safe_velocity fail-safe */
  double max_accel;                   /* SumoCarFollowingParams accel */
  double max_decel;                   /* |SumoCarFollowingParams decel| */
  double length;                      /* vehicle length [m] */
  double sumo_tau;                    /* SumoCarFollowingParams tau */
  double sumo_min_gap;                /* SumoCarFollowingParams min_gap */
  double sumo_max_speed;              /* SumoCarFollowingParams max_speed */
  double initial_speed;               /* VehicleParams.add(initial_speed=) */
} fs_vehicle_spec;

typedef struct fs_config {
  uint32_t struct_size;               /* sizeof(fs_config), ABI check */
  uint32_t abi_version;               /* FS_ABI_VERSION */
  int32_t precision;                  /* enum fs_precision: arithmetic + state type */
  int32_t network;                    /* enum fs_network */
  int32_t env;                        /* enum fs_env */
  int32_t integrator;                 /* enum fs_integrator */
  int32_t num_replicas;               /* R */
  int32_t num_vehicles;               /* N per replica (<= 64; FS_NET_BOTTLENECK: <= FS_MAX_SLOTS_WIDE); open networks: slot capacity */
  int32_t num_rl;                     /* RL vehicles per replica; FS_ENV_MERGE_PO: env_params 'num_rl' */
  int32_t horizon;                    /* EnvParams.horizon; <0 means inf */
  int32_t warmup_steps;               /* EnvParams.warmup_steps */
  int32_t sims_per_step;              /* EnvParams.sims_per_step */
  int32_t junction_mode;              /* 1: no Flow command while on an internal edge (base_controller.py:98-99) */
  int32_t clip_actions;               /* EnvParams.clip_actions */
  int32_t evaluate;                   /* EnvParams.evaluate */
  int32_t device;                     /* HIP device ordinal */
  int32_t track_aux;                  /* 1: keep FS_FIELD_PREV_VEL / FS_FIELD_ACCEL up to date (get_previous_speed) */
  int32_t num_lanes;                  /* lanes of the ring (net_params 'lanes'); > 1 selects the multi-lane kernel */
  int32_t lane_change_mode;           /* SumoLaneChangeParams.lane_change_mode: 0 = execute every commanded change,
                                         otherwise refuse a change that would overlap a vehicle of the target lane */
  int32_t last_lc_quirk;              /* 1: get_last_lc returns the headway, as this fork does (vehicle/traci.py:604-614) */
  uint64_t seed;                      /* SimParams.seed: key of the per-(replica,vehicle,step) noise stream */
  double sim_step;                    /* SimParams.sim_step */
  double slowdown_ramp;               /* v' = v + (next_vel - v)*ramp; dt/(dt+1e-3) models slowDown(.., 1e-3) */
  double junction_length;             /* length of each internal edge */
  double crash_gap;                   /* crash <=> some headway < crash_gap after the move */
  double max_speed;                   /* k.network.max_speed() */
  double target_velocity;             /* env_params.additional_params['target_velocity'] */
  double action_low, action_high;     /* action_space bounds */
  double po_max_length;               /* WaveAttenuationPOEnv max_length normaliser */
  double lane_change_duration;        /* env_params 'lane_change_duration' (lane_change_accel.py:143-147) */
  const fs_vehicle_spec* vehicles;    /* [N] */
  const double* ring_length;          /* [R] length of each replica's ring (sum of its 4 edges) */
  const double* init_pos;             /* [R,N] initial absolute positions */
  const double* init_vel;             /* [R,N] initial speeds, or NULL -> vehicles[i].initial_speed */
  const int32_t* init_lane;           /* [R,N] initial lanes, or NULL -> lane 0 */
  const fs_segment* segments;         /* [num_segments] edge table of a non-ring loop, or NULL */
  int32_t num_segments;               /* 0 for FS_NET_RING */
  int32_t num_inflows;                /* FS_NET_MERGE: entries of `inflows` (<= FS_MAX_INFLOWS) */
  fs_junction junction;               /* crossing model (figure eight) / merge right of way: for FS_NET_MERGE only
                                         enabled, lookahead and time_gap are read (the box is [box_in, merge_x)) */
  /* ---- open networks (FS_NET_MERGE); ignored otherwise ---- */
  const fs_inflow* inflows;           /* [num_inflows] in InFlows.add order */
  const uint8_t* init_alive;          /* [R,N] 1: the slot holds an initial vehicle (init_pos / init_vel / init_lane =
                                         its coordinate, speed and ROUTE) */
  double route_start[2];              /* coordinate of the first metre of route 0 / 1 */
  double merge_x;                     /* coordinate where the two routes join (start of edge 'center') */
  double box_in;                      /* coordinate of the junction entry lines (merge_x - internal length) */
  double end_x;                       /* vehicles whose front reaches end_x have arrived */
  double net_length;                  /* k.network.length(): the normaliser of MergePOEnv.get_state */
  int32_t ma_apply_actions;           /* FS_ENV_MERGE_MA: 0 = actions are never applied, as this fork ships
                                         (multiagent/merge.py:92-96); 1 = column rl_index commands the slot, NaN = none */
  int32_t num_obs_cells;              /* FS_ENV_BOTTLENECK_DV: observed lane-segments (<= 64; <= 128 with num_vehicles > 64),
                                         obs_dim = 4 * cells + 1 */
  /* ---- FS_NET_BOTTLENECK ---- */
  double merge1_x, merge2_x;          /* coordinates where lanes (2q, 2q+1) join / where the two resulting lanes join */
  double zipper_distance;             /* a vehicle this close to a join follows the nearest vehicle of either joining lane */
  double speed_limit;                 /* edge speed limit: desired speed = min(vehicle maxSpeed, speed_limit); 0 = none */
  double outflow_norm;                /* 2000 * scaling: normaliser of the outflow reward */
  const fs_cell* obs_cells;           /* [num_obs_cells] in observation order (edge, segment, lane) */
  const fs_cell* act_cells;           /* [num_rl] controlled lane-segments, action column order */
  int32_t obs_outflow_window;         /* int(20 * sim_step / sim_step): sub-steps of the observed outflow */
  int32_t reward_outflow_window;      /* int(10 * sim_step / sim_step) */
  int32_t track_followers;            /* open networks: 1 = keep the sticky follower entries (FS_FIELD_FOLLOWER, used by the
                                         merge observations and BCM); 0 = skip them (the bottleneck envs never read them) */
  int32_t num_paths;                  /* FS_NET_BOTTLENECK: entry lanes = 4 * scaling: 4 (0 = 4) or 8 (8 -> 4 -> 2 lanes;
                                         needs num_vehicles > 64, i.e. the workgroup-per-replica kernel) */
  /* ---- simplified lane changing on FS_NET_BOTTLENECK (docs/HISTORY.md M11) ---- */
  int32_t lane_change_cooldown_steps; /* sub-steps a vehicle keeps its lane after a change */
  int32_t reserved6;
  double lane_change_min_gain;        /* leader-gap gain [m] a lane change must bring */
  /* ---- observation order of AccelEnv-style heads on single-lane closed loops ---- */
  int32_t sort_vehicles;              /* env_params 'sort_vehicles' (accel.py:101-169): observation entries and RL action
                                         columns follow the absolute position recorded at the last additional_command */
  int32_t noise_exact;                /* 0: the acceleration noise's Box-Muller uses the hardware's log2 / cos (fast; agrees with
                                         numpy to a few ulp of the draw); 1: log and cos are fixed sequences of float32
                                         multiplications, additions and one division (flowsim_kernels.h bm_ln_exact /
                                         bm_cos_exact; oracle/refsim.py exact_ln_f32 / exact_cos_turns_f32) -- the float32
                                         kernels then reproduce the numpy oracle's noisy runs bit for bit
                                         (SumoParams(noise_math='exact'); base_controller.py:109-110) */
  const int32_t* obs_perm;            /* [N] place of slot i's vehicle in get_ids() when InitialConfig.shuffle assigned the
                                         start positions in shuffled id order (envs/base.py:268-292); NULL = identity */
  /* ---- sharding ---- */
  int64_t replica_offset;             /* global index of this handle's replica 0 (one handle per GPU holds a contiguous
                                         block of the job's replicas): the Philox streams (acceleration noise, random
                                         entry lanes) are keyed by offset + local index, so a replica's trajectory does
                                         not depend on how the job is sharded */
  /* ---- FS_ENV_USER ---- */
  double user_env_p[8];               /* the user head's parameters p[0..7] (flow_amd.envs.CompiledEnv(params=...)); read by
                                         FS_ENV_USER handles only */
} fs_config;

typedef struct fs_sim* fs_handle;

/* ---- life cycle ----------------------------------------------------------
 * fs_create replaces Env.__init__ -> Kernel / generate_network /
 * start_simulation / setup_initial_state (flow/envs/base.py:102-229,
 * 268-292; flow/core/kernel/simulation/traci.py:70-174).
 * fs_destroy replaces Env.terminate (flow/envs/base.py:680-703). */
int fs_create(const fs_config* cfg, fs_handle* out);
void fs_destroy(fs_handle h);
const char* fs_last_error(void);
int fs_abi_version(void);

/* observation / action width of the configured env (observation_space.shape[0], action_space.shape[0]) */
int fs_obs_dim(fs_handle h);
int fs_action_dim(fs_handle h);

/* Enqueue all later work of this handle on `hip_stream` (a hipStream_t; NULL is
 * HIP's default stream).  fs_use_own_stream goes back to the non-blocking stream
 * the handle created for itself. */
int fs_set_stream(fs_handle h, void* hip_stream);
int fs_use_own_stream(fs_handle h);
/* Block until the handle's stream is idle. */
int fs_sync(fs_handle h);

/* ---- reset ---------------------------------------------------------------
 * Env.reset (flow/envs/base.py:414-560): re-place the vehicles of the
 * replicas selected by mask (uint8[R], NULL = all) at their initial state,
 * zero their time counters, then run warmup_steps steps with no RL action.
 * obs_out (real32[R,obs_dim], may be NULL) receives the observation of every
 * replica after the call. */
int fs_reset(fs_handle h, const uint8_t* mask, float* obs_out);
int fs_reset_dev(fs_handle h, const uint8_t* mask_dev, float* obs_dev);

/* ---- step ----------------------------------------------------------------
 * Env.step (flow/envs/base.py:294-412) for all R replicas: sims_per_step
 * sub-steps of {controllers -> fail-safes -> apply_acceleration
 * (vehicle/traci.py:952-963) -> simulation_step (simulation/traci.py:54-56)
 * -> vehicle update (vehicle/traci.py:119-259) -> check_collision}, then
 * get_state / compute_reward / done.
 *   actions  real32[R,A] or NULL (reference: rl_actions=None); A = num_rl, or 2*num_rl for
 *            FS_ENV_LANE_CHANGE_ACCEL (fs_action_dim)
 *   obs      real32[R,obs_dim]     rew  real32[R]     done  uint8[R]
 * Observations are float32 as in the reference's Box(dtype=np.float32). */
int fs_step(fs_handle h, const float* actions, float* obs, float* rew, uint8_t* done);
int fs_step_dev(fs_handle h, const float* actions_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev);

/* K consecutive Env.step calls in one launch (state stays in registers).
 *   actions_dev  real32[K,R,num_rl] (action_stride_steps = R*num_rl),
 *                or one real32[R,num_rl] reused every step (stride 0), or NULL
 *   obs_dev      real32[K,R,obs_dim] if obs_every_step, else real32[R,obs_dim] (last step)
 *   rew_dev      real32[K,R] / real32[R]      done_dev uint8[K,R] / uint8[R]
 *   done: 0 = the episode goes on; non-zero = done, bit 0: the horizon was reached (time_counter >= sims_per_step *
 *   (warmup_steps + horizon)), bit 1: a collision ended it (envs/base.py:381-400)
 * A replica that is done keeps stepping (the caller resets it, as
 * Experiment.run / RLlib do after `done`, flow/core/experiment.py:144-161). */
int fs_rollout_dev(fs_handle h, int num_steps, const float* actions_dev, size_t action_stride_steps,
                   float* obs_dev, float* rew_dev, uint8_t* done_dev, int obs_every_step);

/* ---- state access --------------------------------------------------------
 * dst/src are host buffers of `bytes` bytes holding the field in the
 * handle's precision (float or double) or int32 for FS_FIELD_TIME. */
int fs_get_state(fs_handle h, int field, void* dst, size_t bytes);
int fs_set_state(fs_handle h, int field, const void* src, size_t bytes);

/* k.vehicle.add(veh_id, type_id, edge, pos, lane, speed) (flow/core/kernel/vehicle/traci.py:1089-1122 -> TraCI vehicle.add)
 * for a vehicle that HAS a slot and is not in the network: BottleneckAccelEnv.additional_command re-inserts an RL vehicle
 * that left (flow/envs/bottleneck.py:733-757, add_rl_if_exit).  Open networks only.  The vehicle of `slot` (which must be
 * empty: FS_ERR_INVALID otherwise) is placed at route coordinate `x` [m] on entry lane / route `route` with `speed`
 * [m/s], joins the END of the id list (FS_FIELD_SEQ), with its type's maxSpeed and no lane-change history; the
 * neighbour fields (FS_FIELD_LEADER / HEADWAY) are refreshed.  Whether the vehicle fits is the caller's test (the
 * reference lets TraCI raise and ignores it).  Host call between launches: synchronises the handle's stream. */
int fs_add_vehicle(fs_handle h, int replica, int slot, int route, double x, double speed);

/* Family of the step kernel the handle's last fs_step / fs_rollout / fs_policy_rollout launch chose ("k_rollout_pair" with
 * "+speed_mode" and / or "+noise", "k_rollout_idm", "k_ring_pair<Accel | PO | POMA | AccelMA>", "k_rollout_loop",
 * "k_rollout_loop<FULL>", "k_rollout_loop<AccelMA>", "k_rollout_loop<FULL,AccelMA>", "k_ring_policy", "k_loop_policy",
 * "k_ring_policy<POMA>", "k_loop_policy<AccelMA>", "k_merge_policy", "k_merge_policy<PO>", "k_merge_policy<PO,WIDE>",
 * "k_loop_policy<AccelVec>", "k_loop_policy<Adversarial>" (fs_policy_pair_rollout_dev; fs_policy_pair_act_dev:
 * "k_policy_pair_act")
 * (fs_policy_act_dev: "k_policy_act", "k_policy_act_vec", "k_policy_act_wide", "k_policy_act_row"; the PPO update's entry points: "k_ppo_eval",
 * "k_gae", "k_ppo_grad", "k_adv_stats", "k_adv_finish", "k_adam"; fs_episode_stats_dev: "k_episode_stats";
 * fs_population_*: the policy kernel's name with the tag Population, e.g. "k_ring_policy<Population>",
 * "k_ring_policy<POMA,Population>" -- that one string lives in the handle and is valid until its next launch; fs_es_*:
 * "k_es_perturb", "k_es_fitness", "k_es_weights", "k_es_grad"),
 * "k_steps<FAST>", "k_steps<CSET>", "k_steps", "k_steps_ml", "k_steps_open" (also "<mixed>"), "k_steps_wide",
 * "k_merge_queue", "k_drop_queue", "k_obs_mixed"; "" before the first launch).  Diagnostics for tests and bench.py: which
 * configuration class a workload landed in (no reference counterpart).  The string is static.
 * The queue-order kernel of the merge network (k_merge_queue) steps both merge heads, FS_ENV_MERGE_PO and
 * FS_ENV_MERGE_MA, on FS_F32 / FS_F16S handles: IDM (delta = 4) / RL / SUMO-driven slots of one length without fail-safes,
 * Euler, scheduled inflows, at most 64 slots, launches of one or more steps without a replica mask; every other launch
 * of such a handle (warm-up, masked or zero-step launches) and every other configuration steps on k_steps_open.
 * The queue-order kernel of the lane-drop network (k_drop_queue) reports a replica that outgrew its layout (more than
 * 64 vehicles on one entry path, more than 8 arrivals in one sub-step) through fs_sync /
 * fs_get_state: FS_ERR_UNSUPPORTED with fs_last_error naming it; FLOWSIM_NO_QUEUE=1 in the environment of fs_create
 * keeps a handle on the slot-order kernels. */
const char* fs_last_kernel(fs_handle h);

/* ---- policy in the loop ------------------------------------------------------
 * What examples/train.py:110-212 runs per rollout worker -- policy forward pass, Env.step, reset of a finished episode,
 * one Python call and N socket round trips per step -- as ONE launch per fragment of K steps.  Built for the
 * reference's RL ring experiments (examples/exp_configs/rl/singleagent/singleagent_ring.py: IDM vehicles + ONE RL
 * vehicle, WaveAttenuationPOEnv: observation 3, action 1), for its figure-eight experiment
 * (singleagent_figure_eight.py: FS_NET_FIGURE_EIGHT, 13 IDM + ONE RL vehicle, AccelEnv: observation 2 N = 28, or the
 * WaveAttenuationPOEnv head: observation 3) and its default model class: a fully connected network of 1..3
 * hidden layers of 32 tanh units (examples/train.py:152 fcnet_hiddens [32, 32, 32]) with a diagonal Gaussian head.
 *   weights_dev  float32, device: per layer W [out][in] row-major then b [out]; the last layer has 2 outputs (mean,
 *                log std: RLlib's DiagGaussian) or, with log_std_dev != NULL, 1 output and a free log std [1]
 *   seed         keys the action sampling streams (Philox, per global replica, continued from fragment to fragment)
 * The arithmetic (fma order, hardware exp2 / rcp) is defined by flow_amd/csrc/flowsim_policy.h; fs_policy_act_dev is
 * the SAME evaluation as a call of its own, so fs_policy_rollout_dev equals K x (fs_policy_act_dev, fs_step_dev
 * [, fs_reset_dev(done)]) bit for bit.  Other environments / models: FS_ERR_UNSUPPORTED (capture K single steps
 * around any policy instead: flow_amd.envs.VecFlowEnv.capture).
 * Shared agents (the reference's multi-agent experiments map every agent to ONE policy): FS_ENV_WAVE_ATTENUATION_PO_MA on
 * a single-lane ring (multiagent_ring.py; 18..32 vehicles, IDM / RL, Euler, track_aux = 0, warm-up steps inside the
 * fragment allowed) and FS_ENV_ACCEL_PO_MA on a segment-table loop (multiagent_figure_eight.py; up to 16 vehicles,
 * warmup_steps = 0 when a fragment resets), float32 handles only.  Agent c is the RL vehicle with rl_index c: its
 * observation is block c of the observation row, its action column c (the layout of fs_step_dev for these heads);
 * n_ag = num_rl agents, and obs_dim must be ONE agent's block, fs_obs_dim / num_rl (3 or 6).  fs_policy_act_dev takes
 * obs [R, n_ag * obs_dim] and writes act / logp [R, n_ag]: agent c of replica r draws from Philox column 0x40000000 + c
 * at the replica's counter, which advances by one per call (c = 0 is the single-agent stream).  fs_policy_rollout_dev
 * takes obs [K+1, R, n_ag * obs_dim], act / logp [K, R, n_ag], rew / done [K, R] (the reward all agents share; a
 * collision ends nothing and zeroes no reward, multiagent/base.py:188-190).  FS_MIXED / FS_F64 with a multi-agent head and
 * FS_ENV_ACCEL_PO_MA on a ring are refused by name.
 * The multi-agent merge (FS_ENV_MERGE_MA, multiagent_merge.py) with ma_apply_actions = 1, FS_F32 or FS_F16S handles that
 * step on k_merge_queue (the queue-order kernel's conditions: no FLOWSIM_NO_QUEUE, scheduled inflows, no fail-safes, ...;
 * "k_merge_policy"): n_ag = num_rl agents, obs_dim = 5, the same layouts.  Agent c is the RL slot of column c, and it is
 * ABSENT while that slot holds no vehicle in the state its observation is taken from (fs_policy_act_dev: the handle's
 * current state; its observation block is zero).  An absent agent gets act = NaN (fs_step_dev's "no command") and
 * logp = 0; a present agent draws as above, and the counter advances by one per step whether or not any agent is
 * present (the reference lists only the RL vehicles present, flow/envs/multiagent/merge.py:98-143).  Resets inside a
 * fragment: warmup_steps = 0.  ma_apply_actions = 0 (the shipped environment: actions never reach the simulator, roll it
 * out open loop), FS_MIXED / FS_F64 and handles off the queue kernel are refused by name.
 * The single-agent merge (FS_ENV_MERGE_PO, singleagent_merge.py; "k_merge_policy<PO>", with more than six places
 * "k_merge_policy<PO,WIDE>") takes an ACTION-VECTOR head: ONE network maps the whole observation to A = num_rl
 * (fs_action_dim, 1..32) accelerations, evaluated once per replica and step.
 *   obs_dim      fs_obs_dim = 5 A: the whole observation.  A <= 6 (at most 32 inputs): "k_policy_act_vec" /
 *                "k_merge_policy<PO>".  A = 7..32 (35..160 inputs; EXP_NUM 1 and 2 of singleagent_merge.py: 13 and 17): the
 *                wide head's first layer, "k_policy_act_wide" / "k_merge_policy<PO,WIDE>" -- its sum runs over chunks of
 *                32 inputs in an order that depends on obs_dim alone, and lane c of the replica's wave samples column c
 *   weights_dev  the same trunk; the last layer has 2 A outputs -- rows 0 .. A-1 the means, rows A .. 2A-1 the log stds:
 *                RLlib's DiagGaussian order -- or, with log_std_dev != NULL, A outputs and log_std_dev points at A floats
 * Column c draws from Philox column 0x40000000 + c at the replica's counter (the stream agent c of the shared-policy heads
 * uses), which advances by one per step; logp is the JOINT log-probability: the columns' values added in ascending column
 * order, in float32.  Every column is sampled every step -- MergePOEnv ignores the columns beyond its list of controlled
 * vehicles, as it does on an action tape; there is no absent agent on this head.  fs_policy_act_dev takes obs [R, 5 A]
 * and writes act [R, A] and logp [R]; fs_policy_rollout_dev takes obs [K+1, R, 5 A], act [K, R, A] and logp / rew / done
 * [K, R].  Clipping stays where fs_step_dev does it (act holds the samples).  reset_done: a collision ends the episode on
 * this head (bit 1 of done), so a replica is reset in place when done != 0 -- the horizon or a collision -- exactly as
 * fs_reset_dev(done != 0) resets it: the list of controlled vehicles and its join counter survive, FS_F16S states are
 * rounded through halves between steps.  A fragment equals K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done)) bit
 * for bit, on either kernel.  Refused by name (every message names FS_ENV_MERGE_PO): num_rl outside 1..32 (fs_create
 * refuses more than 32 itself), FS_MIXED / FS_F64, handles off the queue kernel, warmup_steps != 0 together with
 * reset_done, and obs_dim != fs_obs_dim (any other policy can run around the step: VecFlowEnv.capture).
 * The lane drop (FS_ENV_BOTTLENECK_DV, singleagent_bottleneck.py: 141 observations, 20 speed offsets) takes the same
 * action-vector head through fs_policy_act_dev ONLY ("k_policy_act_wide", FS_F32 handles): A = num_rl action cells
 * (1..64), obs_dim = fs_obs_dim = 4 cells + 1 (up to 513), the last layer 2 A rows (means, then log stds) or A rows next
 * to A free log stds; obs [R, obs_dim] -> act [R, A], logp [R].  Column c is sampled by lane c of the replica's wave from
 * Philox column 0x40000000 + c at the replica's counter (keyed by the global replica id), which advances by one per call;
 * logp is the float32 sum of the columns in ascending order.  The first layer's sum runs over chunks of 32 inputs in an
 * order that depends on obs_dim alone (flowsim_policy.h policy_wide_layer1), never on R or the launch.
 * fs_policy_rollout_dev is refused by name on these handles (no fused kernel yet): capture K x (fs_policy_act_dev,
 * fs_step_dev, fs_reset_dev(done)) as one graph instead (VecFlowEnv.capture with a DevicePolicy).  Every refusal on
 * this head -- another precision, obs_dim != fs_obs_dim, num_rl outside 1..64, the model class -- names
 * FS_ENV_BOTTLENECK_DV.
 * AccelEnv with SEVERAL RL vehicles on a segment-table loop (FS_ENV_ACCEL without evaluate, num_rl = 2..16 among 9..16
 * vehicles: the reference's flow/benchmarks/figureeight1.py, 7 IDM + 7 RL vehicles, 28 -> 7, and figureeight2.py, 14 RL
 * vehicles, 28 -> 14) takes the same ACTION-VECTOR head with a ROW of 16 lanes per replica ("k_policy_act_row" /
 * "k_loop_policy<AccelVec>"; flowsim_policy.h policy_row_vec_act): obs_dim = fs_obs_dim = 2 N (at most 32: the first layer
 * of the AccelEnv head with one RL vehicle), the last layer 2 A rows (means, then log stds) or A rows next to A free log
 * stds at log_std_dev, A = num_rl.  Column c belongs to the RL vehicle with rl_index c, whatever its slot; it draws from
 * Philox column 0x40000000 + c at the replica's counter, which advances by one per call / step, and logp is the float32
 * sum of the columns' values in ascending column order.  fs_policy_act_dev takes obs [R, 2 N] and writes act [R, A] and
 * logp [R]; fs_policy_rollout_dev takes obs [K+1, R, 2 N], act [K, R, A] and logp / rew / done [K, R] (FS_ENV_MERGE_PO's
 * layouts); a fragment equals K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done)) bit for bit.  The conditions are
 * those of the head with one RL vehicle -- FS_F32, a row of 16 lanes, IDM / RL / Sim vehicles, no fail-safes, Euler,
 * track_aux = 0, no sorting, warmup_steps = 0 when a fragment resets --, and num_rl = 1 keeps its path and kernel names.
 * Refused by name, each message naming FS_ENV_ACCEL and num_rl: FS_MIXED / FS_F64; the WaveAttenuationPOEnv head with
 * num_rl > 1; fs_policy_pair_* (two policies drive ONE RL vehicle); fs_population_* ("fs_population: ...").
 * The mean action (greedy != 0; every kernel named above, eager and fused, and fs_policy_pair_* per policy): act = the
 * head's mean EXACTLY (a select: no std enters it, so it stays finite where exp(log std) overflows) and logp =
 * (-log_std) - 0.9189385332046727f, the density at the mean -- the sampling expression with a zero draw; the action-vector
 * heads add their columns in the order they add them when sampling.  The draw counters advance exactly as they do when
 * sampling (one per call or step, absent agents included; an absent agent still gets NaN and 0), so greedy and sampling
 * calls interleave on one stream: a sampling call after n greedy calls draws what it draws after n sampling calls.  The
 * Gaussian head only.  greedy occupies four bytes that were padding before the first pointer: sizeof(fs_policy) and every
 * other offset are unchanged, and a C caller MUST ZERO the struct (memset, or = {0}) before filling it -- a caller that
 * left the padding uninitialised would switch the mean action on by accident.  On the k_loop_policy family the flag picks
 * the kernel's instantiation (the same fs_last_kernel names; "k_loop_policy<AccelVec>" reads it at run time); every other kernel reads it at run time. */
typedef struct fs_policy {
  uint32_t struct_size;               /* sizeof(fs_policy) */
  int32_t obs_dim;                    /* must equal fs_obs_dim (FS_ENV_MERGE_PO / BOTTLENECK_DV too); shared agents: fs_obs_dim / num_rl */
  int32_t num_hidden;                 /* 1..3 hidden layers ... */
  int32_t hidden_width;               /* ... of 32 units each */
  int32_t activation;                 /* 0 = tanh */
  int32_t greedy;                     /* != 0: act = the mean, logp = the density at the mean (see above); 0: sample */
  const float* weights_dev;
  const float* log_std_dev;           /* NULL: the network's second output is the log std (action-vector heads: [num_rl]) */
  uint64_t seed;
} fs_policy;

/* actions [R] and log-probabilities [R] for the observations obs_dev [R, obs_dim] ([R, n_ag] for [R, n_ag * obs_dim] with
 * shared agents; FS_ENV_MERGE_PO and FS_ENV_BOTTLENECK_DV: actions [R, num_rl], log-probabilities [R]); advances the
 * sampling streams by one draw per replica.  One kernel launch on the handle's stream, no host synchronisation: it can be
 * captured into a graph between fs_step_dev launches (after one eager call, which allocates the draw counters).
 * FS_ENV_USER (FS_F32 handles, "k_policy_act"): with kUserObsRlOnly, n_ag = num_rl agents share the policy, obs_dim =
 * kUserObsPerVehicle, the shared agents' layouts; without it and with num_rl = 1, one agent with obs_dim = fs_obs_dim
 * <= 32.  Every other form is refused by a message that names FS_ENV_USER. */
int fs_policy_act_dev(fs_handle h, const fs_policy* pol, const float* obs_dev, float* act_dev, float* logp_dev);
/* K x (policy -> action -> Env.step), with reset_done != 0 followed by Env.reset of the replicas whose episode ended
 * (placement, FS_FIELD_INIT_RING_LENGTH, warm-up steps).  obs_dev [K+1, R, obs_dim]: obs[0] = observation of the state
 * the fragment starts from (written by the call), obs[k+1] = observation after step k (after the reset, if one
 * happened); act_dev [K, R], logp_dev [K, R] ([K, R, n_ag] with shared agents; FS_ENV_MERGE_PO: act_dev [K, R, num_rl],
 * logp_dev [K, R]), rew_dev [K, R], done_dev [K, R] (flags as in fs_rollout_dev). */
int fs_policy_rollout_dev(fs_handle h, const fs_policy* pol, int num_steps, int reset_done, float* obs_dev,
                          float* act_dev, float* logp_dev, float* rew_dev, uint8_t* done_dev);

/* ---- two policies, one RL vehicle (fs_policy_pair) ----------------------------
 * The reference's adversarial experiment (examples/exp_configs/rl/multiagent/adversarial_figure_eight.py:
 * AdversarialAccelEnv, 13 IDM vehicles + ONE RL vehicle on the figure eight) maps its two agents to a policy each: 'av'
 * and 'adversary' read the SAME observation (AccelEnv's, 2 N values), each draws an action, the vehicle receives
 * av + perturb_weight * adversary, and the adversary's reward is the negation of the av's.  Two fs_policy structs (the
 * model class above; they may differ in num_hidden and in the form of their head) drive the one action column of an
 * FS_ENV_ACCEL handle:
 *   act / logp   agent-major planes: plane 0 the av, plane 1 the adversary (each agent's [K, R] is contiguous: a learner
 *                takes it without a copy)
 *   draws        the av: Philox column 0x40000000 (the single-agent stream) keyed by ITS seed; the adversary: column
 *                0x40000000 + 1 keyed by ITS seed (equal seeds still give independent draws); both at the replica's
 *                counter -- the handle's, shared by the two policies and by fs_policy_act_dev --, which advances by ONE per
 *                call / step
 *   cmd          fmaf(perturb_weight, a_adversary, a_av), float32: THE combination.  fs_step_dev takes cmd [R] as its action
 *                column; clipping stays where fs_step_dev does it (act holds the samples)
 *   rew          the av's reward (desired velocity: it does not read the action); the adversary's is -rew
 * fs_policy_pair_act_dev ("k_policy_pair_act"): obs_dev [R, 2 N] -> act_dev / logp_dev [2, R], cmd_dev [R]; one launch, no
 * host synchronisation.  fs_policy_pair_rollout_dev ("k_loop_policy<Adversarial>"): obs_dev [K+1, R, 2 N], act_dev /
 * logp_dev [2, K, R], rew_dev / done_dev [K, R], reset_done as in fs_policy_rollout_dev.  A fragment equals
 * K x (fs_policy_pair_act_dev, fs_step_dev(cmd), fs_reset_dev(done)) bit for bit, and with perturb_weight = 0 its obs,
 * plane 0, rew and done are fs_policy_rollout_dev(av)'s.
 * Accepted: what fs_policy_rollout_dev takes for the AccelEnv head on a segment-table loop -- FS_F32, FS_ENV_ACCEL without
 * evaluate, num_rl = 1, 9..16 vehicles, the configuration k_rollout_loop steps, warmup_steps = 0 when a fragment resets --
 * with obs_dim = 2 N for BOTH policies.  Everything else -- rings and open networks, other heads, other precisions -- is
 * FS_ERR_UNSUPPORTED, refused before anything launches, with a message that names fs_policy_pair; a perturb_weight that
 * is not finite is FS_ERR_INVALID. */
int fs_policy_pair_act_dev(fs_handle h, const fs_policy* av, const fs_policy* adversary, float perturb_weight,
                           const float* obs_dev /*[R, D]*/, float* act_dev /*[2, R]*/, float* logp_dev /*[2, R]*/,
                           float* cmd_dev /*[R]*/);
int fs_policy_pair_rollout_dev(fs_handle h, const fs_policy* av, const fs_policy* adversary, float perturb_weight,
                               int num_steps, int reset_done, float* obs_dev /*[K+1, R, D]*/, float* act_dev /*[2, K, R]*/,
                               float* logp_dev /*[2, K, R]*/, float* rew_dev /*[K, R]*/, uint8_t* done_dev /*[K, R]*/);

/* ---- policy populations (fs_population) ----------------------------------------
 * M weight sets in ONE launch of the scalar-head policy kernels: replica r evaluates the set at
 * pol->weights_dev + (r / group) * stride; everything else -- log_std_dev, the seed, the draw counters, greedy, every
 * buffer layout -- is fs_policy_act_dev's and fs_policy_rollout_dev's.  A workgroup of those kernels copies the weights
 * into its LDS once per launch and serves fs_population_granule (16) replicas, so group must be a multiple of the granule:
 * the member is then the same for a whole workgroup and nothing after the load differs from the single-policy launch.
 * Rows [m group, (m + 1) group) of a population fragment equal, bit for bit, the same rows of fs_policy_rollout_dev with
 * weight set m on an identically created handle; stride = 0 (all share set 0) and members = 1 equal it on every row.
 * fs_last_kernel: the family's name with Population among its tags ("k_ring_policy<Population>",
 * "k_ring_policy<POMA,Population>", "k_loop_policy<Population>", "k_policy_act<Population>").
 * Refused before anything launches, FS_ERR_INVALID / FS_ERR_UNSUPPORTED with a message that starts "fs_population: ":
 * group not a multiple of the granule; members * group != num_replicas; 0 < stride < the policy's own size in floats;
 * the action-vector heads (FS_ENV_MERGE_PO, FS_ENV_BOTTLENECK_DV) and FS_ENV_MERGE_MA (their kernels give a WAVE to a
 * replica and read first-layer or output weights past the LDS copy) and FS_ENV_ACCEL with num_rl > 1 (the row-per-replica
 * action-vector head: a member's size and stride count one action column).  There is no population form of fs_policy_pair.
 * Whatever fs_policy_rollout_dev refuses on the handle is refused here with its message ("fs_policy: ..."). */
typedef struct fs_population {
  uint32_t struct_size;               /* sizeof(fs_population) */
  int32_t members;                    /* M >= 1 */
  int32_t group;                      /* replicas per member; num_replicas == members * group */
  int32_t reserved;                   /* 0 */
  int64_t stride;                     /* floats between consecutive members' weight sets, >= the policy's own size; 0: all share set 0 */
} fs_population;

/* replicas per workgroup of the kernel that would run for this handle and policy; < 0: a refusal (fs_last_error) */
int fs_population_granule(fs_handle h, const fs_policy* pol);
int fs_population_act_dev(fs_handle h, const fs_policy* pol, const fs_population* pop, const float* obs_dev,
                          float* act_dev, float* logp_dev);
int fs_population_rollout_dev(fs_handle h, const fs_policy* pol, const fs_population* pop, int num_steps, int reset_done,
                              float* obs_dev, float* act_dev, float* logp_dev, float* rew_dev, uint8_t* done_dev);

/* ---- evolution strategies on the device (flow_amd/csrc/flowsim_es.h) ------------
 * ES (Salimans et al. 2017, RLlib's ES) and ARS (Mania et al. 2018, RLlib's ARS) around fs_population_rollout_dev: N
 * antithetic pairs and E evaluation members, M = 2 N + E weight sets.  Every call is launches on the handle's stream, no
 * host synchronisation, capturable; no float atomics; every summation order is fixed by the shapes (flowsim_es.h states
 * each).  The noise is never stored: eps(p, e) = the library's exact Box-Muller draw (fs_config.noise_exact's sequences;
 * oracle/refsim.py gaussian_noise(exact=True) bit for bit) of Philox key noise_seed, counter (e / 4, 0x60000000 |
 * generation, p, 0), draw e % 4.
 *
 * fs_es_perturb_dev ("k_es_perturb"): weights_dev [M, stride] from theta_dev [P]: member 2 p = theta + t, member 2 p + 1 =
 *   theta - t, t = sigma * eps(p, e) (one float32 multiply, then one float32 add / subtract); members 2 N .. M - 1 = theta.
 *   Floats P .. stride - 1 of a row are left alone.
 * fs_es_fitness_dev ("k_es_fitness"): rew_dev / done_dev [K, R] of a fragment -> ret_dev [R] (double), alive_dev [R],
 *   fit_dev [M] (double).  A replica adds its rewards in double, k ascending, up to and including its first done != 0;
 *   after that it is dead (alive = 0).  fit[m] = (sum of ret over the member's replicas, r ascending) / group.
 *   accumulate != 0 continues from ret_dev / alive_dev as an earlier call left them; 0 starts at ret = 0, alive = 1.
 * fs_es_weights_dev ("k_es_weights"): fit_dev [0, 2 N) -> u_dev [N] (float32), stats_dev [4] (double) = {mean, min, max
 *   of the 2 N perturbed returns, mean of the E evaluation members (NaN with E = 0)}.
 *   FS_ES_MODE_ES: rank = position in the ascending order of (value, index); c = (float)(rank / (2 N - 1) - 0.5), the
 *     quotient and difference in double; u[p] = (c[2 p] - c[2 p + 1]) / (float)N in float32.
 *   FS_ES_MODE_ARS: the top directions by max(F+, F-) descending (ties: p ascending) are kept (top <= 0 or > N: all N);
 *     s = the population standard deviation of the 2 b kept returns, in double (mean and squared deviations summed over
 *     the kept directions in ascending p, F+ before F-); u[p] = (float)((F+ - F-) / (b s)) kept, 0 otherwise; s == 0: all 0.
 * fs_es_grad_dev ("k_es_grad"): g[e] = sum over p of u[p] * eps(p, e) in float32 (order: flowsim_es.h), the noise
 *   regenerated.  FS_ES_MODE_ES: grad_dev[e] = -g[e] + l2 * theta_dev[e] (what fs_adam_dev takes); theta is not written.
 *   FS_ES_MODE_ARS: theta_dev[e] = theta_dev[e] + stepsize * g[e] in the same launch; grad_dev may be NULL.
 *   work_dev: fs_es_workspace(num_params, pairs) floats.  pairs <= 2048, num_params <= 2^24. */
enum { FS_ES_MODE_ES = 0, FS_ES_MODE_ARS = 1 };
#define FS_ES_MAX_PAIRS 2048
int fs_es_perturb_dev(fs_handle h, int64_t num_params, int pairs, int eval_members, int64_t stride, const float* theta_dev,
                      float sigma, uint64_t noise_seed, uint32_t generation, float* weights_dev);
int fs_es_fitness_dev(fs_handle h, int num_steps, int members, int group, const float* rew_dev, const uint8_t* done_dev,
                      int accumulate, double* ret_dev, uint8_t* alive_dev, double* fit_dev);
int fs_es_weights_dev(fs_handle h, int mode, int pairs, int eval_members, int top, const double* fit_dev, float* u_dev,
                      double* stats_dev);
size_t fs_es_workspace(int64_t num_params, int pairs);
int fs_es_grad_dev(fs_handle h, int mode, int64_t num_params, int pairs, const float* u_dev, uint64_t noise_seed,
                   uint32_t generation, float l2_or_stepsize, float* theta_dev, float* grad_dev, float* work_dev,
                   size_t work_floats);

/* ---- the PPO update on the device ---------------------------------------------
 * What examples/train_vec.py ppo_update runs in torch between two rollouts -- the no_grad pass, generalised advantage
 * estimation, and per epoch the forward pass, the clipped-surrogate loss and autograd's backward pass over a policy and a
 * value network -- as three launches on the handle's stream (kernels: flow_amd/csrc/flowsim_learn.h).  The handle lends its
 * device, its stream and fs_last_error; none of the calls touches the simulation state, none synchronises the host, so a
 * sequence of them can be captured into a graph.  fs_last_kernel reports "k_ppo_eval", "k_gae", "k_ppo_grad"
 * (and "k_adv_stats", "k_adv_finish", "k_adam" for the statistics and the optimiser below).
 * Model class (fs_policy's): 1..3 hidden layers of 32 tanh units on obs_dim = 1..160 inputs; the policy's head has act_dim
 * = 1..32 outputs, the MEANS, next to a free log std [act_dim]; the value network is the same trunk with one output.
 * Both weight buffers: float32, device, per layer W [out][in] row-major then b [out].
 * log_std_dev == NULL (fs_policy's convention) selects the head of 2 act_dim outputs instead: the policy's last layer has
 * 2 A rows, rows 0 .. A-1 the means and rows A .. 2A-1 the log stds (RLlib's DiagGaussian order), so the standard deviation
 * depends on the observation and there is no free log std.  The packed parameters are then [policy with its 2A-row head]
 * [value weights] -- P = 2 (32 D + 32 + (num_hidden - 1) 1056) + 66 A + 33 -- and every sum's order depends on the head's
 * form as well.  fs_ppo_eval_dev, fs_ppo_eval_dist_dev, fs_ppo_grad_n_dev, fs_ppo_grad_loss_dev, fs_ppo_minibatch_dev,
 * fs_ppo_mb_finish_dev and the three workspace functions take it (fs_last_kernel: "k_ppo_eval_ls", "k_ppo_grad_ls",
 * "k_ppo_grad_loss_ls", "k_ppo_minibatch_ls"); fs_ppo_grad_dev, the gradient with the sample count from the host, refuses it.
 * Everything else -- another width or activation, obs_dim / act_dim out of range -- is refused with FS_ERR_UNSUPPORTED and a
 * message that names fs_ppo_model. */
typedef struct fs_ppo_model {
  uint32_t struct_size;               /* sizeof(fs_ppo_model) */
  int32_t obs_dim;                    /* D: 1..160 */
  int32_t act_dim;                    /* A: 1..32 */
  int32_t num_hidden;                 /* 1..3 hidden layers ... */
  int32_t hidden_width;               /* ... of 32 units each */
  int32_t activation;                 /* 0 = tanh */
  const float* policy_weights_dev;    /* [32 D + 32][(num_hidden - 1) x 1056][33 A]   (log_std_dev == NULL: [.. 33 x 2A]) */
  const float* log_std_dev;           /* [A]; NULL: the head has 2 A outputs, rows A .. 2A-1 are the log stds */
  const float* value_weights_dev;     /* [32 D + 32][(num_hidden - 1) x 1056][33] */
} fs_ppo_model;

/* Forward only: logp_dev [n] = log-probability of act_dev [n, A] under the policy at obs_dev [n, D] (the sum over the
 * columns of -0.5 ((a - mean) / std)^2 - log_std - 0.9189385), val_dev [n] = the value network's output.  act_dev == NULL:
 * values only (logp_dev is not written, the policy's pointers are not read).  A sample whose action row holds a NaN is an
 * absent agent: its action is taken as 0 and its outputs mean nothing (ppo_update never uses them). */
int fs_ppo_eval_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                    float* logp_dev, float* val_dev);
/* Generalised advantage estimation over a fragment: rew, val, done, adv, ret [num_steps, num_cols], last_val [num_cols]; done
 * is the flag byte of fs_rollout_dev, and the episode went on where it is 0.  Backwards over t, in float32, exactly
 *   delta = (rew + (g * nxt) * live) - val;  run = delta + ((gl * live) * run);  adv = run;  ret = adv + val;  nxt = val
 * with g = (float)gamma, gl = (float)(gamma * lam): bit for bit what train_vec.gae computes with torch on the CPU. */
int fs_gae_dev(fs_handle h, int num_steps, int64_t num_cols, const float* rew_dev, const float* val_dev,
               const float* last_val_dev, const uint8_t* done_dev, double gamma, double lam, float* adv_dev, float* ret_dev);
/* Floats of work_dev that fs_ppo_grad_dev needs for n samples of this model (0: the model or n is not valid). */
size_t fs_ppo_workspace(const fs_ppo_model* model, int64_t n);
/* The gradient of ppo_update's loss over n samples, forward and backward in one launch plus a small reduction:
 *   adv_n = (float)((adv - mean) / (std + 1e-8))           adv_dev [n] and mean_std_dev = {mean, std} are float64, device
 *   ratio = exp(logp - logp_old);  pg = min(ratio adv_n, clamp(ratio, 1 - clip, 1 + clip) adv_n);  vf = (v - ret)^2
 *   loss  = (-sum pg + vf_coef sum vf) inv_n_total
 * grad_dev [P]: d loss / d parameter, packed as [policy weights][log_std A][value weights] (the layouts of fs_ppo_model);
 * loss_dev [2] = {sum pg, sum vf}.  accumulate != 0 adds both to what the buffers hold (several shards of one update).
 * Samples with a NaN in their action row are absent: they add nothing, and nothing of their rows reaches an output.
 * The sum over samples has a fixed order that depends on (n, obs_dim, act_dim, num_hidden) alone -- one partial gradient per
 * workgroup in work_dev, added in ascending order, no float atomics -- so the same inputs give the same bits on every call. */
int fs_ppo_grad_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                    const float* logp_old_dev, const double* adv_dev, const float* ret_dev, const double* mean_std_dev,
                    float clip, float vf_coef, float inv_n_total, int accumulate, float* grad_dev, float* loss_dev,
                    float* work_dev, size_t work_floats);

/* fs_ppo_grad_dev with the sample count on the device: mean_std_n_dev [3] = {mean, std, n} (what fs_adv_finish_dev writes)
 * replaces mean_std_dev [2] and the host argument inv_n_total; the kernel takes inv_n_total = (float)(1.0 / n), the bits a
 * host passes for the same n, so with inv_n_total = 1 / n both calls give the same bits.  One kernel body serves both. */
int fs_ppo_grad_n_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                      const float* logp_old_dev, const double* adv_dev, const float* ret_dev, const double* mean_std_n_dev,
                      float clip, float vf_coef, int accumulate, float* grad_dev, float* loss_dev, float* work_dev,
                      size_t work_floats);
/* The float64 advantage statistics of ppo_update.  adv_dev [n] float32 (fs_gae_dev's output); act_dev [n, act_dim] or NULL.
 * A row whose action row holds a NaN is absent (act_dev == NULL: every row is present).  Absent rows are selected out,
 * not multiplied by zero: nothing of such a row reaches an output, whatever its adv holds.
 *   adv64_dev [n] = (double)adv of a present row, 0 of an absent one     (the form fs_ppo_grad_dev reads)
 *   stats_dev [3] = {sum adv, sum adv * adv, count} over the present rows, in double
 * G = min(512, ceil(n / 1024)) workgroups of 256 lanes: lane t of workgroup b adds rows 256 b + t + 256 G k, k ascending;
 * the lanes of a workgroup meet in a binary tree (lane t += lane t + half, half = 128 .. 1); the workgroup that finishes
 * last (an integer ticket) adds the G partial sums: lane t those of workgroups t and t + 256, then the same tree.  The order depends on n alone and there are no float
 * atomics: the same inputs give the same bits.  accumulate != 0 adds the three sums to what stats_dev holds (several local
 * shards, in call order).  The first call on a handle allocates a few KB of scratch and synchronises the device once:
 * make it before a stream capture begins. */
int fs_adv_stats_dev(fs_handle h, int64_t n, const float* adv_dev, const float* act_dev, int act_dim, int accumulate,
                     double* adv64_dev, double* stats_dev);
/* RLlib's episode statistics from a fragment's rew_dev / done_dev [K, R] (K = num_steps, R = the handle's replicas), ONE
 * launch ("k_episode_stats") on the handle's stream, no host synchronisation: it can be captured into a graph (after one
 * eager call, which allocates a few KB of scratch and synchronises the device once).
 * Replica r is walked k = 0 .. K-1: run_ret[r] += (double)rew[k][r], run_len[r] += 1; where done[k][r] != 0 (any bit: the
 * horizon and a collision alike) the episode {run_ret, run_len} is emitted and both return to zero.  The carries
 * run_ret_dev / run_len_dev [R] are read at the start and written at the end (zero them before the first fragment): an
 * episode that straddles fragments counts once, in the fragment where it ends.
 *   stats_dev [8] = {episodes, sum ret, sum ret * ret, min ret, max ret, sum len, min len, max len}, in double; with no
 *   episode min is +inf and max -inf.  accumulate != 0 combines with what stats_dev holds: the sums add, min / max
 *   combine (several fragments, or several local shards in call order).
 * G = min(512, ceil(R / 256)) workgroups of 256 lanes: lane t of workgroup b walks replicas 256 b + t + 256 G j, j
 * ascending, and adds / combines the episodes it meets in that (j, k) order; the lanes of a workgroup meet in a binary
 * tree (lane t (+)= lane t + half, half = 128 .. 1, a lane without an episode holding {0, 0, 0, +inf, -inf, 0, +inf,
 * -inf}); the workgroup that finishes last (an integer ticket) combines the G partials: lane t those of workgroups t and
 * t + 256, then the same tree.  The order depends on (K, R) alone and there are no float atomics: the same inputs give
 * the same bits.  min / max are fmin / fmax. */
int fs_episode_stats_dev(fs_handle h, int num_steps, const float* rew_dev, const uint8_t* done_dev, double* run_ret_dev,
                         int32_t* run_len_dev, double* stats_dev, int accumulate);
/* One thread, in double, exactly (no contraction; division and square root correctly rounded)
 *   n = stats[2];  mean = stats[0] / n;  var = (stats[1] - (n * mean) * mean) / (n - 1);  std = sqrt(var < 0 ? 0 : var)
 * mean_std_n_dev [3] = {mean, std, n}: ppo_update's formula, bit for bit its float64 result.  A launch of its own because
 * the data-parallel all-reduce of stats_dev comes between fs_adv_stats_dev and this. */
int fs_adv_finish_dev(fs_handle h, const double* stats_dev, double* mean_std_n_dev);
/* One step of torch.optim.Adam (no weight decay, amsgrad or maximize) on packed float32 buffers of num_params elements.
 * state_dev [3] = {t, beta1^t, beta2^t} in double lives on the device, so that a replayed graph advances it; it starts
 * as {0, 1, 1}.  Per call, in double:
 *   t += 1;  p1 *= beta1;  p2 *= beta2;  step = (float)(lr / (1 - p1));  rs = (float)sqrt(1 - p2)
 * per element, in float32, nothing contracted:
 *   m = m + (g - m) * (float)(1 - beta1)
 *   v = v * (float)beta2 + (g * g) * (float)(1 - beta2)
 *   w = w - step * (m / (sqrtf(v) / rs + (float)eps))
 * One workgroup of 1024 lanes: every lane reads the state, a barrier follows, lane 0 alone writes it -- no other
 * workgroup exists that could read the advanced state for the same step.  (num_params is 15 649 at the most for an
 * fs_ppo_model: sixteen elements per lane.) */
int fs_adam_dev(fs_handle h, int64_t num_params, float* weights_dev, const float* grad_dev, float* m_dev, float* v_dev,
                double* state_dev, double lr, double beta1, double beta2, double eps);

/* ---- the reference's PPO loss: KL penalty, clipped value loss, entropy --------
 * The loss RLlib's PPO optimises (the reference's examples/train.py trains with it), per present sample, over the sample
 * count n of the whole update:
 *   -pg + kl_coef KL + vf_coef vfl - entropy_coef H
 *   pg  = as in fs_ppo_grad_dev
 *   KL  = sum_c ls - ls_o + (exp(2 ls_o) + (mu_o - mu)^2) / (2 exp(2 ls)) - 0.5        (old || new, diagonal Gaussians)
 *   H   = sum_c ls + 0.5 log(2 pi e)
 *   vfl = max((v - ret)^2, (v_c - ret)^2),   v_c = v_o + clamp(v - v_o, -vf_clip, +vf_clip)
 * mu, ls: the head's means and the free log std now; mu_o, ls_o, v_o: means, log std and value at the time of the rollout.
 * clip: the surrogate's (>= 0).  vf_clip <= 0 or not finite: no value clipping, vfl = (v - ret)^2.  entropy_coef == 0: no
 * entropy term.  kl_state_dev == NULL: no KL term; otherwise kl_state_dev [2] = {kl_coef, mean KL of the last update} in
 * double ON THE DEVICE -- the kernel reads the coefficient there and fs_kl_adapt_dev advances it, so a replayed graph
 * trains with the adapted value.  A term that is off is selected out, not multiplied by zero, and its inputs are not read.
 * A wrong struct_size, a NaN among the coefficients or clip < 0: FS_ERR_INVALID, with a message that names fs_ppo_loss. */
typedef struct fs_ppo_loss {
  uint32_t struct_size;               /* sizeof(fs_ppo_loss) */
  float clip;                         /* the surrogate's clip range */
  float vf_coef;
  float vf_clip;                      /* <= 0 or not finite: off */
  float entropy_coef;                 /* 0: off */
  const double* kl_state_dev;         /* {kl_coef, mean KL}, device; NULL: off */
} fs_ppo_loss;

/* fs_ppo_eval_dev that also writes the head's means, mean_old_dev [n, A]: the no_grad pass of an update whose loss has the
 * KL term (val_dev then serves as v_o).  act_dev, logp_dev and mean_old_dev must not be NULL.  logp_dev and val_dev hold
 * the bits fs_ppo_eval_dev gives.  fs_last_kernel reports "k_ppo_eval".
 * The head of 2 act_dim outputs (model->log_std_dev == NULL): mean_old_dev is [n, 2A], the A means and then the A log stds
 * of the row -- the whole old distribution; fs_last_kernel reports "k_ppo_eval_ls". */
int fs_ppo_eval_dist_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                         float* logp_dev, float* val_dev, float* mean_old_dev);
/* Floats of work_dev that fs_ppo_grad_loss_dev needs: the workgroups of fs_ppo_workspace times (P + 4) -- four loss sums
 * behind a partial gradient instead of two (0: the model or n is not valid). */
size_t fs_ppo_loss_workspace(const fs_ppo_model* model, int64_t n);
/* fs_ppo_grad_n_dev for the loss above: grad_dev [P] as there, loss_sums_dev [4] = {sum pg, sum vfl, sum KL, sum H} over the
 * present samples (sum KL is 0 without the KL term).  mean_old_dev [n, A], log_std_old_dev [A]: may be NULL only without a KL term; val_old_dev
 * [n]: may be NULL only without value clipping.  Nothing of an absent row (a NaN in its action row) reaches an output, its
 * mean_old and val_old included.  The mapping, the workgroup count and so the order of every sum are fs_ppo_grad_dev's:
 * with every term off, grad_dev and loss_sums_dev[0..1] hold the bits of fs_ppo_grad_n_dev.  fs_last_kernel reports
 * "k_ppo_grad_loss".
 * The head of 2 act_dim outputs (model->log_std_dev == NULL): the old log stds are per sample and travel in mean_old_dev
 * [n, 2A] as fs_ppo_eval_dist_dev writes it; log_std_old_dev must be NULL (anything else: FS_ERR_INVALID, by name).  KL and
 * H are the formulas above with ls and ls_o of the sample.  fs_last_kernel reports "k_ppo_grad_loss_ls".  The same holds
 * for fs_ppo_minibatch_dev ("k_ppo_minibatch_ls"). */
int fs_ppo_grad_loss_dev(fs_handle h, const fs_ppo_model* model, const fs_ppo_loss* loss, int64_t n, const float* obs_dev,
                         const float* act_dev, const float* logp_old_dev, const float* mean_old_dev,
                         const float* log_std_old_dev, const float* val_old_dev, const double* adv_dev, const float* ret_dev,
                         const double* mean_std_n_dev, int accumulate, float* grad_dev, float* loss_sums_dev, float* work_dev,
                         size_t work_floats);
/* RLlib's adaptive KL coefficient, once per update, after the last epoch (and after the data-parallel all-reduce of
 * loss_sums_dev).  One thread, in double, nothing contracted:
 *   mean_kl = (double)loss_sums[2] / mean_std_n[2]
 *   coef *= 1.5 if mean_kl > 2.0 kl_target;   coef *= 0.5 if mean_kl < 0.5 kl_target
 *   kl_state = {coef, mean_kl}
 * kl_target must be positive and finite.  fs_last_kernel reports "k_kl_adapt". */
int fs_kl_adapt_dev(fs_handle h, const float* loss_sums_dev, const double* mean_std_n_dev, double* kl_state_dev,
                    double kl_target);

/* ---- minibatch SGD: an epoch is a shuffled pass of minibatch steps ---------------
 * Epoch e of an update permutes the shard's n rows with perm(seed, e, n); minibatch k of size B is rows
 * perm[k B .. min((k + 1) B, n)), the last one kept when it is short; ceil(n / B) steps per epoch, in ascending k.  One step:
 * the loss above (every term on or off) over the minibatch's present rows, divided by the minibatch's OWN count c of present
 * rows, its gradient, one Adam step; c == 0 makes no step (Adam's t, m, v and the weights untouched).  The advantages stay
 * standardised by mean_std_n_dev (whole batch, once per update; its n is not read here), the old distribution and the KL
 * coefficient stay those of the update's start.
 * perm is computed, never stored: a balanced Feistel network of 4 rounds over the smallest even number of bits that holds
 * n - 1 (at least 2), round function murmur3's fmix32 of (right half + round key), round keys from fmix32 of (seed, epoch,
 * round), cycle-walked (re-applied until the value is < n).  32-bit integer operations only: fs_ppo_perm_host, the kernel
 * and flow_amd.utils.device_ppo.epoch_permutation give the same values.
 * fs_ppo_perm_host needs no handle and no GPU: out [n] = perm(seed, epoch, n). */
int fs_ppo_perm_host(uint64_t seed, uint64_t epoch, int64_t n, int64_t* out);

enum { FS_MB_STEP = 0, FS_MB_PARTIAL = 1 };                          /* fs_ppo_minibatch.mode */
enum { FS_MB_ACCUMULATE = 1, FS_MB_FIRST = 2, FS_MB_LAST = 4 };      /* fs_ppo_minibatch.flags */
typedef struct fs_ppo_minibatch {
  uint32_t struct_size;               /* sizeof(fs_ppo_minibatch) */
  int32_t mode;                       /* FS_MB_STEP: reduce, divide, Adam in the launch; FS_MB_PARTIAL: reduce only */
  int32_t flags;                      /* FS_MB_ACCUMULATE (PARTIAL): a later shard of the step -- sums and count are added
                                       * FS_MB_FIRST: the epoch's first minibatch -- loss_sums_dev is overwritten, not added to
                                       * FS_MB_LAST (STEP): the epoch's last minibatch -- *epoch_dev advances */
  int32_t reserved;
  int64_t batch;                      /* B >= 1 (a per-shard size) */
  int64_t index;                      /* k: 0 .. ceil(n / B) - 1 */
  uint64_t seed;
  uint64_t* epoch_dev;                /* the epoch counter, device: read by the launch, so a replayed graph draws fresh
                                       * permutations */
  double* count_dev;                  /* PARTIAL: [1] the step's count of present rows (double, so that it all-reduces) */
  float* weights_dev;                 /* STEP: the packed buffer [policy][log_std A][value] fs_ppo_model points into
                                       * (the head of 2 act_dim outputs: [policy][value]) */
  float* m_dev;                       /* STEP: Adam's moments [P] and state [3], as in fs_adam_dev */
  float* v_dev;
  double* state_dev;
  double lr, beta1, beta2, eps;       /* STEP */
} fs_ppo_minibatch;

/* 4-byte words of work_dev that fs_ppo_minibatch_dev needs: G (P + 4) partial sums and G integer counts, G = the workgroups
 * of fs_ppo_workspace for a batch of `batch` samples -- a function of (batch, model) alone (0: not valid). */
size_t fs_ppo_minibatch_workspace(const fs_ppo_model* model, int64_t batch);
/* One minibatch step in ONE launch (fs_last_kernel: "k_ppo_minibatch"); the arguments are fs_ppo_grad_loss_dev's, the rows
 * are gathered through perm inside the kernel.  Tile t (64 positions of the minibatch) goes to workgroup t mod G; the lane
 * arithmetic runs with 1 in the place of 1 / n (every term is linear in it); a workgroup writes its partial [P + 4] and its
 * integer count of present rows to work_dev and draws an integer ticket; the workgroup that draws the last one adds the G
 * partials in ascending workgroup order -- no float atomics, no workgroup ever waits for another -- and
 *   FS_MB_STEP     c = the sum of the counts;  g[p] = sum[p] * (float)(1.0 / (double)c);  grad_dev[p] = g[p];  the raw loss
 *                  sums are added to loss_sums_dev (FS_MB_FIRST: overwrite it);  fs_adam_dev's sequence with g on
 *                  weights_dev, m_dev, v_dev, state_dev;  c == 0: grad_dev = the sums (exact zeros), no Adam step
 *   FS_MB_PARTIAL  grad_dev, loss_sums_dev, count_dev[0] receive the raw sums and (double)c (FS_MB_ACCUMULATE: they are
 *                  added); fs_ppo_mb_finish_dev follows once every shard is in and the ranks have all-reduced them.
 * FS_MB_STEP on one shard gives the bits of FS_MB_PARTIAL + fs_ppo_mb_finish_dev.  Nothing of an absent row (a NaN in its
 * action row) reaches an output.  Refused before anything launches, by name: a model outside fs_ppo_model's class, batch < 1,
 * an index beyond the epoch, a NULL epoch_dev, and in FS_MB_STEP a NULL state_dev, m_dev, v_dev or weights_dev.  The first
 * call on a handle allocates the ticket and synchronises the device once: make it before a stream capture begins. */
int fs_ppo_minibatch_dev(fs_handle h, const fs_ppo_model* model, const fs_ppo_loss* loss, const fs_ppo_minibatch* mb, int64_t n,
                         const float* obs_dev, const float* act_dev, const float* logp_old_dev, const float* mean_old_dev,
                         const float* log_std_old_dev, const float* val_old_dev, const double* adv_dev, const float* ret_dev,
                         const double* mean_std_n_dev, float* grad_dev, float* loss_sums_dev, float* work_dev,
                         size_t work_floats);
/* The end of a step made of FS_MB_PARTIAL launches (fs_last_kernel: "k_mb_finish"), one workgroup like fs_adam_dev:
 *   c = count_dev[0];  c == 0: nothing;  otherwise g[p] = grad_dev[p] * (float)(1.0 / c);  grad_dev[p] = g[p];  fs_adam_dev's
 *   sequence with g.  flags: FS_MB_LAST advances *epoch_dev (with or without a step). */
int fs_ppo_mb_finish_dev(fs_handle h, int64_t num_params, float* weights_dev, float* grad_dev, float* m_dev, float* v_dev,
                         double* state_dev, const double* count_dev, uint64_t* epoch_dev, int flags, double lr, double beta1,
                         double beta2, double eps);

/* ---- Snapshots: a handle hands out its state and takes it back -----------------------------------------------------------
 * The blob holds every device array a kernel or an fs_* call writes after fs_create -- vehicle state, the arrays a reset
 * redraws (initial positions, speeds, lanes; pending ring lengths and inflow periods), the open networks' bookkeeping, the
 * noise counters, the policy draw counters and the handle's own observation buffer -- field after field, each [R][row] as
 * the handle holds it, every field at a multiple of 16 bytes.  A replica whose Philox streams are keyed by those counters
 * reproduces its future exactly after a restore.  Constants uploaded once, scratch and staging buffers are not in it.
 *   bytes       the device blob (fs_snapshot_dev / fs_restore_dev)
 *   host_bytes  the host blob (fs_snapshot / fs_restore): a 64-byte header, then the device blob
 *   layout      fingerprint of FS_ABI_VERSION, precision, R, N, network, env head, obs_dim, act_dim and every field's tag
 *               and row bytes: blobs of equal layout have the same fields at the same offsets
 *   nonce       this handle's own number (never 0) */
struct fs_snapshot_info {             /* (a struct tag only: the function below has the name) */
  uint64_t bytes;
  uint64_t host_bytes;
  uint64_t layout;
  uint64_t nonce;
  int32_t num_fields;
  int32_t reserved;
};
int fs_snapshot_info(fs_handle h, struct fs_snapshot_info* out);
/* handle -> dst_dev (fs_snapshot_dev) and src_dev -> handle (fs_restore_dev), all fields in ONE launch (k_snapshot) on the
 * handle's stream, for the replicas where mask_dev [R] (uint8, device) is not zero (NULL: all; the rows of the others are
 * left as they are, in the blob and in the handle).  No host synchronisation, no allocation: legal inside a stream capture.
 * fs_restore_dev takes blobs of THIS handle only, named by `nonce`: the handle keeps host mirrors of device state (the
 * list of ring lengths behind the exact-division proofs of the ring kernels, "a speed below -100 is possible") that must
 * cover whatever a restore brings back; fs_snapshot_dev notes them on the host and fs_restore_dev widens the handle's by
 * the notes, which a blob of another handle does not have.  Refused by name before any HIP call: a NULL buffer, wrong
 * bytes, wrong layout, a foreign nonce. */
int fs_snapshot_dev(fs_handle h, void* dst_dev, size_t bytes, const uint8_t* mask_dev);
int fs_restore_dev(fs_handle h, const void* src_dev, size_t bytes, uint64_t layout, uint64_t nonce, const uint8_t* mask_dev);
/* The synchronous host pair, for persistence: fs_snapshot synchronises the handle's stream and fills host_dst
 * [host_bytes]; fs_restore takes a blob of ANY handle of equal layout and rebuilds the host mirrors from its contents (its
 * ring lengths and pending ring lengths join the list the division proofs walk, its speeds are scanned for values below
 * -100; the header carries the rest).  Equal states give equal blobs byte for byte. */
int fs_snapshot(fs_handle h, void* host_dst, size_t bytes);
int fs_restore(fs_handle h, const void* host_src, size_t bytes, uint64_t layout);

/* Append the CURRENT state of one replica to a CSV file (header `time,id,x,speed,lane_number` when the file is new;
 * one row per vehicle, id = slot index, free slots of open networks skipped): the trajectory ("emission") dump of
 * flow/core/kernel/simulation/traci.py:95-101 (SUMO's --emission-output) for callers without the Python layer;
 * flow_amd.core.util.TrajectoryRecorder writes the reference's full column set (flow/core/util.py:57-99). */
int fs_dump_trajectory(fs_handle h, int replica, const char* csv_path);

#ifdef __cplusplus
}
#endif
#endif /* FLOWSIM_H */
