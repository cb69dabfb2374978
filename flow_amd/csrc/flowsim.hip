// flowsim.hip -- C ABI (include/flowsim.h) over the gfx950 kernels in
// flowsim_kernels.h.  Host code only allocates, uploads tables, picks the
// kernel instantiation and enqueues launches; every number the environment
// returns is computed on the GPU.  There is no CPU fallback: without a HIP
// device fs_create fails with FS_ERR_HIP.
#include "flowsim_sim.h"
#include "flowsim_learn.h"
#include "flowsim_es.h"

#include <cmath>

namespace fsim {

int validate(const fs_config* c) {
  if (!c) return fail(FS_ERR_INVALID, "fs_create: cfg is NULL");
  if (c->struct_size != sizeof(fs_config))
    return fail(FS_ERR_INVALID, "fs_create: struct_size mismatch (header/library out of sync)");
  if (c->abi_version != FS_ABI_VERSION) return fail(FS_ERR_INVALID, "fs_create: abi_version mismatch");
  if (c->precision != FS_F32 && c->precision != FS_F64 && c->precision != FS_MIXED && c->precision != FS_F16S)
    return fail(FS_ERR_INVALID, "fs_create: bad precision");
  if (c->precision == FS_F16S && (c->network != FS_NET_MERGE || c->num_vehicles > 64))
    return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_F16S (half state, float32 integrator) is built for FS_NET_MERGE "
                                    "(k_steps_open, <= 64 vehicle slots)");
  if (c->precision == FS_MIXED && (c->network == FS_NET_MERGE || c->network == FS_NET_BOTTLENECK)) {
    // open networks: the float64 kernels with float32 car-following models (k_steps_open<double, ., ., 2>); whatever FS_F64
    // accepts (the lane-drop network beyond 64 slots, k_steps_wide, steps in plain float64)
  } else if (c->precision == FS_MIXED) {
    // float64 state, float32 controllers: k_rollout_pair (all-IDM AccelEnv rollout) and k_ring_pair (IDM + RL vehicles,
    // AccelEnv / WaveAttenuationPOEnv, warm-up steps and masked resets included).  Name the field that does not fit.
    // The figure eight (k_rollout_loop's float64-state instantiation, flowsim_fig8.h): rollouts step there, everything else
    // (resets, masks, single steps of more than 16 vehicles) on the generic float64 kernel -- the reference's arithmetic.
    const bool fig8 = c->network == FS_NET_FIGURE_EIGHT;
    const char* why = nullptr;
    if ((c->network != FS_NET_RING && !fig8) || c->num_lanes > 1) why = "network (single-lane ring or figure eight)";
    else if (c->env == FS_ENV_MULTI_WAVE_ATTENUATION_PO)
      why = "env (FS_ENV_MULTI_WAVE_ATTENUATION_PO is built for FS_F32, and for FS_F64 on the generic kernel)";
    else if (c->env != FS_ENV_ACCEL && c->env != FS_ENV_WAVE_ATTENUATION_PO) why = "env (AccelEnv or WaveAttenuationPOEnv)";
    else if (c->evaluate) why = "evaluate";
    else if (c->sims_per_step != 1) why = "sims_per_step (1)";
    else if (c->integrator != FS_EULER) why = "integrator (Euler)";
    else if (c->junction_mode && !fig8) why = "junction_mode";
    else if (c->track_aux && !fig8) why = "track_aux (the scalar Env's previous-speed / acceleration fields: VecFlowEnv(track_aux=False))";
    else if (c->sort_vehicles || c->obs_perm) why = "sort_vehicles / shuffled ids";
    else if (!fig8 && (c->num_vehicles < 2 || c->num_vehicles > 64 || (c->num_vehicles % 2) != 0)) why = "num_vehicles (even, 2..64)";
    else if (!c->vehicles) why = "vehicles (NULL)";
    for (int i = 0; !why && i < c->num_vehicles; ++i) {
      const fs_vehicle_spec& v = c->vehicles[i];
      if (v.controller != FS_CTRL_IDM && v.controller != FS_CTRL_RL && !(fig8 && v.controller == FS_CTRL_SIM))
        why = "vehicles[].controller (IDMController / RLController)";
      else if (v.fail_safe != FS_FAILSAFE_NONE) why = "vehicles[].fail_safe";
    }
    if (why)
      return fail(FS_ERR_UNSUPPORTED, std::string("fs_create: FS_MIXED does not support this configuration: ") + why);
  }
  if (c->network < FS_NET_RING || c->network > FS_NET_BOTTLENECK)
    return fail(FS_ERR_UNSUPPORTED, "fs_create: network not built");
  const bool open_net = c->network == FS_NET_MERGE || c->network == FS_NET_BOTTLENECK;
  const bool merge_env = c->env == FS_ENV_MERGE_PO || c->env == FS_ENV_MERGE_MA;
  const bool bn_env = c->env == FS_ENV_BOTTLENECK_DV || c->env == FS_ENV_BOTTLENECK;
  if ((c->network == FS_NET_MERGE) != merge_env)
    return fail(FS_ERR_INVALID, "fs_create: the merge envs and FS_NET_MERGE go together");
  if (c->network == FS_NET_MERGE && !c->track_followers)
    return fail(FS_ERR_INVALID, "fs_create: the merge observations need track_followers = 1");
  if ((c->network == FS_NET_BOTTLENECK) != bn_env)
    return fail(FS_ERR_INVALID, "fs_create: the bottleneck envs and FS_NET_BOTTLENECK go together");
  if (c->network == FS_NET_BOTTLENECK) {
    if (c->num_vehicles <= 32)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: the bottleneck heads need more than 32 vehicle slots per replica");
    if (!(c->merge1_x <= c->merge2_x) || !(c->merge2_x < c->end_x) || !(c->zipper_distance >= 0))
      return fail(FS_ERR_INVALID, "fs_create: need merge1_x <= merge2_x < end_x and zipper_distance >= 0");
    if (c->junction.enabled) return fail(FS_ERR_INVALID, "fs_create: the priority-junction model is for FS_NET_MERGE");
    if (c->obs_outflow_window < 1 || c->obs_outflow_window > 20 || c->reward_outflow_window < 1 ||
        c->reward_outflow_window > 20)
      return fail(FS_ERR_INVALID, "fs_create: outflow windows must be 1..20 sub-steps");
    if (c->evaluate) return fail(FS_ERR_UNSUPPORTED, "fs_create: evaluate mode of the bottleneck envs is not built");
    if (c->num_paths != 0 && c->num_paths != 4 && c->num_paths != 8)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: num_paths (4 * scaling) must be 4 or 8");
    if (c->num_paths == 8 && c->num_vehicles <= 64)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: num_paths = 8 (scaling 2) is built in the workgroup-per-replica kernel: "
                                      "more than 64 vehicle slots per replica");
    if (c->env == FS_ENV_BOTTLENECK_DV) {
      const int max_cells = c->num_vehicles > 64 ? 128 : 64;
      if (c->num_obs_cells < 1 || c->num_obs_cells > max_cells || !c->obs_cells)
        return fail(FS_ERR_INVALID, "fs_create: 1..64 observation cells (1..128 with more than 64 vehicle slots)");
      for (int k = 0; k < c->num_obs_cells; ++k)
        if (c->obs_cells[k].lane < 0 || c->obs_cells[k].lane > 63) return fail(FS_ERR_INVALID, "fs_create: cell lane");
      for (int k = 0; k < c->num_rl; ++k)
        if (c->act_cells && (c->act_cells[k].lane < 0 || c->act_cells[k].lane > 63))
          return fail(FS_ERR_INVALID, "fs_create: cell lane");
      if (c->num_rl < 0 || c->num_rl > 64 || (c->num_rl > 0 && !c->act_cells))
        return fail(FS_ERR_INVALID, "fs_create: 0..64 action cells");
    }
  }
  if (open_net) {
    if (c->num_lanes > 1) return fail(FS_ERR_UNSUPPORTED, "fs_create: multi-lane merge is not built");
    if (c->num_segments < 2 || c->num_segments > 2 * FS_MAX_SEGMENTS || !c->segments)
      return fail(FS_ERR_INVALID, "fs_create: FS_NET_MERGE needs the segment tables of both routes");
    int per_route[2] = {0, 0};
    for (int k = 0; k < c->num_segments; ++k) {
      const fs_segment& sg = c->segments[k];
      if (sg.route < 0 || sg.route > (c->network == FS_NET_MERGE ? 1 : 0))
        return fail(FS_ERR_INVALID, "fs_create: segment route out of range");
      if (k > 0 && sg.route < c->segments[k - 1].route)
        return fail(FS_ERR_INVALID, "fs_create: segment rows must be grouped by route");
      if (k > 0 && sg.route == c->segments[k - 1].route && !(sg.start > c->segments[k - 1].start))
        return fail(FS_ERR_INVALID, "fs_create: segment starts must increase");
      if (++per_route[sg.route] > FS_MAX_SEGMENTS) return fail(FS_ERR_INVALID, "fs_create: too many segments");
    }
    if (!per_route[0] || (c->network == FS_NET_MERGE && !per_route[1]))
      return fail(FS_ERR_INVALID, "fs_create: a route has no segment");
    if (c->num_inflows < 0 || c->num_inflows > FS_MAX_INFLOWS || (c->num_inflows > 0 && !c->inflows))
      return fail(FS_ERR_INVALID, "fs_create: bad inflow table");
    for (int f = 0; f < c->num_inflows; ++f) {
      const fs_inflow& fl = c->inflows[f];
      if (c->network == FS_NET_MERGE ? (fl.route < 0 || fl.route > 1)
                                     : (fl.route < -1 || fl.route > (c->num_paths == 8 ? 7 : 3)))
        return fail(FS_ERR_INVALID, "fs_create: inflow route out of range");
      if (fl.probability > 1.0) return fail(FS_ERR_INVALID, "fs_create: inflow probability > 1");
      if (!(fl.probability >= 0.0) && !(fl.period > 0)) return fail(FS_ERR_INVALID, "fs_create: inflow period <= 0");
      if (!(fl.depart_speed >= 0) || !(fl.depart_pos >= 0)) return fail(FS_ERR_INVALID, "fs_create: bad inflow departure");
      bool type_ok = false;
      for (int i = 0; i < c->num_vehicles; ++i) type_ok = type_ok || c->vehicles[i].type == fl.type;
      if (!type_ok) return fail(FS_ERR_INVALID, "fs_create: inflow of a vehicle type that has no slot");
    }
    if (!c->init_alive || !c->init_lane) return fail(FS_ERR_INVALID, "fs_create: FS_NET_MERGE needs init_alive and init_lane (routes)");
    if (!(c->box_in < c->merge_x) || !(c->merge_x < c->end_x) || !(c->net_length > 0))
      return fail(FS_ERR_INVALID, "fs_create: need box_in < merge_x < end_x and net_length > 0");
  }
  if (c->network == FS_NET_RING && (c->num_segments != 0 || c->junction.enabled))
    return fail(FS_ERR_INVALID, "fs_create: a ring takes no segment table / junction");
  if (c->network == FS_NET_FIGURE_EIGHT) {
    if (c->num_segments < 1 || c->num_segments > FS_MAX_SEGMENTS || !c->segments)
      return fail(FS_ERR_INVALID, "fs_create: figure eight needs 1..FS_MAX_SEGMENTS segments");
    if (c->num_lanes > 1) return fail(FS_ERR_UNSUPPORTED, "fs_create: multi-lane figure eight is not built");
    if (c->segments[0].start != 0.0) return fail(FS_ERR_INVALID, "fs_create: segment 0 must start at 0");
    for (int k = 1; k < c->num_segments; ++k)
      if (!(c->segments[k].start > c->segments[k - 1].start))
        return fail(FS_ERR_INVALID, "fs_create: segment starts must increase");
  }
  if (c->env < FS_ENV_ACCEL || c->env > FS_ENV_USER) return fail(FS_ERR_INVALID, "fs_create: bad env");
  if (c->env == FS_ENV_USER) {          // a user head (flow_amd.envs.CompiledEnv): k_steps of a library that holds it
    if (!fs::kHasUserEnv)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_USER: this library was built without a user environment head "
                                      "(flow_amd.build.build_user / flow_amd.envs.CompiledEnv)");
    if (open_net) return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_USER on an open network is not built");
    if (c->num_lanes > 1) return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_USER on a multi-lane ring is not built");
    if (c->precision != FS_F32 && c->precision != FS_F64)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_USER is built for FS_F32 and FS_F64");
    if (c->sort_vehicles) return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_USER with sort_vehicles is not built");
    if (c->num_vehicles > 64) return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_USER with more than 64 vehicles is not built");
  }
  const bool lc_env = c->env == FS_ENV_LANE_CHANGE_ACCEL || c->env == FS_ENV_LANE_CHANGE_ACCEL_PO;
  if (lc_env && c->network != FS_NET_RING)
    return fail(FS_ERR_UNSUPPORTED, "fs_create: the lane-change envs are built for rings (k_steps_ml)");
  if (c->env == FS_ENV_LANE_CHANGE_ACCEL_PO && (c->num_rl < 1 || c->obs_perm))
    return fail(FS_ERR_INVALID, "fs_create: LaneChangeAccelPOEnv needs an RL vehicle and takes no observation permutation");
  if (c->env == FS_ENV_WAVE_ATTENUATION_PO_MA || c->env == FS_ENV_ACCEL_PO_MA) {
    if (open_net || c->num_lanes > 1)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: the multi-agent ring heads are built for single-lane closed loops");
    if (c->num_rl < 1) return fail(FS_ERR_INVALID, "fs_create: a multi-agent ring env needs an RL vehicle");
    if (c->sort_vehicles || c->obs_perm) return fail(FS_ERR_INVALID, "fs_create: sort_vehicles / shuffled ids belong to AccelEnv");
  }
  if (c->env == FS_ENV_MULTI_WAVE_ATTENUATION_PO) {      // one ring of MultiRingNetwork per replica row, one agent per ring
    if (c->network != FS_NET_RING)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_MULTI_WAVE_ATTENUATION_PO on a segment-table loop or an open network "
                                      "is not built (MultiRingNetwork's rings are plain rings)");
    if (c->num_lanes > 1)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_MULTI_WAVE_ATTENUATION_PO on a multi-lane ring is not built");
    if (c->num_rl != 1)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: FS_ENV_MULTI_WAVE_ATTENUATION_PO needs num_rl = 1 (one RL vehicle per ring: "
                                      "the reference's environment works with nothing else)");
    if (c->sort_vehicles || c->obs_perm) return fail(FS_ERR_INVALID, "fs_create: sort_vehicles / shuffled ids belong to AccelEnv");
  }
  if (c->num_lanes > 1 && c->env == FS_ENV_WAVE_ATTENUATION_PO)
    return fail(FS_ERR_UNSUPPORTED, "fs_create: WaveAttenuationPOEnv on a multi-lane ring is not built");
  if (c->num_lanes > 64) return fail(FS_ERR_INVALID, "fs_create: num_lanes > 64");
  if (c->init_lane && !open_net)
    for (size_t e = 0; e < size_t(c->num_replicas > 0 ? c->num_replicas : 0) * (c->num_vehicles > 0 ? c->num_vehicles : 0); ++e)
      if (c->init_lane[e] < 0 || c->init_lane[e] >= (c->num_lanes < 1 ? 1 : c->num_lanes))
        return fail(FS_ERR_INVALID, "fs_create: init_lane out of range");
  if (c->num_replicas < 1) return fail(FS_ERR_INVALID, "fs_create: num_replicas < 1");
  if (c->replica_offset < 0) return fail(FS_ERR_INVALID, "fs_create: replica_offset < 0");
  if (c->sort_vehicles || c->obs_perm) {
    if (c->env != FS_ENV_ACCEL && !lc_env && c->sort_vehicles)
      return fail(FS_ERR_INVALID, "fs_create: sort_vehicles belongs to AccelEnv / LaneChangeAccelEnv");
    if (c->network == FS_NET_MERGE || c->network == FS_NET_BOTTLENECK ||
        (c->num_lanes > 1 && c->sort_vehicles && !lc_env))
      return fail(FS_ERR_UNSUPPORTED, "fs_create: sort_vehicles / shuffled ids are built for closed loops "
                                      "(sort_vehicles on multi-lane rings: LaneChangeAccelEnv)");
    if (c->obs_perm) {
      unsigned long long seen = 0ull;
      for (int i = 0; i < c->num_vehicles && i < 64; ++i) {
        const int q = c->obs_perm[i];
        if (q < 0 || q >= c->num_vehicles || (seen >> q) & 1ull)
          return fail(FS_ERR_INVALID, "fs_create: obs_perm is not a permutation");
        seen |= 1ull << q;
      }
    }
  }
  if (c->num_vehicles < 1) return fail(FS_ERR_INVALID, "fs_create: num_vehicles < 1");
  if (c->num_vehicles > 64 && c->network != FS_NET_BOTTLENECK)
    return fail(FS_ERR_UNSUPPORTED, "fs_create: more than 64 vehicles per replica is built for FS_NET_BOTTLENECK only");
  if (c->num_vehicles > FS_MAX_SLOTS_WIDE)
    return fail(FS_ERR_UNSUPPORTED, "fs_create: more than 256 vehicle slots per replica is not built");
  if (c->num_rl < 0 || (c->num_rl > c->num_vehicles && c->env != FS_ENV_BOTTLENECK_DV))
    return fail(FS_ERR_INVALID, "fs_create: bad num_rl");
  if (c->sims_per_step < 1) return fail(FS_ERR_INVALID, "fs_create: sims_per_step < 1");
  if (c->warmup_steps < 0) return fail(FS_ERR_INVALID, "fs_create: warmup_steps < 0");
  if (!(c->sim_step > 0)) return fail(FS_ERR_INVALID, "fs_create: sim_step <= 0");
  if (!(c->slowdown_ramp > 0) || c->slowdown_ramp > 1) return fail(FS_ERR_INVALID, "fs_create: slowdown_ramp not in (0,1]");
  if (c->junction_length < 0) return fail(FS_ERR_INVALID, "fs_create: junction_length < 0");
  if (!c->vehicles || (!c->ring_length && !open_net) || !c->init_pos)
    return fail(FS_ERR_INVALID, "fs_create: NULL table pointer");
  int seen_rl = 0;
  unsigned long long rl_mask = 0ull;       // num_vehicles <= 64
  for (int i = 0; i < c->num_vehicles; ++i) {
    const fs_vehicle_spec& v = c->vehicles[i];
    if (v.controller < FS_CTRL_SIM || v.controller > FS_CTRL_USER)
      return fail(FS_ERR_INVALID, "fs_create: unknown controller id");
    if (v.fail_safe < FS_FAILSAFE_NONE || v.fail_safe > FS_FAILSAFE_SAFE_VELOCITY)
      return fail(FS_ERR_INVALID, "fs_create: unknown fail_safe id");
    if (open_net && v.controller == FS_CTRL_PISATURATION)
      return fail(FS_ERR_UNSUPPORTED, "fs_create: PISaturation on an open network is not built");
    if (v.controller == FS_CTRL_RL && (c->env == FS_ENV_MERGE_PO || bn_env)) {
      ++seen_rl;                        // the action column is the place in rl_veh, not rl_index
    } else if (v.controller == FS_CTRL_RL) {
      if (v.rl_index < 0 || v.rl_index >= c->num_rl) return fail(FS_ERR_INVALID, "fs_create: rl_index out of range");
      if (rl_mask & (1ull << v.rl_index)) return fail(FS_ERR_INVALID, "fs_create: rl_index used twice");
      rl_mask |= 1ull << v.rl_index;
      ++seen_rl;
    }
    if (!(v.length > 0)) return fail(FS_ERR_INVALID, "fs_create: vehicle length <= 0");
  }
  if (c->env == FS_ENV_MERGE_PO && c->num_rl > 32)      // the removal pass of rl_veh keeps the list places in one 32-bit mask
    return fail(FS_ERR_UNSUPPORTED, "fs_create: MergePOEnv with more than 32 controlled places (num_rl) is not built");
  if (seen_rl != c->num_rl && c->env != FS_ENV_MERGE_PO && !bn_env)
    return fail(FS_ERR_INVALID, "fs_create: num_rl does not match the RL slots");
  if (open_net) {
    // placement sanity of the initial vehicles: inside their route, alive flags consistent
    for (size_t e = 0; e < size_t(c->num_replicas) * c->num_vehicles; ++e) {
      if (!c->init_alive[e]) continue;
      const int rt = c->init_lane[e];
      if (rt < 0 || rt > (c->network == FS_NET_MERGE ? 1 : (c->num_paths == 8 ? 7 : 3)))
        return fail(FS_ERR_INVALID, "fs_create: initial route out of range");
      const double x = c->init_pos[e];
      if (!(x >= c->route_start[c->network == FS_NET_MERGE ? rt : 0]) || !(x < c->end_x))
        return fail(FS_ERR_INVALID, "fs_create: init_pos outside the route");
    }
    return FS_OK;
  }
  if (c->env == FS_ENV_WAVE_ATTENUATION_PO && c->num_rl < 1)
    return fail(FS_ERR_INVALID, "fs_create: WaveAttenuationPOEnv needs an RL vehicle");
  // placement sanity: every replica's vehicles must fit on its loop (network/base.py:603-605)
  for (int r = 0; r < c->num_replicas; ++r) {
    double need = 0;
    for (int i = 0; i < c->num_vehicles; ++i) need += c->vehicles[i].length;
    const double L = c->ring_length[r] + 4 * c->junction_length;
    if (!(c->ring_length[r] > 0) || need > L * (c->num_lanes < 1 ? 1 : c->num_lanes))
      return fail(FS_ERR_NOSPACE, "fs_create: vehicles do not fit on the ring");
    for (int i = 0; i < c->num_vehicles; ++i) {
      const double x = c->init_pos[size_t(r) * c->num_vehicles + i];
      if (!(x >= 0) || !(x < L)) return fail(FS_ERR_INVALID, "fs_create: init_pos outside [0, length)");
    }
  }
  return FS_OK;
}

template <typename T>
int create_typed(const fs_config* cfg, fs_handle* out) {
  Sim<T>* s = new (std::nothrow) Sim<T>();
  if (!s) return fail(FS_ERR_HIP, "fs_create: out of host memory");
  s->cfg = *cfg;
  s->mixed = cfg->precision == FS_MIXED;
  s->f16s = cfg->precision == FS_F16S;
  s->veh.assign(cfg->vehicles, cfg->vehicles + cfg->num_vehicles);
  if (cfg->num_segments > 0) s->segs.assign(cfg->segments, cfg->segments + cfg->num_segments);
  if (cfg->obs_perm) s->obs_perm.assign(cfg->obs_perm, cfg->obs_perm + cfg->num_vehicles);
  if (cfg->network == FS_NET_MERGE || cfg->network == FS_NET_BOTTLENECK) {
    if (cfg->num_inflows > 0) s->inflows.assign(cfg->inflows, cfg->inflows + cfg->num_inflows);
    s->init_alive.assign(cfg->init_alive, cfg->init_alive + size_t(cfg->num_replicas) * cfg->num_vehicles);
    if (cfg->env == FS_ENV_BOTTLENECK_DV) {
      s->obs_cells.assign(cfg->obs_cells, cfg->obs_cells + cfg->num_obs_cells);
      if (cfg->num_rl > 0) s->act_cells.assign(cfg->act_cells, cfg->act_cells + cfg->num_rl);
    }
  }
  s->obs_dim = (cfg->env == FS_ENV_WAVE_ATTENUATION_PO) ? 3
               : (cfg->env == FS_ENV_USER)                  // (the shapes of the head this library was compiled with)
                     ? fs::kUserObsPerVehicle * (fs::kUserObsRlOnly ? cfg->num_rl : cfg->num_vehicles)
               : (cfg->env == FS_ENV_WAVE_ATTENUATION_PO_MA) ? 3 * cfg->num_rl
               : (cfg->env == FS_ENV_MULTI_WAVE_ATTENUATION_PO) ? 3
               : (cfg->env == FS_ENV_ACCEL_PO_MA) ? 6 * cfg->num_rl
               : (cfg->env == FS_ENV_BOTTLENECK_DV) ? 4 * cfg->num_obs_cells + 1
               : (cfg->env == FS_ENV_BOTTLENECK) ? 1
               : (cfg->env == FS_ENV_MERGE_PO || cfg->env == FS_ENV_MERGE_MA)
                     ? 5 * cfg->num_rl
                     : (cfg->env == FS_ENV_LANE_CHANGE_ACCEL_PO)
                           ? (4 * (cfg->num_lanes < 1 ? 1 : cfg->num_lanes) + 1) * cfg->num_rl
                           : (cfg->env == FS_ENV_LANE_CHANGE_ACCEL ? 3 : 2) * cfg->num_vehicles;
  if (s->obs_dim < 1) s->obs_dim = 1;      // an env without RL places still gets a (dummy) buffer
  s->act_dim = cfg->num_rl * ((cfg->env == FS_ENV_LANE_CHANGE_ACCEL || cfg->env == FS_ENV_LANE_CHANGE_ACCEL_PO) ? 2 : 1);
  int seg = 8;
  while (seg < cfg->num_vehicles) seg <<= 1;       // 128 / 256: one workgroup of 2 / 4 waves per replica (k_steps_wide)
  s->seg = seg;
  hipError_t e = hipSetDevice(cfg->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete s;
    return fail(FS_ERR_HIP, std::string("fs_create: no usable HIP device: ") + hipGetErrorString(e));
  }
  s->stream = s->own_stream;
  {   // development switches (tests): FLOWSIM_<NAME>=1 keeps a specialised kernel out of the choice
    const std::pair<const char*, bool SimBase::*> switches[] = {
        {"FLOWSIM_FORCE_GENERIC", &SimBase::force_generic}, {"FLOWSIM_NO_FASTDIV", &SimBase::no_fastdiv},
        {"FLOWSIM_NO_LOOP_KERNEL", &SimBase::no_loop_kernel}, {"FLOWSIM_NO_LOOP_FULL", &SimBase::no_loop_full},
        {"FLOWSIM_NO_RING_RL", &SimBase::no_ring_rl}, {"FLOWSIM_NO_QUEUE", &SimBase::no_queue},
        {"FLOWSIM_NO_PAIR", &SimBase::no_pair}, {"FLOWSIM_PAIR_GENERIC_N", &SimBase::pair_generic_n},
        {"FLOWSIM_KERNEL_DETAIL", &SimBase::kernel_detail}, {"FLOWSIM_PAIR_N_ALWAYS", &SimBase::pair_n_always},
        {"FLOWSIM_NO_MASK_SKIP", &SimBase::no_mask_skip},
        {"FLOWSIM_SNAPSHOT_COPIES", &SimBase::snap_copies}};
    for (const auto& sw : switches) {
      const char* v = std::getenv(sw.first);
      s->*sw.second = v && v[0] == '1';
    }
  }
  int rc = s->init();
  if (rc == FS_OK) {
    hipError_t e2 = hipStreamSynchronize(s->stream);
    if (e2 != hipSuccess) rc = fail(FS_ERR_HIP, std::string("fs_create: ") + hipGetErrorString(e2));
  }
  if (rc != FS_OK) {
    for (void* p : s->allocs) (void)hipFree(p);
    (void)hipStreamDestroy(s->own_stream);
    delete s;
    return rc;
  }
  // the config's table pointers belong to the caller: do not keep them
  s->cfg.vehicles = nullptr;
  s->cfg.ring_length = nullptr;
  s->cfg.init_pos = nullptr;
  s->cfg.init_vel = nullptr;
  s->cfg.init_lane = nullptr;
  s->cfg.segments = nullptr;
  s->cfg.inflows = nullptr;
  s->cfg.init_alive = nullptr;
  s->cfg.obs_cells = nullptr;
  s->cfg.obs_perm = nullptr;
  s->cfg.act_cells = nullptr;
  *out = reinterpret_cast<fs_handle>(static_cast<SimBase*>(s));
  return FS_OK;
}

inline SimBase* S(fs_handle h) { return reinterpret_cast<SimBase*>(h); }

// Every entry point runs on the handle's device whatever the caller's current device is, and leaves the caller's
// current device as it found it (two handles on two GPUs in one process; torch's current device).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int want) {
    if (hipGetDevice(&prev) == hipSuccess && prev != want) switched = hipSetDevice(want) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

}  // namespace fsim

using namespace fsim;

extern "C" {

int fs_abi_version(void) { return FS_ABI_VERSION; }

const char* fs_last_error(void) { return g_err.c_str(); }

int fs_create(const fs_config* cfg, fs_handle* out) {
  if (!out) return fail(FS_ERR_INVALID, "fs_create: out is NULL");
  *out = nullptr;
  int rc = validate(cfg);
  if (rc) return rc;
  int prev = -1;
  const bool have_prev = hipGetDevice(&prev) == hipSuccess;
  rc = (cfg->precision == FS_F32 || cfg->precision == FS_F16S) ? create_typed<float>(cfg, out)
                                                                 : create_typed<double>(cfg, out);
  if (have_prev && prev != cfg->device) (void)hipSetDevice(prev);      // the caller's current device is not ours to change
  return rc;
}

void fs_destroy(fs_handle h) {
  if (!h) return;
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  (void)hipStreamSynchronize(s->stream);
  for (void* p : s->allocs) (void)hipFree(p);
  (void)hipStreamDestroy(s->own_stream);
  delete s;
}

int fs_obs_dim(fs_handle h) { return h ? S(h)->obs_dim : fail(FS_ERR_INVALID, "fs_obs_dim: NULL handle"); }

int fs_action_dim(fs_handle h) { return h ? S(h)->act_dim : fail(FS_ERR_INVALID, "fs_action_dim: NULL handle"); }

int fs_set_stream(fs_handle h, void* hip_stream) {
  if (!h) return fail(FS_ERR_INVALID, "fs_set_stream: NULL handle");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->stream = static_cast<hipStream_t>(hip_stream);
  return FS_OK;
}

int fs_use_own_stream(fs_handle h) {
  if (!h) return fail(FS_ERR_INVALID, "fs_use_own_stream: NULL handle");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->stream = s->own_stream;
  return FS_OK;
}

int fs_sync(fs_handle h) {
  if (!h) return fail(FS_ERR_INVALID, "fs_sync: NULL handle");
  DeviceGuard guard(S(h)->cfg.device);
  HIP_TRY(hipStreamSynchronize(S(h)->stream));
  return S(h)->check_qflag();
}

int fs_reset_dev(fs_handle h, const uint8_t* mask_dev, float* obs_dev) {
  if (!h) return fail(FS_ERR_INVALID, "fs_reset_dev: NULL handle");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  int rc = s->launch_reset(mask_dev);
  if (rc) return rc;
  float* obs = obs_dev ? obs_dev : s->d_obs;
  if (s->cfg.network == FS_NET_MERGE || s->cfg.network == FS_NET_BOTTLENECK) {   // update(reset=True) first
    s->after_reset = 1;
    rc = s->launch_steps(0, mask_dev, nullptr, 0, obs, s->d_rew, s->d_done, 0);
    s->after_reset = 0;
    if (rc) return rc;
    if (s->cfg.warmup_steps > 0)
      return s->launch_steps(s->cfg.warmup_steps, mask_dev, nullptr, 0, obs, s->d_rew, s->d_done, 0);
    return FS_OK;
  }
  if (s->cfg.warmup_steps > 0)   // envs/base.py:554-555: warm-up steps with rl_actions=None
    return s->launch_steps(s->cfg.warmup_steps, mask_dev, nullptr, 0, obs, s->d_rew, s->d_done, 0);
  return s->launch_steps(0, mask_dev, nullptr, 0, obs, s->d_rew, s->d_done, 0);
}

int fs_reset(fs_handle h, const uint8_t* mask, float* obs_out) {
  if (!h) return fail(FS_ERR_INVALID, "fs_reset: NULL handle");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  const size_t R = size_t(s->cfg.num_replicas);
  const uint8_t* dmask = nullptr;
  if (mask) {
    HIP_TRY(hipMemcpyAsync(s->d_mask, mask, R, hipMemcpyHostToDevice, s->stream));
    dmask = s->d_mask;
  }
  int rc = fs_reset_dev(h, dmask, s->d_obs);
  if (rc) return rc;
  if (obs_out)
    HIP_TRY(hipMemcpyAsync(obs_out, s->d_obs, R * s->obs_dim * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return FS_OK;
}

int fs_step_dev(fs_handle h, const float* actions_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev) {
  if (!h) return fail(FS_ERR_INVALID, "fs_step_dev: NULL handle");
  if (!obs_dev || !rew_dev || !done_dev) return fail(FS_ERR_INVALID, "fs_step_dev: NULL output pointer");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_steps(1, nullptr, actions_dev, 0, obs_dev, rew_dev, done_dev, 0);
}

int fs_step(fs_handle h, const float* actions, float* obs, float* rew, uint8_t* done) {
  if (!h) return fail(FS_ERR_INVALID, "fs_step: NULL handle");
  if (!obs || !rew || !done) return fail(FS_ERR_INVALID, "fs_step: NULL output pointer");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  const size_t R = size_t(s->cfg.num_replicas);
  const float* dact = nullptr;
  if (actions && s->act_dim > 0) {
    HIP_TRY(hipMemcpyAsync(s->d_actions, actions, R * s->act_dim * sizeof(float), hipMemcpyHostToDevice, s->stream));
    dact = s->d_actions;
  }
  int rc = s->launch_steps(1, nullptr, dact, 0, s->d_obs, s->d_rew, s->d_done, 0);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(obs, s->d_obs, R * s->obs_dim * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(rew, s->d_rew, R * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(done, s->d_done, R, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return s->check_qflag();        // (a queue-order launch that overflowed a path: the rows just copied are not results)
}

int fs_rollout_dev(fs_handle h, int num_steps, const float* actions_dev, size_t action_stride_steps,
                   float* obs_dev, float* rew_dev, uint8_t* done_dev, int obs_every_step) {
  if (!h) return fail(FS_ERR_INVALID, "fs_rollout_dev: NULL handle");
  if (num_steps < 1) return fail(FS_ERR_INVALID, "fs_rollout_dev: num_steps < 1");
  if (!obs_dev || !rew_dev || !done_dev) return fail(FS_ERR_INVALID, "fs_rollout_dev: NULL output pointer");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_steps(num_steps, nullptr, actions_dev, action_stride_steps, obs_dev, rew_dev, done_dev,
                            obs_every_step ? 1 : 0);
}

int fs_get_state(fs_handle h, int field, void* dst, size_t bytes) {
  if (!h || !dst) return fail(FS_ERR_INVALID, "fs_get_state: NULL argument");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->get_state(field, dst, bytes);
}

int fs_set_state(fs_handle h, int field, const void* src, size_t bytes) {
  if (!h || !src) return fail(FS_ERR_INVALID, "fs_set_state: NULL argument");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->set_state(field, src, bytes);
}

int fs_add_vehicle(fs_handle h, int replica, int slot, int route, double x, double speed) {
  if (!h) return fail(FS_ERR_INVALID, "fs_add_vehicle: NULL handle");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->add_vehicle(replica, slot, route, x, speed);
}

int fs_policy_act_dev(fs_handle h, const fs_policy* pol, const float* obs_dev, float* act_dev, float* logp_dev) {
  if (!h || !pol || !obs_dev || !act_dev || !logp_dev) return fail(FS_ERR_INVALID, "fs_policy_act_dev: NULL argument");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_policy(pol, 0, 0, obs_dev, nullptr, act_dev, logp_dev, nullptr, nullptr);
}

int fs_policy_rollout_dev(fs_handle h, const fs_policy* pol, int num_steps, int reset_done, float* obs_dev,
                          float* act_dev, float* logp_dev, float* rew_dev, uint8_t* done_dev) {
  if (!h || !pol || !obs_dev || !act_dev || !logp_dev || !rew_dev || !done_dev)
    return fail(FS_ERR_INVALID, "fs_policy_rollout_dev: NULL argument");
  if (num_steps < 1) return fail(FS_ERR_INVALID, "fs_policy_rollout_dev: num_steps < 1");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_policy(pol, num_steps, reset_done ? 1 : 0, nullptr, obs_dev, act_dev, logp_dev, rew_dev, done_dev);
}

int fs_policy_pair_act_dev(fs_handle h, const fs_policy* av, const fs_policy* adversary, float perturb_weight,
                           const float* obs_dev, float* act_dev, float* logp_dev, float* cmd_dev) {
  if (!h || !av || !adversary || !obs_dev || !act_dev || !logp_dev || !cmd_dev)
    return fail(FS_ERR_INVALID, "fs_policy_pair_act_dev: NULL argument");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_policy_pair(av, adversary, perturb_weight, 0, 0, obs_dev, nullptr, act_dev, logp_dev, cmd_dev, nullptr,
                                  nullptr);
}

int fs_policy_pair_rollout_dev(fs_handle h, const fs_policy* av, const fs_policy* adversary, float perturb_weight,
                               int num_steps, int reset_done, float* obs_dev, float* act_dev, float* logp_dev,
                               float* rew_dev, uint8_t* done_dev) {
  if (!h || !av || !adversary || !obs_dev || !act_dev || !logp_dev || !rew_dev || !done_dev)
    return fail(FS_ERR_INVALID, "fs_policy_pair_rollout_dev: NULL argument");
  if (num_steps < 1) return fail(FS_ERR_INVALID, "fs_policy_pair_rollout_dev: num_steps < 1");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_policy_pair(av, adversary, perturb_weight, num_steps, reset_done ? 1 : 0, nullptr, obs_dev, act_dev,
                                  logp_dev, nullptr, rew_dev, done_dev);
}

// ---- policy populations (fs_population; Sim::launch_population)
int fs_population_granule(fs_handle h, const fs_policy* pol) {
  if (!h || !pol) {
    fail(FS_ERR_INVALID, "fs_population_granule: NULL argument");
    return -1;
  }
  DeviceGuard guard(S(h)->cfg.device);
  if (S(h)->launch_population(pol, nullptr, 1, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return -1;
  return 16;
}

int fs_population_act_dev(fs_handle h, const fs_policy* pol, const fs_population* pop, const float* obs_dev, float* act_dev,
                          float* logp_dev) {
  if (!h || !pol || !pop || !obs_dev || !act_dev || !logp_dev)
    return fail(FS_ERR_INVALID, "fs_population_act_dev: NULL argument");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_population(pol, pop, 0, 0, 0, obs_dev, nullptr, act_dev, logp_dev, nullptr, nullptr);
}

int fs_population_rollout_dev(fs_handle h, const fs_policy* pol, const fs_population* pop, int num_steps, int reset_done,
                              float* obs_dev, float* act_dev, float* logp_dev, float* rew_dev, uint8_t* done_dev) {
  if (!h || !pol || !pop || !obs_dev || !act_dev || !logp_dev || !rew_dev || !done_dev)
    return fail(FS_ERR_INVALID, "fs_population_rollout_dev: NULL argument");
  if (num_steps < 1) return fail(FS_ERR_INVALID, "fs_population_rollout_dev: num_steps < 1");
  DeviceGuard guard(S(h)->cfg.device);
  return S(h)->launch_population(pol, pop, 0, num_steps, reset_done ? 1 : 0, nullptr, obs_dev, act_dev, logp_dev, rew_dev,
                                 done_dev);
}

// ---- evolution strategies (flowsim_es.h): the handle lends its device, its stream and fs_last_error
static const char* es_shape_why(int64_t num_params, int pairs, int eval_members) {
  if (num_params < 1 || num_params > (int64_t(1) << 24)) return "num_params must be 1 .. 2^24";
  if (pairs < 1 || pairs > fs::ES_MAX_PAIRS) return "pairs must be 1 .. 2048";
  if (eval_members < 0 || eval_members > 65535 - 2 * pairs) return "eval_members out of range";
  return nullptr;
}

int fs_es_perturb_dev(fs_handle h, int64_t num_params, int pairs, int eval_members, int64_t stride, const float* theta_dev,
                      float sigma, uint64_t noise_seed, uint32_t generation, float* weights_dev) {
  if (!h || !theta_dev || !weights_dev) return fail(FS_ERR_INVALID, "fs_es_perturb_dev: NULL argument");
  if (const char* why = es_shape_why(num_params, pairs, eval_members)) return fail(FS_ERR_INVALID, std::string("fs_es_perturb_dev: ") + why);
  if (stride < num_params) return fail(FS_ERR_INVALID, "fs_es_perturb_dev: stride < num_params");
  if (generation > 0x1FFFFFFFu) return fail(FS_ERR_INVALID, "fs_es_perturb_dev: generation must be below 2^29");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_es_perturb";
  return launch_es_perturb(S(h)->stream, num_params, pairs, eval_members, stride, theta_dev, sigma,
                           uint32_t(noise_seed & 0xFFFFFFFFull), uint32_t(noise_seed >> 32), generation, weights_dev);
}

int fs_es_fitness_dev(fs_handle h, int num_steps, int members, int group, const float* rew_dev, const uint8_t* done_dev,
                      int accumulate, double* ret_dev, uint8_t* alive_dev, double* fit_dev) {
  if (!h || !rew_dev || !done_dev || !ret_dev || !alive_dev || !fit_dev)
    return fail(FS_ERR_INVALID, "fs_es_fitness_dev: NULL argument");
  if (num_steps < 1 || members < 1 || group < 1) return fail(FS_ERR_INVALID, "fs_es_fitness_dev: num_steps, members and group must be at least 1");
  if ((long long)members * group != (long long)S(h)->cfg.num_replicas)
    return fail(FS_ERR_INVALID, "fs_es_fitness_dev: members * group != num_replicas");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_es_fitness";
  return launch_es_fitness(S(h)->stream, num_steps, members, group, rew_dev, done_dev, accumulate ? 1 : 0, ret_dev, alive_dev,
                           fit_dev);
}

int fs_es_weights_dev(fs_handle h, int mode, int pairs, int eval_members, int top, const double* fit_dev, float* u_dev,
                      double* stats_dev) {
  if (!h || !fit_dev || !u_dev || !stats_dev) return fail(FS_ERR_INVALID, "fs_es_weights_dev: NULL argument");
  if (mode != FS_ES_MODE_ES && mode != FS_ES_MODE_ARS) return fail(FS_ERR_INVALID, "fs_es_weights_dev: mode must be FS_ES_MODE_ES or FS_ES_MODE_ARS");
  if (const char* why = es_shape_why(1, pairs, eval_members)) return fail(FS_ERR_INVALID, std::string("fs_es_weights_dev: ") + why);
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_es_weights";
  return launch_es_weights(S(h)->stream, mode, pairs, eval_members, top, fit_dev, u_dev, stats_dev);
}

size_t fs_es_workspace(int64_t num_params, int pairs) {
  if (es_shape_why(num_params, pairs, 0)) return 0;
  return fs::es_work_floats(num_params, pairs);
}

int fs_es_grad_dev(fs_handle h, int mode, int64_t num_params, int pairs, const float* u_dev, uint64_t noise_seed,
                   uint32_t generation, float l2_or_stepsize, float* theta_dev, float* grad_dev, float* work_dev,
                   size_t work_floats) {
  if (!h || !u_dev || !theta_dev || !work_dev || (mode == FS_ES_MODE_ES && !grad_dev))
    return fail(FS_ERR_INVALID, "fs_es_grad_dev: NULL argument");
  if (mode != FS_ES_MODE_ES && mode != FS_ES_MODE_ARS) return fail(FS_ERR_INVALID, "fs_es_grad_dev: mode must be FS_ES_MODE_ES or FS_ES_MODE_ARS");
  if (const char* why = es_shape_why(num_params, pairs, 0)) return fail(FS_ERR_INVALID, std::string("fs_es_grad_dev: ") + why);
  if (generation > 0x1FFFFFFFu) return fail(FS_ERR_INVALID, "fs_es_grad_dev: generation must be below 2^29");
  if (work_floats < fs::es_work_floats(num_params, pairs))
    return fail(FS_ERR_INVALID, "fs_es_grad_dev: work_dev is smaller than fs_es_workspace(num_params, pairs) floats");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  if (!s->d_es_ticket) {
    // the first call on a handle allocates (and synchronises the device once): make it outside a stream capture
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, fs::ES_MAX_COLS * sizeof(unsigned)));
    s->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, fs::ES_MAX_COLS * sizeof(unsigned)));
    HIP_TRY(hipDeviceSynchronize());
    s->d_es_ticket = static_cast<unsigned*>(p);
  }
  s->last_kernel = "k_es_grad";
  return launch_es_grad(s->stream, mode, num_params, pairs, u_dev, uint32_t(noise_seed & 0xFFFFFFFFull),
                        uint32_t(noise_seed >> 32), generation, l2_or_stepsize, theta_dev, grad_dev, work_dev, s->d_es_ticket);
}

// ---- the PPO update on the device (flowsim_learn.h): the handle lends its device, its stream and fs_last_error
// the head of 2 A outputs, fs_policy's convention: no free log_std (log_std_dev == NULL), rows A .. 2A-1 are the log stds
static bool ppo_head_ls(const fs_ppo_model* m) { return m && m->struct_size == sizeof(fs_ppo_model) && !m->log_std_dev; }

// (free_head_only: the caller's kernel is not built for the head of 2 A outputs -- fs_ppo_grad_dev, the host-n gradient)
static int ppo_view(const char* who, const fs_ppo_model* m, bool need_policy, fs::PpoView* out, bool free_head_only = false) {
  const std::string w = std::string(who) + ": fs_ppo_model: ";
  if (!m) return fail(FS_ERR_INVALID, w + "NULL");
  if (m->struct_size != sizeof(fs_ppo_model)) return fail(FS_ERR_INVALID, w + "struct_size mismatch");
  if (m->obs_dim < 1 || m->obs_dim > fs::PPO_MAX_OBS)
    return fail(FS_ERR_UNSUPPORTED, w + "obs_dim must be 1..160");
  if (m->act_dim < 1 || m->act_dim > fs::PPO_MAX_ACT)
    return fail(FS_ERR_UNSUPPORTED, w + "act_dim must be 1..32");
  if (m->num_hidden < 1 || m->num_hidden > 3 || m->hidden_width != 32)
    return fail(FS_ERR_UNSUPPORTED, w + "1..3 hidden layers of 32 units");
  if (m->activation != 0) return fail(FS_ERR_UNSUPPORTED, w + "activation must be 0 (tanh)");
  if (need_policy && free_head_only && !m->log_std_dev)
    return fail(FS_ERR_UNSUPPORTED, w + "the head of 2 A outputs (no free log_std: log_std_dev is NULL) is not built for the "
                                        "gradient with the sample count from the host; fs_ppo_grad_n_dev takes it");
  if (!m->value_weights_dev || (need_policy && !m->policy_weights_dev)) return fail(FS_ERR_INVALID, w + "NULL weights");
  *out = fs::PpoView{m->policy_weights_dev, m->log_std_dev, m->value_weights_dev, m->obs_dim, m->act_dim, m->num_hidden};
  return FS_OK;
}

int fs_ppo_eval_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                    float* logp_dev, float* val_dev) {
  if (!h || !obs_dev || !val_dev || (act_dev && !logp_dev)) return fail(FS_ERR_INVALID, "fs_ppo_eval_dev: NULL argument");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_eval_dev: n must be 1 .. 2^31 - 1");
  fs::PpoView pv;
  if (int rc = ppo_view("fs_ppo_eval_dev", model, act_dev != nullptr, &pv)) return rc;
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = act_dev && ppo_net_ls(pv) ? "k_ppo_eval_ls" : "k_ppo_eval";
  return launch_ppo_eval(S(h)->stream, pv, n, obs_dev, act_dev, logp_dev, val_dev);
}

int fs_gae_dev(fs_handle h, int num_steps, int64_t num_cols, const float* rew_dev, const float* val_dev,
               const float* last_val_dev, const uint8_t* done_dev, double gamma, double lam, float* adv_dev, float* ret_dev) {
  if (!h || !rew_dev || !val_dev || !last_val_dev || !done_dev || !adv_dev || !ret_dev)
    return fail(FS_ERR_INVALID, "fs_gae_dev: NULL argument");
  if (num_steps < 1 || num_cols < 1 || num_cols > INT32_MAX) return fail(FS_ERR_INVALID, "fs_gae_dev: num_steps / num_cols out of range");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_gae";
  return launch_gae(S(h)->stream, num_steps, num_cols, rew_dev, val_dev, last_val_dev, done_dev, float(gamma),
                    float(gamma * lam), adv_dev, ret_dev);
}

size_t fs_ppo_workspace(const fs_ppo_model* model, int64_t n) {
  fs::PpoView pv;
  if (n < 1 || n > INT32_MAX || ppo_view("fs_ppo_workspace", model, false, &pv)) return 0;
  return fs::ppo_work_floats(n, pv.D, pv.A, pv.L, ppo_head_ls(model));
}

int fs_ppo_grad_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                    const float* logp_old_dev, const double* adv_dev, const float* ret_dev, const double* mean_std_dev,
                    float clip, float vf_coef, float inv_n_total, int accumulate, float* grad_dev, float* loss_dev,
                    float* work_dev, size_t work_floats) {
  if (ppo_head_ls(model)) {                                  // (refused from the model alone, whatever else is passed)
    fs::PpoView none;
    if (int rc = ppo_view("fs_ppo_grad_dev", model, true, &none, true)) return rc;
  }
  if (!h || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !ret_dev || !mean_std_dev || !grad_dev || !loss_dev || !work_dev)
    return fail(FS_ERR_INVALID, "fs_ppo_grad_dev: NULL argument");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_grad_dev: n must be 1 .. 2^31 - 1");
  fs::PpoView pv;
  if (int rc = ppo_view("fs_ppo_grad_dev", model, true, &pv, true)) return rc;
  if (work_floats < fs::ppo_work_floats(n, pv.D, pv.A, pv.L))
    return fail(FS_ERR_INVALID, "fs_ppo_grad_dev: work_dev is smaller than fs_ppo_workspace(model, n) floats");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_ppo_grad";
  // the clamp's bounds as torch takes them: the doubles 1 -+ clip rounded to float32
  return launch_ppo_grad(S(h)->stream, pv, n, obs_dev, act_dev, logp_old_dev, adv_dev, ret_dev, mean_std_dev,
                         float(1.0 - double(clip)), float(1.0 + double(clip)), vf_coef, inv_n_total, accumulate ? 1 : 0,
                         grad_dev, loss_dev, work_dev);
}

int fs_ppo_grad_n_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                      const float* logp_old_dev, const double* adv_dev, const float* ret_dev, const double* mean_std_n_dev,
                      float clip, float vf_coef, int accumulate, float* grad_dev, float* loss_dev, float* work_dev,
                      size_t work_floats) {
  if (!h || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !ret_dev || !mean_std_n_dev || !grad_dev || !loss_dev || !work_dev)
    return fail(FS_ERR_INVALID, "fs_ppo_grad_n_dev: NULL argument");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_grad_n_dev: n must be 1 .. 2^31 - 1");
  fs::PpoView pv;
  if (int rc = ppo_view("fs_ppo_grad_n_dev", model, true, &pv)) return rc;
  if (work_floats < fs::ppo_work_floats(n, pv.D, pv.A, pv.L, ppo_net_ls(pv)))
    return fail(FS_ERR_INVALID, "fs_ppo_grad_n_dev: work_dev is smaller than fs_ppo_workspace(model, n) floats");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = ppo_net_ls(pv) ? "k_ppo_grad_ls" : "k_ppo_grad";
  return launch_ppo_grad_n(S(h)->stream, pv, n, obs_dev, act_dev, logp_old_dev, adv_dev, ret_dev, mean_std_n_dev,
                           float(1.0 - double(clip)), float(1.0 + double(clip)), vf_coef, accumulate ? 1 : 0, grad_dev,
                           loss_dev, work_dev);
}

int fs_adv_stats_dev(fs_handle h, int64_t n, const float* adv_dev, const float* act_dev, int act_dim, int accumulate,
                     double* adv64_dev, double* stats_dev) {
  if (!h || !adv_dev || !adv64_dev || !stats_dev) return fail(FS_ERR_INVALID, "fs_adv_stats_dev: NULL argument");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_adv_stats_dev: n must be 1 .. 2^31 - 1");
  if (act_dev && (act_dim < 1 || act_dim > fs::PPO_MAX_ACT)) return fail(FS_ERR_INVALID, "fs_adv_stats_dev: act_dim must be 1..32");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  if (!s->d_adv_scratch) {
    // the first call on a handle allocates (and synchronises the device once): make it outside a stream capture
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, fs::ADV_SCRATCH_BYTES));
    s->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, fs::ADV_SCRATCH_BYTES));
    HIP_TRY(hipDeviceSynchronize());
    s->d_adv_scratch = static_cast<double*>(p);
  }
  s->last_kernel = "k_adv_stats";
  return launch_adv_stats(s->stream, n, adv_dev, act_dev, act_dim, accumulate ? 1 : 0, adv64_dev, stats_dev, s->d_adv_scratch);
}

int fs_episode_stats_dev(fs_handle h, int num_steps, const float* rew_dev, const uint8_t* done_dev, double* run_ret_dev,
                         int32_t* run_len_dev, double* stats_dev, int accumulate) {
  if (!h || !rew_dev || !done_dev || !run_ret_dev || !run_len_dev || !stats_dev)
    return fail(FS_ERR_INVALID, "fs_episode_stats_dev: NULL argument");
  if (num_steps < 1) return fail(FS_ERR_INVALID, "fs_episode_stats_dev: num_steps must be at least 1");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  if (!s->d_ep_scratch) {
    // the first call on a handle allocates (and synchronises the device once): make it outside a stream capture
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, fs::EP_SCRATCH_BYTES));
    s->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, fs::EP_SCRATCH_BYTES));
    HIP_TRY(hipDeviceSynchronize());
    s->d_ep_scratch = static_cast<double*>(p);
  }
  s->last_kernel = "k_episode_stats";
  return launch_episode_stats(s->stream, num_steps, (long long)s->cfg.num_replicas, rew_dev, done_dev, run_ret_dev, run_len_dev,
                              stats_dev, accumulate ? 1 : 0, s->d_ep_scratch);
}

int fs_adv_finish_dev(fs_handle h, const double* stats_dev, double* mean_std_n_dev) {
  if (!h || !stats_dev || !mean_std_n_dev) return fail(FS_ERR_INVALID, "fs_adv_finish_dev: NULL argument");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_adv_finish";
  return launch_adv_finish(S(h)->stream, stats_dev, mean_std_n_dev);
}

int fs_adam_dev(fs_handle h, int64_t num_params, float* weights_dev, const float* grad_dev, float* m_dev, float* v_dev,
                double* state_dev, double lr, double beta1, double beta2, double eps) {
  if (!h || !weights_dev || !grad_dev || !m_dev || !v_dev || !state_dev) return fail(FS_ERR_INVALID, "fs_adam_dev: NULL argument");
  if (num_params < 1 || num_params > INT32_MAX) return fail(FS_ERR_INVALID, "fs_adam_dev: num_params must be 1 .. 2^31 - 1");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_adam";
  return launch_adam(S(h)->stream, int(num_params), weights_dev, grad_dev, m_dev, v_dev, state_dev, lr, beta1, beta2, eps);
}

// ---- the reference's PPO loss (KL penalty, clipped value loss, entropy): additive entry points
int fs_ppo_eval_dist_dev(fs_handle h, const fs_ppo_model* model, int64_t n, const float* obs_dev, const float* act_dev,
                         float* logp_dev, float* val_dev, float* mean_old_dev) {
  if (!h || !obs_dev || !act_dev || !logp_dev || !val_dev || !mean_old_dev)
    return fail(FS_ERR_INVALID, "fs_ppo_eval_dist_dev: NULL argument");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_eval_dist_dev: n must be 1 .. 2^31 - 1");
  fs::PpoView pv;
  if (int rc = ppo_view("fs_ppo_eval_dist_dev", model, true, &pv)) return rc;
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = ppo_net_ls(pv) ? "k_ppo_eval_ls" : "k_ppo_eval";
  return launch_ppo_eval_dist(S(h)->stream, pv, n, obs_dev, act_dev, logp_dev, val_dev, mean_old_dev);
}

size_t fs_ppo_loss_workspace(const fs_ppo_model* model, int64_t n) {
  fs::PpoView pv;
  if (n < 1 || n > INT32_MAX || ppo_view("fs_ppo_loss_workspace", model, false, &pv)) return 0;
  return fs::ppo_loss_work_floats(n, pv.D, pv.A, pv.L, ppo_head_ls(model));
}

// fs_ppo_loss and the old distribution's pointers -> the kernels' PpoLossArgs (refusals name fs_ppo_loss).  head_ls (the
// head of 2 A outputs): the old log stds travel in mean_old_dev [n, 2A] and log_std_old_dev must be NULL
static int ppo_loss_args(const char* who, const fs_ppo_loss* loss, const float* mean_old_dev, const float* log_std_old_dev,
                         const float* val_old_dev, fs::PpoLossArgs* out, bool head_ls) {
  const std::string w = std::string(who) + ": fs_ppo_loss: ";
  if (head_ls && log_std_old_dev)
    return fail(FS_ERR_INVALID, std::string(who) + ": log_std_old_dev must be NULL with the head of 2 A outputs (fs_ppo_model's "
                                "log_std_dev is NULL): mean_old_dev holds [n, 2A], a row's means and then its log stds");
  if (!loss) return fail(FS_ERR_INVALID, w + "NULL");
  if (loss->struct_size != sizeof(fs_ppo_loss)) return fail(FS_ERR_INVALID, w + "struct_size mismatch");
  if (std::isnan(loss->clip) || std::isnan(loss->vf_coef) || std::isnan(loss->vf_clip) || std::isnan(loss->entropy_coef))
    return fail(FS_ERR_INVALID, w + "a coefficient is NaN");
  if (loss->clip < 0.0f) return fail(FS_ERR_INVALID, w + "clip must not be negative");
  const bool vclip = loss->vf_clip > 0.0f && std::isfinite(loss->vf_clip);
  if (loss->kl_state_dev && head_ls && !mean_old_dev)
    return fail(FS_ERR_INVALID, w + "the KL term (kl_state_dev) needs mean_old_dev [n, 2A]");
  if (loss->kl_state_dev && !head_ls && (!mean_old_dev || !log_std_old_dev))
    return fail(FS_ERR_INVALID, w + "the KL term (kl_state_dev) needs mean_old_dev and log_std_old_dev");
  if (vclip && !val_old_dev) return fail(FS_ERR_INVALID, w + "value clipping (vf_clip > 0) needs val_old_dev");
  *out = fs::PpoLossArgs{mean_old_dev, log_std_old_dev, val_old_dev, loss->kl_state_dev, vclip ? loss->vf_clip : 0.0f,
                         loss->entropy_coef};
  return FS_OK;
}

int fs_ppo_grad_loss_dev(fs_handle h, const fs_ppo_model* model, const fs_ppo_loss* loss, int64_t n, const float* obs_dev,
                         const float* act_dev, const float* logp_old_dev, const float* mean_old_dev,
                         const float* log_std_old_dev, const float* val_old_dev, const double* adv_dev, const float* ret_dev,
                         const double* mean_std_n_dev, int accumulate, float* grad_dev, float* loss_sums_dev, float* work_dev,
                         size_t work_floats) {
  fs::PpoLossArgs x;
  if (ppo_head_ls(model) && log_std_old_dev)                 // (refused from the arguments alone: the message is ppo_loss_args')
    return ppo_loss_args("fs_ppo_grad_loss_dev", loss, mean_old_dev, log_std_old_dev, val_old_dev, &x, true);
  if (!h || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !ret_dev || !mean_std_n_dev || !grad_dev || !loss_sums_dev ||
      !work_dev)
    return fail(FS_ERR_INVALID, "fs_ppo_grad_loss_dev: NULL argument");
  if (int rc = ppo_loss_args("fs_ppo_grad_loss_dev", loss, mean_old_dev, log_std_old_dev, val_old_dev, &x, ppo_head_ls(model)))
    return rc;
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_grad_loss_dev: n must be 1 .. 2^31 - 1");
  fs::PpoView pv;
  if (int rc = ppo_view("fs_ppo_grad_loss_dev", model, true, &pv)) return rc;
  if (work_floats < fs::ppo_loss_work_floats(n, pv.D, pv.A, pv.L, ppo_net_ls(pv)))
    return fail(FS_ERR_INVALID, "fs_ppo_grad_loss_dev: work_dev is smaller than fs_ppo_loss_workspace(model, n) floats");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = ppo_net_ls(pv) ? "k_ppo_grad_loss_ls" : "k_ppo_grad_loss";
  return launch_ppo_grad_loss(S(h)->stream, pv, x, n, obs_dev, act_dev, logp_old_dev, adv_dev, ret_dev, mean_std_n_dev,
                              float(1.0 - double(loss->clip)), float(1.0 + double(loss->clip)), loss->vf_coef,
                              accumulate ? 1 : 0, grad_dev, loss_sums_dev, work_dev);
}

int fs_kl_adapt_dev(fs_handle h, const float* loss_sums_dev, const double* mean_std_n_dev, double* kl_state_dev,
                    double kl_target) {
  if (!h || !loss_sums_dev || !mean_std_n_dev || !kl_state_dev) return fail(FS_ERR_INVALID, "fs_kl_adapt_dev: NULL argument");
  if (!(kl_target > 0.0) || !std::isfinite(kl_target)) return fail(FS_ERR_INVALID, "fs_kl_adapt_dev: kl_target must be positive and finite");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_kl_adapt";
  return launch_kl_adapt(S(h)->stream, loss_sums_dev, mean_std_n_dev, kl_state_dev, kl_target);
}

// ---- minibatch SGD: one launch per step (k_ppo_minibatch), the chain's finish (k_mb_finish), the permutation on the host
static_assert(FS_MB_STEP == fs::MB_STEP && FS_MB_PARTIAL == fs::MB_PARTIAL && FS_MB_ACCUMULATE == fs::MB_ACCUMULATE &&
              FS_MB_FIRST == fs::MB_FIRST && FS_MB_LAST == fs::MB_LAST, "include/flowsim.h and flowsim_learn.h agree");
int fs_ppo_perm_host(uint64_t seed, uint64_t epoch, int64_t n, int64_t* out) {
  if (!out) return fail(FS_ERR_INVALID, "fs_ppo_perm_host: NULL argument");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_perm_host: n must be 1 .. 2^31 - 1");
  const fs::PermKey k = fs::perm_key(seed, epoch, uint32_t(n));
  for (int64_t i = 0; i < n; ++i) out[i] = int64_t(fs::perm_at(k, uint32_t(i)));
  return FS_OK;
}

size_t fs_ppo_minibatch_workspace(const fs_ppo_model* model, int64_t batch) {
  fs::PpoView pv;
  if (batch < 1 || batch > INT32_MAX || ppo_view("fs_ppo_minibatch_workspace", model, false, &pv)) return 0;
  return fs::ppo_mb_work_floats(batch, pv.D, pv.A, pv.L, ppo_head_ls(model));
}

int fs_ppo_minibatch_dev(fs_handle h, const fs_ppo_model* model, const fs_ppo_loss* loss, const fs_ppo_minibatch* mb, int64_t n,
                         const float* obs_dev, const float* act_dev, const float* logp_old_dev, const float* mean_old_dev,
                         const float* log_std_old_dev, const float* val_old_dev, const double* adv_dev, const float* ret_dev,
                         const double* mean_std_n_dev, float* grad_dev, float* loss_sums_dev, float* work_dev,
                         size_t work_floats) {
  const std::string w = "fs_ppo_minibatch_dev: fs_ppo_minibatch: ";
  if (!mb) return fail(FS_ERR_INVALID, w + "NULL");
  if (mb->struct_size != sizeof(fs_ppo_minibatch)) return fail(FS_ERR_INVALID, w + "struct_size mismatch");
  if (mb->mode != FS_MB_STEP && mb->mode != FS_MB_PARTIAL) return fail(FS_ERR_INVALID, w + "mode must be FS_MB_STEP or FS_MB_PARTIAL");
  if (mb->flags & ~(FS_MB_ACCUMULATE | FS_MB_FIRST | FS_MB_LAST)) return fail(FS_ERR_INVALID, w + "unknown flags");
  if (mb->batch < 1 || mb->batch > INT32_MAX) return fail(FS_ERR_INVALID, w + "batch (B) must be 1 .. 2^31 - 1");
  if (n < 1 || n > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_minibatch_dev: n must be 1 .. 2^31 - 1");
  if (mb->index < 0 || mb->index > (n - 1) / mb->batch) return fail(FS_ERR_INVALID, w + "index (k) must be 0 .. ceil(n / batch) - 1");
  if (!mb->epoch_dev) return fail(FS_ERR_INVALID, w + "epoch_dev is NULL");
  fs::PpoView pv;
  if (int rc = ppo_view("fs_ppo_minibatch_dev", model, true, &pv)) return rc;
  if (mb->mode == FS_MB_STEP) {
    if (!mb->state_dev) return fail(FS_ERR_INVALID, w + "state_dev is NULL (FS_MB_STEP applies Adam)");
    if (!mb->m_dev) return fail(FS_ERR_INVALID, w + "m_dev is NULL (FS_MB_STEP applies Adam)");
    if (!mb->v_dev) return fail(FS_ERR_INVALID, w + "v_dev is NULL (FS_MB_STEP applies Adam)");
    if (!mb->weights_dev) return fail(FS_ERR_INVALID, w + "weights_dev is NULL (FS_MB_STEP applies Adam)");
    if (mb->flags & FS_MB_ACCUMULATE) return fail(FS_ERR_INVALID, w + "FS_MB_ACCUMULATE needs FS_MB_PARTIAL (a step has one shard)");
    const int Pp = fs::ppo_net_params(pv.D, pv.L, pv.A);
    if (ppo_net_ls(pv)) {
      if (pv.pw != mb->weights_dev || pv.vw != mb->weights_dev + fs::ppo_net_params(pv.D, pv.L, 2 * pv.A))
        return fail(FS_ERR_INVALID, w + "weights_dev must be the packed buffer [policy][value] that fs_ppo_model points into");
    } else if (pv.pw != mb->weights_dev || pv.log_std != mb->weights_dev + Pp || pv.vw != mb->weights_dev + Pp + pv.A)
      return fail(FS_ERR_INVALID, w + "weights_dev must be the packed buffer [policy][log_std A][value] that fs_ppo_model points into");
  } else if (!mb->count_dev) {
    return fail(FS_ERR_INVALID, w + "count_dev is NULL (FS_MB_PARTIAL leaves the count there)");
  }
  fs::PpoLossArgs x;
  if (int rc = ppo_loss_args("fs_ppo_minibatch_dev", loss, mean_old_dev, log_std_old_dev, val_old_dev, &x, ppo_net_ls(pv)))
    return rc;
  if (!h || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !ret_dev || !mean_std_n_dev || !grad_dev || !loss_sums_dev ||
      !work_dev)
    return fail(FS_ERR_INVALID, "fs_ppo_minibatch_dev: NULL argument");
  if (work_floats < fs::ppo_mb_work_floats(mb->batch, pv.D, pv.A, pv.L, ppo_net_ls(pv)))
    return fail(FS_ERR_INVALID, "fs_ppo_minibatch_dev: work_dev is smaller than fs_ppo_minibatch_workspace(model, batch) floats");
  SimBase* s = S(h);
  DeviceGuard guard(s->cfg.device);
  if (!s->d_mb_ticket) {
    // the first call on a handle allocates (and synchronises the device once): make it outside a stream capture
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, 64));
    s->allocs.push_back(p);
    HIP_TRY(hipMemset(p, 0, 64));
    HIP_TRY(hipDeviceSynchronize());
    s->d_mb_ticket = static_cast<unsigned*>(p);
  }
  const fs::PpoMbArgs a{mb->seed, reinterpret_cast<unsigned long long*>(mb->epoch_dev), mb->batch, mb->index,
                        mb->mode == FS_MB_STEP ? fs::MB_STEP : fs::MB_PARTIAL, mb->flags, s->d_mb_ticket, grad_dev, loss_sums_dev,
                        mb->count_dev, mb->weights_dev, mb->m_dev, mb->v_dev, mb->state_dev, mb->lr, mb->beta1, mb->beta2, mb->eps};
  s->last_kernel = ppo_net_ls(pv) ? "k_ppo_minibatch_ls" : "k_ppo_minibatch";
  return launch_ppo_minibatch(s->stream, pv, x, a, n, obs_dev, act_dev, logp_old_dev, adv_dev, ret_dev, mean_std_n_dev,
                              float(1.0 - double(loss->clip)), float(1.0 + double(loss->clip)), loss->vf_coef, work_dev);
}

int fs_ppo_mb_finish_dev(fs_handle h, int64_t num_params, float* weights_dev, float* grad_dev, float* m_dev, float* v_dev,
                         double* state_dev, const double* count_dev, uint64_t* epoch_dev, int flags, double lr, double beta1,
                         double beta2, double eps) {
  if (!state_dev) return fail(FS_ERR_INVALID, "fs_ppo_mb_finish_dev: state_dev is NULL");
  if (!m_dev) return fail(FS_ERR_INVALID, "fs_ppo_mb_finish_dev: m_dev is NULL");
  if (!v_dev) return fail(FS_ERR_INVALID, "fs_ppo_mb_finish_dev: v_dev is NULL");
  if (!h || !weights_dev || !grad_dev || !count_dev || !epoch_dev) return fail(FS_ERR_INVALID, "fs_ppo_mb_finish_dev: NULL argument");
  if (num_params < 1 || num_params > INT32_MAX) return fail(FS_ERR_INVALID, "fs_ppo_mb_finish_dev: num_params must be 1 .. 2^31 - 1");
  if (flags & ~FS_MB_LAST) return fail(FS_ERR_INVALID, "fs_ppo_mb_finish_dev: flags may hold FS_MB_LAST alone");
  DeviceGuard guard(S(h)->cfg.device);
  S(h)->last_kernel = "k_mb_finish";
  return launch_mb_finish(S(h)->stream, int(num_params), weights_dev, grad_dev, m_dev, v_dev, state_dev, count_dev,
                          reinterpret_cast<unsigned long long*>(epoch_dev), flags, lr, beta1, beta2, eps);
}

// ---- snapshots (flowsim_snap.h): every refusal is decided from the arguments and the handle's host fields, before any HIP call
// the sequence of copies k_snapshot replaces (FLOWSIM_SNAPSHOT_COPIES=1, unmasked): one stream-ordered copy per field
static int snapshot_copies(SimBase* s, char* blob, bool restore) {
  for (int k = 0; k < s->snap.n; ++k) {
    const fs::SnapEntry& en = s->snap.e[k];
    const size_t n = size_t(s->cfg.num_replicas) * en.row;
    HIP_TRY(hipMemcpyAsync(restore ? en.ptr : blob + en.off, restore ? blob + en.off : en.ptr, n, hipMemcpyDeviceToDevice, s->stream));
  }
  return FS_OK;
}

int fs_snapshot_info(fs_handle h, struct fs_snapshot_info* out) {
  if (!out) return fail(FS_ERR_INVALID, "fs_snapshot_info: out is NULL");
  if (!h) return fail(FS_ERR_INVALID, "fs_snapshot_info: NULL handle");
  const SimBase* s = S(h);
  out->bytes = uint64_t(s->snap_bytes);
  out->host_bytes = uint64_t(s->snap_bytes + sizeof(fs::SnapHostHeader));
  out->layout = s->snap_layout;
  out->nonce = s->snap_nonce;
  out->num_fields = s->snap.n;
  out->reserved = 0;
  return FS_OK;
}

int fs_snapshot_dev(fs_handle h, void* dst_dev, size_t bytes, const uint8_t* mask_dev) {
  if (!dst_dev) return fail(FS_ERR_INVALID, "fs_snapshot_dev: dst_dev is NULL");
  if (bytes == 0) return fail(FS_ERR_INVALID, "fs_snapshot_dev: wrong bytes (0; fs_snapshot_info.bytes)");
  if (!h) return fail(FS_ERR_INVALID, "fs_snapshot_dev: NULL handle");
  SimBase* s = S(h);
  if (bytes != s->snap_bytes)
    return fail(FS_ERR_INVALID, "fs_snapshot_dev: wrong bytes (" + std::to_string(bytes) + "; fs_snapshot_info.bytes is " +
                                    std::to_string(s->snap_bytes) + ")");
  DeviceGuard guard(s->cfg.device);
  s->snap_mirrors_out();
  if (s->snap_copies && !mask_dev) return snapshot_copies(s, static_cast<char*>(dst_dev), false);
  HIP_TRY(fs::launch_snapshot(s->stream, s->snap, false, static_cast<char*>(dst_dev), mask_dev));
  return FS_OK;
}

int fs_restore_dev(fs_handle h, const void* src_dev, size_t bytes, uint64_t layout, uint64_t nonce, const uint8_t* mask_dev) {
  if (!src_dev) return fail(FS_ERR_INVALID, "fs_restore_dev: src_dev is NULL");
  if (bytes == 0) return fail(FS_ERR_INVALID, "fs_restore_dev: wrong bytes (0; fs_snapshot_info.bytes)");
  if (!h) return fail(FS_ERR_INVALID, "fs_restore_dev: NULL handle");
  SimBase* s = S(h);
  if (layout != s->snap_layout)
    return fail(FS_ERR_INVALID, "fs_restore_dev: wrong layout (the blob is of a handle with another precision, shape, network "
                                "or environment: fs_snapshot_info.layout)");
  if (bytes != s->snap_bytes)
    return fail(FS_ERR_INVALID, "fs_restore_dev: wrong bytes (" + std::to_string(bytes) + "; fs_snapshot_info.bytes is " +
                                    std::to_string(s->snap_bytes) + ")");
  if (nonce != s->snap_nonce)
    return fail(FS_ERR_INVALID, "fs_restore_dev: foreign nonce (a device blob goes back into the handle it was taken from; "
                                "fs_snapshot / fs_restore carry state between handles)");
  DeviceGuard guard(s->cfg.device);
  s->snap_mirrors_in();
  if (s->snap_copies && !mask_dev) return snapshot_copies(s, static_cast<char*>(const_cast<void*>(src_dev)), true);
  HIP_TRY(fs::launch_snapshot(s->stream, s->snap, true, static_cast<char*>(const_cast<void*>(src_dev)), mask_dev));
  return FS_OK;
}

int fs_snapshot(fs_handle h, void* host_dst, size_t bytes) {
  if (!host_dst) return fail(FS_ERR_INVALID, "fs_snapshot: host_dst is NULL");
  if (bytes == 0) return fail(FS_ERR_INVALID, "fs_snapshot: wrong bytes (0; fs_snapshot_info.host_bytes)");
  if (!h) return fail(FS_ERR_INVALID, "fs_snapshot: NULL handle");
  SimBase* s = S(h);
  if (bytes != s->snap_bytes + sizeof(fs::SnapHostHeader))
    return fail(FS_ERR_INVALID, "fs_snapshot: wrong bytes (" + std::to_string(bytes) + "; fs_snapshot_info.host_bytes is " +
                                    std::to_string(s->snap_bytes + sizeof(fs::SnapHostHeader)) + ")");
  DeviceGuard guard(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (int qrc = s->check_qflag()) return qrc;
  char* out = static_cast<char*>(host_dst);
  std::memset(out, 0, bytes);                             // (the padding between fields too: equal states, equal blobs)
  fs::SnapHostHeader hd{};
  hd.magic = fs::SNAP_MAGIC;
  hd.layout = s->snap_layout;
  hd.dev_bytes = uint64_t(s->snap_bytes);
  hd.after_reset = s->after_reset;
  std::memcpy(out, &hd, sizeof(hd));
  for (int k = 0; k < s->snap.n; ++k) {
    const fs::SnapEntry& en = s->snap.e[k];
    HIP_TRY(hipMemcpy(out + sizeof(hd) + en.off, en.ptr, size_t(s->cfg.num_replicas) * en.row, hipMemcpyDeviceToHost));
  }
  return FS_OK;
}

int fs_restore(fs_handle h, const void* host_src, size_t bytes, uint64_t layout) {
  if (!host_src) return fail(FS_ERR_INVALID, "fs_restore: host_src is NULL");
  if (bytes == 0) return fail(FS_ERR_INVALID, "fs_restore: wrong bytes (0; fs_snapshot_info.host_bytes)");
  if (!h) return fail(FS_ERR_INVALID, "fs_restore: NULL handle");
  SimBase* s = S(h);
  if (layout != s->snap_layout)
    return fail(FS_ERR_INVALID, "fs_restore: wrong layout (the blob is of a handle with another precision, shape, network or "
                                "environment: fs_snapshot_info.layout)");
  if (bytes != s->snap_bytes + sizeof(fs::SnapHostHeader))
    return fail(FS_ERR_INVALID, "fs_restore: wrong bytes (" + std::to_string(bytes) + "; fs_snapshot_info.host_bytes is " +
                                    std::to_string(s->snap_bytes + sizeof(fs::SnapHostHeader)) + ")");
  const char* in = static_cast<const char*>(host_src);
  fs::SnapHostHeader hd;
  std::memcpy(&hd, in, sizeof(hd));
  if (hd.magic != fs::SNAP_MAGIC || hd.layout != layout || hd.dev_bytes != uint64_t(s->snap_bytes))
    return fail(FS_ERR_INVALID, "fs_restore: wrong layout (the blob's own header does not name this layout: not a blob of "
                                "fs_snapshot, or of another handle shape)");
  DeviceGuard guard(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int k = 0; k < s->snap.n; ++k) {
    const fs::SnapEntry& en = s->snap.e[k];
    HIP_TRY(hipMemcpy(en.ptr, in + sizeof(hd) + en.off, size_t(s->cfg.num_replicas) * en.row, hipMemcpyHostToDevice));
  }
  s->snap_mirrors_blob(in + sizeof(hd));
  s->after_reset = hd.after_reset;
  return FS_OK;
}

const char* fs_last_kernel(fs_handle h) { return h ? reinterpret_cast<SimBase*>(h)->last_kernel : ""; }

int fs_dump_trajectory(fs_handle h, int replica, const char* csv_path) {
  if (!h || !csv_path) return fail(FS_ERR_INVALID, "fs_dump_trajectory: NULL argument");
  SimBase* s = S(h);
  if (replica < 0 || replica >= s->cfg.num_replicas) return fail(FS_ERR_INVALID, "fs_dump_trajectory: replica out of range");
  DeviceGuard guard(s->cfg.device);
  const size_t R = size_t(s->cfg.num_replicas), N = size_t(s->cfg.num_vehicles);
  const bool f32 = s->cfg.precision == FS_F32 || s->cfg.precision == FS_F16S;
  const size_t el = f32 ? sizeof(float) : sizeof(double);
  std::vector<char> pos(R * N * el), vel(R * N * el);
  std::vector<int32_t> tc(R), lane(R * N, 0);
  int rc = s->get_state(FS_FIELD_POS, pos.data(), pos.size());
  if (!rc) rc = s->get_state(FS_FIELD_VEL, vel.data(), vel.size());
  if (!rc) rc = s->get_state(FS_FIELD_TIME, tc.data(), R * sizeof(int32_t));
  const bool open_net = s->cfg.network == FS_NET_MERGE || s->cfg.network == FS_NET_BOTTLENECK;
  if (!rc && (open_net || s->cfg.num_lanes > 1))
    rc = s->get_state(open_net ? FS_FIELD_ROUTE : FS_FIELD_LANE, lane.data(), R * N * sizeof(int32_t));
  if (rc) return rc;
  FILE* probe = std::fopen(csv_path, "r");
  const bool fresh = probe == nullptr;
  if (probe) std::fclose(probe);
  FILE* f = std::fopen(csv_path, "a");
  if (!f) return fail(FS_ERR_INVALID, std::string("fs_dump_trajectory: cannot open ") + csv_path);
  if (fresh) std::fprintf(f, "time,id,x,speed,lane_number\n");
  const double t = double(tc[replica]) * s->cfg.sim_step;
  for (size_t i = 0; i < N; ++i) {
    const size_t e = size_t(replica) * N + i;
    if (open_net && lane[e] < 0) continue;                       // a free slot: no vehicle
    const double x = f32 ? double(reinterpret_cast<const float*>(pos.data())[e]) : reinterpret_cast<const double*>(pos.data())[e];
    const double v = f32 ? double(reinterpret_cast<const float*>(vel.data())[e]) : reinterpret_cast<const double*>(vel.data())[e];
    std::fprintf(f, "%.6f,%zu,%.17g,%.17g,%d\n", t, i, x, v, int(lane[e]));
  }
  std::fclose(f);
  return FS_OK;
}

}  // extern "C"
