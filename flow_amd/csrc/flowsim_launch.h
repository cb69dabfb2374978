// flowsim_launch.h -- the Sim<T>::launch_* that Sim<T>::launch_steps chooses from (flowsim_sim.h): each maps the
// handle's run-time switches to the template arguments of its kernel family and launches it.  Included by
// flowsim_part.hip only, so that each (precision, width) pair and its kernels compile in an object of their own.
#pragma once
#include "flowsim_sim.h"
#ifdef FS_PART_QUEUE
#include "flowsim_queue.h"
#include "flowsim_dropq.h"
#endif

namespace fsim {

#ifdef FS_PART_QUEUE
  template <typename T>
  int Sim<T>::launch_queue(const StepArgs& a) {
    // MergePOEnv always applies its action row (one column per place of rl_veh); the multi-agent head when asked to
    const bool po = dv.env == FS_ENV_MERGE_PO;
    const bool noise = (dv.flags & fs::FLAG_HAS_NOISE) != 0, act = a.actions != nullptr && (po || ov.ma_apply_actions != 0);
    const auto k = pick(noise, [&](auto NZ) {
      return pick(act, [&](auto ACT) {
        return pick(po, [&](auto PO) { return &fs::k_merge_queue<NZ, ACT, false, PO>; });
      });
    });
    last_kernel = "k_merge_queue";
    hipLaunchKernelGGL(k, dim3(dv.R), dim3(64), 0, stream, dv, ov, qc, a.num_steps, a.actions, a.act_stride, a.obs, a.rew,
                       a.done, a.obs_every_step, fs::PolicyView{}, static_cast<float*>(nullptr), static_cast<float*>(nullptr),
                       0);
    return launched();
  }
  // the multi-agent merge with its agents sharing the policy: k_merge_queue's POLICY form (one wave per replica);
  // MergePOEnv with its action-vector policy: k_merge_policy
  template <typename T>
  int Sim<T>::launch_policy_queue(const fs::PolicyView& pv, int num_steps, int reset_done, float* obs, float* act,
                                  float* logp, float* rew, uint8_t* done) {
    const bool noise = (dv.flags & fs::FLAG_HAS_NOISE) != 0;
    if (dv.env == FS_ENV_MERGE_PO) {
      const bool wide = dv.num_rl > fs::FS_POLICY_VEC_MAX;       // more than 32 inputs: policy_wide_act in the loop
      const auto kp = wide ? pick(noise, [&](auto NZ) { return &fs::k_merge_wide_policy<NZ>; })
                           : pick(noise, [&](auto NZ) { return &fs::k_merge_policy<NZ>; });
      last_kernel = wide ? "k_merge_policy<PO,WIDE>" : "k_merge_policy<PO>";
      hipLaunchKernelGGL(kp, dim3(dv.R), dim3(64), 0, stream, dv, ov, qc, num_steps, obs, rew, done, pv, act, logp,
                         reset_done);
      return launched();
    }
    const auto k = pick(noise, [&](auto NZ) { return &fs::k_merge_queue<NZ, true, true>; });
    last_kernel = "k_merge_policy";
    hipLaunchKernelGGL(k, dim3(dv.R), dim3(64), 0, stream, dv, ov, qc, num_steps, static_cast<const float*>(nullptr),
                       size_t(0), obs, rew, done, 1, pv, act, logp, reset_done);
    return launched();
  }
  // the eager form of MergePOEnv's action-vector policy (one wave per replica, as in k_merge_policy)
  template <typename T>
  int Sim<T>::launch_policy_act_vec(const fs::PolicyView& pv, const float* obs_in, float* act, float* logp) {
    last_kernel = "k_policy_act_vec";
    hipLaunchKernelGGL(fs::k_policy_act_vec<16>, dim3(dv.R), dim3(64), 0, stream, pv, dv.R, dv.num_rl, dv.rep0, obs_in,
                       act, logp);
    return launched();
  }
  // the eager form of an action-vector policy with more than 32 inputs (BottleneckDesiredVelocityEnv; MergePOEnv with 7 .. 32
  // places): one wave per replica, four replicas per workgroup
  template <typename T>
  int Sim<T>::launch_policy_act_wide(const fs::PolicyView& pv, const float* obs_in, float* act, float* logp) {
    last_kernel = "k_policy_act_wide";
    hipLaunchKernelGGL(fs::k_policy_act_wide<16>, dim3((dv.R + 3) / 4), dim3(256), 0, stream, pv, dv.R, dv.num_rl, dv.rep0,
                       obs_in, act, logp);
    return launched();
  }
  template <typename T>
  int Sim<T>::launch_dropq(const StepArgs& a) {
    const auto k = dv.env == FS_ENV_BOTTLENECK_DV ? &fs::k_drop_queue<true> : &fs::k_drop_queue<false>;
    last_kernel = "k_drop_queue";
    qflag_armed = true;
    hipLaunchKernelGGL(k, dim3(dv.R), dim3(256), 0, stream, dv, ov, qc, d_qflag, a.num_steps, a.actions, a.act_stride,
                       a.obs, a.rew, a.done, a.obs_every_step);
    return launched();
  }
#endif

  // more than 64 slots per replica (lane-drop network): one workgroup of W waves per replica
  template <typename T>
  template <int W>
  int Sim<T>::launch_wide(const StepArgs& a) {
    // float32 exists twice (CSET = 1: IDM / RL / Sim slots only); num_paths = 8 is the scaling-2 network
    constexpr int C1 = std::is_same<T, float>::value ? 1 : 0;
    const bool cset = C1 == 1 && (dv.flags & fs::FLAG_IDM_SET) && !force_generic && open_div_ok;
    const auto k = cfg.num_paths == 8 ? (cset ? &fs::k_steps_wide<T, W, C1, 8> : &fs::k_steps_wide<T, W, 0, 8>)
                                      : (cset ? &fs::k_steps_wide<T, W, C1, 4> : &fs::k_steps_wide<T, W, 0, 4>);
    last_kernel = "k_steps_wide";
    hipLaunchKernelGGL(k, dim3(dv.R), dim3(64 * W), 0, stream, dv, ov, a.num_steps, a.mask, a.actions, a.act_stride, a.obs,
                       a.rew, a.done, a.obs_every_step, after_reset);
    return launched();
  }

  template <typename T>
  template <int SEG>
  int Sim<T>::launch_open(const StepArgs& a) {
    constexpr int RPW = 64 / SEG;
    const bool idm_set = (dv.flags & fs::FLAG_IDM_SET) && !force_generic;
    // CSET = 1: the branch-free controller selection for IDM / RL / Sim populations -- float32 within the div_core
    // premises; plain float64 always (the same operations as the generic instantiation, without its per-controller
    // exec-mask branches).  CSET = 2 (FS_MIXED): the float64 kernel with the float32 car-following models, within their
    // premises; a population outside them steps in plain float64 (CSET = 0)
    const bool cset = std::is_same<T, float>::value ? idm_set && open_div_ok : idm_set && !mixed;
    const bool mset = mixed && idm_set && open_div_ok;
    constexpr int C2 = std::is_same<T, double>::value ? 2 : 0;
    // k_steps_open<T, SEG, paths, CSET, probabilistic inflows, MergePOEnv head>
    auto kernel = [&](auto P, auto PO) {
      return pick(ov.n_prob > 0, [&](auto PR) {
        return cset ? &fs::k_steps_open<T, SEG, P, 1, PR, PO>
                    : mset ? &fs::k_steps_open<T, SEG, P, C2, PR, PO> : &fs::k_steps_open<T, SEG, P, 0, PR, PO>;
      });
    };
    decltype(kernel(Int<2>(), std::false_type())) k;
    last_kernel = "k_steps_open";
    if (cfg.network == FS_NET_BOTTLENECK) {
      // the lane-drop heads need more than 32 slots (fs_create checks it): only the 64-lane segment is built
      if constexpr (SEG == 64) k = kernel(Int<4>(), std::false_type());
      else return fail(FS_ERR_UNSUPPORTED, "fs_step: FS_NET_BOTTLENECK runs on 64-lane segments only");
    } else {
      k = pick(dv.env == FS_ENV_MERGE_PO, [&](auto PO) { return kernel(Int<2>(), PO); });
      if (mset) last_kernel = "k_steps_open<mixed>";
    }
    hipLaunchKernelGGL(k, dim3((dv.R + RPW - 1) / RPW), dim3(64), 0, stream, dv, ov, a.num_steps, a.mask, a.actions,
                       a.act_stride, a.obs, a.rew, a.done, a.obs_every_step, after_reset);
    return launched();
  }

  template <typename T>
  template <int SEG>
  int Sim<T>::launch_ml(const StepArgs& a) {
    constexpr int RPW = 64 / SEG;
    const bool lcpo = dv.env == FS_ENV_LANE_CHANGE_ACCEL_PO;
    const auto k = pick(dv.lc_enabled, [&](auto LC) {
      return pick(lcpo, [&](auto PO) { return &fs::k_steps_ml<T, SEG, LC, PO>; });
    });
    last_kernel = "k_steps_ml";
    hipLaunchKernelGGL(k, dim3((dv.R + RPW - 1) / RPW), dim3(64), 0, stream, dv, a.num_steps, a.mask, a.actions,
                       a.act_stride, a.obs, a.rew, a.done, a.obs_every_step);
    return launched();
  }

  // k_rollout_loop<head, every IDM delta = 4, FULL: the compiled-in noise / SUMO / junction features, float64 state>
  template <typename T>
  int Sim<T>::launch_loop(const StepArgs& a) {
    constexpr bool MX = !std::is_same<T, float>::value;
    const int f = dv.flags;
    const bool full = (f & fs::FLAG_HAS_NOISE) && (f & fs::FLAG_NEED_SUMO) && dv.junction_on && a.actions != nullptr &&
                      loop_delta4 && !no_loop_full && loop_fastc_ok();
    auto kernel = [&](auto H) {
      return full ? &fs::k_rollout_loop<H, true, true, MX>
                  : loop_delta4 ? &fs::k_rollout_loop<H, true, false, MX> : &fs::k_rollout_loop<H, false, false, MX>;
    };
    auto k = dv.env == FS_ENV_ACCEL ? kernel(Int<0>()) : kernel(Int<1>());      // AccelEnv, WaveAttenuationPOEnv
    last_kernel = full ? "k_rollout_loop<FULL>" : "k_rollout_loop";
    if constexpr (!MX) {
      if (dv.env == FS_ENV_ACCEL_PO_MA) {           // MultiAgentAccelPOEnv (float32 only)
        k = kernel(Int<2>());
        last_kernel = full ? "k_rollout_loop<FULL,AccelMA>" : "k_rollout_loop<AccelMA>";
      }
    }
    const int waves = (dv.R + 3) / 4;
    hipLaunchKernelGGL(k, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, a.num_steps, a.actions, a.act_stride, a.obs,
                       a.rew, a.done);
    return launched();
  }

  // k_ring_pair<T, ROW, head, noise, FAST, MC>
  template <typename T>
  template <int SEG>
  int Sim<T>::launch_ring(const StepArgs& a) {
    constexpr int ROW = SEG >= 16 ? SEG / 2 : 8;
    const bool fast = ringrl_fast_ok();
    const bool po = dv.env == FS_ENV_WAVE_ATTENUATION_PO;
    const bool ma_head = dv.env == FS_ENV_WAVE_ATTENUATION_PO_MA || dv.env == FS_ENV_ACCEL_PO_MA;   // float32 only
    // MC: the 16-step group form with several action columns (rows of 16 lanes only: 17..32 vehicles); the multi-agent
    // heads of that size always take it (it also steps without actions: the warm-up steps of a reset)
    const bool mc = ROW == 16 && std::is_same<T, float>::value && (ma_head || (a.actions != nullptr && dv.num_rl > 1));
    auto kernel = [&](auto H, auto MC) {
      return pick(dv.flags & fs::FLAG_HAS_NOISE, [&](auto NZ) {
        return pick(fast, [&](auto FA) { return &fs::k_ring_pair<T, ROW, H, NZ, FA, MC>; });
      });
    };
    auto single = [&](auto MC) { return po ? kernel(Int<1>(), MC) : kernel(Int<0>(), MC); };   // AccelEnv, the PO head
    decltype(single(std::false_type())) k;
    if constexpr (std::is_same<T, float>::value && ROW == 16) {
      const auto MC = std::true_type();
      k = !ma_head ? pick(mc, single) : dv.env == FS_ENV_ACCEL_PO_MA ? kernel(Int<3>(), MC) : kernel(Int<2>(), MC);
    } else if constexpr (std::is_same<T, float>::value) {
      const auto MC = std::false_type();
      k = !ma_head ? single(MC) : dv.env == FS_ENV_ACCEL_PO_MA ? kernel(Int<3>(), MC) : kernel(Int<2>(), MC);
    } else {
      k = single(std::false_type());
    }
    if constexpr (std::is_same<T, float>::value) {
      if (dv.env == FS_ENV_MULTI_WAVE_ATTENUATION_PO) k = kernel(Int<4>(), std::false_type());   // one action column: never MC
    }
    last_kernel = dv.env == FS_ENV_MULTI_WAVE_ATTENUATION_PO ? "k_ring_pair<MultiRing>" : ma_head ? (dv.env == FS_ENV_ACCEL_PO_MA ? "k_ring_pair<AccelMA>" : "k_ring_pair<POMA>")
                          : (po ? "k_ring_pair<PO>" : "k_ring_pair<Accel>");
    const int waves = (dv.R + (64 / ROW) - 1) / (64 / ROW);
    hipLaunchKernelGGL(k, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, a.num_steps, a.mask, a.actions, a.act_stride,
                       a.obs, a.rew, a.done, a.obs_every_step);
    return launched();
  }

  template <typename T>
  int Sim<T>::launch_obs_mixed(const StepArgs& a) {
    if constexpr (std::is_same<T, double>::value) {
      const int n = dv.R * dv.N;
      last_kernel = "k_obs_mixed";
      hipLaunchKernelGGL((fs::k_obs_mixed<T>), dim3((n + 255) / 256), dim3(256), 0, stream, dv, a.obs);
      return launched();
    } else {
      return fail(FS_ERR_UNSUPPORTED, "k_obs_mixed is a float64 kernel");
    }
  }

  // two vehicles per lane (flowsim_pair.h): k_rollout_pair<T, ROW, DELTA4, FASTDIV, BADCHK, speed mode, noise>
  template <typename T>
  template <int SEG>
  int Sim<T>::launch_pair(const StepArgs& a) {
    constexpr int ROW = SEG >= 16 ? SEG / 2 : 8;
    const bool fd = fastdiv_ok(), bc = neg_speed_possible, sm = speed_mode_any;
    const bool noise = std::is_same<T, float>::value && (dv.flags & fs::FLAG_HAS_NOISE);   // float32 only (pair_ok)
    // with the speed-mode clamps or the noise: exponent 4, the proven divisions and no v < -100 check, or any exponent,
    // IEEE divisions and the check (always valid)
    auto clamped = [&](auto SM, auto NZ) {
      return delta4 && fd && !bc ? &fs::k_rollout_pair<T, ROW, true, true, false, SM, NZ>
                                 : &fs::k_rollout_pair<T, ROW, false, false, true, SM, NZ>;
    };
    decltype(&fs::k_rollout_pair<T, ROW, false, false, true>) k = nullptr;
    if (noise) {
      if constexpr (std::is_same<T, float>::value) k = pick(sm, [&](auto SM) { return clamped(SM, std::true_type()); });
    } else if (sm) {                           // the reference's default speed mode "right_of_way" lands here
      k = clamped(std::true_type(), std::false_type());
    } else {
      k = pick(bc, [&](auto BC) {
        return delta4 && fd ? &fs::k_rollout_pair<T, ROW, true, true, BC>
                            : delta4 ? &fs::k_rollout_pair<T, ROW, true, false, BC> : &fs::k_rollout_pair<T, ROW, false, false, BC>;
      });
    }
    last_kernel = noise ? (sm ? "k_rollout_pair+speed_mode+noise" : "k_rollout_pair+noise")
                        : (sm ? "k_rollout_pair+speed_mode" : "k_rollout_pair");
    const int waves = (dv.R + (64 / ROW) - 1) / (64 / ROW);
    // the reference's ring of 22 vehicles in the hand-written class: k_rollout_pair_n<T, 11, speed mode, noise> -- for
    // launches long enough to pay for it.  The image of the launch's last full block leaves after the loop with nothing
    // to hide behind (11 KB per wave): a launch of 20 steps was 2-7 us (4-20 %) slower on this entry, a step of a long
    // one gains 0.013 us, so the entry pays from a few hundred steps on.
    if constexpr (SEG == 32) {
      if (dv.N == 22 && delta4 && fd && !bc && !pair_generic_n && (a.num_steps >= PAIR_N_MIN_STEPS || pair_n_always)) {
        decltype(&fs::k_rollout_pair_n<T, 11>) kn = nullptr;
        if constexpr (std::is_same<T, float>::value) {
          kn = pick(sm, [&](auto SM) { return pick(noise, [&](auto NZ) { return &fs::k_rollout_pair_n<T, 11, SM, NZ>; }); });
        } else {
          kn = pick(sm, [&](auto SM) { return &fs::k_rollout_pair_n<T, 11, SM>; });
        }
        if (kernel_detail)
          last_kernel = noise ? (sm ? "k_rollout_pair+speed_mode+noise[n11]" : "k_rollout_pair+noise[n11]")
                              : (sm ? "k_rollout_pair+speed_mode[n11]" : "k_rollout_pair[n11]");
        hipLaunchKernelGGL(kn, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, a.num_steps, a.obs, a.rew, a.done);
        return launched();
      }
    }
    hipLaunchKernelGGL(k, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, a.num_steps, a.obs, a.rew, a.done);
    return launched();
  }

  // one vehicle per lane: k_rollout_idm<T, SEG, DELTA4, FASTDIV, BADCHK>, 8 waves per block
  template <typename T>
  template <int SEG>
  int Sim<T>::launch_idm(const StepArgs& a) {
    constexpr int RPW = 64 / SEG;
    const bool fd = fastdiv_ok();
    const auto k = pick(neg_speed_possible, [&](auto BC) {
      return delta4 && fd ? &fs::k_rollout_idm<T, SEG, true, true, BC>
                          : delta4 ? &fs::k_rollout_idm<T, SEG, true, false, BC> : &fs::k_rollout_idm<T, SEG, false, false, BC>;
    });
    last_kernel = "k_rollout_idm";
    const int waves = (dv.R + RPW - 1) / RPW;
    hipLaunchKernelGGL(k, dim3((waves + 7) / 8), dim3(512), 0, stream, dv, a.num_steps, a.obs, a.rew, a.done, d_dump);
    return launched();
  }

  template <typename T>
  template <int SEG>
  int Sim<T>::launch_k_steps(const StepArgs& a) {
    constexpr int RPW = 64 / SEG;
    auto k = &fs::k_steps<T, SEG, 0, 0>;
    last_kernel = "k_steps";
    if (fast_ok(a)) {
      k = &fs::k_steps<T, SEG, 1, 0>;
      last_kernel = "k_steps<FAST>";
    } else if ((dv.flags & fs::FLAG_IDM_SET) && !force_generic) {
      k = &fs::k_steps<T, SEG, 0, 1>;
      last_kernel = "k_steps<CSET>";
    }
#ifdef FS_USER_ENV_HEADER
    // (a library with a user head: its k_steps takes the head's parameters as one more argument, FS_ENV_USER or not)
    fs::UserEnvParams<T> up;
    for (int k = 0; k < 8; ++k) up.p[k] = T(cfg.user_env_p[k]);
    hipLaunchKernelGGL(k, dim3((dv.R + RPW - 1) / RPW), dim3(64), 0, stream, dv, a.num_steps, a.mask, a.actions,
                       a.act_stride, a.obs, a.rew, a.done, a.obs_every_step, up);
#else
    hipLaunchKernelGGL(k, dim3((dv.R + RPW - 1) / RPW), dim3(64), 0, stream, dv, a.num_steps, a.mask, a.actions,
                       a.act_stride, a.obs, a.rew, a.done, a.obs_every_step);
#endif
    return launched();
  }

  template <typename T>
  int Sim<T>::launch_policy_act(const fs::PolicyView& pv, int n_ag, const float* obs_in, float* act, float* logp) {
    last_kernel = "k_policy_act";
    const bool merge = dv.env == FS_ENV_MERGE_MA;        // (agents present or not: the handle's current routes)
    hipLaunchKernelGGL(fs::k_policy_act<16>, dim3((dv.R * 16 + 255) / 256), dim3(256), 0, stream, pv, dv.R, n_ag, dv.rep0,
                       obs_in, act, logp, merge ? static_cast<const int*>(dv.lane) : nullptr,
                       merge ? static_cast<const int*>(dv.ctrl) : nullptr,
                       merge ? static_cast<const int*>(dv.rl_index) : nullptr, dv.N);
    return launched();
  }

  template <typename T>
  int Sim<T>::launch_policy_row16(const fs::PolicyView& pv, int num_steps, int reset_done, float* obs, float* act,
                                  float* logp, float* rew, uint8_t* done) {
    const bool fast = ringrl_fast_ok();
    auto kernel = [&](auto H) {
      return pick(dv.flags & fs::FLAG_HAS_NOISE, [&](auto NZ) {
        return pick(fast, [&](auto FA) { return &fs::k_ring_policy<T, H, NZ, FA>; });
      });
    };
    auto k = kernel(Int<1>());                                     // WaveAttenuationPOEnv
    last_kernel = "k_ring_policy";
    if constexpr (std::is_same<T, float>::value) {
      if (dv.env == FS_ENV_WAVE_ATTENUATION_PO_MA) {                // MultiAgentWaveAttenuationPOEnv (float32 only)
        k = kernel(Int<2>());
        last_kernel = "k_ring_policy<POMA>";
      }
      if (dv.env == FS_ENV_MULTI_WAVE_ATTENUATION_PO) {             // MultiWaveAttenuationPOEnv (float32 only)
        k = kernel(Int<4>());
        last_kernel = "k_ring_policy<MultiRing>";
      }
    }
    const int waves = (dv.R + 3) / 4;
    hipLaunchKernelGGL(k, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, pv, num_steps, reset_done, cfg.warmup_steps,
                       obs, act, logp, rew, done);
    return launched();
  }

  template <typename T>
  int Sim<T>::launch_policy_loop16(const fs::PolicyView& pv, int num_steps, int reset_done, float* obs, float* act,
                                   float* logp, float* rew, uint8_t* done) {
    if constexpr (std::is_same<T, float>::value) {
      const bool fastc = loop_delta4 && loop_fastc_ok();
      // (fs_policy.greedy picks the instantiation on this family: flowsim_policy.h policy_sample)
      auto kernel = [&](auto H) {
        if (pv.greedy)
          return fastc ? &fs::k_greedy_loop_policy<H, true, true>
                       : loop_delta4 ? &fs::k_greedy_loop_policy<H, true, false> : &fs::k_greedy_loop_policy<H, false, false>;
        return fastc ? &fs::k_loop_policy<H, true, true>
                     : loop_delta4 ? &fs::k_loop_policy<H, true, false> : &fs::k_loop_policy<H, false, false>;
      };
      if (dv.env == FS_ENV_ACCEL && dv.num_rl > 1) {      // ONE network, num_rl action columns: k_loop_policy_vec
        const auto kv = fastc ? &fs::k_loop_policy_vec<true, true>
                              : loop_delta4 ? &fs::k_loop_policy_vec<true, false> : &fs::k_loop_policy_vec<false, false>;
        last_kernel = "k_loop_policy<AccelVec>";
        const int waves_v = (dv.R + 3) / 4;
        hipLaunchKernelGGL(kv, dim3((waves_v + 3) / 4), dim3(256), 0, stream, dv, pv, num_steps, reset_done, obs, act, logp,
                           rew, done);
        return launched();
      }
      const auto k = dv.env == FS_ENV_WAVE_ATTENUATION_PO ? kernel(Int<1>())
                     : dv.env == FS_ENV_ACCEL_PO_MA ? kernel(Int<2>()) : kernel(Int<0>());
      last_kernel = dv.env == FS_ENV_ACCEL_PO_MA ? "k_loop_policy<AccelMA>" : "k_loop_policy";
      const int waves = (dv.R + 3) / 4;
      hipLaunchKernelGGL(k, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, pv, num_steps, reset_done, obs, act, logp, rew,
                         done);
      return launched();
    } else {
      return fail(FS_ERR_UNSUPPORTED, "k_loop_policy is a float32 kernel");
    }
  }

  // the eager form of the row-per-replica action-vector head (AccelEnv with 2 .. 16 RL vehicles on a segment-table loop):
  // a row of 16 lanes per replica, as in k_loop_policy_vec
  template <typename T>
  int Sim<T>::launch_policy_act_row16(const fs::PolicyView& pv, const float* obs_in, float* act, float* logp) {
    last_kernel = "k_policy_act_row";
    hipLaunchKernelGGL(fs::k_policy_act_row<16>, dim3((dv.R * 16 + 255) / 256), dim3(256), 0, stream, pv, dv.R, dv.num_rl,
                       dv.rep0, obs_in, act, logp);
    return launched();
  }

  // two policies on the AccelEnv head's one RL vehicle: k_policy_pair_act (obs == nullptr) or k_loop_policy_pair, in
  // k_loop_policy's instantiation for this handle
  template <typename T>
  int Sim<T>::launch_policy_pair16(const fs::PolicyView& pv, const fs::PolicyView& pv2, float pw, int num_steps,
                                   int reset_done, const float* obs_in, float* obs, float* act, float* logp, float* cmd,
                                   float* rew, uint8_t* done) {
    if constexpr (std::is_same<T, float>::value) {
      if (obs == nullptr) {
        last_kernel = "k_policy_pair_act";
        hipLaunchKernelGGL(fs::k_policy_pair_act<16>, dim3((dv.R * 16 + 255) / 256), dim3(256), 0, stream, pv, pv2, pw, dv.R,
                           dv.rep0, obs_in, act, logp, cmd);
        return launched();
      }
      const bool fastc = loop_delta4 && loop_fastc_ok();
      const auto k = fastc ? &fs::k_loop_policy_pair<true, true>
                           : loop_delta4 ? &fs::k_loop_policy_pair<true, false> : &fs::k_loop_policy_pair<false, false>;
      last_kernel = "k_loop_policy<Adversarial>";
      const int waves = (dv.R + 3) / 4;
      hipLaunchKernelGGL(k, dim3((waves + 3) / 4), dim3(256), 0, stream, dv, pv, pv2, pw, num_steps, reset_done, obs, act,
                         logp, rew, done);
      return launched();
    } else {
      return fail(FS_ERR_UNSUPPORTED, "fs_policy_pair: k_loop_policy_pair is a float32 kernel");
    }
  }

}  // namespace fsim
