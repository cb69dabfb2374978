"""VecFlowEnv: R replicas of one Flow environment stepped together on one GPU.

The reference parallelises rollouts as one OS process + one SUMO process per
environment (examples/train.py:149; SubprocVecEnv, examples/train.py:102-103).
Here the R replicas are rows of [R, N] arrays in HBM advanced by one launch;
observations, rewards and done flags stay on the device as torch tensors so a
learner on the same GPU consumes them without a host copy.
"""
import os
from copy import deepcopy

from flow_amd import _lib as L


class VecFlowEnv(object):
    """Parameters: either ``flow_params`` (the reference's dict: env_name, network, env, sim, net,
    veh, initial; flow/utils/registry.py:29-46) or the four objects ``env_class, env_params,
    sim_params, network``.  ``device`` is the HIP ordinal of this process' GPU; ``replica_offset`` the global index
    of this process' first replica when a job is sharded over GPUs (noise streams follow global replica ids).
    ``track_aux=True`` keeps ``k.vehicle.get_previous_speed`` / ``get_accel`` of the wrapped env current (fields the
    specialised rollout kernels do not write: such a handle steps on the generic kernels).

    Attributes: ``num_envs`` environments; ``num_rows`` = ``num_envs * num_rings`` rows of the handle, the leading axis
    of every observation / reward / done / action / mask tensor (``num_rings`` is 1 except on MultiRingNetwork, where row
    ``env * num_rings + ring`` is one ring with its own agent: MultiWaveAttenuationPOEnv)."""

    def __init__(self, flow_params=None, num_replicas=4096, device=0, env_class=None, env_params=None,
                 sim_params=None, network=None, seed=None, replica_offset=0, track_aux=False):
        import torch
        self.torch = torch
        if flow_params is not None:
            from flow_amd.core.params import InitialConfig, TrafficLightParams
            env_class = flow_params["env_name"]
            env_params, sim_params = flow_params["env"], deepcopy(flow_params["sim"])
            network = flow_params["network"](
                name=flow_params["exp_tag"], vehicles=deepcopy(flow_params["veh"]), net_params=flow_params["net"],
                initial_config=flow_params.get("initial", InitialConfig()),
                traffic_lights=flow_params.get("tls", TrafficLightParams()))
        if seed is not None:
            sim_params = deepcopy(sim_params)
            sim_params.seed = seed
        self.num_envs = int(num_replicas)
        self.device = torch.device("cuda", int(device))
        env = env_class.__new__(env_class)
        env.num_replicas = self.num_envs
        env._device_index = int(device)
        env._replica_offset = int(replica_offset)     # global index of replica 0 (flow_amd.dist.shard_range)
        # per-vehicle previous speed / realised acceleration (k.vehicle.get_previous_speed / get_accel) are scalar-Env
        # accessors; keeping them costs the specialised rollout kernels (they do not write those fields)
        env._track_aux = bool(track_aux)
        env.__init__(env_params, sim_params, network)
        if env.FS_ENV is None or getattr(env, "HOST_HEADS", False):
            env.terminate()
            raise NotImplementedError("VecFlowEnv needs an env with an in-kernel observation/reward head")
        if getattr(env, "symmetric", False) or (env.FS_ENV in (L.FS_ENV_BOTTLENECK_DV, L.FS_ENV_BOTTLENECK)
                                                and env_params.evaluate):
            env.terminate()
            raise NotImplementedError("BottleneckDesiredVelocityEnv(symmetric=True) / evaluate=True gather their actions / "
                                      "reward on the host: scalar Env only")
        self.env = env
        self.sim = env.sim
        # MultiRingNetwork: an environment is `num_rings` rows of the handle (row = env * num_rings + ring), and every
        # tensor leads with ROWS; everything else has one row per environment
        self.num_rings = int(env._spec.get("num_rings", 1))
        self.num_rows = self.num_envs * self.num_rings
        self.k = env.k
        self.observation_space = env.observation_space
        self.action_space = env.action_space
        self.obs_dim, self.num_rl, self.act_dim = self.sim.obs_dim, self.sim.num_rl, self.sim.act_dim
        R = self.num_rows
        self._obs = torch.empty((R, self.obs_dim), dtype=torch.float32, device=self.device)
        self._rew = torch.empty((R,), dtype=torch.float32, device=self.device)
        self._done = torch.zeros((R,), dtype=torch.uint8, device=self.device)
        import numpy as np
        self._resample = env.env_params.additional_params.get('ring_length', None) is not None \
            and env.FS_ENV in (L.FS_ENV_WAVE_ATTENUATION, L.FS_ENV_WAVE_ATTENUATION_PO, L.FS_ENV_WAVE_ATTENUATION_PO_MA,
                               L.FS_ENV_USER)
        # BottleneckDesiredVelocityEnv(reset_inflow=True): a new total inflow per episode (_draw_inflow_totals)
        self._reset_inflow = env.FS_ENV == L.FS_ENV_BOTTLENECK_DV \
            and bool(env.env_params.additional_params.get("reset_inflow"))
        self._rng = np.random.default_rng(sim_params.seed)
        self._placement_cache = {}
        self.use_current_stream()

    def use_current_stream(self):
        """Enqueue the simulator's launches on torch's current stream (ordering with learner kernels).  Called by
        every reset / step / rollout, so a caller that switches streams (``with torch.cuda.stream(s):``) is followed:
        the launches, the temporaries they read and the caller's kernels are then all ordered on one stream."""
        st = self.torch.cuda.current_stream(self.device).cuda_stream
        if st != getattr(self, "_bound_stream", None):
            self.sim.set_stream(st)
            self._bound_stream = st

    def _check(self, t, shape, dtype):
        if t is None:
            return None
        if t.device != self.device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("expected a contiguous %s tensor of shape %s on %s" % (dtype, shape, self.device))
        return t

    def _resample_ring_lengths(self, mask_host):
        """WaveAttenuationEnv.reset (flow/envs/ring/wave_attenuation.py:157-210) for the replicas being reset:
        each draws its own ring length in ``ring_length`` and is re-placed with InitialConfig(bunching=50,
        min_gap=0).  Host-side (placement runs once per distinct length), then uploaded."""
        import numpy as np
        from flow_amd.core.kernel.network import NetworkKernel
        from flow_amd.core.params import InitialConfig, NetParams
        from flow_amd.envs.spec import check_placement, initial_positions
        lo, hi = self.env.env_params.additional_params['ring_length']
        idx = np.flatnonzero(mask_host)
        if idx.size == 0:
            return
        lengths = self.sim.get_state(L.FS_FIELD_RING_LENGTH).astype(np.float64)
        pending = self.sim.get_state(L.FS_FIELD_INIT_RING_LENGTH).astype(np.float64)
        init = self.sim.get_state(L.FS_FIELD_INIT_POS).astype(np.float64)
        self._draw_placements(idx, lengths, init)
        pending[idx] = lengths[idx]
        self.sim.set_state(L.FS_FIELD_RING_LENGTH, lengths)         # (sets the pending lengths of ALL replicas too ...)
        self.sim.set_state(L.FS_FIELD_INIT_RING_LENGTH, pending)    # ... so those of the replicas not reset go back
        self.sim.set_state(L.FS_FIELD_INIT_POS, init)

    def _draw_placements(self, idx, lengths, init):
        """random.randint(lo, hi) per replica in ``idx``; InitialConfig(bunching=50, min_gap=0) placement for the drawn
        length (once per distinct length), written into ``lengths`` / ``init``."""
        import numpy as np
        from flow_amd.core.kernel.network import NetworkKernel
        from flow_amd.core.params import InitialConfig, NetParams
        from flow_amd.envs.spec import check_placement, initial_positions
        lo, hi = self.env.env_params.additional_params['ring_length']
        draw = self._rng.integers(lo, hi + 1, idx.size)
        veh_len = np.array([v["length"] for v in self.env._spec["vehicles"]])
        ic = InitialConfig(bunching=50, min_gap=0)
        for length in np.unique(draw):
            if length not in self._placement_cache:
                add = dict(self.env.net_params.additional_params)
                add["length"] = int(length)
                net = self.env.network.__class__(self.env.network.orig_name, self.env.network.vehicles,
                                                 NetParams(additional_params=add), ic)
                nk = NetworkKernel(net, junction_length=self.k.network.junction_length)
                X, lanes = initial_positions(nk, ic, self.sim.N, 1)
                check_placement(X, veh_len, nk.length(), lanes)
                self._placement_cache[length] = X[0]
            sel = idx[draw == length]
            lengths[sel] = float(length)
            init[sel] = self._placement_cache[length][None, :]

    def redraw_ring_lengths(self):
        """Give EVERY replica a fresh pending ring length and start placement for its NEXT reset without touching the
        episode it is in (FS_FIELD_INIT_RING_LENGTH / FS_FIELD_INIT_POS): call between replays of a fragment captured
        with ``reset_done=True``, so that the resets inside the graph redraw the length per episode as
        WaveAttenuationEnv.reset does (flow/envs/ring/wave_attenuation.py:157-210).  Host-side draw + two uploads; the
        uploads synchronise the handle's stream."""
        import numpy as np
        if not self._resample:
            return
        lengths = self.sim.get_state(L.FS_FIELD_INIT_RING_LENGTH).astype(np.float64)
        init = self.sim.get_state(L.FS_FIELD_INIT_POS).astype(np.float64)
        self._draw_placements(np.arange(self.num_rows), lengths, init)
        self.sim.set_state(L.FS_FIELD_INIT_RING_LENGTH, lengths)
        self.sim.set_state(L.FS_FIELD_INIT_POS, init)

    # ---- per-replica inflow rates (open networks with scheduled inflows) ----------------------------------------
    def _base_inflow_rates(self):
        from flow_amd.envs.spec import inflow_base_rates
        return inflow_base_rates(self.env.net_params.inflows.get())

    def set_inflow_rates(self, vehs_per_hour, pending=False):
        """Give every replica its own demand.  ``vehs_per_hour``: ``[R]`` totals -- every inflow of the network keeps
        its share of the network's own total (``flow_amd.envs.spec.inflow_periods``) -- or ``[R, num_inflows]``, one
        rate per ``InFlows.add`` entry.  Written as periods to FS_FIELD_INFLOW_PERIOD: the running episodes step on with
        them (vehicle k of a flow is due at ``begin + k * period``, k the vehicles the replica has emitted so far, so a
        rate written mid-episode moves the next vehicle's due time) and later resets keep them.  ``pending=True``
        writes FS_FIELD_INIT_INFLOW_PERIOD instead: the running episodes are left alone and a replica takes its new rate
        at its next reset, inside a fragment with ``reset_done=True`` included.  Begin, end, number, vehicle types, lanes
        and speeds of the inflows stay the network's.  Uploads synchronise the handle's stream."""
        import numpy as np
        from flow_amd.envs.spec import inflow_periods
        base = self._base_inflow_rates()
        rates = np.asarray(vehs_per_hour, dtype=np.float64)
        R, nf = self.num_rows, len(base)
        if rates.shape == (R,):
            per = inflow_periods(rates, base)
        elif rates.shape == (R, nf):
            if not (np.all(np.isfinite(rates)) and np.all(rates > 0)):
                raise ValueError("VecFlowEnv.set_inflow_rates: rates must be finite and > 0")
            per = 3600.0 / rates
        else:
            raise ValueError("VecFlowEnv.set_inflow_rates: expected [R] = (%d,) totals or [R, num_inflows] = (%d, %d) "
                             "rates, got %s" % (R, R, nf, rates.shape))
        full = np.zeros((R, L.FS_MAX_INFLOWS))
        full[:, :nf] = per
        self.sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD if pending else L.FS_FIELD_INFLOW_PERIOD, full)

    def inflow_rates(self, pending=False):
        """veh/h ``[R, num_inflows]`` the replicas run on now (``pending``: will take at their next reset)."""
        nf = len(self.env._spec["inflows"])
        per = self.sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD if pending else L.FS_FIELD_INFLOW_PERIOD)
        return 3600.0 / per[:, :nf]

    def _draw_inflow_totals(self, n):
        """bottleneck.py:1003-1007: ``uniform(min(inflow_range), max(inflow_range)) * scaling`` per replica."""
        rng_ = self.env.env_params.additional_params["inflow_range"]
        return self._rng.uniform(min(rng_), max(rng_), n) * self.env.scaling

    def _resample_inflow_rates(self, mask_host):
        """BottleneckDesiredVelocityEnv.reset with ``reset_inflow`` (flow/envs/bottleneck.py:988-1085) for the replicas
        being reset: each draws its own total inflow, written as its pending rate -- the reset that follows makes it the
        current one.  Deviation from the reference: the network's inflows keep their order, types, lanes and speeds
        and their shares of the total; the reference rebuilds them as "followerstopper" 10 % / "human" 90 %
        (:1012-1024), the same split whenever the experiment has those shares (exp_configs/rl/singleagent/
        singleagent_bottleneck.py has)."""
        import numpy as np
        from flow_amd.envs.spec import inflow_periods
        idx = np.flatnonzero(mask_host)
        if idx.size == 0:
            return
        base = self._base_inflow_rates()
        pending = self.sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD)
        pending[idx, :len(base)] = inflow_periods(self._draw_inflow_totals(idx.size), base)
        self.sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, pending)

    def redraw_inflow_rates(self):
        """Give EVERY replica a fresh pending total inflow for its NEXT reset without touching the episode it is in
        (FS_FIELD_INIT_INFLOW_PERIOD): call between fragments that reset inside the launch or graph
        (``reset_done=True``), so that those resets redraw the demand per episode as BottleneckDesiredVelocityEnv.reset
        does with ``reset_inflow`` (flow/envs/bottleneck.py:988-1085).  The twin of ``redraw_ring_lengths``; a no-op
        unless the environment has ``reset_inflow`` set."""
        import numpy as np
        if not self._reset_inflow:
            return
        self._resample_inflow_rates(np.ones(self.num_rows, bool))

    def reset(self, mask=None):
        """Reset all replicas (or those where ``mask`` [R] uint8/bool tensor is set); returns obs [R, obs_dim].
        BottleneckDesiredVelocityEnv with ``reset_inflow``: exactly the replicas being reset draw a new total inflow
        first (_resample_inflow_rates; its docstring states how this differs from the reference's rebuilt network)."""
        self.use_current_stream()
        if mask is not None:
            mask = self._check(mask.to(self.torch.uint8), (self.num_rows,), self.torch.uint8)
        if self._resample or self._reset_inflow:
            import numpy as np
            mask_host = np.ones(self.num_rows, bool) if mask is None else mask.cpu().numpy() != 0
            if self._resample:
                self._resample_ring_lengths(mask_host)
            if self._reset_inflow:
                self._resample_inflow_rates(mask_host)
        self.sim.reset_dev(self._obs, mask)
        return self._obs

    def reset_done(self):
        """Reset exactly the replicas whose last ``done`` flag is set.  No host synchronisation, unless the
        environment redraws its network or demand per episode (WaveAttenuationEnv with ``ring_length``,
        BottleneckDesiredVelocityEnv with ``reset_inflow``): those two paths copy the done flags to the host, draw there
        and upload the pending values, so they synchronise the handle's stream with the host on EVERY call."""
        self.use_current_stream()
        if self._resample:
            self._resample_ring_lengths(self._done.cpu().numpy() != 0)
        if self._reset_inflow:
            self._resample_inflow_rates(self._done.cpu().numpy() != 0)
        self.sim.reset_dev(self._obs, self._done)
        return self._obs

    # ---- performance cliffs: say so, once -----------------------------------------------------------------------
    GENERIC_KERNELS = ("k_steps", "k_steps<CSET>", "k_steps_ml")

    def why_generic(self):
        """What sends this handle's rollouts to the generic step kernel (4-7x slower than the specialised rollout
        kernels of closed loops: flow_amd/csrc/flowsim_launch.h), as a list of the configuration fields responsible;
        empty for open networks (they have kernels of their own)."""
        sp = self.env._spec
        if sp.get("network") in ("merge", "bottleneck"):
            return []
        veh, why = sp["vehicles"], []
        CTRL_SIM, CTRL_RL, CTRL_IDM = 0, 1, 2                # (include/flowsim.h FS_CTRL_*)
        if any(v["controller"] not in (CTRL_IDM, CTRL_RL, CTRL_SIM) for v in veh):
            why.append("an acceleration controller other than IDMController / RLController / SimCarFollowingController")
        if any(v.get("fail_safe", 0) for v in veh):
            why.append("fail_safe")
        if len(veh) % 2 and not sp.get("segments"):
            why.append("an odd number of vehicles (the ring kernels hold two per lane)")
        if sp.get("sort_vehicles"):
            why.append("sort_vehicles=True")
        if sp.get("evaluate"):
            why.append("EnvParams(evaluate=True)")
        if sp.get("track_aux"):
            why.append("track_aux=True")
        if int(sp.get("num_lanes", 1)) > 1:
            why.append("a multi-lane ring (k_steps_ml)")
        if int(sp.get("sims_per_step", 1)) != 1:
            why.append("sims_per_step > 1")
        if sp.get("integrator", "euler") != "euler":
            why.append("use_ballistic=True")
        if sp.get("obs_perm") is not None:
            why.append("InitialConfig(shuffle=True) / a placement that is not in driving order")
        heads = [L.FS_ENV_ACCEL, L.FS_ENV_WAVE_ATTENUATION_PO, L.FS_ENV_ACCEL_PO_MA]
        if not sp.get("segments"):
            heads.append(L.FS_ENV_WAVE_ATTENUATION_PO_MA)
        if self.env.FS_ENV not in heads:
            why.append("the environment head of %s" % type(self.env).__name__)
        if os.environ.get("FLOWSIM_FORCE_GENERIC") == "1":
            why.append("FLOWSIM_FORCE_GENERIC=1")
        return why

    def _warn_if_generic(self):
        if getattr(self, "_warned_generic", False) or self.num_rows < 1024:
            return
        if self.sim.last_kernel in self.GENERIC_KERNELS:
            import warnings
            self._warned_generic = True
            why = self.why_generic()
            warnings.warn("VecFlowEnv: %d replicas step on the generic kernel %s (several times slower than the rollout "
                          "kernels of this network) because of: %s" %
                          (self.num_rows, self.sim.last_kernel, "; ".join(why) if why else "this configuration"),
                          stacklevel=3)

    def step(self, actions=None):
        """One Env.step of every replica.  ``actions``: float32 [R, action_dim] device tensor or None."""
        self.use_current_stream()
        a = self._check(actions, (self.num_rows, self.act_dim), self.torch.float32) if self.act_dim else None
        self.sim.step_dev(self._obs, self._rew, self._done, a)
        self._warn_if_generic()
        return self._obs, self._rew, self._done

    def rollout(self, num_steps, actions=None, obs_every_step=True, out=None):
        """``num_steps`` consecutive steps in one launch.  ``actions``: None, [R, num_rl] (held) or
        [K, R, num_rl] (one per step).  Returns (obs, rew, done) with a leading K axis when
        ``obs_every_step``."""
        torch, R, K = self.torch, self.num_rows, int(num_steps)
        self.use_current_stream()
        if out is None:
            lead = (K,) if obs_every_step else ()
            out = (torch.empty(lead + (R, self.obs_dim), dtype=torch.float32, device=self.device),
                   torch.empty(lead + (R,), dtype=torch.float32, device=self.device),
                   torch.empty(lead + (R,), dtype=torch.uint8, device=self.device))
        stride = 0
        if actions is not None and self.act_dim:
            if actions.dim() == 3:
                self._check(actions, (K, R, self.act_dim), torch.float32)
                stride = R * self.act_dim
            else:
                self._check(actions, (R, self.act_dim), torch.float32)
        else:
            actions = None
        self.sim.rollout_dev(K, out[0], out[1], out[2], actions, stride, obs_every_step)
        self._warn_if_generic()
        return out

    def capture(self, num_steps, policy=None, reset_done=False):
        """A closed-loop fragment of ``num_steps`` steps as ONE replayable HIP graph (StepGraph): per step the
        ``policy`` (a callable on the [R, obs_dim] observation tensor returning [R, action_dim] actions, e.g. a torch
        module) and one fs_step_dev launch, captured back to back on one stream.  What the reference's rollout workers
        do with one Python call + socket round trips per step (examples/train.py:110-212) costs one graph launch per
        fragment here; observations and actions never leave HBM.

        ``policy`` may be a ``flow_amd.utils.device_policy.DevicePolicy``: the graph then holds ONE policy kernel per
        step (``fs_policy_act_dev``: k_policy_act, k_policy_act_vec or k_policy_act_wide, whichever the handle takes)
        instead of a torch module's ten-odd, samples the actions from the policy's own Philox streams and keeps their
        log-probabilities in ``graph.logp``.  The graph reads the weights at ``policy.buf``'s fixed address: call
        ``policy.sync()`` between replays to hand it new ones.  A handle without an eager policy kernel raises
        NotImplementedError here.

        ``done`` is the simulator's flag byte (bit 0: horizon reached, bit 1: collision), not a 0/1 value."""
        if reset_done and self._resample:
            import warnings
            warnings.warn("VecFlowEnv.capture(reset_done=True): this environment redraws its ring length on reset "
                          "(WaveAttenuationEnv ring_length, flow/envs/ring/wave_attenuation.py:157-210); a reset inside "
                          "the captured graph re-places a replica on the length it drew at the last vec.reset() / "
                          "vec.reset_done() instead.  Call vec.redraw_ring_lengths() between replays to give every "
                          "replica a fresh pending length for its next in-graph reset.", stacklevel=2)
        if reset_done:
            self._warn_pending_inflow("capture")
        return StepGraph(self, num_steps, policy, reset_done)

    def _warn_pending_inflow(self, what):
        if not self._reset_inflow or getattr(self, "_warned_pending_inflow", False):
            return
        import warnings
        self._warned_pending_inflow = True
        warnings.warn("VecFlowEnv.%s(reset_done=True): this environment redraws its inflow on reset (reset_inflow, "
                      "flow/envs/bottleneck.py:988-1085); every reset inside ONE fragment takes the replica's pending "
                      "rate (FS_FIELD_INIT_INFLOW_PERIOD) -- call vec.redraw_inflow_rates() between fragments, and keep "
                      "fragments shorter than an episode if each episode must draw its own." % what, stacklevel=3)

    def policy_act(self, policy, obs=None, out=None):
        """ONE evaluation of ``policy`` (a ``DevicePolicy``) for every replica in one kernel launch
        (``fs_policy_act_dev``): actions sampled from the policy's Philox streams and their log-probabilities, for the
        observations ``obs [R, obs_dim]`` (default: those of the last reset / step).  Returns ``(act [R, A], logp [R])``
        on the action-vector heads (MergePOEnv, BottleneckDesiredVelocityEnv, AccelEnv with several RL vehicles on the
        figure eight -- flow_amd.benchmarks.figureeight1 / figureeight2 --: ``A = sim.policy_action_dim`` columns, one joint
        log-probability), ``(act [R, n], logp [R, n])`` for ``n = sim.policy_agents`` agents sharing the
        policy.  Every call advances the replicas' draw counters by one."""
        torch, R = self.torch, self.num_rows
        self.use_current_stream()
        A, n_ag = self.sim.policy_action_dim, self.sim.policy_agents
        if policy.act_dim != A:
            raise ValueError("VecFlowEnv.policy_act: the policy has act_dim = %d, this environment takes %d action "
                             "column(s) per evaluation (sim.policy_action_dim)" % (policy.act_dim, A))
        obs = self._obs if obs is None else self._check(obs, (R, self.obs_dim), torch.float32)
        lp_shape = (R,) if n_ag == 1 else (R, n_ag)
        if out is None:
            out = (torch.empty((R, max(A, n_ag)), dtype=torch.float32, device=self.device),
                   torch.empty(lp_shape, dtype=torch.float32, device=self.device))
        else:
            self._check(out[0], (R, max(A, n_ag)), torch.float32)
            self._check(out[1], lp_shape, torch.float32)
        self.sim.policy_act_dev(policy.struct, obs, out[0], out[1])
        return out

    def policy_rollout(self, policy, num_steps, reset_done=False, out=None):
        """``num_steps`` x (policy -> action -> Env.step [-> Env.reset of finished episodes]) in ONE kernel launch
        (``fs_policy_rollout_dev``; ``policy``: a ``flow_amd.utils.device_policy.DevicePolicy``).  Returns device tensors
        ``obs [K+1, R, obs_dim]`` (obs[0]: the state the fragment starts from), ``actions [K, R]``, ``logp [K, R]``,
        ``rew [K, R]``, ``done [K, R]`` (flag byte: bit 0 horizon, bit 1 collision).  Built for the reference's RL ring
        and figure-eight experiments: one RL vehicle (WaveAttenuationPOEnv; AccelEnv on the figure eight), or the
        multi-agent ring (MultiAgentWaveAttenuationPOEnv) and figure eight (MultiAgentAccelPOEnv), whose ``num_rl``
        agents share ``policy`` (its input: one agent's observation block, ``obs_dim / num_rl``): ``actions`` and
        ``logp`` are then ``[K, R, num_rl]`` (column c: agent c, the RL vehicle of rl_index c) and ``rew`` is the shared
        reward.  The multi-agent merge (MultiAgentMergePOEnv with its actions applied: a subclass with
        ``APPLY_ENUMERATE_QUIRK = False``) has the same layout with five values per agent; agent c is the RL slot of
        column c, and while that slot holds no vehicle the agent is absent: its action is NaN (no command), its
        log-probability 0.  The shipped merge environment never applies an action and is refused (roll it out open
        loop).  The single-agent merge (MergePOEnv, ``num_rl`` 1 to 32: k_merge_policy<PO> up to six places,
        k_merge_policy<PO,WIDE> beyond) takes ONE network with an action vector
        (``DevicePolicy(..., act_dim=num_rl)``: the whole observation in, ``num_rl`` accelerations out): ``actions`` is
        ``[K, R, num_rl]`` -- every column sampled every step, the environment ignores those beyond its list of controlled
        vehicles -- and ``logp [K, R]`` the joint log-probability; with ``reset_done`` a replica is reset when its
        ``done`` byte is not zero, collisions included.  AccelEnv on the figure eight with ``num_rl`` = 2..16 RL vehicles
        (flow_amd.benchmarks.figureeight1 / figureeight2: k_loop_policy<AccelVec>) takes the same kind of policy
        (``DevicePolicy(..., act_dim=num_rl)``: the 2 N observations in, ``num_rl`` accelerations out) with the same
        layouts, ``actions [K, R, num_rl]`` and ``logp [K, R]``; column c is the RL vehicle with rl_index c.  ``capture``
        serves every other environment / model."""
        torch, R, K = self.torch, self.num_rows, int(num_steps)
        self.use_current_stream()
        if reset_done and self._resample and not getattr(self, "_warned_pending_length", False):
            import warnings
            self._warned_pending_length = True
            warnings.warn("VecFlowEnv.policy_rollout(reset_done=True): this environment redraws its ring length on reset "
                          "(flow/envs/ring/wave_attenuation.py:157-210); every reset inside ONE fragment takes the replica's "
                          "pending length (FS_FIELD_INIT_RING_LENGTH) -- call vec.redraw_ring_lengths() between fragments, "
                          "and keep fragments shorter than an episode if each episode must draw its own.", stacklevel=2)
        if reset_done:
            self._warn_pending_inflow("policy_rollout")
        n_ag = self.sim.policy_agents
        per_agent = (K, R) if n_ag == 1 else (K, R, n_ag)
        a_dim = self.sim.policy_action_dim               # (MergePOEnv: one evaluation, num_rl columns, one log-probability)
        per_act = per_agent if a_dim == 1 else (K, R, a_dim)
        if out is None:
            out = (torch.empty((K + 1, R, self.obs_dim), dtype=torch.float32, device=self.device),
                   torch.empty(per_act, dtype=torch.float32, device=self.device),
                   torch.empty(per_agent, dtype=torch.float32, device=self.device),
                   torch.empty((K, R), dtype=torch.float32, device=self.device),
                   torch.empty((K, R), dtype=torch.uint8, device=self.device))
        self.sim.policy_rollout_dev(policy.struct, K, out[0], out[1], out[2], out[3], out[4], reset_done=reset_done)
        return out

    def population_act(self, population, obs=None, out=None):
        """``policy_act`` for a population of weight sets (``DevicePolicy.population(...)``; ``fs_population_act_dev``):
        replica ``r`` evaluates member ``r // group``.  Shapes, streams and counters are ``policy_act``'s."""
        torch, R = self.torch, self.num_rows
        self.use_current_stream()
        n_ag = self.sim.policy_agents
        obs = self._obs if obs is None else self._check(obs, (R, self.obs_dim), torch.float32)
        lp_shape = (R,) if n_ag == 1 else (R, n_ag)
        if out is None:
            out = (torch.empty((R, n_ag), dtype=torch.float32, device=self.device),
                   torch.empty(lp_shape, dtype=torch.float32, device=self.device))
        else:
            self._check(out[0], (R, n_ag), torch.float32)
            self._check(out[1], lp_shape, torch.float32)
        self.sim.population_act_dev(population.policy_struct(), population.struct, obs, out[0], out[1])
        return out

    def population_rollout(self, population, num_steps, reset_done=False, out=None):
        """``policy_rollout`` for a population of weight sets (``fs_population_rollout_dev``): ONE launch in which replica
        ``r`` runs member ``r // group``'s policy for the whole fragment.  Rows ``[m * group, (m + 1) * group)`` of every
        returned tensor equal, bit for bit, those of ``policy_rollout`` with member ``m``'s weights.  Built for the heads
        with one action column per evaluation (the rings, ``lord_of_the_rings``, the figure eights); the merges and the
        bottleneck raise NotImplementedError naming fs_population."""
        torch, R, K = self.torch, self.num_rows, int(num_steps)
        self.use_current_stream()
        n_ag = self.sim.policy_agents
        per_agent = (K, R) if n_ag == 1 else (K, R, n_ag)
        if out is None:
            out = (torch.empty((K + 1, R, self.obs_dim), dtype=torch.float32, device=self.device),
                   torch.empty(per_agent, dtype=torch.float32, device=self.device),
                   torch.empty(per_agent, dtype=torch.float32, device=self.device),
                   torch.empty((K, R), dtype=torch.float32, device=self.device),
                   torch.empty((K, R), dtype=torch.uint8, device=self.device))
        self.sim.population_rollout_dev(population.policy_struct(), population.struct, K, out[0], out[1], out[2], out[3], out[4],
                                        reset_done=reset_done)
        return out

    def _pair_weight(self, what, av, adversary, weight):
        for name, pol in (("av", av), ("adversary", adversary)):
            if pol.act_dim != 1:
                raise ValueError("VecFlowEnv.%s: the %s policy has act_dim = %d; each of the two policies emits the one "
                                 "action column of the RL vehicle" % (what, name, pol.act_dim))
        if weight is None:
            weight = self.env.env_params.additional_params.get('perturb_weight')
            if weight is None:
                raise ValueError("VecFlowEnv.%s: no weight given and env_params.additional_params has no 'perturb_weight' "
                                 "(AdversarialAccelEnv's: the vehicle receives av + perturb_weight * adversary)" % what)
        return float(weight)

    def policy_pair_act(self, av, adversary, weight=None, obs=None, out=None):
        """ONE evaluation of two policies (``DevicePolicy`` objects with ``act_dim == 1``) on the same observation, in one
        kernel launch (``fs_policy_pair_act_dev``, k_policy_pair_act): the reference's AdversarialAccelEnv, whose agents
        'av' and 'adversary' map to a policy each.  Returns ``(act [2, R], logp [2, R], cmd [R])``: plane 0 the av's
        sample, plane 1 the adversary's (its own Philox column, keyed by its own seed), and the command the vehicle
        receives, ``cmd = av + weight * adversary`` (one float32 fma) -- what ``step(cmd.unsqueeze(-1))`` takes.
        ``weight=None`` reads ``env_params.additional_params['perturb_weight']``.  Every call advances the replicas' draw
        counters by one."""
        torch, R = self.torch, self.num_rows
        self.use_current_stream()
        weight = self._pair_weight("policy_pair_act", av, adversary, weight)
        obs = self._obs if obs is None else self._check(obs, (R, self.obs_dim), torch.float32)
        if out is None:
            out = (torch.empty((2, R), dtype=torch.float32, device=self.device),
                   torch.empty((2, R), dtype=torch.float32, device=self.device),
                   torch.empty((R,), dtype=torch.float32, device=self.device))
        else:
            self._check(out[0], (2, R), torch.float32)
            self._check(out[1], (2, R), torch.float32)
            self._check(out[2], (R,), torch.float32)
        self.sim.policy_pair_act_dev(av.struct, adversary.struct, weight, obs, out[0], out[1], out[2])
        return out

    def policy_pair_rollout(self, av, adversary, num_steps, reset_done=False, weight=None, out=None):
        """``num_steps`` x (two policies -> ``av + weight * adversary`` -> Env.step [-> Env.reset of finished episodes])
        in ONE kernel launch (``fs_policy_pair_rollout_dev``, k_loop_policy<Adversarial>).  Returns device tensors
        ``(obs [K+1, R, obs_dim], act [2, K, R], logp [2, K, R], rew [K, R], done [K, R])``: ``act[0]`` / ``logp[0]`` are
        the av's, ``act[1]`` / ``logp[1]`` the adversary's (each a contiguous ``[K, R]`` tensor), ``rew`` is the av's
        reward and the adversary's is ``-rew``.  Built for AccelEnv with one RL vehicle on the figure eight
        (AdversarialAccelEnv); any other handle raises NotImplementedError naming fs_policy_pair.  The observation row is
        the kernel's AccelEnv order ``[v..., x...]``; the reference's adversarial state interleaves ``[v_i, x_i]`` -- a
        fixed permutation of the first layer's inputs."""
        torch, R, K = self.torch, self.num_rows, int(num_steps)
        self.use_current_stream()
        weight = self._pair_weight("policy_pair_rollout", av, adversary, weight)
        if out is None:
            out = (torch.empty((K + 1, R, self.obs_dim), dtype=torch.float32, device=self.device),
                   torch.empty((2, K, R), dtype=torch.float32, device=self.device),
                   torch.empty((2, K, R), dtype=torch.float32, device=self.device),
                   torch.empty((K, R), dtype=torch.float32, device=self.device),
                   torch.empty((K, R), dtype=torch.uint8, device=self.device))
        else:
            self._check(out[0], (K + 1, R, self.obs_dim), torch.float32)
            self._check(out[1], (2, K, R), torch.float32)
            self._check(out[2], (2, K, R), torch.float32)
            self._check(out[3], (K, R), torch.float32)
            self._check(out[4], (K, R), torch.uint8)
        self.sim.policy_pair_rollout_dev(av.struct, adversary.struct, weight, K, out[0], out[1], out[2], out[3], out[4],
                                         reset_done=reset_done)
        return out

    def episode_stats(self, rew, done, reset=False, accumulate=True):
        """RLlib's episode statistics of a fragment's ``rew`` / ``done`` ``[K, R]`` (what ``policy_rollout``,
        ``policy_pair_rollout``, ``rollout`` or a ``StepGraph`` return), in ONE kernel launch (``fs_episode_stats_dev``,
        k_episode_stats) without a host synchronisation: returns the float64 device tensor ``[8]`` =
        ``{episodes, sum ret, sum ret^2, min ret, max ret, sum len, min len, max len}`` (the env's buffer: the next call
        rewrites it), accumulated over the calls since the last ``reset=True``;
        ``flow_amd.utils.episode_stats.summarize`` turns it into RLlib's names.  The env owns the per-replica carries (the
        return and length of the episode a replica is in), so an episode that straddles fragments is counted once, in the
        fragment where it ends: feed the fragments in order.  ``reset=True`` zeroes the carries and the statistics first.
        ``accumulate=False``: the statistics are those of THIS fragment's episodes alone; the carries go on all the same.
        Any non-zero ``done`` byte ends an episode, the horizon and a collision alike.
        On the shared-reward multi-agent heads ``rew`` is the reward every agent shares: the return is that of the shared
        reward, one episode per replica.  In the two-policy experiment ``rew`` is the av's; the adversary's return is the
        negation (its mean is ``-mean``, its min ``-max``, its max ``-min``)."""
        torch, R = self.torch, self.num_rows
        K = int(rew.shape[0])
        self._check(rew, (K, R), torch.float32)
        self._check(done, (K, R), torch.uint8)
        self.use_current_stream()
        if getattr(self, "_ep_stats", None) is None:
            self._ep_ret = torch.zeros(R, dtype=torch.float64, device=self.device)
            self._ep_len = torch.zeros(R, dtype=torch.int32, device=self.device)
            self._ep_stats = torch.zeros(8, dtype=torch.float64, device=self.device)
            self._ep_empty = torch.tensor([0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, float("inf"), float("-inf")],
                                          dtype=torch.float64, device=self.device)
            reset = True
        if reset:
            self._ep_ret.zero_()
            self._ep_len.zero_()
            self._ep_stats.copy_(self._ep_empty)
        L.check(self.sim.lib.fs_episode_stats_dev(self.sim._h, K, rew.data_ptr(), done.data_ptr(), self._ep_ret.data_ptr(),
                                                  self._ep_len.data_ptr(), self._ep_stats.data_ptr(),
                                                  1 if accumulate else 0), self.sim.lib)
        return self._ep_stats

    # ---- snapshots: the state of the whole vectorised environment, handed out and taken back -----------------------
    _WARN_FLAGS = ("_warned_generic", "_warned_pending_inflow", "_warned_pending_length")

    def _host_part(self):
        host = {"rng": rng_state_to_plain(self._rng.bit_generator.state),
                "warned": {k: int(bool(getattr(self, k, False))) for k in self._WARN_FLAGS}}
        return host

    def snapshot(self, mask=None, out=None):
        """Everything the next step, reset or policy call of this environment depends on, as a ``VecSnapshot``: the
        simulator's device blob (``fs_snapshot_dev``: ONE kernel launch on the current stream, no host synchronisation),
        clones of the current observation and done flags, the episode-statistics carries, and the host part -- the state of
        the generator that draws ring lengths and inflows at resets and the one-time warning flags.  ``mask`` [R]: only
        those replicas' rows are written (into ``out``, a snapshot taken earlier from this environment, which is reused
        and returned; without ``out`` the other rows are zero).  ``restore`` puts it back: a restored replica reproduces
        its future exactly, the simulator's noise and the policy kernels' samples included."""
        torch = self.torch
        self.use_current_stream()
        if mask is not None:
            mask = self._check(mask.to(torch.uint8), (self.num_rows,), torch.uint8)
        info = self.sim.snapshot_info()
        if out is None:
            out = VecSnapshot(self, torch.zeros(int(info.bytes), dtype=torch.uint8, device=self.device),
                              torch.zeros_like(self._obs), torch.zeros_like(self._done), None, None)
        elif out.owner is not self or out.blob is None:
            raise ValueError("VecFlowEnv.snapshot: `out` must be a snapshot taken from this environment")
        self.sim.snapshot_dev(out.blob, mask)
        have_ep = getattr(self, "_ep_stats", None) is not None
        if have_ep and out.ep is None:
            out.ep = (torch.zeros_like(self._ep_ret), torch.zeros_like(self._ep_len), torch.zeros_like(self._ep_stats))
        if not have_ep:
            out.ep = None
        if mask is None:
            out.obs.copy_(self._obs)
            out.done.copy_(self._done)
            if have_ep:
                for dst, src in zip(out.ep, (self._ep_ret, self._ep_len, self._ep_stats)):
                    dst.copy_(src)
        else:
            m = mask != 0
            out.obs.copy_(torch.where(m[:, None], self._obs, out.obs))
            out.done.copy_(torch.where(m, self._done, out.done))
            if have_ep:
                out.ep[0].copy_(torch.where(m, self._ep_ret, out.ep[0]))
                out.ep[1].copy_(torch.where(m, self._ep_len, out.ep[1]))
                out.ep[2].copy_(self._ep_stats)
        out.host = self._host_part()
        return out

    def restore(self, snap, mask=None):
        """Put a ``VecSnapshot`` of THIS environment back (``fs_restore_dev``: one launch, no host synchronisation) and
        return the observation.  ``mask`` [R]: the device rows of those replicas only -- simulator state, observation, done
        flag, episode carries; the host generator, the accumulated episode statistics and the warning flags are left as
        they are, since they are not per replica (so resets after a masked restore draw new lengths / inflows, not the
        ones they drew the first time)."""
        torch = self.torch
        if snap.owner is not self or snap.blob is None:
            raise ValueError("VecFlowEnv.restore: the snapshot was not taken from this environment "
                             "(VecFlowEnv.load_snapshot takes a state_dict of any environment of equal layout)")
        self.use_current_stream()
        if mask is not None:
            mask = self._check(mask.to(torch.uint8), (self.num_rows,), torch.uint8)
        self.sim.restore_dev(snap.blob, mask)
        self._put_tensors(snap.obs, snap.done, snap.ep, mask)
        if mask is None:
            self._put_host(snap.host)
        return self._obs

    def _put_tensors(self, obs, done, ep, mask):
        torch = self.torch
        if ep is not None and getattr(self, "_ep_stats", None) is None:
            R = self.num_rows
            self._ep_ret = torch.zeros(R, dtype=torch.float64, device=self.device)
            self._ep_len = torch.zeros(R, dtype=torch.int32, device=self.device)
            self._ep_stats = torch.zeros(8, dtype=torch.float64, device=self.device)
            self._ep_empty = torch.tensor([0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, float("inf"), float("-inf")],
                                          dtype=torch.float64, device=self.device)
        if mask is None:
            self._obs.copy_(obs)
            self._done.copy_(done)
            if ep is not None:
                self._ep_ret.copy_(ep[0])
                self._ep_len.copy_(ep[1])
                self._ep_stats.copy_(ep[2])
            elif getattr(self, "_ep_stats", None) is not None:     # taken before the first episode_stats call
                self._ep_ret.zero_()
                self._ep_len.zero_()
                self._ep_stats.copy_(self._ep_empty)
            return
        m = mask != 0
        self._obs.copy_(torch.where(m[:, None], obs.to(self.device), self._obs))
        self._done.copy_(torch.where(m, done.to(self.device), self._done))
        if ep is not None:
            self._ep_ret.copy_(torch.where(m, ep[0].to(self.device), self._ep_ret))
            self._ep_len.copy_(torch.where(m, ep[1].to(self.device), self._ep_len))

    def _put_host(self, host):
        self._rng.bit_generator.state = rng_state_from_plain(host["rng"])
        for k in self._WARN_FLAGS:
            if host["warned"].get(k):
                setattr(self, k, True)
            elif hasattr(self, k):
                delattr(self, k)

    def load_snapshot(self, state):
        """Take the ``VecSnapshot.state_dict()`` of ANY environment of equal layout (another process, a checkpoint):
        ``fs_restore`` rebuilds the handle's host mirrors from the blob.  Raises ValueError naming the layout if the
        blob is of another shape.  Synchronises the handle's stream.  Returns the observation."""
        self.use_current_stream()
        info = self.sim.snapshot_info()
        if int(state["layout"]) != int(info.layout):
            raise ValueError("VecFlowEnv.load_snapshot: wrong layout: the snapshot is of %s, this environment is %s"
                             % (state.get("shape", "another handle"), self._shape_tag()))
        self.sim.restore(state["blob"], layout=int(state["layout"]))
        ep = state.get("ep")
        dev = self.device
        self._put_tensors(state["obs"].to(dev), state["done"].to(dev),
                          None if ep is None else tuple(ep[k].to(dev) for k in ("ret", "len", "stats")), None)
        self._put_host(state["host"])
        return self._obs

    def _shape_tag(self):
        return "%s: %d replicas x %d vehicles, obs_dim %d" % (type(self.env).__name__, self.num_rows, self.sim.N, self.obs_dim)

    # ---- host-side inspection
    def get_state(self, field):
        return self.sim.get_state(field)

    @property
    def positions(self):
        return self.sim.get_state(L.FS_FIELD_POS)

    @property
    def speeds(self):
        return self.sim.get_state(L.FS_FIELD_VEL)

    def vehicle_view(self, replica):
        """The k.vehicle accessor object looking at environment ``replica`` (all ``num_rings`` rows of it)."""
        self.k.vehicle.attach(self.sim, int(replica), rows=self.num_rings)
        return self.k.vehicle

    def close(self):
        self.env.terminate()

    terminate = close


def rng_state_to_plain(state):
    """``np.random.Generator.bit_generator.state`` (PCG64: two 128-bit integers) as strings and small ints, so that it
    survives ``torch.save`` -> ``torch.load(weights_only=True)``."""
    inner = state["state"]
    return {"bit_generator": str(state["bit_generator"]), "state": str(int(inner["state"])), "inc": str(int(inner["inc"])),
            "has_uint32": int(state["has_uint32"]), "uinteger": int(state["uinteger"])}


def rng_state_from_plain(plain):
    return {"bit_generator": plain["bit_generator"], "state": {"state": int(plain["state"]), "inc": int(plain["inc"])},
            "has_uint32": int(plain["has_uint32"]), "uinteger": int(plain["uinteger"])}


class VecSnapshot(object):
    """What ``VecFlowEnv.snapshot`` returns.  ``blob``: the simulator's device blob (uint8, ``fs_snapshot_dev``); ``obs`` /
    ``done``: clones of the environment's current observation and done flags; ``ep``: the episode-statistics carries
    ``(ret [R], len [R], stats [8])`` or None; ``host``: plain dict -- the generator's state (``rng_state_to_plain``) and
    the warning flags.  ``state_dict()`` is the form for checkpoints: plain tensors (CPU), ints and strings only, the
    simulator's part as the HOST blob of ``fs_snapshot``, which ``VecFlowEnv.load_snapshot`` of any environment of equal
    layout takes.  A snapshot made by hand for a checkpoint (``host_blob``: uint8 CPU tensor, ``layout``) needs no
    environment."""

    def __init__(self, owner, blob, obs, done, ep, host, host_blob=None, layout=None, shape=""):
        self.owner, self.blob, self.obs, self.done, self.ep, self.host = owner, blob, obs, done, ep, host
        self.host_blob, self.layout, self.shape = host_blob, layout, shape

    def state_dict(self):
        import torch
        host_blob, layout, shape = self.host_blob, self.layout, self.shape
        if host_blob is None:
            # the host ABI pair speaks of the handle's CURRENT state: put this snapshot in, take the host blob, put the
            # current state back (three launches and one synchronisation: a checkpoint's cost, not a step's)
            vec = self.owner
            vec.use_current_stream()
            now = torch.empty_like(self.blob)
            vec.sim.snapshot_dev(now)
            vec.sim.restore_dev(self.blob)
            host_blob = torch.frombuffer(bytearray(vec.sim.snapshot()), dtype=torch.uint8)
            vec.sim.restore_dev(now)
            layout, shape = int(vec.sim.snapshot_info().layout), vec._shape_tag()
        out = {"version": 1, "layout": int(layout), "shape": str(shape), "blob": host_blob,
               "obs": self.obs.detach().cpu(), "done": self.done.detach().cpu(),
               "host": {"rng": dict(self.host["rng"]), "warned": {k: int(v) for k, v in self.host["warned"].items()}}}
        if self.ep is not None:
            out["ep"] = {k: t.detach().cpu() for k, t in zip(("ret", "len", "stats"), self.ep)}
        return out


class StepGraph(object):
    """``vec.capture(K, policy)``: K x (policy -> actions -> Env.step of every replica) recorded once with HIP stream
    capture (``torch.cuda.CUDAGraph``; libflowsim's launches go to the capturing stream) and replayed per fragment.

    Buffers (device, owned by the graph): ``obs [K+1, R, obs_dim]`` (``obs[0]`` = observation before the first step:
    what ``begin`` set, then the last observation of the previous replay), ``actions [K, R, action_dim]``, ``rew [K, R]``,
    ``done [K, R]`` uint8.  With ``reset_done`` every replica whose episode ended is reset inside the graph
    (masked fs_reset_dev) and ``obs[k+1]`` holds the first observation of its next episode, as a vectorised
    Gym / RLlib VectorEnv does.  The policy must be capturable (no host synchronisation, static shapes).
    Building the graph runs up to two eager warm-up steps: call ``vec.reset()`` and ``begin(obs)`` afterwards.

    ``policy`` a ``DevicePolicy``: per step ONE ``fs_policy_act_dev`` launch writes ``actions[k]`` and ``logp[k]``
    (``logp [K, R]``; ``[K, R, num_rl]`` where ``num_rl`` agents share the policy).  The warm-up steps then advance the
    policy's draw counters too (two draws per replica), as they advance the simulator; the weights are read at
    ``policy.buf``'s address on every replay (``policy.sync()`` hands the graph new ones)."""

    def __init__(self, vec, num_steps, policy=None, reset_done=False):
        torch = vec.torch
        self.vec, self.K, self.policy, self.reset_done = vec, int(num_steps), policy, bool(reset_done)
        R, K = getattr(vec, "num_rows", vec.num_envs), self.K      # (rows; a stand-in without rings has num_envs)
        dev = vec.device
        self.obs = torch.zeros((K + 1, R, vec.obs_dim), dtype=torch.float32, device=dev)
        self.rew = torch.zeros((K, R), dtype=torch.float32, device=dev)
        self.done = torch.zeros((K, R), dtype=torch.uint8, device=dev)
        self.actions = torch.zeros((K, R, max(vec.act_dim, 1)), dtype=torch.float32, device=dev)
        self._carry = torch.zeros((R, vec.obs_dim), dtype=torch.float32, device=dev)
        from flow_amd.utils.device_policy import DevicePolicy
        self._device_policy = isinstance(policy, DevicePolicy)
        self.logp = None
        if self._device_policy:
            n_ag = vec.sim.policy_agents
            if not vec.act_dim or policy.act_dim != vec.sim.policy_action_dim:
                raise ValueError("VecFlowEnv.capture: the policy has act_dim = %d, this environment takes %d action "
                                 "column(s) per evaluation (sim.policy_action_dim)"
                                 % (policy.act_dim, vec.sim.policy_action_dim if vec.act_dim else 0))
            self.logp = torch.zeros((K, R) if n_ag == 1 else (K, R, n_ag), dtype=torch.float32, device=dev)
        self.stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(self.stream):
            vec.use_current_stream()                 # bind BEFORE the capture: fs_set_stream synchronises
            self.obs[0].copy_(vec._obs)
            self._body(2 if K > 1 else 1)            # eager warm-up: lazy host work (divisor proofs, allocator) happens here
            vec.sim.sync()
            self.obs[0].copy_(vec._obs)
        self.stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.obs[0].copy_(self._carry)
            self._body(K)
            self._carry.copy_(self.obs[K])
        # NOTE: the eager warm-up advanced the simulator by up to two steps: vec.reset() + begin(obs) start a rollout

    def _body(self, steps):
        vec, sim = self.vec, self.vec.sim
        for k in range(steps):
            a = None
            if vec.act_dim:
                if self._device_policy:
                    sim.policy_act_dev(self.policy.struct, self.obs[k], self.actions[k], self.logp[k])
                elif self.policy is not None:
                    self.actions[k].copy_(self.policy(self.obs[k]))
                a = self.actions[k]
            sim.step_dev(self.obs[k + 1], self.rew[k], self.done[k], a)
            if self.reset_done:
                sim.reset_dev(self.obs[k + 1], self.done[k])

    def _after_caller(self):
        # the graph's stream is non-blocking: what the caller enqueued on ITS stream so far (vec.reset()'s kernels, the
        # optimiser step that rewrote the policy weights) must have finished before anything here reads it
        self.stream.wait_stream(self.vec.torch.cuda.current_stream(self.vec.device))

    def begin(self, obs0):
        """Set the observation the first step's policy call sees (after ``vec.reset()``)."""
        self._after_caller()
        with self.vec.torch.cuda.stream(self.stream):
            self._carry.copy_(obs0)

    def carry(self):
        """A clone of the observation the next replay's first policy call will see (what ``begin`` set, then the last
        observation of each replay): part of the state of a run that is to be resumed exactly."""
        self._after_caller()
        with self.vec.torch.cuda.stream(self.stream):
            out = self._carry.clone()
        self.vec.torch.cuda.current_stream(self.vec.device).wait_stream(self.stream)
        return out

    def set_carry(self, obs):
        """``begin`` under the name that pairs with ``carry``: a restored run replays from the observation the interrupted
        one would have used."""
        self.begin(obs.to(self.vec.device))

    def replay(self):
        """One fragment: returns (obs [K+1,R,D], actions [K,R,A], rew [K,R], done [K,R]) views, valid until the next
        replay.  Ordered on both sides: the replay starts after the work the caller's current stream holds so far, and
        the caller's current stream waits for the fragment before it runs anything enqueued after this call (no host
        synchronisation either way).  ``done`` is a flag byte (bit 0 horizon, bit 1 collision)."""
        self._after_caller()
        with self.vec.torch.cuda.stream(self.stream):      # CUDAGraph.replay() goes to torch's CURRENT stream
            self.graph.replay()
        self.vec.torch.cuda.current_stream(self.vec.device).wait_stream(self.stream)
        return self.obs, self.actions, self.rew, self.done

    def synchronize(self):
        self.stream.synchronize()
