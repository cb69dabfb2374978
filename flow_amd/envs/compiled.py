"""A user-defined environment whose observation and reward run in the step kernel.

The reference's main extension point is a Python subclass of ``Env`` that writes ``get_state``, ``compute_reward`` and
``_apply_rl_actions`` (flow/envs/base.py).  Here the step loop is a HIP kernel, so a user environment's head is device
code: ``CompiledEnv`` carries it as C++ statement bodies, ``flow_amd.build.build_user`` compiles them into a copy of
libflowsim.so (cached under flow_amd/_user/) and the environment's handle steps on that copy (head FS_ENV_USER, always on
k_steps).  Such an environment is a first-class citizen of ``VecFlowEnv``: thousands of replicas, ``rollout``,
``capture``, ``DevicePolicy``, snapshots, episode statistics.

    class HighwayStyleEnv(CompiledEnv):
        OBSERVE = "rl"             # "rl": one block per RL vehicle at column rl_index, obs_dim = OBS_PER_VEHICLE * num_rl
                                   # "all": AccelEnv's layout, obs[k * N + i], obs_dim = OBS_PER_VEHICLE * N
        OBS_PER_VEHICLE = 5        # 1..8
        OBS_SOURCE = '''           // per vehicle; writes o[0 .. OBS_PER_VEHICLE-1]
            o[0] = v / max_speed;            o[1] = (v_lead - v) / max_speed;   o[2] = h / L;
            o[3] = (v - v_follow) / max_speed;  o[4] = h_follow / L;
        '''
        REWARD_TERMS = 2           # 0..4
        TERM_SOURCE = '''          // per vehicle; writes t[0 .. REWARD_TERMS-1]; each is summed over the replica's vehicles
            const T dv = v - target_velocity;   t[0] = dv * dv;
            t[1] = (is_rl && v > T(0)) ? tmin((tmax(h / v, T(0)) - T(1)) / T(1), T(0)) : T(0);
        '''
        REWARD_SOURCE = '''        // per replica; ends in a return
            if (fail) return T(0);
            const T cost1 = tmax(p[0] - tsqrt(sum[0]), T(0)) / p[0];
            return tmax(cost1 + T(0.1) * sum[1], T(0));
        '''
        def __init__(self, env_params, sim_params, network, simulator='traci'):
            CompiledEnv.__init__(self, env_params, sim_params, network, simulator, params=[max_cost])   # p[0..7]

Names in scope of ``OBS_SOURCE`` and ``TERM_SOURCE`` (per vehicle): ``v``, ``v_lead``, ``h`` (bumper to bumper; 1000
without a leader), ``has_lead``, ``v_follow``, ``h_follow``, ``length``; ``x`` (Flow's coordinate: the table coordinate on
the figure eight, else the ring position); ``L`` (the length the built-in heads divide positions by); ``is_rl``,
``rl_index``; ``action`` (this vehicle's command of the step just taken, clipped the way ``clip_actions`` says; ``T(0)``
for a non-RL vehicle or without actions) and ``has_action``; ``max_speed``, ``target_velocity``, ``dt``, ``N``, ``num_rl``
(the last two as ``T``), ``p[0..7]``; helpers ``tmin``, ``tmax``, ``tabs``, ``tsqrt``.
Names in scope of ``REWARD_SOURCE`` (per replica): ``sum[0..REWARD_TERMS-1]``, ``fail`` (a collision in this step, or a
speed below -100: the built-in heads' condition), ``has_action``, ``N``, ``num_rl``, ``max_speed``, ``target_velocity``,
``dt``, ``p[]``.  ``T`` is ``float`` or ``double`` (the handle's precision); observations are stored as ``float(o[k])``.

The contract (include/flowsim.h FS_ENV_USER; tests/test_compiled_env_gpu.py pins it):

* each ``sum[m]`` is the sum of ``t[m]`` over the replica's vehicles in the built-in heads' tree order
  (``oracle.rewards.tree_sum``);
* the vehicle index ``i`` of the ``"all"`` layout is the one AccelEnv uses without ``sort_vehicles`` (the vehicle's place
  in ``k.vehicle.get_ids()``);
* with ``"rl"`` only an RL vehicle writes, at ``OBS_PER_VEHICLE * rl_index``;
* actions are applied exactly as AccelEnv applies them (accelerations, RL vehicles in ``rl_index`` order), and
  ``action_space`` is AccelEnv's;
* ``done`` is the simulator's flag (horizon, collision);
* ``compute_reward`` and ``get_state`` return what the kernel wrote.

Refused at construction, by name: open networks, ``MultiRingNetwork``, multi-lane rings, ``sort_vehicles``, more than 64
vehicles, precisions other than f32 / f64, ``OBS_PER_VEHICLE`` / ``REWARD_TERMS`` / ``len(params)`` out of range, an empty
source.  A body that does not compile (``REWARD_TERMS = 0`` with ``sum`` used, say) raises with hipcc's message."""
import numpy as np

from flow_amd import _lib as L
from flow_amd.envs.base import Env
from flow_amd.utils.spaces import Box


class CompiledEnv(Env):
    FS_ENV = L.FS_ENV_USER
    OBSERVE = "rl"
    OBS_PER_VEHICLE = None
    OBS_SOURCE = None
    REWARD_TERMS = 0
    TERM_SOURCE = None
    REWARD_SOURCE = None

    def __init__(self, env_params, sim_params, network=None, simulator='traci', scenario=None, params=()):
        net = scenario if scenario is not None else network
        self._user_env = self.check_head(type(self), params)
        self.check_configuration(type(self).__name__, env_params, sim_params, net)
        for p in ('max_accel', 'max_decel'):
            if p not in env_params.additional_params:
                raise KeyError('Environment parameter \'{}\' not supplied'.format(p))
        Env.__init__(self, env_params, sim_params, network, simulator, scenario)

    # ------------------------------------------------------------------ checks (all before anything is compiled or created)
    @staticmethod
    def check_head(cls, params=()):
        """The head of ``cls`` as the dict flow_amd.build.user_env_header takes, plus ``params``; ValueError naming what
        is out of range."""
        name = cls.__name__
        if cls.OBSERVE not in ("rl", "all"):
            raise ValueError("%s: OBSERVE must be \"rl\" or \"all\", got %r" % (name, cls.OBSERVE))
        k = cls.OBS_PER_VEHICLE
        if not isinstance(k, int) or not 1 <= k <= 8:
            raise ValueError("%s: OBS_PER_VEHICLE must be 1..8, got %r" % (name, k))
        terms = cls.REWARD_TERMS
        if not isinstance(terms, int) or not 0 <= terms <= 4:
            raise ValueError("%s: REWARD_TERMS must be 0..4, got %r" % (name, terms))
        params = [float(x) for x in params]
        if len(params) > L.FS_MAX_USER_ENV_PARAMS:
            raise ValueError("%s: params holds %d values; a compiled environment takes at most 8 (p[0..7])"
                             % (name, len(params)))
        for attr in ("OBS_SOURCE", "REWARD_SOURCE") + (("TERM_SOURCE",) if terms else ()):
            text = getattr(cls, attr)
            if not text or not str(text).strip():
                raise ValueError("%s: %s is empty (the C++ body of the head)" % (name, attr))
        return dict(obs=str(cls.OBS_SOURCE), terms=str(cls.TERM_SOURCE or ""), reward=str(cls.REWARD_SOURCE),
                    obs_per_vehicle=k, rl_only=cls.OBSERVE == "rl", reward_terms=terms, params=params)

    @staticmethod
    def check_configuration(name, env_params, sim_params, network):
        """NotImplementedError naming what a user head is not built for."""
        from flow_amd.networks.multi_ring import MultiRingNetwork
        if network.specify_open_routes() is not None:
            raise NotImplementedError("%s: a CompiledEnv on open networks (%s) is not built: single-lane rings and the "
                                      "figure eight are" % (name, type(network).__name__))
        if isinstance(network, MultiRingNetwork):
            raise NotImplementedError("%s: a CompiledEnv on MultiRingNetwork is not built" % name)
        if int(network.net_params.additional_params.get("lanes", 1)) != 1:
            raise NotImplementedError("%s: a CompiledEnv on multi-lane rings is not built (lanes = %s)"
                                      % (name, network.net_params.additional_params.get("lanes")))
        if env_params.additional_params.get("sort_vehicles", False):
            raise NotImplementedError("%s: a CompiledEnv with sort_vehicles is not built" % name)
        if network.vehicles.num_vehicles > 64:
            raise NotImplementedError("%s: a CompiledEnv with more than 64 vehicles is not built (%d)"
                                      % (name, network.vehicles.num_vehicles))
        if env_params.additional_params.get("ring_length") is not None and \
                type(network).__name__ != "RingNetwork":
            raise NotImplementedError("%s: additional_params['ring_length'] (a ring length per episode) needs a RingNetwork"
                                      % name)
        prec = getattr(sim_params, "precision", "f32")
        if prec not in ("f32", "f64", "float32", "float64", np.float32, np.float64):
            raise NotImplementedError("%s: a CompiledEnv is built for the precisions f32 and f64, not %r" % (name, prec))

    @classmethod
    def head_obs_dim(cls, num_vehicles, num_rl):
        """fs_obs_dim of this head: OBS_PER_VEHICLE per RL vehicle ("rl") or per vehicle ("all")."""
        return int(cls.OBS_PER_VEHICLE) * int(num_rl if cls.OBSERVE == "rl" else num_vehicles)

    def fs_user_env(self):
        """What build_spec adds to the spec: the head (``user_env_source``) and its parameters (``user_env_p``)."""
        head = dict(self._user_env)
        return dict(user_env_source=head, user_env_p=head.pop("params"))

    # ------------------------------------------------------------------ the Env hooks
    @property
    def action_space(self):
        return Box(low=-abs(self.env_params.additional_params['max_decel']),
                   high=self.env_params.additional_params['max_accel'],
                   shape=(self.initial_vehicles.num_rl_vehicles, ), dtype=np.float32)

    @property
    def observation_space(self):
        n = self.head_obs_dim(self.initial_vehicles.num_vehicles, self.initial_vehicles.num_rl_vehicles)
        return Box(low=-float("inf"), high=float("inf"), shape=(n, ), dtype=np.float32)

    def _apply_rl_actions(self, rl_actions):
        self.k.vehicle.apply_acceleration(self._rl_action_order(), rl_actions)

    def reset(self):
        """``additional_params['ring_length'] = [lo, hi]`` (a ring): draw a ring length and re-place the vehicles as
        WaveAttenuationEnv.reset does (flow/envs/ring/wave_attenuation.py:157-210), then the generic reset."""
        bounds = self.env_params.additional_params.get('ring_length')
        if bounds is None:
            return super().reset()
        import random
        from flow_amd.envs.base import redraw_ring
        self.step_counter = 0
        length = random.randint(bounds[0], bounds[1])
        X = redraw_ring(self, length)
        self.sim.set_state(L.FS_FIELD_RING_LENGTH, np.full(1, float(length)))
        self.sim.set_state(L.FS_FIELD_INIT_POS, X)
        for i, veh_id in enumerate(self.initial_ids):
            edge, pos = self.k.network.get_edge(float(X[0, i]))
            self.initial_state[veh_id] = (self.k.vehicle.get_type(veh_id), edge, 0, pos,
                                          self.k.vehicle.get_initial_speed(veh_id))
        return super().reset()

    def compute_reward(self, rl_actions, **kwargs):
        """Computed in the step kernel (REWARD_SOURCE over the sums of TERM_SOURCE)."""
        return self._last_reward

    def get_state(self):
        """Computed in the step kernel (OBS_SOURCE)."""
        return np.array(self._last_obs, dtype=np.float64)
