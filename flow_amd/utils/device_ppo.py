"""DeviceLearner: the PPO update of examples/train_vec.py (``ppo_update``) on libflowsim's kernels.

What the torch path does between two rollouts -- a no_grad forward pass over the fragment, ``gae()`` (a Python loop of K
steps), then per epoch a forward pass, the clipped-surrogate loss and autograd's backward pass -- is here three entry
points of the library (include/flowsim.h ``fs_ppo_eval_dev``, ``fs_gae_dev``, ``fs_ppo_grad_dev``; kernels:
flow_amd/csrc/flowsim_learn.h).  The optimiser stays torch's: every parameter's ``.grad`` is a VIEW into the packed
gradient buffer the kernel writes, so ``allreduce_gradients`` and ``opt.step()`` work on it unchanged.
"""
import ctypes as C

from flow_amd import _lib as L

MAX_OBS, MAX_ACT, WIDTH = 160, 32, 32


def _check_trunk(who, hidden, head, n_out, what):
    if not 1 <= len(hidden) <= 3:
        raise NotImplementedError("DeviceLearner (fs_ppo_model): %s has %d hidden layers; 1..3 are built" % (who, len(hidden)))
    if any(l.out_features != WIDTH for l in hidden) or any(l.in_features != WIDTH for l in hidden[1:]):
        raise NotImplementedError("DeviceLearner (fs_ppo_model): %s has a hidden width other than 32 (%s)"
                                  % (who, [l.out_features for l in hidden]))
    if head.in_features != WIDTH or head.out_features != n_out:
        raise NotImplementedError("DeviceLearner (fs_ppo_model): %s maps %d units to %d outputs; %s"
                                  % (who, head.in_features, head.out_features, what))


class DeviceLearner(object):
    """``policy_hidden`` / ``value_hidden``: the ``nn.Linear`` layers of the two trunks (1..3 each, the same number, 32
    units, tanh between them); ``policy_head``: 32 -> A means (1 <= A <= 32) next to the free ``log_std`` [A];
    ``value_head``: 32 -> 1.  The observation has 1..160 values.  Anything else is refused here, by name, before the device
    is touched.  ``sim_or_vec``: a float32 ``FlowSim`` or ``VecFlowEnv`` -- it lends its device and its stream (the
    simulation state is never touched).  ``sync()`` repacks the current parameter values (after every optimiser step)."""

    def __init__(self, sim_or_vec, policy_hidden, policy_head, log_std, value_hidden, value_head):
        import torch
        self.torch = torch
        self.p_hidden, self.p_head, self.log_std_param = list(policy_hidden), policy_head, log_std
        self.v_hidden, self.v_head = list(value_hidden), value_head
        if log_std is None:
            raise NotImplementedError("DeviceLearner (fs_ppo_model): the 2A-output head (means and log stds from the "
                                      "network, no free log_std) is not built")
        A = int(log_std.numel())
        if not 1 <= A <= MAX_ACT:
            raise NotImplementedError("DeviceLearner (fs_ppo_model): act_dim A = %d; 1..32 are built" % A)
        if policy_head.out_features == 2 * A:
            raise NotImplementedError("DeviceLearner (fs_ppo_model): the 2A-output head (%d outputs for A = %d) is not "
                                      "built: the head gives the A means next to the free log_std" % (2 * A, A))
        _check_trunk("the policy network", self.p_hidden, policy_head, A, "the head gives the A = %d means" % A)
        _check_trunk("the value network", self.v_hidden, value_head, 1, "the value head has 1 output")
        if len(self.v_hidden) != len(self.p_hidden):
            raise NotImplementedError("DeviceLearner (fs_ppo_model): the two trunks have %d and %d hidden layers; the same "
                                      "number is built" % (len(self.p_hidden), len(self.v_hidden)))
        D = self.p_hidden[0].in_features
        if not 1 <= D <= MAX_OBS or self.v_hidden[0].in_features != D:
            raise NotImplementedError("DeviceLearner (fs_ppo_model): obs_dim D = %d (value network: %d); 1..160 are built"
                                      % (D, self.v_hidden[0].in_features))
        self.params = []
        for l in self.p_hidden + [policy_head]:
            self.params += [l.weight, l.bias]
        self.n_policy = sum(p.numel() for p in self.params)
        self.params.append(log_std)
        for l in self.v_hidden + [value_head]:
            self.params += [l.weight, l.bias]
        if any(p.dtype != torch.float32 for p in self.params):
            raise NotImplementedError("DeviceLearner (fs_ppo_model): float32 parameters only")
        # ---- the model class holds: the device
        dev = policy_head.weight.device
        if dev.type != "cuda" or any(p.device != dev for p in self.params):
            raise ValueError("DeviceLearner: every parameter must live on one GPU (got %s)" % dev)
        self.vec = sim_or_vec if hasattr(sim_or_vec, "sim") else None
        self.sim = sim_or_vec.sim if self.vec is not None else sim_or_vec
        if self.sim.precision != L.FS_F32:
            raise NotImplementedError("DeviceLearner: a float32 handle lends its stream (float64 / mixed learners are not built)")
        self.device, self.D, self.A, self.num_hidden = dev, D, A, len(self.p_hidden)
        self.P = sum(p.numel() for p in self.params)
        self.weights = torch.zeros(self.P, dtype=torch.float32, device=dev)      # [policy][log_std A][value]
        self.grad = torch.zeros(self.P, dtype=torch.float32, device=dev)         # the same layout
        self.loss = torch.zeros(2, dtype=torch.float32, device=dev)              # {sum pg, sum vf} of the last gradients()
        self._mean_std = torch.zeros(2, dtype=torch.float64, device=dev)
        self._work, self._bound_stream = None, None
        off = self.n_policy
        self.struct = L.fs_ppo_model(struct_size=C.sizeof(L.fs_ppo_model), obs_dim=D, act_dim=A, num_hidden=self.num_hidden,
                                     hidden_width=WIDTH, activation=0, policy_weights_dev=self.weights.data_ptr(),
                                     log_std_dev=self.weights.data_ptr() + 4 * off,
                                     value_weights_dev=self.weights.data_ptr() + 4 * (off + A))
        self.sync()

    def sync(self):
        torch = self.torch
        with torch.no_grad():
            self.weights.copy_(torch.cat([p.detach().reshape(-1) for p in self.params]))

    def attach_grads(self):
        """Every parameter's ``.grad`` becomes its view into the packed gradient buffer (no copies)."""
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.grad[off:off + n].view_as(p)
            off += n

    def _bind(self):
        """The launches go on torch's current stream, where the tensors they read and write are produced and used."""
        if self.vec is not None:
            self.vec.use_current_stream()
            return
        st = self.torch.cuda.current_stream(self.device).cuda_stream
        if st != self._bound_stream:
            self.sim.set_stream(st)
            self._bound_stream = st

    def _f32(self, t, shape, what):
        torch = self.torch
        if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != tuple(shape):
            raise ValueError("DeviceLearner: %s must be a float32 tensor of shape %s on %s" % (what, tuple(shape), self.device))
        return t.contiguous()

    def evaluate(self, obs, act=None):
        """``(logp [n], val [n])`` of ``obs [n, D]`` and ``act [n, A]``; ``act=None``: ``(None, val)``.  A NaN action row
        is an absent agent: its outputs mean nothing."""
        torch = self.torch
        n = int(obs.shape[0])
        obs = self._f32(obs, (n, self.D), "obs")
        act = None if act is None else self._f32(act, (n, self.A), "act")
        logp = torch.empty(n, dtype=torch.float32, device=self.device) if act is not None else None
        val = torch.empty(n, dtype=torch.float32, device=self.device)
        self._bind()
        L.check(self.sim.lib.fs_ppo_eval_dev(self.sim._h, C.byref(self.struct), n, obs.data_ptr(),
                                             act.data_ptr() if act is not None else None,
                                             logp.data_ptr() if logp is not None else None, val.data_ptr()), self.sim.lib)
        return logp, val

    def gae(self, rew, val, last_val, done, gamma=0.999, lam=0.97):
        """``(adv, ret) [K, R]``: train_vec.gae's recurrence, bit for bit what torch computes on the CPU.  ``done`` is the
        simulator's flag byte."""
        torch = self.torch
        K, R = int(rew.shape[0]), int(rew.shape[1])
        rew, val, last_val = self._f32(rew, (K, R), "rew"), self._f32(val, (K, R), "val"), self._f32(last_val, (R,), "last_val")
        if done.dtype == torch.bool:
            done = done.to(torch.uint8)
        if done.dtype != torch.uint8 or tuple(done.shape) != (K, R) or done.device != self.device:
            raise ValueError("DeviceLearner: done must be a uint8 tensor of shape %s on %s" % ((K, R), self.device))
        done = done.contiguous()
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        self._bind()
        L.check(self.sim.lib.fs_gae_dev(self.sim._h, K, R, rew.data_ptr(), val.data_ptr(), last_val.data_ptr(), done.data_ptr(),
                                        float(gamma), float(lam), adv.data_ptr(), ret.data_ptr()), self.sim.lib)
        return adv, ret

    def gradients(self, obs, act, logp_old, adv, ret, mean, std, clip=0.2, vf_coef=0.5, n_total=None, accumulate=False):
        """The gradient of ppo_update's loss over the n samples into ``self.grad`` (``.grad`` of the parameters after
        ``attach_grads()``), its two sums ``{sum pg, sum vf}`` into ``self.loss`` (returned).  ``adv`` is the RAW float64
        advantage; ``mean`` / ``std`` its float64 statistics (0-dim tensors or numbers); ``n_total`` the sample count of
        the whole update (all shards, all ranks).  ``accumulate=True`` adds to what both buffers hold."""
        torch = self.torch
        n = int(obs.shape[0])
        obs, act = self._f32(obs, (n, self.D), "obs"), self._f32(act, (n, self.A), "act")
        logp_old, ret = self._f32(logp_old, (n,), "logp_old"), self._f32(ret, (n,), "ret")
        if adv.dtype != torch.float64 or tuple(adv.shape) != (n,) or adv.device != self.device:
            raise ValueError("DeviceLearner: adv must be a float64 tensor of shape (%d,) on %s" % (n, self.device))
        adv = adv.contiguous()
        self._mean_std[0] = mean
        self._mean_std[1] = std
        need = int(self.sim.lib.fs_ppo_workspace(C.byref(self.struct), n))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=self.device)
        self._bind()
        L.check(self.sim.lib.fs_ppo_grad_dev(self.sim._h, C.byref(self.struct), n, obs.data_ptr(), act.data_ptr(),
                                             logp_old.data_ptr(), adv.data_ptr(), ret.data_ptr(), self._mean_std.data_ptr(),
                                             float(clip), float(vf_coef), 1.0 / float(n if n_total is None else n_total),
                                             int(bool(accumulate)), self.grad.data_ptr(), self.loss.data_ptr(),
                                             self._work.data_ptr(), self._work.numel()), self.sim.lib)
        return self.loss
