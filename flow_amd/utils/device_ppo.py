"""DeviceLearner: the PPO update of examples/train_vec.py (``ppo_update``) on libflowsim's kernels.

What the torch path does between two rollouts -- a no_grad forward pass over the fragment, ``gae()`` (a Python loop of K
steps), then per epoch a forward pass, the clipped-surrogate loss and autograd's backward pass -- is here three entry
points of the library (include/flowsim.h ``fs_ppo_eval_dev``, ``fs_gae_dev``, ``fs_ppo_grad_dev``; kernels:
flow_amd/csrc/flowsim_learn.h).  The optimiser stays torch's: every parameter's ``.grad`` is a VIEW into the packed
gradient buffer the kernel writes, so ``allreduce_gradients`` and ``opt.step()`` work on it unchanged.

``update()`` is the whole of ``ppo_update`` on the learner's stream: the float64 advantage statistics
(``fs_adv_stats_dev``, ``fs_adv_finish_dev``), the gradient with its sample count read on the device
(``fs_ppo_grad_n_dev``) and Adam on the packed buffers (``fs_adam_dev``) join the three kernels above, so nothing between
two rollouts needs the host: a fixed sequence of launches that can be captured into a graph.  After
``adopt_parameters()`` the module's parameters ARE views into the packed weights, the counterpart of ``attach_grads()``.

The loss the reference trains with (RLlib's PPO: KL penalty with an adaptive coefficient, clipped value loss, entropy
bonus) is three more entry points -- ``evaluate_dist`` (``fs_ppo_eval_dist_dev``), ``gradients_loss``
(``fs_ppo_grad_loss_dev``), ``kl_adapt`` (``fs_kl_adapt_dev``) -- and keywords of ``update()``; every term is off by default.
"""
import ctypes as C

from flow_amd import _lib as L

MAX_OBS, MAX_ACT, WIDTH = 160, 32, 32


def _fmix32(h):
    """murmur3's finaliser on uint32 arrays (wrapping arithmetic)."""
    import numpy as np
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85ebca6b)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xc2b2ae35)
    return h ^ (h >> np.uint32(16))


def epoch_permutation(seed, epoch, n):
    """The permutation of ``[0, n)`` that epoch ``epoch`` of a minibatch update with ``shuffle_seed=seed`` walks through
    (int64 [n]): minibatch ``k`` of size ``B`` is rows ``perm[k B : (k + 1) B]``.  A numpy restatement of ``perm_at`` in
    flow_amd/csrc/flowsim_learn.h -- a 4-round balanced Feistel network on the smallest even number of bits that holds
    ``n - 1``, round function fmix32(right half + key), keys from fmix32 of (seed, epoch, round), cycle-walked until the
    value is below ``n`` -- with the values of the kernel (k_ppo_minibatch) and of ``fs_ppo_perm_host``.  No GPU, no
    library."""
    import numpy as np
    n, seed, epoch = int(n), int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError("epoch_permutation: n must be 1 .. 2^31 - 1")
    u = np.uint32
    with np.errstate(over="ignore"):
        bits = (n - 1).bit_length()
        half = 1 if bits < 2 else (bits + 1) // 2
        mask = u((1 << half) - 1)
        b = _fmix32(u(seed & 0xffffffff) + u(0x9e3779b9))
        b = _fmix32(b ^ u(seed >> 32))
        b = _fmix32(b + u(epoch & 0xffffffff))
        b = _fmix32(b ^ u(epoch >> 32))
        keys = [_fmix32(b + u(0x9e3779b9) * u(r + 1)) for r in range(4)]
        x = np.arange(n, dtype=np.uint32)
        todo = np.ones(n, dtype=bool)
        while todo.any():
            l, r = x[todo] >> u(half), x[todo] & mask
            for key in keys:
                l, r = r, l ^ (_fmix32(r + key) & mask)
            x[todo] = (l << u(half)) | r
            todo[todo] = x[todo] >= u(n)
    return x.astype(np.int64)


def _check_trunk(who, hidden, head, n_out, what):
    if not 1 <= len(hidden) <= 3:
        raise NotImplementedError("DeviceLearner (fs_ppo_model): %s has %d hidden layers; 1..3 are built" % (who, len(hidden)))
    if any(l.out_features != WIDTH for l in hidden) or any(l.in_features != WIDTH for l in hidden[1:]):
        raise NotImplementedError("DeviceLearner (fs_ppo_model): %s has a hidden width other than 32 (%s)"
                                  % (who, [l.out_features for l in hidden]))
    if head.in_features != WIDTH or head.out_features != n_out:
        raise NotImplementedError("DeviceLearner (fs_ppo_model): %s maps %d units to %d outputs; %s"
                                  % (who, head.in_features, head.out_features, what))


DESCRIPTOR_NAMES = ("obs_dim D", "act_dim A", "num_hidden", "net_log_std")


def check_descriptor(who, theirs, mine):
    """A checkpoint's model ``(D, A, num_hidden, net_log_std)`` against the one it is loaded into: a mismatch is refused,
    naming the field."""
    theirs, mine = list(theirs), list(mine)
    for name, a, b in zip(DESCRIPTOR_NAMES, theirs, mine):
        if a != b:
            raise ValueError("%s: the checkpoint's model has %s = %s, this one %s = %s (checkpoint (D, A, num_hidden, "
                             "net_log_std) = %s, here %s)" % (who, name, a, name, b, tuple(theirs), tuple(mine)))


class DeviceLearner(object):
    """``policy_hidden`` / ``value_hidden``: the ``nn.Linear`` layers of the two trunks (1..3 each, the same number, 32
    units, tanh between them); ``policy_head``: 32 -> A means (1 <= A <= 32) next to the free ``log_std`` [A] -- or, with
    the keyword ``net_log_std=True`` and ``log_std=None``, 32 -> 2 A outputs, the A means and then the A log stds (RLlib's
    ``free_log_std: false``; every method but ``gradients()``, the host-n form, takes it);
    ``value_head``: 32 -> 1.  The observation has 1..160 values.  Anything else is refused here, by name, before the device
    is touched.  ``sim_or_vec``: a float32 ``FlowSim`` or ``VecFlowEnv`` -- it lends its device and its stream (the
    simulation state is never touched).  ``sync()`` repacks the current parameter values (after every optimiser step)."""

    def __init__(self, sim_or_vec, policy_hidden, policy_head, log_std, value_hidden, value_head, net_log_std=False):
        import torch
        self.torch = torch
        self.p_hidden, self.p_head, self.log_std_param = list(policy_hidden), policy_head, log_std
        self.v_hidden, self.v_head = list(value_hidden), value_head
        self.net_log_std = bool(net_log_std)
        if self.net_log_std:
            # the head of 2 A outputs (RLlib's free_log_std: false): rows 0 .. A-1 the means, rows A .. 2A-1 the log stds
            if log_std is not None:
                raise NotImplementedError("DeviceLearner (fs_ppo_model): net_log_std=True is the 2A-output head, whose log "
                                          "stds come from the network: log_std must be None (got %d values)" % log_std.numel())
            if policy_head.out_features % 2:
                raise NotImplementedError("DeviceLearner (fs_ppo_model): net_log_std=True needs a head of 2 A outputs, the "
                                          "means and then the log stds; %d outputs is odd" % policy_head.out_features)
            A = policy_head.out_features // 2
            if not 1 <= A <= MAX_ACT:
                raise NotImplementedError("DeviceLearner (fs_ppo_model): act_dim A = %d; 1..32 are built" % A)
            _check_trunk("the policy network", self.p_hidden, policy_head, 2 * A,
                         "the head gives the A = %d means and the A log stds" % A)
        else:
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
        if not self.net_log_std:
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
        self.weights = torch.zeros(self.P, dtype=torch.float32, device=dev)      # [policy][log_std A][value]; net_log_std:
        #                                                                          [policy with its 2A-row head][value]
        self.grad = torch.zeros(self.P, dtype=torch.float32, device=dev)         # the same layout
        self.loss = torch.zeros(2, dtype=torch.float32, device=dev)              # {sum pg, sum vf} of the last gradients()
        self._mean_std = torch.zeros(2, dtype=torch.float64, device=dev)
        self._work, self._bound_stream = None, None
        self._adopted, self._cache = False, {}
        self.m = self.v = self.state = None                                      # Adam's buffers (adam_step)
        self._stats = self._mean_std_n = None
        # the full loss (gradients_loss): {sum pg, sum vfl, sum KL, sum H} of the last call; {kl_coef, mean KL} (kl_adapt)
        self.loss_sums = torch.zeros(4, dtype=torch.float32, device=dev)
        self.kl_state = torch.tensor([0.2, 0.0], dtype=torch.float64, device=dev)   # (update(): kl_coef_init on its first KL call)
        self._kl_started = False
        self._work_loss = None
        # minibatch SGD (minibatch_step, update(minibatch=)): the epoch counter the kernel's permutation reads -- the bits of
        # a uint64, on the device next to Adam's state so that a replayed graph draws fresh permutations -- and the count of
        # present rows of a step made of PARTIAL launches
        self.mb_epoch = torch.zeros(1, dtype=torch.int64, device=dev)
        self.mb_count = torch.zeros(1, dtype=torch.float64, device=dev)
        self._work_mb, self._work_mbs = None, {}
        off = self.n_policy
        self.n_dist = 2 * A if self.net_log_std else A       # columns of the old distribution (evaluate_dist's mean_old)
        self.struct = L.fs_ppo_model(struct_size=C.sizeof(L.fs_ppo_model), obs_dim=D, act_dim=A, num_hidden=self.num_hidden,
                                     hidden_width=WIDTH, activation=0, policy_weights_dev=self.weights.data_ptr(),
                                     log_std_dev=None if self.net_log_std else self.weights.data_ptr() + 4 * off,
                                     value_weights_dev=self.weights.data_ptr() + 4 * (off + (0 if self.net_log_std else A)))
        self.sync()

    def sync(self):
        if self._adopted:                                    # (the parameters are views into self.weights: nothing to move)
            return
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

    def adopt_parameters(self):
        """Every parameter's ``.data`` becomes its view into ``self.weights`` (no copies afterwards: ``sync()`` has nothing
        to move, and a torch module over the same parameters reads what the kernels write).  Call it before anything
        captures the module's addresses (``vec.capture`` around the torch policy): a graph captured earlier goes on
        reading the old storage."""
        self.sync()
        off = 0
        for p in self.params:
            n = p.numel()
            p.data = self.weights[off:off + n].view_as(p)
            off += n
        self._adopted = True

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
        if self.net_log_std:
            raise NotImplementedError("DeviceLearner.gradients (fs_ppo_grad_dev): the gradient with the sample count from the "
                                      "host is not built for the 2A-output head (net_log_std=True); gradients_n / "
                                      "gradients_loss / update take it")
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

    # ---- the rest of ppo_update on the device: statistics, the gradient with n on the device, Adam, the whole update
    def _f64(self, n):
        return self.torch.zeros(n, dtype=self.torch.float64, device=self.device)

    def adv_stats(self, adv, act=None, accumulate=False, adv64=None, stats=None):
        """``(adv64 [n], stats [3])``: the float64 copy of the float32 advantages ``adv`` (any shape of n elements) and
        ``{sum adv, sum adv^2, count}`` over the present rows -- a row of ``act [n, A]`` with a NaN is absent; its adv64
        is 0.  ``accumulate=True`` adds the sums to what ``stats`` holds."""
        torch = self.torch
        n = int(adv.numel())
        adv = self._f32(adv.reshape(-1), (n,), "adv")
        act = None if act is None else self._f32(act, (n, int(act.shape[-1])), "act")
        adv64 = torch.empty(n, dtype=torch.float64, device=self.device) if adv64 is None else adv64
        stats = self._f64(3) if stats is None else stats
        self._bind()
        self._adv_stats(n, adv, act, accumulate, adv64, stats)
        return adv64, stats

    def _adv_stats(self, n, adv, act, accumulate, adv64, stats):
        L.check(self.sim.lib.fs_adv_stats_dev(self.sim._h, n, adv.data_ptr(), act.data_ptr() if act is not None else None,
                                              int(act.shape[-1]) if act is not None else 0, int(bool(accumulate)),
                                              adv64.data_ptr(), stats.data_ptr()), self.sim.lib)

    def adv_finish(self, stats, out=None):
        """``{mean, std, n}`` (float64 [3]) of ``stats = {sum, sum of squares, count}``: ppo_update's formula."""
        out = self._f64(3) if out is None else out
        self._bind()
        L.check(self.sim.lib.fs_adv_finish_dev(self.sim._h, stats.data_ptr(), out.data_ptr()), self.sim.lib)
        return out

    def _workspace(self, n):
        need = int(self.sim.lib.fs_ppo_workspace(C.byref(self.struct), n))
        if self._work is None or self._work.numel() < need:
            self._work = self.torch.empty(need, dtype=self.torch.float32, device=self.device)
        return self._work

    def gradients_n(self, obs, act, logp_old, adv, ret, mean_std_n, clip=0.2, vf_coef=0.5, accumulate=False):
        """``gradients()`` with the statistics and the sample count of the whole update on the device: ``mean_std_n`` is
        the float64 ``{mean, std, n}`` of ``adv_finish``; no host value of ``n`` is needed."""
        torch = self.torch
        n = int(obs.shape[0])
        obs, act = self._f32(obs, (n, self.D), "obs"), self._f32(act, (n, self.A), "act")
        logp_old, ret = self._f32(logp_old, (n,), "logp_old"), self._f32(ret, (n,), "ret")
        if adv.dtype != torch.float64 or tuple(adv.shape) != (n,) or adv.device != self.device:
            raise ValueError("DeviceLearner: adv must be a float64 tensor of shape (%d,) on %s" % (n, self.device))
        if mean_std_n.dtype != torch.float64 or mean_std_n.numel() != 3 or mean_std_n.device != self.device:
            raise ValueError("DeviceLearner: mean_std_n must be a float64 tensor of 3 elements on %s" % self.device)
        work = self._workspace(n)
        self._bind()
        self._grad_n(n, obs, act, logp_old, adv.contiguous(), ret, mean_std_n, clip, vf_coef, accumulate, work)
        return self.loss

    def _grad_n(self, n, obs, act, logp_old, adv64, ret, mean_std_n, clip, vf_coef, accumulate, work):
        L.check(self.sim.lib.fs_ppo_grad_n_dev(self.sim._h, C.byref(self.struct), n, obs.data_ptr(), act.data_ptr(),
                                               logp_old.data_ptr(), adv64.data_ptr(), ret.data_ptr(), mean_std_n.data_ptr(),
                                               float(clip), float(vf_coef), int(bool(accumulate)), self.grad.data_ptr(),
                                               self.loss.data_ptr(), work.data_ptr(), work.numel()), self.sim.lib)

    # ---- the reference's loss: KL penalty, clipped value loss, entropy (fs_ppo_eval_dist_dev, fs_ppo_grad_loss_dev,
    # fs_kl_adapt_dev)
    def evaluate_dist(self, obs, act):
        """``evaluate()`` that also returns the head's means: ``(logp [n], val [n], mean_old [n, A])``, the old
        distribution of the KL term (``val`` serves as the old value of the clipped value loss).  ``logp`` and ``val``
        hold the bits ``evaluate()`` gives.  ``net_log_std``: ``mean_old`` is ``[n, 2A]``, a row's A means and then its A
        log stds -- the whole old distribution, which ``gradients_loss`` / ``minibatch_step`` take as ``mean_old`` with
        ``log_std_old=None``."""
        torch = self.torch
        n = int(obs.shape[0])
        obs, act = self._f32(obs, (n, self.D), "obs"), self._f32(act, (n, self.A), "act")
        logp = torch.empty(n, dtype=torch.float32, device=self.device)
        val = torch.empty(n, dtype=torch.float32, device=self.device)
        mean_old = torch.empty(n, self.n_dist, dtype=torch.float32, device=self.device)
        self._bind()
        self._eval_dist(n, obs, act, logp, val, mean_old)
        return logp, val, mean_old

    def _eval_dist(self, n, obs, act, logp, val, mean_old):
        L.check(self.sim.lib.fs_ppo_eval_dist_dev(self.sim._h, C.byref(self.struct), n, obs.data_ptr(), act.data_ptr(),
                                                  logp.data_ptr(), val.data_ptr(), mean_old.data_ptr()), self.sim.lib)

    def _loss_workspace(self, n):
        need = int(self.sim.lib.fs_ppo_loss_workspace(C.byref(self.struct), n))
        if self._work_loss is None or self._work_loss.numel() < need:
            self._work_loss = self.torch.empty(need, dtype=self.torch.float32, device=self.device)
        return self._work_loss

    def gradients_loss(self, obs, act, logp_old, adv, ret, mean_std_n, mean_old=None, log_std_old=None, val_old=None,
                       clip=0.2, vf_coef=0.5, vf_clip=None, entropy_coef=0.0, kl=False, accumulate=False):
        """``gradients_n()`` for the reference's loss (include/flowsim.h ``fs_ppo_loss``): per present sample
        ``-pg + kl_coef KL(old || new) + vf_coef max((v - ret)^2, (v_c - ret)^2) - entropy_coef H`` over the sample count
        in ``mean_std_n``.  ``kl=True``: the KL term, its coefficient read ON THE DEVICE from ``self.kl_state[0]``
        (``mean_old [n, A]`` and ``log_std_old [A]`` are then needed); ``vf_clip`` (``None`` / ``inf``: off) needs
        ``val_old [n]``.  The gradient goes to ``self.grad``, ``{sum pg, sum vfl, sum KL, sum H}`` to ``self.loss_sums``
        (returned); ``self.loss`` is not touched.  With every term off, ``self.grad`` and ``self.loss_sums[:2]`` hold the
        bits of ``gradients_n()``."""
        torch = self.torch
        n = int(obs.shape[0])
        obs, act = self._f32(obs, (n, self.D), "obs"), self._f32(act, (n, self.A), "act")
        logp_old, ret = self._f32(logp_old, (n,), "logp_old"), self._f32(ret, (n,), "ret")
        if adv.dtype != torch.float64 or tuple(adv.shape) != (n,) or adv.device != self.device:
            raise ValueError("DeviceLearner: adv must be a float64 tensor of shape (%d,) on %s" % (n, self.device))
        if mean_std_n.dtype != torch.float64 or mean_std_n.numel() != 3 or mean_std_n.device != self.device:
            raise ValueError("DeviceLearner: mean_std_n must be a float64 tensor of 3 elements on %s" % self.device)
        mean_old = None if mean_old is None else self._f32(mean_old, (n, self.n_dist), "mean_old")
        log_std_old = None if log_std_old is None else self._f32(log_std_old, (self.A,), "log_std_old")
        val_old = None if val_old is None else self._f32(val_old, (n,), "val_old")
        work = self._loss_workspace(n)
        self._bind()
        self._grad_loss(n, obs, act, logp_old, mean_old, log_std_old, val_old, adv.contiguous(), ret, mean_std_n, clip, vf_coef,
                        vf_clip, entropy_coef, kl, accumulate, work)
        return self.loss_sums

    def _grad_loss(self, n, obs, act, logp_old, mean_old, log_std_old, val_old, adv64, ret, mean_std_n, clip, vf_coef, vf_clip,
                   entropy_coef, kl, accumulate, work):
        ptr = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
        loss = L.fs_ppo_loss(struct_size=C.sizeof(L.fs_ppo_loss), clip=float(clip), vf_coef=float(vf_coef),
                             vf_clip=0.0 if vf_clip is None else float(vf_clip), entropy_coef=float(entropy_coef),
                             kl_state_dev=self.kl_state.data_ptr() if kl else None)
        L.check(self.sim.lib.fs_ppo_grad_loss_dev(self.sim._h, C.byref(self.struct), C.byref(loss), n, obs.data_ptr(),
                                                  act.data_ptr(), logp_old.data_ptr(), ptr(mean_old), ptr(log_std_old),
                                                  ptr(val_old), adv64.data_ptr(), ret.data_ptr(), mean_std_n.data_ptr(),
                                                  int(bool(accumulate)), self.grad.data_ptr(), self.loss_sums.data_ptr(),
                                                  work.data_ptr(), work.numel()), self.sim.lib)

    def kl_adapt(self, kl_target, mean_std_n, loss_sums=None):
        """RLlib's rule, on the device, in double: ``mean_kl = loss_sums[2] / mean_std_n[2]``; ``self.kl_state[0]`` times
        1.5 where it exceeds ``2 kl_target``, times 0.5 where it is below ``0.5 kl_target``; ``self.kl_state[1] = mean_kl``.
        Once per update, after the last epoch's ``gradients_loss`` (and the all-reduce of ``loss_sums``)."""
        sums = self.loss_sums if loss_sums is None else loss_sums
        self._bind()
        L.check(self.sim.lib.fs_kl_adapt_dev(self.sim._h, sums.data_ptr(), mean_std_n.data_ptr(), self.kl_state.data_ptr(),
                                             float(kl_target)), self.sim.lib)
        return self.kl_state

    # ---- minibatch SGD: one launch per step (fs_ppo_minibatch_dev), the chain's finish (fs_ppo_mb_finish_dev)
    def _mb_workspace(self, batch):
        """The workspace of minibatch steps of ``batch`` rows: one buffer per size, made once and KEPT -- a graph captured
        at one batch size holds its buffer's address, so a later call at a larger size must not free it."""
        need = int(self.sim.lib.fs_ppo_minibatch_workspace(C.byref(self.struct), int(batch)))
        if need not in self._work_mbs:
            self._work_mbs[need] = self.torch.empty(max(need, 1), dtype=self.torch.float32, device=self.device)
        self._work_mb = self._work_mbs[need]
        return self._work_mb

    def minibatch_step(self, obs, act, logp_old, adv, ret, mean_std_n, batch, index, shuffle_seed=0, mean_old=None,
                       log_std_old=None, val_old=None, clip=0.2, vf_coef=0.5, vf_clip=None, entropy_coef=0.0, kl=False,
                       partial=False, accumulate=False, first=None, last=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        """ONE minibatch step of a shuffled epoch in one launch (``fs_ppo_minibatch_dev``): minibatch ``index`` of size
        ``batch`` of the ``n`` rows, i.e. rows ``epoch_permutation(shuffle_seed, self.mb_epoch, n)[index * batch :
        (index + 1) * batch]`` -- gathered inside the kernel --, the loss of ``gradients_loss`` over them divided by the
        minibatch's own count of present rows, its gradient into ``self.grad``, and one Adam step on ``self.weights``
        (``m``, ``v``, ``state`` as ``adam_step`` keeps them).  The raw loss sums are added to ``self.loss_sums``
        (``first``: overwrite; default: ``index == 0``); ``last`` (default: the epoch's last minibatch) advances
        ``self.mb_epoch``.  A minibatch without a present row makes no step.  ``adv`` is the raw float64 advantage and
        ``mean_std_n`` its statistics over the whole batch.
        ``partial=True``: the launch only reduces -- raw sums into ``self.grad`` / ``self.loss_sums``, the count into
        ``self.mb_count`` (``accumulate=True``: a later shard of the same step, added) -- and ``mb_finish()`` ends the step
        once every shard (and rank) is in.  One shard without ``partial`` gives the bits of ``partial`` + ``mb_finish``."""
        torch = self.torch
        n = int(obs.shape[0])
        obs, act = self._f32(obs, (n, self.D), "obs"), self._f32(act, (n, self.A), "act")
        logp_old, ret = self._f32(logp_old, (n,), "logp_old"), self._f32(ret, (n,), "ret")
        if adv.dtype != torch.float64 or tuple(adv.shape) != (n,) or adv.device != self.device:
            raise ValueError("DeviceLearner: adv must be a float64 tensor of shape (%d,) on %s" % (n, self.device))
        if mean_std_n.dtype != torch.float64 or mean_std_n.numel() != 3 or mean_std_n.device != self.device:
            raise ValueError("DeviceLearner: mean_std_n must be a float64 tensor of 3 elements on %s" % self.device)
        mean_old = None if mean_old is None else self._f32(mean_old, (n, self.n_dist), "mean_old")
        log_std_old = None if log_std_old is None else self._f32(log_std_old, (self.A,), "log_std_old")
        val_old = None if val_old is None else self._f32(val_old, (n,), "val_old")
        batch, index = int(batch), int(index)
        steps = -(-n // max(batch, 1))
        self._adam_buffers()
        work = self._mb_workspace(batch)
        self._bind()
        self._mb_step(n, obs, act, logp_old, mean_old, log_std_old, val_old, adv.contiguous(), ret, mean_std_n, batch, index,
                      shuffle_seed, clip, vf_coef, vf_clip, entropy_coef, kl, partial, accumulate,
                      index == 0 if first is None else first, index == steps - 1 if last is None else last, lr, betas, eps, work)
        return self.loss_sums

    def _mb_step(self, n, obs, act, logp_old, mean_old, log_std_old, val_old, adv64, ret, mean_std_n, batch, index, seed, clip,
                 vf_coef, vf_clip, entropy_coef, kl, partial, accumulate, first, last, lr, betas, eps, work):
        ptr = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
        loss = L.fs_ppo_loss(struct_size=C.sizeof(L.fs_ppo_loss), clip=float(clip), vf_coef=float(vf_coef),
                             vf_clip=0.0 if vf_clip is None else float(vf_clip), entropy_coef=float(entropy_coef),
                             kl_state_dev=self.kl_state.data_ptr() if kl else None)
        flags = (L.FS_MB_ACCUMULATE if accumulate else 0) | (L.FS_MB_FIRST if first else 0) | (L.FS_MB_LAST if last else 0)
        mb = L.fs_ppo_minibatch(struct_size=C.sizeof(L.fs_ppo_minibatch), mode=L.FS_MB_PARTIAL if partial else L.FS_MB_STEP,
                                flags=flags, batch=batch, index=index, seed=int(seed) & (2 ** 64 - 1),
                                epoch_dev=self.mb_epoch.data_ptr(), count_dev=self.mb_count.data_ptr(),
                                weights_dev=self.weights.data_ptr(), m_dev=self.m.data_ptr(), v_dev=self.v.data_ptr(),
                                state_dev=self.state.data_ptr(), lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]),
                                eps=float(eps))
        L.check(self.sim.lib.fs_ppo_minibatch_dev(self.sim._h, C.byref(self.struct), C.byref(loss), C.byref(mb), n,
                                                  obs.data_ptr(), act.data_ptr(), logp_old.data_ptr(), ptr(mean_old),
                                                  ptr(log_std_old), ptr(val_old), adv64.data_ptr(), ret.data_ptr(),
                                                  mean_std_n.data_ptr(), self.grad.data_ptr(), self.loss_sums.data_ptr(),
                                                  work.data_ptr(), work.numel()), self.sim.lib)

    def mb_finish(self, last=False, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        """The end of a step made of ``minibatch_step(partial=True)`` launches (``fs_ppo_mb_finish_dev``): ``self.grad``
        (raw sums) times ``float(1 / self.mb_count)``, then ``adam_step``'s sequence; no step where the count is 0.
        ``last=True`` advances ``self.mb_epoch``."""
        self._adam_buffers()
        self._bind()
        L.check(self.sim.lib.fs_ppo_mb_finish_dev(self.sim._h, self.P, self.weights.data_ptr(), self.grad.data_ptr(),
                                                  self.m.data_ptr(), self.v.data_ptr(), self.state.data_ptr(),
                                                  self.mb_count.data_ptr(), self.mb_epoch.data_ptr(),
                                                  L.FS_MB_LAST if last else 0, float(lr), float(betas[0]), float(betas[1]),
                                                  float(eps)), self.sim.lib)

    @staticmethod
    def minibatch_fused(batch, D, A, num_hidden):
        """Does ``update(minibatch=batch)`` make a one-shard step as ONE launch (True) or as the chain PARTIAL +
        ``mb_finish`` (False)?  A rule on (B, D, A, L) alone, from profiles/ppo_minibatch_bench.json (DESIGN.md 4.3
        "Minibatches"): at (3, 1), (25, 5) and (141, 20), each at B = 128, 1024 and 4096, the chain took 0.93 .. 0.97 of the
        one launch's time, the ranges apart at all nine points -- Adam by the one wave of the tail costs more than a second
        launch of 1024 lanes -- so the rule is the chain, everywhere.  Both give the same bits."""
        return False

    def _adam_buffers(self):
        torch = self.torch
        if self.state is None:
            self.m, self.v = torch.zeros_like(self.weights), torch.zeros_like(self.weights)
            self.state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=self.device)

    def adam_step(self, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        """One step of torch's Adam (no weight decay, amsgrad or maximize) on ``self.weights`` with ``self.grad``
        (``fs_adam_dev``).  The learner owns ``m``, ``v`` [P] and ``state`` = float64 ``{t, beta1^t, beta2^t}``, all on the
        device.  The module's parameters see the step after ``adopt_parameters()``."""
        self._adam_buffers()
        self._bind()
        L.check(self.sim.lib.fs_adam_dev(self.sim._h, self.P, self.weights.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(),
                                         self.v.data_ptr(), self.state.data_ptr(), float(lr), float(betas[0]), float(betas[1]),
                                         float(eps)), self.sim.lib)

    # ---- checkpoints: everything update() carries from one call to the next
    def descriptor(self):
        """The model the packed buffers are laid out for: ``(D, A, num_hidden, net_log_std)``."""
        return (int(self.D), int(self.A), int(self.num_hidden), bool(self.net_log_std))

    def state_dict(self):
        """Plain CPU tensors and numbers: the packed ``weights``, Adam's ``m`` / ``v`` / ``state`` ({t, beta1^t, beta2^t}),
        ``kl_state`` ({coefficient, last mean KL}; ``kl_started``: whether an update has set the coefficient yet), the
        minibatch epoch counter ``mb_epoch`` and the model ``descriptor``.  Synchronises the device (it copies to the
        host)."""
        self.sync()
        self._adam_buffers()
        cpu = lambda t: t.detach().to("cpu").clone()                               # noqa: E731
        return dict(descriptor=list(self.descriptor()), weights=cpu(self.weights), m=cpu(self.m), v=cpu(self.v),
                    state=cpu(self.state), kl_state=cpu(self.kl_state), kl_started=bool(self._kl_started),
                    mb_epoch=cpu(self.mb_epoch))

    def load_state_dict(self, sd):
        """Copies a ``state_dict()`` into the learner's buffers IN PLACE: parameters that are views of ``weights``
        (``adopt_parameters``) and a DevicePolicy that ``share``s the buffer see the loaded values, and a captured graph
        keeps its addresses.  Parameters that were not adopted are written too.  A state made for another model
        ``(D, A, num_hidden, net_log_std)`` is refused by name."""
        torch = self.torch
        check_descriptor("DeviceLearner.load_state_dict", sd["descriptor"], self.descriptor())
        if int(sd["weights"].numel()) != self.P:
            raise ValueError("DeviceLearner.load_state_dict: the checkpoint holds %d packed weights, this learner %d"
                             % (int(sd["weights"].numel()), self.P))
        self._adam_buffers()
        with torch.no_grad():
            for name in ("weights", "m", "v", "state", "kl_state", "mb_epoch"):
                getattr(self, name).copy_(sd[name].to(self.device))
            if not self._adopted:
                off = 0
                for p in self.params:
                    n = p.numel()
                    p.copy_(self.weights[off:off + n].view_as(p))
                    off += n
        self._kl_started = bool(sd.get("kl_started", True))

    def _shard_buffers(self, j, K, R):
        """Intermediates of shard ``j`` of ``update()``, allocated once per shape."""
        torch = self.torch
        buf = self._cache.get((j, K, R))
        if buf is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            buf = dict(logp=torch.empty(K * R, **f32), val=torch.empty(K * R, **f32), last_val=torch.empty(R, **f32),
                       adv=torch.empty(K, R, **f32), ret=torch.empty(K, R, **f32),
                       adv64=torch.empty(K * R, dtype=torch.float64, device=self.device))
            self._cache[(j, K, R)] = buf
        return buf

    def update(self, shards, epochs=4, clip=0.2, vf_coef=0.5, gamma=0.999, lam=0.97, lr=3e-4, betas=(0.9, 0.999), eps=1e-8,
               group=None, kl_target=None, kl_coef_init=0.2, entropy_coef=0.0, vf_clip=None, minibatch=None, shuffle_seed=0,
               fused=None):
        """One PPO update over ``shards`` = [(obs [K+1, R, D], act [K, R(, A)], rew [K, R], done [K, R] uint8)], the whole of
        train_vec.ppo_update on the learner's stream: per shard eval (two launches), gae and the statistics; the
        all-reduce of the three sums (in a data-parallel run); finish; per epoch the gradient over the shards (kernel and
        reduction), the all-reduce of the packed gradient, Adam.  One shard and 4 epochs: 2 + 1 + 1 + 1 + 4 x 3 = 17
        launches.  No host synchronisation; no allocation after the first call at a shape (contiguous float32 / uint8
        shards as the rollouts return them), so the call can be captured into a graph after one eager call ON the capture
        stream (that call binds the handle to the stream -- fs_set_stream synchronises -- and makes every buffer, the
        library's scratch for the statistics included).  The parameters must have been adopted (``adopt_parameters()``):
        Adam moves ``self.weights``.
        ``kl_target`` / ``entropy_coef`` / ``vf_clip``: the reference's loss (``gradients_loss``).  With any of them on,
        the first eval of a shard is ``evaluate_dist`` (its ``val`` is the old value) followed by one device-to-device
        copy of ``log_std`` into the shard's ``log_std_old``; every epoch's gradient is ``gradients_loss``; after the last
        epoch come the all-reduce of ``loss_sums`` (data-parallel runs) and, with ``kl_target`` set, ``kl_adapt``: the
        coefficient lives in ``self.kl_state`` on the device (``kl_coef_init`` before the first such update), so a
        replayed graph advances it.  ``self.loss`` is then left alone: the sums are ``self.loss_sums``.  With the
        defaults the launches are exactly the 17 above.
        ``minibatch`` (a per-shard size B; ``None``: everything above, launch for launch): an epoch is a shuffled pass of
        ``ceil(n / B)`` minibatch steps (``minibatch_step`` states one step), each ONE launch for one shard in one process
        (``fused=True``: 5 + epochs x ceil(n / B) launches, plus the copy and ``kl_adapt`` with the loss terms on) or the
        chain of two, PARTIAL + ``mb_finish`` (what the rule ``minibatch_fused`` picks: it measured faster); for several
        shards (of equal n: ``ValueError`` otherwise) or ranks, one PARTIAL launch per shard, the all-reduces of the raw
        sums and of the count, and ``mb_finish``.  The statistics, the old distribution and the KL coefficient stay those of
        the update's start; ``loss_sums`` accumulate over an epoch's minibatches, so ``kl_adapt`` sees the last epoch's
        mean KL, each minibatch's evaluated before its own step.  The permutations are
        ``epoch_permutation(shuffle_seed, self.mb_epoch, n)``; ``self.mb_epoch`` advances on the device with every epoch.
        ``epochs=0`` makes the prelude alone: no step, and no ``kl_adapt`` either (no KL was seen; ``loss_sums`` is left).
        ``fused`` (``None``: the rule ``minibatch_fused``) picks the one-launch step or the chain for one shard in one
        process -- the same bits either way (scripts/bench_ppo_minibatch.py times both).
        Returns ``self.loss_sums``."""
        import torch.distributed as dist
        torch, lib, h = self.torch, self.sim.lib, self.sim._h
        if self._stats is None:
            self._stats, self._mean_std_n = self._f64(3), self._f64(3)
        if not self._adopted:
            raise RuntimeError("DeviceLearner.update: call adopt_parameters() first -- Adam moves self.weights, and only "
                               "adopted parameters are views of them")
        self._adam_buffers()
        self._bind()
        kl_on = kl_target is not None
        vclip_on = vf_clip is not None and 0.0 < float(vf_clip) < float("inf")
        full = kl_on or vclip_on or float(entropy_coef) != 0.0
        if minibatch is not None:
            minibatch = int(minibatch)
            if minibatch < 1:
                raise ValueError("DeviceLearner.update: minibatch must be at least 1 (got %d)" % minibatch)
            sizes = set(int(s[2].shape[0]) * int(s[2].shape[1]) for s in shards)
            if len(sizes) != 1:
                raise ValueError("DeviceLearner.update: minibatch steps take rows [kB, (k + 1)B) of every shard's own "
                                 "permutation, so the shards must hold the same number of samples (got %s)" % sorted(sizes))
            work_mb = self._mb_workspace(minibatch)
        if kl_on and not self._kl_started:
            self.kl_state[0].fill_(float(kl_coef_init))       # (the first such call is eager: never inside a capture)
            self.kl_state[1].fill_(0.0)
            self._kl_started = True
        prepared = []
        for j, (obs, act, rew, done) in enumerate(shards):
            K, R = int(rew.shape[0]), int(rew.shape[1])
            n = K * R
            if done.dtype != torch.uint8 or tuple(done.shape) != (K, R) or done.device != self.device:
                raise ValueError("DeviceLearner: done must be a uint8 tensor of shape %s on %s" % ((K, R), self.device))
            obs = self._f32(obs, (K + 1, R, self.D), "obs")
            o, last = obs[:K].reshape(n, self.D), obs[K]
            a = self._f32(act.reshape(n, -1), (n, self.A), "act")
            rew, done = self._f32(rew, (K, R), "rew"), done.contiguous()
            b = self._shard_buffers(j, K, R)
            if full:
                if "mean_old" not in b:
                    b["mean_old"] = torch.empty(n, self.n_dist, dtype=torch.float32, device=self.device)
                    b["log_std_old"] = None if self.net_log_std else torch.empty(self.A, dtype=torch.float32, device=self.device)
                self._eval_dist(n, o, a, b["logp"], b["val"], b["mean_old"])
                if not self.net_log_std:                     # (net_log_std: the old log stds are columns A .. 2A-1 of mean_old)
                    b["log_std_old"].copy_(self.weights[self.n_policy:self.n_policy + self.A])
                self._loss_workspace(n)
            else:
                L.check(lib.fs_ppo_eval_dev(h, C.byref(self.struct), n, o.data_ptr(), a.data_ptr(), b["logp"].data_ptr(),
                                            b["val"].data_ptr()), lib)
            L.check(lib.fs_ppo_eval_dev(h, C.byref(self.struct), R, last.data_ptr(), None, None, b["last_val"].data_ptr()), lib)
            L.check(lib.fs_gae_dev(h, K, R, rew.data_ptr(), b["val"].data_ptr(), b["last_val"].data_ptr(), done.data_ptr(),
                                   float(gamma), float(lam), b["adv"].data_ptr(), b["ret"].data_ptr()), lib)
            self._adv_stats(n, b["adv"], a, j > 0, b["adv64"], self._stats)
            self._workspace(n)                               # (grows to the largest shard's need)
            prepared.append((n, o, a, b))
        spread = dist.is_available() and dist.is_initialized()
        if spread:
            dist.all_reduce(self._stats, op=dist.ReduceOp.SUM, group=group)
        L.check(lib.fs_adv_finish_dev(h, self._stats.data_ptr(), self._mean_std_n.data_ptr()), lib)
        if minibatch is not None:
            n = prepared[0][0]
            steps = -(-n // minibatch)
            if fused is None:
                fused = self.minibatch_fused(minibatch, self.D, self.A, self.num_hidden)
            chain = spread or len(prepared) > 1 or not fused
            for _ in range(epochs):
                for k in range(steps):
                    for j, (n, o, a, b) in enumerate(prepared):
                        self._mb_step(n, o, a, b["logp"], b.get("mean_old") if full else None,
                                      b.get("log_std_old") if full else None, b["val"] if full else None, b["adv64"],
                                      b["ret"], self._mean_std_n, minibatch, k, shuffle_seed, clip, vf_coef,
                                      vf_clip if vclip_on else None, entropy_coef, kl_on, chain, j > 0, k == 0,
                                      k == steps - 1, lr, betas, eps, work_mb)
                    if chain:
                        if spread:
                            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=group)
                            dist.all_reduce(self.mb_count, op=dist.ReduceOp.SUM, group=group)
                        self.mb_finish(k == steps - 1, lr, betas, eps)
            if epochs < 1:                                   # (no epoch: no KL was seen, the coefficient stays -- ppo_update's rule)
                return self.loss_sums
            if spread:
                dist.all_reduce(self.loss_sums, op=dist.ReduceOp.SUM, group=group)
            if kl_on:
                self.kl_adapt(kl_target, self._mean_std_n)
            return self.loss_sums
        for _ in range(epochs):
            for j, (n, o, a, b) in enumerate(prepared):
                if full:
                    self._grad_loss(n, o, a, b["logp"], b["mean_old"], b["log_std_old"], b["val"], b["adv64"], b["ret"],
                                    self._mean_std_n, clip, vf_coef, vf_clip if vclip_on else None, entropy_coef, kl_on,
                                    j > 0, self._work_loss)
                else:
                    self._grad_n(n, o, a, b["logp"], b["adv64"], b["ret"], self._mean_std_n, clip, vf_coef, j > 0, self._work)
            if spread:
                dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=group)
            self.adam_step(lr, betas, eps)
        if full:
            if spread:
                dist.all_reduce(self.loss_sums, op=dist.ReduceOp.SUM, group=group)
            if kl_on:
                self.kl_adapt(kl_target, self._mean_std_n)
            return self.loss_sums
        return self.loss
