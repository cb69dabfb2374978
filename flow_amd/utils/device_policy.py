"""DevicePolicy: a torch fully connected Gaussian policy in the form libflowsim's policy-in-the-loop entry points take.

What the reference's rollout workers evaluate per step through RLlib (examples/train.py:149-160: the default model,
``fcnet_hiddens [32, 32, 32]``, tanh, a diagonal Gaussian over the action) is here a flat float32 weight buffer on the
device that ``fs_policy_rollout_dev`` / ``fs_policy_act_dev`` read (include/flowsim.h ``fs_policy``): K steps of
policy -> action -> Env.step are ONE kernel launch, observations and actions never leave the chip's registers.
"""
import ctypes as C

from flow_amd import _lib as L


class DevicePolicy(object):
    """``hidden``: the ``nn.Linear`` layers of the trunk (1..3, 32 units each, tanh between them); ``head``: the output
    ``nn.Linear`` (2 outputs = mean and log std; 1 output with ``log_std`` a 1-element parameter / tensor).  ``sync()``
    copies the current parameter values into the packed device buffer (call it after every optimiser step);
    ``share(learner)`` runs the policy on a DeviceLearner's packed weights instead, with nothing to copy.

    ``act_dim`` > 1: ONE network with an action vector (MergePOEnv, ``FlowSim.policy_action_dim``): ``head`` has
    ``2 * act_dim`` outputs -- the means, then the log stds: RLlib's DiagGaussian order -- or ``act_dim`` outputs with
    ``log_std`` of ``act_dim`` elements.  The packed buffer is the same: per layer W [out][in] row-major, then b [out].

    ``greedy`` (``fs_policy.greedy``; also a property that can be set between launches, nothing is repacked): every
    policy kernel applies the MEAN action -- ``act = mu`` exactly, ``logp`` the density at the mean -- instead of a
    sample.  The sampling streams advance as they do when sampling, so greedy and sampling calls interleave on one
    stream.  A captured graph holds the flag's value at capture."""

    def __init__(self, hidden, head, log_std=None, seed=0, act_dim=1, greedy=False):
        import torch
        self.torch = torch
        self.hidden, self.head, self.log_std_param = list(hidden), head, log_std
        self.act_dim = A = int(act_dim)
        if not 1 <= len(self.hidden) <= 3 or any(l.out_features != 32 for l in self.hidden):
            raise NotImplementedError("DevicePolicy: 1..3 hidden layers of 32 units (the kernel's model class)")
        n_out = A if log_std is not None else 2 * A
        if A < 1 or head.out_features != n_out or head.in_features != 32:
            raise NotImplementedError("DevicePolicy: the head maps 32 units to %d output(s)" % n_out)
        if log_std is not None and log_std.numel() != A:
            raise NotImplementedError("DevicePolicy: log_std has %d element(s), one per action column" % A)
        dev = head.weight.device
        n = sum(l.weight.numel() + l.bias.numel() for l in self.hidden) + head.weight.numel() + head.bias.numel()
        self.buf = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ls = torch.zeros(A, dtype=torch.float32, device=dev) if log_std is not None else None
        self.struct = L.fs_policy(struct_size=C.sizeof(L.fs_policy), obs_dim=self.hidden[0].in_features,
                                  num_hidden=len(self.hidden), hidden_width=32, activation=0,
                                  greedy=1 if greedy else 0, weights_dev=self.buf.data_ptr(),
                                  log_std_dev=self.ls.data_ptr() if self.ls is not None else None, seed=int(seed))
        self.sync()

    @property
    def greedy(self):
        return bool(self.struct.greedy)

    @greedy.setter
    def greedy(self, on):
        self.struct.greedy = 1 if on else 0

    def share(self, learner):
        """Run on the storage of ``learner`` (a ``flow_amd.utils.device_ppo.DeviceLearner`` over the same network): the
        struct's ``weights_dev`` and ``log_std_dev`` point into ``learner.weights`` -- [policy weights][log_std A][value
        weights], the policy's part in this class's own layout -- so the rollout kernels read the very buffer the
        learner's Adam writes, and ``sync()`` has nothing to do.  The head's form must be the learner's -- the free
        ``log_std`` with a free-``log_std`` learner, the head of 2 x act_dim outputs with a ``net_log_std=True`` learner
        (``weights_dev`` is then the learner's policy part, [policy with its 2A-row head], and ``log_std_dev`` stays NULL)
        -- and so must the layer shapes.  Share before a graph captures the policy (``vec.capture``)."""
        net_ls = bool(getattr(learner, "net_log_std", False))
        if self.ls is None and not net_ls:
            raise NotImplementedError("DevicePolicy.share: the head of 2 x act_dim outputs (no free log_std) cannot share a "
                                      "DeviceLearner's storage: its packed weights hold the act_dim means next to log_std")
        if self.ls is not None and net_ls:
            raise NotImplementedError("DevicePolicy.share: a policy with a free log_std cannot share the storage of a "
                                      "DeviceLearner(net_log_std=True): its packed weights hold the head of 2 x act_dim "
                                      "outputs and no log_std")
        mine = (self.hidden[0].in_features, len(self.hidden), self.act_dim)
        theirs = (learner.D, learner.num_hidden, learner.A)
        if mine != theirs:
            raise NotImplementedError("DevicePolicy.share: the policy has (obs_dim, hidden layers, act_dim) = %s, the "
                                      "learner %s: the packed layouts differ" % (mine, theirs))
        if learner.weights.device != self.buf.device or learner.n_policy != self.buf.numel():
            raise ValueError("DevicePolicy.share: the learner's weights live on %s with %d policy values; the policy has %d on %s"
                             % (learner.weights.device, learner.n_policy, self.buf.numel(), self.buf.device))
        self.shared = learner
        self.buf = learner.weights[:learner.n_policy]
        self.struct.weights_dev = self.buf.data_ptr()
        if net_ls:                                           # (the log stds are rows A .. 2A-1 of the head: no slot, NULL)
            self.struct.log_std_dev = None
            return self
        self.ls = learner.weights[learner.n_policy:learner.n_policy + self.act_dim]
        self.struct.log_std_dev = self.ls.data_ptr()
        return self

    def population(self, weights, members, group):
        """A view of this policy over ``members`` weight sets for ``VecFlowEnv.population_act`` / ``population_rollout``:
        ``weights`` is a float32 device tensor ``[members, stride]`` (row m: member m's packed buffer, this class's
        layout, ``stride >= buf.numel()``), or a 1-d tensor of one set that all members share (stride 0); ``group`` replicas
        in a row run each member, ``members * group == num_replicas``.  The log std, the seed and ``greedy`` stay this
        policy's.  The view holds ``weights``: write new sets into it between launches, nothing is copied."""
        return PolicyPopulation(self, weights, members, group)

    def sync(self):
        if getattr(self, "shared", None) is not None:       # (the learner's buffer is the policy's: nothing to repack)
            return
        torch = self.torch
        with torch.no_grad():
            parts = []
            for l in self.hidden + [self.head]:
                parts += [l.weight.reshape(-1), l.bias.reshape(-1)]
            self.buf.copy_(torch.cat([p.detach().float() for p in parts]))
            if self.ls is not None:
                self.ls.copy_(self.log_std_param.detach().float().reshape(self.act_dim))

    def unpack(self):
        """The inverse of ``sync()``: copy the packed buffer's values into the modules' parameters (a trainer that writes
        the buffer itself -- ``flow_amd.utils.device_es.DeviceES`` -- calls it before the modules are saved).  The log
        std is not touched."""
        torch, at = self.torch, 0
        with torch.no_grad():
            for l in self.hidden + [self.head]:
                for p in (l.weight, l.bias):
                    p.copy_(self.buf[at:at + p.numel()].reshape(p.shape))
                    at += p.numel()

    def reference(self, obs):
        """(mean, log std) of the same network evaluated by torch (float32): agrees with the kernels to ~1e-6.
        ``act_dim`` > 1: both are ``[..., act_dim]``."""
        torch = self.torch
        h = obs
        for l in self.hidden:
            h = torch.tanh(l(h))
        out = self.head(h)
        A = self.act_dim
        if A > 1:
            if self.ls is not None:
                return out, self.log_std_param.reshape(A).expand_as(out)
            return out[..., :A], out[..., A:]
        if self.ls is not None:
            return out[..., 0], self.log_std_param.reshape(1).expand_as(out[..., 0])
        return out[..., 0], out[..., 1]


class PolicyPopulation(object):
    """``DevicePolicy.population``'s view: ``struct`` is the ``fs_population``, ``policy_struct()`` the policy's ``fs_policy``
    with ``weights_dev`` at the population's weights (built per call: ``greedy`` and the seed are read from the policy)."""

    def __init__(self, policy, weights, members, group):
        torch = policy.torch
        if policy.act_dim != 1:
            raise NotImplementedError("fs_population: not built for the action-vector heads (DevicePolicy(act_dim > 1))")
        P, M = policy.buf.numel(), int(members)
        if weights.dtype != torch.float32 or not weights.is_contiguous() or weights.device != policy.buf.device:
            raise ValueError("DevicePolicy.population: weights must be a contiguous float32 tensor on the policy's device")
        if weights.dim() == 1:
            if weights.numel() < P:
                raise ValueError("DevicePolicy.population: a shared weight set has %d values, the policy %d" % (weights.numel(), P))
            stride = 0
        elif weights.dim() == 2 and weights.shape[0] == M:
            stride = int(weights.shape[1])                  # (the library refuses a stride below the policy's size by name)
        else:
            raise ValueError("DevicePolicy.population: weights must be [members, stride] or one shared set")
        self.policy, self.weights, self.members, self.group, self.stride = policy, weights, M, int(group), stride
        self.struct = L.fs_population(struct_size=C.sizeof(L.fs_population), members=M, group=int(group), reserved=0,
                                      stride=stride)

    def policy_struct(self):
        src = self.policy.struct
        return L.fs_policy(struct_size=src.struct_size, obs_dim=src.obs_dim, num_hidden=src.num_hidden,
                           hidden_width=src.hidden_width, activation=src.activation, greedy=src.greedy,
                           weights_dev=self.weights.data_ptr(), log_std_dev=src.log_std_dev, seed=src.seed)
