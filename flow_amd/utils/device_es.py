"""DeviceES: evolution strategies (RLlib's ES) and augmented random search (RLlib's ARS) on the device.

What the reference's ``flow/benchmarks/rllib/es_runner.py`` and ``ars_runner.py`` do with a pool of CPU workers -- whole
episodes of slightly different policies, a ranking of their returns, one weighted sum of noise vectors -- is here one
population of perturbed policies in ONE rollout launch per fragment (``fs_population_rollout_dev``: a workgroup loads its
member's weights, include/flowsim.h ``fs_population``) and four small kernels around it (``fs_es_*``,
flow_amd/csrc/flowsim_es.h).  There is no backward pass and no noise table: the noise is a Philox stream that the gradient
kernel draws a second time.
"""
from flow_amd import _lib as L


def centered_ranks_ref(fit2n):
    """numpy restatement of k_es_weights, mode ES: float32 ``u [N]`` from the 2 N perturbed returns (float64)."""
    import numpy as np
    f = np.asarray(fit2n, np.float64)
    n2 = f.size
    order = sorted(range(n2), key=lambda i: (f[i], i))
    rank = np.empty(n2, np.int64)
    rank[order] = np.arange(n2)
    c = (rank.astype(np.float64) / np.float64(n2 - 1) - 0.5).astype(np.float32)
    return ((c[0::2] - c[1::2]) / np.float32(n2 // 2)).astype(np.float32)


def ars_weights_ref(fit2n, top=0):
    """numpy restatement of k_es_weights, mode ARS: float32 ``u [N]``; ``top`` <= 0 or > N keeps every direction."""
    import numpy as np
    f = np.asarray(fit2n, np.float64)
    N = f.size // 2
    b = N if (top <= 0 or top > N) else int(top)
    key = np.maximum(f[0::2], f[1::2])
    kept = sorted(sorted(range(N), key=lambda p: (-key[p], p))[:b])
    s = np.float64(0.0)
    for p in kept:
        s = s + f[2 * p]
        s = s + f[2 * p + 1]
    mean = s / np.float64(2 * b)
    ss = np.float64(0.0)
    for p in kept:
        da, db = f[2 * p] - mean, f[2 * p + 1] - mean
        ss = ss + da * da
        ss = ss + db * db
    scale = np.float64(b) * np.sqrt(ss / np.float64(2 * b))
    u = np.zeros(N, np.float32)
    if scale != 0.0:
        for p in kept:
            u[p] = np.float32((f[2 * p] - f[2 * p + 1]) / scale)
    return u


class DeviceES(object):
    """``vec``: a VecFlowEnv whose handle takes a policy population; ``policy``: a ``DevicePolicy`` (its packed buffer is
    theta's layout and its initial value; its log std, seed and model class are the population's).  ``pairs`` N antithetic
    directions and ``eval_members`` E unperturbed members: ``M = 2 N + E`` members of ``group = num_rows / M`` replicas
    each (a multiple of the handle's granule).  ``mode='es'``: centered ranks, ``grad = -g + l2 * theta``, Adam with
    ``lr``; ``mode='ars'``: ``theta += stepsize * g`` with the top ``top`` directions scaled by the standard deviation
    of their returns.

    ``generation(horizon, fragment)`` is perturb -> reset -> ceil(horizon / fragment) population fragments with the mean
    action, each followed by the fitness kernel -> weights -> gradient [-> Adam], all on the current stream with no
    host round trip after the reset; it returns the device tensor ``stats [4]`` = {mean, min, max of the perturbed
    members' returns, mean of the evaluation members'} (the next generation rewrites it)."""

    def __init__(self, vec, policy, pairs, eval_members=0, sigma=0.02, mode="es", lr=0.02, stepsize=None, l2=0.005, top=0,
                 noise_seed=0, betas=(0.9, 0.999), eps=1e-8):
        import torch
        self.torch = torch
        if mode not in ("es", "ars"):
            raise ValueError("DeviceES: mode must be 'es' or 'ars'")
        self.vec, self.policy, self.mode = vec, policy, mode
        self.N, self.E = int(pairs), int(eval_members)
        self.M = 2 * self.N + self.E
        if not 1 <= self.N <= L.FS_ES_MAX_PAIRS or self.E < 0:
            raise ValueError("DeviceES: pairs must be 1 .. %d and eval_members at least 0" % L.FS_ES_MAX_PAIRS)
        R = vec.num_rows
        granule = vec.sim.population_granule(policy.struct)       # (raises with the library's message on a refused handle)
        if R % self.M or (R // self.M) % granule:
            raise ValueError("DeviceES: %d replicas do not divide into %d members (2 x %d pairs + %d evaluation members) of a "
                             "multiple of %d replicas (fs_population_granule)" % (R, self.M, self.N, self.E, granule))
        self.group = R // self.M
        self.sigma = float(sigma)
        self.lr = float(lr)                                        # (ES: Adam's; ARS: stepsize, lr if it is not given)
        self.stepsize = float(lr if stepsize is None else stepsize)
        self.l2, self.top, self.betas, self.eps = float(l2), int(top), (float(betas[0]), float(betas[1])), float(eps)
        self.noise_seed = int(noise_seed)
        self.gen = 0
        dev = policy.buf.device
        self.P = P = policy.buf.numel()
        self.stride = (P + 3) // 4 * 4
        self.theta = policy.buf                                    # (in place: the policy's own buffer is the mean policy)
        self.weights = torch.zeros((self.M, self.stride), dtype=torch.float32, device=dev)
        self.pop = policy.population(self.weights, self.M, self.group)
        self.grad = torch.zeros(P, dtype=torch.float32, device=dev)
        self.m, self.v = torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.float32, device=dev)
        self.state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)
        self.ret = torch.zeros(R, dtype=torch.float64, device=dev)
        self.alive = torch.ones(R, dtype=torch.uint8, device=dev)
        self.fit = torch.zeros(self.M, dtype=torch.float64, device=dev)
        self.u = torch.zeros(self.N, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4, dtype=torch.float64, device=dev)
        lib = vec.sim.lib
        self.work = torch.zeros(max(int(lib.fs_es_workspace(P, self.N)), 1), dtype=torch.float32, device=dev)
        self.rollout_kernel = ""                                   # (fs_last_kernel of the population fragment)
        self._outs = {}                                            # (the fragment's buffers, by its length)

    # ---- the steps of a generation, each one launch ---------------------------------------------------------------
    def _call(self, rc):
        L.check(rc, self.vec.sim.lib)

    def perturb(self):
        sim = self.vec.sim
        self._call(sim.lib.fs_es_perturb_dev(sim._h, self.P, self.N, self.E, self.stride, self.theta.data_ptr(), self.sigma,
                                             self.noise_seed, self.gen, self.weights.data_ptr()))

    def fitness(self, rew, done, accumulate):
        sim = self.vec.sim
        self._call(sim.lib.fs_es_fitness_dev(sim._h, int(rew.shape[0]), self.M, self.group, rew.data_ptr(), done.data_ptr(),
                                             1 if accumulate else 0, self.ret.data_ptr(), self.alive.data_ptr(),
                                             self.fit.data_ptr()))

    def direction_weights(self):
        sim = self.vec.sim
        mode = L.FS_ES_MODE_ES if self.mode == "es" else L.FS_ES_MODE_ARS
        self._call(sim.lib.fs_es_weights_dev(sim._h, mode, self.N, self.E, self.top, self.fit.data_ptr(), self.u.data_ptr(),
                                             self.stats.data_ptr()))

    def gradient(self):
        sim = self.vec.sim
        es = self.mode == "es"
        self._call(sim.lib.fs_es_grad_dev(sim._h, L.FS_ES_MODE_ES if es else L.FS_ES_MODE_ARS, self.P, self.N,
                                          self.u.data_ptr(), self.noise_seed, self.gen, self.l2 if es else self.stepsize,
                                          self.theta.data_ptr(), self.grad.data_ptr(), self.work.data_ptr(),
                                          self.work.numel()))

    def adam(self):
        sim = self.vec.sim
        self._call(sim.lib.fs_adam_dev(sim._h, self.P, self.theta.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(),
                                       self.v.data_ptr(), self.state.data_ptr(), self.lr, self.betas[0], self.betas[1],
                                       self.eps))

    def generation(self, horizon, fragment=100):
        vec = self.vec
        vec.use_current_stream()
        self.perturb()
        vec.reset()
        greedy = self.policy.greedy
        self.policy.greedy = True
        try:
            left, first = int(horizon), True
            while left > 0:
                K = min(int(fragment), left)
                out = self._outs[K] = vec.population_rollout(self.pop, K, reset_done=False, out=self._outs.get(K))
                if first:
                    self.rollout_kernel = vec.sim.last_kernel
                self.fitness(out[3], out[4], accumulate=not first)
                left -= K
                first = False
        finally:
            self.policy.greedy = greedy
        self.direction_weights()
        self.gradient()
        if self.mode == "es":
            self.adam()
        self.gen += 1
        return self.stats

    # ---- checkpoints ----------------------------------------------------------------------------------------------
    def state_dict(self):
        """Plain CPU tensors and numbers: theta, Adam's ``m`` / ``v`` / ``state``, the generation counter and the noise
        seed.  Synchronises the device.  The environments are not the learner's: their noise streams and the generator
        that draws ring lengths run on across the generations' resets, so an exact resume also takes
        ``vec.snapshot().state_dict()`` / ``vec.load_snapshot``."""
        return {"theta": self.theta.detach().cpu().clone(), "m": self.m.cpu().clone(), "v": self.v.cpu().clone(),
                "state": self.state.cpu().clone(), "generation": int(self.gen), "noise_seed": int(self.noise_seed),
                "mode": self.mode, "pairs": self.N, "eval_members": self.E}

    def load_state_dict(self, sd):
        """Copies a ``state_dict()`` into the buffers IN PLACE (theta is the policy's buffer)."""
        if tuple(sd["theta"].shape) != (self.P,):
            raise ValueError("DeviceES.load_state_dict: theta has %s values, this policy %d" % (tuple(sd["theta"].shape), self.P))
        with self.torch.no_grad():
            self.theta.copy_(sd["theta"])
            self.m.copy_(sd["m"])
            self.v.copy_(sd["v"])
            self.state.copy_(sd["state"])
        self.gen, self.noise_seed = int(sd["generation"]), int(sd["noise_seed"])

