"""train_vec.py -- a minimal on-device PPO loop over VecFlowEnv (the GPU counterpart of the reference's
examples/train.py:110-212, where RLlib rollout workers each drive one SUMO process).

    python examples/train_vec.py --replicas 1024 --iterations 20
    python examples/train_vec.py --replicas 4096 --gpus 8        # data-parallel: one process per GPU (RCCL)

Environment: the reference's single-agent ring experiment (examples/exp_configs/rl/singleagent/singleagent_ring.py:
WaveAttenuationPOEnv, 21 IDM humans + 1 RL vehicle on a 230..270 m ring).  A rollout fragment of K steps -- policy
forward, action sampling, Env.step of every replica, reset of finished episodes -- is ONE replay of a captured HIP
graph (VecFlowEnv.capture); observations, actions, rewards and the PPO update all stay in HBM.

--gpus N (the reference's num_workers / ray.init(num_cpus), examples/train.py:149,195): N child processes, one per GPU,
started BEFORE anything touches a GPU; rank r steps the replica block shard_range(R, r, N) (VecFlowEnv(replica_offset=):
the Philox streams are keyed by the global replica id, so the trajectories do not depend on N); the policy is replicated
and every PPO step all-reduces the flat gradient and the advantage statistics over RCCL (flow_amd/dist.py).  The update
is written over SHARDS (ppo_update): a rank holds one, and a single process holding all of them -- gradients accumulated
shard by shard -- makes the same update, which is what tests/test_train_dist_gloo.py checks bit for bit.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn as nn


def ring_flow_params(horizon):
    from flow_amd.controllers import ContinuousRouter, IDMController, RLController
    from flow_amd.core.params import EnvParams, InitialConfig, NetParams, SumoParams, VehicleParams
    from flow_amd.envs import WaveAttenuationPOEnv
    from flow_amd.networks import RingNetwork
    veh = VehicleParams()
    veh.add(veh_id="human", acceleration_controller=(IDMController, {"noise": 0.2}),
            routing_controller=(ContinuousRouter, {}), num_vehicles=21)
    veh.add(veh_id="rl", acceleration_controller=(RLController, {}), routing_controller=(ContinuousRouter, {}),
            num_vehicles=1)
    return dict(exp_tag="stabilizing_the_ring", env_name=WaveAttenuationPOEnv, network=RingNetwork, simulator="traci",
                sim=SumoParams(sim_step=0.1, render=False, seed=3),
                env=EnvParams(horizon=horizon, warmup_steps=0,
                              additional_params={"max_accel": 1, "max_decel": 1, "ring_length": None}),
                net=NetParams(additional_params={"length": 260, "lanes": 1, "speed_limit": 30, "resolution": 40}),
                veh=veh, initial=InitialConfig(bunching=20))


class GaussianPolicy(nn.Module):
    """``net_log_std`` (RLlib's default model, ``free_log_std: false`` -- what the reference trains): the last layer of
    ``self.mu`` has ``2 * act_dim`` outputs, the means and then the log stds (RLlib's DiagGaussian order, DevicePolicy's),
    so the standard deviation depends on the observation, and there is no ``log_std`` parameter.  The log-std rows start
    with zero weights and bias -0.5: the first rollout samples as the free form does at its start."""

    def __init__(self, obs_dim, act_dim, hidden=32, net_log_std=False):
        super().__init__()
        self.net_log_std, self.act_dim = bool(net_log_std), act_dim
        self.mu = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, 2 * act_dim if net_log_std else act_dim))
        self.value = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                   nn.Linear(hidden, 1))
        if net_log_std:
            with torch.no_grad():
                self.mu[4].weight[act_dim:].zero_()
                self.mu[4].bias[act_dim:].fill_(-0.5)
        else:
            self.log_std = nn.Parameter(torch.full((act_dim,), -0.5))

    def _dist(self, obs):
        """(means, log stds) [n, A] of the head of 2 A outputs."""
        out = self.mu(obs)
        return out[..., :self.act_dim], out[..., self.act_dim:]

    def act(self, obs, explore=True):         # what the captured graph runs every step
        """A sample of the action distribution; ``explore=False``: its mean (evaluation without exploration noise)."""
        with torch.no_grad():
            if self.net_log_std:
                mu, ls = self._dist(obs)
                return mu + torch.randn_like(mu) * ls.exp() if explore else mu
            mu = self.mu(obs)
            return mu + torch.randn_like(mu) * self.log_std.exp() if explore else mu

    def logp_value(self, obs, act):
        if self.net_log_std:
            return self.logp_value_dist(obs, act)[:2]
        mu = self.mu(obs)
        std = self.log_std.exp()
        logp = (-0.5 * ((act - mu) / std) ** 2 - self.log_std - 0.9189385).sum(-1)
        return logp, self.value(obs).squeeze(-1)

    def logp_value_dist(self, obs, act):
        """``logp_value`` and the distribution itself: (logp, value, means [n, A], log_std [A]) -- what the KL term of
        ppo_update keeps from its no_grad pass.  ``net_log_std``: the log stds are per sample, [n, A]."""
        if self.net_log_std:
            mu, ls = self._dist(obs)
            logp = (-0.5 * ((act - mu) / ls.exp()) ** 2 - ls - 0.9189385).sum(-1)
            return logp, self.value(obs).squeeze(-1), mu, ls
        mu = self.mu(obs)
        std = self.log_std.exp()
        logp = (-0.5 * ((act - mu) / std) ** 2 - self.log_std - 0.9189385).sum(-1)
        return logp, self.value(obs).squeeze(-1), mu, self.log_std


class AdaptiveKL(object):
    """RLlib's adaptive KL coefficient (``kl_coeff``, ``kl_target``): ``coef`` weighs KL(old || new) in ppo_update's loss
    and is adapted once per update, after the last epoch, from the mean KL that epoch's gradient pass saw (before its
    optimiser step): times 1.5 above ``2 target``, times 0.5 below ``0.5 target``."""

    def __init__(self, target=0.02, coef=0.2):
        self.target, self.coef, self.mean_kl = float(target), float(coef), None

    def adapt(self, mean_kl):
        self.mean_kl = float(mean_kl)
        if self.mean_kl > 2.0 * self.target:
            self.coef *= 1.5
        elif self.mean_kl < 0.5 * self.target:
            self.coef *= 0.5
        return self.coef


def gae(rew, val, done, last_val, gamma=0.999, lam=0.97):
    """Generalised advantage estimation over a [K, R] fragment.  ``done`` is the simulator's FLAG BYTE (bit 0: horizon
    reached, bit 1: collision -- include/flowsim.h), so "the episode went on" is ``done == 0``, not ``1 - done``."""
    K = rew.shape[0]
    adv = torch.zeros_like(rew)
    run = torch.zeros_like(last_val)
    nxt = last_val
    for t in range(K - 1, -1, -1):
        live = (done[t] == 0).float()
        delta = rew[t] + gamma * nxt * live - val[t]
        run = delta + gamma * lam * live * run
        adv[t] = run
        nxt = val[t]
    return adv, adv + val


def ppo_update(pi, opt, shards, epochs=4, clip=0.2, group=None, learner=None, kl=None, entropy_coef=0.0, vf_clip=None,
               vf_coef=0.5, minibatch=None, shuffle_seed=0, epoch0=0):
    """One PPO update over `shards` = [(obs [K+1, R, D], act [K, R, A], rew [K, R], done [K, R])]: the shards this
    process holds (one per rank in data-parallel runs, all of them in a single process).  Every quantity that couples the
    shards is a SUM: the advantage statistics and the gradient -- summed over the local shards here, over the ranks by
    allreduce_sum / allreduce_gradients -- so N ranks with one shard each and one process with N shards agree.
    A sample whose action is NaN is an agent that was absent (the multi-agent merge's fused rollout: its RL slot held no
    vehicle): it is left out of the advantage statistics and the loss, and its action is never read.
    ``learner`` (flow_amd.utils.device_ppo.DeviceLearner over pi's parameters): the three torch stages -- the no_grad pass,
    gae() and every epoch's forward and backward pass -- run on the library's kernels instead (fs_ppo_eval_dev, fs_gae_dev,
    fs_ppo_grad_dev); the float64 advantage statistics, the all-reduces and opt.step() are the same code.  Without one, the
    update is torch alone.
    ``kl`` (an AdaptiveKL), ``entropy_coef``, ``vf_clip``: the loss the reference trains with (RLlib's PPO), per present
    sample and over the global count n
        -pg + kl.coef KL(old || new) + vf_coef max((v - ret)^2, (v_c - ret)^2) - entropy_coef H
        KL = sum_c ls - ls_o + (exp(2 ls_o) + (mu_o - mu)^2) / (2 exp(2 ls)) - 0.5,   H = sum_c ls + 0.5 log(2 pi e)
        v_c = v_o + clamp(v - v_o, -vf_clip, +vf_clip)
    with mu_o, ls_o, v_o from the no_grad pass (``pi.logp_value_dist``).  ``vf_clip`` None or inf: vfl = (v - ret)^2.
    A policy whose log stds come from the network (``GaussianPolicy(net_log_std=True)``) hands over ls and ls_o per sample,
    [n, A]: the same formulas, H = sum_c ls[s, c] + 0.5 log(2 pi e) per sample.
    After the last epoch ``kl.adapt`` sees that epoch's mean KL (summed over shards and ranks).  With a learner the same
    loss runs on fs_ppo_eval_dist_dev / fs_ppo_grad_loss_dev.  With the defaults the arithmetic is what it was.
    ``minibatch`` (RLlib's ``sgd_minibatch_size``, a per-shard size B; None: everything above): an epoch is a shuffled
    pass of minibatch steps, the way RLlib's do_minibatch_sgd makes ``num_sgd_iter`` passes (_ppo_epochs_minibatch states
    the semantics; it is the definition DeviceLearner.update(minibatch=) is tested against).  Epoch e of this call draws
    ``epoch_permutation(shuffle_seed, epoch0 + e, n)``.  With a ``learner`` (the --device_update path, torch's Adam) this is
    not built: use --device_adam, where the whole step is one launch."""
    from flow_amd.dist import allreduce_gradients, allreduce_sum
    if learner is not None and getattr(learner, "net_log_std", False):
        raise NotImplementedError("ppo_update(learner=...) with the 2A-output head (net_log_std): the gradient around torch's "
                                  "Adam (--device_update, fs_ppo_grad_dev) is not built for it; --device_adam runs the whole "
                                  "update on the device (DeviceLearner.update)")
    if minibatch is not None and learner is not None:
        raise NotImplementedError("ppo_update(learner=..., minibatch=...): minibatch steps around torch's Adam (--device_update) "
                                  "are not built; --device_adam runs them on the device (DeviceLearner.update(minibatch=))")
    vclip = vf_clip is not None and 0.0 < float(vf_clip) < float("inf")
    full = kl is not None or vclip or float(entropy_coef) != 0.0
    prepared, stats = [], None
    if learner is not None:
        learner.sync()
    for obs, act, rew, done in shards:
        K, R = rew.shape
        o, a = obs[:K].reshape(K * R, -1), act.reshape(K * R, -1)
        present = ~torch.isnan(a).any(-1)
        if bool(present.all()):
            present = None                                   # (every sample present: the plain sums)
        elif learner is None:
            a = torch.where(present[:, None], a, torch.zeros_like(a))
        with torch.no_grad():
            mu_old = ls_old = None
            if learner is not None and full:
                logp_old, val, mu_old = learner.evaluate_dist(o, a)
                ls_old = learner.log_std_param.detach().clone()
                last_val = learner.evaluate(obs[K], None)[1]
                adv, ret = learner.gae(rew, val.view(K, R), last_val, done)
            elif learner is not None:                        # (the kernels take the NaN rows as they are: absent)
                logp_old, val = learner.evaluate(o, a)
                last_val = learner.evaluate(obs[K], None)[1]
                adv, ret = learner.gae(rew, val.view(K, R), last_val, done)
            else:
                if full:
                    logp_old, val, mu_old, ls_old = pi.logp_value_dist(o, a)
                    mu_old, ls_old = mu_old.detach().clone(), ls_old.detach().clone()
                else:
                    logp_old, val = pi.logp_value(o, a)
                last_val = pi.value(obs[K]).squeeze(-1)
                adv, ret = gae(rew, val.view(K, R), done, last_val)
            adv = adv.reshape(-1).double()
            if present is None:
                st = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(adv.numel()), dtype=torch.float64, device=adv.device)])
            else:
                m = present.double()
                st = torch.stack([(adv * m).sum(), (adv * adv * m).sum(), m.sum()])
            stats = st if stats is None else stats + st
        prepared.append((o, a, logp_old, adv, ret.reshape(-1), present) + ((val.reshape(-1), mu_old, ls_old) if full else ()))
    stats = allreduce_sum(stats, group)
    n = stats[2]
    mean = stats[0] / n
    std = ((stats[1] - n * mean * mean) / (n - 1)).clamp_min(0).sqrt()
    params = list(pi.parameters())
    if minibatch is not None:
        _ppo_epochs_minibatch(pi, opt, prepared, params, epochs, clip, group, kl, float(entropy_coef),
                              float(vf_clip) if vclip else None, vf_coef, mean, std, n, full, int(minibatch), shuffle_seed,
                              epoch0)
        return
    if full:
        _ppo_epochs_full(pi, opt, prepared, params, epochs, clip, group, learner, kl, float(entropy_coef),
                         float(vf_clip) if vclip else None, vf_coef, mean, std, n)
        return
    for _ in range(epochs):
        if learner is not None:
            # one launch per shard writes (the first shard) or adds to (the others, in this order) the packed gradient
            # that every parameter's .grad is a view of
            for j, (o, a, logp_old, adv, ret, present) in enumerate(prepared):
                learner.gradients(o, a, logp_old, adv, ret, mean, std, clip=clip, vf_coef=vf_coef, n_total=float(n),
                                  accumulate=j > 0)
            learner.attach_grads()
        else:
            opt.zero_grad()
            for o, a, logp_old, adv, ret, present in prepared:
                adv_n = ((adv - mean) / (std + 1e-8)).float()
                logp, v = pi.logp_value(o, a)
                ratio = (logp - logp_old).exp()
                pg = torch.min(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n)
                vf = (v - ret).pow(2)
                if present is not None:
                    pg = torch.where(present, pg, torch.zeros_like(pg))
                    vf = torch.where(present, vf, torch.zeros_like(vf))
                # the GLOBAL mean as a sum of per-shard sums
                loss = (-pg.sum() + vf_coef * vf.sum()) / float(n)
                loss.backward()                              # (accumulates over the local shards)
        allreduce_gradients(params, group)
        opt.step()
        if learner is not None:
            learner.sync()                                   # the optimiser moved the weights: repack them for the kernels


def _entropy(ls):
    """H of the diagonal Gaussian: sum_c ls + 0.5 log(2 pi e) -- one number for the free log_std [A], one per sample for
    log stds from the network [n, A]."""
    import math
    h = ls + 0.5 * math.log(2.0 * math.pi * math.e)
    return h.sum() if ls.dim() == 1 else h.sum(-1)


def _ppo_epochs_full(pi, opt, prepared, params, epochs, clip, group, learner, kl, entropy_coef, vf_clip, vf_coef, mean, std, n):
    """The epochs of ppo_update with the reference's loss terms on (its docstring states the loss)."""
    from flow_amd.dist import allreduce_gradients, allreduce_sum
    sum_kl = None
    if learner is not None:
        mean_std_n = torch.stack([mean, std, n]).to(torch.float64)
        if kl is not None:
            learner.kl_state[0].fill_(kl.coef)
    for _ in range(epochs):
        if learner is not None:
            for j, (o, a, logp_old, adv, ret, present, v_old, mu_old, ls_old) in enumerate(prepared):
                learner.gradients_loss(o, a, logp_old, adv, ret, mean_std_n, mean_old=mu_old, log_std_old=ls_old, val_old=v_old,
                                       clip=clip, vf_coef=vf_coef, vf_clip=vf_clip, entropy_coef=entropy_coef,
                                       kl=kl is not None, accumulate=j > 0)
            learner.attach_grads()
            sum_kl = learner.loss_sums[2].double()
        else:
            opt.zero_grad()
            sum_kl = None
            for o, a, logp_old, adv, ret, present, v_old, mu_old, ls_old in prepared:
                adv_n = ((adv - mean) / (std + 1e-8)).float()
                logp, v, mu, ls = pi.logp_value_dist(o, a)
                ratio = (logp - logp_old).exp()
                per = -torch.min(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n)
                vfl = (v - ret).pow(2)
                if vf_clip is not None:
                    v_c = v_old + (v - v_old).clamp(-vf_clip, vf_clip)
                    vfl = torch.max(vfl, (v_c - ret).pow(2))
                per = per + vf_coef * vfl
                if kl is not None:
                    kl_s = (ls - ls_old + ((2.0 * ls_old).exp() + (mu_old - mu).pow(2)) / (2.0 * (2.0 * ls).exp()) - 0.5).sum(-1)
                    per = per + kl.coef * kl_s
                    shard_kl = (kl_s.detach() if present is None else torch.where(present, kl_s.detach(), torch.zeros_like(kl_s))).sum()
                    sum_kl = shard_kl if sum_kl is None else sum_kl + shard_kl
                if entropy_coef != 0.0:
                    per = per - entropy_coef * _entropy(ls)
                if present is not None:
                    per = torch.where(present, per, torch.zeros_like(per))
                # the GLOBAL mean as a sum of per-shard sums
                (per.sum() / float(n)).backward()            # (accumulates over the local shards)
        allreduce_gradients(params, group)
        opt.step()
        if learner is not None:
            learner.sync()
    if kl is not None:
        kl.adapt(float(allreduce_sum(sum_kl.double().reshape(1), group)[0]) / float(n))


def _ppo_epochs_minibatch(pi, opt, prepared, params, epochs, clip, group, kl, entropy_coef, vf_clip, vf_coef, mean, std, n, full,
                          B, shuffle_seed, epoch0):
    """The epochs of ppo_update as shuffled passes of minibatch steps -- the definition of ``minibatch=B``:
    * the advantages stay standardised by (mean, std) of the WHOLE batch, and logp_old, mu_old, ls_old, v_old by the one
      no_grad pass before the first epoch; kl.coef stays constant through the update;
    * epoch e permutes a shard's n rows with perm = epoch_permutation(shuffle_seed, epoch0 + e, n); minibatch k is rows
      perm[kB : (k + 1)B] (the last one kept when it is short), ceil(n / B) steps per epoch in ascending k; with several
      shards (of equal n: ValueError otherwise) step k takes those rows of EVERY shard;
    * one step: ppo_update's loss (the terms on or off) summed over the minibatch's present rows of all shards and ranks,
      divided by THEIR count c -- not by n --, its gradient, one optimiser step; c == 0: no step at all;
    * after the last epoch kl.adapt sees (the sum of that epoch's minibatches' per-sample KL, each evaluated before its
      own step) / n."""
    from flow_amd.dist import allreduce_gradients, allreduce_sum
    from flow_amd.utils.device_ppo import epoch_permutation
    sizes = sorted(set(int(p[0].shape[0]) for p in prepared))
    if len(sizes) != 1:
        raise ValueError("ppo_update(minibatch=): the shards must hold the same number of samples (got %s)" % sizes)
    n_rows = sizes[0]
    if B < 1:
        raise ValueError("ppo_update(minibatch=): the minibatch size must be at least 1 (got %d)" % B)
    sum_kl = None
    for e in range(epochs):
        perm = torch.as_tensor(epoch_permutation(shuffle_seed, epoch0 + e, n_rows), device=prepared[0][0].device)
        sum_kl = torch.zeros((), dtype=torch.float64, device=prepared[0][0].device)
        for k in range(-(-n_rows // B)):
            idx = perm[k * B:(k + 1) * B]
            opt.zero_grad()
            total, count = None, 0.0
            for shard in prepared:
                o, a, logp_old, adv, ret, present = (None if t is None else t[idx] for t in shard[:6])
                adv_n = ((adv - mean) / (std + 1e-8)).float()
                if full:
                    v_old, mu_old, ls_old = shard[6][idx], shard[7][idx], shard[8]
                    if ls_old.dim() > 1:                     # (log stds from the network: per sample)
                        ls_old = ls_old[idx]
                    logp, v, mu, ls = pi.logp_value_dist(o, a)
                else:
                    logp, v = pi.logp_value(o, a)
                ratio = (logp - logp_old).exp()
                per = -torch.min(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n)
                vfl = (v - ret).pow(2)
                if vf_clip is not None:
                    v_c = v_old + (v - v_old).clamp(-vf_clip, vf_clip)
                    vfl = torch.max(vfl, (v_c - ret).pow(2))
                per = per + vf_coef * vfl
                if kl is not None:
                    kl_s = (ls - ls_old + ((2.0 * ls_old).exp() + (mu_old - mu).pow(2)) / (2.0 * (2.0 * ls).exp()) - 0.5).sum(-1)
                    per = per + kl.coef * kl_s
                    kl_d = kl_s.detach()
                    sum_kl = sum_kl + (kl_d if present is None else torch.where(present, kl_d, torch.zeros_like(kl_d))).sum().double()
                if entropy_coef != 0.0:
                    per = per - entropy_coef * _entropy(ls)
                if present is not None:
                    per = torch.where(present, per, torch.zeros_like(per))
                total = per.sum() if total is None else total + per.sum()
                count += float(idx.numel()) if present is None else float(present.sum())
            count = float(allreduce_sum(torch.tensor([count], dtype=torch.float64, device=idx.device), group)[0])
            if count == 0.0:
                continue                                     # (nobody present: no step, the optimiser's state untouched)
            (total / count).backward()                       # the minibatch's own mean, as a sum of per-shard sums
            allreduce_gradients(params, group)
            opt.step()
    if kl is not None and sum_kl is not None:                # (no epoch: no KL was seen, the coefficient stays)
        kl.adapt(float(allreduce_sum(sum_kl.reshape(1), group)[0]) / float(n))


def model_descriptor(pi):
    """``(obs_dim, act_dim, num_hidden, net_log_std)`` of a GaussianPolicy: DeviceLearner.descriptor()'s tuple."""
    return (int(pi.mu[0].in_features), int(pi.act_dim), sum(isinstance(m, nn.Linear) for m in pi.mu) - 1, bool(pi.net_log_std))


def policy_state(pi, opt=None, kl=None, learner=None):
    """What one policy carries from one update to the next, as plain CPU tensors and numbers.  ``learner`` with
    ``device_adam`` (no ``opt``): ``DeviceLearner.state_dict()`` -- packed weights, Adam's m / v / {t, beta1^t, beta2^t},
    the KL state, the minibatch epoch counter.  Otherwise (torch, --device_update): ``opt.state_dict()`` and AdaptiveKL's
    two numbers.  ``pi.state_dict()`` is kept on every path: the model alone can be loaded anywhere."""
    cpu = lambda v: v.detach().to("cpu").clone() if torch.is_tensor(v) else v     # noqa: E731
    out = dict(descriptor=list(model_descriptor(pi)), pi={k: cpu(v) for k, v in pi.state_dict().items()})
    if learner is not None and opt is None:
        out["learner"] = learner.state_dict()
    else:
        sd = opt.state_dict()
        out["opt"] = dict(state={k: {n: cpu(v) for n, v in st.items()} for k, st in sd["state"].items()},
                          param_groups=sd["param_groups"])
        out["kl"] = None if kl is None else [float(kl.coef), None if kl.mean_kl is None else float(kl.mean_kl)]
    return out


def restore_policy(entry, pi, opt=None, kl=None, learner=None, log=print, name="policy", model_only=False):
    """Load ``entry`` (a ``policy_state``) in place: the model always; the optimiser state, the KL coefficient and the
    epoch counter where the checkpoint was written on THIS update path (``learner`` without ``opt``: device_adam;
    ``opt``: torch's Adam, with or without the device update) -- onto another path the log says that they were dropped.
    ``model_only`` (evaluation): nothing but the model is wanted.  A model of another shape is refused by name."""
    from flow_amd.utils.device_ppo import check_descriptor
    check_descriptor("restore_policy (%s)" % name, entry["descriptor"], model_descriptor(pi))
    device_adam = learner is not None and opt is None
    if device_adam and "learner" in entry and not model_only:
        learner.load_state_dict(entry["learner"])            # (in place: pi's adopted parameters are views of it)
        return True
    with torch.no_grad():
        pi.load_state_dict(entry["pi"])                       # (copies in place: adopted views stay views)
    if learner is not None:
        learner.sync()
    if model_only:
        return False
    if opt is not None and "opt" in entry:
        opt.load_state_dict(entry["opt"])
        if kl is not None and entry.get("kl") is not None:
            kl.coef, kl.mean_kl = entry["kl"][0], entry["kl"][1]
        return True
    log("restore: %s: the checkpoint was written on another update path (%s): the model is loaded, the optimiser state, "
        "the KL coefficient and the epoch counter were dropped" % (name, "device_adam" if "learner" in entry else "torch Adam"))
    return False


def save_checkpoint(directory, iteration, flow_params, policies, seed=0, update_path="torch", model=None, env=None):
    """``directory/checkpoint_<iteration>/``: ``state.pt`` -- a ``torch.save`` of plain tensors and numbers:
    ``policies`` ({name: policy_state(...)}: one entry, 'av', or the adversarial trainer's two), ``iteration``, ``seed``,
    ``update_path`` ('torch', 'device_update' or 'device_adam') and ``model`` (how the trainer was called: shared_agents,
    fuse_action_vector, adversarial) -- and ``params.json``, the flow params through FlowParamsEncoder, as the reference
    puts next to its checkpoints.  ``env`` (``env_state``: --checkpoint_env_state) adds the entry ``env``, the environments'
    state; without it the file is what it was.  Returns the checkpoint's path."""
    import json
    from flow_amd.utils.rllib import FlowParamsEncoder
    path = os.path.join(str(directory), "checkpoint_%d" % int(iteration))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "params.json"), "w") as f:
        json.dump(flow_params, f, cls=FlowParamsEncoder, sort_keys=True, indent=4)
    state = dict(iteration=int(iteration), seed=int(seed), update_path=str(update_path), model=dict(model or {}),
                 policies=policies)
    if env is not None:
        state["env"] = env
    torch.save(state, os.path.join(path, "state.pt"))
    return path


def env_state(vec, graph=None, torch_sampling=False, world=1):
    """The ``env`` entry of a checkpoint (--checkpoint_env_state): ``VecFlowEnv.snapshot().state_dict()`` -- the simulator's
    host blob, the observation, the generator that draws ring lengths and inflows, the episode-statistics carries --, the
    rollout graph's carry where there is a graph, and torch's CUDA generator state where the graph samples from it (the
    torch module's ``pi.act``) -- and ``handle_seed``, the Philox key of the handle: a constant of the handle, not part of its
    state, which an experiment with ``SumoParams(seed=None)`` draws anew per process (``checkpoint_handle_seed``).  Plain
    tensors, ints and strings: ``load_checkpoint`` reads it with ``weights_only=True``."""
    out = dict(snapshot=vec.snapshot().state_dict(), world=int(world), handle_seed=int(vec.env._spec["seed"]))
    if graph is not None:
        out["carry"] = graph.carry().cpu()
    if torch_sampling:
        out["torch_cuda_rng"] = torch.cuda.get_rng_state(vec.device).clone()
    return out


def checkpoint_handle_seed(ck):
    """The handle seed the environments of checkpoint ``ck`` ran on (None: the checkpoint holds no environment state): the
    trainer creates its ``VecFlowEnv`` with it, so that the continued Philox streams are the interrupted run's."""
    env = None if ck is None else ck.get("env")
    return None if env is None or "handle_seed" not in env else int(env["handle_seed"])


def restore_env_state(entry, vec, graph=None, torch_sampling=False, world=1, log=print):
    """Continue the environments of a checkpoint instead of starting them from a reset: True if done.  An entry of another
    layout (another --replicas, another experiment) or of a data-parallel run is not an error: the log names the
    difference and the caller's reset stands."""
    if entry is None:
        log("restore: the checkpoint holds no environment state (written without --checkpoint_env_state): the environments "
            "start from a reset, the sampling streams from their seeds")
        return False
    snap = entry["snapshot"]
    here = int(vec.sim.snapshot_info().layout)
    if world > 1 or int(entry.get("world", 1)) > 1:
        log("restore: the checkpoint's environment state is one rank's shard (data-parallel runs keep rank 0's only): the "
            "environments start from a reset")
        return False
    if int(snap["layout"]) != here or (graph is not None) != ("carry" in entry):
        log("restore: the checkpoint's environment state has another layout (%s; this run: %s%s): the environments start from "
            "a reset, the sampling streams from their seeds"
            % (snap.get("shape", "?"), vec._shape_tag(), "" if (graph is not None) == ("carry" in entry) else "; another rollout path"))
        return False
    vec.load_snapshot(snap)
    if graph is not None:
        graph.set_carry(entry["carry"])
    if torch_sampling and "torch_cuda_rng" in entry:
        torch.cuda.set_rng_state(entry["torch_cuda_rng"], vec.device)
    log("restore: the environments continue from the checkpoint's state (simulator, draw counters, observation%s)"
        % ("; the torch-sampled graph: torch's CUDA generator state too" if torch_sampling else ""))
    return True


def load_checkpoint(path):
    """What ``save_checkpoint`` wrote at ``path`` (a ``checkpoint_<iteration>`` directory): the dict of ``state.pt`` with
    ``flow_params`` (``params.json`` through ``get_flow_params``) next to it."""
    from flow_amd.utils.rllib import get_flow_params
    state = torch.load(os.path.join(str(path), "state.pt"), map_location="cpu", weights_only=True)
    state["flow_params"] = get_flow_params(os.path.join(str(path), "params.json"))
    return state


def add_checkpoint_flags(ap):
    """Checkpoints and the episode statistics of the log (train_vec.py and train.py), all off by default."""
    ap.add_argument("--checkpoint_dir", type=str, default=None,
                    help="write checkpoint_<iteration>/ (state.pt, params.json) here every --checkpoint_freq iterations and at the end")
    ap.add_argument("--checkpoint_freq", type=int, default=None, help="iterations between checkpoints (with --checkpoint_dir)")
    ap.add_argument("--restore", type=str, default=None,
                    help="a checkpoint_<iteration> directory: continue at iteration + 1 with its weights, optimiser state, KL "
                         "coefficient and epoch counter (the environments start from a reset, the sampling streams from their seeds, "
                         "unless the checkpoint was written with --checkpoint_env_state: then they continue)")
    ap.add_argument("--checkpoint_env_state", action="store_true",
                    help="checkpoints also hold the environments' state (VecFlowEnv.snapshot: simulator, Philox counters, "
                         "observation, the rollout graph's carry); --restore of such a checkpoint continues the environments "
                         "instead of resetting them: where the library draws the samples, the run is the uninterrupted run's "
                         "bit for bit")
    ap.add_argument("--evaluation_interval", type=int, default=None,
                    help="after every N-th update, evaluate the MEAN action for --evaluation_steps steps on the trainer's own "
                         "handle, inside a snapshot / restore bracket (training is bit for bit what it is without); the "
                         "iteration line gains evaluation/episode_reward_mean|min|max, evaluation/episode_len_mean, "
                         "evaluation/episodes")
    ap.add_argument("--evaluation_steps", type=int, default=None, help="steps per evaluation (default: the experiment's horizon)")
    ap.add_argument("--episode_stats", action="store_true",
                    help="append RLlib's episode_reward_mean / min / max, episode_len_mean and episodes (of the episodes that "
                         "ended in the iteration's fragment) to the iteration line (k_episode_stats)")


def _checkpoint_due(it, last, freq):
    return it == last or (freq is not None and freq > 0 and (it + 1) % freq == 0)


def choose_rollout(vec, pi, fragment, seed, log, shared_agents=False, fuse_action_vector=False, learner=None, world=1,
                   rank=0, greedy=False, fuse_shared_agents=False):
    """How a fragment of ``fragment`` closed-loop steps runs for this environment and model -- train_on_device's choice,
    which examples/evaluate.py shares: ``(fused, graph, graph_policy)``, exactly one of ``fused`` (a DevicePolicy for
    ``vec.policy_rollout``) and ``graph`` (a StepGraph, begun after a reset) set.  ``learner``: a DeviceLearner whose
    buffer a DevicePolicy shares (device_adam).  ``greedy``: the mean action instead of a sample -- ``fs_policy.greedy`` in
    the kernels, ``pi.act(obs, explore=False)`` around the torch module.  ``fuse_shared_agents``: shared agents on a head
    without a fused kernel (a CompiledEnv with OBSERVE = "rl") take the graph around the eager policy kernel too."""
    n_ag = vec.act_dim if shared_agents else 1
    k_ag = vec.obs_dim // n_ag
    free_log_std = None if pi.net_log_std else pi.log_std
    device_adam = learner is not None
    # the rollout: ONE kernel per fragment where the library has the fused policy + step form for this experiment and
    # model (fs_policy_rollout_dev: rings / the figure eight with one RL vehicle, the multi-agent ring, figure eight and
    # merge -- its actions applied -- with their agents sharing the policy, 1..3 hidden layers of 32 tanh units);
    # otherwise K single steps around the torch policy captured as one HIP graph.  (Shared agents: the network's input is
    # one agent's block, k_ag values; on the merge an agent whose RL slot is empty has a NaN action, which ppo_update
    # leaves out.)
    fused, graph, graph_policy = None, None, None
    shared = "; one policy shared by %d agents per replica" % n_ag if shared_agents else ""
    try:
        from flow_amd.utils.device_policy import DevicePolicy
        if fuse_action_vector and not shared_agents:
            fused = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=free_log_std, seed=seed, act_dim=vec.act_dim, greedy=greedy)
        else:
            fused = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=free_log_std, seed=seed, greedy=greedy)
        if device_adam:
            fused.share(learner)                               # the rollout kernels read the buffer the learner's Adam writes
        vec.reset()
        vec.policy_rollout(fused, 1, reset_done=True)           # (probe: raises NotImplementedError when not built)
        kernel = vec.sim.last_kernel
        vec.reset()
        log("rollout: fused policy + step kernel (%s)%s" % (kernel, shared))
    except NotImplementedError as e:
        why = e
        in_graph = (fuse_action_vector and not shared_agents) or (fuse_shared_agents and shared_agents)
        graph_policy, fused = (fused if in_graph else None), None
        if graph_policy is not None:
            # no fused kernel for this head (BottleneckDesiredVelocityEnv, a CompiledEnv): the library's eager policy kernel, where it is
            # built, goes into the captured fragment in the torch module's place -- one launch per step instead of ten-odd
            try:
                vec.reset()
                vec.policy_act(graph_policy)                   # (probe)
                kernel = vec.sim.last_kernel
                graph = vec.capture(fragment, policy=graph_policy, reset_done=True)
                graph.begin(vec.reset())
                log("rollout: HIP graph of %d single steps around the policy kernel (%s)" % (fragment, kernel))
            except NotImplementedError:
                graph_policy = None
    if fused is None and graph is None:
        log("rollout: HIP graph of %d single steps around the torch policy (%s)%s" % (fragment, why, shared))
        if world > 1:
            torch.manual_seed(seed + 1000 * (rank + 1))       # the graph's torch.randn: another stream per rank
        R_ = getattr(vec, "num_rows", vec.num_envs)

        def act_shared(obs):                                   # [R, agents * k] -> [R, agents]: every agent its own sample
            return pi.act(obs.view(R_ * n_ag, k_ag), explore=not greedy).view(R_, n_ag)
        graph = vec.capture(fragment, policy=act_shared if shared_agents else (lambda obs: pi.act(obs, explore=not greedy)) if greedy else pi.act,
                            reset_done=True)
        graph.begin(vec.reset())
    return fused, graph, graph_policy


class Evaluator(object):
    """In-training evaluation on the trainer's own handle (train_on_device(evaluation_interval=)): ``run()`` = snapshot,
    reset, S steps of the MEAN action, episode statistics, restore.  The greedy policy or graph is ``choose_rollout(...,
    greedy=True)``'s, built ONCE here inside a bracket of its own (its probe and warm-up steps move the simulator, and the
    torch generator is put back too); a DevicePolicy shares the learner's buffer under device_adam and is repacked from the
    module otherwise.  The statistics use carries of their own, not training's.  ``graphs``: the trainer's StepGraphs -- their
    carries live outside the environment and are left alone."""

    def __init__(self, vec, pi, steps, seed, log, shared_agents=False, fuse_action_vector=False, learner=None, world=1, rank=0,
                 graphs=()):
        self.vec, self.S, self.world = vec, int(steps), world
        dev, R = vec.device, getattr(vec, "num_rows", vec.num_envs)
        rng, rng_host = torch.cuda.get_rng_state(dev), torch.get_rng_state()
        self.snap = vec.snapshot()
        self.fused, self.graph, self.graph_policy = choose_rollout(
            vec, pi, self.S, seed, lambda m: log("evaluation: " + m), shared_agents=shared_agents,
            fuse_action_vector=fuse_action_vector, learner=learner, world=world, rank=rank, greedy=True)
        vec.restore(self.snap)
        torch.cuda.set_rng_state(rng, dev)
        torch.set_rng_state(rng_host)
        self.ret = torch.zeros(R, dtype=torch.float64, device=dev)
        self.len = torch.zeros(R, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(8, dtype=torch.float64, device=dev)
        self.empty = torch.tensor([0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, float("inf"), float("-inf")],
                                  dtype=torch.float64, device=dev)

    def run(self):
        from flow_amd import _lib as L
        from flow_amd.utils import episode_stats as es
        vec, S = self.vec, self.S
        vec.snapshot(out=self.snap)
        obs0 = vec.reset()                                      # every replica evaluates whole episodes
        if self.fused is not None:
            self.fused.sync()
            _, _, _, rew, done = vec.policy_rollout(self.fused, S, reset_done=True)
        else:
            if self.graph_policy is not None:
                self.graph_policy.sync()
            self.graph.begin(obs0)
            _, _, rew, done = self.graph.replay()
        vec.use_current_stream()
        self.ret.zero_()
        self.len.zero_()
        self.stats.copy_(self.empty)
        L.check(vec.sim.lib.fs_episode_stats_dev(vec.sim._h, S, rew.data_ptr(), done.data_ptr(), self.ret.data_ptr(),
                                                 self.len.data_ptr(), self.stats.data_ptr(), 0), vec.sim.lib)
        summary = es.summarize(es.allreduce(self.stats))
        vec.restore(self.snap)
        return summary

    @staticmethod
    def log_suffix(summary):
        if not summary["episodes"]:
            return "  evaluation/episodes 0"
        return ("  evaluation/episode_reward_mean %.4f  evaluation/episode_reward_min %.4f  evaluation/episode_reward_max %.4f"
                "  evaluation/episode_len_mean %.1f  evaluation/episodes %d"
                % (summary["episode_reward_mean"], summary["episode_reward_min"], summary["episode_reward_max"],
                   summary["episode_len_mean"], summary["episodes"]))


def train_on_device(flow_params, replicas=1024, fragment=100, iterations=20, epochs=4, lr=3e-4, seed=0, log=print,
                    rank=0, world=1, shared_agents=False, fuse_action_vector=False, fuse_shared_agents=False,
                    device_update=False, device_adam=False,
                    kl_target=None, kl_coeff=0.2, entropy_coeff=0.0, vf_clip=None, vf_coef=0.5, clip=0.2,
                    sgd_minibatch_size=None, net_log_std=False, checkpoint_dir=None, checkpoint_freq=None, restore=None,
                    episode_stats=False, on_episodes=None, checkpoint_env_state=False, evaluation_interval=None,
                    evaluation_steps=None, on_evaluation=None):
    """PPO on R replicas of ``flow_params`` with everything in HBM: returns the mean step reward per iteration.
    ``world`` > 1: this process is rank ``rank`` of a data-parallel run (torch.distributed is initialised): it steps its
    block of the R replicas on its own GPU.
    ``shared_agents``: a multi-agent experiment whose agents share ONE policy (the reference's multi-agent ring /
    figure-eight / merge experiments map every agent to the policy 'av': examples/exp_configs/rl/multiagent/*.py
    policy_mapping_fn): the observation row holds one block per agent, the action row one column per agent; every agent
    is a sample of the shared policy and receives the shared reward.
    ``fuse_action_vector``: an experiment whose ONE network emits several action columns (MergePOEnv:
    singleagent_merge.py) rolls out through the fused policy + step kernel as well (k_merge_policy<PO>; with more than six
    places, EXP_NUM 1 and 2, k_merge_policy<PO,WIDE>); where no fused
    kernel exists but the eager policy kernel does (BottleneckDesiredVelocityEnv: singleagent_bottleneck.py,
    k_policy_act_wide), the captured graph holds that kernel instead of the torch module.  Off by default: the library's
    kernels draw their samples from its Philox streams, the torch policy from torch.randn, so the two are different
    (equally valid) trajectories.
    ``fuse_shared_agents``: the same for shared agents on a head without a fused kernel (a flow_amd.envs.CompiledEnv with
    OBSERVE = "rl": compiled_highway_ring.py): the captured graph holds k_policy_act, which runs the replica's agents
    through the shared policy, instead of the torch module.  Off by default.
    ``device_update``: the PPO update runs on the library's kernels (DeviceLearner: fs_ppo_eval_dev, fs_gae_dev,
    fs_ppo_grad_dev) instead of torch forward passes, the Python loop of gae() and autograd.  Off by default.
    ``device_adam``: the WHOLE update runs on the device (DeviceLearner.update: the statistics, the gradient and Adam
    as well -- fs_adv_stats_dev, fs_adv_finish_dev, fs_ppo_grad_n_dev, fs_adam_dev), with no host round trip between two
    rollouts; it implies the device update.  The learner is built first and the policy's parameters become views into
    its packed weights before anything is captured; a fused or graph DevicePolicy runs on that same buffer, and no
    torch.optim.Adam is built.  Off by default.
    ``kl_target`` / ``kl_coeff`` / ``entropy_coeff`` / ``vf_clip`` (RLlib's names): the terms of the loss the reference
    trains with -- the KL penalty with its adaptive coefficient (starting at ``kl_coeff``), the entropy bonus, the clipped
    value loss (ppo_update states the loss) -- on whichever path the update takes; ``vf_coef`` and ``clip`` are the value
    loss's weight and the surrogate's clip range.  All off by default.  With a KL target the log shows, per iteration, the
    mean KL of the update's last epoch and the coefficient after its adaptation.
    ``sgd_minibatch_size`` (RLlib's name; None: one optimiser step per epoch over the whole fragment): every epoch is a
    shuffled pass of minibatch steps of this many samples (ppo_update(minibatch=) states the semantics).  With
    ``device_adam`` a step runs on the device (DeviceLearner.update(minibatch=)); the torch update runs the same steps in
    torch; ``device_update`` alone (torch's Adam around the kernels) does not build them and says so.  The epochs of
    iteration ``it`` draw the permutations of epochs ``it * epochs ..`` on both paths.
    ``net_log_std``: the policy's head has 2 x act_dim outputs, the means and the log stds (``GaussianPolicy(net_log_std=
    True)``: RLlib's default model, the reference's).  The torch update takes it, and so does ``device_adam`` -- the learner
    is ``DeviceLearner(net_log_std=True)`` and a fused or graph DevicePolicy reads its buffer through ``share`` --;
    ``device_update`` alone (the host-n gradient around torch's Adam) does not build it and says so.  Off by default.
    ``checkpoint_dir`` / ``checkpoint_freq``: rank 0 writes ``save_checkpoint`` every ``checkpoint_freq`` iterations and
    after the last one.  ``restore`` (a ``checkpoint_<iteration>`` directory): the weights, the optimiser state, the KL
    coefficient and the epoch counter are loaded (``restore_policy``) and ``iterations`` more iterations run, numbered
    from ``iteration + 1``; the environments start from a reset and the sampling streams from their seeds, so the run is
    not the uninterrupted run's bit for bit -- the update is.  ``episode_stats``: the iteration line ends with RLlib's
    ``episode_reward_mean / min / max``, ``episode_len_mean`` and ``episodes`` over the episodes that ended in the
    iteration's fragment (``VecFlowEnv.episode_stats``: one launch per fragment; the shared reward on the multi-agent
    heads); ``on_episodes`` (a callable) then receives ``(iteration, summary dict)`` of every iteration.
    ``checkpoint_env_state``: the checkpoints also hold the environments' state (``env_state``); ``restore`` of such a
    checkpoint continues the environments instead of resetting them (``restore_env_state``; the log says which it did).
    Where the LIBRARY draws the samples -- the fused kernels, and the graph around a DevicePolicy (``fuse_action_vector``) --
    iterations k + 1 .. n after a restore are then the uninterrupted run's bit for bit: weights, optimiser state, history,
    episode statistics.  The graph around the torch module samples from torch's CUDA generator, whose state is saved and set
    back as well (DESIGN.md 4.3 says what was shown for that path).  Single process only: a data-parallel run keeps no
    environment state.
    ``evaluation_interval`` N (RLlib's name) with ``evaluation_steps`` S (default: the horizon): after every N-th update the
    environments are snapshot (``VecFlowEnv.snapshot``), reset, stepped S times with the MEAN action (``choose_rollout(...,
    greedy=True)``'s policy or graph, built once, on the learner's weights), and restored; the episodes that ended are
    summarised (k_episode_stats with carries of their own) into ``evaluation/episode_reward_mean|min|max``,
    ``evaluation/episode_len_mean`` and ``evaluation/episodes`` on the iteration line, and ``on_evaluation(iteration,
    summary)`` receives them.  Training with any N is training without it, bit for bit.  All off by
    default: the line, the history and every launch are then what they were."""
    from flow_amd.dist import allreduce_sum, shard_range
    if net_log_std and device_update and not device_adam:
        raise NotImplementedError("train_on_device(net_log_std=True, device_update=True): the 2A-output head is not built for "
                                  "the device update around torch's Adam (fs_ppo_grad_dev); add device_adam (--device_adam), "
                                  "which runs the whole update on the device")
    from flow_amd.envs import VecFlowEnv
    local = int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else 0
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    torch.manual_seed(seed)                                   # the same initial policy on every rank
    lo, hi = shard_range(replicas, rank, world)
    ck = load_checkpoint(restore) if restore is not None else None
    vec = VecFlowEnv(flow_params, num_replicas=hi - lo, device=local, replica_offset=lo,
                     seed=checkpoint_handle_seed(ck) if world == 1 else None)
    n_ag = vec.act_dim if shared_agents else 1
    if shared_agents and (vec.act_dim < 1 or vec.obs_dim % vec.act_dim):
        raise ValueError("shared_agents: the observation (%d) is not one block per action column (%d)" % (vec.obs_dim, vec.act_dim))
    k_ag = vec.obs_dim // n_ag
    pi = GaussianPolicy(k_ag if shared_agents else vec.obs_dim, 1 if shared_agents else vec.act_dim,
                        net_log_std=net_log_std).to(dev)
    free_log_std = None if net_log_std else pi.log_std
    learner, opt = None, None
    if device_adam:
        from flow_amd.utils.device_ppo import DeviceLearner
        learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], free_log_std, [pi.value[0], pi.value[2]], pi.value[4],
                                net_log_std=net_log_std)
        learner.adopt_parameters()                             # (before the rollout graph captures the parameters' addresses)
    else:
        opt = torch.optim.Adam(pi.parameters(), lr=lr)
    fused, graph, graph_policy = choose_rollout(vec, pi, fragment, seed, log, shared_agents=shared_agents,
                                                fuse_action_vector=fuse_action_vector, learner=learner if device_adam else None,
                                                world=world, rank=rank, fuse_shared_agents=fuse_shared_agents)
    K, R = fragment, getattr(vec, "num_rows", hi - lo)                              # (rows: hi - lo environments x num_rings)
    if device_adam:
        log("update: on the device, Adam included (k_ppo_eval, k_gae, k_adv_stats, k_adv_finish, k_ppo_grad, k_adam)")
    elif device_update:
        from flow_amd.utils.device_ppo import DeviceLearner
        learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])
        log("update: on the device (k_ppo_eval, k_gae, k_ppo_grad)")
    kl = AdaptiveKL(kl_target, kl_coeff) if kl_target is not None and not device_adam else None
    update_path = "device_adam" if device_adam else "device_update" if device_update else "torch"
    start = 0
    torch_sampling = fused is None and graph_policy is None      # the graph's samples come from torch's CUDA generator
    env_continues = False
    if restore is not None:
        restore_policy(ck["policies"]["av"], pi, opt, kl, learner, log=log if rank == 0 else (lambda *a: None), name="av")
        start = int(ck["iteration"]) + 1
        if rank == 0:
            log("restore: %s (iteration %d, written on %s): continuing at iteration %d" % (restore, ck["iteration"], ck["update_path"], start))
        if "env" in ck or checkpoint_env_state:
            env_continues = restore_env_state(ck.get("env"), vec, graph, torch_sampling, world,
                                              log=log if rank == 0 else (lambda *a: None))
    evaluator = None
    if evaluation_interval:
        evaluator = Evaluator(vec, pi, int(evaluation_steps or flow_params["env"].horizon), seed, log if rank == 0 else (lambda *a: None),
                              shared_agents=shared_agents, fuse_action_vector=fuse_action_vector,
                              learner=learner if device_adam else None, world=world, rank=rank, graphs=(graph,))
    history = []
    for it in range(start, start + iterations):
        vec.redraw_ring_lengths()                              # pending ring length per replica for its next in-graph reset
        vec.redraw_inflow_rates()                              # ... pending total inflow (reset_inflow; a no-op without it)
        t0 = time.perf_counter()
        if fused is not None:
            fused.sync()                                       # the optimiser moved the weights: repack them for the kernel
            obs, act, _, rew, done = vec.policy_rollout(fused, K, reset_done=True)
            torch.cuda.synchronize(dev)
        else:
            if graph_policy is not None:
                graph_policy.sync()                            # the graph reads the weights at the packed buffer's address
            obs, act, rew, done = graph.replay()               # K closed-loop steps of R replicas: one graph launch
            graph.synchronize()
        t_roll = time.perf_counter() - t0
        if shared_agents:                                      # agents become samples: [K(+1), R * agents, .]
            shard = (obs.reshape(K + 1, R * n_ag, k_ag), act.reshape(K, R * n_ag, 1),
                     rew.repeat_interleave(n_ag, dim=1), done.repeat_interleave(n_ag, dim=1))
        else:
            shard = (obs, act, rew, done)
        if device_adam:
            learner.update([shard], epochs=epochs, lr=lr, clip=clip, vf_coef=vf_coef, kl_target=kl_target,
                           kl_coef_init=kl_coeff, entropy_coef=entropy_coeff, vf_clip=vf_clip, minibatch=sgd_minibatch_size,
                           shuffle_seed=seed)
        else:
            ppo_update(pi, opt, [shard], epochs=epochs, clip=clip, learner=learner, kl=kl, entropy_coef=entropy_coeff,
                       vf_clip=vf_clip, vf_coef=vf_coef, minibatch=sgd_minibatch_size, shuffle_seed=seed,
                       epoch0=it * epochs)
        kl_log = ""
        if kl_target is not None:                              # (read after the update: the device's state under device_adam)
            coef, mean_kl = learner.kl_state.tolist() if device_adam else (kl.coef, kl.mean_kl)
            kl_log = "  KL %.5f  kl_coeff %.4g" % (mean_kl, coef)
        tot = allreduce_sum(torch.stack([rew.double().sum(), torch.tensor(float(rew.numel()), dtype=torch.float64, device=dev),
                                         (done != 0).sum().double()]))
        mean_rew = float(tot[0] / tot[1])
        history.append(mean_rew)
        ep_log = ""
        if episode_stats:                                      # (the episodes that ended in this fragment; carries kept)
            from flow_amd.utils import episode_stats as es
            summary = es.summarize(es.allreduce(vec.episode_stats(rew, done, reset=it == start and not env_continues,
                                                                   accumulate=False)))
            if on_episodes is not None:
                on_episodes(it, summary)
            ep_log = es.log_suffix(summary)
        if evaluator is not None and (it + 1) % int(evaluation_interval) == 0:
            ev = evaluator.run()
            if on_evaluation is not None:
                on_evaluation(it, ev)
            ep_log += evaluator.log_suffix(ev)
        if rank == 0:
            log("iteration %3d  mean step reward %8.4f  rollout %.1f ms (%.2f M env-steps/s per GPU, %d GPU%s)  episodes ended %d%s%s"
                % (it, mean_rew, t_roll * 1e3, K * R / t_roll / 1e6, world, "s" if world > 1 else "", int(tot[2]), kl_log, ep_log))
            if checkpoint_dir is not None and _checkpoint_due(it, start + iterations - 1, checkpoint_freq):
                path = save_checkpoint(checkpoint_dir, it, flow_params, dict(av=policy_state(pi, opt, kl, learner)), seed=seed,
                                       update_path=update_path,
                                       model=dict(shared_agents=bool(shared_agents), fuse_action_vector=bool(fuse_action_vector),
                                                  adversarial=False),
                                       env=env_state(vec, graph, torch_sampling, world) if checkpoint_env_state else None)
                log("checkpoint: %s" % path)
    vec.close()
    return history


ES_DEFAULTS = {"es": dict(sigma=0.02, stepsize=0.02, l2=0.005),       # es_runner.py: noise_stdev, stepsize; RLlib ES l2_coeff
               "ars": dict(sigma=0.2, stepsize=0.2, l2=0.0)}             # ars_runner.py: noise_stdev 0.2, sgd_stepsize 0.2


def es_refusal(flow_params, gpus=1):
    """What ``train_es_on_device`` refuses from the experiment's parameters alone, before anything touches a device: the
    message, or None."""
    from flow_amd import _lib as L
    if int(gpus) > 1:
        return ("--rl_trainer es|ars: --gpus %d is not built: data-parallel ES (members sharded over GPUs, returns gathered "
                "before the ranking) -- run on one GPU" % int(gpus))
    head = getattr(flow_params["env_name"], "FS_ENV", None)
    names = {L.FS_ENV_MERGE_PO: "FS_ENV_MERGE_PO", L.FS_ENV_BOTTLENECK_DV: "FS_ENV_BOTTLENECK_DV", L.FS_ENV_MERGE_MA: "FS_ENV_MERGE_MA"}
    if head in names:
        return ("fs_population: not built for %s (%s): the policy kernels of the merges and the bottleneck give a wave to a "
                "replica; --rl_trainer device trains this experiment" % (names[head], flow_params["env_name"].__name__))
    return None


def train_es_on_device(flow_params, mode="es", replicas=1024, fragment=100, iterations=20, sigma=None, stepsize=None, l2=None,
                       top=0, eval_members=0, seed=0, log=print, shared_agents=False, gpus=1, checkpoint_dir=None,
                       checkpoint_freq=None, restore=None, on_generation=None):
    """Evolution strategies (``mode='es'``: RLlib's ES, the reference's flow/benchmarks/rllib/es_runner.py) or augmented
    random search (``'ars'``: ars_runner.py) on R replicas of ``flow_params``: ``flow_amd.utils.device_es.DeviceES``.
    ``replicas`` divided by the handle's granule (16) is the number of members M; ``eval_members`` E of them run the
    unperturbed policy, the other M - E are (M - E) / 2 antithetic pairs.  A generation rolls every member out for one
    whole episode (``horizon`` steps in fragments of ``fragment``) with the mean action, one launch per fragment.
    ``sigma`` / ``stepsize`` / ``l2`` default to the reference runners' values (``ES_DEFAULTS``); ``top`` (ARS): the
    directions used, 0 = all.  The iteration line shows ``episode_reward_mean|min|max`` over the perturbed members and,
    with evaluation members, ``evaluation/episode_reward_mean``.  ``checkpoint_dir`` / ``checkpoint_freq`` / ``restore``:
    ``save_checkpoint`` / ``load_checkpoint`` with the policy entry examples/evaluate.py reads (the model, in fs_policy's
    layout), ``es`` = ``DeviceES.state_dict()`` and the environments' state (``env_state``: the simulator's noise
    streams and the generator that draws ring lengths run on across the generations' resets); a generation depends on
    nothing else, so a restored run prints the lines the uninterrupted run prints.  Returns the perturbed members' mean
    return per generation."""
    why = es_refusal(flow_params, gpus)
    if why:
        raise NotImplementedError(why)
    if mode not in ES_DEFAULTS:
        raise ValueError("train_es_on_device: mode must be 'es' or 'ars'")
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_es import DeviceES
    from flow_amd.utils.device_policy import DevicePolicy
    d = ES_DEFAULTS[mode]
    sigma, stepsize, l2 = (d["sigma"] if sigma is None else sigma, d["stepsize"] if stepsize is None else stepsize,
                           d["l2"] if l2 is None else l2)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(seed)
    ck = load_checkpoint(restore) if restore is not None else None
    vec = VecFlowEnv(flow_params, num_replicas=replicas, device=0, seed=checkpoint_handle_seed(ck))
    n_ag = vec.act_dim if shared_agents else 1
    if shared_agents and (vec.act_dim < 1 or vec.obs_dim % vec.act_dim):
        raise ValueError("shared_agents: the observation (%d) is not one block per action column (%d)" % (vec.obs_dim, vec.act_dim))
    pi = GaussianPolicy(vec.obs_dim // n_ag, 1 if shared_agents else vec.act_dim).to(dev)
    if pi.act_dim != 1:
        raise NotImplementedError("fs_population: not built for the action-vector heads (%d action columns per evaluation)" % pi.act_dim)
    pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=seed)
    granule = vec.sim.population_granule(pol.struct)           # (raises NotImplementedError with the library's message)
    R = vec.num_rows
    members = R // granule
    if R % granule or members - eval_members < 2 or (members - eval_members) % 2:
        raise ValueError("train_es_on_device: %d rows / %d (fs_population_granule) = %d members; less %d evaluation members "
                         "they must be an even number of at least 2 (antithetic pairs)" % (R, granule, members, eval_members))
    es = DeviceES(vec, pol, pairs=(members - eval_members) // 2, eval_members=eval_members, sigma=sigma, mode=mode,
                  lr=stepsize, stepsize=stepsize, l2=l2, top=top, noise_seed=seed)
    horizon = int(flow_params["env"].horizon)
    log("%s: %d pairs + %d evaluation members x %d replicas, sigma %g, stepsize %g%s; kernels %s"
        % (mode.upper(), es.N, es.E, es.group, sigma, stepsize, ", l2 %g" % l2 if mode == "es" else ", top %d" % (top or es.N),
           "k_es_perturb, k_es_fitness, k_es_weights, k_es_grad" + (", k_adam" if mode == "es" else "")))
    start = 0
    if ck is not None:
        entry = ck["policies"]["av"]
        if "es" not in entry or entry["es"].get("mode") != mode:
            raise ValueError("restore: %s was not written by --rl_trainer %s" % (restore, mode))
        es.load_state_dict(entry["es"])
        start = int(ck["iteration"]) + 1
        log("restore: %s (iteration %d, written on %s): continuing at iteration %d" % (restore, ck["iteration"], ck["update_path"], start))
        restore_env_state(ck.get("env"), vec, None, False, 1, log=log)
    history = []
    for it in range(start, start + iterations):
        t0 = time.perf_counter()
        stats = es.generation(horizon, fragment)
        mean, lo, hi, ev = stats.tolist()                       # (the generation's one host synchronisation)
        t_gen = time.perf_counter() - t0
        history.append(mean)
        if on_generation is not None:
            on_generation(it, dict(episode_reward_mean=mean, episode_reward_min=lo, episode_reward_max=hi,
                                   evaluation_episode_reward_mean=ev if es.E else None))
        log("iteration %3d  episode_reward_mean %.4f  episode_reward_min %.4f  episode_reward_max %.4f%s  generation %.1f ms "
            "(%.2f M env-steps/s)  kernel %s"
            % (it, mean, lo, hi, "  evaluation/episode_reward_mean %.4f" % ev if es.E else "", t_gen * 1e3,
               horizon * R / t_gen / 1e6, es.rollout_kernel))
        if checkpoint_dir is not None and _checkpoint_due(it, start + iterations - 1, checkpoint_freq):
            pol.unpack()                                        # (theta -> the modules evaluate.py loads)
            entry = dict(descriptor=list(model_descriptor(pi)),
                         pi={k: v.detach().to("cpu").clone() for k, v in pi.state_dict().items()}, es=es.state_dict())
            path = save_checkpoint(checkpoint_dir, it, flow_params, dict(av=entry), seed=seed, update_path=mode,
                                   model=dict(shared_agents=bool(shared_agents), fuse_action_vector=False, adversarial=False),
                                   env=env_state(vec))
            log("checkpoint: %s" % path)
    vec.close()
    return history


def add_es_flags(ap):
    ap.add_argument("--es_sigma", type=float, default=None,
                    help="es / ars: standard deviation of the parameter noise (default: the reference runners' noise_stdev, 0.02 / 0.2)")
    ap.add_argument("--es_stepsize", type=float, default=None,
                    help="es: Adam's step size (default 0.02); ars: sgd_stepsize (default 0.2)")
    ap.add_argument("--es_l2", type=float, default=None, help="es: l2_coeff of the gradient (default 0.005, RLlib's)")
    ap.add_argument("--es_top", type=int, default=0, help="ars: directions used per update, the best first (default 0: all)")
    ap.add_argument("--es_eval_members", type=int, default=0,
                    help="es / ars: members that run the unperturbed policy (evaluation/episode_reward_mean on the iteration line)")


def update_adversarial(rollout, update_av, update_adversary):
    """The update step of train_adversarial_on_device: ``rollout`` is what ``VecFlowEnv.policy_pair_rollout`` returns,
    ``(obs, act [2, K, R], logp, rew, done)``.  The av learns from ``(obs, act[0], rew, done)``, the adversary from
    ``(obs, act[1], -rew, done)`` -- the same observations, its own samples, the opposite reward
    (multiagent/ring/accel.py:50-52).  ``update_av`` / ``update_adversary``: callables on one shard, each a per-policy
    update (``ppo_update`` or ``DeviceLearner.update`` with that policy's own optimiser state)."""
    obs, act, _, rew, done = rollout
    update_av((obs, act[0].unsqueeze(-1), rew, done))
    update_adversary((obs, act[1].unsqueeze(-1), -rew, done))


def train_adversarial_on_device(flow_params, replicas=1024, fragment=100, iterations=20, epochs=4, lr=3e-4, seed=0, log=print,
                                device_update=False, device_adam=False, kl_target=None, kl_coeff=0.2, entropy_coeff=0.0,
                                vf_clip=None, vf_coef=0.5, clip=0.2, sgd_minibatch_size=None, net_log_std=False,
                                checkpoint_dir=None, checkpoint_freq=None, restore=None, episode_stats=False,
                                on_episodes=None, checkpoint_env_state=False):
    """PPO on TWO policies with opposite rewards (the reference's adversarial_figure_eight.py: POLICY_GRAPHS 'av' and
    'adversary', policy_mapping_fn the identity): both read AccelEnv's observation, each draws an action, the RL vehicle
    receives ``av + perturb_weight * adversary``.  One fragment is ONE launch (``VecFlowEnv.policy_pair_rollout``:
    k_loop_policy<Adversarial>), followed by one update per policy (``update_adversarial``).  Returns the av's mean step
    reward per iteration (the adversary's is its negation).
    The two ``GaussianPolicy(obs_dim, 1)`` start from different torch seeds and sample with different seeds.  The loss
    and model keywords are ``train_on_device``'s, applied to both policies, and so are the three update paths -- torch
    ``ppo_update`` with an optimiser per policy, ``device_update``, ``device_adam`` (a ``DeviceLearner`` per policy,
    adopted, its ``DevicePolicy`` sharing its weights) -- each a per-policy call.  One process, one GPU; a handle the
    pair kernel refuses raises NotImplementedError with the library's message (there is no captured-graph fallback).
    The observation row is the kernel's AccelEnv order ``[v..., x...]``, where the reference's adversarial state
    interleaves ``[v_i, x_i]``: a fixed permutation of the first layer's inputs, irrelevant to training from scratch.
    ``checkpoint_dir`` / ``checkpoint_freq`` / ``restore`` / ``episode_stats`` / ``on_episodes``: ``train_on_device``'s; a checkpoint holds
    both policies ('av' and 'adversary'), and the episode statistics are the av's (the adversary's return is the negation).
    ``checkpoint_env_state``: ``train_on_device``'s -- both policies sample in the library, so a restored run is the
    uninterrupted run's bit for bit.  In-training evaluation is not built for two policies."""
    if net_log_std and device_update and not device_adam:
        raise NotImplementedError("train_adversarial_on_device(net_log_std=True, device_update=True): the 2A-output head is "
                                  "not built for the device update around torch's Adam (fs_ppo_grad_dev); add device_adam "
                                  "(--device_adam), which runs the whole update on the device")
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from flow_amd.utils.device_ppo import DeviceLearner
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ck = load_checkpoint(restore) if restore is not None else None
    vec = VecFlowEnv(flow_params, num_replicas=replicas, device=0, seed=checkpoint_handle_seed(ck))
    if vec.act_dim != 1:
        raise ValueError("train_adversarial_on_device: two policies drive ONE action column; this environment has %d" % vec.act_dim)

    class Side(object):                                        # one policy with its optimiser state
        pass
    sides = []
    for j, name in enumerate(("av", "adversary")):
        sd = Side()
        sd.name = name
        torch.manual_seed(seed + 7919 * j)                     # different initial weights
        sd.pi = pi = GaussianPolicy(vec.obs_dim, 1, net_log_std=net_log_std).to(dev)
        free_log_std = None if net_log_std else pi.log_std
        sd.learner, sd.opt, sd.kl = None, None, None
        if device_adam:
            sd.learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], free_log_std, [pi.value[0], pi.value[2]],
                                       pi.value[4], net_log_std=net_log_std)
            sd.learner.adopt_parameters()
        else:
            sd.opt = torch.optim.Adam(pi.parameters(), lr=lr)
            if device_update:
                sd.learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]],
                                           pi.value[4])
            if kl_target is not None:
                sd.kl = AdaptiveKL(kl_target, kl_coeff)
        sd.policy = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=free_log_std, seed=seed + 104729 * j)
        if device_adam:
            sd.policy.share(sd.learner)
        sides.append(sd)
    av, adv = sides
    vec.reset()
    vec.policy_pair_rollout(av.policy, adv.policy, 1, reset_done=True)      # (probe: raises with the library's message)
    weight = float(vec.env.env_params.additional_params['perturb_weight'])
    log("rollout: fused two-policy + step kernel (%s); the vehicle receives av + %g * adversary" % (vec.sim.last_kernel, weight))
    vec.reset()
    if device_adam:
        log("update: on the device, Adam included, one DeviceLearner per policy (k_ppo_eval, k_gae, k_adv_stats, "
            "k_adv_finish, k_ppo_grad, k_adam)")
    elif device_update:
        log("update: on the device, one DeviceLearner per policy (k_ppo_eval, k_gae, k_ppo_grad)")
    K, R = fragment, replicas
    update_path = "device_adam" if device_adam else "device_update" if device_update else "torch"
    start = 0
    env_continues = False
    if restore is not None:
        for sd in sides:
            restore_policy(ck["policies"][sd.name], sd.pi, sd.opt, sd.kl, sd.learner, log=log, name=sd.name)
        start = int(ck["iteration"]) + 1
        log("restore: %s (iteration %d, written on %s): continuing at iteration %d" % (restore, ck["iteration"], ck["update_path"], start))
        if "env" in ck or checkpoint_env_state:
            env_continues = restore_env_state(ck.get("env"), vec, log=log)
    history = []
    for it in range(start, start + iterations):
        def updater(sd):
            if device_adam:
                return lambda shard: sd.learner.update([shard], epochs=epochs, lr=lr, clip=clip, vf_coef=vf_coef,
                                                       kl_target=kl_target, kl_coef_init=kl_coeff, entropy_coef=entropy_coeff,
                                                       vf_clip=vf_clip, minibatch=sgd_minibatch_size, shuffle_seed=seed)
            return lambda shard: ppo_update(sd.pi, sd.opt, [shard], epochs=epochs, clip=clip, learner=sd.learner, kl=sd.kl,
                                            entropy_coef=entropy_coeff, vf_clip=vf_clip, vf_coef=vf_coef,
                                            minibatch=sgd_minibatch_size, shuffle_seed=seed, epoch0=it * epochs)
        t0 = time.perf_counter()
        av.policy.sync()                                       # the optimisers moved the weights: repack them for the kernel
        adv.policy.sync()
        rollout = vec.policy_pair_rollout(av.policy, adv.policy, K, reset_done=True)
        torch.cuda.synchronize(dev)
        t_roll = time.perf_counter() - t0
        update_adversarial(rollout, updater(av), updater(adv))
        kl_log = ""
        if kl_target is not None:                              # (read after the updates: the device's state under device_adam)
            for sd in sides:
                coef, mean_kl = sd.learner.kl_state.tolist() if device_adam else (sd.kl.coef, sd.kl.mean_kl)
                kl_log += "  %s KL %.5f  kl_coeff %.4g" % (sd.name, mean_kl, coef)
        rew, done = rollout[3], rollout[4]
        mean_rew = float(rew.double().mean())
        history.append(mean_rew)
        ep_log = ""
        if episode_stats:                                      # (the av's return; the adversary's is its negation)
            from flow_amd.utils import episode_stats as es
            summary = es.summarize(vec.episode_stats(rew, done, reset=it == start and not env_continues, accumulate=False))
            if on_episodes is not None:
                on_episodes(it, summary)
            ep_log = es.log_suffix(summary)
        log("iteration %3d  mean step reward %8.4f  rollout %.1f ms (%.2f M env-steps/s per GPU, 1 GPU)  episodes ended %d%s%s"
            % (it, mean_rew, t_roll * 1e3, K * R / t_roll / 1e6, int((done != 0).sum()), kl_log, ep_log))
        if checkpoint_dir is not None and _checkpoint_due(it, start + iterations - 1, checkpoint_freq):
            path = save_checkpoint(checkpoint_dir, it, flow_params,
                                   {sd.name: policy_state(sd.pi, sd.opt, sd.kl, sd.learner) for sd in sides}, seed=seed,
                                   update_path=update_path,
                                   model=dict(shared_agents=False, fuse_action_vector=False, adversarial=True),
                                   env=env_state(vec) if checkpoint_env_state else None)
            log("checkpoint: %s" % path)
    vec.close()
    return history


def spawn_ranks(gpus, argv):
    """--gpus N without a launcher: start the N ranks as child processes.  Nothing in THIS process has touched a GPU
    (torch.cuda.device_count() does not initialise it); never an exec of a process that has."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < gpus:
        raise SystemExit("train_vec.py --gpus %d: this node exposes %d GPU(s)" % (gpus, have))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    for pr in procs:
        rc = max(rc, abs(pr.wait()))
    raise SystemExit(rc)


def add_ppo_loss_flags(ap):
    """The terms of the reference's PPO loss (RLlib's names), all off by default (train_vec.py and train.py)."""
    ap.add_argument("--kl_target", type=float, default=None,
                    help="add the KL penalty KL(old || new) with RLlib's adaptive coefficient towards this mean KL (the reference: 0.02)")
    ap.add_argument("--kl_coeff", type=float, default=0.2, help="the KL coefficient's initial value (with --kl_target)")
    ap.add_argument("--entropy_coeff", type=float, default=0.0, help="weight of the entropy bonus")
    ap.add_argument("--vf_clip", type=float, default=None,
                    help="clip the value loss: max((v - ret)^2, (v_old + clamp(v - v_old, +-vf_clip) - ret)^2)")
    ap.add_argument("--sgd_minibatch_size", type=int, default=None,
                    help="make every epoch a shuffled pass of minibatch steps of this many samples (the reference: 128); on "
                         "the device with --device_adam.  Default: one step per epoch over the whole fragment")


def add_model_flags(ap):
    """The policy head's form (train_vec.py and train.py)."""
    ap.add_argument("--net_log_std", action="store_true",
                    help="the policy's head has 2 x act_dim outputs, the means and the log stds (RLlib's default model, "
                         "free_log_std: false -- the reference's), instead of a free log_std parameter; on the device with "
                         "--device_adam")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--fragment", type=int, default=100, help="env steps per captured graph")
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel over this many GPUs of the node (one process each)")
    ap.add_argument("--device_update", action="store_true",
                    help="run the PPO update on the library's kernels (DeviceLearner) instead of torch")
    ap.add_argument("--device_adam", action="store_true",
                    help="run the whole PPO update, Adam included, on the device (DeviceLearner.update); implies --device_update")
    add_ppo_loss_flags(ap)
    add_model_flags(ap)
    add_checkpoint_flags(ap)
    args = ap.parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    force = os.environ.get("TRAIN_FORCE_DIST") == "1"            # the N > 1 code path (RCCL init, all-reduces) with one rank
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args.gpus, sys.argv[1:] if argv is None else argv)
    if args.gpus != world and not (args.gpus == 1 and world == 1):
        raise SystemExit("train_vec.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 or force:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29544")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    try:
        return train_on_device(ring_flow_params(args.horizon), replicas=args.replicas, fragment=args.fragment,
                               iterations=args.iterations, epochs=args.epochs, lr=args.lr, rank=rank, world=world,
                               device_update=args.device_update or args.device_adam, device_adam=args.device_adam,
                               kl_target=args.kl_target, kl_coeff=args.kl_coeff, entropy_coeff=args.entropy_coeff,
                               vf_clip=args.vf_clip, sgd_minibatch_size=args.sgd_minibatch_size,
                               net_log_std=args.net_log_std, checkpoint_dir=args.checkpoint_dir,
                               checkpoint_freq=args.checkpoint_freq, restore=args.restore, episode_stats=args.episode_stats,
                               checkpoint_env_state=args.checkpoint_env_state, evaluation_interval=args.evaluation_interval,
                               evaluation_steps=args.evaluation_steps)
    finally:
        if world > 1 or force:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
