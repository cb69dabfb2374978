"""examples/train_vec.py ppo_update with absent agents (the multi-agent merge's fused rollout marks an agent whose RL slot
holds no vehicle with a NaN action): with every sample present the update is the plain one bit for bit; NaN samples are
left out of the advantage statistics and the loss, so the update is finite and does not see their actions."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))

K, R, D = 12, 10, 5


def plain_update(pi, opt, shards, epochs=4, clip=0.2):
    """ppo_update as it reads for fully present shards (single process)."""
    from train_vec import gae
    prepared, stats = [], None
    for obs, act, rew, done in shards:
        K_, R_ = rew.shape
        o, a = obs[:K_].reshape(K_ * R_, -1), act.reshape(K_ * R_, -1)
        with torch.no_grad():
            logp_old, val = pi.logp_value(o, a)
            last_val = pi.value(obs[K_]).squeeze(-1)
            adv, ret = gae(rew, val.view(K_, R_), done, last_val)
            adv = adv.reshape(-1).double()
            st = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(adv.numel()), dtype=torch.float64)])
            stats = st if stats is None else stats + st
        prepared.append((o, a, logp_old, adv, ret.reshape(-1)))
    n = stats[2]
    mean = stats[0] / n
    std = ((stats[1] - n * mean * mean) / (n - 1)).clamp_min(0).sqrt()
    for _ in range(epochs):
        opt.zero_grad()
        for o, a, logp_old, adv, ret in prepared:
            adv_n = ((adv - mean) / (std + 1e-8)).float()
            logp, v = pi.logp_value(o, a)
            ratio = (logp - logp_old).exp()
            loss = (-torch.min(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n).sum()
                    + 0.5 * (v - ret).pow(2).sum()) / float(n)
            loss.backward()
        opt.step()


def fragment(seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((K + 1, R, D), generator=g)
    act = torch.randn((K, R, 1), generator=g)
    rew = torch.rand((K, R), generator=g)
    done = (torch.rand((K, R), generator=g) < 0.05).to(torch.uint8)
    return obs, act, rew, done


def policy():
    from train_vec import GaussianPolicy
    torch.manual_seed(0)
    pi = GaussianPolicy(D, 1)
    return pi, torch.optim.Adam(pi.parameters(), lr=3e-3)


def params(pi):
    return torch.cat([p.detach().reshape(-1) for p in pi.parameters()])


def test_every_sample_present_is_the_plain_update():
    from train_vec import ppo_update
    shards = [fragment(1), fragment(2)]
    a, oa = policy()
    b, ob = policy()
    ppo_update(a, oa, shards)
    plain_update(b, ob, shards)
    assert torch.equal(params(a), params(b))


def test_absent_samples_are_left_out():
    from train_vec import ppo_update
    obs, act, rew, done = fragment(3)
    absent = torch.rand((K, R), generator=torch.Generator().manual_seed(4)) < 0.3
    act_nan = act.clone()
    act_nan[absent] = float("nan")
    act_other = act_nan.clone()
    act_other[absent] = -float("nan")                       # (another NaN: the absent samples' values do not count)
    start, _ = policy()
    a, oa = policy()
    ppo_update(a, oa, [(obs, act_nan, rew, done)])
    b, ob = policy()
    ppo_update(b, ob, [(obs, act_other, rew, done)])
    pa = params(a)
    assert torch.isfinite(pa).all() and not torch.equal(pa, params(start))
    assert torch.equal(pa, params(b))
    # the same update from the present samples' actions, whatever stands at the absent places (finite values included
    # would be a different update: the statistics and the loss count only the present samples)
    c, oc = policy()
    ppo_update(c, oc, [(obs, act, rew, done)])
    assert not torch.equal(pa, params(c))
