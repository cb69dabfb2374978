"""Episode statistics in RLlib's names, from the eight doubles ``fs_episode_stats_dev`` keeps
(``VecFlowEnv.episode_stats``): ``{episodes, sum ret, sum ret^2, min ret, max ret, sum len, min len, max len}``.

What a user of the reference reads off an RLlib run -- ``episode_reward_mean / min / max``, ``episode_len_mean`` -- and off
``flow/visualize/visualizer_rllib.py`` -- the per-round ``Return`` and its ``Average, std``.  On the shared-reward
multi-agent heads the return is that of the reward every agent shares (one episode per replica); the adversary's return
in the two-policy experiment is the negation of the av's.
"""
import math

EMPTY = (0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, float("inf"), float("-inf"))
SUMS, MINS, MAXS = (0, 1, 2, 5), (3, 6), (4, 7)


def _values(stats):
    vals = stats.tolist() if hasattr(stats, "tolist") else list(stats)
    if len(vals) != 8:
        raise ValueError("episode statistics are 8 values (got %d)" % len(vals))
    return [float(v) for v in vals]


def combine(list_of_stats):
    """The statistics of several shards (or fragments kept apart) as one list of 8 floats: the sums add, in the list's
    order, and min / max combine.  A pure function of host values (tensors are read with ``tolist()``)."""
    out = list(EMPTY)
    for stats in list_of_stats:
        s = _values(stats)
        for k in SUMS:
            out[k] = out[k] + s[k]
        for k in MINS:
            out[k] = min(out[k], s[k])
        for k in MAXS:
            out[k] = max(out[k], s[k])
    return out


def allreduce(stats, group=None):
    """``stats`` [8] (a float64 tensor) combined over the ranks of a data-parallel run: the sums through
    ``flow_amd.dist.allreduce_sum``, min / max through one ``all_reduce`` each way -- MIN over {min ret, min len, -max ret,
    -max len}.  Without an initialised process group: ``stats`` itself."""
    import torch.distributed as dist
    from flow_amd.dist import allreduce_sum
    if not (dist.is_available() and dist.is_initialized()):
        return stats
    out = stats.clone()
    out[list(SUMS)] = allreduce_sum(stats[list(SUMS)].clone(), group)
    ext = stats[list(MINS) + list(MAXS)].clone()
    ext[2:] = -ext[2:]
    dist.all_reduce(ext, op=dist.ReduceOp.MIN, group=group)
    ext[2:] = -ext[2:]
    out[list(MINS) + list(MAXS)] = ext
    return out


def summarize(stats):
    """RLlib's names: ``episodes`` (int), ``episode_reward_mean / min / max``, ``episode_reward_std`` (the population
    standard deviation numpy's ``std`` gives, as visualizer_rllib.py prints it), ``episode_len_mean / min / max``.  With no
    episode ended every one but ``episodes`` is None."""
    n, s1, s2, rmin, rmax, sl, lmin, lmax = _values(stats)
    if n < 1.0:
        return dict(episodes=0, episode_reward_mean=None, episode_reward_min=None, episode_reward_max=None,
                    episode_reward_std=None, episode_len_mean=None, episode_len_min=None, episode_len_max=None)
    mean = s1 / n
    var = s2 / n - mean * mean
    return dict(episodes=int(n), episode_reward_mean=mean, episode_reward_min=rmin, episode_reward_max=rmax,
                episode_reward_std=math.sqrt(var) if var > 0.0 else 0.0, episode_len_mean=sl / n, episode_len_min=int(lmin),
                episode_len_max=int(lmax))


def log_suffix(summary):
    """The tail ``--episode_stats`` appends to a trainer's iteration line."""
    if not summary["episodes"]:
        return "  episode_reward_mean None  episode_reward_min None  episode_reward_max None  episode_len_mean None  episodes 0"
    return ("  episode_reward_mean %.4f  episode_reward_min %.4f  episode_reward_max %.4f  episode_len_mean %.1f  episodes %d"
            % (summary["episode_reward_mean"], summary["episode_reward_min"], summary["episode_reward_max"],
               summary["episode_len_mean"], summary["episodes"]))
