"""k_episode_stats in numpy: the order include/flowsim.h documents for fs_episode_stats_dev, operation for operation, so
the kernel can be held to it bit for bit (tests/test_episode_stats_gpu.py), and a plain per-replica loop to hold THIS to
(tests/test_episode_stats_cpu.py)."""
import numpy as np

THREADS, MAX_GROUPS = 256, 512
EMPTY = np.array([0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, np.inf, -np.inf])
_OPS = [np.add, np.add, np.add, np.fmin, np.fmax, np.add, np.fmin, np.fmax]


def groups(R):
    return max(1, min(MAX_GROUPS, -(-R // THREADS)))


def _combine(a, b):
    """[8, ...] (+) [8, ...]: add, fmin or fmax per statistic."""
    return np.stack([op(a[k], b[k]) for k, op in enumerate(_OPS)])


def _tree(lanes):
    """lanes [8, 256, ...] -> [8, ...]: lane t (+)= lane t + half, half = 128 .. 1."""
    red = lanes.copy()
    half = THREADS // 2
    while half >= 1:
        red[:, :half] = _combine(red[:, :half], red[:, half:2 * half])
        half //= 2
    return red[:, 0]


def episode_stats_ref(rew, done, run_ret=None, run_len=None, stats=None, accumulate=False):
    """(stats [8] float64, run_ret [R] float64, run_len [R] int32) of ``rew`` [K, R] float32 and ``done`` [K, R] uint8,
    from the carries ``run_ret`` / ``run_len`` (None: zeros).  ``accumulate``: combined with ``stats``."""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    K, R = rew.shape
    ret = np.zeros(R) if run_ret is None else np.array(run_ret, np.float64)
    ln = np.zeros(R, np.int32) if run_len is None else np.array(run_len, np.int32)
    G = groups(R)
    # lane (b, t) walks replicas 256 b + t + 256 G j, j ascending: all lanes at once, pass j by pass j
    part = np.repeat(EMPTY[:, None], G * THREADS, axis=1)
    for j in range(-(-R // (G * THREADS))):
        r = np.arange(j * G * THREADS, min(R, (j + 1) * G * THREADS))
        lane = r - j * G * THREADS
        for k in range(K):
            ret[r] = ret[r] + rew[k, r].astype(np.float64)
            ln[r] += 1
            e = done[k, r] != 0
            if e.any():
                le, re_ = lane[e], ret[r[e]]
                ll = ln[r[e]].astype(np.float64)
                one = np.stack([np.ones_like(re_), re_, re_ * re_, re_, re_, ll, ll, ll])
                part[:, le] = _combine(part[:, le], one)
                ret[r[e]] = 0.0
                ln[r[e]] = 0
    wg = _tree(part.reshape(8, G, THREADS).transpose(0, 2, 1))          # [8, G]: the workgroups' partials
    # the last workgroup: lane t combines workgroups t and t + 256, then the same tree
    lanes = np.repeat(EMPTY[:, None], THREADS, axis=1)
    for g0 in range(0, G, THREADS):
        n = min(THREADS, G - g0)
        lanes[:, :n] = _combine(lanes[:, :n], wg[:, g0:g0 + n])
    out = _tree(lanes)
    if accumulate:
        out = _combine(np.asarray(stats, np.float64), out)
    return out, ret, ln


def episode_stats_loop(rew, done, run_ret=None, run_len=None):
    """The plain definition: per replica, a Python loop over the steps; the episodes' (return, length) in the order
    (replica, step), and the carries."""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    K, R = rew.shape
    ret = np.zeros(R) if run_ret is None else np.array(run_ret, np.float64)
    ln = np.zeros(R, np.int64) if run_len is None else np.array(run_len, np.int64)
    episodes = []
    for r in range(R):
        for k in range(K):
            ret[r] += float(rew[k, r])
            ln[r] += 1
            if done[k, r] != 0:
                episodes.append((ret[r], int(ln[r])))
                ret[r], ln[r] = 0.0, 0
    return episodes, ret, ln
