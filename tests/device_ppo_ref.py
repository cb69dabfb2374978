"""Restatements, on the CPU, of the two reduction orders flow_amd/csrc/flowsim_learn.h states (DESIGN.md section 4.3,
"Deterministic reduction" and `k_adv_stats`), and the packed-gradient size.  No test in here: tests/test_device_ppo_cpu.py
and tests/test_device_ppo_scale_gpu.py import it.

* compose_ref: how k_ppo_grad and k_ppo_reduce put a gradient together from the block sums of its 64-sample tiles.  Every
  element of the packed gradient and of the two loss sums receives ONE float32 add per tile: workgroup g starts from +0 and
  adds the sums of tiles g, g + G, g + 2 G, ... in ascending order; the G partial results are then added in ascending order.
* adv_stats_ref: the order of k_adv_stats' three double sums, which depends on n alone."""
import numpy as np
import torch

TILE = 64


def packed(D, A, layers):
    """Elements of the packed gradient [policy][log_std A][value] (flowsim_learn.h ppo_params)."""
    net = 32 * D + 32 + (layers - 1) * 1056
    return (net + 33 * A) + A + (net + 33)


def compose_ref(tile_sums, G):
    """tile_sums [tiles, C] float32 (CPU), G workgroups -> [C] float32:
        acc_g = (((0 + T_g) + T_{g+G}) + T_{g+2G}) ...          out = ((acc_0 + acc_1) + acc_2) + ... + acc_{G-1}
    elementwise in float32, one rounding per add, nothing fused.  A workgroup without a tile contributes its zeros."""
    T = torch.as_tensor(tile_sums)
    assert T.dtype == torch.float32 and T.dim() == 2 and T.device.type == "cpu" and G >= 1
    tiles, C = T.shape
    acc = torch.zeros(G, C, dtype=torch.float32)
    for first in range(0, tiles, G):                        # round k: tile first + g goes to workgroup g
        rows = T[first:first + G]
        acc[:rows.shape[0]] = acc[:rows.shape[0]] + rows
    out = acc[0].clone()
    for g in range(1, G):
        out = out + acc[g]
    return out


def adv_groups(n):
    return min(512, max(1, -(-n // 1024)))


def _tree(red):
    """red [..., 256] -> [...]: lane t += lane t + half, half = 128 .. 1."""
    red = red.copy()
    half = 128
    while half >= 1:
        red[..., :half] = red[..., :half] + red[..., half:2 * half]
        half //= 2
    return red[..., 0]


def adv_stats_ref(adv, present):
    """adv float32 [n], present bool [n] -> float64 [3] = {sum adv, sum adv^2, count} in k_adv_stats' order: with G =
    adv_groups(n), lane t of workgroup b starts from +0.0 and adds rows 256 b + t + 256 G k, k ascending, in double (an
    absent row adds 0.0, whatever it holds); the 256 lanes meet in the tree; then lane t adds the partial sums of
    workgroups t and t + 256 in that order, and the same tree follows.  (Rows and workgroups that do not exist are padded
    with +0.0: no sum here can be -0.0, so x + 0.0 == x bit for bit.)"""
    adv, present = np.asarray(adv), np.asarray(present)
    assert adv.dtype == np.float32 and present.dtype == np.bool_ and adv.shape == present.shape and adv.ndim == 1
    n = adv.shape[0]
    G = adv_groups(n)
    stride = 256 * G
    K = -(-n // stride)
    a = np.zeros(K * stride, dtype=np.float64)
    a[:n] = np.where(present, adv.astype(np.float64), np.float64(0.0))
    one = np.zeros(K * stride, dtype=np.float64)
    one[:n] = present.astype(np.float64)
    terms = np.stack([a, a * a, one]).reshape(3, K, G, 256)  # (the square of a float32 value is exact in double)
    lanes = np.zeros((3, G, 256), dtype=np.float64)
    for k in range(K):
        lanes = lanes + terms[:, k]
    part = np.zeros((3, 512), dtype=np.float64)
    part[:, :G] = _tree(lanes)
    part = part.reshape(3, 2, 256)
    return _tree((np.zeros((3, 256), dtype=np.float64) + part[:, 0]) + part[:, 1])
