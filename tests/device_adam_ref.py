"""numpy restatements of the two operation sequences include/flowsim.h writes out for fs_adam_dev and fs_adv_finish_dev, and
the Adam problem (inputs, torch float64 result, torch float32's own error) that the CPU and the GPU test share.  No test in
here: tests/test_device_adam_cpu.py and tests/test_device_adam_gpu.py import it."""
import functools

import numpy as np
import torch

MARGIN = 10.0                 # the project's bound (tests/test_device_ppo_gpu.py): so many times torch float32's own error
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8


def adam_ref(w, g, m, v, state, lr=LR, betas=BETAS, eps=EPS):
    """One fs_adam_dev call: float32 arrays w, g, m, v and the float64 state {t, beta1^t, beta2^t} -> (w, m, v, state)."""
    f = np.float32
    assert w.dtype == g.dtype == m.dtype == v.dtype == np.float32 and state.dtype == np.float64
    b1, b2 = np.float64(betas[0]), np.float64(betas[1])
    t, p1, p2 = state[0] + np.float64(1.0), state[1] * b1, state[2] * b2
    step = f(np.float64(lr) / (np.float64(1.0) - p1))
    rs = f(np.sqrt(np.float64(1.0) - p2))
    c1, bb2, c2, e = f(np.float64(1.0) - b1), f(b2), f(np.float64(1.0) - b2), f(eps)
    m = m + (g - m) * c1
    v = v * bb2 + (g * g) * c2
    w = w - step * (m / (np.sqrt(v) / rs + e))
    assert w.dtype == m.dtype == v.dtype == np.float32
    return w, m, v, np.array([t, p1, p2], dtype=np.float64)


def finish_ref(stats):
    """fs_adv_finish_dev: float64 {sum, sum of squares, count} -> {mean, std, n}."""
    s0, s1, n = (np.float64(x) for x in stats)
    mean = s0 / n
    var = (s1 - (n * mean) * mean) / (n - np.float64(1.0))
    return np.array([mean, np.sqrt(np.maximum(var, np.float64(0.0))), n], dtype=np.float64)


def fresh_state():
    return np.array([0.0, 1.0, 1.0], dtype=np.float64)


def draw_gradients(P, steps, seed):
    """[steps] float32 gradients of P elements with magnitudes spread over 1e-6 .. 1, both signs; every seventh element is
    an exact zero in every step (m = v = 0 throughout), and a tenth of the others in any one step."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        mag = 10.0 ** (-6.0 * torch.rand(P, generator=g, dtype=torch.float64))
        sign = torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0).double()
        x = (mag * sign).float()
        x[torch.rand(P, generator=g) < 0.1] = 0.0
        x[::7] = 0.0
        out.append(x)
    return out


def displacement_error(w, w64, w0):
    """max|w - w64| / max|w64 - w0|: the error against float64 over what the update moved."""
    w, w64, w0 = (np.asarray(x, dtype=np.float64) for x in (w, w64, w0))
    return float(np.abs(w - w64).max() / np.abs(w64 - w0).max())


@functools.lru_cache(maxsize=None)
def adam_problem(P, steps=10):
    """w0, the gradients, torch.optim.Adam's float64 result after `steps` steps, and torch float32's error by
    displacement_error on the same inputs (all on the CPU: the same bits on every machine)."""
    g = torch.Generator().manual_seed(31 * P + steps)
    w0 = torch.randn(P, generator=g)
    grads = draw_gradients(P, steps, seed=P)
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        p = torch.nn.Parameter(w0.to(dt).clone())
        opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=EPS)
        for x in grads:
            p.grad = x.to(dt).clone()
            opt.step()
        out[name] = p.detach().numpy().copy()
    w0 = w0.numpy().copy()
    return dict(w0=w0, grads=[x.numpy().copy() for x in grads], w64=out["f64"], w32=out["f32"],
                err32=displacement_error(out["f32"], out["f64"], w0))


def run_adam_ref(w0, grads):
    """The restatement over all the gradients from a fresh state: [(w, m, v, state) after each step]."""
    w, m, v, st = w0.copy(), np.zeros_like(w0), np.zeros_like(w0), fresh_state()
    out = []
    for x in grads:
        w, m, v, st = adam_ref(w, x, m, v, st)
        out.append((w, m, v, st))
    return out
