"""What a user-written environment head costs, and what it replaces:
python scripts/bench_compiled_env.py [--replicas 4096] [--reps 7] [--out profiles/compiled_env_bench.json]

A 22-vehicle ring (21 noisy IDM vehicles + 1 RL vehicle), fragments of 100 steps on an action tape, `reps` fragments per
form, the forms alternated in ONE process, on a device-synchronised host clock:
  compiled_head  AccelEnv restated as a CompiledEnv (examples/compiled_env.py AccelStyleEnv): head FS_ENV_USER in k_steps,
                 `replicas` replicas, one launch per fragment -- as a user gets it (IDM + RL slots: k_steps<CSET>)
  builtin_head   the built-in AccelEnv head on k_steps (the handle is created with FLOWSIM_FORCE_GENERIC=1, which also keeps
                 the CSET instantiation out: plain k_steps)
  compiled_head_generic  compiled_head created with FLOWSIM_FORCE_GENERIC=1 as well: the SAME instantiation as builtin_head,
                 so compiled_generic_over_builtin_seconds is what the user head itself costs
  python_hooks   the scalar Env with Python hooks (FS_ENV = None) computing the same observation and reward on the host
                 from env.k.vehicle: ONE replica, one launch and one host round trip per step -- what a user-written
                 environment ran on before
One JSON object on stdout (and in --out): seconds per fragment, environment steps per second, and the ratios with their
ranges (min / max of one form over max / min of the other)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
STEPS = 100


def seconds(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def ratio(a, b):
    """a / b of two spreads, with the range the two ranges allow."""
    return {"median": a["median"] / b["median"], "min": a["min"] / b["max"], "max": a["max"] / b["min"]}


def host_env_class():
    import numpy as np
    from flow_amd.envs import Env
    from flow_amd.utils.spaces import Box

    class HostAccelEnv(Env):
        """AccelEnv's observation and reward computed in Python from the vehicle kernel, as a user's Env subclass does."""

        @property
        def action_space(self):
            return Box(low=-1, high=1, shape=(self.initial_vehicles.num_rl_vehicles, ), dtype=np.float32)

        @property
        def observation_space(self):
            return Box(low=0, high=1, shape=(2 * self.initial_vehicles.num_vehicles, ), dtype=np.float32)

        def _apply_rl_actions(self, rl_actions):
            self.k.vehicle.apply_acceleration(self.k.vehicle.get_rl_ids(), rl_actions)

        def get_state(self):
            ids = self.k.vehicle.get_ids()
            speed = [self.k.vehicle.get_speed(v) / self.k.network.max_speed() for v in ids]
            pos = [self.k.vehicle.get_x_by_id(v) / self.k.network.length() for v in ids]
            return np.array(speed + pos)

        def compute_reward(self, rl_actions, **kwargs):
            vel = np.array(self.k.vehicle.get_speed(self.k.vehicle.get_ids()))
            if any(vel < -100) or kwargs.get("fail"):
                return 0.0
            target = self.env_params.additional_params["target_velocity"]
            max_cost = np.linalg.norm(np.array([target] * len(vel)))
            cost = np.linalg.norm(vel - target)
            return max(max_cost - cost, 0) / (max_cost + np.finfo(np.float32).eps)
    return HostAccelEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from compiled_env import AccelStyleEnv, ring_flow_params
    from flow_amd.envs import AccelEnv, VecFlowEnv
    torch.cuda.set_device(0)
    R = args.replicas

    def params(env_name):
        fp = ring_flow_params(env_name=env_name, num_vehicles=22, num_rl=1, user_humans=False, horizon=10 ** 6)
        fp["env"].additional_params["sort_vehicles"] = False
        return fp
    user = VecFlowEnv(params(AccelStyleEnv), num_replicas=R, device=0, seed=7)
    os.environ["FLOWSIM_FORCE_GENERIC"] = "1"                  # (read by fs_create: these two handles only)
    try:
        stock = VecFlowEnv(params(AccelEnv), num_replicas=R, device=0, seed=7)
        user_generic = VecFlowEnv(params(AccelStyleEnv), num_replicas=R, device=0, seed=7)
    finally:
        os.environ.pop("FLOWSIM_FORCE_GENERIC")
    fp = params(host_env_class())
    host = fp["env_name"](fp["env"], fp["sim"], fp["network"](name="host", vehicles=fp["veh"], net_params=fp["net"],
                                                              initial_config=fp["initial"]))
    tape = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (STEPS, R, 1)).astype(np.float32)).to(user.device)
    host_tape = tape[:, 0].cpu().numpy()
    legs = []
    for name, vec in (("compiled_head", user), ("builtin_head", stock), ("compiled_head_generic", user_generic)):
        vec.reset()
        out = vec.rollout(STEPS, tape)                             # warm-up
        legs.append((name, vec.sim.last_kernel, R, (lambda vec=vec, out=out: seconds(torch, lambda: vec.rollout(STEPS, tape, out=out))), []))
    host.reset()

    def host_fragment():
        def run():
            for k in range(STEPS):
                host.step(host_tape[k])
        return seconds(torch, run)
    host_fragment()                                                # warm-up
    legs.append(("python_hooks", host.sim.last_kernel, 1, host_fragment, []))
    for _ in range(args.reps):                                     # alternately: drifts of the clock hit every form alike
        for _, _, _, fn, ts in legs:
            ts.append(fn())
    # the two heads compute the same numbers
    user.reset(), stock.reset()
    a, b = user.rollout(STEPS, tape), stock.rollout(STEPS, tape)
    same = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
    res = {"steps": STEPS, "reps": args.reps, "replicas": R, "vehicles": 22, "device": torch.cuda.get_device_name(0),
           "clock": "host, device-synchronised", "heads_bit_equal": same}
    for name, kernel, rows, _, ts in legs:
        s = spread(ts)
        res[name] = {"kernel": kernel, "replicas": rows, "seconds": s,
                     "env_steps_per_s": {"median": STEPS * rows / s["median"], "min": STEPS * rows / s["max"],
                                         "max": STEPS * rows / s["min"]}}
    res["compiled_over_builtin_seconds"] = ratio(res["compiled_head"]["seconds"], res["builtin_head"]["seconds"])
    res["compiled_generic_over_builtin_seconds"] = ratio(res["compiled_head_generic"]["seconds"], res["builtin_head"]["seconds"])
    res["compiled_over_python_hooks_env_steps_per_s"] = ratio(res["compiled_head"]["env_steps_per_s"],
                                                              res["python_hooks"]["env_steps_per_s"])
    user.close(), stock.close(), user_generic.close(), host.terminate()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
