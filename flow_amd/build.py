"""Build libflowsim.so (HIP, gfx950) in-tree.  hipcc cross-compiles without a GPU.

The library is several objects: `flowsim.hip` (C ABI, validation, handle) and `flowsim_part.hip` compiled once per
(precision, lanes per replica) pair -- each pair instantiates its own step kernels, so the objects compile in parallel --
and once more for the PPO update's kernels (`learn_f32`, flowsim_learn.h).
Objects are cached under flow_amd/csrc/_obj/ with a stamp = hash of the CONTENTS of every source and header plus the
flags: an edit to any of them recompiles every object (they share the headers' struct layouts), a change of flags only
the objects it concerns.  The library is current only if every object's stamp is (needs_build)."""
import concurrent.futures
import hashlib
import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "flowsim.hip")
PART = os.path.join(CSRC, "flowsim_part.hip")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(PKG, "libflowsim.so")

# the ROCm release the hand-written register assignment of k_rollout_pair (v112..v145, flowsim_pair_step_a*.inc) was
# validated on; tests/test_codegen.py re-checks the assignment against the disassembly on every build
VALIDATED_ROCM = "7.2"

HEADERS = ["flowsim_sim.h", "flowsim_launch.h", "flowsim_kernels.h", "flowsim_open.h", "flowsim_wide.h",
           "flowsim_pair.h", "flowsim_pair_step_a.inc", "flowsim_pair_step_a_sm.inc", "flowsim_fig8.h", "flowsim_ringrl.h", "flowsim_policy.h", "flowsim_queue.h", "flowsim_queue_consts.h", "flowsim_dropq.h",
           "flowsim_learn.h", "flowsim_es.h", "flowsim_snap.h",
           "flowsim_part.hip"]
DEPS = [SRC] + [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(ROOT, "include", "flowsim.h")]
assert all(os.path.exists(d) for d in DEPS)
_known = set(os.path.basename(d) for d in DEPS)
assert all(f in _known for f in os.listdir(CSRC) if f.endswith((".h", ".inc", ".hip"))), "flow_amd/build.py: a source under csrc/ is not in DEPS"

# -ffp-contract=off: the kernels are the float32 bit-twin of the oracle only if a*b+c is never fused
COMMON_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wno-unused-function"]
HIPCC_FLAGS = COMMON_FLAGS + ["-fPIC", "-shared"]       # (kept for callers that compile a single file themselves)


def parts():
    """[(object name, source, extra -D flags)] of the library."""
    out = [("main", SRC, [])]
    for t, tn in (("float", "f32"), ("double", "f64")):
        for seg in (8, 16, 32, 64):
            out.append(("seg%d_%s" % (seg, tn), PART, ["-DFS_PART_T=" + t, "-DFS_PART_SEG=%d" % seg]))
        for w in (2, 4):
            out.append(("wide%d_%s" % (w, tn), PART, ["-DFS_PART_T=" + t, "-DFS_PART_WIDE=%d" % w]))
    out.append(("queue_f32", PART, ["-DFS_PART_T=float", "-DFS_PART_QUEUE=1"] +
                (["-DFS_QDIAG=1"] if os.environ.get("FLOWSIM_QDIAG") else [])))     # cycle counters of k_merge_queue's sections
    out.append(("learn_f32", PART, ["-DFS_PART_T=float", "-DFS_PART_LEARN=1"]))     # the PPO update (flowsim_learn.h)
    return out


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libflowsim.so cannot be built (no CPU fallback exists)")


def include_flags():
    return ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def _stamp(extra):
    h = hashlib.sha256()
    for d in DEPS:
        h.update(os.path.relpath(d, ROOT).encode())     # (relative: the same tree at another path has the same stamps)
        with open(d, "rb") as f:
            h.update(hashlib.sha256(f.read()).digest())
    h.update(" ".join(COMMON_FLAGS + extra).encode())
    return h.hexdigest()[:16]


def _have_stamp(out):
    if not (os.path.exists(out) and os.path.exists(out + ".stamp")):
        return None
    with open(out + ".stamp") as f:
        return f.read().strip()


def needs_build():
    """The library is missing, older than a source, or some object was built from other sources / flags than the current
    ones (build(only=...) links stale objects: their stamps say so and the next plain build() recompiles them)."""
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    if any(os.path.getmtime(d) > t for d in DEPS):
        return True
    return any(_have_stamp(os.path.join(OBJ, name + ".o")) != _stamp(extra) for name, _, extra in parts())


def _compile(job):
    name, src, extra, out, verbose = job
    cmd = [find_hipcc()] + COMMON_FLAGS + ["-fPIC", "-c"] + extra + include_flags() + ["-o", out + ".tmp", src]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed (%s):\n%s%s" % (name, res.stdout, res.stderr))
    os.replace(out + ".tmp", out)
    return out


def _jobs():
    return max(1, min(len(parts()), int(os.environ.get("FLOWSIM_BUILD_JOBS", os.cpu_count() or 4))))


def build_variant(lib, defines, names=None, verbose=False):
    """A development build of the library with extra -D flags (phase timers, diagnostics) at path `lib`; objects under
    _obj/<basename>/.  `names`: the parts to compile with the flags (the others are taken from the plain build)."""
    build()
    obj_dir = os.path.join(OBJ, os.path.basename(lib))
    os.makedirs(obj_dir, exist_ok=True)
    objs, todo = [], []
    for name, src, extra in parts():
        if names and name not in names:
            objs.append(os.path.join(OBJ, name + ".o"))
            continue
        out = os.path.join(obj_dir, name + ".o")
        objs.append(out)
        todo.append((name, src, extra + list(defines), out, verbose))
    with concurrent.futures.ThreadPoolExecutor(_jobs()) as pool:
        list(pool.map(_compile, todo))
    res = subprocess.run([find_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs,
                         capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    return lib


def build(force=False, verbose=False, only=None):
    """Compile the objects (in parallel) and link flow_amd/libflowsim.so; returns its path.  `only` = names of the
    parts to recompile whatever their stamps say (development)."""
    if not force and not only and not needs_build():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    objs, todo, stamps = [], [], {}
    for name, src, extra in parts():
        out = os.path.join(OBJ, name + ".o")
        stamp, have = _stamp(extra), _have_stamp(out)
        objs.append(out)
        # development (`only`): the named parts are recompiled, every other object is linked as it is -- its stale
        # stamp makes needs_build() true, so the next plain build() recompiles it
        if force or (only and name in only) or (not only and have != stamp) or not os.path.exists(out):
            todo.append((name, src, extra, out, verbose))
            stamps[out] = stamp
    with concurrent.futures.ThreadPoolExecutor(_jobs()) as pool:
        for out in pool.map(_compile, todo):
            with open(out + ".stamp", "w") as f:
                f.write(stamps[out])
    cmd = [find_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(LIB + ".tmp", LIB)
    return LIB


USER_DIR = os.path.join(PKG, "_user")
USER_SIGNATURE = ("template <typename T>\n__device__ __forceinline__ T fs_user_accel(T v, T v_lead, T h, bool has_lead, "
                  "T v_follow, T h_follow, T dt, T max_accel, const T* p)")


def user_header(body):
    """The header a user controller is compiled from: ``body`` = the statements of its get_accel (C++, ending in a
    return), with the vehicle's speed ``v``, the leader's ``v_lead``, the bumper-to-bumper headway ``h``, ``has_lead``,
    the follower's speed and headway, the step ``dt``, the vehicle type's ``max_accel`` and its parameters ``p[0..7]`` in
    scope; T is float or double (the handle's precision).  flowsim_kernels.h includes it inside namespace fs, after the
    helper functions (tmin / tmax / tabs / tsqrt)."""
    body = "\n".join("  " + ln.strip() for ln in str(body).strip().splitlines())    # (the text is the cache key: normalised)
    return ("// generated by flow_amd.build.build_user -- the get_accel of a flow_amd.controllers.CompiledController\n"
            "%s {\n%s\n}\n" % (USER_SIGNATURE, body))


USER_ENV_VEHICLE_ARGS = ("T v, T v_lead, T h, bool has_lead, T v_follow, T h_follow, T length, T x, T L, bool is_rl, "
                         "int rl_index, T action, bool has_action, T max_speed, T target_velocity, T dt, T N, T num_rl, "
                         "const T* p")
USER_ENV_SIGNATURES = {
    "obs": "template <typename T>\n__device__ __forceinline__ void fs_user_obs(" + USER_ENV_VEHICLE_ARGS + ", T* o)",
    "terms": "template <typename T>\n__device__ __forceinline__ void fs_user_terms(" + USER_ENV_VEHICLE_ARGS + ", T* %s)",
    "reward": ("template <typename T>\n__device__ __forceinline__ T fs_user_reward(const T* %s, bool fail, bool has_action, "
               "T N, T num_rl, T max_speed, T target_velocity, T dt, const T* p)"),
}


def _norm_body(body):
    return "\n".join("  " + ln.strip() for ln in str(body).strip().splitlines())    # (the text is the cache key: normalised)


def user_env_header(env):
    """The header a user environment head is compiled from (include/flowsim.h FS_ENV_USER).  ``env``: a dict with the C++
    statement bodies ``obs`` and ``terms`` (per vehicle; they write ``o[0 .. obs_per_vehicle-1]`` / ``t[0 ..
    reward_terms-1]``) and ``reward`` (per replica, ending in a return; it reads ``sum[0 .. reward_terms-1]``), and the
    shapes ``obs_per_vehicle`` (1..8), ``rl_only`` (one block per RL vehicle, else AccelEnv's layout) and ``reward_terms``
    (0..4).  flow_amd.envs.CompiledEnv lists the names in scope.  With ``reward_terms = 0`` neither ``t`` nor ``sum`` is
    declared: a body that uses one does not compile.  flowsim_kernels.h includes the header inside namespace fs, after
    the helper functions (tmin / tmax / tabs / tsqrt)."""
    k, terms = int(env["obs_per_vehicle"]), int(env["reward_terms"])
    if not 1 <= k <= 8:
        raise ValueError("user environment head: obs_per_vehicle (OBS_PER_VEHICLE) must be 1..8, got %d" % k)
    if not 0 <= terms <= 4:
        raise ValueError("user environment head: reward_terms (REWARD_TERMS) must be 0..4, got %d" % terms)
    for name in ("obs", "reward") + (("terms",) if terms else ()):
        if not env.get(name) or not str(env[name]).strip():
            raise ValueError("user environment head: the %s body is empty" % name)
    return ("// generated by flow_amd.build.build_user -- the head of a flow_amd.envs.CompiledEnv\n"
            "constexpr int kUserObsPerVehicle = %d;\nconstexpr bool kUserObsRlOnly = %s;\nconstexpr int kUserRewardTerms = %d;\n"
            "%s {\n%s\n}\n%s {\n%s\n}\n%s {\n%s\n}\n"
            % (k, "true" if env["rl_only"] else "false", terms,
               USER_ENV_SIGNATURES["obs"], _norm_body(env["obs"]),
               USER_ENV_SIGNATURES["terms"] % ("t" if terms else "/* no terms */"), _norm_body(env.get("terms") or "") if terms else "",
               USER_ENV_SIGNATURES["reward"] % ("sum" if terms else "/* no sums */"), _norm_body(env["reward"])))


def user_tag(body=None, env=None):
    """The cache key of a user library: the generated header texts (controller, environment head) and the sources."""
    text = user_header(body) if body is not None else ""       # (a controller alone keeps the key it always had)
    if env is not None:
        text += "\0" + user_env_header(env)
    return hashlib.sha256((text + _stamp([])).encode()).hexdigest()[:16]


def build_user(body=None, verbose=False, env=None):
    """A copy of the library with the user's code in it: flow_amd/_user/<hash>/libflowsim.so.  ``body``: the get_accel of a
    CompiledController (its FS_CTRL_USER slots run it, -DFS_USER_CONTROLLER_HEADER); ``env``: the head of a CompiledEnv
    (user_env_header's dict; FS_ENV_USER handles run it, -DFS_USER_ENV_HEADER); either or both.
    Every part but the queue kernels' and the learner's is recompiled (in parallel; the C ABI object too: it refuses
    FS_CTRL_USER slots and FS_ENV_USER handles without the headers); cached by the hash of the texts and of the sources."""
    if body is None and env is None:
        raise ValueError("build_user: give the controller body, the environment head, or both")
    texts = {}
    if body is not None:
        texts["user_controller.h"] = ("FS_USER_CONTROLLER_HEADER", user_header(body))
    if env is not None:
        texts["user_env.h"] = ("FS_USER_ENV_HEADER", user_env_header(env))
    tag = user_tag(body, env)
    out_dir = os.path.join(USER_DIR, tag)
    lib = os.path.join(out_dir, "libflowsim.so")
    if os.path.exists(lib):
        return lib
    build()
    if not all(os.path.exists(os.path.join(OBJ, name + ".o")) for name, _, _ in parts()):
        build(force=True)                              # (a tree that holds the library but not its objects)
    os.makedirs(out_dir, exist_ok=True)
    for stale in os.listdir(USER_DIR):                 # copies built from other sources than the current ones
        tagfile = os.path.join(USER_DIR, stale, "sources.stamp")
        if stale != tag and os.path.exists(tagfile) and open(tagfile).read().strip() != _stamp([]):
            shutil.rmtree(os.path.join(USER_DIR, stale), ignore_errors=True)
    with open(os.path.join(out_dir, "sources.stamp"), "w") as f:
        f.write(_stamp([]))
    defines = []
    for fname, (macro, text) in texts.items():
        hdr = os.path.join(out_dir, fname)
        with open(hdr, "w") as f:
            f.write(text)
        defines.append('-D%s="%s"' % (macro, hdr))
    objs, todo = [], []
    for name, src, extra in parts():
        if name.startswith(("queue", "learn")):           # (no controller or head in them: the plain build's objects)
            objs.append(os.path.join(OBJ, name + ".o"))
            continue
        out = os.path.join(out_dir, name + ".o")
        objs.append(out)
        todo.append((name, src, extra + defines, out, verbose))
    with concurrent.futures.ThreadPoolExecutor(_jobs()) as pool:
        list(pool.map(_compile, todo))
    res = subprocess.run([find_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib + ".tmp"] + objs,
                         capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(lib + ".tmp", lib)
    for job in todo:                                   # (the objects are not needed again: the library is the cache)
        os.remove(job[3])
    return lib


def device_asm(out_dir, names=None):
    """Device assembly (gfx950) of the parts, for the code-generation guards: {part name: path of its .s}."""
    os.makedirs(out_dir, exist_ok=True)
    jobs = []
    for name, src, extra in parts():
        if names and name not in names:
            continue
        out = os.path.join(out_dir, name + ".s")
        jobs.append((name, [find_hipcc()] + COMMON_FLAGS + ["-S", "--cuda-device-only"] + extra + include_flags() +
                     ["-o", out, src], out))

    def run(job):
        res = subprocess.run(job[1], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc -S failed (%s):\n%s" % (job[0], res.stderr[-2000:]))
        return job[0], job[2]

    with concurrent.futures.ThreadPoolExecutor(_jobs()) as pool:
        return dict(pool.map(run, jobs))


if __name__ == "__main__":
    import sys
    print(build(force="--force" in sys.argv, verbose=True, only=[a for a in sys.argv[1:] if not a.startswith("-")]))
