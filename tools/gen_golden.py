#!/usr/bin/env python3
"""Generate golden fixtures under tests/golden/ by driving the REFERENCE's own env code.

Runs only in the build container (needs /root/reference, read-only).  Nothing from the
reference is copied: the fixtures are data (inputs + the outputs the reference produced).

What is imported, unmodified, from the reference:
  backend/mlagents/envs.py        (BasicMoveToGoalEnv, LegacySingleAgentGymAdapter, make_*_env)
  backend/examples/gridworld.py   (GridWorldEnv)
  backend/examples/ball3d.py      (Ball3DEnv)
  backend/examples/push.py        (PushEnv)
  backend/examples/walljump.py    (WallJumpEnv)
  backend/examples/bicycle.py, brick_break.py, glider.py   (BicycleEnv, BrickBreakEnv, GliderEnv: SURVEY.md 8f rank N3)
`gymnasium` is not installed here, so a ~20-line stand-in (Env with a no-op reset, Box/Discrete
holders) is placed in sys.modules first; it carries no arithmetic.

The driver below restates what SB3's DummyVecEnv + Monitor do around those envs
 with the build's per-(env, episode) seeding contract:
    episode k of env i is reset with  seed s(i,k) = (base + i + k * 2**20) mod 2**32
(k = 0 coincides with the reference's own `seed + rank`, backend/mlagents/training.py:80).
Actions come from a counter-based tape  a(i,t) = mix32(tape_seed, i, t) % n_actions.

The three float tasks (bicycle, brickbreak, glider) are generated in a child process that runs with
NPY_DISABLE_CPU_FEATURES set to the AVX-512 groups: numpy then takes np.tan / np.arctan2 of a float64 from libm instead of its
AVX-512 SVML kernels (which differ from libm in the last bit for ~0.5 % of the arguments), i.e. the fixtures are the reference as it
runs on a host without AVX-512 -- the configuration a plain-C restatement can match bit for bit.  The five earlier fixtures are
generated with numpy's default dispatch, as before.

Usage:  python tools/gen_golden.py [task ...]   (writes tests/golden/<task>.npz; no arguments = every task + the RNG fixture)
        python tools/gen_golden.py edges        (writes tests/golden/{bicycle,brickbreak,glider}_edges.npz and nothing else: hand-built states
                                                 at the terminal / clip / time-limit branches, one adapter step each, same child process)
"""
from __future__ import annotations

import importlib.util
import os
import subprocess
import sys
import types

import numpy as np

REF = "/root/reference/backend"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

EP_STRIDE = 1 << 20


def episode_seed(base: int, i: int, k: int) -> int:
    return (base + i + k * EP_STRIDE) & 0xFFFFFFFF


def mix32(seed, i, t):
    """murmur3-finalizer style counter hash, all arithmetic mod 2**32 (vectorised)."""
    with np.errstate(over="ignore"):
        x = (np.uint32(seed) * np.uint32(0x9E3779B1)) ^ (np.asarray(i, np.uint32) * np.uint32(0x85EBCA77)) ^ (
            np.asarray(t, np.uint32) * np.uint32(0xC2B2AE3D)
        )
        x = np.asarray(x, np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    return x


def action_tape(tape_seed: int, n_envs: int, T: int, n_actions: int) -> np.ndarray:
    t = np.arange(T, dtype=np.uint32)[:, None]
    i = np.arange(n_envs, dtype=np.uint32)[None, :]
    return (mix32(tape_seed, i, t) % np.uint32(n_actions)).astype(np.int32)


def install_standin_gymnasium():
    gym = types.ModuleType("gymnasium")

    class Env:
        metadata = {}

        def reset(self, *, seed=None, options=None):
            return None

        def close(self):
            pass

    class Space:
        pass

    class Box(Space):
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.low, self.high, self.shape, self.dtype = low, high, shape, dtype

    class Discrete(Space):
        def __init__(self, n):
            self.n = int(n)

    spaces = types.ModuleType("gymnasium.spaces")
    spaces.Space, spaces.Box, spaces.Discrete = Space, Box, Discrete
    gym.Env, gym.spaces = Env, spaces
    sys.modules["gymnasium"] = gym
    sys.modules["gymnasium.spaces"] = spaces


def load_reference_envs():
    install_standin_gymnasium()
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_mlagents_envs", os.path.join(REF, "mlagents", "envs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------
# internal-state capture / injection for the legacy envs (attribute names are the reference's)
# ------------------------------------------------------------------------------------------
def get_state(task: str, env) -> np.ndarray:
    """Flat float64 state vector of the underlying env object (layout documented per task)."""
    if task == "basic":
        return np.array([env.position, env.steps], dtype=np.float64)
    e = env.env
    if task == "gridworld":
        return np.array(
            [*e.agent_pos, *e.green_goals[0], *e.red_goals[0], int(e.current_goal_type), e.steps], dtype=np.float64
        )
    if task == "push":
        return np.array([*e.agent_pos, *e.box_pos, e.goal_pos[0], e.steps], dtype=np.float64)
    if task == "walljump":
        return np.array([e.agent_x, e.in_air, e.wall_height, e.steps], dtype=np.float64)
    if task == "ball3d":
        first = 1.0 if e.rot.dtype == np.float32 else 0.0
        return np.array([*e.rot, *e.pos, *e.vel, e.steps, first], dtype=np.float64)
    if task == "bicycle":
        return np.array([e.x, e.z, e.theta, e.phi, e.phi_dot, e.delta, *e.goal_pos, e.dist_to_goal, e.steps], dtype=np.float64)
    if task == "brickbreak":
        return np.array([e.paddle_x, *e.ball_pos, *e.ball_vel, e.steps, *e.bricks.flatten()], dtype=np.float64)
    if task == "glider":
        return np.array([*e.pos, *e.vel, *e.rot, *e.ang_vel, e.current_waypoint_index, e.steps], dtype=np.float64)
    raise KeyError(task)


FACTORY = {"brickbreak": "make_brick_break_env"}  # registry id -> factory name where they differ (backend/mlagents/registry.py:133-146)


def factory(mod, task):
    return getattr(mod, FACTORY.get(task, f"make_{task}_env"))


def vec_rollout(mod, task: str, n_envs: int, T: int, base_seed: int, tape_seed: int):
    make = factory(mod, task)
    envs = [make() for _ in range(n_envs)]
    n_act = envs[0].action_space.n
    D = envs[0].observation_space.shape[0]
    actions = action_tape(tape_seed, n_envs, T, n_act)
    ep_idx = [0] * n_envs
    reset_obs = np.zeros((n_envs, D), np.float32)
    for i, env in enumerate(envs):
        o, _ = env.reset(seed=episode_seed(base_seed, i, 0))
        reset_obs[i] = o
    obs = np.zeros((T, n_envs, D), np.float32)
    term_obs = np.zeros((T, n_envs, D), np.float32)
    rew64 = np.zeros((T, n_envs), np.float64)
    rew32 = np.zeros((T, n_envs), np.float32)
    term = np.zeros((T, n_envs), np.bool_)
    trunc = np.zeros((T, n_envs), np.bool_)
    ep_ret = np.zeros((T, n_envs), np.float64)
    ep_ret_round = np.zeros((T, n_envs), np.float64)
    ep_len = np.zeros((T, n_envs), np.int32)
    steps_info = np.zeros((T, n_envs), np.int32)
    mon_rewards = [[] for _ in range(n_envs)]
    for t in range(T):
        for i, env in enumerate(envs):
            o, r, te, tr, info = env.step(int(actions[t, i]))
            assert isinstance(te, bool) and isinstance(tr, bool)
            mon_rewards[i].append(float(r))  # Monitor.step
            rew64[t, i] = float(r)
            rew32[t, i] = np.float32(r)  # DummyVecEnv buf_rews is float32
            term[t, i], trunc[t, i] = te, tr
            steps_info[t, i] = info["steps"]
            if te or tr:
                s = sum(mon_rewards[i])
                ep_ret[t, i] = s
                ep_ret_round[t, i] = round(s, 6)
                ep_len[t, i] = len(mon_rewards[i])
                mon_rewards[i] = []
                term_obs[t, i] = o
                ep_idx[i] += 1
                o, _ = env.reset(seed=episode_seed(base_seed, i, ep_idx[i]))
            obs[t, i] = o
    return dict(
        actions=actions,
        reset_obs=reset_obs,
        obs=obs,
        terminal_obs=term_obs,
        rewards_f64=rew64,
        rewards_f32=rew32,
        terminated=term,
        truncated=trunc,
        ep_ret=ep_ret,
        ep_ret_round6=ep_ret_round,
        ep_len=ep_len,
        info_steps=steps_info,
        episodes_per_env=np.array(ep_idx, np.int32),
        meta=np.array([n_envs, T, base_seed, tape_seed, n_act, D], np.int64),
    )


def seeded_resets(mod, task: str, seeds: np.ndarray):
    make = factory(mod, task)
    env = make()
    D = env.observation_space.shape[0]
    obs = np.zeros((len(seeds), D), np.float32)
    states = []
    for j, s in enumerate(seeds):
        o, _ = env.reset(seed=int(s))
        obs[j] = o
        states.append(get_state(task, env))
    return dict(reset_seeds=seeds.astype(np.uint32), reset_seed_obs=obs, reset_seed_state=np.stack(states))


# ------------------------------------------------------------------------------------------
# single transitions under state injection (legacy 3-tuple, below the adapter)
# ------------------------------------------------------------------------------------------
def grid_transitions(mod, rng):
    from examples.gridworld import GridWorldEnv

    e = GridWorldEnv()
    rows_in, rows_out, obs_out = [], [], []
    cells = [(x, y) for x in range(5) for y in range(5)]
    for _ in range(6000):
        idx = rng.choice(25, size=3, replace=False)
        a, g, r = cells[idx[0]], cells[idx[1]], cells[idx[2]]
        gt = int(rng.integers(0, 2))
        steps = int(rng.choice([0, 1, 50, 98, 99]))
        act = int(rng.integers(0, 5))
        e.agent_pos, e.green_goals, e.red_goals, e.current_goal_type, e.steps = a, [g], [r], gt, steps
        o, rew, done = e.step(act)
        rows_in.append([*a, *g, *r, gt, steps, act])
        rows_out.append([*e.agent_pos, e.steps, float(rew), float(done)])
        obs_out.append(o)
    return dict(tr_in=np.array(rows_in, np.int32), tr_out=np.array(rows_out, np.float64), tr_obs=np.stack(obs_out))


def push_transitions(mod, rng):
    from examples.push import PushEnv

    e = PushEnv()
    rows_in, rows_out, obs_out = [], [], []
    cells = [(x, y) for x in range(6) for y in range(6)]
    for _ in range(8000):
        idx = rng.choice(36, size=2, replace=False)
        a, b = cells[idx[0]], cells[idx[1]]
        gx = int(rng.integers(0, 6))
        steps = int(rng.choice([0, 1, 60, 118, 119]))
        act = int(rng.integers(0, 5))
        e.agent_pos, e.box_pos, e.goal_pos, e.steps = a, b, (gx, 5), steps
        o, rew, done = e.step(act)
        rows_in.append([*a, *b, gx, steps, act])
        rows_out.append([*e.agent_pos, *e.box_pos, e.steps, float(rew), float(done)])
        obs_out.append(o)
    return dict(tr_in=np.array(rows_in, np.int32), tr_out=np.array(rows_out, np.float64), tr_obs=np.stack(obs_out))


def ball3d_transitions(mod, rng):
    from examples.ball3d import Ball3DEnv

    e = Ball3DEnv()
    rows_in, rows_out, obs_out = [], [], []
    for n in range(6000):
        first = bool(n % 3 == 0)
        if first:  # state right after a reset: rot is a float32 array
            rot = rng.uniform(-0.25, 0.25, 2).astype(np.float32)
        else:  # later steps: rot is float64 (np.clip with np.float64 bounds)
            rot = np.clip(rng.uniform(-0.5, 0.5, 2), -np.deg2rad(25.0), np.deg2rad(25.0))
        pos = rng.uniform(-3.2, 3.2, 2).astype(np.float32)
        vel = rng.uniform(-4.0, 4.0, 2).astype(np.float32)
        steps = int(rng.choice([0, 1, 100, 198, 199]))
        act = int(rng.integers(0, 5))
        e.rot, e.pos, e.vel, e.steps = rot.copy(), pos.copy(), vel.copy(), steps
        rows_in.append([*rot.astype(np.float64), *pos.astype(np.float64), *vel.astype(np.float64), steps, float(first), act])
        o, rew, done = e.step(act)
        assert e.rot.dtype == np.float64 and isinstance(rew, np.float32)
        rows_out.append([*e.rot, *e.pos.astype(np.float64), *e.vel.astype(np.float64), e.steps, float(rew), float(done)])
        obs_out.append(o)
    return dict(tr_in=np.array(rows_in, np.float64), tr_out=np.array(rows_out, np.float64), tr_obs=np.stack(obs_out))


def walljump_transitions(mod, rng):
    from examples.walljump import WallJumpEnv

    e = WallJumpEnv()
    rows_in, rows_out, obs_out = [], [], []
    for x in range(20):
        for in_air in range(4):
            for wall in (0, 1):
                for act in range(4):
                    steps = int(rng.choice([0, 1, 148, 149]))
                    e.agent_x, e.in_air, e.wall_height, e.steps = x, in_air, wall, steps
                    o, rew, done = e.step(act)
                    rows_in.append([x, in_air, wall, steps, act])
                    rows_out.append([e.agent_x, e.in_air, e.wall_height, e.steps, float(rew), float(done)])
                    obs_out.append(o)
    return dict(tr_in=np.array(rows_in, np.int32), tr_out=np.array(rows_out, np.float64), tr_obs=np.stack(obs_out))


def float_task_transitions(mod, task, rng):
    """Single legacy steps (below the adapter) from states visited by seeded random-action episodes: state in, action -> state out,
    reward, done, observation.  The injected state is the flat vector of get_state()."""
    env = factory(mod, task)()
    n_act = env.action_space.n
    rows_in, rows_out, obs_out = [], [], []
    for ep in range(40):
        env.reset(seed=1000 + ep)
        e = env.env
        for t in range(100):
            act = int(rng.integers(0, n_act))
            rows_in.append([*get_state(task, env), act])
            o, rew, done = e.step(act)
            rows_out.append([*get_state(task, env), float(rew), float(done)])
            obs_out.append(np.asarray(o, np.float64))
            if done:
                break
    return dict(tr_in=np.array(rows_in, np.float64), tr_out=np.array(rows_out, np.float64), tr_obs=np.stack(obs_out))


def basic_transitions(mod):
    env = mod.make_basic_env()
    rows_in, rows_out, obs_out = [], [], []
    for pos in range(21):
        for steps in (0, 48, 49):
            for act in range(3):
                env.reset(seed=1, options={"position": pos})
                env.steps = steps
                o, r, te, tr, info = env.step(act)
                rows_in.append([pos, steps, act])
                rows_out.append([info["position"], info["steps"], float(r), float(te), float(tr)])
                obs_out.append(o)
    return dict(tr_in=np.array(rows_in, np.int32), tr_out=np.array(rows_out, np.float64), tr_obs=np.stack(obs_out))


def rng_fixture():
    """numpy legacy global-RNG primitives (the third-party algorithm the legacy envs consume)."""
    seeds = np.array([0, 1, 5, 7, 123, 321, 10_001, 2**20 + 3, 2**31 + 17, 2**32 - 1], np.uint64)
    raw, shuf25, shuf36, choice2, randint6, unif = [], [], [], [], [], []
    for s in seeds:
        np.random.seed(int(s))
        raw.append(np.random.randint(0, 2**32, size=1300, dtype=np.uint64))  # crosses two twists
        np.random.seed(int(s))
        cells = list(range(25))
        np.random.shuffle(cells)
        shuf25.append(cells)
        choice2.append(int(np.random.choice([0, 1])))
        np.random.seed(int(s))
        cells = list(range(36))
        np.random.shuffle(cells)
        shuf36.append(cells)
        randint6.append(int(np.random.randint(0, 6)))
        np.random.seed(int(s))
        unif.append(np.random.uniform(-1.5, 1.5, size=6))
    return dict(
        seeds=seeds,
        raw_u32=np.array(raw, np.uint32),
        shuffle25=np.array(shuf25, np.int32),
        choice2_after25=np.array(choice2, np.int32),
        shuffle36=np.array(shuf36, np.int32),
        randint6_after36=np.array(randint6, np.int32),
        uniform_pm1p5=np.array(unif, np.float64),
    )


# ------------------------------------------------------------------------------------------
# `edges` mode: hand-built states at the branches random action tapes never reach, one step THROUGH THE ADAPTER each
# (tests/golden/{bicycle,brickbreak,glider}_edges.npz).  Every scenario is built once per action of the task (the action changes where
# the step lands, so the state is solved per action), unless its label ends in `_a<k>`: then only action k is taken.
# ------------------------------------------------------------------------------------------
def set_state(task: str, env, st) -> None:
    """Inverse of get_state() for the three float tasks; the adapter's own step counter is set to the inner env's."""
    e = env.env
    st = np.asarray(st, np.float64)
    if task == "bicycle":
        e.x, e.z, e.theta, e.phi, e.phi_dot, e.delta = (float(v) for v in st[:6])
        e.goal_pos = st[6:8].copy()
        e.dist_to_goal = np.float64(st[8])
        e.steps = int(st[9])
    elif task == "brickbreak":
        e.paddle_x = float(st[0])
        e.ball_pos, e.ball_vel = st[1:3].copy(), st[3:5].copy()
        e.steps = int(st[5])
        e.bricks = st[6:46].reshape(5, 8).copy()
    elif task == "glider":
        e.pos, e.vel, e.rot, e.ang_vel = st[0:3].copy(), st[3:6].copy(), st[6:9].copy(), st[9:12].copy()
        e.current_waypoint_index = int(st[12])
        e.steps = int(st[13])
    else:
        raise KeyError(task)
    env.steps = e.steps


sys.path.insert(0, os.path.dirname(OUT))
from _edges import STEPS_AT, actions_of  # noqa: E402  (tests/_edges.py: the label convention and the state layout, defined once)

LO, HI = 1e-6, 1e-3  # margins of a trig / sqrt-dependent deciding quantity from its threshold, relative to max(1, |threshold|)


def deciding(task: str, env, st_in):
    """(name, value, threshold) of every comparison of the step just taken whose left side went through sqrt / sin / cos / tan / arctan2,
    recomputed from the reference's own state with the reference's own expressions."""
    e = env.env
    if task == "bicycle":
        return [("new_dist", float(e.dist_to_goal), 2.0), ("phi", abs(float(e.phi)), float(e.max_phi))]
    if task == "glider":
        dist = float(np.linalg.norm(e.waypoints[int(st_in[12])] - e.pos))
        v_air = st_in[3:6] - e._wind_model(st_in[0:3])
        vam = float(np.linalg.norm(v_air))
        q = [("dist", dist, 15.0), ("dist", dist, 500.0), ("lateral", abs(float(e.pos[1])), 250.0), ("alt", float(e.pos[2]), 250.0),
             ("alt", float(e.pos[2]), 25.0), ("alt", float(e.pos[2]), 5.0), ("vam", vam, 0.1)]
        if vam > 0.1 and v_air[0] != 0:
            q.append(("aoa", abs(float(np.arctan2(-v_air[2], v_air[0]))), float(e.max_aoa)))
        return q
    return []  # brickbreak: add / multiply / compare only, its rows sit exactly on the thresholds


def record_edges(mod, task: str, rows):
    """rows: (label, state_in, action, near) with near = names of the deciding quantities the label puts just inside / outside."""
    env = factory(mod, task)()
    env.reset(seed=1)
    out = {k: [] for k in ("state_in", "action", "state_out", "obs64", "obs32", "rew64", "rew32", "terminated", "truncated", "labels")}
    for label, st_in, act, near in rows:
        st_in = np.asarray(st_in, np.float64)
        set_state(task, env, st_in)
        assert np.array_equal(get_state(task, env), st_in), label
        o32, r, te, tr, info = env.step(int(act))
        assert isinstance(r, float) and isinstance(te, bool) and isinstance(tr, bool) and o32.dtype == np.float32
        assert info["steps"] == env.env.steps == int(st_in[STEPS_AT[task]]) + 1
        o64 = np.asarray(env.env._get_obs(), np.float64)  # a pure function of the state: the float64 array step() returned
        assert np.array_equal(o64.astype(np.float32), o32), label
        found = set()
        for name, val, thr in deciding(task, env, st_in):
            scale = max(1.0, abs(thr))
            assert abs(val - thr) >= LO * scale, (label, act, name, val, thr)
            if name in near and abs(val - thr) <= HI * scale:
                found.add(name)
        assert found == set(near), (label, act, near, found, deciding(task, env, st_in))
        for k, v in (("state_in", st_in), ("action", act), ("state_out", get_state(task, env)), ("obs64", o64), ("obs32", o32), ("rew64", r),
                     ("rew32", np.float32(r)), ("terminated", te), ("truncated", tr), ("labels", label)):
            out[k].append(v)
    d = dict(state_in=np.stack(out["state_in"]), action=np.array(out["action"], np.int32), state_out=np.stack(out["state_out"]),
             obs64=np.stack(out["obs64"]), obs32=np.stack(out["obs32"]), rew64=np.array(out["rew64"], np.float64),
             rew32=np.array(out["rew32"], np.float32), terminated=np.array(out["terminated"], np.bool_),
             truncated=np.array(out["truncated"], np.bool_), labels=np.array(out["labels"]))
    return d


def bicycle_edges(mod):
    env = factory(mod, "bicycle")()
    e = env.env
    dt, max_phi, max_delta = e.dt, float(e.max_phi), float(e.max_delta)
    rows = []

    def add(label, *, goal_d=12.0, phi_out=None, steps=10, delta=0.1, x=0.3, z=-0.2, theta=0.4, phi=0.05, near=()):
        for a in actions_of("bicycle", label):
            # phi' = phi + (phi_dot + phi_ddot * dt) * dt with phi_ddot free of phi_dot, x' and z' free of phi: one probe step gives both
            set_state("bicycle", env, [x, z, theta, phi, 0.0, delta, 0.0, 0.0, 0.0, steps])
            e.step(a)
            phi_dot = 0.02 if phi_out is None else (phi_out - e.phi) / dt
            goal = np.array([e.x + goal_d * np.cos(0.7), e.z + goal_d * np.sin(0.7)])
            dist_in = np.linalg.norm(goal - np.array([x, z]))
            rows.append((label, [x, z, theta, phi, phi_dot, delta, *goal, dist_in, steps], a, near))

    m = 2e-4
    add("goal_inside", goal_d=2.0 - m, near=("new_dist",))
    add("goal_outside", goal_d=2.0 + m, near=("new_dist",))
    for sign, tag in ((1.0, "pos"), (-1.0, "neg")):
        add(f"fall_{tag}", phi_out=sign * (max_phi + m), phi=sign * 0.7, near=("phi",))
        add(f"upright_{tag}", phi_out=sign * (max_phi - m), phi=sign * 0.7, near=("phi",))
    add("goal_and_fall", goal_d=2.0 - m, phi_out=max_phi + m, phi=0.7, near=("new_dist", "phi"))
    add("goal_and_upright", goal_d=2.0 - m, phi_out=max_phi - m, phi=0.7, near=("new_dist", "phi"))
    add("fall_and_goal_outside", goal_d=2.0 + m, phi_out=-(max_phi + m), phi=-0.7, near=("new_dist", "phi"))
    # the steering clip: delta + steer_change is an addition, the rows may sit anywhere
    add("delta_clip_hi", delta=max_delta + 0.06)   # clipped under every action
    add("delta_clip_lo", delta=-(max_delta + 0.06))
    add("delta_below_clip_hi", delta=max_delta - 0.06)  # clipped under none
    add("delta_above_clip_lo", delta=-(max_delta - 0.06))
    add("delta_clip_hi_by_a2", delta=max_delta - 0.02)  # +0.05 crosses it
    add("delta_clip_lo_by_a0", delta=-(max_delta - 0.02))
    add("delta_near_clip_hi_a1", delta=max_delta - 0.02)  # the same states under the action that stays inside
    add("delta_near_clip_lo_a1", delta=-(max_delta - 0.02))
    for s in (1998, 1999, 2000):
        add(f"steps{s}_continue", steps=s)
        add(f"steps{s}_fall", steps=s, phi_out=max_phi + m, phi=0.7, near=("phi",))
        add(f"steps{s}_goal", steps=s, goal_d=2.0 - m, near=("new_dist",))
    # landing on the goal: theta' = 0 exactly (delta + steer_change == 0.0, tan(0) == 0), x' = 0 + 5 * 0.02 and z' = 0 + 0 need no libm value that
    # could differ between hosts, so `new_dist == 0` (and 1e-9) is met by every implementation of the same arithmetic
    for label, off in (("on_goal_exact", 0.0), ("on_goal_1e-9", 1e-9)):
        for a in range(3):
            delta = {0: 0.05, 1: 0.0, 2: -0.05}[a]
            set_state("bicycle", env, [0.0, 0.0, 0.0, 0.05, 0.02, delta, 5.0, 5.0, 7.0, 10])
            e.step(a)
            assert e.theta == 0.0 and e.z == 0.0 and e.delta == 0.0
            goal = np.array([e.x + off * 0.6, e.z + off * 0.8])
            rows.append((label, [0.0, 0.0, 0.0, 0.05, 0.02, delta, *goal, np.linalg.norm(goal), 10], a, ()))
    # start states for multi-step replays: `pre_<x>_a1` is one no-steer step before a state whose outcome (`any_<x>`, recorded from that one
    # state under every action) does not depend on the action -- margins of 0.05 / 0.01 against an action's 5e-4 on the position and the lean
    def after(st, actions):
        set_state("bicycle", env, st)
        for a in actions:
            e.step(a)
        return get_state("bicycle", env)

    def pre_any(tag, st):
        rows.append((f"pre_{tag}_a1", st, 1, ()))
        for a in range(3):
            rows.append((f"any_{tag}", after(st, [1]), a, ()))

    base = [0.3, -0.2, 0.4, 0.05, 0.02, 0.0, 0.0, 0.0, 0.0, 10]
    two = after(base, [1, 1])
    goal = [two[0] + 1.95 * np.cos(two[2]), two[1] + 1.95 * np.sin(two[2])]  # 2.05 away after one step, 1.95 after two
    pre_any("goal", [*base[:6], *goal, np.hypot(goal[0] - base[0], goal[1] - base[1]), 10])
    far = [base[0] + 12.0 * np.cos(0.7), base[1] + 12.0 * np.sin(0.7)]
    pre_any("continue", [*base[:6], *far, 12.0, 10])
    lo, hi = 0.6, 0.8  # phi of the start state by bisection: phi'' = max_phi + 0.01 with phi_dot = 1 rad/s, i.e. phi' ~ max_phi - 0.01
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if after([0.3, -0.2, 0.4, mid, 1.0, 0.0, *far, 12.0, 10], [1, 1])[3] < max_phi + 0.01 else (lo, mid)
    pre_any("fall", [0.3, -0.2, 0.4, lo, 1.0, 0.0, *far, 12.0, 10])
    d = record_edges(mod, "bicycle", rows)
    nd = d["state_out"][:, 8]
    assert np.all(nd[d["labels"] == "on_goal_exact"] == 0.0)
    assert np.all((nd[d["labels"] == "on_goal_1e-9"] > 0) & (nd[d["labels"] == "on_goal_1e-9"] <= 1e-9))
    return d


def brickbreak_edges(mod):
    def nxt(thr, toward, v=None):
        """The float64 next to `thr` on the side of `toward` that a ball moving by `v` per step can land on exactly."""
        t = np.nextafter(thr, toward)
        while v is not None and (t - v) + v != t:
            t = np.nextafter(t, toward)
        assert abs(t - thr) <= 4e-15 * thr
        return t

    FULL = np.ones((5, 8))
    rows = []

    def add(label, ball_out, vel, *, paddle_out=8.0, paddle_in=None, steps=10, bricks=FULL):
        for a in actions_of("brickbreak", label):
            p_in = paddle_in if paddle_in is not None else paddle_out - {0: -3.0, 1: 0.0, 2: 3.0}[a]
            ball_out_, vel_ = np.asarray(ball_out, np.float64), np.asarray(vel, np.float64)
            ball_in = ball_out_ - vel_
            assert np.array_equal(ball_in + vel_, ball_out_), (label, ball_in, vel_)  # the step lands exactly where the label says
            rows.append((label, [p_in, *ball_in, *vel_, steps, *np.asarray(bricks, np.float64).flatten()], a, ()))

    def only(*cells):
        b = np.zeros((5, 8))
        for r, c in cells:
            b[r, c] = 1.0
        return b

    def without(*cells):
        b = FULL.copy()
        for r, c in cells:
            b[r, c] = 0.0
        return b

    up, down = (0.5, 1.0), (0.25, -1.0)
    add("win_last_brick", (17.5, 25.0), up, bricks=only((2, 3)))
    add("win_and_lost", (20.0, 0.5), down, bricks=only())
    add("win_no_bricks_midair", (20.0, 12.0), up, bricks=only())
    add("two_bricks_left_hit_one", (17.5, 25.0), up, bricks=only((2, 3), (4, 7)))
    # walls: `<= ball_radius`, `>= width - ball_radius`, `>= height - ball_radius`
    add("wall_left_on", (1.0, 12.0), (-0.5, 1.0))
    add("wall_left_off", (nxt(1.0, 2.0, -0.5), 12.0), (-0.5, 1.0))
    add("wall_right_on", (39.0, 12.0), (0.5, 1.0))
    add("wall_right_off", (nxt(39.0, 0.0, 0.5), 12.0), (0.5, 1.0))
    add("ceiling_on", (12.5, 39.0), (0.5, 1.0))
    add("ceiling_off", (12.5, nxt(39.0, 0.0, 1.0)), (0.5, 1.0))
    # paddle: `vel_y < 0`, `ball_y - ball_radius <= 2`, `paddle_x - 4 <= ball_x <= paddle_x + 4`
    P = 20.0
    add("paddle_band_on", (21.0, 3.0), down, paddle_out=P)
    add("paddle_band_off", (21.0, nxt(3.0, 4.0, -1.0)), down, paddle_out=P)
    add("paddle_left_on", (P - 4.0, 2.5), down, paddle_out=P)
    add("paddle_left_off", (nxt(P - 4.0, 0.0, 0.25), 2.5), down, paddle_out=P)
    add("paddle_right_on", (P + 4.0, 2.5), down, paddle_out=P)
    add("paddle_right_off", (nxt(P + 4.0, 40.0, 0.25), 2.5), down, paddle_out=P)
    add("paddle_ball_rising", (21.0, 2.5), (0.25, 1.0), paddle_out=P)
    add("paddle_ball_level", (21.0, 2.5), (0.25, 0.0), paddle_out=P)
    # lost: `ball_y < ball_radius`
    add("lost_on", (30.0, 1.0), down)
    add("lost_off", (30.0, nxt(1.0, 0.0, -1.0)), down)
    add("paddle_hit_and_lost", (21.0, 0.5), down, paddle_out=P)
    # the paddle's own clip at paddle_width / 2 and width - paddle_width / 2
    add("paddle_clip_lo", (20.0, 12.0), up, paddle_in=0.5)
    add("paddle_clip_hi", (20.0, 12.0), up, paddle_in=39.5)
    add("paddle_at_lo", (20.0, 12.0), up, paddle_in=4.0)
    add("paddle_at_hi", (20.0, 12.0), up, paddle_in=36.0)
    add("paddle_lands_on_lo_a0", (20.0, 12.0), up, paddle_in=7.0)
    add("paddle_lands_on_hi_a2", (20.0, 12.0), up, paddle_in=33.0)
    # brick edges, `>=` / `<=` on both axes, and the row-major order of the scan on shared edges
    add("brick_bottom_on", (17.5, 20.0), up)
    add("brick_bottom_off", (17.5, nxt(20.0, 0.0, 1.0)), up)
    add("brick_top_on", (17.5, 30.0), up)
    add("brick_top_off", (17.5, nxt(30.0, 40.0, 1.0)), up)
    add("xedge_both", (20.0, 25.0), up)
    add("xedge_lower_gone", (20.0, 25.0), up, bricks=without((2, 3)))
    add("xedge_upper_gone", (20.0, 25.0), up, bricks=without((2, 4)))
    add("xedge_both_gone", (20.0, 25.0), up, bricks=without((2, 3), (2, 4)))
    add("yedge_both", (17.5, 24.0), up)
    add("yedge_lower_gone", (17.5, 24.0), up, bricks=without((1, 3)))
    add("yedge_upper_gone", (17.5, 24.0), up, bricks=without((2, 3)))
    corner = [(1, 3), (1, 4), (2, 3), (2, 4)]
    for k in range(5):
        add(f"corner_gone{k}", (20.0, 24.0), up, bricks=without(*corner[:k]))
    add("wall_left_and_brick", (0.5, 21.0), (-0.5, 1.0))
    add("wall_right_and_brick", (39.5, 29.0), (0.5, 1.0))
    for s in (1998, 1999):
        add(f"steps{s}_continue", (20.0, 12.0), up, steps=s)
        add(f"steps{s}_lost", (30.0, 0.5), down, steps=s)
        add(f"steps{s}_brick", (17.5, 25.0), up, steps=s)
        add(f"steps{s}_win", (17.5, 25.0), up, steps=s, bricks=only((2, 3)))
    # start states for multi-step replays (see bicycle_edges): the ball is two steps from its target, out of the paddle's reach either way
    def pre_any(tag, ball_out, vel, bricks):
        ball_out, vel = np.asarray(ball_out, np.float64), np.asarray(vel, np.float64)
        flat = np.asarray(bricks, np.float64).flatten()
        rows.append((f"pre_{tag}_a1", [8.0, *(ball_out - 2 * vel), *vel, 10, *flat], 1, ()))
        for a in range(3):
            rows.append((f"any_{tag}", [8.0, *(ball_out - vel), *vel, 11, *flat], a, ()))

    pre_any("win", (17.5, 21.0), (0.5, 1.5), only((0, 3)))
    pre_any("lost", (30.0, 0.5), (0.25, -1.0), FULL)
    pre_any("continue", (20.0, 12.0), (0.5, 1.0), FULL)
    return record_edges(mod, "brickbreak", rows)


def glider_edges(mod):
    env = factory(mod, "glider")()
    e = env.env
    dt, max_aoa = e.dt, float(e.max_aoa)
    WP = [w.copy() for w in e.waypoints]
    U = np.array([0.48, 0.6, 0.64])  # a unit vector
    rows = []

    def va_at(aoa, mag=14.0, side=-0.5):
        return np.array([mag * np.cos(aoa), side, -mag * np.sin(aoa)])

    def add(label, pos_out, *, va=None, vel_x=None, rot=(0.1, -0.05, 0.3), ang_vel=(0.02, -0.03, 0.01), wp=0, steps=10, near=()):
        """Solve pos_in so that the step lands on pos_out: pos' = pos + vel' * dt, and vel' depends on pos only through the wind at (x, y)."""
        va_ = va_at(np.arctan2(1.0, 14.0)) if va is None else np.asarray(va, np.float64)
        pos_out = np.asarray(pos_out, np.float64)
        for a in actions_of("glider", label):
            pos_in = pos_out - np.array([15.0, 0.0, -1.0]) * dt
            for _ in range(12):
                vel_in = e._wind_model(pos_in) + va_
                if vel_x is not None:
                    vel_in[0] = vel_x  # exactly, whatever the wind
                st = [*pos_in, *vel_in, *rot, *ang_vel, wp, steps]
                set_state("glider", env, st)
                e.step(a)
                pos_in = pos_in + (pos_out - e.pos)
            rows.append((label, st, a, near))

    cruise = np.array([10.0, 20.0, 100.0])
    add("cruise", cruise)
    for w in (0, 1):
        add(f"wp{w}_reached", WP[w] + (15.0 - 1.5e-3) * U, wp=w, near=("dist",))
        add(f"wp{w}_missed", WP[w] + (15.0 + 1.5e-3) * U, wp=w, near=("dist",))
    for sign, tag in ((1.0, "pos"), (-1.0, "neg")):
        add(f"corridor_{tag}_outside", [10.0, sign * (250.0 + 0.025), 100.0], near=("lateral",))
        add(f"corridor_{tag}_inside", [10.0, sign * (250.0 - 0.025), 100.0], near=("lateral",))
        add(f"corridor_{tag}_far", [10.0, sign * 300.0, 100.0])
    add("alt_high_over", [10.0, 20.0, 250.0 + 0.025], near=("alt",))
    add("alt_high_under", [10.0, 20.0, 250.0 - 0.025], near=("alt",))
    add("alt_high_far", [10.0, 20.0, 300.0])
    add("alt_low_under", [10.0, 20.0, 25.0 - 2.5e-3], near=("alt",))
    add("alt_low_over", [10.0, 20.0, 25.0 + 2.5e-3], near=("alt",))
    add("crash", [10.0, 20.0, 5.0 - 5e-4], near=("alt",))
    add("no_crash", [10.0, 20.0, 5.0 + 5e-4], near=("alt",))
    for sign, tag in ((1.0, "pos"), (-1.0, "neg")):
        add(f"stall_{tag}", cruise, va=va_at(sign * (max_aoa + 1e-4)), near=("aoa",))
        add(f"no_stall_{tag}", cruise, va=va_at(sign * (max_aoa - 1e-4)), near=("aoa",))
    far = WP[0] + np.array([500.0, 0.0, 0.0])
    add("too_far", far + [0.05, 0.0, 0.0], near=("dist",))
    add("not_too_far", far - [0.05, 0.0, 0.0], near=("dist",))
    add("crash_and_stall", [10.0, 20.0, 5.0 - 5e-4], va=va_at(max_aoa + 1e-4), near=("alt", "aoa"))
    add("crash_and_too_far", [far[0] + 0.5, 0.0, 5.0 - 5e-4], near=("alt",))
    add("stall_and_too_far", far + [0.05, 0.0, 0.0], va=va_at(-(max_aoa + 1e-4)), near=("dist", "aoa"))
    add("crash_stall_too_far", [far[0] + 0.5, 0.0, 5.0 - 5e-4], va=va_at(max_aoa + 1e-4), near=("alt", "aoa"))
    # `v_air_mag > 0.1`: below it the aerodynamic force and the angle of attack are dropped, so a 30-degree v_air stalls on one side only
    add("vair_over_steep", cruise, va=va_at(np.pi / 6, mag=0.1 + 1e-4, side=0.0), near=("vam",))
    add("vair_under_steep", cruise, va=va_at(np.pi / 6, mag=0.1 - 1e-4, side=0.0), near=("vam",))
    add("vair_over_level", cruise, va=va_at(0.0, mag=0.1 + 1e-4, side=0.0), near=("vam",))
    add("vair_under_level", cruise, va=va_at(0.0, mag=0.1 - 1e-4, side=0.0), near=("vam",))
    # `v_air[0] != 0`: vel[0] == 1.0 exactly against the wind's constant 1.0 (a subtraction, no margin needed) drops an angle of attack of 56 degrees
    add("vair_x_zero", cruise, va=(0.0, 2.0, -3.0), vel_x=1.0)
    add("vair_x_tiny", cruise, va=(0.0, 2.0, -3.0), vel_x=1.0 + 1e-3)
    # roll / pitch clamps (additions and a clip: the rows may sit anywhere): 0.95 * (2 -+ 0.3) * 0.02 carries every action past the bound
    add("roll_clamp_hi", cruise, rot=(float(e.max_roll) - 1e-3, -0.05, 0.3), ang_vel=(2.0, -0.03, 0.01))
    add("roll_clamp_lo", cruise, rot=(-float(e.max_roll) + 1e-3, -0.05, 0.3), ang_vel=(-2.0, -0.03, 0.01))
    add("pitch_clamp_hi", cruise, rot=(0.1, float(e.max_pitch) - 1e-3, 0.3), ang_vel=(0.02, 2.0, 0.01))
    add("pitch_clamp_lo", cruise, rot=(0.1, -float(e.max_pitch) + 1e-3, 0.3), ang_vel=(0.02, -2.0, 0.01))
    for s in (3998, 3999):
        add(f"steps{s}_cruise", cruise, steps=s)
        add(f"steps{s}_crash", [10.0, 20.0, 5.0 - 5e-4], steps=s, near=("alt",))
        add(f"steps{s}_wp_reached", WP[1] + (15.0 - 1.5e-3) * U, wp=1, steps=s, near=("dist",))
    # start states for multi-step replays (see bicycle_edges): `pre_<x>_a0` lands on `any_<x>`'s state, whose next step crosses 5 m / the 15 m
    # waypoint sphere by 8e-3 / 0.1 -- an action moves that step's landing point by 2e-5
    def solve_two(pos_two, wp):
        pos_two = np.asarray(pos_two, np.float64)
        pos_in = pos_two - 2 * np.array([15.0, 0.0, -1.0]) * dt
        for _ in range(12):
            st = [*pos_in, *(e._wind_model(pos_in) + va_at(np.arctan2(1.0, 14.0))), 0.1, -0.05, 0.3, 0.02, -0.03, 0.01, wp, 10]
            set_state("glider", env, st)
            e.step(0)
            mid = get_state("glider", env)
            e.step(0)
            pos_in = pos_in + (pos_two - e.pos)
        return st, mid

    def pre_any(tag, pos_two, wp=0):
        st, mid = solve_two(pos_two, wp)
        rows.append((f"pre_{tag}_a0", st, 0, ()))
        for a in range(5):
            rows.append((f"any_{tag}", mid, a, ()))

    _, mid = solve_two([-40.0, 20.0, 5.0], 0)  # (x = -40: an 8 m/s downdraft of the wind model, the glider sinks through both steps)
    sink = mid[2] - 5.0  # height lost per step on this glide path: the crash row crosses 5 m in the middle of its second step
    assert sink > 4e-3, sink
    pre_any("crash", [-40.0, 20.0, 5.0 - sink / 2])
    pre_any("cruise", cruise)
    pre_any("wp_reached", WP[1] - 14.9 * np.array([15.0, 0.0, -1.0]) / np.linalg.norm([15.0, 0.0, -1.0]), wp=1)
    return record_edges(mod, "glider", rows)


def save_npz_reproducible(path: str, d: dict) -> None:
    """np.savez_compressed stamps every member with the wall clock; this writes the same container with a fixed stamp, so that a second
    run gives the same bytes."""
    import zipfile

    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, val in d.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w", force_zip64=True) as fid:
                np.lib.format.write_array(fid, np.asanyarray(val), allow_pickle=False)


def edges_main():
    mod = load_reference_envs()
    for task, build in (("bicycle", bicycle_edges), ("brickbreak", brickbreak_edges), ("glider", glider_edges)):
        d = build(mod)
        path = os.path.join(OUT, f"{task}_edges.npz")
        save_npz_reproducible(path, d)
        labels, counts = np.unique(d["labels"], return_counts=True)
        print(task, "edges:", len(d["labels"]), "rows,", len(labels), "labels ->", path, os.path.getsize(path), "B")
        print("   ", ", ".join(f"{l} x{c}" for l, c in zip(labels, counts)))


FLOAT_TASKS = ("bicycle", "brickbreak", "glider")
NO_AVX512 = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"


def main():
    os.makedirs(OUT, exist_ok=True)
    want = sys.argv[1:]
    if want == ["edges"]:  # the edge fixtures only; none of the files below is touched
        if os.environ.get("NPY_DISABLE_CPU_FEATURES") != NO_AVX512:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "edges"], env={**os.environ, "NPY_DISABLE_CPU_FEATURES": NO_AVX512})
        else:
            edges_main()
        return
    cfg = {
        # task: (n_envs, T, base_seed, tape_seed)
        "basic": (8, 400, 1, 11),
        "gridworld": (16, 700, 1, 12),
        "push": (16, 900, 1, 13),
        "ball3d": (16, 900, 1, 14),
        "walljump": (16, 700, 1, 15),
        "bicycle": (16, 500, 1, 16),
        "brickbreak": (16, 900, 1, 17),
        "glider": (16, 2600, 1, 18),
    }
    floats = [t for t in FLOAT_TASKS if not want or t in want]
    if floats and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NO_AVX512:
        # the float tasks: a child with the AVX-512 dispatch of numpy disabled (see the module docstring)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), *floats], env={**os.environ, "NPY_DISABLE_CPU_FEATURES": NO_AVX512})
        want = [t for t in (want or [*cfg, "rng"]) if t not in FLOAT_TASKS]
        if not want:
            return
    mod = load_reference_envs()
    rng = np.random.default_rng(20261002)
    for task, (n, T, base, tape) in cfg.items():
        if task in FLOAT_TASKS and os.environ.get("NPY_DISABLE_CPU_FEATURES") != NO_AVX512:
            continue
        # (the shared generator advances per task in table order whether or not the task is written, so a partial run reproduces the files)
        if task in FLOAT_TASKS:
            rng_t = np.random.default_rng(20261002 + tape)
        d = vec_rollout(mod, task, n, T, base, tape) if (not want or task in want) else None
        if d is not None:
            # a second rollout at the reference test-suite's seed (tests/test_mlagents.py:86 uses 321)
            d2 = vec_rollout(mod, task, 4, 300, 321, tape + 100)
            d.update({f"b_{k}": v for k, v in d2.items()})
            d.update(seeded_resets(mod, task, np.concatenate([np.arange(0, 200), [321, 10_001, 2**20 + 1, 2**32 - 1]])))
        if task == "gridworld":
            tr = grid_transitions(mod, rng)
        elif task == "push":
            tr = push_transitions(mod, rng)
        elif task == "ball3d":
            tr = ball3d_transitions(mod, rng)
        elif task == "walljump":
            tr = walljump_transitions(mod, rng)
        elif task in FLOAT_TASKS:
            tr = float_task_transitions(mod, task, rng_t)
        else:
            tr = basic_transitions(mod)
        if d is None:
            continue
        d.update(tr)
        path = os.path.join(OUT, f"{task}.npz")
        np.savez_compressed(path, **d)
        print(task, "episodes/env:", d["episodes_per_env"].tolist(), "->", path, os.path.getsize(path), "B")
    if not want or "rng" in want:
        path = os.path.join(OUT, "numpy_legacy_rng.npz")
        np.savez_compressed(path, **rng_fixture())
        print("rng ->", path, os.path.getsize(path), "B")


if __name__ == "__main__":
    main()
